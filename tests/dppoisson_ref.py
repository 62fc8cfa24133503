"""NumPy restatement of the doubly periodic Poisson slab solver, for the tests.

It takes nothing from the product.  Everything that runs per particle, per node or per wave number takes a `real` dtype: np.float64
is the reference the GPU tests compare against, np.float32 runs the same steps in single precision and measures the bars of the
single-precision tests.  What the product computes once on the host in double (grid sizes, tables, cosine tables, quadrature
weights, surface spectra, the analytic correction's exponentials) is computed in double here too and cast.

Conventions.  A field has shape (nz, ny, nx); plane k lies at z_k = (H/2 + 3 He) cos(pi k / (nz - 1)); node (i, j) lies at
((i / nx - 1/2) Lx, (j / ny - 1/2) Ly).  Spectra are FULL planes of nx ny wave numbers, system s = i + nx j, with the normalised
forward transform (divided by nx ny) of tests/chebyshev_bvp_ref.py; the surface values are transformed with the same normalisation,
so setSurfaceValuesZeroModeFourier(v) is a uniform wall value v.
"""
import math

import numpy as np

import chebyshev_bvp_ref as cb

_erf = np.vectorize(math.erf, otypes=[np.float64])


class Refusal(ValueError):
    pass


# ------------------------------------------------------------------------------------------------------------- host closed forms
def greens_near_potential(r2, split, gw, eps):
    """NearField.cuh:14-35."""
    r2 = np.asarray(r2, dtype=np.float64)
    gw2 = gw * gw
    r = np.sqrt(r2)
    far = r > gw * 1e-2
    rs = np.where(far, r, 1.0)
    G_far = 1.0 / (4.0 * np.pi * eps * rs) * (_erf(rs / (2 * gw)) - _erf(rs / np.sqrt(4 * gw2 + 1 / (split * split))))
    pi32 = np.pi ** 1.5
    invsp2 = 1.0 / (split * split)
    selfterm = 1.0 / (4 * pi32 * gw) - 1.0 / (2 * pi32 * np.sqrt(4 * gw2 + invsp2))
    r2term = 1.0 / (6.0 * pi32 * (4.0 * gw2 + invsp2) ** 1.5) - 1.0 / (48.0 * pi32 * gw2 * gw)
    r4term = 1.0 / (640.0 * pi32 * gw2 * gw2 * gw) - 1.0 / (20.0 * pi32 * (4 * gw2 + invsp2) ** 2.5)
    G_near = (selfterm + r2 * r2term + r2 * r2 * r4term) / eps
    return np.where(far, G_far, G_near)


def greens_near_field(r2, split, gw, eps):
    """NearField.cuh:37-61: the factor of r_ij in the field."""
    r2 = np.asarray(r2, dtype=np.float64)
    r = np.sqrt(r2)
    gw2 = gw * gw
    newgw = np.sqrt(gw2 + 1 / (4.0 * split * split))
    newgw2 = newgw * newgw
    far = r > gw * 1e-2
    rs = np.where(far, r, 1.0)
    invrterm = np.exp(-0.25 * rs * rs / newgw2) / np.sqrt(np.pi * newgw2) - np.exp(-0.25 * rs * rs / gw2) / np.sqrt(np.pi * gw2)
    invr2term = _erf(0.5 * rs / newgw) - _erf(0.5 * rs / gw)
    f_far = 1 / (4 * np.pi) * (invrterm / rs - invr2term / (rs * rs))
    pi32 = np.pi ** 1.5
    rterm = 1 / (24 * pi32) * (1.0 / (gw2 * gw) - 1 / (newgw2 * newgw))
    r3term = 1 / (160 * pi32) * (1.0 / (newgw2 * newgw2 * newgw) - 1.0 / (gw2 * gw2 * gw))
    f_near = r * rterm + r2 * r * r3term
    fmod = np.where(far, f_far, f_near)
    return np.where(r2 == 0, 0.0, fmod / (np.where(r2 == 0, 1.0, r) * eps))


def cut_off_distance(gw, split, eps_in, tolerance, nsd):
    """computeCutOffDistance (NearField.cuh:63-77)."""
    rn, dr = gw, gw * 0.01
    while True:
        rn += dr
        a = float(greens_near_field(rn * rn, split, gw / math.sqrt(2.0), eps_in))
        b = float(greens_near_field(rn * rn, 1e-10, gw / math.sqrt(2.0), eps_in))
        if not abs(a / b) > tolerance:
            break
    return rn + nsd * gw


_FORBIDDEN = (28, 98, 150, 154, 162, 196, 242)


def next_fft_wise(n):
    """nextFFTWiseSize3D (utils/Grid.cuh:140-215): 2^a 3^b 5^c 7^d 11^e with a >= 1, c <= 5, d <= 4, e <= 3, a few sizes barred."""
    c = max(int(n), 1)
    while True:
        m, ok = c, c % 2 == 0 and c not in _FORBIDDEN
        for p, emax in ((2, 64), (3, 64), (5, 5), (7, 4), (11, 3)):
            e = 0
            while m % p == 0:
                m //= p
                e += 1
            ok = ok and e <= emax
        if ok and m == 1:
            return c
        c += 1


def propose_cell_dim(gt, upsampling, L):
    """FarField.cuh:20-41."""
    h = gt / upsampling
    cx, cy = max(16, int(L[0] / h)), max(16, int(L[1] / h))
    cz = max(16, int(math.ceil(math.pi * 0.5 * L[2] / h)))
    cz = 2 * cz - 2
    cx, cy, cz = next_fft_wise(cx), next_fft_wise(cy), next_fft_wise(cz)
    return cx, cy, (cz + 2) // 2


def clencurt(i, n):
    """misc/ChevyshevUtils.cuh:13-30."""
    v = 1.0
    if n % 2 == 0:
        if i == 0 or i == n:
            return 1.0 / (n * n - 1.0)
        for k in range(1, n // 2):
            v -= 2 * math.cos(2 * k * math.pi * i / n) / (4.0 * k * k - 1)
        v -= math.cos(math.pi * i) / (n * n - 1.0)
    else:
        if i == 0 or i == n:
            return 1.0 / (n * n)
        for k in range(1, (n - 1) // 2 + 1):
            v -= 2 * math.cos(2 * k * math.pi * i / n) / (4.0 * k * k - 1)
    return 2.0 * v / n


class Parameters:
    def __init__(self, Lxy, H, gw, split=-1.0, Nxy=-1, permitivity=(1.0, 1.0, 1.0), tolerance=1e-4, upsampling=1.2, support=12,
                 numberStandardDeviations=4.0):
        """permitivity = (top, bottom, inside)."""
        self.Lxy, self.H, self.gw, self.split, self.Nxy = (float(Lxy[0]), float(Lxy[1])), float(H), float(gw), float(split), int(Nxy)
        self.permitivity = tuple(float(e) for e in permitivity)
        self.tolerance, self.upsampling, self.support, self.nsd = float(tolerance), float(upsampling), int(support), float(numberStandardDeviations)


class DPPoissonSlabRef:
    def __init__(self, par, real=np.float64, surface_top=None, surface_bottom=None):
        """surface_top / surface_bottom: callables (x, y) -> value, or None for zero."""
        self.real = real
        self.cplx = np.complex128 if real == np.float64 else np.complex64
        p = self.par = par
        et, eb, ei = p.permitivity
        split = p.split
        # initialization.cu:39-57
        if split <= 0:
            if p.Nxy <= 0:
                raise Refusal("Missing input parameters")
            gt0 = p.upsampling * p.Lxy[0] / p.Nxy
            split = math.sqrt(1 / (4 * (gt0 * gt0 - p.gw * p.gw)))
        elif p.Nxy > 0:
            raise Refusal("Invalid input parameters")
        smin, smax = 3.2 / (p.H + p.nsd * p.gw), 1 / (p.gw * math.sqrt(12))
        if split < smin or split > smax or not split == split:
            raise Refusal("Invalid splitting parameter")
        self.metTop, self.metBot = math.isinf(et), math.isinf(eb)
        if self.metBot and not self.metTop:
            raise Refusal("[DPPoissonSlab] Bottom metallic wall not implemented")
        self.split = split
        # FarField.cuh:96-131
        self.gt = math.sqrt(p.gw * p.gw + 1.0 / (4.0 * split * split))
        self.He = 1.25 * p.nsd * self.gt
        if self.He > min(p.Lxy[0], p.Lxy[1], p.H):
            raise Refusal("[DPPoissonSlab] Incompatible parameters")
        self.Htot = p.H + 6 * self.He
        self.cells = propose_cell_dim(self.gt, p.upsampling, (p.Lxy[0], p.Lxy[1], self.Htot))
        nx, ny, nz = self.cells
        self.h = p.Lxy[0] / nx
        self.hy = p.Lxy[1] / ny
        if p.support > min(nx, ny) or p.support < 1:
            raise Refusal("[DPPoissonSlab] the window support does not fit the grid")
        # NearField.cuh:116-147
        self.rcut = cut_off_distance(p.gw, split, ei, p.tolerance, p.nsd)
        if self.rcut > p.H:
            raise Refusal("[DPPoissonSlab] Incompatible parameters")
        self.ntable = max(1 << 16, min(1 << 20, 2 * int(self.rcut / (p.gw * p.tolerance * 1e2))))
        # spreadInterp.cuh:22-36, CorrectionCompute.cuh:297-305
        self.rmax = p.support * self.h * 0.5
        czmax = int(math.ceil((nz - 1) * (math.acos((0.5 * p.H + self.He) / (0.5 * self.Htot)) / math.pi)))
        self.supportZ = 2 * czmax + 1
        max_exp = 709.0 if real == np.float64 else 88.0
        self.kmax = min(max_exp / self.He, math.pi / self.h)
        self.thetaTop = math.acos((3 * self.He + p.H) / (0.5 * self.Htot) - 1)
        self.thetaBot = math.acos((3 * self.He) / (0.5 * self.Htot) - 1)
        self.zplane = 0.5 * self.Htot * np.cos(np.pi * np.arange(nz) / (nz - 1))
        self.qw = np.array([0.5 * self.Htot * clencurt(i, nz - 1) for i in range(nz)]) * (self.h * self.hy)
        ix = np.arange(nx)
        iy = np.arange(ny)
        kx = 2 * np.pi / p.Lxy[0] * (ix - nx * (ix >= nx // 2 + 1))
        ky = 2 * np.pi / p.Lxy[1] * (iy - ny * (iy >= ny // 2 + 1))
        self.kx = np.tile(kx, ny)
        self.ky = np.repeat(ky, nx)
        self.kmod = np.sqrt(self.kx ** 2 + self.ky ** 2)
        # for an even size the unpaired Nyquist index carries no x (y) derivative; an odd size has no unpaired index
        self.pairedX = np.tile(~((ix == nx // 2) & (nx % 2 == 0)), ny)
        self.pairedY = np.repeat(~((iy == ny // 2) & (ny % 2 == 0)), nx)
        self._tables = None
        self._near_table = None
        self.set_surface_values(surface_top, surface_bottom)
        self.outside_count = 0
        self.stage = {}

    # ------------------------------------------------------------------------------------------------------------ configuration
    def info(self):
        return dict(cells=tuple(self.cells), He=self.He, gt=self.gt, h=self.h, support=self.par.support, supportZ=self.supportZ,
                    nearFieldCutOff=self.rcut, nTable=self.ntable, kmax=self.kmax, split=self.split)

    def set_surface_values(self, top, bottom):
        nx, ny, _ = self.cells
        x = (np.arange(nx) / nx - 0.5) * self.par.Lxy[0]
        y = (np.arange(ny) / ny - 0.5) * self.par.Lxy[1]
        out = []
        for f in (top, bottom):
            v = np.zeros((ny, nx))
            if f is not None:
                for j in range(ny):
                    for i in range(nx):
                        v[j, i] = f(x[i], y[j])
            out.append((np.fft.fft2(v) / (nx * ny)).reshape(-1))
        self.surfTop, self.surfBot = out

    def set_surface_zero_mode(self, top, bottom):
        self.surfTop[0], self.surfBot[0] = top, bottom

    # ------------------------------------------------------------------------------------------------------------ spread / gather
    def _axis(self, x, L, n, h):
        """Nodes and weights of one periodic axis for the (scalar, `real`) coordinate x: IBM.cu:10-31, spreadInterp.cuh:52-59."""
        R, s = self.real, self.par.support
        x = R(x)
        xin = x - R(np.floor(x / R(L) + R(0.5))) * R(L)
        c = int((xin + R(0.5) * R(L)) * R(1.0 / h))
        if c == n:
            c = 0
        P = s // 2

        def dist(node):
            d = xin - (R(-0.5) * R(L) + R(h) * R(node))
            return d - R(np.floor(d / R(L) + R(0.5))) * R(L)
        if abs(dist(c - P)) > R(s) * R(h) / R(2.0):
            P -= 1
        nodes = c - P + np.arange(s)
        r = np.array([dist(m % n) for m in nodes], dtype=R)
        return nodes % n, self._phi(r)

    def _phi(self, r):
        R = self.real
        r = np.asarray(r, dtype=R)
        pref, tau = R(1.0 / (self.gt * math.sqrt(2 * math.pi))), R(-1.0 / (2.0 * self.gt * self.gt))
        return np.where(np.abs(r) > R(self.rmax) * R(1.000001), R(0), pref * np.exp(tau * r * r)).astype(R)

    def _sources(self, z, q):
        """(height, spread value, grid) of a particle: itself and its images; grid 0 = near-wall charges, 1 = the rest."""
        R, p = self.real, self.par
        et, eb, ei = p.permitivity
        half, thr = R(0.5 * p.H), R(2 * self.He)
        z, q = R(z), R(q)
        if not abs(z) <= half:
            return None
        near = abs(half - abs(z)) <= thr
        out = [(z, -q, 0 if near else 1)]
        if near and abs(half - z) <= thr:
            ratio = R(1.0) if math.isinf(et) else R((et / ei - 1) / (et / ei + 1))
            out.append((R(2.0) * half - z, q * ratio, 1))
        if near and abs(-half - z) <= thr:
            ratio = R(1.0) if math.isinf(eb) else R((eb / ei - 1) / (eb / ei + 1))
            out.append((R(-2.0) * half - z, q * ratio, 1))
        return out

    def spread(self, pos, q):
        R = self.real
        nx, ny, nz = self.cells
        grids = np.zeros((2, nz, ny, nx), dtype=R)
        zp = self.zplane.astype(R)
        self.outside_count = 0
        for a in range(len(q)):
            src = self._sources(pos[a, 2], q[a])
            if src is None:
                self.outside_count += 1
                continue
            jx, wx = self._axis(pos[a, 0], self.par.Lxy[0], nx, self.h)
            jy, wy = self._axis(pos[a, 1], self.par.Lxy[1], ny, self.hy)
            wxy = (wy[:, None] * wx[None, :]).astype(R)
            for zs, qs, g in src:
                wz = self._phi(zs - zp)
                ks = np.nonzero(wz)[0]
                grids[g][np.ix_(ks, jy, jx)] += (qs * wxy)[None, :, :] * wz[ks][:, None, None]
        return grids[0], grids[0] + grids[1]

    def gather(self, pos, field4):
        """field4: (4, nz, ny, nx) real.  -> (N, 4)"""
        R = self.real
        nx, ny, nz = self.cells
        zp, qw = self.zplane.astype(R), self.qw.astype(R)
        out = np.zeros((len(pos), 4), dtype=R)
        for a in range(len(pos)):
            z = R(pos[a, 2])
            if not abs(z) <= R(0.5 * self.par.H):
                continue
            jx, wx = self._axis(pos[a, 0], self.par.Lxy[0], nx, self.h)
            jy, wy = self._axis(pos[a, 1], self.par.Lxy[1], ny, self.hy)
            wz = self._phi(z - zp) * qw
            ks = np.nonzero(wz)[0]
            w = (wz[ks][:, None, None] * (wy[:, None] * wx[None, :])[None]).astype(R)
            for c in range(4):
                out[a, c] = (field4[c][np.ix_(ks, jy, jx)] * w).sum(dtype=R)
        return out

    # ------------------------------------------------------------------------------------------------------------ far field
    def _bvp_tables(self):
        if self._tables is None:
            Hh = 0.5 * self.Htot
            k = self.kmod
            nz_ = k != 0
            self._tables = cb.tables(k, Hh, self.cells[2], np.where(nz_, Hh, 0.0), np.where(nz_, Hh * Hh * k, 1.0), np.where(nz_, Hh, 0.0),
                                     np.where(nz_, -Hh * Hh * k, 1.0))
        return self._tables

    def _solve(self, fhat):
        """fhat: (nz, nsys) Chebyshev coefficients of the spread charges.  -> (phi_n, dphi_n) (BVPPoisson.cuh:38-97)."""
        R, C = self.real, self.cplx
        nz = self.cells[2]
        Hh = 0.5 * self.Htot
        fn = (fhat * R(1.0 / self.par.permitivity[2])).astype(C)
        zero = np.zeros((1, fn.shape[1]), dtype=C)
        cn, _ = cb.solve(self._bvp_tables(), Hh, fn[None], zero, zero, R)
        cn = cn[0]
        d = np.zeros_like(cn)
        for i in range(nz - 2, -1, -1):
            up = d[i + 2] if i + 2 < nz else 0
            d[i] = up + (R(2.0) * R(i + 1) * cn[i + 1]) * R(1.0 / Hh)
        d[0] = d[0] * R(0.5)
        return cn, d

    def _walls(self, cn, d):
        """(phi, Ez) at (top, bottom): the series at the two wall angles (MismatchCompute.cuh:118-134)."""
        R = self.real
        i = np.arange(self.cells[2])
        ct, cbm = np.cos(i * self.thetaTop).astype(R), np.cos(i * self.thetaBot).astype(R)
        acc = [np.zeros(cn.shape[1], dtype=self.cplx) for _ in range(4)]
        for n in range(len(i)):
            acc[0] = acc[0] + cn[n] * ct[n]
            acc[1] = acc[1] + cn[n] * cbm[n]
            acc[2] = acc[2] - d[n] * ct[n]
            acc[3] = acc[3] - d[n] * cbm[n]
        return acc  # phiTop, phiBot, EzTop, EzBot

    def far_field(self, pos, q):
        R, C, p = self.real, self.cplx, self.par
        nx, ny, nz = self.cells
        et, eb, ei = p.permitivity
        pos, q = np.asarray(pos), np.asarray(q)
        gnear, gall = self.spread(pos, q)
        self.stage["grid_near"], self.stage["grid_all"] = gnear, gall
        spec = [cb.fourier_chebyshev_forward(g.astype(C), R).reshape(nz, nx * ny) for g in (gnear, gall)]
        out_c, out_d = self._solve(spec[0])
        in_c, in_d = self._solve(spec[1])
        oT, oB, oET, oEB = self._walls(out_c, out_d)
        iT, iB, iET, iEB = self._walls(in_c, in_d)
        sT, sB = self.surfTop.astype(C), self.surfBot.astype(C)
        # MismatchCompute.cuh:50-84
        if not self.metTop:
            f = R(2.0 * ei / (et + ei))
            mPH = iT - f * oT
            mEH = R(et) * f * oET - R(ei) * iET - sT
        else:
            mEH = np.zeros_like(iT)
            mPH = iT - sT
        if not self.metBot:
            f = R(2.0 * ei / (eb + ei))
            mP0 = iB - f * oB
            mE0 = R(eb) * f * oEB - R(ei) * iEB + sB
        else:
            mE0 = np.zeros_like(iB)
            mP0 = iB - sB
        # computeLinearModeCorrection (MismatchCompute.cuh:86-115), wave number 0
        H = R(p.H)
        if self.metTop and not self.metBot:
            E = R(2.0 / (eb / ei + 1.0)) * oEB[0]
            A0 = E * R(eb / ei) - R(mE0[0].real) / R(ei)
            B0 = -mPH[0] - A0 * H
        elif self.metTop and self.metBot:
            A0 = -(mPH[0] - mP0[0]) / H
            B0 = -mP0[0]
        else:
            Cc = R(2.0 / (et / ei + 1.0)) * oET[0]
            E = R(2.0 / (eb / ei + 1.0)) * oEB[0]
            A0 = (E * R(eb / ei) - mE0[0] / R(ei) + Cc * R(et / ei) - mEH[0] / R(ei)) * R(0.5)
            B0 = C(0)
        self.stage["mismatch"] = np.concatenate([mP0, mPH, mE0, mEH, [A0, B0]]).astype(C)
        # the analytic correction at the planes, in double from the `real` mismatch (CorrectionCompute.cuh:13-121)
        dphi, phi = self._correction(mP0, mPH, mE0, mEH, A0, B0)
        cE = cb.chebyshev_forward(dphi.astype(C), R)
        cP = cb.chebyshev_forward(phi.astype(C), R)
        kx, ky = self.kx.astype(R), self.ky.astype(R)
        phin = in_c + cP
        sol = np.zeros((4, nz, nx * ny), dtype=C)
        sol[0] = (C(-1j) * kx * self.pairedX)[None, :] * phin
        sol[1] = (C(-1j) * ky * self.pairedY)[None, :] * phin
        sol[2] = -in_d - cE
        sol[3] = phin
        self.k0mode = sol[:, :, 0].T.copy()
        grid4 = np.stack([cb.fourier_chebyshev_inverse(s.reshape(nz, ny, nx), R).real.astype(R) for s in sol])
        self.stage["field_grid"] = grid4
        return self.gather(pos, grid4)

    def _correction(self, mP0, mPH, mE0, mEH, A0, B0):
        """(dphi/dz, phi) of the correction at the planes, (nz, nsys) complex128.  Every exponent is <= k He."""
        p = self.par
        et_, eb_, ei = p.permitivity
        H, He = p.H, self.He
        nz = self.cells[2]
        k = self.kmod.astype(self.real).astype(np.float64)
        mP0, mPH, mE0, mEH = [m.astype(np.complex128) for m in (mP0, mPH, mE0, mEH)]
        dphi = np.zeros((nz, k.shape[0]), dtype=np.complex128)
        phi = np.zeros_like(dphi)
        ok = (k <= self.kmax) & (k > 0)
        ks = np.where(ok, k, 1.0)
        for i in range(nz):
            zc = float(self.real(self.zplane[i]))
            if not abs(zc) < 0.5 * H + He:
                continue
            z = zc + 0.5 * H
            if not self.metTop and not self.metBot:
                eb, et = eb_ / ei, et_ / ei
                den = np.exp(-2.0 * H * ks) * (-1.0 + eb + et - eb * et) + (1.0 + eb) * (1.0 + et)
                a = mE0 / ei - eb * ks * mP0
                b = mEH / ei + et * ks * mPH
                ezm2H = np.exp(ks * (z - 2.0 * H)) * (-1.0 + et) * a
                emz = np.exp(-z * ks) * (1.0 + et) * a
                emHmz = np.exp((-H - z) * ks) * (-1.0 + eb) * b
                emHpz = np.exp(ks * (-H + z)) * (1.0 + eb) * b
                dz = -(ezm2H + emz + emHmz + emHpz) / den
                ph = (-ezm2H + emz + emHmz - emHpz) / (den * ks)
            elif self.metTop and self.metBot:
                e1, e2 = np.exp(-ks * H), np.exp(-2.0 * ks * H)
                first = (mPH - e1 * mP0) * np.exp(ks * (z - H)) / (e2 - 1.0)
                second = (-mP0 + e1 * mPH) / (1.0 - e2) * np.exp(-ks * z)
                dz = ks * first - ks * second
                ph = first + second
            else:
                eb = eb_ / ei
                e1, e2 = np.exp(-ks * H), np.exp(-2.0 * ks * H)
                den = ks * (e2 * (1.0 - eb) + (1.0 + eb))
                a = mE0 / ei + eb * ks * mP0
                AiE = (-(1.0 + eb) * ks * mPH + e1 * a) / den * np.exp(ks * (z - H))
                BiE = ((-1.0 + eb) * ks * mPH * e1 - a) / den * np.exp(-ks * z)
                dz = ks * AiE - ks * BiE
                ph = AiE + BiE
            dphi[i] = np.where(ok, dz, 0)
            phi[i] = np.where(ok, ph, 0)
            dphi[i, 0] = A0
            phi[i, 0] = complex(A0) * z + complex(B0)
        return dphi, phi

    # ------------------------------------------------------------------------------------------------------------ near field
    def near_table(self):
        if self._near_table is None:
            p = self.par
            R = self.real
            r2 = (np.arange(self.ntable) / float(self.ntable - 1)) * (self.rcut * self.rcut)
            r2 = r2.astype(R).astype(np.float64)
            self._near_table = (greens_near_potential(r2, self.split, p.gw, p.permitivity[2]).astype(R),
                                greens_near_field(r2, self.split, p.gw, p.permitivity[2]).astype(R))
        return self._near_table

    def _table(self, r2):
        """TabulatedFunction with linear interpolation on [0, rcut^2] (misc/TabulatedFunction.cuh)."""
        R = self.real
        tp, tf = self.near_table()
        rmax = R(self.rcut * self.rcut)
        nm1 = self.ntable - 1
        r2 = np.asarray(r2, dtype=R)
        r = r2 * R(1.0 / (self.rcut * self.rcut))
        i = np.clip((r * R(nm1)).astype(np.int64), 0, nm1 - 1)
        w = (r - i.astype(R) * R(1.0 / nm1)) * R(nm1)
        out = []
        for t in (tp, tf):
            v0, v1 = t[i], t[i + 1]
            v = v0 + w * (v1 - v0)
            v = np.where(r <= 0, t[0], v)
            out.append(np.where(r2 >= rmax, R(0), v).astype(R))
        return out

    def near_field(self, pos, q):
        R, p = self.real, self.par
        et, eb, ei = p.permitivity
        pos = np.asarray(pos).astype(R)
        q = np.asarray(q).astype(R)
        N = len(q)
        out = np.zeros((N, 4), dtype=R)
        half, H, rc = R(0.5 * p.H), R(p.H), R(self.rcut)
        inside = np.abs(pos[:, 2]) <= half
        L = np.array(p.Lxy, dtype=R)

        def ratio(e):
            return R(1.0) if math.isinf(e) else R((e - ei) / (e + ei))
        zj = pos[:, 2]
        has_image = np.abs(np.abs(zj) - half) < rc
        src = [(zj, q, inside)]
        e_near = np.where(zj < 0, ratio(eb), ratio(et)).astype(R)
        src.append((np.where(zj > 0, H, -H) - zj, -q * e_near, inside & has_image))
        if rc >= half:
            e_far = np.where(zj < 0, ratio(et), ratio(eb)).astype(R)
            src.append((np.where(zj > 0, -H, H) - zj, -q * e_far, inside & has_image))
        for a in range(N):
            if not inside[a]:
                continue
            dxy = pos[a, :2][None, :] - pos[:, :2]
            dxy = dxy - np.floor(dxy / L + R(0.5)) * L
            for zs, qs, on in src:
                dz = pos[a, 2] - zs
                r2 = (dxy[:, 0] * dxy[:, 0] + dxy[:, 1] * dxy[:, 1] + dz * dz).astype(R)
                gp, gf = self._table(r2)
                sel = on & (r2 < rc * rc)
                out[a, 0] += (qs * gf * dxy[:, 0])[sel].sum(dtype=R)
                out[a, 1] += (qs * gf * dxy[:, 1])[sel].sum(dtype=R)
                out[a, 2] += (qs * gf * dz)[sel].sum(dtype=R)
                out[a, 3] += (qs * gp)[sel].sum(dtype=R)
        return out

    def field_potential(self, pos, q):
        """(Ex, Ey, Ez, phi) at the particles: far field plus near field."""
        return self.far_field(pos, q) + self.near_field(pos, q)
