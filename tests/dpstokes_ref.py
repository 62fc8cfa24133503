"""NumPy restatement of the doubly periodic Stokes solver and its integrator's update rules, for the tests.

It takes nothing from the product.  Everything that runs per particle, per node or per wave number takes a `real` dtype: np.float64
is the reference the GPU tests compare against, np.float32 runs the same steps in single precision and measures the bars of the
single-precision tests.  What the product computes once on the host in double (window norms, plane heights, quadrature weights, BVP
tables, the slit matrices' inverses, the analytic correction's exponentials) is computed in double here too and cast.

Conventions.  A field has shape (nz, ny, nx); plane k lies at z_k = (H/2) cos(pi k / (nz - 1)), k = 0 at the top wall; node (i, j)
lies at ((i / nx - 1/2) Lx, (j / ny - 1/2) Ly).  Spectra are FULL planes of nx ny wave numbers, system s = i + nx j, with the
normalised forward transform (divided by nx ny) of tests/chebyshev_bvp_ref.py, so the k = 0 column of a velocity IS the plane average.
"""
import math

import numpy as np

import chebyshev_bvp_ref as cb
from dppoisson_ref import clencurt

MODES = ("none", "bottom", "slit")
MAX_SUPPORT = 16


class Refusal(ValueError):
    pass


def bm_norm(alpha, beta):
    """IBM_kernels::BarnettMagland::computeNorm: 2 * Simpson(BM, 0, alpha) on 20000 intervals."""
    n = 20000
    r = np.arange(n + 1) * (alpha / n)
    w = np.where(np.arange(n + 1) % 2 == 1, 4.0, 2.0)
    w[[0, n]] = 1.0
    z = r / alpha
    v = np.exp(beta * (np.sqrt(np.maximum(1.0 - z * z, 0.0)) - 1.0))
    return 2.0 * (alpha / n) / 3.0 * math.fsum(w * v)


class Parameters:
    def __init__(self, nx, ny, nz=-1, viscosity=0.0, Lx=0.0, Ly=0.0, H=0.0, w=6.0, beta=(-1.0, -1.0, -1.0), alpha=-1.0, mode="none"):
        self.nx, self.ny, self.nz, self.viscosity = int(nx), int(ny), int(nz), float(viscosity)
        self.Lx, self.Ly, self.H, self.w, self.alpha, self.mode = float(Lx), float(Ly), float(H), float(w), float(alpha), mode
        beta = (beta, -1.0, -1.0) if np.isscalar(beta) else beta
        self.beta = tuple(float(b) for b in beta)


class DPStokesRef:
    def __init__(self, par, real=np.float64):
        self.real = real
        self.cplx = np.complex128 if real == np.float64 else np.complex64
        p = self.par = par
        if p.viscosity <= 0:
            raise Refusal("[DPStokes] Viscosity was not set")
        if p.H <= 0:
            raise Refusal("[DPStokes] H (height) was not set")
        if p.Lx <= 0 or p.Ly <= 0:
            raise Refusal("[DPStokes] Domain width (Lx, Ly) was not set")
        if p.mode not in MODES:
            raise Refusal("unknown wall mode")
        nx, ny = p.nx, p.ny
        self.hx, self.hy = p.Lx / nx, p.Ly / ny
        nz = p.nz if p.nz >= 0 else int(math.pi * p.H / min(self.hx, self.hy))
        if nz < 4:
            raise Refusal("nz < 4")
        self.cells = (nx, ny, nz)
        self.support = int(p.w + 0.5)
        if self.support > MAX_SUPPORT:
            raise Refusal("support above 16")
        bx = p.beta[0]
        self.beta = (bx, p.beta[1] if p.beta[1] >= 0 else bx, p.beta[2] if p.beta[2] >= 0 else bx)
        self.alpha = p.alpha
        self.a = (self.hx, self.hy, min(self.hx, self.hy))
        self.invnorm = tuple(1.0 / bm_norm(self.alpha, b) for b in self.beta)
        self.rmax = p.w * max(self.hx, self.hy) * 0.5
        self.zplane = 0.5 * p.H * np.cos(np.pi * np.arange(nz) / (nz - 1))
        self.qw = np.array([0.5 * p.H * clencurt(i, nz - 1) for i in range(nz)]) * (self.hx * self.hy)
        ix, iy = np.arange(nx), np.arange(ny)
        kx = 2 * np.pi / p.Lx * (ix - nx * (ix >= nx // 2 + 1))
        ky = 2 * np.pi / p.Ly * (iy - ny * (iy >= ny // 2 + 1))
        self.kx, self.ky = np.tile(kx, ny), np.repeat(ky, nx)
        self.kmod = np.sqrt(self.kx ** 2 + self.ky ** 2)
        # ik is zero on the unpaired (Nyquist) index of an even size; an odd size has no unpaired index
        self.kxPaired = self.kx * np.tile(~((ix == nx // 2) & (nx % 2 == 0)), ny)
        self.kyPaired = self.ky * np.repeat(~((iy == ny // 2) & (ny % 2 == 0)), nx)
        self._tables = self._zero_tables = self._invA = None
        self.outside_count = 0
        self.stage = {}

    # ------------------------------------------------------------------------------------------------------------ window
    def _phi(self, r, axis):
        """bm.phi(r / a) / a (spreadInterp.cuh:112-118, IBM_kernels.cuh:83-112)."""
        R = self.real
        r = np.asarray(r, dtype=R)
        z = (r / R(self.a[axis])) / R(self.alpha)
        dz2 = R(1.0) - z * z
        k = np.exp(R(self.beta[axis]) * (np.sqrt(np.maximum(dz2, R(0))) - R(1.0)))
        return (np.where(dz2 < 0, R(0), k * R(self.invnorm[axis])) / R(self.a[axis])).astype(R)

    def _phi_z(self, z, zp):
        """phi(r) - phi(r_img): the image in the nearer wall is subtracted, in every mode (spreadInterp.cuh:122-129)."""
        R = self.real
        H = R(self.par.H)
        r = (R(z) - zp).astype(R)
        top, bot = H - R(2.0) * R(z) + r, -H - R(2.0) * R(z) + r
        rimg = np.minimum(np.abs(top), np.abs(bot))
        return (self._phi(r, 2) - self._phi(rimg, 2)).astype(R)

    def _axis(self, x, L, n, h, axis):
        """Nodes and weights of one periodic axis (IBM.cu:10-31)."""
        R, s = self.real, self.support
        x = R(x)
        xin = x - R(np.floor(x / R(L) + R(0.5))) * R(L)
        c = int((xin + R(0.5) * R(L)) * R(1.0 / h))
        if c == n:
            c = 0
        c = min(max(c, 0), n - 1)
        P = s // 2

        def dist(node):
            d = xin - (R(-0.5) * R(L) + R(h) * R(node))
            return d - R(np.floor(d / R(L) + R(0.5))) * R(L)
        if abs(dist(c - P)) > R(s) * R(h) / R(2.0):
            P -= 1
        nodes = c - P + np.arange(s)
        r = np.array([dist(m % n) for m in nodes], dtype=R)
        return nodes % n, self._phi(r, axis)

    def _inside(self, p):
        return bool(np.all(np.isfinite(p[:3])) and abs(self.real(p[2])) <= self.real(0.5 * self.par.H))

    def _weights(self, p):
        nx, ny, _ = self.cells
        jx, wx = self._axis(p[0], self.par.Lx, nx, self.hx, 0)
        jy, wy = self._axis(p[1], self.par.Ly, ny, self.hy, 1)
        wz = self._phi_z(p[2], self.zplane.astype(self.real))
        return jx, jy, (wy[:, None] * wx[None, :]).astype(self.real), wz

    def spread(self, pos, force):
        R = self.real
        nx, ny, nz = self.cells
        grid = np.zeros((3, nz, ny, nx), dtype=R)
        self.outside_count = 0
        for a in range(len(pos)):
            if not self._inside(pos[a]):
                self.outside_count += 1
                continue
            jx, jy, wxy, wz = self._weights(pos[a])
            ks = np.nonzero(wz)[0]
            w3 = (wxy[None, :, :] * wz[ks][:, None, None]).astype(R)
            for c in range(3):
                grid[c][np.ix_(ks, jy, jx)] += w3 * R(force[a, c])
        return grid

    def gather(self, pos, grid3):
        R = self.real
        qw = self.qw.astype(R)
        out = np.zeros((len(pos), 3), dtype=R)
        for a in range(len(pos)):
            if not self._inside(pos[a]):
                continue
            jx, jy, wxy, wz = self._weights(pos[a])
            wz = wz * qw
            ks = np.nonzero(wz)[0]
            w3 = (wxy[None, :, :] * wz[ks][:, None, None]).astype(R)
            for c in range(3):
                out[a, c] = (grid3[c][np.ix_(ks, jy, jx)] * w3).sum(dtype=R)
        return out

    # ------------------------------------------------------------------------------------------------------------ solve
    def _bvp_tables(self):
        if self._tables is None:
            Hh, k = 0.5 * self.par.H, self.kmod
            nzr = k != 0  # initialization.cu:74-96
            self._tables = cb.tables(k, Hh, self.cells[2], np.where(nzr, Hh, 0.0), np.where(nzr, Hh * Hh * k, 1.0), np.where(nzr, Hh, 0.0),
                                     np.where(nzr, -Hh * Hh * k, 1.0))
        return self._tables

    def _derivative(self, c):
        """Chebyshev coefficients of d/dz by the backward recurrence (BVPStokes.cuh:57-70)."""
        R = self.real
        nz, Hh = self.cells[2], 0.5 * self.par.H
        d = np.zeros_like(c)
        for i in range(nz - 2, -1, -1):
            up = d[i + 2] if i + 2 < nz else 0
            d[i] = up + (R(2.0) * R(i + 1) * c[i + 1]) * R(1.0 / Hh)
        d[0] = d[0] * R(0.5)
        return d

    def solve(self, fhat):
        """fhat: (3, nz, nsys) coefficients of the spread force.  -> (4, nz, nsys): u, v, w, p before the wall correction
        (BVPStokes.cuh:187-276); the k = 0 column is zero."""
        R, C = self.real, self.cplx
        Hh, mu = 0.5 * self.par.H, self.par.viscosity
        kx, ky, k = self.kxPaired.astype(R), self.kyPaired.astype(R), self.kmod.astype(R)
        fx, fy, fz = [f.astype(C) for f in fhat]
        tab = self._bvp_tables()
        nsys = fx.shape[1]
        zero = np.zeros((1, nsys), dtype=C)
        rhs = (C(1j) * (kx[None, :] * fx + ky[None, :] * fy) + self._derivative(fz)).astype(C)
        p = cb.solve(tab, Hh, rhs[None], zero, zero, R)[0][0]
        pH = np.zeros(nsys, dtype=C)
        pmH = np.zeros(nsys, dtype=C)
        for i in range(p.shape[0]):
            pH = pH + p[i]
            pmH = pmH + (p[i] if i % 2 == 0 else -p[i])
        ks = np.where(k > 0, k, R(1))
        on = (k > 0).astype(R)
        invmu = R(1.0 / mu)
        out = np.zeros((4,) + p.shape, dtype=C)
        for c, (kd, f) in enumerate(((kx, fx), (ky, fy))):
            r = ((C(1j) * kd[None, :] * p - f) * invmu).astype(C)
            fac = (R(0.5) * kd / (R(mu) * ks) * on).astype(R)
            al = (-fac * (C(1j) * pH)).astype(C)
            be = (fac * (C(1j) * pmH)).astype(C)
            out[c] = cb.solve(tab, Hh, r[None], al[None], be[None], R)[0][0]
        r = ((self._derivative(p) - fz) * invmu).astype(C)
        al = (R(0.5 / mu) * on * pH).astype(C)
        be = (R(0.5 / mu) * on * pmH).astype(C)
        out[2] = cb.solve(tab, Hh, r[None], al[None], be[None], R)[0][0]
        out[3] = p
        out[:, :, 0] = 0
        return out

    # ------------------------------------------------------------------------------------------------------------ wall correction
    def slit_matrix(self, kx, ky, k):
        """evaluateSlitCorrectionMatrix (Correction.cuh:493-566), row major, complex128.  (kx, ky) is the wave vector that multiplies i, zero
        on an unpaired index as in the solve; k the modulus of the full wave vector."""
        H, hm = self.par.H, 0.5 / self.par.viscosity
        e = math.exp(-k * H)
        A = np.zeros((8, 8), dtype=np.complex128)
        A[0, [0, 1, 6, 7]] = hm, e * hm, -k, k * e
        A[1, [0, 1, 6, 7]] = (1.0 - k * H) * e * hm, (1.0 + k * H) * hm, -k * e, k
        A[2, [2, 3]] = 1, e
        A[3, [4, 5]] = 1, e
        A[4, [6, 7]] = 1, e
        A[5, [0, 1, 2, 3]] = -1j * kx * H * e * hm / k, 1j * kx * H * hm / k, e, 1
        A[6, [0, 1, 4, 5]] = -1j * ky * H * e * hm / k, 1j * ky * H * hm / k, e, 1
        A[7, [0, 1, 6, 7]] = H * e * hm, H * hm, e, 1
        return A

    def slit_inverses(self):
        if self._invA is None:
            n = self.kmod.shape[0]
            self._invA = np.zeros((n, 8, 8), dtype=np.complex128)
            for s in range(1, n):
                self._invA[s] = np.linalg.inv(self.slit_matrix(self.kxPaired[s], self.kyPaired[s], self.kmod[s]))
        return self._invA

    def zero_mode_factors(self):
        """(tfi, tsi, bfi, bsi) of the k = 0 solve (Correction.cuh:44-68, :600-614)."""
        return (1.0, 0.0, 0.0, -1.0) if self.par.mode == "bottom" else (0.0, -1.0, 0.0, -1.0)

    def correction(self, sol, fhat):
        """The analytic correction in Chebyshev space plus the zero mode: (4, nz, nsys) to be added to `sol` (Correction.cuh)."""
        R, C = self.real, self.cplx
        mode, H, mu = self.par.mode, self.par.H, self.par.viscosity
        nz, nsys = sol.shape[1], sol.shape[2]
        top = [np.zeros(nsys, dtype=C) for _ in range(3)]
        bot = [np.zeros(nsys, dtype=C) for _ in range(3)]
        for c in range(3):
            for i in range(nz):
                top[c] = top[c] + sol[c, i]
                bot[c] = bot[c] + (sol[c, i] if i % 2 == 0 else -sol[c, i])
        # in double from the `real` wall values, as section 17 does
        u0, v0, w0 = [-(b.astype(np.complex128)) for b in bot]
        uH, vH, wH = [-(t.astype(np.complex128)) for t in top]
        kx, ky, k = self.kxPaired, self.kyPaired, self.kmod  # ik as the solve takes it: zero on an unpaired index
        ks = np.where(k > 0, k, 1.0)
        corr = np.zeros((4, nz, nsys), dtype=np.complex128)
        if mode == "slit":
            b = np.stack([-1j * (kx * u0 + ky * v0), -1j * (kx * uH + ky * vH), u0, v0, w0, uH, vH, wH], axis=1)
            Cc = np.einsum("sij,sj->si", self.slit_inverses(), b)
            hm = 0.5 / mu
        for i in range(nz):
            z = float(self.zplane[i]) + 0.5 * H
            ekz = np.exp(-ks * z)
            if mode == "slit":
                ekzmH = np.exp(ks * (z - H))
                par = -1j * hm / ks * z * (Cc[:, 0] * ekz - Cc[:, 1] * ekzmH)
                corr[0, i] = kx * par + Cc[:, 2] * ekz + Cc[:, 3] * ekzmH
                corr[1, i] = ky * par + Cc[:, 4] * ekz + Cc[:, 5] * ekzmH
                corr[2, i] = Cc[:, 0] * hm * z * ekz + Cc[:, 1] * hm * z * ekzmH + Cc[:, 6] * ekz + Cc[:, 7] * ekzmH
                corr[3, i] = Cc[:, 0] * z * ekz + Cc[:, 1] * ekzmH
            else:
                S = kx * u0 + ky * v0
                par = -(S + 1j * ks * w0) / ks * z * ekz
                corr[0, i] = kx * par + u0 * ekz
                corr[1, i] = ky * par + v0 * ekz
                corr[2, i] = (ks * w0 - 1j * S) * z * ekz + w0 * ekz
        corr[:, :, 0] = 0
        out = np.stack([cb.chebyshev_forward(corr[c].astype(C), R) for c in range(4)])
        # the zero mode: mu u'' = -f with the mode's boundary conditions, x and y only
        if self._zero_tables is None:
            f = self.zero_mode_factors()
            self._zero_tables = cb.tables([0.0], 0.5 * H, nz, [f[0]], [f[1]], [f[2]], [f[3]])
        zero = np.zeros((1, 1), dtype=C)
        for c in range(2):
            fn = (-(fhat[c][:, 0:1].astype(C)) * R(1.0 / mu)).astype(C)
            out[c, :, 0] = cb.solve(self._zero_tables, 0.5 * H, fn[None], zero, zero, R)[0][0][:, 0]
        return out.astype(C)

    # ------------------------------------------------------------------------------------------------------------ the call
    def fluid(self, pos, force):
        """The corrected Chebyshev-space (u, v, w, p): (4, nz, nsys)."""
        R, C = self.real, self.cplx
        nx, ny, nz = self.cells
        pos, force = np.asarray(pos), np.asarray(force)
        grid = self.spread(pos, force)
        self.stage["grid"] = grid
        fhat = np.stack([cb.fourier_chebyshev_forward(g.astype(C), R).reshape(nz, nx * ny) for g in grid])
        self.stage["fhat"] = fhat
        sol = self.solve(fhat)
        self.stage["uncorrected"] = sol
        if self.par.mode != "none":
            sol = (sol + self.correction(sol, fhat)).astype(C)
        return sol

    def Mdot(self, pos, force):
        R = self.real
        nx, ny, nz = self.cells
        sol = self.fluid(pos, force)
        self.stage["fluid"] = sol
        grid3 = np.stack([cb.fourier_chebyshev_inverse(sol[c].reshape(nz, ny, nx), R).real.astype(R) for c in range(3)])
        return self.gather(np.asarray(pos), grid3)

    def average_velocity(self, pos, force, direction=0):
        """computeAverageVelocity (DPStokesSlab.cuh:275-315): the k = 0 column of u (or v) summed at the planes."""
        if direction not in (0, 1):
            raise Refusal("[DPStokesSlab] Can only average in direction X (0) or Y (1)")
        nz = self.cells[2]
        c = self.fluid(pos, force)[direction][:, 0].real.astype(np.float64)
        i = np.arange(nz)
        return np.array([np.sum(c * np.cos(i * (j * np.pi / (nz - 1)))) for j in range(nz)])

    # ------------------------------------------------------------------------------------------------------------ integrator rules
    def thermal_drift(self, pos, W, temperature, dt, delta):
        """(T dt / delta) [M(q + delta W / 2) W - M(q - delta W / 2) W] (DPStokesSlab.cuh:436-456)."""
        R = self.real
        pos, W = np.asarray(pos, dtype=R), np.asarray(W, dtype=R)
        plus, minus = pos.copy(), pos.copy()
        plus[:, :3] = pos[:, :3] + R(0.5 * delta) * W
        minus[:, :3] = pos[:, :3] - R(0.5 * delta) * W
        return (R(dt * temperature / delta) * (self.Mdot(plus, W) - self.Mdot(minus, W))).astype(R)

    @staticmethod
    def update(pos, mf, dt, noise=None, noise_prev=None, rfd=None):
        """BDIntegrate (DPStokesSlab.cuh:395-418)."""
        R = pos.dtype.type
        d = mf * R(dt)
        if noise is not None:
            fl = R(dt) * R(0.5) * (noise + noise_prev) if noise_prev is not None else R(dt) * noise
            d = d + (fl + rfd)
        out = pos.copy()
        out[:, :3] = pos[:, :3] + d
        return out
