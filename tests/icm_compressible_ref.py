"""NumPy restatement of Hydro::ICM_Compressible (Integrator/Hydro/ICM_Compressible.cuh and ICM_Compressible/*.cuh), written from the
formulas; a test helper like sph_ref.py.  Triply periodic, fields as arrays [nz, ny, nx], every operation in `dtype`.

Staggered grid: rho at the cell centres r_i, g_a and v_a on the faces r_i + h_a/2.  With s_b the shift by one cell along b, one sub-stage
is U^c = A U^a + B (U^b + dU(U^b)) with

    d rho = -dt sum_b (g_b - s_-b g_b) / h_b
    d g_a = -dt [K_a + (pi(s_a rho) - pi(rho)) / h_a - eta L_a - (xi + eta/3) D_a] + N_a + dt f_a,     pi = c^2 rho
    K_a   = sum_b (Z_ab - s_-b Z_ab) / h_b,    Z_ab = 1/2 (g_b + s_a g_b) 1/2 (v_a + s_b v_a)
    L_a   = (sum_b (s_b v_a - 2 v_a + s_-b v_a) / h_b) / h_a                       (the reference's form: the Laplacian for cubic cells)
    D_a   = (sum_b (s_a v_b - s_a s_-b v_b - v_b + s_-b v_b) / h_b) / h_a
    N_a   = sum_b (W_ab - s_-b W_ab) / h_b,    W = W_A + w W_B
    v_a   = g_a / (1/2 (rho + s_a rho))

and (A, B, w) = (0, 1, -sqrt 3), (3/4, 1/4, +sqrt 3), (1/3, 2/3, 0), U^a the fluid at n, U^b the previous sub-stage.  The combination
is evaluated as U^a + B ((U^b + dU) - U^a) (A = 1 - B; the first sub-stage is U^b + dU alone), which returns U^a exactly when nothing
changes: with the rounded 1/3 and 2/3 the literal form moves a third of all float32 densities of a fluid at rest by one ulp.  The noise is
W[e, z, y, x, (A, B)], e = xx, yy, zz, xy, xz, yz: diagonal p_c w + p_t trace with w ~ N(0, 2), off-diagonal p_c w with w ~ N(0, 1),
p_c = sqrt(2 eta T dt / dV), p_t = sqrt(xi T dt / (3 dV)) - p_c / 3.  Particles: q^{n+1/2} = q^n + dt/2 J(q^n) v^n, forces at q^{n+1/2}
spread with the three-point Peskin window on the grid of each component (positions shifted by -h_a/2), q^{n+1} = q^n + dt/2 J(q^{n+1/2})
(v^n + v^{n+1})."""
import numpy as np

ENTRY = {(0, 0): 0, (1, 1): 1, (2, 2): 2, (0, 1): 3, (1, 0): 3, (0, 2): 4, (2, 0): 4, (1, 2): 5, (2, 1): 5}
STAGES = ((0.0, 1.0, -1.0), (0.75, 0.25, 1.0), (1.0 / 3.0, 2.0 / 3.0, 0.0))     # A, B, the sign of sqrt(3) W_B


def shift(f, a, k=1):
    """f at the cell k steps along axis a (0 = x): shift(f, 0)[z, y, x] = f[z, y, x + 1]"""
    return np.roll(f, -k, axis=2 - a)


def shift2(f, a, ka, b, kb):
    return shift(shift(f, a, ka), b, kb)


class Fluid:
    def __init__(self, cells, L, shear, bulk, c, dt, T=0.0, dtype=np.float64):
        self.dtype = np.dtype(dtype)
        t = self.t = self.dtype.type
        self.n = tuple(int(x) for x in cells)                                   # nx, ny, nz
        self.L = np.broadcast_to(np.asarray(L, dtype), (3,)).astype(dtype)
        self.h = (self.L / np.array(self.n).astype(dtype)).astype(dtype)
        self.dV = t(self.h[0] * self.h[1] * self.h[2])
        self.shear, self.bulk, self.c, self.dt, self.T = t(shear), t(bulk), t(c), t(dt), t(T)
        shape = (self.n[2], self.n[1], self.n[0])
        self.rho = np.ones(shape, dtype)
        self.v = [np.zeros(shape, dtype) for _ in range(3)]
        self.g = [np.zeros(shape, dtype) for _ in range(3)]
        self.steps = 0

    def centers(self):
        """(cell / n + 0.5) L per axis as [nz, ny, nx] arrays: where the reference evaluates its initial fields"""
        z, y, x = np.meshgrid(*[np.arange(m) for m in self.n[::-1]], indexing="ij")
        t = self.t
        return [(c.astype(self.dtype) / t(n) + t(0.5)) * l for c, n, l in zip((x, y, z), self.n, self.L)]

    def set(self, rho=None, v=None):
        if rho is not None:
            self.rho = np.array(rho, self.dtype).reshape(self.rho.shape)
        if v is not None:
            self.v = [np.array(c, self.dtype).reshape(self.rho.shape) for c in v]
        self.g = [self.v[a] * self.face_density(self.rho, a) for a in range(3)]

    def face_density(self, rho, a):
        return self.t(0.5) * (rho + shift(rho, a))

    def prefactors(self):
        t = self.t
        pc = np.sqrt((self.dt * t(2) * self.shear * self.T) / self.dV)
        pt = np.sqrt((self.dt * self.bulk * self.T) / (t(3) * self.dV)) - t(1) / t(3) * pc
        return t(pc), t(pt)

    def noise_from_normals(self, w):
        """w[6, nz, ny, nx, 2]: N(0, 2) in the first three entries and N(0, 1) in the others -> the stress W"""
        pc, pt = self.prefactors()
        w = np.asarray(w, self.dtype)
        W = pc * w
        trace = w[0] + w[1] + w[2]
        for e in range(3):
            W[e] = pc * w[e] + pt * trace
        return W

    def draw(self, rng):
        w = rng.standard_normal((6,) + self.rho.shape + (2,))
        w[:3] *= np.sqrt(2.0)
        return self.noise_from_normals(w.astype(self.dtype))

    def increments(self, rho, g, v, W, wB, forcing):
        t, h, dt = self.t, self.h, self.dt
        ih = [t(1) / h[a] for a in range(3)]
        div = np.zeros_like(rho)
        for b in range(3):
            div = div + ih[b] * (g[b] - shift(g[b], b, -1))
        drho = -div * dt
        dg = []
        c2 = self.c * self.c
        for a in range(3):
            kin = np.zeros_like(rho)
            for b in range(3):
                Z = (t(0.5) * (g[b] + shift(g[b], a))) * (t(0.5) * (v[a] + shift(v[a], b)))
                kin = kin + ih[b] * (Z - shift(Z, b, -1))
            grad_pi = ih[a] * (c2 * shift(rho, a) - c2 * rho)
            lap = [(shift(v[a], b) - t(2) * v[a] + shift(v[a], b, -1)) / h[b] for b in range(3)]
            lap = (lap[0] + lap[1] + lap[2]) / h[a]
            gd = [(shift(v[b], a) - shift2(v[b], a, 1, b, -1) - v[b] + shift(v[b], b, -1)) / h[b] for b in range(3)]
            gd = (gd[0] + gd[1] + gd[2]) / h[a]
            stress = -grad_pi + self.shear * lap + (self.bulk + self.shear / t(3)) * gd
            m = np.zeros_like(rho) + kin
            m = m - stress
            inc = -dt * m
            fl = np.zeros_like(rho)
            if W is not None:
                for b in range(3):
                    Zf = t(1) * W[ENTRY[a, b], ..., 0] + wB * W[ENTRY[a, b], ..., 1]
                    fl = fl + ih[b] * (Zf - shift(Zf, b, -1))
            f = forcing[a] if forcing is not None else np.zeros_like(rho)
            dg.append(inc + fl + dt * f)
        return drho, dg

    def step_fluid(self, W=None, forcing=None):
        """the three Runge-Kutta sub-stages: the fluid goes from n to n + 1"""
        t = self.t
        if W is not None:
            W = np.asarray(W, self.dtype)
        a = (self.rho, self.g)
        b = (self.rho, self.g, self.v)
        for A, B, s in STAGES:
            B, wB = t(B), t(s) * t(np.sqrt(t(3.0)))
            combine = (lambda ua, x: x) if A == 0 else (lambda ua, x: ua + B * (x - ua))     # A U^a + B x with A = 1 - B
            drho, dg = self.increments(b[0], b[1], b[2], W, wB, forcing)
            rho = combine(a[0], b[0] + drho)
            g = [combine(a[1][c], b[1][c] + dg[c]) for c in range(3)]
            v = [g[c] / self.face_density(rho, c) for c in range(3)]
            b = (rho, g, v)
        self.rho, self.g, self.v = b
        self.steps += 1

    # ---- particles ------------------------------------------------------------------------------------------------------------------------
    def phi(self, r):
        """three-point Peskin window of the distance r (in length units) with h = h_x, 1/h included"""
        t = self.t
        q = np.abs(r) / self.h[0]
        inner = (t(1) / t(3)) * (t(1) + np.sqrt(np.maximum(t(1) - t(3) * q * q, t(0))))
        omq = t(1) - q
        outer = (t(1) / t(6)) * (t(5) - t(3) * q - np.sqrt(np.maximum(t(1) - t(3) * omq * omq, t(0))))
        return np.where(q < t(0.5), inner, np.where(q < t(1.5), outer, t(0))) / self.h[0]

    def _pbc(self, d):
        return d - np.floor(d / self.L + self.t(0.5)) * self.L

    def stencil(self, pos, a):
        """cells [N, 27, 3] (x, y, z) and weights [N, 27] of the window of component a (positions shifted by -h_a / 2)"""
        t = self.t
        p = np.array(pos, self.dtype)[:, :3].copy()
        p[:, a] -= t(0.5) * self.h[a]
        n = np.array(self.n)
        cell = np.floor((self._pbc(p) + t(0.5) * self.L) / self.h).astype(np.int64)
        cell = np.where(cell == n, 0, cell)
        off = np.array([[i % 3 - 1, (i // 3) % 3 - 1, i // 9 - 1] for i in range(27)])
        cj = (cell[:, None, :] + off[None]) % n
        centre = (cj.astype(self.dtype) + t(0.5)) * self.h - t(0.5) * self.L
        r = self._pbc(p[:, None, :] - centre)
        w = self.phi(r[..., 0]) * self.phi(r[..., 1]) * self.phi(r[..., 2])
        return cj, w

    def gather(self, pos, v):
        """J(pos) v: [N, 3]"""
        out = np.zeros((len(pos), 3), self.dtype)
        for a in range(3):
            cj, w = self.stencil(pos, a)
            out[:, a] = (w * v[a][cj[..., 2], cj[..., 1], cj[..., 0]] * self.dV).sum(1)
        return out

    def spread(self, pos, F):
        """S(pos) F: three fields [nz, ny, nx]"""
        out = [np.zeros_like(self.rho) for _ in range(3)]
        F = np.asarray(F, self.dtype)
        for a in range(3):
            cj, w = self.stencil(pos, a)
            np.add.at(out[a], (cj[..., 2], cj[..., 1], cj[..., 0]), w * F[:, a, None])
        return out

    def forward(self, pos, force_fn=None, W=None):
        """one forwardTime: returns q^{n+1}; pos [N, >= 3] (an empty array: fluid only); force_fn(q^{n+1/2}) -> [N, 3]"""
        t = self.t
        q0 = np.array(pos, self.dtype)[:, :3]
        vn = [c.copy() for c in self.v]
        forcing = None
        if len(q0):
            qh = q0 + t(0.5) * self.dt * self.gather(q0, vn)
            if force_fn is not None:
                forcing = self.spread(qh, force_fn(qh))
        self.step_fluid(W, forcing)
        if not len(q0):
            return q0
        return q0 + t(0.5) * self.dt * self.gather(qh, [vn[a] + self.v[a] for a in range(3)])


# ---- the reference's random stream ---------------------------------------------------------------------------------------------------------
def saru_normals(oracle, seed, step, ncells, dtype=np.float64):
    """The 12 normals of every cell as the reference draws them: Saru(seed, step, cell), six single-precision Box-Muller pairs (oracle.saru_gf:
    sine first) on the generator's 32-bit stream; [6, ncells, 2], the first three entries with standard deviation sqrt(2) (fmaf(x, std, 0) is
    the rounded product).  Also returns the first 12 raw integers of every generator."""
    ints = np.stack([oracle.saru_u32((seed, step, i), 12) for i in range(ncells)])          # [ncells, 12]
    w = np.stack([oracle.saru_gf((seed, step, i), 0.0, 1.0, 6).reshape(6, 2) for i in range(ncells)], 1)      # float32 [6, ncells, 2]
    w[:3] *= np.float32(np.sqrt(np.float32(2)))
    return w.astype(dtype), ints
