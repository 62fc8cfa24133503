"""NumPy restatement of Hydro::ICM_Compressible between two walls in z (ICM_Compressible_impl<Walls>: ICM_Compressible/GhostCells.cuh,
ICM_Compressible.cu:70-142, ICM_Compressible.cuh:374-434), written from the formulas; the scheme of icm_compressible_ref.py with the z
neighbours taken from explicit ghost planes.

A field is an array [nz + 2, ny, nx]: plane 0 lies below the bottom wall, plane nz + 1 above the top wall, planes 1 .. nz are the fluid.
x and y stay periodic.  Every interior cell is advanced by the periodic stencils (also g_z of the top layer, which lives on the top wall's
face); only the ghost planes know about the walls.  They are written by `walls`, any object with

    walls(which, rho_adj, v_adj, g_adj) -> (rho_ghost, v_ghost, g_ghost)      which = "bottom" | "top"; planes [ny, nx], v and g lists of 3
    walls.updateSimulationTime(t)                                             optional

where "adj" is the interior layer next to that wall.  Fills happen where the reference's do: on the initial fluid (fill, velocity to
momentum, fill, and once more), and after each Runge-Kutta sub-stage s = 1, 2, 3 in the order
    density and momentum update -> updateSimulationTime((steps + {1/3, 2/3, 1}) dt) -> fill -> v = g / face density on the interior (the
    top face reads the ghost density) -> fill.
The time (steps + 1/2) dt is sent before the forces and triggers no fill.  The particle windows do not see the walls: they wrap
periodically (misc/IBM.cu:41-59), so spread and gather are the periodic ones on the interior.  Thermal noise is refused: the reference
reads a ghost stress it never draws."""
import numpy as np

import icm_compressible_ref as ref


class MovingWalls:
    """The built-in rule: rho_ghost = rho_adj, v_ghost = 2 u - v_adj, g_ghost = 2 u rho_adj - g_adj with u = (u_x, u_y, 0) per wall
    (test/Hydro/ICM_Compressible/walltest.cu:38-71 for both tangential components and both walls).  velocities(t) -> ((bx, by), (tx, ty));
    the walls hold the velocities of the last time they heard, those of t = 0 before the first."""

    def __init__(self, velocities, dtype=np.float64):
        self.velocities, self.t = velocities, np.dtype(dtype).type
        self.updateSimulationTime(0.0)

    def updateSimulationTime(self, time):
        bottom, top = self.velocities(time)
        t = self.t
        self.u = {"bottom": [t(bottom[0]), t(bottom[1]), t(0)], "top": [t(top[0]), t(top[1]), t(0)]}

    def __call__(self, which, rho, v, g):
        t, u = self.t, self.u[which]
        return rho, [t(2) * u[c] - v[c] for c in range(3)], [t(2) * u[c] * rho - g[c] for c in range(3)]


class FreeSlipWalls:
    """another rule: the tangential velocity is continued evenly, the normal one reflected"""

    def __call__(self, which, rho, v, g):
        return rho, [v[0], v[1], -v[2]], [g[0], g[1], -g[2]]


def pad(f):
    """[nz, ny, nx] -> [nz + 2, ny, nx] with zero ghost planes"""
    return np.concatenate([np.zeros_like(f[:1]), f, np.zeros_like(f[:1])], 0)


class WallFluid(ref.Fluid):
    """ref.Fluid between two walls.  rho, v, g are the interior [nz, ny, nx] (views of the padded P_rho, P_v, P_g)."""

    def __init__(self, cells, L, shear, bulk, c, dt, walls, T=0.0, dtype=np.float64):
        if T > 0:
            raise ValueError("walls with temperature > 0: the reference reads a ghost stress it never draws")
        if int(cells[2]) < 1:
            raise ValueError("walls need at least one layer of cells in z")
        super().__init__(cells, L, shear, bulk, c, dt, T, dtype)
        self.walls = walls
        self._install(pad(self.rho), [pad(c) for c in self.g], [pad(c) for c in self.v])
        self.set()

    def _install(self, rho, g, v):
        self.P_rho, self.P_g, self.P_v = rho, g, v
        self.rho, self.g, self.v = rho[1:-1], [c[1:-1] for c in g], [c[1:-1] for c in v]

    def fill(self, rho, g, v):
        """fillGhostCells on one level, in place: both ghost planes from the adjacent interior layers"""
        for which, ghost, adj in (("bottom", 0, 1), ("top", -1, -2)):
            r, vv, gg = self.walls(which, rho[adj], [c[adj] for c in v], [c[adj] for c in g])
            rho[ghost] = r
            for c in range(3):
                v[c][ghost], g[c][ghost] = vv[c], gg[c]

    def update_time(self, time):
        if hasattr(self.walls, "updateSimulationTime"):
            self.walls.updateSimulationTime(time)

    def set(self, rho=None, v=None):
        """initializeFluid (:374-414) and setUpGhostCells (:418-422)"""
        shape = (self.n[2], self.n[1], self.n[0])
        if rho is not None:
            self.P_rho[1:-1] = np.array(rho, self.dtype).reshape(shape)
        if v is not None:
            for c in range(3):
                self.P_v[c][1:-1] = np.array(v[c], self.dtype).reshape(shape)
        self.fill(self.P_rho, self.P_g, self.P_v)
        for a in range(3):
            self.P_g[a][1:-1] = (self.P_v[a] * self.face_density(self.P_rho, a))[1:-1]
        self.fill(self.P_rho, self.P_g, self.P_v)
        self.fill(self.P_rho, self.P_g, self.P_v)

    def step_fluid(self, W=None, forcing=None):
        """the three Runge-Kutta sub-stages with their ghost fills: the fluid goes from n to n + 1.  The periodic operators run on the
        padded arrays: their wrap in z only reaches the ghost planes' own results, which the fills overwrite."""
        if W is not None:
            raise ValueError("walls with noise: the reference reads a ghost stress it never draws")
        t = self.t
        if forcing is not None:
            forcing = [pad(np.asarray(c, self.dtype)) for c in forcing]
        a = (self.P_rho, self.P_g)
        b = (self.P_rho, self.P_g, self.P_v)
        for (A, B, s), third in zip(ref.STAGES, (1.0 / 3.0, 2.0 / 3.0, 1.0)):
            B = t(B)
            combine = (lambda ua, x: x) if A == 0 else (lambda ua, x: ua + B * (x - ua))
            drho, dg = self.increments(b[0], b[1], b[2], None, t(0), forcing)
            rho = combine(a[0], b[0] + drho)
            g = [combine(a[1][c], b[1][c] + dg[c]) for c in range(3)]
            v = [np.zeros_like(rho) for _ in range(3)]          # (the first fill's velocities are overwritten by the second)
            self.update_time((self.steps + third) * float(self.dt))
            self.fill(rho, g, v)
            for c in range(3):
                v[c][1:-1] = (g[c] / self.face_density(rho, c))[1:-1]
            self.fill(rho, g, v)
            b = (rho, g, v)
        self._install(*b)
        self.steps += 1

    def forward(self, pos, force_fn=None, W=None):
        """one forwardTime; as ref.Fluid.forward, with the time (steps + 1/2) dt sent before the forces"""
        t = self.t
        q0 = np.array(pos, self.dtype)[:, :3]
        vn = [c.copy() for c in self.v]
        forcing = None
        if len(q0):
            qh = q0 + t(0.5) * self.dt * self.gather(q0, vn)
        self.update_time((self.steps + 0.5) * float(self.dt))
        if len(q0) and force_fn is not None:
            forcing = self.spread(qh, force_fn(qh))
        self.step_fluid(W, forcing)
        if not len(q0):
            return q0
        return q0 + t(0.5) * self.dt * self.gather(qh, [vn[a] + self.v[a] for a in range(3)])
