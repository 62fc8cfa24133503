"""Host-side mirror of the reference's doubly periodic Stokes solver and its integrator (Integrator/BDHI/DoublyPeriodic/
DPStokesSlab.cuh): class names, parameters, error behaviour.  Every call goes through the C ABI (uammd_dpstokes_*, csrc/dpstokes.hip,
DESIGN.md 18); no CPU fallback."""
import ctypes as C

import torch

from . import _lib
from ._lib import check
from .md import Box, Integrator, _ptr, current_stream


class WallMode:
    """DPStokesSlab_ns::WallMode (StokesSlab/utils.cuh)."""
    none, bottom, slit = 0, 1, 2
    names = {"none": 0, "bottom": 1, "slit": 2}


def _mode(m):
    return WallMode.names[m] if isinstance(m, str) else int(m)


def _refusal(lib):
    msg = lib.uammd_hip_last_error().decode()
    # std::runtime_error("[DPStokes] Invalid argument") in the reference (initialization.cu:12-26, :54-57)
    return ValueError(msg) if msg.startswith(("[DPStokes]", "uammd_dpstokes")) else _lib.UammdHipError(msg)


class DPStokes:
    """DPStokesSlab_ns::DPStokes (DPStokesSlab.cuh:141-344): the mobility of particles in a fluid that is periodic in x and y and open,
    bounded by a bottom wall or confined in a slit, z in [-H/2, H/2].  `real` picks the build (the reference's DOUBLE_PRECISION); the
    calls take device arrays of that precision: positions (N, 3) or (N, 4), forces (N, 3) or (N, 4)."""
    WallMode = WallMode

    class Parameters:
        """DPStokes::Parameters (DPStokesSlab.cuh:149-174).  w_d, beta_d and alpha_d belong to the torque kernel, which is out of scope:
        they are accepted and not read."""

        def __init__(self, nx=0, ny=0, nz=-1, viscosity=0.0, Lx=0.0, Ly=0.0, H=0.0, w=0.0, w_d=0.0, beta=(-1.0, -1.0, -1.0),
                     beta_d=(-1.0, -1.0, -1.0), alpha=-1.0, alpha_d=-1.0, mode=WallMode.none):
            self.nx, self.ny, self.nz, self.viscosity, self.Lx, self.Ly, self.H = nx, ny, nz, viscosity, Lx, Ly, H
            self.w, self.w_d, self.beta, self.beta_d, self.alpha, self.alpha_d, self.mode = w, w_d, beta, beta_d, alpha, alpha_d, mode

    @staticmethod
    def _cpar(par):
        p = _lib.DPStokesParameters()
        p.nx, p.ny, p.nz = int(par.nx), int(par.ny), int(par.nz)
        p.viscosity, p.Lx, p.Ly, p.H, p.w, p.alpha = float(par.viscosity), float(par.Lx), float(par.Ly), float(par.H), float(par.w), float(par.alpha)
        beta = (par.beta, -1.0, -1.0) if isinstance(par.beta, (int, float)) else tuple(par.beta)
        for a in range(3):
            p.beta[a] = float(beta[a])
        p.mode = _mode(par.mode)
        return p

    @staticmethod
    def _info(info):
        return dict(cells=tuple(int(c) for c in info.cells), support=int(info.support), hx=float(info.hx), hy=float(info.hy),
                    rmax=float(info.rmax), beta=tuple(float(b) for b in info.beta))

    @staticmethod
    def configuration(par, real=torch.float32):
        """What the constructor would decide (cells, support, hx, hy, beta) or refuse, on the host: no GPU needed."""
        lib, info = _lib.load(), _lib.DPStokesInfo()
        if lib.uammd_dpstokes_create(C.byref(DPStokes._cpar(par)), int(real == torch.float64), None, C.byref(info)) != 0:
            raise _refusal(lib)
        return DPStokes._info(info)

    def __init__(self, par, real=torch.float32, _handle=None, _owner=None):
        self.lib = _lib.load()
        self.par, self.real, self.double = par, real, real == torch.float64
        self._owner = _owner  # an integrator's solver belongs to the integrator
        info = _lib.DPStokesInfo()
        if _handle is None:
            h = C.c_void_p()
            if self.lib.uammd_dpstokes_create(C.byref(self._cpar(par)), int(self.double), C.byref(h), C.byref(info)) != 0:
                raise _refusal(self.lib)
            self.h = h
        else:
            self.h = C.c_void_p(_handle)
            check(self.lib.uammd_dpstokes_create(C.byref(self._cpar(par)), int(self.double), None, C.byref(info)))
        self.info = self._info(info)
        self.cells = self.info["cells"]

    def __del__(self):
        try:
            if getattr(self, "h", None) and self._owner is None:
                self.lib.uammd_dpstokes_destroy(self.h)
            self.h = None
        except Exception:
            pass

    def set_option(self, name, value):
        check(self.lib.uammd_dpstokes_set_option(self.h, name.encode(), int(value)))

    def _rows(self, a, what):
        if a.dtype != self.real or a.dim() != 2 or a.shape[1] not in (3, 4) or not a.is_contiguous():
            raise ValueError(f"{what}: a contiguous (N, 3) or (N, 4) array of {self.real}")
        return int(a.shape[1])

    def Mdot(self, pos, forces, torques=None):
        """-> (N, 3) velocities M F.  Torques are not implemented (the dipole kernel is out of scope)."""
        if torques is not None:
            raise NotImplementedError("[DPStokes] Torques are not implemented")
        n = int(pos.shape[0])
        out = torch.zeros((n, 3), dtype=self.real, device=pos.device)
        fn = self.lib.uammd_dpstokes_mdot_f64 if self.double else self.lib.uammd_dpstokes_mdot
        check(fn(self.h, _ptr(pos), self._rows(pos, "pos"), _ptr(forces), self._rows(forces, "forces"), None, n, _ptr(out), current_stream()))
        return out

    def computeAverageVelocity(self, pos, forces, direction=0):
        """-> nz floats: the plane average of u (direction 0) or v (1) at the planes, plane 0 at the top wall."""
        import numpy as np
        if direction not in (0, 1):
            raise RuntimeError("[DPStokesSlab] Can only average in direction X (0) or Y (1)")
        out = (C.c_double * self.cells[2])()
        fn = self.lib.uammd_dpstokes_average_velocity_f64 if self.double else self.lib.uammd_dpstokes_average_velocity
        check(fn(self.h, _ptr(pos), self._rows(pos, "pos"), _ptr(forces), self._rows(forces, "forces"), int(pos.shape[0]), int(direction), out,
                 current_stream()))
        return np.array(out[:], dtype=np.float64)

    def fluid_cheb(self):
        """The corrected Chebyshev-space (u, v, w, p) of the last call: complex numpy array (4, nz, nx ny)."""
        nx, ny, nz = self.cells
        out = torch.zeros((4, nz, nx * ny, 2), dtype=self.real, device="cuda")
        fn = self.lib.uammd_dpstokes_fluid_cheb_f64 if self.double else self.lib.uammd_dpstokes_fluid_cheb
        check(fn(self.h, _ptr(out)))
        a = out.cpu().numpy()
        return a[..., 0] + 1j * a[..., 1]

    def outside_count(self):
        n = C.c_int()
        check(self.lib.uammd_dpstokes_outside_count(self.h, C.byref(n)))
        return n.value

    STAGES = ("classify", "spread", "forward (fx, fy)", "forward fz", "pressure solve", "velocity solves", "correction constants",
              "correction at the planes", "correction z passes", "zero mode + assemble", "inverse (u, v)", "inverse (w, p)", "gather")

    def stage_times(self):
        """Milliseconds per stage of the last call, after set_option('time_stages', 1): dict in the order of STAGES."""
        ms = (C.c_double * len(self.STAGES))()
        check(self.lib.uammd_dpstokes_stage_times(self.h, ms))
        return dict(zip(self.STAGES, [float(v) for v in ms]))


class DPStokesIntegrator(Integrator):
    """DPStokesSlab_ns::DPStokesIntegrator (DPStokesSlab.cuh:424-583): Brownian dynamics with the DPStokes mobility; fluctuations by
    Lanczos, the thermal drift by random finite differences.  real = torch.float64 keeps a double copy of the positions between steps
    (pd's stay single precision) — the reference's DOUBLE_PRECISION build."""

    class Parameters(DPStokes.Parameters):
        """DPStokesIntegrator::Parameters (DPStokesSlab.cuh:499-505) plus deltaRFD, the random-finite-difference step (the reference's
        1e-6, fixed there), and the seeds (0: drawn from pd's generator as the reference draws them)."""

        def __init__(self, temperature=0.0, useLeimkuhler=False, dt=0.0, tolerance=1e-7, deltaRFD=-1.0, seed=0, seedRFD=0, **kw):
            super().__init__(**kw)
            self.temperature, self.useLeimkuhler, self.dt, self.tolerance = temperature, useLeimkuhler, dt, tolerance
            self.deltaRFD, self.seed, self.seedRFD = deltaRFD, seed, seedRFD

    def __init__(self, pd, par, real=torch.float32):
        super().__init__(pd)
        self.lib = _lib.load()
        self.par, self.real, self.double = par, real, real == torch.float64
        self.seed = par.seed if par.seed else (pd.rng.next32() if pd is not None else 1)       # DPStokesSlab.cuh:520-521
        self.seedRFD = par.seedRFD if par.seedRFD else (pd.rng.next32() if pd is not None else 2)
        ip = _lib.DPStokesIntegratorParameters()
        ip.temperature, ip.dt, ip.tolerance, ip.deltaRFD = float(par.temperature), float(par.dt), float(par.tolerance), float(par.deltaRFD)
        ip.useLeimkuhler, ip.seed, ip.seedRFD = int(bool(par.useLeimkuhler)), int(self.seed) & 0xFFFFFFFF, int(self.seedRFD) & 0xFFFFFFFF
        h = C.c_void_p()
        if self.lib.uammd_dpstokes_integrator_create(C.byref(DPStokes._cpar(par)), C.byref(ip), int(self.double), C.byref(h)) != 0:
            raise _refusal(self.lib)
        self.h = h
        self.dpstokes = DPStokes(par, real, _handle=self.lib.uammd_dpstokes_integrator_solver(h), _owner=self)
        self._pos64 = None

    def __del__(self):
        try:
            if getattr(self, "h", None):
                self.lib.uammd_dpstokes_integrator_destroy(self.h)
                self.h = None
        except Exception:
            pass

    def _sfx(self, name):
        return getattr(self.lib, name + ("_f64" if self.double else ""))

    # ---- arrays of the handle's precision
    def step_arrays(self, pos, force):
        """One update of `pos` (in place) under `force`, both device arrays of the handle's precision."""
        check(self._sfx("uammd_dpstokes_integrator_step")(self.h, _ptr(pos), self.dpstokes._rows(pos, "pos"), _ptr(force),
                                                          self.dpstokes._rows(force, "force"), int(pos.shape[0]), current_stream()))

    def thermal_drift(self, pos, W):
        """(T dt / delta) [M(q + delta W / 2) W - M(q - delta W / 2) W] for the caller's W (N, 3)."""
        out = torch.zeros((int(pos.shape[0]), 3), dtype=self.real, device=pos.device)
        self.dpstokes._rows(W, "W")
        check(self._sfx("uammd_dpstokes_integrator_thermal_drift")(self.h, _ptr(pos), self.dpstokes._rows(pos, "pos"), _ptr(W),
                                                                   int(pos.shape[0]), _ptr(out), current_stream()))
        return out

    def fluctuations(self, pos, W):
        """M^(1/2) W for the caller's W (N, 3), by Lanczos at the integrator's tolerance."""
        out = torch.zeros((int(pos.shape[0]), 3), dtype=self.real, device=pos.device)
        if W.shape[1] != 3:
            raise ValueError("W: (N, 3)")
        self.dpstokes._rows(W, "W")
        check(self._sfx("uammd_dpstokes_integrator_fluctuations")(self.h, _ptr(pos), self.dpstokes._rows(pos, "pos"), _ptr(W),
                                                                  int(pos.shape[0]), _ptr(out), current_stream()))
        return out

    LAST = {"mf": 0, "fluctuations": 1, "drift": 2, "previous_fluctuations": 3}

    def last(self, name, n):
        """Test hook: what the last step added up, (n, 3): 'mf', 'fluctuations', 'drift', 'previous_fluctuations'."""
        out = torch.zeros((n, 3), dtype=self.real, device="cuda")
        check(self.lib.uammd_dpstokes_integrator_last(self.h, self.LAST[name], n, _ptr(out)))
        return out

    # ---- the Integrator's call, on pd
    def forwardTime(self):
        pd, par = self.pd, self.par
        if self.steps == 0:  # setUpInteractors (DPStokesSlab.cuh:569-578)
            box = Box([float(par.Lx), float(par.Ly), float(par.H)])
            box.setPeriodicity(1, 1, 0)
            for it in self.interactors:
                it.updateBox(box)
                it.updateTimeStep(par.dt)
                it.updateTemperature(par.temperature)
                if hasattr(it, "updateViscosity"):
                    it.updateViscosity(par.viscosity)
        pd.getForce("write").zero_()
        for it in self.interactors:
            it.updateSimulationTime(par.dt * self.steps)
            it.sum(force=True)
        if hasattr(pd, "torque") and getattr(pd, "torque", None) is not None:
            raise RuntimeError("[DPStokes] Torques are not yet implemented")
        pos, force = pd.getPos("readwrite"), pd.getForce("read")
        if not self.double:
            self.step_arrays(pos, force)
        else:
            if self._pos64 is None or self._pos64.shape != pos.shape or not torch.equal(self._pos64.float(), pos):
                self._pos64 = pos.double()
            self.step_arrays(self._pos64, force.double())
            pos.copy_(self._pos64.float())
        self.steps += 1
