"""Host-side mirror of the reference's triply periodic electrostatics Interactor (Interactor/SpectralEwaldPoisson.cuh):
class names, parameters, error behaviour.  Every call goes through the C ABI (uammd_poisson_*); no CPU fallback."""
import ctypes as C

import torch

from . import _lib
from ._lib import PoissonInfo, PoissonParameters, check
from .md import Interactor, _ptr, current_stream


class Poisson(Interactor):
    """Poisson(pd, par) — SpectralEwaldPoisson.cuh:83-136."""

    class Parameters:
        """Poisson::Parameters (SpectralEwaldPoisson.cuh:94-103).  cells and support exist in the reference's struct but its
        constructor never reads them; they are accepted and ignored here too."""

        def __init__(self, box=None, epsilon=-1.0, tolerance=1e-5, gw=-1.0, split=-1.0, upsampling=-1.0, cells=(-1, -1, -1),
                     support=-1):
            self.box, self.epsilon, self.tolerance, self.gw, self.split = box, epsilon, tolerance, gw, split
            self.upsampling, self.cells, self.support = upsampling, cells, support

    def __init__(self, pd, par):
        self.lib = _lib.load()
        self.pd = pd
        p = PoissonParameters()
        for k in range(3):
            p.boxSize[k] = float(par.box.boxSize[k])
        p.epsilon, p.tolerance, p.gw, p.split, p.upsampling = (float(par.epsilon), float(par.tolerance), float(par.gw),
                                                                float(par.split), float(par.upsampling))
        h, info = C.c_void_p(), PoissonInfo()
        try:
            check(self.lib.uammd_poisson_create(C.byref(p), C.byref(h), C.byref(info)))
        except _lib.UammdHipError as e:
            if "[Poisson]" in str(e):   # std::invalid_argument in the reference (.cu:95-102, :111-116)
                raise ValueError(str(e)) from e
            raise
        self.h = h
        self.box, self.epsilon, self.split, self.gw, self.tolerance = par.box, par.epsilon, par.split, par.gw, par.tolerance
        self.cells, self.support = [int(c) for c in info.cells], int(info.support)
        self.nearFieldCutOff, self.nTable, self.cellSize = float(info.nearFieldCutOff), int(info.nTable), float(info.h)

    def __del__(self):
        try:
            if getattr(self, "h", None):
                self.lib.uammd_poisson_destroy(self.h)
                self.h = None
        except Exception:
            pass

    def set_option(self, name, value):
        check(self.lib.uammd_poisson_set_option(self.h, name.encode(), int(value)))

    def sum(self, force=False, energy=False, virial=False):
        """Poisson::sum (SpectralEwaldPoisson.cuh:110-123): far field (adds to force AND energy), then the near-field passes."""
        if virial:
            raise RuntimeError("[Poisson] not implemented")
        pd = self.pd
        check(self.lib.uammd_poisson_sum(self.h, _ptr(pd.getPos("read")), _ptr(pd.getCharge("read")), pd.N,
                                         _ptr(pd.getForce("readwrite")), _ptr(pd.getEnergy("readwrite")), int(bool(force)),
                                         int(bool(energy)), current_stream()))

    def computeFieldPotentialAtParticles(self):
        """-> real4[N] (Ex, Ey, Ez, phi); like the reference's call it also adds the far field to pd force/energy."""
        pd = self.pd
        out = torch.zeros((pd.N, 4), dtype=torch.float32, device=pd.device)
        check(self.lib.uammd_poisson_field_potential(self.h, _ptr(pd.getPos("read")), _ptr(pd.getCharge("read")), pd.N, _ptr(out),
                                                     _ptr(pd.getForce("readwrite")), _ptr(pd.getEnergy("readwrite")),
                                                     current_stream()))
        return out

    SPREAD, CONVOLVE, GATHER = 0, 1, 2
    GATHER_FORMS = {1: "col1", 2: "col2", 3: "flat"}

    def probe(self, stage, pos=None, charge=None, grid=None, fieldPotential=None, force=None, energy=None):
        """Test hook (uammd_poisson_probe): one stage of the far field alone, on the caller's device arrays instead of pd's.
        SPREAD (pos, charge) -> the charge grid float[nz][ny][nxpad]; CONVOLVE (grid: a charge grid) -> the float4 grid
        [nz][ny][nxpad][4]; GATHER (pos, charge, grid: a float4 grid) adds to fieldPotential (created as zeros if None) and to the
        optional force / energy.  Returns (result, info): info = dict(tile, waves, S, gather) of what ran (tile-owned spread: waves > 0,
        S = 0 for the generic body; gather: 'col1', 'col2' or 'flat')."""
        nx, ny, nz = self.cells
        nxpad = 2 * (nx // 2 + 1)
        n = 0 if pos is None else int(pos.shape[0])
        if stage == self.SPREAD:
            out = torch.empty((nz, ny, nxpad), dtype=torch.float32, device="cuda")
        elif stage == self.CONVOLVE:
            out = torch.empty((nz, ny, nxpad, 4), dtype=torch.float32, device="cuda")
        else:
            out = torch.zeros((n, 4), dtype=torch.float32, device="cuda") if fieldPotential is None else fieldPotential
        if grid is not None:
            want = (nz, ny, nxpad) if stage == self.CONVOLVE else (nz, ny, nxpad, 4)
            if tuple(grid.shape) != want or grid.dtype != torch.float32 or not grid.is_contiguous():
                raise ValueError(f"probe: grid must be a contiguous float32 array of shape {want}")
        info = (C.c_int * 6)()
        check(self.lib.uammd_poisson_probe(self.h, int(stage), _ptr(pos), _ptr(charge), n, _ptr(grid), _ptr(out), _ptr(force),
                                           _ptr(energy), info, current_stream()))
        return out, dict(tile=(info[0], info[1], info[2]), waves=info[3], S=info[4], gather=self.GATHER_FORMS.get(info[5]))


class DPPoissonSlab(Interactor):
    """DPPoissonSlab(pd, par) — Interactor/DoublyPeriodic/DPPoissonSlab.cuh:17-96: charges between two walls at z = +-H/2, periodic in x
    and y.  `real` picks the build: torch.float32 works on pd's arrays; torch.float64 (the reference's DOUBLE_PRECISION) computes on
    double copies of them and adds the results back.  The *_arrays calls take arrays of the handle's precision directly."""

    class Permitivity:
        def __init__(self, top=1.0, bottom=1.0, inside=1.0):
            self.top, self.bottom, self.inside = top, bottom, inside

    class SurfaceValueDispatch:
        """Surface charge density of a wall — or its potential when the wall is metallic (infinite permittivity)."""

        def top(self, x, y):
            return 0.0

        def bottom(self, x, y):
            return 0.0

    class Parameters:
        """DPPoissonSlab::Parameters (DPPoissonSlab.cuh:21-38)."""

        def __init__(self, Lxy=None, H=0.0, gw=-1.0, split=-1.0, Nxy=-1, permitivity=None, tolerance=1e-4, upsampling=1.2, support=12,
                     numberStandardDeviations=4.0, surfaceValues=None, printK0Mode=False):
            self.Lxy, self.H, self.gw, self.split, self.Nxy = Lxy, H, gw, split, Nxy
            self.permitivity = permitivity if permitivity is not None else DPPoissonSlab.Permitivity()
            self.tolerance, self.upsampling, self.support = tolerance, upsampling, support
            self.numberStandardDeviations, self.surfaceValues, self.printK0Mode = numberStandardDeviations, surfaceValues, printK0Mode

    @staticmethod
    def _cpar(par):
        p = _lib.DPPoissonParameters()
        p.Lxy[0], p.Lxy[1] = float(par.Lxy[0]), float(par.Lxy[1])
        p.H, p.gw, p.split, p.Nxy = float(par.H), float(par.gw), float(par.split), int(par.Nxy)
        p.permitivity[0], p.permitivity[1], p.permitivity[2] = (float(par.permitivity.top), float(par.permitivity.bottom),
                                                                float(par.permitivity.inside))
        p.tolerance, p.upsampling, p.support = float(par.tolerance), float(par.upsampling), int(par.support)
        p.numberStandardDeviations = float(par.numberStandardDeviations)
        return p

    @staticmethod
    def _info(info):
        return dict(cells=tuple(int(c) for c in info.cells), He=float(info.He), gt=float(info.gt), h=float(info.h), support=int(info.support),
                    supportZ=int(info.supportZ), nearFieldCutOff=float(info.nearFieldCutOff), nTable=int(info.nTable), kmax=float(info.kmax),
                    split=float(info.split))

    @staticmethod
    def _create(lib, par, double, handle):
        info = _lib.DPPoissonInfo()
        if lib.uammd_dppoisson_create(C.byref(DPPoissonSlab._cpar(par)), int(double), handle, C.byref(info)) != 0:
            msg = lib.uammd_hip_last_error().decode()
            # std::invalid_argument / runtime_error in the reference (initialization.cu:15-84, FarField.cuh:43-51, NearField.cuh:79-88)
            refusal = msg.startswith(("Missing input", "Invalid input", "Invalid splitting", "[DPPoissonSlab]"))
            raise ValueError(msg) if refusal else _lib.UammdHipError(msg)
        return DPPoissonSlab._info(info)

    @staticmethod
    def configuration(par, real=torch.float32):
        """What the constructor would decide (cells, He, gt, h, supports, near cut-off, table size, kmax), on the host: no GPU needed."""
        return DPPoissonSlab._create(_lib.load(), par, real == torch.float64, None)

    def __init__(self, pd, par, real=torch.float32):
        self.lib = _lib.load()
        self.pd, self.par, self.real = pd, par, real
        self.double = real == torch.float64
        h = C.c_void_p()
        self.info = self._create(self.lib, par, self.double, C.byref(h))
        self.h = h
        self.cells = self.info["cells"]
        if par.surfaceValues is not None:
            nx, ny = self.cells[0], self.cells[1]
            top, bottom = (C.c_double * (nx * ny))(), (C.c_double * (nx * ny))()
            for j in range(ny):
                for i in range(nx):
                    x, y = (i / nx - 0.5) * float(par.Lxy[0]), (j / ny - 0.5) * float(par.Lxy[1])
                    top[i + nx * j] = float(par.surfaceValues.top(x, y))
                    bottom[i + nx * j] = float(par.surfaceValues.bottom(x, y))
            check(self.lib.uammd_dppoisson_set_surface_values(self.h, top, bottom))

    def __del__(self):
        try:
            if getattr(self, "h", None):
                self.lib.uammd_dppoisson_destroy(self.h)
                self.h = None
        except Exception:
            pass

    def set_option(self, name, value):
        check(self.lib.uammd_dppoisson_set_option(self.h, name.encode(), int(value)))

    def setSurfaceValuesZeroModeFourier(self, top, bottom):
        check(self.lib.uammd_dppoisson_set_surface_zero_mode(self.h, float(top), float(bottom)))

    # ---- arrays of the handle's precision
    def sum_arrays(self, pos, charge, force, energy, virial=False):
        fn = self.lib.uammd_dppoisson_sum_f64 if self.double else self.lib.uammd_dppoisson_sum
        check(fn(self.h, _ptr(pos), _ptr(charge), int(pos.shape[0]), _ptr(force), _ptr(energy), int(bool(virial)), current_stream()))

    def field_potential_arrays(self, pos, charge, force=None, energy=None):
        n = int(pos.shape[0])
        out = torch.zeros((n, 4), dtype=self.real, device=pos.device)
        force = torch.zeros((n, 4), dtype=self.real, device=pos.device) if force is None else force
        energy = torch.zeros((n,), dtype=self.real, device=pos.device) if energy is None else energy
        fn = self.lib.uammd_dppoisson_field_potential_f64 if self.double else self.lib.uammd_dppoisson_field_potential
        check(fn(self.h, _ptr(pos), _ptr(charge), n, _ptr(out), _ptr(force), _ptr(energy), current_stream()))
        return out

    # ---- the Interactor's calls, on pd
    def _on_pd(self, call):
        pd = self.pd
        pos, charge, force, energy = pd.getPos("read"), pd.getCharge("read"), pd.getForce("readwrite"), pd.getEnergy("readwrite")
        if not self.double:
            return call(pos, charge, force, energy)
        f64, e64 = torch.zeros_like(force, dtype=torch.float64), torch.zeros_like(energy, dtype=torch.float64)
        out = call(pos.double(), charge.double(), f64, e64)
        force += f64.float()
        energy += e64.float()
        return out

    def sum(self, force=False, energy=False, virial=False):
        """DPPoissonSlab::sum (DPPoissonSlab.cuh:47-55): both parts always run and always add to force and energy."""
        if virial:
            raise RuntimeError("[Poisson] not implemented")
        self._on_pd(lambda p, q, f, e: self.sum_arrays(p, q, f, e))

    def computeFieldPotentialAtParticles(self):
        """-> real4[N] (Ex, Ey, Ez, phi); like the reference's call it also adds to pd's force and energy."""
        return self._on_pd(lambda p, q, f, e: self.field_potential_arrays(p, q, f, e))

    def computeFieldAtParticles(self):
        """Deprecated in the reference (DPPoissonSlab.cuh:57-72): the same with w zeroed."""
        out = self.computeFieldPotentialAtParticles()
        out[:, 3] = 0
        return out

    def getK0Mode(self):
        """The corrected k = 0 column of the last call: complex array (nz, 4) = (Ex, Ey, Ez, phi)."""
        import numpy as np
        nz = self.cells[2]
        buf = (C.c_double * (8 * nz))()
        check(self.lib.uammd_dppoisson_get_k0_mode(self.h, buf))
        a = np.frombuffer(buf, dtype=np.float64).reshape(nz, 4, 2)
        return a[..., 0] + 1j * a[..., 1]

    def outside_count(self):
        n = C.c_int()
        check(self.lib.uammd_dppoisson_outside_count(self.h, C.byref(n)))
        return n.value

    STAGES = ("classify", "spread", "forward transform", "solve + mismatch", "correction", "z pass dphi", "z pass phi", "assemble",
              "inverse (Ex, Ey)", "inverse (Ez, phi)", "gather", "cell list + pack", "near field")

    def stage_times(self):
        """Milliseconds per stage of the last call, after set_option('time_stages', 1): dict in the order of STAGES."""
        ms = (C.c_double * len(self.STAGES))()
        check(self.lib.uammd_dppoisson_stage_times(self.h, ms))
        return dict(zip(self.STAGES, [float(v) for v in ms]))

    def get_stage(self, name):
        """Test hook: 'grid_near', 'grid_all' (nz, ny, nx) after set_option('keep_stages', 1); 'mismatch' (4 nx ny + 2 complex)."""
        nx, ny, nz = self.cells
        if name == "mismatch":
            out = torch.zeros((4 * nx * ny + 2, 2), dtype=self.real, device="cuda")
        else:
            out = torch.zeros((nz, ny, nx), dtype=self.real, device="cuda")
        check(self.lib.uammd_dppoisson_get_stage(self.h, name.encode(), _ptr(out)))
        return out
