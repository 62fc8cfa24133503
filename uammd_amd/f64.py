"""DOUBLE_PRECISION build of path B (the `_f64` entry points of include/uammd_hip.h): the reference makes `real` a build switch
(global/defines.h:9-11) and compiles every accuracy assertion it ships in double.  Thin mirrors of the same classes, arrays are
torch.float64 on the GPU: positions / forces real4 = double[N, 4], velocities real3 = double[N, 3]."""
import ctypes as C
import math

import numpy as np
import torch

from . import _lib
from ._lib import FCMParameters64, IBMKernel64, MATVEC64, check


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _d3(v):
    v = np.broadcast_to(np.asarray(v, dtype=np.float64), (3,))
    return (C.c_double * 3)(*[float(x) for x in v])


def _i3(v):
    v = np.broadcast_to(np.asarray(v), (3,))
    return (C.c_int * 3)(*[int(x) for x in v])


class Kernels:
    @staticmethod
    def Gaussian(h, tolerance):
        """FCM_ns::Kernels::Gaussian(h, tolerance) in double -> (kernel, a_eff)  (FCM_kernels.cuh:22-58)."""
        k, a = IBMKernel64(), C.c_double(0)
        check(_lib.load().uammd_fcm_gaussian_kernel_f64(float(h), float(tolerance), C.byref(k), C.byref(a)))
        return k, float(a.value)

    @staticmethod
    def adviseGridSize(hydrodynamicRadius, tolerance):
        return float(_lib.load().uammd_fcm_advise_grid_size_f64(float(hydrodynamicRadius), float(tolerance)))

    @staticmethod
    def Peskin3pt(h):
        h = np.broadcast_to(np.asarray(h, dtype=np.float64), (3,))
        return IBMKernel64(1, (C.c_int * 3)(3, 3, 3), 0.0, 0.0, float("inf"), (C.c_double * 3)(*[1.0 / x if x > 0 else 0.0 for x in h]))

    @staticmethod
    def Peskin4pt(h):
        h = np.broadcast_to(np.asarray(h, dtype=np.float64), (3,))
        return IBMKernel64(2, (C.c_int * 3)(4, 4, 4), 0.0, 0.0, float("inf"), (C.c_double * 3)(*[1.0 / x if x > 0 else 0.0 for x in h]))

    @staticmethod
    def Constant(support):
        s = np.broadcast_to(np.asarray(support), (3,))
        return IBMKernel64(3, (C.c_int * 3)(int(s[0]), int(s[1]), int(s[2])), 0.0, 0.0, float("inf"), (C.c_double * 3)(0, 0, 0))


class IBM:
    """IBM<Kernel, Grid, LinearIndex3D>::spread / gather (misc/IBM.cuh:99-203) on interleaved user grids, in double."""

    def __init__(self, kernel, L, periodic, cellDim, nxStride=None):
        self.lib = _lib.load()
        self.kernel, self.L, self.periodic, self.cellDim = kernel, L, periodic, [int(c) for c in cellDim]
        self.nxStride = int(nxStride) if nxStride is not None else self.cellDim[0]

    def _args(self):
        return _d3(self.L), _i3([int(p) for p in np.broadcast_to(self.periodic, (3,))]), _i3(self.cellDim), self.nxStride, C.byref(self.kernel)

    def spread(self, pos, v, gridData):
        ncomp = 1 if v.dim() == 1 else v.shape[1]
        assert pos.dtype == v.dtype == gridData.dtype == torch.float64
        check(self.lib.uammd_ibm_spread_f64(_ptr(pos), pos.shape[1], _ptr(v), ncomp, pos.shape[0], *self._args(), _ptr(gridData), _stream()))

    def gather(self, pos, Jq, gridData):
        ncomp = 1 if Jq.dim() == 1 else Jq.shape[1]
        assert pos.dtype == Jq.dtype == gridData.dtype == torch.float64
        check(self.lib.uammd_ibm_gather_f64(_ptr(pos), pos.shape[1], _ptr(Jq), ncomp, pos.shape[0], *self._args(), _ptr(gridData), _stream()))


class FCM_impl:
    """FCM_impl<Gaussian> (Integrator/BDHI/FCM/FCM_impl.cuh), deterministic part, in double."""

    def __init__(self, L, cells, kernel, viscosity, hydrodynamicRadius):
        self.lib = _lib.load()
        self.L = np.broadcast_to(np.asarray(L, dtype=np.float64), (3,)).copy()
        self.cells = [int(c) for c in cells]
        self.viscosity, self.hydrodynamicRadius = float(viscosity), float(hydrodynamicRadius)
        p = FCMParameters64()
        for k in range(3):
            p.boxSize[k], p.cells[k] = float(self.L[k]), self.cells[k]
        p.viscosity, p.kernel = self.viscosity, kernel
        h = C.c_void_p()
        check(self.lib.uammd_fcm_create_f64(C.byref(p), C.byref(h)))
        self.h = h

    def __del__(self):
        try:
            if getattr(self, "h", None):
                self.lib.uammd_fcm_destroy_f64(self.h)
                self.h = None
        except Exception:
            pass

    def getSelfMobility(self):
        return float(self.lib.uammd_fcm_self_mobility(self.hydrodynamicRadius, self.viscosity, float(self.L[0])))

    def computeHydrodynamicDisplacements(self, pos, force, out=None):
        n = pos.shape[0]
        v = out if out is not None else torch.zeros((n, 3), dtype=torch.float64, device=pos.device)
        check(self.lib.uammd_fcm_displacements_f64(self.h, _ptr(pos), _ptr(force), n, _ptr(v), _stream()))
        return v


class PSE:
    """BDHI::PSE deterministic mobility (BDHI_PSE.cuh:92-120 with T = 0): M F = M_far F + M_near F, in double."""

    def __init__(self, L, viscosity, hydrodynamicRadius, tolerance, psi, shearStrain=0.0):
        from .bdhi import nextFFTWiseSize3D
        self.lib = _lib.load()
        L3 = np.broadcast_to(np.asarray(L, dtype=np.float64), (3,)).copy()
        self.L, self.viscosity, self.rh = L3, float(viscosity), float(hydrodynamicRadius)
        h, rc, npts = C.c_void_p(), C.c_double(0), C.c_int(0)
        check(self.lib.uammd_pse_near_create_f64(_d3(L3), self.viscosity, self.rh, float(tolerance), float(psi), C.byref(h), C.byref(rc), C.byref(npts)))
        self.near, self.rcut, self.nPointsTable = h, float(rc.value), int(npts.value)
        raw = _i3(0)
        check(self.lib.uammd_pse_far_raw_cells_f64(_d3(L3), float(psi), float(tolerance), raw))
        self.cells = nextFFTWiseSize3D(list(raw))
        hf, sup, eta = C.c_void_p(), C.c_int(0), C.c_double(0)
        check(self.lib.uammd_pse_far_create_f64(_d3(L3), _i3(self.cells), self.viscosity, self.rh, float(tolerance), float(psi), float(shearStrain),
                                                C.byref(hf), C.byref(sup), C.byref(eta)))
        self.far, self.support, self.eta = hf, int(sup.value), float(eta.value)

    def __del__(self):
        try:
            if getattr(self, "near", None):
                self.lib.uammd_pse_near_destroy_f64(self.near)
                self.near = None
            if getattr(self, "far", None):
                self.lib.uammd_fcm_destroy_f64(self.far)
                self.far = None
        except Exception:
            pass

    def getSelfMobility(self):
        return float(self.lib.uammd_fcm_self_mobility(self.rh, self.viscosity, float(self.L[0])))

    def computeMF(self, pos, force):
        n = pos.shape[0]
        MF = torch.zeros((n, 3), dtype=torch.float64, device=pos.device)
        check(self.lib.uammd_fcm_displacements_f64(self.far, _ptr(pos), _ptr(force), n, _ptr(MF), _stream()))      # the far field ADDS
        check(self.lib.uammd_pse_near_mdot_f64(self.near, _ptr(pos), _ptr(force), 4, n, _ptr(MF), _stream()))
        return MF


class LanczosSolver:
    """lanczos::Solver with real = double (misc/LanczosAlgorithm.cuh:32-83).  dot(v, Mv) writes Mv = M v on float64 GPU tensors."""

    def __init__(self):
        self.lib = _lib.load()
        h = C.c_void_p()
        check(self.lib.uammd_lanczos_create_f64(C.byref(h)))
        self.h = h

    def __del__(self):
        try:
            if getattr(self, "h", None):
                self.lib.uammd_lanczos_destroy_f64(self.h)
                self.h = None
        except Exception:
            pass

    def setIterationHardLimit(self, n):
        check(self.lib.uammd_lanczos_set_iteration_hard_limit_f64(self.h, int(n)))

    def getLastRunRequiredSteps(self):
        s = C.c_int(0)
        check(self.lib.uammd_lanczos_get_last_run_required_steps_f64(self.h, C.byref(s)))
        return int(s.value)

    def run(self, dot, Bv, v, tolerance):
        n = v.numel()
        err = []

        def _wrap(ptr, count):
            class _Raw:
                pass
            r = _Raw()
            r.__cuda_array_interface__ = {"shape": (count,), "typestr": "<f8", "data": (int(ptr), False), "version": 2}
            return torch.as_tensor(r, device="cuda")

        def cb(ctx, d_v, d_Mv, nn, stream):
            try:
                dot(_wrap(d_v, nn), _wrap(d_Mv, nn))
                return 0
            except Exception as e:   # noqa: BLE001 - reported through the C status
                err.append(e)
                return -1
        it = C.c_int(0)
        fn = MATVEC64(cb)
        rc = self.lib.uammd_lanczos_run_f64(self.h, fn, None, _ptr(Bv), _ptr(v), float(tolerance), n, _stream(), C.byref(it))
        if err:
            raise err[0]
        check(rc)
        return int(it.value)


class BDHI2D:
    """BDHI::True2D / BDHI::Quasi2D with real = double (Integrator/Hydro/BDHI_quasi2D.cuh:155-257): one step's particle velocities
    (real2[N]) and the position update.  mode: "True2D" | "Quasi2D"."""

    def __init__(self, mode, L, hydrodynamicRadius, viscosity, temperature, dt, seed, cells=(-1, -1)):
        self.lib = _lib.load()
        Lx, Ly = (L, L) if np.isscalar(L) else (L[0], L[1])
        p = _lib.BDHI2DParametersF64()
        p.boxSize[0], p.boxSize[1] = float(Lx), float(Ly)
        p.hydrodynamicRadius, p.viscosity, p.temperature, p.dt = float(hydrodynamicRadius), float(viscosity), float(temperature), float(dt)
        p.cells[0], p.cells[1] = int(cells[0]), int(cells[1])
        p.seed, p.kernel = int(seed), {"True2D": 0, "Quasi2D": 1}[mode]
        h, cd, sup = C.c_void_p(), (C.c_int * 2)(0, 0), C.c_int(0)
        check(self.lib.uammd_bdhi2d_create_f64(C.byref(p), C.byref(h), C.byref(cd), C.byref(sup)))
        self.h, self.cells, self.support, self.dt = h, [int(cd[0]), int(cd[1])], int(sup.value), float(dt)

    def __del__(self):
        try:
            if getattr(self, "h", None):
                self.lib.uammd_bdhi2d_destroy_f64(self.h)
                self.h = None
        except Exception:
            pass

    def velocities(self, pos, force=None):
        n = pos.shape[0]
        vel = torch.empty((n, 2), dtype=torch.float64, device=pos.device)
        check(self.lib.uammd_bdhi2d_velocities_f64(self.h, _ptr(pos), _ptr(force), n, _ptr(vel), _stream()))
        return vel

    def forwardTime(self, pos, force=None):
        vel = self.velocities(pos, force)
        check(self.lib.uammd_bdhi2d_update_positions_f64(_ptr(pos), _ptr(vel), pos.shape[0], self.dt, _stream()))
        return vel


class Poisson:
    """Poisson with real = double (Interactor/SpectralEwaldPoisson.cuh:83-136): sum(force, energy) and the field / potential at the
    particles.  Near field over all pairs."""

    def __init__(self, L, epsilon, gw, tolerance=1e-5, split=-1.0, upsampling=-1.0):
        self.lib = _lib.load()
        p = _lib.PoissonParametersF64()
        L3 = np.broadcast_to(np.asarray(L, dtype=np.float64), (3,))
        for a in range(3):
            p.boxSize[a] = float(L3[a])
        p.epsilon, p.tolerance, p.gw, p.split, p.upsampling = float(epsilon), float(tolerance), float(gw), float(split), float(upsampling)
        h, info = C.c_void_p(), _lib.PoissonInfoF64()
        if self.lib.uammd_poisson_create_f64(C.byref(p), C.byref(h), C.byref(info)) != 0:
            msg = self.lib.uammd_hip_last_error().decode()
            raise ValueError(msg) if "[Poisson]" in msg else RuntimeError(msg)
        self.h = h
        self.cells, self.support, self.nearFieldCutOff, self.ntable = [int(c) for c in info.cells], int(info.support), float(info.nearFieldCutOff), int(info.nTable)

    def __del__(self):
        try:
            if getattr(self, "h", None):
                self.lib.uammd_poisson_destroy_f64(self.h)
                self.h = None
        except Exception:
            pass

    def sum(self, pos, charge, force4, energy, force=True, energy_flag=False):
        check(self.lib.uammd_poisson_sum_f64(self.h, _ptr(pos), _ptr(charge), pos.shape[0], _ptr(force4), _ptr(energy), int(force), int(energy_flag), _stream()))

    def computeFieldPotentialAtParticles(self, pos, charge):
        n = pos.shape[0]
        fp = torch.zeros((n, 4), dtype=torch.float64, device=pos.device)
        check(self.lib.uammd_poisson_field_potential_f64(self.h, _ptr(pos), _ptr(charge), n, _ptr(fp), None, None, _stream()))
        return fp


class BD:
    """BD::EulerMaruyama / MidPoint / AdamsBashforth / Leimkuhler with real = double (Integrator/BrownianDynamics.cuh:57-183): positions and
    forces double[N, 4]; `forces(pos)` fills the force array before each position update, as the scheme's interactors would (None: free
    particles).  seed: the reference takes the System generator's third draw."""
    SCHEMES = {"EulerMaruyama": 0, "MidPoint": 1, "AdamsBashforth": 2, "Leimkuhler": 3}

    def __init__(self, scheme, temperature, viscosity, hydrodynamicRadius, dt, seed, K=None, is2D=False, forces=None):
        self.lib = _lib.load()
        self.scheme = self.SCHEMES[scheme]
        self.temperature, self.dt, self.is2D, self.seed = float(temperature), float(dt), bool(is2D), int(seed) & 0xFFFFFFFF
        self.selfMobility = 1.0 / (6.0 * math.pi * float(viscosity) * float(hydrodynamicRadius))
        self.K = None if K is None else (C.c_double * 9)(*[float(x) for x in np.asarray(K, dtype=np.float64).reshape(9)])
        self.forces, self.steps, self.aux, self.force = forces, 0, None, None

    def _eval(self, pos):
        if self.force is None or self.force.shape != pos.shape:
            self.force = torch.zeros_like(pos)
        self.force.zero_()
        if self.forces is not None:
            self.forces(pos, self.force)

    def _advance(self, pos, substep, original_index=None):
        check(self.lib.uammd_bd_scheme_step_f64(self.scheme, substep, _ptr(pos), _ptr(self.aux), None, _ptr(original_index), _ptr(self.force), self.K,
                                                self.selfMobility, None, self.dt, int(self.is2D), self.temperature, pos.shape[0], self.steps, self.seed,
                                                _stream()))

    def forwardTime(self, pos, original_index=None):
        self.steps += 1
        if self.scheme == 1:       # MidPoint: two force evaluations (BrownianDynamics.cu:216-232)
            if self.aux is None:
                self.aux = torch.empty_like(pos)
            self._eval(pos)
            self._advance(pos, 0)
            self._eval(pos)
            self._advance(pos, 1)
        elif self.scheme == 2:     # AdamsBashforth: the previous step's forces are kept (:291-308)
            if self.steps == 1:
                self._eval(pos)
            self.aux = self.force.clone()
            self._eval(pos)
            self._advance(pos, 0)
        else:
            self._eval(pos)
            self._advance(pos, 0, original_index if self.scheme == 3 else None)


# ---- path A in double (md_f64.hip, verletlist_f64.hip, bonded_f64.hip, dpd_f64.hip): neighbour lists, LJ, bonds, DPD, Verlet integrators -----
class Box:
    """Box (utils/Box.cuh) with double sides."""

    def __init__(self, L, periodic=(True, True, True)):
        self.boxSize = np.broadcast_to(np.asarray(L, dtype=np.float64), (3,)).copy()
        self.periodic = [bool(p) for p in np.broadcast_to(np.asarray(periodic), (3,))]

    def __eq__(self, o):
        return isinstance(o, Box) and np.array_equal(self.boxSize, o.boxSize) and list(self.periodic) == list(o.periodic)


def _check_rows(t, width):
    assert t.dtype == torch.float64 and t.is_contiguous() and t.dim() == 2 and t.shape[1] == width, "expected a contiguous float64 [N, %d]" % width


class CellList:
    """The NeighbourList concept on double positions [N, 4] (uammd_celllist_*_f64): update(box, cutoff, pos) + getCellList +
    transverse_lj.  No ParticleData behind it: the caller says when the positions changed by calling update again."""
    GENERAL, SCAN32, AUTO = 1, 11, 0

    def __init__(self):
        self.lib = _lib.load()
        h = C.c_void_p()
        check(self.lib.uammd_celllist_create_f64(C.byref(h)))
        self.h = h
        self.N = 0

    def __del__(self):
        try:
            if getattr(self, "h", None):
                self.lib.uammd_celllist_destroy_f64(self.h)
                self.h = None
        except Exception:
            pass

    def check_errors(self):
        check(self.lib.uammd_celllist_check_errors_f64(self.h, _stream()))

    @staticmethod
    def create_update_grid(box, cutoff):
        """CellList::createUpdateGrid (CellList.cuh:100-126) in double: (cellDim, the box the list is built on)."""
        lib = _lib.load()
        cd, Lo, po = _i3(0), _d3(0.0), _i3(0)
        check(lib.uammd_celllist_create_grid_f64(_d3(box.boxSize), _i3([int(p) for p in box.periodic]), _d3(cutoff), cd, Lo, po))
        return list(cd), Box(list(Lo), [bool(p) for p in po])

    def update_grid(self, pos, box, cellDim):
        """CellListBase::update(pos, N, grid, st) (CellListBase.cuh:124-140)."""
        _check_rows(pos, 4)
        self.N = pos.shape[0]
        self._pos_ref = pos
        check(self.lib.uammd_celllist_update_f64(self.h, _ptr(pos), self.N, _d3(box.boxSize), _i3([int(p) for p in box.periodic]),
                                                 _i3(cellDim), _stream()))

    def update(self, box, cutoff, pos):
        """CellList::update(box, cutOff, st) (CellList.cuh:149-163); the list is rebuilt on every call."""
        cd, ubox = self.create_update_grid(box, cutoff)
        self.update_grid(pos, ubox, cd)

    def getCellList(self):
        d = _lib.CellListData64()
        check(self.lib.uammd_celllist_get_f64(self.h, C.byref(d)))
        return d

    @staticmethod
    def _wrap(ptr, shape, dtype):
        if int(np.prod(shape)) == 0:
            return torch.empty(shape, dtype=dtype, device="cuda")

        class _Raw:   # zero-copy view of library-owned device memory through __cuda_array_interface__
            pass
        r = _Raw()
        r.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": {torch.float64: "<f8", torch.int32: "<i4"}[dtype],
                                      "data": (int(ptr), False), "version": 2}
        return torch.as_tensor(r, device="cuda")

    def to_host(self):
        """Copies the list to numpy (tests): hash, index, sortPos, cellStart, cellEnd, VALID_CELL."""
        d = self.getCellList()
        n = d.numberParticles
        nc = d.cellDim[0] * d.cellDim[1] * d.cellDim[2]
        torch.cuda.synchronize()
        return dict(index=self._wrap(d.d_groupIndex, (n,), torch.int32).cpu().numpy(),
                    hash=self._wrap(d.d_sortHash, (n,), torch.int32).cpu().numpy().view(np.uint32),
                    sortPos=self._wrap(d.d_sortPos, (n, 4), torch.float64).cpu().numpy(),
                    cellStart=self._wrap(d.d_cellStart, (nc,), torch.int32).cpu().numpy().view(np.uint32),
                    cellEnd=self._wrap(d.d_cellEnd, (nc,), torch.int32).cpu().numpy(),
                    validCell=int(d.VALID_CELL), cellDim=np.array(list(d.cellDim), np.int32),
                    L=np.array(list(d.boxSize), np.float64), periodic=np.array(list(d.periodic), np.int32))

    def transverse_lj(self, param_table, ntypes, box, force=None, energy=None, virial=None, global_index=None, algo=0):
        check(self.lib.uammd_lj_transverse_celllist_f64(self.h, _ptr(param_table), int(ntypes), _d3(box.boxSize),
                                                        _i3([int(p) for p in box.periodic]), _ptr(force), _ptr(energy), _ptr(virial),
                                                        _ptr(global_index), int(algo), _stream()))


class LJ:
    """Potential::LJ = Radial<LJFunctor> with BasicParameterHandler in double; the type table grows as md._LJ's does."""

    class InputPairParameters:
        def __init__(self, cutOff=2.5, sigma=1.0, epsilon=1.0, shift=False):
            self.cutOff, self.sigma, self.epsilon, self.shift = cutOff, sigma, epsilon, shift

    def __init__(self):
        self.lib = _lib.load()
        self.ntypes = 1
        self.cutOff = 0.0
        self.table = np.zeros((1, 4), np.float64)
        self._dev = None

    def setPotParameters(self, ti, tj, p):
        self.cutOff = max(float(p.cutOff), self.cutOff)
        new = max(self.ntypes, ti + 1, tj + 1)
        if new != self.ntypes:
            tmp = np.zeros((new * new, 4), np.float64)
            for i in range(self.ntypes):
                for j in range(self.ntypes):
                    tmp[i + new * j] = self.table[i + self.ntypes * j]
            self.table, self.ntypes = tmp, new
        out = _lib.LJPairParameters64()
        check(self.lib.uammd_lj_process_pair_parameters_f64(float(p.cutOff), float(p.sigma), float(p.epsilon), int(bool(p.shift)), C.byref(out)))
        row = np.array([out.cutOff2, out.sigma2, out.epsilonDivSigma2, out.shift], np.float64)
        self.table[ti + self.ntypes * tj] = row
        if ti != tj:
            self.table[tj + self.ntypes * ti] = row
        self._dev = None

    def getCutOff(self):
        return self.cutOff

    def device_table(self):
        if self._dev is None:
            self._dev = torch.from_numpy(self.table.copy()).cuda()
        return self._dev


class VerletList:
    """The NeighbourList concept on double positions [N, 4] over the Verlet list (uammd_verletlist_*_f64): update(box, cutoff, pos) +
    getVerletList + transverse_lj.  No ParticleData behind it: every update looks at the positions it is given (the drift check decides
    whether the list is rebuilt)."""

    def __init__(self):
        self.lib = _lib.load()
        h = C.c_void_p()
        check(self.lib.uammd_verletlist_create_f64(C.byref(h)))
        self.h = h
        self.N = 0
        self.rebuilds = 0

    def __del__(self):
        try:
            if getattr(self, "h", None):
                self.lib.uammd_verletlist_destroy_f64(self.h)
                self.h = None
        except Exception:
            pass

    def forceNextUpdate(self):
        check(self.lib.uammd_verletlist_force_next_update_f64(self.h))

    def setCutOffMultiplier(self, multiplier):
        check(self.lib.uammd_verletlist_set_cutoff_multiplier_f64(self.h, float(multiplier)))

    def getNumberOfStepsSinceLastUpdate(self):
        steps = C.c_int()
        check(self.lib.uammd_verletlist_get_steps_since_last_update_f64(self.h, C.byref(steps)))
        return steps.value

    def update(self, box, cutoff, pos):
        """VerletListBase::update (VerletListBase.cuh:107-117); returns whether the list was rebuilt."""
        _check_rows(pos, 4)
        rebuilt = C.c_int(0)
        self._pos_ref = pos
        check(self.lib.uammd_verletlist_update_f64(self.h, _ptr(pos), pos.shape[0], _d3(box.boxSize), _i3([int(p) for p in box.periodic]),
                                                   float(cutoff), _stream(), C.byref(rebuilt)))
        self.N = pos.shape[0]
        self.rebuilds += rebuilt.value
        return bool(rebuilt.value)

    def getVerletList(self):
        d = _lib.VerletListData()
        check(self.lib.uammd_verletlist_get_f64(self.h, C.byref(d)))
        return d

    def to_host(self):
        """Copies the list to numpy (tests): neighbourList[capacity, N] (entry k of sorted particle i at [k, i]), numberNeighbours,
        sortPos, groupIndex."""
        d = self.getVerletList()
        n, cap = d.numberParticles, d.maxNeighboursPerParticle
        torch.cuda.synchronize()
        w = CellList._wrap
        return dict(neighbourList=w(d.d_neighbourList, (cap, n), torch.int32).cpu().numpy(),
                    numberNeighbours=w(d.d_numberNeighbours, (n,), torch.int32).cpu().numpy(),
                    sortPos=w(d.d_sortPos, (n, 4), torch.float64).cpu().numpy(),
                    groupIndex=w(d.d_groupIndex, (n,), torch.int32).cpu().numpy(),
                    maxNeighboursPerParticle=cap, particleStride=d.particleStride, numberParticles=n)

    def transverse_lj(self, param_table, ntypes, box, force=None, energy=None, virial=None, global_index=None, algo=0):
        check(self.lib.uammd_lj_transverse_verletlist_f64(self.h, _ptr(param_table), int(ntypes), _d3(box.boxSize),
                                                          _i3([int(p) for p in box.periodic]), _ptr(force), _ptr(energy), _ptr(virial),
                                                          _ptr(global_index), _stream()))


class PairForcesLJ:
    """PairForces<Potential::LJ, NeighbourList> in double (PairForces.cu:43-78): the neighbour list (a CellList unless nl=VerletList() is
    given) unless the box is at most 3 cut-offs in every direction, then all pairs.  sum() ACCUMULATES into the arrays it is given
    (Transverser::set does +=)."""

    def __init__(self, box, potential, algo=0, nl=None):
        self.lib = _lib.load()
        self.box, self.pot, self.algo, self.nl = box, potential, algo, nl

    def sum(self, pos, force=None, energy=None, virial=None):
        _check_rows(pos, 4)
        rc = float(self.pot.getCutOff())
        L = self.box.boxSize
        tbl = self.pot.device_table()
        if L[0] <= 3 * rc and L[1] <= 3 * rc and L[2] <= 3 * rc:     # PairForces.cu:43-53
            check(self.lib.uammd_lj_transverse_nbody_f64(_ptr(pos), pos.shape[0], _ptr(tbl), self.pot.ntypes, _d3(L),
                                                         _i3([int(p) for p in self.box.periodic]), _ptr(force), _ptr(energy), _ptr(virial),
                                                         None, _stream()))
            return
        if self.nl is None:
            self.nl = CellList()
        self.nl.update(self.box, rc, pos)
        self.nl.transverse_lj(tbl, self.pot.ntypes, self.box, force, energy, virial, None, self.algo)


class BondedForces:
    """BondedForces / AngularBondedForces / TorsionalBondedForces in double (uammd_bonded_*_f64).  kind: "harmonic", "fene", "angular",
    "torsional" or "fourier"; ids int[nbonds, members] (a negative id -(j+1) names fixedPoints[j], two-member kinds only); info
    double[nbonds, 2] in the bond file's order ("k p0"); box: the kind's Box (None: no minimum image).  refresh(id2index) follows a
    reordering of the particles and has to be called once before the first sum."""
    KINDS = {"harmonic": (0, 2, False), "fene": (1, 2, True), "angular": (2, 3, True), "torsional": (3, 4, True), "fourier": (4, 4, True)}

    def __init__(self, kind, ids, info, box=None, fixedPoints=None):
        self.lib = _lib.load()
        self.kind, self.members, swap = self.KINDS[kind]
        self.box = box if box is not None else Box(0.0, (False, False, False))
        ids = np.ascontiguousarray(np.asarray(ids, np.int32).reshape(-1, self.members))
        info = np.asarray(info, np.float64).reshape(-1, 2)
        if info.shape[0] != ids.shape[0]:
            raise ValueError("one BondInfo per bond")
        fixedPoints = np.zeros((0, 4)) if fixedPoints is None else np.asarray(fixedPoints, np.float64)
        fp = np.zeros((fixedPoints.shape[0], 4), np.float64)
        fp[:, :fixedPoints.shape[1]] = fixedPoints
        structInfo = np.ascontiguousarray(info[:, ::-1] if swap else info)      # BondInfo order: {k, r0} for Harmonic, {p0, k} otherwise
        self.nbonds = ids.shape[0]
        h = C.c_void_p()
        check(self.lib.uammd_bonded_create_f64(C.byref(h)))
        self.h = h
        check(self.lib.uammd_bonded_upload_f64(self.h, self.kind, self.nbonds, ids.ctypes.data_as(C.c_void_p),
                                               structInfo.ctypes.data_as(C.c_void_p), fp.shape[0], fp.ctypes.data_as(C.c_void_p),
                                               _d3(self.box.boxSize), _i3([int(p) for p in self.box.periodic])))

    def __del__(self):
        try:
            if getattr(self, "h", None):
                torch.cuda.synchronize()
                self.lib.uammd_bonded_destroy_f64(self.h)
                self.h = None
        except Exception:
            pass

    def refresh(self, id2index):
        """id2index int32[N] on the device: the current index of the particle with each id (ParticleData::getIdOrderedIndices)."""
        assert id2index.dtype == torch.int32 and id2index.is_contiguous()
        check(self.lib.uammd_bonded_refresh_f64(self.h, _ptr(id2index), id2index.shape[0], _stream()))

    def shape(self):
        """(rows, entries, rows on the lane-per-row shape, rows on the wave-per-row shape)."""
        r, e, lr, wr = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        check(self.lib.uammd_bonded_get_shape_f64(self.h, C.byref(r), C.byref(e), C.byref(lr), C.byref(wr)))
        return r.value, e.value, lr.value, wr.value

    def sum(self, pos, force=None, energy=None, virial=None):
        _check_rows(pos, 4)
        check(self.lib.uammd_bonded_sum_f64(self.h, _ptr(pos), _ptr(force), _ptr(energy), _ptr(virial), _stream()))


class PairForcesDPD:
    """PairForces<Potential::DPD> in double (DPD.cuh:121-170, PairForces.cu:43-68): sum(pos, vel, force) ACCUMULATES the DPD pair force.
    sigma = sqrt(2 kT) / sqrt(dt) in double (DPD.cuh:69); the step advances once per sum; the cell list when the box exceeds 3 cut-offs
    in every periodic direction, else all pairs."""
    needs_velocities = True      # the integrators call sum(pos, vel, force)

    def __init__(self, box, cutOff=1.0, A=1.0, gamma=1.0, temperature=0.0, dt=0.0, seed=0):
        self.lib = _lib.load()
        self.box, self.rcut, self.A, self.gamma = box, float(cutOff), float(A), float(gamma)
        self.temperature, self.dt, self.seed = float(temperature), float(dt), int(seed) & 0xFFFFFFFFFFFFFFFF
        self.sigma = math.sqrt(2.0 * self.temperature) / math.sqrt(self.dt) if self.dt > 0 else (0.0 if self.temperature == 0 else float("inf"))
        self.step = 0
        self.nl = None

    def uses_cell_list(self):
        L = self.box.boxSize
        return all(L[k] > 3 * self.rcut for k in range(3) if self.box.periodic[k])

    def sum(self, pos, vel, force, global_index=None):
        _check_rows(pos, 4), _check_rows(vel, 3), _check_rows(force, 4)
        self.step += 1
        L, per = _d3(self.box.boxSize), _i3([int(p) for p in self.box.periodic])
        args = (self.rcut, self.A, self.gamma, self.sigma, self.seed, self.step, pos.shape[0], _ptr(force), _ptr(global_index), _stream())
        if self.uses_cell_list():
            if self.nl is None:
                self.nl = CellList()
            members = pos if global_index is None else pos[global_index.long()].contiguous()      # the list is built on the members
            self.nl.update(self.box, self.rcut, members)
            check(self.lib.uammd_dpd_transverse_celllist_f64(self.nl.h, _ptr(vel), L, per, *args))
        else:
            n = pos.shape[0] if global_index is None else global_index.shape[0]
            check(self.lib.uammd_dpd_transverse_nbody_f64(_ptr(pos), _ptr(vel), n, L, per, *args))


def _sum_interactors(interactors, pos, vel, force):
    for it in interactors:
        if getattr(it, "needs_velocities", False):
            it.sum(pos, vel, force)
        else:
            it.sum(pos, force)


def initVelocities(vel, velAmplitude, seed, is2D=False, index=None):
    """VerletNVT::Basic_ns::initialVelocities (Basic.cu:12-29) on vel double[N, 3]; index: the group's members (None = everybody)."""
    _check_rows(vel, 3)
    n = vel.shape[0] if index is None else index.shape[0]
    check(_lib.load().uammd_verletnvt_initial_velocities_f64(_ptr(vel), _ptr(index), float(velAmplitude), int(bool(is2D)), n,
                                                             int(seed) & 0xFFFFFFFF, _stream()))


def sumKineticEnergy(vel, energy, mass=None, defaultMass=1.0, index=None):
    """energy[i] += m |v|^2 / 2 (Basic.cu:173-207); defaultMass > 0 wins over the mass array."""
    _check_rows(vel, 3)
    n = vel.shape[0] if index is None else index.shape[0]
    check(_lib.load().uammd_sum_kinetic_energy_f64(_ptr(vel), _ptr(energy), _ptr(mass), float(defaultMass), _ptr(index), n, _stream()))


class VerletNVT:
    """VerletNVT::GronbechJensen / Basic in double (Integrator/VerletNVT.cuh): forwardTime(pos, vel, force, interactors) with interactors
    that offer sum(pos, force).  seed: the reference takes the System generator's third draw."""
    KINDS = ("GronbechJensen", "Basic")

    def __init__(self, kind, temperature, dt, friction, seed, is2D=False, mass=None, defaultMass=1.0, index=None):
        assert kind in self.KINDS
        self.lib = _lib.load()
        self.fn = self.lib.uammd_verletnvt_gj_f64 if kind == "GronbechJensen" else self.lib.uammd_verletnvt_basic_f64
        self.temperature, self.dt, self.friction, self.is2D = float(temperature), float(dt), float(friction), bool(is2D)
        self.seed = int(seed) & 0xFFFFFFFF
        self.noiseAmplitude = math.sqrt(2 * self.dt * self.friction * self.temperature)
        self.mass, self.defaultMass, self.index, self.steps = mass, (0.0 if mass is not None else float(defaultMass)), index, 0

    def integrate(self, step, pos, vel, force):
        n = pos.shape[0] if self.index is None else self.index.shape[0]
        check(self.fn(step, _ptr(pos), _ptr(vel), _ptr(force), _ptr(self.mass), self.defaultMass, _ptr(self.index), n, self.dt, self.friction,
                      int(self.is2D), self.noiseAmplitude, self.steps, self.seed, _stream()))

    def forwardTime(self, pos, vel, force, interactors=()):     # GronbechJensen.cu:88-115, Basic.cu:116-150
        _check_rows(pos, 4), _check_rows(vel, 3), _check_rows(force, 4)
        self.steps += 1
        if self.steps == 1:
            force.zero_()
            _sum_interactors(interactors, pos, vel, force)
        self.integrate(1, pos, vel, force)      # (the first half step leaves the forces at zero)
        _sum_interactors(interactors, pos, vel, force)
        self.integrate(2, pos, vel, force)


class VerletNVE:
    """VerletNVE in double (Integrator/VerletNVE.cu:133-188): half kick + drift, force reset, the interactors' forces, half kick.  The
    velocities are the caller's (initVelocities or its own)."""

    def __init__(self, dt, is2D=False, mass=None, defaultMass=1.0, index=None):
        self.lib = _lib.load()
        self.dt, self.is2D, self.mass, self.defaultMass, self.index, self.steps = float(dt), bool(is2D), mass, float(defaultMass), index, 0

    def integrate(self, step, pos, vel, force):
        n = pos.shape[0] if self.index is None else self.index.shape[0]
        check(self.lib.uammd_verletnve_f64(step, _ptr(pos), _ptr(vel), _ptr(force), _ptr(self.mass), self.defaultMass, _ptr(self.index), n,
                                           self.dt, int(self.is2D), _stream()))

    def _reset_forces(self, force):             # VerletNVE.cu:152-158: the members' forces only
        if self.index is None:
            force.zero_()
        else:
            force[self.index.long()] = 0.0

    def forwardTime(self, pos, vel, force, interactors=()):     # VerletNVE.cu:160-188
        _check_rows(pos, 4), _check_rows(vel, 3), _check_rows(force, 4)
        self.steps += 1
        if self.steps == 1:
            self._reset_forces(force)
            _sum_interactors(interactors, pos, vel, force)
        self.integrate(1, pos, vel, force)
        self._reset_forces(force)
        _sum_interactors(interactors, pos, vel, force)
        self.integrate(2, pos, vel, force)
