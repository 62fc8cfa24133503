"""Monte Carlo NVT: MC_NVT.Anderson, Anderson's checkerboard algorithm.

Mirror of the reference's Integrator/MonteCarlo/NVT/Anderson.cuh:47-119 and Anderson.cu with Potential.LJ; the step runs in
libuammd_hip.so (uammd_mc_anderson_step, uammd_amd/csrc/mc.hip).  The host draws — the origin of the checkerboard and the order of the
subgrids — come from pd.rng, the mirror of System::rng(), in the reference's order, so the C++ class and this one walk the same
trajectory from the same system seed.

    pot = Potential.LJ(); pot.setPotParameters(0, 0, pot.InputPairParameters(2.5, 1.0, 1.0, True))
    mc = MC_NVT.Anderson(pd, pot, MC_NVT.Anderson.Parameters(box=Box(32.0), temperature=1.5))
    mc.forwardTime()

The Metropolis rule uses the whole pair energy.
"""
import ctypes as C
import logging

import numpy as np

from ._lib import check, f3, i3
from .md import Integrator, _ptr, current_stream

_log = logging.getLogger("uammd_amd")


def create_grid(boxSize, cutOff):
    """Anderson_ns::createGrid (Anderson.cu:52-65): int(L / rc) per axis, made even by subtracting 1, z = 1 when L.z == 0."""
    L = np.broadcast_to(np.asarray(boxSize, dtype=np.float32), (3,))
    cd = [int(np.float32(l) / np.float32(cutOff)) for l in L]
    cd = [c - 1 if c % 2 != 0 else c for c in cd]
    if L[2] == 0:
        cd[2] = 1
    return cd


def check_grid_validity(cellDim):
    """Anderson_ns::checkGridValidity (Anderson.cu:67-73)."""
    return not (cellDim[0] < 3 or cellDim[1] < 3 or cellDim[2] == 2)


def update_jump_size(jumpSize, ratio, target, cellSize, is2D):
    """Anderson::updateJumpSize (Anderson.cu:133-153) in the reference's types: jumpSize float, the factors double."""
    jumpSize, ratio, target = np.float32(jumpSize), np.float32(ratio), np.float32(target)
    cs = [np.float32(c) for c in cellSize]
    minJump = cs[0] / np.float32(100000)
    if ratio < target:
        jumpSize = np.float32(float(jumpSize) * 0.9)
        if jumpSize <= minJump:
            jumpSize = minJump
    elif ratio > target:
        jumpSize = np.float32(float(jumpSize) * 1.02)
        jumpSize = min(jumpSize, cs[0], cs[1])
        if not is2D:
            jumpSize = min(jumpSize, cs[2])
    return np.float32(jumpSize)


class _Anderson(Integrator):
    """MC_NVT::Anderson<Potential::LJ>."""

    class Parameters:
        def __init__(self, box=None, temperature=-1.0, triesPerCell=10, initialJumpSize=1.0, acceptanceRatio=0.5, tuneSteps=10, seed=0):
            self.box, self.temperature, self.triesPerCell = box, temperature, triesPerCell
            self.initialJumpSize, self.acceptanceRatio, self.tuneSteps, self.seed = initialJumpSize, acceptanceRatio, tuneSteps, seed

    def __init__(self, pd, pot, par):
        super().__init__(pd)
        self.pot, self.par = pot, par
        self.updatables = []
        self.jumpSize = np.float32(par.initialJumpSize)
        if np.float32(par.temperature) < 0:                       # Anderson.cu:84-87
            _log.error("[MC_NVT::Anderson] Please specify a temperature!")
            raise ValueError("Negative temperature detected")
        self.is2D = bool(np.float32(par.box.boxSize[2]) == 0)
        self.updateSimulationBox(par.box)
        seed = int(par.seed)
        if seed == 0:                                             # Anderson.cu:98-101
            seed = pd.rng.next32()
        self.seed = seed & 0xFFFFFFFF
        self.currentAcceptanceRatio = np.float32(0)
        self.currentOrigin = np.zeros(3, np.float32)
        h = C.c_void_p()
        check(self.lib.uammd_mc_anderson_create(C.byref(h)))
        self.h = h

    def __del__(self):
        try:
            if getattr(self, "h", None):
                self.lib.uammd_mc_anderson_destroy(self.h)
                self.h = None
        except Exception:
            pass

    def addUpdatable(self, u):
        self.updatables.append(u)

    def updateSimulationBox(self, box):
        """Anderson::updateSimulationBox (Anderson.cu:107-124); an invalid grid raises (the reference builds the exception and drops it)."""
        for u in self.updatables:
            u.updateBox(self.par.box)
        rcut = np.float32(self.pot.getCutOff())
        cd = create_grid(box.boxSize, rcut)
        if not check_grid_validity(cd):
            _log.error("[MC_NVT::Anderson] I cannot work with such a large cut off (%e) in this box (%e)!", rcut, box.boxSize[0])
            raise ValueError("Cut off is too large")
        self.box, self.cellDim = box, cd
        self.cellSize = [np.float32(box.boxSize[k]) / np.float32(cd[k]) for k in range(3)]
        self.maxOriginDisplacement = np.float32(0.5 * float(np.float32(box.boxSize[0])))
        if getattr(self, "h", None):
            self.resetAcceptanceCounters()

    def resetAcceptanceCounters(self):
        self._counters(reset=True)

    def _counters(self, reset):
        t, a = C.c_ulonglong(0), C.c_ulonglong(0)
        check(self.lib.uammd_mc_anderson_counters(self.h, C.byref(t), C.byref(a), int(reset), current_stream()))
        return t.value, a.value

    def cell_counters(self):
        """(tried, accepted) per cell since the last reset, as numpy uint32 arrays (tests)."""
        n = self.cellDim[0] * self.cellDim[1] * self.cellDim[2]
        t, a = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
        check(self.lib.uammd_mc_anderson_cell_counters(self.h, t.ctypes.data_as(C.c_void_p), a.ctypes.data_as(C.c_void_p), current_stream()))
        return t, a

    def draw_origin(self):
        """Anderson::updateOrigin (Anderson.cu:177-185): three uniforms in double, the product in double, then the cast to float."""
        u = self.pd.rng.uniform3(-1.0, 1.0)
        o = np.array([np.float32(x * float(self.maxOriginDisplacement)) for x in u], np.float32)
        if self.is2D:
            o[2] = 0
        return o

    def draw_subgrid_order(self):
        """Anderson::performStep's shuffle (Anderson.cu:219-225)."""
        n = 4 if self.is2D else 8
        order = list(range(8))
        for i in range(n - 1):
            j = i + self.pd.rng.next() % (n - i)
            order[i], order[j] = order[j], order[i]
        return order[:n]

    def forwardTime(self):
        """Anderson::forwardTime (Anderson.cu:155-175)."""
        par = self.par
        if self.steps == 0:
            for u in self.updatables:
                u.updateTemperature(par.temperature)
        self.steps += 1
        self.currentOrigin = self.draw_origin()
        order = self.draw_subgrid_order()
        beta = np.float32(1.0 / float(np.float32(par.temperature)))
        pos = self.pd.getPos("readwrite")
        check(self.lib.uammd_mc_anderson_step(self.h, _ptr(pos), self.pd.N, f3(self.box.boxSize), i3([int(p) for p in self.box.periodic]),
                                              i3(self.cellDim), f3(self.currentOrigin), (C.c_int * len(order))(*order), len(order),
                                              int(par.triesPerCell), float(beta), float(self.jumpSize), self.steps & 0xFFFFFFFF, self.seed,
                                              _ptr(self.pot.device_table()), self.pot.ntypes, current_stream()))
        if self.steps % par.tuneSteps == 0 and self.steps > 1:
            tried, accepted = self._counters(reset=True)
            with np.errstate(invalid="ignore", divide="ignore"):
                self.currentAcceptanceRatio = np.float32(accepted) / np.float32(tried)
            self.jumpSize = update_jump_size(self.jumpSize, self.currentAcceptanceRatio, par.acceptanceRatio, self.cellSize, self.is2D)

    def sumEnergy(self):
        """Anderson::sumEnergy (Anderson.cu:377-400): the per-particle pair energy replaces pd's energy; returns 0."""
        self.currentOrigin = np.zeros(3, np.float32)
        check(self.lib.uammd_mc_anderson_energy(self.h, _ptr(self.pd.getPos("read")), self.pd.N, f3(self.box.boxSize),
                                                i3([int(p) for p in self.box.periodic]), i3(self.cellDim), _ptr(self.pot.device_table()),
                                                self.pot.ntypes, _ptr(self.pd.getEnergy("write")), current_stream()))
        return 0.0

    def getCurrentStepSize(self):
        return float(self.jumpSize)

    def getCurrentAcceptanceRatio(self):
        return float(self.currentAcceptanceRatio)


class MC_NVT:
    Anderson = _Anderson
