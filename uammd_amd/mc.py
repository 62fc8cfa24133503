"""Monte Carlo: MC_NVT.Anderson, Anderson's checkerboard algorithm, and MC.ForceBiased, the Metropolized Euler-Maruyama scheme (below).

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
from .md import Integrator, ParticleGroup, _ptr, current_stream

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


class Optimize:
    """forcebiased_ns::Optimize (ForceBiased.cuh:88-138) in the reference's types: the step size and the ratios float, the counters int.
    Every 1000 tries the step grows by 1.02 when the ratio is above the target (and the step below 2) or shrinks by 0.9 when it is below
    (and the step above 1e-8); the ratio is published at each control."""
    ncontrol = 1000

    def __init__(self, targetAcceptanceRatio, initialStepSize=1.0):
        self.targetRatio = np.float32(targetAcceptanceRatio)
        self.jumpSize = np.float32(initialStepSize)
        self.currentAcceptanceRatio = np.float32(0)
        self.naccept = self.ntry = 0

    def _adjust(self):
        ratio = np.float32(self.naccept) / np.float32(self.ntry)
        if ratio > self.targetRatio and self.jumpSize < np.float32(2):
            self.jumpSize = np.float32(self.jumpSize * np.float32(1.02))
        elif ratio < self.targetRatio and self.jumpSize > np.float32(1e-8):
            self.jumpSize = np.float32(self.jumpSize * np.float32(0.9))
        self.ntry = self.naccept = 0
        self.currentAcceptanceRatio = ratio

    def registerAccept(self):
        self.naccept += 1
        self.registerReject()

    def registerReject(self):
        self.ntry += 1
        if self.ntry % self.ncontrol == 0:
            self._adjust()

    def getStepSize(self):
        return self.jumpSize

    def getCurrentAcceptanceRatio(self):
        return self.currentAcceptanceRatio


class _ForceBiased(Integrator):
    """MC::ForceBiased (Integrator/MonteCarlo/ForceBiased.cuh): force biased Monte Carlo, the Metropolized Euler-Maruyama scheme of
    Bou-Rabee and Vanden-Eijnden (MALA).  It samples exp(-beta U) for ANY interactors, through Interactor.sum(force=True, energy=True).

        mala = MC.ForceBiased(pd, MC.ForceBiased.Parameters(beta=1.0, stepSize=1e-4, acceptanceRatio=0.5))
        mala.addInteractor(pairForces)
        mala.forwardTime()            # tries new configurations until one is accepted
        mala.getCurrentEnergy(), mala.getCurrentStepSize(), mala.getCurrentAcceptanceRatio(), mala.getLastNumberOfTrials()

    A trial: Y = X + h F(X) + sqrt(2 h / beta) xi (uammd_mc_forcebiased_propose), force and energy zeroed, the interactors summed on Y, then
    uammd_mc_forcebiased_decide forms E_Y, T_XY, T_YX in double on the device, decides Z < exp(-beta ((E_Y - E_X) + (T_YX - T_XY))) and keeps Y
    or puts X back; uammd_mc_forcebiased_result is the one host synchronisation.  The host draws keep the reference's order: the seed is
    pd.rng.next32() at construction, Z = pd.rng.uniform(0, 1) once per trial (cast to float, the reference's `real Z`).

    Where this class departs from the reference:
      * U = sum_i energy[i], NOT half of it.  Every interactor of this library deposits half of a pair's energy on each partner, so the sum
        is already U; the reference halves it again and so weighs exp(-beta U / 2) against a drift built from the whole force.
        getCurrentEnergy() returns U.  A user interactor that deposits the WHOLE pair energy on both partners double counts: deposit half.
      * getLastNumberOfTrials() / getTotalNumberOfTrials().  forwardTime() returns only at an acceptance, so the states seen after each call
        are NOT a Boltzmann sample on their own: the state a call STARTS from has to be weighted by the number of trials that call took
        (it is the state of the chain for that many steps).
      * maxTrials (default 1 000 000): that many consecutive rejections raise instead of looping for ever (a NaN landscape rejects always).
        The positions and forces are then those of the stored configuration X.
      * a group other than "All" is refused (the reference indexes its stored arrays by group size but the particle arrays globally).
      * the three sums and the exponent are in double (float thrust::reduce in the reference).
    """

    class Parameters:
        def __init__(self, beta=-1.0, stepSize=0.1, acceptanceRatio=0.5, maxTrials=1000000):
            self.beta, self.stepSize, self.acceptanceRatio, self.maxTrials = beta, stepSize, acceptanceRatio, maxTrials

    def __init__(self, pd, par):
        pg = None
        if isinstance(pd, ParticleGroup):
            pg, pd = pd, pd.getParticleData()
        super().__init__(pd)
        self.par = par
        self.updatables = []
        self.beta = np.float32(par.beta)
        _log.info("[MC::ForceBiased] Initialized")
        with np.errstate(divide="ignore"):
            _log.info("[MC::ForceBiased] Temperature: %g", np.float64(1.0) / np.float64(self.beta))
        _log.info("[MC::ForceBiased] Target acceptance ratio: %g", par.acceptanceRatio)
        _log.info("[MC::ForceBiased] Initial step size: %g", par.stepSize)
        if self.beta < 0 or np.float32(par.stepSize) <= 0 or np.float32(par.acceptanceRatio) <= 0:   # ForceBiased.cuh:172-176
            _log.error("[MC::ForceBiased] ERROR: parameters beta, stepSize and acceptanceRatio must be >=0")
            raise RuntimeError("Invalid parameter")
        if int(par.maxTrials) < 1:
            _log.error("[MC::ForceBiased] ERROR: maxTrials must be at least 1")
            raise RuntimeError("Invalid parameter")
        if pg is not None and not pg.allParticles:
            _log.error("[MC::ForceBiased] ERROR: only the group of all particles is supported")
            raise RuntimeError("[MC::ForceBiased] A group other than \"All\" is not supported")
        self.optimizeStepSize = Optimize(par.acceptanceRatio, par.stepSize)
        self.maxTrials = int(par.maxTrials)
        self.step = 0
        self.currentEnergy = 0.0
        self.lastTrials = self.totalTrials = 0
        self.lastRecord = None
        self.seed = pd.rng.next32() & 0xFFFFFFFF
        h = C.c_void_p()
        check(self.lib.uammd_mc_forcebiased_create(C.byref(h)))
        self.h = h

    def __del__(self):
        try:
            if getattr(self, "h", None):
                self.lib.uammd_mc_forcebiased_destroy(self.h)
                self.h = None
        except Exception:
            pass

    def addUpdatable(self, u):
        self.updatables.append(u)

    def getCurrentEnergy(self):
        return self.currentEnergy

    def getCurrentStepSize(self):
        return float(self.optimizeStepSize.getStepSize())

    def getCurrentAcceptanceRatio(self):
        return float(self.optimizeStepSize.getCurrentAcceptanceRatio())

    def getLastNumberOfTrials(self):
        """Trials the last forwardTime() took; the state that call STARTED from carries this weight in an average."""
        return self.lastTrials

    def getTotalNumberOfTrials(self):
        return self.totalTrials

    def _forceEnergy(self):
        """updateForceEnergyEstimation (ForceBiased.cuh:326-354) up to the sum: the two fills and the interactors."""
        pd = self.pd
        f, e = pd.getForce("write"), pd.getEnergy("write")
        check(self.lib.uammd_fill_zero(_ptr(f), f.numel() * 4, current_stream()))
        check(self.lib.uammd_fill_zero(_ptr(e), e.numel() * 4, current_stream()))
        for it in self.interactors:
            it.sum(force=True, energy=True, virial=False)

    def _result(self):
        acc, out = C.c_int(0), (C.c_double * 6)()
        check(self.lib.uammd_mc_forcebiased_result(self.h, C.byref(acc), out, current_stream()))
        self.lastRecord = tuple(out)
        self.currentEnergy = out[5]
        return bool(acc.value)

    def firstStep(self):
        """firstStep and updateInteractors (ForceBiased.cuh:203-218): the current configuration becomes X."""
        pd = self.pd
        self._forceEnergy()
        check(self.lib.uammd_mc_forcebiased_begin(self.h, _ptr(pd.getPos("read")), _ptr(pd.getForce("read")), _ptr(pd.getEnergy("read")),
                                                  pd.N, current_stream()))
        for u in list(self.interactors) + self.updatables:
            with np.errstate(divide="ignore"):
                u.updateTemperature(float(np.float64(1.0) / np.float64(self.beta)))

    def proposeNewStep(self):
        """The first half of a trial (ForceBiased.cuh:296-308, 336-346): pos = Y, force = F(Y), energy = the per-particle energies of Y."""
        pd = self.pd
        self.step += 1
        self.trialStepSize = float(self.optimizeStepSize.getStepSize())
        check(self.lib.uammd_mc_forcebiased_propose(self.h, _ptr(pd.getPos("readwrite")), pd.N, self.trialStepSize, float(self.beta),
                                                    self.step & 0xFFFFFFFF, self.seed, None, current_stream()))
        self._forceEnergy()

    def decideNewStep(self):
        """The second half (ForceBiased.cuh:235-278): draws Z, decides on the device, reads the record; True when Y was accepted."""
        pd = self.pd
        self.lastZ = float(np.float32(pd.rng.uniform(0.0, 1.0)))
        check(self.lib.uammd_mc_forcebiased_decide(self.h, _ptr(pd.getPos("readwrite")), _ptr(pd.getForce("readwrite")),
                                                   _ptr(pd.getEnergy("read")), pd.N, self.trialStepSize, float(self.beta), self.lastZ,
                                                   current_stream()))
        accepted = self._result()
        if accepted:
            self.optimizeStepSize.registerAccept()
        else:
            self.optimizeStepSize.registerReject()
        return accepted

    def tryNewStep(self):
        """One trial (ForceBiased.cuh:220-233)."""
        self.proposeNewStep()
        return self.decideNewStep()

    def forwardTime(self):
        """ForceBiased::forwardTime (ForceBiased.cuh:191-200): tries until one trial is accepted."""
        if self.step == 0:
            self.firstStep()
        self.lastTrials = 0
        while True:
            self.lastTrials += 1
            self.totalTrials += 1
            if self.tryNewStep():
                return
            if self.lastTrials >= self.maxTrials:
                _log.error("[MC::ForceBiased] %d consecutive trials were rejected", self.lastTrials)
                raise RuntimeError(f"[MC::ForceBiased] {self.lastTrials} consecutive trials were rejected (maxTrials)")


class MC:
    ForceBiased = _ForceBiased
    Optimize = Optimize
