"""MC::ForceBiased on the MI355X (uammd_amd/csrc/forcebiased.hip) against the NumPy restatement
tests/forcebiased_ref.py: the three sums, the decision, the commit, the proposal, live trials over PairForces, exact sampling of a
harmonic trap and the Lennard-Jones equation of state.

The bound on a sum of N terms formed and added in double is (N + 8) 2^-53 sum |term|: N - 1 additions in any order lose at most
(N - 1) u sum |term| to first order (u = 2^-53), a term is a handful of double operations on exactly converted floats (three subtractions,
three products with h, three squares and two additions: under 8 u relative), and the division by 4 h is one more rounding."""
import ctypes as C
import json
import math
import os
import subprocess

import numpy as np
import pytest
import torch

import forcebiased_ref as ref
from util import lattice_positions

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
F = np.float32
U53 = 2.0 ** -53
SIZES = [1, 63, 64, 65, 257, 5000, 20000]
# the 20-batch standard error of the restatement's trial-weighted <U> on the trap (tests/test_forcebiased_cpu.py prints it)
SE_REF = 0.0892


class Handle:
    """The C ABI on torch tensors."""

    def __init__(self, hip, borrowed=None):
        """borrowed: the handle of an integrator, which stays its owner."""
        from uammd_amd._lib import check
        self.lib, self.check, self.owned = hip.load(), check, borrowed is None
        self.h = C.c_void_p() if self.owned else borrowed
        if self.owned:
            check(self.lib.uammd_mc_forcebiased_create(C.byref(self.h)))

    def __del__(self):
        if self.owned:
            self.lib.uammd_mc_forcebiased_destroy(self.h)

    @staticmethod
    def _p(t):
        return None if t is None else C.c_void_p(t.data_ptr())

    def begin(self, pos, force, energy):
        self.check(self.lib.uammd_mc_forcebiased_begin(self.h, self._p(pos), self._p(force), self._p(energy), pos.shape[0], None))

    def propose(self, pos, h, beta, step, seed, noise=None):
        self.check(self.lib.uammd_mc_forcebiased_propose(self.h, self._p(pos), pos.shape[0], h, beta, step, seed, self._p(noise), None))

    def decide(self, pos, force, energy, h, beta, Z):
        self.check(self.lib.uammd_mc_forcebiased_decide(self.h, self._p(pos), self._p(force), self._p(energy), pos.shape[0], h, beta, Z, None))

    def result(self):
        acc, out = C.c_int(-1), (C.c_double * 6)()
        self.check(self.lib.uammd_mc_forcebiased_result(self.h, C.byref(acc), out, None))
        return acc.value, dict(zip(("EX", "EY", "TXY", "TYX", "exponent", "current"), out))

    def stored(self, n):
        p, f = (torch.empty((n, 4), dtype=torch.float32, device="cuda") for _ in range(2))
        self.check(self.lib.uammd_mc_forcebiased_stored(self.h, self._p(p), self._p(f), None))
        torch.cuda.synchronize()
        return p.cpu().numpy(), f.cpu().numpy()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _decades(rng, shape):
    """Random floats of both signs with magnitudes over six decades."""
    return (rng.choice([-1.0, 1.0], shape) * 10.0 ** rng.uniform(-3, 3, shape)).astype(F)


def _wide_case(n):
    rng = np.random.default_rng(1000 + n)
    X, Y, FX, FY = (_decades(rng, (n, 4)) for _ in range(4))
    return dict(X=X, Y=Y, FX=FX, FY=FY, e0=_decades(rng, n), e=_decades(rng, n), h=0.01, beta=2.0)


def _trap_case(n, uphill=False):
    """A trial of the harmonic trap with an exponent of order one: the step shrinks as 1 / sqrt(N), which keeps the trial's own exponent
    (about beta h^2 |X|^2 / 2) near 0.2 at every N, and E_Y is raised by 1, which puts the exponent near -2, so p = exp(exponent) is an
    ordinary number under 1.  uphill: E_X is raised by 10 instead and the exponent is near +20."""
    rng = np.random.default_rng(2000 + n)
    h, beta = float(F(0.05 * min(1.0, math.sqrt(64.0 / n)))), 2.0
    X = np.zeros((n, 4), F)
    X[:, :3] = rng.normal(0, 0.7, (n, 3))
    X[:, 3] = rng.integers(0, 5, n)
    fe = ref.trap(1.0)
    FX, e0 = fe(X)
    xi = rng.normal(0, 1, (n, 4)).astype(F) / F(np.sqrt(n))     # (a short move, so that exp(exponent) stays in range at every n)
    Y = ref.propose(X, FX, h, beta, xi)
    Y[:, 3] = 7
    FY, e = fe(Y)
    FX[:, 3], FY[:, 3] = 3, 4
    if uphill:
        e0 = e0 + F(10.0 / n)
    else:
        e = e + F(1.0 / n)
    return dict(X=X, Y=Y, FX=FX, FY=FY, e0=e0.astype(F), e=e.astype(F), h=h, beta=beta)


def _trial(hip, c, Z):
    """begin on (X, FX, e0), decide on (Y, FY, e): the record, the caller's arrays afterwards and the handle."""
    fb = Handle(hip)
    fb.begin(_dev(c["X"]), _dev(c["FX"]), _dev(c["e0"]))
    pos, force, e = _dev(c["Y"]), _dev(c["FY"]), _dev(c["e"])
    fb.decide(pos, force, e, c["h"], c["beta"], Z)
    acc, rec = fb.result()
    return acc, rec, pos.cpu().numpy(), force.cpu().numpy(), fb


def _expected(c):
    EX = ref.clamp_energy(c["e0"].astype(np.float64).sum())
    S, A = ref.sums(c["X"], c["Y"], c["FX"], c["FY"], c["e"], c["h"])
    return EX, S, A, ref.decide(EX, S, c["h"], c["beta"], 0.0)


def _same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32))


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind", ["wide", "trap"])
def test_sums(hip, n, kind):
    """1. E_Y, T_XY, T_YX of the record against float64 NumPy within (N + 8) 2^-53 sum |term|; E_X likewise; two calls, the same bits."""
    c = _wide_case(n) if kind == "wide" else _trap_case(n)
    EX, S, A, want = _expected(c)
    acc, rec, _, _, _ = _trial(hip, c, 0.5)
    b = (n + 8) * U53
    h4 = 4.0 * float(F(c["h"]))
    print(f"N {n} {kind}: E_Y {rec['EY']:.17g} ({want['EY']:.17g})  T_XY {rec['TXY']:.17g} ({want['TXY']:.17g})  "
          f"T_YX {rec['TYX']:.17g} ({want['TYX']:.17g})  bounds {b * A[0]:.3g} {b * A[1] / h4:.3g} {b * A[2] / h4:.3g}")
    assert abs(rec["EX"] - EX) <= b * np.abs(c["e0"].astype(np.float64)).sum()
    assert abs(rec["EY"] - want["EY"]) <= b * A[0]
    assert abs(rec["TXY"] - want["TXY"]) <= b * A[1] / h4
    assert abs(rec["TYX"] - want["TYX"]) <= b * A[2] / h4
    acc2, rec2, _, _, _ = _trial(hip, c, 0.5)
    assert acc2 == acc and all(np.float64(rec[k]).view(np.uint64) == np.float64(rec2[k]).view(np.uint64) for k in rec)


@pytest.mark.parametrize("n", SIZES)
def test_decision(hip, n):
    """2. accepted == Z < exp(exponent of the record), at Z = 0, just under and just over p = exp(exponent), and the largest float under 1;
    a trial with a positive exponent accepts every Z."""
    top = 1.0 - 2.0 ** -24
    for c in (_trap_case(n), _wide_case(n), _trap_case(n, uphill=True)):
        _, rec0, _, _, _ = _trial(hip, c, 0.0)
        p = ref.exp_or_inf(rec0["exponent"])
        zs = [z for z in (0.0, p * (1 - 1e-6), p * (1 + 1e-6), top) if 0.0 <= z < 1.0]
        for Z in zs:
            acc, rec, _, _, _ = _trial(hip, c, Z)
            assert rec["exponent"] == rec0["exponent"]
            assert acc == int(Z < p), (n, Z, p, rec)
            assert rec["current"] == (rec["EY"] if acc else rec["EX"])
    EX, S, A, want = _expected(_trap_case(n))
    assert -50 < want["exponent"] < 0 < 1e-300 < math.exp(want["exponent"])          # p is an ordinary number: both sides of it are tried
    c = _trap_case(n, uphill=True)
    assert _expected(c)[3]["exponent"] > 0 and _trial(hip, c, top)[0] == 1


def test_decision_corners(hip):
    """2. NaN or inf in energy: E_Y = FLT_MAX and a rejection even at Z = 0; an inf in F(Y) rejects; E_X = FLT_MAX from begin accepts any
    finite Y."""
    n = 257
    base = _trap_case(n)
    for bad in (np.nan, np.inf, -np.inf):
        c = dict(base, e=base["e"].copy())
        c["e"][100] = bad
        acc, rec, pos, force, _ = _trial(hip, c, 0.0)
        assert rec["EY"] == ref.FLT_MAX and acc == 0 and rec["current"] == rec["EX"]
        assert _same_bits(pos, c["X"]) and _same_bits(force, c["FX"])
    c = dict(base, FY=base["FY"].copy())
    c["FY"][200, 1] = np.inf
    acc, rec, _, _, _ = _trial(hip, c, 0.0)
    assert acc == 0 and rec["TYX"] == np.inf and rec["exponent"] == -np.inf
    for bad in (np.nan, np.inf):
        c = dict(base, e0=base["e0"].copy())
        c["e0"][3] = bad
        acc, rec, _, _, _ = _trial(hip, c, 1.0 - 2.0 ** -24)
        assert rec["EX"] == ref.FLT_MAX and acc == 1 and rec["current"] == rec["EY"] and math.isfinite(rec["EY"])


@pytest.mark.parametrize("n", [1, 65, 5000])
def test_commit(hip, n):
    """3. accepted: the stored arrays are Y, F(Y) to the bit, the caller's arrays are untouched, the energy is E_Y; rejected: the caller's
    pos and force hold X, F(X) to the bit, .w included, the stored arrays are unchanged, the energy is E_X."""
    c = _trap_case(n)
    acc, rec, pos, force, fb = _trial(hip, c, 0.0)
    sp, sf = fb.stored(n)
    assert acc == 1 and rec["current"] == rec["EY"]
    assert _same_bits(sp, c["Y"]) and _same_bits(sf, c["FY"]) and _same_bits(pos, c["Y"]) and _same_bits(force, c["FY"])
    # the next trial starts from the accepted state: E_X of its record is this E_Y
    fb.decide(_dev(c["X"]), _dev(c["FX"]), _dev(c["e0"]), c["h"], c["beta"], 0.0)
    assert fb.result()[1]["EX"] == rec["EY"]
    c = dict(c, e=c["e"] + F(100.0 / n))                      # far uphill: rejected at any Z > 0
    acc, rec, pos, force, fb = _trial(hip, c, 0.5)
    sp, sf = fb.stored(n)
    assert acc == 0 and rec["current"] == rec["EX"]
    assert _same_bits(pos, c["X"]) and _same_bits(force, c["FX"]) and (pos[:, 3] == c["X"][:, 3]).all() and (force[:, 3] == 3).all()
    assert _same_bits(sp, c["X"]) and _same_bits(sf, c["FX"])
    fb.decide(_dev(c["Y"]), _dev(c["FY"]), _dev(c["e"]), c["h"], c["beta"], 0.5)
    assert fb.result()[1]["EX"] == rec["EX"]


KEYS = [(0x1234ABCD, 1), (77, 4000)]
_NORMALS = {}


def _oracle_normals(o32, key, n):
    """The oracle's normals of a key, drawn once at the largest size (a particle's draws do not depend on N)."""
    if key not in _NORMALS:
        _NORMALS[key] = ref.normals(o32, key[0], key[1], 5000)
    return _NORMALS[key][:n]


@pytest.mark.parametrize("n", [s for s in SIZES if s <= 5000])
def test_proposal(hip, o32, n):
    """4. The exported normals against the oracle's within 1e-6; given the exported normals the positions are the restatement's to the bit;
    the same key, the same bits; another step or seed, other normals."""
    c = _trap_case(n)
    h, beta = 0.3, 2.0
    fb = Handle(hip)
    fb.begin(_dev(c["X"]), _dev(c["FX"]), _dev(c["e0"]))
    out = {}
    for seed, step in KEYS + [(KEYS[0][0], 2), (KEYS[0][0] + 1, 1)]:
        pos = torch.full((n, 4), -5.0, dtype=torch.float32, device="cuda")
        noise = torch.full((n, 4), -5.0, dtype=torch.float32, device="cuda")
        fb.propose(pos, h, beta, step, seed, noise)
        torch.cuda.synchronize()
        out[(seed, step)] = (pos.cpu().numpy(), noise.cpu().numpy())
    for key in KEYS:
        pos, noise = out[key]
        want = _oracle_normals(o32, key, n)
        assert np.abs(noise[:, :3] - want[:, :3]).max() <= 1e-6 and (noise[:, 3] == 0).all()
        assert _same_bits(pos, ref.propose(c["X"], c["FX"], h, beta, noise))
        assert (pos[:, 3] == c["X"][:, 3]).all()
        pos2 = torch.empty((n, 4), dtype=torch.float32, device="cuda")
        fb.propose(pos2, h, beta, key[1], key[0], None)         # without the export
        torch.cuda.synchronize()
        assert _same_bits(pos2.cpu().numpy(), pos)
    base = out[KEYS[0]][1][:, :3]
    for other in ((KEYS[0][0], 2), (KEYS[0][0] + 1, 1)):
        assert np.abs(out[other][1][:, :3] - base).max() > 0.1 * np.abs(base).max()


def _lj_system(hip, n=216, L=7.6, seed=0xF00D, jitter=0.05, beta=1.0, stepSize=1e-4, maxTrials=1000000, shift=True, pos=None):
    pd = hip.ParticleData(n, seed=seed)
    pd.setPos(lattice_positions(n, L, seed=7, jitter=jitter) if pos is None else pos)
    pot = hip.Potential.LJ()
    pot.setPotParameters(0, 0, pot.InputPairParameters(2.5, 1.0, 1.0, shift))
    mala = hip.MC.ForceBiased(pd, hip.MC.ForceBiased.Parameters(beta=beta, stepSize=stepSize, acceptanceRatio=0.5, maxTrials=maxTrials))
    mala.addInteractor(hip.PairForces(pd, hip.Box(L), pot))
    return pd, mala


def _host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy().copy()


def test_live_trials_over_pair_forces(hip):
    """5. MC.ForceBiased with PairForces (LJ, rc 2.5, shifted) on 216 particles in L = 7.6, 50 calls.  After every trial the exponent is
    rebuilt in float64 from the arrays read back (X and F(X) from the handle, Y, F(Y) and the energies from ParticleData before the
    decision); the record agrees within the bound of the sums carried through the exponent, and the decision is Z < exp(exponent) whenever
    that bound decides it.  The step size and the published ratio follow Optimize fed with the observed decisions."""
    n = 216
    pd, mala = _lj_system(hip, stepSize=3e-4)
    fb = Handle(hip, borrowed=mala.h)
    opt = ref.Optimize(0.5, 3e-4)
    mala.firstStep()
    EX = None
    trials = accepted_total = undecided = 0
    b = (n + 8) * U53
    for call in range(50):
        while True:
            trials += 1
            X, FX = fb.stored(n)
            mala.proposeNewStep()
            Y, FY, e = _host(pd.getPos()), _host(pd.getForce()), _host(pd.getEnergy())
            h = mala.trialStepSize
            assert h == float(opt.step)
            acc = mala.decideNewStep()
            rec = dict(zip(("EX", "EY", "TXY", "TYX", "exponent", "current"), mala.lastRecord))
            if EX is not None:
                assert rec["EX"] == EX
            S, A = ref.sums(X, Y, FX, FY, e, h)
            want = ref.decide(rec["EX"], S, h, mala.beta, mala.lastZ)
            h4 = 4.0 * float(F(h))
            beta = float(mala.beta)
            tol = beta * b * (A[0] + (A[1] + A[2]) / h4) + 8 * U53 * beta * (abs(rec["EY"]) + abs(rec["EX"]) + rec["TXY"] + rec["TYX"])
            assert abs(rec["EY"] - want["EY"]) <= b * A[0]
            assert abs(rec["exponent"] - want["exponent"]) <= tol, (rec, want, tol)
            if mala.lastZ == 0.0 or abs(math.log(mala.lastZ) - rec["exponent"]) > tol:
                assert acc == want["accepted"]
            else:
                undecided += 1
            assert acc == (mala.lastZ < ref.exp_or_inf(rec["exponent"]))
            opt.register(acc)
            assert mala.getCurrentStepSize() == float(opt.step) and mala.getCurrentAcceptanceRatio() == float(opt.ratio)
            EX = rec["current"]
            if acc:
                accepted_total += 1
                assert _same_bits(_host(pd.getPos()), Y) and _same_bits(_host(pd.getForce()), FY)
                break
            assert _same_bits(_host(pd.getPos()), X) and _same_bits(_host(pd.getForce()), FX)
        total = _host(pd.getEnergy()).astype(np.float64)
        assert abs(mala.getCurrentEnergy() - total.sum()) <= b * np.abs(total).sum()
    print(f"live: {trials} trials for 50 calls, {undecided} within rounding of the threshold, E {mala.getCurrentEnergy():.6f}")
    assert accepted_total == 50 and undecided <= 1


def test_same_seed_same_trajectory(hip):
    """5. The same system seed twice: the same positions, energies and trial counts to the bit."""
    runs = []
    for _ in range(2):
        pd, mala = _lj_system(hip, stepSize=3e-4)
        counts = []
        for _ in range(50):
            mala.forwardTime()
            counts.append(mala.getLastNumberOfTrials())
        runs.append((_host(pd.getPos()), counts, mala.getCurrentEnergy(), mala.getTotalNumberOfTrials()))
    assert _same_bits(runs[0][0], runs[1][0]) and runs[0][1:] == runs[1][1:]
    assert runs[0][3] == sum(runs[0][1]) >= 50
    pd, mala = _lj_system(hip, stepSize=3e-4, seed=0xBEEF)
    for _ in range(50):
        mala.forwardTime()
    assert not _same_bits(_host(pd.getPos()), runs[0][0])


def test_max_trials_raises_and_leaves_x(hip):
    """5. Two coincident particles: E_X is finite (the pair contributes nothing at r = 0) but every proposal separates them by a hair and
    is rejected; maxTrials = 3 raises after 3 trials with the positions at X."""
    start = lattice_positions(216, 7.6, seed=7, jitter=0.05)
    start[1] = start[0]
    pd, mala = _lj_system(hip, maxTrials=3, pos=start)
    with pytest.raises(RuntimeError, match="3 consecutive trials"):
        mala.forwardTime()
    assert mala.getLastNumberOfTrials() == 3 and mala.getTotalNumberOfTrials() == 3
    assert math.isfinite(mala.lastRecord[0]) and mala.lastRecord[0] < 1e6 and mala.getCurrentEnergy() == mala.lastRecord[0]
    assert _same_bits(_host(pd.getPos()), start)


def test_exact_sampling_of_the_harmonic_trap(hip):
    """6. The trap of tests/test_forcebiased_cpu.py (N = 64, k = 1, beta = 2, h0 = 0.3, 10 000 calls, the first fifth dropped) with a
    Python Interactor written in torch: the trial-weighted <U> is within 5 se_ref of 3 N / (2 beta) = 48, se_ref = 0.0892 being the
    restatement's 20-batch standard error (never this run's own); the factor 5 covers this run being one more draw from the same
    distribution.  The unweighted mean over the states after each call is printed beside it (biased upwards).
    Measured on an MI355X: weighted 48.126, unweighted 49.408, 18 817 trials."""
    N, k, beta, h0, calls = 64, 1.0, 2.0, 0.3, 10000
    pd = hip.ParticleData(N, seed=0xABCDEF)
    rng = np.random.default_rng(2024)
    start = np.zeros((N, 4), F)
    start[:, :3] = rng.normal(0, np.sqrt(1 / (beta * k)), (N, 3))
    pd.setPos(start)

    class Trap(hip.Interactor):
        def sum(self, force=True, energy=False, virial=False):
            p = pd.getPos("read")[:, :3]
            if force:
                pd.getForce("readwrite")[:, :3] -= k * p
            if energy:
                pd.getEnergy("readwrite").add_((0.5 * k) * (p * p).sum(dim=1))

    mala = hip.MC.ForceBiased(pd, hip.MC.ForceBiased.Parameters(beta=beta, stepSize=h0, acceptanceRatio=0.5))
    mala.addInteractor(Trap())
    mala.firstStep()
    mala._result()
    u_start, u_after, trials = [], [], []
    for _ in range(calls):
        u_start.append(mala.getCurrentEnergy())
        mala.forwardTime()
        u_after.append(mala.getCurrentEnergy())
        trials.append(mala.getLastNumberOfTrials())
    drop = calls // 5
    mean, se_own = ref.weighted_mean_and_error(u_start[drop:], trials[drop:])
    print(f"trap on the device: weighted <U> {mean:.4f}  unweighted <U> {np.mean(u_after[drop:]):.4f}  (own se {se_own:.4f}, se_ref {SE_REF})  "
          f"trials {sum(trials)}  step {mala.getCurrentStepSize():.4f}  ratio {mala.getCurrentAcceptanceRatio():.3f}")
    assert abs(mean - 48.0) <= 5 * SE_REF, mean


EOS = {round(r["rho"], 2): r for r in json.load(open(os.path.join(HERE, "golden", "lj_eos_T3.json")))["rows"]}


@pytest.mark.parametrize("rho", [0.3, 0.6])
def test_lj_equation_of_state(hip, rho):
    """7. N = 512 on a lattice with jitter 0.05, T = 3, shifted LJ with rc = 2.5, h0 = 2e-4, target 0.5, 2000 + 3000 calls, U / N sampled
    after every 10th call as the reference's program writes it; E = 1.5 T + U / N against tests/golden/lj_eos_T3.json within 2 %, the bar
    tests/test_gpu_mc.py uses on the same file.  U is the sum of the per-particle energies.
    A NumPy MALA at N = 500 gave 3.0602 (-0.32 %) at rho = 0.3 and 1.7785 (+0.72 %) at rho = 0.6; measured on an MI355X:
    rho = 0.3: E = 3.0635 (-0.21 %), final step 1.30e-4, 10 377 trials;  rho = 0.6: 1.7658 (+0.00 %), 9.51e-5, 13 653 trials."""
    n, T = 512, 3.0
    L = (n / rho) ** (1.0 / 3.0)
    pd, mala = _lj_system(hip, n=n, L=L, beta=1.0 / T, stepSize=2e-4)
    for _ in range(2000):
        mala.forwardTime()
    samples = []
    for j in range(3000):
        mala.forwardTime()
        if j % 10 == 0:
            samples.append(mala.getCurrentEnergy() / n)
    E = 1.5 * T + float(np.mean(samples))
    gold = EOS[round(rho, 2)]["E"]
    print(f"rho {rho}: E {E:.4f}  golden {gold:.4f}  deviation {100 * (E / gold - 1):+.2f} %  step {mala.getCurrentStepSize():.3e}  "
          f"trials {mala.getTotalNumberOfTrials()}")
    assert abs(E / gold - 1) <= 0.02


def test_cxx_class(hip):
    """The C++ class: its constructor's refusals (they need a ParticleData, so a GPU) and examples/forcebiased.cpp, which ends by comparing
    getCurrentEnergy() with the sum of pd->getEnergy()."""
    build = os.path.join(ROOT, "examples", "_build")
    r = subprocess.run([os.path.join(build, "forcebiased_host"), "refusals"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    for what in ("default beta", "stepSize 0", "acceptanceRatio 0", "maxTrials 0"):
        assert f"{what}: Invalid parameter" in lines, r.stdout
    assert "seed draw: one next32" in lines and f"accessors: 0 {float(F(0.1)):g} 0 0 0" in lines, r.stdout
    r = subprocess.run([os.path.join(build, "forcebiased"), "512", "0.6", "3.0", "300"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    print(r.stdout.strip())
    fields = r.stdout.split()
    assert int(fields[fields.index("trials") + 1]) >= 450 and math.isfinite(float(fields[fields.index("U/N") + 1]))
