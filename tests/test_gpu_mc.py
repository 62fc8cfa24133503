"""GPU tests of MC_NVT.Anderson (uammd_amd/mc.py, uammd_amd/csrc/mc.hip).

Parity is BIT EQUALITY of positions and per-cell counters with the restatement tests/mc_ref.py after every step: the fixtures have no
undecided try (tests/test_mc_cpu.py asserts it), so every decision is determined.  The workgroup of the wave kernel holds 4 cells; the
subgrids of the 6^3 fixtures have 27, of the 6 x 4 x 8 fixture 24 and of the 4^3 fixture 8, so a partly filled last workgroup is covered
by every 6^3 fixture."""
import json
import os

import numpy as np
import pytest
import torch

import mc_ref
from util import lattice_positions

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
F = np.float32


def _tunable(hip, name, value):
    assert hip.load().uammd_hip_set_tunable(name.encode(), int(value)) == 0


@pytest.fixture(autouse=True)
def _default_tunables(hip):
    yield
    _tunable(hip, "mc_baseline", 0)
    _tunable(hip, "mc_stage_capacity", 512)


def _make(hip, name, **over):
    fx = mc_ref.Fixture(name)
    pd = hip.ParticleData(len(fx.pos), seed=fx.sysseed)
    pd.setPos(fx.pos.copy())
    pot = hip.Potential.LJ()
    for (ti, tj), (rc, sigma, eps, shift) in fx.pairs.items():
        pot.setPotParameters(ti, tj, pot.InputPairParameters(rc, sigma, eps, shift))
    assert np.array_equal(pot.table, fx.table)
    par = dict(box=hip.Box(fx.L), temperature=mc_ref.TEMPERATURE, triesPerCell=mc_ref.TRIES, initialJumpSize=mc_ref.JUMP,
               tuneSteps=1000, seed=mc_ref.SARU_SEED)
    par.update(over)
    mc = hip.MC_NVT.Anderson(pd, pot, hip.MC_NVT.Anderson.Parameters(**par))
    assert mc.cellDim == fx.cellDim
    return fx, pd, mc


def _trajectory(hip, name):
    """[(positions, tried, accepted)] after each step, as raw words."""
    fx, pd, mc = _make(hip, name)
    out = []
    for _ in range(mc_ref.STEPS):
        mc.forwardTime()
        t, a = mc.cell_counters()
        out.append((pd.getPos().cpu().numpy().view(np.uint32).copy(), t, a, mc.currentOrigin.copy()))
    return out


def _assert_parity(hip, name):
    ref = mc_ref.reference_run(name)
    got = _trajectory(hip, name)
    for step, ((pos, t, a, origin), (rpos, rt, ra, info, rorigin, _)) in enumerate(zip(got, ref), 1):
        assert np.array_equal(origin, rorigin)
        bad = np.flatnonzero((pos != rpos.view(np.uint32)).any(1))
        print(f"[{name}] step {step}: {len(bad)} rows differ, tried {int(t.sum())} ({int(rt.sum())}), accepted {int(a.sum())} ({int(ra.sum())})")
        assert np.array_equal(t, rt), f"step {step}: tried differs in cells {np.flatnonzero(t != rt)[:8]}"
        assert np.array_equal(a, ra), f"step {step}: accepted differs in cells {np.flatnonzero(a != ra)[:8]}"
        assert len(bad) == 0, f"step {step}: rows {bad[:8]} differ"
    return got


@pytest.mark.parametrize("name", ["cube6", "cube6_shifted", "cube6_two_types"])
def test_parity_6x6x6(hip, name):
    """Tests 1 and 10: 27 cells per subgrid, 7 workgroups of 4 waves with the last one partly filled."""
    _assert_parity(hip, name)


def test_parity_smallest_grid(hip):
    """Test 2: 4^3, a cell's -1 and +1 neighbours are two cells apart through the periodic wrap."""
    _assert_parity(hip, "cube4")


def test_parity_three_extents(hip):
    """Test 3: 6 x 4 x 8 cells from L / rc = 6.2, 4.08, 8.12."""
    _assert_parity(hip, "brick")


@pytest.mark.parametrize("baseline", [0, 1])
def test_2d_visits_every_cell_once(hip, baseline):
    """Test 4: four subgrids, z untouched, sum of tried per step = non-empty cells x triesPerCell and no cell tried twice."""
    _tunable(hip, "mc_baseline", baseline)
    got = _assert_parity(hip, "flat")
    ref = mc_ref.reference_run("flat")
    prev = np.zeros(64, np.uint32)
    for (pos, t, a, _), r in zip(got, ref):
        assert (pos.view(F)[:, 2] == 0).all()
        per_step = t - prev
        prev = t
        assert set(np.unique(per_step)) <= {0, mc_ref.TRIES}
        nonempty = 64 - int((per_step == 0).sum())
        assert per_step.sum() == nonempty * mc_ref.TRIES and nonempty > 32


def test_parity_dilute(hip):
    """Test 5: 40 particles in 216 cells; empty cells try nothing."""
    got = _assert_parity(hip, "dilute")
    assert (got[-1][1] == 0).sum() > 100


def test_parity_cell_above_64(hip):
    """Test 6: a cell with more rows than the wave has lanes."""
    assert max(r[3]["max_in_cell"] for r in mc_ref.reference_run("packed")) > 64
    _assert_parity(hip, "packed")


@pytest.mark.parametrize("capacity", [0, 150])
def test_global_memory_fallback(hip, capacity):
    """Test 7: neighbourhoods of the 6^3 fixture hold up to ~205 rows; with 150 rows of staging some waves stage and others do not, with
    0 none does.  Same bits."""
    assert max(r[3]["max_neighbourhood"] for r in mc_ref.reference_run("cube6")) > 150
    _tunable(hip, "mc_stage_capacity", capacity)
    _assert_parity(hip, "cube6")
    _tunable(hip, "mc_stage_capacity", 0)
    _assert_parity(hip, "packed")


def test_baseline_kernel_same_bits(hip):
    """Test 8 (with test_2d_visits_every_cell_once[1]): the thread-per-cell kernel against the wave kernel."""
    wave = _trajectory(hip, "cube6")
    _tunable(hip, "mc_baseline", 1)
    base = _trajectory(hip, "cube6")
    for w, b in zip(wave, base):
        assert all(np.array_equal(x, y) for x, y in zip(w, b))
    _assert_parity(hip, "cube6")


def test_two_runs_same_bits(hip):
    """Test 9."""
    a, b = _trajectory(hip, "cube6_two_types"), _trajectory(hip, "cube6_two_types")
    for x, y in zip(a, b):
        assert all(np.array_equal(p, q) for p, q in zip(x, y))


def test_sum_energy(hip):
    """Test 11: per-particle energies against the LJ traversal on create_update_grid's list, to float summation order."""
    fx, pd, mc = _make(hip, "cube6_shifted")
    mc.forwardTime()
    pd.getEnergy("write").fill_(7.0)          # sumEnergy replaces what was there
    assert mc.sumEnergy() == 0.0
    got = pd.getEnergy().cpu().numpy().copy()
    cd, ubox = hip.CellList.create_update_grid(mc.box, fx.rc)
    cl = hip.CellList()
    cl.update_grid(pd.getPos(), ubox, cd)
    want = torch.zeros(pd.N, dtype=torch.float32, device="cuda")
    cl.transverse_lj(mc.pot.device_table(), 1, mc.box, None, want, None)
    want = want.cpu().numpy()
    assert np.abs(want).max() > 1.0
    assert np.abs(got - want).max() <= 1e-5 * np.abs(want).max()
    assert np.array_equal(mc.currentOrigin, np.zeros(3, F))


def test_tuning_follows_the_rule(hip):
    """Test 12: 40 steps, tuneSteps 10, target 0.5, from jump 1.0: the jump size follows updateJumpSize on the GPU's own counters, which
    are reset on tune steps."""
    from uammd_amd.mc import update_jump_size
    fx, pd, mc = _make(hip, "cube6", initialJumpSize=1.0, tuneSteps=10, acceptanceRatio=0.5)
    jump = F(1.0)
    changed = 0
    for step in range(1, 41):
        before = mc._counters(reset=False)
        mc.forwardTime()
        if step % 10 == 0:
            assert mc._counters(reset=False) == (0, 0)
            t, a = mc.cell_counters()
            assert t.sum() == 0 and a.sum() == 0
        else:
            assert mc._counters(reset=False)[0] > before[0]
        if step % 10 == 0:
            ratio = mc.getCurrentAcceptanceRatio()
            assert 0.0 < ratio < 1.0
            new = update_jump_size(jump, F(ratio), 0.5, mc.cellSize, False)
            changed += new != jump
            jump = new
        assert F(mc.getCurrentStepSize()) == jump
    assert changed == 4


def test_acceptance_ratio_is_accepted_over_tried(hip):
    fx, pd, mc = _make(hip, "cube6", tuneSteps=3)
    for _ in range(2):
        mc.forwardTime()
    t2, a2 = mc._counters(reset=False)
    tc, ac = mc.cell_counters()
    assert (t2, a2) == (int(tc.sum()), int(ac.sum()))
    mc.forwardTime()
    ref = mc_ref.reference_run("cube6")[2]
    assert mc.getCurrentAcceptanceRatio() == float(F(int(ref[2].sum())) / F(int(ref[1].sum())))
    assert mc._counters(reset=False) == (0, 0)


def test_error_paths(hip):
    """Test 13: an invalid grid and a negative temperature raise before anything is launched."""
    import ctypes as C
    from uammd_amd._lib import f3, i3
    pd = hip.ParticleData(10)
    pot = hip.Potential.LJ()
    pot.setPotParameters(0, 0, pot.InputPairParameters(2.5, 1.0, 1.0, False))
    P = hip.MC_NVT.Anderson.Parameters
    with pytest.raises(ValueError):
        hip.MC_NVT.Anderson(pd, pot, P(box=hip.Box(15.0), temperature=-1.0))
    with pytest.raises(ValueError):
        hip.MC_NVT.Anderson(pd, pot, P(box=hip.Box(9.0), temperature=1.0))
    with pytest.raises(ValueError):
        hip.MC_NVT.Anderson(pd, pot, P(box=hip.Box((15.0, 15.0, 5.1)), temperature=1.0))
    lib = hip.load()
    fx, pd, mc = _make(hip, "cube4")
    before = pd.getPos().clone()
    order = (C.c_int * 8)(*range(8))
    ptr = C.c_void_p(pd.getPos().data_ptr())
    tbl = C.c_void_p(mc.pot.device_table().data_ptr())

    def step(cd, nsub, h=mc.h, p=ptr):
        return lib.uammd_mc_anderson_step(h, p, pd.N, f3(fx.L), i3([1, 1, 1]), i3(cd), f3(0.0), order, nsub, 10, 1.0, 0.1, 1, 1, tbl, 1,
                                          hip.current_stream())
    assert step([4, 4, 2], 8) == -1 and b"invalid grid" in lib.uammd_hip_last_error()
    assert step([2, 4, 4], 8) == -1
    assert step([5, 4, 4], 8) == -1
    assert step([4, 4, 4], 4) == -1 and b"numberSubgrids" in lib.uammd_hip_last_error()
    assert step([4, 4, 1], 8) == -1
    assert step([4, 4, 4], 8, h=None) == -1
    assert step([4, 4, 4], 8, p=None) == -1
    torch.cuda.synchronize()
    assert torch.equal(pd.getPos(), before)
    assert lib.uammd_hip_set_tunable(b"mc_stage_capacity", 100000) != 0 and lib.uammd_hip_set_tunable(b"mc_baseline", 2) != 0


EOS = {round(r["rho"], 2): r for r in json.load(open(os.path.join(HERE, "golden", "lj_eos_T3.json")))["rows"]}


def _eos_energy(hip, rho, temperature=3.0, relax=500, steps=1000, every=10):
    n, rc = 16384, 2.5
    L = (n / rho) ** (1.0 / 3.0)
    pd = hip.ParticleData(n)
    pd.setPos(lattice_positions(n, L, seed=7, jitter=0.05))
    pot = hip.Potential.LJ()
    pot.setPotParameters(0, 0, pot.InputPairParameters(rc, 1.0, 1.0, True))
    par = hip.MC_NVT.Anderson.Parameters(box=hip.Box(L), temperature=temperature, triesPerCell=40, initialJumpSize=0.1, tuneSteps=20,
                                         acceptanceRatio=0.8)
    mc = hip.MC_NVT.Anderson(pd, pot, par)
    for _ in range(relax):
        mc.forwardTime()
    U = []
    for s in range(steps):
        mc.forwardTime()
        if s % every == 0:
            mc.sumEnergy()
            U.append(float(pd.getEnergy().double().sum()) / n)
    return float(np.mean(U)), mc


@pytest.mark.parametrize("rho", [0.3, 0.6, 0.8])
def test_lj_equation_of_state(hip, rho):
    """Test 14, the reference's acceptance criterion (test/MC/ShortRange/test.bash) at the state points tests/test_gpu_lj_eos.py uses:
    N = 16384, T = 3, shifted LJ, 40 tries per cell, jump 0.1, tuneSteps 20, target 0.8, 500 + 1000 steps sampled every 10;
    E = 1.5 T + U / N against tests/golden/lj_eos_T3.json within 2 %.

    U is the sum of the per-particle energies: each carries half of its pairs (Potential.cuh:47-65), as in tests/test_gpu_lj_eos.py on
    the same golden file.  The reference's MonteCarlo.cu halves that sum once more, and its Metropolis rule takes the per-particle half
    for the pair energy; the two together put E = 1.5 T + U(2T) / 2N on the plot, far from the equation of state.

    Measured on an MI355X at this length (the test prints E, the golden value and the deviation in percent):
    rho = 0.3: E / N = 3.0701 against 3.0700 (+0.00 %);  rho = 0.6: 1.7659 against 1.7657 (+0.01 %);
    rho = 0.8: 1.2523 against 1.2453 (+0.56 %)."""
    U, mc = _eos_energy(hip, rho)
    E = 1.5 * 3.0 + U
    ref = EOS[rho]["E"]
    print(f"[MC EOS rho={rho}] E/N = {E:.4f} (reference tool {ref:.4f}, deviation {100 * (E - ref) / abs(ref):+.2f} %), "
          f"jump {mc.getCurrentStepSize():.4f}, acceptance {mc.getCurrentAcceptanceRatio():.3f}")
    assert abs(E - ref) <= 0.02 * abs(ref)
