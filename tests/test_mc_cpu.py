"""CPU tests of the Monte Carlo module: the host rules of MC_NVT.Anderson (grid, jump-size tuning, the draws from System::rng()) and
the restatement tests/mc_ref.py that the GPU parity tests compare against, including its guarantee that no try of a parity fixture is
undecided (see mc_ref's docstring)."""
import numpy as np
import pytest

import mc_ref
from uammd_amd.md import Box, Xorshift128plus
from uammd_amd.mc import MC_NVT, check_grid_validity, create_grid, update_jump_size

F = np.float32


class _HostOnlyParticleData:
    """What the host side of the integrator touches: the System::rng() mirror."""

    def __init__(self, seed):
        self.N = 0
        self.rng = Xorshift128plus()
        self.rng.set_seed(seed)


class _Pot:
    ntypes = 1

    def getCutOff(self):
        return 2.5


def test_grid_rule_and_validity():
    assert create_grid((15.0, 15.0, 15.0), 2.5) == [6, 6, 6]
    assert create_grid((17.6, 18.0, 20.0), 2.5) == [6, 6, 8]          # 7 -> 6, 7 -> 6, 8
    assert create_grid((15.5, 10.2, 20.3), 2.5) == [6, 4, 8]
    assert create_grid((20.0, 20.0, 0.0), 2.5) == [8, 8, 1]           # 2D
    assert check_grid_validity([6, 6, 6]) and check_grid_validity([8, 8, 1]) and check_grid_validity([4, 4, 4])
    assert create_grid((15.0, 15.0, 5.1), 2.5)[2] == 2 and not check_grid_validity(create_grid((15.0, 15.0, 5.1), 2.5))
    assert create_grid((9.0, 15.0, 15.0), 2.5)[0] == 2 and not check_grid_validity(create_grid((9.0, 15.0, 15.0), 2.5))   # 3 -> 2
    assert not check_grid_validity([6, 2, 6])
    assert mc_ref.create_grid((17.6, 18.0, 20.0), 2.5) == [6, 6, 8]


def test_invalid_grid_and_negative_temperature_raise():
    P = MC_NVT.Anderson.Parameters
    with pytest.raises(ValueError, match="Negative temperature"):
        MC_NVT.Anderson(_HostOnlyParticleData(1), _Pot(), P(box=Box(15.0), temperature=-1.0))
    with pytest.raises(ValueError, match="Cut off is too large"):
        MC_NVT.Anderson(_HostOnlyParticleData(1), _Pot(), P(box=Box(9.0), temperature=1.0))
    with pytest.raises(ValueError, match="Cut off is too large"):
        MC_NVT.Anderson(_HostOnlyParticleData(1), _Pot(), P(box=Box((15.0, 15.0, 5.1)), temperature=1.0))


def test_jump_size_rule():
    cs = [F(2.5), F(2.0), F(1.5)]
    assert update_jump_size(1.0, 0.3, 0.5, cs, False) == F(float(F(1.0)) * 0.9)
    assert update_jump_size(1.0, 0.7, 0.5, cs, False) == F(float(F(1.0)) * 1.02)
    assert update_jump_size(1.0, 0.5, 0.5, cs, False) == F(1.0)                      # on target: unchanged
    assert update_jump_size(1.49, 0.7, 0.5, cs, False) == F(1.5)                     # capped by the smallest edge, z included in 3D
    assert update_jump_size(1.99, 0.7, 0.5, cs, True) == F(2.0)                      # x and y only in 2D
    floor = F(2.5) / F(100000)
    assert update_jump_size(floor, 0.1, 0.5, cs, False) == floor                     # floored at cellSize.x / 100000
    assert update_jump_size(float(floor) * 1.05, 0.1, 0.5, cs, False) == floor
    j = F(1.0)
    for _ in range(5):
        j = update_jump_size(j, 0.0, 0.5, cs, False)
    want = F(1.0)
    for _ in range(5):
        want = F(float(want) * 0.9)
    assert j == want and j.dtype == np.float32


@pytest.mark.parametrize("L,is2D", [((15.0, 15.0, 15.0), False), ((20.0, 20.0, 0.0), True)])
def test_host_draws_follow_the_system_generator(L, is2D):
    """Seed, then per step three uniforms for the origin and n - 1 next() for the shuffle, in that order (Anderson.cu:98-101,177-185,219-225)."""
    seed = 0xC0FFEE
    mc = MC_NVT.Anderson(_HostOnlyParticleData(seed), _Pot(), MC_NVT.Anderson.Parameters(box=Box(L), temperature=1.5))
    r = Xorshift128plus()
    r.set_seed(seed)
    assert mc.seed == r.next32()                                   # par.seed == 0: drawn first
    n = 4 if is2D else 8
    for _ in range(4):
        got_o, got_s = mc.draw_origin(), mc.draw_subgrid_order()
        u = [-1.0 + (float(r.next()) / float(0xFFFFFFFFFFFFFFFF)) * 2.0 for _ in range(3)]
        want_o = [F(x * float(F(0.5 * L[0]))) for x in u]
        if is2D:
            want_o[2] = F(0)
        order = list(range(8))
        for i in range(n - 1):
            j = i + r.next() % (n - i)
            order[i], order[j] = order[j], order[i]
        assert got_o.dtype == np.float32 and list(got_o) == want_o
        assert got_s == order[:n] and sorted(got_s) == list(range(n))
    fixed = MC_NVT.Anderson(_HostOnlyParticleData(seed), _Pot(), MC_NVT.Anderson.Parameters(box=Box(L), temperature=1.5, seed=77))
    r2 = Xorshift128plus()
    r2.set_seed(seed)
    assert fixed.seed == 77 and fixed.pd.rng.s == r2.s             # a given seed draws nothing


def test_saru_float_reaches_one():
    """(int)(u >> 1) * 2^-31 rounds up to 1.0 for the top 64 integers: the pick must be clamped."""
    top = (np.array([0xFFFFFFFF, 0xFFFFFF80, 0xFFFFFF7F], np.uint32) >> np.uint32(1)).astype(np.int32).astype(F) * mc_ref.TWO_M31
    assert top[0] == F(1.0) and top[1] == F(1.0) and top[2] < F(1.0)


def test_restatement_on_a_two_particle_toy(o32):
    """Two particles in one cell of a 4^3 grid: moves that lower the energy are accepted whatever Z is, a move out of the cell is
    rejected without drawing Z (the stream then continues with the next try's pick), every cell is visited once, empty cells count nothing."""
    L, cd = (10.0, 10.0, 10.0), [4, 4, 4]
    tab = mc_ref.lj_table(mc_ref.ONE, 1)
    pos = np.zeros((2, 4), F)
    pos[0, :3] = (-3.75, -3.75, -3.75)          # the centre of cell (0, 0, 0)
    pos[1, :3] = (-3.75 + 0.9, -3.75, -3.75)    # r = 0.9 < 2^(1/6): strongly repulsive
    origin = np.zeros(3, F)
    p, tried, acc, info = mc_ref.mc_step(o32, pos, L, [1, 1, 1], cd, origin, list(range(8)), 40, 1.0, 0.3, 1, 5, tab, 1)
    assert (info["visits"] == 1).all()
    assert tried[0] == 40 and tried[1:].sum() == 0 and info["tries"] == 40
    d0 = np.linalg.norm(pos[1, :3] - pos[0, :3])
    d1 = np.linalg.norm(p[1, :3].astype(np.float64) - p[0, :3])
    assert acc[0] > 0 and d1 > d0                                   # the pair relaxed apart: downhill moves were taken
    # a jump larger than the cell: most tries leave the cell and consume four draws, not five
    big = mc_ref.mc_step(o32, pos, L, [1, 1, 1], cd, origin, list(range(8)), 40, 1.0, 5.0, 1, 5, tab, 1)
    assert big[3]["out_of_cell"] > 20 and big[1][0] == 40 and big[2][0] <= 40 - big[3]["out_of_cell"]
    # downhill is always accepted: replay the first in-cell try by hand
    f = mc_ref.saru_f(o32, 5, 1, 0, 5)
    pick = min(int(f[0] * F(2)), 1)
    new = pos[pick].copy()
    new[:3] = [pos[pick, k] + F(0.3) * (F(2) * f[1 + k] - F(1)) for k in range(3)]
    other = pos[1 - pick]
    u_old = mc_ref.pair_energy(pos[pick], other[None], np.asarray(L, F), [True] * 3, tab, 1)[0][0]
    u_new = mc_ref.pair_energy(new, other[None], np.asarray(L, F), [True] * 3, tab, 1)[0][0]
    one = mc_ref.mc_step(o32, pos, L, [1, 1, 1], cd, origin, list(range(8)), 1, 1.0, 0.3, 1, 5, tab, 1)
    moved = not np.array_equal(one[0], pos)
    if u_new <= u_old:
        assert moved and one[2][0] == 1
    else:
        assert moved == (np.log(float(f[4])) + (u_new - u_old) <= 0)


@pytest.mark.parametrize("name", list(mc_ref.FIXTURES))
def test_parity_fixture_has_no_undecided_try(name):
    fx = mc_ref.Fixture(name)
    run = mc_ref.reference_run(name)
    assert len(run) == mc_ref.STEPS
    assert sum(r[3]["undecided"] for r in run) == 0
    assert sum(r[3]["tries"] for r in run) > 1000 and int(run[-1][2].sum()) > 100      # the fixture exercises both outcomes
    assert sum(r[3]["out_of_cell"] for r in run) > 50
    for r in run:
        assert (r[3]["visits"] == 1).all()
    if name == "packed":
        assert max(r[3]["max_in_cell"] for r in run) > 64
    if name == "dilute":
        assert (run[-1][1] == 0).sum() > fx.cellDim[0] ** 3 // 2
    if name == "flat":
        assert fx.cellDim == [8, 8, 1] and all(len(r[5]) == 4 for r in run) and (run[-1][0][:, 2] == 0).all()
    if name == "cube4":
        assert fx.cellDim == [4, 4, 4]
    if name == "brick":
        assert fx.cellDim == [6, 4, 8]
