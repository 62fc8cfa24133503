"""GPU parity of the double-precision Verlet list (uammd_amd/csrc/verletlist_f64.hip, f64.VerletList) against the -DDOUBLE_PRECISION
oracle (oracle/src/lj.c K7 / K8 + oracle/verletlist.py host logic on oracle.real = float64).

Bars: the list itself (groupIndex, numberNeighbours, every valid entry, capacity, the sortPos bits) is exact.  Forces keep the list order
and the oracle's FMA placement: per particle |dF_i| <= BAR = 1e-5 * 2^-29 times the particle's largest force component (the f64 suite's
rule: the float bar carried over by the ratio of the unit roundoffs); the number of differing 64-bit words is printed and asserted zero
on the fixtures where the first GPU run found zero (all four).  The rebuild schedule is a function of double comparisons on bit-identical
trajectories: exact."""
import math

import numpy as np
import pytest
import torch

from util import lattice_positions

pytestmark = pytest.mark.gpu

BAR = 1e-5 * 2.0 ** -29      # 1.86e-14

# n, L, rc, periodic, ntypes
FIXTURES = {"liquid": (6400, 20.0, 2.5, (1, 1, 1), 1),                      # the capacity must reach 96
            "noncubic3": (3000, (14.0, 17.0, 21.0), 2.5, (1, 1, 1), 3),
            "open-z": (2000, (16.0, 16.0, 9.0), 2.5, (1, 1, 0), 1),          # z collapses to one cell
            "dilute": (500, 30.0, 1.2, (1, 1, 1), 1)}                        # capacity stays 32
BITWISE = ("liquid", "noncubic3", "open-z", "dilute")


def _positions(n, L, periodic=(1, 1, 1), seed=77, ntypes=1, jitter=0.15):
    """util.lattice_positions in float64 plus +-1e-7 of uniform noise (inputs that no float holds); unwrapped rows in the periodic
    directions: x += Lx on every 7th row, z -= 2 Lz on every 11th."""
    pos = lattice_positions(n, L, seed=seed, jitter=jitter, ntypes=ntypes, dtype=np.float64)
    pos[:, :3] += np.random.default_rng(seed + 1).uniform(-1e-7, 1e-7, (n, 3))
    L3 = np.broadcast_to(np.asarray(L, np.float64), (3,))
    for k in range(3):
        if not periodic[k]:
            pos[:, k] = np.clip(pos[:, k], -L3[k] / 2 + 0.01, L3[k] / 2 - 0.01)
    if periodic[0]:
        pos[::7, 0] += L3[0]
    if periodic[2]:
        pos[::11, 2] -= 2 * L3[2]
    return pos


def _pot(f64, rc, ntypes=1):
    pot = f64.LJ()
    for ti in range(ntypes):
        for tj in range(ti, ntypes):
            pot.setPotParameters(ti, tj, pot.InputPairParameters(rc * (1.0 - 0.04 * ti), 1.0 + 0.03 * tj, 1.0 + 0.1 * ti + 0.2 * tj,
                                                                 (ti + tj) % 2 == 1))
    return pot


_cache = {}


def _reference(o64, f64, name):
    """The oracle's list and forces of one fixture, computed once and shared (never modified)."""
    if name not in _cache:
        from oracle.verletlist import VerletListOracle
        n, L, rc, periodic, ntypes = FIXTURES[name]
        pos = _positions(n, L, periodic, ntypes=ntypes)
        pot = _pot(f64, rc, ntypes)
        ref = VerletListOracle(o64)
        ref.update(pos, L, list(periodic), float(pot.getCutOff()))
        f1 = ref.lj_forces(L, list(periodic), pot.table, pot.ntypes)[0]
        fev = ref.lj_forces(L, list(periodic), pot.table, pot.ntypes, want_energy=True, want_virial=True)
        for a in (pos, f1) + tuple(fev):
            a.setflags(write=False)
        _cache[name] = dict(pos=pos, pot=pot, ref=ref, f=f1, fev=fev)
    return _cache[name]


def _compare_lists(h, ref):
    n = len(ref.numberNeighbours)
    assert h["particleStride"] == n and h["numberParticles"] == n
    assert h["maxNeighboursPerParticle"] == ref.maxNeighboursPerParticle
    assert np.array_equal(h["groupIndex"], ref.groupIndex)
    assert np.array_equal(h["numberNeighbours"], ref.numberNeighbours)
    m = ref.maxNeighboursPerParticle
    a = h["neighbourList"]                                   # [capacity, n]
    b = ref.neighbourList.reshape(m + 1, n)[:m]
    valid = np.arange(m)[:, None] < ref.numberNeighbours[None, :]
    assert np.array_equal(a[valid], b[valid])
    assert np.array_equal(h["sortPos"].view(np.uint64), np.ascontiguousarray(ref.sortPos).view(np.uint64))
    return valid


def _rel_err(got, ref):
    """per particle: the largest component error over the particle's largest force component"""
    fmax = np.abs(ref[:, :3]).max(axis=1) + 1e-300
    return (np.abs(got[:, :3] - ref[:, :3]).max(axis=1) / fmax).max()


def _words(a, b):
    return int((np.ascontiguousarray(a).view(np.uint64) != np.ascontiguousarray(b).view(np.uint64)).sum())


def _forces(vl, pot, box, n, fev):
    f = torch.zeros((n, 4), dtype=torch.float64, device="cuda")
    e = torch.zeros(n, dtype=torch.float64, device="cuda") if fev else None
    v = torch.zeros(n, dtype=torch.float64, device="cuda") if fev else None
    vl.transverse_lj(pot.device_table(), pot.ntypes, box, f, e, v)
    torch.cuda.synchronize()
    return tuple(None if t is None else t.cpu().numpy() for t in (f, e, v))


# ---- 1 -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(FIXTURES))
def test_list_and_forces_match_oracle(hip, o64, name):
    from uammd_amd import f64
    n, L, rc, periodic, ntypes = FIXTURES[name]
    fx = _reference(o64, f64, name)
    ref, pot = fx["ref"], fx["pot"]
    box = f64.Box(L, periodic)
    vl = f64.VerletList()
    d_pos = torch.from_numpy(np.array(fx["pos"], order="C")).cuda()
    assert vl.update(box, float(pot.getCutOff()), d_pos) and vl.rebuilds == 1
    h = vl.to_host()
    valid = _compare_lists(h, ref)
    if name == "liquid":
        assert h["maxNeighboursPerParticle"] == 96
    if name == "dilute":
        assert h["maxNeighboursPerParticle"] == 32
    own = (h["neighbourList"] == np.arange(n)[None, :]) & valid      # the particle is its own neighbour, exactly once
    assert np.all(own.sum(axis=0) == 1)
    f, _, _ = _forces(vl, pot, box, n, False)
    err, nbits = _rel_err(f, fx["f"]), _words(f[:, :3], fx["f"][:, :3])
    print(f"[{name}] F: max rel err {err:.3e}, words differing {nbits} / {3 * n}")
    assert err <= BAR and np.all(f[:, 3] == 0)
    f2, e2, v2 = _forces(vl, pot, box, n, True)
    rf, re_, rv = fx["fev"]
    err2 = _rel_err(f2, rf)
    erre = np.abs(e2 - re_).max() / max(np.abs(re_).max(), 1e-300)      # (the dilute fixture has no pair inside its cut-off: all zeros)
    errv = np.abs(v2 - rv).max() / max(np.abs(rv).max(), 1e-300)
    nbits2 = _words(f2[:, :3], rf[:, :3]) + _words(e2, re_) + _words(v2, rv)
    print(f"[{name}] F+E+V: max rel err F {err2:.3e} E {erre:.3e} V {errv:.3e}, words differing {nbits2} / {5 * n}")
    assert err2 <= BAR and erre <= BAR and errv <= BAR
    if name in BITWISE:
        assert nbits == 0 and nbits2 == 0


# ---- 2 -------------------------------------------------------------------------------------------------------------------------------
def test_skin_shell_membership(hip, o64):
    """2000 pairs at distances within 64 ulp on either side of 1.08 rc, anchors anywhere in the box (so the pairs cross cell faces) and
    partners stored where the vector ends (so they cross box faces): membership equals the oracle's exactly."""
    from oracle.verletlist import VerletListOracle
    from uammd_amd import f64
    L, rc, npairs = 20.0, 2.5, 2000
    rcut = rc * 1.08
    rng = np.random.default_rng(41)
    a = rng.uniform(-L / 2, L / 2, (npairs, 3))
    u = rng.normal(0, 1, (npairs, 3))
    u /= np.linalg.norm(u, axis=1)[:, None]
    u[::5] = np.eye(3)[rng.integers(0, 3, len(u[::5]))]          # a fifth along the axes: the distance is then a single coordinate
    m = rng.integers(-64, 65, npairs)
    r = rcut * (1.0 + m * 2.0 ** -52)
    pos = np.zeros((2 * npairs, 4))
    pos[0::2, :3] = a
    pos[1::2, :3] = a + u * r[:, None]
    ref = VerletListOracle(o64)
    ref.update(pos, L, [1, 1, 1], rc)
    vl = f64.VerletList()
    vl.update(f64.Box(L), rc, torch.from_numpy(pos).cuda())
    h = vl.to_host()
    _compare_lists(h, ref)
    # the fixture does sit on the edge: of the partners, some are in their anchor's list and some are not
    inv = np.empty(2 * npairs, np.int64)
    inv[ref.groupIndex] = np.arange(2 * npairs)
    nl = ref.neighbourList.reshape(ref.maxNeighboursPerParticle + 1, -1)
    inside = np.array([inv[2 * p + 1] in nl[:ref.numberNeighbours[inv[2 * p]], inv[2 * p]] for p in range(npairs)])
    print(f"[skin shell] {inside.sum()} of {npairs} partners inside, capacity {h['maxNeighboursPerParticle']}")
    assert 0.25 * npairs < inside.sum() < 0.75 * npairs


# ---- 3 -------------------------------------------------------------------------------------------------------------------------------
def test_forces_equal_celllist_forces_up_to_rounding(hip):
    """The same pairs as f64.CellList, summed in another order: 1e-5 * 2^-29 of max|F|."""
    from uammd_amd import f64
    n, L, rc = 8000, 21.5443469, 2.5
    pos = lattice_positions(n, L, seed=5, jitter=0.12, dtype=np.float64)
    box, pot = f64.Box(L), _pot(f64, rc)
    d_pos = torch.from_numpy(pos).cuda()
    vl, cl = f64.VerletList(), f64.CellList()
    vl.update(box, rc, d_pos)
    cl.update(box, rc, d_pos)
    f1 = torch.zeros((n, 4), dtype=torch.float64, device="cuda")
    f2 = torch.zeros_like(f1)
    vl.transverse_lj(pot.device_table(), 1, box, f1)
    cl.transverse_lj(pot.device_table(), 1, box, f2)
    err = (f1 - f2).abs().max().item() / f2.abs().max().item()
    print(f"[verlet list vs cell list] max |dF| / max|F| = {err:.3e}")
    assert err <= BAR


# ---- 4 -------------------------------------------------------------------------------------------------------------------------------
def test_rebuild_schedule_and_trajectory_match_oracle(hip, o64):
    """40 Gronbech-Jensen steps at T = 0 through f64.VerletNVT + PairForcesLJ(nl=f64.VerletList()): rebuilds at the oracle loop's steps,
    the same position bits, the same number of steps since the last rebuild."""
    from oracle.verletlist import VerletListOracle
    from uammd_amd import f64
    n, L, rc, dt, nsteps = 4096, 17.3, 2.5, 0.005, 40
    pos = lattice_positions(n, L, seed=21, jitter=0.05, dtype=np.float64)
    vel = np.random.default_rng(9).normal(0, 1.2, (n, 3))
    ref = VerletListOracle(o64)
    par = o64.lj_params(rc, 1.0, 1.0)
    p, v = pos.copy(), vel.copy()

    def ref_forces():
        ref.handlePosWriteRequested()
        ref.update(p, L, 1, rc)
        return ref.lj_forces(L, 1, par, 1)[0]
    f = ref_forces()
    ref_steps = []
    for s in range(1, nsteps + 1):
        o64.verletnvt_gj(1, p, v, f, dt, 1.0, 0.0, s, 1234)
        before = ref.rebuilds
        f = ref_forces()
        if ref.rebuilds != before:
            ref_steps.append(s)
        o64.verletnvt_gj(2, p, v, f, dt, 1.0, 0.0, s, 1234)

    pot = f64.LJ()
    pot.setPotParameters(0, 0, pot.InputPairParameters(rc, 1.0, 1.0, False))
    vl = f64.VerletList()
    pf = f64.PairForcesLJ(f64.Box(L), pot, nl=vl)
    integ = f64.VerletNVT("GronbechJensen", 0.0, dt, 1.0, 1234)
    dp, dv = torch.from_numpy(pos.copy()).cuda(), torch.from_numpy(vel.copy()).cuda()
    df = torch.zeros((n, 4), dtype=torch.float64, device="cuda")
    steps = []
    for s in range(1, nsteps + 1):
        before = vl.rebuilds
        integ.forwardTime(dp, dv, df, [pf])
        if vl.rebuilds != before and s > 1:
            steps.append(s)
        elif s == 1 and vl.rebuilds > 1:
            steps.append(1)
    torch.cuda.synchronize()
    print(f"[rebuild schedule] oracle {ref_steps}, product {steps}")
    assert len(ref_steps) >= 2, "the configuration must exercise the drift rebuild"
    assert steps == ref_steps
    assert np.array_equal(dp.cpu().numpy().view(np.uint64), p.view(np.uint64))
    assert vl.getNumberOfStepsSinceLastUpdate() == ref.getNumberOfStepsSinceLastUpdate()


# ---- 5 -------------------------------------------------------------------------------------------------------------------------------
def test_wrapper_logic(hip):
    from uammd_amd import f64
    from uammd_amd._lib import UammdHipError
    n, L, rc = 1000, 12.0, 2.5
    pos = torch.from_numpy(lattice_positions(n, L, seed=2, jitter=0.1, dtype=np.float64)).cuda()
    box = f64.Box(L)
    vl = f64.VerletList()
    assert vl.update(box, rc, pos) and vl.rebuilds == 1 and vl.getNumberOfStepsSinceLastUpdate() == 0
    assert not vl.update(box, rc, pos)                 # nobody moved: the drift check says no rebuild
    assert vl.rebuilds == 1 and vl.getNumberOfStepsSinceLastUpdate() == 1
    moved = pos.clone()
    moved[17, 0] += 0.04 * rc + 1e-3                   # one particle past the threshold (1.08 rc - rc) / 2
    assert vl.update(box, rc, moved) and vl.rebuilds == 2 and vl.getNumberOfStepsSinceLastUpdate() == 0
    moved[17, 0] += 0.04 * rc - 1e-3                   # short of it
    assert not vl.update(box, rc, moved)
    assert vl.update(box, 2.0, moved) and vl.rebuilds == 3                       # new cut-off
    assert vl.update(f64.Box(L + 1.0), 2.0, moved) and vl.rebuilds == 4          # new box
    assert vl.update(f64.Box(L + 1.0, (1, 1, 0)), 2.0, moved) and vl.rebuilds == 5   # new periodicity
    assert vl.update(f64.Box(L + 1.0, (1, 1, 0)), 2.0, moved[:900].contiguous()) and vl.rebuilds == 6   # new N
    assert vl.to_host()["numberParticles"] == 900
    vl.forceNextUpdate()
    assert vl.update(f64.Box(L + 1.0, (1, 1, 0)), 2.0, moved[:900].contiguous()) and vl.rebuilds == 7
    vl.setCutOffMultiplier(1.0)                        # threshold 0 <= 1e-6: every update rebuilds (VerletListBase.cuh:181-183)
    for k in range(3):
        assert vl.update(box, rc, pos)
    assert vl.rebuilds == 10
    with pytest.raises(UammdHipError, match="at least 1"):
        vl.setCutOffMultiplier(0.9)
    with pytest.raises(UammdHipError, match="positive"):
        vl.update(box, 0.0, pos)
    assert vl.update(box, rc, pos) and vl.rebuilds == 11           # the next valid call still works
    empty = torch.zeros((0, 4), dtype=torch.float64, device="cuda")
    assert not vl.update(box, rc, empty)                           # N = 0: a no-op
    assert vl.getVerletList().numberParticles == 0
    f = torch.zeros((n, 4), dtype=torch.float64, device="cuda")
    pot = _pot(f64, rc)
    vl.transverse_lj(pot.device_table(), 1, box, f)
    torch.cuda.synchronize()
    assert not f.any()


def test_nan_position_is_an_error_code(hip):
    from uammd_amd import f64
    from uammd_amd._lib import UammdHipError
    n, L, rc = 700, 16.0, 2.5
    pos = lattice_positions(n, L, seed=3, jitter=0.1, dtype=np.float64)
    bad = pos.copy()
    bad[13, 1] = np.nan
    vl = f64.VerletList()
    with pytest.raises(UammdHipError, match="NaN positions"):
        vl.update(f64.Box(L), rc, torch.from_numpy(bad).cuda())
    assert vl.update(f64.Box(L), rc, torch.from_numpy(pos).cuda())           # a clean build passes
    assert vl.to_host()["numberNeighbours"].min() >= 1


def test_capacity_growth_and_unused_entries(hip, o64):
    """300 particles in one cell push the capacity beyond 96 (to the multiple of 32 above the largest count, as the reference's +32 loop
    ends).  The traversal reads no entry beyond numberNeighbours: the unused part of the list is overwritten with the index of another
    particle of the cluster (a valid row that would change every force) and the forces keep the oracle's bits."""
    from oracle.verletlist import VerletListOracle
    from uammd_amd import f64
    L, rc = 16.0, 2.5
    rng = np.random.default_rng(12)
    bg = lattice_positions(700, L, seed=4, jitter=0.1, dtype=np.float64)
    blob = np.zeros((300, 4))
    g = np.stack(np.meshgrid(np.arange(7), np.arange(7), np.arange(7), indexing="ij"), -1).reshape(-1, 3)[:300]
    blob[:, :3] = 1.9 + 0.3 * g + rng.uniform(-0.02, 0.02, (300, 3))       # spacing 0.3, inside the cell [1.6, 4.8)^3 of the 5^3 grid
    pos = np.concatenate([bg, blob])
    n = len(pos)
    ref = VerletListOracle(o64)
    ref.update(pos, L, [1, 1, 1], rc)
    assert ref.maxNeighboursPerParticle > 96 and list(ref.cl["cellDim"]) == [5, 5, 5]
    box, pot = f64.Box(L), _pot(f64, rc)
    vl = f64.VerletList()
    vl.update(box, rc, torch.from_numpy(pos).cuda())
    h = vl.to_host()
    valid = _compare_lists(h, ref)
    cap = h["maxNeighboursPerParticle"]
    assert cap == ref.maxNeighboursPerParticle and cap % 32 == 0 and cap > h["numberNeighbours"].max() >= cap - 32
    d = vl.getVerletList()
    view = f64.CellList._wrap(d.d_neighbourList, (cap, n), torch.int32)      # the library's own buffer
    inv = np.empty(n, np.int64)
    inv[h["groupIndex"]] = np.arange(n)
    poison = torch.from_numpy(np.where(valid, h["neighbourList"], inv[700 + (np.arange(n) % 300)][None, :]).astype(np.int32)).cuda()
    view.copy_(poison)
    torch.cuda.synchronize()
    f = torch.zeros((n, 4), dtype=torch.float64, device="cuda")
    vl.transverse_lj(pot.device_table(), 1, box, f)
    torch.cuda.synchronize()
    rf = ref.lj_forces(L, [1, 1, 1], pot.table, 1)[0]
    got = f.cpu().numpy()
    err, nbits = _rel_err(got, rf), _words(got[:, :3], rf[:, :3])
    print(f"[capacity {cap}] largest count {h['numberNeighbours'].max()}, max rel err {err:.3e}, words differing {nbits}")
    assert err <= BAR
