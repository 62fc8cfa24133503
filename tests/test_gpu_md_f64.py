"""GPU parity of the double-precision path A (uammd_amd/csrc/md_f64.hip, uammd_amd/f64.py) against the -DDOUBLE_PRECISION oracle.

The kernels keep the reference's neighbour order and the oracle's FMA placement, so cell tables, sorted rows and (for the cubic and non
cubic periodic fixtures, asserted) forces are expected bit for bit.  The stated bars: per particle |dF_i| <= 1e-5 * 2^-29 (the float
suite's 1e-5 carried to double by the ratio of the unit roundoffs) times the particle's largest force component; 4 x the oracle's own
distance from the all-pairs sum; 1e-11 |E0| for an NVE energy series summed in another order; 2e-6 x the largest kick where the thermostat's
single-precision Gaussians (logf / sincosf differ between libm and the device by a float ulp) enter."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import dpd_ref
from util import canon_cell_tables, lattice_positions

pytestmark = pytest.mark.gpu

BAR = 1e-5 * 2.0 ** -29      # 1.86e-14
ALGOS = {"general": 1, "scan32": 11}
RC = 2.5

# L, periodic, n, unwrapped
FIXTURES = {"L16": (16.0, (1, 1, 1), 3276, True), "noncubic": ((33.0, 22.0, 45.5), (1, 1, 1), 6000, True),
            "zcollapsed": ((30.0, 30.0, 9.0), (1, 1, 1), 6000, False), "nonperiodic-y": (40.0, (1, 0, 1), 6000, False),
            "onecell": (7.0, (1, 1, 1), 274, False)}


def _positions(n, L, periodic=(1, 1, 1), unwrapped=False, seed=1234, ntypes=1, jitter=0.12):
    """util.lattice_positions in float64 plus +-1e-7 of uniform noise (inputs that no float holds); unwrapped: x += Lx on every 7th row,
    z -= 2 Lz on every 11th, as tests/test_gpu_lj.py."""
    pos = lattice_positions(n, L, seed=seed, jitter=jitter, ntypes=ntypes, dtype=np.float64)
    pos[:, :3] += np.random.default_rng(seed + 1).uniform(-1e-7, 1e-7, (n, 3))
    L3 = np.broadcast_to(np.asarray(L, np.float64), (3,))
    for k in range(3):
        if not periodic[k]:
            pos[:, k] = np.clip(pos[:, k], -L3[k] / 2 + 0.01, L3[k] / 2 - 0.01)
    if unwrapped:
        pos[::7, 0] += L3[0]
        pos[::11, 2] -= 2 * L3[2]
    return pos


_cache = {}


def _fixture(o64, name):
    """Inputs and the oracle's answers of one fixture, computed once and shared (never modified)."""
    if name not in _cache:
        L, periodic, n, unwrapped = FIXTURES[name]
        pos = _positions(n, L, periodic, unwrapped)
        cd, oL, oper = o64.celllist_create_grid(L, periodic, RC)
        cl = o64.celllist_build(pos, oL, oper, cd)
        tbl = o64.lj_params(RC, 1.0, 1.0, False).reshape(1, 4)
        fref, _, _ = o64.lj_transverse_celllist(cl, L, periodic, tbl, 1, n)
        fnb = o64.lj_nbody_f64(pos, L, periodic, RC, 1.0, 1.0)
        for a in (pos, fref, fnb):
            a.setflags(write=False)
        _cache[name] = dict(L=L, periodic=periodic, n=n, pos=pos, cl=cl, fref=fref, fnb=fnb, cd=cd)
    return _cache[name]


def _pot(f64, rows):
    pot = f64.LJ()
    for (ti, tj, rc, sigma, eps, shift) in rows:
        pot.setPotParameters(ti, tj, pot.InputPairParameters(rc, sigma, eps, shift))
    return pot


def _gpu_list(f64, pos, L, periodic, rc=RC):
    box = f64.Box(L, periodic)
    cl = f64.CellList()
    d_pos = torch.from_numpy(np.array(pos, dtype=np.float64, order="C")).cuda()      # (a copy: the shared fixtures are read-only)
    cl.update(box, rc, d_pos)
    return cl, box, d_pos


def _transverse(f64, cl, box, pot, n, algo, fev=(True, False, False)):
    f = torch.zeros((n, 4), dtype=torch.float64, device="cuda") if fev[0] else None
    e = torch.zeros(n, dtype=torch.float64, device="cuda") if fev[1] else None
    v = torch.zeros(n, dtype=torch.float64, device="cuda") if fev[2] else None
    cl.transverse_lj(pot.device_table(), pot.ntypes, box, f, e, v, None, algo)
    torch.cuda.synchronize()
    return tuple(None if t is None else t.cpu().numpy() for t in (f, e, v))


def _check_force(got, ref, label):
    fmax = np.abs(ref[:, :3]).max(axis=1) + 1e-300
    err = np.abs(got[:, :3] - ref[:, :3]).max(axis=1) / fmax
    nbits = int((np.ascontiguousarray(got[:, :3]).view(np.uint64) != np.ascontiguousarray(ref[:, :3]).view(np.uint64)).sum())
    print(f"[{label}] max rel err vs f64 oracle {err.max():.3e}; words differing bitwise: {nbits} / {got[:, :3].size}")
    assert err.max() <= BAR
    assert np.all(got[:, 3] == 0)
    return nbits


def _check_tables(got, ref):
    assert np.array_equal(got["index"], ref["index"])
    assert np.array_equal(got["hash"], ref["hash"])
    assert np.array_equal(got["sortPos"].view(np.uint64), ref["sortPos"].view(np.uint64))
    gs, ge = canon_cell_tables(got)
    rs, re_ = canon_cell_tables(ref)
    assert np.array_equal(gs, rs) and np.array_equal(ge, re_)


# ---- gpu_f64_01 --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(FIXTURES))
def test_celllist_vs_oracle(hip, o64, name):
    from uammd_amd import f64
    fx = _fixture(o64, name)
    cl, _, _ = _gpu_list(f64, fx["pos"], fx["L"], fx["periodic"])
    got = cl.to_host()
    assert list(got["cellDim"]) == list(fx["cd"]) and got["validCell"] == fx["n"]
    _check_tables(got, fx["cl"])
    cl.check_errors()


@pytest.mark.parametrize("n", [1, 129])
def test_celllist_small_counts_and_rebuilds(hip, o64, n):
    """N = 1, N = 129 (not a multiple of any block); the second and third build of a list move the epoch as the reference's does."""
    from uammd_amd import f64
    L = 16.0
    pos = _positions(n, L, seed=5 + n)
    cl, box, d_pos = _gpu_list(f64, pos, L, (1, 1, 1))
    cd, oL, oper = o64.celllist_create_grid(L, (1, 1, 1), RC)
    state = np.array([-1, -1], np.int64)
    cs, ce = np.zeros(int(np.prod(cd)), np.uint32), np.zeros(int(np.prod(cd)), np.int32)
    for build in range(3):
        if build:
            pos = _positions(n, L, seed=50 + n + build)
            d_pos.copy_(torch.from_numpy(pos))
            cl.update(box, RC, d_pos)
        valid, clear = o64.next_valid_cell(n, state)
        if clear:
            cs[:] = 0
        ref = o64.celllist_build(pos, oL, oper, cd, valid_cell=valid, cell_start=cs, cell_end=ce)
        got = cl.to_host()
        assert got["validCell"] == valid == n * (build + 1)
        _check_tables(got, ref)
    empty = f64.CellList()
    empty.update(box, RC, torch.zeros((0, 4), dtype=torch.float64, device="cuda"))      # N = 0: a no-op
    assert empty.getCellList().numberParticles == 0


def test_celllist_nan_row(hip, o64):
    """A NaN row: the next get fails with the reference's message; the row is in no cell and the others' tables are those of the list
    built without it.  The same for a particle outside a non-periodic box; check_errors reports at once."""
    from uammd_amd import f64
    from uammd_amd._lib import UammdHipError
    L, n = 16.0, 700
    pos = _positions(n, L, seed=77)
    bad = pos.copy()
    bad[13, 1] = np.nan
    cl, box, d_pos = _gpu_list(f64, bad, L, (1, 1, 1))
    torch.cuda.synchronize()
    with pytest.raises(UammdHipError, match="NaN positions"):
        cl.getCellList()
    got = cl.to_host()                                   # the flag was consumed
    cd, oL, oper = o64.celllist_create_grid(L, (1, 1, 1), RC)
    keep = np.delete(np.arange(n), 13)
    ref = o64.celllist_build(pos[keep], oL, oper, cd)
    assert got["index"][-1] == 13 and np.array_equal(got["index"][:-1], keep[ref["index"]])
    assert np.array_equal(got["sortPos"][:-1].view(np.uint64), ref["sortPos"].view(np.uint64))
    got["validCell"], ref["validCell"] = int(got["validCell"]), int(ref["validCell"])
    gs, ge = canon_cell_tables(got)
    rs, re_ = canon_cell_tables(ref)
    assert got["validCell"] == n and np.array_equal(gs, rs) and np.array_equal(ge, re_)
    # the traversal computes nothing for the row and nobody sees it as a neighbour
    pot = _pot(f64, [(0, 0, RC, 1.0, 1.0, False)])
    f = torch.zeros((n, 4), dtype=torch.float64, device="cuda")
    cl.transverse_lj(pot.device_table(), 1, box, f, None, None, None, 1)
    torch.cuda.synchronize()
    fr, _, _ = o64.lj_transverse_celllist(ref, L, (1, 1, 1), pot.table, 1, n - 1)
    g = f.cpu().numpy()
    assert not g[13].any() and np.array_equal(g[keep, :3], fr[:, :3])
    out = pos.copy()
    out[3, 1] = 25.0
    pbox = f64.Box(40.0, (1, 0, 1))
    cl2 = f64.CellList()
    cl2.update(pbox, RC, torch.from_numpy(out).cuda())
    with pytest.raises(UammdHipError, match="NaN positions or particles outside"):
        cl2.check_errors()
    cl2.update(pbox, RC, torch.from_numpy(pos).cuda())   # a clean build passes
    cl2.check_errors()


# ---- gpu_f64_02 / 03 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", list(ALGOS))
@pytest.mark.parametrize("name", list(FIXTURES))
def test_lj_force_vs_oracle_and_yardstick(hip, o64, name, algo):
    """gpu_f64_02: the per-particle bar against the f64 oracle's cell-list traversal, bit equality asserted for GENERAL on the periodic
    cubic and non-cubic fixtures (printed for the rest).  gpu_f64_03: max|F - all pairs| / max|F| within 4 x the oracle's own."""
    from uammd_amd import f64
    fx = _fixture(o64, name)
    cl, box, _ = _gpu_list(f64, fx["pos"], fx["L"], fx["periodic"])
    pot = _pot(f64, [(0, 0, RC, 1.0, 1.0, False)])
    got, _, _ = _transverse(f64, cl, box, pot, fx["n"], ALGOS[algo])
    nbits = _check_force(got, fx["fref"], f"{algo} {name} cellDim={list(fx['cd'])}")
    if algo == "general" and name in ("L16", "noncubic"):
        assert nbits == 0
    fmax = np.abs(fx["fnb"]).max()
    own = np.abs(fx["fref"][:, :3] - fx["fnb"]).max() / fmax
    mine = np.abs(got[:, :3] - fx["fnb"]).max() / fmax
    print(f"[{algo} {name}] vs all pairs / max|F|: kernel {mine:.3e}, oracle's own {own:.3e}")
    assert own > 0 and mine <= 4 * own
    if algo == "scan32":      # AUTO is SCAN32 where the image covers the grid and GENERAL elsewhere, as a SCAN32 request is: the same launch
        auto, _, _ = _transverse(f64, cl, box, pot, fx["n"], 0)
        assert np.array_equal(auto.view(np.uint64), got.view(np.uint64))
    # accumulated into: a second call doubles the forces, force.w stays 0
    f = torch.from_numpy(got.copy()).cuda()
    cl.transverse_lj(pot.device_table(), 1, box, f, None, None, None, ALGOS[algo])
    assert np.array_equal(f.cpu().numpy(), 2 * got)


@pytest.mark.parametrize("algo", list(ALGOS))
def test_lj_three_types_energy_virial(hip, o64, algo):
    """Three types with the parameter pattern of test_gpu_lj.py::_setup (cut-offs, sigma, epsilon differ, alternating shift), n = 6000."""
    from uammd_amd import f64
    n, L = 6000, 20.0
    pos = _positions(n, L, seed=99, ntypes=3)
    rows = [(ti, tj, RC * (1.0 - 0.05 * ti), 1.0 + 0.03 * tj, 1.0 + 0.1 * ti + 0.2 * tj, (ti + tj) % 2 == 1) for ti in range(3) for tj in range(ti, 3)]
    pot = _pot(f64, rows)
    assert pot.ntypes == 3
    for (ti, tj, rc, sigma, eps, shift) in rows:
        assert np.array_equal(pot.table[ti + 3 * tj], o64.lj_params(rc, sigma, eps, shift))
    cd, oL, oper = o64.celllist_create_grid(L, (1, 1, 1), pot.getCutOff())
    ref_cl = o64.celllist_build(pos, oL, oper, cd)
    rf, re_, rv = o64.lj_transverse_celllist(ref_cl, L, (1, 1, 1), pot.table, 3, n, True, True, True)
    cl, box, _ = _gpu_list(f64, pos, L, (1, 1, 1), pot.getCutOff())
    gf, ge, gv = _transverse(f64, cl, box, pot, n, ALGOS[algo], (True, True, True))
    _check_force(gf, rf, f"{algo} three types")
    print(f"[{algo}] energy err {np.abs(ge - re_).max() / np.abs(re_).max():.3e}, virial err {np.abs(gv - rv).max() / np.abs(rv).max():.3e}")
    assert np.abs(ge - re_).max() <= BAR * np.abs(re_).max()
    assert np.abs(gv - rv).max() <= BAR * np.abs(rv).max()
    # energy alone (force and virial null)
    _, ge2, _ = _transverse(f64, cl, box, pot, n, ALGOS[algo], (False, True, False))
    assert np.array_equal(ge2, ge)


def test_lj_nbody_vs_oracle(hip, o64):
    """The all-pairs kernel at L = 7 (at most 3 cut-offs: what PairForcesLJ chooses there), one and three types, through f64.PairForcesLJ."""
    from uammd_amd import f64
    L, n = 7.0, 274
    for ntypes in (1, 3):
        pos = _positions(n, L, seed=11, ntypes=ntypes)
        rows = [(0, 0, RC, 1.0, 1.0, False)] if ntypes == 1 else [(ti, tj, RC * (1.0 - 0.05 * ti), 1.0 + 0.03 * tj, 1.0 + 0.1 * ti + 0.2 * tj,
                                                                      (ti + tj) % 2 == 1) for ti in range(3) for tj in range(ti, 3)]
        pot = _pot(f64, rows)
        rf, re_, rv = o64.lj_transverse_nbody(pos, L, (1, 1, 1), pot.table, ntypes, True, True, True)
        pf = f64.PairForcesLJ(f64.Box(L), pot)
        f = torch.zeros((n, 4), dtype=torch.float64, device="cuda")
        e = torch.zeros(n, dtype=torch.float64, device="cuda")
        v = torch.zeros(n, dtype=torch.float64, device="cuda")
        pf.sum(torch.from_numpy(pos).cuda(), f, e, v)
        torch.cuda.synchronize()
        assert pf.nl is None                                  # all pairs, no list
        _check_force(f.cpu().numpy(), rf, f"nbody ntypes={ntypes}")
        assert np.abs(e.cpu().numpy() - re_).max() <= BAR * np.abs(re_).max()
        assert np.abs(v.cpu().numpy() - rv).max() <= BAR * np.abs(rv).max()


# ---- gpu_f64_04 --------------------------------------------------------------------------------------------------------------------------
def test_pair_rule_edges(hip, o64):
    """A dimer along x in a periodic box of 6^3 cells at r = rc (nothing), nextafter(rc, 0) (the oracle's force), 2^(1/6) (|F| <= 24 * 2^-50),
    1 (F = -/+ 24 exactly) and 0 (nothing, no NaN): x0 = 0.5 makes (x0 + r) - x0 == r exactly.  The same dimers stored at (+L, -2L, 0): there
    x0 + L + r rounds, so the separation the kernel sees is the stored one and the expectation is the oracle's bits on the stored rows
    (and still nothing at r = 0).  Both kernels give the same bits throughout."""
    from uammd_amd import f64
    L = 15.0
    pot = _pot(f64, [(0, 0, RC, 1.0, 1.0, False)])
    seps = [RC, np.nextafter(RC, 0.0), 2.0 ** (1.0 / 6.0), 1.0, 0.0]
    cd, oL, oper = o64.celllist_create_grid(L, (1, 1, 1), RC)
    assert list(cd) == [6, 6, 6]
    for shift in ((0.0, 0.0, 0.0), (L, -2 * L, 0.0)):
        results = {}
        for algo in ALGOS:
            out = []
            for r in seps:
                pos = np.zeros((2, 4))
                pos[0, :3] = (0.5, 0.25, -0.75)
                pos[1, :3] = (0.5 + r, 0.25, -0.75)
                pos[:, :3] += shift
                cl, box, _ = _gpu_list(f64, pos, L, (1, 1, 1))
                f, _, _ = _transverse(f64, cl, box, pot, 2, ALGOS[algo])
                ref, _, _ = o64.lj_transverse_celllist(o64.celllist_build(pos, oL, oper, cd), L, (1, 1, 1), pot.table, 1, 2)
                assert np.array_equal(f.view(np.uint64), ref.view(np.uint64)), (algo, shift, r)
                out.append(f)
            results[algo] = out
            f_rc, f_in, f_min, f_1, f_0 = out
            assert not f_0.any() and np.isfinite(f_0).all()
            if shift[0] == 0.0:
                assert not f_rc.any()
                assert f_in[0, 0] != 0 and f_in[0, 0] == -f_in[1, 0]
                assert np.abs(f_min).max() <= 24.0 * 2.0 ** -50
                assert f_1[0, 0] == -24.0 and f_1[1, 0] == 24.0 and not f_1[:, 1:].any()
        for a, b in zip(results["general"], results["scan32"]):
            assert np.array_equal(a.view(np.uint64), b.view(np.uint64))


# ---- gpu_f64_05 --------------------------------------------------------------------------------------------------------------------------
def test_scan32_is_a_superset(hip):
    """2000 pairs at rc (1 + k 2^-52), k in -64 ... 64, random directions, one partner within 1e-3 of a cell face or a box face, stored up to
    1.5 L from the origin; plus one cell of 300 particles (queue back-pressure).  SCAN32 == GENERAL bitwise: force, energy, virial."""
    from uammd_amd import f64
    L, ncell = 16.0, 6
    h = L / ncell
    rng = np.random.default_rng(2024)
    npairs = 2000
    a = rng.uniform(-L / 2, L / 2, (npairs, 3))
    face = -L / 2 + h * rng.integers(0, ncell + 1, npairs)            # cell faces, the two box faces among them
    axis = rng.integers(0, 3, npairs)
    a[np.arange(npairs), axis] = face + rng.uniform(-1e-3, 1e-3, npairs)
    d = rng.normal(size=(npairs, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    k = rng.integers(-64, 65, npairs)
    b = a + d * (RC * (1.0 + k * 2.0 ** -52))[:, None]
    a += L * rng.integers(-1, 2, (npairs, 3))                         # stored in a neighbouring image: |x| up to 1.5 L
    b += L * rng.integers(-1, 2, (npairs, 3))
    crowd = np.array([-L / 2 + 2.5 * h] * 3) + rng.uniform(-0.45 * h, 0.45 * h, (300, 3))
    pos = np.zeros((2 * npairs + 300, 4))
    pos[:, :3] = np.concatenate([a, b, crowd])
    n = len(pos)
    pot = _pot(f64, [(0, 0, RC, 1.0, 1.0, True)])
    cl, box, _ = _gpu_list(f64, pos, L, (1, 1, 1))
    out = {algo: _transverse(f64, cl, box, pot, n, ALGOS[algo], (True, True, True)) for algo in ALGOS}
    r2 = ((b - a - L * np.round((b - a) / L)) ** 2).sum(1)
    print(f"pairs inside / at / beyond the cut-off in float64 NumPy: {(r2 < RC * RC).sum()} / {(r2 == RC * RC).sum()} / {(r2 > RC * RC).sum()}")
    assert np.isfinite(out["general"][0]).all() and np.abs(out["general"][0]).max() > 0
    for g, s in zip(out["general"], out["scan32"]):
        assert np.array_equal(g.view(np.uint64), s.view(np.uint64))


# ---- gpu_f64_06 --------------------------------------------------------------------------------------------------------------------------
def test_energy_derivative_is_the_force(hip):
    """What float cannot do: E(1.3 +- 1e-6) of a dimer through d_energy; -(E+ - E-) / 2e-6 equals the computed force to 1e-8 relative
    (truncation ~1e-11, rounding ~1e-10).  The single-precision library misses by more than 1e-2."""
    from uammd_amd import f64
    L, r0, hstep = 15.0, 1.3, 1e-6

    def dimer64(r):
        pos = np.zeros((2, 4))
        pos[1, 0] = r
        pot = _pot(f64, [(0, 0, RC, 1.0, 1.0, False)])
        cl, box, _ = _gpu_list(f64, pos, L, (1, 1, 1))
        f, e, _ = _transverse(f64, cl, box, pot, 2, 1, (True, True, False))
        return float(e.sum()), float(f[1, 0])

    def dimer32(r):
        pos = np.zeros((2, 4), np.float32)
        pos[1, 0] = r
        box = hip.Box(L)
        pot = hip.Potential.LJ()
        pot.setPotParameters(0, 0, pot.InputPairParameters(RC, 1.0, 1.0, False))
        cl = hip.CellList()
        cd, ubox = hip.CellList.create_update_grid(box, RC)
        cl.update_grid(torch.from_numpy(pos).cuda(), ubox, cd)
        f = torch.zeros((2, 4), dtype=torch.float32, device="cuda")
        e = torch.zeros(2, dtype=torch.float32, device="cuda")
        cl.transverse_lj(pot.device_table(), 1, box, f, e, None, None, 1)
        torch.cuda.synchronize()
        return float(e.cpu().numpy().astype(np.float64).sum()), float(f.cpu().numpy()[1, 0])

    errs = {}
    for name, fn in (("f64", dimer64), ("f32", dimer32)):
        ep, _ = fn(r0 + hstep)
        em, _ = fn(r0 - hstep)
        _, force = fn(r0)
        fd = -(ep - em) / (2 * hstep)
        errs[name] = abs(fd - force) / abs(force)
        print(f"[{name}] force {force:.12e}, central difference {fd:.12e}, relative difference {errs[name]:.3e}")
    assert errs["f64"] <= 1e-8
    assert errs["f32"] > 1e-2


# ---- gpu_f64_07 --------------------------------------------------------------------------------------------------------------------------
def _md_state(n, seed=3):
    rng = np.random.default_rng(seed)
    pos = _positions(n, 20.0, seed=seed)
    vel = rng.normal(0, 1, (n, 3))
    force = np.zeros((n, 4))
    force[:, :3] = rng.normal(0, 5, (n, 3))
    mass = rng.uniform(0.5, 2.0, n)
    return pos, vel, force, mass


def _cuda(*arrays):
    return tuple(None if a is None else torch.from_numpy(np.ascontiguousarray(a).copy()).cuda() for a in arrays)


@pytest.mark.parametrize("case", ["masses", "2D", "subgroup"])
@pytest.mark.parametrize("T", [0.0, 1.3])
@pytest.mark.parametrize("kind", ["gj", "basic"])
def test_verletnvt_steps_vs_oracle(hip, o64, kind, T, case):
    """Both half steps of GronbechJensen and Basic: 1000 rows with masses, a 2D case, a subgroup of every third row.  No noise: the bits of
    pos, vel, force; with noise 2e-6 x the largest kick."""
    from uammd_amd._lib import check, load
    lib = load()
    n, dt, friction, seed, stepnum = 1000, 0.005, 1.0, 0xC0FFEE, 17
    noise = math.sqrt(2 * dt * friction * T)
    pos, vel, force, mass = _md_state(n)
    index = np.arange(0, n, 3, dtype=np.int32) if case == "subgroup" else None
    is2D = case == "2D"
    members = n if index is None else len(index)
    rp, rv, rf = pos.copy(), vel.copy(), force.copy()
    dp, dv, df, dm, di = _cuda(pos, vel, force, mass, index)
    ofn = o64.lib.oracle_verletnvt_gj if kind == "gj" else o64.lib.oracle_verletnvt_basic
    gfn = lib.uammd_verletnvt_gj_f64 if kind == "gj" else lib.uammd_verletnvt_basic_f64
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    t = lambda a: None if a is None else C.c_void_p(a.data_ptr())
    for step in (1, 2):
        if step == 2:       # forces of the new configuration
            rf[:, :3] = force[::-1, :3]
            df.copy_(torch.from_numpy(rf))
        ofn(step, p(rp), p(rv), p(rf), p(mass), C.c_double(0.0), p(index), members, C.c_double(dt), C.c_double(friction), int(is2D),
            C.c_double(noise), C.c_uint(stepnum), C.c_uint(seed))
        check(gfn(step, t(dp), t(dv), t(df), t(dm), 0.0, t(di), members, dt, friction, int(is2D), noise, stepnum, seed, None))
        torch.cuda.synchronize()
        gp, gv, gf = dp.cpu().numpy(), dv.cpu().numpy(), df.cpu().numpy()
        assert np.array_equal(gf, rf)
        if T == 0.0:
            assert np.array_equal(gp.view(np.uint64), rp.view(np.uint64)) and np.array_equal(gv.view(np.uint64), rv.view(np.uint64))
        else:
            # the largest kick: b / m x noise amplitude x the largest Gaussian (|g| < 6 over 6000 draws), positions take dt / 2 of it
            kick = 6.0 * noise * max(1.0 / np.sqrt(mass.min()), np.sqrt(0.5 / mass.min()))
            print(f"[{kind} {case} step {step}] |dv| {np.abs(gv - rv).max():.3e}, |dx| {np.abs(gp - rp).max():.3e}, bar {2e-6 * kick:.3e}")
            assert np.abs(gv - rv).max() <= 2e-6 * kick and np.abs(gp - rp).max() <= 2e-6 * kick
        if index is not None:     # rows outside the group are untouched
            rest = np.setdiff1d(np.arange(n), index)
            assert np.array_equal(gp[rest], pos[rest]) and np.array_equal(gv[rest], vel[rest])
        if is2D:
            assert not gv[:, 2].any()


@pytest.mark.parametrize("case", ["masses", "2D", "subgroup", "defaultMass"])
def test_verletnve_steps_vs_float64_numpy(hip, case):
    """uammd_verletnve_f64 against dpd_ref.nve_half: no noise, so the bits of pos and vel always."""
    from uammd_amd._lib import check, load
    lib = load()
    n, dt = 1000, 0.004
    pos, vel, force, mass = _md_state(n, seed=8)
    index = np.arange(0, n, 3, dtype=np.int32) if case == "subgroup" else None
    is2D = case == "2D"
    rows = np.arange(n) if index is None else index
    m = np.full(n, 1.7) if case == "defaultMass" else mass
    dp, dv, df, dm, di = _cuda(pos, vel, force, None if case == "defaultMass" else mass, index)
    t = lambda a: None if a is None else C.c_void_p(a.data_ptr())
    rp, rv = pos.copy(), vel.copy()
    for step in (1, 2):
        rp[rows], rv[rows] = dpd_ref.nve_half(rp[rows], rv[rows], force[rows], m[rows], dt, step, is2D)
        check(lib.uammd_verletnve_f64(step, t(dp), t(dv), t(df), t(dm), 1.7, t(di), len(rows), dt, int(is2D), None))
        torch.cuda.synchronize()
        assert np.array_equal(dp.cpu().numpy().view(np.uint64), rp.view(np.uint64))
        assert np.array_equal(dv.cpu().numpy().view(np.uint64), rv.view(np.uint64))
        assert np.array_equal(df.cpu().numpy(), force)          # read only


def test_initial_velocities_and_kinetic_energy(hip, o64):
    from uammd_amd import f64
    n, T = 5000, 2.0
    vamp = math.sqrt(3 * T)
    for is2D in (False, True):
        ref = o64.verletnvt_initial_velocities(n, vamp, 4242, is2D=is2D)
        v = torch.zeros((n, 3), dtype=torch.float64, device="cuda")
        f64.initVelocities(v, vamp, 4242, is2D=is2D)
        torch.cuda.synchronize()
        g = v.cpu().numpy()
        print(f"[initial velocities 2D={is2D}] max diff {np.abs(g - ref).max():.3e}, bar {2e-6 * 6 * vamp:.3e}")
        assert np.abs(g - ref).max() <= 2e-6 * 6.0 * vamp          # the largest kick: 6 standard deviations
        assert abs(g[:, :2].std() - vamp) < 0.05 * vamp and (not g[:, 2].any()) == is2D
    idx = np.arange(0, n, 3, dtype=np.int32)
    v = torch.full((n, 3), 7.0, dtype=torch.float64, device="cuda")
    f64.initVelocities(v, vamp, 4242, index=torch.from_numpy(idx).cuda())
    g = v.cpu().numpy()
    assert np.abs(g[idx] - o64.verletnvt_initial_velocities(len(idx), vamp, 4242)).max() <= 2e-6 * 6.0 * vamp   # member t draws stream t
    assert (np.delete(g, idx, axis=0) == 7.0).all()
    # kinetic energy: energy[i] += m |v|^2 / 2
    rng = np.random.default_rng(1)
    vel, mass, e0 = rng.normal(0, 1.5, (n, 3)), rng.uniform(0.5, 2.0, n), rng.normal(0, 1, n)
    dv, dm, de = _cuda(vel, mass, e0)
    f64.sumKineticEnergy(dv, de, mass=dm, defaultMass=0.0)
    term = 0.5 * mass * (vel * vel).sum(1)
    assert np.abs(de.cpu().numpy() - (e0 + term)).max() <= BAR * np.abs(term).max() + 2.0 ** -52 * np.abs(e0).max()
    de2 = torch.zeros(n, dtype=torch.float64, device="cuda")
    f64.sumKineticEnergy(dv, de2, mass=dm, defaultMass=3.0)             # defaultMass > 0 wins
    assert np.abs(de2.cpu().numpy() - 1.5 * (vel * vel).sum(1)).max() <= BAR * np.abs(term).max() * 6


# ---- gpu_f64_08 --------------------------------------------------------------------------------------------------------------------------
def test_nve_end_to_end_energy(hip):
    """926 particles, L = 10.5, rc = 2.5 shifted, dt = 0.004, 100 steps through f64.VerletNVE + f64.PairForcesLJ: the total energy after
    every step within 1e-11 |E0| of dpd_ref.nve_run_lj (float64 NumPy, all pairs: sums in another order).  The single-precision classes
    on the same input miss that bar (their own distance is ~3e-7 |E0|)."""
    from uammd_amd import f64
    n, L, dt, steps = 926, 10.5, 0.004, 100
    pos = lattice_positions(n, L, seed=7, jitter=0.05, dtype=np.float64)
    vel = np.random.default_rng(3).normal(0, 1, (n, 3))
    vel -= vel.mean(0)
    ref = dpd_ref.nve_run_lj(pos, vel, L, RC, dt, steps)
    e0 = abs(ref[0])

    pot = _pot(f64, [(0, 0, RC, 1.0, 1.0, True)])
    pf = f64.PairForcesLJ(f64.Box(L), pot)
    integ = f64.VerletNVE(dt)
    dp, dv = _cuda(pos, vel)
    df = torch.zeros((n, 4), dtype=torch.float64, device="cuda")

    def energy64():
        e = torch.zeros(n, dtype=torch.float64, device="cuda")
        pf.sum(dp, None, e, None)
        f64.sumKineticEnergy(dv, e)
        return float(e.sum())

    got = [energy64()]
    for _ in range(steps):
        integ.forwardTime(dp, dv, df, [pf])
        got.append(energy64())
    err64 = np.abs(np.array(got) - ref).max() / e0
    print(f"[f64] max |E - ref| / |E0| over {steps} steps: {err64:.3e} (E0 = {ref[0]:.6f}, drift of the reference {abs(ref[-1] - ref[0]) / e0:.2e})")
    assert pf.nl is not None and err64 <= 1e-11

    pd = hip.ParticleData(n)
    pos32 = np.zeros((n, 4), np.float32)
    pos32[:, :3] = pos[:, :3]
    pd.setPos(pos32)
    pd.getVel("write").copy_(torch.from_numpy(vel.astype(np.float32)))
    pot32 = hip.Potential.LJ()
    pot32.setPotParameters(0, 0, pot32.InputPairParameters(RC, 1.0, 1.0, True))
    pf32 = hip.PairForces(pd, hip.Box(L), pot32)
    nve32 = hip.VerletNVE(pd, dt=dt, initVelocities=False)
    nve32.addInteractor(pf32)

    def energy32():
        pd.getEnergy("write").zero_()
        pf32.sum(force=False, energy=True)
        nve32.sumEnergy()
        return float(pd.getEnergy("read").double().sum())

    got32 = [energy32()]
    for _ in range(steps):
        nve32.forwardTime()
        got32.append(energy32())
    err32 = np.abs(np.array(got32) - ref).max() / e0
    print(f"[f32] max |E - ref| / |E0|: {err32:.3e}")
    assert err32 > 1e-11
