"""PSE near field: every product kernel against a float64 sum over all N^2 ordered pairs.

The truth (`near_truth`) is numpy in float64 and shares nothing with the kernels or with the oracle's cell list: no cells, no 27-cell
walk, every ordered pair (i = j included) through the sheared minimum image of RPYNearTransverser::computeShearedDistancePBC (y image
first with x shifted by shear * Ly * s1, then z, then x), `r < rcut` decided in float64, F and G by linear interpolation on the
nPointsTable - 1 equal intervals of the float64 oracle's table.  The table is the float64 oracle's closed form sampled on the float32
cut-off the handle and the float32 oracle use (so that its float32 rounding is their table, bit for bit).

Product paths (all cases run on all five; `uammd_pse_near_last_product` is asserted for every id):
  P1 "exact_order"                                    k_pse_near                 kind 1 (also bit-identical to the float32 oracle)
  P2 "pair_list" 0                                    k_pse_near8                kind 2
  P3 "lazy_list" + "pair_list", skin 0                k_pse_pairs_build<., 0> + k_pse_near_pairs   kind 3
  P4 "lazy_list" + "pair_list", skin 40 %             MODE 1, and MODE 2 after a move of 0.02 skin  kind 3
  P5 "near_kernel" 0                                  k_pse_near_cell            kind 4
through uammd_pse_near_dot (stride 3, overwrites a prefilled buffer) and uammd_pse_near_mdot (stride 4, adds to a prefilled buffer).

Pass rule, no written tolerance: e_gpu = max |gpu - truth| and e_o32 = max |float32 oracle - truth| over all components of the case;
e_gpu <= 4 * e_o32 + ulp32(max |truth|) (mdot: the ulp of prefill + result).  The stochastic product: relative L2 error against
sqrtm(M64) z (eigh of the dense float64 matrix) at most 4 x the float32 oracle's near_stochastic error against the same truth.

The worst e_gpu / bar per family is printed when the module finishes (run with -s).
"""
import ctypes as C
import math

import numpy as np
import pytest

A_H, VISC, TOL, PSI, SEED = 1.0, 1.0, 1e-3, 1.0, 1234
BOX = (12.0, 15.0, 19.0)
# CellList::createUpdateGrid gives a direction that holds three cells or fewer ONE cell.  (12, 15, 19) holds 4 x 5 x 7 cells of rc but only
# 3 x 4 x 5 of rc + skin, so a handle with a skin keeps the plain grid there and no candidate lists (found by these tests: the cases in
# that box assert exactly this); the kept lists themselves are exercised in WIDE, four cells of rc + skin in every direction.
WIDE = (15.0, 17.0, 19.0)
SHEAR = float(np.float32(0.15))
PATHS = {
    "P1": dict(exact_order=1),
    "P2": dict(pair_list=0),
    "P3": dict(lazy_list=1, pair_list=1, list_skin_percent=0),
    "P4": dict(lazy_list=1, pair_list=1, list_skin_percent=40),
    "P5": dict(near_kernel=0),
}
KIND = {"P1": 1, "P2": 2, "P3": 3, "P4": 3, "P5": 4}
SUPERSET = 1.00001   # the scan's test on r^2 (k_pse_near8, k_pse_pairs_build): a pair inside it keeps a record slot


# ---------------------------------------------------------------------------------------------------------------------------------
# the float64 truth
# ---------------------------------------------------------------------------------------------------------------------------------
def _round_half_away(q):
    return np.sign(q) * np.floor(np.abs(q) + 0.5)


def near_truth(pos, box, shear, rcut, table, v=None, dense=True):
    """M_near over all N^2 ordered pairs in float64.  Returns {"Mv": [N, 3] or None, "M": [3N, 3N] or None, "r": [N, N]}."""
    x = np.asarray(pos)[:, :3].astype(np.float64)
    n = len(x)
    Lx, Ly, Lz = (float(b) for b in box)
    rcut, shear = float(rcut), float(shear)
    table = np.asarray(table, np.float64)
    d = x[None, :, :] - x[:, None, :]                 # d[i, j] = x_j - x_i
    dx, dy, dz = d[..., 0].copy(), d[..., 1].copy(), d[..., 2].copy()
    dx += shear * dy
    s1 = _round_half_away(dy / Ly)
    dx -= shear * Ly * s1
    dy -= Ly * s1
    dz -= Lz * _round_half_away(dz / Lz)
    dx -= Lx * _round_half_away(dx / Lx)
    r2 = dx * dx + dy * dy + dz * dz
    r = np.sqrt(r2)
    inside = r < rcut
    nint = len(table) - 1
    u = np.where(inside, r / rcut * nint, 0.0)
    i = np.minimum(np.floor(u).astype(np.int64), nint - 1)
    w = u - i
    F = np.where(inside, table[i, 0] * (1.0 - w) + table[i + 1, 0] * w, 0.0)
    G = np.where(inside, table[i, 1] * (1.0 - w) + table[i + 1, 1] * w, 0.0)
    Cc = np.where(inside & (r2 > 0.0), (G - F) / np.where(r2 > 0.0, r2, 1.0), 0.0)
    rv = np.stack([dx, dy, dz], axis=-1)
    out = {"r": r, "Mv": None, "M": None}
    if dense:
        M4 = np.zeros((n, 3, n, 3))
        for a in range(3):
            for b in range(3):
                M4[:, a, :, b] = Cc * rv[..., a] * rv[..., b]
            M4[:, a, :, a] += F
        out["M"] = M4.reshape(3 * n, 3 * n)
    if v is not None:
        v = np.asarray(v, np.float64)[:, :3]
        rdotv = np.einsum("ijk,jk->ij", rv, v)
        out["Mv"] = F @ v + np.einsum("ij,ijk->ik", Cc * rdotv, rv)
    return out


def ulp32(x):
    return float(np.spacing(np.float32(abs(float(x)))))


class Refs:
    """The two oracles with the handle's parameters; the float64 one re-sampled on the float32 cut-off."""

    def __init__(self, o32, o64):
        self.o32, self.o64 = o32, o64
        self._by = {}

    def get(self, box, shear):
        key = (tuple(float(b) for b in box), float(shear))
        if key not in self._by:
            from oracle.pse import PSEOracle
            from oracle.oracle import _p
            r32 = PSEOracle(self.o32, list(box), A_H, VISC, TOL, PSI, shearStrain=shear, seed_near=SEED)
            r64 = PSEOracle(self.o64, list(box), A_H, VISC, TOL, PSI, shearStrain=shear, seed_near=SEED)
            assert r64.nPointsTable == r32.nPointsTable
            # the float64 oracle's own cut-off is sqrt(-log tol) / psi in double; the product (and the float32 oracle) cut and sample
            # the table at its float32 rounding: the truth has to describe THAT operator
            r64.rcut = np.float64(r32.rcut)
            r64.table = np.zeros((r64.nPointsTable, 2), np.float64)
            self.o64.lib.oracle_pse_near_table(self.o64.creal(A_H), self.o64.creal(PSI), self.o64.creal(VISC), self.o64.creal(r64.rcut),
                                               r64.nPointsTable, _p(r64.table))
            # ... and divide by 6 pi a eta rounded to float32, as NearField.cuh's `real normalization` does in a float32 build
            n64 = 6 * math.pi * A_H * VISC
            r64.table *= n64 / float(np.float32(n64))
            self._by[key] = (r32, r64)
        return self._by[key]


@pytest.fixture(scope="module")
def refs(o32, o64):
    return Refs(o32, o64)


def _rcut32():
    return float(np.float32(math.sqrt(-math.log(TOL)) / PSI))


RC = _rcut32()
NINT = (1 << 14) - 1
SKIN = float(np.float32(0.4) * np.float32(RC))


# ---------------------------------------------------------------------------------------------------------------------------------
# the systems
# ---------------------------------------------------------------------------------------------------------------------------------
def _pos4(x):
    p = np.zeros((len(x), 4), np.float32)
    p[:, :3] = np.asarray(x, np.float64).astype(np.float32)
    return p


def _gas(rng, n, box, frac=0.7):
    L = np.asarray(box, np.float64)
    return rng.uniform(-frac * L, frac * L, (n, 3))


def _case_A():
    """256 isolated pairs on a body-centred tetragonal lattice of (40, 48, 56): nearest sites 7.96 >= 3 rcut apart."""
    box = (40.0, 48.0, 56.0)
    sites = []
    for k in range(10):
        for j in range(6):
            for i in range(5):
                s = np.array([8.0 * i + 4.0 * (k % 2), 8.0 * j + 4.0 * (k % 2), 56.0 * k / 10.0])
                s -= np.array([16.0, 24.0, 28.0])       # coordinates in [-L/2, L/2); multiples of 4 (x, y) include 0, z = 0 at k = 5
                sites.append(s)
    sites = np.array(sites)
    dr = RC / NINT
    crit = [0.0, 1e-6, 0.5 * dr, dr, 2 * dr, (NINT - 1) * dr, 2 * A_H * (1 - 1e-6), 2 * A_H, 2 * A_H * (1 + 1e-6),
            RC * (1 - 2e-6), RC * (1 + 2e-6)]
    used = np.zeros(len(sites), bool)
    pairs = []       # (site, axis, radius)
    for r in crit:   # the sharp radii start from coordinate 0 along their axis: the float32 separation IS float32(r)
        for ax in range(3):
            idx = [s for s in range(len(sites)) if not used[s] and sites[s][ax] == 0.0][0]
            used[idx] = True
            pairs.append((idx, ax, r))
    rest = [s for s in range(len(sites)) if not used[s]]
    nmid = 256 - len(pairs)
    ks = np.unique(np.concatenate([np.arange(0, 8), np.linspace(8, NINT - 1, nmid - 8).astype(np.int64)]))
    assert len(ks) == nmid
    for q, k in enumerate(ks):
        pairs.append((rest[q], q % 3, (k + 0.5) * dr))
    rng = np.random.default_rng(11)
    x = np.zeros((512, 3), np.float32)
    v = np.zeros((512, 3), np.float32)
    info = []
    for q, (s, ax, r) in enumerate(pairs):
        p1 = sites[s].astype(np.float32)
        p2 = p1.copy()
        p2[ax] = np.float32(p1[ax] + np.float32(r))
        x[2 * q], x[2 * q + 1] = p1, p2
        v[2 * q, ax] = rng.normal()                 # along the separation: the partner reads G
        v[2 * q + 1, (ax + 1 + q % 2) % 3] = rng.normal()     # across it: the partner reads F
        info.append((ax, r, float(np.float64(p2[ax]) - np.float64(p1[ax]))))
    # the cut-off pairs lie on their side of rcut by at least 5e-7 relative, in float64 on the float32 coordinates
    for ax, r, sep in info:
        if r == crit[-2]:
            assert sep <= RC * (1 - 5e-7)
        if r == crit[-1]:
            assert RC * (1 + 5e-7) <= sep and sep * sep < RC * RC * (SUPERSET - 1e-6)
    c = sites[[p[0] for p in pairs]]
    dd = c[None] - c[:, None]
    dd -= np.asarray(box) * np.round(dd / np.asarray(box))
    dist = np.sqrt((dd ** 2).sum(-1)) + 1e9 * np.eye(len(c))
    assert dist.min() >= 3 * RC
    return dict(box=box, shear=0.0, pos=_pos4(x), v=v, kept=True, family="A")


def _keeps_lists(box):
    return all(int(np.float32(b) / (np.float32(RC) + np.float32(SKIN))) > 3 for b in box)


def _case_B(shift=False, shear=0.0, box=BOX):
    """Twelve particles: pairs through the x, y and z faces, one edge and one corner at 0.7 rcut, and one pair inside the box."""
    Lx, Ly, Lz = box
    h = np.array([Lx, Ly, Lz]) / 2
    sep = 0.7 * RC

    def pair(anchor, direction, back):
        u = np.asarray(direction, np.float64)
        u = u / np.linalg.norm(u)
        a = np.asarray(anchor, np.float64) - back * sep * u
        b = a + sep * u
        b = b - 2 * h * np.floor((b + h) / (2 * h))      # the partner comes back in through the opposite face
        return [a, b]
    x = []
    x += pair([h[0], -3.0, 5.0], [1.0, 0.2, -0.1], 0.3)          # +x face
    x += pair([2.0, -h[1], -6.0], [0.15, -1.0, 0.1], 0.6)        # -y face (with shear: the image shifts x by shear * Ly)
    x += pair([-3.0, 4.0, h[2]], [-0.1, 0.2, 1.0], 0.5)          # +z face
    x += pair([-h[0], h[1], 1.0], [-1.0, 1.0, 0.1], 0.5)         # the (-x, +y) edge
    x += pair([h[0], h[1], -h[2]], [1.0, 1.0, -1.0], 0.5)        # the (+x, +y, -z) corner
    x += pair([0.5, 0.5, -2.0], [0.3, -0.5, 0.8], 0.5)           # inside
    x = np.array(x)
    if shift:
        x = x + np.array([1.0, -1.0, 2.0]) * 2 * h
    rng = np.random.default_rng(12)
    return dict(box=box, shear=shear, pos=_pos4(x), v=rng.normal(0, 1, (12, 3)).astype(np.float32), kept=shear == 0.0, family="B")


def _case_C(n):
    """A gas at 0.05 per unit volume.  The box is (12, 15, 19) scaled up to hold n at that density; below 171 particles it cannot shrink
    (three cells of rc + skin along x), so the gas fills a part of the +-0.7 L region that keeps the density instead."""
    s = max(1.0, (n / (0.05 * 3420.0)) ** (1.0 / 3.0))
    box = tuple(float(np.float32(b * s)) for b in BOX)
    rng = np.random.default_rng(100 + n)
    frac = 0.7 * min(1.0, (n / 171.0) ** (1.0 / 3.0))
    x = _gas(rng, n, box, frac)
    return dict(box=box, shear=0.0, pos=_pos4(x), v=rng.normal(0, 1, (n, 3)).astype(np.float32), kept=True, family="C")


def _ball(rng, m, radius):
    u = rng.normal(0, 1, (m, 3))
    u /= np.linalg.norm(u, axis=1)[:, None]
    return u * (radius * rng.uniform(0, 1, (m, 1)) ** (1.0 / 3.0))


def _case_D(m, extra=0):
    rng = np.random.default_rng(200 + m + extra)
    x = _ball(rng, m, 0.4 * RC)
    if extra:
        x = np.concatenate([x, _gas(rng, extra, BOX, 0.5)])
    n = len(x)
    return dict(box=BOX, shear=0.0, pos=_pos4(x), v=rng.normal(0, 1, (n, 3)).astype(np.float32), kept=False, family="D", cluster=m)


def _case_E(shear, box=BOX, n=600):
    rng = np.random.default_rng(300)
    x = _gas(rng, n, box)
    return dict(box=box, shear=shear, pos=_pos4(x), v=rng.normal(0, 1, (n, 3)).astype(np.float32), kept=shear == 0.0, family="E")


def _case_G():
    rng = np.random.default_rng(400)
    x = _gas(rng, 300, BOX)
    return dict(box=BOX, shear=0.0, pos=_pos4(x), v=rng.normal(0, 1, (300, 3)).astype(np.float32), kept=True, family="G")


C_SIZES = (1, 7, 31, 32, 33, 127, 129, 255, 257, 480, 481, 513)
D_SIZES = (79, 80, 81, 95, 96, 97, 255, 256, 257, 300, 520)
CASES = {"A-pairs": _case_A, "B-faces": _case_B, "B-shifted": lambda: _case_B(shift=True), "B-shear": lambda: _case_B(shear=SHEAR)}
CASES.update({f"C-{n}": (lambda n=n: _case_C(n)) for n in C_SIZES})
CASES.update({f"D-{m}": (lambda m=m: _case_D(m)) for m in D_SIZES})
CASES["D-300+300"] = lambda: _case_D(300, 300)
CASES.update({"E-gas": lambda: _case_E(0.0), "E-shear": lambda: _case_E(SHEAR)})
# the same in a box where the lists are kept, and in one with a single cell along x (nine neighbour cells instead of 27)
CASES.update({"B-wide": lambda: _case_B(box=WIDE), "E-wide": lambda: _case_E(0.0, WIDE), "E-thin": lambda: _case_E(0.0, (9.0, 15.0, 19.0), 400)})

_BUILT = {}


def _moved(case):
    """every particle 0.02 skin further, in a direction of its own (the move that turns P4's next build into a scan of the kept lists)"""
    rng = np.random.default_rng(5)
    u = rng.normal(0, 1, (len(case["pos"]), 3))
    u /= np.linalg.norm(u, axis=1)[:, None]
    p = case["pos"].copy()
    p[:, :3] = (p[:, :3].astype(np.float64) + 0.02 * SKIN * u).astype(np.float32)
    return p


def _reference(refs, pos, v, f4, prefill, box, shear):
    """truth and float32 oracle for both forms at one set of positions, and the band the record count must lie in"""
    r32, r64 = refs.get(box, shear)
    t = near_truth(pos, r32.L.astype(np.float64), shear, r64.rcut, r64.table, v, dense=False)
    cl = r32._near_list(pos)
    o_dot = np.zeros((len(pos), 3), np.float32)
    r32._near_dot(cl, v, 3, o_dot)
    o_mdot = prefill.copy()
    r32._near_dot(cl, f4, 4, o_mdot)
    r2 = t["r"] ** 2
    rc2 = float(r64.rcut) ** 2
    band = (int(np.count_nonzero(r2 < rc2 * (SUPERSET - 1e-6))), int(np.count_nonzero(r2 < rc2 * (SUPERSET + 1e-6))))
    return dict(pos=pos, truth_dot=t["Mv"], truth_mdot=prefill.astype(np.float64) + t["Mv"], o_dot=o_dot, o_mdot=o_mdot, band=band,
                maxhits=int(np.count_nonzero(r2 < rc2 * SUPERSET, axis=1).max()))


def _built(name, refs):
    if name not in _BUILT:
        case = CASES[name]()
        n = len(case["pos"])
        rng = np.random.default_rng(6)
        f4 = np.full((n, 4), 3.0, np.float32)          # (the fourth component is not the product's business)
        f4[:, :3] = case["v"]
        case["f4"] = f4
        case["prefill"] = rng.normal(0, 1, (n, 3)).astype(np.float32)
        case["at0"] = _reference(refs, case["pos"], case["v"], f4, case["prefill"], case["box"], case["shear"])
        case["at1"] = None
        _BUILT[name] = case
    return _BUILT[name]


def _built_moved(name, refs):
    case = _built(name, refs)
    if case["at1"] is None:
        case["at1"] = _reference(refs, _moved(case), case["v"], case["f4"], case["prefill"], case["box"], case["shear"])
    return case


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU checks of the truth (no GPU)
# ---------------------------------------------------------------------------------------------------------------------------------
def test_truth_tables_agree(refs):
    r32, r64 = refs.get(BOX, 0.0)
    assert float(r32.rcut) == RC and r32.nPointsTable == NINT + 1
    assert np.array_equal(r64.table.astype(np.float32).view(np.uint32), r32.table.view(np.uint32))


@pytest.mark.parametrize("name", ["E-gas", "E-shear"])
def test_truth_equals_float64_oracle(refs, name):
    case = CASES[name]()
    r32, r64 = refs.get(case["box"], case["shear"])
    t = near_truth(case["pos"], r64.L, case["shear"], r64.rcut, r64.table, case["v"], dense=True)
    want = np.zeros((len(case["pos"]), 3), np.float64)
    r64._near_dot(r64._near_list(case["pos"]), case["v"].astype(np.float64), 3, want)
    scale = np.abs(want).max()
    assert np.abs(t["Mv"] - want).max() <= 1e-12 * scale
    assert np.abs(t["M"] @ case["v"].astype(np.float64).reshape(-1) - want.reshape(-1)).max() <= 1e-12 * scale


def test_truth_matrix_symmetric_positive_definite(refs):
    case = _case_G()
    r32, r64 = refs.get(case["box"], 0.0)
    M = near_truth(case["pos"], r64.L, 0.0, r64.rcut, r64.table)["M"]
    assert np.abs(M - M.T).max() <= 1e-13 * np.abs(M).max()
    w = np.linalg.eigvalsh(0.5 * (M + M.T))
    print("G: eigenvalues of M64 in [%.3e, %.3e]" % (w[0], w[-1]))
    assert w[0] > 0.0


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU plumbing
# ---------------------------------------------------------------------------------------------------------------------------------
class Near:
    def __init__(self, lib, box, shear, opts):
        from uammd_amd._lib import check, f3
        self.lib, self.check = lib, check
        self.h = C.c_void_p()
        rc, npts = C.c_float(), C.c_int()
        check(lib.uammd_pse_near_create(f3(box), VISC, A_H, TOL, PSI, shear, SEED, C.byref(self.h), C.byref(rc), C.byref(npts)))
        assert rc.value == RC and npts.value == NINT + 1
        self.opts = dict(opts)
        self.set(**opts)
        assert self.kind() == 0

    def set(self, **opts):
        for k, val in opts.items():
            self.check(self.lib.uammd_pse_near_set_option(self.h, k.encode(), int(val)))

    def reset_lists(self):
        """back to a handle that has kept nothing: the option call clears the kept lists, their row width and their history"""
        if "list_skin_percent" in self.opts:
            self.set(list_skin_percent=self.opts["list_skin_percent"])

    def changed(self):
        self.check(self.lib.uammd_pse_near_positions_changed(self.h))

    def kind(self):
        k = C.c_int(-1)
        self.check(self.lib.uammd_pse_near_last_product(self.h, C.byref(k)))
        return k.value

    def records(self):
        used, cap = C.c_longlong(-1), C.c_longlong(-1)
        self.check(self.lib.uammd_pse_near_pair_records(self.h, C.byref(used), C.byref(cap)))
        return used.value, cap.value

    def stats(self):
        s = (C.c_longlong * 4)()
        self.check(self.lib.uammd_pse_near_list_stats(self.h, s))
        return list(s)

    def dot(self, d_pos, d_v):
        import torch
        from uammd_amd.md import _ptr, current_stream
        n = d_pos.shape[0]
        out = torch.full((n, 3), 7.0, dtype=torch.float32, device="cuda")
        self.check(self.lib.uammd_pse_near_dot(self.h, _ptr(d_pos), _ptr(d_v), n, _ptr(out), current_stream()))
        return out.cpu().numpy()

    def mdot(self, d_pos, d_f4, prefill):
        import torch
        from uammd_amd.md import _ptr, current_stream
        n = d_pos.shape[0]
        out = torch.from_numpy(prefill.copy()).cuda()
        self.check(self.lib.uammd_pse_near_mdot(self.h, _ptr(d_pos), _ptr(d_f4), n, _ptr(out), current_stream()))
        return out.cpu().numpy()

    def destroy(self):
        self.lib.uammd_pse_near_destroy(self.h)


class Env:
    def __init__(self, hip):
        from uammd_amd import _lib
        self.lib = _lib.load()
        self.handles = {}
        self.worst = {}

    def near(self, box, shear, path, tag=None):
        key = (tuple(box), float(shear), path, tag)
        if key not in self.handles:
            self.handles[key] = Near(self.lib, box, shear, PATHS[path] if isinstance(path, str) else dict(path))
        return self.handles[key]

    def judge(self, family, what, got, truth, oracle, scale):
        e_gpu = float(np.abs(got.astype(np.float64) - truth).max())
        e_o32 = float(np.abs(oracle.astype(np.float64) - truth).max())
        bar = 4.0 * e_o32 + ulp32(scale)
        ratio = e_gpu / bar
        if ratio > self.worst.get(family, (0.0, ""))[0]:
            self.worst[family] = (ratio, what)
        print(f"{what}: e_gpu {e_gpu:.3e} e_o32 {e_o32:.3e} bar {bar:.3e} ratio {ratio:.3f}")
        assert e_gpu <= bar, (what, e_gpu, e_o32, bar)


@pytest.fixture(scope="module")
def env(hip):
    e = Env(hip)
    yield e
    print("\nworst e_gpu / bar per family:", {k: (round(r, 3), w) for k, (r, w) in sorted(e.worst.items())})
    for h in e.handles.values():
        h.destroy()


def _both_forms(env, near, case, at, what, family, expect_kind, bitwise=False, d_pos=None):
    import torch
    if d_pos is None:
        d_pos = torch.from_numpy(at["pos"]).cuda()
    else:
        d_pos.copy_(torch.from_numpy(at["pos"]))     # the SAME device array: the handle keeps its lists only for one address
    d_v = torch.from_numpy(case["v"]).cuda()
    d_f4 = torch.from_numpy(case["f4"]).cuda()
    near.changed()
    got = near.dot(d_pos, d_v)
    assert near.kind() == expect_kind, (what, near.kind())
    env.judge(family, what + " dot", got, at["truth_dot"], at["o_dot"], np.abs(at["truth_dot"]).max())
    if bitwise:
        assert np.array_equal(got.view(np.uint32), at["o_dot"].view(np.uint32)), what
    got = near.mdot(d_pos, d_f4, case["prefill"])
    assert near.kind() == expect_kind, (what, near.kind())
    env.judge(family, what + " mdot", got, at["truth_mdot"], at["o_mdot"], np.abs(at["truth_mdot"]).max())
    if bitwise:
        assert np.array_equal(got.view(np.uint32), at["o_mdot"].view(np.uint32)), what
    return d_pos, d_v


def _settle(near, product):
    """A build whose candidate rows overflowed keeps no lists; the next one has wider rows.  Repeats the product at unchanged positions
    until one made its records from kept lists (at most twice wider rows, then this call) and returns whether one did."""
    before = near.stats()[1]
    for _ in range(4):
        product()
        if near.stats()[1] > before:
            return True
    return False


def _check_records(near, at, what, unfit):
    used, cap = near.records()
    if unfit:
        assert used == 0, (what, used)
    else:
        assert at["band"][0] <= used <= at["band"][1] and used <= cap, (what, used, at["band"], cap)


@pytest.mark.gpu
@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("name", list(CASES))
def test_product_paths(env, refs, name, path):
    case = _built(name, refs)
    fam = case["family"]
    at0 = case["at0"]
    # more than 96 hits for one particle: the record paths must hand the handle to k_pse_near8 (a handle of its own: this is for good)
    unfit = path in ("P3", "P4") and at0["maxhits"] > 96
    if fam == "D":
        m = case["cluster"]
        assert at0["maxhits"] >= m and (at0["maxhits"] == m or name == "D-300+300")
    near = env.near(case["box"], case["shear"], path, tag=name if unfit else None)
    near.reset_lists()
    kind = 2 if unfit else KIND[path]
    s0 = near.stats()
    d_pos, d_v = _both_forms(env, near, case, at0, f"{name} {path}", fam, kind, bitwise=path == "P1")
    if path in ("P3", "P4"):
        _check_records(near, at0, f"{name} {path}", unfit)
        if fam == "D" and not unfit:
            assert near.records()[0] == case["cluster"] ** 2
    if path == "P3":
        s = near.stats()
        assert s[3] == 0 and s[1] == s0[1]
    if path == "P4":
        s1 = near.stats()
        assert s1[0] == s0[0] + 1 and s1[1] == s0[1] and s1[2] == s0[2], (s0, s1)      # one build from scratch served both forms
        kept = case["kept"] and not unfit and _keeps_lists(case["box"])
        assert s1[3] == (1 if kept else 0) or fam == "D", (name, s1)
        if kept:
            def again():
                near.changed()
                env.judge(fam, f"{name} {path} again", near.dot(d_pos, d_v), at0["truth_dot"], at0["o_dot"], np.abs(at0["truth_dot"]).max())
                assert near.kind() == kind
            assert _settle(near, again), near.stats()
            s1 = near.stats()
            assert s1[2] == s0[2] and s1[3] == 1, (s0, s1)
        # ... and after a move of 0.02 skin: the records come from the kept candidates (MODE 2) where the lists can be kept
        case = _built_moved(name, refs)
        at1 = case["at1"]
        _both_forms(env, near, case, at1, f"{name} {path} moved", fam, kind, d_pos=d_pos)
        _check_records(near, at1, f"{name} {path} moved", unfit)
        s2 = near.stats()
        if kept:
            assert s2[0] == s1[0] and s2[1] == s1[1] + 1 and s2[2] == s1[2] and s2[3] == 1, (s1, s2)
        elif case["shear"] != 0.0 or not _keeps_lists(case["box"]):
            assert s2[0] == s1[0] + 1 and s2[1] == s1[1] and s2[3] == 0, (s1, s2)


# ---------------------------------------------------------------------------------------------------------------------------------
# F: kept lists at the edge of their claim
# ---------------------------------------------------------------------------------------------------------------------------------
def _f_system(box=WIDE):
    """600 particles that leave the slab 1.5 < z < 9.5 (wrapped) empty, and three pairs along x in the middle of it (z = 5.5,
    y = -5, 0, 5): (start separation, how far EACH particle moves towards the other) in units of the skin beyond rc."""
    rng = np.random.default_rng(500)
    L = np.asarray(box)
    x = np.zeros((0, 3))
    while len(x) < 600:
        g = _gas(rng, 600, box)
        zw = g[:, 2] - L[2] * np.floor(g[:, 2] / L[2] + 0.5)
        x = np.concatenate([x, g[(zw < 1.5) | (zw > 9.5)]])
    x = x[:600]
    pairs = [(0.90, 0.48), (-0.05, -0.10), (0.99, 0.48)]
    start, move = [], []
    for (s, mv), y in zip(pairs, (-5.0, 0.0, 5.0)):
        half = 0.5 * (RC + s * SKIN)
        start += [[-half, y, 5.5], [half, y, 5.5]]
        move += [[mv * SKIN, 0, 0], [-mv * SKIN, 0, 0]]
    return x, np.array(start), np.array(move)


def _f_run(env, refs, near, pos, v, what, kind=3):
    import torch
    r32, r64 = refs.get(near.box, 0.0)
    t = near_truth(pos, r32.L.astype(np.float64), 0.0, r64.rcut, r64.table, v, dense=False)
    o = np.zeros((len(pos), 3), np.float32)
    r32._near_dot(r32._near_list(pos), v, 3, o)
    near.d_pos.copy_(torch.from_numpy(pos))       # the SAME device array: the handle keeps its lists only for one address
    near.changed()
    got = near.dot(near.d_pos, torch.from_numpy(v).cuda())
    assert near.kind() == kind
    env.judge("F", what, got, t["Mv"], o, np.abs(t["Mv"]).max())
    return t


def _f_near(env, box, n, tag):
    import torch
    near = env.near(box, 0.0, "P4", tag=tag)
    near.box = box
    near.d_pos = torch.zeros((n, 4), dtype=torch.float32, device="cuda")
    return near


@pytest.mark.gpu
def test_kept_lists_sharp_pairs_where_no_list_is_kept(env, refs):
    """(i)-(iv) in (12, 15, 19): the grid of rc + skin has one cell along x, the handle keeps the plain grid and builds per step."""
    gas, start, move = _f_system(BOX)
    rng = np.random.default_rng(501)
    n = len(gas) + len(start)
    v = rng.normal(0, 1, (n, 3)).astype(np.float32)
    near = _f_near(env, BOX, n, "F-sharp-12")
    pos = _pos4(np.concatenate([gas, start]))
    _f_run(env, refs, near, pos, v, "F (12, 15, 19) build")
    pos[600:, :3] = (pos[600:, :3].astype(np.float64) + move).astype(np.float32)
    t = _f_run(env, refs, near, pos, v, "F (12, 15, 19) (i)-(iii)")
    assert [bool(t["r"][600 + 2 * q, 601 + 2 * q] < RC) for q in range(3)] == [True, False, False]
    pos[17, 0] = np.float32(pos[17, 0] + np.float32(0.6 * SKIN))
    _f_run(env, refs, near, pos, v, "F (12, 15, 19) (iv)")
    assert near.stats() == [3, 0, 0, 0]


@pytest.mark.gpu
def test_kept_lists_sharp_pairs(env, refs):
    gas, start, move = _f_system()
    rng = np.random.default_rng(501)
    n = len(gas) + len(start)
    v = rng.normal(0, 1, (n, 3)).astype(np.float32)
    near = _f_near(env, WIDE, n, "F-sharp")
    pos0 = _pos4(np.concatenate([gas, start]))
    t0 = _f_run(env, refs, near, pos0, v, "F full build")
    assert near.stats() == [1, 0, 0, 1]
    assert _settle(near, lambda: _f_run(env, refs, near, pos0, v, "F full build again"))
    s0 = near.stats()
    assert s0[2:] == [0, 1]
    r0 = t0["r"]
    for q, inside in enumerate((False, True, False)):        # where the pairs start
        assert (r0[600 + 2 * q, 601 + 2 * q] < RC) == inside
        assert r0[600 + 2 * q, 601 + 2 * q] < RC + SKIN
    # (i)-(iii): the pairs move as written, everybody else 0.02 skin
    u = rng.normal(0, 1, (600, 3))
    u /= np.linalg.norm(u, axis=1)[:, None]
    x1 = np.concatenate([pos0[:600, :3].astype(np.float64) + 0.02 * SKIN * u, pos0[600:, :3].astype(np.float64) + move])
    pos1 = _pos4(x1)
    disp = np.linalg.norm(pos1[:, :3].astype(np.float64) - pos0[:, :3].astype(np.float64), axis=1)
    assert disp.max() < 0.5 * SKIN
    t1 = _f_run(env, refs, near, pos1, v, "F (i)-(iii) candidate scan")
    assert near.stats() == [s0[0], s0[1] + 1, 0, 1]           # the candidate scan (MODE 2), no repeat, no build from scratch
    r1 = t1["r"]
    for q, inside in enumerate((True, False, False)):         # where they end: (i) inside, (ii) and (iii) outside
        assert (r1[600 + 2 * q, 601 + 2 * q] < RC) == inside
    used, _ = near.records()
    band = (np.count_nonzero(r1 ** 2 < RC * RC * (SUPERSET - 1e-6)), np.count_nonzero(r1 ** 2 < RC * RC * (SUPERSET + 1e-6)))
    assert band[0] <= used <= band[1]
    # (iv) one particle 0.6 skin away from where a list was made: the scan of the kept lists is thrown away and repeated from scratch.
    # (From a handle with no history at pos1: after a reading of 0.48 skin the host would not try the kept lists at all.)
    near.reset_lists()
    assert _settle(near, lambda: _f_run(env, refs, near, pos1, v, "F (iv) fresh build"))
    sa = near.stats()
    assert sa[2:] == [0, 1]
    pos2 = pos1.copy()
    pos2[17, 0] = np.float32(pos2[17, 0] + np.float32(0.6 * SKIN))
    _f_run(env, refs, near, pos2, v, "F (iv) bound broken")
    sb = near.stats()
    assert sb[2] == sa[2] + 1 and sb[1] == sa[1] + 1 and sb[0] == sa[0] + 1, (sa, sb)


@pytest.mark.gpu
def test_kept_lists_rows_grow_and_give_up(env, refs):
    """(v) 40 particles within rc + skin of each other in an otherwise thin gas: 40 candidates each against rows of 32."""
    rng = np.random.default_rng(502)
    x = np.concatenate([_ball(rng, 40, 0.5 * (RC + SKIN) * 0.98) + np.array([1.0, 2.0, 3.0]), _gas(rng, 60, WIDE, 0.5)])
    n = len(x)
    v = rng.normal(0, 1, (n, 3)).astype(np.float32)
    near = _f_near(env, WIDE, n, "F-rows")
    pos = _pos4(x)
    _f_run(env, refs, near, pos, v, "F (v) rows of 32 overflow")
    s = near.stats()
    assert s == [1, 0, 0, 1]
    # wider rows (48, then 72): a later build keeps its lists and the call after it scans them

    def step():
        pos[:, :3] += np.float32(0.01 * SKIN)
        _f_run(env, refs, near, pos, v, "F (v) wider rows")
    assert _settle(near, step)
    s = near.stats()
    assert s[0] >= 2 and s[1] == 1 and s[2] == 0 and s[3] == 1, s
    # lists that never survive two steps: the handle gives the mechanism up, the products stay right
    for step in range(12):
        pos[step, 1] = np.float32(pos[step, 1] + np.float32(0.6 * SKIN))
        _f_run(env, refs, near, pos, v, f"F (v) short-lived {step}")
        if near.stats()[3] == 0:
            break
    assert near.stats()[3] == 0
    pos[:, :3] += np.float32(0.01 * SKIN)
    _f_run(env, refs, near, pos, v, "F (v) given up")
    assert near.stats()[3] == 0


@pytest.mark.gpu
def test_kept_lists_box_too_thin_for_skin(env, refs):
    """(vi) (9, 15, 19): three cells of rc along x (which the grid makes ONE cell), two of rc + skin: the plain grid, no kept lists."""
    box = (9.0, 15.0, 19.0)
    assert int(box[0] / RC) == 3 and int(box[0] / (RC + SKIN)) == 2
    rng = np.random.default_rng(503)
    n = 400
    pos = _pos4(_gas(rng, n, box))
    v = rng.normal(0, 1, (n, 3)).astype(np.float32)
    near = _f_near(env, box, n, "F-thin")
    _f_run(env, refs, near, pos, v, "F (vi) thin box")
    assert near.stats() == [1, 0, 0, 0]
    pos[:, :3] += np.float32(0.01 * SKIN)
    _f_run(env, refs, near, pos, v, "F (vi) thin box moved")
    assert near.stats() == [2, 0, 0, 0]


# ---------------------------------------------------------------------------------------------------------------------------------
# G: the stochastic product against a true square root
# ---------------------------------------------------------------------------------------------------------------------------------
_G = {}


def _g_reference(refs):
    if not _G:
        case = _case_G()
        r32, r64 = refs.get(BOX, 0.0)
        M = near_truth(case["pos"], r32.L.astype(np.float64), 0.0, r64.rcut, r64.table)["M"]
        w, Q = np.linalg.eigh(0.5 * (M + M.T))
        assert w[0] > 0
        _G.update(case=case, M=M, sqrtM=(Q * np.sqrt(w)) @ Q.T, r32=r32)
    return _G


G_PATHS = {"default": (dict(lazy_list=1), 5, 6), "P2": (PATHS["P2"], 2, 2), "P5": (PATHS["P5"], 4, 4), "P1": (PATHS["P1"], 1, 1)}


@pytest.mark.gpu
@pytest.mark.parametrize("path", list(G_PATHS))
def test_stochastic_against_true_square_root(env, refs, path):
    import torch
    from uammd_amd.md import _ptr, current_stream
    g = _g_reference(refs)
    case, r32 = g["case"], g["r32"]
    opts, kind, kind_rider = G_PATHS[path]
    n = len(case["pos"])
    T, pref, seed2 = 0.8, 1.1, 555
    near = env.near(BOX, 0.0, tuple(sorted(opts.items())), tag="G-" + path)
    d_pos = torch.from_numpy(case["pos"]).cuda()
    variance = np.float32(pref * math.sqrt(2 * T))           # oracle/pse.py:near_stochastic's arguments
    z = torch.zeros((n, 3), dtype=torch.float32, device="cuda")
    near.check(near.lib.uammd_pse_near_noise(near.h, n, float(variance), seed2, _ptr(z), current_stream()))
    z = z.cpu().numpy().astype(np.float64).reshape(-1)
    truth = (g["sqrtM"] @ z).reshape(n, 3)
    if "o_err" not in g:
        o = r32.near_stochastic(case["pos"], T, pref, seed2)
        g["o_err"] = float(np.linalg.norm(o - truth) / np.linalg.norm(truth))
    bar = 4.0 * g["o_err"]

    def solve(rider):
        out = torch.zeros((n, 3), dtype=torch.float32, device="cuda")
        it = C.c_int(0)
        near.changed()
        MF = None
        if rider:
            MF = torch.from_numpy(g["prefill"]).cuda()
            near.d_f4 = torch.from_numpy(g["f4"]).cuda()
            near.check(near.lib.uammd_pse_near_set_mdot_rider(near.h, _ptr(near.d_f4), _ptr(MF)))
        near.check(near.lib.uammd_pse_near_stochastic(near.h, _ptr(d_pos), n, T, pref, seed2, _ptr(out), current_stream(), C.byref(it)))
        got = out.cpu().numpy()
        err = float(np.linalg.norm(got - truth) / np.linalg.norm(truth))
        ratio = err / bar
        if ratio > env.worst.get("G", (0.0, ""))[0]:
            env.worst["G"] = (ratio, f"G {path} rider={rider}")
        print(f"G {path} rider={rider}: {it.value} iterations, rel L2 error {err:.3e}, float32 oracle {g['o_err']:.3e}, ratio {ratio:.3f}")
        assert 1 <= it.value <= 60
        assert err <= bar, (path, err, g["o_err"])
        return None if MF is None else MF.cpu().numpy()

    solve(False)
    assert near.kind() == kind
    if "f4" not in g:
        rng = np.random.default_rng(401)
        f4 = np.full((n, 4), 3.0, np.float32)
        f4[:, :3] = rng.normal(0, 1, (n, 3))
        g["f4"], g["prefill"] = f4, rng.normal(0, 1, (n, 3)).astype(np.float32)
        g["truth_MF"] = g["prefill"].astype(np.float64) + (g["M"] @ f4[:, :3].astype(np.float64).reshape(-1)).reshape(n, 3)
        o_mf = g["prefill"].copy()
        r32.near_mdot(case["pos"], f4, o_mf)
        g["o_MF"] = o_mf
    MF = solve(True)
    assert near.kind() == kind_rider
    env.judge("G", f"G {path} rider M F", MF, g["truth_MF"], g["o_MF"], np.abs(g["truth_MF"]).max())
