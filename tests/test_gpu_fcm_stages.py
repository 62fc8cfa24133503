"""The two ends of the FCM solve (csrc/fcm.hip) on their own through uammd_fcm_probe: the spread node by node in front of the forward
FFT and the gather particle by particle on a grid of the caller's, each against the FLOAT64 oracle's ibm_spread / ibm_gather fed the
same float32 positions, forces and grids cast to double.  tests/test_gpu_ibm_fcm.py lets the spread flow into the FFT and compares
displacements in the L2 norm and the Fourier grid in the max norm, where one dropped tail node, one list entry dropped or doubled at a
chunk boundary, a wrong overflow record or a missing last plane of one gather form stays ten times below the bar.

Yardstick (that of tests/test_gpu_poisson_stages.py).  No tolerance is written down here.  Every check computes its error measure
twice: for the GPU and, inline, for the float32 oracle (the same algorithm in plain C), both against the float64 oracle.  The GPU must
stay within FACTOR = 4 times the float32 oracle's figure plus one float32 ulp of the reference value.  Measures:
    spread   per component, max over nodes of |g - g64| / A, A = the float64 spread of |F|; nodes with A = 0 hold exactly 0.0f; no NaN
             anywhere in [0, nx) x [0, ny) x [0, nz) although the probe fills the grids with NaNs in front of a tile-owned spread (it has
             no memset: it must write every node of every tile); padding columns are not inspected
    unit     one particle with force (1, -2, 3): every stencil node relative to ITS OWN float64 value, tails included; all others exactly 0
    gather   max over particles and components of |v - v64| / B, B = the float64 gather of |grid|, on a white-noise grid
Dense cases assert A > 0 on EVERY node, so no test passes by leaving nodes out.  Boxes have h = 1 (L = cells): cell faces are exact in
float32 and both oracles agree on the cells.  The window is a Gaussian of width max(support) / 6 with the support set on the kernel
struct (no cut-off radius), so supports are chosen; one case each runs Peskin 3pt / 4pt, Barnett-Magland and the six-point window.
`info` of the probe says what ran; the tests assert from it, and the module's last test asserts that the session covered every
instantiation the launch code can choose.

Worst GPU / float32-oracle ratios measured on an MI355X (the bar is 4), per family: A (dense sets, every tile geometry, every window
kind) 1.11, B (one particle at every offset of a tile, faces, outside the box) 1.03, C (list and chunk edges, N = 150 001) 1.00, D (slot
layout, speculative round, overflow records, every preparation) 1.03, E (every gather form) 1.77 — at N = 1, where the float32 oracle happens to land
within 1e-8 of float64; 1.06 from N = 7.  F (the probe leaves the handle as a solve would) has no ratio.  DESIGN.md section 5.7 keeps
these with the wrong builds the tests were tried on, and the two defects found: the tile shift of a 9-node edge at step -2
(test_spread_dense[27x27x27-s16-*]) and the packed gather's grid when four particles per wave are asked for up to two rounds
(test_gather_forms[packed-1-2-per-wave-4], [packed-2-2-per-wave-4])."""
import itertools
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

FACTOR = 4.0
KINDS = {0: "gaussian", 1: "peskin3", 2: "peskin4", 3: "constant", 4: "barnett_magland", 5: "sixpoint"}

WORST = {}                       # family -> worst GPU / float32-oracle ratio of this session (printed by every check)
SEEN = {"spread": set(), "edges": set(), "prepare": set(), "gather": set(), "preparation": set()}   # what ran, from info


# ---- configurations: a grid, a window, both oracles' view of it, handles per option set, references computed once -----------------------
def _tile_of(n, s):   # fcm_tiles_usable: 8 where it divides the axis, then 9, then the shorter edges; >= 3 tiles; support <= 2 (T - 1)
    for t in (8, 9, 7, 6, 5, 4):
        if n % t == 0 and n // t >= 3 and s <= 2 * (t - 1):
            return t
    return 0


class Ctx:
    def __init__(self, hip, o32, o64, cells, support, kind="gaussian"):
        self.hip, self.o = hip, {32: o32, 64: o64}
        self.cells = [int(c) for c in cells]
        self.L = np.asarray(self.cells, np.float32)
        self.nxpad = 2 * (self.cells[0] // 2 + 1)
        K = hip.Kernels
        if kind == "gaussian":
            self.support = tuple(int(s) for s in np.broadcast_to(np.asarray(support), (3,)))
            sigma = max(self.support) / 6.0
            k, _ = K.Gaussian(1.0, 1e-3)
            k.support[:] = self.support
            k.prefactor, k.tau, k.rmax = 1.0 / (math.sqrt(2 * math.pi) * sigma), -0.5 / sigma ** 2, float("inf")
        else:
            k = {"peskin3": lambda: K.Peskin3pt(1.0), "peskin4": lambda: K.Peskin4pt(1.0), "sixpoint": lambda: K.GaussianFlexibleSixPoint(1.0),
                 "barnett_magland": lambda: K.BarnettMagland(3.0, 13.8, 6, lengthUnit=1.0)}[kind]()
            self.support = tuple(int(s) for s in k.support)
        self.kind, self.k = kind, k
        # both oracles get the float32 parameters that the device gets
        self.ok = {b: o.ibm_kernel(KINDS[k.kind], list(k.support), float(k.prefactor), float(k.tau), float(k.rmax), [float(v) for v in k.invh])
                   for b, o in self.o.items()}
        self.tile = tuple(_tile_of(n, s) for n, s in zip(self.cells, self.support))
        self.handles, self.refs = {}, {}

    def handle(self, **options):
        key = tuple(sorted(options.items()))
        if key not in self.handles:
            fcm = self.hip.BDHI.FCM_impl(self.hip.Box(self.L), self.cells, self.k, 1.0, 1234, 1.0)
            for name, value in options.items():
                fcm.set_option(name, value)
            self.handles[key] = fcm
        return self.handles[key]

    def spread_oracle(self, bits, pos, f3):
        g = self.o[bits].ibm_spread(pos, f3, self.L, 1, self.cells, self.ok[bits])
        return g.astype(np.float64)                                     # (nz, ny, nx, 3)

    def gather_oracle(self, bits, pos, grid3):
        return self.o[bits].ibm_gather(pos, grid3, self.L, 1, self.cells, self.ok[bits]).astype(np.float64)

    def origin(self, bits, p3):
        ci, P, _, _, _, _ = self.o[bits].ibm_stencil(np.asarray(p3, np.float32), self.L, 1, self.cells, self.ok[bits])
        return (ci - P) % self.cells

    def place(self, origin, frac):
        """Positions whose stencils start at the nodes `origin` (n, 3), at `frac` (n, 3) inside their cells: the cell is the origin plus
        a shift that, for an even support, depends on the half of the cell the particle sits in."""
        half = self.L.astype(np.float64) / 2
        p3 = np.empty(origin.shape)
        for i, (o, f) in enumerate(zip(origin, frac)):
            _, P, _, _, _, _ = self.o[64].ibm_stencil((f + 1.0 - half).astype(np.float32), self.L, 1, self.cells, self.ok[64])
            p3[i] = (o + P) % self.cells + f - half
        return _p4(p3)

    def spread_ref(self, key, pos, force, dense):
        """(g64, A, e32 per component) of a particle set, computed once per key."""
        if key not in self.refs:
            f3 = force[:, :3]
            g64, A = self.spread_oracle(64, pos, f3), self.spread_oracle(64, pos, np.abs(f3))
            on = A > 0
            assert on.any()
            if dense:   # a condition on the inputs, not a measurement
                assert on.all(), f"{self.cells} support {self.support}: {np.count_nonzero(~on)} nodes outside every stencil"
            d = np.abs(self.spread_oracle(32, pos, f3) - g64)
            e32 = [float((d[..., c][on[..., c]] / A[..., c][on[..., c]]).max()) for c in range(3)]
            self.refs[key] = (g64, A, e32)
        return self.refs[key]

    def gather_ref(self, key, pos, grid3):
        if key not in self.refs:
            g64 = grid3.astype(np.float64)
            v64, B = self.gather_oracle(64, pos, g64), self.gather_oracle(64, pos, np.abs(g64))
            assert np.all(B > 0)
            e32 = float((np.abs(self.gather_oracle(32, pos, grid3) - v64) / B).max())
            self.refs[key] = (v64, B, e32)
        return self.refs[key]

    def spread_gpu(self, fcm, pos, force, kept=False):
        """(grids as (nz, ny, nx, 3), info); the probe's NaN fill is always on."""
        dp = pos if torch.is_tensor(pos) else torch.from_numpy(pos).cuda()
        df = force if torch.is_tensor(force) else torch.from_numpy(force).cuda()
        g, info = fcm.probe(fcm.PROBE_SPREAD, dp, df, nan_fill=True, positions_kept=kept)
        torch.cuda.synchronize()
        SEEN["preparation"].add(info["preparation"])
        if info["tiles"]:
            SEEN["spread"].add((info["W"], info["slots"], info["E"], info["spec"]))
            SEEN["edges"].update(info["tile"])
            assert info["tile"] == self.tile and info["E"] == (9 if max(self.tile) > 8 else 8)
        assert (info["lanes"] > 0) == (info["prepKernel"] is not None)
        if info["lanes"]:
            SEEN["prepare"].add((self.kind, info["prepKernel"], info["lanes"]))
        return g.cpu().numpy().transpose(1, 2, 3, 0)[:, :, :self.cells[0]], info

    def gather_gpu(self, fcm, pos, grid3, packed=False, **kw):
        """grid3: (nz, ny, nx, 3).  Planar: padded to the solver's layout (the padding columns hold 7.0: they are not data)."""
        nx, ny, nz = self.cells
        if packed:
            kw["inter"] = torch.from_numpy(np.ascontiguousarray(grid3)).cuda()
        else:
            g = np.full((3, nz, ny, self.nxpad), 7.0, np.float32)
            g[:, :, :, :nx] = grid3.transpose(3, 0, 1, 2)
            kw["grid"] = torch.from_numpy(g).cuda()
        v, info = fcm.probe(fcm.PROBE_GATHER, torch.from_numpy(pos).cuda(), **kw)
        torch.cuda.synchronize()
        SEEN["gather"].add((info["form"], info["R"], info["P"], info["SZMAX"], info["packed"]))
        assert info["packed"] == packed
        return v.cpu().numpy(), info


_CTX = {}


@pytest.fixture
def ctx(hip, o32, o64):
    def get(cells, support, kind="gaussian"):
        key = (tuple(cells), support, kind)
        if key not in _CTX:
            _CTX[key] = Ctx(hip, o32, o64, cells, support, kind)
        return _CTX[key]
    return get


def _ulp(ref64):
    return np.spacing(np.abs(ref64).astype(np.float32)).astype(np.float64)


def _note(family, what, got, yard):
    ratio = got / yard if yard > 0 else (0.0 if got == 0 else np.inf)
    WORST[family] = max(WORST.get(family, 0.0), ratio)
    print(f"[{family}] {what}: gpu {got:.3e} f32-oracle {yard:.3e} ratio {ratio:.2f} (worst of the family so far {WORST[family]:.2f})")
    return ratio


def _check_spread(family, what, g, ref):
    g64, A, e32 = ref
    assert g.shape == g64.shape and g.dtype == np.float32
    assert not np.isnan(g).any(), f"{what}: {np.count_nonzero(np.isnan(g))} nodes were never written"
    on = A > 0
    assert np.all(g[~on] == 0.0), f"{what}: {np.count_nonzero(g[~on])} nodes outside every stencil are not 0.0f"
    bad = []
    for c in range(3):
        m = on[..., c]
        e = float((np.maximum(np.abs(g[..., c] - g64[..., c]) - _ulp(g64[..., c]), 0.0)[m] / A[..., c][m]).max())
        _note(family, f"{what} component {c}", e, e32[c])
        if not e <= FACTOR * e32[c]:
            bad.append((c, e, e32[c]))
    assert not bad, f"{what}: (component, gpu, f32 oracle) {bad}"


def _check_gather(family, what, v, ref):
    v64, B, e32 = ref
    assert v.shape == v64.shape and np.isfinite(v).all()
    e = float((np.maximum(np.abs(v - v64) - _ulp(v64), 0.0) / B).max())
    _note(family, what, e, e32)
    assert e <= FACTOR * e32, f"{what}: {e:.3e} > {FACTOR} x {e32:.3e}"


def _p4(p3):
    pos = np.zeros((len(p3), 4), np.float32)
    pos[:, :3] = p3
    return pos


def _forces(rng, n):
    f = np.zeros((n, 4), np.float32)
    f[:, :3] = rng.normal(0, 1, (n, 3))
    return f


# ---- A. dense sets on every tile geometry -------------------------------------------------------------------------------------------------
def _dense(c, n=2000, seed=7):
    """A third uniform, a third in clusters on tile corners, a third unwrapped up to +- 1.5 L; particles exactly on -L/2, on L/2 - 1e-3 and
    on cell faces; and a lattice (every cell for the compact windows, every other cell for the Gaussian) that puts every node inside a
    stencil."""
    rng = np.random.default_rng(seed + sum(c.cells) + sum(c.support))
    L = c.L.astype(np.float64)
    t = np.asarray([e or 8 for e in c.tile])
    k = n // 3
    corners = (rng.integers(0, np.asarray(c.cells) // t, (6, 3)) * t).astype(np.float64) - L / 2
    step = 2 if c.kind == "gaussian" else 1
    lattice = np.stack(np.meshgrid(*(np.arange(0, m, step) for m in c.cells), indexing="ij"), -1).reshape(-1, 3) + 0.37 - L / 2
    faces = np.stack([rng.integers(0, m, 12) for m in c.cells], -1) - L / 2 + np.where(rng.random((12, 3)) < 0.5, 0.0, 0.41)
    p3 = np.concatenate([[-L / 2, L / 2 - 1e-3], faces, rng.uniform(-0.5, 0.5, (k, 3)) * L,
                         corners[rng.integers(0, 6, k)] + rng.normal(0, 0.7, (k, 3)), rng.uniform(-1.5, 1.5, (k, 3)) * L, lattice])
    pos = _p4(p3)
    return pos, _forces(rng, len(pos))


DENSE = [((24, 24, 24), 4), ((24, 24, 24), 6), ((24, 24, 24), 9), ((24, 24, 24), 14), ((27, 27, 27), 7), ((27, 27, 27), 16),
         ((24, 27, 28), 9), ((12, 15, 18), (6, 8, 10)), ((20, 24, 28), 8), ((68, 68, 68), 6)]
EDGES = {(24, 24, 24): (8, 8, 8), (27, 27, 27): (9, 9, 9), (24, 27, 28): (8, 9, 7), (12, 15, 18): (4, 5, 6), (20, 24, 28): (5, 8, 7),
         (68, 68, 68): (4, 4, 4)}


def _id(v):
    return "x".join(map(str, v)) if isinstance(v, tuple) else str(v)


@pytest.mark.parametrize("mode", ["w2", "w4", "atomic"])
@pytest.mark.parametrize("cells,support", DENSE, ids=[f"{_id(c)}-s{_id(s)}" for c, s in DENSE])
def test_spread_dense(ctx, cells, support, mode):
    """68^3: 17^3 = 4913 tiles, k_fcm_tile_scan's two rounds of 4096 and its scalar tail.  24^3 at supports >= 10: every tile is a source
    of every tile, at steps 0, -1 and -2 around the box.  12 x 15 x 18: tile edges shorter than the layout (the lx >= td.x rows)."""
    c = ctx(cells, support)
    assert c.tile == EDGES[cells]
    pos, force = _dense(c)
    ref = c.spread_ref("dense", pos, force, dense=True)
    if mode == "atomic":
        g, info = c.spread_gpu(c.handle(atomic_spread=1), pos, force)
        assert not info["tiles"] and info["preparation"] == 0
    else:
        g, info = c.spread_gpu(c.handle(slots=0, spread_waves=int(mode[1])), pos, force)
        assert info["tiles"] and info["W"] == int(mode[1]) and not info["slots"] and not info["spec"] and info["preparation"] == 1
        assert (info["prepKernel"], info["lanes"]) == ("k_fcm_prepare", 4)
    _check_spread("A", f"{cells} support {support} {mode}", g, ref)


@pytest.mark.parametrize("kind", ["peskin3", "peskin4", "barnett_magland", "sixpoint"])
def test_spread_window_kinds(ctx, kind):
    """k_fcm_prepare is instantiated per window kind."""
    c = ctx((24, 24, 24), None, kind)
    pos, force = _dense(c)
    ref = c.spread_ref("dense", pos, force, dense=True)
    for waves in (2, 4):
        g, info = c.spread_gpu(c.handle(slots=0, spread_waves=waves), pos, force)
        assert info["tiles"] and info["W"] == waves
        _check_spread("A", f"{kind} support {c.support} w{waves}", g, ref)
    g, info = c.spread_gpu(c.handle(atomic_spread=1), pos, force)
    _check_spread("A", f"{kind} atomic", g, ref)


# ---- B. one particle: every stencil node against its own float64 value ----------------------------------------------------------------------
def _unit_places(c):
    """name -> position: the stencil origin at every offset 0 .. T - 1 inside a tile, per axis (the stencil then spans one, two or three
    tiles), the box faces, and one and two box lengths outside."""
    L = c.L.astype(np.float64)
    T = max(c.tile)
    places, seen = {}, [set(), set(), set()]
    for k in range(T):
        p = np.asarray([(b + k) % n + 0.3 for b, n in zip((5, 12, 20), c.cells)]) - L / 2
        places[f"offset {k}"] = p
        o = c.origin(64, p)
        for a in range(3):
            seen[a].add(int(o[a]) % c.tile[a])
    assert all(s == set(range(t)) for s, t in zip(seen, c.tile))
    generic = np.asarray([3.3, -7.1, 9.9])
    places.update({"lower face": -L / 2, "below upper face": L / 2 - 1e-3, "one box up": generic + L, "two boxes down": generic - 2 * L,
                   "two boxes up, faces": -L / 2 + 2 * L})
    return {k: np.asarray(v, np.float32) for k, v in places.items()}


UNIT = [((24, 24, 24), 5), ((24, 24, 24), 8), ((24, 24, 24), 13), ((27, 27, 27), 9)]


@pytest.mark.parametrize("cells,support", UNIT, ids=[f"{_id(c)}-s{s}" for c, s in UNIT])
def test_spread_unit_force_places(ctx, cells, support):
    c = ctx(cells, support)
    force = np.zeros((1, 4), np.float32)
    force[0, :3] = (1.0, -2.0, 3.0)
    # (the handle with the slot layout is used again and again with one particle: sorted the first time, slots prepared on the spot after)
    runs = {"w2": c.handle(slots=0, spread_waves=2), "w4": c.handle(slots=0, spread_waves=4), "slots": c.handle(spread_waves=2),
            "atomic": c.handle(atomic_spread=1)}
    for name, p3 in _unit_places(c).items():
        assert np.array_equal(c.origin(32, p3), c.origin(64, p3)), name          # both oracles pick the same stencil
        pos = _p4(p3[None])
        g64, g32 = c.spread_oracle(64, pos, force[:, :3]), c.spread_oracle(32, pos, force[:, :3])
        on = g64 != 0
        assert np.count_nonzero(on) == 3 * support ** 3 and np.array_equal(g32 != 0, on)
        e32 = float((np.abs(g32 - g64)[on] / np.abs(g64[on])).max())
        for run, fcm in runs.items():
            g, info = c.spread_gpu(fcm, pos, force)
            assert info["tiles"] == (run != "atomic")
            assert not np.isnan(g).any(), (name, run)
            assert np.all(g[~on] == 0.0), (name, run)
            e = float((np.maximum(np.abs(g - g64) - _ulp(g64), 0.0)[on] / np.abs(g64[on])).max())
            _note("B", f"{cells} support {support} {name} {run}", e, e32)
            assert e <= FACTOR * e32, (name, run, e, e32)
    assert c.handle(spread_waves=2).last_preparation()[0] == 4    # the reused handle did take the slot layout


# ---- C. list and chunk edges ----------------------------------------------------------------------------------------------------------------
def _one_tile(c, n, tile=(1, 2, 0), seed=3):
    """n particles whose stencil origins all lie in one tile: that tile lists exactly n candidates."""
    rng = np.random.default_rng(seed + n)
    t = np.asarray(c.tile)
    pos = c.place(np.asarray(tile) * t + rng.integers(0, t, (n, 3)), rng.uniform(0.05, 0.95, (n, 3)))
    for p in pos:
        assert tuple(c.origin(32, p[:3]) // t) == tuple(tile)
    return pos, _forces(rng, n)


@pytest.mark.parametrize("waves", [2, 4])
@pytest.mark.parametrize("which", ["1", "2", "3", "cap-1", "cap", "cap+1", "2cap+1"])
def test_spread_list_chunks(ctx, which, waves):
    """One tile's listed population around the list capacity per chunk (capEntries, from info): the chunk boundary must neither drop nor
    double an entry, and the odd tail of a wave's share re-reads an entry with zero force.  Every other tile is empty and still written."""
    c = ctx((24, 24, 24), 4)
    fcm = c.handle(slots=0, spread_waves=waves)
    count = {"1": lambda cap: 1, "2": lambda cap: 2, "3": lambda cap: 3, "cap-1": lambda cap: cap - 1, "cap": lambda cap: cap,
             "cap+1": lambda cap: cap + 1, "2cap+1": lambda cap: 2 * cap + 1}[which]
    cap = 128
    for _ in range(3):   # capEntries depends on N through the LDS budget: settle on the N that meets its own capacity
        n = count(cap)
        pos, force = _one_tile(c, n)
        g, info = c.spread_gpu(fcm, pos, force)
        if info["capEntries"] == cap:
            break
        cap = info["capEntries"]
    assert info["capEntries"] == cap and n == count(cap) and info["W"] == waves
    _check_spread("C", f"one tile lists {which} = {n} (capEntries {cap}) w{waves}", g, c.spread_ref(("one tile", n), pos, force, dense=False))


def test_spread_150001_particles(ctx):
    """Above 150 000 particles k_fcm_prepare runs with one lane per particle; about fifty chunks per tile."""
    c = ctx((24, 24, 24), 4)
    rng = np.random.default_rng(150001)
    n = 150001
    pos = _p4(rng.uniform(-0.5, 0.5, (n, 3)) * c.L)
    force = _forces(rng, n)
    g, info = c.spread_gpu(c.handle(slots=0), pos, force)
    assert info["tiles"] and (info["prepKernel"], info["lanes"]) == ("k_fcm_prepare", 1) and info["W"] == 4
    assert n / 27 * (1 + 3 / 8) ** 3 / info["capEntries"] > 40
    _check_spread("C", "N = 150001", g, c.spread_ref("150001", pos, force, dense=True))


# ---- D. the slot layout -----------------------------------------------------------------------------------------------------------------------
def _slot_set(c, seed=5):
    """A dilute set placed by the tile of the stencil origin: a few particles in most tiles; tiles just below, at and above 8 W = the
    speculative round's slots per tile, 16 with two waves and 32 with four; and clusters beyond the slot capacity (40 on 32^3, 56 on
    27^3) in the first and in the last tile, whose targets lie across the periodic wrap at steps -1 and -2."""
    rng = np.random.default_rng(seed)
    t, nt = np.asarray(c.tile), np.asarray(c.cells) // np.asarray(c.tile)
    pop = {tuple(int(v) for v in tl): int(rng.integers(0, 6)) for tl in itertools.product(*(range(m) for m in nt))}
    last = tuple(int(m) - 1 for m in nt)
    pop.update({(1, 1, 1): 15, (2, 1, 1): 16, (1, 2, 1): 17, (1, 1, 2): 24, (2, 2, 1): 31, (2, 1, 2): 32, (1, 2, 2): 33, (0, 0, 0): 70, last: 75})
    origin = np.concatenate([np.asarray(tl) * t + rng.integers(0, t, (k, 3)) for tl, k in pop.items() if k])
    pos = c.place(origin, rng.uniform(0.05, 0.95, origin.shape))[rng.permutation(len(origin))]
    tiles = [tuple(int(v) for v in c.origin(32, p[:3]) // t) for p in pos]
    assert all(tiles.count(tl) == k for tl, k in pop.items())
    return pos, _forces(rng, len(pos)), pop


SLOT_CASES = [((32, 32, 32), 6, 2, True), ((32, 32, 32), 6, 4, False), ((32, 32, 32), 13, 2, False), ((32, 32, 32), 13, 4, False),
              ((27, 27, 27), 7, 2, True), ((27, 27, 27), 7, 4, False), ((27, 27, 27), 13, 2, False), ((27, 27, 27), 13, 4, False)]


@pytest.mark.parametrize("cells,support,waves,spec", SLOT_CASES, ids=[f"{_id(c)}-s{s}-w{w}" for c, s, w, _ in SLOT_CASES])
def test_spread_slot_layout(ctx, cells, support, waves, spec):
    """k_fcm_step_prep leaves the slot layout behind a step (dt = 0: the positions stay); the probe, told that the positions were kept,
    claims it; a second probe prepares it on the spot from the entry order.  SPEC: two waves and eight source tiles."""
    c = ctx(cells, support)
    pos, force, pop = _slot_set(c)
    n = len(pos)
    fcm = c.handle(spread_waves=waves)
    dp, df = torch.from_numpy(pos).cuda(), torch.from_numpy(force).cuda()
    fcm.stepEulerMaruyama(dp, df, n, 0.0, 0.0, 0.0)
    assert fcm.last_preparation() == (fcm.PREP_SORTED_FRESH, fcm.UPDATE_STEP_PREP)
    torch.cuda.synchronize()
    assert np.array_equal(dp.cpu().numpy(), pos)
    ref = c.spread_ref("slots", pos, force, dense=False)
    for want in (fcm.PREP_SLOTS_CLAIMED, fcm.PREP_SLOTS_SELF):
        g, info = c.spread_gpu(fcm, dp, df, kept=True)
        assert info["preparation"] == want and info["slots"] and info["spec"] == spec and info["W"] == waves
        assert info["slotCap"] == max(32, (3 * n // (len(pop)) + 16 + 7) & ~7) < max(pop.values())          # overflow records exist
        assert (info["prepKernel"], info["lanes"]) == ((None, 0) if want == fcm.PREP_SLOTS_CLAIMED else ("k_fcm_step_prep", 4))
        _check_spread("D", f"{cells} support {support} w{waves} preparation {want} spec {spec}", g, ref)
    fcm = c.handle(slots=0, spread_waves=waves)
    g, info = c.spread_gpu(fcm, pos, force)
    assert not info["slots"] and not info["spec"]
    _check_spread("D", f"{cells} support {support} w{waves} slots = 0", g, ref)
    # without the slot layout the step's update bins for the compact one, and the probe claims that binning
    fcm.stepEulerMaruyama(dp, df, n, 0.0, 0.0, 0.0)
    assert fcm.last_preparation()[1] == fcm.UPDATE_BIN
    g, info = c.spread_gpu(fcm, dp, df, kept=True)
    assert info["preparation"] == fcm.PREP_SORTED_CLAIMED and not info["slots"] and (info["prepKernel"], info["lanes"]) == ("k_fcm_prepare", 4)
    _check_spread("D", f"{cells} support {support} w{waves} slots = 0, binning claimed", g, ref)


# ---- E. the gather forms ----------------------------------------------------------------------------------------------------------------------
COUNTS = [1, 7, 8, 9, 17, 2000]   # groups of 4 P particles end in the middle of a workgroup


def _gather_set(c, n):
    rng = np.random.default_rng(40 + n)
    L = c.L.astype(np.float64)
    p3 = rng.uniform(-0.5, 0.5, (n, 3)) * L
    p3[0] = -L / 2 + 0.25                 # stencils that wrap in every axis
    if n > 2:
        p3[1] = L / 2 - 1e-3
        p3[2] = np.asarray([3.3, -7.1, 9.9]) + L
    return _p4(p3)


def _noise3(c):
    nx, ny, nz = c.cells
    return np.random.default_rng(nx * ny + nz).standard_normal((nz, ny, nx, 3), dtype=np.float32)


# id -> (cells, support, handle options, packed, what info must say: form, R, P, SZMAX)
G24 = (24, 24, 24)
GATHER = {
    "tile-s4": (G24, 4, dict(tile_gather=1), False, ("tile", 0, 0, 0)),
    "tile-s6": (G24, 6, dict(tile_gather=1), False, ("tile", 0, 0, 0)),
    "prep-s5": (G24, 5, dict(interleaved_gather=0), False, ("prep", 0, 0, 0)),
    "prep-s9": (G24, 9, dict(interleaved_gather=0), False, ("prep", 0, 0, 0)),
    "atomic-s6": (G24, 6, dict(atomic_spread=1), False, ("atomic", 0, 0, 0)),
    "atomic-s13": (G24, 13, dict(atomic_spread=1), False, ("atomic", 0, 0, 0)),
    "inter-s9": (G24, 9, {}, False, ("inter", 8, 1, 0)),
    "inter-s13": (G24, 13, {}, False, ("inter", 8, 1, 0)),
    "inter-8-1-noncubic": ((20, 24, 28), 8, dict(gather_per_wave=-2), False, ("inter", 8, 1, 0)),
    "col-2-6-s4": (G24, 4, {}, False, ("col", 0, 2, 6)),
    "col-2-6-s886": (G24, (8, 8, 6), {}, False, ("col", 0, 2, 6)),
    "col-2-8-s8": (G24, 8, {}, False, ("col", 0, 2, 8)),
    "col-2-8-s557": (G24, (5, 5, 7), {}, False, ("col", 0, 2, 8)),
    "col-2-8-noncubic": ((20, 24, 28), 8, {}, False, ("col", 0, 2, 8)),
    "half-6-6": (G24, 6, {}, False, ("half", 6, 2, 6)),
    "half-6-8": (G24, (6, 6, 8), {}, False, ("half", 6, 2, 8)),
    "half-6-8-s667": (G24, (6, 6, 7), {}, False, ("half", 6, 2, 8)),
    "half-7-7": (G24, 7, {}, False, ("half", 7, 2, 7)),
    "half-7-8": (G24, (7, 7, 8), {}, False, ("half", 7, 2, 8)),
    "half-7-7-27": ((27, 27, 27), 7, {}, False, ("half", 7, 2, 7)),
    "packed-1-2": (G24, 4, {}, True, ("inter", 1, 2, 0)),
    "packed-2-2": (G24, 5, {}, True, ("inter", 2, 2, 0)),
    "packed-1-2-per-wave-4": (G24, 4, dict(gather_per_wave=4), True, ("inter", 1, 2, 0)),
    "packed-2-2-per-wave-4": (G24, 5, dict(gather_per_wave=4), True, ("inter", 2, 2, 0)),
    "packed-4-2": (G24, 6, {}, True, ("inter", 4, 2, 0)),
    "packed-4-4": (G24, 6, dict(gather_per_wave=4), True, ("inter", 4, 4, 0)),
    "packed-8-1": (G24, 7, {}, True, ("inter", 8, 1, 0)),
    "packed-8-1-s13": (G24, 13, {}, True, ("inter", 8, 1, 0)),
}
for _s, _r in ((4, 1), (5, 2), (6, 4)):
    for _p in (1, 2, 4):
        GATHER[f"inter-{_r}-{_p}"] = (G24, _s, dict(gather_per_wave=-_p), False, ("inter", _r, _p, 0))
GATHER["inter-8-1"] = (G24, 7, dict(gather_per_wave=-4), False, ("inter", 8, 1, 0))


@pytest.mark.parametrize("case", sorted(GATHER))
def test_gather_forms(ctx, case):
    cells, support, options, packed, want = GATHER[case]
    c = ctx(cells, support)
    fcm = c.handle(slots=0, **options)
    grid3 = _noise3(c)
    for n in COUNTS:
        pos = _gather_set(c, n)
        ref = c.gather_ref(("gather", n), pos, grid3)
        v, info = c.gather_gpu(fcm, pos, grid3, packed=packed)
        assert (info["form"], info["R"], info["P"], info["SZMAX"]) == want and not info["accumulate"]
        _check_gather("E", f"{case} N {n}", v, ref)
        if n in (9, 2000):   # accumulate, this call only: one float32 addition per component onto a non-zero output
            out0 = np.random.default_rng(n).normal(0, 1, (n, 3)).astype(np.float32)
            out, info = c.gather_gpu(fcm, pos, grid3, packed=packed, out=torch.from_numpy(out0.copy()).cuda(), accumulate=True)
            assert info["accumulate"]
            assert np.array_equal(out, out0 + v)
            v2, info = c.gather_gpu(fcm, pos, grid3, packed=packed)
            assert not info["accumulate"] and np.array_equal(v2.view(np.uint32), v.view(np.uint32))


def test_gather_after_slot_layout(ctx):
    """The gather reads the stencils in the entry order that the slot layout keeps (preparation on the spot, no forces)."""
    c = ctx(G24, 6)
    fcm = c.handle()
    grid3 = _noise3(c)
    pos = _gather_set(c, 2000)
    ref = c.gather_ref(("gather", 2000), pos, grid3)
    for want in (fcm.PREP_SORTED_FRESH, fcm.PREP_SLOTS_SELF, fcm.PREP_SLOTS_SELF):
        v, info = c.gather_gpu(fcm, pos, grid3)
        assert info["preparation"] == want
        _check_gather("E", f"default handle, preparation {want}", v, ref)


# ---- F. the probe leaves the handle as a solve would ------------------------------------------------------------------------------------------
def _real_system(hip, n=600, cells=(32, 32, 32)):
    L = np.asarray(cells, np.float32)
    rng = np.random.default_rng(77)
    pos = _p4(rng.uniform(-0.5, 0.5, (n, 3)) * L)
    k, a_eff = hip.Kernels.Gaussian(1.0, 1e-3)
    return L, pos, _forces(rng, n), lambda: hip.BDHI.FCM_impl(hip.Box(L), list(cells), k, 0.9, 5, a_eff)


def _probes(fcm, dp, df, kept):
    nx, ny, nz = fcm.cells
    seed2 = fcm.seed2()
    g, info = fcm.probe(fcm.PROBE_SPREAD, dp, df, nan_fill=True, positions_kept=kept)
    assert info["tiles"] and torch.isfinite(g[..., :nx]).all()
    noise = torch.from_numpy(np.random.default_rng(1).standard_normal((3, nz, ny, 2 * (nx // 2 + 1)), dtype=np.float32)).cuda()
    v, info = fcm.probe(fcm.PROBE_GATHER, dp, grid=noise)
    assert torch.isfinite(v).all() and fcm.seed2() == seed2
    return info


def test_probe_between_solves(hip):
    """solve, probe, solve: the second solve as without the probe, deterministic and thermal (the noise counter is untouched), at the
    rounding bar that test_fcm_gather_particles_per_wave uses for two solves of one handle."""
    L, pos, force, make = _real_system(hip)
    n = len(pos)
    dp, df = torch.from_numpy(pos).cuda(), torch.from_numpy(force).cuda()
    out = {}
    for probed in (False, True):
        fcm = make()
        first = fcm.computeHydrodynamicDisplacements(dp, df, n, 0.7, 2.0).cpu().numpy()
        if probed:
            _probes(fcm, dp, df, False)
        out[probed] = (first, fcm.computeHydrodynamicDisplacements(dp, df, n, 0.0, 0.0).cpu().numpy(),
                       fcm.computeHydrodynamicDisplacements(dp, df, n, 0.7, 2.0).cpu().numpy(), fcm.seed2())
    assert out[False][3] == out[True][3] == 2
    for a, b in zip(out[False][:3], out[True][:3]):
        assert np.isfinite(b).all() and np.abs(a).max() > 0
        assert np.abs(a - b).max() <= 2e-6 * np.abs(a).max()


@pytest.mark.parametrize("kept", [False, True])
def test_probe_between_steps(hip, kept):
    """step, probe, step: velocities and positions as without the probe.  kept: the probe claims what the first step's update prepared,
    and the second step, told the same, finds nothing pending and prepares for itself."""
    L, pos, force, make = _real_system(hip)
    n, dt = len(pos), 0.01
    df = torch.from_numpy(force).cuda()
    out = {}
    for probed in (False, True):
        fcm = make()
        dp = torch.from_numpy(pos.copy()).cuda()
        v = torch.empty((n, 3), dtype=torch.float32, device="cuda")
        fcm.stepEulerMaruyama(dp, df, n, 0.0, 0.0, dt, out=v)
        if probed:
            info = _probes(fcm, dp, df, kept)
            assert info["preparation"] in (fcm.PREP_SLOTS_SELF, fcm.PREP_SORTED_FRESH)
        fcm.stepEulerMaruyama(dp, df, n, 0.0, 0.0, dt, out=v, positions_kept=True)
        fcm.stepEulerMaruyama(dp, df, n, 0.0, 0.0, dt, out=v, positions_kept=True)
        torch.cuda.synchronize()
        out[probed] = (v.cpu().numpy(), dp.cpu().numpy())
    (va, pa), (vb, pb) = out[False], out[True]
    assert np.isfinite(vb).all() and np.abs(va).max() > 0
    assert np.abs(va - vb).max() <= 2e-6 * np.abs(va).max()
    # three steps of |v| dt, each velocity within the bar, plus the rounding of a coordinate of the box
    assert np.abs(pa - pb).max() <= 3 * 2e-6 * np.abs(va).max() * dt + 2 * np.spacing(np.float32(L.max() / 2))


# ---- what ran -----------------------------------------------------------------------------------------------------------------------------------
def test_zz_session_covered_every_instantiation():
    """From the probe's info over the whole module (run it whole): every instantiation that the launch code can choose without an
    environment variable.  SPEC with four waves exists only behind UAMMD_FCM_SPEC_DENSE."""
    spread = {(w, s, e, False) for w in (2, 4) for s in (False, True) for e in (8, 9)} | {(2, True, 8, True), (2, True, 9, True)}
    assert spread <= SEEN["spread"], sorted(spread - SEEN["spread"])
    assert {4, 5, 6, 7, 8, 9} <= SEEN["edges"]
    prepare = {(k, "k_fcm_prepare", 4) for k in ("gaussian", "peskin3", "peskin4", "barnett_magland", "sixpoint")}
    prepare |= {("gaussian", "k_fcm_prepare", 1), ("gaussian", "k_fcm_step_prep", 4)}
    assert prepare <= SEEN["prepare"], sorted(prepare - SEEN["prepare"], key=str)
    assert {0, 1, 2, 3, 4} <= SEEN["preparation"]     # none (atomic) and all four preparations
    gather = {("tile", 0, 0, 0, False), ("prep", 0, 0, 0, False), ("atomic", 0, 0, 0, False), ("inter", 8, 1, 0, False),
              ("col", 0, 2, 6, False), ("col", 0, 2, 8, False), ("half", 6, 2, 6, False), ("half", 6, 2, 8, False), ("half", 7, 2, 7, False),
              ("half", 7, 2, 8, False), ("inter", 1, 2, 0, True), ("inter", 2, 2, 0, True), ("inter", 4, 2, 0, True), ("inter", 4, 4, 0, True),
              ("inter", 8, 1, 0, True)} | {("inter", r, p, 0, False) for r in (1, 2, 4) for p in (1, 2, 4)}
    assert gather <= SEEN["gather"], sorted(gather - SEEN["gather"])
    print("worst GPU / float32-oracle ratio per family:", {k: round(v, 2) for k, v in sorted(WORST.items())})
