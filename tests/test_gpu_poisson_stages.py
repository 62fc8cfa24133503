"""The triply periodic Poisson solver (csrc/poisson.hip) stage by stage through uammd_poisson_probe: the spread node by node, the
Fourier-space solve grid by grid and the gather particle by particle, each against the FLOAT64 oracle fed the same float32 positions,
charges and grids cast to double (oracle.poisson.PoissonOracle on the f64 library, its ibm_spread / ibm_gather, numpy's float64 FFT
plus oracle_poisson_convolve).  tests/test_gpu_poisson.py compares forces end to end in the max norm, where the convolution and the
gather smear a wrong tail weight, a misplaced row of the LDS tile or a wrong flush below its 2e-5.

Yardstick.  No tolerance is written down here.  Every check computes its error measure twice: for the GPU and, inline, for the float32
oracle (the same algorithm in plain C), both against the float64 oracle.  The GPU must stay within FACTOR = 4 times the float32
oracle's figure — it differs from it by the order of the sums, FMA contraction and the exponential — plus one float32 ulp of the
reference value (so a float32 oracle that happens to round exactly cannot fail a correct kernel).  Measures:
    spread   max over nodes of |g - g64| / A,  A = the float64 spread of |q| (nodes with A = 0 and the padding columns must hold 0.0f)
    unit     one unit charge: every stencil node relative to ITS OWN float64 value, tails included; all other nodes exactly 0
    gather   max over particles and components of |v - v64| / B,  B = the float64 gather of |grid|
    solve    per component, rms = |X - R|_2 / |R|_2 and max = max |X - R| / rms(R)
`info` of the probe says what ran (tile dimensions, waves per workgroup, the compile-time support, the gather's form); the tests assert
the coverage from it and do not assume it.

Worst GPU / float32-oracle ratios measured on an MI355X (the bar is 4), per family: A (every support) 1.03, B (unit charge at crafted
places) 1.01, C (occupancy edges) 1.30, D (non-cubic) 1.00, E (gather) 1.24, F (solve) 1.18, G (thin boxes) 1.02.  In A, C and D the
float32 oracle's own error is that of float32 positions in the Gaussian's tails, which the GPU shares.  DESIGN.md section 5.6 keeps
these with the wrong builds the tests were tried on (which ids fail under which)."""
import itertools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

FACTOR = 4.0
EPS, GW = 1.7, 0.5
SPREAD, CONVOLVE, GATHER = 0, 1, 2

# (L, tolerance, split, upsampling) -> support; found by running the oracle's constructor over L in {16, 20, 22, 24, 33, 40},
# tolerances 3e-1 ... 1e-7, splits {-1, 0.4, 0.7, 1.0} and upsamplings {-1, 2, 2.5, 3}; the test asserts the support the constructor gives.
BY_SUPPORT = {
    3: (22.0, 1e-1, -1.0, -1.0), 4: (24.0, 3e-2, -1.0, -1.0), 5: (22.0, 3e-2, -1.0, 2.0), 6: (22.0, 1e-2, -1.0, 2.0),
    7: (16.0, 1e-3, -1.0, -1.0), 8: (24.0, 3e-4, 1.0, -1.0), 9: (20.0, 1e-4, -1.0, -1.0), 10: (16.0, 1e-4, -1.0, -1.0),
    11: (22.0, 1e-7, -1.0, 2.0), 12: (20.0, 3e-4, -1.0, 3.0), 13: (16.0, 3e-6, -1.0, -1.0), 14: (16.0, 3e-7, 1.0, 2.0),
    15: (22.0, 1e-6, 0.7, -1.0), 16: (22.0, 1e-7, 1.0, 2.0), 17: (16.0, 3e-6, 1.0, 2.5), 18: (22.0, 1e-7, 0.7, -1.0),
    19: (20.0, 3e-5, 1.0, 3.0), 20: (20.0, 1e-5, 1.0, 3.0), 21: (16.0, 3e-6, 1.0, 3.0)}
UNIT = {4: (16.0, 1e-1, -1.0, 2.0), 9: (16.0, 3e-5, -1.0, 2.0), 14: (16.0, 3e-7, 1.0, 2.0)}   # L = 16, 32 cells, h = 0.5
S9 = UNIT[9]                                    # 32^3, tiles of 8^3, three waves per workgroup
MANY_TILES = (22.0, 6.5e-2, -1.0, 4.0)          # 88^3: 1331 tiles, support 9
NONCUBIC = (14.5, 16.3, 19.9)                   # cells (32, 36, 44): tiles (8, 9, 11)
THIN = [((32.0, 32.0, 4.0), 1e-4, -1.0, -1.0), ((32.0, 4.0, 4.0), 1e-5, -1.0, -1.0)]

WORST = {}   # family -> worst GPU / float32-oracle ratio of this session (printed by every check)


# ---- handles, oracles, references: built once per configuration and shared ------------------------------------------------------------
class Ctx:
    def __init__(self, hip, o32, o64, cfg):
        from oracle.poisson import PoissonOracle
        L, tol, split, ups = cfg
        self.cfg, self.L = cfg, L
        par = hip.Poisson.Parameters(box=hip.Box(L), epsilon=EPS, gw=GW, tolerance=tol, split=split, upsampling=ups)
        self.gpu = hip.Poisson(None, par)
        self.o = {32: o32, 64: o64}
        self.po = {32: PoissonOracle(o32, L, EPS, GW, tol, split, ups), 64: PoissonOracle(o64, L, EPS, GW, tol, split, ups)}
        self.cells = [int(c) for c in self.po[64].cells]
        self.support = self.po[64].support
        # the construction heuristics are host code on all three sides: identical
        assert self.gpu.cells == self.cells == [int(c) for c in self.po[32].cells]
        assert self.gpu.support == self.support == self.po[32].support
        self.nxpad = self.po[64].nxpad
        self.refs = {}

    def spread_oracle(self, bits, pos, q):
        po = self.po[bits]
        return self.o[bits].ibm_spread(pos, q, po.L, 1, po.cells, po.kernel, nx_stride=self.nxpad)[..., 0].astype(np.float64)

    def gather_oracle(self, bits, pos, grid4):
        po = self.po[bits]
        return self.o[bits].ibm_gather(pos, grid4, po.L, 1, po.cells, po.kernel, nx_stride=self.nxpad).astype(np.float64)

    def stencil(self, bits, p3):
        po = self.po[bits]
        ci, P, sup, _, _, _ = self.o[bits].ibm_stencil(p3, po.L, 1, po.cells, po.kernel)
        return (ci - P) % po.cells

    def spread_ref(self, key, pos, q):
        """(g64, A, e32) of a particle set, computed once per key."""
        if key not in self.refs:
            g64, A = self.spread_oracle(64, pos, q), self.spread_oracle(64, pos, np.abs(q))
            on = A > 0
            assert on.any() and not on[:, :, self.cells[0]:].any()
            e32 = float((np.abs(self.spread_oracle(32, pos, q) - g64)[on] / A[on]).max())
            self.refs[key] = (g64, A, e32)
        return self.refs[key]

    def spread_gpu(self, pos, q, atomic):
        self.gpu.set_option("atomic_spread", int(atomic))
        try:
            g, info = self.gpu.probe(SPREAD, torch.from_numpy(pos).cuda(), torch.from_numpy(q).cuda())
            torch.cuda.synchronize()
        finally:
            self.gpu.set_option("atomic_spread", 0)
        return g.cpu().numpy(), info

    def gather_gpu(self, pos, q, grid4, **kw):
        v, info = self.gpu.probe(GATHER, torch.from_numpy(pos).cuda(), torch.from_numpy(q).cuda(), grid=grid4, **kw)
        torch.cuda.synchronize()
        return v.cpu().numpy(), info


_CTX = {}


@pytest.fixture
def ctx(hip, o32, o64):
    def get(cfg):
        if cfg not in _CTX:
            _CTX[cfg] = Ctx(hip, o32, o64, cfg)
        return _CTX[cfg]
    return get


def _system(n, L, seed):
    rng = np.random.default_rng(seed)
    pos = np.zeros((n, 4), np.float32)
    pos[:, :3] = rng.uniform(-0.5, 0.5, (n, 3)) * np.asarray(L, np.float64)
    q = rng.normal(0, 1, n).astype(np.float32)
    return pos, q


def _ulp(ref64):
    return np.spacing(np.abs(ref64).astype(np.float32)).astype(np.float64)


def _note(family, what, got, yard):
    ratio = got / yard if yard > 0 else (0.0 if got == 0 else np.inf)
    WORST[family] = max(WORST.get(family, 0.0), ratio)
    print(f"[{family}] {what}: gpu {got:.3e} f32-oracle {yard:.3e} ratio {ratio:.2f} (worst of the family so far {WORST[family]:.2f})")
    return ratio


def _check_spread(family, what, g, ref):
    g64, A, e32 = ref
    on = A > 0
    assert g.shape == g64.shape and g.dtype == np.float32
    assert np.all(g[~on] == 0.0), f"{what}: {np.count_nonzero(g[~on])} nodes outside every stencil (or padding) are not 0.0f"
    e = float((np.maximum(np.abs(g - g64) - _ulp(g64), 0.0)[on] / A[on]).max())
    _note(family, what, e, e32)
    assert e <= FACTOR * e32, f"{what}: {e:.3e} > {FACTOR} x {e32:.3e}"


def _tile_of(n):   # uammd_poisson_create: the divisor of the axis in [4, 12] closest to 8
    best = 0
    for d in range(4, 13):
        if n % d == 0 and (not best or abs(d - 8) < abs(best - 8)):
            best = d
    return best


# ---- A. the spread node by node, every support -----------------------------------------------------------------------------------------
def _spread_case(ctx, cfg, atomic, n=300, seed=11, family="A"):
    c = ctx(cfg)
    pos, q = _system(n, c.L, seed)
    g, info = c.spread_gpu(pos, q, atomic)
    if atomic:
        assert info["waves"] == 0 and info["tile"] == (0, 0, 0)
    _check_spread(family, f"{cfg} support {c.support} {'atomic' if atomic else 'tiles ' + str(info)}", g, c.spread_ref(("sys", n, seed), pos, q))
    return c, info


@pytest.mark.parametrize("atomic", [0, 1], ids=["tiles", "atomic"])
@pytest.mark.parametrize("support", sorted(BY_SUPPORT))
def test_spread_every_support(ctx, support, atomic):
    c, info = _spread_case(ctx, BY_SUPPORT[support], atomic)
    assert c.support == support
    if not atomic and info["waves"]:
        assert info["S"] == (support if 7 <= support <= 12 else 0)
        assert info["tile"] == tuple(_tile_of(n) for n in c.cells)


def test_spread_cases_cover_every_instantiation(ctx):
    """What ran, from the probe's info (one charge per configuration is enough to ask)."""
    S, generic, waves, edges = set(), set(), set(), set()
    for support, cfg in BY_SUPPORT.items():
        c = ctx(cfg)
        pos, q = _system(1, c.L, 3)
        _, info = c.spread_gpu(pos, q, 0)
        waves.add(info["waves"])
        if info["waves"]:
            edges.update(info["tile"])
            (S if info["S"] else generic).add(info["S"] or support)
    assert S == {7, 8, 9, 10, 11, 12}
    assert min(generic) < 7 and max(generic) > 12 and generic >= {3, 4, 5, 6, 13}
    assert waves == {0, 1, 2, 3, 4}            # 0: the halo tile does not fit 64 KB, the atomic spread ran
    assert edges >= {6, 7, 8, 9, 11}


# ---- B. one unit charge at crafted places ----------------------------------------------------------------------------------------------
def _places(c):
    """name -> float32 position; L = 16 and h = 0.5, so cell faces and centres are exact in both precisions."""
    s, h, lo = c.support, 0.5, -8.0

    def at(want, starts, frac=0.3):   # per axis, the first cell from `starts` whose stencil origin satisfies `want`
        p = []
        for a, c0 in enumerate(starts):
            for k in range(32):
                x = np.float32(lo + ((c0 + k) % 32 + frac) * h)
                p3 = np.zeros(3, np.float32)
                p3[a] = x
                if want(int(c.stencil(64, p3)[a])):
                    p.append(x)
                    break
        assert len(p) == 3
        return p
    generic = [np.float32(lo + (cc + 0.3) * h) for cc in (13, 17, 22)]
    places = {"centre": [lo + (cc + 0.5) * h for cc in (13, 17, 22)], "lower corner": [lo] * 3,
              "below upper corner": [np.nextafter(np.float32(8.0), np.float32(0.0))] * 3,
              "tile first": at(lambda o: o % 8 == 0, (5, 12, 20)), "tile last": at(lambda o: o % 8 == 7, (5, 12, 20)),
              "straddle": at(lambda o: o == 32 - s // 2, (0, 0, 0))}
    for a in range(3):
        p = list(generic)
        p[a] = lo + (11 + 3 * a) * h
        places["face " + "xyz"[a]] = p
    return {k: np.asarray(v, np.float32) for k, v in places.items()}


def _unit_restated(c, p3, origin):
    """The float64 spread of one unit charge for a PRESCRIBED stencil origin, in numpy: w(d) = prefactor exp(tau d^2) per axis, d the
    minimum-image distance to the node centre.  Pinned on the float64 oracle at every place where the origins agree."""
    po, s, n, L = c.po[64], c.support, 32, 16.0
    nodes, w = [], []
    for a in range(3):
        k = (int(origin[a]) + np.arange(s)) % n
        d = float(p3[a]) + L / 2 - (k + 0.5) * (L / n)
        d -= L * np.floor(d / L + 0.5)
        nodes.append(k)
        w.append(po.kernel_prefactor * np.exp(po.kernel_tau * d * d))
    g = np.zeros((n, n, c.nxpad))
    g[np.ix_(nodes[2], nodes[1], nodes[0])] = w[2][:, None, None] * w[1][None, :, None] * w[0][None, None, :]
    return g


@pytest.mark.parametrize("support", sorted(UNIT))
def test_spread_unit_charge_places(ctx, support):
    """Both oracles pick the same stencil origin at every place but one: the last float below +L/2 with an odd support.  There
    (x + L/2) / h rounds to 32.0 in float32 — cell 32 = cell 0 — and stays in cell 31 in double, so the float32 stencil sits one node
    further; the reference of that place is the float64 restatement above at the float32 origin."""
    c = ctx(UNIT[support])
    assert c.support == support and c.cells == [32, 32, 32]
    q = np.ones(1, np.float32)
    for name, p3 in _places(c).items():
        o32_, o64_ = c.stencil(32, p3), c.stencil(64, p3)
        pos = np.zeros((1, 4), np.float32)
        pos[0, :3] = p3
        g32 = c.spread_oracle(32, pos, q)
        if name == "below upper corner" and support % 2:
            assert np.array_equal(o32_, (o64_ + 1) % 32)
            g64 = _unit_restated(c, p3, o32_)
        else:
            assert np.array_equal(o32_, o64_), (name, o32_, o64_)      # both oracles pick the same stencil
            g64 = c.spread_oracle(64, pos, q)
            assert np.allclose(_unit_restated(c, p3, o64_), g64, rtol=1e-12, atol=0.0)
        if name == "tile first":
            assert np.all(o32_ % 8 == 0)
        if name == "tile last":
            assert np.all(o32_ % 8 == 7)
        if name == "straddle":
            assert np.all(o32_ + support > 32)
        on = g64 != 0
        assert np.count_nonzero(on) == support ** 3 and np.array_equal(g32 != 0, on)
        e32 = float((np.abs(g32 - g64)[on] / np.abs(g64[on])).max())
        for atomic in (0, 1):
            g, info = c.spread_gpu(pos, q, atomic)
            assert (info["waves"] == 0) == bool(atomic)
            assert np.all(g[~on] == 0.0), (name, atomic)
            e = float((np.maximum(np.abs(g - g64) - _ulp(g64), 0.0)[on] / np.abs(g64[on])).max())
            _note("B", f"support {support} {name} {'atomic' if atomic else 'tiles'}", e, e32)
            assert e <= FACTOR * e32, (name, atomic, e, e32)


# ---- C. occupancy edges of the binning and of the batch loop, support 9 ----------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_spread_particle_counts(ctx, n):
    c, info = _spread_case(ctx, S9, 0, n=n, seed=5, family="C")
    assert c.support == 9 and info["S"] == 9 and info["waves"] == 3
    _spread_case(ctx, S9, 1, n=n, seed=5, family="C")


def _one_tile(c, n):   # stencil origins in tile (1, 2, 0): cells [o, o + 8) + P, P = 4
    rng = np.random.default_rng(8)
    pos = np.zeros((n, 4), np.float32)
    cell = np.array([8, 16, 0]) + 4 + rng.integers(0, 8, (n, 3))
    pos[:, :3] = -8.0 + (cell + rng.uniform(0.05, 0.95, (n, 3))) * 0.5
    return pos, rng.normal(0, 1, n).astype(np.float32)


def _coincident(c, n):
    pos, q = _system(n, c.L, 4)
    pos[:] = pos[0]
    return pos, q


def _one_per_tile(c, n=None):
    rng = np.random.default_rng(9)
    t = np.array(list(itertools.product(range(4), repeat=3)))
    pos = np.zeros((len(t), 4), np.float32)
    pos[:, :3] = -8.0 + ((t * 8 + 4 + rng.integers(0, 8, t.shape)) % 32 + rng.uniform(0.05, 0.95, t.shape)) * 0.5
    tiles = sorted(tuple(int(v) for v in c.stencil(32, p[:3]) // 8) for p in pos)
    assert tiles == sorted(map(tuple, t.tolist()))          # exactly one origin in each of the 64 tiles
    return pos, rng.normal(0, 1, len(t)).astype(np.float32)


@pytest.mark.parametrize("name,make", [("one tile", _one_tile), ("coincident", _coincident), ("one per tile", _one_per_tile)])
def test_spread_occupancy(ctx, name, make):
    c = ctx(S9)
    pos, q = make(c, 300)
    if name == "one tile":
        assert {tuple(int(v) for v in c.stencil(32, p[:3]) // 8) for p in pos} == {(1, 2, 0)}
    ref = c.spread_ref((name,), pos, q)
    for atomic in (0, 1):
        g, info = c.spread_gpu(pos, q, atomic)
        assert info["waves"] == (0 if atomic else 3)
        _check_spread("C", f"{name} {'atomic' if atomic else 'tiles'}", g, ref)


def test_spread_more_than_1024_tiles(ctx):
    c, info = _spread_case(ctx, MANY_TILES, 0, family="C")
    assert c.support == 9 and c.cells == [88, 88, 88] and info["tile"] == (8, 8, 8) and info["S"] == 9   # 11^3 = 1331 tiles: two scan rounds


# ---- D. non-cubic ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", list(itertools.permutations(NONCUBIC)), ids=lambda L: "x".join(str(v) for v in L))
def test_spread_noncubic(ctx, L):
    cfg = (L, 1e-4, -1.0, -1.0)
    c, info = _spread_case(ctx, cfg, 0, family="D")
    want = {14.5: 32, 16.3: 36, 19.9: 44}
    assert c.cells == [want[v] for v in L] and c.support == 9
    assert info["tile"] == tuple({32: 8, 36: 9, 44: 11}[n] for n in c.cells) and info["S"] == 9 and info["waves"] >= 1
    _spread_case(ctx, cfg, 1, family="D")


# ---- E. gather -------------------------------------------------------------------------------------------------------------------------
def _noise4(c, seed=21):
    nx, ny, nz = c.cells
    return np.random.default_rng(seed).standard_normal((nz, ny, c.nxpad, 4), dtype=np.float32)


def _gather_ref(c, key, pos, grid4):
    if key not in c.refs:
        g64 = grid4.astype(np.float64)
        v64, B = c.gather_oracle(64, pos, g64), c.gather_oracle(64, pos, np.abs(g64))
        e32 = float((np.abs(c.gather_oracle(32, pos, grid4) - v64) / B).max())
        c.refs[key] = (v64, B, e32)
    return c.refs[key]


def _check_gather(what, v, ref, family="E"):
    v64, B, e32 = ref
    e = float((np.maximum(np.abs(v - v64) - _ulp(v64), 0.0) / B).max())
    _note(family, what, e, e32)
    assert e <= FACTOR * e32, f"{what}: {e:.3e} > {FACTOR} x {e32:.3e}"


FORM = {5: "col1", 8: "col1", 9: "col2", 11: "col2", 12: "flat", 19: "flat"}


@pytest.mark.parametrize("n", [1, 3, 5, 257])
@pytest.mark.parametrize("support", sorted(FORM))
def test_gather_matches_float64(ctx, support, n):
    c = ctx(BY_SUPPORT[support])
    pos, q = _system(n, c.L, 30 + n)
    grid4 = _noise4(c)
    v, info = c.gather_gpu(pos, q, torch.from_numpy(grid4).cuda())
    assert c.support == support and info["gather"] == FORM[support]
    _check_gather(f"support {support} N {n} {info['gather']}", v, _gather_ref(c, ("gather", n), pos, grid4))


@pytest.mark.parametrize("support", [5, 9])
def test_gather_flat_form_forced(ctx, monkeypatch, support):
    c = ctx(BY_SUPPORT[support])
    pos, q = _system(257, c.L, 30 + 257)
    grid4 = _noise4(c)
    dgrid = torch.from_numpy(grid4).cuda()
    ref = _gather_ref(c, ("gather", 257), pos, grid4)
    vcol, info = c.gather_gpu(pos, q, dgrid)
    assert info["gather"] == FORM[support]
    monkeypatch.setenv("UAMMD_POISSON_FLAT_GATHER", "1")
    vflat, info = c.gather_gpu(pos, q, dgrid)
    assert info["gather"] == "flat"
    _check_gather(f"support {support} forced flat", vflat, ref)
    # the two forms against each other, under the same bound
    v64, B, e32 = ref
    assert np.all(np.abs(vflat.astype(np.float64) - vcol) <= FACTOR * e32 * B + _ulp(v64))


@pytest.mark.parametrize("support", [8, 11, 19])
def test_gather_invariants(ctx, support):
    """No tolerance: a particle's result does not depend on the others, nor on the call; outputs are ADDED through the group index."""
    c = ctx(BY_SUPPORT[support])
    n = 257
    pos, q = _system(n, c.L, 30 + n)
    dgrid = torch.from_numpy(_noise4(c)).cuda()
    v, _ = c.gather_gpu(pos, q, dgrid)
    v2, _ = c.gather_gpu(pos, q, dgrid)
    assert np.array_equal(v.view(np.uint32), v2.view(np.uint32))
    for i in (0, 100, 256):
        alone, _ = c.gather_gpu(pos[i:i + 1], q[i:i + 1], dgrid)
        assert np.array_equal(alone[0].view(np.uint32), v[i].view(np.uint32)), i
    # shuffled order: the results follow the particles
    perm = np.random.default_rng(1).permutation(n)
    vs, _ = c.gather_gpu(pos[perm], q[perm], dgrid)
    assert np.array_equal(vs.view(np.uint32), v[perm].view(np.uint32))
    # accumulation onto non-zero arrays: one float32 addition per component, of q times the gathered value for force and energy
    rng = np.random.default_rng(2)
    fp0, f0 = rng.normal(0, 1, (n, 4)).astype(np.float32), rng.normal(0, 1, (n, 4)).astype(np.float32)
    e0 = rng.normal(0, 1, n).astype(np.float32)
    fp, f, e = (torch.from_numpy(a.copy()).cuda() for a in (fp0, f0, e0))
    c.gather_gpu(pos, q, dgrid, fieldPotential=fp, force=f, energy=e)
    fp, f, e = fp.cpu().numpy(), f.cpu().numpy(), e.cpu().numpy()
    assert np.array_equal(fp, fp0 + v)
    assert np.array_equal(f[:, :3], f0[:, :3] + q[:, None] * v[:, :3])
    assert np.array_equal(f[:, 3].view(np.uint32), f0[:, 3].view(np.uint32))        # force.w unchanged
    assert np.array_equal(e, e0 + q * v[:, 3])


# ---- F. the Fourier-space solve --------------------------------------------------------------------------------------------------------
def _solve_oracle(po, gq, bits):
    """rfftn -> oracle_poisson_convolve -> 4 x irfftn (unnormalised, as the device transforms), in the oracle's precision."""
    from oracle.oracle import _p
    nx, ny, nz = (int(v) for v in po.cells)
    if bits == 64:
        fwd, inv, kw = np.fft.rfftn, np.fft.irfftn, {}
    else:
        from oracle.fcm import _fft, _kw
        fwd, inv, kw = _fft.rfftn, _fft.irfftn, _kw
    gk = np.ascontiguousarray(fwd(gq.astype(po.real), axes=(0, 1, 2), **kw).astype(po.cplx))
    out = np.zeros(gk.shape + (4,), po.cplx)
    po.o.lib.oracle_poisson_convolve(_p(gk), _p(out), _p(po.L), _p(po.cells), po.o.creal(po.epsilon))
    return np.stack([inv(out[..., k], s=(nz, ny, nx), axes=(0, 1, 2), **kw) * (nx * ny * nz) for k in range(4)], -1).astype(np.float64)


def _solve_gpu(c, gq, pad=0.0):
    nx, ny, nz = c.cells
    g = np.full((nz, ny, c.nxpad), pad, np.float32)
    g[:, :, :nx] = gq
    out, info = c.gpu.probe(CONVOLVE, grid=torch.from_numpy(g).cuda())
    torch.cuda.synchronize()
    assert info["gather"] is None and info["waves"] == -1
    return out.cpu().numpy()[:, :, :nx]


@pytest.mark.parametrize("cfg", [UNIT[9], (NONCUBIC, 1e-4, -1.0, -1.0)], ids=["32x32x32", "32x36x44"])
def test_solve_white_noise(ctx, cfg):
    c = ctx(cfg)
    nx, ny, nz = c.cells
    assert nx % 2 == 0 and ny % 2 == 0 and nz % 2 == 0
    gq = np.random.default_rng(nx * ny + nz).standard_normal((nz, ny, nx), dtype=np.float32)
    R, Y = _solve_oracle(c.po[64], gq, 64), _solve_oracle(c.po[32], gq, 32)
    X = _solve_gpu(c, gq, pad=7.0)          # the padding columns are not data
    for k in range(4):
        rms = np.sqrt(np.mean(R[..., k] ** 2))
        for name, m in (("rms", lambda Z: np.sqrt(np.mean((Z[..., k] - R[..., k]) ** 2)) / rms),
                        ("max", lambda Z: np.abs(Z[..., k] - R[..., k]).max() / rms)):
            got, yard = float(m(X)), float(m(Y))
            _note("F", f"{c.cells} component {k} {name}", got, yard)
            assert got <= FACTOR * yard, (k, name, got, yard)


@pytest.mark.parametrize("mode", list(itertools.product((0, 1), repeat=3)), ids=lambda m: "k" + "".join(map(str, m)))
def test_solve_pure_mode_is_zero(ctx, mode):
    """k = 0 and the seven Nyquist combinations have no field and no potential (.cu:433-476): +-1 grids transform exactly on the
    power-of-two grid, so the result is exactly zero."""
    c = ctx(UNIT[9])
    z, y, x = np.meshgrid(*(np.arange(32),) * 3, indexing="ij")
    gq = ((-1.0) ** (mode[0] * x + mode[1] * y + mode[2] * z)).astype(np.float32)
    assert np.all(_solve_gpu(c, gq) == 0.0)


# ---- G. thin boxes: a window wider than a short axis takes the atomic spread ------------------------------------------------------------
@pytest.mark.parametrize("cfg", THIN, ids=["32x32x4", "32x4x4"])
def test_thin_box(ctx, cfg):
    c = ctx(cfg)
    assert c.support > min(c.cells) + 1 and all(_tile_of(n) for n in c.cells)   # tiles exist and would fit: the one-wrap rule turns them off
    pos, q = _system(300, c.L, 17)
    g, info = c.spread_gpu(pos, q, 0)
    assert info["waves"] == 0 and info["tile"] == (0, 0, 0)
    _check_spread("G", f"{cfg} support {c.support} cells {c.cells} spread", g, c.spread_ref(("sys", 300, 17), pos, q))
    grid4 = _noise4(c)
    v, info = c.gather_gpu(pos, q, torch.from_numpy(grid4).cuda())
    _check_gather(f"{cfg} gather {info['gather']}", v, _gather_ref(c, ("gather", 300), pos, grid4), family="G")
