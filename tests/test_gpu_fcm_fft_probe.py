"""The solver's own batched 3-D real FFT (csrc/fcm_fft.hpp and its launchers in csrc/fcm.hip) bin by bin against a float64 DFT, through
uammd_fcm_fft_probe: the pipeline's transforms and nothing else, on white noise, for every admissible length of every axis.

The velocity-level tests of test_gpu_fcm_fft.py weight a mode by the window's transform squared over k^2 and do not see most of the
spectrum (the FFT section); here every bin counts the same.

Measures, over the three components of a grid (X = the pipeline's output, R = the float64 reference of the same float32 input):
    e_rms = |X - R|_2 / |R|_2           e_max = max_bin |X - R| / rms_bin |R|
Bars:
    structural  e_max <= 1e-4 (a cap: one wrong bin gives e_max of order 1, single-precision pocketfft gives about 1e-6)
    precision   both measures <= 4 x the larger of two float32 yardsticks on the same input: scipy.fft (pocketfft) in single precision
                and torch.fft on the GPU (rocFFT) — neither is code under test.
rocFFT takes 0.3 to 1 s to plan every new shape (134 of the 139 s the sweep took with it), so the rocFFT yardstick is computed for the
named branch cases and for one grid per distinct pass plan (the z grids of test_fft_probe_pass_plans); everywhere else the bar is
4 x pocketfft alone, which can only be the stricter one."""
import numpy as np
import pytest
import scipy.fft as sfft
import torch

pytestmark = pytest.mark.gpu

FORWARD_XY, FORWARD_XYZ, INVERSE_ZYX = 0, 1, 2
PLANAR, FLOAT4, PACKED = 0, 1, 2
ROWS_LINES, PLANE_P2, PLANE_DENSE, PLANE_LARGE = 0, 1, 2, 3
STRUCTURAL_CAP = 1e-4
PRECISION_FACTOR = 4.0
MAX_NODES = 1 << 21
WORKERS = 8


# ---- what the launchers serve, restated in plain Python ---------------------------------------------------------------------------------
def _factors(n):
    e = []
    for p in (2, 3, 5, 7, 11):
        k = 0
        while n % p == 0:
            n //= p
            k += 1
        e.append(k)
    return e if n == 1 else None


def _admissible(lo, hi, even=False):
    return [n for n in range(lo, hi + 1) if _factors(n) is not None and not (even and n % 2)]


X_LENGTHS, Y_LENGTHS, Z_LENGTHS = _admissible(16, 512, even=True), _admissible(2, 256), _admissible(2, 512)
assert (len(X_LENGTHS), len(Y_LENGTHS), len(Z_LENGTHS)) == (89, 95, 137)


def _is_pow2(n):   # the shift-and-mask instantiations: powers of two from 4 up
    return n >= 4 and n & (n - 1) == 0


def _xy_path(nx, ny):
    """fcm_fft_forward_xy's choice (fcm_plane_fft_usable with a device that grants the 96 KB the launch asks for)."""
    nh = nx // 2
    lds = 8 * (nx + ny + ny * (nh + 1))
    if not (nx >= 32 and ny >= 16 and ny * nh // 4 <= 2048 and (nh + 1) * ny // 4 <= 3072 and lds <= 96 * 1024):
        return ROWS_LINES
    if _is_pow2(nx) and _is_pow2(ny):
        return PLANE_P2
    return PLANE_DENSE if lds <= 80 * 1024 else PLANE_LARGE


def _plane_lds(nx, ny):
    return 8 * (nx + ny + ny * (nx // 2 + 1))


def _plan(n):
    """The radices of fft_lds_any's passes over a line of n points, in order."""
    e2, e3, e5, e7, e11 = _factors(n)
    if _is_pow2(n):
        return [4] * {0: 0, 2: 1, 1: 2}[e2 % 3] + [8] * ((e2 - 2 * {0: 0, 2: 1, 1: 2}[e2 % 3]) // 3)
    passes2 = lambda a: (a + 2) // 3
    n9, r3 = e3 // 2, e3 & 1
    n12 = n6 = 0
    n3, a2 = r3, e2
    if r3:
        plain = passes2(e2) + 1
        if e2 >= 2 and passes2(e2 - 2) + 1 < plain:
            n12, n3, a2 = 1, 0, e2 - 2
        elif e2 >= 1 and passes2(e2 - 1) + 1 < plain:
            n6, n3, a2 = 1, 0, e2 - 1
    n8, n4, n2 = a2 // 3, 0, 0
    if a2 % 3 == 2:
        n4 = 1
    elif a2 % 3 == 1:
        if n8 > 0:
            n8, n4 = n8 - 1, 2
        else:
            n2 = 1
    return [2] * n2 + [4] * n4 + [8] * n8 + [6] * n6 + [12] * n12 + [3] * n3 + [9] * n9 + [5] * e5 + [7] * e7 + [11] * e11


for _n in Z_LENGTHS:
    assert int(np.prod(_plan(_n))) == _n, _n


# ---- inputs, references, yardsticks -------------------------------------------------------------------------------------------------------
def _seed(cells, salt=0):
    return (cells[0] * 1_000_003 + cells[1] * 1009 + cells[2]) * 7 + salt


def _white(cells, salt=0):
    nx, ny, nz = cells
    return np.random.default_rng(_seed(cells, salt)).standard_normal((3, nz, ny, nx), dtype=np.float32)


def _measures(got, ref):
    d = np.abs(got - ref)
    rms = np.sqrt(np.mean(np.abs(ref) ** 2))
    return float(np.sqrt(np.mean(d ** 2)) / rms), float(d.max() / rms)


def _padded(a, pad):
    """(3, nz, ny, nx) reals -> the solver's rows of nx + 2 floats on the device, the two pad floats holding `pad`."""
    g = np.full(a.shape[:-1] + (a.shape[-1] + 2,), pad, np.float32)
    g[..., :-2] = a
    return torch.from_numpy(g).cuda()


def _as_complex(g):
    return np.ascontiguousarray(g.cpu().numpy()).view(np.complex64)


def _spectrum_device(s):
    return torch.from_numpy(np.ascontiguousarray(s).view(np.float32)).cuda()


def forward_case(hip, cells, mode=FORWARD_XYZ, with_torch=True):
    """White noise through the forward passes: ((e_rms, e_max) of the pipeline, of scipy float32, of torch float32 or None, info)."""
    a = _white(cells)
    axes = (1, 2, 3) if mode == FORWARD_XYZ else (2, 3)
    ref = sfft.rfftn(a.astype(np.float64), axes=axes, workers=WORKERS)
    g = _padded(a, 1e30)   # a read of the padding shows
    path, tile, _ = hip.bdhi.fft_probe(cells, mode, g)
    torch.cuda.synchronize()
    mine = _measures(_as_complex(g), ref)
    y32 = sfft.rfftn(a, axes=axes, workers=WORKERS)
    assert y32.dtype == np.complex64
    yard = [_measures(y32, ref), None]
    if with_torch:
        yard[1] = _measures(torch.fft.rfftn(torch.from_numpy(a).cuda(), dim=axes).cpu().numpy(), ref)
    return mine, yard[0], yard[1], (path, tile)


def inverse_case(hip, cells, with_torch=True):
    """The complex64 spectrum of a real white field through the inverse passes, against irfftn x nx ny nz of that spectrum in float64."""
    nx, ny, nz = cells
    s = sfft.rfftn(_white(cells, salt=1).astype(np.float64), axes=(1, 2, 3), workers=WORKERS).astype(np.complex64)
    n = nx * ny * nz
    ref = sfft.irfftn(s.astype(np.complex128), s=(nz, ny, nx), axes=(1, 2, 3), workers=WORKERS) * n
    g = _spectrum_device(s)
    path, tile, _ = hip.bdhi.fft_probe(cells, INVERSE_ZYX, g)
    torch.cuda.synchronize()
    assert path == -1
    mine = _measures(g.cpu().numpy()[..., :nx], ref)
    y32 = sfft.irfftn(s, s=(nz, ny, nx), axes=(1, 2, 3), workers=WORKERS)
    assert y32.dtype == np.float32
    yard = [_measures(y32.astype(np.float64) * n, ref), None]
    if with_torch:
        t = torch.fft.irfftn(torch.from_numpy(s).cuda(), s=(nz, ny, nx), dim=(1, 2, 3), norm="forward")
        yard[1] = _measures(t.cpu().numpy(), ref)
    return mine, yard[0], yard[1], (path, tile)


def _bars(mine, ys, yt):
    """(ratio of e_rms, ratio of e_max) to the larger yardstick."""
    return tuple(mine[i] / max(ys[i], yt[i] if yt is not None else 0.0) for i in range(2))


RESULTS = []   # (cells, mode, e_rms, e_max, ratio_rms, ratio_max): filled as the tests run, for whoever wants to tabulate them


def check_grid(hip, cells, with_torch=True):
    """Both directions of one grid against both bars; the x/y path and the z tile against what the launchers should have picked."""
    nx, ny, nz = cells
    failures = []
    for mode, run in ((FORWARD_XYZ, lambda: forward_case(hip, cells, FORWARD_XYZ, with_torch)), (INVERSE_ZYX, lambda: inverse_case(hip, cells, with_torch))):
        mine, ys, yt, (path, tile) = run()
        r = _bars(mine, ys, yt)
        RESULTS.append((tuple(cells), mode, mine[0], mine[1], r[0], r[1]))
        print(f"fft_probe {nx}x{ny}x{nz} mode {mode}: e_rms {mine[0]:.3e} e_max {mine[1]:.3e}  scipy32 {ys[0]:.3e} {ys[1]:.3e}  "
              f"torch {'%.3e %.3e' % yt if yt else '-'}  ratios {r[0]:.2f} {r[1]:.2f}  path {path} tile {tile}")
        assert tile == (8 if nz <= 256 else 4), (cells, tile)
        if mode == FORWARD_XYZ and _plane_lds(nx, ny) <= 64 * 1024:   # (above 64 KB the choice depends on what the device grants)
            assert path == _xy_path(nx, ny), (cells, path)
        if not (np.isfinite(mine[1]) and mine[1] <= STRUCTURAL_CAP and max(r) <= PRECISION_FACTOR):
            where = ""
            if mode == FORWARD_XYZ:   # name the axis: the same input through the x and y passes alone
                m2, s2, t2, _ = forward_case(hip, cells, FORWARD_XY, with_torch)
                where = f"; FORWARD_XY alone: e_rms {m2[0]:.3e} e_max {m2[1]:.3e}, ratios {_bars(m2, s2, t2)} (within its bars: the z pass)"
            failures.append(f"{nx}x{ny}x{nz} mode {mode}: e_rms {mine[0]:.3e} e_max {mine[1]:.3e}, ratios to the yardstick {r}{where}")
    return failures


# ---- the sweep: every admissible length of every axis ----------------------------------------------------------------------------------------
def _sweep_grids():
    """137 grids, one per z length, each with an x and a y length not yet seen while those last (the node counts' geometric mean is the
    product of the three lists' whatever the pairing, so the shorter lists are filled up with their four smallest lengths, not with a
    second round); long axes with short ones.  Three small planes more for the power-of-two plane kernel, which the pairing misses."""
    n = len(Z_LENGTHS)
    fill = lambda lengths: sorted(lengths + [lengths[i % 4] for i in range(n - len(lengths))])
    planes = sorted(zip(fill(X_LENGTHS), reversed(fill(Y_LENGTHS))), key=lambda p: p[0] * p[1])
    return [(x, y, z) for (x, y), z in zip(planes, sorted(Z_LENGTHS, reverse=True))] + [(32, 16, 4), (64, 64, 8), (128, 32, 16)]


SWEEP = _sweep_grids()
assert {g[0] for g in SWEEP} == set(X_LENGTHS) and {g[1] for g in SWEEP} == set(Y_LENGTHS) and {g[2] for g in SWEEP} == set(Z_LENGTHS)
assert max(g[0] * g[1] * g[2] for g in SWEEP) <= MAX_NODES
# The x/y paths.  `plane large` (mixed radix, more than 80 KB of LDS) cannot be reached by any admissible plane, and not because of the
# device's LDS limit: the plane kernel's butterfly budget ny (nx / 2) / 4 <= 2048 holds its LDS, 8 (nx + ny + ny (nx / 2 + 1)) bytes, to
# 70 144.
REACHABLE_PATHS = {_xy_path(x, y) for x in X_LENGTHS for y in Y_LENGTHS}
assert REACHABLE_PATHS == {ROWS_LINES, PLANE_P2, PLANE_DENSE}
assert max(_plane_lds(x, y) for x in X_LENGTHS for y in Y_LENGTHS if _xy_path(x, y) != ROWS_LINES) == 70144 < 80 * 1024
# the smallest grid of the sweep on each reachable path whose plane fits the 64 KB every device grants
PATH_GRIDS = {}
for _g in sorted(SWEEP, key=lambda g: -g[0] * g[1] * g[2]):
    if _plane_lds(_g[0], _g[1]) <= 64 * 1024:
        PATH_GRIDS[_xy_path(_g[0], _g[1])] = _g
assert set(PATH_GRIDS) == REACHABLE_PATHS, "the sweep does not reach every x/y path"
N_CHUNKS = 14   # ten grids each, large and small mixed: grid i of the list by size goes to chunk i mod 14
SWEEP_CHUNKS = [sorted(SWEEP, key=lambda g: g[0] * g[1] * g[2])[i::N_CHUNKS] for i in range(N_CHUNKS)]
assert sorted(g for c in SWEEP_CHUNKS for g in c) == sorted(SWEEP)


@pytest.mark.parametrize("chunk", SWEEP_CHUNKS, ids=[f"chunk{i:02d}" for i in range(N_CHUNKS)])
def test_fft_probe_sweep(hip, chunk):
    failures = []
    for cells in chunk:
        failures += check_grid(hip, cells, with_torch=False)
    assert not failures, "\n".join(failures)


def test_fft_probe_sweep_reports_every_xy_path(hip):
    """info[0] over the sweep: rows + lines, the power-of-two plane kernel and the two-per-CU plane kernel (see REACHABLE_PATHS for the
    fourth)."""
    seen = {}
    for want, cells in PATH_GRIDS.items():
        nx, ny, nz = cells
        g = torch.zeros((3, nz, ny, nx + 2), dtype=torch.float32, device="cuda")
        seen[want] = hip.bdhi.fft_probe(cells, FORWARD_XY, g)[0]
    torch.cuda.synchronize()
    assert seen == {p: p for p in REACHABLE_PATHS}, seen


# ---- named small cases: the smallest shape that reaches each branch -----------------------------------------------------------------------------
BRANCH_GRIDS = [
    # z tiles on lengths whose first forward / last inverse pass is fused with the loads / stores (log2 nz not a multiple of 3, >= 5):
    # 72 lines = nine full tiles of 8; 36 lines = four full tiles and one of 4 that takes the plain branch.  64 and 512 never fuse.
    ((16, 8, 32), "z 32: full tiles"), ((16, 4, 32), "z 32: partial last tile"),
    ((16, 8, 128), "z 128: full tiles"), ((16, 4, 128), "z 128: partial last tile"),
    ((16, 8, 256), "z 256: full tiles"), ((16, 4, 256), "z 256: partial last tile"),
    ((16, 8, 64), "z 64: plain"), ((16, 4, 512), "z 512: plain, tiles of 4"), ((16, 3, 512), "z 512: partial last tile of 4"),
    # row tail blocks: 27 rows in blocks of 16 (k_fft_x_r2c), 9 rows in blocks of 8 or 5 (k_fft_x_c2r); the fused first pass of the
    # power-of-two rows is radix 8 for nx / 2 = 8, 64 and radix 4 for 16, 32, 128
    ((16, 3, 3), "row tails, first pass radix 8"), ((128, 3, 3), "row tails, first pass radix 8"),
    ((32, 3, 3), "row tails, first pass radix 4"), ((64, 3, 3), "row tails, first pass radix 4"), ((256, 3, 3), "row tails, first pass radix 4"),
    ((50, 3, 3), "row tails, mixed radix"), ((512, 3, 3), "row tails, 8 and 2 rows per block"),
    # k_fft_lines: nkx = nx / 2 + 1 that is no multiple of 16; a two-point y axis with power-of-two x (the general instantiation)
    ((16, 8, 4), "nkx 9: one narrow tile"), ((64, 8, 4), "nkx 33: two full tiles and one of a single line"),
    ((16, 2, 4), "ny 2"), ((64, 2, 8), "ny 2"), ((30, 6, 4), "nkx 16: one full tile, mixed radix"),
    # k_fft_lines' own fused first / last passes: full tiles of 32, 128, 256 lines (the forward only where the plane kernel does not serve)
    ((64, 32, 2), "y 32 fused, inverse"), ((64, 128, 2), "y 128 fused, inverse"), ((512, 128, 2), "y 128 fused, both directions"),
    ((512, 256, 2), "y 256 fused, both directions"), ((64, 64, 2), "y 64 plain"),
    # the plane kernel: power-of-two planes with and without its fused passes (columns of 16 = 4 x 4 never fuse), mixed radix
    ((32, 16, 2), "plane p2, columns 16"), ((32, 32, 3), "plane p2 fused, rows radix 4"), ((128, 64, 2), "plane p2 fused, rows radix 8"),
    ((64, 256, 2), "plane p2, 256 rows"), ((36, 18, 2), "plane mixed radix"), ((54, 54, 3), "plane mixed radix"),
]

# one length per pass plan fft_lds_any distinguishes, with the plan it is there for
PLAN_LENGTHS = {
    2: [2], 4: [4], 8: [8], 16: [4, 4], 32: [4, 8], 64: [8, 8], 128: [4, 4, 8], 256: [4, 8, 8], 512: [8, 8, 8],   # (2: general; the rest shifts)
    10: [2, 5], 20: [4, 5], 40: [8, 5], 80: [4, 4, 5], 160: [4, 8, 5], 320: [8, 8, 5],     # leading 2, one and two leading 4 in the general passes
    3: [3], 6: [6], 12: [12], 24: [8, 3], 48: [4, 12], 96: [8, 12], 192: [8, 8, 3], 384: [4, 8, 12],   # an odd power of three: 12, 6 or 3
    27: [3, 9], 54: [6, 9], 108: [12, 9], 216: [8, 3, 9], 432: [4, 12, 9], 243: [3, 9, 9], 486: [6, 9, 9],
    9: [9], 18: [2, 9], 36: [4, 9], 72: [8, 9], 81: [9, 9], 144: [4, 4, 9], 288: [4, 8, 9], 162: [2, 9, 9], 324: [4, 9, 9],
    5: [5], 25: [5, 5], 7: [7], 49: [7, 7], 11: [11], 121: [11, 11], 242: [2, 11, 11],
    14: [2, 7], 22: [2, 11], 35: [5, 7], 55: [5, 11], 77: [7, 11], 462: [6, 7, 11], 125: [5, 5, 5], 343: [7, 7, 7],
}
for _n, _p in PLAN_LENGTHS.items():
    assert _plan(_n) == _p, (_n, _plan(_n), _p)
# every sequence of power-of-two and power-of-three passes that an admissible length takes in the general instantiation is listed (31 of them)
_lead = lambda p: tuple(r for r in p if r in (2, 4, 8, 6, 12, 3, 9))
assert {_lead(_plan(n)) for n in Z_LENGTHS if not _is_pow2(n)} == {_lead(p) for n, p in PLAN_LENGTHS.items() if not _is_pow2(n)}
assert {tuple(_plan(n)) for n in Z_LENGTHS if _is_pow2(n)} == {tuple(p) for n, p in PLAN_LENGTHS.items() if _is_pow2(n)}


def _plan_grids(axis):
    out = []
    for n in PLAN_LENGTHS:
        if axis == "x" and 16 <= 2 * n <= 512:
            out.append((2 * n, 3, 2))    # the rows' complex transform has nx / 2 points
        if axis == "y" and n <= 256:
            out.append((16, n, 2))
        if axis == "z":
            out.append((16, 2, n))
    return out


@pytest.mark.parametrize("cells,why", BRANCH_GRIDS, ids=["x".join(map(str, g)) for g, _ in BRANCH_GRIDS])
def test_fft_probe_branch(hip, cells, why):
    failures = check_grid(hip, cells)
    assert not failures, why + ": " + "\n".join(failures)


# (the z grids, with the rocFFT yardstick, in four parts of a few seconds)
@pytest.mark.parametrize("axis,part", [("x", 0), ("y", 0), ("z", 0), ("z", 1), ("z", 2), ("z", 3)], ids=["x", "y", "z0", "z1", "z2", "z3"])
def test_fft_probe_pass_plans(hip, axis, part):
    failures = []
    grids = _plan_grids(axis)
    for cells in grids[part::4] if axis == "z" else grids:
        plan = PLAN_LENGTHS[cells["xyz".index(axis)] // (2 if axis == "x" else 1)]
        failures += [f"plan {plan}: {f}" for f in check_grid(hip, cells, with_torch=axis == "z")]
    assert not failures, "\n".join(failures)


# ---- impulses: component order, sign convention and index mapping, independently of the statistics ----------------------------------------------
IMPULSE_GRIDS = [(32, 16, 32), (30, 12, 20), (44, 21, 10)]
# One input is not zero, so every output is a product of the twiddle factors on its way and nothing else.  At most three passes per axis
# and the rows' untangling step: ten factors, each exact to about two float32 ulps (the rounded ratio in sincospif's argument, sincospif
# itself, the complex product).  A wrong index or a table one size too coarse is off by 2 pi / n >= 1e-2.
IMPULSE_TOL = 10 * 2 * 2.0 ** -23


def _phase(cells, node, sign):
    nx, ny, nz = cells
    x0, y0, z0 = node
    kz, ky, kx = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx // 2 + 1), indexing="ij")
    return np.exp(sign * 2j * np.pi * (kx * x0 / nx + ky * y0 / ny + kz * z0 / nz))


@pytest.mark.parametrize("cells", IMPULSE_GRIDS, ids=["x".join(map(str, g)) for g in IMPULSE_GRIDS])
def test_fft_probe_impulse_forward(hip, cells):
    nx, ny, nz = cells
    rng = np.random.default_rng(_seed(cells, 2))
    for c in range(3):
        x0, y0, z0 = int(rng.integers(1, nx)), int(rng.integers(1, ny)), int(rng.integers(1, nz))
        a = np.zeros((3, nz, ny, nx), np.float32)
        a[c, z0, y0, x0] = 1.0
        g = _padded(a, 1e30)
        hip.bdhi.fft_probe(cells, FORWARD_XYZ, g)
        got = _as_complex(g)
        for o in range(3):
            if o == c:
                assert np.abs(got[o] - _phase(cells, (x0, y0, z0), -1)).max() <= IMPULSE_TOL, (cells, c)
            else:
                assert not got[o].any(), (cells, c, o)


@pytest.mark.parametrize("cells", IMPULSE_GRIDS, ids=["x".join(map(str, g)) for g in IMPULSE_GRIDS])
def test_fft_probe_single_bin_inverse(hip, cells):
    """One bin (with its Hermitian mate where the half spectrum stores one: kx = 0) gives 2 Re(v exp(+i k r))."""
    nx, ny, nz = cells
    rng = np.random.default_rng(_seed(cells, 3))
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    for c, kx in ((0, int(rng.integers(1, nx // 2))), (1, 0), (2, int(rng.integers(1, nx // 2)))):
        ky, kz = int(rng.integers(1, (ny + 1) // 2)), int(rng.integers(1, (nz + 1) // 2))   # (not self-conjugate: 0 < k < n / 2)
        th = float(rng.uniform(0, 2 * np.pi))
        v = np.complex64(np.cos(th) + 1j * np.sin(th))
        s = np.zeros((3, nz, ny, nx // 2 + 1), np.complex64)
        s[c, kz, ky, kx] = v
        if kx == 0:
            s[c, nz - kz, ny - ky, 0] = np.conj(v)
        g = _spectrum_device(s)
        hip.bdhi.fft_probe(cells, INVERSE_ZYX, g)
        got = g.cpu().numpy()[..., :nx]
        want = 2.0 * np.real(complex(v) * np.exp(2j * np.pi * (kx * x / nx + ky * y / ny + kz * z / nz)))
        for o in range(3):
            if o == c:
                assert np.abs(got[o] - want).max() <= 2 * IMPULSE_TOL, (cells, c)
            else:
                assert not got[o].any(), (cells, c, o)


# ---- the three output targets of the inverse ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cells", [(16, 12, 10), (16, 8, 16), (50, 7, 9)], ids=["16x12x10", "16x8x16", "50x7x9"])
def test_fft_probe_inverse_targets_hold_the_same_bits(hip, cells):
    """The planar grids, the gather's float4 grid and its packed form (which the solver takes only above 128 MB)."""
    nx, ny, nz = cells
    s = sfft.rfftn(_white(cells, salt=4).astype(np.float64), axes=(1, 2, 3)).astype(np.complex64)
    out = {}
    for target in (PLANAR, FLOAT4, PACKED):
        g = _spectrum_device(s)
        _, _, inter = hip.bdhi.fft_probe(cells, INVERSE_ZYX, g, target)
        out[target] = g[..., :nx].clone() if target == PLANAR else inter
    assert out[FLOAT4].shape == (nz, ny, nx, 4) and out[PACKED].shape == (nz, ny, nx, 3)
    planar = out[PLANAR].permute(1, 2, 3, 0).contiguous()
    assert planar.abs().max() > 0
    assert torch.equal(out[FLOAT4][..., :3].contiguous().view(torch.int32), planar.view(torch.int32))
    assert torch.equal(out[PACKED].view(torch.int32), planar.view(torch.int32))
    assert not out[FLOAT4][..., 3].any()


# ---- lengths the pipeline does not serve ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cells", [(15, 8, 8), (26, 8, 8), (16, 26, 8), (16, 8, 13), (14, 8, 8), (16, 512, 4), (16, 4, 1024), (514, 4, 4)],
                         ids=lambda c: "x".join(map(str, c)))
def test_fft_probe_rejects(hip, cells):
    nx, ny, nz = cells
    shape = (3, nz, ny, 2 * (nx // 2 + 1))
    before = torch.arange(int(np.prod(shape)), dtype=torch.float32, device="cuda").reshape(shape)
    for mode in (FORWARD_XY, FORWARD_XYZ, INVERSE_ZYX):
        g = before.clone()
        with pytest.raises(hip.UammdHipError):
            hip.bdhi.fft_probe(cells, mode, g)
        torch.cuda.synchronize()
        assert torch.equal(g, before)
