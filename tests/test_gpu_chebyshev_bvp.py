"""GPU tests of the fast Chebyshev transforms and the batched boundary value problem solver, through the Python
layer, against the float64 NumPy restatement in tests/chebyshev_bvp_ref.py.

Bars.  Double build: 1e-13 absolute for the transforms (the bar of the reference's own unit tests), 1e-12 of max |c_n| for the solver.
Single build: the bar is measured here, not guessed - the largest difference between the float32 and the float64 restatement over the
cases of this file, times 4 for a different summation order.  Every test prints its figures before it asserts.
"""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import chebyshev_bvp_ref as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EX = os.path.join(ROOT, "examples")

# column counts off a multiple of 64, odd and even nz, the smallest nz, more than one block of columns and of outputs
SHAPES = [(1, 1, 2), (1, 1, 3), (1, 1, 127), (5, 3, 8), (16, 8, 5), (18, 16, 33), (70, 1, 64)]
OPS = {"chebyshev": ("chebyshevTransform", "inverseChebyshevTransform", ref.chebyshev_forward, ref.chebyshev_inverse),
       "fourier_chebyshev": ("fourierChebyshevTransform", "inverseFourierChebyshevTransform", ref.fourier_chebyshev_forward,
                             ref.fourier_chebyshev_inverse)}


@functools.lru_cache(maxsize=None)
def _field(shape):
    nx, ny, nz = shape
    rng = np.random.default_rng(20240 + nx + 100 * ny + 10000 * nz)
    return rng.uniform(-1, 1, (nz, ny, nx)) + 1j * rng.uniform(-1, 1, (nz, ny, nx))


@functools.lru_cache(maxsize=None)
def _expected(form, shape, real):
    """(forward, inverse, round trip) of the field, by the restatement in `real` precision."""
    fwd, inv = OPS[form][2], OPS[form][3]
    f = _field(shape)
    c = fwd(f, real)
    return c, inv(f, real), inv(c, real)


@functools.lru_cache(maxsize=None)
def _single_precision_bars():
    """4 x the largest float32-against-float64 difference of the restatement over the shapes and both forms, separately for the forward
    transform (values of order one), the inverse of random coefficients (sums of nx ny nz terms of order one) and the round trip."""
    worst = np.zeros(3)
    for form in OPS:
        for shape in SHAPES:
            worst = np.maximum(worst, [np.abs(a - b).max() for a, b in zip(_expected(form, shape, np.float64), _expected(form, shape, np.float32))])
    return 4 * worst


@pytest.mark.parametrize("dtype", [torch.complex128, torch.complex64], ids=["f64", "f32"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("form", sorted(OPS))
def test_transforms(form, shape, dtype):
    from uammd_amd.chebyshev import FastChebyshevTransform
    nx, ny, nz = shape
    bars = np.full(3, 1e-13) if dtype == torch.complex128 else _single_precision_bars()
    fct = FastChebyshevTransform(nx, ny, nz, dtype)
    forward, inverse = getattr(fct, OPS[form][0]), getattr(fct, OPS[form][1])
    x = torch.from_numpy(_field(shape)).to(dtype).cuda().reshape(-1)
    before = x.clone()
    c = forward(x)
    got = [c, inverse(x), inverse(c)]
    torch.cuda.synchronize()
    assert torch.equal(x, before)    # out of place
    errs = [np.abs(g.cpu().numpy().reshape(nz, ny, nx) - want).max() for g, want in zip(got, _expected(form, shape, np.float64))]
    print(f"{form} {shape} {dtype}: forward {errs[0]:.2e}, inverse {errs[1]:.2e}, round trip {errs[2]:.2e} (bars {bars[0]:.2e}, {bars[1]:.2e}, {bars[2]:.2e})")
    assert all(e <= b for e, b in zip(errs, bars))


def test_transform_errors_return_a_message():
    from uammd_amd import UammdHipError, _lib
    from uammd_amd.chebyshev import FastChebyshevTransform
    with pytest.raises(UammdHipError, match="nz >= 2"):
        FastChebyshevTransform(4, 4, 1)
    fct = FastChebyshevTransform(4, 2, 5, torch.complex64)
    x = torch.zeros(40, dtype=torch.complex64, device="cuda")
    with pytest.raises(UammdHipError, match="in == out"):
        fct.chebyshevTransform(x, out=x)
    with pytest.raises(UammdHipError, match="in == out"):
        fct.inverseFourierChebyshevTransform(x, out=x)
    lib = _lib.load()
    assert lib.uammd_fct_chebyshev(fct.h, None, C.c_void_p(x.data_ptr()), 1, None) != 0 and b"null" in lib.uammd_hip_last_error()
    assert lib.uammd_fct_fourier_chebyshev(fct.h, C.c_void_p(x.data_ptr()), None, 1, None) != 0 and b"null" in lib.uammd_hip_last_error()
    assert lib.uammd_fct_chebyshev_f64(fct.h, C.c_void_p(x.data_ptr()), C.c_void_p(x.data_ptr() + 8), 1, None) != 0
    assert b"single precision" in lib.uammd_hip_last_error()
    torch.cuda.synchronize()
    assert not x.any()


# ---- boundary value problem ---------------------------------------------------------------------------------------------------------------
NSYS = [1, 2, 31, 65, 1000]
NZ = [4, 8, 32, 65]
HS = [1.0, 1.7]
NRHS = 3


@functools.lru_cache(maxsize=None)
def _bvp_case(nsys, nz, H):
    """Wave numbers mixed in one batch (k = 0, with its own boundary factors, and k H = 40 among them), random right-hand sides, and the
    restatement's solution in both precisions."""
    palette = np.array([0.0, 0.3, 2.0, 7.5, 40.0 / H, 1.1, 13.0])
    k = palette[np.arange(nsys) % len(palette)]
    factors = ref.boundary_factors(k, H)
    rng = np.random.default_rng(7 + nsys + 1000 * nz + int(10 * H))
    fn = rng.uniform(-1, 1, (NRHS, nz, nsys)) + 1j * rng.uniform(-1, 1, (NRHS, nz, nsys))
    alpha = rng.uniform(-1, 1, (NRHS, nsys)) + 1j * rng.uniform(-1, 1, (NRHS, nsys))
    beta = rng.uniform(-1, 1, (NRHS, nsys)) + 1j * rng.uniform(-1, 1, (NRHS, nsys))
    tab = ref.tables(k, H, nz, *factors)
    cn64, an64 = ref.solve(tab, H, fn, alpha, beta)
    cn32, _ = ref.solve(tab, H, fn.astype(np.complex64), alpha.astype(np.complex64), beta.astype(np.complex64), np.float32)
    single = np.abs(cn32 - cn64).max() / np.abs(cn64).max()
    return k, factors, fn, alpha, beta, cn64, an64, single


@functools.lru_cache(maxsize=None)
def _bvp_single_precision_bar():
    return 4 * max(_bvp_case(nsys, nz, H)[7] for nsys in NSYS for nz in NZ for H in HS)


@pytest.mark.parametrize("H", HS)
@pytest.mark.parametrize("nz", NZ)
@pytest.mark.parametrize("nsys", NSYS)
def test_bvp_against_the_restatement(nsys, nz, H):
    from uammd_amd.bvp import BatchedBVP
    k, (tfi, tsi, bfi, bsi), fn, alpha, beta, cn64, an64, _ = _bvp_case(nsys, nz, H)
    scale_c, scale_a = np.abs(cn64).max(), np.abs(an64).max()
    own_c = np.abs(cn64).max(axis=(0, 1))    # per system: k H = 40 gives coefficients a thousand times smaller than its neighbours'
    for dtype, bar in ((torch.complex128, 1e-12), (torch.complex64, _bvp_single_precision_bar())):
        bvp = BatchedBVP(k, H, nz, (tfi, tsi), (bfi, bsi), dtype)
        for layout in ("interleaved", "contiguous"):
            host = fn if layout == "interleaved" else np.ascontiguousarray(fn.transpose(0, 2, 1))
            d_fn = torch.from_numpy(host).to(dtype).cuda()
            before = d_fn.clone()
            cn, an = bvp.solve(d_fn, torch.from_numpy(alpha).to(dtype).cuda(), torch.from_numpy(beta).to(dtype).cuda(), layout)
            cn2, an2 = bvp.solve(d_fn, torch.from_numpy(alpha).to(dtype).cuda(), torch.from_numpy(beta).to(dtype).cuda(), layout)
            torch.cuda.synchronize()
            assert torch.equal(d_fn, before)                               # fn is left alone
            assert torch.equal(cn, cn2) and torch.equal(an, an2)           # two runs, the same bits
            cn, an = cn.cpu().numpy(), an.cpu().numpy()
            if layout == "contiguous":
                cn, an = cn.transpose(0, 2, 1), an.transpose(0, 2, 1)
            ec, ea = np.abs(cn - cn64).max() / scale_c, np.abs(an - an64).max() / scale_a
            print(f"nsys {nsys} nz {nz} H {H} {dtype} {layout}: cn {ec:.2e}, an {ea:.2e} (bar {bar:.2e})")
            assert ec <= bar
            if dtype == torch.complex128:    # stricter than the batch-wide measure: every system against its own largest coefficient
                eo = (np.abs(cn - cn64).max(axis=(0, 1)) / own_c).max()
                print(f"    per system: {eo:.2e}")
                assert eo <= 1e-12
            assert ea <= 10 * bar    # an is not pinned by the issue; y'' carries k^2 H^2 times the rounding of y


@pytest.mark.parametrize("dtype", [torch.complex128, torch.complex64], ids=["f64", "f32"])
def test_bvp_result_does_not_depend_on_the_batch(dtype):
    """Identical copies give identical bits wherever they sit (index 0 and index 999), and a system solved alone gives the bits it
    gives inside a batch of 1000 with other wave numbers around it."""
    from uammd_amd.bvp import BatchedBVP
    nz, H, n = 32, 1.0, 1000
    rng = np.random.default_rng(3)
    one = rng.uniform(-1, 1, (1, nz, 1)) + 1j * rng.uniform(-1, 1, (1, nz, 1))
    ab = torch.tensor([[1.0 + 0.5j]], dtype=dtype).cuda()
    factors = ref.boundary_factors([2.0], H)
    alone = BatchedBVP([2.0], H, nz, factors[:2], factors[2:], dtype)
    c1, a1 = alone.solve(torch.from_numpy(one).to(dtype).cuda(), ab, ab)
    # identical copies
    copies = BatchedBVP(np.full(n, 2.0), H, nz, (np.full(n, factors[0][0]), np.full(n, factors[1][0])),
                        (np.full(n, factors[2][0]), np.full(n, factors[3][0])), dtype)
    cN, aN = copies.solve(torch.from_numpy(np.repeat(one, n, axis=2)).to(dtype).cuda(), ab.repeat(1, n), ab.repeat(1, n))
    assert torch.equal(cN, cN[:, :, :1].expand(-1, -1, n)) and torch.equal(aN, aN[:, :, :1].expand(-1, -1, n))
    assert torch.equal(cN[:, :, 999], c1[:, :, 0]) and torch.equal(aN[:, :, 0], a1[:, :, 0])
    # the same system at index 0 and at index 999 of a mixed batch, in the contiguous layout too
    k = np.linspace(0.0, 30.0, n)
    k[0] = k[999] = 2.0
    f = ref.boundary_factors(k, H)
    mixed = BatchedBVP(k, H, nz, f[:2], f[2:], dtype)
    fn = rng.uniform(-1, 1, (1, nz, n)) + 1j * rng.uniform(-1, 1, (1, nz, n))
    fn[:, :, 0] = fn[:, :, 999] = one[:, :, 0]
    alpha = ab.repeat(1, n)
    cM, aM = mixed.solve(torch.from_numpy(fn).to(dtype).cuda(), alpha, alpha)
    assert torch.equal(cM[:, :, 0], c1[:, :, 0]) and torch.equal(cM[:, :, 999], c1[:, :, 0])
    assert torch.equal(aM[:, :, 0], a1[:, :, 0]) and torch.equal(aM[:, :, 999], a1[:, :, 0])
    cC, aC = mixed.solve(torch.from_numpy(np.ascontiguousarray(fn.transpose(0, 2, 1))).to(dtype).cuda(), alpha, alpha, "contiguous")
    assert torch.equal(cC.transpose(1, 2), cM) and torch.equal(aC.transpose(1, 2), aM)


def test_bvp_errors_return_a_message():
    from uammd_amd import UammdHipError, _lib
    from uammd_amd.bvp import BatchedBVP
    good = ((1.0, 2.0), (1.0, -2.0))
    with pytest.raises(UammdHipError, match="nz >= 4"):
        BatchedBVP([1.0, 2.0], 1.0, 3, *good)
    with pytest.raises(UammdHipError, match="system 1.*non-finite"):
        BatchedBVP([1.0, float("nan")], 1.0, 8, *good)
    with pytest.raises(UammdHipError, match="system 2.*singular"):
        BatchedBVP([1.0, 2.0, 3.0], 1.0, 8, ([1.0, 1.0, 0.0], [2.0, 2.0, 0.0]), ([1.0, 1.0, 0.0], [-2.0, -2.0, 0.0]))
    bvp = BatchedBVP([1.0, 2.0], 1.0, 8, *good, dtype=torch.complex64)
    lib = _lib.load()
    x = torch.zeros(16, dtype=torch.complex64, device="cuda")
    y = torch.zeros(16, dtype=torch.complex64, device="cuda")
    z = torch.zeros(16, dtype=torch.complex64, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())
    assert lib.uammd_bvp_solve(bvp.h, None, p(x), p(x), p(y), p(z), 1, 1, 2, None) != 0 and b"null" in lib.uammd_hip_last_error()
    assert lib.uammd_bvp_solve(bvp.h, p(x), p(x), p(x), p(y), None, 1, 1, 2, None) != 0 and b"null" in lib.uammd_hip_last_error()
    assert lib.uammd_bvp_solve(bvp.h, p(x), p(x), p(x), p(x), p(z), 1, 1, 2, None) != 0 and b"different arrays" in lib.uammd_hip_last_error()
    assert lib.uammd_bvp_solve(bvp.h, p(x), p(x), p(x), p(y), p(z), 1, 3, 2, None) != 0 and b"strides" in lib.uammd_hip_last_error()
    assert lib.uammd_bvp_solve_f64(bvp.h, p(x), p(x), p(x), p(y), p(z), 1, 1, 2, None) != 0 and b"single precision" in lib.uammd_hip_last_error()
    torch.cuda.synchronize()
    assert not y.any() and not z.any()    # nothing ran


# ---- C++ programs -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("exe", ["bvp_user_kernel", "bvp_user_kernel_dp"])
def test_user_kernel_program(exe, tmp_path):
    r = subprocess.run([os.path.join(EX, "_build", exe)], cwd=tmp_path, capture_output=True, text=True, timeout=300)
    print(r.stdout + r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr


# The reference's own GoogleTest files of the two components, built by examples/Makefile from where they lie (-DDOUBLE_PRECISION) and run
# as tests/test_cxx_interface.py::test_reference_unit_tests_run runs the others:
#   misc/bvp/test_bvp.cu (4: identical copies, the analytic solution at 1e-13 for fixed and random k, random right-hand sides)
#   misc/chebyshev/fastChebyshevTransform.cu (19: the naive transforms, the periodic extension, the fast transforms against the naive
#   ones 1e-13 / 1e-14 for nz = 2 ... 127, round trips in 1-D and for 660 grid sizes in 3-D, Gaussians and a sine against closed forms)
REF_GTESTS = {"test_bvp": 4, "fastChebyshevTransform": 19}


@pytest.mark.parametrize("name", sorted(REF_GTESTS))
def test_reference_unit_tests_of_the_components_run(name, tmp_path):
    exe = os.path.join(EX, "_build", "ref_gtest_" + name)
    if not os.path.exists(exe):
        pytest.skip("ref_gtest_%s was not built (no reference tree where `make -C examples` ran)" % name)
    r = subprocess.run([exe], cwd=tmp_path, capture_output=True, text=True, timeout=1200)
    out = r.stdout + r.stderr
    print(out[-6000:])
    ran = re.search(r"\[==========\] (\d+) tests ran", out)
    assert ran and int(ran.group(1)) == REF_GTESTS[name], "not every TEST of the file ran"
    failed = re.findall(r"^\[  FAILED  \] (\S+)$", out, flags=re.M)
    assert r.returncode == 0 and not failed, failed
