"""CPU tests of the Chebyshev transforms and the batched boundary value problem solver: the float64 NumPy
restatement in tests/chebyshev_bvp_ref.py is pinned on known answers, the host precomputation (uammd_amd/csrc/bvp_host.hpp) is compiled
into a stand-alone program under the address and undefined-behaviour sanitizers and compared with the restatement, the new entry points
are declared, exported and bound, and the programs that use the C++ headers pass the compiler's front end.  No GPU."""
import os
import re
import subprocess

import numpy as np
import pytest

import chebyshev_bvp_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
REF = "/root/reference"
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")


# ---- transforms --------------------------------------------------------------------------------------------------------------------------
def test_samples_of_chebyshev_polynomials_transform_to_unit_vectors():
    nz = 64
    j = np.arange(nz)
    samples = np.cos(np.pi * np.outer(j, np.arange(nz)) / (nz - 1)).astype(np.complex128)   # column m: T_m at the extrema
    c = ref.chebyshev_forward(samples)
    err = np.abs(c - np.eye(nz)).max()
    print(f"T_m -> e_m, nz = {nz}: {err:.2e}")
    assert err <= 1e-14


def test_round_trip_every_size():
    rng = np.random.default_rng(1234)
    worst = 0.0
    for nz in range(2, 128):
        f = rng.uniform(-1, 1, (nz, 3)) + 1j * rng.uniform(-1, 1, (nz, 3))
        worst = max(worst, np.abs(ref.chebyshev_inverse(ref.chebyshev_forward(f)) - f).max())
    print(f"round trip, nz = 2 ... 127: {worst:.2e}")
    assert worst <= 1e-13


def test_smallest_grid():
    f = np.array([[3.0 + 1j], [1.0 - 2j]])
    c = ref.chebyshev_forward(f)
    assert np.allclose(c, [[2.0 - 0.5j], [1.0 + 1.5j]], rtol=0, atol=1e-15)     # (f0 + f1) / 2, (f0 - f1) / 2
    assert np.allclose(ref.chebyshev_inverse(c), f, rtol=0, atol=1e-15)


def test_fourier_chebyshev_of_a_plane_wave():
    nz, ny, nx = 9, 4, 6
    z = ref.nodes(nz, 1.0)
    x = np.arange(nx) / nx
    f = (z ** 2)[:, None, None] * np.exp(2j * np.pi * 2 * x)[None, None, :] * np.ones((1, ny, 1))
    c = ref.fourier_chebyshev_forward(f)
    want = np.zeros_like(c)
    want[0, 0, 2], want[2, 0, 2] = 0.5, 0.5     # z^2 = (T_0 + T_2) / 2 at wave number (2, 0)
    assert np.abs(c - want).max() <= 1e-14
    assert np.abs(ref.fourier_chebyshev_inverse(c) - f).max() <= 1e-13


def test_single_precision_restatement_agrees_with_double():
    rng = np.random.default_rng(5)
    f = rng.uniform(-1, 1, (8, 3, 5)) + 1j * rng.uniform(-1, 1, (8, 3, 5))
    a, b = ref.fourier_chebyshev_forward(f), ref.fourier_chebyshev_forward(f, np.float32)
    assert b.dtype == np.complex64 and np.abs(a - b).max() <= 1e-6
    a, b = ref.fourier_chebyshev_inverse(f), ref.fourier_chebyshev_inverse(f, np.float32)
    assert np.abs(a - b).max() <= 2e-5


# ---- boundary value problem ---------------------------------------------------------------------------------------------------------------
def _solve_manufactured(k, H, nz, kind):
    fn, alpha, beta, y = ref.manufactured_problem(k, H, nz, kind)
    tab = ref.tables(k, H, nz, *ref.boundary_factors(k, H))
    cn, an = ref.solve(tab, H, fn[None], alpha[None], beta[None])
    return np.abs(ref.chebyshev_inverse(cn[0]) - y[:, None]).max()


@pytest.mark.parametrize("H", [1.0, 1.7])
@pytest.mark.parametrize("nz", [32, 64])
def test_manufactured_solution(H, nz):
    err = _solve_manufactured([0.0, 0.3, 2.0, 7.5, 40.0], H, nz, "smooth")
    print(f"H = {H}, nz = {nz}: max |y - exact| = {err:.2e}")
    assert err <= 1e-12


@pytest.mark.parametrize("nz", [4, 5, 6, 8])
def test_quadratic_is_exact_on_the_smallest_grids(nz):
    err = _solve_manufactured([0.0, 1.1], 1.3, nz, "quadratic")
    print(f"nz = {nz}: {err:.2e}")
    assert err <= 1e-13


def test_solve_leaves_the_right_hand_side_alone():
    fn, alpha, beta, _ = ref.manufactured_problem([2.0], 1.0, 16)
    before = fn.copy()
    ref.solve(ref.tables([2.0], 1.0, 16, *ref.boundary_factors([2.0], 1.0)), 1.0, fn[None], alpha[None], beta[None])
    assert np.array_equal(fn, before)


# ---- the host precomputation, stand-alone under the sanitizers ----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def bvp_tables_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("bvp") / "bvp_tables")
    r = subprocess.run(["g++", "-std=c++14", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        os.path.join(ROOT, "tests", "cxx", "bvp_tables.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def _run_tables(exe, nz, H, systems):
    args = [exe, str(nz), repr(H)] + [repr(float(v)) for s in systems for v in s]
    return subprocess.run(args, capture_output=True, text=True, timeout=120)


@pytest.mark.parametrize("nz,H", [(4, 1.0), (5, 1.7), (32, 1.0), (65, 1.7)])
def test_host_tables_match_the_restatement(bvp_tables_exe, nz, H):
    k = np.array([0.0, 0.3, 2.0, 7.5, 40.0 / H])
    tfi, tsi, bfi, bsi = ref.boundary_factors(k, H)
    r = _run_tables(bvp_tables_exe, nz, H, zip(k, tfi, tsi, bfi, bsi))
    assert r.returncode == 0 and r.stderr == "", r.stderr[-3000:]    # the sanitizers are silent
    got = {}
    for line in r.stdout.splitlines():
        w = line.split()
        got.setdefault(w[0], []).append([float(x) for x in w[2:]])
    want = ref.tables(k, H, nz, tfi, tsi, bfi, bsi)
    assert set(got) == set(want)
    for name in want:
        g = np.array(got[name])
        assert g.shape == want[name].shape, name
        scale = np.abs(want[name]).max(axis=0)   # per system, relative to the table's largest entry (a table of zeros, at k = 0, must be zeros)
        err = (np.abs(g - want[name]).max(axis=0) / np.where(scale > 0, scale, np.finfo(float).tiny)).max()
        print(f"nz = {nz}, H = {H}, {name}: {err:.2e}")
        assert err <= 1e-12, name


@pytest.mark.parametrize("nz,system,word", [(3, (1.0, 1.0, 1.0, 1.0, -1.0), "nz >= 4"), (8, (float("nan"), 1.0, 1.0, 1.0, -1.0), "non-finite"),
                                            (8, (float("inf"), 1.0, 1.0, 1.0, -1.0), "non-finite"), (8, (2.0, 0.0, 0.0, 0.0, 0.0), "singular")])
def test_host_precomputation_refuses_bad_batches(bvp_tables_exe, nz, system, word):
    good = (1.0, 1.0, 1.0, 1.0, -1.0)
    r = _run_tables(bvp_tables_exe, nz, 1.0, [good, system])
    assert r.returncode == 2 and word in r.stderr, r.stderr
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    if nz >= 4:
        assert "system 1" in r.stderr    # the message names the system at fault


# ---- entry points, Python layer, compilation ----------------------------------------------------------------------------------------------
NEW = ["uammd_fct_create", "uammd_fct_destroy", "uammd_fct_chebyshev", "uammd_fct_chebyshev_f64", "uammd_fct_fourier_chebyshev",
       "uammd_fct_fourier_chebyshev_f64", "uammd_bvp_create", "uammd_bvp_destroy", "uammd_bvp_solve", "uammd_bvp_solve_f64",
       "uammd_bvp_device_tables"]


def test_entry_points_declared_exported_and_bound():
    from uammd_amd import _lib
    from uammd_amd import build as hipbuild
    hipbuild.build()
    _lib.load()
    header = open(os.path.join(INC, "uammd_hip.h")).read()
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for n in NEW:
        assert re.search(r"\b" + n + r"\s*\(", header), n
        assert re.search(r" T " + n + r"\b", nm), n
        assert n in _lib.SIGNATURES, n


def test_create_refuses_bad_arguments_without_a_gpu():
    """The argument checks come before anything touches the device."""
    import ctypes as C
    from uammd_amd import _lib
    lib = _lib.load()
    h = C.c_void_p()
    assert lib.uammd_fct_create(4, 4, 1, 0, C.byref(h)) != 0 and b"nz >= 2" in lib.uammd_hip_last_error()
    assert lib.uammd_fct_create(4, 4, 8, 0, None) != 0 and b"null" in lib.uammd_hip_last_error()
    one = (C.c_double * 1)(1.0)
    nan = (C.c_double * 1)(float("nan"))
    zero = (C.c_double * 1)(0.0)
    assert lib.uammd_bvp_create(1, 3, 1.0, one, one, one, one, one, 1, C.byref(h)) != 0 and b"nz >= 4" in lib.uammd_hip_last_error()
    assert lib.uammd_bvp_create(1, 8, 1.0, nan, one, one, one, one, 1, C.byref(h)) != 0 and b"non-finite" in lib.uammd_hip_last_error()
    assert lib.uammd_bvp_create(1, 8, 1.0, one, zero, zero, zero, zero, 1, C.byref(h)) != 0 and b"singular" in lib.uammd_hip_last_error()
    assert lib.uammd_bvp_create(1, 8, 1.0, None, one, one, one, one, 1, C.byref(h)) != 0 and b"null" in lib.uammd_hip_last_error()
    assert not h.value


def test_python_layer():
    import inspect
    from uammd_amd.bvp import BatchedBVP
    from uammd_amd.chebyshev import FastChebyshevTransform
    assert list(inspect.signature(FastChebyshevTransform.__init__).parameters)[1:] == ["nx", "ny", "nz", "dtype"]
    assert list(inspect.signature(BatchedBVP.__init__).parameters)[1:] == ["k", "H", "nz", "top", "bottom", "dtype"]
    assert list(inspect.signature(BatchedBVP.solve).parameters)[1:4] == ["fn", "alpha", "beta"]


def test_stub_of_the_doubly_periodic_poisson_solver_is_unchanged():
    text = open(os.path.join(INC, "uammd", "Interactor", "DoublyPeriodic", "DPPoissonSlab.cuh")).read()
    assert "throw" in text


def test_user_kernel_program_compiles_in_both_precisions():
    for extra in ([], ["-DDOUBLE_PRECISION"]):
        r = subprocess.run([f"{ROCM}/bin/hipcc", "--offload-arch=gfx950", "-std=c++17", "-fsyntax-only", "-w"] + extra +
                           [f"-I{INC}/uammd", f"-I{INC}", os.path.join(ROOT, "tests", "cxx", "bvp_user_kernel.hip")], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]


@pytest.mark.skipif(not os.path.isdir(REF), reason="the reference tree is not on this machine")
@pytest.mark.parametrize("rel", ["../test/misc/bvp/test_bvp.cu", "../test/misc/chebyshev/fastChebyshevTransform.cu"])
def test_reference_unit_test_passes_the_front_end(rel, tmp_path):
    from test_reference_programs_compile import REF as SRC, _source
    src, _ = _source(rel, tmp_path, ".hip")
    r = subprocess.run([f"{ROCM}/bin/hipcc", "--offload-arch=gfx950", "-std=c++17", "-fsyntax-only", "-DDOUBLE_PRECISION", "-DMAXLOGLEVEL=1",
                        "-I", os.path.dirname(os.path.join(SRC, rel)), "-I", os.path.join(ROOT, "tests", "cxx", "gtest_lite"),
                        "-I", os.path.join(INC, "uammd"), "-I", INC, src], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
