"""CPU tests of the double-precision path A (uammd_amd/csrc/md_f64.hip): the host-only entry points against the -DDOUBLE_PRECISION oracle,
the scope boundary (the UAMMD-shaped headers still refuse double), and the host logic (uammd_amd/csrc/md_f64_host.hpp) under the address
and undefined-behaviour sanitizers through a stand-alone program."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
INC = os.path.join(ROOT, "include")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")

INF = float("inf")
GRID_CASES = [(16.0, (1, 1, 1)), (27.7, (1, 1, 1)), ((33.0, 22.0, 45.5), (1, 1, 1)), ((30.0, 30.0, 9.0), (1, 1, 1)), (7.0, (1, 1, 1)),
              ((40.0, INF, 40.0), (1, 1, 1)), (107.7217345, (1, 1, 1)), ((40.0, 40.0, 40.0), (1, 0, 1)), (np.finfo(np.float64).max, (1, 1, 1))]


@pytest.fixture(scope="module")
def lib():
    from uammd_amd import _lib
    from uammd_amd import build as hipbuild
    hipbuild.build()
    return _lib.load()


@pytest.mark.parametrize("L,periodic", GRID_CASES, ids=[str(c[0]) for c in GRID_CASES])
def test_create_grid_f64_vs_oracle(lib, o64, L, periodic):
    """cpu_f64_01: uammd_celllist_create_grid_f64 == the double oracle's createUpdateGrid, cut-offs 2.5 and 2.5 * 0.9."""
    from uammd_amd._lib import check
    d3, i3 = C.c_double * 3, C.c_int * 3
    L3 = np.broadcast_to(np.asarray(L, np.float64), (3,))
    for rc in (2.5, 2.5 * 0.9):
        cd, Lo, po = i3(), d3(), i3()
        check(lib.uammd_celllist_create_grid_f64(d3(*L3), i3(*periodic), d3(rc, rc, rc), cd, Lo, po))
        rcd, rL, rper = o64.celllist_create_grid(L3, periodic, rc)
        assert list(cd) == list(rcd), (L, rc)
        assert np.array_equal(np.array(list(Lo)), rL) and list(po) == list(rper)
    if L == 107.7217345:      # the division is exact in double: 43 cells, where the float rule's 107.7217345f / 2.5f also lands
        check(lib.uammd_celllist_create_grid_f64(d3(*L3), i3(*periodic), d3(2.5, 2.5, 2.5), cd, Lo, po))
        assert list(cd) == [43, 43, 43] and list(Lo) == [107.7217345] * 3


@pytest.mark.parametrize("shift", [False, True])
@pytest.mark.parametrize("rc,sigma,eps", [(2.5, 1.0, 1.0), (2.5 * 0.9, 1.06, 1.3)])
def test_process_pair_parameters_f64_vs_oracle(lib, o64, rc, sigma, eps, shift):
    """cpu_f64_02: bit for bit the oracle's processPairParameters in double; and through f64.LJ's type table."""
    from uammd_amd._lib import LJPairParameters64, check
    p = LJPairParameters64()
    check(lib.uammd_lj_process_pair_parameters_f64(rc, sigma, eps, int(shift), C.byref(p)))
    got = np.array([p.cutOff2, p.sigma2, p.epsilonDivSigma2, p.shift], np.float64)
    ref = o64.lj_params(rc, sigma, eps, shift)
    assert ref.dtype == np.float64 and np.array_equal(got.view(np.uint64), ref.view(np.uint64)), (got, ref)
    assert (got[3] != 0.0) == shift
    from uammd_amd import f64
    pot = f64.LJ()
    pot.setPotParameters(0, 0, pot.InputPairParameters(2.5, 1.0, 1.0, False))
    pot.setPotParameters(0, 2, pot.InputPairParameters(rc, sigma, eps, shift))      # the table grows to 3 x 3, symmetric
    assert pot.ntypes == 3 and pot.table.shape == (9, 4) and pot.getCutOff() == 2.5
    assert np.array_equal(pot.table[0 + 3 * 2], ref) and np.array_equal(pot.table[2 + 3 * 0], ref)
    assert np.array_equal(pot.table[0], o64.lj_params(2.5, 1.0, 1.0, False)) and not pot.table[1 + 3 * 1].any()


def test_headers_still_refuse_double_precision():
    """cpu_f64_03: the scope boundary.  The double backend exists behind the C ABI only; the forwarding headers of path A stop a
    -DDOUBLE_PRECISION build as before (opening some of them while VerletNVE.cuh and VerletList.cuh refuse would be half a build)."""
    for header in ("Integrator/VerletNVT.cuh", "Interactor/PairForces.cuh"):
        r = subprocess.run(["g++", "-std=c++14", "-fsyntax-only", "-DDOUBLE_PRECISION", "-D__HIP_PLATFORM_AMD__", f"-I{ROCM}/include",
                            f"-I{INC}/uammd", "-x", "c++", "-include", header, "/dev/null"], capture_output=True, text=True)
        assert r.returncode != 0 and "single-precision backend only" in r.stderr, header


def test_refusals_without_a_gpu(lib):
    """Argument checks that never reach the device: null handles, an unknown algorithm, a bad step."""
    from uammd_amd._lib import CellListData64
    d3, i3 = C.c_double * 3, C.c_int * 3
    assert lib.uammd_celllist_update_f64(None, None, 5, d3(1, 1, 1), i3(1, 1, 1), i3(1, 1, 1), None) != 0
    assert b"null handle" in lib.uammd_hip_last_error()
    h = C.c_void_p()
    assert lib.uammd_celllist_create_f64(C.byref(h)) == 0
    try:
        assert lib.uammd_celllist_update_f64(h, None, 0, d3(9, 9, 9), i3(1, 1, 1), i3(1, 1, 1), None) == 0          # N = 0: a no-op
        assert lib.uammd_lj_transverse_celllist_f64(h, C.c_void_p(8), 1, d3(9, 9, 9), i3(1, 1, 1), None, None, None, None, 1, None) == 0
        assert lib.uammd_lj_transverse_celllist_f64(h, C.c_void_p(8), 1, d3(9, 9, 9), i3(1, 1, 1), None, None, None, None, 8, None) == -1
        assert b"unknown algorithm" in lib.uammd_hip_last_error()
        assert lib.uammd_celllist_update_f64(h, C.c_void_p(8), 5, d3(1, 1, 1), i3(1, 1, 1), i3(0, 1, 1), None) != 0
        assert b"invalid grid" in lib.uammd_hip_last_error()
        d = CellListData64()
        assert lib.uammd_celllist_get_f64(h, C.byref(d)) == 0 and d.numberParticles == 0
    finally:
        assert lib.uammd_celllist_destroy_f64(h) == 0
    assert lib.uammd_verletnve_f64(3, C.c_void_p(8), C.c_void_p(8), C.c_void_p(8), None, 1.0, None, 4, 0.1, 0, None) == -1
    assert b"step must be 1 or 2" in lib.uammd_hip_last_error()
    assert lib.uammd_verletnvt_gj_f64(1, C.c_void_p(8), C.c_void_p(8), C.c_void_p(8), None, 0.0, None, 4, 0.1, 1.0, 0, 0.0, 0, 0, None) == -1
    assert b"defaultMass" in lib.uammd_hip_last_error()
    assert lib.uammd_verletnvt_gj_f64(1, None, None, None, None, 1.0, None, 0, 0.1, 1.0, 0, 0.0, 0, 0, None) == 0           # N = 0


def test_host_logic_under_the_sanitizers(tmp_path):
    """tests/cxx/md_f64_host.cpp: the grid rule, the parameter processing, the epoch rule, the argument checks and a host model of the
    build on heap blocks of exactly the handle's buffer sizes, with -fsanitize=address,undefined; and the header is plain C++14."""
    exe = str(tmp_path / "md_f64_host")
    r = subprocess.run(["g++", "-std=c++14", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra",
                        os.path.join(HERE, "cxx", "md_f64_host.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0 and "warning" not in r.stderr, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "md_f64_host: ok" in r.stdout and "ERROR" not in r.stderr and "runtime error" not in r.stderr, \
        (r.stdout[-2000:], r.stderr[-3000:])
    src = open(os.path.join(ROOT, "uammd_amd", "csrc", "md_f64_host.hpp")).read()
    assert "#include <hip" not in src and "hipStream_t" not in src
