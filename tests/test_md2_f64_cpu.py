"""CPU tests of the second half of path A in double (uammd_amd/csrc/verletlist_f64.hip, bonded_f64.hip, dpd_f64.hip): every new symbol is
declared, exported and bound; the argument refusals that never reach the device; and the Verlet list's host logic
(uammd_amd/csrc/verletlist_f64_host.hpp) under the address and undefined-behaviour sanitizers through a stand-alone program."""
import ctypes as C
import os
import re
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

NEW_SYMBOLS = [
    "uammd_verletlist_create_f64", "uammd_verletlist_destroy_f64", "uammd_verletlist_update_f64", "uammd_verletlist_force_next_update_f64",
    "uammd_verletlist_set_cutoff_multiplier_f64", "uammd_verletlist_get_steps_since_last_update_f64", "uammd_verletlist_get_f64",
    "uammd_lj_transverse_verletlist_f64",
    "uammd_bonded_create_f64", "uammd_bonded_destroy_f64", "uammd_bonded_upload_f64", "uammd_bonded_refresh_f64", "uammd_bonded_sum_f64",
    "uammd_bonded_get_shape_f64",
    "uammd_dpd_transverse_celllist_f64", "uammd_dpd_transverse_nbody_f64"]

d3, i3 = C.c_double * 3, C.c_int * 3


@pytest.fixture(scope="module")
def lib():
    from uammd_amd import _lib
    from uammd_amd import build as hipbuild
    hipbuild.build()
    return _lib.load()


def test_every_new_symbol_is_declared_exported_and_bound(lib):
    from uammd_amd import _lib
    src = open(os.path.join(ROOT, "include", "uammd_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(uammd_[a-z0-9_]+)\s*\(", src))
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (uammd_[a-z0-9_]+)", nm))
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert name in exported, name
        assert name in _lib.SIGNATURES, name
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    for cls in ("VerletList", "BondedForces", "PairForcesDPD"):
        from uammd_amd import f64
        assert hasattr(f64, cls)


def test_verletlist_refusals_without_a_gpu(lib):
    """Null handles, a non-positive cut-off, a multiplier below 1: -1 and a message, before anything is launched; N = 0 is a no-op."""
    from uammd_amd._lib import VerletListData
    err = lib.uammd_hip_last_error
    assert lib.uammd_verletlist_create_f64(None) == -1
    assert lib.uammd_verletlist_update_f64(None, C.c_void_p(8), 4, d3(9, 9, 9), i3(1, 1, 1), 2.5, None, None) == -1
    assert b"null handle" in err()
    assert lib.uammd_verletlist_force_next_update_f64(None) == -1 and b"null handle" in err()
    assert lib.uammd_verletlist_set_cutoff_multiplier_f64(None, 1.08) == -1 and b"null handle" in err()
    assert lib.uammd_verletlist_get_steps_since_last_update_f64(None, None) == -1
    assert lib.uammd_verletlist_get_f64(None, None) == -1
    assert lib.uammd_lj_transverse_verletlist_f64(None, C.c_void_p(8), 1, d3(9, 9, 9), i3(1, 1, 1), None, None, None, None, None) == -1
    assert lib.uammd_verletlist_destroy_f64(None) == 0
    h = C.c_void_p()
    assert lib.uammd_verletlist_create_f64(C.byref(h)) == 0
    try:
        assert lib.uammd_verletlist_set_cutoff_multiplier_f64(h, 0.99) == -1 and b"multiplier must be at least 1" in err()
        assert lib.uammd_verletlist_set_cutoff_multiplier_f64(h, float("nan")) == -1
        assert lib.uammd_verletlist_update_f64(h, C.c_void_p(8), 4, d3(9, 9, 9), i3(1, 1, 1), 0.0, None, None) == -1
        assert b"cut-off must be positive" in err()
        assert lib.uammd_verletlist_update_f64(h, C.c_void_p(8), 4, d3(9, 9, 9), i3(1, 1, 1), -2.5, None, None) == -1
        assert lib.uammd_verletlist_update_f64(h, None, 4, d3(9, 9, 9), i3(1, 1, 1), 2.5, None, None) == -1 and b"null positions" in err()
        assert lib.uammd_verletlist_update_f64(h, C.c_void_p(8), -4, d3(9, 9, 9), i3(1, 1, 1), 2.5, None, None) == -1
        rebuilt = C.c_int(7)
        assert lib.uammd_verletlist_update_f64(h, None, 0, d3(9, 9, 9), i3(1, 1, 1), 2.5, None, C.byref(rebuilt)) == 0     # N = 0: a no-op
        assert rebuilt.value == 0
        d = VerletListData()
        assert lib.uammd_verletlist_get_f64(h, C.byref(d)) == 0 and d.numberParticles == 0 and d.maxNeighboursPerParticle == 32
        steps = C.c_int(5)
        assert lib.uammd_verletlist_get_steps_since_last_update_f64(h, C.byref(steps)) == 0 and steps.value == -1
        assert lib.uammd_lj_transverse_verletlist_f64(h, C.c_void_p(8), 1, d3(9, 9, 9), i3(1, 1, 1), None, None, None, None, None) == 0
        assert lib.uammd_lj_transverse_verletlist_f64(h, C.c_void_p(8), 0, d3(9, 9, 9), i3(1, 1, 1), None, None, None, None, None) == -1
        assert lib.uammd_verletlist_set_cutoff_multiplier_f64(h, 1.0) == 0 and lib.uammd_verletlist_force_next_update_f64(h) == 0
    finally:
        assert lib.uammd_verletlist_destroy_f64(h) == 0


def test_bonded_and_dpd_refusals_without_a_gpu(lib):
    err = lib.uammd_hip_last_error
    assert lib.uammd_bonded_create_f64(None) == -1
    h = C.c_void_p()
    assert lib.uammd_bonded_create_f64(C.byref(h)) == 0
    try:
        assert lib.uammd_bonded_sum_f64(h, C.c_void_p(8), C.c_void_p(8), None, None, None) == -1          # sum before upload
        assert b"no bond set uploaded" in err()
        assert lib.uammd_bonded_refresh_f64(h, C.c_void_p(8), 4, None) == -1 and b"no bond set uploaded" in err()
        assert lib.uammd_bonded_upload_f64(h, 7, 0, None, None, 0, None, d3(9, 9, 9), i3(1, 1, 1)) == -1 and b"bad arguments" in err()
        ids = (C.c_int * 2)(0, -3)      # fixed point 2 of 1
        info = (C.c_double * 2)(1.0, 1.0)
        fp = (C.c_double * 4)(0, 0, 0, 0)
        assert lib.uammd_bonded_upload_f64(h, 0, 1, ids, info, 1, fp, d3(9, 9, 9), i3(1, 1, 1)) == -1
        assert b"fixed point 2, there are 1" in err()
        ids3 = (C.c_int * 3)(0, 1, -1)  # angular bonds take no fixed points
        assert lib.uammd_bonded_upload_f64(h, 2, 1, ids3, info, 1, fp, d3(9, 9, 9), i3(1, 1, 1)) == -1
        r, e, lr, wr = C.c_int(-1), C.c_int(-1), C.c_int(-1), C.c_int(-1)
        assert lib.uammd_bonded_get_shape_f64(h, C.byref(r), C.byref(e), C.byref(lr), C.byref(wr)) == 0
        assert (r.value, e.value, lr.value, wr.value) == (0, 0, 0, 0)
    finally:
        assert lib.uammd_bonded_destroy_f64(h) == 0
    assert lib.uammd_bonded_sum_f64(None, None, None, None, None, None) == -1
    assert lib.uammd_bonded_get_shape_f64(None, None, None, None, None) == -1
    v8 = C.c_void_p(8)
    assert lib.uammd_dpd_transverse_celllist_f64(None, v8, d3(9, 9, 9), i3(1, 1, 1), 1.0, 25.0, 4.5, 1.0, 1, 1, 10, v8, None, None) == -1
    assert b"null argument" in err()
    assert lib.uammd_dpd_transverse_nbody_f64(v8, v8, 10, d3(9, 9, 9), i3(1, 1, 1), 0.0, 25.0, 4.5, 1.0, 1, 1, 10, v8, None, None) == -1
    assert b"cutOff > 0" in err()
    assert lib.uammd_dpd_transverse_nbody_f64(v8, v8, 10, d3(9, 9, 9), i3(1, 1, 1), 1.0, 25.0, -1.0, 1.0, 1, 1, 10, v8, None, None) == -1
    assert lib.uammd_dpd_transverse_nbody_f64(v8, v8, 0, d3(9, 9, 9), i3(1, 1, 1), 1.0, 25.0, 4.5, 1.0, 1, 1, 0, v8, None, None) == 0   # N = 0


def test_verletlist_host_logic_under_the_sanitizers(tmp_path):
    """tests/cxx/verletlist_f64_host.cpp: rebuild decisions over every sequence of changes up to length four, the threshold rule, the
    capacity growth and a host model of fill and traversal on heap blocks of exactly the handle's buffer sizes, with
    -fsanitize=address,undefined; and the header is plain C++14."""
    exe = str(tmp_path / "verletlist_f64_host")
    r = subprocess.run(["g++", "-std=c++14", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra",
                        os.path.join(HERE, "cxx", "verletlist_f64_host.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0 and "warning" not in r.stderr, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "verletlist_f64_host: ok" in r.stdout and "ERROR" not in r.stderr and "runtime error" not in r.stderr, \
        (r.stdout[-2000:], r.stderr[-3000:])
    src = open(os.path.join(ROOT, "uammd_amd", "csrc", "verletlist_f64_host.hpp")).read()
    assert "#include <hip" not in src and "hipStream_t" not in src
