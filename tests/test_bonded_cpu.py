"""BondedForces on the host, no GPU: the CSR rows of a bond set (uammd_bonded_build_rows, host logic only) against a restatement of the
reference's BondProcessor / buildBondList, the bond-file reader's errors, and the reference's bonded programs through the front end."""
import os
import re
import subprocess

import numpy as np
import pytest

from bonded_ref import rows_restated

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "bonds")


def _rows(ids, m):
    from uammd_amd.bonded import build_rows
    return build_rows(np.asarray(ids, np.int32), m)


def _check(ids, m):
    got = _rows(ids, m)
    want = rows_restated(ids, m)
    for g, w in zip(got, want):
        assert np.array_equal(g, w), (got, want)
    return got


def test_rows_per_particle_order_and_repeated_members():
    # particle 1 is in three bonds, listed in registration (file) order; rows in ascending id whatever the file order
    ids = [[5, 1], [1, 2], [3, 1], [2, 5]]
    rid, rs, eb = _check(ids, 2)
    assert list(rid) == [1, 2, 3, 5]
    assert list(eb[rs[0]:rs[1]]) == [0, 1, 2]


def test_rows_fixed_points_register_nothing():
    from uammd_amd.bonded import read_bond_file
    path = os.path.join(GOLD, "harmonic.bonds")
    ids, info, fp = read_bond_file(path, 2)
    assert ids.shape == (3, 2) and fp.shape == (0, 4) and np.allclose(info, [[10, 2]] * 3)
    ids = np.array([[0, 1], [1, 2], [4, -1], [1, -2]], np.int32)
    rid, rs, eb = _check(ids, 2)
    assert list(rid) == [0, 1, 2, 4] and list(eb[rs[1]:rs[2]]) == [0, 1, 3]


def test_rows_zero_count_block_then_fixed_points(tmp_path):
    from uammd_amd.bonded import read_bond_file
    f = tmp_path / "fp.bonds"
    f.write_text("0\n2\n3 1.0 2.0 3.0 5 0.5\n0 -1 0 0 7 0.25\n")
    ids, info, fp = read_bond_file(str(f), 2)
    assert ids.tolist() == [[3, -1], [0, -2]]
    assert np.allclose(info, [[5, 0.5], [7, 0.25]]) and np.allclose(fp, [[1, 2, 3, 0], [-1, 0, 0, 0]])
    rid, rs, eb = _check(ids, 2)
    assert list(rid) == [0, 3] and list(eb) == [1, 0]


@pytest.mark.parametrize("m", [2, 3, 4])
def test_rows_random_sets(m):
    rng = np.random.default_rng(m)
    ids = rng.integers(0, 50, (400, m))
    _check(ids, m)
    rid, rs, eb = _rows(ids, m)
    assert rs[-1] == ids.size


def test_python_reader_errors(tmp_path):
    from uammd_amd.bonded import read_bond_file
    with pytest.raises(RuntimeError, match="cannot be opened"):
        read_bond_file(str(tmp_path / "missing.bonds"), 2)
    f = tmp_path / "short.bonds"
    f.write_text("3\n0 1 1 1\n1 2 1 1\n")
    with pytest.raises(OSError, match="too soon"):
        read_bond_file(str(f), 2)


def _gxx(src, out, extra=()):
    cmd = ["g++", "-std=c++14", "-O1", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I", os.path.join(ROOT, "include", "uammd"), *extra, src,
           "-o", out, "-L", os.path.join(ROOT, "uammd_amd", "lib"), "-luammd_hip", "-L/opt/rocm/lib", "-lamdhip64",
           "-Wl,-rpath," + os.path.join(ROOT, "uammd_amd", "lib"), "-Wl,-rpath,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]


def test_cxx_reader_errors(tmp_path):
    """the C++ reader raises the reference's exceptions: std::runtime_error for a file that cannot be opened, std::ios_base::failure
    for one that ends before its count (BondedForces.cu:83-107,141-145).  Host code only: runs without a GPU."""
    from uammd_amd import build as hipbuild
    hipbuild.build()
    exe = str(tmp_path / "bonds_builtin")
    _gxx(os.path.join(ROOT, "tests", "cxx", "bonds_builtin.cpp"), exe)
    short = tmp_path / "short.bonds"
    short.write_text("2\n0 1 1 1\n")
    r = subprocess.run([exe, "errors", str(short)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "missing: runtime_error" in r.stdout and "short: ios_base::failure" in r.stdout, r.stdout


@pytest.mark.parametrize("hdr", ["Interactor/BondedForces.cuh", "Interactor/AngularBondedForces.cuh", "Interactor/TorsionalBondedForces.cuh"])
def test_headers_plain_cxx14_and_single_precision_only(hdr, tmp_path):
    src = tmp_path / "t.cpp"
    src.write_text(f'#include "{hdr}"\nint main() {{ return 0; }}\n')
    base = ["g++", "-std=c++14", "-fsyntax-only", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I", os.path.join(ROOT, "include", "uammd")]
    r = subprocess.run(base + [str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run(base + ["-DDOUBLE_PRECISION", str(src)], capture_output=True, text=True)
    assert r.returncode != 0 and "single-precision backend only" in r.stderr


REF = "/root/reference"


@pytest.mark.skipif(not os.path.isdir(REF), reason="the reference tree is not on this machine")
@pytest.mark.parametrize("rel", ["examples/interaction_modules/Bonds.cu", "test/Bonds/Bonds.cu"])
def test_reference_bond_programs_compile(rel, tmp_path):
    """the reference's bonded programs pass hipcc's front end against include/uammd, read from where they lie with the one-token
    substitutions of INTEGRATION.md §2.7b (nothing copied).  test/Bonds/{AngularBond,TorsionalBonds}.cu are out of scope: they call a
    constructor (pd, sys, params, ...) with `readFile` that the reference's own BondedForces no longer has."""
    text = open(os.path.join(REF, rel)).read()
    for pat, rep in ((r"\bcudaStream_t\b", "hipStream_t"), (r"thrust::cuda::par\b", "thrust::hip::par"),
                     (r"\bcudaDeviceSynchronize\b", "hipDeviceSynchronize"), (r"\bcudaStreamCreate\b", "hipStreamCreate"),
                     (r"\bcudaStreamDestroy\b", "hipStreamDestroy")):
        text = re.sub(pat, rep, text)
    src = tmp_path / "prog.hip"
    src.write_text(text)
    cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-fsyntax-only", "-I", os.path.join(ROOT, "include", "uammd"),
           "-I", os.path.join(ROOT, "include"), str(src)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
