"""CPU tests of Potential::DPD and VerletNVE: the user programs of tests/cxx compile (plain g++ for the built-in potential, hipcc for a
dissipation functor of the user's), the float64 restatement in tests/dpd_ref.py reproduces closed forms, and the new entry points are
declared, exported and bound.  No GPU."""
import os
import re
import subprocess

import numpy as np

import dpd_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")


def _run(cmd):
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, " ".join(cmd) + "\n" + r.stderr[-3000:]


def test_builtin_program_compiles_with_plain_gxx():
    _run(["g++", "-std=c++14", "-fsyntax-only", "-w", "-D__HIP_PLATFORM_AMD__", f"-I{ROCM}/include", f"-I{INC}/uammd",
          os.path.join(ROOT, "tests", "cxx", "dpd_builtin.cpp")])


def test_user_dissipation_program_compiles_with_hipcc():
    _run([f"{ROCM}/bin/hipcc", "--offload-arch=gfx950", "-std=c++17", "-fsyntax-only", "-w", f"-I{INC}/uammd", f"-I{INC}",
          os.path.join(ROOT, "tests", "cxx", "dpd_user.hip")])


def test_double_precision_is_refused():
    for header in ("Integrator/VerletNVE.cuh", "Interactor/Potential/DPD.cuh"):
        r = subprocess.run(["g++", "-std=c++14", "-fsyntax-only", "-DDOUBLE_PRECISION", "-D__HIP_PLATFORM_AMD__", f"-I{ROCM}/include",
                            f"-I{INC}/uammd", "-x", "c++", "-include", header, "/dev/null"], capture_output=True, text=True)
        assert r.returncode != 0 and "single-precision backend only" in r.stderr, header


def test_conservative_force_closed_form():
    """gamma = 0, kT = 0: |F| = A (1 - r/rc) along rij, opposite on the partner; nothing at or beyond the cut-off."""
    for r in (0.1, 0.5, 0.999):
        pos = np.array([[0.2, 0.0, 0.0], [0.2 + r, 0.0, 0.0]])
        F = dpd_ref.dpd_forces(pos, np.zeros((2, 3)), 10.0, (True,) * 3, 1.0, 25.0, 0.0, 0.0, 0.01)
        assert np.allclose(F[0], [-25.0 * (1 - r), 0, 0], rtol=1e-12, atol=1e-12)
        assert np.allclose(F[1], -F[0])
    pos = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0]])
    assert not dpd_ref.dpd_forces(pos, np.zeros((2, 3)), 10.0, (True,) * 3, 1.0, 25.0, 0.0, 0.0, 0.01).any()
    # across the periodic boundary
    pos = np.array([[-4.9, 0.0, 0.0], [4.8, 0.0, 0.0]])
    F = dpd_ref.dpd_forces(pos, np.zeros((2, 3)), 10.0, (True,) * 3, 1.0, 25.0, 0.0, 0.0, 0.01)
    assert np.allclose(F[0], [25.0 * (1 - 0.3), 0, 0], rtol=1e-9)
    assert not dpd_ref.dpd_forces(pos, np.zeros((2, 3)), 10.0, (False, True, True), 1.0, 25.0, 0.0, 0.0, 0.01).any()


def test_dissipative_force_closed_form():
    """A = 0, kT = 0: two particles approaching head-on feel -gamma wr^2 (rhat . v) rhat."""
    r, g, v = 0.6, 4.5, 0.7
    rhat = np.array([1.0, 2.0, -2.0]) / 3.0
    pos = np.array([r * rhat, np.zeros(3)])
    vel = np.array([-v * rhat, v * rhat])           # vij = -2 v rhat: approaching
    F = dpd_ref.dpd_forces(pos, vel, 10.0, (True,) * 3, 1.0, 0.0, g, 0.0, 0.01)
    want = -g * (1 - r) ** 2 * (-2 * v) * rhat      # repels the approaching particle
    assert np.allclose(F[0], want, rtol=1e-12) and np.allclose(F[1], -want, rtol=1e-12)
    assert np.dot(F[0], rhat) > 0


def test_random_force_scaling_and_symmetry():
    """kT on, A = gamma-term isolated: Fr = xi sigma sqrt(gamma) wr / r rij with the pair's own Gaussian, and sum F = 0 on a random fluid."""
    xi = lambda k: np.full(len(k), 0.5)
    pos = np.array([[0.0, 0.0, 0.0], [0.0, 0.4, 0.0]])
    F = dpd_ref.dpd_forces(pos, np.zeros((2, 3)), 10.0, (True,) * 3, 1.0, 0.0, 4.0, 2.0, 0.01, xi=xi)
    assert np.allclose(F[1], [0, 0.5 * np.sqrt(2 * 2.0) / np.sqrt(0.01) * 2.0 * 0.6, 0], rtol=1e-12)
    rng = np.random.default_rng(5)
    n, L = 1500, (1500 / 3.0) ** (1 / 3.0)
    pos = rng.uniform(-L / 2, L / 2, (n, 3))
    vel = rng.normal(0, 1, (n, 3))
    F = dpd_ref.dpd_forces(pos, vel, L, (True,) * 3, 1.0, 25.0, 4.5, 1.0, 0.01, xi=lambda k: rng.standard_normal(len(k)))
    assert np.abs(F.sum(0)).max() <= 1e-12 * np.abs(F).sum()
    assert np.abs(F).max() > 1.0


def test_pair_key_wraps_like_unsigned():
    assert dpd_ref.pair_keys(np.array([7]), np.array([3]), 10)[0] == 3 + 10 * 7
    assert dpd_ref.pair_keys(np.array([99999]), np.array([99998]), 100000)[0] == (99998 + 100000 * 99999) % 2 ** 32


def test_nve_half_steps():
    pos, vel, f = np.zeros((1, 3)), np.array([[1.0, 0.0, 2.0]]), np.array([[2.0, 4.0, 0.0, 9.0]])
    p1, v1 = dpd_ref.nve_half(pos, vel, f, [2.0], 0.1, 1)
    assert np.allclose(v1, [[1.05, 0.1, 2.0]]) and np.allclose(p1, 0.1 * v1)
    p2, v2 = dpd_ref.nve_half(pos, vel, f, [2.0], 0.1, 2, is2D=True)
    assert np.allclose(v2, [[1.05, 0.1, 0.0]]) and not p2.any()


def test_entry_points_declared_exported_and_bound():
    from uammd_amd import _lib
    from uammd_amd import build as hipbuild
    hipbuild.build()
    _lib.load()
    names = {"uammd_dpd_transverse_celllist", "uammd_dpd_transverse_nbody", "uammd_verletnve"}
    header = open(os.path.join(INC, "uammd_hip.h")).read()
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for n in names:
        assert re.search(r"\b" + n + r"\s*\(", header), n
        assert re.search(r" T " + n + r"\b", nm), n
        assert n in _lib.SIGNATURES, n


def test_python_layer_exports():
    import uammd_amd as hip
    assert hip.Potential.DPD is hip.DPD and callable(hip.VerletNVE)
    pot = hip.Potential.DPD(cutOff=1.0, dt=0.01, gamma=4.5, temperature=1.0, A=25.0)
    s0 = pot.sigma
    assert abs(s0 - np.sqrt(2.0) / 0.1) < 1e-5 and pot.getCutOff() == 1.0
    pot.updateTimeStep(0.04)
    assert abs(pot.sigma - s0 / 2) < 1e-5
    pot.updateTemperature(4.0)
    assert abs(pot.sigma - s0) < 1e-5
