"""SPH without a GPU: closed forms of the NumPy restatement (tests/sph_ref.py), the absence of undecided particles in the GPU parity
fixtures, the headers and programs through the compilers' front ends, the C entry point and the Python layer's interface."""
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import sph_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
REF = "/root/reference/examples"
PER = (True, True, True)


def _two(r, h=1.0, vel=None, mass=None, L=20.0, per=PER, K=100.0, rho0=0.4, nu=0.0, axis=0, dtype=np.float64):
    pos = np.zeros((2, 3))
    pos[1, axis] = r
    vel = np.zeros((2, 3)) if vel is None else np.asarray(vel, float)
    return sph_ref.sph_sums(pos, vel, mass, L, per, h, K, rho0, nu, dtype=dtype)


# ---- closed forms of the restatement ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h", [1.0, 2.4, 0.37])
def test_kernel_value_at_zero_and_at_the_edge(h):
    assert np.isclose(sph_ref.W([0, 0, 0], h)[0], 1.0 / (np.pi * h ** 3), rtol=1e-14)
    for q in (2.0, 2.0 + 1e-9, 2.5, 40.0):
        assert sph_ref.W([q * h, 0, 0], h)[0] == 0.0 and not sph_ref.G([0, q * h, 0], h).any()
    eps = 1e-7
    assert 0 < sph_ref.W([(2 - eps) * h, 0, 0], h)[0] < 1e-18 / h ** 3            # ~ eps^3: continuous at q = 2
    assert 0 < np.abs(sph_ref.G([(2 - eps) * h, 0, 0], h)).max() < 1e-12 / h ** 3  # ~ eps^2 q
    # W is continuous at q = 1 as well (both branches give 1 / (4 pi h^3))
    for q in (1 - 1e-9, 1 + 1e-9):
        assert np.isclose(sph_ref.W([0, 0, q * h], h)[0], 1.0 / (4 * np.pi * h ** 3), rtol=1e-7)


def test_gradient_is_the_formula_as_written():
    """inner branch c (3 r - 4 h) rij, outer c (2 h - r)^2 rij, c = -3 / (4 pi h^6): opposite signs, and a jump at q = 1"""
    h = 1.3
    c = -3.0 / (4 * np.pi * h ** 6)
    rin, rout = 0.5 * h, 1.5 * h
    assert np.allclose(sph_ref.G([rin, 0, 0], h)[0], [c * (3 * rin - 4 * h) * rin, 0, 0], rtol=1e-14)
    assert np.allclose(sph_ref.G([0, -rout, 0], h)[0], [0, -c * (2 * h - rout) ** 2 * rout, 0], rtol=1e-14)
    assert sph_ref.G([rin, 0, 0], h)[0, 0] > 0 > sph_ref.G([rout, 0, 0], h)[0, 0]
    below, above = sph_ref.G([h * (1 - 1e-12), 0, 0], h)[0, 0], sph_ref.G([h * (1 + 1e-12), 0, 0], h)[0, 0]
    assert np.isclose(below, c * (-h) * h, rtol=1e-9) and np.isclose(above, c * h * h * h, rtol=1e-9)
    assert not sph_ref.G([0, 0, 0], h).any()


def test_two_particle_density_includes_the_self_term():
    h, r = 1.0, 0.6
    w0, wr = 1 / np.pi, ((2 - r) ** 3 - 4 * (1 - r) ** 3) / (4 * np.pi)
    rho, P, F, und = _two(r, h)
    assert np.allclose(rho, w0 + wr, rtol=1e-14) and np.allclose(P, 100.0 * (w0 + wr - 0.4), rtol=1e-13) and len(und) == 0
    rho, _, _, _ = _two(r, h, mass=[2.0, 3.0])
    assert np.allclose(rho, [2 * w0 + 3 * wr, 3 * w0 + 2 * wr], rtol=1e-14)
    rho, _, F, _ = _two(2.5, h)
    assert np.allclose(rho, w0, rtol=1e-14) and not F.any()


@pytest.mark.parametrize("r,sign", [(0.6, +1), (1.6, -1)])
def test_two_particle_force_sign_in_each_branch(r, sign):
    """P > 0 on both (rho0 = 0): F_0 = m0 m1 (P0/rho0^2 + P1/rho1^2) g rij with rij = +r x; g > 0 inside q <= 1 and < 0 outside"""
    h, K = 1.0, 100.0
    rho, P, F, _ = _two(r, h, mass=[2.0, 3.0], K=K, rho0=0.0)
    c = -3 / (4 * np.pi)
    g = c * (3 * r - 4 * h) if r <= h else c * (2 * h - r) ** 2
    want = 2.0 * 3.0 * (K / rho[0] + K / rho[1]) * g * r
    assert np.isclose(F[0, 0], want, rtol=1e-13) and np.isclose(F[1, 0], -want, rtol=1e-13) and not F[:, 1:].any()
    assert np.sign(F[0, 0]) == sign


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_periodic_face_and_open_direction(axis):
    L, r = 6.0, 0.8
    direct = _two(r, L=L, axis=axis, nu=3.0, vel=[[0.1, 0.2, 0.3], [-0.3, 0.1, 0.2]])
    pos = np.zeros((2, 3))
    pos[0, axis], pos[1, axis] = 0.5 * L - 0.3, -0.5 * L + 0.5      # the same separation across the face
    vel = np.array([[0.1, 0.2, 0.3], [-0.3, 0.1, 0.2]])
    across = sph_ref.sph_sums(pos, vel, None, L, PER, 1.0, 100.0, 0.4, 3.0)
    for a, b in zip(direct[:3], across[:3]):
        assert np.allclose(a, b, rtol=1e-12, atol=1e-13)
    per = tuple(k != axis for k in range(3))
    rho, _, F, _ = sph_ref.sph_sums(pos, vel, None, L, per, 1.0, 100.0, 0.4, 3.0)
    assert np.allclose(rho, 1 / np.pi, rtol=1e-14) and not F.any()


def test_viscosity_is_odd_under_a_velocity_swap():
    r, h, nu = 0.7, 1.0, 5.0
    v = np.array([[0.3, -0.1, 0.2], [-0.2, 0.4, 0.1]])
    F0 = _two(r, h, nu=0.0)[2]
    Fa = _two(r, h, nu=nu, vel=v)[2] - F0
    Fb = _two(r, h, nu=nu, vel=v[::-1])[2] - F0
    assert np.abs(Fa).max() > 1e-3 and np.allclose(Fa, -Fb, rtol=1e-10, atol=1e-15)
    g = -3 / (4 * np.pi) * (3 * r - 4 * h)
    assert np.isclose(Fa[0, 0], -nu * ((v[1, 0] - v[0, 0]) * r) / (r * r + 0.001 * h * h) * g * r, rtol=1e-10)


@pytest.mark.parametrize("masses", [False, True])
def test_total_force_vanishes(masses):
    n, L = 1500, 8.0
    pos, vel = sph_ref.random_fluid(n, L, seed=3)
    m = sph_ref.random_masses(n, 3) if masses else None
    rho, P, F, _ = sph_ref.sph_sums(pos, vel, m, L, PER, 1.0, 100.0, 0.4, 50.0)
    assert np.abs(F.sum(0)).max() <= 1e-12 * np.abs(F).sum() and np.abs(F).max() > 1.0
    assert rho.min() >= (0.5 if masses else 1.0) / np.pi * (1 - 1e-12)


def test_float32_restatement_is_close_to_float64():
    pos, vel, m, L, per, par = sph_ref.fixture("cubic")
    a = sph_ref.sph_sums(pos, vel, m, L, per, par["h"], par["K"], par["rho0"], par["nu"])
    b = sph_ref.sph_sums(pos, vel, m, L, per, par["h"], par["K"], par["rho0"], par["nu"], dtype=np.float32)
    assert b[2].dtype == np.float32
    ef, ed = np.abs(a[2] - b[2]).max() / np.abs(a[2]).max(), np.abs(a[0] - b[0]).max() / np.abs(a[0]).max()
    print(f"float32 against float64: force {ef:.2e}, density {ed:.2e}")
    assert ef <= 2e-5 and ed <= 2e-5


def test_nve_step_of_the_restatement():
    f = lambda p, v: np.tile([2.0, 0.0, -4.0], (len(p), 1))
    p, v = sph_ref.nve_step(np.zeros((2, 4)), np.ones((2, 3)), [1.0, 2.0], 0.1, f)
    assert np.allclose(v, [[1.2, 1.0, 0.6], [1.1, 1.0, 0.8]]) and np.allclose(p[:, :3], [[0.11, 0.1, 0.08], [0.105, 0.1, 0.09]])


# ---- the GPU parity fixtures have no undecided particle -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(sph_ref.FIXTURES))
def test_parity_fixture_has_no_undecided_particle(name):
    pos, vel, m, L, per, par = sph_ref.fixture(name)
    rho, P, F, undecided = sph_ref.sph_sums(pos, vel, m, L, per, par["h"], par["K"], par["rho0"], par["nu"])
    assert len(undecided) == 0, undecided
    assert np.isfinite(F).all() and np.abs(F).max() > 0
    # (about a hundred neighbours each: the base case of the issue)
    assert 90 <= len(pos) / np.prod(np.broadcast_to(L, 3)) * (4 / 3 * np.pi * (2 * par["h"]) ** 3) <= 130


# ---- compilation -----------------------------------------------------------------------------------------------------------------------------
def test_sph_builtin_passes_plain_gxx():
    r = subprocess.run(["g++", "-std=c++14", "-fsyntax-only", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I", os.path.join(INC, "uammd"),
                        "-I", INC, os.path.join(ROOT, "tests", "cxx", "sph_builtin.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]


@pytest.mark.skipif(not os.path.isdir(REF), reason="the reference tree is not on this machine")
@pytest.mark.parametrize("rel", ["integration_schemes/others/SPH_test.cu", "misc/dambreak.cu"])
def test_reference_sph_program_compiles_with_hipcc(rel, tmp_path):
    from test_reference_programs_compile import _source
    src, _ = _source(rel, tmp_path, ".hip")
    r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-fsyntax-only", "-I", os.path.dirname(os.path.join(REF, rel)),
                        "-I", os.path.join(INC, "uammd"), "-I", INC, src], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]


def test_double_precision_is_refused_by_name(tmp_path):
    src = tmp_path / "sph_dp.cpp"
    src.write_text('#include "Interactor/SPH.cuh"\nint main() { return 0; }\n')
    r = subprocess.run(["g++", "-std=c++14", "-fsyntax-only", "-DDOUBLE_PRECISION", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                        "-I", os.path.join(INC, "uammd"), "-I", INC, str(src)], capture_output=True, text=True)
    assert r.returncode != 0 and "SPH.cuh: this module has a single-precision backend only" in r.stderr, r.stderr[-2000:]


# ---- entry point and Python layer ------------------------------------------------------------------------------------------------------------
def test_entry_point_declared_exported_and_bound():
    from uammd_amd import _lib
    from uammd_amd import build as hipbuild
    hipbuild.build()
    _lib.load()
    n = "uammd_sph_sum_verletlist"
    header = open(os.path.join(INC, "uammd_hip.h")).read()
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\b" + n + r"\s*\(", header)
    assert re.search(r" T " + n + r"\b", nm)
    assert n in _lib.SIGNATURES and len(_lib.SIGNATURES[n][1]) == 13


def test_python_layer():
    import uammd_amd as hip
    assert issubclass(hip.SPH, hip.Interactor) and hip.SPH.NeighbourList is hip.VerletList
    par = inspect.signature(hip.SPH.__init__).parameters
    assert list(par)[1:] == ["pd", "box", "support", "viscosity", "gasStiffness", "restDensity", "nl"]
    assert [par[k].default for k in list(par)[3:]] == [1.0, 50.0, 100.0, 0.4, None]
    pd = hip.ParticleData(10, device="cpu")
    box = hip.Box(10.0)
    sph = hip.SPH(hip.ParticleGroup(pd), box)            # the group of all particles is accepted
    assert sph.support == 1.0 and sph.nl is None and sph.density() is None and sph.pressure() is None
    with pytest.raises(RuntimeError, match="Not compatible with groups"):
        hip.SPH(hip.ParticleGroup(pd, [0, 1, 2]), box)
