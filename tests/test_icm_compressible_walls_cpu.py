"""Hydro::ICM_Compressible between two walls, without a GPU: pins of the restatement tests/icm_compressible_walls_ref.py (the yardstick of
tests/test_gpu_icm_compressible_walls.py) — the Couette profile is a fixed point, a sine on top of it decays at the analytic rate, the
walls hear the reference's times and the fills use the velocities of their sub-stage — the library's host-only parameter checks, and the
C++ header under plain g++."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import icm_compressible_walls_ref as wref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = ["-I", os.path.join(ROOT, "include", "uammd"), "-I", os.path.join(ROOT, "include")]
GXX = ["g++", "-std=c++14", "-x", "c++", "-fsyntax-only", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include"] + INC

COUETTE = dict(cells=(4, 4, 16), L=(4.0, 4.0, 16.0), shear=1.3, bulk=0.7, c=4.0, dt=0.05, rho0=0.8, U=2e-2, amplitude=1e-2)


def couette(dtype, amplitude, p=COUETTE):
    """(fluid, profile, mode): bottom wall at (U, 0), top at rest, v_x = U (1 - (k + 1/2) / nz) + amplitude sin(pi (k + 1/2) / nz)"""
    walls = wref.MovingWalls(lambda t: ((p["U"], 0.0), (0.0, 0.0)), dtype)
    f = wref.WallFluid(p["cells"], p["L"], p["shear"], p["bulk"], p["c"], p["dt"], walls, 0.0, dtype)
    nz = p["cells"][2]
    k = np.arange(nz, dtype=np.float64)[:, None, None] + np.zeros(f.rho.shape)
    profile, mode = p["U"] * (1 - (k + 0.5) / nz), np.sin(np.pi * (k + 0.5) / nz)
    f.set(rho=np.full(f.rho.shape, p["rho0"]), v=[profile + amplitude * mode, 0 * mode, 0 * mode])
    return f, profile, mode


def couette_growth(p=COUETTE):
    """G = 1 + z + z^2/2 + z^3/6, z = -(eta / rho0) dt (4 / h^2) sin^2(pi / (2 nz)): the RK3 amplification of the sine, which the odd
    reflection v_ghost = 2 u - v_adj makes an exact eigenvector of the z stencil"""
    nz, h = p["cells"][2], p["L"][2] / p["cells"][2]
    z = -(p["shear"] / p["rho0"]) * p["dt"] * (4 / h ** 2) * np.sin(np.pi / (2 * nz)) ** 2
    return 1 + z + z * z / 2 + z ** 3 / 6


def test_the_couette_profile_is_a_fixed_point():
    """The ghost value 2 U - v_0 continues the line, so the discrete Laplacian vanishes.  Every step rounds v_x a few times per cell at
    eps |v_x| <= eps U: 8 eps U per step bounds the drift; everything else stays exactly what it was."""
    f, profile, _ = couette(np.float64, 0.0)
    steps = 100
    for _ in range(steps):
        f.step_fluid()
    err = np.abs(f.v[0] - profile).max()
    bound = steps * 8 * np.finfo(np.float64).eps * COUETTE["U"]
    print(f"Couette profile after {steps} steps: max |v_x - profile| = {err:.3e}, bound {bound:.3e}")
    assert err <= bound
    assert (f.rho == COUETTE["rho0"]).all() and not f.v[1].any() and not f.v[2].any()
    assert np.array_equal(f.P_v[0][0], 2 * COUETTE["U"] - f.P_v[0][1]) and np.array_equal(f.P_v[0][-1], -f.P_v[0][-2])


def test_a_sine_on_the_couette_profile_decays_at_the_analytic_rate():
    f, profile, mode = couette(np.float64, COUETTE["amplitude"])
    steps = 200
    for _ in range(steps):
        f.step_fluid()
    assert not f.v[1].any() and not f.v[2].any() and (f.rho == COUETTE["rho0"]).all()
    expect = COUETTE["amplitude"] * couette_growth() ** steps
    got = 2 * ((f.v[0] - profile) * mode).mean()
    err = abs(got / expect - 1)
    print(f"sine between the walls: amplitude {got:.15e}, analytic {expect:.15e}, relative error {err:.2e}")
    assert err <= 1e-12                                          # the figures of the periodic shear-wave pin
    assert np.abs(f.v[0] - profile - expect * mode).max() <= 1e-12 * expect


class Recording(wref.MovingWalls):
    def __init__(self, velocities):
        self.times, self.fills = [], []
        super().__init__(velocities)
        self.times.clear()

    def updateSimulationTime(self, time):
        self.times.append(time)
        super().updateSimulationTime(time)

    def __call__(self, which, rho, v, g):
        self.fills.append((which, self.times[-1] if self.times else None, tuple(float(x) for x in self.u[which])))
        return super().__call__(which, rho, v, g)


def test_the_walls_hear_the_four_times_and_the_fills_use_the_sub_stage_velocities():
    dt, steps = 0.05, 3
    walls = Recording(lambda t: ((1.0 + t, 2.0 * t), (-t, 3.0 - t)))
    f = wref.WallFluid((3, 4, 2), (3.0, 4.0, 2.0), 1.3, 0.7, 4.0, dt, walls)
    assert len(walls.fills) == 2 * 3 and all(u == ("bottom", None, (1.0, 0.0, 0.0)) or u == ("top", None, (0.0, 3.0, 0.0)) for u in walls.fills)
    walls.fills.clear()
    pos = np.array([[0.1, 0.2, 0.95], [1.0, -1.5, -0.9995]])
    for _ in range(steps):
        pos = f.forward(pos, lambda q: np.ones_like(q))
    want = [(s + frac) * dt for s in range(steps) for frac in (0.5, 1 / 3, 2 / 3, 1.0)]
    assert np.allclose(walls.times, want, rtol=1e-14, atol=0) and len(walls.times) == 4 * steps
    fills = [(s + frac) * dt for s in range(steps) for frac in (1 / 3, 2 / 3, 1.0) for _ in range(4)]     # two fills of two walls each
    assert len(walls.fills) == len(fills)
    for (which, heard, u), t in zip(walls.fills, fills):
        assert abs(heard - t) <= 1e-14 * t
        assert np.allclose(u, (1.0 + t, 2.0 * t, 0.0) if which == "bottom" else (-t, 3.0 - t, 0.0), rtol=1e-14, atol=0)
    assert [w for w, _, _ in walls.fills[:4]] == ["bottom", "top", "bottom", "top"]


def test_another_rule_can_be_stated():
    """free slip: an even continuation of a uniform tangential flow is a fixed point, whatever its speed"""
    f = wref.WallFluid((3, 4, 2), (3.0, 4.0, 2.0), 1.3, 0.7, 4.0, 0.05, wref.FreeSlipWalls())
    one = np.ones(f.rho.shape)
    f.set(rho=0.9 * one, v=[0.3 * one, -0.2 * one, 0 * one])
    for _ in range(10):
        f.step_fluid()
    assert np.abs(f.v[0] - 0.3).max() <= 1e-15 and np.abs(f.v[1] + 0.2).max() <= 1e-15 and not f.v[2].any() and (f.rho == 0.9).all()


def test_noise_is_refused_with_walls():
    with pytest.raises(ValueError, match="ghost stress"):
        wref.WallFluid((3, 4, 2), (3.0, 4.0, 2.0), 1.3, 0.7, 4.0, 0.05, wref.FreeSlipWalls(), T=0.1)


# ---- the library's host-only checks ---------------------------------------------------------------------------------------------------------
def _validate(**kw):
    from uammd_amd import _lib
    lib = _lib.load()
    p = _lib.ICMCompressibleParameters()
    assert "walls" in [f[0] for f in p._fields_], "uammd_icmc_parameters has no wall mode"
    p.boxSize[:] = [8.0, 8.0, 8.0]
    p.cells[:] = kw.pop("cells", [8, 8, 8])
    p.shearViscosity, p.bulkViscosity, p.speedOfSound, p.dt, p.hydrodynamicRadius = 1.0, 1.0, 4.0, 0.05, -1.0
    for k, v in kw.items():
        setattr(p, k, v)
    rc = lib.uammd_icmc_validate(C.byref(p))
    return rc, (lib.uammd_hip_last_error() or b"").decode()


def test_validation_refuses_noise_with_walls_and_says_why():
    rc, msg = _validate(temperature=0.1, walls=1)
    assert rc == -2 and "walls" in msg and "temperature" in msg and "never draws" in msg, msg
    assert _validate(temperature=0.0, walls=1)[0] == 0
    assert _validate(temperature=0.0, walls=2)[0] == 0 and _validate(temperature=0.1, walls=2)[0] == -2       # external walls likewise
    assert _validate(temperature=0.1, walls=0)[0] == 0
    assert _validate(temperature=0.1)[0] == 0                      # a zero-initialised mode: no walls
    rc, msg = _validate(walls=1, cells=[8, 8, 0])
    assert rc == -2 and "layer" in msg, msg
    rc, msg = _validate(walls=7)
    assert rc == -2 and "wall mode" in msg, msg


# ---- the C++ header under plain g++ ---------------------------------------------------------------------------------------------------------
def test_icmc_walls_program_passes_plain_gxx():
    r = subprocess.run(GXX + [os.path.join(ROOT, "tests", "cxx", "icmc_walls.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]


def test_a_foreign_enabled_walls_class_is_still_refused(tmp_path):
    body = ('#include "Integrator/Hydro/ICM_Compressible.cuh"\nusing namespace uammd;\n'
            "struct Mine : public Hydro::icm_compressible::MovingWalls {};\n"
            "struct Foreign : public ParameterUpdatable { static constexpr bool isEnabled() { return true; } };\n"
            "int main() { auto pd = std::make_shared<ParticleData>(0); Hydro::ICM_Compressible_impl<%s>::Parameters par;\n"
            "  Hydro::ICM_Compressible_impl<%s> icm(pd, par); return 0; }\n")
    for name, ok in (("Mine", True), ("Hydro::icm_compressible::MovingWalls", True), ("Foreign", False)):
        src = tmp_path / f"walls_{ok}_{len(name)}.cpp"
        src.write_text(body % (name, name))
        r = subprocess.run(GXX + [str(src)], capture_output=True, text=True)
        assert (r.returncode == 0) == ok, r.stderr[-3000:]
        if not ok:
            assert "walls are not supported" in r.stderr, r.stderr[-3000:]


REF = "/root/reference/test"


@pytest.mark.skipif(not os.path.isdir(REF), reason="the reference tree is not on this machine")
def test_reference_walltest_passes_the_front_end(tmp_path):
    """test/Hydro/ICM_Compressible/walltest.cu, read from where it lies with the one-token substitutions of the reference-program corpus:
    its ICMWalls is a user-written Walls class (device code), so this is the hipcc path of ICM_Compressible_impl<Walls>"""
    from test_reference_programs_compile import _source
    rel = "../test/Hydro/ICM_Compressible/walltest.cu"
    src, _ = _source(rel, tmp_path, ".hip")
    cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-fsyntax-only", "-I", os.path.join(REF, "Hydro", "ICM_Compressible")] + INC + [src]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]


def test_user_walls_program_passes_the_front_end():
    src = os.path.join(ROOT, "tests", "cxx", "icmc_walls_user.hip")
    r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-std=c++17", "-fsyntax-only"] + INC + [src], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
