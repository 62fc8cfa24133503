"""The C++ side of Hydro::ICM_Compressible (include/uammd/Integrator/Hydro/ICM_Compressible.cuh).

Without a GPU: the header and tests/cxx/icmc_builtin.cpp pass plain g++, a double-precision build and a Walls class with walls are refused
by name, and the two programs of the reference that use the module — examples/integration_schemes/icm.cu and integrators.cu, read from
where they lie with the one-token substitutions of tests/test_reference_programs_compile.py — pass the compiler's front end.
On the GPU: tests/cxx/icmc_builtin.cpp (built by examples/Makefile) against the Python layer on the same input, and the reference's icm.cu
(100 steps on 35^3 cells at T = 1 with 16384 particles) runs to the end."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "examples", "_build")
INC = ["-I", os.path.join(ROOT, "include", "uammd"), "-I", os.path.join(ROOT, "include")]
GXX = ["g++", "-std=c++14", "-x", "c++", "-fsyntax-only", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include"] + INC
REF = "/root/reference/examples"


def test_icmc_builtin_passes_plain_gxx():
    r = subprocess.run(GXX + [os.path.join(ROOT, "tests", "cxx", "icmc_builtin.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]


def test_double_precision_is_refused_by_name(tmp_path):
    src = tmp_path / "dp.cpp"
    src.write_text('#include "Integrator/Hydro/ICM_Compressible.cuh"\nint main() { return 0; }\n')
    r = subprocess.run(GXX + ["-DDOUBLE_PRECISION", str(src)], capture_output=True, text=True)
    assert r.returncode != 0 and "single-precision backend only" in r.stderr, r.stderr[-2000:]


def test_walls_are_refused_at_compile_time(tmp_path):
    body = ('#include "Integrator/Hydro/ICM_Compressible.cuh"\nusing namespace uammd;\n'
            "struct Walls : public ParameterUpdatable { static constexpr bool isEnabled() { return %s; } };\n"
            "int main() { auto pd = std::make_shared<ParticleData>(1); Hydro::ICM_Compressible_impl<Walls>::Parameters par;\n"
            "  Hydro::ICM_Compressible_impl<Walls> icm(pd, par); return 0; }\n")
    for enabled, ok in (("false", True), ("true", False)):
        src = tmp_path / f"walls_{enabled}.cpp"
        src.write_text(body % enabled)
        r = subprocess.run(GXX + [str(src)], capture_output=True, text=True)
        assert (r.returncode == 0) == ok, r.stderr[-3000:]
        if not ok:
            assert "walls are not supported" in r.stderr, r.stderr[-3000:]


@pytest.mark.skipif(not os.path.isdir(REF), reason="the reference tree is not on this machine")
@pytest.mark.parametrize("rel", ["integration_schemes/icm.cu", "integration_schemes/integrators.cu"])
def test_reference_program_passes_the_front_end(rel, tmp_path):
    from test_reference_programs_compile import _source
    src, _ = _source(rel, tmp_path, ".hip")
    cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-fsyntax-only", "-I", os.path.dirname(os.path.join(REF, rel))] + INC + [src]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]


@pytest.mark.gpu
def test_icmc_builtin_matches_the_python_layer():
    import math
    import torch
    import uammd_amd as hip
    exe = os.path.join(BUILD, "icmc_builtin")
    assert os.path.exists(exe), f"{exe} is not built (examples/Makefile)"
    steps, dt = 5, 0.05
    r = subprocess.run([exe, str(steps)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    lines = {l.split()[1]: l.split() for l in r.stdout.splitlines() if l.startswith("icmc ")}
    print(r.stdout.strip())
    times = [float(x) for x in lines["times"][2:6]]
    assert np.allclose(times, [0.5 * dt, dt / 3, 2 * dt / 3, dt], rtol=1e-6, atol=0)
    g = lines["grid"]
    assert [int(x) for x in g[2:5]] == [5, 7, 6] and int(g[6]) == 210 and int(g[8]) == 7 * 9 * 8 and int(g[10]) == 1 and int(g[12]) == 1
    # the same input through the Python layer: the same library calls on the same numbers (the spreading's atomics may add in another order)
    N = 64
    i = np.arange(N)
    pos = np.stack([(i % 4) * 1.1 - 1.9, ((i // 4) % 4) * 1.7 - 2.3, (i // 16) * 1.3 - 2.1, i % 3], 1).astype(np.float32)
    F = np.stack([(i % 7 - 3) / 4.0, (i % 5 - 2) / 3.0, (i % 3 - 1) / 2.0], 1).astype(np.float32)
    pd = hip.ParticleData(N)
    pd.setPos(pos)

    class Constant:
        def __init__(self):
            self.F = torch.from_numpy(F).cuda()

        def sum(self, force=False, energy=False, virial=False):
            pd.getForce("readwrite")[:, :3] += self.F

        def updateSimulationTime(self, t): pass

    par = hip.Hydro.ICM_Compressible.Parameters(
        shearViscosity=1.3, bulkViscosity=0.7, speedOfSound=4.0, dt=dt, boxSize=[5.0, 7.0, 6.0], cellDim=[5, 7, 6], seed=77,
        initialDensity=lambda r: 1 + 0.05 * math.sin(2 * math.pi * r[0] / 5), initialVelocityX=lambda r: 0.05 * math.sin(2 * math.pi * r[1] / 7),
        initialVelocityZ=lambda r: 0.02 * math.cos(2 * math.pi * r[0] / 5))
    icm = hip.Hydro.ICM_Compressible(pd, par)
    icm.addInteractor(Constant())
    for _ in range(steps):
        icm.forwardTime()
    torch.cuda.synchronize()
    w = (np.arange(210) % 17 + 1).astype(np.float64)
    rho = icm.getCurrentDensity().cpu().numpy().astype(np.float64).ravel()
    v = icm.getCurrentVelocity().cpu().numpy().astype(np.float64).reshape(3, -1)
    mom = icm.getMomentum().cpu().numpy().astype(np.float64).reshape(3, -1)
    q = pd.getPos("read").cpu().numpy().astype(np.float64)
    d = lines["density"]
    got = [float(d[2])] + [float(x) for x in d[4:7]] + [float(x) for x in d[8:11]] + [float(x) for x in d[12:15]]
    wq = (i % 17 + 1).astype(np.float64)
    mine = [(w * rho).sum()] + [(w * c).sum() for c in v] + [(w * c).sum() for c in mom] + [(wq * q[:, c]).sum() for c in range(3)]
    scale = [np.abs(w * rho).sum()] + [np.abs(w * c).sum() for c in v] + [np.abs(w * c).sum() for c in mom] + [np.abs(wq[:, None] * q[:, :3]).sum()] * 3
    for name, a, b, s in zip("rho vx vy vz gx gy gz qx qy qz".split(), got, mine, scale):
        print(f"{name}: program {a:.9g}, python layer {b:.9g}")
        assert abs(a - b) <= 2e-6 * s, name


@pytest.mark.gpu
def test_reference_icm_example_runs():
    exe = os.path.join(BUILD, "ref_icm")
    if not os.path.exists(exe):
        pytest.skip("ref_icm was not built (no reference tree where `make -C examples` ran)")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "Fluid cells: 35 35 35" in r.stdout + r.stderr or "fluid cells: 35 35 35" in r.stdout + r.stderr
