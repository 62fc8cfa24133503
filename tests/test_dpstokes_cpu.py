"""CPU tests of the doubly periodic Stokes solver: the NumPy restatement tests/dpstokes_ref.py is pinned on facts
it did not produce, then the host-only parts of the product (the host tables under the sanitizers, the ABI, the constructor's refusals,
the C++ header and the example under g++)."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest
from numpy.polynomial import chebyshev as npcheb

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
INC = os.path.join(ROOT, "include")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
sys.path.insert(0, HERE)
import chebyshev_bvp_ref as cb  # noqa: E402
import dpstokes_ref as dr  # noqa: E402

W = 6.0
GRID = dict(nx=12, ny=14, nz=19, viscosity=0.9, Lx=8.0, Ly=9.0, H=6.0, w=W, beta=1.714 * W, alpha=0.5 * W)


def _particles(n, Lx, Ly, H, seed, zfrac=1.0):
    rng = np.random.default_rng(seed)
    pos = np.stack([rng.uniform(-Lx, Lx, n), rng.uniform(-Ly, Ly, n), rng.uniform(-0.5 * H * zfrac, 0.5 * H * zfrac, n)], axis=1)
    return pos, rng.normal(0, 1, (n, 3))


_runs = {}


def _run(mode):
    """One restatement run per mode on the same 20 particles, shared by the tests below."""
    if mode not in _runs:
        ref = dr.DPStokesRef(dr.Parameters(mode=mode, **GRID))
        pos, force = _particles(20, GRID["Lx"], GRID["Ly"], GRID["H"], 1)
        _runs[mode] = (ref, pos, force, ref.fluid(pos, force))
    return _runs[mode]


# ------------------------------------------------------------------------------------------------- 1. no-slip
@pytest.mark.parametrize("mode", ["slit", "bottom"])
def test_no_slip_at_the_walls(mode):
    """The corrected velocity, summed at a wall from its Chebyshev coefficients (T_n(1) = 1, T_n(-1) = (-1)^n), is zero for every wave
    number: at both walls in a slit, at the bottom wall above one.  Bar: 1e-12 of the largest coefficient."""
    _, _, _, sol = _run(mode)
    nz = sol.shape[1]
    top = np.abs(sol[:3].sum(axis=1)).max()
    bot = np.abs((sol[:3] * ((-1.0) ** np.arange(nz))[None, :, None]).sum(axis=1)).max()
    big = np.abs(sol[:3]).max()
    print(f"{mode}: top wall {top:.3e}, bottom wall {bot:.3e}, largest coefficient {big:.3e}")
    assert bot <= 1e-12 * big
    if mode == "slit":
        assert top <= 1e-12 * big
    else:
        assert top > 1e-3 * big  # (the fluid moves at the open top: the identity above is not vacuous)


# ------------------------------------------------------------------------------------------------- 2. the zero mode
@pytest.mark.parametrize("mode", ["slit", "bottom"])
@pytest.mark.parametrize("direction", [0, 1])
def test_average_velocity_solves_the_zero_mode_equation(mode, direction):
    """computeAverageVelocity equals the solution of mu u'' = -fbar with u = 0 at the bottom wall and u = 0 (slit) or u' = 0 (bottom) at
    the top, obtained by integrating the k = 0 Chebyshev coefficients of the spread force twice with numpy's chebint and fixing the two
    constants.  The solver works with nz coefficients, so each integral is cut at nz coefficients before the constants are fixed, and u'
    at the top is the first integral's series there: the discrete problem's own solution (what the cut leaves out is the size of the
    force's last coefficient / (4 nz^2), printed; with the derivative of the cut u instead, the bottom-wall profile moves by 1e-5)."""
    ref, pos, force, _ = _run(mode)
    nz, Hh, mu = ref.cells[2], 0.5 * GRID["H"], GRID["viscosity"]
    got = ref.average_velocity(pos, force, direction)
    f0 = ref.stage["fhat"][direction][:, 0]
    assert np.abs(f0.imag).max() <= 1e-15 * np.abs(f0.real).max()
    a = -f0.real * Hh * Hh / mu                    # d^2 u / dx^2 in x = z / (H / 2)
    d = npcheb.chebint(a)[:nz]
    d[0] = 0.0
    u = npcheb.chebint(d)[:nz]
    # u + A + B x with the boundary conditions
    ub, ut, dut = npcheb.chebval(-1.0, u), npcheb.chebval(1.0, u), npcheb.chebval(1.0, d)  # (u' is the first integral's own series)
    if mode == "slit":
        B = -(ut - ub) / 2.0
        A = -ub + B
    else:
        B = -dut
        A = -ub + B
    x = np.cos(np.pi * np.arange(nz) / (nz - 1))
    want = npcheb.chebval(x, u) + A + B * x
    tail = abs(a[nz - 1]) / (4.0 * nz * nz) / np.abs(want).max()
    err = np.abs(got - want).max() / np.abs(want).max()
    print(f"{mode} direction {direction}: relative error {err:.3e} (bar 1e-12); the cut at nz coefficients leaves out about {tail:.1e} of it")
    assert err <= 1e-12
    assert abs(want[-1]) <= 1e-13 * np.abs(want).max() and (mode == "bottom" or abs(want[0]) <= 1e-13 * np.abs(want).max())


def test_average_velocity_refuses_z():
    ref, pos, force, _ = _run("slit")
    with pytest.raises(ValueError):
        ref.average_velocity(pos, force, 2)


# ------------------------------------------------------------------------------------------------- 3. a lone particle
@pytest.mark.parametrize("mode", dr.MODES)
def test_lone_particle_moves_along_the_force(mode):
    """PulledParticleDoesNotMoveInOtherDirection (test/BDHI/DPStokes/dpstokes_test.cu:64-93): off-diagonal self-mobility entries are
    zero to 1e-13 of the diagonal, the reference test's own bar."""
    ref = _run(mode)[0]
    p = np.array([[0.3, -0.2, 0.5]])
    M = np.array([ref.Mdot(p, np.eye(3)[c:c + 1])[0] for c in range(3)])
    off = np.abs(M - np.diag(np.diag(M))).max()
    print(f"{mode}: diagonal {np.diag(M)}, largest off-diagonal entry {off:.3e}")
    assert np.all(np.diag(M) > 0) and off <= 1e-13 * np.diag(M).min()


# ------------------------------------------------------------------------------------------------- 4. periodicity
def _reference_grid(Lx, Ly, H=16.0, a=1.0):
    """getDPStokesParamtersOnlyForce (dpstokes_test.cu:37-55)."""
    h = a / 1.554
    return dr.Parameters(int(Lx / h + 0.5), int(Ly / h + 0.5), int(math.pi * H / (2 * h)), viscosity=1 / (6 * math.pi), Lx=Lx, Ly=Ly, H=H,
                         w=6.0, beta=1.714 * 6.0, alpha=3.0, mode="slit")


def test_doubling_the_box_changes_nothing():
    """PeriodicityDoubleBoxSize{X, Y}MatchesSingle (dpstokes_test.cu:337-387) with 20 particles instead of 100: the same particles
    repeated in a box twice as long give the same velocities, to the reference's 1e-3 absolute."""
    n, L = 20, 16.0
    rng = np.random.default_rng(42)
    pos = np.stack([rng.uniform(-0.5, 0.5, n) * L, rng.uniform(-0.5, 0.5, n) * L, rng.uniform(-0.5, 0.5, n) * 16.0 * 0.8], axis=1)
    force = rng.uniform(-0.5, 0.5, (n, 3))
    force -= force.mean(axis=0)
    par = _reference_grid(L, L)
    assert (par.nx, par.ny, par.nz) == (25, 25, 39)
    single = dr.DPStokesRef(par).Mdot(pos, force)
    for axis in (0, 1):
        shift = np.zeros(3)
        shift[axis] = L
        Lx, Ly = (2 * L, L) if axis == 0 else (L, 2 * L)
        double = dr.DPStokesRef(_reference_grid(Lx, Ly)).Mdot(np.concatenate([pos, pos + shift]), np.concatenate([force, force]))
        err = np.abs(double[:n] - single).max()
        print(f"doubled along {'xy'[axis]}: largest difference {err:.3e} (bar 1e-3), largest velocity {np.abs(single).max():.3e}")
        assert err <= 1e-3
        assert np.abs(double[n:] - double[:n]).max() <= 1e-3


# ------------------------------------------------------------------------------------------------- 5. host tables
def _library():
    from uammd_amd import _lib
    from uammd_amd import build as hipbuild
    hipbuild.build()
    return _lib.load(), _lib


def test_host_tables_under_the_sanitizers(tmp_path):
    """tests/cxx/dpstokes_tables.cpp, a stand-alone program over csrc/dpstokes_host.hpp, built with the address and undefined-behaviour
    sanitizers: they stay silent, and the slit inverses and the zero-mode rows match numpy to 1e-12 relative per matrix."""
    exe = str(tmp_path / "dpstokes_tables")
    r = subprocess.run(["g++", "-std=c++14", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall",
                        os.path.join(HERE, "cxx", "dpstokes_tables.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    g = GRID
    r = subprocess.run([exe] + [repr(v) for v in (g["nx"], g["ny"], g["Lx"], g["Ly"], g["viscosity"], g["H"], g["nz"])], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0 and "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    ref = dr.DPStokesRef(dr.Parameters(mode="slit", **GRID))
    want = ref.slit_inverses()
    seen, worst = 0, 0.0
    for line in r.stdout.splitlines():
        words = line.split()
        if words[0] == "inv":
            s = int(words[1])
            v = np.array(words[2:], dtype=np.float64).reshape(8, 8, 2)
            got = v[..., 0] + 1j * v[..., 1]
            err = np.abs(got - want[s]).max() / np.abs(want[s]).max()
            worst = max(worst, err)
            assert err <= 1e-12, (s, err)
            seen += 1
        elif words[0] == "zero":
            mode = {1: "bottom", 2: "slit"}[int(words[1])]
            v = np.array(words[2:], dtype=np.float64)
            f = dr.DPStokesRef(dr.Parameters(mode=mode, **GRID)).zero_mode_factors()
            t = cb.tables([0.0], 0.5 * g["H"], g["nz"], [f[0]], [f[1]], [f[2]], [f[3]])
            rows, m22 = v[:2 * g["nz"]], v[2 * g["nz"]:]
            assert np.abs(rows - t["cinvA"][:, 0]).max() <= 1e-12 * np.abs(t["cinvA"]).max()
            assert np.abs(m22 - t["m22"][:, 0]).max() <= 1e-12 * np.abs(t["m22"]).max()
            seen += 1000
        elif words[0] == "singular":
            assert words[1] == "refused"
            seen += 100000
    print(f"largest relative error of an inverse: {worst:.3e}")
    assert seen == 100000 + 2000 + g["nx"] * g["ny"] - 1


def test_shared_slab_tables_under_the_sanitizers(tmp_path):
    """tests/cxx/dp_slab_tables.cpp, a stand-alone program over csrc/dp_slab_host.hpp (the tables this solver shares with the doubly
    periodic Poisson solver), built with the address and undefined-behaviour sanitizers: they stay silent and every check of the program
    holds (the Clenshaw-Curtis weights, mirror, wave_vector against the formula it replaced, the boundary factors).  The header is
    plain C++: no HIP include."""
    header = os.path.join(ROOT, "uammd_amd", "csrc", "dp_slab_host.hpp")
    src = open(header).read()
    assert "#include <hip" not in src and "hipStream_t" not in src and "__device__" not in src
    exe = str(tmp_path / "dp_slab_tables")
    r = subprocess.run(["g++", "-std=c++14", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra",
                        "-Werror", os.path.join(HERE, "cxx", "dp_slab_tables.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout[-2000:])
    assert r.returncode == 0 and "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stdout[-3000:] + r.stderr[-3000:]
    assert "dp_slab tables ok" in r.stdout and "FAILED" not in r.stdout


# ------------------------------------------------------------------------------------------------- 6. ABI and surfaces
SYMBOLS = ["uammd_dpstokes_" + n for n in ("create", "destroy", "mdot", "average_velocity", "fluid_cheb", "outside_count", "set_option",
                                           "stage_times", "integrator_create", "integrator_destroy", "integrator_step",
                                           "integrator_thermal_drift", "integrator_fluctuations")]


def test_the_library_exports_the_new_symbols():
    lib, _ = _library()
    no_f64 = ("create", "destroy", "outside_count", "set_option", "stage_times", "integrator_create", "integrator_destroy")
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        if not name.endswith(no_f64):
            assert hasattr(lib, name + "_f64"), name + "_f64"


def _pars(hip, cls=None, **change):
    kw = dict(nx=12, ny=14, nz=19, viscosity=0.9, Lx=8.0, Ly=9.0, H=6.0, w=W, beta=(1.714 * W, -1.0, -1.0), alpha=0.5 * W, mode="slit")
    kw.update(change)
    return (cls or hip.DPStokes.Parameters)(**kw)


REFUSALS = [(dict(viscosity=0.0), "[DPStokes] Viscosity was not set"), (dict(H=0.0), "[DPStokes] H (height) was not set"),
            (dict(Lx=0.0), "[DPStokes] Domain width (Lx, Ly) was not set"), (dict(Ly=-1.0), "[DPStokes] Domain width (Lx, Ly) was not set"),
            (dict(w=17.0, alpha=8.5, nx=32, ny=32), "support = 17"), (dict(nz=3), "nz = 3")]


@pytest.mark.parametrize("change,message", REFUSALS)
def test_refusals(change, message):
    """The reference's three refusals keep its messages; a support above 16 nodes and nz < 4 have messages of their own.  The restatement
    refuses the same inputs."""
    import uammd_amd as hip
    _library()
    with pytest.raises(ValueError) as e:
        hip.DPStokes.configuration(_pars(hip, **change))
    assert message in str(e.value), str(e.value)
    with pytest.raises(ValueError):
        hip.DPStokes(_pars(hip, **change))
    kw = dict(GRID, mode="slit")
    kw.update(change)
    with pytest.raises(dr.Refusal):
        dr.DPStokesRef(dr.Parameters(**kw))


def test_configuration_matches_the_restatement():
    import uammd_amd as hip
    _library()
    info = hip.DPStokes.configuration(_pars(hip, nz=-1))
    ref = dr.DPStokesRef(dr.Parameters(**dict(GRID, nz=-1, mode="slit")))
    assert info["cells"] == ref.cells and info["support"] == ref.support == 6
    assert info["cells"][2] == int(math.pi * 6.0 / min(8.0 / 12, 9.0 / 14))
    assert info["beta"] == (1.714 * W,) * 3


def test_torques_are_refused():
    import torch
    import uammd_amd as hip
    lib, _ = _library()
    # the Python call refuses before it reads anything; so does the C call, before it touches the device
    with pytest.raises(NotImplementedError):
        hip.DPStokes.Mdot(object.__new__(hip.DPStokes), None, None, torques=torch.zeros((1, 3)))
    one = (C.c_float * 4)()
    assert lib.uammd_dpstokes_mdot(None, one, 4, one, 4, one, 1, one, None) == -3
    assert "not implemented" in lib.uammd_hip_last_error().decode()


def test_single_precision_with_temperature_needs_deltaRFD():
    """delta = 1e-6 is below the resolution of a single-precision coordinate: the float build refuses temperature > 0 unless deltaRFD is
    given, and says why; temperature = 0 and the double build's refusal-free path are decided on the host too."""
    import torch
    import uammd_amd as hip
    _library()
    P = hip.DPStokesIntegrator.Parameters
    with pytest.raises(ValueError) as e:
        hip.DPStokesIntegrator(None, _pars(hip, P, temperature=1.0, dt=0.01), real=torch.float32)
    assert "deltaRFD" in str(e.value) and "single precision" in str(e.value), str(e.value)
    with pytest.raises(ValueError) as e:   # the solver's refusals come first
        hip.DPStokesIntegrator(None, _pars(hip, P, temperature=1.0, dt=0.01, viscosity=0.0), real=torch.float64)
    assert "Viscosity" in str(e.value)


def _gxx(args):
    return subprocess.run(["g++", "-std=c++14", "-fsyntax-only", "-w", "-D__HIP_PLATFORM_AMD__", f"-I{ROCM}/include", f"-I{INC}/uammd", f"-I{INC}"] + args,
                          capture_output=True, text=True)


@pytest.mark.parametrize("extra", [[], ["-DDOUBLE_PRECISION"]])
def test_header_and_example_compile_with_gxx(extra, tmp_path):
    tu = tmp_path / "tu.cpp"
    tu.write_text('#include "Integrator/BDHI/DoublyPeriodic/DPStokesSlab.cuh"\n'
                  "using namespace uammd;\n"
                  "int use(DPStokesSlab_ns::DPStokes &s, DPStokesSlab_ns::cached_vector<real3> &v) {\n"
                  "  DPStokesSlab_ns::DPStokes::Parameters p; p.mode = DPStokesSlab_ns::WallMode::slit;\n"
                  "  DPStokesSlab_ns::DPStokesIntegrator::Parameters q; q.temperature = 0; q.useLeimkuhler = true;\n"
                  "  v[0] = {1, 2, 3}; real3 x = v[0]; auto mf = s.Mdot(v.data().get(), v.data().get(), (int)v.size());\n"
                  "  return (int)mf.size() + (int)x.x + (int)s.computeAverageVelocity(v.data().get(), v.data().get(), 1).size();\n"
                  "}\n")
    r = _gxx(extra + [str(tu)])
    assert r.returncode == 0, r.stderr[-3000:]
    r = _gxx(extra + [os.path.join(ROOT, "examples", "dpstokes_selfmobility.cpp")])
    assert r.returncode == 0, r.stderr[-3000:]
