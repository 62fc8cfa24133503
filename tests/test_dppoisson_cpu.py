"""CPU tests of the doubly periodic Poisson slab solver: the NumPy restatement tests/dppoisson_ref.py is pinned on
answers it did not produce, then the host-only parts of the product (the constructor's decisions and refusals through the C ABI, the C++
header under g++, the reference's programs under the compiler's front end)."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
INC = os.path.join(ROOT, "include")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
REF = "/root/reference"
sys.path.insert(0, HERE)
import dppoisson_ref as dr  # noqa: E402

INF = float("inf")


# ------------------------------------------------------------------------------------------------- 1. the reference's own known answer
def _quadrupole(L, probes=40):
    d = 0.08
    ref = dr.DPPoissonSlabRef(dr.Parameters((L, L), 5.0, 0.2 * math.sqrt(2.0 / 3.0), split=1.70103))
    pos = np.zeros((4 + probes, 3))
    q = np.zeros(4 + probes)
    pos[0, 0], pos[3, 0] = -d, d
    q[:4] = [1, -1, -1, 1]
    pos[4:, 0] = 1.5 + np.arange(probes) / probes * 2.5
    fp = ref.field_potential(pos, q)
    x = pos[4:, 0]
    eE = np.abs(fp[4:, 0] - 2 / (4 * np.pi) * 3 * d * d / x ** 4).max()
    eP = np.abs(fp[4:, 3] - 2 / (4 * np.pi) * d * d / x ** 3).max()
    print(f"quadrupole L = {L}: |Ex - theory| {eE:.3e} (bar 1e-5), |phi - theory| {eP:.3e} (bar 1e-4)")
    assert eE < 1e-5 and eP < 1e-4


def test_quadrupole():
    """test/Potentials/Poisson/DoublyPeriodic/test_dp_quadrupole.cu with Lxy = 25 (the nearest periodic image adds about 2e-8)."""
    _quadrupole(25.0)


@pytest.mark.skipif(os.environ.get("UAMMD_RUN_SLOW") != "1", reason="the reference's Lxy = 50 takes a minute: UAMMD_RUN_SLOW=1")
def test_quadrupole_at_the_reference_size():
    _quadrupole(50.0)


# ------------------------------------------------------------------------------------------------- 2. wall potentials
def _charges(n, Lxy, H, seed, zfrac=1.0):
    rng = np.random.default_rng(seed)
    pos = np.stack([rng.uniform(-0.5 * Lxy[0], 0.5 * Lxy[0], n), rng.uniform(-0.5 * Lxy[1], 0.5 * Lxy[1], n),
                    rng.uniform(-0.5 * H * zfrac, 0.5 * H * zfrac, n)], axis=1)
    q = rng.normal(0, 1, n)
    return pos, q - q.mean()


def _wall_potential_runs(Lxy=(8.0, 7.0), **window):
    """Two runs on the same 20 charges (two of them exactly on the walls) between metallic walls: grounded, and at (V_t, V_b)."""
    H, Vt, Vb = 4.0, 0.7, -0.2
    par = dr.Parameters(Lxy, H, 0.2, split=1.2, permitivity=(INF, INF, 1.7), tolerance=1e-3, **window)
    pos, q = _charges(20, Lxy, H, 1)
    pos[0, 2], pos[1, 2] = 0.5 * H, -0.5 * H
    a = dr.DPPoissonSlabRef(par)
    b = dr.DPPoissonSlabRef(par)
    b.set_surface_zero_mode(Vt, Vb)
    return a, a.far_field(pos, q), b, b.far_field(pos, q), -(Vt - Vb) / H, pos, q, par


def test_wall_potentials_add_a_uniform_field():
    """The field with wall potentials (V_t, V_b) minus the field with (0, 0) is (0, 0, -(V_t - V_b) / H) at every particle, to 1e-12
    relative: the k = 0 correction is linear and exact.  A particle reads the grid through the truncated Gaussian window, so the identity
    can only hold to the window's own quadrature: the parameters are chosen so that this lies below the bar — support 32 at upsampling 2
    cuts the window at 8 standard deviations (3 erfc(8 / sqrt 2) = 4e-15), numberStandardDeviations 6.5 puts the edge of the correction,
    H/2 + He, 8.1 standard deviations beyond a charge on a wall, and upsampling 2 resolves the window for the Clenshaw-Curtis sum in z.
    Measured 5.3e-14.  (With the defaults, support 12 at upsampling 1.2 = 5 standard deviations, the same difference is off by
    3 erfc(5 / sqrt 2) = 1.7e-6: next test.)"""
    _, a, _, b, expect, _, _, _ = _wall_potential_runs((9.0, 8.0), upsampling=2.0, support=32, numberStandardDeviations=6.5)
    dev = np.abs((b - a)[:, :3] - np.array([0, 0, expect])).max()
    print(f"wall potentials: largest deviation from (0, 0, {expect}) is {dev:.3e}")
    assert dev <= 1e-12 * abs(expect)


def test_wall_potentials_add_a_uniform_field_on_the_grid():
    """The same with the default window (support 12, upsampling 1.2): 1e-12 on the planes inside the slab, before the gather, and at the
    particles within the window's own quadrature deficit, 3 erfc(5 / sqrt 2) = 1.72e-6 (bar: twice that)."""
    ra, a, rb, b, expect, pos, q, par = _wall_potential_runs()
    diff = rb.stage["field_grid"] - ra.stage["field_grid"]
    slab = np.abs(ra.zplane) <= 0.5 * par.H   # (between a wall and H/2 + He the rounding of the walls' spectra grows like exp(k He): 2e-10 here)
    assert np.abs(diff[2][slab] - expect).max() <= 1e-12 * abs(expect)
    assert np.abs(diff[:2][:, slab]).max() <= 1e-12 * abs(expect)
    assert np.abs(diff[2][np.abs(ra.zplane) >= 0.5 * par.H + ra.He]).max() <= 1e-12 * abs(expect)
    deficit = 3 * math.erfc(5 / math.sqrt(2))
    dev = np.abs((b - a)[:, :3] - np.array([0, 0, expect])).max()
    assert dev <= 2 * deficit * abs(expect)
    # the same with the walls' values sampled at the nodes instead of set as the k = 0 entries
    c = dr.DPPoissonSlabRef(par, surface_top=lambda x, y: 0.7, surface_bottom=lambda x, y: -0.2)
    assert np.abs(c.far_field(pos, q) - b).max() <= 1e-12 * abs(expect)   # (their spectra's rounding at k != 0 grows like exp(k He) beyond the walls, where a window's weight is below 4e-6)


# ------------------------------------------------------------------------------------------------- 3. one dielectric interface
def _pair_field(r, gw, eps):
    """-d/dr [erf(r / 2 gw) / (4 pi eps r)]: the field between two Gaussian charges of width gw."""
    return (math.erf(r / (2 * gw)) / (r * r) - math.exp(-r * r / (4 * gw * gw)) / (r * gw * math.sqrt(math.pi))) / (4 * math.pi * eps)


def _image_lattice_sum(pos, q, i, zwall, ratio, Lxy, gw, eps, rng_cells):
    """Ez at charge i from the images of every charge in the wall at zwall, and of their periodic copies within rng_cells cells."""
    total = 0.0
    for j in range(len(q)):
        zi = 2 * zwall - pos[j, 2]
        for m in range(-rng_cells, rng_cells + 1):
            for n in range(-rng_cells, rng_cells + 1):
                dx, dy, dz = pos[i, 0] - pos[j, 0] - m * Lxy[0], pos[i, 1] - pos[j, 1] - n * Lxy[1], pos[i, 2] - zi
                r = math.sqrt(dx * dx + dy * dy + dz * dz)
                total += -q[j] * ratio * _pair_field(r, gw, eps) * dz / r
    return total


def test_one_dielectric_interface_against_the_image_sum():
    Lxy, H, gw, tol = (8.0, 7.0), 4.0, 0.2, 1e-3
    eps_in, eps_b = 1.7, 0.3
    mk = lambda eb: dr.DPPoissonSlabRef(dr.Parameters(Lxy, H, gw, split=1.2, permitivity=(eps_in, eb, eps_in), tolerance=tol))  # noqa: E731
    ref = mk(eps_b)
    d = 1.0
    half_diag = 0.5 * math.hypot(ref.h, ref.hy)
    c = half_diag / math.sqrt(2)
    pos = np.array([[0.13, -0.21, -0.5 * H + d], [0.13 + c, -0.21 + c, -0.5 * H + d]])
    q = np.array([0.9, -0.9])
    with_wall, without = ref.field_potential(pos, q), mk(eps_in).field_potential(pos, q)
    got = (with_wall - without)[:, 2]
    bar = 10 * tol * np.abs(with_wall[:, 2]).max()
    ratio = (eps_b - eps_in) / (eps_b + eps_in)
    cells = 8
    while True:
        want = np.array([_image_lattice_sum(pos, q, i, -0.5 * H, ratio, Lxy, gw, eps_in, cells) for i in range(2)])
        wider = np.array([_image_lattice_sum(pos, q, i, -0.5 * H, ratio, Lxy, gw, eps_in, 2 * cells) for i in range(2)])
        if np.abs(wider - want).max() < bar / 10:
            break
        cells *= 2
    err = np.abs(got - wider).max()
    print(f"one interface: Ez from the wall {got}, image sum {wider} ({2 * cells} cells), error {err:.3e}, bar {bar:.3e}")
    assert err <= bar


# ------------------------------------------------------------------------------------------------- 4. split independence
SPLIT_WALLS = {"uniform": ((1.0, 1.0, 1.0), True), "metal_top": ((INF, 0.3, 1.7), False), "metal_both": ((INF, INF, 1.7), False),
               "dielectric": ((2.5, 0.3, 1.7), True)}


@pytest.mark.parametrize("wall", list(SPLIT_WALLS))
def test_split_independence(wall):
    """The same 50 charges at split 1.0 and 1.4: the same field and potential within 10 x tolerance x the largest value.  Between two walls that are not metallic (a dielectric jump, or none)
    nothing fixes the zero of the potential (the k = 0 line has B0 = 0 and the boundary value problem pins phi = 0 at the
    ends of a domain whose height depends on split; the reference warns that it does not subtract phi(0, 0, 0)): there the potentials are
    compared up to their mean difference, 2.8e-3 here, which a neutral system's energy does not see."""
    Lxy, H, gw, tol = (8.0, 7.0), 4.0, 0.2, 1e-3
    eps, gauge_free = SPLIT_WALLS[wall]
    pos, q = _charges(50, Lxy, H, 2, zfrac=0.9)
    top = (lambda x, y: 0.7) if math.isinf(eps[0]) else None
    bottom = (lambda x, y: -0.2) if math.isinf(eps[1]) else None
    out = [dr.DPPoissonSlabRef(dr.Parameters(Lxy, H, gw, split=s, permitivity=eps, tolerance=tol), surface_top=top,
                               surface_bottom=bottom).field_potential(pos, q) for s in (1.0, 1.4)]
    diff = out[0] - out[1]
    if gauge_free:
        diff[:, 3] -= diff[:, 3].mean()
    for cols, what in ((slice(0, 3), "E"), (slice(3, 4), "phi")):
        scale = np.abs(out[0][:, cols]).max()
        err = np.abs(diff[:, cols]).max()
        print(f"{wall}: split 1.0 against 1.4, {what}: {err:.3e}, bar {10 * tol * scale:.3e}")
        assert err <= 10 * tol * scale


# ------------------------------------------------------------------------------------------------- 5. construction
def _cpar(Lxy, H, gw, split=-1.0, Nxy=-1, eps=(1.0, 1.0, 1.0), tol=1e-4):
    from uammd_amd._lib import DPPoissonParameters
    p = DPPoissonParameters()
    p.Lxy[0], p.Lxy[1] = Lxy
    p.H, p.gw, p.split, p.Nxy = H, gw, split, Nxy
    for k in range(3):
        p.permitivity[k] = eps[k]
    p.tolerance, p.upsampling, p.support, p.numberStandardDeviations = tol, 1.2, 12, 4.0
    return p


def _configure(p, double=1):
    from uammd_amd import _lib
    from uammd_amd import build as hipbuild
    hipbuild.build()
    lib = _lib.load()
    info = _lib.DPPoissonInfo()
    e = lib.uammd_dppoisson_create(C.byref(p), double, None, C.byref(info))
    return e, info, (lib.uammd_hip_last_error().decode() if e else "")


def test_reference_configurations():
    """The two configurations of the reference's tests.  The second one's plane is 176 x 176: the grid rule only keeps sizes with a factor of
    two (utils/Grid.cuh:179-181), so it steps over 175 = 5^2 7."""
    e, i, _ = _configure(_cpar((50.0, 50.0), 5.0, 0.163299, split=1.70103))
    assert e == 0 and list(i.cells) == [180, 180, 85] and abs(i.He - 1.681) < 1e-3 and i.nTable == 65536
    want = dr.DPPoissonSlabRef(dr.Parameters((50.0, 50.0), 5.0, 0.163299, split=1.70103)).info()
    assert abs(i.nearFieldCutOff - want["nearFieldCutOff"]) < 1e-12 and abs(i.gt - want["gt"]) < 1e-15 and i.supportZ == want["supportZ"]
    e, i, _ = _configure(_cpar((100.0, 100.0), 10.0, 0.2, split=0.75, tol=1e-7))
    assert e == 0 and list(i.cells) == [176, 176, 85] and abs(i.nearFieldCutOff - 6.536) < 1e-3 and i.nTable == 1 << 20
    want = dr.DPPoissonSlabRef(dr.Parameters((100.0, 100.0), 10.0, 0.2, split=0.75, tolerance=1e-7)).info()
    assert tuple(i.cells) == want["cells"] and abs(i.nearFieldCutOff - want["nearFieldCutOff"]) < 1e-12 and i.nTable == want["nTable"]
    # float and double builds differ in kmax only
    e, f, _ = _configure(_cpar((100.0, 100.0), 10.0, 0.2, split=0.75, tol=1e-7), double=0)
    assert e == 0 and f.kmax == min(88.0 / f.He, math.pi / f.h) and i.kmax == min(709.0 / i.He, math.pi / i.h)


REFUSALS = [
    (dict(split=-1.0), "Missing input parameters"),
    (dict(split=1.2, Nxy=20), "Invalid input parameters"),
    (dict(split=0.1), "Invalid splitting parameter"),
    (dict(split=5.0), "Invalid splitting parameter"),
    (dict(split=1.2, eps=(1.0, INF, 1.0)), "[DPPoissonSlab] Bottom metallic wall not implemented"),
    (dict(split=1.2, Lxy=(2.0, 7.0)), "[DPPoissonSlab] Incompatible parameters"),
    (dict(split=1.3, H=2.4), "[DPPoissonSlab] Incompatible parameters"),
]


@pytest.mark.parametrize("change,message", REFUSALS)
def test_refusals_carry_the_reference_message(change, message):
    kw = dict(Lxy=(8.0, 7.0), H=4.0, gw=0.2, tol=1e-3)
    kw.update(change)
    e, _, msg = _configure(_cpar(**kw))
    assert e != 0 and msg.startswith(message), msg
    # the restatement refuses the same input, and the Python layer turns the refusal into a ValueError
    with pytest.raises(ValueError):
        dr.DPPoissonSlabRef(dr.Parameters(kw["Lxy"], kw["H"], kw["gw"], split=kw.get("split", -1.0), Nxy=kw.get("Nxy", -1),
                                          permitivity=kw.get("eps", (1.0, 1.0, 1.0)), tolerance=kw["tol"]))
    import uammd_amd as hip
    P = hip.DPPoissonSlab
    with pytest.raises(ValueError):
        P.configuration(P.Parameters(Lxy=kw["Lxy"], H=kw["H"], gw=kw["gw"], split=kw.get("split", -1.0), Nxy=kw.get("Nxy", -1),
                                     permitivity=P.Permitivity(*kw.get("eps", (1.0, 1.0, 1.0))), tolerance=kw["tol"]))


def test_split_from_nxy_on_the_host():
    e, i, _ = _configure(_cpar((8.0, 7.0), 4.0, 0.2, Nxy=20, tol=1e-3))
    gt = 1.2 * 8.0 / 20
    assert e == 0 and abs(i.split - math.sqrt(1 / (4 * (gt * gt - 0.04)))) < 1e-14 and abs(i.gt - gt) < 1e-14


# ------------------------------------------------------------------------------------------------- 6. programs
CXX_PROGRAM = os.path.join(ROOT, "tests", "cxx", "dppoisson_builtin.cpp")


@pytest.mark.parametrize("extra", [[], ["-DDOUBLE_PRECISION"]])
def test_builtin_program_compiles_with_gxx(extra):
    r = subprocess.run(["g++", "-std=c++14", "-fsyntax-only", "-w", "-D__HIP_PLATFORM_AMD__", f"-I{ROCM}/include", f"-I{INC}/uammd"] + extra + [CXX_PROGRAM],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]


def test_host_only_part_under_the_sanitizers(tmp_path):
    """The program's host-only mode, built as a stand-alone program with the address and undefined-behaviour sanitizers, and run."""
    from uammd_amd import _lib
    from uammd_amd import build as hipbuild
    hipbuild.build()
    exe = str(tmp_path / "dppoisson_host_asan")
    libdir = os.path.dirname(_lib.LIB_PATH)
    r = subprocess.run(["g++", "-std=c++14", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-w", "-D__HIP_PLATFORM_AMD__",
                        f"-I{ROCM}/include", f"-I{INC}/uammd", CXX_PROGRAM, "-o", exe, f"-L{libdir}", "-luammd_hip", f"-L{ROCM}/lib", "-lamdhip64",
                        f"-Wl,-rpath,{libdir}", f"-Wl,-rpath,{ROCM}/lib"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    r = subprocess.run([exe, "host"], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0 and "FAIL" not in r.stdout and "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stdout + r.stderr[-3000:]
    assert r.stdout.count("ok  ") == 9


@pytest.mark.skipif(not os.path.isdir(REF), reason="the reference tree is not on this machine")
@pytest.mark.parametrize("rel,extra", [("examples/interaction_modules/DoublyPeriodicPoisson.cu", []),
                                       ("examples/interaction_modules/DoublyPeriodicPoisson.cu", ["-DDOUBLE_PRECISION"]),
                                       ("test/Potentials/Poisson/DoublyPeriodic/test_dp_quadrupole.cu", ["-DDOUBLE_PRECISION", "-DMAXLOGLEVEL=1"]),
                                       ("test/Potentials/Poisson/DoublyPeriodic/test_dp_quadrupole.cu", ["-DMAXLOGLEVEL=1"])])
def test_reference_programs_pass_the_front_end(rel, extra, tmp_path):
    src = os.path.join(REF, rel)
    text = open(src).read()
    for a, b in (("cudaStream_t", "hipStream_t"), ("thrust::cuda::par", "thrust::hip::par"), ("cudaDeviceSynchronize", "hipDeviceSynchronize")):
        text = text.replace(a, b)
    tmp = tmp_path / "program.hip"
    tmp.write_text(text)
    r = subprocess.run([f"{ROCM}/bin/hipcc", "--offload-arch=gfx950", "-std=c++17", "-fsyntax-only", "-w"] + extra +
                       [f"-I{os.path.dirname(src)}", f"-I{REF}/test/Potentials/Poisson/common", f"-I{ROOT}/tests/cxx/gtest_lite", f"-I{INC}/uammd", f"-I{INC}",
                        str(tmp)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
