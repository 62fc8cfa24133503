"""GPU tests of the doubly periodic Poisson slab solver against the NumPy restatement tests/dppoisson_ref.py.

Bars.  Double: 1e-10 of the largest |value| of each output (the bar of the triply periodic solver's double build in
tests/test_gpu_f64.py).  Float: 4 x the error of the restatement run in float32 against itself in float64 on the same input, capped at
1e-3 of the largest |value|; the cap is a condition: the float32 restatement alone must stay below a quarter of it.

Shapes (each constructs, and 2 rcut <= min(Lx, Ly)):
  A  Lxy (8, 7), H 4, gw 0.2,  split 1.2, tol 1e-3 -> 20 x 18 x 73,  rcut 3.31 >= H/2: the opposite-side image is taken
  B  Lxy (9, 7), H 6, gw 0.15, split 1.8, tol 1e-4 -> 36 x 30 x 97,  rcut 2.53 <  H/2
  C  Lxy (6, 6), H 6, gw 0.1,  split 2.8, tol 1e-3 -> 36 x 36 x 113, 2 He = 2.05 < H/2: the only one with charges FAR from both walls
(the reference's grid rule only yields even plane sizes, utils/Grid.cuh:179-181, so no shape has an odd one).
"""
import ctypes as C
import functools
import math
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import dppoisson_ref as dr  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = {
    "A": dict(Lxy=(8.0, 7.0), H=4.0, gw=0.2, split=1.2, tolerance=1e-3),
    "B": dict(Lxy=(9.0, 7.0), H=6.0, gw=0.15, split=1.8, tolerance=1e-4),
    "C": dict(Lxy=(6.0, 6.0), H=6.0, gw=0.1, split=2.8, tolerance=1e-3),
}
INF = float("inf")
# name -> (top, bottom, inside), surface values (top, bottom) as callables of (x, y, Lx) or None
WALLS = {
    "uniform": ((1.0, 1.0, 1.0), None),
    "dielectric": ((2.5, 0.3, 1.7), (lambda x, y, Lx: 0.1 * math.cos(2 * math.pi * x / Lx), lambda x, y, Lx: -0.05)),
    "metal_top": ((INF, 0.3, 1.7), (lambda x, y, Lx: 0.7, lambda x, y, Lx: 0.0)),
    "metal_both": ((INF, INF, 1.7), (lambda x, y, Lx: 0.7, lambda x, y, Lx: -0.2)),
}
CASES = [("A", w) for w in WALLS] + [("B", w) for w in WALLS] + [("C", "uniform"), ("C", "dielectric")]
REALS = ["double", "float"]


def _np(real):
    return np.float64 if real == "double" else np.float32


def _torch(real):
    import torch
    return torch.float64 if real == "double" else torch.float32


def particles(shape, n=300, seed=5, zmax=None):
    """n random charges, neutral: two exactly on the walls, one pair at the same position, the rest uniform in the slab."""
    s = SHAPES[shape]
    rng = np.random.default_rng(seed)
    pos = np.zeros((n, 3))
    pos[:, 0] = rng.uniform(-0.5 * s["Lxy"][0], 0.5 * s["Lxy"][0], n)
    pos[:, 1] = rng.uniform(-0.5 * s["Lxy"][1], 0.5 * s["Lxy"][1], n)
    zm = 0.5 * s["H"] if zmax is None else zmax
    pos[:, 2] = rng.uniform(-zm, zm, n)
    q = rng.normal(0, 1, n)
    if n >= 8 and zmax is None:
        pos[0, 2], pos[1, 2] = 0.5 * s["H"], -0.5 * s["H"]
        pos[3] = pos[2]
        pos[4, 2], pos[5, 2] = 0.01, -0.02   # the middle
    if n > 1:
        q -= q.mean()
    return pos, q


@functools.lru_cache(maxsize=None)
def reference(shape, wall, real, n=300, seed=5, zmax=None):
    s = SHAPES[shape]
    eps, surf = WALLS[wall]
    par = dr.Parameters(s["Lxy"], s["H"], s["gw"], split=s["split"], permitivity=eps, tolerance=s["tolerance"])
    Lx = s["Lxy"][0]
    top = bottom = None
    if surf is not None:
        top, bottom = (lambda x, y: surf[0](x, y, Lx)), (lambda x, y: surf[1](x, y, Lx))
    ref = dr.DPPoissonSlabRef(par, _np(real), top, bottom)
    pos, q = particles(shape, n, seed, zmax)
    far = ref.far_field(pos, q)
    out = dict(ref=ref, far=far, near=ref.near_field(pos, q), stage={k: np.array(v) for k, v in ref.stage.items()}, outside=ref.outside_count)
    out["total"] = out["far"] + out["near"]
    return out


def product(shape, wall, real, **kw):
    import uammd_amd as hip
    s = SHAPES[shape]
    eps, surf = WALLS[wall]
    P = hip.DPPoissonSlab
    par = P.Parameters(Lxy=s["Lxy"], H=s["H"], gw=s["gw"], split=s["split"], tolerance=s["tolerance"],
                       permitivity=P.Permitivity(*eps))
    par.__dict__.update(kw)
    if surf is not None:
        Lx = s["Lxy"][0]

        class Surf(P.SurfaceValueDispatch):
            def top(self, x, y):
                return surf[0](x, y, Lx)

            def bottom(self, x, y):
                return surf[1](x, y, Lx)
        par.surfaceValues = Surf()
    return P(None, par, real=_torch(real))


def upload(pos, q, real):
    import torch
    p4 = np.zeros((len(q), 4))
    p4[:, :3] = pos
    return (torch.as_tensor(p4, dtype=_torch(real), device="cuda").contiguous(),
            torch.as_tensor(np.asarray(q), dtype=_torch(real), device="cuda").contiguous())


def run(slab, pos, q, real):
    import torch
    p, c = upload(pos, q, real)
    force = torch.zeros((len(q), 4), dtype=_torch(real), device="cuda")
    force[:, 3] = 7.0
    energy = torch.zeros((len(q),), dtype=_torch(real), device="cuda")
    fp = slab.field_potential_arrays(p, c, force, energy)
    torch.cuda.synchronize()
    return fp.cpu().numpy().astype(np.float64), force.cpu().numpy().astype(np.float64), energy.cpu().numpy().astype(np.float64)


def bars(shape, wall, real, key, pick=lambda d, k: d[k], n=300, seed=5, zmax=None):
    """(reference values, bar per entry) for one output of the restatement."""
    r64 = pick(reference(shape, wall, "double", n, seed, zmax), key)
    scale = np.abs(r64).max()
    if real == "double":
        return r64, 1e-10 * scale
    r32 = pick(reference(shape, wall, "float", n, seed, zmax), key).astype(r64.dtype)
    own = np.abs(r32 - r64).max()
    cap = 1e-3 * scale
    assert own <= cap / 4, f"the float32 restatement alone is off by {own:.3e}, more than a quarter of the cap {cap:.3e}"
    return r64, min(4 * own, cap)


def close(got, want, bar, what):
    err = np.abs(np.asarray(got) - np.asarray(want)).max()
    print(f"{what}: max error {err:.3e}, bar {bar:.3e}, largest value {np.abs(want).max():.3e}")
    assert err <= bar, f"{what}: {err:.3e} > {bar:.3e}"


def field_close(got, shape, wall, real, what, **kw):
    """E (three components against the largest |E|) and phi, each against its own bar."""
    want, barE = bars(shape, wall, real, "total", lambda d, k: d[k][:, :3], **kw)
    close(got[:, :3], want, barE, what + " E")
    want, barP = bars(shape, wall, real, "total", lambda d, k: d[k][:, 3], **kw)
    close(got[:, 3], want, barP, what + " phi")
    return barE, barP


# --------------------------------------------------------------------------------------------------------------------- configuration
@pytest.mark.parametrize("shape", list(SHAPES))
def test_info_matches_restatement(shape):
    import uammd_amd as hip
    s = SHAPES[shape]
    P = hip.DPPoissonSlab
    for real in REALS:
        got = P.configuration(P.Parameters(Lxy=s["Lxy"], H=s["H"], gw=s["gw"], split=s["split"], tolerance=s["tolerance"]), _torch(real))
        want = dr.DPPoissonSlabRef(dr.Parameters(s["Lxy"], s["H"], s["gw"], split=s["split"], tolerance=s["tolerance"]), _np(real)).info()
        for k in ("cells", "support", "supportZ", "nTable"):
            assert got[k] == want[k], (k, got[k], want[k])
        for k in ("He", "gt", "h", "nearFieldCutOff", "kmax", "split"):
            assert abs(got[k] - want[k]) <= 1e-12 * abs(want[k]), (k, got[k], want[k])
        assert 2 * got["nearFieldCutOff"] <= min(s["Lxy"])


# --------------------------------------------------------------------------------------------------------------------- stages
@pytest.mark.parametrize("real", REALS)
@pytest.mark.parametrize("shape,wall", [("A", "dielectric"), ("B", "metal_top"), ("C", "dielectric")])
def test_stages(shape, wall, real):
    slab = product(shape, wall, real)
    slab.set_option("keep_stages", 1)
    pos, q = particles(shape)
    run(slab, pos, q, real)
    for name in ("grid_near", "grid_all"):
        want, bar = bars(shape, wall, real, name, lambda d, k: d["stage"][k])
        close(slab.get_stage(name).cpu().numpy(), want, bar, f"{shape} {wall} {real} {name}")
    m = slab.get_stage("mismatch").cpu().numpy().astype(np.float64)
    m = m[:, 0] + 1j * m[:, 1]
    nsys = slab.cells[0] * slab.cells[1]
    # potentials and fields have their own scales: (mP0, mPH), (mE0, mEH), then the k = 0 line
    for lo, hi, what in ((0, 2 * nsys, "mismatch potential"), (2 * nsys, 4 * nsys, "mismatch field"), (4 * nsys, 4 * nsys + 2, "linear mode")):
        want, bar = bars(shape, wall, real, "mismatch", lambda d, k: d["stage"][k][lo:hi])
        close(m[lo:hi], want, bar, f"{shape} {wall} {real} {what}")


# --------------------------------------------------------------------------------------------------------------------- sum and field
@pytest.mark.parametrize("real", REALS)
@pytest.mark.parametrize("shape,wall", CASES)
def test_field_potential_and_sum(shape, wall, real):
    import torch
    slab = product(shape, wall, real)
    pos, q = particles(shape)
    fp, force, energy = run(slab, pos, q, real)
    barE, barP = field_close(fp, shape, wall, real, f"{shape} {wall} {real}")
    qmax = np.abs(q).max()
    assert np.all(force[:, 3] == 7.0), "force.w was touched"
    close(force[:, :3], q[:, None] * fp[:, :3], barE * qmax, "force = q E")
    close(energy, q * fp[:, 3], barP * qmax, "energy = q phi")
    assert slab.outside_count() == 0
    # sum: the same increments; twice adds twice
    p, c = upload(pos, q, real)
    f2 = torch.zeros((len(q), 4), dtype=_torch(real), device="cuda")
    e2 = torch.zeros((len(q),), dtype=_torch(real), device="cuda")
    slab.sum_arrays(p, c, f2, e2)
    once = f2.cpu().numpy().astype(np.float64)
    close(once[:, :3], force[:, :3], barE * qmax, "sum against the field call")
    slab.sum_arrays(p, c, f2, e2)
    close(f2.cpu().numpy()[:, :3], 2 * once[:, :3], barE * qmax, "twice adds twice")
    close(e2.cpu().numpy(), 2 * energy, barP * qmax, "twice adds twice (energy)")


@pytest.mark.parametrize("real", REALS)
@pytest.mark.parametrize("shape,wall", [("A", "metal_top"), ("C", "dielectric")])
def test_simple_spread_agrees(shape, wall, real):
    pos, q = particles(shape)
    a = product(shape, wall, real)
    fa, _, _ = run(a, pos, q, real)
    b = product(shape, wall, real)
    b.set_option("simple_spread", 1)
    fb, _, _ = run(b, pos, q, real)
    for cols, what in ((slice(0, 3), "E"), (slice(3, 4), "phi")):
        if real == "double":
            bar = 1e-12 * np.abs(fa[:, cols]).max()
        else:
            _, bar = bars(shape, wall, real, "total", lambda d, k: d[k][:, cols])
        close(fb[:, cols], fa[:, cols], bar, f"simple_spread {what}")


def test_other_stream_same_bits():
    import torch
    pos, q = particles("B")
    slab = product("B", "dielectric", "double")
    a, fa, ea = run(slab, pos, q, "double")
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        b, fb, eb = run(slab, pos, q, "double")
    st.synchronize()
    assert np.array_equal(a, b) and np.array_equal(fa, fb) and np.array_equal(ea, eb)


# --------------------------------------------------------------------------------------------------------------------- edge cases
def test_no_particles():
    import torch
    slab = product("A", "uniform", "float")
    p = torch.zeros((0, 4), dtype=torch.float32, device="cuda")
    c = torch.zeros((0,), dtype=torch.float32, device="cuda")
    slab.sum_arrays(p, c, p.clone(), c.clone())
    assert slab.field_potential_arrays(p, c).shape == (0, 4)


@pytest.mark.parametrize("real", REALS)
def test_one_particle(real):
    pos, q = particles("A", n=1, seed=9)
    q[0] = 0.8
    fp, _, _ = run(product("A", "dielectric", real), pos, q, real)
    want64 = _single("A", "dielectric", "double", pos, q)
    scale = np.abs(want64).max(axis=0)
    if real == "double":
        bar = 1e-10 * np.array([scale[:3].max()] * 3 + [scale[3]])
    else:
        own = np.abs(_single("A", "dielectric", "float", pos, q) - want64)
        cap = 1e-3 * np.array([scale[:3].max()] * 3 + [scale[3]])
        assert np.all(own.max(axis=0) <= cap / 4)
        bar = np.minimum(4 * np.array([own[:, :3].max()] * 3 + [own[:, 3].max()]), cap)
    err = np.abs(fp - want64).max(axis=0)
    print("one particle:", err, bar)
    assert np.all(err <= bar)


def _single(shape, wall, real, pos, q):
    s = SHAPES[shape]
    eps, surf = WALLS[wall]
    Lx = s["Lxy"][0]
    ref = dr.DPPoissonSlabRef(dr.Parameters(s["Lxy"], s["H"], s["gw"], split=s["split"], permitivity=eps, tolerance=s["tolerance"]), _np(real),
                              (lambda x, y: surf[0](x, y, Lx)) if surf else None, (lambda x, y: surf[1](x, y, Lx)) if surf else None)
    return ref.field_potential(pos, q).astype(np.float64)


@pytest.mark.parametrize("real", REALS)
def test_none_near_a_wall(real):
    """Shape C with every charge in |z| < 0.9: nothing lies within 2 He of a wall, the near-wall grid and both image lists are empty.
    (In shapes A and B every charge lies within 2 He of a wall: the far list is empty in every test on them.)"""
    pos, q = particles("C", n=60, seed=11, zmax=0.9)
    slab = product("C", "dielectric", real)
    slab.set_option("keep_stages", 1)
    fp, _, _ = run(slab, pos, q, real)
    assert np.abs(slab.get_stage("grid_near").cpu().numpy()).max() == 0.0
    field_close(fp, "C", "dielectric", real, f"none near a wall {real}", n=60, seed=11, zmax=0.9)


def test_split_from_nxy():
    import uammd_amd as hip
    import torch
    P = hip.DPPoissonSlab
    s = SHAPES["A"]
    par = P.Parameters(Lxy=s["Lxy"], H=s["H"], gw=s["gw"], Nxy=20, tolerance=s["tolerance"])
    got = P(None, par, real=torch.float64).info
    gt = 1.2 * 8.0 / 20
    assert abs(got["split"] - math.sqrt(1 / (4 * (gt * gt - 0.04)))) < 1e-14
    want = dr.DPPoissonSlabRef(dr.Parameters(s["Lxy"], s["H"], s["gw"], Nxy=20, tolerance=s["tolerance"])).info()
    assert got["cells"] == want["cells"] and abs(got["nearFieldCutOff"] - want["nearFieldCutOff"]) < 1e-12


def test_particles_outside_the_slab():
    pos, q = particles("B")
    slab = product("B", "dielectric", "double")
    base, fbase, ebase = run(slab, pos, q, "double")
    extra = np.array([[0.3, 0.2, 3.0 + 1e-9], [1.0, -2.0, -17.0], [-4.0, 3.0, 1e30]])
    at = [10, 150, 302]
    pos2, q2 = pos.copy(), q.copy()
    for a, e in zip(at, extra):
        pos2 = np.insert(pos2, a, e, axis=0)
        q2 = np.insert(q2, a, 1.5)
    got, fgot, egot = run(slab, pos2, q2, "double")
    assert slab.outside_count() == 3
    keep = np.ones(len(q2), bool)
    keep[at] = False
    assert np.all(got[~keep] == 0) and np.all(fgot[~keep][:, :3] == 0) and np.all(egot[~keep] == 0)
    assert np.array_equal(got[keep], base) and np.array_equal(fgot[keep], fbase) and np.array_equal(egot[keep], ebase)


# --------------------------------------------------------------------------------------------------------------------- known answers
def _gaussian_pair_field(r, gw):
    """|E| between two Gaussian charges of width gw, unit charges, free space: -d/dr [erf(r / 2 gw) / (4 pi r)]."""
    return math.erf(r / (2 * gw)) / (4 * math.pi * r * r) - math.exp(-r * r / (4 * gw * gw)) / (4 * math.pi * r * gw * math.sqrt(math.pi))


@pytest.mark.parametrize("H,what", [(10.0, "force"), (20.0, "field")])
def test_three_charges_single_simulation(H, what):
    """The reference's SingleSimulationTest pair (test/Potentials/Poisson/DoublyPeriodic/test_poisson.cu:202-235) with the origin inside the slab.
    Measured (MI355X, double): F = (1.989364e-2, -2.5e-18, -9.4e-10), E = (1.989363e-2, -1.9e-19, -2.1e-10) against the free-space Gaussian
    pair field 1.989437e-2: 3.7e-5 relative.  |E_z| = 2.1e-10 is above the reference's 1e-10, which it writes signed."""
    import torch
    import uammd_amd as hip
    P = hip.DPPoissonSlab
    L, r, tol, gw = 100.0, 2.0, 1e-7, 0.2
    rng = np.random.default_rng(3 if what == "force" else 4)
    ori = np.array([rng.uniform(-0.5, 0.5) * L, rng.uniform(-0.5, 0.5) * L, rng.uniform(-1, 1) * (0.5 * H - 1)])
    pos = np.array([[-0.5 * r, 0, 0], [0.5 * r, 0, 0], [0.5 * r, 0, 0]]) + ori
    q = np.array([1.0, -0.5, -0.5])
    slab = P(None, P.Parameters(Lxy=(L, L), H=H, gw=gw, split=0.75, tolerance=tol), real=torch.float64)
    fp, force, _ = run(slab, pos, q, "double")
    expect = _gaussian_pair_field(r, gw)
    if what == "force":
        print("F =", force[0, :3], "free space", expect)
        assert force[0, 1] < tol and force[0, 2] < tol and force[0, 0] > 0   # as the reference writes them (test_poisson.cu:211-213): signed
        assert abs(force[0, 1]) < tol and abs(force[0, 2]) < tol
        assert abs(force[0, 0] - expect) <= 1e-3 * expect
    else:
        print("E =", fp[0, :3], "free space", expect)
        assert fp[0, 1] < 1e-10 and fp[0, 2] < 1e-10   # as the reference writes them (test_poisson.cu:225-226): signed
        # In magnitude |E_z| = 2.1e-10 does NOT meet 1e-10: the signed form holds here only by its sign.  What the algorithm promises for
        # a component that vanishes by symmetry is the quadrature deficit of its window, truncated at 5 standard deviations, on the
        # field's terms: 3 erfc(5 / sqrt 2) = 1.7e-6 of |E|
        window = 3 * math.erfc(5 / math.sqrt(2))
        assert abs(fp[0, 1]) <= window * abs(fp[0, 0]) and abs(fp[0, 2]) <= window * abs(fp[0, 0])
        assert abs(fp[0, 0] - expect) <= 1e-3 * expect


def test_stage_times():
    """The per-stage device timing tools/time_dppoisson.py reads: refused unless asked for, thirteen times, the near field's 0 when skipped."""
    import uammd_amd as hip
    from uammd_amd import _lib
    pos, q = particles("A")
    slab = product("A", "uniform", "float")
    run(slab, pos, q, "float")
    with pytest.raises(_lib.UammdHipError, match="time_stages"):
        slab.stage_times()
    slab.set_option("time_stages", 1)
    base, _, _ = run(slab, pos, q, "float")
    t = slab.stage_times()
    assert list(t) == list(hip.DPPoissonSlab.STAGES) and len(t) == 13 and all(v > 0 for v in t.values())
    slab.set_option("skip_near_field", 1)
    run(slab, pos, q, "float")
    t = slab.stage_times()
    assert t["near field"] == 0 and t["cell list + pack"] == 0 and t["gather"] > 0
    slab.set_option("skip_near_field", 0)
    again, _, _ = run(slab, pos, q, "float")
    assert np.array_equal(base, again)   # timing changes no result


# --------------------------------------------------------------------------------------------------------------------- error paths
def test_error_paths_launch_nothing():
    import torch
    import uammd_amd as hip
    from uammd_amd import _lib
    lib = _lib.load()
    slab = product("A", "uniform", "float")
    pos, q = particles("A")
    p, c = upload(pos, q, "float")
    f = torch.zeros((len(q), 4), dtype=torch.float32, device="cuda")
    e = torch.zeros((len(q),), dtype=torch.float32, device="cuda")
    vp = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    assert lib.uammd_dppoisson_sum(slab.h, vp(p), None, len(q), vp(f), vp(e), 0, None) != 0
    assert b"null" in lib.uammd_hip_last_error()
    assert lib.uammd_dppoisson_sum_f64(slab.h, vp(p), vp(c), len(q), vp(f), vp(e), 0, None) != 0
    assert b"single precision" in lib.uammd_hip_last_error()
    assert lib.uammd_dppoisson_sum(slab.h, vp(p), vp(c), len(q), vp(f), vp(e), 1, None) != 0
    assert b"not implemented" in lib.uammd_hip_last_error()
    with pytest.raises(RuntimeError, match="not implemented"):
        hip.DPPoissonSlab.sum(slab, virial=True)
    torch.cuda.synchronize()
    assert float(f.abs().max()) == 0.0 and float(e.abs().max()) == 0.0


# --------------------------------------------------------------------------------------------------------------------- programs
@pytest.mark.parametrize("name", ["dppoisson_builtin", "dppoisson_builtin_dp"])
def test_builtin_program(name):
    exe = os.path.join(ROOT, "examples", "_build", name)
    assert os.path.exists(exe), f"{exe} was not built"
    res = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(res.stdout[-2000:], res.stderr[-2000:])
    assert res.returncode == 0


def test_reference_quadrupole_unit_test():
    exe = os.path.join(ROOT, "examples", "_build", "ref_gtest_dppoisson_test_dp_quadrupole")
    if not os.path.exists(exe):
        pytest.skip("the reference's unit test was not built (the reference tree was absent at build time)")
    res = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(res.stdout[-3000:], res.stderr[-2000:])
    assert res.returncode == 0 and "[  PASSED  ] 1 test" in res.stdout
