"""GPU tests of the doubly periodic Stokes solver and its integrator against the NumPy restatement
tests/dpstokes_ref.py.

Bars.  Double: 1e-10 of the largest |value| of each output (the bar of section 17).  Float: 4 x the error of the restatement run in
float32 against itself in float64 on the same input (the rule of sections 16 and 17).

Shapes, with w = 6 unless said otherwise, beta = 1.714 w, alpha = w / 2:
  A  12 x 14 x 19, (Lx, Ly, H) = (8, 9, 6): even sizes, nx != ny
  A10  shape A with w = 10: a footprint of 100 columns, so the gather's second column per lane runs (w = 6 only ever runs the first)
  B  15 x 12 x 22, (10, 8, 7): an odd size, so no unpaired index in x
  C  25 x 25 x 39, (16, 16, 16), viscosity 1 / 6 pi: the grid of the reference's periodicity test
Particles: uniform in the slab and beyond the primary cell in x and y; from four particles on, one on each wall and one within a
support of each wall.
"""
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
import dpstokes_ref as dr  # noqa: E402

pytestmark = pytest.mark.gpu

W = 6.0
SHAPES = {
    "A": dict(nx=12, ny=14, nz=19, viscosity=0.9, Lx=8.0, Ly=9.0, H=6.0),
    "B": dict(nx=15, ny=12, nz=22, viscosity=1.3, Lx=10.0, Ly=8.0, H=7.0),
    "C": dict(nx=25, ny=25, nz=39, viscosity=1 / (6 * math.pi), Lx=16.0, Ly=16.0, H=16.0),
}
SHAPES["A10"] = SHAPES["A"]
WIDTH = {"A10": 10.0}
CASES = [("A", 65, "none"), ("A", 65, "bottom"), ("A", 65, "slit"), ("B", 300, "slit"), ("B", 2, "bottom"), ("B", 1, "none"),
         ("C", 300, "slit"), ("C", 65, "bottom"), ("C", 2, "none"), ("A10", 65, "slit")]
REALS = ["double", "float"]


def _np(real):
    return np.float64 if real == "double" else np.float32


def _torch(real):
    import torch
    return torch.float64 if real == "double" else torch.float32


def particles(shape, n, seed=7):
    s = SHAPES[shape]
    rng = np.random.default_rng(seed)
    pos = np.stack([rng.uniform(-s["Lx"], s["Lx"], n), rng.uniform(-s["Ly"], s["Ly"], n), rng.uniform(-0.5 * s["H"], 0.5 * s["H"], n)], axis=1)
    force = rng.normal(0, 1, (n, 3))
    reach = 0.5 * WIDTH.get(shape, W) * min(s["Lx"] / s["nx"], s["Ly"] / s["ny"])
    if n >= 4:
        pos[0, 2], pos[1, 2] = 0.5 * s["H"], -0.5 * s["H"]
        pos[2, 2], pos[3, 2] = 0.5 * s["H"] - 0.3 * reach, -0.5 * s["H"] + 0.6 * reach
    elif n == 2:
        pos[0, 2], pos[1, 2] = 0.5 * s["H"] - 0.4 * reach, -0.5 * s["H"]
    return pos, force


def parameters(shape, mode):
    w = WIDTH.get(shape, W)
    return dr.Parameters(w=w, beta=1.714 * w, alpha=0.5 * w, mode=mode, **SHAPES[shape])


@functools.lru_cache(maxsize=None)
def reference(shape, n, mode, real):
    """One restatement run per case and precision, shared by the tests and left unchanged."""
    ref = dr.DPStokesRef(parameters(shape, mode), _np(real))
    pos, force = particles(shape, n)
    mf = ref.Mdot(pos.astype(_np(real)), force.astype(_np(real)))
    out = dict(mf=mf.astype(np.float64), fluid=ref.stage["fluid"].astype(np.complex128))
    for v in out.values():
        v.setflags(write=False)
    return out


def product(shape, mode, real, cls=None, **kw):
    import uammd_amd as hip
    cls = cls or hip.DPStokes
    w = WIDTH.get(shape, W)
    par = cls.Parameters(w=w, beta=(1.714 * w, -1.0, -1.0), alpha=0.5 * w, mode=mode, **SHAPES[shape], **kw)
    return cls(par, real=_torch(real)) if cls is hip.DPStokes else cls(None, par, real=_torch(real))


def upload(a, real, columns=None):
    import torch
    a = np.asarray(a, dtype=np.float64)
    if columns == 4:
        a = np.concatenate([a, np.zeros((len(a), 1))], axis=1)
    return torch.as_tensor(a, dtype=_torch(real), device="cuda").contiguous()


def mdot(solver, pos, force, real, columns=None):
    import torch
    out = solver.Mdot(upload(pos, real, columns), upload(force, real, columns))
    torch.cuda.synchronize()
    return out.cpu().numpy().astype(np.float64)


def bar_of(shape, n, mode, real, key, sel=slice(None)):
    want = reference(shape, n, mode, "double")[key][sel]
    big = np.abs(want).max()
    if real == "double":
        return want, 1e-10 * big, big
    return want, 4 * np.abs(reference(shape, n, mode, "float")[key][sel] - want).max(), big


# ------------------------------------------------------------------------------------------------- Mdot, fluid_cheb, average velocity
@pytest.mark.parametrize("real", REALS)
@pytest.mark.parametrize("shape,n,mode", CASES)
def test_mdot_and_fluid_against_the_restatement(shape, n, mode, real):
    solver = product(shape, mode, real)
    pos, force = particles(shape, n)
    got = mdot(solver, pos, force, real)
    want, bar, big = bar_of(shape, n, mode, real, "mf")
    err = np.abs(got - want).max()
    print(f"{shape} N={n} {mode} {real}: Mdot error {err:.3e} (bar {bar:.3e}, largest {big:.3e})")
    fluid = solver.fluid_cheb()
    assert solver.outside_count() == 0
    errs = []
    for name, sel in (("velocity", slice(0, 3)), ("pressure", slice(3, 4))):
        wantf, barf, bigf = bar_of(shape, n, mode, real, "fluid", sel)
        e = np.abs(fluid[sel] - wantf).max()
        print(f"    {name} coefficients: error {e:.3e} (bar {barf:.3e}, largest {bigf:.3e})")
        errs.append((e, barf))
    assert err <= bar
    for e, barf in errs:
        assert e <= barf
    # rows of 4 reals (the integrator's arrays) give the same bits as rows of 3
    assert np.array_equal(mdot(solver, pos, force, real, columns=4), got)


@pytest.mark.parametrize("real", REALS)
@pytest.mark.parametrize("shape,n,mode", [("A", 65, "slit"), ("B", 300, "slit"), ("C", 65, "bottom"), ("A", 65, "none")])
def test_average_velocity(shape, n, mode, real):
    import torch
    solver = product(shape, mode, real)
    pos, force = particles(shape, n)
    nz = SHAPES[shape]["nz"]
    i = np.arange(nz)
    for direction in (0, 1):
        got = solver.computeAverageVelocity(upload(pos, real), upload(force, real), direction)
        torch.cuda.synchronize()

        def profile(r):
            c = reference(shape, n, mode, r)["fluid"][direction][:, 0].real
            return np.array([np.sum(c * np.cos(i * (j * np.pi / (nz - 1)))) for j in range(nz)])
        want = profile("double")
        big = max(np.abs(want).max(), np.abs(reference(shape, n, mode, "double")["fluid"][:3]).max())
        bar = 1e-10 * big if real == "double" else 4 * np.abs(profile("float") - want).max()
        err = np.abs(got - want).max()
        print(f"{shape} {mode} {real} direction {direction}: error {err:.3e} (bar {bar:.3e}, largest {big:.3e})")
        if mode == "none":
            assert np.all(got == 0)   # the k = 0 column is zero without walls
        else:
            assert err <= bar
    with pytest.raises(RuntimeError):
        solver.computeAverageVelocity(upload(pos, real), upload(force, real), 2)


# ------------------------------------------------------------------------------------------------- the particle outside the slab
@pytest.mark.parametrize("real", REALS)
@pytest.mark.parametrize("z", ["above", "below", "nan"])
def test_particle_outside_the_slab(real, z):
    shape, n, mode = "A", 65, "slit"
    solver = product(shape, mode, real)
    pos, force = particles(shape, n)
    base = mdot(solver, pos, force, real)
    assert solver.outside_count() == 0
    H = SHAPES[shape]["H"]
    at = 30
    extra = np.array([[0.3, -0.4, {"above": 0.5 * H + 1e-3, "below": -0.5 * H - 2.0, "nan": float("nan")}[z]]])
    pos2 = np.concatenate([pos[:at], extra, pos[at:]])
    force2 = np.concatenate([force[:at], [[5.0, -6.0, 7.0]], force[at:]])   # (a larger force than any other: it must not even set the spread's scale)
    got = mdot(solver, pos2, force2, real)
    assert solver.outside_count() == 1
    assert np.all(got[at] == 0)
    assert np.array_equal(np.delete(got, at, axis=0), base)


# ------------------------------------------------------------------------------------------------- reproducibility
@pytest.mark.parametrize("real", REALS)
@pytest.mark.parametrize("shape,n,mode", [("A", 65, "slit"), ("C", 300, "slit"), ("B", 300, "slit")])
def test_same_bits_on_every_run_and_in_any_order(shape, n, mode, real):
    solver = product(shape, mode, real)
    pos, force = particles(shape, n)
    a = mdot(solver, pos, force, real)
    b = mdot(solver, pos, force, real)
    assert np.array_equal(a, b)
    c = mdot(solver, pos[::-1].copy(), force[::-1].copy(), real)
    assert np.array_equal(c[::-1], a)
    perm = np.random.default_rng(3).permutation(n)
    d = mdot(solver, pos[perm], force[perm], real)
    assert np.array_equal(d, a[perm])
    if real == "double":
        solver.set_option("simple_spread", 1)
        e = mdot(solver, pos, force, real)
        solver.set_option("simple_spread", 0)
        err = np.abs(e - a).max() / np.abs(a).max()
        print(f"{shape} N={n}: simple_spread differs by {err:.3e} of the largest velocity (bar 1e-12)")
        assert err <= 1e-12


def test_example_program():
    """examples/dpstokes_selfmobility.cpp: the self mobility against height in a slit, and one step of the integrator."""
    exe = os.path.join(ROOT, "examples", "_build", "dpstokes_selfmobility")
    assert os.path.exists(exe), "build() builds the examples"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    rows = [line.split() for line in r.stdout.splitlines() if line[:1] == " " and len(line.split()) == 3]
    assert len(rows) == 10


def test_zero_forces_give_zero():
    solver = product("A", "slit", "double")
    pos, force = particles("A", 65)
    assert np.all(mdot(solver, pos, 0 * force, "double") == 0)


# ------------------------------------------------------------------------------------------------- the integrator
def _integrator(real="double", shape="A", mode="slit", **kw):
    import uammd_amd as hip
    return product(shape, mode, real, cls=hip.DPStokesIntegrator, **kw)


@pytest.mark.parametrize("real", REALS)
def test_zero_temperature_step_is_dt_mdot(real):
    """One step moves the particles by dt Mdot to the bit."""
    import torch
    shape, n, mode, dt = "A", 65, "slit", 0.37
    pos, force = particles(shape, n)
    pos[:, 2] *= 0.9
    integ = _integrator(real, dt=dt, temperature=0.0)
    p, f = upload(pos, real, 4), upload(force, real, 4)
    p0 = p.clone()
    mf = product(shape, mode, real).Mdot(p0, f)
    integ.step_arrays(p, f)
    torch.cuda.synchronize()
    want = p0.clone()
    want[:, :3] += mf * torch.tensor(dt, dtype=_torch(real), device="cuda")
    assert torch.equal(p, want)
    assert not torch.equal(p, p0)
    assert torch.equal(integ.last("mf", n), mf)


def _thermal(n=20, **kw):
    pos, force = particles("A", n)
    pos[:, 2] *= 0.8
    return pos, force, dict(dt=0.01, temperature=1.3, tolerance=1e-7, seed=1234, seedRFD=4321, **kw)


def test_thermal_drift_against_the_restatement():
    """thermal_drift with a given W agrees with the restatement to 2 eps (T dt / delta), eps the absolute Mdot agreement measured here:
    the drift is a difference of two Mdot results scaled by T dt / delta.  eps is taken at the positions those two results are
    computed at, q + delta W / 2 and q - delta W / 2, and at q, the largest of the three."""
    pos, _, kw = _thermal()
    Wn = np.random.default_rng(11).normal(0, 1, (len(pos), 3))
    ref = dr.DPStokesRef(parameters("A", "slit"))
    for given, delta in ((-1.0, 1e-6), (1e-4, 1e-4)):   # the reference's default, and an explicit deltaRFD
        integ = _integrator(deltaRFD=given, **kw)
        eps = max(np.abs(mdot(integ.dpstokes, pos + s * delta * Wn, Wn, "double") - ref.Mdot(pos + s * delta * Wn, Wn)).max() for s in (0.0, 0.5, -0.5))
        got = integ.thermal_drift(upload(pos, "double", 4), upload(Wn, "double")).cpu().numpy()
        want = ref.thermal_drift(pos, Wn, kw["temperature"], kw["dt"], delta)
        err, bar = np.abs(got - want).max(), 2 * eps * kw["temperature"] * kw["dt"] / delta
        print(f"thermal drift, delta {delta:g}: error {err:.3e} (bar {bar:.3e}; Mdot agrees to eps = {eps:.3e}; largest drift {np.abs(want).max():.3e})")
        assert err <= bar
        assert np.abs(want).max() > 100 * bar   # (the bar means something)


def test_fluctuations_applied_twice_are_mdot():
    """M^(1/2) (M^(1/2) W) = M W to 10 x the Lanczos tolerance (1e-7), relative to the largest entry of M W."""
    pos, _, kw = _thermal()
    integ = _integrator(**kw)
    Wn = upload(np.random.default_rng(12).normal(0, 1, (len(pos), 3)), "double")
    p = upload(pos, "double", 4)
    half = integ.fluctuations(p, Wn)
    twice = integ.fluctuations(p, half).cpu().numpy()
    want = integ.dpstokes.Mdot(p, Wn).cpu().numpy()
    err = np.abs(twice - want).max() / np.abs(want).max()
    print(f"fluctuations twice against Mdot: {err:.3e} (bar {10 * kw['tolerance']:.1e})")
    assert err <= 10 * kw["tolerance"]


def _trajectory(steps, **kw):
    import torch
    pos, force, base = _thermal()
    base.update(kw)
    integ = _integrator(**base)
    p, f = upload(pos, "double", 4), upload(force, "double", 4)
    out, terms = [], []
    for _ in range(steps):
        before = p.clone()
        integ.step_arrays(p, f)
        torch.cuda.synchronize()
        out.append(p.cpu().numpy().copy())
        names = ["mf", "fluctuations", "drift"] + (["previous_fluctuations"] if base.get("useLeimkuhler") else [])
        terms.append(dict(before=before.cpu().numpy(), **{k: integ.last(k, len(pos)).cpu().numpy() for k in names}))
    return out, terms, base


def test_same_seed_same_trajectory_and_the_update_rules():
    """Two integrators with the same seeds give the same trajectory over 5 steps, bit for bit; another seed does not.  useLeimkuhler
    equals Euler-Maruyama in the first step (the previous noise is the noise) and differs from the second on; every step of either
    equals the restatement's update rule applied to the terms the step added up."""
    a, terms_a, par = _trajectory(5)
    b, _, _ = _trajectory(5)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    c, _, _ = _trajectory(1, seed=99)
    assert not np.array_equal(c[0], a[0])
    lk, terms_lk, _ = _trajectory(3, useLeimkuhler=True)
    assert np.array_equal(lk[0], a[0])
    assert not np.array_equal(lk[1], a[1])
    for got, t in zip(a, terms_a):
        want = dr.DPStokesRef.update(t["before"], t["mf"], par["dt"], noise=t["fluctuations"], rfd=t["drift"])
        assert np.array_equal(got, want)
        assert np.abs(t["fluctuations"]).max() > 0 and np.abs(t["drift"]).max() > 0
    for i, (got, t) in enumerate(zip(lk, terms_lk)):
        want = dr.DPStokesRef.update(t["before"], t["mf"], par["dt"], noise=t["fluctuations"], noise_prev=t["previous_fluctuations"], rfd=t["drift"])
        assert np.array_equal(got, want)
        if i > 0:
            assert np.array_equal(t["previous_fluctuations"], terms_lk[i - 1]["fluctuations"])


# ------------------------------------------------------------------------------------------------- the reference's own unit tests
REF_GTEST = os.path.join(ROOT, "examples", "_build", "ref_gtest_dpstokes_test")
FDB = "*ObeysFluctuationDissipationBalance*"


def _gtest(filter_, timeout):
    r = subprocess.run([REF_GTEST, f"--gtest_filter={filter_}"], capture_output=True, text=True, timeout=timeout)
    print(r.stdout[-4000:])
    assert r.returncode == 0 and "FAILED" not in r.stdout and "PASSED" in r.stdout, r.stdout[-4000:] + r.stderr[-2000:]


@pytest.mark.skipif(not os.path.exists(REF_GTEST), reason="the reference's dpstokes_test was not built (needs the reference tree at build time)")
def test_reference_unit_tests():
    """test/BDHI/DPStokes/dpstokes_test.cu compiled from where it lies against include/uammd, at the file's own tolerances."""
    _gtest("-" + FDB, 300)


@pytest.mark.skipif(not os.path.exists(REF_GTEST) or os.environ.get("UAMMD_RUN_SLOW") != "1",
                    reason="10^5 steps, minutes: UAMMD_RUN_SLOW=1 (and the reference's dpstokes_test built)")
def test_reference_fluctuation_dissipation_balance():
    _gtest(FDB, 3000)
