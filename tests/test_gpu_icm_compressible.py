"""Hydro::ICM_Compressible on the GPU (uammd_amd/csrc/icm_compressible.hip) through the Python layer on the C ABI, against the NumPy
restatement in tests/icm_compressible_ref.py.

PARITY BOUND.  For every compared field, the GPU's maximum error against the FLOAT64 restatement, relative to the field's maximum, may be
at most 4 x the same error of the FLOAT32 restatement (computed here, on the same inputs).  The float32 restatement performs the kernel's
operations in the kernel's order without FMA; the factor 4 leaves room for another summation order (the particle sums, the atomics of
the spreading) and for the explicit FMAs of the window.  On the CPU the float32 error after 20 steps is 7e-7 to 1.6e-5, and a 1 % change
of the bulk viscosity shows at 1e-3 or more."""
import json
import os

import numpy as np
import pytest
import torch

import icm_compressible_ref as ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -24
GRIDS = [(5, 7, 6), (70, 9, 5), (32, 32, 32)]        # odd with every wrap inside a three-cell window; a partial tile in x; a cube
PAR = dict(shear=1.3, bulk=0.7, c=4.0, dt=0.05)


def _hip():
    import uammd_amd as hip
    return hip


def _make(cells, h=1.0, T=0.0, N=0, seed=1234, par=PAR):
    """the integrator and the two restatements (float64, float32) of one configuration"""
    hip = _hip()
    L = [c * h for c in cells]
    pd = hip.ParticleData(N)
    p = hip.Hydro.ICM_Compressible.Parameters(shearViscosity=par["shear"], bulkViscosity=par["bulk"], speedOfSound=par["c"], temperature=T,
                                              dt=par["dt"], boxSize=L, cellDim=cells, seed=seed)
    icm = hip.Hydro.ICM_Compressible(pd, p)
    refs = [ref.Fluid(cells, L, par["shear"], par["bulk"], par["c"], par["dt"], T, ty) for ty in (np.float64, np.float32)]
    return pd, icm, refs


def _set(icm, refs, rho, v):
    """the same float32 numbers on the three sides"""
    rho = np.asarray(rho, np.float32)
    v = [np.asarray(c, np.float32) for c in v]
    icm.setFluid(*[torch.from_numpy(np.ascontiguousarray(a)) for a in (rho, *v)])
    for f in refs:
        f.set(rho=rho, v=v)


def _smooth(f, drho=0.05, dv=0.05):
    x, y, z = [2 * np.pi * c.astype(np.float64) / l for c, l in zip(f.centers(), f.L.astype(np.float64))]
    rho = 1 + drho * np.sin(x + 0.3) * np.cos(y - 0.2) * np.cos(z + 0.1)
    v = [dv * np.sin(y + 0.5) * np.cos(z), dv * np.cos(x + 0.4) * np.sin(z - 0.3), dv * np.sin(x - 0.1) * np.sin(y + 0.2)]
    return rho, v


def _state(icm):
    torch.cuda.synchronize()
    rho = icm.getCurrentDensity().cpu().numpy().astype(np.float64)
    g = icm.getMomentum().cpu().numpy().astype(np.float64)
    v = icm.getCurrentVelocity(collocated=False).cpu().numpy().astype(np.float64)
    return rho, g, v


def _bound(what, got, r64, r32):
    """prints the two errors and asserts the parity bound"""
    got, r64, r32 = [np.asarray(a, np.float64) for a in (got, r64, r32)]
    scale = np.abs(r64).max()
    if scale == 0:
        assert not got.any(), what
        return
    eg, e32 = np.abs(got - r64).max() / scale, np.abs(r32 - r64).max() / scale
    print(f"{what}: GPU {eg:.3e}, float32 restatement {e32:.3e} (max |field| = {scale:.4g})")
    assert eg <= 4 * e32, what


def _compare_fluid(what, icm, refs):
    rho, g, v = _state(icm)
    f64, f32 = refs
    _bound(f"{what} rho", rho, f64.rho, f32.rho)
    _bound(f"{what} g", g, np.array(f64.g), np.array(f32.g))
    _bound(f"{what} v", v, np.array(f64.v), np.array(f32.v))


# ---- the fluid alone --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cells", GRIDS, ids=lambda c: "x".join(map(str, c)))
def test_fluid_parity(cells):
    pd, icm, refs = _make(cells)
    _set(icm, refs, *_smooth(refs[0]))
    for _ in range(20):
        icm.forwardTime()
        for f in refs:
            f.step_fluid()
    _compare_fluid(f"{cells} after 20 steps", icm, refs)
    col = icm.getCurrentVelocity().cpu().numpy()
    stag = icm.getCurrentVelocity(collocated=False).cpu().numpy()
    for a in range(3):                                                     # the collocated export: the mean of the two faces
        assert np.array_equal(col[a], np.float32(0.5) * (stag[a] + ref.shift(stag[a], a, -1)))


def test_rest_stays_at_rest():
    """The state of the reference's acceptance run (test/Hydro/ICM_Compressible data.main): no pressure difference may be contracted into
    an FMA, and the Runge-Kutta combination must return the unchanged value."""
    par = dict(shear=53.71, bulk=127.05, c=14.67, dt=1.0)
    pd, icm, refs = _make((5, 7, 6), h=100.0, par=par)
    rho0 = np.full(refs[0].rho.shape, 0.632, np.float32)
    _set(icm, refs, rho0, [0 * rho0] * 3)
    for _ in range(100):
        icm.forwardTime()
    rho, g, v = _state(icm)
    assert np.array_equal(icm.getCurrentDensity().cpu().numpy().view(np.uint32), rho0.view(np.uint32))
    assert np.array_equal(icm.getMomentum().cpu().numpy().view(np.uint32), np.zeros((3,) + rho0.shape, np.uint32))
    assert not v.any()


def test_shear_wave():
    from test_icm_compressible_cpu import SHEAR, shear_growth, shear_wave
    pd, icm, refs = _make(SHEAR["cells"], par=dict(shear=SHEAR["shear"], bulk=SHEAR["bulk"], c=SHEAR["c"], dt=SHEAR["dt"]))
    f32, mode = shear_wave(np.float32)
    icm.setFluid(*[torch.from_numpy(a.copy()) for a in (f32.rho, *f32.v)])
    steps = 200
    for _ in range(steps):
        icm.forwardTime()
        f32.step_fluid()
    rho, g, v = _state(icm)
    assert not v[1].any() and not v[2].any() and (rho == np.float32(SHEAR["rho0"])).all()          # nothing but v_x moves
    analytic = SHEAR["amplitude"] * shear_growth() ** steps * mode
    _bound(f"shear wave after {steps} steps, v_x against A G^n", v[0], analytic, f32.v[0])


# ---- the stochastic stress --------------------------------------------------------------------------------------------------------------------
def _reference_noise(o32, f, seed, step):
    """(W, bound): the restatement's stress from the oracle's Saru and the bound of the comparison — normals to 1e-6 (the project's
    tolerance for gf), then the float rounding of p_c w + p_t trace"""
    w, _ = ref.saru_normals(o32, seed, step, f.rho.size)     # (the library exposes no integers: a wrong 32-bit stream shows as wrong normals)
    w = w.reshape((6,) + f.rho.shape + (2,))
    W = f.noise_from_normals(w)
    pc, pt = [abs(float(p)) for p in f.prefactors()]
    trace = np.abs(w[0]) + np.abs(w[1]) + np.abs(w[2])
    bound = 1e-6 * np.sqrt(2) * (pc + 3 * pt) + 4 * EPS * (pc * np.abs(w) + pt * trace[None])
    return W, bound


@pytest.mark.parametrize("cells", [(5, 7, 6), (70, 9, 5)], ids=lambda c: "x".join(map(str, c)))
def test_noise_is_the_reference_stream(o32, cells):
    seed = 4711
    pd, icm, refs = _make(cells, T=0.01, seed=seed)
    got = {s: icm.get_noise(s).cpu().numpy() for s in (0, 1, 9)}
    for s, g in got.items():
        W, bound = _reference_noise(o32, refs[0], seed, s)
        err = np.abs(g - W)
        print(f"{cells} step {s}: max |W - W_ref| = {err.max():.3e} (max |W_ref| = {np.abs(W).max():.3e}), worst use of the bound {(err / bound).max():.3f}")
        assert (err <= bound).all()
    assert np.array_equal(icm.get_noise(1).cpu().numpy().view(np.uint32), got[1].view(np.uint32))     # the same (seed, step): the same bits
    assert not np.array_equal(got[0], got[1]) and np.abs(got[0] - got[1]).max() > 0.1 * np.abs(got[0]).max()
    other = _make(cells, T=0.01, seed=seed + 1)[1].get_noise(0).cpu().numpy()
    assert np.abs(other - got[0]).max() > 0.1 * np.abs(got[0]).max()


def test_the_steps_draw_the_noise_of_their_number(o32):
    """two steps with the integrator's own draws against the restatement fed Saru(seed, 0, .) and Saru(seed, 1, .)"""
    seed, cells = 99, (5, 7, 6)
    pd, icm, refs = _make(cells, T=0.01, seed=seed)
    _set(icm, refs, *_smooth(refs[0]))
    for step in range(2):
        icm.forwardTime()
        W = icm.get_noise(step).cpu().numpy()
        for f in refs:
            f.step_fluid(W)
    _compare_fluid("own draws, 2 steps", icm, refs)


@pytest.mark.parametrize("cells", GRIDS, ids=lambda c: "x".join(map(str, c)))
def test_stochastic_step_with_injected_noise(cells):
    pd, icm, refs = _make(cells, T=0.01)
    _set(icm, refs, *_smooth(refs[0]))
    rng = np.random.default_rng(8)
    for _ in range(20):
        W = refs[0].draw(rng).astype(np.float32)
        icm.set_noise(torch.from_numpy(W))
        icm.forwardTime()
        for f in refs:
            f.step_fluid(W)
    _compare_fluid(f"{cells} T = 0.01, injected noise, 20 steps", icm, refs)


def test_conservation():
    """200 steps at T = 0.01 on (5, 7, 6).  Every sub-stage adds a discrete divergence to each cell: the sum over cells changes only by
    rounding, at most 8 eps of the field's scale per cell and sub-stage — a worst-case bound, not a measurement."""
    cells, steps = (5, 7, 6), 200
    pd, icm, refs = _make(cells, T=0.01)
    _set(icm, refs, *_smooth(refs[0]))
    rho0, g0, _ = _state(icm)
    gmax = np.abs(g0).reshape(3, -1).max(1)
    for _ in range(steps):
        icm.forwardTime()
    rho, g, _ = _state(icm)
    gmax = np.maximum(gmax, np.abs(g).reshape(3, -1).max(1))
    ncells = rho.size
    dm, bm = abs(rho.sum() - rho0.sum()), steps * 3 * ncells * 8 * EPS * 1.0
    print(f"mass: |d sum rho| = {dm:.3e}, bound {bm:.3e}")
    assert np.isfinite(rho).all() and dm <= bm
    for a in range(3):
        dp, bp = abs(g[a].sum() - g0[a].sum()), steps * 3 * ncells * 8 * EPS * gmax[a]
        print(f"momentum {a}: |d sum g| = {dp:.3e}, bound {bp:.3e} (max |g| = {gmax[a]:.3e})")
        assert dp <= bp


def test_equilibrium_fluctuations():
    """The fixture's configuration (tests/golden/icm_compressible/make_reference.py) with the integrator's own noise: both ratios within
    the fixture's mean +- 5 across-seed standard deviations."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden", "icm_compressible"))
    from make_reference import ratios
    with open(os.path.join(ROOT, "tests", "golden", "icm_compressible", "equilibrium_reference.json")) as fh:
        fix = json.load(fh)
    c = fix["config"]
    pd, icm, refs = _make(tuple(c["cells"]), h=c["L"] / c["cells"][0], T=c["temperature"], seed=2024,
                          par=dict(shear=c["shearViscosity"], bulk=c["bulkViscosity"], c=c["speedOfSound"], dt=c["dt"]))
    rho0 = np.full(refs[0].rho.shape, c["rho0"], np.float32)
    _set(icm, refs, rho0, [0 * rho0] * 3)
    acc = []
    for step in range(1, c["steps"] + 1):
        icm.forwardTime()
        if step > c["first"] and step % c["every"] == 0:
            acc.append(torch.cat([icm.getCurrentDensity()[None], icm.getCurrentVelocity(collocated=False)]))
    samples = torch.stack(acc).cpu().numpy()
    r = np.mean([ratios(s[0], s[1:], c) for s in samples], axis=0)
    for got, key in zip(r, ("density_variance_ratio", "velocity_square_ratio")):
        m, s = fix[key]["mean"], fix[key]["std"]
        print(f"{key}: {got:.5f}, fixture {m:.5f} +- {s:.5f} ({(got - m) / s:+.2f} sigma)")
        assert abs(got - m) <= 5 * s, key


# ---- particles --------------------------------------------------------------------------------------------------------------------------------
class Fixed:
    """a constant force per particle"""

    def __init__(self, pd, F):
        self.pd = pd
        self.F = torch.from_numpy(np.ascontiguousarray(F, np.float32)).cuda()
        self.times = []

    def sum(self, force=False, energy=False, virial=False):
        self.pd.getForce("readwrite")[:, :3] += self.F

    def updateSimulationTime(self, t):
        self.times.append(t)


def _particles(cells, n=64, seed=6):
    """n positions: a quarter within 1e-3 h of a cell face in every direction, all spread over (-L, L): outside the primary box on both sides"""
    rng = np.random.default_rng(seed)
    L = np.array(cells, np.float64)
    pos = rng.uniform(-1.0, 1.0, (n, 3)) * L
    k = n // 4
    pos[:k] = np.round(pos[:k]) + 0.5 * (np.array(cells) % 2) + rng.uniform(-1e-3, 1e-3, (k, 3))      # faces at integers (+ 1/2 for odd n)
    p4 = np.zeros((n, 4), np.float32)
    p4[:, :3] = pos
    p4[:, 3] = np.arange(n) % 3
    assert (np.abs(pos) > 0.5 * L).any(1).sum() > n // 4 and (pos < -0.5 * L).any() and (pos > 0.5 * L).any()
    return p4


def test_tracers_follow_a_uniform_flow():
    cells, steps = (5, 7, 6), 10
    p4 = _particles(cells)
    pd, icm, refs = _make(cells, N=len(p4))
    pd.setPos(p4)
    v0 = np.array([0.3, -0.2, 0.45], np.float32)
    one = np.ones(refs[0].rho.shape, np.float32)
    _set(icm, refs, 0.9 * one, [v0[a] * one for a in range(3)])
    for _ in range(steps):
        icm.forwardTime()
    torch.cuda.synchronize()
    got = pd.getPos("read").cpu().numpy()
    assert np.array_equal(got[:, 3], p4[:, 3])                                 # pos.w is kept
    expect = p4[:, :3].astype(np.float64) + steps * PAR["dt"] * v0.astype(np.float64)
    # per step: one rounding of the new position (eps |q|) and the 27-term window sum of v0 (each weight a product of three windows of
    # a few ulps each: 64 eps of |v0| dt covers it)
    bound = steps * (2 * EPS * np.abs(expect).max() + 64 * EPS * np.abs(v0).max() * PAR["dt"])
    err = np.abs(got[:, :3] - expect).max()
    print(f"tracers in a uniform flow, {steps} steps: max error {err:.3e}, bound {bound:.3e}")
    assert err <= bound
    assert (np.abs(got[:, :3]) > 0.5 * np.array(cells)).any()                  # positions are not folded


def test_one_step_gives_the_fluid_the_impulse_of_the_forces():
    cells = (5, 7, 6)
    p4 = _particles(cells)
    pd, icm, refs = _make(cells, N=len(p4))
    pd.setPos(p4)
    F = np.random.default_rng(7).normal(0, 1, (len(p4), 3)).astype(np.float32)
    icm.addInteractor(Fixed(pd, F))
    icm.forwardTime()
    rho, g, v = _state(icm)
    got = g.reshape(3, -1).sum(1) * 1.0                                        # dV = 1
    want = PAR["dt"] * F.astype(np.float64).sum(0)
    # the weights of a particle sum to 1 to 32 eps (three windows of a few ulps each), the cell sums round once per operation
    bound = 128 * EPS * PAR["dt"] * np.abs(F).sum()
    print(f"sum g dV = {got}, dt sum F = {want}, max difference {np.abs(got - want).max():.3e}, bound {bound:.3e}")
    assert np.abs(got - want).max() <= bound


def test_full_step_parity_with_particles():
    cells, steps = (5, 7, 6), 10
    p4 = _particles(cells)
    pd, icm, refs = _make(cells, N=len(p4))
    pd.setPos(p4)
    _set(icm, refs, *_smooth(refs[0]))
    F = np.random.default_rng(9).normal(0, 1, (len(p4), 3)).astype(np.float32)
    fixed = Fixed(pd, F)
    icm.addInteractor(fixed)
    q = [p4[:, :3].astype(np.float64), p4[:, :3].copy()]
    for _ in range(steps):
        icm.forwardTime()
        q = [f.forward(p, lambda qh: F.astype(f.dtype)) for f, p in zip(refs, q)]
    _compare_fluid(f"{len(p4)} particles, {steps} steps", icm, refs)
    got = pd.getPos("read").cpu().numpy()
    _bound("positions", got[:, :3], q[0], q[1])
    dt = PAR["dt"]
    assert np.allclose(fixed.times[:4], [0.5 * dt, dt / 3, 2 * dt / 3, dt], rtol=1e-6) and len(fixed.times) == 4 * steps


# ---- the interface ------------------------------------------------------------------------------------------------------------------------------
def test_api():
    hip = _hip()
    P = hip.Hydro.ICM_Compressible.Parameters
    pd = hip.ParticleData(0)
    good = dict(shearViscosity=1.0, bulkViscosity=1.0, speedOfSound=4.0, dt=0.05, boxSize=[32.0, 32.0, 32.0])
    icm = hip.Hydro.ICM_Compressible(pd, P(hydrodynamicRadius=1.0, **good))
    assert icm.getGridSize() == [35, 35, 35]                                   # int(32 / 0.91)
    for _ in range(3):                                                         # N = 0: a fluid-only run
        icm.forwardTime()
    torch.cuda.synchronize()
    assert (icm.getCurrentDensity() == 1).all() and not icm.getCurrentVelocity().any() and icm.getCurrentVelocity().shape == (3, 35, 35, 35)
    bad = [dict(shearViscosity=0.0), dict(bulkViscosity=-1.0), dict(temperature=-1.0), dict(dt=-0.1), dict(speedOfSound=0.0),
           dict(boxSize=[0.0, 1.0, 1.0]), dict(), dict(cellDim=[8, 8, 8], hydrodynamicRadius=1.0)]
    words = ["shear viscosity", "bulk viscosity", "temperature", "dt", "speed of sound", "box size", "either an hydrodynamic radius",
             "either an hydrodynamic radius"]
    for change, word in zip(bad, words):
        kw = dict(good, cellDim=[8, 8, 8])
        if not change:
            kw.pop("cellDim")
        kw.update(change)
        drawn = list(pd.rng.s)
        with pytest.raises(ValueError, match=word):
            hip.Hydro.ICM_Compressible(pd, P(**kw))
        assert list(pd.rng.s) == drawn                                         # a refused parameter set draws no seed
    # the initial fields as callables, evaluated at (cell / n + 0.5) L, and as arrays
    a = hip.Hydro.ICM_Compressible(pd, P(cellDim=[4, 3, 2], **dict(good, boxSize=[4.0, 3.0, 2.0]), initialDensity=lambda r: 1 + 0.1 * r[0],
                                         initialVelocityY=lambda r: 0.01 * r[2]))
    f = ref.Fluid((4, 3, 2), (4.0, 3.0, 2.0), 1.0, 1.0, 4.0, 0.05, 0.0, np.float32)
    x, y, z = f.centers()
    assert np.array_equal(a.getCurrentDensity().cpu().numpy(), (1 + 0.1 * x.astype(np.float64)).astype(np.float32))
    vy = a.getCurrentVelocity(collocated=False).cpu().numpy()[1]
    assert np.allclose(vy, 0.01 * z, rtol=1e-6) and not a.getCurrentVelocity(collocated=False)[0].any()
    b = hip.Hydro.ICM_Compressible(pd, P(cellDim=[4, 3, 2], **dict(good, boxSize=[4.0, 3.0, 2.0]), initialDensity=a.getCurrentDensity().cpu().numpy()))
    assert torch.equal(a.getCurrentDensity(), b.getCurrentDensity())
    with pytest.raises(ValueError):
        a.set_noise(torch.zeros(5))
    with pytest.raises(ValueError):
        a.setFluid(density=torch.zeros(5))
