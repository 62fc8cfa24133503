"""Pins of the NumPy restatement of Hydro::ICM_Compressible (tests/icm_compressible_ref.py), the yardstick of tests/test_gpu_icm_compressible.py:
the analytic decay of a shear wave, conservation of mass and momentum with noise, the moments of the stochastic stress, the window, and
the spread / gather pair.  No GPU."""
import numpy as np

import icm_compressible_ref as ref

SHEAR = dict(cells=(6, 16, 5), L=(6.0, 16.0, 5.0), shear=1.3, bulk=0.7, c=4.0, dt=0.05, rho0=0.8, amplitude=1e-2)


def shear_wave(dtype, p=SHEAR):
    f = ref.Fluid(p["cells"], p["L"], p["shear"], p["bulk"], p["c"], p["dt"], 0.0, dtype)
    y = f.centers()[1]
    mode = np.sin(2 * np.pi * y.astype(np.float64) / p["L"][1])
    f.set(rho=np.full(f.rho.shape, p["rho0"]), v=[p["amplitude"] * mode, 0 * mode, 0 * mode])
    return f, mode


def shear_growth(p=SHEAR):
    """G = 1 + z + z^2/2 + z^3/6, z = -(eta / rho0) (2 / h^2) (1 - cos k h) dt: the RK3 amplification of the discrete shear mode"""
    h, k = p["L"][1] / p["cells"][1], 2 * np.pi / p["L"][1]
    z = -(p["shear"] / p["rho0"]) * (2 / h ** 2) * (1 - np.cos(k * h)) * p["dt"]
    return 1 + z + z * z / 2 + z ** 3 / 6


def test_shear_wave_decays_at_the_analytic_rate():
    f, mode = shear_wave(np.float64)
    for _ in range(200):
        f.step_fluid()
    assert not f.v[1].any() and not f.v[2].any() and (f.rho == SHEAR["rho0"]).all()          # nothing but v_x moves
    expect = SHEAR["amplitude"] * shear_growth() ** 200
    got = 2 * (f.v[0] * mode).mean()
    err = abs(got / expect - 1)
    print(f"shear wave: amplitude {got:.15e}, analytic {expect:.15e}, relative error {err:.2e}")
    assert err <= 1e-12
    assert np.abs(f.v[0] - expect * mode).max() <= 1e-12 * expect


def smooth_state(f, seed=3, drho=0.05, dv=0.05):
    """rho = 1 +- drho and |v_a| <= dv, smooth and periodic, different in every direction"""
    x, y, z = [2 * np.pi * c.astype(np.float64) / l for c, l in zip(f.centers(), f.L.astype(np.float64))]
    rho = 1 + drho * np.sin(x + 0.3) * np.cos(y - 0.2) * np.cos(z + 0.1)
    v = [dv * np.sin(y + 0.5) * np.cos(z), dv * np.cos(x + 0.4) * np.sin(z - 0.3), dv * np.sin(x - 0.1) * np.sin(y + 0.2)]
    f.set(rho=rho, v=v)


def test_mass_and_momentum_are_conserved_with_noise():
    f = ref.Fluid((5, 7, 6), (5.0, 7.0, 6.0), 1.0, 1.0, 4.0, 0.05, 0.01, np.float64)
    smooth_state(f)
    rng = np.random.default_rng(11)
    m0, p0 = f.rho.sum(), [g.sum() for g in f.g]
    for _ in range(1500):
        f.step_fluid(f.draw(rng))
    em = abs(f.rho.sum() - m0) / m0
    ep = max(abs(g.sum() - q) / np.abs(g).sum() for g, q in zip(f.g, p0))
    print(f"1500 steps at T = 0.01: mass {em:.2e}, momentum {ep:.2e} (relative to sum |g|)")
    assert np.isfinite(f.rho).all() and em <= 1e-12 and ep <= 1e-12


def test_noise_is_symmetric_with_the_moments_of_the_prefactors():
    assert all(ref.ENTRY[a, b] == ref.ENTRY[b, a] for a in range(3) for b in range(3))
    assert sorted(set(ref.ENTRY.values())) == list(range(6))
    shear, bulk, T, dt = 1.3, 0.7, 0.02, 0.05
    f = ref.Fluid((24, 24, 24), 36.0, shear, bulk, 4.0, dt, T, np.float64)
    W = f.draw(np.random.default_rng(5))
    n = W[0].size
    tol = 5 * np.sqrt(2.0 / n)                       # five standard errors of a variance estimate from n normals
    base = T * dt / f.dV
    trace = W[0] + W[1] + W[2]
    checks = {"trace": (trace.var(), 18 * bulk * base), "xx - yy": ((W[0] - W[1]).var(), 8 * shear * base),
              "yy - zz": ((W[1] - W[2]).var(), 8 * shear * base)}
    for e, name in ((3, "xy"), (4, "xz"), (5, "yz")):
        checks[name] = (W[e].var(), 2 * shear * base)
    for name, (got, want) in checks.items():
        print(f"var({name}) = {got:.5e}, expected {want:.5e}")
        assert abs(got / want - 1) <= tol, name
    assert abs(np.mean(trace * (W[0] - W[1]))) <= tol * np.sqrt(18 * bulk * 8 * shear) * base     # trace and deviator uncorrelated
    assert abs(np.mean(W[..., 0] * W[..., 1])) <= tol * 4 * max(shear, bulk) * base             # W_A and W_B uncorrelated


def test_saru_normals_have_unit_moments():
    import oracle
    w, ints = ref.saru_normals(oracle.get("f32"), 1234, 7, 2000)
    assert ints.dtype == np.uint32 and len(np.unique(ints)) > 0.99 * ints.size
    assert abs(w[3:].var() - 1) < 0.03 and abs(w[:3].var() - 2) < 0.06 and abs(w.mean()) < 0.03
    w2, _ = ref.saru_normals(oracle.get("f32"), 1234, 8, 50)
    assert not np.array_equal(w[:, :50], w2)


def test_window_sums_to_one():
    f = ref.Fluid((8, 8, 8), 10.0, 1.0, 1.0, 4.0, 0.05)
    rng = np.random.default_rng(2)
    x = rng.uniform(-0.5, 0.5, 1000) * f.h[0]
    total = sum(f.phi(x - k * f.h[0]) for k in range(-2, 3)) * f.h[0]
    assert np.abs(total - 1).max() <= 1e-14
    assert f.phi(np.array([1.5 * f.h[0], 1.7 * f.h[0]])).max() == 0 and f.phi(np.array([1.4999999 * f.h[0]]))[0] < 1e-6 / f.h[0]


def test_gather_of_a_uniform_field_and_spread_of_a_force():
    f = ref.Fluid((5, 7, 6), (5.0, 7.0, 6.0), 1.0, 1.0, 4.0, 0.05)
    rng = np.random.default_rng(4)
    pos = rng.uniform(-1.0, 1.0, (64, 3)) * f.L                       # half of them outside the primary box
    u = f.gather(pos, [np.full(f.rho.shape, c) for c in (0.3, -0.2, 0.7)])
    assert np.abs(u - [0.3, -0.2, 0.7]).max() <= 1e-14
    F = rng.normal(0, 1, (64, 3))
    s = f.spread(pos, F)
    assert np.abs(np.array([c.sum() for c in s]) * f.dV - F.sum(0)).max() <= 1e-13
    field = [rng.normal(0, 1, f.rho.shape) for _ in range(3)]       # adjointness: F . J v = dV sum (S F) v
    lhs, rhs = (F * f.gather(pos, field)).sum(), sum((a * b).sum() for a, b in zip(s, field)) * f.dV
    assert abs(lhs - rhs) <= 1e-12 * abs(lhs)
