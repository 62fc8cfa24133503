"""The reference's polymer and DPD setups end to end in double behind uammd_amd/f64.py: a Kremer-Grest melt (WCA on f64.VerletList + FENE
through f64.BondedForces) under f64.VerletNVE against a float64 NumPy run, and a DPD fluid's total momentum.

Bars: 1e-11 |E0| for an NVE energy series summed in another order (the f64 suite's bar); the float test's momentum bound 1e-4 n sqrt(kT)
times 2^-29."""
import numpy as np
import pytest
import torch

import bonded_ref
import dpd_ref

pytestmark = pytest.mark.gpu

S = 2.0 ** -29


def _wca_numpy(pos, L, rc):
    """dpd_ref.lj_forces_energy's truncated and shifted LJ (sigma = epsilon = 1) over dpd_ref.pairs: forces and the total energy"""
    I, J, rij = dpd_ref.pairs(pos, L, (True, True, True), rc)
    r2 = (rij * rij).sum(-1)
    ir2 = 1.0 / r2
    ir6 = ir2 ** 3
    fmod = (48.0 * ir6 - 24.0) * ir6 * ir2            # f_i = fmod (ri - rj)
    F = np.zeros((len(pos), 3))
    np.add.at(F, I, fmod[:, None] * rij)
    np.add.at(F, J, -fmod[:, None] * rij)
    eshift = 4.0 * (rc ** -12 - rc ** -6)
    return F, float((4.0 * ir6 * (ir6 - 1.0) - eshift).sum())


def test_kremer_grest_nve_energy(hip):
    """121 chains of 11 beads on an 11^3 simple-cubic lattice of spacing 0.967 (L = 10.637), chains along x, jitter 0.02; WCA
    (rc = 2^(1/6), shifted) + FENE (k = 30, r0 = 1.5); velocities from f64.initVelocities at kT = 1; 200 steps of dt = 0.002.  The total
    energy after every step within 1e-11 |E0| of the float64 NumPy run; the single-precision classes' distance is printed beside it."""
    from uammd_amd import f64
    m, a, dt, steps = 11, 0.967, 0.002, 200
    n, L, rc = m ** 3, m * a, 2.0 ** (1.0 / 6.0)
    g = np.stack(np.meshgrid(np.arange(m), np.arange(m), np.arange(m), indexing="ij"), -1).reshape(-1, 3)      # x slowest ...
    g = g[:, ::-1]                                                                                          # ... now x fastest: a chain is a row along x
    pos = np.zeros((n, 4))
    pos[:, :3] = (g + 0.5) * a - L / 2 + np.random.default_rng(3).uniform(-0.02, 0.02, (n, 3))
    ids = (np.arange(n).reshape(m * m, m)[:, :-1].reshape(-1, 1) + np.array([[0, 1]])).astype(np.int32)     # 121 x 10 bonds
    info = np.tile([30.0, 1.5], (len(ids), 1))
    assert np.abs(np.linalg.norm(pos[ids[:, 1], :3] - pos[ids[:, 0], :3], axis=1) - a).max() < 0.08

    box = f64.Box(L)
    pot = f64.LJ()
    pot.setPotParameters(0, 0, pot.InputPairParameters(rc, 1.0, 1.0, True))
    vl = f64.VerletList()
    pf = f64.PairForcesLJ(box, pot, nl=vl)
    bf = f64.BondedForces("fene", ids, info, box)
    bf.refresh(torch.arange(n, dtype=torch.int32, device="cuda"))
    dp = torch.from_numpy(pos.copy()).cuda()
    dv = torch.zeros((n, 3), dtype=torch.float64, device="cuda")
    f64.initVelocities(dv, 1.0, 4242)
    df = torch.zeros((n, 4), dtype=torch.float64, device="cuda")
    vel = dv.cpu().numpy().copy()
    integ = f64.VerletNVE(dt)

    def energy64():
        e = torch.zeros(n, dtype=torch.float64, device="cuda")
        pf.sum(dp, None, e, None)
        bf.sum(dp, None, e, None)
        f64.sumKineticEnergy(dv, e)
        return float(e.sum())

    got = [energy64()]
    for _ in range(steps):
        integ.forwardTime(dp, dv, df, [pf, bf])
        got.append(energy64())
    assert vl.rebuilds >= 1 and pf.nl is vl

    # the float64 NumPy run: VerletNVE::forwardTime's sequence over all-pairs WCA and the restated FENE
    def forces(p):
        F, U = _wca_numpy(p, L, rc)
        fb, eb, _ = bonded_ref.per_particle("fene", p, ids, info, [L] * 3)
        return F + fb, U + float(eb.sum())
    p, v, mass = pos.copy(), vel.copy(), np.ones(n)
    F, U = forces(p)
    ref = [U + 0.5 * (v * v).sum()]
    for _ in range(steps):
        p, v = dpd_ref.nve_half(p, v, F, mass, dt, 1)
        F, U = forces(p)
        _, v = dpd_ref.nve_half(p, v, F, mass, dt, 2)
        ref.append(U + 0.5 * (v * v).sum())
    ref = np.array(ref)
    e0 = abs(ref[0])
    err64 = np.abs(np.array(got) - ref).max() / e0
    print(f"[f64] max |E - ref| / |E0| over {steps} steps: {err64:.3e} (E0 = {ref[0]:.6f}, drift of the reference "
          f"{abs(ref[-1] - ref[0]) / e0:.2e}, list rebuilds {vl.rebuilds})")

    # the single-precision classes on the same input, for comparison
    from uammd_amd import bonded
    pd = hip.ParticleData(n)
    pd.setPos(pos.astype(np.float32))
    pd.getVel("write").copy_(torch.from_numpy(vel.astype(np.float32)))
    pot32 = hip.Potential.LJ()
    pot32.setPotParameters(0, 0, pot32.InputPairParameters(rc, 1.0, 1.0, True))
    pf32 = hip.PairForces(pd, hip.Box(L), pot32, nl=hip.VerletList(pd))
    bf32 = bonded.BondedForces(pd, bondType=bonded.BondedType.FENE(hip.Box(L)), ids=ids, info=info.astype(np.float32))
    nve32 = hip.VerletNVE(pd, dt=dt, initVelocities=False)
    nve32.addInteractor(pf32)
    nve32.addInteractor(bf32)

    def energy32():
        pd.getEnergy("write").zero_()
        pf32.sum(force=False, energy=True)
        bf32.sum(force=False, energy=True)
        nve32.sumEnergy()
        return float(pd.getEnergy("read").double().sum())

    got32 = [energy32()]
    for _ in range(steps):
        nve32.forwardTime()
        got32.append(energy32())
    err32 = np.abs(np.array(got32) - ref).max() / e0
    print(f"[f32] max |E - ref| / |E0|: {err32:.3e}")
    assert err64 <= 1e-11


def test_dpd_fluid_momentum(hip):
    """3000 particles at rho = 3, 50 steps of f64.VerletNVE + f64.PairForcesDPD: the total momentum stays within the float test's bound
    (1e-4 n sqrt(kT)) times 2^-29."""
    from uammd_amd import f64
    n, kT, dt, steps = 3000, 1.0, 0.01, 50
    L = (n / 3.0) ** (1.0 / 3.0)
    rng = np.random.default_rng(8)
    pos = np.zeros((n, 4))
    pos[:, :3] = rng.uniform(-L / 2, L / 2, (n, 3)) * 0.999
    vel = rng.normal(0, np.sqrt(kT), (n, 3))
    vel -= vel.mean(0)
    dpd = f64.PairForcesDPD(f64.Box(L), cutOff=1.0, A=25.0, gamma=4.5, temperature=kT, dt=dt, seed=1234)
    integ = f64.VerletNVE(dt)
    dp, dv = torch.from_numpy(pos).cuda(), torch.from_numpy(vel).cuda()
    df = torch.zeros((n, 4), dtype=torch.float64, device="cuda")
    worst = 0.0
    for _ in range(steps):
        integ.forwardTime(dp, dv, df, [dpd])
        worst = max(worst, float(dv.sum(0).abs().max()))
    T = float((dv * dv).sum()) / (3 * n)
    bar = 1e-4 * n * np.sqrt(kT) * S
    print(f"[dpd fluid] max |P| over {steps} steps: {worst:.3e}, bar {bar:.3e}; kinetic temperature after them {T:.3f}; force sums {dpd.step}")
    assert dpd.step == steps + 1 and dpd.uses_cell_list()
    assert worst <= bar
    assert np.isfinite(T) and T > 0.5          # (the uniformly random start releases potential energy: the fluid is still cooling to kT)
