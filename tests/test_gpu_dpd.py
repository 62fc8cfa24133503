"""Potential::DPD and VerletNVE on the GPU (uammd_amd/csrc/dpd.hip, k_verletnve in integrators.hip) through the Python layer on the C ABI,
against the float64 NumPy restatement in tests/dpd_ref.py: force parity on the list and the all-pairs path, pair symmetry, determinism and
the key following the index through a reorder, the step counter and the updatables, groups, the NVE integrator by itself, the DPD
thermostat end to end, and the C++ programs of tests/cxx."""
import json
import os
import subprocess

import numpy as np
import pytest
import torch

import dpd_ref
from util import lattice_positions

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "examples", "_build")
GOLD = os.path.join(ROOT, "tests", "golden", "dpd", "temperature_reference.json")

TOL = 2e-5          # max |F - F_ref| / max |F_ref|: the project's bar for pair kinds that are a handful of float operations
DPD = dict(cutOff=1.0, dt=0.01, gamma=4.5, temperature=1.0, A=25.0)


def _hip():
    import uammd_amd as hip
    return hip


def _fluid(n, L, seed):
    rng = np.random.default_rng(seed)
    L3 = np.broadcast_to(np.asarray(L, np.float64), (3,))
    pos = np.zeros((n, 4), np.float32)
    pos[:, :3] = rng.uniform(-0.5, 0.5, (n, 3)) * L3 * 0.999
    vel = rng.normal(0.0, 1.0, (n, 3)).astype(np.float32)      # Maxwell at kT = 1, m = 1
    return pos, vel


def _system(pos, vel, L, periodic=(True, True, True), group=None, **kw):
    hip = _hip()
    pd = hip.ParticleData(len(pos))
    pd.setPos(pos)
    pd.getVel("write").copy_(torch.from_numpy(np.ascontiguousarray(vel)).cuda())
    box = hip.Box(L, periodic)
    pot = hip.Potential.DPD(**{**DPD, **kw})
    target = pd if group is None else hip.ParticleGroup(pd, group)
    return pd, box, pot, hip.PairForces(target, box, pot)


def _sum(pd, pf):
    pd.getForce("write").zero_()
    pf.sum(force=True)
    torch.cuda.synchronize()
    return pd.getForce("read").cpu().numpy()


def _ref(pd, box, pot, members=None, **kw):
    """The restatement on the ParticleData's current arrays with the potential's current seed and step."""
    pos = pd.getPos("read").cpu().numpy().astype(np.float64)
    vel = pd.getVel("read").cpu().numpy().astype(np.float64)
    par = dict(rc=pot.rcut, A=pot.A, gamma=pot.gamma, kT=pot.temperature, dt=pot.dt)
    par.update(kw)
    F = np.zeros((pd.N, 3))
    m = np.arange(pd.N) if members is None else np.asarray(members)
    F[m] = dpd_ref.dpd_forces(pos[m], vel[m], box.boxSize.astype(np.float64), tuple(box.periodic), par["rc"], par["A"], par["gamma"], par["kT"],
                              par["dt"], seed=pot.seed, step=pot.step, keys=m, nkey=pd.N)
    return F


def _err(got, want, what=""):
    e = np.abs(got[:, :3] - want).max() / np.abs(want).max()
    print(f"{what}: max|F - F_ref| / max|F_ref| = {e:.3e}  (max|F_ref| = {np.abs(want).max():.4g})")
    return e


# ---- 1. force parity ---------------------------------------------------------------------------------------------------------------------
CASES = {"cubic": (3000, 10.0, (True, True, True)), "anisotropic_open_z": (3000, (12.5, 10.0, 8.0), (True, True, False)),
         "all_pairs": (200, 2.5, (True, True, True))}


@pytest.mark.parametrize("case", list(CASES))
def test_force_parity(case):
    n, L, per = CASES[case]
    pos, vel = _fluid(n, L, seed=11)
    pd, box, pot, pf = _system(pos, vel, L, per)
    got = _sum(pd, pf)
    assert pot.step == 1 and pot.seed is not None
    assert _err(got, _ref(pd, box, pot), case) <= TOL
    assert not got[:, 3].any()


@pytest.mark.parametrize("off", ["A", "gamma", "temperature"])
@pytest.mark.parametrize("case", ["cubic", "all_pairs"])
def test_force_parity_one_term_off(case, off):
    """A wrong sign or a missing sqrt(gamma) / 1/sqrt(dt) in one term cannot hide behind the others."""
    n, L, per = CASES[case]
    pos, vel = _fluid(n, L, seed=12)
    pd, box, pot, pf = _system(pos, vel, L, per, **{off: 0.0})
    got = _sum(pd, pf)
    assert _err(got, _ref(pd, box, pot), f"{case}, {off} = 0") <= TOL


# ---- 2. pair symmetry --------------------------------------------------------------------------------------------------------------------
def test_pair_symmetry():
    n = 100000
    L = (n / 3.0) ** (1.0 / 3.0)
    pos, vel = _fluid(n, L, seed=13)
    pd, box, pot, pf = _system(pos, vel, L)
    F = _sum(pd, pf)[:, :3].astype(np.float64)
    total, scale = np.abs(F.sum(0)).max(), np.abs(F).sum()
    print(f"|sum F| = {total:.3e}, sum |F| = {scale:.3e}, ratio {total / scale:.3e}")
    assert total <= 1e-5 * scale


# ---- 3. determinism, and the key follows the index ----------------------------------------------------------------------------------------
def test_determinism_and_reorder():
    n, L = 3000, 10.0
    pos, vel = _fluid(n, L, seed=14)
    pd, box, pot, pf = _system(pos, vel, L)
    a = _sum(pd, pf)
    pot.step -= 1                              # the same step again
    b = _sum(pd, pf)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    pd.hintSortByHash(box, [1.0, 1.0, 1.0])
    pd.sortParticles()
    assert not np.array_equal(pd.id.cpu().numpy(), np.arange(n))
    pot.step -= 1
    c = _sum(pd, pf)
    assert _err(c, _ref(pd, box, pot), "after sortParticles, new indices as keys") <= TOL
    # the same particles now draw other numbers: the forces are NOT a permutation of the earlier ones
    ids = pd.id.cpu().numpy()
    assert np.abs(c[:, :3] - a[ids, :3]).max() > 1e-2 * np.abs(a[:, :3]).max()


# ---- 4. step counter and updatables ---------------------------------------------------------------------------------------------------------
def test_step_counter_and_updatables():
    n, L = 3000, 10.0
    pos, vel = _fluid(n, L, seed=15)
    pd, box, pot, pf = _system(pos, vel, L)
    sums = []
    for k in (1, 2, 3):
        got = _sum(pd, pf)
        assert pot.step == k
        assert _err(got, _ref(pd, box, pot), f"step {k}") <= TOL
        sums.append(got)
    assert np.abs(sums[0] - sums[1]).max() > 1.0          # another step, other noise
    seed = pot.seed
    pf.updateTimeStep(0.04)                               # PairForces forwards to the potential: sigma halves
    got = _sum(pd, pf)
    assert pot.dt == 0.04 and pot.seed == seed
    assert _err(got, _ref(pd, box, pot, dt=0.04), "dt = 0.04") <= TOL
    pf.updateTemperature(2.0)
    got = _sum(pd, pf)
    assert _err(got, _ref(pd, box, pot, dt=0.04, kT=2.0), "kT = 2") <= TOL
    # energy / virial are not defined: nothing is added, the step still advances (one transverser request)
    e0 = pd.getEnergy("write").zero_()
    step = pot.step
    pf.sum(force=False, energy=True)
    torch.cuda.synchronize()
    assert pot.step == step + 1 and not pd.getEnergy("read").any() and e0 is not None


# ---- 5. groups -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["cubic", "all_pairs"])
def test_group_of_every_other_particle(case):
    n, L, per = CASES[case]
    if case == "cubic":
        n = 6000                                         # 3000 members: still rho = 1.5 among them, the list path
        L = 12.6
    pos, vel = _fluid(n, L, seed=16)
    members = np.arange(0, n, 2)
    pd, box, pot, pf = _system(pos, vel, L, per, group=members.tolist())
    got = _sum(pd, pf)
    want = _ref(pd, box, pot, members=members)
    assert _err(got, want, f"group, {case}") <= TOL
    assert not got[1::2].any()


# ---- 6. VerletNVE by itself -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("is2D", [False, True])
@pytest.mark.parametrize("indexed", [False, True])
@pytest.mark.parametrize("step", [1, 2])
def test_nve_kernel(step, indexed, is2D):
    """uammd_verletnve against the float64 formula, 1e-6 of the largest entry (one multiply-add chain per component)."""
    hip = _hip()
    from uammd_amd.md import _ptr, current_stream
    from uammd_amd._lib import check
    lib = hip.load()
    rng = np.random.default_rng(20 + step)
    n, dt = 1000, 0.01
    pos = rng.uniform(-5, 5, (n, 4)).astype(np.float32)
    vel = rng.normal(0, 1, (n, 3)).astype(np.float32)
    force = rng.normal(0, 30, (n, 4)).astype(np.float32)
    mass = rng.uniform(0.5, 2.0, n).astype(np.float32)
    index = np.sort(rng.permutation(n)[: n // 3]).astype(np.int32) if indexed else None
    d = [torch.from_numpy(x.copy()).cuda() for x in (pos, vel, force, mass)]
    di = torch.from_numpy(index).cuda() if indexed else None
    check(lib.uammd_verletnve(step, _ptr(d[0]), _ptr(d[1]), _ptr(d[2]), _ptr(d[3]), 7.0, _ptr(di), len(index) if indexed else n, dt,
                              int(is2D), current_stream()))
    torch.cuda.synchronize()
    m = np.arange(n) if index is None else index
    wp, wv = pos.astype(np.float64), vel.astype(np.float64)
    p1, v1 = dpd_ref.nve_half(pos[m, :3], vel[m], force[m], mass[m], dt, step, is2D)
    wp[m, :3], wv[m] = p1, v1
    gp, gv = d[0].cpu().numpy(), d[1].cpu().numpy()
    ev, ep = np.abs(gv - wv).max() / np.abs(wv).max(), np.abs(gp - wp).max() / np.abs(wp).max()
    print(f"step {step} indexed {indexed} is2D {is2D}: vel {ev:.2e} pos {ep:.2e}")
    assert ev <= 1e-6 and ep <= 1e-6
    assert np.array_equal(gp[:, 3], pos[:, 3]) and np.array_equal(d[2].cpu().numpy(), force)
    if step == 2:
        assert np.array_equal(gp, pos)
    # without a mass array the default mass is used
    d2 = [torch.from_numpy(x.copy()).cuda() for x in (pos, vel, force)]
    check(lib.uammd_verletnve(2, _ptr(d2[0]), _ptr(d2[1]), _ptr(d2[2]), None, 7.0, None, n, dt, 0, current_stream()))
    _, v2 = dpd_ref.nve_half(pos[:, :3], vel, force, np.full(n, 7.0), dt, 2)
    assert np.abs(d2[1].cpu().numpy() - v2).max() <= 1e-6 * np.abs(v2).max()


LJ = dict(n=500, L=8.55, rc=2.5, dt=0.002)     # rho* = 0.8; L > 3 rc: the list path


def _lj_system(seed=31, vel_scale=1.0, mass=None):
    hip = _hip()
    pos = lattice_positions(LJ["n"], LJ["L"], seed=seed, jitter=0.05)
    vel = np.random.default_rng(seed).normal(0, vel_scale, (LJ["n"], 3)).astype(np.float32)
    vel -= vel.mean(0)
    pd = hip.ParticleData(LJ["n"])
    pd.setPos(pos)
    pd.getVel("write").copy_(torch.from_numpy(vel).cuda())
    if mass is not None:
        pd.getMass("write").copy_(torch.from_numpy(mass).cuda())
    box = hip.Box(LJ["L"])
    pot = hip.Potential.LJ()
    pot.setPotParameters(0, 0, pot.InputPairParameters(LJ["rc"], 1.0, 1.0, True))
    return pd, box, hip.PairForces(pd, box, pot), pos, vel


class _Recorder:
    def __init__(self, pd=None):
        self.heard, self.pd, self.vel = [], pd, None

    def updateTimeStep(self, dt):
        self.heard.append(("dt", dt))
        if self.pd is not None:     # (called after initializeVelocities and before the first force sum and kick, VerletNVE.cu:160-171)
            self.vel = self.pd.getVel("read").cpu().numpy().copy()

    def updateSimulationTime(self, t):
        self.heard.append(("t", t))

    def updateTemperature(self, T):
        self.heard.append(("T", T))

    def updateBox(self, box):
        self.heard.append(("box", box))


def _by_hand(pd, pf, steps, dt, mass=None, default_mass=1.0, index=None):
    """zero forces -> sum -> [uammd_verletnve(1) -> zero forces -> sum -> uammd_verletnve(2)] x steps"""
    hip = _hip()
    from uammd_amd.md import _ptr, current_stream
    from uammd_amd._lib import check
    lib = hip.load()
    n = pd.N if index is None else len(index)

    def half(step):
        check(lib.uammd_verletnve(step, _ptr(pd.getPos("readwrite")), _ptr(pd.getVel("readwrite")), _ptr(pd.getForce("read")), _ptr(mass),
                                  default_mass, _ptr(index), n, dt, 0, current_stream()))

    def forces():
        pd.getForce("write").zero_()
        pf.sum(force=True)
    forces()
    for _ in range(steps):
        half(1)
        forces()
        half(2)
    torch.cuda.synchronize()


def _bits(t):
    return t.cpu().numpy().view(np.uint32)


def test_nve_sequencing_and_updatables():
    hip = _hip()
    pd, box, pf, _, _ = _lj_system()
    pd2, _, pf2, _, _ = _lj_system()
    verlet = hip.VerletNVE(pd, dt=LJ["dt"], initVelocities=False)
    verlet.addInteractor(pf)
    rec = _Recorder()
    verlet.addUpdatable(rec)
    verlet.addUpdatable(rec)                       # (added twice, hears once)
    for _ in range(3):
        verlet.forwardTime()
    _by_hand(pd2, pf2, 3, LJ["dt"])
    assert np.array_equal(_bits(pd.getPos()), _bits(pd2.getPos())) and np.array_equal(_bits(pd.getVel()), _bits(pd2.getVel()))
    assert np.array_equal(_bits(pd.getForce()), _bits(pd2.getForce()))
    assert rec.heard[0] == ("dt", LJ["dt"]) and [h[0] for h in rec.heard] == ["dt", "t", "t", "t"]
    assert np.allclose([h[1] for h in rec.heard[1:]], [k * LJ["dt"] for k in (1, 2, 3)], rtol=1e-12)
    moved = np.abs(pd.getPos().cpu().numpy()[:, :3] - lattice_positions(LJ["n"], LJ["L"], seed=31, jitter=0.05)[:, :3]).max()
    assert 1e-4 < moved < 0.1


def test_nve_init_velocities_target_energy():
    hip = _hip()
    pd, box, pf, pos, _ = _lj_system()
    target = 2.0
    verlet = hip.VerletNVE(pd, dt=LJ["dt"], energy=target, initVelocities=True)
    verlet.addInteractor(pf)
    rec = _Recorder(pd)
    verlet.addUpdatable(rec)
    verlet.forwardTime()
    v = rec.vel.astype(np.float64)                 # the module's velocities before the first kick
    pd2, _, pf2, _, _ = _lj_system()
    pd2.getEnergy("write").zero_()
    pf2.sum(force=False, energy=True)
    torch.cuda.synchronize()
    U = pd2.getEnergy("read").cpu().numpy().astype(np.float64).sum() / pd.N
    K = 0.5 * (v * v).sum() / pd.N
    speed = np.sqrt((v * v).sum(1))
    print(f"U/N = {U:.6f}, K/N = {K:.6f}, U/N + K/N = {U + K:.7f} (target {target}), speed spread {np.ptp(speed) / speed.mean():.2e}")
    assert abs(U + K - target) <= 1e-5 * abs(target)
    assert np.ptp(speed) <= 1e-6 * speed.mean()
    # directions are spread over the sphere
    assert np.abs((v / speed[:, None]).mean(0)).max() < 0.15
    # a target below U cannot be met
    pd3, _, pf3, _, _ = _lj_system()
    bad = hip.VerletNVE(pd3, dt=LJ["dt"], energy=U - 1.0, initVelocities=True)
    bad.addInteractor(pf3)
    with pytest.raises(RuntimeError, match="Cannot fix energy"):
        bad.forwardTime()


def test_nve_energy_conservation():
    """N = 500, rho* = 0.8, rc = 2.5 (shifted), dt = 0.002, 2000 steps from the same state on the GPU and in float64 NumPy: the largest
    excursion max_t |E(t) - E(0)| / N on the GPU stays below twice the restatement's.
    Measured on MI355X (gfx950): gpu 1.802e-04, float64 1.802e-04 (E(0)/N = -2.839837 on both)."""
    hip = _hip()
    steps = 2000
    pd, box, pf, pos, vel = _lj_system(seed=32, vel_scale=1.0)
    verlet = hip.VerletNVE(pd, dt=LJ["dt"], initVelocities=False)
    verlet.addInteractor(pf)

    def energy():
        e = pd.getEnergy("write")
        e.zero_()
        pf.sum(force=False, energy=True)
        return e.double().sum() + 0.5 * pd.getVel("read").double().pow(2).sum()

    E = [energy()]
    for _ in range(steps):
        verlet.forwardTime()
        E.append(energy())
    E = torch.stack(E).cpu().numpy()
    Eref = dpd_ref.nve_run_lj(pos, vel, LJ["L"], LJ["rc"], LJ["dt"], steps)
    gpu, ref = np.abs(E - E[0]).max() / pd.N, np.abs(Eref - Eref[0]).max() / pd.N
    print(f"E(0)/N: gpu {E[0] / pd.N:.6f} float64 {Eref[0] / pd.N:.6f}; largest excursion per particle: gpu {gpu:.3e}, float64 {ref:.3e}")
    assert abs(E[0] - Eref[0]) <= 1e-5 * abs(Eref[0])
    assert gpu <= 2.0 * ref


def test_nve_masses_and_group():
    hip = _hip()
    mass = np.random.default_rng(33).uniform(0.5, 2.0, LJ["n"]).astype(np.float32)
    # mass allocated AND par.mass given: the array wins in the kick (VerletNVE.cu:76)
    pd, box, pf, _, _ = _lj_system(mass=mass)
    verlet = hip.VerletNVE(pd, dt=LJ["dt"], initVelocities=False, mass=3.0)
    verlet.addInteractor(pf)
    verlet.forwardTime()
    pd2, _, pf2, _, _ = _lj_system(mass=mass)
    _by_hand(pd2, pf2, 1, LJ["dt"], mass=pd2.getMass("read"), default_mass=3.0)
    assert np.array_equal(_bits(pd.getVel()), _bits(pd2.getVel())) and np.array_equal(_bits(pd.getPos()), _bits(pd2.getPos()))
    pd3, _, pf3, _, _ = _lj_system()
    _by_hand(pd3, pf3, 1, LJ["dt"], mass=None, default_mass=3.0)
    assert not np.array_equal(_bits(pd.getVel()), _bits(pd3.getVel()))
    # a group of half the particles: the others do not move
    pd4, _, pf4, pos, vel = _lj_system()
    members = np.arange(0, LJ["n"], 2)
    pg = hip.ParticleGroup(pd4, members.tolist())
    verlet = hip.VerletNVE(pg, dt=LJ["dt"], initVelocities=False)
    verlet.addInteractor(pf4)
    for _ in range(2):
        verlet.forwardTime()
    p, v = pd4.getPos().cpu().numpy(), pd4.getVel().cpu().numpy()
    assert np.array_equal(p[1::2], pos[1::2]) and np.array_equal(v[1::2], vel[1::2])
    assert (np.abs(p[::2, :3] - pos[::2, :3]).max(1) > 0).all() and (np.abs(v[::2] - vel[::2]).max(1) > 0).all()
    pd5, _, pf5, _, _ = _lj_system()
    _by_hand(pd5, pf5, 2, LJ["dt"], index=pg.getIndexIterator())
    assert np.array_equal(_bits(pd4.getPos()), _bits(pd5.getPos())) and np.array_equal(_bits(pd4.getVel()), _bits(pd5.getVel()))


# ---- 7. the DPD thermostat ----------------------------------------------------------------------------------------------------------------------
def _temperature_bar(mean, err):
    ref = json.load(open(GOLD))
    bar = 4.0 * np.hypot(err, ref["stderr"])
    print(f"kinetic temperature {mean:.5f} +- {err:.5f}; float64 scheme {ref['mean']:.5f} +- {ref['stderr']:.5f} (N = {ref['N']}, "
          f"{ref['measured']} steps); difference {mean - ref['mean']:+.5f}, bar {bar:.5f}")
    assert bar <= 0.01 * ref["temperature"], "the comparison is too noisy to mean anything"
    assert abs(mean - ref["mean"]) <= bar


def test_dpd_thermostat():
    """N = 24000, rho = 3, A = 25, gamma = 4.5, kT = 1, dt = 0.01, at rest at the start: the momentum stays at zero and the kinetic
    temperature over the last 2000 of 3000 steps agrees with the float64 run of the same scheme (tests/golden/dpd) within 4 combined
    standard errors.  Measured on MI355X (gfx950): 1.00242 +- 0.00090 against 1.00264 +- 0.00136 for the float64 scheme (difference
    -0.00022, bar 0.00652); largest total-momentum component over the run 6.3e-4 (bound 2.4)."""
    hip = _hip()
    n, steps, measured = 24000, 3000, 2000
    L = (n / 3.0) ** (1.0 / 3.0)
    pos, _ = _fluid(n, L, seed=41)
    pd, box, pot, pf = _system(pos, np.zeros((n, 3), np.float32), L)
    verlet = hip.VerletNVE(pd, dt=DPD["dt"], initVelocities=False)
    verlet.addInteractor(pf)
    T, P = [], []
    for s in range(steps):
        verlet.forwardTime()
        v = pd.getVel("read").double()
        P.append(v.sum(0).abs().max())
        if s >= steps - measured:
            T.append(v.pow(2).sum() / (3.0 * n))
    T, P = torch.stack(T).cpu().numpy(), torch.stack(P).cpu().numpy()
    assert pot.step == steps + 1
    print(f"largest |total momentum| component over the run: {P.max():.3e} (bound {1e-4 * n:.3g})")
    assert P.max() <= 1e-4 * n * np.sqrt(DPD["temperature"])
    _temperature_bar(*dpd_ref.block_average(T, 20))


# ---- 8. the C++ programs -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prog", ["dpd_builtin", "dpd_user"])
def test_cxx_program(prog):
    exe = os.path.join(BUILD, prog)
    assert os.path.exists(exe), f"{exe} is not built (examples/Makefile)"
    n = 24000
    r = subprocess.run([exe, str(n), "3000", "2000"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("dpd N")][-1].split()
    mean, err, p = float(line[4]), float(line[6]), np.array([float(x) for x in line[8:11]])
    print(" ".join(line))
    assert int(line[2]) == n
    assert np.abs(p).max() <= 1e-4 * n
    _temperature_bar(mean, err)
