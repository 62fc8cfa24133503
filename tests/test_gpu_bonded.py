"""BondedForces / AngularBondedForces / TorsionalBondedForces on the GPU (uammd_amd/csrc/bonded.hip) against the float64 NumPy
restatement in tests/bonded_ref.py: every built-in kind, finite differences, momentum conservation of the torsional bond, the rows
following a reorder, both traversal shapes and the reference-shaped baseline, the reference's test/Bonds scenarios through
BD::EulerMaruyama, Kremer-Grest through VerletNVT::GronbechJensen, and the C++ programs of tests/cxx."""
import os
import subprocess

import numpy as np
import pytest
import torch

from bonded_ref import per_particle

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "bonds")
BUILD = os.path.join(ROOT, "examples", "_build")

# max |got - want| / max |want| per kind: the pair kinds are a handful of float operations; the angular kinds go through acos / sin and
# rsqrt, whose float32 error grows near the ends of their range.  Torsional divides by sin(phi) with phi = acos(cos phi) in float32: a
# dihedral near 0 or pi loses digits in phi (d phi ~ d cos / sin phi), measured 2.5e-3 of the largest force on 600 random bonds
TOL = {"harmonic": 2e-5, "fene": 2e-5, "fixed": 2e-5, "angular": 2e-4, "torsional": 5e-3, "fourier": 5e-4}


def _md():
    import uammd_amd as hip
    from uammd_amd import bonded
    return hip, bonded


def _pd(pos):
    hip, _ = _md()
    pos = np.asarray(pos, np.float32)
    p4 = np.zeros((len(pos), 4), np.float32)
    p4[:, :3] = pos[:, :3]
    pd = hip.ParticleData(len(pos))
    pd.setPos(p4)
    return pd


def _type(kind, L):
    hip, bonded = _md()
    box = hip.Box(L)
    return {"harmonic": bonded.BondedType.Harmonic, "fene": bonded.BondedType.FENE, "fixed": bonded.BondedType.Harmonic,
            "angular": bonded.BondedType.Angular, "torsional": bonded.BondedType.Torsional,
            "fourier": bonded.BondedType.FourierLAMMPS}[kind](box)


def _config(kind, nb, L, seed):
    """nb bonds with distinct members around random anchors: members within ~1.2 of each other, positions wrapped into the box so that
    many bonds cross the periodic boundary."""
    rng = np.random.default_rng(seed)
    m = {"harmonic": 2, "fene": 2, "fixed": 2, "angular": 3, "torsional": 4, "fourier": 4}[kind]
    anchor = rng.uniform(-L / 2, L / 2, (nb, 1, 3))
    steps = rng.normal(0, 1, (nb, m, 3))
    steps /= np.linalg.norm(steps, axis=2, keepdims=True)
    steps *= rng.uniform(0.6, 1.2, (nb, m, 1))
    steps[:, 0] = 0
    P = anchor + np.cumsum(steps, axis=1)
    P -= np.floor(P / L + 0.5) * L
    pos = P.reshape(-1, 3)
    ids = np.arange(nb * m, dtype=np.int32).reshape(nb, m)
    info = np.stack([rng.uniform(1, 10, nb), rng.uniform(0.5, 1.0, nb) if kind != "fene" else np.full(nb, 1.5)], axis=1)
    if kind == "angular":
        info[:, 1] = rng.uniform(0, np.pi, nb)
        info[: nb // 8, 1] = 0.0                   # the ang0 == 0 branch
    if kind in ("torsional", "fourier"):
        info[:, 1] = rng.uniform(-np.pi, np.pi, nb)
    fixed = None
    if kind == "fixed":
        fixed = np.zeros((nb, 4), np.float32)
        fixed[:, :3] = P[:, 1]
        ids[:, 1] = -(np.arange(nb) + 1)
        pos = P[:, 0]
        ids[:, 0] = np.arange(nb)
    # repeat members: every particle is in several bonds (rows longer than one entry)
    if kind not in ("fixed",):
        extra = ids[rng.permutation(nb)].copy()
        extra = np.roll(extra, 1, axis=1)
        keep = np.array([len(set(r)) == m for r in extra])
        ids = np.concatenate([ids, extra[keep]])
        info = np.concatenate([info, info[: keep.sum()]])
    return pos.astype(np.float32), ids.astype(np.int32), info.astype(np.float32), fixed


def _sum(bf, pd, force, energy, virial):
    N = pd.N
    pd.getForce("write").zero_()
    pd.getEnergy("write").zero_()
    pd.getVirial("write").zero_()
    bf.sum(force=force, energy=energy, virial=virial)
    torch.cuda.synchronize()
    return (pd.getForce().cpu().numpy()[:, :3].astype(np.float64), pd.getEnergy().cpu().numpy().astype(np.float64),
            pd.getVirial().cpu().numpy().astype(np.float64), N)


def _cls(kind):
    _, bonded = _md()
    return {2: bonded.BondedForces, 3: bonded.AngularBondedForces, 4: bonded.TorsionalBondedForces}[_type(kind, 1.0).members]


def _err(got, want, scale=None):
    s = np.abs(want).max() if scale is None else scale
    return np.abs(got - want).max() / (s if s > 0 else 1.0)


@pytest.mark.parametrize("kind", ["harmonic", "fene", "fixed", "angular", "torsional", "fourier"])
def test_kind_against_numpy(kind):
    L = 8.0
    pos, ids, info, fixed = _config(kind, 600, L, seed=list(TOL).index(kind))
    pd = _pd(pos)
    bf = _cls(kind)(pd, bondType=_type(kind, L), ids=ids, info=info, fixedPoints=fixed)
    f_ref, e_ref, v_ref = per_particle("harmonic" if kind == "fixed" else kind, pd.getPos().cpu().numpy(), ids, info, [L] * 3,
                                       fixedPoints=fixed)
    assert np.abs(f_ref).max() > 0
    for req in [(True, False, False), (False, True, False), (False, False, True), (True, True, True)]:
        f, e, v, _ = _sum(bf, pd, *req)
        if req[0]:
            assert _err(f, f_ref) < TOL[kind], (kind, req, _err(f, f_ref))
        else:
            assert not f.any()
        if req[1]:
            assert _err(e, e_ref) < TOL[kind], (kind, req, _err(e, e_ref))
        else:
            assert not e.any()
        if req[2]:
            # (FourierLAMMPS's per-member virial is identically zero in exact arithmetic: each term is dot(cross(w, r), r); rounding
            # is measured against the force scale, the bonds being ~1 long)
            vs = max(np.abs(v_ref).max(), np.abs(f_ref).max())
            assert _err(v, v_ref, vs) < TOL[kind], (kind, req, _err(v, v_ref, vs))
        else:
            assert not v.any()
    if kind in ("angular", "torsional"):     # the reference computes neither energy nor virial for these
        _, e, v, _ = _sum(bf, pd, True, True, True)
        assert not e.any() and not v.any()


@pytest.mark.parametrize("kind", ["harmonic", "fene", "fourier"])
def test_finite_differences(kind):
    L = 8.0
    pos, ids, info, fixed = _config(kind, 12, L, seed=5)
    pd = _pd(pos)
    bf = _cls(kind)(pd, bondType=_type(kind, L), ids=ids, info=info, fixedPoints=fixed)
    f, _, _, N = _sum(bf, pd, True, False, False)
    p0 = pd.getPos().cpu().numpy().copy()
    h = 2e-3
    for i in range(0, N, max(1, N // 6)):
        for d in range(3):
            E = []
            for s in (+1, -1):
                p = p0.copy()
                p[i, d] += s * h
                pd.setPos(p)
                E.append(_sum(bf, pd, False, True, False)[1].sum())
            fd = -(E[0] - E[1]) / (2 * h)
            assert abs(fd - f[i, d]) <= 2e-2 * max(1.0, np.abs(f).max()), (kind, i, d, fd, f[i, d])
    pd.setPos(p0)


def test_torsional_net_force_and_torque_vanish():
    """each torsional bond alone: the four members' forces add to zero and so do their torques.  The reference's shifted member mapping
    (ids[1..4]) breaks both."""
    L = 8.0
    pos, ids, info, _ = _config("torsional", 500, L, seed=11)
    ids, info = ids[:500], info[:500]          # disjoint bonds: a particle's force is its one bond's share
    pd = _pd(pos)
    bf = _md()[1].TorsionalBondedForces(pd, bondType=_type("torsional", L), ids=ids, info=info)
    f, _, _, _ = _sum(bf, pd, True, False, False)
    P = pd.getPos().cpu().numpy()[:, :3].astype(np.float64)
    F = f[ids]                                  # [nb, 4, 3]
    R = P[ids]
    R = R - R[:, :1]
    R -= np.floor(R / L + 0.5) * L               # unwrapped around member 0
    scale = np.abs(F).max()
    assert scale > 0
    assert np.abs(F.sum(axis=1)).max() <= 1e-5 * scale
    assert np.abs(np.cross(R, F).sum(axis=1)).max() <= 1e-4 * scale


def test_rows_follow_sort_particles():
    hip, bonded = _md()
    L = 8.0
    pos, ids, info, _ = _config("fourier", 400, L, seed=3)
    pd = _pd(pos)
    bf = bonded.TorsionalBondedForces(pd, bondType=_type("fourier", L), ids=ids, info=info)
    f0, e0, v0, N = _sum(bf, pd, True, True, True)
    id0 = pd.id.cpu().numpy().copy()
    pd.hintSortByHash(hip.Box(L), 1.0)
    pd.sortParticles()
    id1 = pd.id.cpu().numpy()
    assert not np.array_equal(id0, id1)
    f1, e1, v1, _ = _sum(bf, pd, True, True, True)
    byid = lambda a, idv: a[np.argsort(idv)]  # noqa: E731
    assert np.array_equal(byid(f1, id1), byid(f0, id0))
    assert np.array_equal(byid(e1, id1), byid(e0, id0))
    assert np.array_equal(byid(v1, id1), byid(v0, id0))


def _chain_melt(n, length, L, rng):
    nchains = n // length
    steps = rng.normal(0, 1, (nchains, length, 3))
    steps /= np.linalg.norm(steps, axis=2, keepdims=True)
    steps[:, 0] = rng.uniform(-L / 2, L / 2, (nchains, 3))
    P = np.cumsum(steps, axis=1).reshape(-1, 3)
    P -= np.floor(P / L + 0.5) * L
    b = np.arange(n).reshape(nchains, length)
    ids = np.stack([b[:, :-1].ravel(), b[:, 1:].ravel()], axis=1).astype(np.int32)
    return P.astype(np.float32), ids


def _dense_graph(n, maxPartners, L, rng):
    cnt = rng.integers(0, maxPartners + 1, n)
    first = np.repeat(np.arange(n), cnt)
    second = rng.integers(0, n, first.size)
    second = np.where(second == first, (second + 1) % n, second)
    return rng.uniform(-L / 2, L / 2, (n, 3)).astype(np.float32), np.stack([first, second], axis=1).astype(np.int32)


@pytest.mark.parametrize("workload", ["chain", "dense"])
def test_both_shapes_and_baseline(workload):
    _, bonded = _md()
    rng = np.random.default_rng(17)
    if workload == "chain":
        L = 50.0
        pos, ids = _chain_melt(100000, 100, L, rng)
    else:
        L = 20.0
        pos, ids = _dense_graph(5000, 1000, L, rng)
    info = np.stack([np.full(len(ids), 5.0), np.full(len(ids), 0.8)], axis=1).astype(np.float32)   # (the chain's steps are 1 long)
    pd = _pd(pos)
    bf = bonded.BondedForces(pd, bondType=_type("harmonic", L), ids=ids, info=info)
    rows, entries, lane, wave = bf.shape()
    assert entries == 2 * len(ids)
    if workload == "chain":
        assert wave == 0 and lane == rows
    else:
        assert wave > 0.9 * rows
    f_ref, e_ref, v_ref = per_particle("harmonic", pd.getPos().cpu().numpy(), ids, info, [L] * 3)
    a = _sum(bf, pd, True, True, True)
    b = _sum(bf, pd, True, True, True)
    for x, y in zip(a[:3], b[:3]):
        assert np.array_equal(x, y)          # bit-identical run to run
    tol = 1e-4   # (float32 with the hardware rsqrt: the energy 0.25 k (r - r0)^2 at r - r0 ~ 0.2 carries ~2e-5)
    assert _err(a[0], f_ref) < tol and _err(a[1], e_ref) < tol and _err(a[2], v_ref) < tol
    bonded.set_tunable("bonded_baseline", 1)
    try:
        c = _sum(bf, pd, True, True, True)
    finally:
        bonded.set_tunable("bonded_baseline", 0)
    assert _err(c[0], f_ref) < tol and _err(c[1], e_ref) < tol and _err(c[2], v_ref) < tol


def _bd(pos, bondText, tmp_path, steps):
    hip, bonded = _md()
    f = tmp_path / "particles.bonds"
    f.write_text(bondText)
    pd = _pd(pos)
    par = hip.BD.EulerMaruyama.Parameters(temperature=0.0, viscosity=1 / (6 * np.pi), hydrodynamicRadius=1.0, dt=0.02)
    bd = hip.BD.EulerMaruyama(pd, par)
    bd.addInteractor(bonded.BondedForces(pd, bonded.BondedForces.Parameters(file=str(f)), bonded.BondedType.Harmonic(hip.Box(32.0))))
    for _ in range(steps):
        bd.forwardTime()
    torch.cuda.synchronize()
    return pd.getPos().cpu().numpy()[:, :3].astype(np.float64)


def test_reference_pair_scenario(tmp_path):
    """test/Bonds/test.bash pairTest: two particles at x = -5 and 5, one bond k = 1 r0 = 1, BD at T = 0, dt 0.02, 500 time units."""
    p = _bd([[-5, 0, 0], [5, 0, 0]], "1\n0 1 1 1\n0\n", tmp_path, 25000)
    d = p[1] - p[0]
    assert abs(d[0] - 1) < 1e-4 and abs(d[1]) < 1e-4 and abs(d[2]) < 1e-4, d


def test_reference_chain_scenario(tmp_path):
    """test/Bonds/test.bash chainTest: ten particles at x = 2, 4, ..., 20 in a chain with r0 = 1, particle 0 tied to (-3, 0, -3)."""
    pos = [[2 * (i + 1), 0, 0] for i in range(10)]
    text = "9\n" + "".join(f"{i} {i + 1} 1 1\n" for i in range(9)) + "1\n0 -3 0 -3 1 0\n"
    p = _bd(pos, text, tmp_path, 25000)
    assert np.linalg.norm(p[0] - [-3, 0, -3]) < 1e-3
    assert np.abs(np.linalg.norm(np.diff(p, axis=0), axis=1) - 1).max() < 1e-3


def test_kremer_grest_gronbech_jensen():
    hip, bonded = _md()
    n, length = 10000, 100
    Lx, Lyz, sp = 100.0, 12.0, 0.97
    yz = (np.arange(10) + 0.5) * 1.2 - Lyz / 2
    P = np.array([[-Lx / 2 + 0.5 + sp * j, y, z] for y in yz for z in yz for j in range(length)], np.float32)
    ids = np.array([[c * length + j, c * length + j + 1] for c in range(n // length) for j in range(length - 1)], np.int32)
    L = np.array([Lx, Lyz, Lyz], np.float32)
    box = hip.Box(L)

    def system(with_bonds):
        pd = _pd(P)
        pot = hip.Potential.LJ()
        pot.setPotParameters(0, 0, pot.InputPairParameters(2 ** (1 / 6), 1.0, 1.0, True))
        lj = hip.PairForces(pd, box, pot)
        fene = bonded.BondedForces(pd, bondType=bonded.BondedType.FENE(box), ids=ids,
                                   info=np.tile(np.float32([30.0, 1.5]), (len(ids), 1)))
        par = hip.VerletNVT.GronbechJensen.Parameters(temperature=1.0, dt=0.005, friction=1.0)
        integ = hip.VerletNVT.GronbechJensen(pd, par)
        integ.addInteractor(lj)
        if with_bonds:
            integ.addInteractor(fene)
        return pd, lj, fene, integ

    pd, lj, fene, integ = system(True)
    fs = []
    for it in (lj, fene):
        pd.getForce("write").zero_()
        it.sum(force=True)
        fs.append(pd.getForce().clone())
    pd.getForce("write").zero_()
    for it in integ.getInteractors():        # what forwardTime's first step sums
        it.sum(force=True)
    assert torch.equal(pd.getForce(), fs[0] + fs[1])
    assert fs[1].abs().max() > 0
    for _ in range(1000):
        integ.forwardTime()
    torch.cuda.synchronize()
    assert integ.fused_steps == 0            # two interactors: the fused one-interactor step is not taken
    p = pd.getPos().cpu().numpy()[:, :3].astype(np.float64)
    assert np.isfinite(p).all() and np.isfinite(pd.getVel().cpu().numpy()).all()
    idx = np.argsort(pd.id.cpu().numpy())
    d = p[idx][ids[:, 1]] - p[idx][ids[:, 0]]
    d -= np.floor(d / L + 0.5) * L
    assert np.linalg.norm(d, axis=1).max() < 1.5
    pd1, _, _, integ1 = system(False)           # LJ alone: the fused step is taken (the check above tells the two apart)
    integ1.forwardTime()
    integ1.forwardTime()
    assert integ1.fused_steps > 0


def _run(prog, *args):
    exe = os.path.join(BUILD, prog)
    assert os.path.exists(exe), f"{exe}: run build() first"
    r = subprocess.run([exe, *args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout


def test_cxx_builtin_kinds_on_reference_files():
    out = _run("bonds_builtin", GOLD)
    rows = {}
    for line in out.splitlines():
        t = line.split()
        if len(t) == 7:
            rows.setdefault(t[0], []).append([float(x) for x in t[2:]])
    with open(os.path.join(GOLD, "init.pos")) as f:
        tok = f.read().split()
    pos = np.array(tok[1:1 + 3 * int(tok[0])], np.float64).reshape(-1, 3)
    from uammd_amd.bonded import read_bond_file
    for kind, fn, m in (("harmonic", "harmonic.bonds", 2), ("angular", "angular.bonds", 3), ("torsional", "torsional.bonds", 4)):
        ids, info, _ = read_bond_file(os.path.join(GOLD, fn), m)
        f, e, v = per_particle(kind, pos, ids, info, [32.0] * 3)
        got = np.array(rows[kind])
        assert got.shape == (4, 5)
        assert _err(got[:, :3], f) < TOL[kind], kind
        assert _err(got[:, 3], e) < TOL[kind] and _err(got[:, 4], v) < TOL[kind], kind


def test_cxx_user_bond_type(tmp_path):
    out = _run("bonds_user", str(tmp_path))
    from uammd_amd.bonded import read_bond_file
    for name, fn, L in (("chain", "chain.bonds", 40.0), ("dense", "dense.bonds", 12.0)):
        t = np.array([[float(x) for x in line.split()[1:]] for line in out.splitlines() if line.startswith(name + " ")])
        order = np.argsort(t[:, 0])
        t = t[order]
        pos, got = t[:, 1:4], t[:, 4:]
        ids, info, _ = read_bond_file(str(tmp_path / fn), 2)
        k = info[:, 0].astype(np.float64) * 1.5             # k (1 + t) at t = 0.5: the ParameterUpdatable kind heard the update
        d = pos[ids[:, 1]] - pos[ids[:, 0]]
        d -= np.floor(d / L + 0.5) * L
        r = np.linalg.norm(d, axis=1)
        fmag = (k * (r - info[:, 1]) / r)[:, None]
        F = np.zeros((len(pos), 3))
        np.add.at(F, ids[:, 0], fmag * d)
        np.add.at(F, ids[:, 1], -fmag * d)
        E = np.zeros(len(pos))
        e = 0.25 * k * (r - info[:, 1]) ** 2
        np.add.at(E, ids[:, 0], e)
        np.add.at(E, ids[:, 1], e)
        assert _err(got[:, :3], F) < 1e-4, name
        assert _err(got[:, 3], E) < 1e-4, name
