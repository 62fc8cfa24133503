"""Bonded forces in double on the GPU (uammd_amd/csrc/bonded_f64.hip, f64.BondedForces) against the float64 NumPy restatement in
tests/bonded_ref.py.

Bars: the float suite's TOL of each kind times 2^-29 (the ratio of the unit roundoffs), relative to max|ref| as in that suite.  The
angular and torsional bars include the conditioning of acos near +-1, so the fixtures keep every bond angle and dihedral at least 0.05 rad
from 0 and pi (asserted where they are built).  Measured errors are printed."""
import ctypes as C

import numpy as np
import pytest
import torch

from bonded_ref import KIND_MEMBERS, per_particle

pytestmark = pytest.mark.gpu

S = 2.0 ** -29
TOL = {"harmonic": 2e-5 * S, "fene": 2e-5 * S, "fixed": 2e-5 * S, "angular": 2e-4 * S, "torsional": 5e-3 * S, "fourier": 5e-4 * S}
L = 12.0
MARGIN = 0.05


def _angles(P):
    """bond angles (between successive bond vectors) and dihedrals (between successive bond planes) along chains P[c, b, 3]"""
    d = np.diff(P, axis=1)
    u = d / np.linalg.norm(d, axis=2, keepdims=True)
    th = np.arccos(np.clip((u[:, :-1] * u[:, 1:]).sum(-1), -1, 1))
    n = np.cross(d[:, :-1], d[:, 1:])
    n /= np.linalg.norm(n, axis=2, keepdims=True)
    ph = np.arccos(np.clip((n[:, :-1] * n[:, 1:]).sum(-1), -1, 1))
    return th, ph


def _chains(nchains=64, beads=8, seed=1, margin=MARGIN):
    """Random-walk chains with bonds 0.8 to 1.15 long; a step is drawn again until its bond angle and dihedral keep `margin` from 0 and pi.
    Returns the unwrapped chains P[c, b, 3]."""
    rng = np.random.default_rng(seed)
    P = np.zeros((nchains, beads, 3))
    for c in range(nchains):
        P[c, 0] = rng.uniform(-L / 2, L / 2, 3)
        for b in range(1, beads):
            while True:
                u = rng.normal(0, 1, 3)
                P[c, b] = P[c, b - 1] + u / np.linalg.norm(u) * rng.uniform(0.8, 1.15)
                th, ph = _angles(P[c:c + 1, :b + 1]) if b >= 2 else (np.array([1.0]), np.array([1.0]))
                if min(th.min(), np.pi - th.max()) >= margin and (ph.size == 0 or min(ph.min(), np.pi - ph.max()) >= margin):
                    break
    th, ph = _angles(P)
    assert min(th.min(), np.pi - th.max()) >= margin and min(ph.min(), np.pi - ph.max()) >= margin
    return P


def _stored(P, seed=2):
    """rows wrapped into the box (so bonds cross its faces) and then moved by -1, 0 or +1 box lengths: stored up to 1.5 L away"""
    rng = np.random.default_rng(seed)
    x = P.reshape(-1, 3)
    x = x - np.floor(x / L + 0.5) * L
    x = x + L * rng.integers(-1, 2, x.shape)
    assert np.abs(x).max() <= 1.5 * L and np.abs(x).max() > 0.5 * L
    pos = np.zeros((len(x), 4))
    pos[:, :3] = x
    return pos


def _bonds(kind, nchains, beads, seed=3):
    """ids along the chains (bonds, angles or dihedrals) and info in the file's order "k p0" """
    rng = np.random.default_rng(seed)
    m = KIND_MEMBERS[kind]
    first = (np.arange(nchains)[:, None] * beads + np.arange(beads - m + 1)[None, :]).reshape(-1)
    ids = (first[:, None] + np.arange(m)[None, :]).astype(np.int32)
    nb = len(ids)
    if kind == "harmonic":
        info = np.stack([rng.uniform(1, 10, nb), rng.uniform(0.5, 1.0, nb)], 1)
    elif kind == "fene":
        info = np.stack([rng.uniform(1, 30, nb), np.full(nb, 1.5)], 1)
    elif kind == "angular":
        info = np.stack([rng.uniform(1, 10, nb), rng.uniform(0.1, np.pi - 0.1, nb)], 1)
        info[: nb // 8, 1] = 0.0                   # the ang0 == 0 branch
    else:
        info = np.stack([rng.uniform(1, 10, nb), rng.uniform(-np.pi, np.pi, nb)], 1)
    return ids, info


_cache = {}


def _fixture(kind):
    """positions, bonds and the float64 restatement's answer: computed once and shared (never modified)"""
    if kind not in _cache:
        base = "harmonic" if kind in ("fixed", "fixed-fene") else kind
        P = _chains()
        pos = _stored(P)
        fixed = None
        if kind in ("fixed", "fixed-fene"):
            base = "harmonic" if kind == "fixed" else "fene"
            rng = np.random.default_rng(7)
            ids, info = _bonds(base, 64, 8)
            who = rng.permutation(len(pos))[:32]
            u = rng.normal(0, 1, (32, 3))
            fixed = np.zeros((32, 4))
            fixed[:, :3] = P.reshape(-1, 3)[who] + u / np.linalg.norm(u, axis=1)[:, None] * rng.uniform(0.5, 1.1, (32, 1))
            ids = np.concatenate([ids, np.stack([who, -(np.arange(32) + 1)], 1).astype(np.int32)])
            info = np.concatenate([info, np.stack([rng.uniform(1, 10, 32), np.full(32, 0.7 if base == "harmonic" else 1.5)], 1)])
        else:
            ids, info = _bonds(base, 64, 8)
        ref = per_particle(base, pos, ids, info, [L] * 3, fixedPoints=fixed)
        for a in (pos, ids, info) + tuple(ref):
            a.setflags(write=False)
        _cache[kind] = dict(base=base, pos=pos, ids=ids, info=info, fixed=fixed, ref=ref)
    return _cache[kind]


def _interactor(fx):
    from uammd_amd import f64
    bf = f64.BondedForces(fx["base"], fx["ids"], fx["info"], f64.Box(L), fixedPoints=fx["fixed"])
    n = len(fx["pos"])
    bf.refresh(torch.arange(n, dtype=torch.int32, device="cuda"))
    return bf


def _sum(bf, d_pos, req=(True, True, True)):
    n = d_pos.shape[0]
    f = torch.zeros((n, 4), dtype=torch.float64, device="cuda") if req[0] else None
    e = torch.zeros(n, dtype=torch.float64, device="cuda") if req[1] else None
    v = torch.zeros(n, dtype=torch.float64, device="cuda") if req[2] else None
    bf.sum(d_pos, f, e, v)
    torch.cuda.synchronize()
    return tuple(None if t is None else t.cpu().numpy() for t in (f, e, v))


def _err(got, want, scale=None):
    s = np.abs(want).max() if scale is None else scale
    return np.abs(got - want).max() / (s if s > 0 else 1.0)


def _check(kind, got, ref, label):
    f, e, v = got
    f_ref, e_ref, v_ref = ref
    ef = _err(f[:, :3], f_ref)
    ee = _err(e, e_ref)
    # (FourierLAMMPS's per-member virial is identically zero in exact arithmetic: rounding is measured against the force scale)
    ev = _err(v, v_ref, max(np.abs(v_ref).max(), np.abs(f_ref).max()))
    print(f"[{label}] rel err F {ef:.3e} E {ee:.3e} V {ev:.3e}, bar {TOL[kind]:.3e}")
    assert ef <= TOL[kind] and ee <= TOL[kind] and ev <= TOL[kind]
    assert not f[:, 3].any()


# ---- 1 -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["harmonic", "fene", "fixed", "fixed-fene", "angular", "torsional", "fourier"])
def test_kind_against_numpy(hip, kind):
    fx = _fixture(kind)
    bar = "fixed" if kind.startswith("fixed") else kind
    bf = _interactor(fx)
    d_pos = torch.from_numpy(np.array(fx["pos"])).cuda()
    assert np.abs(fx["ref"][0]).max() > 0
    _check(bar, _sum(bf, d_pos), fx["ref"], kind)
    f, e, v = _sum(bf, d_pos, (True, False, False))            # forces alone: the same bits as with energy and virial
    assert e is None and np.array_equal(f, _sum(bf, d_pos)[0])
    if kind in ("angular", "torsional"):                       # the reference computes neither energy nor virial for these
        _, e, v = _sum(bf, d_pos)
        assert not e.any() and not v.any()


# ---- 2 -------------------------------------------------------------------------------------------------------------------------------
def test_both_shapes(hip):
    """A hub with 200 harmonic bonds among chain rows of 1 to 4 entries: the wave-per-row shape for the hub at the default threshold, for
    every row with two entries or more at 1, for none at 1000; within the bar and the same bits run to run at each."""
    from uammd_amd import f64
    from uammd_amd._lib import check, load
    lib = load()
    fx = _fixture("harmonic")
    n = len(fx["pos"])
    rng = np.random.default_rng(5)
    pos = np.concatenate([fx["pos"], [[0.3, -0.2, 0.1, 0.0]]])
    spokes = rng.permutation(n)[:200]
    ids = np.concatenate([fx["ids"], np.stack([np.full(200, n), spokes], 1).astype(np.int32)])
    info = np.concatenate([fx["info"], np.stack([rng.uniform(1, 10, 200), rng.uniform(0.5, 3.0, 200)], 1)])
    ref = per_particle("harmonic", pos, ids, info, [L] * 3)
    bf = f64.BondedForces("harmonic", ids, info, f64.Box(L))
    bf.refresh(torch.arange(n + 1, dtype=torch.int32, device="cuda"))
    d_pos = torch.from_numpy(pos).cuda()
    try:
        for thr, waves in ((32, 1), (1, None), (1000, 0)):
            check(lib.uammd_hip_set_tunable(b"bonded_wave_threshold", thr))
            rows, entries, lane, wave = bf.shape()
            assert rows == n + 1 and entries == 2 * len(ids) and lane + wave == rows
            if waves is not None:
                assert wave == waves
            else:
                assert wave > 200 and lane > 0                 # chain ends have one entry
            if thr == 32:
                assert lane > 0 and wave > 0                   # both shapes in use
            a = _sum(bf, d_pos)
            _check("harmonic", a, ref, f"hub, threshold {thr}")
            b = _sum(bf, d_pos)
            for x, y in zip(a, b):
                assert np.array_equal(x.view(np.uint64), y.view(np.uint64))
    finally:
        check(lib.uammd_hip_set_tunable(b"bonded_wave_threshold", 32))


# ---- 3 -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["harmonic", "fene", "fourier"])
def test_energy_derivative_is_the_force(hip, kind):
    """Central differences of the summed energy with h = 1e-5 reproduce EVERY force component to 1e-8 max(1, max|F|): truncation
    ~ h^2 E''' / 6 and rounding ~ u |E| / h are both below 1e-9 on this fixture (8 chains of 8 beads; bond angles at least 0.5 rad from 0
    and pi, because the third derivative of a dihedral grows as 1 / sin^3 of the bond angles)."""
    from uammd_amd import f64
    P = _chains(8, 8, seed=21, margin=0.5)
    pos = _stored(P, seed=22)
    ids, info = _bonds(kind, 8, 8, seed=23)
    n = len(pos)
    bf = f64.BondedForces(kind, ids, info, f64.Box(L))
    bf.refresh(torch.arange(n, dtype=torch.int32, device="cuda"))
    d_pos = torch.from_numpy(pos).cuda()
    f = _sum(bf, d_pos, (True, False, False))[0]
    h = 1e-5
    e = torch.zeros(n, dtype=torch.float64, device="cuda")

    def energy():
        e.zero_()
        bf.sum(d_pos, None, e, None)
        return float(e.sum())

    worst = 0.0
    for i in range(n):
        for d in range(3):
            x0 = float(pos[i, d])
            d_pos[i, d] = x0 + h
            ep = energy()
            d_pos[i, d] = x0 - h
            em = energy()
            d_pos[i, d] = x0
            worst = max(worst, abs(-(ep - em) / (2 * h) - f[i, d]))
    bar = 1e-8 * max(1.0, np.abs(f).max())
    print(f"[{kind}] max |dE/dx + F| = {worst:.3e}, bar {bar:.3e}, max|F| {np.abs(f).max():.3f}")
    assert worst <= bar


# ---- 4 -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["fene", "fourier"])
def test_rows_follow_a_reorder(hip, kind):
    fx = _fixture(kind)
    bf = _interactor(fx)
    n = len(fx["pos"])
    d_pos = torch.from_numpy(np.array(fx["pos"])).cuda()
    before = _sum(bf, d_pos)
    id2index = np.random.default_rng(31).permutation(n).astype(np.int32)       # the particle with id i now sits at id2index[i]
    moved = np.zeros_like(fx["pos"])
    moved[id2index] = fx["pos"]
    bf.refresh(torch.from_numpy(id2index).cuda())
    after = _sum(bf, torch.from_numpy(moved).cuda())
    for a, b in zip(before, after):
        assert np.array_equal(b[id2index].view(np.uint64), a.view(np.uint64))


# ---- 5 -------------------------------------------------------------------------------------------------------------------------------
def test_torsional_net_force_and_torque_vanish(hip):
    """each torsional bond alone: the four members' forces and torques add to zero, to the float test's bounds x 2^-29"""
    from uammd_amd import f64
    P = _chains()
    pos = _stored(P)
    ids, info = _bonds("torsional", 64, 8)
    ids, info = ids.reshape(64, 5, 4)[:, ::4].reshape(-1, 4), info.reshape(64, 5, 2)[:, ::4].reshape(-1, 2)     # beads 0-3 and 4-7: disjoint
    bf = f64.BondedForces("torsional", ids, info, f64.Box(L))
    bf.refresh(torch.arange(len(pos), dtype=torch.int32, device="cuda"))
    f = _sum(bf, torch.from_numpy(pos).cuda(), (True, False, False))[0][:, :3]
    F = f[ids]
    R = pos[:, :3][ids]
    R = R - R[:, :1]
    R -= np.floor(R / L + 0.5) * L               # unwrapped around member 0
    scale = np.abs(F).max()
    net, torque = np.abs(F.sum(axis=1)).max() / scale, np.abs(np.cross(R, F).sum(axis=1)).max() / scale
    print(f"[torsional] net force {net:.3e} (bar {1e-5 * S:.3e}), net torque {torque:.3e} (bar {1e-4 * S:.3e}) of max|F| = {scale:.3f}")
    assert scale > 0 and net <= 1e-5 * S and torque <= 1e-4 * S


# ---- 6 -------------------------------------------------------------------------------------------------------------------------------
def test_refusals(hip):
    """sum before refresh, refresh with too few particles, a fixed point beyond nfixed: an error code and a message each, and the next
    valid call still works."""
    from uammd_amd import f64
    from uammd_amd._lib import UammdHipError
    fx = _fixture("harmonic")
    n = len(fx["pos"])
    d_pos = torch.from_numpy(np.array(fx["pos"])).cuda()
    f = torch.zeros((n, 4), dtype=torch.float64, device="cuda")
    bf = f64.BondedForces("harmonic", fx["ids"], fx["info"], f64.Box(L))
    with pytest.raises(UammdHipError, match="uploaded and refreshed"):
        bf.sum(d_pos, f)
    with pytest.raises(UammdHipError, match=f"names particle {n - 1}, there are {n - 1}"):
        bf.refresh(torch.arange(n - 1, dtype=torch.int32, device="cuda"))
    with pytest.raises(UammdHipError, match="uploaded and refreshed"):
        bf.sum(d_pos, f)
    assert not f.any()
    bf.refresh(torch.arange(n, dtype=torch.int32, device="cuda"))
    bf.sum(d_pos, f)
    torch.cuda.synchronize()
    assert _err(f.cpu().numpy()[:, :3], fx["ref"][0]) <= TOL["harmonic"]
    bad = np.array([[0, -2]], np.int32)                      # fixed point 1 of 1
    with pytest.raises(UammdHipError, match="fixed point 1, there are 1"):
        f64.BondedForces("harmonic", bad, [[1.0, 1.0]], f64.Box(L), fixedPoints=np.zeros((1, 4)))
    # a failed upload leaves a handle as it was
    ids = np.ascontiguousarray(bad)
    info = np.ones((1, 2))
    fp = np.zeros((1, 4))
    d3, i3 = C.c_double * 3, C.c_int * 3
    assert bf.lib.uammd_bonded_upload_f64(bf.h, 0, 1, ids.ctypes.data_as(C.c_void_p), info.ctypes.data_as(C.c_void_p), 1,
                                          fp.ctypes.data_as(C.c_void_p), d3(L, L, L), i3(1, 1, 1)) == -1
    f.zero_()
    bf.sum(d_pos, f)
    torch.cuda.synchronize()
    assert _err(f.cpu().numpy()[:, :3], fx["ref"][0]) <= TOL["harmonic"]
