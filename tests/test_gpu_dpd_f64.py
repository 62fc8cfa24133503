"""DPD in double on the GPU (uammd_amd/csrc/dpd_f64.hip, f64.PairForcesDPD) against the float64 NumPy restatement tests/dpd_ref.py.

Bars: without the random term 2e-5 * 2^-29 of max|F_ref| (the float suite's bar carried over by the ratio of the unit roundoffs); with it
2e-6 of max|F_ref|, the f64 suite's rule where single-precision Gaussians enter (logf / sincosf differ between libm and the device by a
float ulp, and xi is Saru's single-precision Box-Muller x promoted to double)."""
import math

import numpy as np
import pytest
import torch

import dpd_ref

pytestmark = pytest.mark.gpu

S = 2.0 ** -29
TOL0 = 2e-5 * S         # temperature 0
TOLN = 2e-6             # with noise
DPD = dict(cutOff=1.0, A=25.0, gamma=4.5, temperature=1.0, dt=0.01, seed=0x5EED1234ABCD)
CASES = {"cubic": (3000, 10.0, (True, True, True)), "anisotropic_open_z": (3000, (12.5, 10.0, 8.0), (True, True, False))}


def _fluid(n, L, seed):
    rng = np.random.default_rng(seed)
    L3 = np.broadcast_to(np.asarray(L, np.float64), (3,))
    pos = np.zeros((n, 4))
    pos[:, :3] = rng.uniform(-0.5, 0.5, (n, 3)) * L3 * 0.999
    vel = rng.normal(0.0, 1.0, (n, 3))
    return pos, vel


def _sum(pf, pos, vel, group=None):
    d_pos, d_vel = torch.from_numpy(pos).cuda(), torch.from_numpy(vel).cuda()
    f = torch.zeros((len(pos), 4), dtype=torch.float64, device="cuda")
    pf.sum(d_pos, d_vel, f, None if group is None else torch.from_numpy(np.asarray(group, np.int32)).cuda())
    torch.cuda.synchronize()
    return f.cpu().numpy()


def _ref(pf, pos, vel, members=None):
    n = len(pos)
    m = np.arange(n) if members is None else np.asarray(members)
    F = np.zeros((n, 3))
    F[m] = dpd_ref.dpd_forces(pos[m], vel[m], pf.box.boxSize, tuple(pf.box.periodic), pf.rcut, pf.A, pf.gamma, pf.temperature, pf.dt,
                              seed=pf.seed, step=pf.step, keys=m, nkey=n)
    return F


def _err(got, want, what):
    e = np.abs(got[:, :3] - want).max() / np.abs(want).max()
    print(f"[{what}] max|F - F_ref| / max|F_ref| = {e:.3e}  (max|F_ref| = {np.abs(want).max():.4g})")
    return e


def _pf(L, per, **kw):
    from uammd_amd import f64
    return f64.PairForcesDPD(f64.Box(L, per), **{**DPD, **kw})


# ---- 1 -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(CASES))
def test_parity_without_noise(hip, case):
    n, L, per = CASES[case]
    pos, vel = _fluid(n, L, seed=11)
    pf = _pf(L, per, temperature=0.0)
    assert pf.uses_cell_list()
    got = _sum(pf, pos, vel)
    assert pf.step == 1
    assert _err(got, _ref(pf, pos, vel), f"{case}, kT = 0") <= TOL0
    assert not got[:, 3].any()


# ---- 2 -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("off", [None, "A", "gamma"])
@pytest.mark.parametrize("case", list(CASES))
def test_parity_with_noise(hip, case, off):
    n, L, per = CASES[case]
    pos, vel = _fluid(n, L, seed=12)
    pf = _pf(L, per, **({} if off is None else {off: 0.0}))
    assert pf.sigma == math.sqrt(2.0 * pf.temperature) / math.sqrt(pf.dt)
    got = _sum(pf, pos, vel)
    assert _err(got, _ref(pf, pos, vel), f"{case}, {off} = 0" if off else case) <= (TOL0 if off == "gamma" else TOLN)


# ---- 3 -------------------------------------------------------------------------------------------------------------------------------
def test_pair_symmetry(hip):
    """|sum F| <= 1e-5 * 2^-29 sum |F| (the float test's bound carried over), summed exactly"""
    n, L, per = CASES["cubic"]
    pos, vel = _fluid(n, L, seed=13)
    F = _sum(_pf(L, per), pos, vel)[:, :3]
    total = max(abs(math.fsum(F[:, k])) for k in range(3))
    scale = math.fsum(np.abs(F).ravel())
    print(f"[pair symmetry] |sum F| = {total:.3e}, sum |F| = {scale:.3e}, ratio {total / scale:.3e}, bar {1e-5 * S:.3e}")
    assert total <= 1e-5 * S * scale


# ---- 4 -------------------------------------------------------------------------------------------------------------------------------
def test_nbody_against_the_list_and_groups(hip):
    from uammd_amd import f64
    from uammd_amd._lib import check
    n, L, per = 3000, 10.0, (True, True, True)
    pos, vel = _fluid(n, L, seed=16)
    pf = _pf(L, per)
    a = _sum(pf, pos, vel)
    # all pairs with the same key, seed and step: the same pairs in another order
    d_pos, d_vel = torch.from_numpy(pos).cuda(), torch.from_numpy(vel).cuda()
    f = torch.zeros((n, 4), dtype=torch.float64, device="cuda")
    d3, i3 = f64._d3, f64._i3
    check(pf.lib.uammd_dpd_transverse_nbody_f64(f64._ptr(d_pos), f64._ptr(d_vel), n, d3(L), i3([1, 1, 1]), pf.rcut, pf.A, pf.gamma, pf.sigma,
                                                pf.seed, pf.step, n, f64._ptr(f), None, f64._stream()))
    torch.cuda.synchronize()
    b = f.cpu().numpy()
    err = np.abs(a - b).max() / np.abs(a).max()
    print(f"[nbody vs cell list] max |dF| / max|F| = {err:.3e}")
    assert err <= TOL0
    # a group of every other particle through d_globalIndex, on the list ...
    members = np.arange(0, n, 2)
    pf2 = _pf(L, per)
    got = _sum(pf2, pos, vel, members)
    assert pf2.uses_cell_list()
    assert _err(got, _ref(pf2, pos, vel, members), "group, cell list") <= TOLN
    assert not got[1::2].any()
    # ... and on a box of 2.9 cut-offs, where the wrapper must choose all pairs
    ns, Ls = 200, 2.9
    pos_s, vel_s = _fluid(ns, Ls, seed=17)
    pf3 = _pf(Ls, per)
    assert not pf3.uses_cell_list()
    got = _sum(pf3, pos_s, vel_s)
    assert pf3.nl is None
    assert _err(got, _ref(pf3, pos_s, vel_s), "L = 2.9, all pairs") <= TOLN
    pf4 = _pf(Ls, per)
    ms = np.arange(0, ns, 2)
    got = _sum(pf4, pos_s, vel_s, ms)
    assert _err(got, _ref(pf4, pos_s, vel_s, ms), "L = 2.9, group") <= TOLN
    assert not got[1::2].any()


# ---- 5 -------------------------------------------------------------------------------------------------------------------------------
def test_determinism_steps_and_scratch(hip):
    n, L, per = CASES["cubic"]
    pos, vel = _fluid(n, L, seed=14)
    pf = _pf(L, per)
    a = _sum(pf, pos, vel)
    pf.step -= 1                               # the same step again
    b = _sum(pf, pos, vel)
    assert np.array_equal(a.view(np.uint64), b.view(np.uint64))
    c = _sum(pf, pos, vel)                     # the next step: other noise
    assert pf.step == 2 and np.abs(c - a).max() > 1.0
    assert _err(c, _ref(pf, pos, vel), "step 2") <= TOLN
    # another N on the same interactor: the list's scratch rows follow its size
    for n2 in (4321, 1500):
        L2 = (n2 / 3.0) ** (1.0 / 3.0)
        pos2, vel2 = _fluid(n2, L2, seed=15 + n2)
        pf.box.boxSize[:] = L2
        got = _sum(pf, pos2, vel2)
        assert _err(got, _ref(pf, pos2, vel2), f"N = {n2} on the same handle") <= TOLN
