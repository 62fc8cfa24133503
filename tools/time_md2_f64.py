#!/usr/bin/env python
"""Event timing of the double-precision Verlet list, bonded and DPD kernels next to their single-precision counterparts on the same input
(tools, not part of bench.py's contract; sibling of time_lj_f64.py).  Every figure is the mean of REPS (20) launches between two device
events after a warm-up launch of the same shape; f64 and f32 alternate within each of three runs.  The figures go to stdout and, as JSON,
to the file named by OUT.
  verlet list  1e6-particle melted LJ box (the state time_lj_f64.py prepares): traversal, forced rebuild, drift-only update
  bonded       1000 chains of 100 beads (1e5), FENE bonds and FourierLAMMPS dihedrals along the chains
  dpd          1e5 particles at rho = 3, rc = 1: the cell-list transverser on a built list
usage: python tools/time_md2_f64.py [verlet|bonded|dpd ...]"""
import ctypes as C
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch
import uammd_amd as hip
from uammd_amd import _lib, bonded, f64
from uammd_amd._lib import check, f3, i3
from util import lattice_positions

what = sys.argv[1:] or ["verlet", "bonded", "dpd"]
reps = int(os.environ.get("REPS", "20"))
lib = _lib.load()
out = {"reps": reps}


def timed(fn):
    fn(); torch.cuda.synchronize()          # warm-up of this shape
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def runs(pairs):
    res = []
    for run in range(3):
        r = {name: timed(fn) for name, fn in pairs}
        res.append(r)
        print(f"run {run}: " + ", ".join(f"{k} {v:.4f}" for k, v in r.items()), flush=True)
    return res


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


if "verlet" in what:
    n = int(os.environ.get("N_VERLET", "1000000"))
    L = 107.7217345 * (n / 1e6) ** (1 / 3)
    pd = hip.ParticleData(n, seed=1234)
    pd.setPos(lattice_positions(n, L, seed=1234, jitter=0.1))
    box = hip.Box(L)
    pot = hip.Potential.LJ(); pot.setPotParameters(0, 0, pot.InputPairParameters(2.5, 1.0, 1.0, False))
    integ = hip.VerletNVT.GronbechJensen(pd, hip.VerletNVT.GronbechJensen.Parameters(temperature=1.0, dt=0.005, friction=1.0))
    pf = hip.PairForces(pd, box, pot); pf.algo = 7
    integ.addInteractor(pf)
    pd.hintSortByHash(box, [2.5] * 3)
    for _ in range(int(os.environ.get("MELT", "300"))):
        integ.forwardTime()
    pd.sortParticles()
    integ.forwardTime()
    pos32 = pd.getPos("read").clone()
    g = torch.Generator(device="cuda").manual_seed(5)
    pos64 = pos32.double()
    pos64[:, :3] += (torch.rand((n, 3), generator=g, device="cuda", dtype=torch.float64) - 0.5) * 2e-7
    box64 = f64.Box(L)
    pot64 = f64.LJ(); pot64.setPotParameters(0, 0, pot64.InputPairParameters(2.5, 1.0, 1.0, False))
    vl32, vl64 = hip.VerletList(), f64.VerletList()
    vl32.update(box, 2.5, pos32)
    vl64.update(box64, 2.5, pos64)
    f_32 = torch.zeros((n, 4), dtype=torch.float32, device="cuda")
    f_64 = torch.zeros((n, 4), dtype=torch.float64, device="cuda")

    def rebuild32():
        vl32._handle_reorder(); vl32.update(box, 2.5, pos32)

    def rebuild64():
        vl64.forceNextUpdate(); vl64.update(box64, 2.5, pos64)

    def drift32():
        vl32._handle_pos_write(); vl32.update(box, 2.5, pos32)

    print(f"verlet list, n = {n}: capacity f32 {vl32.getVerletList().maxNeighboursPerParticle}, f64 {vl64.getVerletList().maxNeighboursPerParticle}")
    out["verlet"] = {"n": n, "L": L, "runs": runs([
        ("traverse_f64_ms", lambda: vl64.transverse_lj(pot64.device_table(), 1, box64, f_64)),
        ("traverse_f32_ms", lambda: vl32.transverse_lj(pot.device_table(), 1, box, f_32)),
        ("rebuild_f64_ms", rebuild64), ("rebuild_f32_ms", rebuild32),
        ("update_no_rebuild_f64_ms", lambda: vl64.update(box64, 2.5, pos64)), ("update_no_rebuild_f32_ms", drift32)])}
    del vl32, vl64, f_32, f_64, pd, pf, integ

if "bonded" in what:
    nchains, beads = 1000, 100
    n = nchains * beads
    L = 60.0
    rng = np.random.default_rng(3)
    steps = rng.normal(0, 1, (nchains, beads, 3))
    steps *= 0.97 / np.linalg.norm(steps, axis=2, keepdims=True)
    steps[:, 0] = rng.uniform(-L / 2, L / 2, (nchains, 3))
    P = np.cumsum(steps, axis=1).reshape(-1, 3)
    P -= np.floor(P / L + 0.5) * L
    pos = np.zeros((n, 4)); pos[:, :3] = P
    out["bonded"] = {"n": n}
    for kind, m, info in (("fene", 2, [30.0, 1.5]), ("fourier", 4, [2.0, 0.4])):
        first = (np.arange(nchains)[:, None] * beads + np.arange(beads - m + 1)[None, :]).reshape(-1)
        ids = (first[:, None] + np.arange(m)[None, :]).astype(np.int32)
        inf = np.tile(info, (len(ids), 1))
        pd = hip.ParticleData(n)
        pd.setPos(pos.astype(np.float32))
        btype = (bonded.BondedType.FENE if kind == "fene" else bonded.BondedType.FourierLAMMPS)(hip.Box(L))
        cls = bonded.BondedForces if m == 2 else bonded.TorsionalBondedForces
        b32 = cls(pd, bondType=btype, ids=ids, info=inf.astype(np.float32))
        b64 = f64.BondedForces(kind, ids, inf, f64.Box(L))
        b64.refresh(torch.arange(n, dtype=torch.int32, device="cuda"))
        d_pos = torch.from_numpy(pos).cuda()
        f_64 = torch.zeros((n, 4), dtype=torch.float64, device="cuda")
        print(f"bonded {kind}, n = {n}, {len(ids)} bonds, shape {b64.shape()}")
        out["bonded"][kind] = runs([(f"{kind}_f64_ms", lambda: b64.sum(d_pos, f_64)), (f"{kind}_f32_ms", lambda: b32.sum(force=True))])

if "dpd" in what:
    n = 100000
    L = (n / 3.0) ** (1.0 / 3.0)
    rng = np.random.default_rng(13)
    pos = np.zeros((n, 4)); pos[:, :3] = rng.uniform(-0.5, 0.5, (n, 3)) * L * 0.999
    vel = rng.normal(0, 1, (n, 3))
    p64, v64 = torch.from_numpy(pos).cuda(), torch.from_numpy(vel).cuda()
    p32, v32 = p64.float(), v64.float()
    cl32, cl64 = hip.CellList(), f64.CellList()
    cl32.update(hip.Box(L), 1.0, p32)
    cl64.update(f64.Box(L), 1.0, p64)
    f_32 = torch.zeros((n, 4), dtype=torch.float32, device="cuda")
    f_64 = torch.zeros((n, 4), dtype=torch.float64, device="cuda")
    sigma = float(np.sqrt(2.0) / np.sqrt(0.01))
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def dpd64():
        check(lib.uammd_dpd_transverse_celllist_f64(cl64.h, ptr(v64), f64._d3(L), f64._i3(1), 1.0, 25.0, 4.5, sigma, 1234, 1, n, ptr(f_64), None, st))

    def dpd32():
        check(lib.uammd_dpd_transverse_celllist(cl32.h, ptr(v32), f3(L), i3(1), 1.0, 25.0, 4.5, sigma, 1234, 1, n, ptr(f_32), None, st))

    print(f"dpd, n = {n}, L = {L:.4f}")
    out["dpd"] = {"n": n, "L": L, "runs": runs([("dpd_f64_ms", dpd64), ("dpd_f32_ms", dpd32)])}

print(json.dumps(out), flush=True)
if os.environ.get("OUT"):
    with open(os.environ["OUT"], "w") as fh:
        json.dump(out, fh, indent=1)
