#!/usr/bin/env python
"""Traversal-only timing of the double-precision LJ kernels (GENERAL, SCAN32) next to the single-precision GENERAL kernel on one melted
C3-like configuration, and of the double-precision cell-list build (tools, not part of bench.py's contract; sibling of time_lj.py).
Three alternating runs of the three traversals on one box; the figures go to stdout and, as JSON, to the file named by OUT.
usage: python tools/time_lj_f64.py [N]"""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch
import uammd_amd as hip
from uammd_amd import f64
from util import lattice_positions

n = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
L = 107.7217345 * (n / 1e6) ** (1 / 3)
pd = hip.ParticleData(n, seed=1234)
pd.setPos(lattice_positions(n, L, seed=1234, jitter=0.1))
box = hip.Box(L)
pot = hip.Potential.LJ(); pot.setPotParameters(0, 0, pot.InputPairParameters(2.5, 1.0, 1.0, False))
integ = hip.VerletNVT.GronbechJensen(pd, hip.VerletNVT.GronbechJensen.Parameters(temperature=1.0, dt=0.005, friction=1.0))
pf = hip.PairForces(pd, box, pot); pf.algo = 7
integ.addInteractor(pf)
pd.hintSortByHash(box, [2.5] * 3)
for _ in range(int(os.environ.get("MELT", "300"))):     # the melted state time_lj.py prepares (rho* = 0.8, T = 1)
    integ.forwardTime()
pd.sortParticles()
integ.forwardTime()
cl32 = pf.nl
pos32 = pd.getPos("read")
g = torch.Generator(device="cuda").manual_seed(5)
pos64 = pos32.double()
pos64[:, :3] += (torch.rand((n, 3), generator=g, device="cuda", dtype=torch.float64) - 0.5) * 2e-7   # inputs no float holds
box64 = f64.Box(L)
pot64 = f64.LJ(); pot64.setPotParameters(0, 0, pot64.InputPairParameters(2.5, 1.0, 1.0, False))
cl64 = f64.CellList()
reps = int(os.environ.get("REPS", "20"))


def timed(fn):
    fn(); torch.cuda.synchronize()          # warm-up of this shape
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


f_32 = torch.zeros((n, 4), dtype=torch.float32, device="cuda")
f_64 = torch.zeros((n, 4), dtype=torch.float64, device="cuda")
out = {"n": n, "L": L, "reps": reps, "runs": []}
out["build_f64_ms"] = timed(lambda: cl64.update(box64, 2.5, pos64))
out["build_f32_ms"] = timed(lambda: (cl32.__setattr__("force_next_update", True), cl32.update(box, 2.5, pos32)))
forces = {}
for name, algo in (("general", 1), ("scan32", 11)):
    f_64.zero_()
    cl64.transverse_lj(pot64.device_table(), 1, box64, f_64, None, None, None, algo)
    torch.cuda.synchronize()
    forces[name] = f_64.cpu().numpy().copy()
out["scan32_words_differing_from_general"] = int((forces["general"].view(np.uint64) != forces["scan32"].view(np.uint64)).sum())
f_32.zero_()
cl32.transverse_lj(pot.device_table(), 1, box, f_32, None, None, None, 1)
torch.cuda.synchronize()
out["f32_vs_f64_max_dF_over_max_F"] = float(np.abs(f_32.cpu().numpy()[:, :3] - forces["general"][:, :3]).max() / np.abs(forces["general"][:, :3]).max())
for run in range(3):
    r = {"f64_general_ms": timed(lambda: cl64.transverse_lj(pot64.device_table(), 1, box64, f_64, None, None, None, 1)),
         "f64_scan32_ms": timed(lambda: cl64.transverse_lj(pot64.device_table(), 1, box64, f_64, None, None, None, 11)),
         "f32_general_ms": timed(lambda: cl32.transverse_lj(pot.device_table(), 1, box, f_32, None, None, None, 1))}
    out["runs"].append(r)
    print(f"run {run}: " + ", ".join(f"{k} {v:.4f}" for k, v in r.items()), flush=True)
print(json.dumps(out), flush=True)
if os.environ.get("OUT"):
    with open(os.environ["OUT"], "w") as fh:
        json.dump(out, fh, indent=1)
