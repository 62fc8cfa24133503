#!/usr/bin/env python
"""Timing of MC_NVT.Anderson (tools, not part of bench.py's contract).

  W1  N = 1 000 000, rho = 0.8, T = 1.5, rc = 2.5, shifted LJ, 10 tries per cell, jump 0.1   (the benchmark liquid)
  W2  N =    10 000, rho = 0.6, T = 2,   rc = 2.5,             40 tries per cell, jump 0.1   (the size of the reference's test)
  start: jittered lattice, RELAX steps of the integrator itself; no tuning while timing (tuneSteps beyond the run).

What is timed (device events around >= 1 s of steps after warm-up, ROUNDS rounds, the two paths alternating, each in a process of its own):
  wave      the wave-per-cell kernel with the neighbourhood staged in LDS (the default)
  baseline  "mc_baseline" = 1: the reference-shaped kernel, one thread per cell, global memory
per path: ms per forwardTime, tries per second (from the integrator's own counters), and the share of the step outside the subgrid
launches (the same step with triesPerCell = 0: shift, list build, unshift, scatter and the host draws).

usage: python tools/time_mc.py [--quick] [--json FILE]
       rocprofv3 --kernel-trace --stats -- python tools/time_mc.py --one W1 0
"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

ROUNDS, RELAX = 3, 50
WORK = {"W1": dict(n=1_000_000, rho=0.8, T=1.5, tries=10), "W2": dict(n=10_000, rho=0.6, T=2.0, tries=40),
        "Wq": dict(n=100_000, rho=0.8, T=1.5, tries=10)}


def _opt(name, k=1):
    return [sys.argv[i + 1:i + 1 + k] for i, a in enumerate(sys.argv) if a == name]


def timed(fn, min_ms=1000.0):
    import torch
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(10):
        fn()
    b.record()
    torch.cuda.synchronize()
    reps = max(10, int(min_ms / max(a.elapsed_time(b) / 10, 1e-3)))
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps, reps


def one(name, baseline):
    import uammd_amd as hip
    from util import lattice_positions
    w = WORK[name]
    n = w["n"]
    L = (n / w["rho"]) ** (1.0 / 3.0)
    assert hip.load().uammd_hip_set_tunable(b"mc_baseline", int(baseline)) == 0
    pot = hip.Potential.LJ()
    pot.setPotParameters(0, 0, pot.InputPairParameters(2.5, 1.0, 1.0, True))

    def make(tries):
        pd = hip.ParticleData(n, seed=1)
        pd.setPos(lattice_positions(n, L, seed=3, jitter=0.1))
        par = hip.MC_NVT.Anderson.Parameters(box=hip.Box(L), temperature=w["T"], triesPerCell=tries, initialJumpSize=0.1,
                                             tuneSteps=10 ** 9, seed=7)
        return hip.MC_NVT.Anderson(pd, pot, par)
    mc = make(w["tries"])
    for _ in range(RELAX):
        mc.forwardTime()
    mc.resetAcceptanceCounters()
    ms, reps = timed(mc.forwardTime)
    tried, accepted = mc._counters(reset=False)
    steps = reps + 15
    rest = make(0)
    rest.pd.setPos(mc.pd.getPos().cpu().numpy())
    ms_rest, _ = timed(rest.forwardTime, 300.0)
    print(json.dumps({"workload": name, "path": "baseline" if baseline else "wave", "N": n, "cellDim": mc.cellDim, "reps": reps,
                      "ms_forwardTime": round(ms, 5), "tries_per_step": tried // steps, "tries_per_second": round(tried / steps / (ms * 1e-3)),
                      "acceptance": round(accepted / max(tried, 1), 4), "ms_outside_subgrid_launches": round(ms_rest, 5),
                      "share_outside_subgrid_launches": round(ms_rest / ms, 4)}))


def main():
    if "--one" in sys.argv:
        name, baseline = _opt("--one", 2)[0]
        return one(name, int(baseline))
    out = []
    for name in (("W2", "Wq") if "--quick" in sys.argv else ("W2", "W1")):
        rows = {0: [], 1: []}
        for _ in range(ROUNDS):
            for b in (0, 1):
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", name, str(b)], capture_output=True, text=True, timeout=900)
                if r.returncode != 0:
                    raise RuntimeError(r.stderr[-2000:])
                rows[b].append(json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1]))
        for b, rs in rows.items():
            rec = dict(rs[0])
            for key in ("ms_forwardTime", "tries_per_second", "ms_outside_subgrid_launches", "share_outside_subgrid_launches"):
                vals = [r[key] for r in rs]
                rec[key] = round(float(np.median(vals)), 5)
                rec[key + "_spread"] = round(float(max(vals) - min(vals)), 5)
            rec["rounds"] = ROUNDS
            print(json.dumps(rec), flush=True)
            out.append(rec)
    for j in _opt("--json"):
        with open(j[0], "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
