#!/usr/bin/env python
"""Timing of the doubly periodic Stokes solver (tools, not part of bench.py's contract).

Mdot per wall mode at 128 x 128 x 65 (cells of a / 1.554 with a = 1, the rule of the reference's test; H = 2 h nz / pi) with 2e4 and 2e5
random particles, float and double.  Device events around >= 0.3 s of work after warm-up, three rounds that alternate between the paths
compared; the median and the spread are printed, one JSON line per row.

  mdot         the whole DPStokes::Mdot with the owner-computes spread
  mdot_simple  the same with the plain spread (option simple_spread: a lane per particle, atomic adds)
  stages       the time of every stage of a call, from device events the library records between its stage launches (option
               time_stages), the median of 30 calls after warm-up; for the default spread and, the spread stage only, for simple_spread

usage: python tools/time_dpstokes.py [--json FILE] [--quick]
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

ROUNDS, MIN_MS = 3, 300.0


def timed(fn):
    import torch
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(3):
        fn()
    b.record()
    torch.cuda.synchronize()
    reps = max(3, int(MIN_MS / max(a.elapsed_time(b) / 3, 1e-3)))
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def compare(paths):
    rows = {k: [] for k in paths}
    for _ in range(ROUNDS):
        for k, fn in paths.items():
            rows[k].append(timed(fn))
    return {k: (float(np.median(v)), float(max(v) - min(v))) for k, v in rows.items()}


def main():
    import torch
    import uammd_amd as hip
    global MIN_MS
    quick = "--quick" in sys.argv
    if quick:
        MIN_MS = 30.0
    out = []
    P = hip.DPStokes
    n_xy, nz, h = 128, 65, 1.0 / 1.554
    L = n_xy * h
    H = 2 * h * nz / np.pi
    w = 6.0
    for real in (torch.float32, torch.float64):
        for mode in ("none", "bottom", "slit"):
            for n in ((20000,) if quick else (20000, 200000)):
                rng = np.random.default_rng(1)
                pos = np.zeros((n, 4))
                pos[:, :2] = rng.uniform(-0.5 * L, 0.5 * L, (n, 2))
                pos[:, 2] = rng.uniform(-0.5 * H, 0.5 * H, n)
                p = torch.as_tensor(pos, dtype=real, device="cuda")
                f = torch.as_tensor(rng.normal(0, 1, (n, 4)), dtype=real, device="cuda")
                par = lambda: P.Parameters(nx=n_xy, ny=n_xy, nz=nz, viscosity=1.0, Lx=L, Ly=L, H=H, w=w, beta=(1.714 * w, -1.0, -1.0),  # noqa: E731
                                           alpha=0.5 * w, mode=mode)
                owner, simple = P(par(), real=real), P(par(), real=real)
                simple.set_option("simple_spread", 1)
                res = compare({"mdot": lambda: owner.Mdot(p, f), "mdot_simple": lambda: simple.Mdot(p, f)})

                def stages(solver):
                    solver.set_option("time_stages", 1)
                    rows = []
                    for it in range(35):
                        solver.Mdot(p, f)
                        if it >= 5:
                            rows.append(list(solver.stage_times().values()))
                    solver.set_option("time_stages", 0)
                    return dict(zip(P.STAGES, np.median(np.array(rows), axis=0).tolist()))
                st, st_simple = stages(owner), stages(simple)
                row = dict(cells=[n_xy, n_xy, nz], particles=n, mode=mode, precision="double" if real == torch.float64 else "float",
                           mdot_ms=res["mdot"][0], mdot_simple_spread_ms=res["mdot_simple"][0], spread_of_rounds_ms={k: v[1] for k, v in res.items()},
                           stages_ms=st, stages_total_ms=sum(st.values()), spread_stage_ms={"owner": st["spread"], "simple": st_simple["spread"]})
                print(json.dumps(row), flush=True)
                out.append(row)
    if "--json" in sys.argv:
        with open(sys.argv[sys.argv.index("--json") + 1], "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
