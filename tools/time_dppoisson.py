#!/usr/bin/env python
"""Timing of the doubly periodic Poisson slab solver (tools, not part of bench.py's contract).

The quadrupole configuration's grid (Lxy 50, H 5, gw 0.2 sqrt(2/3), split 1.70103: 180 x 180 x 85) with 2e4 and 2e5 random charges, float
and double.  Device events around >= 0.3 s of work after warm-up, three rounds that alternate between the paths compared; the median and
the spread are printed, one JSON line per row.

  sum          the whole DPPoissonSlab::sum: far field, then near field
  far          the far field alone (option skip_near_field)
  far_simple   the far field with the plain spread (option simple_spread: a lane per particle, atomic adds) instead of the owner-computes one
  stages       the time of every stage of a sum, from device events the library records between its stage launches (option time_stages),
               the median of 30 calls after warm-up; for the default spread and, the spread stage only, for simple_spread
  bytes        what each stage must move at the least, G = nx ny nz complex values, R = one particle record (position and charge), and
               the fraction of the copy rate HBM sustains that the stage reaches:
                 classify 2 R N (+ the float copy and the window cells) | spread: G written, R N read | a Fourier-Chebyshev transform: 4 G
                 (z pass in and out, plane transform in place) | solve: G read, 4 G written (y'' twice, both solutions), the tables
                 twice | correction: 2 G written | a z pass: 2 G | assemble: 3 G read, 2 G written | gather: 2 G read, 3 R N | list and
                 pack: 3 R N | near field: R N read, 3 R N read and written

usage: python tools/time_dppoisson.py [--json FILE]
"""
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

HBM_COPY_TBS = 6.29   # measured float4 copy rate of the MI355X (8.0 TB/s spec)
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
    out = []
    P = hip.DPPoissonSlab
    L, H = 50.0, 5.0
    for real in (torch.float32, torch.float64):
        for n in (20000, 200000):
            rng = np.random.default_rng(1)
            pos = np.zeros((n, 4))
            pos[:, :2] = rng.uniform(-0.5 * L, 0.5 * L, (n, 2))
            pos[:, 2] = rng.uniform(-0.5 * H, 0.5 * H, n)
            q = rng.normal(0, 1, n)
            q -= q.mean()
            p, c = torch.as_tensor(pos, dtype=real, device="cuda"), torch.as_tensor(q, dtype=real, device="cuda")
            f, e = torch.zeros((n, 4), dtype=real, device="cuda"), torch.zeros((n,), dtype=real, device="cuda")
            par = lambda: P.Parameters(Lxy=(L, L), H=H, gw=0.2 * math.sqrt(2.0 / 3.0), split=1.70103)  # noqa: E731
            whole, far, simple = P(None, par(), real=real), P(None, par(), real=real), P(None, par(), real=real)
            far.set_option("skip_near_field", 1)
            simple.set_option("skip_near_field", 1)
            simple.set_option("simple_spread", 1)
            res = compare({"sum": lambda: whole.sum_arrays(p, c, f, e), "far": lambda: far.sum_arrays(p, c, f, e),
                           "far_simple": lambda: simple.sum_arrays(p, c, f, e)})
            nx, ny, nz = whole.cells
            w = 8 if real == torch.float64 else 4
            G, R = nx * ny * nz * 2 * w, 5 * w
            tables = 2 * nx * ny * (5 * nz + 5) * w
            must = {"classify": 2 * R * n + 32 * n, "spread": G + R * n, "forward transform": 4 * G, "solve + mismatch": 5 * G + tables,
                    "correction": 2 * G, "z pass dphi": 2 * G, "z pass phi": 2 * G, "assemble": 5 * G, "inverse (Ex, Ey)": 4 * G,
                    "inverse (Ez, phi)": 4 * G, "gather": 2 * G + 3 * R * n, "cell list + pack": 3 * R * n, "near field": 7 * R * n}

            def stages(slab):
                slab.set_option("time_stages", 1)
                rows = []
                for it in range(35):
                    slab.sum_arrays(p, c, f, e)
                    if it >= 5:
                        rows.append(list(slab.stage_times().values()))
                slab.set_option("time_stages", 0)
                return dict(zip(P.STAGES, np.median(np.array(rows), axis=0).tolist()))
            st = stages(whole)
            simple_all = P(None, par(), real=real)
            simple_all.set_option("simple_spread", 1)
            st_simple = stages(simple_all)
            stage_rows = {k: dict(ms=v, bytes=must[k], bound_ms=must[k] / (HBM_COPY_TBS * 1e9), fraction_of_copy_rate=must[k] / (HBM_COPY_TBS * 1e9) / v)
                          for k, v in st.items()}
            furthest = min(stage_rows, key=lambda k: stage_rows[k]["fraction_of_copy_rate"])
            row = dict(cells=[nx, ny, nz], charges=n, precision="double" if real == torch.float64 else "float",
                       sum_ms=res["sum"][0], far_ms=res["far"][0], far_simple_spread_ms=res["far_simple"][0],
                       spread_of_rounds_ms={k: v[1] for k, v in res.items()}, stages=stage_rows, stages_total_ms=sum(st.values()),
                       spread_stage_ms={"owner": st["spread"], "simple": st_simple["spread"]}, furthest_from_its_bound=furthest)
            print(json.dumps(row), flush=True)
            out.append(row)
    if "--json" in sys.argv:
        with open(sys.argv[sys.argv.index("--json") + 1], "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
