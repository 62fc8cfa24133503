#!/usr/bin/env python
"""Timing of the SPH interactor (tools, not part of bench.py's contract).

  W1  N = 1 000 000, W2  N = 100 000: the state of the reference's SPH example (fcc lattice at number density 0.247 in a periodic cube,
  support 2.4, rest density 0.3, gas stiffness 60, viscosity 10, dt 0.01), started with Gaussian velocities of 0.2 per component and taken
  after EQUIL steps of VerletNVE + SPH, particles sorted as a simulation keeps them.

What is timed (device events around >= 1 s of work after warm-up, ROUNDS rounds alternating between the two paths in the same call):
  library   SPH::sum through the C ABI (uammd_sph_sum_verletlist) with the list kept / rebuilt every sum; VerletNVE::forwardTime
            (the latter over at most 115 steps, so that the fluid stays in the state described)
  baseline  the same two sums as user Transversers through the generic device::transverseList on the same VerletList, with a transform
            for the pressure between them (tools/sph_generic_baseline.hip): what a user had to write before the library had the kernels
and, computed from the state: listed pairs per sum, pairs inside the support, and two lower bounds for the two traversals together,
  flop_bound_ms    listed pairs x the flops of a pair (counted from the formulas) at the fp32 vector peak
  cache_bound_ms   listed pairs x 32 B of cache-level reads (the two 16-byte rows pass 2 gathers per pair) at an aggregate L2 rate
neither of which is a memory-traffic model: they say how far from "free" a traversal is.

build (on a machine with hipcc; the binary travels):
  mkdir -p tools/_build
  hipcc --offload-arch=gfx950 -O2 -std=c++17 -ffp-contract=off -w -Iinclude/uammd -Iinclude tools/sph_generic_baseline.hip \
        -o tools/_build/sph_baseline -Luammd_amd/lib -luammd_hip -Wl,-rpath,$PWD/uammd_amd/lib

usage: python tools/time_sph.py [--quick] [--json FILE] [--baseline BINARY]
       python tools/time_sph.py --make-state N ; rocprofv3 --kernel-trace --stats -- python tools/time_sph.py --min-ms 200 --library-times tools/_build/sph_state_N.bin
"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

EQUIL, ROUNDS = 50, 3
PAR = dict(support=2.4, viscosity=10.0, gasStiffness=60.0, restDensity=0.3)
DT, DENSITY, AMPLITUDE = 0.01, 0.247, 0.2
# flops of one listed pair, counted from the formulas with sqrt and division as one each:
#   density  3 sub, 9 minimum image, 5 dot, sqrt, div, 2 sub, 4 + 5 mul/sub of the cubes, mul, add                         = 32
#   force    3 sub, 9 minimum image, 3 sub, 5 + 5 dots, sqrt, mul, 4 for the branch of G, add + div + mul, 2 add, mul, 6 fma  = 48
FLOP_PER_PAIR = {"density": 32, "force": 48}
ROW_BYTES = 32            # cache-level reads per listed pair: the position row and the info row of pass 2
PEAK_FP32_TFLOPS = 157.3  # MI355X vector fp32 peak (spec)
L2_TBS = 34.5             # aggregate L2 read rate assumed for the cache-level bound


def _opt(name):
    return [sys.argv[i + 1] for i, a in enumerate(sys.argv[:-1]) if a == name]


MIN_MS = 1000.0   # (--min-ms X: shorter, for a profiler run of --library-times)


def timed(fn, min_ms=None, max_reps=None):
    """ms per call: warm-up, then device events around enough repetitions for >= min_ms of work (at most max_reps of them)."""
    import torch
    min_ms = MIN_MS if min_ms is None else min_ms
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
    if max_reps:
        reps = min(reps, max_reps)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps, reps


def _system(n, L, p, v):
    import torch
    import uammd_amd as hip
    pd = hip.ParticleData(n)
    pd.setPos(p)
    pd.getVel("write").copy_(torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).cuda())
    box = hip.Box(L)
    return pd, box, hip.SPH(pd, box, **PAR)


def make_state(n, path):
    import torch
    import uammd_amd as hip
    from uammd_amd.initial_conditions import init_lattice
    L = float(np.float32((n / DENSITY) ** (1.0 / 3.0)))
    p = init_lattice(L, n, "fcc")
    p[:, 3] = 0
    rng = np.random.default_rng(n)
    v = AMPLITUDE * rng.normal(0.0, 1.0, (n, 3))
    v -= v.mean(0)
    pd, box, sph = _system(n, L, p, v)
    verlet = hip.VerletNVE(pd, dt=DT, initVelocities=False)
    verlet.addInteractor(sph)
    pd.hintSortByHash(box, [PAR["support"]] * 3)
    pd.sortParticles()
    for _ in range(EQUIL):
        verlet.forwardTime()
    pd.hintSortByHash(box, [PAR["support"]] * 3)
    pd.sortParticles()
    torch.cuda.synchronize()
    p, v = pd.getPos().cpu().numpy(), pd.getVel().cpu().numpy()
    assert np.isfinite(p).all() and np.isfinite(v).all()
    p[:, :3] -= np.floor(p[:, :3] / np.float32(L) + 0.5) * np.float32(L)
    with open(path, "wb") as f:
        f.write(np.int32(n).tobytes() + np.float32(L).tobytes() + p.astype(np.float32).tobytes() + v.astype(np.float32).tobytes())
    return L


def load_state(path):
    raw = open(path, "rb").read()
    n, L = int(np.frombuffer(raw, np.int32, 1)[0]), float(np.frombuffer(raw, np.float32, 1, 4)[0])
    p = np.frombuffer(raw, np.float32, 4 * n, 8).reshape(n, 4).copy()
    v = np.frombuffer(raw, np.float32, 3 * n, 8 + 16 * n).reshape(n, 3).copy()
    return n, L, p, v


def pairs_inside(p, L, rc):
    """ordered pairs (i, j) within rc, the self pairs included: what a sum over an exact list would evaluate"""
    from scipy.spatial import cKDTree
    w = p[:, :3].astype(np.float64)
    w -= np.floor(w / L) * L
    w = np.where(w >= L, 0.0, w)
    t = cKDTree(w, boxsize=L)
    return int(t.count_neighbors(t, rc))


def library_times(path):
    """run in a process of its own; prints one JSON line"""
    import torch
    import uammd_amd as hip
    from uammd_amd._lib import check
    n, L, p, v = load_state(path)
    pd, box, sph = _system(n, L, p, v)
    pd.getForce("write").zero_()
    sph.sum()
    torch.cuda.synchronize()
    sum_abs = float(np.abs(pd.getForce().cpu().numpy()[:, :3].astype(np.float64)).sum())
    listed = int(sph.nl.to_host()["numberNeighbours"].astype(np.int64).sum())

    def rebuilt():
        sph.nl.force_next_update = True
        check(sph.lib.uammd_verletlist_force_next_update(sph.nl.h))
        sph.sum()
    ms_build, reps = timed(rebuilt)
    ms_kept, _ = timed(sph.sum)
    verlet = hip.VerletNVE(pd, dt=DT, initVelocities=False)
    verlet.addInteractor(sph)
    # (at most 100 steps: this fluid is under tension, rho < rho0, and clumps as it runs on, which leaves the state the sums are timed in)
    ms_step, _ = timed(verlet.forwardTime, max_reps=100)
    print(json.dumps({"N": n, "reps": reps, "ms_sum_with_list_build": round(ms_build, 5), "ms_sum_list_kept": round(ms_kept, 5),
                      "ms_forwardTime": round(ms_step, 5), "sum_abs_force": sum_abs, "listed_pairs": listed}))


def run_json(cmd, env=None):
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=900)
    if r.returncode != 0:
        raise RuntimeError(" ".join(cmd) + f" -> {r.returncode}\n" + r.stderr[-2000:])
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])


def main():
    global MIN_MS
    if _opt("--min-ms"):
        MIN_MS = float(_opt("--min-ms")[0])
    if "--library-times" in sys.argv:
        return library_times(_opt("--library-times")[0])
    bdir = os.path.join(ROOT, "tools", "_build")
    os.makedirs(bdir, exist_ok=True)
    if "--make-state" in sys.argv:   # the state file alone (for a profiler run of --library-times)
        n = int(_opt("--make-state")[0])
        return print(make_state(n, os.path.join(bdir, f"sph_state_{n}.bin")))
    quick = "--quick" in sys.argv
    baseline = (_opt("--baseline") or [os.path.join(bdir, "sph_baseline")])[0]
    out = []
    for name, n in (("W2", 100_000), ("W1", 1_000_000 if not quick else 200_000)):
        path = os.path.join(bdir, f"sph_state_{n}.bin")
        L = make_state(n, path)
        _, _, p, _ = load_state(path)
        inside = pairs_inside(p, L, 2.0 * PAR["support"])
        paths = {"library": [sys.executable, os.path.abspath(__file__), "--library-times", path]}
        if os.path.exists(baseline):
            paths["baseline_generic"] = [baseline, path, "200" if n <= 100_000 else "30"]
        rows = {k: [] for k in paths}
        for _ in range(ROUNDS):
            for k, cmd in paths.items():
                rows[k].append(run_json(cmd))
        listed = rows["library"][0]["listed_pairs"]
        rec = {"workload": name, "N": n, "L": round(L, 4), "steps_before": EQUIL, "listed_ordered_pairs": listed,
               "listed_per_particle": round(listed / n, 2), "ordered_pairs_inside_2h": inside, "inside_fraction": round(inside / listed, 3),
               "flop_bound_ms": round(listed * sum(FLOP_PER_PAIR.values()) / (PEAK_FP32_TFLOPS * 1e12) * 1e3, 5),
               "cache_bound_ms": round(listed * ROW_BYTES / (L2_TBS * 1e12) * 1e3, 5)}
        print(json.dumps(rec), flush=True)
        out.append(rec)
        for k, rs in rows.items():
            rec = {"workload": name, "path": k}
            for key in ("ms_sum_with_list_build", "ms_sum_list_kept", "ms_forwardTime"):
                vals = [r[key] for r in rs if key in r]
                if vals:
                    rec[key] = round(float(np.median(vals)), 5)
                    rec[key + "_spread"] = round(float(max(vals) - min(vals)), 5)
            rec["sum_abs_force"] = rs[0]["sum_abs_force"]
            rec["listed_pairs_per_second"] = round(listed / (rec["ms_sum_list_kept"] * 1e-3), 0)
            print(json.dumps(rec), flush=True)
            out.append(rec)
        if "baseline_generic" in rows:
            lib = next(r for r in out if r["workload"] == name and r.get("path") == "library")
            base = next(r for r in out if r["workload"] == name and r.get("path") == "baseline_generic")
            for key in ("ms_sum_list_kept", "ms_sum_with_list_build"):
                spread = max(lib[key + "_spread"], base[key + "_spread"])
                diff = base[key] - lib[key]
                verdict = "tie" if abs(diff) <= spread else ("library faster" if diff > 0 else "library slower")
                rec = {"workload": name, "compared": key, "baseline_over_library": round(base[key] / lib[key], 3), "verdict": verdict}
                print(json.dumps(rec), flush=True)
                out.append(rec)
    for j in _opt("--json"):
        with open(j, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
