#!/usr/bin/env python
"""Timing of the DPD pair force and of VerletNVE (tools, not part of bench.py's contract).

  W1  N = 1 000 000, rho = 3, rc = 1 (L = 69.336), A = 25, gamma = 4.5, kT = 1, dt = 0.01
  W2  N =   100 000, same state
  positions and velocities from an equilibrated run (uniform random start at rest, EQUIL steps of VerletNVE + DPD), particles sorted as
  a simulation keeps them.

What is timed (device events around >= 1 s of work after warm-up, ROUNDS rounds alternating between the paths):
  library   PairForces<Potential::DPD>::sum through the C ABI (uammd_dpd_transverse_celllist): list rebuilt every sum / list kept;
            VerletNVE::forwardTime
  baseline  the same formula as a user potential through device/PairForces.hip.hpp on the CellList (tools/dpd_generic_baseline.hip),
            built against this tree's headers and, where given, against another tree's (--baseline NAME=BINARY, e.g. the parent commit's)
  nodraw    the library with the draw replaced by a constant (a diagnostic BUILD, -DUAMMD_DPD_NO_DRAW: --nodraw-lib FILE), which gives
            the fraction of the kernel's time the generator accounts for
and, computed from the state: accepted pairs per sum and per second.

build (on a machine with hipcc; the binaries travel):
  mkdir -p tools/_build
  hipcc --offload-arch=gfx950 -O2 -std=c++17 -ffp-contract=off -w -Iinclude/uammd -Iinclude tools/dpd_generic_baseline.hip \
        -o tools/_build/dpd_baseline_this -Luammd_amd/lib -luammd_hip -Wl,-rpath,$PWD/uammd_amd/lib
  (against another checkout's include/: the same line with its -I, output tools/_build/dpd_baseline_parent)
  make -C uammd_amd/csrc FLAGS+=-DUAMMD_DPD_NO_DRAW ... or compile dpd.hip alone with that flag and link it with the other objects into
  tools/_build/libuammd_hip_nodraw.so

usage: python tools/time_dpd.py [--quick] [--json FILE] [--baseline NAME=BINARY ...] [--nodraw-lib FILE]
       python tools/time_dpd.py --make-state N ; rocprofv3 --kernel-trace --stats -- python tools/time_dpd.py --library-times tools/_build/dpd_state_N.bin
"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

EQUIL, ROUNDS = 300, 3
PAR = dict(cutOff=1.0, dt=0.01, gamma=4.5, temperature=1.0, A=25.0)


def _opt(name):
    return [sys.argv[i + 1] for i, a in enumerate(sys.argv[:-1]) if a == name]


def timed(fn, min_ms=1000.0):
    """ms per call: warm-up, then device events around enough repetitions for >= min_ms of work."""
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


def make_state(n, path):
    import torch
    import uammd_amd as hip
    L = (n / 3.0) ** (1.0 / 3.0)
    rng = np.random.default_rng(n)
    pos = np.zeros((n, 4), np.float32)
    pos[:, :3] = rng.uniform(-L / 2, L / 2, (n, 3)) * 0.999
    pd = hip.ParticleData(n)
    pd.setPos(pos)
    pd.getVel("write").zero_()
    box = hip.Box(L)
    verlet = hip.VerletNVE(pd, dt=PAR["dt"], initVelocities=False)
    verlet.addInteractor(hip.PairForces(pd, box, hip.Potential.DPD(**PAR)))
    for s in range(EQUIL):
        verlet.forwardTime()
        if s % 100 == 99:
            pd.hintSortByHash(box, [1.0] * 3)
            pd.sortParticles()
    pd.hintSortByHash(box, [1.0] * 3)
    pd.sortParticles()
    torch.cuda.synchronize()
    p, v = pd.getPos().cpu().numpy(), pd.getVel().cpu().numpy()
    p[:, :3] -= np.floor(p[:, :3] / np.float32(L) + 0.5) * np.float32(L)
    with open(path, "wb") as f:
        f.write(np.int32(n).tobytes() + np.float32(L).tobytes() + p.astype(np.float32).tobytes() + v.astype(np.float32).tobytes())
    T = float((v.astype(np.float64) ** 2).sum() / (3 * n))
    return L, T


def load_state(path):
    raw = open(path, "rb").read()
    n, L = int(np.frombuffer(raw, np.int32, 1)[0]), float(np.frombuffer(raw, np.float32, 1, 4)[0])
    p = np.frombuffer(raw, np.float32, 4 * n, 8).reshape(n, 4).copy()
    v = np.frombuffer(raw, np.float32, 3 * n, 8 + 16 * n).reshape(n, 3).copy()
    return n, L, p, v


def accepted_pairs(p, L):
    """ordered pairs (i, j), i != j, within the cut-off: what one sum evaluates (each pair twice, once per member)"""
    from scipy.spatial import cKDTree
    w = p[:, :3].astype(np.float64)
    w -= np.floor(w / L) * L
    w = np.where(w >= L, 0.0, w)
    t = cKDTree(w, boxsize=L)
    return t.count_neighbors(t, PAR["cutOff"]) - len(w)


def library_times(path):
    """run in a process of its own (the library variant is chosen before it is loaded); prints one JSON line"""
    import torch
    import uammd_amd as hip
    n, L, p, v = load_state(path)
    pd = hip.ParticleData(n)
    pd.setPos(p)
    pd.getVel("write").copy_(torch.from_numpy(v).cuda())
    box = hip.Box(L)
    pf = hip.PairForces(pd, box, hip.Potential.DPD(**PAR))

    def rebuilt():
        pf.nl.force_next_update = True
        pf.sum(force=True)
    pf.sum(force=True)
    ms_build, reps = timed(rebuilt)
    ms_kept, _ = timed(lambda: pf.sum(force=True))
    verlet = hip.VerletNVE(pd, dt=PAR["dt"], initVelocities=False)
    verlet.addInteractor(pf)
    ms_step, _ = timed(verlet.forwardTime)
    print(json.dumps({"N": n, "reps": reps, "ms_sum_with_list_build": round(ms_build, 5), "ms_sum_list_kept": round(ms_kept, 5),
                      "ms_forwardTime": round(ms_step, 5)}))


def run_json(cmd, env=None):
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=900)
    if r.returncode != 0:
        raise RuntimeError(" ".join(cmd) + f" -> {r.returncode}\n" + r.stderr[-2000:])
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])


def main():
    if "--library-times" in sys.argv:
        lib = os.environ.get("UAMMD_TIME_DPD_LIB")
        if lib:
            from uammd_amd import _lib
            _lib.LIB_PATH = lib
        return library_times(_opt("--library-times")[0])
    if "--make-state" in sys.argv:   # the state file alone (for a profiler run of --library-times)
        n = int(_opt("--make-state")[0])
        os.makedirs(os.path.join(ROOT, "tools", "_build"), exist_ok=True)
        return print(make_state(n, os.path.join(ROOT, "tools", "_build", f"dpd_state_{n}.bin")))
    quick = "--quick" in sys.argv
    out = []
    bdir = os.path.join(ROOT, "tools", "_build")
    os.makedirs(bdir, exist_ok=True)
    baselines = dict(b.split("=", 1) for b in _opt("--baseline"))
    nodraw = (_opt("--nodraw-lib") or [None])[0]
    for name, n in (("W2", 100_000), ("W1", 1_000_000 if not quick else 200_000)):
        path = os.path.join(bdir, f"dpd_state_{n}.bin")
        L, T = make_state(n, path)
        _, _, p, _ = load_state(path)
        pairs = int(accepted_pairs(p, L))
        rec = {"workload": name, "N": n, "L": round(L, 4), "equilibration_steps": EQUIL, "kinetic_temperature": round(T, 4),
               "accepted_ordered_pairs": pairs, "per_particle": round(pairs / n, 2)}
        print(json.dumps(rec), flush=True)
        out.append(rec)
        paths = {"library": [sys.executable, os.path.abspath(__file__), "--library-times", path]}
        for b, exe in baselines.items():
            paths["baseline_" + b] = [exe, path, "200" if n <= 100_000 else "40"]
        rows = {k: [] for k in paths}
        for _ in range(ROUNDS):
            for k, cmd in paths.items():
                rows[k].append(run_json(cmd))
        if nodraw:
            env = dict(os.environ, UAMMD_TIME_DPD_LIB=nodraw)
            rows["library_nodraw"] = [run_json(paths["library"], env) for _ in range(ROUNDS)]
        for k, rs in rows.items():
            rec = {"workload": name, "path": k}
            for key in ("ms_sum_with_list_build", "ms_sum_list_kept", "ms_forwardTime"):
                vals = [r[key] for r in rs if key in r]
                if vals:
                    rec[key] = round(float(np.median(vals)), 5)
                    rec[key + "_spread"] = round(float(max(vals) - min(vals)), 5)
            if "ms_sum_list_kept" in rec:
                rec["accepted_pairs_per_second"] = round(pairs / (rec["ms_sum_list_kept"] * 1e-3), 0)
            print(json.dumps(rec), flush=True)
            out.append(rec)
        if nodraw:
            full = next(r for r in out if r["workload"] == name and r.get("path") == "library")["ms_sum_list_kept"]
            nd = next(r for r in out if r["workload"] == name and r.get("path") == "library_nodraw")["ms_sum_list_kept"]
            rec = {"workload": name, "generator_fraction_of_sum": round(1.0 - nd / full, 3)}
            print(json.dumps(rec), flush=True)
            out.append(rec)
    for j in _opt("--json"):
        with open(j, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
