#!/usr/bin/env python
"""Timing of Hydro.ICM_Compressible (tools, not part of bench.py's contract).

  grids 32^3, 64^3, 128^3 of unit cells, eta = xi = 1, c = 4, dt = 0.05, rho = 1 + a smooth 5 % wave;
  T = 0 and T = 0.01 (the integrator's own draws);  0 and 16384 particles (uniform in the box, a constant random force each).

What is timed: ms per forwardTime through the Python layer (device events around >= 0.3 s of steps after warm-up), the median of ROUNDS
rounds that alternate over the four (T, particles) cases of a grid;
per row also the share of a byte model of the three sub-stages at the copy rate of SURVEY 8d (6.29 TB/s): per cell and sub-stage 7 fields
of time b, rho and g of time a, 3 forcing and 7 written (21 floats; 18 without particles) plus 12 noise floats when T > 0.

--walls adds, for every grid, the T = 0 cases between two moving walls (the built-in rule, steady wall velocities), alternating with the
periodic ones in the same rounds: rows with "walls": true.  Noise with walls is refused, so T > 0 has no such row.

usage: python tools/time_icm_compressible.py [--quick] [--walls] [--json FILE]
       rocprofv3 --kernel-trace --stats -- python tools/time_icm_compressible.py --one 64 0.01 16384 50
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

ROUNDS = 3
COPY_RATE = 6.29e12


def _opt(name, k=1):
    return [sys.argv[i + 1:i + 1 + k] for i, a in enumerate(sys.argv) if a == name]


class Fixed:
    def __init__(self, pd, F):
        import torch
        self.pd, self.F = pd, torch.from_numpy(F).cuda()

    def sum(self, force=False, energy=False, virial=False):
        self.pd.getForce("readwrite")[:, :3] += self.F

    def updateSimulationTime(self, t):
        pass


class SteadyWalls:
    def velocities(self, t):
        return (0.04, -0.03), (-0.02, 0.05)


def make(n, T, N, walls=False):
    import torch
    import uammd_amd as hip
    rng = np.random.default_rng(1)
    pd = hip.ParticleData(N)
    if N:
        p = np.zeros((N, 4), np.float32)
        p[:, :3] = rng.uniform(-0.5, 0.5, (N, 3)) * n
        pd.setPos(p)
    par = hip.Hydro.ICM_Compressible.Parameters(shearViscosity=1.0, bulkViscosity=1.0, speedOfSound=4.0, temperature=T, dt=0.05,
                                                boxSize=[float(n)] * 3, cellDim=[n] * 3, seed=5,
                                                walls=SteadyWalls() if walls else None)
    icm = hip.Hydro.ICM_Compressible(pd, par)
    x = (np.arange(n) + 0.5) * 2 * np.pi / n
    rho = (1 + 0.05 * np.sin(x)[None, None, :] * np.cos(x)[None, :, None] * np.cos(x)[:, None, None]).astype(np.float32)
    icm.setFluid(density=torch.from_numpy(rho))
    if N:
        icm.addInteractor(Fixed(pd, rng.normal(0, 0.1, (N, 3)).astype(np.float32)))
    return icm


def timed(fn, min_ms=300.0):
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
    return a.elapsed_time(b) / reps


def model_ms(n, T, N):
    floats = 7 + 4 + 7 + (3 if N else 0) + (12 if T > 0 else 0)
    return 3 * floats * 4 * n ** 3 / COPY_RATE * 1e3


def main():
    if "--one" in sys.argv:
        import torch
        n, T, N, steps = _opt("--one", 4)[0]
        icm = make(int(n), float(T), int(N))
        for _ in range(int(steps)):
            icm.forwardTime()
        torch.cuda.synchronize()
        return
    quick = "--quick" in sys.argv
    out = []
    for n in ((32, 64) if quick else (32, 64, 128)):
        cases = [(T, N, False) for T in (0.0, 0.01) for N in (0, 16384)]
        if "--walls" in sys.argv:
            cases += [(0.0, N, True) for N in (0, 16384)]
        icms = {c: make(n, *c) for c in cases}
        ms = {c: [] for c in cases}
        for _ in range(ROUNDS):
            for c in cases:
                ms[c].append(timed(icms[c].forwardTime, 100.0 if quick else 300.0))
        for (T, N, w) in cases:
            med = float(np.median(ms[T, N, w]))
            rec = {"grid": n, "T": T, "particles": N, "walls": w, "ms_forwardTime": round(med, 5),
                   "ms_spread": round(max(ms[T, N, w]) - min(ms[T, N, w]), 5), "ms_runs": [round(x, 5) for x in ms[T, N, w]],
                   "rounds": ROUNDS, "byte_model_ms": round(model_ms(n, T, N), 5), "byte_model_share": round(model_ms(n, T, N) / med, 4)}
            print(json.dumps(rec), flush=True)
            out.append(rec)
        del icms
    for j in _opt("--json"):
        with open(j[0], "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
