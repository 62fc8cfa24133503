#!/usr/bin/env python
"""Timing of the bonded kernels (tools, not part of bench.py's contract): ms per BondedForces sum for the four computable sets that the
reference's examples/interaction_modules/Bonds.cu prints (force, force+energy, force+virial, all three), the CSR shapes against the
reference-shaped baseline ("bonded_baseline" = 1), a sweep of "bonded_wave_threshold", and the compulsory-byte roofline fraction.

  W1  chain melt: 1e6 beads in chains of 100, FENE (k 30, R0 1.5) + Angular (k 5, ang0 0)
  W2  the shape Bonds.cu times: 5e4 particles with uniform(0, 1000) harmonic partners each (~2.5e7 bonds)

usage: python tools/time_bonded.py [--quick] [--json FILE]      (--quick: W1 1e5 beads, W2 5e3 particles; one line of JSON per measurement)
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import uammd_amd as hip  # noqa: E402
from uammd_amd import bonded  # noqa: E402

HBM = 6.3e12   # achievable HBM bandwidth, bytes/s (float4 copy)
COMBOS = [("force", (True, False, False)), ("force+energy", (True, True, False)), ("force+virial", (True, False, True)),
          ("all", (True, True, True))]


def chain_melt(n, length, L, rng):
    nchains = n // length
    steps = rng.normal(0, 1, (nchains, length, 3)).astype(np.float32)
    steps /= np.linalg.norm(steps, axis=2, keepdims=True)
    steps *= 0.97
    steps[:, 0] = rng.uniform(-L / 2, L / 2, (nchains, 3))
    P = np.cumsum(steps, axis=1).reshape(-1, 3)
    P -= np.floor(P / L + 0.5) * L
    b = np.arange(n, dtype=np.int32).reshape(nchains, length)
    pairs = np.stack([b[:, :-1].ravel(), b[:, 1:].ravel()], axis=1)
    triples = np.stack([b[:, :-2].ravel(), b[:, 1:-1].ravel(), b[:, 2:].ravel()], axis=1)
    return P, pairs, triples


def dense(n, maxPartners, L, rng):
    cnt = rng.integers(0, maxPartners + 1, n)
    first = np.repeat(np.arange(n, dtype=np.int32), cnt)
    second = rng.integers(0, n, first.size).astype(np.int32)
    second = np.where(second == first, (second + 1) % n, second).astype(np.int32)
    return rng.uniform(-L / 2, L / 2, (n, 3)).astype(np.float32), np.stack([first, second], axis=1)


def make_pd(P):
    pd = hip.ParticleData(len(P))
    p4 = np.zeros((len(P), 4), np.float32)
    p4[:, :3] = P
    pd.setPos(p4)
    return pd


def time_sum(its, pd, req, reps):
    f = pd.getForce("write")
    e = pd.getEnergy("write")
    v = pd.getVirial("write")
    for _ in range(3):
        for it in its:
            it.sum(*req)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        for it in its:
            it.sum(*req)
    b.record()
    torch.cuda.synchronize()
    del f, e, v
    return a.elapsed_time(b) / reps


def compulsory_bytes(N, its, req):
    """bytes every correct sum must move once: positions of the particles with bonds, read-modify-write of each requested output, and the
    bond entries (member indices + BondInfo) of the CSR; index lists of the rows (rowIndex, rowStart, row list) counted too."""
    total = 0
    for it in its:
        rows, entries, _, _ = it.shape()
        m = it.bondType.members
        total += 16 * rows + entries * (4 * m + 8) + rows * 12
        total += rows * ((32 if req[0] else 0) + (8 if req[1] else 0) + (8 if req[2] else 0))
    return total


def measure(name, pd, its, reps, out):
    for base in (0, 1):
        bonded.set_tunable("bonded_baseline", base)
        for label, req in COMBOS:
            ms = time_sum(its, pd, req, reps)
            byt = compulsory_bytes(pd.N, its, req)
            rec = {"workload": name, "variant": "baseline" if base else "csr", "computables": label, "ms": round(ms, 4),
                   "compulsory_MB": round(byt / 1e6, 2), "roofline_fraction": round(byt / HBM / (ms * 1e-3), 3)}
            print(json.dumps(rec), flush=True)
            out.append(rec)
    bonded.set_tunable("bonded_baseline", 0)


def sweep(name, pd, its, reps, out):
    for T in (2, 4, 8, 16, 32, 64, 128, 256, 1 << 30):
        bonded.set_tunable("bonded_wave_threshold", T)
        ms = time_sum(its, pd, (True, False, False), reps)
        shapes = [it.shape() for it in its]
        rec = {"workload": name, "sweep_threshold": T, "force_ms": round(ms, 4), "wave_rows": sum(s[3] for s in shapes),
               "lane_rows": sum(s[2] for s in shapes)}
        print(json.dumps(rec), flush=True)
        out.append(rec)
    bonded.set_tunable("bonded_wave_threshold", 32)


def main():
    quick = "--quick" in sys.argv
    out = []
    rng = np.random.default_rng(1)
    n1 = 100_000 if quick else 1_000_000
    L1 = (n1 / 0.85) ** (1 / 3)
    P, pairs, triples = chain_melt(n1, 100, L1, rng)
    pd = make_pd(P)
    box = hip.Box(L1)
    fene = bonded.BondedForces(pd, bondType=bonded.BondedType.FENE(box), ids=pairs, info=np.tile(np.float32([30, 1.5]), (len(pairs), 1)))
    ang = bonded.AngularBondedForces(pd, bondType=bonded.BondedType.Angular(box), ids=triples,
                                     info=np.tile(np.float32([5, 0]), (len(triples), 1)))
    pd.hintSortByHash(box, [1.5] * 3)
    pd.sortParticles()                 # spatially sorted as a simulation keeps it
    reps = 50
    measure("W1", pd, [fene, ang], reps, out)
    sweep("W1", pd, [fene, ang], reps, out)
    del fene, ang, pd
    torch.cuda.synchronize()
    n2 = 5_000 if quick else 50_000
    P, pairs = dense(n2, 1000, 50.0, rng)
    pd = make_pd(P)
    harm = bonded.BondedForces(pd, bondType=bonded.BondedType.Harmonic(hip.Box(50.0)), ids=pairs,
                               info=np.tile(np.float32([1, 1]), (len(pairs), 1)))
    print(json.dumps({"workload": "W2", "particles": n2, "bonds": int(len(pairs))}), flush=True)
    reps = 5 if not quick else 20
    measure("W2", pd, [harm], reps, out)
    sweep("W2", pd, [harm], reps, out)
    if "--json" in sys.argv:
        with open(sys.argv[sys.argv.index("--json") + 1], "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
