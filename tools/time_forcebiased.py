#!/usr/bin/env python
"""Timing of MC.ForceBiased (tools, not part of bench.py's contract).

  N = 16 384 Lennard-Jones particles (rc = 2.5, shifted), rho = 0.6, T = 3, h0 = 2e-4, target 0.5; start: jittered lattice, RELAX calls.

Per trial, medians over ROUNDS rounds of TRIALS trials each:
  own_ms         the integrator's own kernels: device events around propose + the two fills, and around reduce + commit
  interactor_ms  device events around the interactors (cell list and LJ traversal with force and energy)
  trial_ms       the whole trial on the host clock, the one synchronisation included (no events inside)
  plain_trial_ms the same trial with the sums read back one by one: the library's proposal, the same fills and interactor, then three
                 reductions with a host read each (sum e, sum |Y - X - h F(X)|^2, sum |X - Y - h F(Y)|^2 as torch expressions in double),
                 the decision on the host and two full-array copies to store or restore (the shape of the reference's integrator).
                 An accepted plain trial also re-adopts the state in the library (uammd_mc_forcebiased_begin: two more copies and two
                 small kernels, no synchronisation) so that the next proposal starts from it; that is counted against the plain variant.

usage: python tools/time_forcebiased.py [--n N] [--json FILE]
"""
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

ROUNDS, TRIALS, RELAX = 5, 400, 300


def _opt(name, default):
    return [sys.argv[i + 1] for i, a in enumerate(sys.argv) if a == name][-1:] or [default]


def main():
    import torch
    import uammd_amd as hip
    from util import lattice_positions
    n, rho, T = int(_opt("--n", 16384)[0]), 0.6, 3.0
    L = (n / rho) ** (1.0 / 3.0)
    pd = hip.ParticleData(n, seed=1)
    pd.setPos(lattice_positions(n, L, seed=3, jitter=0.05))
    pot = hip.Potential.LJ()
    pot.setPotParameters(0, 0, pot.InputPairParameters(2.5, 1.0, 1.0, True))
    mala = hip.MC.ForceBiased(pd, hip.MC.ForceBiased.Parameters(beta=1.0 / T, stepSize=2e-4, acceptanceRatio=0.5))
    mala.addInteractor(hip.PairForces(pd, hip.Box(L), pot))
    for _ in range(RELAX):
        mala.forwardTime()
    lib, ptr, st = mala.lib, hip.md._ptr, hip.current_stream
    beta = float(mala.beta)

    def events(k):
        return [torch.cuda.Event(enable_timing=True) for _ in range(k)]

    def trial_with_events():
        e = events(4)
        pos = pd.getPos("readwrite")
        mala.step += 1
        h = mala.trialStepSize = float(mala.optimizeStepSize.getStepSize())
        e[0].record()
        hip._lib.check(lib.uammd_mc_forcebiased_propose(mala.h, ptr(pos), n, h, beta, mala.step, mala.seed, None, st()))
        f, en = pd.getForce("write"), pd.getEnergy("write")
        hip._lib.check(lib.uammd_fill_zero(ptr(f), f.numel() * 4, st()))
        hip._lib.check(lib.uammd_fill_zero(ptr(en), en.numel() * 4, st()))
        e[1].record()
        for it in mala.interactors:
            it.sum(force=True, energy=True, virial=False)
        e[2].record()
        mala.lastZ = float(np.float32(pd.rng.uniform(0.0, 1.0)))
        hip._lib.check(lib.uammd_mc_forcebiased_decide(mala.h, ptr(pd.getPos("readwrite")), ptr(f), ptr(en), n, h, beta, mala.lastZ, st()))
        e[3].record()
        acc = mala._result()
        (mala.optimizeStepSize.registerAccept if acc else mala.optimizeStepSize.registerReject)()
        return e[0].elapsed_time(e[1]) + e[2].elapsed_time(e[3]), e[1].elapsed_time(e[2])

    # the plain variant keeps a stored configuration of its own, in step with the library's
    sX, sF = pd.getPos().clone(), pd.getForce().clone()
    sE = [mala.getCurrentEnergy()]

    def plain_trial():
        pos = pd.getPos("readwrite")
        mala.step += 1
        h = float(mala.optimizeStepSize.getStepSize())
        hip._lib.check(lib.uammd_mc_forcebiased_propose(mala.h, ptr(pos), n, h, beta, mala.step, mala.seed, None, st()))
        f, en = pd.getForce("write"), pd.getEnergy("write")
        hip._lib.check(lib.uammd_fill_zero(ptr(f), f.numel() * 4, st()))
        hip._lib.check(lib.uammd_fill_zero(ptr(en), en.numel() * 4, st()))
        txy = (((pos[:, :3].double() - sX[:, :3].double()) - h * sF[:, :3].double()) ** 2).sum().item() / (4 * h)
        for it in mala.interactors:
            it.sum(force=True, energy=True, virial=False)
        ey = en.double().sum().item()
        tyx = (((sX[:, :3].double() - pos[:, :3].double()) - h * f[:, :3].double()) ** 2).sum().item() / (4 * h)
        x = -beta * ((ey - sE[0]) + (tyx - txy))
        Z = float(np.float32(pd.rng.uniform(0.0, 1.0)))
        if not math.isnan(x) and Z < (math.exp(x) if x < 700 else math.inf):
            sX.copy_(pos)
            sF.copy_(f)
            sE[0] = ey
            # the library's proposal reads the handle's stored arrays: they follow (see the docstring)
            hip._lib.check(lib.uammd_mc_forcebiased_begin(mala.h, ptr(pos), ptr(f), ptr(en), n, st()))
        else:
            pd.getPos("readwrite").copy_(sX)
            f.copy_(sF)

    def wall(fn, count):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(count):
            fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / count

    rows = {"own_ms": [], "interactor_ms": [], "trial_ms": [], "plain_trial_ms": []}
    for _ in range(ROUNDS):
        seg = [trial_with_events() for _ in range(TRIALS)]
        torch.cuda.synchronize()
        rows["own_ms"].append(float(np.median([s[0] for s in seg])))
        rows["interactor_ms"].append(float(np.median([s[1] for s in seg])))
        rows["trial_ms"].append(wall(mala.tryNewStep, TRIALS))
        # re-adopt the current state for both variants, then time the plain one
        sX.copy_(pd.getPos())
        sF.copy_(pd.getForce())
        sE[0] = mala.getCurrentEnergy()
        rows["plain_trial_ms"].append(wall(plain_trial, TRIALS))
        mala.firstStep()
        mala._result()
    out = {"N": n, "rho": rho, "T": T, "rounds": ROUNDS, "trials_per_round": TRIALS, "stepSize": mala.getCurrentStepSize(),
           "acceptance": mala.getCurrentAcceptanceRatio(),
           "launches_per_trial_own": 5, "synchronisations_per_trial": 1, "plain_host_reads_per_trial": 3}
    for k, v in rows.items():
        out[k] = round(float(np.median(v)), 5)
        out[k + "_spread"] = round(float(max(v) - min(v)), 5)
    print(json.dumps(out), flush=True)
    for j in _opt("--json", None):
        if j:
            with open(j, "w") as f:
                json.dump(out, f, indent=1)
                f.write("\n")


if __name__ == "__main__":
    main()
