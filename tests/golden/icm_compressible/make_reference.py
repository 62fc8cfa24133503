"""Regenerates equilibrium_reference.json: the equilibrium fluctuations of the float64 restatement (tests/icm_compressible_ref.py) of
Hydro::ICM_Compressible in the configuration tests/test_gpu_icm_compressible.py runs on the GPU.

    python tests/golden/icm_compressible/make_reference.py [seeds]

Per seed: 12^3 cells of h = 1, eta = xi = 1, c = 4, dt = 0.05, T = 0.01, rho0 = 1, 1500 steps, a sample every 5 steps after step 300 of
var(rho) / (rho0 T / (c^2 dV)) and of <v_a^2> / (T / (rho0 dV)) (staggered velocities, mean over the three components).  The file keeps the
mean and the standard deviation ACROSS seeds of both ratios.  Neither ratio is 1: the scheme has a time-step bias (0.93 and 1.02 here), so
this file is the yardstick, not the continuum theory."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import icm_compressible_ref as ref  # noqa: E402

CONFIG = dict(cells=[12, 12, 12], L=12.0, shearViscosity=1.0, bulkViscosity=1.0, speedOfSound=4.0, dt=0.05, temperature=0.01, rho0=1.0,
              steps=1500, first=300, every=5)


def ratios(rho, v, c=CONFIG):
    """the two ratios of one state (arrays of any float type)"""
    dV = (c["L"] / c["cells"][0]) ** 3
    rho = np.asarray(rho, np.float64)
    vr = rho.var() / (c["rho0"] * c["temperature"] / (c["speedOfSound"] ** 2 * dV))
    vv = np.mean([np.mean(np.asarray(a, np.float64) ** 2) for a in v]) / (c["temperature"] / (c["rho0"] * dV))
    return vr, vv


def run(seed, c=CONFIG):
    f = ref.Fluid(c["cells"], c["L"], c["shearViscosity"], c["bulkViscosity"], c["speedOfSound"], c["dt"], c["temperature"], np.float64)
    f.set(rho=np.full(f.rho.shape, c["rho0"]))
    rng = np.random.default_rng(seed)
    acc = []
    for step in range(1, c["steps"] + 1):
        f.step_fluid(f.draw(rng))
        if step > c["first"] and step % c["every"] == 0:
            acc.append(ratios(f.rho, f.v, c))
    return np.mean(acc, axis=0)


if __name__ == "__main__":
    seeds = list(range(1, 1 + (int(sys.argv[1]) if len(sys.argv) > 1 else 8)))
    r = np.array([run(s) for s in seeds])
    out = dict(config=CONFIG, seeds=seeds, density_variance_ratio=dict(mean=float(r[:, 0].mean()), std=float(r[:, 0].std(ddof=1))),
               velocity_square_ratio=dict(mean=float(r[:, 1].mean()), std=float(r[:, 1].std(ddof=1))), per_seed=r.tolist())
    with open(os.path.join(HERE, "equilibrium_reference.json"), "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out, indent=1))
