"""Records the kinetic temperature of the DPD scheme in float64 (tests/dpd_ref.py: VerletNVE + the DPD pair force, NumPy's Gaussian
stream) for tests/test_gpu_dpd.py: rho = 3, rc = 1, A = 25, gamma = 4.5, kT = 1, dt = 0.01, uniform random start at rest, N = 8000,
3000 steps of which the last 2000 are block-averaged (20 blocks).  Writes temperature_reference.json beside itself.

    python tests/golden/dpd/make_reference.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
import dpd_ref  # noqa: E402

N, STEPS, MEASURED, BLOCKS = 8000, 3000, 2000, 20
T = dpd_ref.dpd_run(N, STEPS, seed=1)
mean, err = dpd_ref.block_average(T[-MEASURED:], BLOCKS)
out = dict(N=N, steps=STEPS, measured=MEASURED, blocks=BLOCKS, rho=3.0, cutOff=1.0, A=25.0, gamma=4.5, temperature=1.0, dt=0.01,
           mean=mean, stderr=err, T_step100=float(T[99]), T_step300=float(T[299]))
with open(os.path.join(HERE, "temperature_reference.json"), "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
print(out)
