#!/usr/bin/env python
"""Regenerates tests/golden/lj_melt_21952.npy: a Lennard-Jones liquid, 21 952 particles at rho* = 0.8 (12^3 cells of edge 2.513 at
rc = 2.5), melted from a jittered lattice by 1500 GronbechJensen steps at T = 1, dt = 0.005 — the configuration tools/drain_model.py
prices drain policies on.  Positions only (N x 3 float32, folded into the box).  Needs the GPU.
usage: python tests/golden/make_lj_melt_golden.py [output.npy]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import uammd_amd as hip
from util import lattice_positions

n = 21952
L = (n / 0.8) ** (1.0 / 3.0)
pd = hip.ParticleData(n, seed=1234)
pd.setPos(lattice_positions(n, L, seed=1234, jitter=0.1))
box = hip.Box(L)
pot = hip.Potential.LJ()
pot.setPotParameters(0, 0, pot.InputPairParameters(2.5, 1.0, 1.0, False))
integ = hip.VerletNVT.GronbechJensen(pd, hip.VerletNVT.GronbechJensen.Parameters(temperature=1.0, dt=0.005, friction=1.0))
integ.addInteractor(hip.PairForces(pd, box, pot))
for _ in range(1500):
    integ.forwardTime()
p = pd.getPos("read")[:, :3].cpu().numpy().astype(np.float64)
p -= np.floor(p / L + 0.5) * L
out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "lj_melt_21952.npy")
np.save(out, p.astype(np.float32))
print("wrote", out, p.shape)
