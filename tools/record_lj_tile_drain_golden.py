#!/usr/bin/env python
"""Records tests/golden/lj_tile_drain_parent.npz: the tile kernels' forces (and, for one case, energies and virials) on the
configurations of tests/lj_tile_drain_cases.py, computed by the library of ONE commit — the parent of a change that must not move a
bit (tests/test_gpu_lj_tile_drain.py compares against them word for word).  Run it on the GPU with that commit's library:
  UAMMD_HIP_LIB=<libuammd_hip.so built from COMMIT> python tools/record_lj_tile_drain_golden.py COMMIT [output.npz]
The file names the commit and, per case, a digest of the positions the forces belong to."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
import uammd_amd as hip
import lj_tile_drain_cases as dc

commit = sys.argv[1]
out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "tests", "golden", "lj_tile_drain_parent.npz")
data = {"parent_commit": np.array(commit), "library": np.array(os.path.basename(os.environ.get("UAMMD_HIP_LIB", "libuammd_hip.so")))}
for name, algo in dc.RUNS:
    c = dc.case(name)
    f, e, v, _, cd = dc.run(hip, torch, c, algo)
    k = dc.key(name, algo)
    data[k + "/pos_sha1"] = np.array(dc.digest(c["pos"]))
    data[k + "/f"] = f[:, :3].copy()
    if e is not None:
        data[k + "/e"], data[k + "/v"] = e, v
    print(f"{k}: N {len(f)}, cells {cd}, max|F| {np.abs(f).max():.4g}")
np.savez_compressed(out, **data)
print("wrote", out, os.path.getsize(out), "bytes; parent", commit)
