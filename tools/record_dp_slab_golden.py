#!/usr/bin/env python
"""Records tests/golden/dp_slab_parent.npz: what the doubly periodic solvers give on the default (bit-reproducible) path for the cases of
tests/test_gpu_dp_slab_parent.py, which then holds every later build to these bits.  Run it on the GPU from the commit whose results
are to be kept (UAMMD_HIP_LIB selects another build of the library).

usage: python tools/record_dp_slab_golden.py [FILE]
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import test_gpu_dp_slab_parent as cases
    path = sys.argv[1] if len(sys.argv) > 1 else cases.GOLDEN
    out = cases.record(path)
    print(f"{len(out)} entries, {os.path.getsize(path)} bytes -> {path}")


if __name__ == "__main__":
    main()
