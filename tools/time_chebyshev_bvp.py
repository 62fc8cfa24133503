#!/usr/bin/env python
"""Timing of the Chebyshev z pass and of the batched boundary value problem solve (tools, not part of bench.py's contract).

Shapes: 128 x 128 x 65 and 256 x 256 x 33 (nx x ny x nz).  Device events around >= 0.5 s of work after warm-up, three rounds that
alternate between the paths compared; the median and the spread are printed, one JSON line per row.

  z pass    uammd_fct_chebyshev (float, forward and inverse): the cosine sums taken directly on the nz planes
  baseline  the reference's method with the same FFT library: write the even extension of length 2 nz - 2 (one kernel), a strided batched
            1-D complex FFT over it (torch.fft.fft along axis 0: hipFFT on rocFFT), scale planes 0 ... nz - 1 (one kernel)
  bound     the z pass must read and write nx ny nz complex values once: 2 nk nz sizeof(complex) bytes at the copy rate HBM sustains
  solve     uammd_bvp_solve{,_f64} on nk systems, nrhs = 1 and 3, in the solvers' interleaved layout, against the bytes it must move:
            fn read, an and cn written (3 nz complex per system and right-hand side) and the tables read once per right-hand side
            (5 nz + 5 reals per system)

usage: python tools/time_chebyshev_bvp.py [--json FILE]
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

SHAPES = [(128, 128, 65), (256, 256, 33)]
HBM_COPY_TBS = 6.29   # measured float4 copy rate of the MI355X (8.0 TB/s spec)
ROUNDS, MIN_MS = 3, 500.0


def timed(fn):
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
    reps = max(10, int(MIN_MS / max(a.elapsed_time(b) / 10, 1e-3)))
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def compare(paths):
    rows = {k: [] for k in paths}
    for _ in range(ROUNDS):
        for k, fn in paths.items():
            rows[k].append(timed(fn))
    return {k: (float(np.median(v)), float(max(v) - min(v))) for k, v in rows.items()}


def main():
    import torch
    from uammd_amd.bvp import BatchedBVP
    from uammd_amd.chebyshev import FastChebyshevTransform
    assert torch.cuda.is_available(), "this tool measures on the GPU"
    out = []
    for nx, ny, nz in SHAPES:
        nk, n = nx * ny, nz - 1
        g = torch.Generator(device="cuda").manual_seed(nz)
        f = torch.view_as_complex(torch.rand((nz, nk, 2), generator=g, device="cuda", dtype=torch.float32) * 2 - 1).contiguous()
        fct = FastChebyshevTransform(nx, ny, nz, torch.complex64)
        res = torch.empty_like(f)
        scale = torch.full((nz, 1), 2.0 / (2 * n), device="cuda")
        scale[0] = scale[n] = 1.0 / (2 * n)
        ext = torch.empty((2 * n, nk), dtype=torch.complex64, device="cuda")

        def reference_method():
            ext[:nz] = f
            ext[nz:] = f[1:n].flip(0)
            return torch.fft.fft(ext, dim=0)[:nz] * scale

        # the two paths compute the same thing
        a = fct.chebyshevTransform(f.reshape(-1), out=res.reshape(-1)).reshape(nz, nk)
        b = reference_method()
        agree = float((a - b).abs().max())
        t = compare({"z_pass_forward": lambda: fct.chebyshevTransform(f.reshape(-1), out=res.reshape(-1)),
                     "z_pass_inverse": lambda: fct.inverseChebyshevTransform(f.reshape(-1), out=res.reshape(-1)),
                     "even_extension_fft": reference_method})
        bound_ms = 2 * nk * nz * 8 / (HBM_COPY_TBS * 1e12) * 1e3
        rec = {"what": "z pass, float", "shape": [nx, ny, nz], "max_abs_difference_between_paths": agree, "traffic_bound_ms": round(bound_ms, 5)}
        for k, (ms, spread) in t.items():
            rec[k + "_ms"], rec[k + "_spread_ms"] = round(ms, 5), round(spread, 5)
        rec["baseline_over_z_pass"] = round(t["even_extension_fft"][0] / t["z_pass_forward"][0], 3)
        print(json.dumps(rec), flush=True)
        out.append(rec)
        # the batched solve
        H = 1.0
        k = np.sqrt(np.add.outer(np.fft.fftfreq(ny, 1.0 / ny) ** 2, np.fft.fftfreq(nx, 1.0 / nx) ** 2)).reshape(-1) * 2 * np.pi / 32.0
        nonzero = k != 0
        top = (np.where(nonzero, H, 0.0), np.where(nonzero, k * H * H, 1.0))
        bottom = (np.where(nonzero, H, 0.0), np.where(nonzero, -k * H * H, 1.0))
        for dtype, size in ((torch.complex64, 4), (torch.complex128, 8)):
            bvp = BatchedBVP(k, H, nz, top, bottom, dtype)
            for nrhs in (1, 3):
                fn = torch.view_as_complex(torch.rand((nrhs, nz, nk, 2), generator=g, device="cuda", dtype=torch.float32) * 2 - 1).to(dtype).contiguous()
                ab = torch.ones((nrhs, nk), dtype=dtype, device="cuda")
                ms, spread = compare({"solve": lambda: bvp.solve(fn, ab, ab)})["solve"]
                nbytes = nrhs * nk * (3 * nz * 2 * size + (5 * nz + 5) * size + 4 * size)
                rec = {"what": "bvp solve (with the allocation of an and cn)", "precision": "double" if size == 8 else "float", "nsys": nk, "nz": nz,
                       "nrhs": nrhs, "ms": round(ms, 5), "spread_ms": round(spread, 5), "compulsory_bytes": nbytes,
                       "traffic_bound_ms": round(nbytes / (HBM_COPY_TBS * 1e12) * 1e3, 5), "achieved_TBs": round(nbytes / (ms * 1e-3) / 1e12, 3)}
                print(json.dumps(rec), flush=True)
                out.append(rec)
    for j in [sys.argv[i + 1] for i, a in enumerate(sys.argv[:-1]) if a == "--json"]:
        with open(j, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
