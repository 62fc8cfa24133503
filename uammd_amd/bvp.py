"""Batched boundary value problem solver in Chebyshev space.

Mirror of the reference's misc/BoundaryValueProblem/BVPSolver.cuh (BVP::BatchedBVPHandlerReal); the solve runs in libuammd_hip.so
(uammd_bvp_*, uammd_amd/csrc/bvp.hip, tables from csrc/bvp_host.hpp).  One system per wave number:

    y''(z) - k^2 y(z) = f(z) on [-H, H],  tfi y'(H) / H + tsi y(H) / H^2 = alpha,  bfi y'(-H) / H + bsi y(-H) / H^2 = beta

    bvp = BatchedBVP(k, H, nz, top=(tfi, tsi), bottom=(bfi, bsi), dtype=torch.complex128)   # k, tfi, ...: nsys host values each
    cn, an = bvp.solve(fn, alpha, beta)      # fn: (nrhs, nz, nsys) Chebyshev coefficients of f; alpha, beta: (nrhs, nsys)

cn holds the coefficients of y and an those of y''; fn is left as it was.
"""
import ctypes as C

import numpy as np
import torch

from ._lib import check, load
from .md import _ptr, current_stream


class BatchedBVP:
    def __init__(self, k, H, nz, top, bottom, dtype=torch.complex64):
        if dtype not in (torch.complex64, torch.complex128):
            raise ValueError("BatchedBVP: dtype must be torch.complex64 or torch.complex128")
        self.lib = load()
        k = np.atleast_1d(np.asarray(k, dtype=np.float64))
        self.nsys, self.nz, self.H, self.dtype = int(k.shape[0]), int(nz), float(H), dtype
        self.double = dtype == torch.complex128
        arrays = [np.ascontiguousarray(np.broadcast_to(np.asarray(a, dtype=np.float64), k.shape)) for a in (k, top[0], top[1], bottom[0], bottom[1])]
        dp = C.POINTER(C.c_double)
        self.h = C.c_void_p()
        check(self.lib.uammd_bvp_create(self.nsys, self.nz, self.H, *[a.ctypes.data_as(dp) for a in arrays], int(self.double),
                                        C.byref(self.h)))

    def __del__(self):
        if getattr(self, "h", None):
            self.lib.uammd_bvp_destroy(self.h)
            self.h = None

    def solve(self, fn, alpha, beta, layout="interleaved"):
        """fn: (nrhs, nz, nsys) with layout "interleaved" (the solvers' layout), (nrhs, nsys, nz) with "contiguous"; a leading axis of
        one may be left out.  alpha, beta: (nrhs, nsys).  Returns (cn, an) shaped like fn."""
        shape = {"interleaved": (self.nz, self.nsys), "contiguous": (self.nsys, self.nz)}[layout]
        strides = (1, self.nsys) if layout == "interleaved" else (self.nz, 1)
        if fn.dim() == 2:
            fn = fn.unsqueeze(0)
        nrhs = fn.shape[0]
        if tuple(fn.shape[1:]) != shape or fn.dtype != self.dtype or not fn.is_cuda or not fn.is_contiguous():
            raise ValueError(f"BatchedBVP.solve: fn must be a contiguous {self.dtype} device tensor of shape (nrhs, {shape[0]}, {shape[1]})")
        alpha, beta = alpha.reshape(-1), beta.reshape(-1)
        for t in (alpha, beta):
            if t.numel() != nrhs * self.nsys or t.dtype != self.dtype or not t.is_cuda or not t.is_contiguous():
                raise ValueError(f"BatchedBVP.solve: alpha and beta must hold nrhs * nsys = {nrhs * self.nsys} {self.dtype} device values")
        an, cn = torch.empty_like(fn), torch.empty_like(fn)
        name = "uammd_bvp_solve_f64" if self.double else "uammd_bvp_solve"
        check(getattr(self.lib, name)(self.h, _ptr(fn), _ptr(alpha), _ptr(beta), _ptr(an), _ptr(cn), nrhs, strides[0], strides[1],
                                      current_stream()))
        return cn, an
