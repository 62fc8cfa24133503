"""Fast Chebyshev and Fourier-Chebyshev transforms.

Mirror of the reference's misc/Chebyshev/FastChebyshevTransform.cuh; the transforms run in libuammd_hip.so (uammd_fct_*,
uammd_amd/csrc/chebyshev.hip: the z pass is a HIP kernel of this project, the plane transform is rocFFT).

    fct = FastChebyshevTransform(nx, ny, nz, torch.complex128)
    cn = fct.fourierChebyshevTransform(fx)            # fx: complex tensor of nx * ny * nz values, element (i, j, k) at i + nx (j + ny k)
    fx2 = fct.inverseFourierChebyshevTransform(cn)

Plane k lies at the height cos(pi k / (nz - 1)); the definitions and scalings are in include/uammd_hip.h and DESIGN.md section 16.
"""
import ctypes as C

import torch

from ._lib import check, load
from .md import _ptr, current_stream

FORWARD, INVERSE = 1, -1


class FastChebyshevTransform:
    def __init__(self, nx, ny, nz, dtype=torch.complex64):
        if dtype not in (torch.complex64, torch.complex128):
            raise ValueError("FastChebyshevTransform: dtype must be torch.complex64 or torch.complex128")
        self.lib = load()
        self.nx, self.ny, self.nz, self.dtype = int(nx), int(ny), int(nz), dtype
        self.double = dtype == torch.complex128
        self.h = C.c_void_p()
        check(self.lib.uammd_fct_create(self.nx, self.ny, self.nz, int(self.double), C.byref(self.h)))

    def __del__(self):
        if getattr(self, "h", None):
            self.lib.uammd_fct_destroy(self.h)
            self.h = None

    def _run(self, planes, x, direction, out):
        n = self.nx * self.ny * self.nz
        if x.dtype != self.dtype or not x.is_cuda or not x.is_contiguous() or x.numel() != n:
            raise ValueError(f"FastChebyshevTransform: expected a contiguous {self.dtype} device tensor of {n} values")
        if out is None:
            out = torch.empty_like(x)
        elif out.dtype != self.dtype or not out.is_cuda or not out.is_contiguous() or out.numel() != n:
            raise ValueError(f"FastChebyshevTransform: out must be a contiguous {self.dtype} device tensor of {n} values")
        name = ("uammd_fct_fourier_chebyshev" if planes else "uammd_fct_chebyshev") + ("_f64" if self.double else "")
        check(getattr(self.lib, name)(self.h, _ptr(x), _ptr(out), direction, current_stream()))
        return out

    def chebyshevTransform(self, fx, out=None):
        """nx * ny signals sampled at the Chebyshev extrema -> their Chebyshev coefficients (chebyshevTransform3DCufft)."""
        return self._run(False, fx, FORWARD, out)

    def inverseChebyshevTransform(self, fn, out=None):
        return self._run(False, fn, INVERSE, out)

    def fourierChebyshevTransform(self, fx, out=None):
        """The same with a 2-D Fourier transform in every plane, divided by nx * ny (fourierChebyshevTransform3DCufft)."""
        return self._run(True, fx, FORWARD, out)

    def inverseFourierChebyshevTransform(self, fn, out=None):
        return self._run(True, fn, INVERSE, out)
