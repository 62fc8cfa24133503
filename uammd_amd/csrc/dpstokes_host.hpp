// Host precomputation of the doubly periodic Stokes solver's wall correction (dpstokes.hip; StokesSlab/Correction.cuh:493-626 in the
// reference).  Plain C++, no HIP: dpstokes.hip includes it, and so does a stand-alone program that prints the tables
// (tests/cxx/dpstokes_tables.cpp).  Always double precision, whatever precision the solve runs in.
//
//   slit: per wave number k != 0 the eight constants of the analytic correction solve A C = b, A the 8 x 8 complex matrix of
//         evaluateSlitCorrectionMatrix; the inverse is kept, row major.  Elimination with partial pivoting, no library.
//   k = 0: mu u'' = -f with u(-H/2) = 0 and u'(H/2) = 0 (bottom) or u(H/2) = 0 (slit): the batched solver's rows (bvp_host.hpp) for one
//         system with k = 0 and the boundary factors below.
#pragma once
#include "bvp_host.hpp"
#include "dp_slab_host.hpp"

#include <complex>
#include <utility>

namespace uammd_hip {
namespace dps {

enum WallMode { kNone = 0, kBottom = 1, kSlit = 2 };
using cplx = std::complex<double>;

// evaluateSlitCorrectionMatrix (Correction.cuh:493-566); unknowns (C0, D0, C1, D1, C2, D2, C3, D3), rows: the two divergence
// conditions, then u, v, w at the bottom wall and u, v, w at the top wall.  (kx, ky) multiplies i and is zero on an unpaired (Nyquist)
// index, as in the solve; k is the modulus of the full wave vector.
inline void slit_matrix(double kx, double ky, double k, double viscosity, double H, cplx *A) {
  const double hm = 0.5 / viscosity, e = std::exp(-k * H);
  const cplx i(0.0, 1.0);
  for (int n = 0; n < 64; ++n) A[n] = 0.0;
  A[0] = hm; A[1] = e * hm; A[6] = -k; A[7] = k * e;
  A[8] = (1.0 - k * H) * e * hm; A[9] = (1.0 + k * H) * hm; A[14] = -k * e; A[15] = k;
  A[16 + 2] = 1.0; A[16 + 3] = e;
  A[24 + 4] = 1.0; A[24 + 5] = e;
  A[32 + 6] = 1.0; A[32 + 7] = e;
  A[40] = -i * (kx * H * e * hm / k); A[41] = i * (kx * H * hm / k); A[42] = e; A[43] = 1.0;
  A[48] = -i * (ky * H * e * hm / k); A[49] = i * (ky * H * hm / k); A[52] = e; A[53] = 1.0;
  A[56] = H * e * hm; A[57] = H * hm; A[62] = e; A[63] = 1.0;
}

// inv <- A^-1 (n x n, row major) by Gauss-Jordan elimination with partial pivoting; A is destroyed.  false: a pivot vanished.
inline bool invert(int n, cplx *A, cplx *inv) {
  for (int r = 0; r < n; ++r)
    for (int c = 0; c < n; ++c) inv[r * n + c] = r == c ? 1.0 : 0.0;
  for (int col = 0; col < n; ++col) {
    int piv = col;
    double best = std::abs(A[col * n + col]);
    for (int r = col + 1; r < n; ++r)
      if (std::abs(A[r * n + col]) > best) { best = std::abs(A[r * n + col]); piv = r; }
    if (!(best > 0.0) || !std::isfinite(best)) return false;
    if (piv != col)
      for (int c = 0; c < n; ++c) { std::swap(A[piv * n + c], A[col * n + c]); std::swap(inv[piv * n + c], inv[col * n + c]); }
    const cplx d = 1.0 / A[col * n + col];
    for (int c = 0; c < n; ++c) { A[col * n + c] *= d; inv[col * n + c] *= d; }
    for (int r = 0; r < n; ++r) {
      if (r == col) continue;
      const cplx f = A[r * n + col];
      if (f == 0.0) continue;
      for (int c = 0; c < n; ++c) { A[r * n + c] -= f * A[col * n + c]; inv[r * n + c] -= f * inv[col * n + c]; }
    }
  }
  return true;
}

using dp::mirror;
using dp::wave_vector;

// out[64 s + 8 r + c]: the inverse of wave number s; the k = 0 block stays zero (the zero mode has a solve of its own).
// Returns 0, or -2 with a message that names the wave number at fault.
inline int slit_inverses(int nx, int ny, double Lx, double Ly, double viscosity, double H, std::vector<cplx> &out, std::string &err) {
  const int nsys = nx * ny;
  out.assign((size_t)64 * nsys, 0.0);
  cplx A[64], condCheck[64];
  for (int s = 1; s < nsys; ++s) {
    const int sm = mirror(s, nx, ny);
    if (sm < s) {  // the matrix of -k is the conjugate: so is its inverse, to the bit
      for (int n = 0; n < 64; ++n) out[(size_t)64 * s + n] = std::conj(out[(size_t)64 * sm + n]);
      continue;
    }
    double kx, ky, k;
    wave_vector(s, nx, ny, Lx, Ly, kx, ky, k);
    slit_matrix(kx, ky, k, viscosity, H, A);
    bool ok = invert(8, A, condCheck);
    for (int n = 0; ok && n < 64; ++n) ok = std::isfinite(condCheck[n].real()) && std::isfinite(condCheck[n].imag());
    if (!ok) {
      char msg[256];
      std::snprintf(msg, sizeof(msg), "[DPStokes] the slit correction matrix of wave number %d (kx = %g, ky = %g) is singular", s, kx, ky);
      err = msg;
      return -2;
    }
    for (int n = 0; n < 64; ++n) out[(size_t)64 * s + n] = condCheck[n];
  }
  return 0;
}

// boundary factors (tfi, tsi, bfi, bsi) of the k = 0 solve (Correction.cuh:44-68, :600-614)
inline void zero_mode_factors(int mode, double f[4]) {
  f[0] = mode == kBottom ? 1.0 : 0.0;
  f[1] = mode == kBottom ? 0.0 : -1.0;
  f[2] = 0.0;
  f[3] = -1.0;
}

// the rows of the k = 0 solve: cinvA[2 nz] = C and m22[4] = -D
inline int zero_mode_rows(int mode, int nz, double halfH, bvp::HostTables &t, std::string &err) {
  double f[4];
  zero_mode_factors(mode, f);
  const double k0 = 0.0;
  return bvp::precompute(1, nz, halfH, &k0, &f[0], &f[1], &f[2], &f[3], t, err);
}

}  // namespace dps
}  // namespace uammd_hip
