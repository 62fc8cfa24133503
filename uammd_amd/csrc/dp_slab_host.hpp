// Host tables both doubly periodic solvers build from (dppoisson.hip, dpstokes.hip): the Chebyshev planes with their
// Clenshaw-Curtis weights, the wave vectors of a full plane, and the boundary factors of the per-wave-number boundary value problems.
// Plain C++14, no HIP: the solvers include it, and so does a stand-alone program that checks it (tests/cxx/dp_slab_tables.cpp).  Always
// double precision, whatever precision the solve runs in; the tables feed results that are compared to the bit, so the expressions here
// are written once and left alone.
#pragma once
#include <cmath>
#include <vector>

namespace uammd_hip {
namespace dp {

inline double clencurt(int i, int n) {  // misc/ChevyshevUtils.cuh:13-30
  double v = 1;
  if (n % 2 == 0) {
    if (i == 0 || i == n) return 1.0 / (n * (double)n - 1.0);
    for (int k = 1; k <= n / 2 - 1; k++) v -= 2 * std::cos(2 * k * M_PI * i / n) / (4.0 * k * k - 1);
    v -= std::cos(M_PI * i) / (n * (double)n - 1.0);
  } else {
    if (i == 0 || i == n) return 1.0 / (n * (double)n);
    for (int k = 1; k <= (n - 1) / 2; k++) v -= 2 * std::cos(2 * k * M_PI * i / n) / (4.0 * k * k - 1);
  }
  return 2.0 * v / n;
}

// nz planes over [-Hh, Hh], plane 0 at the top, and the weights of a sum over nodes that integrates over the slab
inline void chebyshev_planes(int nz, double Hh, double hx, double hy, std::vector<double> &zp, std::vector<double> &qw) {
  zp.resize(nz);
  qw.resize(nz);
  for (int i = 0; i < nz; ++i) {
    zp[i] = Hh * std::cos(M_PI * i / (nz - 1));
    qw[i] = Hh * clencurt(i, nz - 1) * (hx * hy);
  }
}

// system s = i + nx j of a full plane: the modulus of its wave vector, and the wave vector with a zero on an unpaired index (for an even
// size the Nyquist index carries no derivative along its axis; an odd size has no unpaired index)
inline void wave_vector(int s, int nx, int ny, double Lx, double Ly, double &kx, double &ky, double &k) {
  const int i = s % nx, j = s / nx;
  kx = 2 * M_PI / Lx * (i - nx * (i >= nx / 2 + 1));
  ky = 2 * M_PI / Ly * (j - ny * (j >= ny / 2 + 1));
  k = std::sqrt(kx * kx + ky * ky);
  if (nx % 2 == 0 && i == nx / 2) kx = 0.0;
  if (ny % 2 == 0 && j == ny / 2) ky = 0.0;
}
constexpr int mirror(int s, int nx, int ny) {  // the system of the opposite wave vector (constexpr: the kernels call it too)
  const int i = s % nx, j = s / nx;
  return (i ? nx - i : 0) + nx * (j ? ny - j : 0);
}

// the boundary factors the batched solver takes per wave number, top and bottom (BoundaryConditions.cuh:13-33,
// StokesSlab/initialization.cu:74-96): (0, 1, 0, 1) at k = 0, else (Hh, Hh^2 k, Hh, -Hh^2 k)
inline void bvp_boundary_factors(double k, double Hh, double &tfi, double &tsi, double &bfi, double &bsi) {
  const bool nonzero = k != 0;
  tfi = nonzero ? Hh : 0.0;
  tsi = nonzero ? Hh * Hh * k : 1.0;
  bfi = nonzero ? Hh : 0.0;
  bsi = nonzero ? -Hh * Hh * k : 1.0;
}

}  // namespace dp
}  // namespace uammd_hip
