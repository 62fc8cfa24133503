// Host precomputation of the batched boundary value problem solver (bvp.hip; misc/BoundaryValueProblem/BVPSolver.cuh:1-30 in the
// reference).  Plain C++, no HIP: bvp.hip includes it, and so does a stand-alone program that prints the tables (tests/cxx/bvp_tables.cpp).
// Always double precision, whatever precision the solve runs in.
//
//   y''(z) - k^2 y(z) = f(z) on [-H, H],  tfi y'(H) / H + tsi y(H) / H^2 = alpha,  bfi y'(-H) / H + bsi y(-H) / H^2 = beta
//
// in Chebyshev space.  With x = z / H, a = coefficients of y'', u = y / H^2 its second integral in x:
//   d = J a + d0 e_0,  u = J d + c0 e_0 = T a + d0 e_1 + c0 e_0,  T = J J
//   J(1, 0) = 1, J(1, 2) = -1/2, J(j, j -+ 1) = +- 1 / (2 j) for j >= 2, row 0 empty (the constants live there), a_i = d_i = 0 for i >= nz
//   A a = f + k^2 H^2 (c0, d0, 0, ...),  A = I - k^2 H^2 T  (diagonals 0 and +- 2 only)
//   boundary rows  C_top = tfi J^T 1 + tsi T^T 1,  C_bot = bfi J^T s + bsi T^T s,  s_j = (-1)^j;  D = (tsi, tfi + tsi; bsi, bfi - bsi)
//   (C A^-1 B - D) (c0; d0) = C A^-1 f - (alpha; beta),  B = -k^2 H^2 (e_0 e_1)
// Only the two rows C A^-1 are needed: A^T w = c, twice, by the elimination the solve itself uses - O(nz) per system, no dense inverse.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <string>
#include <vector>

namespace uammd_hip {
namespace bvp {

// Tables of a batch, element i of system s at s + nsys i (a lane per system reads coalesced).
struct HostTables {
  int nsys = 0, nz = 0;
  double H = 0;
  std::vector<double> beta;         // nz rows: the pivots of the elimination of A (KBPENTA's beta, without its unused leading zero)
  std::vector<double> diagonal_p2;  // nz rows: A(i, i + 2), zero in the last two
  std::vector<double> diagonal_m2;  // nz rows: A(i, i - 2), zero in the first two
  std::vector<double> cinvA;        // 2 nz rows: C_top A^-1, then C_bot A^-1
  std::vector<double> m22;          // 4 rows: C A^-1 B - D, row major
  std::vector<double> kH2;          // 1 row: k^2 H^2
};

// x <- M^-1 x for M with diagonal `diag`, M(i, i - 2) = lower(i), M(i, i + 2) = upper(i); piv receives the pivots
template <class Lower, class Upper>
inline void solve_three_diagonals(int nz, const double *diag, Lower lower, Upper upper, double *piv, double *x) {
  for (int i = 0; i < nz; ++i) piv[i] = i < 2 ? diag[i] : diag[i] - lower(i) * upper(i - 2) / piv[i - 2];
  for (int i = 2; i < nz; ++i) x[i] -= lower(i) * x[i - 2] / piv[i - 2];
  for (int i = nz - 1; i >= 0; --i) x[i] = (i + 2 < nz ? x[i] - upper(i) * x[i + 2] : x[i]) / piv[i];
}

// the first-integral matrix J restricted to nz coefficients
inline double J(int row, int col, int nz) {
  if (row < 1 || row >= nz || col < 0 || col >= nz) return 0.0;
  if (row == 1) return col == 0 ? 1.0 : (col == 2 ? -0.5 : 0.0);
  if (col == row - 1) return 1.0 / (2.0 * row);
  if (col == row + 1) return -1.0 / (2.0 * row);
  return 0.0;
}
// T = J J: entries on the diagonals 0 and +- 2
inline double T(int row, int col, int nz) {
  if (row < 0 || row >= nz || col < 0 || col >= nz) return 0.0;
  if (col == row) return J(row, row - 1, nz) * J(row - 1, row, nz) + J(row, row + 1, nz) * J(row + 1, row, nz);
  if (col == row - 2) return J(row, row - 1, nz) * J(row - 1, col, nz);
  if (col == row + 2) return J(row, row + 1, nz) * J(row + 1, col, nz);
  return 0.0;
}

// Fills `out`; returns 0, or non-zero with a message that names the system at fault (nothing is usable then).
inline int precompute(int nsys, int nz, double H, const double *k, const double *tfi, const double *tsi, const double *bfi,
                      const double *bsi, HostTables &out, std::string &err) {
  char msg[256];
  if (nsys < 1) { err = "the batch needs at least one system"; return -2; }
  if (nz < 4) {
    std::snprintf(msg, sizeof(msg), "nz = %d: the second-integral recurrence needs nz >= 4", nz);
    err = msg;
    return -2;
  }
  if (!(H > 0) || !std::isfinite(H)) { err = "H must be positive and finite"; return -2; }
  out.nsys = nsys; out.nz = nz; out.H = H;
  const size_t n = (size_t)nsys;
  out.beta.assign(n * nz, 0.0);
  out.diagonal_p2.assign(n * nz, 0.0);
  out.diagonal_m2.assign(n * nz, 0.0);
  out.cinvA.assign(n * 2 * nz, 0.0);
  out.m22.assign(n * 4, 0.0);
  out.kH2.assign(n, 0.0);
  // what does not depend on the system: T's three diagonals and the column sums of J and T, plain and with alternating signs
  std::vector<double> t0(nz), tp2(nz), tm2(nz), sumJ(nz, 0.0), sumT(nz, 0.0), altJ(nz, 0.0), altT(nz, 0.0);
  for (int i = 0; i < nz; ++i) {
    t0[i] = T(i, i, nz); tp2[i] = T(i, i + 2, nz); tm2[i] = T(i, i - 2, nz);
    for (int j = 0; j < nz; ++j) {
      const double sign = (j % 2) ? -1.0 : 1.0;
      sumJ[i] += J(j, i, nz); altJ[i] += sign * J(j, i, nz);
      sumT[i] += T(j, i, nz); altT[i] += sign * T(j, i, nz);
    }
  }
  std::vector<double> diag(nz), p2(nz), m2(nz), piv(nz), pivT(nz), w(nz);
  for (int s = 0; s < nsys; ++s) {
    if (!std::isfinite(k[s]) || !std::isfinite(tfi[s]) || !std::isfinite(tsi[s]) || !std::isfinite(bfi[s]) || !std::isfinite(bsi[s])) {
      std::snprintf(msg, sizeof(msg), "system %d: non-finite wave number or boundary factor (k = %g)", s, k[s]);
      err = msg;
      return -2;
    }
    const double kH2 = k[s] * k[s] * H * H;
    for (int i = 0; i < nz; ++i) { diag[i] = 1.0 - kH2 * t0[i]; p2[i] = -kH2 * tp2[i]; m2[i] = -kH2 * tm2[i]; }
    double rows[2][2];  // the first two entries of C_top A^-1 and C_bot A^-1
    for (int r = 0; r < 2; ++r) {
      const double fi = r ? bfi[s] : tfi[s], si = r ? bsi[s] : tsi[s];
      for (int i = 0; i < nz; ++i) w[i] = r ? fi * altJ[i] + si * altT[i] : fi * sumJ[i] + si * sumT[i];
      // A^T has A(i - 2, i) = p2[i - 2] below and A(i + 2, i) = m2[i + 2] above.  At k = 0, A = I and the row stays as it is.
      if (kH2 != 0.0)
        solve_three_diagonals(nz, diag.data(), [&](int i) { return p2[i - 2]; }, [&](int i) { return m2[i + 2]; }, pivT.data(), w.data());
      for (int i = 0; i < nz; ++i) out.cinvA[s + n * (size_t)(r * nz + i)] = w[i];
      rows[r][0] = w[0]; rows[r][1] = w[1];
    }
    for (int i = 0; i < nz; ++i) piv[i] = i < 2 ? diag[i] : diag[i] - m2[i] * p2[i - 2] / piv[i - 2];
    for (int i = 0; i < nz; ++i) {
      if (!std::isfinite(piv[i]) || piv[i] == 0.0) {
        std::snprintf(msg, sizeof(msg), "system %d (k = %g): pivot %d of the second-integral matrix is %g", s, k[s], i, piv[i]);
        err = msg;
        return -2;
      }
      out.beta[s + n * i] = piv[i]; out.diagonal_p2[s + n * i] = p2[i]; out.diagonal_m2[s + n * i] = m2[i];
    }
    const double m[4] = {-kH2 * rows[0][0] - tsi[s], -kH2 * rows[0][1] - (tfi[s] + tsi[s]),
                         -kH2 * rows[1][0] - bsi[s], -kH2 * rows[1][1] - (bfi[s] - bsi[s])};
    const double det = m[0] * m[3] - m[1] * m[2];
    if (!std::isfinite(det) || det == 0.0) {
      std::snprintf(msg, sizeof(msg), "system %d (k = %g): the 2 x 2 boundary system is singular (determinant %g)", s, k[s], det);
      err = msg;
      return -2;
    }
    for (int i = 0; i < 4; ++i) out.m22[s + n * i] = m[i];
    out.kH2[s] = kH2;
  }
  return 0;
}

}  // namespace bvp
}  // namespace uammd_hip
