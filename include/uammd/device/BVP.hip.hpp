// One system of the batched boundary value problem solver, as device code.  The library's kernel (csrc/bvp.hip) and the
// solver object user kernels call (misc/BoundaryValueProblem/BVPSolver.cuh: getGPUSolver().solve) both run this function on the same
// device tables, so the two give the same bits.  Self-contained: a hipcc translation unit needs nothing else.
//
// U is the tables' scalar (float or double); T the right-hand side's value type: anything with T + T, T - T, T * U, T / U and T() = 0
// (the runtime's float2 / double2, thrust::complex, a plain real).  fn, an and cn are random-access: x[i] reads, x[i] = v writes.
#pragma once
#include <hip/hip_runtime.h>

namespace uammd {
namespace BVP {
namespace device {

// Element i of system s of every table sits at s + nsys i (uammd_amd/csrc/bvp_host.hpp computes them).
template <class U> struct Tables {
  const U *beta = nullptr;         // nz rows: pivots
  const U *diagonal_p2 = nullptr;  // nz rows: A(i, i + 2)
  const U *diagonal_m2 = nullptr;  // nz rows: A(i, i - 2)
  const U *cinvA = nullptr;        // 2 nz rows: C_top A^-1, C_bot A^-1
  const U *m22 = nullptr;          // 4 rows: C A^-1 B - D
  const U *kH2 = nullptr;          // 1 row
  int nsys = 0, nz = 0;
  U H2 = 0;                        // H^2
  // the tables as the library keeps them (uammd_bvp_device_tables): one array, in the order above
  static Tables over(const U *d, int nsys, int nz, U H2) {
    const size_t n = (size_t)nsys;
    Tables t;
    t.beta = d;
    t.diagonal_p2 = d + n * nz;
    t.diagonal_m2 = d + n * 2 * nz;
    t.cinvA = d + n * 3 * nz;
    t.m22 = d + n * 5 * nz;
    t.kH2 = d + n * (5 * nz + 4);
    t.nsys = nsys;
    t.nz = nz;
    t.H2 = H2;
    return t;
  }
};

// fn is read only.  an receives the coefficients of y'', cn those of y.
template <class U, class T, class FnIterator, class AnIterator, class CnIterator>
__device__ inline void solveSystem(const Tables<U> &t, int s, const FnIterator &fn, T alpha, T beta, const AnIterator &an,
                                   const CnIterator &cn) {
  const int nz = t.nz;
  const size_t n = (size_t)t.nsys;
  // (c0; d0) from the 2 x 2 system
  T r0 = T(), r1 = T();
  for (int i = 0; i < nz; ++i) {
    const T f = fn[i];
    r0 = r0 + f * t.cinvA[s + n * i];
    r1 = r1 + f * t.cinvA[s + n * (nz + i)];
  }
  r0 = r0 - alpha;
  r1 = r1 - beta;
  const U m0 = t.m22[s], m1 = t.m22[s + n], m2 = t.m22[s + 2 * n], m3 = t.m22[s + 3 * n];
  const U det = m0 * m3 - m1 * m2;
  const T c0 = (r0 * m3 - r1 * m1) / det;
  const T d0 = (r1 * m0 - r0 * m2) / det;
  // A a = f + k^2 H^2 (c0, d0, 0, ...): forward elimination, then back substitution, on the diagonals 0 and +- 2
  const U kH2 = t.kH2[s];
  {
    const T f0 = fn[0], f1 = fn[1];
    an[0] = f0 + c0 * kH2;
    an[1] = f1 + d0 * kH2;
  }
  for (int i = 2; i < nz; ++i) {
    const T f = fn[i], below = an[i - 2];
    an[i] = f - below * t.diagonal_m2[s + n * i] / t.beta[s + n * (i - 2)];
  }
  for (int i = nz - 1; i >= 0; --i) {
    T v = an[i];
    if (i + 2 < nz) {
      const T above = an[i + 2];
      v = v - above * t.diagonal_p2[s + n * i];
    }
    an[i] = v / t.beta[s + n * i];
  }
  // y = H^2 (second integral of a with the constants c0, d0); every a_i and d_i with i >= nz is zero
  auto a = [&](int i) -> T { return i < nz ? T(an[i]) : T(); };
  auto d = [&](int i) -> T {  // first integral
    if (i == 0) return d0;
    if (i >= nz) return T();
    if (i == 1) return a(0) - a(2) * U(0.5);
    return (a(i - 1) - a(i + 1)) * (U(0.5) / U(i));
  };
  cn[0] = c0 * t.H2;
  cn[1] = (d0 - d(2) * U(0.5)) * t.H2;
  for (int i = 2; i < nz; ++i) cn[i] = ((d(i - 1) - d(i + 1)) * (U(0.5) / U(i))) * t.H2;
}

}  // namespace device
}  // namespace BVP
}  // namespace uammd
