// Batched boundary value problem solver: the include path and public names of the reference's
// src/misc/BoundaryValueProblem/BVPSolver.cuh, written for this build.  A hipcc header, like device/*.hip.hpp.
//
//   y''(z) - k^2 y(z) = f(z) on [-H, H],  tfi y'(H) / H + tsi y(H) / H^2 = alpha,  bfi y'(-H) / H + bsi y(-H) / H^2 = beta
//
// in Chebyshev space, one independent system per wave number.  BatchedBVPHandlerReal takes the wave numbers and the
// boundary factors, has libuammd_hip compute the tables on the host in double precision (uammd_bvp_create) and keeps them on the
// device.  getGPUSolver() returns a small copyable object for kernels of the user's own: solve(instance, fn, alpha, beta, an, cn)
// runs one system over any random-access iterators and reads the same tables with the same device function (device/BVP.hip.hpp) as
// the library's batched kernel, uammd_bvp_solve, which solve() of the handler launches.  Real tables, complex (or real) right-hand
// sides: the instantiation the reference's solvers use.  real = double with -DDOUBLE_PRECISION.
#pragma once
// (thrust and device code: the contents need a translation unit compiled by hipcc; a plain C++ compiler sees an empty header)
#if defined(__HIPCC__)
#include "../../uammd.cuh"
#include "../../device/BVP.hip.hpp"
#include "BVPMemory.cuh"
#include "MatrixUtils.h"
#include <memory>
#include <vector>

namespace uammd {
namespace BVP {

class BatchedBVPHandlerReal;

struct BatchedBVPGPUSolverReal {
  // fn: coefficients of f (read only); an receives those of y'', cn those of y
  template <class T, class FnIterator, class AnIterator, class CnIterator>
  __device__ void solve(int instance, const FnIterator &fn, T alpha, T beta, const AnIterator &an, const CnIterator &cn) const {
    device::solveSystem(tables, instance, fn, alpha, beta, an, cn);
  }

private:
  device::Tables<real> tables;
  friend class BatchedBVPHandlerReal;
};

class BatchedBVPHandlerReal {
  std::shared_ptr<uammd_bvp> handle;
  int numberSystems, nz;
  real H;

public:
  // klist[i]: wave number of system i; top[i] / bot[i]: objects with getFirstIntegralFactor() and getSecondIntegralFactor()
  template <class WaveVectorIterator, class BatchedTopBC, class BatchedBottomBC>
  BatchedBVPHandlerReal(const WaveVectorIterator &klist, BatchedTopBC top, BatchedBottomBC bot, int numberSystems, real H, int nz)
      : numberSystems(numberSystems), nz(nz), H(H) {
    std::vector<double> par[5];
    for (auto &p : par) p.resize(numberSystems > 0 ? numberSystems : 0);
    for (int i = 0; i < numberSystems; ++i) {
      const auto t = top[i];
      const auto b = bot[i];
      par[0][i] = klist[i];
      par[1][i] = t.getFirstIntegralFactor();
      par[2][i] = t.getSecondIntegralFactor();
      par[3][i] = b.getFirstIntegralFactor();
      par[4][i] = b.getSecondIntegralFactor();
    }
    uammd_bvp *h = nullptr;
#if defined(DOUBLE_PRECISION)
    const int dp = 1;
#else
    const int dp = 0;
#endif
    uammd::detail::check(uammd_bvp_create(numberSystems, nz, H, par[0].data(), par[1].data(), par[2].data(), par[3].data(), par[4].data(), dp, &h));
    handle = std::shared_ptr<uammd_bvp>(h, [](uammd_bvp *p) { uammd_bvp_destroy(p); });
  }

  BatchedBVPGPUSolverReal getGPUSolver() {
    uammd_bvp_tables t;
    uammd::detail::check(uammd_bvp_device_tables(handle.get(), &t));
    BatchedBVPGPUSolverReal solver;
    solver.tables = device::Tables<real>::over(static_cast<const real *>(t.d_tables), t.nsys, t.nz, H * H);
    return solver;
  }

  // All systems for nrhs right-hand sides with the library's kernel: complex values, element i of system s at s sysStride + i coefStride,
  // (1, numberSystems) or (nz, 1); alpha and beta hold nrhs numberSystems values.
  template <class Complex>
  void solve(const Complex *fn, const Complex *alpha, const Complex *beta, Complex *an, Complex *cn, int nrhs, long long sysStride,
             long long coefStride, hipStream_t st = 0) {
    static_assert(sizeof(Complex) == 2 * sizeof(real), "solve takes complex values of the build's precision");
    auto in = [](const Complex *p) { return reinterpret_cast<const real *>(p); };
    auto out = [](Complex *p) { return reinterpret_cast<real *>(p); };
#if defined(DOUBLE_PRECISION)
    uammd::detail::check(uammd_bvp_solve_f64(handle.get(), in(fn), in(alpha), in(beta), out(an), out(cn), nrhs, sysStride, coefStride, st));
#else
    uammd::detail::check(uammd_bvp_solve(handle.get(), in(fn), in(alpha), in(beta), out(an), out(cn), nrhs, sysStride, coefStride, st));
#endif
  }

  int getNumberSystems() const { return numberSystems; }
};

}  // namespace BVP
}  // namespace uammd
#endif  // __HIPCC__
