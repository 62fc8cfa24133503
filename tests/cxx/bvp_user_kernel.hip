// A user kernel on the boundary value problem solver: misc/BoundaryValueProblem/BVPSolver.cuh with misc/Chebyshev/FastChebyshevTransform.cuh.
// For a batch of wave numbers it samples f = y'' - k^2 y of a known y at the Chebyshev extrema of [-H, H], transforms it to Chebyshev
// coefficients (chebyshevTransform3DCufft), calls solver.solve from a kernel of its own on strided views of the interleaved arrays
// (make_interleaved_iterator, one thread per wave number), transforms the solution back (inverseChebyshevTransform3DCufft) and compares it
// with y.  It also runs the same batch through the library's kernel (BatchedBVPHandlerReal::solve) and asks for the same bits.
// Built in both precisions (examples/Makefile: bvp_user_kernel, bvp_user_kernel_dp); exit status 0 when every check holds.
#include "misc/BoundaryValueProblem/BVPSolver.cuh"
#include "misc/Chebyshev/FastChebyshevTransform.cuh"
#include "utils/container.h"
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

using namespace uammd;
using complex = thrust::complex<real>;

struct Robin {   // y' + k y at the top, y' - k y at the bottom (decaying solutions outside the slab); Dirichlet at k = 0
  real k, H, sign;
  real getFirstIntegralFactor() const { return k != 0 ? H : real(0); }
  real getSecondIntegralFactor() const { return k != 0 ? sign * k * H * H : real(1); }
};
struct RobinOf {
  const real *k;
  real H, sign;
  Robin operator[](int i) const { return Robin{k[i], H, sign}; }
};

template <class Solver>
__global__ void solveAll(Solver solver, complex *fn, const complex *alpha, const complex *beta, complex *an, complex *cn, int nsys) {
  const int id = blockIdx.x * blockDim.x + threadIdx.x;
  if (id >= nsys) return;
  auto f = chebyshev::make_interleaved_iterator(fn, id, nsys);
  auto a = chebyshev::make_interleaved_iterator(an, id, nsys);
  auto c = chebyshev::make_interleaved_iterator(cn, id, nsys);
  solver.solve(id, f, alpha[id], beta[id], a, c);
}

int main() {
  const int nz = 32, nsys = 70;   // more than one wave
  const real H = real(1.7);
  std::vector<real> k(nsys);
  for (int s = 0; s < nsys; ++s) k[s] = s == 0 ? real(0) : (s == 1 ? real(40.0 / 1.7) : real(0.3) + real(0.11) * s);
  std::vector<double> z(nz), y(nz), yp(nz), ypp(nz);
  for (int i = 0; i < nz; ++i) {
    z[i] = double(H) * std::cos(M_PI * i / (nz - 1));
    const double e = std::exp(-z[i] * z[i]);
    y[i] = e + 0.3 * std::sin(2 * z[i]);
    yp[i] = -2 * z[i] * e + 0.6 * std::cos(2 * z[i]);
    ypp[i] = (4 * z[i] * z[i] - 2) * e - 1.2 * std::sin(2 * z[i]);
  }
  std::vector<complex> f((size_t)nz * nsys), alpha(nsys), beta(nsys);
  RobinOf top{k.data(), H, real(1)}, bot{k.data(), H, real(-1)};
  for (int s = 0; s < nsys; ++s) {
    for (int i = 0; i < nz; ++i) {
      const double v = ypp[i] - double(k[s]) * double(k[s]) * y[i];
      f[s + (size_t)nsys * i] = complex(real(v), real(-0.5 * v));   // the imaginary part solves the same problem scaled by -1/2
    }
    const double a = top[s].getFirstIntegralFactor() * yp[0] / H + top[s].getSecondIntegralFactor() * y[0] / (double(H) * H);
    const double b = bot[s].getFirstIntegralFactor() * yp[nz - 1] / H + bot[s].getSecondIntegralFactor() * y[nz - 1] / (double(H) * H);
    alpha[s] = complex(real(a), real(-0.5 * a));
    beta[s] = complex(real(b), real(-0.5 * b));
  }
  uninitialized_cached_vector<complex> d_f(f), d_alpha(alpha), d_beta(beta);
  const int3 n = make_int3(nsys, 1, nz);
  auto fn = chebyshev::chebyshevTransform3DCufft(d_f, n);   // nsys (2 nz - 2) values; the solver reads the first nz planes
  uninitialized_cached_vector<complex> an(fn.size()), cn(fn.size()), an2(fn.size()), cn2(fn.size());
  BVP::BatchedBVPHandlerReal bvp(k, top, bot, nsys, H, nz);
  auto solver = bvp.getGPUSolver();
  solveAll<<<nsys / 64 + 1, 64>>>(solver, fn.data().get(), d_alpha.data().get(), d_beta.data().get(), an.data().get(), cn.data().get(), nsys);
  if (hipDeviceSynchronize() != hipSuccess) { std::printf("the user kernel failed\n"); return 1; }
  bvp.solve(fn.data().get(), d_alpha.data().get(), d_beta.data().get(), an2.data().get(), cn2.data().get(), 1, 1, nsys);
  auto yy = chebyshev::inverseChebyshevTransform3DCufft(cn, n);
  std::vector<complex> got = yy, c1 = cn, c2 = cn2, a1 = an, a2 = an2;
  const size_t used = (size_t)nz * nsys;
  const bool sameBits = std::memcmp(c1.data(), c2.data(), used * sizeof(complex)) == 0 && std::memcmp(a1.data(), a2.data(), used * sizeof(complex)) == 0;
  double err = 0;
  for (int s = 0; s < nsys; ++s)
    for (int i = 0; i < nz; ++i) {
      const complex v = got[s + (size_t)nsys * i];
      err = std::fmax(err, std::fmax(std::fabs(double(v.real()) - y[i]), std::fabs(double(v.imag()) + 0.5 * y[i])));
    }
  // double: the bar of the CPU restatement's check of this solution.  float: the single-precision solve is allowed 1.6e-6 of max |c_n| per
  // coefficient (tests/test_gpu_chebyshev_bvp.py) and y sums nz = 32 of them with |T_n| <= 1: 32 x 1.6e-6 = 5e-5.
  const double bar = sizeof(real) == sizeof(double) ? 1e-12 : 5e-5;
  std::printf("bvp_user_kernel: %d systems, nz = %d, max |y - exact| = %.3e (bar %.1e), user kernel and library kernel %s\n", nsys, nz, err, bar,
              sameBits ? "give the same bits" : "DIFFER");
  return (err <= bar && sameBits) ? 0 : 1;
}
