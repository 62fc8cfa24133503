// Checks the host tables both doubly periodic solvers build from (uammd_amd/csrc/dp_slab_host.hpp).  Plain C++14, no HIP, no library: a
// CPU test builds this with the address and undefined-behaviour sanitizers and runs it (tests/test_dpstokes_cpu.py).
//   1  clencurt(i, n), i = 0 .. n, sums to 2 and integrates x^m over [-1, 1] exactly for even m <= n (Clenshaw-Curtis on n + 1 points
//      is exact up to degree n), n = nz - 1 odd and even; chebyshev_planes puts them on [-Hh, Hh] times hx hy.  Bar 1e-13: a weight is
//      2 / n times a sum of n / 2 cosines, an error of a few 1e-16 each, and a rule sums at most 73 of them.
//   2  mirror is an involution that fixes the zero index and the unpaired Nyquist indices.
//   3  wave_vector gives, to the bit, what stood inline in the Poisson solver's table loop before both solvers shared it.
//   4  bvp_boundary_factors gives (0, 1, 0, 1) at k = 0 and (Hh, Hh^2 k, Hh, -Hh^2 k) otherwise.
#include "../../uammd_amd/csrc/dp_slab_host.hpp"

#include <cstdio>

using namespace uammd_hip;

static int failures = 0;
#define EXPECT(cond, ...)                                   \
  do {                                                      \
    if (!(cond)) {                                          \
      ++failures;                                           \
      std::printf("FAILED %s: ", #cond);                    \
      std::printf(__VA_ARGS__);                             \
      std::printf("\n");                                    \
    }                                                       \
  } while (0)

static void check_clencurt(int nz) {
  const int n = nz - 1;
  double sum = 0;
  for (int i = 0; i <= n; ++i) sum += dp::clencurt(i, n);
  EXPECT(std::fabs(sum - 2.0) <= 1e-13, "nz %d: the weights sum to %.17g", nz, sum);
  for (int m = 0; m <= n; m += 2) {
    double integral = 0;
    for (int i = 0; i <= n; ++i) integral += dp::clencurt(i, n) * std::pow(std::cos(M_PI * i / n), m);
    EXPECT(std::fabs(integral - 2.0 / (m + 1)) <= 1e-13, "nz %d: x^%d integrates to %.17g, not %.17g", nz, m, integral, 2.0 / (m + 1));
  }
  const double Hh = 3.5, hx = 0.25, hy = 0.4;
  std::vector<double> zp, qw;
  dp::chebyshev_planes(nz, Hh, hx, hy, zp, qw);
  EXPECT((int)zp.size() == nz && (int)qw.size() == nz, "nz %d: %zu planes, %zu weights", nz, zp.size(), qw.size());
  EXPECT(zp[0] == Hh && zp[n] == -Hh, "nz %d: the planes end at %.17g and %.17g", nz, zp[0], zp[n]);
  double volume = 0;
  for (int i = 0; i <= n; ++i) {
    volume += qw[i];
    EXPECT(i == 0 || zp[i] < zp[i - 1], "nz %d: plane %d is not below plane %d", nz, i, i - 1);
    EXPECT(qw[i] == Hh * dp::clencurt(i, n) * (hx * hy), "nz %d: weight %d", nz, i);
  }
  EXPECT(std::fabs(volume - 2.0 * Hh * hx * hy) <= 1e-13 * 2.0 * Hh * hx * hy, "nz %d: the weights sum to %.17g", nz, volume);
}

static void check_plane(int nx, int ny) {
  const double Lx = 8.0, Ly = 9.0;
  for (int s = 0; s < nx * ny; ++s) {
    const int i = s % nx, j = s / nx;
    const int sm = dp::mirror(s, nx, ny);
    EXPECT(sm >= 0 && sm < nx * ny && dp::mirror(sm, nx, ny) == s, "%d x %d: mirror(mirror(%d)) = %d", nx, ny, s, dp::mirror(sm, nx, ny));
    const bool ownX = i == 0 || (nx % 2 == 0 && i == nx / 2), ownY = j == 0 || (ny % 2 == 0 && j == ny / 2);
    EXPECT((sm == s) == (ownX && ownY), "%d x %d: mirror(%d) = %d", nx, ny, s, sm);
    // the formula of the Poisson solver's table loop, as it stood
    const double wx = 2 * M_PI / Lx * (i - nx * (i >= nx / 2 + 1)), wy = 2 * M_PI / Ly * (j - ny * (j >= ny / 2 + 1));
    const double k = std::sqrt(wx * wx + wy * wy);
    const double kx = (nx % 2 == 0 && i == nx / 2) ? 0.0 : wx;
    const double ky = (ny % 2 == 0 && j == ny / 2) ? 0.0 : wy;
    double gx, gy, gk;
    dp::wave_vector(s, nx, ny, Lx, Ly, gx, gy, gk);
    EXPECT(gx == kx && gy == ky && gk == k, "%d x %d: wave vector %d is (%.17g, %.17g, %.17g), not (%.17g, %.17g, %.17g)", nx, ny, s, gx, gy, gk, kx,
           ky, k);
  }
}

static void check_boundary_factors() {
  const double Hh = 2.75;
  double a, b, c, d;
  dp::bvp_boundary_factors(0.0, Hh, a, b, c, d);
  EXPECT(a == 0.0 && b == 1.0 && c == 0.0 && d == 1.0, "k = 0: (%g, %g, %g, %g)", a, b, c, d);
  const double ks[3] = {1e-3, 0.7853981633974483, 41.0};
  for (double k : ks) {
    dp::bvp_boundary_factors(k, Hh, a, b, c, d);
    EXPECT(a == Hh && b == Hh * Hh * k && c == Hh && d == -Hh * Hh * k, "k = %g: (%g, %g, %g, %g)", k, a, b, c, d);
  }
}

int main() {
  const int nzs[5] = {4, 5, 19, 22, 73};
  for (int nz : nzs) check_clencurt(nz);
  const int planes[4][2] = {{12, 14}, {15, 12}, {25, 25}, {20, 18}};
  for (const auto &p : planes) check_plane(p[0], p[1]);
  check_boundary_factors();
  if (failures) std::printf("%d checks FAILED\n", failures);
  else std::printf("dp_slab tables ok\n");
  return failures ? 1 : 0;
}
