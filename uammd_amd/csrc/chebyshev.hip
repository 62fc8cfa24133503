// Fast Chebyshev and Fourier-Chebyshev transforms for gfx950 (misc/Chebyshev/FastChebyshevTransform.cuh:147-260 in the reference;
// DESIGN.md 16).  Element (i, j, k) of a complex field sits at i + nx (j + ny k); plane k lies at the height cos(pi k / n), n = nz - 1.
//
//   forward   c_k = pm_k / (2 n) [f_0 + (-1)^k f_n + 2 sum_{j = 1}^{n - 1} f_j cos(pi j k / n)],  pm_k = 1 for k in {0, n}, else 2
//   inverse   f_j = sum_k c_k cos(pi j k / n)
//   the Fourier-Chebyshev forms add a 2-D complex transform over (i, j) in every plane: forward e^{-i...} / (nx ny), inverse e^{+i...}
//
// The z pass (k_cheb_z).  The reference writes the even extension of length 2 nz - 2 to memory and runs a strided 1-D FFT over it.
// Here the cosine sums are taken directly on the nz planes: a wave owns 64 consecutive columns, so every plane row it loads is
// contiguous, and the index of the table value, (j k) mod 2 n, is the same in all its lanes (kept in integers and stepped by k, so the
// argument reduction is exact).  The table cos(pi m / n), m in [0, 2 n), comes from the host in extended precision.  Each lane holds
// kOut outputs k in registers and feeds every loaded input to all of them.  The pm scaling and the 1 / (nx ny) of the plane transform
// are folded into the store.
//   float   cos(pi (n - j) k / n) = (-1)^k cos(pi j k / n): planes j and n - j are added (even k) or subtracted (odd k) first, which
//           halves the products and the table reads.
//   double  no pairing (the pre-addition would round); the table is a double-double (hi + lo), each product's rounding error is
//           recovered with an fma, and the sum is compensated: the result is the exactly rounded sum to within an ulp or two.  The
//           reference's own tests ask 1e-15 absolute of one transform, which a plain sum of 32 terms misses.
// The plane transform is rocFFT, batched over the nz contiguous planes, in place on the output of the z pass: the two transforms act
// on different axes and commute, so running the z pass first (in -> out) needs no work array in either direction.
#include "rocfft_plans.hpp"

#include <cmath>
#include <new>
#include <vector>

namespace uammd_hip {

namespace fct {
constexpr int kOut = 8;  // outputs k per lane
}

template <class R> struct Cplx { R x, y; };

// s + c += x (t + tl), compensated
template <class R> UH_D void add_product(R &s, R &c, R x, R t, R tl) {
  const R p = x * t;
  const R pe = fma_(x, t, -p) + x * tl;
  const R sum = s + p;
  const R bb = sum - s;
  const R err = (s - (sum - bb)) + (p - bb);
  s = sum;
  c += err + pe;
}

template <class R, bool kAccurate>
__global__ __launch_bounds__(64) void k_cheb_z(const Cplx<R> *__restrict__ in, Cplx<R> *__restrict__ out, int nk, int nz,
                                               const R *__restrict__ tabHi, const R *__restrict__ tabLo, int forward, R norm) {
  constexpr int KO = fct::kOut;
  const int col = blockIdx.x * 64 + threadIdx.x;
  const int k0 = blockIdx.y * KO;
  if (col >= nk) return;
  const int n = nz - 1, n2 = 2 * n;
  const size_t plane = (size_t)nk;
  const Cplx<R> *src = in + col;
  R sr[KO], si[KO], cr[KO], ci[KO];
  int idx[KO], step[KO];
#pragma unroll
  for (int q = 0; q < KO; ++q) {
    sr[q] = si[q] = cr[q] = ci[q] = R(0);
    idx[q] = 0;
    step[q] = (k0 + q) % n2;
  }
  const R endWeight = forward ? R(0.5) : R(1);  // forward: the two end planes count half (exact), the scale below carries pm / n
  if (kAccurate) {
    for (int j = 0; j <= n; ++j) {
      Cplx<R> a = src[plane * j];
      if (j == 0 || j == n) { a.x *= endWeight; a.y *= endWeight; }
#pragma unroll
      for (int q = 0; q < KO; ++q) {
        const R t = tabHi[idx[q]], tl = tabLo[idx[q]];
        add_product(sr[q], cr[q], a.x, t, tl);
        add_product(si[q], ci[q], a.y, t, tl);
        idx[q] += step[q];
        if (idx[q] >= n2) idx[q] -= n2;
      }
    }
#pragma unroll
    for (int q = 0; q < KO; ++q) { sr[q] += cr[q]; si[q] += ci[q]; }
  } else {
    for (int j = 0; 2 * j < n; ++j) {
      Cplx<R> a = src[plane * j], b = src[plane * (n - j)];
      if (j == 0) { a.x *= endWeight; a.y *= endWeight; b.x *= endWeight; b.y *= endWeight; }
      const Cplx<R> e = {a.x + b.x, a.y + b.y}, o = {a.x - b.x, a.y - b.y};
#pragma unroll
      for (int q = 0; q < KO; ++q) {
        const R t = tabHi[idx[q]];
        const Cplx<R> v = (q & 1) ? o : e;  // k0 is a multiple of the even kOut: k's parity is q's
        sr[q] = fma_(v.x, t, sr[q]);
        si[q] = fma_(v.y, t, si[q]);
        idx[q] += step[q];
        if (idx[q] >= n2) idx[q] -= n2;
      }
    }
    if (n % 2 == 0) {  // the middle plane pairs with itself; idx has reached (n / 2) k mod 2 n
      const Cplx<R> a = src[plane * (n / 2)];
#pragma unroll
      for (int q = 0; q < KO; ++q) {
        const R t = tabHi[idx[q]];
        sr[q] = fma_(a.x, t, sr[q]);
        si[q] = fma_(a.y, t, si[q]);
      }
    }
  }
#pragma unroll
  for (int q = 0; q < KO; ++q) {
    const int k = k0 + q;
    if (k < nz) {
      const R scale = forward ? norm * ((k == 0 || k == n) ? R(1) : R(2)) / R(n) : norm;
      out[col + plane * k] = {sr[q] * scale, si[q] * scale};
    }
  }
}
static_assert(fct::kOut % 2 == 0, "k_cheb_z takes k's parity from the register index");

struct FCT {
  int nx = 0, ny = 0, nz = 0;
  bool doublePrecision = false;
  DeviceBuffer table;  // hi[2 n], then lo[2 n] in the double build
  RealFFT planes;      // the two complex plans (forward, inverse) with their execution info; unused when nx ny == 1
};

// cos(pi m / n), m in [0, 2 n): folded in integers onto an angle in [0, pi / 4]
static long double cos_pi_ratio(int m, int n) {
  if (m > n) m = 2 * n - m;
  long double sign = 1;
  if (2 * m > n) { sign = -1; m = n - m; }
  if (2 * m == n) return 0;
  const long double pi = 3.141592653589793238462643383279502884L;
  return sign * (4 * m <= n ? cosl(pi * m / n) : sinl(pi * (n - 2 * m) / (2 * (long double)n)));
}

template <class R> static int fct_upload_table(FCT *h) {
  const int n2 = 2 * (h->nz - 1);
  std::vector<R> host(2 * (size_t)n2);
  for (int m = 0; m < n2; ++m) {
    const long double v = cos_pi_ratio(m, h->nz - 1);
    host[m] = (R)v;
    host[n2 + m] = (R)(v - (long double)host[m]);
  }
  if (int e = h->table.reserve(host.size() * sizeof(R))) return e;
  UH_CHECK(hipMemcpy(h->table.ptr, host.data(), host.size() * sizeof(R), hipMemcpyHostToDevice));
  return 0;
}

static int fct_make_plans(FCT *h) {
  const size_t nx = h->nx, ny = h->ny;
  if (nx * ny == 1) return 0;
  // an axis of length one is left out of the plan
  const size_t rank = (nx > 1 && ny > 1) ? 2 : 1;
  const size_t lengths[2] = {nx > 1 ? nx : ny, ny}, strides[2] = {1, nx};
  const rocfft_precision prec = h->doublePrecision ? rocfft_precision_double : rocfft_precision_single;
  if (int e = rocfft_make_plan(&h->planes.fwd, rocfft_transform_type_complex_forward, prec, rank, lengths, strides, nx * ny, strides, nx * ny,
                               (size_t)h->nz))
    return e;
  if (int e = rocfft_make_plan(&h->planes.inv, rocfft_transform_type_complex_inverse, prec, rank, lengths, strides, nx * ny, strides, nx * ny,
                               (size_t)h->nz))
    return e;
  return h->planes.create_info({h->planes.fwd, h->planes.inv});
}

template <class R>
static int fct_run(FCT *h, const void *in, void *out, int direction, bool withPlanes, void *stream, const char *who) {
  if (!h || !in || !out) { set_last_error("%s: null argument", who); return -1; }
  if (h->doublePrecision != (sizeof(R) == sizeof(double))) {
    set_last_error("%s: the handle was created for %s precision", who, h->doublePrecision ? "double" : "single");
    return -1;
  }
  if (in == out) { set_last_error("%s: the transform is out of place, in == out", who); return -1; }
  if (direction != UAMMD_FCT_FORWARD && direction != UAMMD_FCT_INVERSE) { set_last_error("%s: direction = %d", who, direction); return -1; }
  const int nk = h->nx * h->ny, n2 = 2 * (h->nz - 1);
  const bool forward = direction == UAMMD_FCT_FORWARD, planes = withPlanes && nk > 1;
  const R norm = (forward && planes) ? R(1) / R(nk) : R(1);
  const R *hi = (const R *)h->table.ptr;
  const dim3 grid((nk + 63) / 64, (h->nz + fct::kOut - 1) / fct::kOut);
  hipLaunchKernelGGL((k_cheb_z<R, sizeof(R) == sizeof(double)>), grid, dim3(64), 0, (hipStream_t)stream, (const Cplx<R> *)in,
                     (Cplx<R> *)out, nk, h->nz, hi, hi + n2, forward ? 1 : 0, norm);
  UH_CHECK(hipGetLastError());
  if (planes) {
    if (int e = h->planes.set_stream(stream)) return e;
    if (int e = h->planes.execute(forward ? h->planes.fwd : h->planes.inv, out)) return e;
  }
  return 0;
}

extern "C" {

int uammd_fct_create(int nx, int ny, int nz, int double_precision, uammd_fct **out) {
  if (!out) { set_last_error("uammd_fct_create: null argument"); return -1; }
  if (nx < 1 || ny < 1) { set_last_error("uammd_fct_create: nx = %d, ny = %d", nx, ny); return -2; }
  if (nz < 2) { set_last_error("uammd_fct_create: nz = %d: a Chebyshev grid has at least the two end planes (nz >= 2)", nz); return -2; }
  if ((long long)nx * ny > 0x7fffffffLL / nz) { set_last_error("uammd_fct_create: %d x %d x %d does not fit the index type", nx, ny, nz); return -2; }
  FCT *h = new (std::nothrow) FCT();
  if (!h) { set_last_error("uammd_fct_create: out of memory"); return -1; }
  h->nx = nx; h->ny = ny; h->nz = nz;
  h->doublePrecision = double_precision != 0;
  int e = h->doublePrecision ? fct_upload_table<double>(h) : fct_upload_table<float>(h);
  if (!e) e = fct_make_plans(h);
  if (e) { delete h; return e; }
  *out = reinterpret_cast<uammd_fct *>(h);
  return 0;
}

int uammd_fct_destroy(uammd_fct *h) {
  delete reinterpret_cast<FCT *>(h);
  return 0;
}

int uammd_fct_chebyshev(uammd_fct *h, const float *d_in, float *d_out, int direction, void *stream) {
  return fct_run<float>(reinterpret_cast<FCT *>(h), d_in, d_out, direction, false, stream, "uammd_fct_chebyshev");
}
int uammd_fct_chebyshev_f64(uammd_fct *h, const double *d_in, double *d_out, int direction, void *stream) {
  return fct_run<double>(reinterpret_cast<FCT *>(h), d_in, d_out, direction, false, stream, "uammd_fct_chebyshev_f64");
}
int uammd_fct_fourier_chebyshev(uammd_fct *h, const float *d_in, float *d_out, int direction, void *stream) {
  return fct_run<float>(reinterpret_cast<FCT *>(h), d_in, d_out, direction, true, stream, "uammd_fct_fourier_chebyshev");
}
int uammd_fct_fourier_chebyshev_f64(uammd_fct *h, const double *d_in, double *d_out, int direction, void *stream) {
  return fct_run<double>(reinterpret_cast<FCT *>(h), d_in, d_out, direction, true, stream, "uammd_fct_fourier_chebyshev_f64");
}

}  // extern "C"

}  // namespace uammd_hip
