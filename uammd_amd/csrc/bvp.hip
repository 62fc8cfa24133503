// Batched boundary value problem solver for gfx950 (misc/BoundaryValueProblem/BVPSolver.cuh:161-290 in the reference):
//   y'' - k^2 y = f on [-H, H] in Chebyshev space, one independent system per wave number, complex right-hand sides, real tables.
// The tables are computed on the host in double precision (bvp_host.hpp) and uploaded once per handle in the interleaved layout.
// One lane per (system, right-hand side): consecutive lanes take consecutive systems, so every table row is one coalesced load, and
// with the solvers' layout (sysStride = 1) so is every row of fn, an and cn.  No lane talks to another and nothing is reduced across
// lanes: a system's result does not depend on where in the batch it sits or on the batch's size.
#include "bvp_host.hpp"
#include "celllist.hpp"
#include "../../include/uammd/device/BVP.hip.hpp"

#include <new>

namespace uammd_hip {

struct BVPHandle {
  int nsys = 0, nz = 0;
  bool doublePrecision = false;
  DeviceBuffer tables;
  uammd::BVP::device::Tables<float> t32;
  uammd::BVP::device::Tables<double> t64;
};

template <class T> struct StridedRow {
  T *p;
  long long stride;
  __device__ T &operator[](int i) const { return p[(long long)i * stride]; }
};

template <class U, class T>
__global__ __launch_bounds__(64) void k_bvp_solve(uammd::BVP::device::Tables<U> t, const T *fn, const T *alpha, const T *beta, T *an,
                                                  T *cn, int nrhs, long long sysStride, long long coefStride, long long rhsStride) {
  const int s = blockIdx.x * 64 + threadIdx.x;
  const int r = blockIdx.y;
  if (s >= t.nsys || r >= nrhs) return;
  const long long base = (long long)r * rhsStride + (long long)s * sysStride;
  uammd::BVP::device::solveSystem(t, s, StridedRow<const T>{fn + base, coefStride}, alpha[(size_t)r * t.nsys + s],
                                  beta[(size_t)r * t.nsys + s], StridedRow<T>{an + base, coefStride}, StridedRow<T>{cn + base, coefStride});
}

template <class U> static int bvp_upload(BVPHandle *h, const bvp::HostTables &tab) {
  const size_t n = (size_t)tab.nsys, total = n * (5 * (size_t)tab.nz + 5);
  std::vector<U> host;
  host.reserve(total);
  for (const std::vector<double> *v : {&tab.beta, &tab.diagonal_p2, &tab.diagonal_m2, &tab.cinvA, &tab.m22, &tab.kH2})
    for (double x : *v) host.push_back((U)x);
  if (int e = h->tables.reserve(total * sizeof(U))) return e;
  UH_CHECK(hipMemcpy(h->tables.ptr, host.data(), total * sizeof(U), hipMemcpyHostToDevice));
  return 0;
}

template <class U, class T>
static int bvp_solve(BVPHandle *h, const uammd::BVP::device::Tables<U> &t, const void *fn, const void *alpha, const void *beta, void *an,
                     void *cn, int nrhs, long long sysStride, long long coefStride, void *stream, const char *who) {
  if (!h || !fn || !alpha || !beta || !an || !cn) { set_last_error("%s: null argument", who); return -1; }
  if (h->doublePrecision != (sizeof(U) == sizeof(double))) {
    set_last_error("%s: the handle was created for %s precision", who, h->doublePrecision ? "double" : "single");
    return -1;
  }
  if (nrhs < 1) { set_last_error("%s: nrhs = %d", who, nrhs); return -1; }
  if (fn == an || fn == cn || an == cn) { set_last_error("%s: fn, an and cn must be three different arrays", who); return -1; }
  // the two layouts in which the nsys x nz elements of one right-hand side tile a block without overlap
  const bool interleaved = sysStride == 1 && coefStride >= h->nsys, contiguous = coefStride == 1 && sysStride >= h->nz;
  if (!interleaved && !contiguous) {
    set_last_error("%s: strides (%lld, %lld) overlap for %d systems of %d coefficients", who, sysStride, coefStride, h->nsys, h->nz);
    return -1;
  }
  const long long rhsStride = interleaved ? coefStride * h->nz : sysStride * h->nsys;
  const dim3 grid((h->nsys + 63) / 64, nrhs);
  hipLaunchKernelGGL((k_bvp_solve<U, T>), grid, dim3(64), 0, (hipStream_t)stream, t, (const T *)fn, (const T *)alpha, (const T *)beta,
                     (T *)an, (T *)cn, nrhs, sysStride, coefStride, rhsStride);
  UH_CHECK(hipGetLastError());
  return 0;
}

extern "C" {

int uammd_bvp_create(int nsys, int nz, double H, const double *k, const double *tfi, const double *tsi, const double *bfi,
                     const double *bsi, int double_precision, uammd_bvp **out) {
  if (!out || !k || !tfi || !tsi || !bfi || !bsi) { set_last_error("uammd_bvp_create: null argument"); return -1; }
  bvp::HostTables tab;
  std::string err;
  if (int e = bvp::precompute(nsys, nz, H, k, tfi, tsi, bfi, bsi, tab, err)) {
    set_last_error("uammd_bvp_create: %s", err.c_str());
    return e;
  }
  BVPHandle *h = new (std::nothrow) BVPHandle();
  if (!h) { set_last_error("uammd_bvp_create: out of memory"); return -1; }
  h->nsys = nsys;
  h->nz = nz;
  h->doublePrecision = double_precision != 0;
  if (int e = h->doublePrecision ? bvp_upload<double>(h, tab) : bvp_upload<float>(h, tab)) { delete h; return e; }
  if (h->doublePrecision) h->t64 = uammd::BVP::device::Tables<double>::over((const double *)h->tables.ptr, nsys, nz, H * H);
  else h->t32 = uammd::BVP::device::Tables<float>::over((const float *)h->tables.ptr, nsys, nz, (float)(H * H));
  *out = reinterpret_cast<uammd_bvp *>(h);
  return 0;
}

int uammd_bvp_destroy(uammd_bvp *h) {
  delete reinterpret_cast<BVPHandle *>(h);
  return 0;
}

int uammd_bvp_device_tables(uammd_bvp *h_, uammd_bvp_tables *out) {
  BVPHandle *h = reinterpret_cast<BVPHandle *>(h_);
  if (!h || !out) { set_last_error("uammd_bvp_device_tables: null argument"); return -1; }
  out->d_tables = h->tables.ptr;
  out->nsys = h->nsys;
  out->nz = h->nz;
  out->double_precision = h->doublePrecision;
  return 0;
}

int uammd_bvp_solve(uammd_bvp *h, const float *d_fn, const float *d_alpha, const float *d_beta, float *d_an, float *d_cn, int nrhs,
                    long long sysStride, long long coefStride, void *stream) {
  BVPHandle *b = reinterpret_cast<BVPHandle *>(h);
  if (!b) { set_last_error("uammd_bvp_solve: null argument"); return -1; }
  return bvp_solve<float, float2>(b, b->t32, d_fn, d_alpha, d_beta, d_an, d_cn, nrhs, sysStride, coefStride, stream, "uammd_bvp_solve");
}

int uammd_bvp_solve_f64(uammd_bvp *h, const double *d_fn, const double *d_alpha, const double *d_beta, double *d_an, double *d_cn, int nrhs,
                        long long sysStride, long long coefStride, void *stream) {
  BVPHandle *b = reinterpret_cast<BVPHandle *>(h);
  if (!b) { set_last_error("uammd_bvp_solve_f64: null argument"); return -1; }
  return bvp_solve<double, double2>(b, b->t64, d_fn, d_alpha, d_beta, d_an, d_cn, nrhs, sysStride, coefStride, stream,
                                    "uammd_bvp_solve_f64");
}

}  // extern "C"

}  // namespace uammd_hip
