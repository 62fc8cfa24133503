// The rocFFT host plumbing of the spectral solvers (fcm.hip with its z-slab solver, fib.hip, icm.hip, quasi2d.hip, poisson.hip and their
// double-precision builds in f64.hip): the status check, the once-per-process set-up, the grid size rule, one function that builds one
// plan, and the forward / inverse pair of in-place real transforms with its work buffer that every handle holds.  Host code only; the
// bodies that are not inline live in rocfft_plans.hip.
#pragma once
#include "celllist.hpp"

#include <rocfft/rocfft.h>

#include <initializer_list>

namespace uammd_hip {

#define UH_ROCFFT(expr)                                                                      \
  do {                                                                                       \
    rocfft_status s_ = (expr);                                                               \
    if (s_ != rocfft_status_success) {                                                       \
      uammd_hip::set_last_error("%s failed with rocfft_status %d (%s:%d)", #expr, (int)s_, __FILE__, __LINE__); \
      return -10 - (int)s_;                                                                  \
    }                                                                                        \
  } while (0)

int rocfft_setup_once();  // rocfft_setup(), once per process

// nextFFTWiseSize3D (utils/Grid.cuh:142-213; restated in FIB.cu:31-84 and ICM.cu:29-84), one axis:
// smallest even 2^a 3^b 5^c 7^d 11^e >= n with c<=5, d<=4, e<=3
int next_fft_wise(int n);

// One in-place plan.  The array types follow from the transform type (real forward: real -> hermitian interleaved, real inverse the
// reverse, complex: complex interleaved both ways); the plan description is destroyed on every path.
int rocfft_make_plan(rocfft_plan *plan, rocfft_transform_type type, rocfft_precision precision, size_t rank, const size_t *lengths,
                     const size_t *inStride, size_t inDistance, const size_t *outStride, size_t outDistance, size_t batch);

// The padded layout that lets R2C / C2R run in place on a grid of `rank` (2 or 3) axes: rows of nxpad = 2 (nx/2 + 1) reals = nx/2 + 1
// complex numbers; planeReal reals = planeCplx complex numbers per component plane.
inline void fft_padded_layout(int rank, const int *cells, int *nxpad, size_t *planeReal, size_t *planeCplx) {
  *nxpad = 2 * (cells[0] / 2 + 1);
  *planeCplx = (size_t)(cells[0] / 2 + 1) * cells[1] * (rank == 3 ? cells[2] : 1);
  *planeReal = 2 * *planeCplx;
}

// Forward (R2C) and inverse (C2R) in-place transforms of component planes in the padded layout, and what executing them needs.
struct RealFFT {
  rocfft_plan fwd = nullptr, inv = nullptr;
  rocfft_execution_info info = nullptr;
  DeviceBuffer work;
  size_t workBytes = 0;
  // real strides {1, nxpad, nxpad ny} with distance planeReal, complex strides {1, nkx, nkx ny} with distance planeCplx
  int create(int rank, const int *cells, int nxpad, size_t planeReal, size_t planeCplx, rocfft_precision precision, size_t batchForward,
             size_t batchInverse);
  // the execution info, with a work buffer as large as the largest of `plans` wants (create() calls it for fwd and inv; the z-slab
  // solver for its own four plans)
  int create_info(std::initializer_list<rocfft_plan> plans);
  int set_stream(void *stream) {
    UH_ROCFFT(rocfft_execution_info_set_stream(info, stream));
    return 0;
  }
  int execute(rocfft_plan plan, void *grid) {
    void *bufs[1] = {grid};
    UH_ROCFFT(rocfft_execute(plan, bufs, nullptr, info));
    return 0;
  }
  int forward(void *grid) { return execute(fwd, grid); }
  int inverse(void *grid) { return execute(inv, grid); }
  ~RealFFT();
};

}  // namespace uammd_hip
