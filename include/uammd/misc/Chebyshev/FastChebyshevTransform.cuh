// Transforms between values at the Chebyshev extrema and Chebyshev (or Fourier-Chebyshev) coefficients: the include path and names of the
// reference's src/misc/Chebyshev/FastChebyshevTransform.cuh, written for this build.  A hipcc header, like device/*.hip.hpp.
//
// The transforms themselves are entry points of libuammd_hip (uammd_fct_*, uammd_hip.h; uammd_amd/csrc/chebyshev.hip): the z pass takes the
// cosine sums directly on the nz planes and the plane transform is rocFFT.  No even extension is materialised on the way - but the
// containers these functions RETURN keep the reference's extent, nx ny (2 nz - 2), with planes nz ... 2 nz - 3 holding the even mirror
// (plane k equals plane 2 nz - 2 - k), which is what the FFT of an even signal leaves there and what callers index with.
// Element (i, j, k) sits at i + nx (j + ny k); plane k lies at cos(pi k / (nz - 1)).  real = double with -DDOUBLE_PRECISION.
#pragma once
// (thrust and device code: the contents need a translation unit compiled by hipcc; a plain C++ compiler sees an empty header)
#if defined(__HIPCC__)
#include "../../uammd.cuh"
#include "../../utils/complex.cuh"
#include "../../utils/cufftPrecisionAgnostic.h"
#include "../ChevyshevUtils.cuh"
#include <list>
#include <thrust/iterator/counting_iterator.h>
#include <thrust/iterator/permutation_iterator.h>
#include <thrust/iterator/transform_iterator.h>
#include <thrust/sequence.h>
#include <thrust/transform.h>

namespace uammd {
namespace chebyshev {
namespace detail {
// index of element z of signal `id` among `offset` interleaved signals
struct BatchedIteratorTransform {
  int id, offset;
  __host__ __device__ BatchedIteratorTransform(int id, int offset) : id(id), offset(offset) {}
  inline __host__ __device__ int operator()(int z) const { return id + offset * z; }
};
}  // namespace detail

// A view of signal `id` of `offset` interleaved signals (element k of signal id at id + k offset) in which its elements are consecutive.
template <class RandomAccessIterator> inline __host__ __device__ auto make_interleaved_iterator(RandomAccessIterator ptr, int id, int offset) {
  return thrust::make_permutation_iterator(ptr, thrust::make_transform_iterator(thrust::make_counting_iterator(0),
                                                                                detail::BatchedIteratorTransform(id, offset)));
}

namespace detail {

// plane k of n.x n.y n.z values, from the flat index
struct PlaneScale {
  int planeSize, nz;
  real inner, ends;   // factors of the planes 0 < k < nz - 1 and of the two end planes
  template <class T> __device__ T operator()(T v, int id) const {
    const int k = id / planeSize;
    return v * ((k == 0 || k == nz - 1) ? ends : inner);
  }
};

// FFT of the even extension -> Chebyshev coefficients: v pm_k / ((2 nz - 2) normalization), pm = 1 on the two end planes and 2 inside.
// Returns a new container.
template <class Container> auto scaleFFTToChebyshev(Container v, int3 n, real normalization) {
  const real base = real(1.0) / ((real(2.0) * n.z - real(2.0)) * normalization);
  thrust::transform(v.begin(), v.end(), thrust::make_counting_iterator(0), v.begin(), PlaneScale{n.x * n.y, n.z, real(2.0) * base, base});
  return v;
}

// Chebyshev coefficients -> the cosine-series coefficients the inverse FFT of the even extension takes: v / pm_k.  Returns a new container.
template <class Container> auto scaleChebyshevToiFFT(Container v, int3 n) {
  thrust::transform(v.begin(), v.end(), thrust::make_counting_iterator(0), v.begin(), PlaneScale{n.x * n.y, n.z, real(0.5), real(1.0)});
  return v;
}

// planes nz ... 2 nz - 3 of nk interleaved signals <- planes nz - 2 ... 1
template <class Iterator> __global__ void periodicExtendD(Iterator v, int nk, int nz) {
  const int id = blockIdx.x * blockDim.x + threadIdx.x;
  if (id >= nk) return;
  for (int z = nz; z < 2 * nz - 2; z++) v[id + (size_t)nk * z] = v[id + (size_t)nk * (2 * nz - 2 - z)];
}

// The even extension in z of nk interleaved signals of nz values, for any element type.  Returns a new container of nk (2 nz - 2) values.
template <class Container> auto periodicExtend(Container v, int nk, int nz) {
  v.resize((size_t)nk * (2 * nz - 2));
  if (nz > 2) {
    const int nthreads = 128;
    periodicExtendD<<<nk / nthreads + 1, nthreads>>>(thrust::raw_pointer_cast(v.data()), nk, nz);
    uammd::detail::hipCheck(hipGetLastError(), "periodicExtend");
  }
  return v;
}

// The library handle of a grid size, kept for the next call with that size: creating it builds the cosine table and, for nx ny > 1,
// two rocFFT plans, which costs far more than a transform of a small grid.  The most recent sizes are kept; the list is never torn
// down at exit (the runtime may be gone by then).
inline uammd_fct *transformHandle(int3 n) {
  struct Entry { int3 n; uammd_fct *h; };
  static std::list<Entry> *recent = new std::list<Entry>();
  constexpr size_t kept = 32;
  for (auto it = recent->begin(); it != recent->end(); ++it)
    if (it->n.x == n.x && it->n.y == n.y && it->n.z == n.z) {
      recent->splice(recent->begin(), *recent, it);
      return recent->front().h;
    }
  uammd_fct *h = nullptr;
#if defined(DOUBLE_PRECISION)
  uammd::detail::check(uammd_fct_create(n.x, n.y, n.z, 1, &h));
#else
  uammd::detail::check(uammd_fct_create(n.x, n.y, n.z, 0, &h));
#endif
  recent->push_front(Entry{n, h});
  if (recent->size() > kept) {
    uammd::detail::hipCheck(hipDeviceSynchronize(), "transformHandle");
    uammd_fct_destroy(recent->back().h);
    recent->pop_back();
  }
  return h;
}

// in (at least nx ny nz values) -> a new container of nx ny (2 nz - 2) values: the transform in planes 0 ... nz - 1, their mirror above
template <class Container> Container transform(const Container &in, int3 n, bool planes, int direction) {
  static_assert(sizeof(typename Container::value_type) == 2 * sizeof(real), "the transforms take complex values of the build's precision");
  const size_t nk = (size_t)n.x * n.y;
  if (n.z < 2 || in.size() < nk * n.z) throw std::runtime_error("[FastChebyshevTransform] the input holds fewer than nx ny nz values (nz >= 2)");
  Container out(nk * (n.z > 2 ? 2 * n.z - 2 : 2));
  uammd_fct *h = transformHandle(n);
  const real *src = reinterpret_cast<const real *>(thrust::raw_pointer_cast(in.data()));
  real *dst = reinterpret_cast<real *>(thrust::raw_pointer_cast(out.data()));
#if defined(DOUBLE_PRECISION)
  uammd::detail::check(planes ? uammd_fct_fourier_chebyshev_f64(h, src, dst, direction, nullptr) : uammd_fct_chebyshev_f64(h, src, dst, direction, nullptr));
#else
  uammd::detail::check(planes ? uammd_fct_fourier_chebyshev(h, src, dst, direction, nullptr) : uammd_fct_chebyshev(h, src, dst, direction, nullptr));
#endif
  if (n.z > 2) {
    const int nthreads = 128;
    periodicExtendD<<<(int)(nk / nthreads + 1), nthreads>>>(thrust::raw_pointer_cast(out.data()), (int)nk, n.z);
    uammd::detail::hipCheck(hipGetLastError(), "FastChebyshevTransform: mirror");
  }
  return out;
}

}  // namespace detail

// Values at the Chebyshev extrema in z, real space in the plane -> Chebyshev coefficients in z for each wave number of the plane
// (forward plane transform divided by nx ny).
template <class Container> auto fourierChebyshevTransform3DCufft(Container i_fx, int3 n) { return detail::transform(i_fx, n, true, UAMMD_FCT_FORWARD); }

// One signal sampled at its size() Chebyshev extrema -> its Chebyshev coefficients.
template <class Container> auto chebyshevTransform1DCufft(Container fx) {
  const int nz = fx.size();
  return fourierChebyshevTransform3DCufft(fx, make_int3(1, 1, nz));
}

// The inverse of fourierChebyshevTransform3DCufft (the plane transform is not normalised).
template <class Container> auto inverseFourierChebyshevTransform3DCufft(Container fn, int3 n) { return detail::transform(fn, n, true, UAMMD_FCT_INVERSE); }

// nz Chebyshev coefficients -> the signal at the Chebyshev extrema.
template <class Container> auto inverseChebyshevTransform1DCufft(Container fn, int nz) {
  return inverseFourierChebyshevTransform3DCufft(fn, make_int3(1, 1, nz));
}

// nx ny interleaved signals sampled at the Chebyshev extrema -> the Chebyshev coefficients of each (no plane transform).
template <class Container> auto chebyshevTransform3DCufft(Container fx, int3 n) { return detail::transform(fx, n, false, UAMMD_FCT_FORWARD); }

// The inverse of chebyshevTransform3DCufft.
template <class Container> auto inverseChebyshevTransform3DCufft(Container fn, int3 n) { return detail::transform(fn, n, false, UAMMD_FCT_INVERSE); }

}  // namespace chebyshev
}  // namespace uammd
#endif  // __HIPCC__
