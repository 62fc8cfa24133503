// Small linear algebra of the boundary value problem solver: the include path of the reference's
// src/misc/BoundaryValueProblem/MatrixUtils.h.  The dense inverse that header takes from LAPACK or Eigen has no counterpart here: the two
// rows of C A^-1 the solver needs come from two O(nz) eliminations on the host (uammd_amd/csrc/bvp_host.hpp).
#pragma once
// (thrust and device code: the contents need a translation unit compiled by hipcc; a plain C++ compiler sees an empty header)
#if defined(__HIPCC__)
#include "../../global/defines.h"
#include <thrust/pair.h>
namespace uammd {
namespace BVP {

// A x = b for a real 2 x 2 matrix A = (A.x A.y; A.z A.w) and two values of any type with T * real, T - T and T / real
template <class T> __host__ __device__ thrust::pair<T, T> solve2x2System(real4 A, thrust::pair<T, T> b) {
  const real det = A.x * A.w - A.y * A.z;
  return thrust::make_pair(T((b.first * A.w - b.second * A.y) / det), T((b.second * A.x - b.first * A.z) / det));
}
template <class T> __host__ __device__ thrust::pair<T, T> solve2x2System(real A[4], thrust::pair<T, T> b) {
  real4 m;
  m.x = A[0]; m.y = A[1]; m.z = A[2]; m.w = A[3];
  return solve2x2System(m, b);
}

}  // namespace BVP
}  // namespace uammd
#endif  // __HIPCC__
