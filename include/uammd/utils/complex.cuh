// utils/complex.cuh: the complex type of user code - thrust's, which device code can use (same include path and names as the
// reference's src/utils/complex.cuh).  Needs a translation unit compiled by hipcc, as thrust does.
#pragma once
// (thrust and device code: the contents need a translation unit compiled by hipcc; a plain C++ compiler sees an empty header)
#if defined(__HIPCC__)
#include "../global/defines.h"
#include <thrust/complex.h>
namespace uammd {
template <class T> using complex_t = thrust::complex<T>;
using complex = thrust::complex<real>;
}  // namespace uammd
#endif  // __HIPCC__
