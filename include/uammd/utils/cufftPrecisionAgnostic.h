// utils/cufftPrecisionAgnostic.h: the precision-agnostic names user code has for the FFT library's element types
// (cufftReal_t<T>, cufftComplex_t<T>; same include path as the reference's src/utils/cufftPrecisionAgnostic.h).  On this platform they
// are the runtime's own types: float / double and float2 / double2 (x = real part, y = imaginary part), which is what hipFFT and rocFFT
// take as interleaved complex.  The plan and execution wrappers of that header have no counterpart: the transforms of this build are
// entry points of libuammd_hip (uammd_hip.h).
#pragma once
#include "../global/defines.h"
namespace uammd {
namespace detail {
template <class T> struct FFTElementTypes;
template <> struct FFTElementTypes<float> { using real_type = float; using complex_type = ::float2; };
template <> struct FFTElementTypes<double> { using real_type = double; using complex_type = ::double2; };
}  // namespace detail
template <class T> using cufftReal_t = typename detail::FFTElementTypes<T>::real_type;
template <class T> using cufftComplex_t = typename detail::FFTElementTypes<T>::complex_type;
}  // namespace uammd
