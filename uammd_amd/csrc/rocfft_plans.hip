// The bodies of rocfft_plans.hpp.  Host code only: this file holds no kernel.
#include "rocfft_plans.hpp"

#include <algorithm>
#include <mutex>

namespace uammd_hip {

static std::once_flag g_rocfft_once;
int rocfft_setup_once() {
  std::call_once(g_rocfft_once, []() { (void)rocfft_setup(); });
  return 0;
}

int next_fft_wise(int n) {
  static const int primes[5] = {2, 3, 5, 7, 11}, maxExp[5] = {64, 64, 5, 4, 3};
  for (int c = std::max(n, 1);; ++c) {
    if (c % 2) continue;
    int m = c;
    bool ok = true;
    for (int p = 0; p < 5; ++p) {
      int e = 0;
      while (m % primes[p] == 0) { m /= primes[p]; ++e; }
      ok = ok && e <= maxExp[p];
    }
    if (ok && m == 1) return c;
  }
}

int rocfft_make_plan(rocfft_plan *plan, rocfft_transform_type type, rocfft_precision precision, size_t rank, const size_t *lengths,
                     const size_t *inStride, size_t inDistance, const size_t *outStride, size_t outDistance, size_t batch) {
  if (int e = rocfft_setup_once()) return e;
  rocfft_array_type in = rocfft_array_type_complex_interleaved, out = rocfft_array_type_complex_interleaved;
  if (type == rocfft_transform_type_real_forward) { in = rocfft_array_type_real; out = rocfft_array_type_hermitian_interleaved; }
  if (type == rocfft_transform_type_real_inverse) { in = rocfft_array_type_hermitian_interleaved; out = rocfft_array_type_real; }
  rocfft_plan_description d = nullptr;
  UH_ROCFFT(rocfft_plan_description_create(&d));
  const int e = [&]() -> int {
    UH_ROCFFT(rocfft_plan_description_set_data_layout(d, in, out, nullptr, nullptr, rank, inStride, inDistance, rank, outStride, outDistance));
    UH_ROCFFT(rocfft_plan_create(plan, rocfft_placement_inplace, type, precision, rank, lengths, batch, d));
    return 0;
  }();
  const rocfft_status destroyed = rocfft_plan_description_destroy(d);
  if (e) return e;
  UH_ROCFFT(destroyed);
  return 0;
}

int RealFFT::create(int rank, const int *cells, int nxpad, size_t planeReal, size_t planeCplx, rocfft_precision precision, size_t batchForward,
                    size_t batchInverse) {
  const size_t nx = cells[0], ny = cells[1], nz = rank == 3 ? cells[2] : 1, nkx = nx / 2 + 1;
  const size_t lengths[3] = {nx, ny, nz};
  const size_t rstr[3] = {1, (size_t)nxpad, (size_t)nxpad * ny}, cstr[3] = {1, nkx, nkx * ny};
  if (int e = rocfft_make_plan(&fwd, rocfft_transform_type_real_forward, precision, rank, lengths, rstr, planeReal, cstr, planeCplx, batchForward))
    return e;
  if (int e = rocfft_make_plan(&inv, rocfft_transform_type_real_inverse, precision, rank, lengths, cstr, planeCplx, rstr, planeReal, batchInverse))
    return e;
  return create_info({fwd, inv});
}

int RealFFT::create_info(std::initializer_list<rocfft_plan> plans) {
  workBytes = 0;
  for (rocfft_plan p : plans) {
    size_t w = 0;
    UH_ROCFFT(rocfft_plan_get_work_buffer_size(p, &w));
    workBytes = std::max(workBytes, w);
  }
  UH_ROCFFT(rocfft_execution_info_create(&info));
  if (workBytes) {
    if (int e = work.reserve(workBytes)) return e;
    UH_ROCFFT(rocfft_execution_info_set_work_buffer(info, work.ptr, workBytes));
  }
  return 0;
}

RealFFT::~RealFFT() {
  if (fwd) rocfft_plan_destroy(fwd);
  if (inv) rocfft_plan_destroy(inv);
  if (info) rocfft_execution_info_destroy(info);
}

}  // namespace uammd_hip
