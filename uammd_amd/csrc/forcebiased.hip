// Force biased Monte Carlo for gfx950 (Integrator/MonteCarlo/ForceBiased.cuh): the Metropolized Euler-Maruyama scheme (MALA) of
// Bou-Rabee and Vanden-Eijnden, the integrator's own part of a trial.  The forces and energies come from the caller's interactors.
//
//   begin    X = pos, F(X) = force, E_X = sum_i energy[i]                                            (ForceBiased.cuh:211-218)
//   propose  xi = (gf(0,1).x, gf(0,1).y, gf(0,1).x) from Saru(seed, step, i);  pos = X + (h F(X) + sqrt(2 h / beta) xi)   (:56-72)
//   decide   E_Y = sum_i energy[i],  T_XY = sum |Y - X - h F(X)|^2 / (4 h),  T_YX = sum |X - Y - h F(Y)|^2 / (4 h)      (:75-86, :311-324)
//            accept if Z < exp(-beta ((E_Y - E_X) + (T_YX - T_XY)))                                 (:235-262)
//            accepted: stored <- (pos, force), E_X <- E_Y;  rejected: (pos, force) <- stored        (:264-278)
//
// Shape.  The reference spends four reductions with a host read each, four full-array copies and two fills per trial; at
// the sizes this sampler is used the launches and synchronisations are the cost.  Here a trial is three kernels of the integrator's own:
//   k_fb_propose reads the STORED arrays, so a rejected trial needs no restore pass before the next proposal;
//   k_fb_reduce  forms the three sums in one pass (terms and sums in double), wave shuffle -> LDS -> one triple per block, plain stores;
//   k_fb_commit  every block adds the (at most kMaxPartials) triples in the same fixed order in its prologue, so every block knows the
//                decision without a hand-off between workgroups, block 0 writes the record, and each block moves its slice.
// and one host synchronisation (uammd_mc_forcebiased_result).  No atomics: the same inputs give the same bits on every run.
// E_X lives in a pair of slots that the host alternates between: a commit reads one and writes the other, so no block can read the
// energy that block 0 has already replaced.
#include "device_common.hpp"
#include "saru.hpp"
#include "celllist.hpp"

#include <cfloat>
#include <new>

namespace uammd_hip {

namespace fb {
constexpr int kBlock = 256;
constexpr int kMaxPartials = 256;  // the commit's prologue reads 3 x this many doubles at most, one triple per thread
constexpr int kRecord = 8;         // E_X before, E_Y, T_XY, T_YX, exponent, current energy, accepted, unused
}  // namespace fb

struct MCForceBiased {
  DeviceBuffer storedPos, storedForce, partial, state;  // state: double eX[2], double record[kRecord]
  double *hostRecord = nullptr;                          // pinned mirror of the record
  int N = 0;       // the size adopted by begin (0: nothing adopted)
  int cur = 0;     // the slot of eX that holds the stored energy
  ~MCForceBiased() {
    if (hostRecord) (void)hipHostFree(hostRecord);
  }
};

// The totals of v[0..2] over the workgroup, to every thread: shuffle ladder inside a wave, the four waves through LDS, added in wave order.
UH_D void fb_block_sum3(double v[3], double (*sh)[4]) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    double x = v[c];
    for (int off = 32; off > 0; off >>= 1) x += __shfl_down(x, off);
    if (lane == 0) sh[c][wv] = x;
  }
  __syncthreads();
#pragma unroll
  for (int c = 0; c < 3; ++c) v[c] = ((sh[c][0] + sh[c][1]) + sh[c][2]) + sh[c][3];
}

UH_D double fb_sq3(double a, double b, double c) { return (a * a + b * b) + c * c; }

// one triple (sum energy, sum |Y - X - h F(X)|^2, sum |X - Y - h F(Y)|^2) per block; ENERGY_ONLY: the first alone (begin)
template <bool ENERGY_ONLY>
__global__ void __launch_bounds__(fb::kBlock) k_fb_reduce(const float4 *__restrict__ X, const float4 *__restrict__ Y, const float4 *__restrict__ FX,
                                                          const float4 *__restrict__ FY, const float *__restrict__ energy, int n, double h,
                                                          double *__restrict__ partial) {
  __shared__ double sh[3][4];
  double v[3] = {0.0, 0.0, 0.0};
  for (int i = (int)blockIdx.x * fb::kBlock + (int)threadIdx.x; i < n; i += (int)gridDim.x * fb::kBlock) {
    v[0] += (double)energy[i];
    if (!ENERGY_ONLY) {
      const float4 x = X[i], y = Y[i], fx = FX[i], fy = FY[i];
      v[1] += fb_sq3(((double)y.x - (double)x.x) - h * (double)fx.x, ((double)y.y - (double)x.y) - h * (double)fx.y,
                     ((double)y.z - (double)x.z) - h * (double)fx.z);
      v[2] += fb_sq3(((double)x.x - (double)y.x) - h * (double)fy.x, ((double)x.y - (double)y.y) - h * (double)fy.y,
                     ((double)x.z - (double)y.z) - h * (double)fy.z);
    }
  }
  fb_block_sum3(v, sh);
  if (threadIdx.x == 0) {
    partial[3 * blockIdx.x + 0] = v[0];
    partial[3 * blockIdx.x + 1] = v[1];
    partial[3 * blockIdx.x + 2] = v[2];
  }
}

// the block's copy of the totals of the partial triples (nparts <= kMaxPartials = the block size)
UH_D void fb_total(const double *__restrict__ partial, int nparts, double v[3], double (*sh)[4]) {
  const int k = threadIdx.x;
  v[0] = v[1] = v[2] = 0.0;
  if (k < nparts) {
    v[0] = partial[3 * k + 0];
    v[1] = partial[3 * k + 1];
    v[2] = partial[3 * k + 2];
  }
  fb_block_sum3(v, sh);
}

// an energy that is not finite, or past the range of real, becomes the largest real (ForceBiased.cuh:347-351)
UH_D double fb_energy(double e) { return fabs(e) <= (double)FLT_MAX ? e : (double)FLT_MAX; }

__global__ void __launch_bounds__(fb::kBlock) k_fb_begin(const double *__restrict__ partial, int nparts, double *__restrict__ eX,
                                                         double *__restrict__ rec) {
  __shared__ double sh[3][4];
  double v[3];
  fb_total(partial, nparts, v, sh);
  if (threadIdx.x == 0) {
    const double e = fb_energy(v[0]);
    *eX = e;
    rec[0] = e; rec[1] = e; rec[2] = 0.0; rec[3] = 0.0; rec[4] = 0.0; rec[5] = e; rec[6] = 1.0; rec[7] = 0.0;
  }
}

__global__ void __launch_bounds__(fb::kBlock) k_fb_commit(float4 *__restrict__ pos, float4 *__restrict__ force, float4 *__restrict__ sPos,
                                                          float4 *__restrict__ sForce, int n, const double *__restrict__ partial, int nparts,
                                                          double h, double beta, double Z, const double *__restrict__ eXin,
                                                          double *__restrict__ eXout, double *__restrict__ rec) {
  __shared__ double sh[3][4];
  double v[3];
  fb_total(partial, nparts, v, sh);
  const double EX = *eXin;
  const double EY = fb_energy(v[0]);
  const double TXY = v[1] / (4.0 * h), TYX = v[2] / (4.0 * h);
  const double exponent = -beta * ((EY - EX) + (TYX - TXY));
  const bool accept = Z < exp(exponent);  // a NaN compares false: rejected
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    const double now = accept ? EY : EX;
    *eXout = now;
    rec[0] = EX; rec[1] = EY; rec[2] = TXY; rec[3] = TYX; rec[4] = exponent; rec[5] = now; rec[6] = accept ? 1.0 : 0.0; rec[7] = 0.0;
  }
  for (int i = (int)blockIdx.x * fb::kBlock + (int)threadIdx.x; i < n; i += (int)gridDim.x * fb::kBlock) {
    if (accept) {
      sPos[i] = pos[i];
      sForce[i] = force[i];
    } else {
      pos[i] = sPos[i];
      force[i] = sForce[i];
    }
  }
}

__global__ void __launch_bounds__(fb::kBlock) k_fb_propose(const float4 *__restrict__ sPos, const float4 *__restrict__ sForce,
                                                           float4 *__restrict__ pos, float4 *__restrict__ noise, int n, float h, float amp,
                                                           uint seed, uint step) {
  const int i = (int)blockIdx.x * fb::kBlock + (int)threadIdx.x;
  if (i >= n) return;
  Saru rng(seed, step, (uint)i);
  const float2 a = rng.gf(0.0f, 1.0f);
  const float c = rng.gf(0.0f, 1.0f).x;
  const float4 x = sPos[i], f = sForce[i];
  if (noise) noise[i] = make_float4(a.x, a.y, c, 0.0f);
  pos[i] = make_float4(x.x + (f.x * h + amp * a.x), x.y + (f.y * h + amp * a.y), x.z + (f.z * h + amp * c), x.w);
}

static int fb_blocks(int n) {
  const int b = (n + fb::kBlock - 1) / fb::kBlock;
  return b < fb::kMaxPartials ? b : fb::kMaxPartials;
}

// what every call checks before anything touches the device
static int fb_check(const char *who, const MCForceBiased *h, int N, bool adopted) {
  if (N <= 0) { set_last_error("%s: numberParticles must be positive, got %d", who, N); return -1; }
  if (adopted && h->N != N) {
    set_last_error("%s: numberParticles is %d but uammd_mc_forcebiased_begin adopted %d", who, N, h->N);
    return -1;
  }
  return 0;
}
static int fb_check_step(const char *who, float stepSize, float beta) {
  if (!(stepSize > 0.0f)) { set_last_error("%s: stepSize must be positive, got %g", who, (double)stepSize); return -1; }
  if (!(beta >= 0.0f)) { set_last_error("%s: beta must not be negative, got %g", who, (double)beta); return -1; }
  return 0;
}

}  // namespace uammd_hip

using namespace uammd_hip;

extern "C" {

int uammd_mc_forcebiased_create(uammd_mc_forcebiased **out) {
  if (!out) { set_last_error("uammd_mc_forcebiased_create: null argument"); return -1; }
  MCForceBiased *h = new (std::nothrow) MCForceBiased();
  if (!h) { set_last_error("uammd_mc_forcebiased_create: out of memory"); return -1; }
  *out = reinterpret_cast<uammd_mc_forcebiased *>(h);
  return 0;
}

int uammd_mc_forcebiased_destroy(uammd_mc_forcebiased *h) {
  delete reinterpret_cast<MCForceBiased *>(h);
  return 0;
}

int uammd_mc_forcebiased_begin(uammd_mc_forcebiased *hh, const float *d_pos, const float *d_force, const float *d_energy, int numberParticles,
                               void *stream) {
  if (!hh || !d_pos || !d_force || !d_energy) { set_last_error("uammd_mc_forcebiased_begin: null argument"); return -1; }
  MCForceBiased *h = reinterpret_cast<MCForceBiased *>(hh);
  const int N = numberParticles;
  if (int e = fb_check("uammd_mc_forcebiased_begin", h, N, false)) return e;
  hipStream_t st = (hipStream_t)stream;
  h->N = 0;
  if (int e = h->storedPos.reserve(sizeof(float4) * (size_t)N)) return e;
  if (int e = h->storedForce.reserve(sizeof(float4) * (size_t)N)) return e;
  if (int e = h->partial.reserve(sizeof(double) * 3 * fb::kMaxPartials)) return e;
  if (int e = h->state.reserve(sizeof(double) * (2 + fb::kRecord))) return e;
  if (!h->hostRecord) UH_CHECK(hipHostMalloc((void **)&h->hostRecord, sizeof(double) * fb::kRecord, hipHostMallocDefault));
  UH_CHECK(hipMemcpyAsync(h->storedPos.ptr, d_pos, sizeof(float4) * (size_t)N, hipMemcpyDeviceToDevice, st));
  UH_CHECK(hipMemcpyAsync(h->storedForce.ptr, d_force, sizeof(float4) * (size_t)N, hipMemcpyDeviceToDevice, st));
  const int nb = fb_blocks(N);
  double *state = (double *)h->state.ptr;
  hipLaunchKernelGGL(k_fb_reduce<true>, dim3(nb), dim3(fb::kBlock), 0, st, (const float4 *)nullptr, (const float4 *)nullptr,
                     (const float4 *)nullptr, (const float4 *)nullptr, d_energy, N, 0.0, (double *)h->partial.ptr);
  h->cur = 0;
  hipLaunchKernelGGL(k_fb_begin, dim3(1), dim3(fb::kBlock), 0, st, (const double *)h->partial.ptr, nb, state + h->cur, state + 2);
  UH_CHECK(hipGetLastError());
  h->N = N;
  return 0;
}

int uammd_mc_forcebiased_propose(uammd_mc_forcebiased *hh, float *d_pos, int numberParticles, float stepSize, float beta, unsigned int step,
                                 unsigned int seed, float *d_noise, void *stream) {
  if (!hh || !d_pos) { set_last_error("uammd_mc_forcebiased_propose: null argument"); return -1; }
  MCForceBiased *h = reinterpret_cast<MCForceBiased *>(hh);
  const int N = numberParticles;
  if (int e = fb_check_step("uammd_mc_forcebiased_propose", stepSize, beta)) return e;
  if (int e = fb_check("uammd_mc_forcebiased_propose", h, N, true)) return e;
  const float amp = (float)std::sqrt(2.0 * (double)stepSize / (double)beta);  // EulerMaruyama's noiseAmp (ForceBiased.cuh:59-62)
  hipLaunchKernelGGL(k_fb_propose, dim3((N + fb::kBlock - 1) / fb::kBlock), dim3(fb::kBlock), 0, (hipStream_t)stream,
                     (const float4 *)h->storedPos.ptr, (const float4 *)h->storedForce.ptr, reinterpret_cast<float4 *>(d_pos),
                     reinterpret_cast<float4 *>(d_noise), N, stepSize, amp, seed, step);
  UH_CHECK(hipGetLastError());
  return 0;
}

int uammd_mc_forcebiased_decide(uammd_mc_forcebiased *hh, float *d_pos, float *d_force, const float *d_energy, int numberParticles,
                                float stepSize, float beta, double Z, void *stream) {
  if (!hh || !d_pos || !d_force || !d_energy) { set_last_error("uammd_mc_forcebiased_decide: null argument"); return -1; }
  MCForceBiased *h = reinterpret_cast<MCForceBiased *>(hh);
  const int N = numberParticles;
  if (int e = fb_check_step("uammd_mc_forcebiased_decide", stepSize, beta)) return e;
  if (int e = fb_check("uammd_mc_forcebiased_decide", h, N, true)) return e;
  hipStream_t st = (hipStream_t)stream;
  const int nb = fb_blocks(N);
  double *state = (double *)h->state.ptr, *partial = (double *)h->partial.ptr;
  float4 *pos = reinterpret_cast<float4 *>(d_pos), *force = reinterpret_cast<float4 *>(d_force);
  float4 *sPos = (float4 *)h->storedPos.ptr, *sForce = (float4 *)h->storedForce.ptr;
  hipLaunchKernelGGL(k_fb_reduce<false>, dim3(nb), dim3(fb::kBlock), 0, st, (const float4 *)sPos, (const float4 *)pos, (const float4 *)sForce,
                     (const float4 *)force, d_energy, N, (double)stepSize, partial);
  hipLaunchKernelGGL(k_fb_commit, dim3(nb), dim3(fb::kBlock), 0, st, pos, force, sPos, sForce, N, (const double *)partial, nb, (double)stepSize,
                     (double)beta, Z, (const double *)(state + h->cur), state + (h->cur ^ 1), state + 2);
  UH_CHECK(hipGetLastError());
  h->cur ^= 1;
  return 0;
}

int uammd_mc_forcebiased_result(uammd_mc_forcebiased *hh, int *accepted, double out[6], void *stream) {
  if (!hh || !accepted || !out) { set_last_error("uammd_mc_forcebiased_result: null argument"); return -1; }
  MCForceBiased *h = reinterpret_cast<MCForceBiased *>(hh);
  if (h->N <= 0) { set_last_error("uammd_mc_forcebiased_result: nothing adopted yet (uammd_mc_forcebiased_begin)"); return -1; }
  hipStream_t st = (hipStream_t)stream;
  UH_CHECK(hipMemcpyAsync(h->hostRecord, (const double *)h->state.ptr + 2, sizeof(double) * fb::kRecord, hipMemcpyDeviceToHost, st));
  UH_CHECK(hipStreamSynchronize(st));
  for (int k = 0; k < 6; ++k) out[k] = h->hostRecord[k];
  *accepted = h->hostRecord[6] != 0.0 ? 1 : 0;
  return 0;
}

int uammd_mc_forcebiased_stored(uammd_mc_forcebiased *hh, float *d_pos_out, float *d_force_out, void *stream) {
  if (!hh || !d_pos_out || !d_force_out) { set_last_error("uammd_mc_forcebiased_stored: null argument"); return -1; }
  MCForceBiased *h = reinterpret_cast<MCForceBiased *>(hh);
  if (h->N <= 0) { set_last_error("uammd_mc_forcebiased_stored: nothing adopted yet (uammd_mc_forcebiased_begin)"); return -1; }
  hipStream_t st = (hipStream_t)stream;
  UH_CHECK(hipMemcpyAsync(d_pos_out, h->storedPos.ptr, sizeof(float4) * (size_t)h->N, hipMemcpyDeviceToDevice, st));
  UH_CHECK(hipMemcpyAsync(d_force_out, h->storedForce.ptr, sizeof(float4) * (size_t)h->N, hipMemcpyDeviceToDevice, st));
  return 0;
}

}  // extern "C"
