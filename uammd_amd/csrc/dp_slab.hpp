// What the two doubly periodic solvers share on a Chebyshev slab grid (dppoisson.hip, dpstokes.hip), templated on the
// grid type of cheb_grid.hpp, which brings the window: the classification of a particle, the gather, the atomic spread, the tile
// geometry and particle scan of the owner-computes spread, the small vector and complex helpers, and the host plumbing of a handle
// (uploads, the transform dispatch, the stage timer).  The host tables are in dp_slab_host.hpp, which has no HIP in it.
//
// A particle's record is T4 (folded x, folded y, z, and a fourth value of the solver's) with an int4 (first window node in x, in y,
// flags, 0); flag dp::kOutside marks a particle that is never spread or gathered.
#pragma once
#include "celllist.hpp"
#include "cheb_grid.hpp"
#include "dp_slab_host.hpp"

#include <algorithm>
#include <vector>

namespace uammd_hip {

template <class U> struct VecOf;
template <> struct VecOf<float> { using T2 = float2; using T4 = float4; };
template <> struct VecOf<double> { using T2 = double2; using T4 = double4; };

namespace dp {
constexpr int kOutside = 8;      // cellrec.z: |z| > H/2 or a non-finite coordinate
constexpr int kMaxSupport = 16;  // the gather keeps ceil(support^2 / 64) <= 4 columns per lane
constexpr int kTile = 8;         // the owner spread's block: kTile x kTile nodes x kTile planes per wave
}  // namespace dp

template <class U> UH_D U bcast(U v, int lane) { return __shfl(v, lane, 64); }

template <class T> struct Row {  // one wave number's column of a field stored wave number fastest
  T *p;
  size_t stride;
  __device__ T &operator[](int i) const { return p[(size_t)i * stride]; }
};

struct cd2 { double x, y; };  // the corrections are evaluated in double in either build
UH_D cd2 operator+(cd2 a, cd2 b) { return {a.x + b.x, a.y + b.y}; }
UH_D cd2 operator-(cd2 a, cd2 b) { return {a.x - b.x, a.y - b.y}; }
UH_D cd2 operator-(cd2 a) { return {-a.x, -a.y}; }
UH_D cd2 operator*(cd2 a, double s) { return {a.x * s, a.y * s}; }
UH_D cd2 operator*(double s, cd2 a) { return {a.x * s, a.y * s}; }
UH_D cd2 operator/(cd2 a, double s) { return {a.x / s, a.y / s}; }
UH_D cd2 cmul(cd2 a, cd2 b) { return {a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x}; }
UH_D cd2 times_i(cd2 a) { return {-a.y, a.x}; }
UH_D cd2 times_minus_i(cd2 a) { return {a.y, -a.x}; }

// Two real fields packed in one complex spectrum G, wave number s and its mirror sm: Chebyshev coefficient n of the spectrum of the real
// part (c = 0), A(k) = (G(k) + conj G(-k)) / 2, or of the imaginary part (c = 1), B(k) = (G(k) - conj G(-k)) / (2 i)
template <class U> UH_D typename VecOf<U>::T2 dp_hermitian_part(const typename VecOf<U>::T2 *g, size_t nsys, int s, int sm, int n, int c) {
  const typename VecOf<U>::T2 a = g[s + nsys * n], b = g[sm + nsys * n];
  typename VecOf<U>::T2 f;
  if (c == 1) {
    f.x = U(0.5) * (a.y + b.y);
    f.y = -(U(0.5) * (a.x - b.x));
  } else {
    f.x = U(0.5) * (a.x + b.x);
    f.y = U(0.5) * (a.y - b.y);
  }
  return f;
}

// ---- classification ----------------------------------------------------------------------------------------------------------------
// false: a coordinate is not finite or |z| > half, and r, c are left alone; else the folded coordinates and the window's first nodes
template <class U, class Grid> UH_D bool dp_place(const Grid &g, U x, U y, U z, U half, typename VecOf<U>::T4 &r, int4 &c) {
  const bool finite = (x - x == U(0)) && (y - y == U(0)) && (z - z == U(0));
  if (!finite || !(abs_(z) <= half)) return false;
  r.x = Grid::fold(x, g.Lx);
  r.y = Grid::fold(y, g.Ly);
  r.z = z;
  c.x = g.leftmost_x(r.x);
  c.y = g.leftmost_y(r.y);
  return true;
}

// ---- gather: a wave per particle, lanes over the x-y footprint, a loop over the planes ---------------------------------------------
// NC of the four real fields packed as (u.x, u.y) in uv and (v.x, v.y) in wp are summed with the window and the quadrature weights;
// lane 0 hands the sums to Sink::write(a, r, sums, out...), and every lane of an outside particle's wave calls
// Sink::outside(a, lane, out...).  The sink has no state: the output arrays are kernel arguments, so that they stay __restrict__ and the
// plane heights and weights, which no store can then clobber, stay scalar loads.
template <class U, class Grid, int NC, class Sink, class... Out>
__global__ __launch_bounds__(256) void k_dp_gather(const typename VecOf<U>::T4 *__restrict__ rec, const int4 *__restrict__ cellrec, int N, Grid g,
                                                   const typename VecOf<U>::T2 *__restrict__ uv, const typename VecOf<U>::T2 *__restrict__ wp,
                                                   Out *__restrict__... out) {
  using T2 = typename VecOf<U>::T2;
  const int lane = threadIdx.x & 63;
  const int a = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (a >= N) return;
  const int4 c = cellrec[a];
  if (c.z & dp::kOutside) {
    Sink::outside(a, lane, out...);
    return;
  }
  const typename VecOf<U>::T4 r = rec[a];
  const int s = g.support, cols = s * s;
  constexpr int G = (dp::kMaxSupport * dp::kMaxSupport + 63) / 64;
  U wxy[G];
  size_t node[G];
#pragma unroll
  for (int q = 0; q < G; ++q) {
    const int col = lane + 64 * q;
    wxy[q] = U(0);
    node[q] = 0;
    if (col < cols) {
      const int jj = col / s, ii = col - jj * s;
      const int i = Grid::wrap(c.x + ii, g.nx), j = Grid::wrap(c.y + jj, g.ny);
      wxy[q] = g.weight_x(r.x, i) * g.weight_y(r.y, j);
      node[q] = (size_t)j * g.nx + i;
    }
  }
  int lo, hi;
  g.plane_range(r.z, lo, hi);
  lo = __builtin_amdgcn_readfirstlane(lo);
  hi = __builtin_amdgcn_readfirstlane(hi);
  const size_t plane = (size_t)g.nx * g.ny;
  U acc[NC];
#pragma unroll
  for (int m = 0; m < NC; ++m) acc[m] = U(0);
  for (int k = lo; k <= hi; ++k) {
    const U wz = g.weight_z(r.z, g.zplane[k]) * g.qw[k];  // the quadrature weight folded in
    if (wz == U(0)) continue;
#pragma unroll
    for (int q = 0; q < G; ++q) {
      if (64 * q < cols) {  // (wave-uniform)
        const T2 u = uv[node[q] + plane * (size_t)k], v = wp[node[q] + plane * (size_t)k];
        const U w = wxy[q] * wz;
        const U value[4] = {u.x, u.y, v.x, v.y};
#pragma unroll
        for (int m = 0; m < NC; ++m) acc[m] += w * value[m];
      }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
    for (int m = 0; m < NC; ++m) acc[m] += __shfl_xor(acc[m], o, 64);
  }
  if (lane != 0) return;
  Sink::write(a, r, acc, out...);
}

// ---- the plain spread (the cross-check): a lane per particle, atomic adds into zeroed grids -----------------------------------------
template <class U, int K> struct DpSource {  // one source of a particle
  bool on;
  U zs, amplitude[K];
  int grid[K], comp[K];
};
// Source::get(n, a, r, flags) is source n < Source::kSources of particle a, a DpSource: whether it is on, its height zs, and kAmplitudes
// amplitudes, amplitude m added to real component comp[m] of complex grid grid[m] (out0 or out1).
template <class U, class Grid, class Source>
__global__ __launch_bounds__(64) void k_dp_spread_simple(const typename VecOf<U>::T4 *__restrict__ rec, const int4 *__restrict__ cellrec, int N,
                                                         Grid g, Source source, U *__restrict__ out0, U *__restrict__ out1) {
  const int a = blockIdx.x * 64 + threadIdx.x;
  if (a >= N) return;
  const int4 c = cellrec[a];
  if (c.z & dp::kOutside) return;
  const typename VecOf<U>::T4 r = rec[a];
  const size_t plane = (size_t)g.nx * g.ny;
  for (int n = 0; n < Source::kSources; ++n) {
    const auto src = source.get(n, a, r, c.z);
    if (!src.on) continue;
    int lo, hi;
    g.plane_range(src.zs, lo, hi);
    for (int k = lo; k <= hi; ++k) {
      const U wz = g.weight_z(src.zs, g.zplane[k]);
      if (wz == U(0)) continue;
      for (int jj = 0; jj < g.support; ++jj) {
        const int j = Grid::wrap(c.y + jj, g.ny);
        const U wy = g.weight_y(r.y, j);
        for (int ii = 0; ii < g.support; ++ii) {
          const int i = Grid::wrap(c.x + ii, g.nx);
          const U w = (g.weight_x(r.x, i) * wy) * wz;
          if (w == U(0)) continue;
          const size_t at = 2 * ((size_t)j * g.nx + i + plane * (size_t)k);
#pragma unroll
          for (int m = 0; m < Source::kAmplitudes; ++m) unsafeAtomicAdd(&(src.grid[m] ? out1 : out0)[at + src.comp[m]], w * src.amplitude[m]);
        }
      }
    }
  }
}

// ---- the owner-computes spread: what a wave knows about its tile, and its scan of the particles --------------------------------------
UH_D bool dp_ring_overlap(int first, int width, int tile0, int n) {  // [first, first + width) against [tile0, tile0 + kTile) mod n
  int d = tile0 - first;
  d = d < 0 ? d + n : (d >= n ? d - n : d);
  return d < width || n - d < dp::kTile;
}

// A wave owns kTile x kTile nodes x kTile planes: lane l the node column (tx0 + l % 8, ty0 + l / 8) over planes p0 ... p0 + 7.  Launched
// over dp_owner_grid with 64 lanes.
template <class U, class Grid> struct DpTile {
  static constexpr int T = dp::kTile;
  int lane, tx0, ty0, p0, ni, nj, last;
  bool nodeOK, planeOK;    // my node lies on the grid; plane p0 + lane % 8 does
  U zTop, zBottom, zMine;  // the tile's planes span [zBottom, zTop]; zMine the height of plane p0 + lane % 8 (clamped)

  UH_D explicit DpTile(const Grid &g) {
    lane = threadIdx.x;
    const int tilesX = (g.nx + T - 1) / T;
    tx0 = (int)(blockIdx.x % tilesX) * T, ty0 = (int)(blockIdx.x / tilesX) * T, p0 = (int)blockIdx.y * T;
    ni = tx0 + (lane & (T - 1)), nj = ty0 + (lane >> 3);
    nodeOK = ni < g.nx && nj < g.ny;
    last = g.nz - 1;
    zTop = g.zplane[p0], zBottom = g.zplane[min(p0 + T - 1, last)];
    zMine = g.zplane[min(p0 + (lane & (T - 1)), last)];
    planeOK = p0 + (lane & (T - 1)) <= last;
  }
  UH_D bool touches_z(const Grid &g, U zs) const { return zs - g.reach_z() <= zTop && zs + g.reach_z() >= zBottom; }
  UH_D bool touches_xy(const Grid &g, const int4 &c) const {
    return dp_ring_overlap(c.x, g.support, tx0, g.nx) && dp_ring_overlap(c.y, g.support, ty0, g.ny);
  }
  // the x-y weight my node takes from a particle at (px, py) whose window starts at node (x0, y0)
  UH_D U wxy(const Grid &g, U px, U py, int x0, int y0) const {
    const int ii = Grid::wrap(ni - x0, g.nx), jj = Grid::wrap(nj - y0, g.ny);
    U w = U(0);
    if (nodeOK && ii < g.support && jj < g.support) w = g.weight_x(px, ni) * g.weight_y(py, nj);
    return w;
  }
  // The particles 64 at a time: load(a) brings particle a into the lane's own registers and says whether it touches this tile (false
  // for a >= N); add(l) then runs for every hit of the batch in index order, wave-uniform, and reads lane l's registers by bcast.
  template <class Load, class Add> UH_D void scan(int N, Load load, Add add) const {
    for (int base = 0; base < N; base += 64) {
      unsigned long long m = __ballot(load(base + lane));
      while (m) {
        const int l = __builtin_ctzll(m);
        m &= m - 1;
        add(l);
      }
    }
  }
  UH_D bool has_plane(int p) const { return p0 + p <= last; }
  UH_D size_t at(const Grid &g, int p) const { return (size_t)nj * g.nx + ni + (size_t)g.nx * g.ny * (size_t)(p0 + p); }  // my node on plane p0 + p
};

inline dim3 dp_owner_grid(int nx, int ny, int nz) {
  constexpr int T = dp::kTile;
  return dim3(((nx + T - 1) / T) * ((ny + T - 1) / T), (nz + T - 1) / T);
}

// ---- host plumbing of a handle --------------------------------------------------------------------------------------------------------
template <class U> static int upload(DeviceBuffer &b, const std::vector<double> &v) {
  std::vector<U> tmp(v.begin(), v.end());
  if (int e = b.reserve(std::max<size_t>(tmp.size(), 1) * sizeof(U))) return e;
  if (!tmp.empty()) UH_CHECK(hipMemcpy(b.ptr, tmp.data(), tmp.size() * sizeof(U), hipMemcpyHostToDevice));
  return 0;
}

// the Fourier-Chebyshev transform of the planes and columns (planes) or the Chebyshev transform of the columns alone, in U
template <class U>
static int fct_run(uammd_fct *fct, bool planes, const typename VecOf<U>::T2 *in, typename VecOf<U>::T2 *out, int dir, hipStream_t st) {
  if (sizeof(U) == sizeof(double))
    return planes ? uammd_fct_fourier_chebyshev_f64(fct, (const double *)in, (double *)out, dir, st)
                  : uammd_fct_chebyshev_f64(fct, (const double *)in, (double *)out, dir, st);
  return planes ? uammd_fct_fourier_chebyshev(fct, (const float *)in, (float *)out, dir, st)
                : uammd_fct_chebyshev(fct, (const float *)in, (float *)out, dir, st);
}

static int dp_check_precision(bool handleDouble, bool wantDouble, const char *who) {
  if (handleDouble == wantDouble) return 0;
  set_last_error("%s: the handle was created for %s precision", who, handleDouble ? "double" : "single");
  return -1;
}

// Option time_stages: device events between the N stage launches of a run.  Nothing is recorded, created or waited for unless enabled.
template <int N> struct StageTimer {
  hipEvent_t event[N + 1] = {};
  int marks = 0;
  bool enabled = false;
  StageTimer() = default;
  StageTimer(const StageTimer &) = delete;
  StageTimer &operator=(const StageTimer &) = delete;
  ~StageTimer() {
    for (hipEvent_t e : event)
      if (e) (void)hipEventDestroy(e);
  }
  void enable(bool on) { enabled = on; marks = 0; }
  void reset() { marks = 0; }
  int mark(hipStream_t st) {  // one event after every stage (and one before the first)
    if (!enabled) return 0;
    hipEvent_t &e = event[marks];
    if (!e) UH_CHECK(hipEventCreate(&e));
    UH_CHECK(hipEventRecord(e, st));
    ++marks;
    return 0;
  }
  // milliseconds each stage of the last run took (synchronises); a stage that did not run reads 0
  int times(double *ms, const char *who) {
    if (!enabled || marks < 2) { set_last_error("%s: set option time_stages before the call", who); return -1; }
    UH_CHECK(hipEventSynchronize(event[marks - 1]));
    for (int i = 0; i < N; ++i) {
      ms[i] = 0;
      if (i + 1 < marks) {
        float t = 0;
        UH_CHECK(hipEventElapsedTime(&t, event[i], event[i + 1]));
        ms[i] = t;
      }
    }
    return 0;
  }
};

}  // namespace uammd_hip
