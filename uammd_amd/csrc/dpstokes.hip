// Doubly periodic Stokes mobility and its integrator (Integrator/BDHI/DoublyPeriodic/DPStokesSlab.cuh and StokesSlab/* in the reference;
// DESIGN.md 18): particles in a fluid that is periodic in x and y and open, bounded by a bottom wall, or confined in a slit, z in
// [-H/2, H/2].
//
//   create     the refusals, the grid, the window, the BVP tables, the slit matrices' inverses       initialization.cu, spreadInterp.cuh:70-135
//   Mdot       (1) classify  (2) spread the three force components  (3) forward transforms          DPStokesSlab.cuh:220-251
//              (4) pressure solve, (5) the three velocity solves and their values at the walls       BVPStokes.cuh:187-276
//              (6) the constants of the analytic correction, the correction at the planes,           Correction.cuh
//                  to Chebyshev space; the zero mode; added
//              (7) inverse transforms, gather with the Clenshaw-Curtis weights                       spreadInterp.cuh:284-301
//   integrator M F, sqrt(2 T / dt) M^(1/2) W by Lanczos, the random-finite-difference drift, update  DPStokesSlab.cuh:424-583
//
// How the work is laid out here.
//  * The three spread grids are real, so fx + i fy and fz + i 0 go through TWO complex forward transforms; the solve kernels separate
//    the Hermitian parts on the fly and never materialise a spectrum per component.  The output goes back as u + i v and w + i p through
//    two inverse transforms.  Every kernel treats wave number k and -k as mirror images, and the slit inverse of -k is the conjugate of
//    that of k by construction, so the spectra stay Hermitian to the bit and the packed real parts do not mix.
//  * The spread is owner-computes, as in dppoisson.hip: a wave owns 8 x 8 nodes x 8 planes, keeps the 3 x 8 sums of a lane's node column
//    in registers, scans the particles 64 at a time and adds the hits in index order; the x, y and z weights of a hit are evaluated once
//    for the three components.  No atomics, no memset.  The sums are kept as 64-bit integers: every contribution w f is scaled by a power
//    of two chosen so that the particles inside the slab cannot overflow the sum (from their number and their largest force component,
//    both found by the classification), and truncated.  Integer addition is associative, so a node's sum does not depend on the order
//    of the particles at all: the same bits on every run AND for any permutation of the particles.  The truncation is below
//    2^-(62 - ceil(log2 N)) of the largest possible contribution: 2^-53 of it at N = 300, 2^-44 at N = 2 10^5.
//    set_option("simple_spread", 1) takes a lane per particle with floating-point atomic adds instead (the cross-check).
//  * The pressure solve takes a lane per wave number.  The three velocity solves depend only on the pressure and not on each other: they
//    take a lane per (wave number, component), three times the lanes.  Each solve is a serial chain of five passes over nz coefficients
//    with dependent loads, so at 128 x 128 a lane per wave number would leave three SIMDs in four with no wave at all.
//  * The correction is evaluated in double in either build, as section 17 does; every exponent is <= 0.
// A particle with |z| > H/2 (or a non-finite coordinate) is never spread or gathered and receives zero; it is counted.  The reference has
// no such guard.
#include "dp_slab.hpp"
#include "dpstokes_host.hpp"
#include "saru.hpp"
#include "../../include/uammd/device/BVP.hip.hpp"

#include <algorithm>
#include <cmath>
#include <new>
#include <string>
#include <vector>

namespace uammd_hip {

namespace dps {
constexpr int kOutside = dp::kOutside;
constexpr int kStages = 13;  // uammd_dpstokes_stage_times
constexpr int kFields = 14;

struct Host {  // everything create() works out before it touches the device
  int cells[3] = {0, 0, 0}, support = 0;
  double hx = 0, hy = 0, az = 0, rmax = 0, beta[3] = {0, 0, 0}, invnorm[3] = {0, 0, 0};
  double wmax = 0;  // an upper bound of a window's weight at a node: phi_x(0) phi_y(0) phi_z(0), and a hair
};

UH_D unsigned long long bits(float v) { return (unsigned long long)__float_as_uint(v); }
UH_D unsigned long long bits(double v) { return (unsigned long long)__double_as_longlong(v); }
template <class U> UH_D U from_bits(unsigned long long b);
template <> UH_D float from_bits<float>(unsigned long long b) { return __uint_as_float((unsigned)b); }
template <> UH_D double from_bits<double>(unsigned long long b) { return __longlong_as_double((long long)b); }
}  // namespace dps

UH_D float fmax_(float a, float b) { return fmaxf(a, b); }
UH_D double fmax_(double a, double b) { return fmax(a, b); }

// ---- (1) classification: the flag, the folded coordinates, the window's first nodes ---------------------------------------------------
template <class U>
__global__ __launch_bounds__(256) void k_dps_classify(const U *__restrict__ pos, int ps, const U *__restrict__ force, int fs, int N,
                                                      ChebGridBM<U> g, U half, typename VecOf<U>::T4 *__restrict__ rec, int4 *__restrict__ cellrec,
                                                      unsigned *__restrict__ counters) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  const bool active = i < N;
  bool outside = false;
  U fmax = U(0);
  if (active) {
    const U px = pos[(size_t)i * ps], py = pos[(size_t)i * ps + 1], pz = pos[(size_t)i * ps + 2];
    typename VecOf<U>::T4 r;
    r.x = r.y = r.z = r.w = U(0);
    int4 c = make_int4(0, 0, 0, 0);
    // (read before the window is placed, so that the loads are in flight meanwhile; a particle outside the slab does not use it)
    const U largest = fmax_(fmax_(abs_(force[(size_t)i * fs]), abs_(force[(size_t)i * fs + 1])), abs_(force[(size_t)i * fs + 2]));
    if (!dp_place(g, px, py, pz, half, r, c)) {
      outside = true;
      c.z = dps::kOutside;
    } else {
      fmax = largest;
    }
    rec[i] = r;
    cellrec[i] = c;
  }
  // counters: [0] particles outside, [1] inside, [2, 3] the bits of the largest |force component| of a particle inside (ordered like the
  // value for a non-negative number; a NaN sorts above infinity)
  const unsigned long long mOut = __ballot(active && outside), mIn = __ballot(active && !outside);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) fmax = fmax_(fmax, __shfl_xor(fmax, o, 64));
  if ((threadIdx.x & 63) == 0) {
    if (mOut) atomicAdd(&counters[0], (unsigned)__popcll(mOut));
    if (mIn) {
      atomicAdd(&counters[1], (unsigned)__popcll(mIn));
      atomicMax((unsigned long long *)(counters + 2), dps::bits(fmax));
    }
  }
}

// the power of two the spread's contributions are scaled by before they are truncated to integers: N_inside contributions of at most
// fmax wmax each stay below 2^62 in sum.  0: nothing to spread; NaN: a force is not finite.
template <class U> UH_D double dps_spread_scale(const unsigned *counters, U wmax) {
  const unsigned inside = counters[1];
  const U fmax = dps::from_bits<U>(*(const unsigned long long *)(counters + 2));
  if (inside == 0 || fmax == U(0)) return 0.0;
  const double top = (double)fmax * (double)wmax;
  if (!(top - top == 0.0)) return top - top;  // NaN
  const int nb = inside > 1 ? 32 - __clz((int)(inside - 1)) : 0;
  int shift = 62 - nb - (ilogb(top) + 1);
  shift = shift > 1000 ? 1000 : (shift < -1000 ? -1000 : shift);
  return ldexp(1.0, shift);
}

// ---- (2) the spread, owner-computes (the tile and the scan: DpTile) ----------------------------------------------------------------------
template <class U>
__global__ __launch_bounds__(64) void k_dps_spread_owner(const typename VecOf<U>::T4 *__restrict__ rec, const int4 *__restrict__ cellrec,
                                                         const U *__restrict__ force, int fs, int N, ChebGridBM<U> g,
                                                         const unsigned *__restrict__ counters, U wmax,
                                                         typename VecOf<U>::T2 *__restrict__ outXY, typename VecOf<U>::T2 *__restrict__ outZ) {
  constexpr int T = dp::kTile;
  const double scale = dps_spread_scale<U>(counters, wmax);
  const DpTile<U, ChebGridBM<U>> tile(g);
  const bool planeMine = tile.lane < T && tile.planeOK;  // lanes 0-7 evaluate the z weight of plane p0 + lane
  long long accX[T], accY[T], accZ[T];
#pragma unroll
  for (int p = 0; p < T; ++p) accX[p] = accY[p] = accZ[p] = 0;
  typename VecOf<U>::T4 r;
  U fx, fy, fz;
  int4 c;
  tile.scan(
      N,
      [&](int a) {
        r.x = r.y = r.z = r.w = U(0);
        fx = fy = fz = U(0);
        c = make_int4(0, 0, dps::kOutside, 0);
        if (a >= N) return false;
        c = cellrec[a];
        r = rec[a];
        if (c.z & dps::kOutside) return false;
        const bool hit = tile.touches_z(g, r.z) && tile.touches_xy(g, c);
        if (hit) { fx = force[(size_t)a * fs]; fy = force[(size_t)a * fs + 1]; fz = force[(size_t)a * fs + 2]; }
        return hit;
      },
      [&](int l) {
        const U px = bcast(r.x, l), py = bcast(r.y, l), pz = bcast(r.z, l);
        const U qx = bcast(fx, l), qy = bcast(fy, l), qz = bcast(fz, l);
        const U wxy = tile.wxy(g, px, py, __shfl(c.x, l, 64), __shfl(c.y, l, 64));
        const U wl = planeMine ? g.weight_z(pz, tile.zMine) : U(0);
#pragma unroll
        for (int p = 0; p < T; ++p) {
          const U w = wxy * bcast(wl, p);
          accX[p] += (long long)((double)(w * qx) * scale);
          accY[p] += (long long)((double)(w * qy) * scale);
          accZ[p] += (long long)((double)(w * qz) * scale);
        }
      });
  if (!tile.nodeOK) return;
  const double back = scale == 0.0 ? 0.0 : 1.0 / scale;  // (a power of two, or NaN when a force is not finite)
#pragma unroll
  for (int p = 0; p < T; ++p)
    if (tile.has_plane(p)) {
      typename VecOf<U>::T2 v;
      v.x = (U)((double)accX[p] * back); v.y = (U)((double)accY[p] * back);
      outXY[tile.at(g, p)] = v;
      v.x = (U)((double)accZ[p] * back); v.y = U(0);
      outZ[tile.at(g, p)] = v;
    }
}

// the one source of the plain spread (k_dp_spread_simple): the force, (fx, fy) into the first grid and fz into the real part of the second
template <class U> struct DpsSource {
  static constexpr int kSources = 1, kAmplitudes = 3;
  const U *force;
  int fs;
  UH_D DpSource<U, 3> get(int, int a, const typename VecOf<U>::T4 &r, int) const {
    return {true, r.z, {force[(size_t)a * fs], force[(size_t)a * fs + 1], force[(size_t)a * fs + 2]}, {0, 0, 1}, {0, 1, 0}};
  }
};

// ---- (4, 5) the solves -----------------------------------------------------------------------------------------------------------------
// Chebyshev coefficient n of component c (0, 1: the two real fields packed in one spectrum; 2: the real field of the other spectrum) of
// wave number s, sm its mirror
template <class U> UH_D typename VecOf<U>::T2 dps_component(const typename VecOf<U>::T2 *xy, const typename VecOf<U>::T2 *z, size_t nsys,
                                                            int s, int sm, int n, int c) {
  return dp_hermitian_part<U>(c == 2 ? z : xy, nsys, s, sm, n, c == 1 ? 1 : 0);
}

// the pressure: y'' - k^2 y = i k . f + d fz / dz, alpha = beta = 0 (BVPStokes.cuh:54-76, :239-245)
template <class U>
__global__ __launch_bounds__(64) void k_dps_pressure(uammd::BVP::device::Tables<U> t, const typename VecOf<U>::T2 *__restrict__ specXY,
                                                     const typename VecOf<U>::T2 *__restrict__ specZ, int nx, int ny, U invHalfHeight,
                                                     const U *__restrict__ kxPaired, const U *__restrict__ kyPaired,
                                                     typename VecOf<U>::T2 *__restrict__ rhs, typename VecOf<U>::T2 *__restrict__ an,
                                                     typename VecOf<U>::T2 *__restrict__ pressure) {
  using T2 = typename VecOf<U>::T2;
  const int s = blockIdx.x * 64 + threadIdx.x;
  const int nsys = nx * ny;
  if (s >= nsys) return;
  const size_t n = (size_t)nsys;
  const int nz = t.nz;
  T2 zero;
  zero.x = zero.y = U(0);
  if (s == 0) {  // the k = 0 column is zero; with walls the zero mode has a solve of its own
    for (int m = 0; m < nz; ++m) pressure[n * m] = zero;
    return;
  }
  const int sm = dps::mirror(s, nx, ny);
  const U kx = kxPaired[s], ky = kyPaired[s];
  T2 d2 = zero, d1 = zero;
  for (int m = nz - 1; m >= 0; --m) {
    T2 d = zero;
    if (m <= nz - 2) {
      const T2 up = dps_component<U>(specXY, specZ, n, s, sm, m + 1, 2);
      d.x = d2.x + (U(2.0) * U(m + 1) * up.x) * invHalfHeight;
      d.y = d2.y + (U(2.0) * U(m + 1) * up.y) * invHalfHeight;
    }
    d2 = d1;
    d1 = d;
    if (m == 0) { d.x *= U(0.5); d.y *= U(0.5); }
    const T2 fx = dps_component<U>(specXY, specZ, n, s, sm, m, 0), fy = dps_component<U>(specXY, specZ, n, s, sm, m, 1);
    T2 r;
    r.x = -(kx * fx.y + ky * fy.y) + d.x;
    r.y = (kx * fx.x + ky * fy.x) + d.y;
    rhs[s + n * m] = r;
  }
  uammd::BVP::device::solveSystem(t, s, Row<T2>{rhs + s, n}, zero, zero, Row<T2>{an + s, n}, Row<T2>{pressure + s, n});
}

// the three velocities, a lane per (wave number, component): right-hand sides and boundary values of BVPStokes.cuh:78-184, then the
// solution at the two walls (sums and alternating sums of its coefficients)
template <class U>
__global__ __launch_bounds__(64) void k_dps_velocity(uammd::BVP::device::Tables<U> t, const typename VecOf<U>::T2 *__restrict__ specXY,
                                                     const typename VecOf<U>::T2 *__restrict__ specZ,
                                                     const typename VecOf<U>::T2 *__restrict__ pressure, int nx, int ny, U invHalfHeight,
                                                     U viscosity, const U *__restrict__ kmod, const U *__restrict__ kxPaired,
                                                     const U *__restrict__ kyPaired, typename VecOf<U>::T2 *__restrict__ rhs,
                                                     typename VecOf<U>::T2 *__restrict__ an, typename VecOf<U>::T2 *__restrict__ vel,
                                                     typename VecOf<U>::T2 *__restrict__ wall) {
  using T2 = typename VecOf<U>::T2;
  const int id = blockIdx.x * 64 + threadIdx.x;
  const int nsys = nx * ny;
  if (id >= 3 * nsys) return;
  const int c = id / nsys, s = id - c * nsys;
  const size_t n = (size_t)nsys, field = n * (size_t)t.nz;
  const int nz = t.nz;
  T2 zero;
  zero.x = zero.y = U(0);
  T2 *out = vel + field * c + s, *r = rhs + field * c + s, *a = an + field * c + s;
  if (s == 0) {
    for (int m = 0; m < nz; ++m) out[n * m] = zero;
    wall[(size_t)2 * id] = zero;
    wall[(size_t)2 * id + 1] = zero;
    return;
  }
  const int sm = dps::mirror(s, nx, ny);
  const U invmu = U(1.0) / viscosity;
  const T2 *p = pressure + s;
  T2 pH = zero, pmH = zero;
  for (int m = 0; m < nz; ++m) {
    const T2 v = p[n * m];
    pH.x += v.x; pH.y += v.y;
    if (m % 2 == 0) { pmH.x += v.x; pmH.y += v.y; }
    else { pmH.x -= v.x; pmH.y -= v.y; }
  }
  T2 alpha, beta;
  if (c < 2) {
    const U kd = c == 0 ? kxPaired[s] : kyPaired[s];
    for (int m = 0; m < nz; ++m) {
      const T2 f = dps_component<U>(specXY, specZ, n, s, sm, m, c), pv = p[n * m];
      T2 v;
      v.x = (-(kd * pv.y) - f.x) * invmu;
      v.y = (kd * pv.x - f.y) * invmu;
      r[n * m] = v;
    }
    const U fac = (U(0.5) * kd) / (viscosity * kmod[s]);
    alpha.x = fac * pH.y; alpha.y = -(fac * pH.x);   // -fac (i pH)
    beta.x = -(fac * pmH.y); beta.y = fac * pmH.x;   //  fac (i pmH)
  } else {
    T2 d2 = zero, d1 = zero;
    for (int m = nz - 1; m >= 0; --m) {
      T2 d = zero;
      if (m <= nz - 2) {
        const T2 up = p[n * (m + 1)];
        d.x = d2.x + (U(2.0) * U(m + 1) * up.x) * invHalfHeight;
        d.y = d2.y + (U(2.0) * U(m + 1) * up.y) * invHalfHeight;
      }
      d2 = d1;
      d1 = d;
      if (m == 0) { d.x *= U(0.5); d.y *= U(0.5); }
      const T2 f = dps_component<U>(specXY, specZ, n, s, sm, m, 2);
      T2 v;
      v.x = (d.x - f.x) * invmu;
      v.y = (d.y - f.y) * invmu;
      r[n * m] = v;
    }
    const U fac = U(0.5) / viscosity;
    alpha.x = fac * pH.x; alpha.y = fac * pH.y;
    beta.x = fac * pmH.x; beta.y = fac * pmH.y;
  }
  uammd::BVP::device::solveSystem(t, s, Row<T2>{r, n}, alpha, beta, Row<T2>{a, n}, Row<T2>{out, n});
  T2 top = zero, bot = zero;
  for (int m = 0; m < nz; ++m) {
    const T2 v = out[n * m];
    top.x += v.x; top.y += v.y;
    if (m % 2 == 0) { bot.x += v.x; bot.y += v.y; }
    else { bot.x -= v.x; bot.y -= v.y; }
  }
  wall[(size_t)2 * id] = top;
  wall[(size_t)2 * id + 1] = bot;
}

// ---- (6) the wall correction (Correction.cuh), in double ---------------------------------------------------------------------------------
// the constants of a wave number, 8 complex at c nsys + s: slit C = A^-1 b (fillRightHandSide, Correction.cuh:286-324); bottom keeps
// (u0, v0, w0) = minus the solution at the bottom wall in the first three
template <class U>
__global__ __launch_bounds__(64) void k_dps_constants(const typename VecOf<U>::T2 *__restrict__ wall, const double2 *__restrict__ invA,
                                                      const double *__restrict__ kxPaired, const double *__restrict__ kyPaired, int nsys, int mode,
                                                      double2 *__restrict__ constants) {
  const int s = blockIdx.x * 64 + threadIdx.x;
  if (s >= nsys) return;
  const size_t n = (size_t)nsys;
  cd2 top[3], bot[3];
  for (int c = 0; c < 3; ++c) {
    const typename VecOf<U>::T2 t = wall[2 * (c * n + s)], b = wall[2 * (c * n + s) + 1];
    top[c] = cd2{-(double)t.x, -(double)t.y};
    bot[c] = cd2{-(double)b.x, -(double)b.y};
  }
  cd2 out[8];
  for (int r = 0; r < 8; ++r) out[r] = cd2{0.0, 0.0};
  if (s != 0) {
    if (mode == dps::kSlit) {
      const double kx = kxPaired[s], ky = kyPaired[s];
      cd2 b[8];
      b[0] = times_minus_i(kx * bot[0] + ky * bot[1]);
      b[1] = times_minus_i(kx * top[0] + ky * top[1]);
      b[2] = bot[0]; b[3] = bot[1]; b[4] = bot[2];
      b[5] = top[0]; b[6] = top[1]; b[7] = top[2];
      for (int r = 0; r < 8; ++r) {
        cd2 acc{0.0, 0.0};
        for (int c = 0; c < 8; ++c) {
          const double2 m = invA[(size_t)(8 * r + c) * n + s];
          acc = acc + cmul(cd2{m.x, m.y}, b[c]);
        }
        out[r] = acc;
      }
    } else {
      out[0] = bot[0]; out[1] = bot[1]; out[2] = bot[2];
    }
  }
  for (int r = 0; r < 8; ++r) constants[r * n + s] = make_double2(out[r].x, out[r].y);
}

// the correction at the planes, one lane per (wave number, plane): (u, v, w, p) into four fields (p only in a slit)
template <class U>
__global__ __launch_bounds__(256) void k_dps_correction(const double2 *__restrict__ constants, const double *__restrict__ kmod,
                                                        const double *__restrict__ kxPaired, const double *__restrict__ kyPaired,
                                                        const double *__restrict__ zplane, int nsys, int nz, int mode, double H, double viscosity,
                                                        typename VecOf<U>::T2 *__restrict__ out) {
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (size_t)nsys * nz) return;
  const int s = (int)(idx % (size_t)nsys), plane = (int)(idx / (size_t)nsys);
  const size_t n = (size_t)nsys, field = n * nz;
  cd2 u{0.0, 0.0}, v{0.0, 0.0}, w{0.0, 0.0}, p{0.0, 0.0};
  if (s != 0) {
    const double k = kmod[s], kx = kxPaired[s], ky = kyPaired[s];
    const double z = zplane[plane] + 0.5 * H;  // height above the bottom wall
    const double ekz = exp(-k * z);
    auto C = [&](int r) { const double2 c = constants[r * n + s]; return cd2{c.x, c.y}; };
    if (mode == dps::kSlit) {
      const double ekzmH = exp(k * (z - H)), hm = 0.5 / viscosity;
      const cd2 C0 = C(0), C1 = C(1);
      const cd2 par = times_minus_i((hm / k * z) * (C0 * ekz - C1 * ekzmH));
      u = kx * par + C(2) * ekz + C(3) * ekzmH;
      v = ky * par + C(4) * ekz + C(5) * ekzmH;
      w = C0 * (hm * z * ekz) + C1 * (hm * z * ekzmH) + C(6) * ekz + C(7) * ekzmH;
      p = C0 * (z * ekz) + C1 * ekzmH;
    } else {
      const cd2 u0 = C(0), v0 = C(1), w0 = C(2);
      const cd2 S = kx * u0 + ky * v0;
      const cd2 par = -((S + times_i(k * w0)) * (z * ekz / k));
      u = kx * par + u0 * ekz;
      v = ky * par + v0 * ekz;
      w = (k * w0 + times_minus_i(S)) * (z * ekz) + w0 * ekz;
    }
  }
  typename VecOf<U>::T2 o;
  o.x = (U)u.x; o.y = (U)u.y; out[idx] = o;
  o.x = (U)v.x; o.y = (U)v.y; out[field + idx] = o;
  o.x = (U)w.x; o.y = (U)w.y; out[2 * field + idx] = o;
  if (mode == dps::kSlit) { o.x = (U)p.x; o.y = (U)p.y; out[3 * field + idx] = o; }
}

// the zero mode: mu u'' = -f for x (lane 0) and y (lane 1) with the mode's boundary rows, -D (c0; d0) = C f (Correction.cuh:70-126)
template <class U>
__global__ __launch_bounds__(64) void k_dps_zero_mode(uammd::BVP::device::Tables<U> t0, const typename VecOf<U>::T2 *__restrict__ specXY,
                                                      size_t nsys, U viscosity, typename VecOf<U>::T2 *__restrict__ scratch) {
  using T2 = typename VecOf<U>::T2;
  const int c = threadIdx.x;
  if (c >= 2) return;
  const int nz = t0.nz;
  T2 *fn = scratch + (size_t)3 * nz * c, *an = fn + nz, *cn = an + nz;
  const U invmu = U(1.0) / viscosity;
  for (int m = 0; m < nz; ++m) {
    const T2 g = specXY[nsys * m];  // the k = 0 column is its own mirror: fx = Re, fy = Im
    T2 f;
    f.x = -((c == 0 ? g.x : g.y) * invmu);
    f.y = U(0);
    fn[m] = f;
  }
  T2 zero;
  zero.x = zero.y = U(0);
  uammd::BVP::device::solveSystem(t0, 0, fn, zero, zero, an, cn);
}

// ---- add the correction and the zero mode, keep the corrected coefficients, pack them as (u + i v), (w + i p) ---------------------------
template <class U>
__global__ __launch_bounds__(64) void k_dps_assemble(typename VecOf<U>::T2 *__restrict__ vel, typename VecOf<U>::T2 *__restrict__ pressure,
                                                     const typename VecOf<U>::T2 *__restrict__ corr, const typename VecOf<U>::T2 *__restrict__ zeroMode,
                                                     int nsys, int nz, int mode, typename VecOf<U>::T2 *__restrict__ uv,
                                                     typename VecOf<U>::T2 *__restrict__ wp) {
  using T2 = typename VecOf<U>::T2;
  const int s = blockIdx.x * 64 + threadIdx.x;
  if (s >= nsys) return;
  const size_t n = (size_t)nsys, field = n * nz;
  for (int m = 0; m < nz; ++m) {
    const size_t at = s + n * m;
    T2 u = vel[at], v = vel[field + at], w = vel[2 * field + at], p = pressure[at];
    if (mode != dps::kNone) {
      if (s == 0) {
        u = zeroMode[2 * nz + m];
        v = zeroMode[5 * nz + m];
      } else {
        const T2 cu = corr[at], cv = corr[field + at], cw = corr[2 * field + at];
        u.x += cu.x; u.y += cu.y;
        v.x += cv.x; v.y += cv.y;
        w.x += cw.x; w.y += cw.y;
        if (mode == dps::kSlit) {
          const T2 cp = corr[3 * field + at];
          p.x += cp.x; p.y += cp.y;
        }
      }
      vel[at] = u; vel[field + at] = v; vel[2 * field + at] = w; pressure[at] = p;
    }
    T2 o;
    o.x = u.x - v.y; o.y = u.y + v.x;
    uv[at] = o;
    o.x = w.x - p.y; o.y = w.y + p.x;
    wp[at] = o;
  }
}

// ---- (7) gather (k_dp_gather): the three velocities; a particle outside the slab receives zero -------------------------------------------
template <class U> struct DpsSink {
  UH_D static void outside(int a, int lane, U *mf) {
    if (lane < 3) mf[(size_t)3 * a + lane] = U(0);
  }
  UH_D static void write(int a, const typename VecOf<U>::T4 &, const U *sum, U *mf) {
    mf[(size_t)3 * a] = sum[0];
    mf[(size_t)3 * a + 1] = sum[1];
    mf[(size_t)3 * a + 2] = sum[2];
  }
};

// ---- the integrator's kernels (DPStokesSlab.cuh:363-418) ----------------------------------------------------------------------------------
template <class U> __global__ __launch_bounds__(256) void k_dps_noise(U *__restrict__ out, int N, uint s1, uint s2, float std) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  Saru rng(s1, s2, (uint)i);
  const float2 a = rng.gf(0.0f, std);
  const float b = rng.gf(0.0f, std).x;
  out[(size_t)3 * i] = (U)a.x;
  out[(size_t)3 * i + 1] = (U)a.y;
  out[(size_t)3 * i + 2] = (U)b;
}

template <class U>
__global__ __launch_bounds__(256) void k_dps_shift(const U *__restrict__ pos, int ps, const U *__restrict__ w, U sign, int N, U *__restrict__ out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  for (int c = 0; c < 3; ++c) out[(size_t)3 * i + c] = pos[(size_t)i * ps + c] + sign * w[(size_t)3 * i + c];
}

template <class U>
__global__ __launch_bounds__(256) void k_dps_drift(const U *__restrict__ plus, const U *__restrict__ minus, U factor, int n, U *__restrict__ out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[i] = factor * (plus[i] - minus[i]);
}

// BDIntegrate: noise, noisePrev and rfd may be null
template <class U>
__global__ __launch_bounds__(256) void k_dps_update(U *__restrict__ pos, int ps, const U *__restrict__ mf, const U *__restrict__ noise,
                                                    const U *__restrict__ noisePrev, const U *__restrict__ rfd, U dt, int N) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  for (int c = 0; c < 3; ++c) {
    const size_t at = (size_t)3 * i + c;
    U d = mf[at] * dt;
    if (noise) {
      const U fluct = noisePrev ? dt * U(0.5) * (noise[at] + noisePrev[at]) : dt * noise[at];
      d += fluct + rfd[at];
    }
    pos[(size_t)i * ps + c] += d;
  }
}

// ---- host -----------------------------------------------------------------------------------------------------------------------------
namespace dps {

static double bm_norm(double alpha, double beta) {  // IBM_kernels.cuh:60-97: 2 Simpson(BM, 0, alpha) on 20000 intervals, compensated sum
  const int Nr = 20000;
  const double dx = alpha / Nr;
  double sum = 0, comp = 0;
  for (int i = 0; i <= Nr; ++i) {
    const double weight = (i == 0 || i == Nr) ? 1.0 : (i % 2 ? 4.0 : 2.0);
    const double z = (i * dx) / alpha, dz2 = 1.0 - z * z;
    const double v = weight * (dz2 < 0 ? 0.0 : std::exp(beta * (std::sqrt(dz2) - 1.0)));
    const double y = v - comp, t = sum + y;
    comp = (t - sum) - y;
    sum = t;
  }
  return 2.0 * (dx / 3.0 * sum);
}

// Everything the constructor decides, on the host in double (no device call): 0, or -2 with a message.
static int configure(const uammd_dpstokes_parameters &p, Host &o) {
  if (!(p.viscosity > 0)) { set_last_error("[DPStokes] Viscosity was not set"); return -2; }   // initialization.cu:12-26
  if (!(p.H > 0)) { set_last_error("[DPStokes] H (height) was not set"); return -2; }
  if (!(p.Lx > 0) || !(p.Ly > 0)) { set_last_error("[DPStokes] Domain width (Lx, Ly) was not set"); return -2; }
  if (p.nx < 1 || p.ny < 1) { set_last_error("[DPStokes] Invalid argument: cell dimensions must be positive"); return -2; }
  if (p.mode < kNone || p.mode > kSlit) { set_last_error("uammd_dpstokes_create: mode = %d (0 none, 1 bottom, 2 slit)", p.mode); return -2; }
  if (!std::isfinite(p.viscosity) || !std::isfinite(p.H) || !std::isfinite(p.Lx) || !std::isfinite(p.Ly)) {
    set_last_error("uammd_dpstokes_create: viscosity, H, Lx and Ly must be finite");
    return -2;
  }
  if (!(p.w > 0) || !(p.alpha > 0) || !(p.beta[0] > 0) || !std::isfinite(p.w) || !std::isfinite(p.alpha) || !std::isfinite(p.beta[0])) {
    set_last_error("uammd_dpstokes_create: the window needs w, alpha and beta.x positive (got %g, %g, %g)", p.w, p.alpha, p.beta[0]);
    return -2;
  }
  o.hx = p.Lx / p.nx;
  o.hy = p.Ly / p.ny;
  o.cells[0] = p.nx;
  o.cells[1] = p.ny;
  o.cells[2] = p.nz >= 0 ? p.nz : (int)(M_PI * p.H / std::min(o.hx, o.hy));
  if (o.cells[2] < 4) {
    set_last_error("uammd_dpstokes_create: nz = %d: the second-integral recurrence of the boundary value solver needs nz >= 4", o.cells[2]);
    return -2;
  }
  o.support = (int)(p.w + 0.5);
  if (o.support > dp::kMaxSupport) {
    set_last_error("uammd_dpstokes_create: support = %d: the window takes at most %d nodes per axis (w <= %g)", o.support, dp::kMaxSupport,
                   dp::kMaxSupport + 0.49);
    return -2;
  }
  if (o.support < 1 || o.support > std::min(p.nx, p.ny)) {
    set_last_error("uammd_dpstokes_create: support = %d must be at least 1 and fit the %d x %d plane", o.support, p.nx, p.ny);
    return -2;
  }
  o.beta[0] = p.beta[0];
  o.beta[1] = p.beta[1] < 0 ? p.beta[0] : p.beta[1];  // spreadInterp.cuh:353-356
  o.beta[2] = p.beta[2] < 0 ? p.beta[0] : p.beta[2];
  for (int a = 0; a < 3; ++a) o.invnorm[a] = 1.0 / bm_norm(p.alpha, o.beta[a]);
  o.az = std::min(o.hx, o.hy);
  o.rmax = std::max(p.w * std::max(o.hx, o.hy) * 0.5, p.alpha * o.az);
  o.wmax = 1.001 * (o.invnorm[0] / o.hx) * (o.invnorm[1] / o.hy) * (o.invnorm[2] / o.az);
  return 0;
}

}  // namespace dps

struct DPStokes {
  uammd_dpstokes_parameters par{};
  dps::Host cfg;
  bool doublePrecision = false, simpleSpread = false;
  int nsys = 0, nz = 0;
  uammd_fct *fct = nullptr;
  uammd_bvp *bvp = nullptr, *bvpZero = nullptr;
  DeviceBuffer zplane, qw, kmod, kxPaired, kyPaired, zplaneD, kmodD, kxPairedD, kyPairedD, invA;
  DeviceBuffer fields, wall, constants, zeroMode, counters;
  DeviceBuffer rec, cellrec;
  bool ran = false;
  StageTimer<dps::kStages> timer;  // option time_stages (uammd_dpstokes_stage_times)
  ~DPStokes() {
    if (fct) uammd_fct_destroy(fct);
    if (bvp) uammd_bvp_destroy(bvp);
    if (bvpZero) uammd_bvp_destroy(bvpZero);
  }
};

template <class U> static ChebGridBM<U> dps_grid(const DPStokes *h) {
  const auto &p = h->par;
  const auto &c = h->cfg;
  ChebGridBM<U> g;
  g.nx = c.cells[0]; g.ny = c.cells[1]; g.nz = c.cells[2];
  g.support = c.support;
  g.Lx = (U)p.Lx; g.Ly = (U)p.Ly; g.span = (U)p.H;
  g.hx = (U)c.hx; g.hy = (U)c.hy;
  g.invhx = (U)(1.0 / c.hx); g.invhy = (U)(1.0 / c.hy);
  g.alpha = (U)p.alpha; g.az = (U)c.az;
  g.betax = (U)c.beta[0]; g.betay = (U)c.beta[1]; g.betaz = (U)c.beta[2];
  g.invnormx = (U)c.invnorm[0]; g.invnormy = (U)c.invnorm[1]; g.invnormz = (U)c.invnorm[2];
  g.rmax = (U)c.rmax;
  g.reachz = (U)(p.alpha * c.az) * U(1.000001);
  g.zplane = (const U *)h->zplane.ptr;
  g.qw = (const U *)h->qw.ptr;
  return g;
}

template <class U> static int dps_build(DPStokes *h) {
  const auto &p = h->par;
  const auto &c = h->cfg;
  const int nx = c.cells[0], ny = c.cells[1], nz = c.cells[2], nsys = nx * ny;
  h->nsys = nsys;
  h->nz = nz;
  const double Hh = 0.5 * p.H;
  std::vector<double> zp, qw, k(nsys), kx(nsys), ky(nsys), tfi(nsys), tsi(nsys), bfi(nsys), bsi(nsys);
  dp::chebyshev_planes(nz, Hh, c.hx, c.hy, zp, qw);
  for (int s = 0; s < nsys; ++s) {
    dp::wave_vector(s, nx, ny, p.Lx, p.Ly, kx[s], ky[s], k[s]);
    dp::bvp_boundary_factors(k[s], Hh, tfi[s], tsi[s], bfi[s], bsi[s]);
  }
  int e = upload<U>(h->zplane, zp);
  if (!e) e = upload<U>(h->qw, qw);
  if (!e) e = upload<U>(h->kmod, k);
  if (!e) e = upload<U>(h->kxPaired, kx);
  if (!e) e = upload<U>(h->kyPaired, ky);
  if (e) return e;
  if (p.mode != dps::kNone) {  // what the correction reads, in double
    e = upload<double>(h->zplaneD, zp);
    if (!e) e = upload<double>(h->kmodD, k);
    if (!e) e = upload<double>(h->kxPairedD, kx);
    if (!e) e = upload<double>(h->kyPairedD, ky);
    if (e) return e;
    if (p.mode == dps::kSlit) {
      std::vector<dps::cplx> inv;
      std::string err;
      if (dps::slit_inverses(nx, ny, p.Lx, p.Ly, p.viscosity, p.H, inv, err)) { set_last_error("%s", err.c_str()); return -2; }
      std::vector<double> flat((size_t)128 * nsys);  // entry major: entry n of wave number s at n nsys + s
      for (int s = 0; s < nsys; ++s)
        for (int n = 0; n < 64; ++n) {
          flat[2 * ((size_t)n * nsys + s)] = inv[(size_t)64 * s + n].real();
          flat[2 * ((size_t)n * nsys + s) + 1] = inv[(size_t)64 * s + n].imag();
        }
      if (int e2 = upload<double>(h->invA, flat)) return e2;
    }
    double f[4];
    dps::zero_mode_factors(p.mode, f);
    const double k0 = 0.0;
    if (int e2 = uammd_bvp_create(1, nz, Hh, &k0, &f[0], &f[1], &f[2], &f[3], h->doublePrecision, &h->bvpZero)) return e2;
    if (int e2 = h->constants.reserve(sizeof(double2) * 8 * (size_t)nsys)) return e2;
    if (int e2 = h->zeroMode.reserve(2 * sizeof(U) * 6 * (size_t)nz)) return e2;
  }
  if (int e2 = uammd_fct_create(nx, ny, nz, h->doublePrecision, &h->fct)) return e2;
  if (int e2 = uammd_bvp_create(nsys, nz, Hh, k.data(), tfi.data(), tsi.data(), bfi.data(), bsi.data(), h->doublePrecision, &h->bvp)) return e2;
  if (int e2 = h->fields.reserve(2 * sizeof(U) * (size_t)nsys * nz * dps::kFields)) return e2;
  if (int e2 = h->wall.reserve(2 * sizeof(U) * 6 * (size_t)nsys)) return e2;
  if (int e2 = h->counters.reserve(8 * sizeof(unsigned))) return e2;
  UH_CHECK(hipMemset(h->counters.ptr, 0, 8 * sizeof(unsigned)));
  return 0;
}

// DPStokes::Mdot (DPStokesSlab.cuh:220-251).  d_mf == nullptr stops after the corrected Chebyshev coefficients (computeAverageVelocity).
template <class U>
static int dps_run(DPStokes *h, const U *d_pos, int ps, const U *d_force, int fs, int N, U *d_mf, hipStream_t st) {
  using T2 = typename VecOf<U>::T2;
  const auto &p = h->par;
  const ChebGridBM<U> g = dps_grid<U>(h);
  const int nsys = h->nsys, nz = h->nz, mode = p.mode;
  const size_t field = (size_t)nsys * nz;
  if (int e = h->rec.reserve(sizeof(typename VecOf<U>::T4) * (size_t)N)) return e;
  if (int e = h->cellrec.reserve(sizeof(int4) * (size_t)N)) return e;
  // fields: 0, 1 the spectra of (fx + i fy), (fz); 2, 3 the spread grids; 4-6 right-hand sides; 7-9 second derivatives; 10 pressure;
  // 11-13 velocities.  Later: the correction at the planes in 6-9 and in Chebyshev space in 2-5; the packed output in 6, 7 and its
  // inverse transforms in 8, 9.
  T2 *F[dps::kFields];
  for (int i = 0; i < dps::kFields; ++i) F[i] = (T2 *)h->fields.ptr + field * i;
  const typename VecOf<U>::T4 *rec = (const typename VecOf<U>::T4 *)h->rec.ptr;
  const int4 *cellrec = (const int4 *)h->cellrec.ptr;
  h->timer.reset();
  auto mark = [&]() { return h->timer.mark(st); };
  if (int e = mark()) return e;
  // (1)
  UH_CHECK(hipMemsetAsync(h->counters.ptr, 0, 8 * sizeof(unsigned), st));
  hipLaunchKernelGGL((k_dps_classify<U>), dim3((N + 255) / 256), dim3(256), 0, st, d_pos, ps, d_force, fs, N, g, (U)(0.5 * p.H),
                     (typename VecOf<U>::T4 *)h->rec.ptr, (int4 *)h->cellrec.ptr, (unsigned *)h->counters.ptr);
  if (int e = mark()) return e;
  // (2)
  if (h->simpleSpread) {
    UH_CHECK(hipMemsetAsync(F[2], 0, sizeof(T2) * field * 2, st));
    hipLaunchKernelGGL((k_dp_spread_simple<U, ChebGridBM<U>, DpsSource<U>>), dim3((N + 63) / 64), dim3(64), 0, st, rec, cellrec, N, g,
                       DpsSource<U>{d_force, fs}, (U *)F[2], (U *)F[3]);
  } else {
    hipLaunchKernelGGL((k_dps_spread_owner<U>), dp_owner_grid(g.nx, g.ny, nz), dim3(64), 0, st, rec, cellrec, d_force, fs, N, g,
                       (const unsigned *)h->counters.ptr, (U)h->cfg.wmax, F[2], F[3]);
  }
  UH_CHECK(hipGetLastError());
  if (int e = mark()) return e;
  auto fctRun = [&](bool planes, const T2 *in, T2 *out, int dir) { return fct_run<U>(h->fct, planes, in, out, dir, st); };
  // (3)
  if (int e = fctRun(true, F[2], F[0], UAMMD_FCT_FORWARD)) return e;
  if (int e = mark()) return e;
  if (int e = fctRun(true, F[3], F[1], UAMMD_FCT_FORWARD)) return e;
  if (int e = mark()) return e;
  // (4, 5)
  uammd_bvp_tables bt;
  if (int e = uammd_bvp_device_tables(h->bvp, &bt)) return e;
  const double Hh = 0.5 * p.H;
  const auto tables = uammd::BVP::device::Tables<U>::over((const U *)bt.d_tables, nsys, nz, (U)(Hh * Hh));
  const U *kmod = (const U *)h->kmod.ptr, *kxP = (const U *)h->kxPaired.ptr, *kyP = (const U *)h->kyPaired.ptr;
  hipLaunchKernelGGL((k_dps_pressure<U>), dim3((nsys + 63) / 64), dim3(64), 0, st, tables, (const T2 *)F[0], (const T2 *)F[1], g.nx, g.ny,
                     (U)(1.0 / Hh), kxP, kyP, F[4], F[7], F[10]);
  UH_CHECK(hipGetLastError());
  if (int e = mark()) return e;
  hipLaunchKernelGGL((k_dps_velocity<U>), dim3((3 * nsys + 63) / 64), dim3(64), 0, st, tables, (const T2 *)F[0], (const T2 *)F[1],
                     (const T2 *)F[10], g.nx, g.ny, (U)(1.0 / Hh), (U)p.viscosity, kmod, kxP, kyP, F[4], F[7], F[11], (T2 *)h->wall.ptr);
  UH_CHECK(hipGetLastError());
  if (int e = mark()) return e;
  // (6)
  if (mode != dps::kNone) {
    hipLaunchKernelGGL((k_dps_constants<U>), dim3((nsys + 63) / 64), dim3(64), 0, st, (const T2 *)h->wall.ptr, (const double2 *)h->invA.ptr,
                       (const double *)h->kxPairedD.ptr, (const double *)h->kyPairedD.ptr, nsys, mode, (double2 *)h->constants.ptr);
    UH_CHECK(hipGetLastError());
    if (int e = mark()) return e;
    hipLaunchKernelGGL((k_dps_correction<U>), dim3((unsigned)((field + 255) / 256)), dim3(256), 0, st, (const double2 *)h->constants.ptr,
                       (const double *)h->kmodD.ptr, (const double *)h->kxPairedD.ptr, (const double *)h->kyPairedD.ptr,
                       (const double *)h->zplaneD.ptr, nsys, nz, mode, p.H, p.viscosity, F[6]);
    UH_CHECK(hipGetLastError());
    if (int e = mark()) return e;
    const int ncorr = mode == dps::kSlit ? 4 : 3;  // (the bottom wall's correction has no pressure)
    for (int c = 0; c < ncorr; ++c)
      if (int e = fctRun(false, F[6 + c], F[2 + c], UAMMD_FCT_FORWARD)) return e;
    if (int e = mark()) return e;
    uammd_bvp_tables bz;
    if (int e = uammd_bvp_device_tables(h->bvpZero, &bz)) return e;
    const auto t0 = uammd::BVP::device::Tables<U>::over((const U *)bz.d_tables, 1, nz, (U)(Hh * Hh));
    hipLaunchKernelGGL((k_dps_zero_mode<U>), dim3(1), dim3(64), 0, st, t0, (const T2 *)F[0], (size_t)nsys, (U)p.viscosity, (T2 *)h->zeroMode.ptr);
    UH_CHECK(hipGetLastError());
  } else {
    for (int i = 0; i < 3; ++i)
      if (int e = mark()) return e;
  }
  // the corrected coefficients stay in 10-13 (uammd_dpstokes_fluid_cheb); packed into 6 (u + i v) and 7 (w + i p)
  hipLaunchKernelGGL((k_dps_assemble<U>), dim3((nsys + 63) / 64), dim3(64), 0, st, F[11], F[10], (const T2 *)F[2], (const T2 *)h->zeroMode.ptr,
                     nsys, nz, mode, F[6], F[7]);
  UH_CHECK(hipGetLastError());
  if (int e = mark()) return e;
  h->ran = true;
  if (!d_mf) return 0;
  // (7)
  if (int e = fctRun(true, F[6], F[8], UAMMD_FCT_INVERSE)) return e;
  if (int e = mark()) return e;
  if (int e = fctRun(true, F[7], F[9], UAMMD_FCT_INVERSE)) return e;
  if (int e = mark()) return e;
  hipLaunchKernelGGL((k_dp_gather<U, ChebGridBM<U>, 3, DpsSink<U>, U>), dim3((N + 3) / 4), dim3(256), 0, st, rec, cellrec, N, g, (const T2 *)F[8],
                     (const T2 *)F[9], d_mf);
  UH_CHECK(hipGetLastError());
  if (int e = mark()) return e;
  return 0;
}

static int dps_check(DPStokes *h, bool wantDouble, const void *pos, int ps, const void *force, int fs, const void *torque, int N, const char *who) {
  if (torque) { set_last_error("[DPStokes] Torques are not implemented (%s: pass a null torque pointer)", who); return -3; }
  if (!h) { set_last_error("%s: null handle", who); return -1; }
  if (int e = dp_check_precision(h->doublePrecision, wantDouble, who)) return e;
  if (N < 0) { set_last_error("%s: numberParticles = %d", who, N); return -1; }
  if ((ps != 3 && ps != 4) || (fs != 3 && fs != 4)) { set_last_error("%s: positions and forces are rows of 3 or 4 reals (got %d, %d)", who, ps, fs); return -1; }
  if (N > 0 && (!pos || !force)) { set_last_error("%s: null argument", who); return -1; }
  return 0;
}

static int dps_mdot(DPStokes *h, bool wantDouble, const void *pos, int ps, const void *force, int fs, const void *torque, int N, void *mf,
                    void *stream, const char *who) {
  if (int e = dps_check(h, wantDouble, pos, ps, force, fs, torque, N, who)) return e;
  if (N == 0) return 0;
  if (!mf) { set_last_error("%s: null argument", who); return -1; }
  return wantDouble ? dps_run<double>(h, (const double *)pos, ps, (const double *)force, fs, N, (double *)mf, (hipStream_t)stream)
                    : dps_run<float>(h, (const float *)pos, ps, (const float *)force, fs, N, (float *)mf, (hipStream_t)stream);
}

// the k = 0 column of velocity component `direction` after a run, as nz host doubles (real parts)
static int dps_zero_column(DPStokes *h, int direction, std::vector<double> &col, hipStream_t st) {
  const size_t real = h->doublePrecision ? sizeof(double) : sizeof(float);
  const size_t field = (size_t)h->nsys * h->nz;
  const char *src = (const char *)h->fields.ptr + 2 * real * field * (11 + direction);
  std::vector<double> raw64(2 * (size_t)h->nz);
  std::vector<float> raw32(2 * (size_t)h->nz);
  void *dst = h->doublePrecision ? (void *)raw64.data() : (void *)raw32.data();
  UH_CHECK(hipStreamSynchronize(st));
  UH_CHECK(hipMemcpy2D(dst, 2 * real, src, 2 * real * (size_t)h->nsys, 2 * real, h->nz, hipMemcpyDeviceToHost));
  col.resize(h->nz);
  for (int i = 0; i < h->nz; ++i) col[i] = h->doublePrecision ? raw64[2 * i] : (double)raw32[2 * i];
  return 0;
}

// ---- the integrator ---------------------------------------------------------------------------------------------------------------------
struct DPStokesIntegrator {
  DPStokes *solver = nullptr;
  uammd_dpstokes_integrator_parameters par{};
  double deltaRFD = 0;
  uammd_lanczos *lanczos = nullptr;
  uammd_lanczos_f64 *lanczos64 = nullptr;
  DeviceBuffer mf, bdw, previousNoise, lastPrevious, rfd, noise, noiseRFD, shifted, plus, minus;
  int previousNoiseSize = 0;
  unsigned steps = 0, stepsRFD = 0, stepsLanczos = 0;
  // the positions the Lanczos callback applies the mobility at
  const void *dotPos = nullptr;
  int dotStride = 4, dotN = 0;
  ~DPStokesIntegrator() {
    if (lanczos) uammd_lanczos_destroy(lanczos);
    if (lanczos64) uammd_lanczos_destroy_f64(lanczos64);
    delete solver;
  }
};

static int dpsi_dot32(void *ctx, const float *v, float *mv, int n, void *stream) {
  DPStokesIntegrator *I = (DPStokesIntegrator *)ctx;
  return dps_run<float>(I->solver, (const float *)I->dotPos, I->dotStride, v, 3, I->dotN, mv, (hipStream_t)stream);
}
static int dpsi_dot64(void *ctx, const double *v, double *mv, int n, void *stream) {
  DPStokesIntegrator *I = (DPStokesIntegrator *)ctx;
  return dps_run<double>(I->solver, (const double *)I->dotPos, I->dotStride, v, 3, I->dotN, mv, (hipStream_t)stream);
}

// d_out = M^(1/2) d_w at d_pos by Lanczos (computeFluctuations, DPStokesSlab.cuh:463-478, with the caller's vector)
template <class U> static int dpsi_fluctuations(DPStokesIntegrator *I, const U *d_pos, int ps, const U *d_w, int N, U *d_out, hipStream_t st) {
  I->dotPos = d_pos;
  I->dotStride = ps;
  I->dotN = N;
  UH_CHECK(hipMemsetAsync(d_out, 0, sizeof(U) * 3 * (size_t)N, st));
  int iterations = 0;
  if (sizeof(U) == sizeof(double))
    return uammd_lanczos_run_f64(I->lanczos64, dpsi_dot64, I, (double *)d_out, (const double *)d_w, I->par.tolerance, 3 * N, st, &iterations);
  return uammd_lanczos_run(I->lanczos, dpsi_dot32, I, (float *)d_out, (const float *)d_w, (float)I->par.tolerance, 3 * N, st, &iterations);
}

// d_out = (T dt / delta) [M(q + delta W / 2) W - M(q - delta W / 2) W] (computeThermalDrift, DPStokesSlab.cuh:436-456, with the caller's W)
template <class U> static int dpsi_thermal_drift(DPStokesIntegrator *I, const U *d_pos, int ps, const U *d_w, int N, U *d_out, hipStream_t st) {
  const size_t bytes = sizeof(U) * 3 * (size_t)N;
  if (int e = I->shifted.reserve(bytes)) return e;
  if (int e = I->plus.reserve(bytes)) return e;
  if (int e = I->minus.reserve(bytes)) return e;
  const dim3 grid((N + 255) / 256), block(256);
  U *shifted = (U *)I->shifted.ptr, *plus = (U *)I->plus.ptr, *minus = (U *)I->minus.ptr;
  hipLaunchKernelGGL((k_dps_shift<U>), grid, block, 0, st, d_pos, ps, d_w, (U)(0.5 * I->deltaRFD), N, shifted);
  if (int e = dps_run<U>(I->solver, shifted, 3, d_w, 3, N, plus, st)) return e;
  hipLaunchKernelGGL((k_dps_shift<U>), grid, block, 0, st, d_pos, ps, d_w, (U)(-0.5 * I->deltaRFD), N, shifted);
  if (int e = dps_run<U>(I->solver, shifted, 3, d_w, 3, N, minus, st)) return e;
  hipLaunchKernelGGL((k_dps_drift<U>), dim3((3 * N + 255) / 256), block, 0, st, (const U *)plus, (const U *)minus,
                     (U)(I->par.dt * I->par.temperature / I->deltaRFD), 3 * N, d_out);
  UH_CHECK(hipGetLastError());
  return 0;
}

// forwardTime after the interactors have summed their forces (DPStokesSlab.cuh:528-564)
template <class U> static int dpsi_step(DPStokesIntegrator *I, U *d_pos, int ps, const U *d_force, int fs, int N, hipStream_t st) {
  const size_t bytes = sizeof(U) * 3 * (size_t)N;
  const auto &par = I->par;
  if (int e = I->mf.reserve(bytes)) return e;
  U *mf = (U *)I->mf.ptr;
  if (int e = dps_run<U>(I->solver, d_pos, ps, d_force, fs, N, mf, st)) return e;
  const dim3 grid((N + 255) / 256), block(256);
  if (par.temperature != 0) {
    if (int e = I->bdw.reserve(bytes)) return e;
    if (int e = I->rfd.reserve(bytes)) return e;
    if (int e = I->noise.reserve(bytes)) return e;
    if (int e = I->noiseRFD.reserve(bytes)) return e;
    U *bdw = (U *)I->bdw.ptr, *rfd = (U *)I->rfd.ptr, *noise = (U *)I->noise.ptr, *noiseRFD = (U *)I->noiseRFD.ptr;
    I->stepsLanczos++;
    hipLaunchKernelGGL((k_dps_noise<U>), grid, block, 0, st, noise, N, par.seed, I->stepsLanczos, (float)std::sqrt(2 * par.temperature / par.dt));
    if (int e = dpsi_fluctuations<U>(I, d_pos, ps, noise, N, bdw, st)) return e;
    U *prev = nullptr;
    if (par.useLeimkuhler) {
      if (I->previousNoiseSize != N) {
        if (int e = I->previousNoise.reserve(bytes)) return e;
        UH_CHECK(hipMemcpyAsync(I->previousNoise.ptr, bdw, bytes, hipMemcpyDeviceToDevice, st));
        I->previousNoiseSize = N;
      }
      prev = (U *)I->previousNoise.ptr;
    }
    I->stepsRFD++;
    hipLaunchKernelGGL((k_dps_noise<U>), grid, block, 0, st, noiseRFD, N, par.seedRFD, I->stepsRFD, 1.0f);
    if (int e = dpsi_thermal_drift<U>(I, d_pos, ps, noiseRFD, N, rfd, st)) return e;
    hipLaunchKernelGGL((k_dps_update<U>), grid, block, 0, st, d_pos, ps, (const U *)mf, (const U *)bdw, (const U *)prev, (const U *)rfd, (U)par.dt, N);
    if (prev) {  // (the average's other half is kept for uammd_dpstokes_integrator_last: a swap of two pointers, no copy)
      std::swap(I->previousNoise.ptr, I->lastPrevious.ptr);
      std::swap(I->previousNoise.cap, I->lastPrevious.cap);
      if (int e = I->previousNoise.reserve(bytes)) return e;
      UH_CHECK(hipMemcpyAsync(I->previousNoise.ptr, bdw, bytes, hipMemcpyDeviceToDevice, st));
    }
  } else {
    hipLaunchKernelGGL((k_dps_update<U>), grid, block, 0, st, d_pos, ps, (const U *)mf, (const U *)nullptr, (const U *)nullptr, (const U *)nullptr,
                       (U)par.dt, N);
  }
  UH_CHECK(hipGetLastError());
  I->steps++;
  return 0;
}

static int dpsi_check(DPStokesIntegrator *I, bool wantDouble, const void *pos, int ps, int N, const char *who) {
  if (!I) { set_last_error("%s: null handle", who); return -1; }
  if (int e = dp_check_precision(I->solver->doublePrecision, wantDouble, who)) return e;
  if (N < 0) { set_last_error("%s: numberParticles = %d", who, N); return -1; }
  if (ps != 3 && ps != 4) { set_last_error("%s: positions are rows of 3 or 4 reals (got %d)", who, ps); return -1; }
  if (N > 0 && !pos) { set_last_error("%s: null argument", who); return -1; }
  return 0;
}

}  // namespace uammd_hip

using namespace uammd_hip;

extern "C" {

int uammd_dpstokes_create(const uammd_dpstokes_parameters *par, int double_precision, uammd_dpstokes **out, uammd_dpstokes_info *info) {
  if (!par || (!out && !info)) { set_last_error("uammd_dpstokes_create: null argument"); return -1; }
  dps::Host cfg;
  if (int e = dps::configure(*par, cfg)) return e;
  if (info) {
    for (int a = 0; a < 3; ++a) info->cells[a] = cfg.cells[a];
    info->support = cfg.support;
    info->hx = cfg.hx; info->hy = cfg.hy; info->rmax = cfg.rmax;
    for (int a = 0; a < 3; ++a) info->beta[a] = cfg.beta[a];
  }
  if (!out) return 0;  // host only: the configuration, nothing built
  DPStokes *h = new (std::nothrow) DPStokes();
  if (!h) { set_last_error("uammd_dpstokes_create: out of host memory"); return -3; }
  h->par = *par;
  h->cfg = cfg;
  h->doublePrecision = double_precision != 0;
  const int e = h->doublePrecision ? dps_build<double>(h) : dps_build<float>(h);
  if (e) { delete h; return e; }
  *out = reinterpret_cast<uammd_dpstokes *>(h);
  return 0;
}

int uammd_dpstokes_destroy(uammd_dpstokes *h) {
  delete reinterpret_cast<DPStokes *>(h);
  return 0;
}

int uammd_dpstokes_set_option(uammd_dpstokes *h_, const char *name, int value) {
  DPStokes *h = reinterpret_cast<DPStokes *>(h_);
  if (!h || !name) { set_last_error("uammd_dpstokes_set_option: null argument"); return -1; }
  const std::string n(name);
  if (n == "simple_spread") { h->simpleSpread = value != 0; return 0; }
  if (n == "time_stages") { h->timer.enable(value != 0); return 0; }
  set_last_error("uammd_dpstokes_set_option: unknown option %s", name);
  return -1;
}

int uammd_dpstokes_mdot(uammd_dpstokes *h, const float *d_pos, int posStride, const float *d_force, int forceStride, const float *d_torque,
                        int numberParticles, float *d_mf, void *stream) {
  return dps_mdot(reinterpret_cast<DPStokes *>(h), false, d_pos, posStride, d_force, forceStride, d_torque, numberParticles, d_mf, stream,
                  "uammd_dpstokes_mdot");
}
int uammd_dpstokes_mdot_f64(uammd_dpstokes *h, const double *d_pos, int posStride, const double *d_force, int forceStride, const double *d_torque,
                            int numberParticles, double *d_mf, void *stream) {
  return dps_mdot(reinterpret_cast<DPStokes *>(h), true, d_pos, posStride, d_force, forceStride, d_torque, numberParticles, d_mf, stream,
                  "uammd_dpstokes_mdot_f64");
}

static int dps_average(uammd_dpstokes *h_, bool wantDouble, const void *pos, int ps, const void *force, int fs, int N, int direction, double *out,
                       void *stream, const char *who) {
  DPStokes *h = reinterpret_cast<DPStokes *>(h_);
  if (int e = dps_check(h, wantDouble, pos, ps, force, fs, nullptr, N, who)) return e;
  if (direction != 0 && direction != 1) { set_last_error("[DPStokesSlab] Can only average in direction X (0) or Y (1)"); return -2; }
  if (!out) { set_last_error("%s: null argument", who); return -1; }
  for (int i = 0; i < h->nz; ++i) out[i] = 0;
  if (N == 0) return 0;
  const int e = wantDouble ? dps_run<double>(h, (const double *)pos, ps, (const double *)force, fs, N, nullptr, (hipStream_t)stream)
                           : dps_run<float>(h, (const float *)pos, ps, (const float *)force, fs, N, nullptr, (hipStream_t)stream);
  if (e) return e;
  std::vector<double> col;
  if (int e2 = dps_zero_column(h, direction, col, (hipStream_t)stream)) return e2;
  const int nz = h->nz;
  for (int i = 0; i < nz; ++i) {  // DPStokesSlab.cuh:306-311
    const double arg = i * M_PI / (nz - 1);
    for (int j = 0; j < nz; ++j) out[i] += col[j] * std::cos(j * arg);
  }
  return 0;
}
int uammd_dpstokes_average_velocity(uammd_dpstokes *h, const float *d_pos, int posStride, const float *d_force, int forceStride,
                                    int numberParticles, int direction, double *averageVelocity, void *stream) {
  return dps_average(h, false, d_pos, posStride, d_force, forceStride, numberParticles, direction, averageVelocity, stream,
                     "uammd_dpstokes_average_velocity");
}
int uammd_dpstokes_average_velocity_f64(uammd_dpstokes *h, const double *d_pos, int posStride, const double *d_force, int forceStride,
                                        int numberParticles, int direction, double *averageVelocity, void *stream) {
  return dps_average(h, true, d_pos, posStride, d_force, forceStride, numberParticles, direction, averageVelocity, stream,
                     "uammd_dpstokes_average_velocity_f64");
}

// the corrected Chebyshev-space (u, v, w, p) of the last call into DEVICE memory: 4 nz nx ny complex, coefficient m of wave number s of
// component c at (c nz + m) nx ny + s (synchronises)
static int dps_fluid_cheb(uammd_dpstokes *h_, bool wantDouble, void *d_out, const char *who) {
  DPStokes *h = reinterpret_cast<DPStokes *>(h_);
  if (!h || !d_out) { set_last_error("%s: null argument", who); return -1; }
  if (int e = dp_check_precision(h->doublePrecision, wantDouble, who)) return e;
  if (!h->ran) { set_last_error("%s: nothing has run on this handle", who); return -1; }
  UH_CHECK(hipDeviceSynchronize());  // the last run may have used any stream
  const size_t real = wantDouble ? sizeof(double) : sizeof(float);
  const size_t fieldBytes = 2 * real * (size_t)h->nsys * h->nz;
  const char *base = (const char *)h->fields.ptr;
  UH_CHECK(hipMemcpy(d_out, base + fieldBytes * 11, 3 * fieldBytes, hipMemcpyDeviceToDevice));
  UH_CHECK(hipMemcpy((char *)d_out + 3 * fieldBytes, base + fieldBytes * 10, fieldBytes, hipMemcpyDeviceToDevice));
  return 0;
}
int uammd_dpstokes_fluid_cheb(uammd_dpstokes *h, float *d_out) { return dps_fluid_cheb(h, false, d_out, "uammd_dpstokes_fluid_cheb"); }
int uammd_dpstokes_fluid_cheb_f64(uammd_dpstokes *h, double *d_out) { return dps_fluid_cheb(h, true, d_out, "uammd_dpstokes_fluid_cheb_f64"); }

// particles of the last call that lay outside the slab (synchronises)
int uammd_dpstokes_outside_count(uammd_dpstokes *h_, int *count) {
  DPStokes *h = reinterpret_cast<DPStokes *>(h_);
  if (!h || !count) { set_last_error("uammd_dpstokes_outside_count: null argument"); return -1; }
  unsigned c[8];
  UH_CHECK(hipDeviceSynchronize());
  UH_CHECK(hipMemcpy(c, h->counters.ptr, sizeof(c), hipMemcpyDeviceToHost));
  *count = (int)c[0];
  return 0;
}

int uammd_dpstokes_stage_times(uammd_dpstokes *h_, double *ms) {
  DPStokes *h = reinterpret_cast<DPStokes *>(h_);
  if (!h || !ms) { set_last_error("uammd_dpstokes_stage_times: null argument"); return -1; }
  return h->timer.times(ms, "uammd_dpstokes_stage_times");
}

int uammd_dpstokes_integrator_create(const uammd_dpstokes_parameters *par, const uammd_dpstokes_integrator_parameters *ipar, int double_precision,
                                     uammd_dpstokes_integrator **out) {
  if (!par || !ipar || !out) { set_last_error("uammd_dpstokes_integrator_create: null argument"); return -1; }
  dps::Host cfg;
  if (int e = dps::configure(*par, cfg)) return e;
  if (!(ipar->dt > 0) || !std::isfinite(ipar->dt)) { set_last_error("uammd_dpstokes_integrator_create: dt = %g must be positive", ipar->dt); return -2; }
  if (!(ipar->temperature >= 0)) { set_last_error("uammd_dpstokes_integrator_create: temperature = %g", ipar->temperature); return -2; }
  double delta = ipar->deltaRFD;
  if (ipar->temperature > 0) {
    if (!(ipar->tolerance > 0)) { set_last_error("uammd_dpstokes_integrator_create: the Lanczos tolerance must be positive (got %g)", ipar->tolerance); return -2; }
    if (!(delta > 0)) {
      if (!double_precision) {
        set_last_error("[DPStokes] temperature > 0 in single precision needs deltaRFD: the reference's random-finite-difference step, 1e-6, is "
                       "below the resolution of a single-precision coordinate (about 1e-7 of its size), so q + delta W / 2 would round back to "
                       "q and the thermal drift would be rounding noise");
        return -2;
      }
      delta = 1e-6;  // DPStokesSlab.cuh:522
    }
  }
  uammd_dpstokes *solver = nullptr;
  if (int e = uammd_dpstokes_create(par, double_precision, &solver, nullptr)) return e;
  DPStokesIntegrator *I = new (std::nothrow) DPStokesIntegrator();
  if (!I) { uammd_dpstokes_destroy(solver); set_last_error("uammd_dpstokes_integrator_create: out of host memory"); return -3; }
  I->solver = reinterpret_cast<DPStokes *>(solver);
  I->par = *ipar;
  I->deltaRFD = delta;
  const int e = double_precision ? uammd_lanczos_create_f64(&I->lanczos64) : uammd_lanczos_create(&I->lanczos);
  if (e) { delete I; return e; }
  *out = reinterpret_cast<uammd_dpstokes_integrator *>(I);
  return 0;
}

int uammd_dpstokes_integrator_destroy(uammd_dpstokes_integrator *h) {
  delete reinterpret_cast<DPStokesIntegrator *>(h);
  return 0;
}

uammd_dpstokes *uammd_dpstokes_integrator_solver(uammd_dpstokes_integrator *h) {
  DPStokesIntegrator *I = reinterpret_cast<DPStokesIntegrator *>(h);
  return I ? reinterpret_cast<uammd_dpstokes *>(I->solver) : nullptr;
}

// test hook: what the last step added up, real3[N] into DEVICE memory in the handle's precision (synchronises):
// which = 0 M F, 1 the fluctuations sqrt(2 T / dt) M^(1/2) W, 2 the thermal drift, 3 the fluctuations of the step before (useLeimkuhler)
int uammd_dpstokes_integrator_last(uammd_dpstokes_integrator *h, int which, int numberParticles, void *d_out) {
  DPStokesIntegrator *I = reinterpret_cast<DPStokesIntegrator *>(h);
  if (!I || !d_out) { set_last_error("uammd_dpstokes_integrator_last: null argument"); return -1; }
  const DeviceBuffer *b = which == 0 ? &I->mf : which == 1 ? &I->bdw : which == 2 ? &I->rfd : which == 3 ? &I->lastPrevious : nullptr;
  const size_t bytes = (I->solver->doublePrecision ? sizeof(double) : sizeof(float)) * 3 * (size_t)std::max(numberParticles, 0);
  if (!b || !b->ptr || b->cap < bytes || I->steps == 0) {
    set_last_error("uammd_dpstokes_integrator_last: which = %d holds nothing for %d particles (no step yet, or temperature = 0)", which, numberParticles);
    return -1;
  }
  UH_CHECK(hipDeviceSynchronize());
  UH_CHECK(hipMemcpy(d_out, b->ptr, bytes, hipMemcpyDeviceToDevice));
  return 0;
}

int uammd_dpstokes_integrator_step(uammd_dpstokes_integrator *h, float *d_pos, int posStride, const float *d_force, int forceStride,
                                   int numberParticles, void *stream) {
  DPStokesIntegrator *I = reinterpret_cast<DPStokesIntegrator *>(h);
  if (int e = dpsi_check(I, false, d_pos, posStride, numberParticles, "uammd_dpstokes_integrator_step")) return e;
  if (int e = dps_check(I->solver, false, d_pos, posStride, d_force, forceStride, nullptr, numberParticles, "uammd_dpstokes_integrator_step")) return e;
  if (numberParticles == 0) { I->steps++; return 0; }
  return dpsi_step<float>(I, d_pos, posStride, d_force, forceStride, numberParticles, (hipStream_t)stream);
}
int uammd_dpstokes_integrator_step_f64(uammd_dpstokes_integrator *h, double *d_pos, int posStride, const double *d_force, int forceStride,
                                       int numberParticles, void *stream) {
  DPStokesIntegrator *I = reinterpret_cast<DPStokesIntegrator *>(h);
  if (int e = dpsi_check(I, true, d_pos, posStride, numberParticles, "uammd_dpstokes_integrator_step_f64")) return e;
  if (int e = dps_check(I->solver, true, d_pos, posStride, d_force, forceStride, nullptr, numberParticles, "uammd_dpstokes_integrator_step_f64")) return e;
  if (numberParticles == 0) { I->steps++; return 0; }
  return dpsi_step<double>(I, d_pos, posStride, d_force, forceStride, numberParticles, (hipStream_t)stream);
}

int uammd_dpstokes_integrator_thermal_drift(uammd_dpstokes_integrator *h, const float *d_pos, int posStride, const float *d_w, int numberParticles,
                                            float *d_drift, void *stream) {
  DPStokesIntegrator *I = reinterpret_cast<DPStokesIntegrator *>(h);
  if (int e = dpsi_check(I, false, d_pos, posStride, numberParticles, "uammd_dpstokes_integrator_thermal_drift")) return e;
  if (numberParticles == 0) return 0;
  if (!d_w || !d_drift) { set_last_error("uammd_dpstokes_integrator_thermal_drift: null argument"); return -1; }
  if (!(I->deltaRFD > 0)) { set_last_error("uammd_dpstokes_integrator_thermal_drift: the integrator was created with temperature = 0 and no deltaRFD"); return -1; }
  return dpsi_thermal_drift<float>(I, d_pos, posStride, d_w, numberParticles, d_drift, (hipStream_t)stream);
}
int uammd_dpstokes_integrator_thermal_drift_f64(uammd_dpstokes_integrator *h, const double *d_pos, int posStride, const double *d_w,
                                                int numberParticles, double *d_drift, void *stream) {
  DPStokesIntegrator *I = reinterpret_cast<DPStokesIntegrator *>(h);
  if (int e = dpsi_check(I, true, d_pos, posStride, numberParticles, "uammd_dpstokes_integrator_thermal_drift_f64")) return e;
  if (numberParticles == 0) return 0;
  if (!d_w || !d_drift) { set_last_error("uammd_dpstokes_integrator_thermal_drift_f64: null argument"); return -1; }
  if (!(I->deltaRFD > 0)) { set_last_error("uammd_dpstokes_integrator_thermal_drift_f64: the integrator was created with temperature = 0 and no deltaRFD"); return -1; }
  return dpsi_thermal_drift<double>(I, d_pos, posStride, d_w, numberParticles, d_drift, (hipStream_t)stream);
}

int uammd_dpstokes_integrator_fluctuations(uammd_dpstokes_integrator *h, const float *d_pos, int posStride, const float *d_w, int numberParticles,
                                           float *d_out, void *stream) {
  DPStokesIntegrator *I = reinterpret_cast<DPStokesIntegrator *>(h);
  if (int e = dpsi_check(I, false, d_pos, posStride, numberParticles, "uammd_dpstokes_integrator_fluctuations")) return e;
  if (numberParticles == 0) return 0;
  if (!d_w || !d_out) { set_last_error("uammd_dpstokes_integrator_fluctuations: null argument"); return -1; }
  return dpsi_fluctuations<float>(I, d_pos, posStride, d_w, numberParticles, d_out, (hipStream_t)stream);
}
int uammd_dpstokes_integrator_fluctuations_f64(uammd_dpstokes_integrator *h, const double *d_pos, int posStride, const double *d_w,
                                               int numberParticles, double *d_out, void *stream) {
  DPStokesIntegrator *I = reinterpret_cast<DPStokesIntegrator *>(h);
  if (int e = dpsi_check(I, true, d_pos, posStride, numberParticles, "uammd_dpstokes_integrator_fluctuations_f64")) return e;
  if (numberParticles == 0) return 0;
  if (!d_w || !d_out) { set_last_error("uammd_dpstokes_integrator_fluctuations_f64: null argument"); return -1; }
  return dpsi_fluctuations<double>(I, d_pos, posStride, d_w, numberParticles, d_out, (hipStream_t)stream);
}

}  // extern "C"
