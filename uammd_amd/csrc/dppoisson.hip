// Doubly periodic electrostatics in a slab (Interactor/DoublyPeriodic/DPPoissonSlab.cuh and PoissonSlab/* in the reference):
// charges between two walls at z = +-H/2, periodic in x and y, each wall a dielectric jump or a metal.
//
//   create     split from Nxy, the refusals, gt, He, the grid, the near cut-off, the tables      initialization.cu, FarField.cuh:20-131, NearField.cuh:63-147
//   far field  (1) classify  (2) spread -q of the near-wall charges, transform, solve: "outside"  FarField.cuh:133-177
//              (3) add the other charges and the images, transform, solve: "inside"               spreadInterp.cuh, BVPPoisson.cuh:38-97
//              (4, 5) both solutions at the walls, the four mismatch values, the k = 0 line       MismatchCompute.cuh
//              (6) the analytic correction at the planes, to Chebyshev space, added               CorrectionCompute.cuh
//              (7) inverse transform, gather with the Clenshaw-Curtis weights, force += q E ...   spreadInterp.cuh:317-341
//   near field cell list on (Lx, Ly, H), tabulated pair functions over r^2, wall images          NearField.cuh:149-252
//
// How the work is laid out here.
//  * One complex grid carries both spreads: the real part the near-wall charges of step (2), the imaginary part everything step (3)
//    adds.  Both are real fields, so ONE Fourier-Chebyshev transform gives both spectra: A(k) = (G(k) + conj G(-k)) / 2,
//    B(k) = (G(k) - conj G(-k)) / (2 i); the solve kernel reads the two columns and never materialises either spectrum.
//  * The spread is owner-computes: a wave owns 8 x 8 nodes x 8 planes, keeps the 2 x 8 sums of a lane's node column in registers, scans
//    the particles 64 at a time (a ballot of "does this window touch my block") and adds the hits in index order.  No atomics, no
//    memset, every node written once, and the sum order is fixed: the same bits on every run and on every stream.  A particle's
//    images share its x and y weights, so the up to three sources of a particle cost one pair of x, y weights per lane.
//    set_option("simple_spread", 1) takes the plain form instead: a lane per particle, atomic adds (the cross-check).
//  * The four output fields are real as well: (Ex + i Ey) and (Ez + i phi) go through TWO inverse transforms instead of four.
//  * Steps (2)-(6) are per wave number: k_dpp_solve solves both systems through device/BVP.hip.hpp on the bvp handle's tables and
//    evaluates both at the walls; k_dpp_correction evaluates the correction (in double, as the reference does in either build; every
//    exponent <= k He); the handle's z pass takes it to Chebyshev space; k_dpp_assemble adds it and forms the four components.
// A particle with |z| > H/2 (or a non-finite coordinate) is never spread, gathered or used as a neighbour and receives nothing; it is
// counted.  The reference has no such guard.
#include "dp_slab.hpp"
#include "../../include/uammd/device/BVP.hip.hpp"

#include <algorithm>
#include <cmath>
#include <complex>
#include <new>
#include <string>
#include <vector>

namespace uammd_hip {

namespace dpp {
constexpr int kNear = 1, kTop = 2, kBottom = 4, kOutside = dp::kOutside;
constexpr int kStages = 13;  // uammd_dppoisson_stage_times: classify, spread, forward, solve, correction, 2 z passes, assemble, 2 inverses, gather, list, near

struct Host {  // everything create() works out before it touches the device
  double split = 0, gt = 0, He = 0, Htot = 0, h = 0, hy = 0, rcut = 0, rmax = 0, kmax = 0, thetaTop = 0, thetaBot = 0;
  int cells[3] = {0, 0, 0}, ntable = 0, supportZ = 0;
  bool metTop = false, metBot = false;
};
}  // namespace dpp

template <class U> struct NearTable {
  const typename VecOf<U>::T2 *table;  // (potential, field factor) over r^2
  int Nm1;
  U rmax, interval, dr;
};

// ---- (1) classification: flags, the folded record, the window's first nodes, the float copy the cell list sorts --------------------
template <class U>
__global__ __launch_bounds__(256) void k_dpp_classify(const typename VecOf<U>::T4 *__restrict__ pos, const U *__restrict__ charge, int N,
                                                      ChebGrid<U> g, U half, U threshold, typename VecOf<U>::T4 *__restrict__ rec,
                                                      int4 *__restrict__ cellrec, float4 *__restrict__ pos32, unsigned *__restrict__ counters) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  int flags = 0;
  const bool active = i < N;
  if (active) {
    const typename VecOf<U>::T4 p = pos[i];
    const U q = charge[i];
    typename VecOf<U>::T4 r;
    r.x = r.y = r.z = r.w = U(0);
    int4 c = make_int4(0, 0, 0, 0);
    if (!dp_place(g, p.x, p.y, p.z, half, r, c)) {
      flags = dpp::kOutside;
    } else {
      r.w = q;
      if (abs_(half - abs_(p.z)) <= threshold) {  // spreadInterp.cuh:109-132
        flags = dpp::kNear;
        if (abs_(half - p.z) <= threshold) flags |= dpp::kTop;
        if (abs_(-half - p.z) <= threshold) flags |= dpp::kBottom;
      }
    }
    c.z = flags;
    rec[i] = r;
    cellrec[i] = c;
    pos32[i] = make_float4((float)r.x, (float)r.y, (float)r.z, 0.f);
  }
  const unsigned long long mNear = __ballot(active && (flags & dpp::kNear)), mOut = __ballot(active && (flags & dpp::kOutside));
  const unsigned long long mTop = __ballot(active && (flags & dpp::kTop)), mBot = __ballot(active && (flags & dpp::kBottom));
  const unsigned long long mAll = __ballot(active);
  if ((threadIdx.x & 63) == 0) {
    if (mNear) atomicAdd(&counters[0], (unsigned)__popcll(mNear));
    const unsigned far = (unsigned)(__popcll(mAll) - __popcll(mNear) - __popcll(mOut));
    if (far) atomicAdd(&counters[1], far);
    if (mTop) atomicAdd(&counters[2], (unsigned)__popcll(mTop));
    if (mBot) atomicAdd(&counters[3], (unsigned)__popcll(mBot));
    if (mOut) atomicAdd(&counters[4], (unsigned)__popcll(mOut));
  }
}

// ---- (2, 3) the spread, owner-computes (the tile and the scan: DpTile) ----------------------------------------------------------------
template <class U>
__global__ __launch_bounds__(64) void k_dpp_spread_owner(const typename VecOf<U>::T4 *__restrict__ rec, const int4 *__restrict__ cellrec, int N,
                                                         ChebGrid<U> g, U half, U ratioTop, U ratioBot, typename VecOf<U>::T2 *__restrict__ out) {
  constexpr int T = dp::kTile;
  const DpTile<U, ChebGrid<U>> tile(g);
  const int lane = tile.lane;
  U accR[T], accI[T];
#pragma unroll
  for (int p = 0; p < T; ++p) accR[p] = accI[p] = U(0);
  typename VecOf<U>::T4 r;
  int4 c;
  tile.scan(
      N,
      [&](int a) {
        r.x = r.y = r.z = r.w = U(0);
        c = make_int4(0, 0, dpp::kOutside, 0);
        if (a >= N) return false;
        c = cellrec[a];
        r = rec[a];
        if (c.z & dpp::kOutside) return false;
        const bool oz = tile.touches_z(g, r.z) || ((c.z & dpp::kTop) && tile.touches_z(g, U(2) * half - r.z)) ||
                        ((c.z & dpp::kBottom) && tile.touches_z(g, U(-2) * half - r.z));
        return oz && tile.touches_xy(g, c);
      },
      [&](int l) {
        const U px = bcast(r.x, l), py = bcast(r.y, l), pz = bcast(r.z, l), pq = bcast(r.w, l);
        const int x0 = __shfl(c.x, l, 64), y0 = __shfl(c.y, l, 64), fl = __shfl(c.z, l, 64);
        const U wxy = tile.wxy(g, px, py, x0, y0);
        U wl = U(0);
        {  // lanes 0-23 evaluate (source, plane) = (lane / 8, lane % 8)
          const int src = lane >> 3;
          U zs = pz, qs = -pq;  // every spread carries -q (spreadInterp.cuh:428-434); an image's charge is -q ratio, so it spreads +q ratio
          bool on = src == 0;
          if (src == 1) { zs = U(2) * half - pz; qs = pq * ratioTop; on = (fl & dpp::kTop) != 0; }
          if (src == 2) { zs = U(-2) * half - pz; qs = pq * ratioBot; on = (fl & dpp::kBottom) != 0; }
          if (on && tile.planeOK && src < 3) wl = qs * g.weight_z(zs, tile.zMine);
        }
        const bool nearWall = (fl & dpp::kNear) != 0;
#pragma unroll
        for (int p = 0; p < T; ++p) {
          const U w0 = bcast(wl, p), w1 = bcast(wl, T + p), w2 = bcast(wl, 2 * T + p);
          if (nearWall) accR[p] += wxy * w0;
          else accI[p] += wxy * w0;
          accI[p] += wxy * w1;
          accI[p] += wxy * w2;
        }
      });
  if (!tile.nodeOK) return;
#pragma unroll
  for (int p = 0; p < T; ++p)
    if (tile.has_plane(p)) {
      typename VecOf<U>::T2 v;
      v.x = accR[p];
      v.y = accI[p];
      out[tile.at(g, p)] = v;
    }
}

// the sources of the plain spread (k_dp_spread_simple): the charge, and its image in each wall it is near; one complex grid, the real
// part the near-wall charges themselves, the imaginary part everything else
template <class U> struct DppSource {
  static constexpr int kSources = 3, kAmplitudes = 1;
  U half, ratioTop, ratioBot;
  UH_D DpSource<U, 1> get(int n, int, const typename VecOf<U>::T4 &r, int flags) const {
    DpSource<U, 1> s{true, r.z, {-r.w}, {0}, {(n == 0 && (flags & dpp::kNear)) ? 0 : 1}};
    if (n == 1) { s.on = (flags & dpp::kTop) != 0; s.zs = U(2) * half - r.z; s.amplitude[0] = r.w * ratioTop; }
    if (n == 2) { s.on = (flags & dpp::kBottom) != 0; s.zs = U(-2) * half - r.z; s.amplitude[0] = r.w * ratioBot; }
    s.on = s.on && s.amplitude[0] != U(0);  // (a wall without a jump has images of charge zero: three times the atomic adds for nothing)
    return s;
  }
};

// ---- (2)-(5) both solves, both solutions at the walls, the mismatch ------------------------------------------------------------------
// the Chebyshev coefficients of the right-hand side of one wave number, separated from the packed spectrum on the fly
template <class U> struct DppRhs {
  using T2 = typename VecOf<U>::T2;
  const T2 *g;
  size_t nsys;
  int s, sm;
  U scale;
  bool inside;
  __device__ T2 operator[](int n) const {
    T2 f = dp_hermitian_part<U>(g, nsys, s, sm, n, 0);
    if (inside) {
      const T2 b = dp_hermitian_part<U>(g, nsys, s, sm, n, 1);
      f.x += b.x;
      f.y += b.y;
    }
    f.x *= scale;
    f.y *= scale;
    return f;
  }
};

template <class U> struct DppWalls {
  U epsTop, epsBottom, epsInside, H;
  int metTop, metBottom;
};

template <class U>
__global__ __launch_bounds__(64) void k_dpp_solve(uammd::BVP::device::Tables<U> t, const typename VecOf<U>::T2 *__restrict__ spectrum, int nx, int ny,
                                                  U invEps, U invHalfHeight, const U *__restrict__ cosTop, const U *__restrict__ cosBot,
                                                  const typename VecOf<U>::T2 *__restrict__ surfTop,
                                                  const typename VecOf<U>::T2 *__restrict__ surfBot, DppWalls<U> w,
                                                  typename VecOf<U>::T2 *__restrict__ an, typename VecOf<U>::T2 *__restrict__ cnOut,
                                                  typename VecOf<U>::T2 *__restrict__ cnIn, typename VecOf<U>::T2 *__restrict__ mismatch) {
  using T2 = typename VecOf<U>::T2;
  const int s = blockIdx.x * 64 + threadIdx.x;
  const int nsys = nx * ny;
  if (s >= nsys) return;
  const int i = s % nx, j = s / nx;
  const int sm = (i ? nx - i : 0) + nx * (j ? ny - j : 0);
  const size_t n = (size_t)nsys;
  T2 zero;
  zero.x = zero.y = U(0);
  const int nz = t.nz;
  T2 wall[2][4];  // [outside, inside][phi top, phi bottom, Ez top, Ez bottom]
  for (int which = 0; which < 2; ++which) {
    T2 *cn = which ? cnIn : cnOut;
    uammd::BVP::device::solveSystem(t, s, DppRhs<U>{spectrum, n, s, sm, invEps, which == 1}, zero, zero, Row<T2>{an + s, n}, Row<T2>{cn + s, n});
    // dphi/dz by the backward recurrence (BVPPoisson.cuh:38-56), summed into the series at the two wall angles as it goes
    T2 d2 = zero, d1 = zero, pT = zero, pB = zero, eT = zero, eB = zero;
    for (int m = nz - 1; m >= 0; --m) {
      const T2 c = cn[s + n * m];
      T2 d = zero;
      if (m <= nz - 2) {
        const T2 up = cn[s + n * (m + 1)];
        d.x = d2.x + (U(2.0) * U(m + 1) * up.x) * invHalfHeight;
        d.y = d2.y + (U(2.0) * U(m + 1) * up.y) * invHalfHeight;
      }
      d2 = d1;
      d1 = d;
      if (m == 0) { d.x *= U(0.5); d.y *= U(0.5); }
      const U ct = cosTop[m], cb = cosBot[m];
      pT.x += c.x * ct; pT.y += c.y * ct;
      pB.x += c.x * cb; pB.y += c.y * cb;
      eT.x -= d.x * ct; eT.y -= d.y * ct;
      eB.x -= d.x * cb; eB.y -= d.y * cb;
    }
    wall[which][0] = pT; wall[which][1] = pB; wall[which][2] = eT; wall[which][3] = eB;
  }
  // MismatchCompute.cuh:50-84
  const T2 sT = surfTop[s], sB = surfBot[s];
  T2 mP0, mPH, mE0, mEH;
  if (!w.metTop) {
    const U f = U(2.0) * w.epsInside / (w.epsTop + w.epsInside);
    mPH.x = wall[1][0].x - f * wall[0][0].x; mPH.y = wall[1][0].y - f * wall[0][0].y;
    mEH.x = w.epsTop * f * wall[0][2].x - w.epsInside * wall[1][2].x - sT.x;
    mEH.y = w.epsTop * f * wall[0][2].y - w.epsInside * wall[1][2].y - sT.y;
  } else {
    mEH = zero;
    mPH.x = wall[1][0].x - sT.x; mPH.y = wall[1][0].y - sT.y;
  }
  if (!w.metBottom) {
    const U f = U(2.0) * w.epsInside / (w.epsBottom + w.epsInside);
    mP0.x = wall[1][1].x - f * wall[0][1].x; mP0.y = wall[1][1].y - f * wall[0][1].y;
    mE0.x = w.epsBottom * f * wall[0][3].x - w.epsInside * wall[1][3].x + sB.x;
    mE0.y = w.epsBottom * f * wall[0][3].y - w.epsInside * wall[1][3].y + sB.y;
  } else {
    mE0 = zero;
    mP0.x = wall[1][1].x - sB.x; mP0.y = wall[1][1].y - sB.y;
  }
  mismatch[s] = mP0;
  mismatch[n + s] = mPH;
  mismatch[2 * n + s] = mE0;
  mismatch[3 * n + s] = mEH;
  if (s == 0) {  // computeLinearModeCorrection (MismatchCompute.cuh:86-115)
    T2 A0 = zero, B0 = zero;
    if (w.metTop && !w.metBottom) {
      const U eb = w.epsBottom / w.epsInside;
      const U e = U(2.0) / (eb + U(1.0));
      A0.x = (e * wall[0][3].x) * eb - mE0.x / w.epsInside;  // (the reference takes the real part of the mismatch here)
      A0.y = (e * wall[0][3].y) * eb;
      B0.x = -mPH.x - A0.x * w.H; B0.y = -mPH.y - A0.y * w.H;
    } else if (w.metTop && w.metBottom) {
      A0.x = -(mPH.x - mP0.x) / w.H; A0.y = -(mPH.y - mP0.y) / w.H;
      B0.x = -mP0.x; B0.y = -mP0.y;
    } else {
      const U et = w.epsTop / w.epsInside, eb = w.epsBottom / w.epsInside;
      const U c = U(2.0) / (et + U(1.0)), e = U(2.0) / (eb + U(1.0));
      A0.x = ((e * wall[0][3].x) * eb - mE0.x / w.epsInside + (c * wall[0][2].x) * et - mEH.x / w.epsInside) * U(0.5);
      A0.y = ((e * wall[0][3].y) * eb - mE0.y / w.epsInside + (c * wall[0][2].y) * et - mEH.y / w.epsInside) * U(0.5);
    }
    mismatch[4 * n] = A0;
    mismatch[4 * n + 1] = B0;
  }
}

// ---- (6) the analytic correction at the planes (CorrectionCompute.cuh:13-121), one lane per (wave number, plane), in double ----------
struct DppCorrection {
  double epsTop, epsBottom, epsInside, H, He, kmax;
  int metTop, metBottom;
};

template <class U>
__global__ __launch_bounds__(256) void k_dpp_correction(const typename VecOf<U>::T2 *__restrict__ mismatch, const U *__restrict__ kmod,
                                                        const U *__restrict__ zplane, int nsys, int nz, DppCorrection c,
                                                        typename VecOf<U>::T2 *__restrict__ dphi, typename VecOf<U>::T2 *__restrict__ phi) {
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (size_t)nsys * nz) return;
  const int s = (int)(idx % (size_t)nsys), plane = (int)(idx / (size_t)nsys);
  const double k = (double)kmod[s], zc = (double)zplane[plane], H = c.H;
  cd2 dz{0.0, 0.0}, ph{0.0, 0.0};
  if (fabs(zc) < 0.5 * H + c.He && k <= c.kmax) {
    const double z = zc + 0.5 * H;
    const size_t n = (size_t)nsys;
    auto load = [&](size_t at) { const typename VecOf<U>::T2 v = mismatch[at]; return cd2{(double)v.x, (double)v.y}; };
    if (k > 0) {
      const cd2 mP0 = load(s), mPH = load(n + s), mE0 = load(2 * n + s), mEH = load(3 * n + s);
      if (!c.metTop && !c.metBottom) {
        const double eb = c.epsBottom / c.epsInside, et = c.epsTop / c.epsInside;
        const double den = exp(-2.0 * H * k) * (-1.0 + eb + et - eb * et) + (1.0 + eb) * (1.0 + et);
        const cd2 a = mE0 / c.epsInside - (eb * k) * mP0, b = mEH / c.epsInside + (et * k) * mPH;
        const cd2 ezm2H = (exp(k * (z - 2.0 * H)) * (-1.0 + et)) * a, emz = (exp(-z * k) * (1.0 + et)) * a;
        const cd2 emHmz = (exp((-H - z) * k) * (-1.0 + eb)) * b, emHpz = (exp(k * (-H + z)) * (1.0 + eb)) * b;
        dz = -(ezm2H + emz + emHmz + emHpz) / den;
        ph = (-ezm2H + emz + emHmz - emHpz) / (den * k);
      } else if (c.metTop && c.metBottom) {  // (the reference's A e^{kz} + B e^{-kz} with e^{-kH} taken into both: no exponent above k He)
        const double e1 = exp(-k * H), e2 = exp(-2.0 * k * H);
        const cd2 first = (mPH - e1 * mP0) * exp(k * (z - H)) / (e2 - 1.0);
        const cd2 second = (-mP0 + e1 * mPH) / (1.0 - e2) * exp(-k * z);
        dz = k * first - k * second;
        ph = first + second;
      } else {
        const double eb = c.epsBottom / c.epsInside;
        const double e1 = exp(-k * H), e2 = exp(-2.0 * k * H);
        const double den = k * (e2 * (1.0 - eb) + (1.0 + eb));
        const cd2 a = mE0 / c.epsInside + (eb * k) * mP0;
        const cd2 AiE = (-((1.0 + eb) * k) * mPH + e1 * a) / den * exp(k * (z - H));
        const cd2 BiE = (((-1.0 + eb) * k) * mPH * e1 - a) / den * exp(-k * z);
        dz = k * AiE - k * BiE;
        ph = AiE + BiE;
      }
    } else {
      const cd2 A0 = load(4 * n), B0 = load(4 * n + 1);
      dz = A0;
      ph = A0 * z + B0;
    }
  }
  typename VecOf<U>::T2 o;
  o.x = (U)dz.x; o.y = (U)dz.y;
  dphi[idx] = o;
  o.x = (U)ph.x; o.y = (U)ph.y;
  phi[idx] = o;
}

// ---- (6, 7) add the correction, form the four components, pack them as (Ex + i Ey), (Ez + i phi) ------------------------------------
template <class U>
__global__ __launch_bounds__(64) void k_dpp_assemble(const typename VecOf<U>::T2 *__restrict__ cnIn, const typename VecOf<U>::T2 *__restrict__ corrE,
                                                     const typename VecOf<U>::T2 *__restrict__ corrP, int nsys, int nz, U invHalfHeight,
                                                     const U *__restrict__ kxPaired, const U *__restrict__ kyPaired,
                                                     typename VecOf<U>::T2 *__restrict__ exy, typename VecOf<U>::T2 *__restrict__ ezphi,
                                                     typename VecOf<U>::T2 *__restrict__ k0mode) {
  using T2 = typename VecOf<U>::T2;
  const int s = blockIdx.x * 64 + threadIdx.x;
  if (s >= nsys) return;
  const size_t n = (size_t)nsys;
  const U kx = kxPaired[s], ky = kyPaired[s];
  T2 d2, d1;
  d2.x = d2.y = d1.x = d1.y = U(0);
  for (int m = nz - 1; m >= 0; --m) {
    const size_t at = s + n * m;
    const T2 c = cnIn[at];
    T2 d;
    d.x = d.y = U(0);
    if (m <= nz - 2) {
      const T2 up = cnIn[at + n];
      d.x = d2.x + (U(2.0) * U(m + 1) * up.x) * invHalfHeight;
      d.y = d2.y + (U(2.0) * U(m + 1) * up.y) * invHalfHeight;
    }
    d2 = d1;
    d1 = d;
    if (m == 0) { d.x *= U(0.5); d.y *= U(0.5); }
    const T2 cp = corrP[at], ce = corrE[at];
    T2 p, ex, ey, ez;
    p.x = c.x + cp.x; p.y = c.y + cp.y;
    ex.x = kx * p.y; ex.y = -(kx * p.x);  // -i k phi; the unpaired Nyquist index of an even size carries kxPaired = 0 (BVPPoisson.cuh:85-92)
    ey.x = ky * p.y; ey.y = -(ky * p.x);
    ez.x = -d.x - ce.x; ez.y = -d.y - ce.y;
    T2 o;
    o.x = ex.x - ey.y; o.y = ex.y + ey.x;
    exy[at] = o;
    o.x = ez.x - p.y; o.y = ez.y + p.x;
    ezphi[at] = o;
    if (s == 0) { k0mode[4 * m] = ex; k0mode[4 * m + 1] = ey; k0mode[4 * m + 2] = ez; k0mode[4 * m + 3] = p; }
  }
}

// ---- (7) gather (k_dp_gather): force += q E, energy += q phi, field += (E, phi) ---------------------------------------------------------
template <class U> struct DppSink {
  using T4 = typename VecOf<U>::T4;
  UH_D static void outside(int, int, T4 *, U *, T4 *) {}
  UH_D static void write(int a, const T4 &r, const U *sum, T4 *force, U *energy, T4 *field) {
    const U q = r.w;
    typename VecOf<U>::T4 f = force[a];
    f.x += q * sum[0]; f.y += q * sum[1]; f.z += q * sum[2];
    force[a] = f;
    energy[a] += q * sum[3];
    if (field) {
      typename VecOf<U>::T4 e = field[a];
      e.x += sum[0]; e.y += sum[1]; e.z += sum[2]; e.w += sum[3];
      field[a] = e;
    }
  }
};

// ---- near field (NearField.cuh:149-230) ----------------------------------------------------------------------------------------------
template <class U>
__global__ __launch_bounds__(256) void k_dpp_pack_sorted(const typename VecOf<U>::T4 *__restrict__ rec, const int *__restrict__ index, int N,
                                                         typename VecOf<U>::T4 *__restrict__ packed) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < N) packed[i] = rec[index[i]];  // (a particle outside the slab carries charge 0 here)
}

template <class U> UH_D typename VecOf<U>::T2 near_table_get(const NearTable<U> &t, U rs) {
  typename VecOf<U>::T2 out;
  out.x = out.y = U(0);
  if (rs >= t.rmax) return out;
  const U r = rs * t.interval;
  if (r <= U(0)) return t.table[0];
  int i = (int)(r * U(t.Nm1));
  i = i > t.Nm1 - 1 ? t.Nm1 - 1 : i;
  const U w = (r - U(i) * t.dr) * U(t.Nm1);
  const typename VecOf<U>::T2 v0 = t.table[i], v1 = t.table[i + 1];
  out.x = v0.x + w * (v1.x - v0.x);
  out.y = v0.y + w * (v1.y - v0.y);
  return out;
}

template <class U>
__global__ __launch_bounds__(128) void k_dpp_near(const typename VecOf<U>::T4 *__restrict__ packed, const float4 *__restrict__ sortPos,
                                                  const int *__restrict__ index, const int4 *__restrict__ cellrec,
                                                  const uint *__restrict__ cellStart, const int *__restrict__ cellEnd, uint validCell, int N,
                                                  GridT<float> cgrid, U Lx, U Ly, U H, U rcut, NearTable<U> tab, U ratioTop, U ratioBot,
                                                  typename VecOf<U>::T4 *__restrict__ force, U *__restrict__ energy,
                                                  typename VecOf<U>::T4 *__restrict__ field) {
  const int id = blockIdx.x * 128 + threadIdx.x;
  if (id >= N) return;
  const int ori = index[id];
  if (cellrec[ori].z & dpp::kOutside) return;
  const typename VecOf<U>::T4 pi = packed[id];
  const float4 pf = sortPos[id];
  const int3 n = cgrid.cellDim;
  const int npx = n.x > 1 ? 3 : 1, npy = n.y > 1 ? 3 : 1, npz = n.z > 1 ? 3 : 1;
  const int3 celli = cgrid.getCell(real3f{pf.x, pf.y, pf.z});
  const U half = U(0.5) * H, rc2 = rcut * rcut;
  const bool opposite = rcut >= half;
  U tx = U(0), ty = U(0), tz = U(0), tw = U(0);
  for (int cc = 0; cc < npx * npy * npz; ++cc) {
    int3 cellj = celli;
    if (npx > 1) cellj.x += cc % 3 - 1;
    if (npy > 1) cellj.y += (cc / npx) % 3 - 1;
    if (npz > 1) cellj.z += cc / (npx * npy) - 1;
    cellj.x = cgrid.pbc_x(cellj.x);
    cellj.y = cgrid.pbc_y(cellj.y);
    if (cellj.x < 0 || cellj.x >= n.x || cellj.y < 0 || cellj.y >= n.y || cellj.z < 0 || cellj.z >= n.z) continue;
    const int icellj = cgrid.getCellIndex(cellj);
    const uint cs = cellStart[icellj];
    if (cs < validCell) continue;
    const int first = (int)(cs - validCell), last = cellEnd[icellj];
    for (int jn = first; jn < last; ++jn) {
      const typename VecOf<U>::T4 pj = packed[jn];
      const U qj = pj.w;
      if (qj == U(0)) continue;
      const U dx = ChebGrid<U>::fold(pi.x - pj.x, Lx), dy = ChebGrid<U>::fold(pi.y - pj.y, Ly);
      const U dxy2 = dx * dx + dy * dy;
      if (dxy2 >= rc2) continue;
      auto pair = [&](U zs, U qs) {
        const U dz = pi.z - zs;
        const U r2 = dxy2 + dz * dz;
        if (r2 >= rc2) return;
        const typename VecOf<U>::T2 gf = near_table_get(tab, r2);
        tx += (qs * gf.y) * dx; ty += (qs * gf.y) * dy; tz += (qs * gf.y) * dz; tw += qs * gf.x;
      };
      pair(pj.z, qj);
      if (abs_(abs_(pj.z) - half) < rcut) {
        const bool up = pj.z > U(0);
        pair((up ? H : -H) - pj.z, -qj * (pj.z < U(0) ? ratioBot : ratioTop));                    // the nearest wall's image
        if (opposite) pair((up ? -H : H) - pj.z, -qj * (pj.z < U(0) ? ratioTop : ratioBot));   // the image in the other wall
      }
    }
  }
  const U qi = pi.w;
  typename VecOf<U>::T4 f = force[ori];
  f.x += qi * tx; f.y += qi * ty; f.z += qi * tz;
  force[ori] = f;
  energy[ori] += qi * tw;
  if (field) {
    typename VecOf<U>::T4 e = field[ori];
    e.x += tx; e.y += ty; e.z += tz; e.w += tw;
    field[ori] = e;
  }
}

template <class U>
__global__ __launch_bounds__(256) void k_dpp_stage_grid(const typename VecOf<U>::T2 *__restrict__ packed, size_t total, int all, U *__restrict__ out) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const typename VecOf<U>::T2 v = packed[i];
  out[i] = all ? v.x + v.y : v.x;
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------
namespace dpp {

static double greens_near_potential(double r2, double split, double gw, double permitivity) {  // NearField.cuh:14-35
  const double gw2 = gw * gw;
  if (std::sqrt(r2) > gw * 1e-2) {
    const double r = std::sqrt(r2);
    return 1.0 / (4.0 * M_PI * permitivity * r) * (std::erf(r / (2 * gw)) - std::erf(r / std::sqrt(4 * gw2 + 1 / (split * split))));
  }
  const double pi32 = std::pow(M_PI, 1.5);
  const double invsp2 = 1.0 / (split * split);
  const double selfterm = 1.0 / (4 * pi32 * gw) - 1.0 / (2 * pi32 * std::sqrt(4 * gw2 + invsp2));
  const double r2term = 1.0 / (6.0 * pi32 * std::pow(4.0 * gw2 + invsp2, 1.5)) - 1.0 / (48.0 * pi32 * gw2 * gw);
  const double r4term = 1.0 / (640.0 * pi32 * gw2 * gw2 * gw) - 1.0 / (20.0 * pi32 * std::pow(4 * gw2 + invsp2, 2.5));
  return (selfterm + r2 * r2term + r2 * r2 * r4term) / permitivity;
}
static double greens_near_field(double r2, double split, double gw, double permitivity) {  // NearField.cuh:37-61
  const double r = std::sqrt(r2), gw2 = gw * gw;
  const double newgw = std::sqrt(gw2 + 1 / (4.0 * split * split)), newgw2 = newgw * newgw;
  if (r2 == 0) return 0;
  double fmod = 0;
  if (r > gw * 1e-2) {
    const double invrterm = std::exp(-0.25 * r2 / newgw2) / std::sqrt(M_PI * newgw2) - std::exp(-0.25 * r2 / gw2) / std::sqrt(M_PI * gw2);
    const double invr2term = std::erf(0.5 * r / newgw) - std::erf(0.5 * r / gw);
    fmod += 1 / (4 * M_PI) * (invrterm / r - invr2term / r2);
  } else {
    const double pi32 = std::pow(M_PI, 1.5);
    const double rterm = 1 / (24 * pi32) * (1.0 / (gw2 * gw) - 1 / (newgw2 * newgw));
    const double r3term = 1 / (160 * pi32) * (1.0 / (newgw2 * newgw2 * newgw) - 1.0 / (gw2 * gw2 * gw));
    fmod += r * rterm + r2 * r * r3term;
  }
  return fmod / (r * permitivity);
}

static int next_fft_size(int n) {  // nextFFTWiseSize3D (utils/Grid.cuh:140-215): 2^a 3^b 5^c 7^d 11^e, a >= 1, c <= 5, d <= 4, e <= 3, a few sizes barred
  static const int primes[5] = {2, 3, 5, 7, 11}, maxExp[5] = {64, 64, 5, 4, 3}, barred[7] = {28, 98, 150, 154, 162, 196, 242};
  for (int c = std::max(n, 1);; ++c) {
    if (c % 2) continue;
    if (std::find(barred, barred + 7, c) != barred + 7) continue;
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

// Everything the constructor decides, on the host in double (no device call): 0, or -2 with the reference's message.
static int configure(const uammd_dppoisson_parameters &p, bool doublePrecision, Host &o) {
  const double top = p.permitivity[0], bottom = p.permitivity[1], inside = p.permitivity[2];
  if (!(p.Lxy[0] > 0) || !(p.Lxy[1] > 0) || !(p.H > 0) || !(p.gw > 0) || !(p.tolerance > 0) || !(p.upsampling > 0) || !(inside > 0) ||
      !(top > 0) || !(bottom > 0) || std::isinf(inside) || !(p.numberStandardDeviations > 0)) {
    set_last_error("uammd_dppoisson_create: Lxy, H, gw, tolerance, upsampling, numberStandardDeviations and the permittivities must be positive");
    return -2;
  }
  double split = p.split;
  if (split <= 0) {  // initialization.cu:39-57
    if (p.Nxy <= 0) { set_last_error("Missing input parameters: [DPPoissonSlab] I need either split or Nxy"); return -2; }
    const double gt = p.upsampling * (p.Lxy[0] / p.Nxy);
    split = std::sqrt(1 / (4 * (gt * gt - p.gw * p.gw)));
  } else if (p.Nxy > 0) {
    set_last_error("Invalid input parameters: [DPPoissonSlab] Pass only split OR Nxy, not both");
    return -2;
  }
  const double minimumSplit = 3.2 / (p.H + p.numberStandardDeviations * p.gw), maximumSplit = 1 / (p.gw * std::sqrt(12.0));
  if (!(split >= minimumSplit) || !(split <= maximumSplit)) {
    set_last_error("Invalid splitting parameter: outside of valid range [%g:%g] (got %g)", minimumSplit, maximumSplit, split);
    return -2;
  }
  o.metTop = std::isinf(top);
  o.metBot = std::isinf(bottom);
  if (o.metBot && !o.metTop) {
    set_last_error("[DPPoissonSlab] Bottom metallic wall not implemented: if only one wall is metallic, it must be the top wall");
    return -2;
  }
  o.split = split;
  o.gt = std::sqrt(p.gw * p.gw + 1.0 / (4.0 * split * split));
  o.He = 1.25 * p.numberStandardDeviations * o.gt;
  const double minBox = std::min({p.Lxy[0], p.Lxy[1], p.H});
  if (o.He > minBox) {
    set_last_error("[DPPoissonSlab] Incompatible parameters: Extra height is too high (%g, max is %g), increase splitting parameter or lower tolerance",
                   o.He, minBox);
    return -2;
  }
  o.Htot = p.H + 6 * o.He;
  {  // proposeCellDim (FarField.cuh:20-41)
    const double h = o.gt / p.upsampling;
    int cx = std::max(16, (int)(p.Lxy[0] / h)), cy = std::max(16, (int)(p.Lxy[1] / h));
    int cz = std::max(16, (int)std::ceil(M_PI * 0.5 * o.Htot / h));
    cz = 2 * cz - 2;
    o.cells[0] = next_fft_size(cx);
    o.cells[1] = next_fft_size(cy);
    o.cells[2] = (next_fft_size(cz) + 2) / 2;
  }
  o.h = p.Lxy[0] / o.cells[0];
  o.hy = p.Lxy[1] / o.cells[1];
  if (p.support < 1 || p.support > dp::kMaxSupport || p.support > std::min(o.cells[0], o.cells[1])) {
    set_last_error("uammd_dppoisson_create: support = %d; the window takes 1 to %d nodes per axis and must fit the %d x %d plane", p.support,
                   dp::kMaxSupport, o.cells[0], o.cells[1]);
    return -2;
  }
  {  // computeCutOffDistance (NearField.cuh:63-77)
    double rn = p.gw, ratio;
    const double dr = p.gw * 0.01;
    do {
      rn += dr;
      ratio = std::fabs(greens_near_field(rn * rn, split, p.gw / std::sqrt(2.0), inside) / greens_near_field(rn * rn, 1e-10, p.gw / std::sqrt(2.0), inside));
    } while (ratio > p.tolerance);
    o.rcut = rn + p.numberStandardDeviations * p.gw;
  }
  if (o.rcut > p.H) {
    set_last_error("[DPPoissonSlab] Incompatible parameters: Close range cut off is too large (%g, max is %g), increase splitting parameter or lower "
                   "tolerance", o.rcut, p.H);
    return -2;
  }
  o.ntable = std::max(1 << 16, std::min(1 << 20, 2 * (int)(o.rcut / (p.gw * p.tolerance * 1e2))));
  o.rmax = p.support * o.h * 0.5;
  const int czmax = (int)std::ceil((o.cells[2] - 1) * (std::acos((0.5 * p.H + o.He) / (0.5 * o.Htot)) / M_PI));
  o.supportZ = 2 * czmax + 1;
  o.kmax = std::min((doublePrecision ? 709.0 : 88.0) / o.He, M_PI / o.h);
  o.thetaTop = std::acos((3 * o.He + p.H) / (0.5 * o.Htot) - 1);  // MismatchCompute.cuh:196-198
  o.thetaBot = std::acos((3 * o.He) / (0.5 * o.Htot) - 1);
  return 0;
}

}  // namespace dpp

struct DPPoisson {
  uammd_dppoisson_parameters par{};
  dpp::Host cfg;
  bool doublePrecision = false, simpleSpread = false, keepStages = false, skipNear = false;
  int nsys = 0, nz = 0;
  uammd_fct *fct = nullptr;
  uammd_bvp *bvp = nullptr;
  DeviceBuffer zplane, qw, cosTop, cosBot, kmod, kxPaired, kyPaired, surfTop, surfBot, nearTable;
  DeviceBuffer field[6], mismatch, k0mode, counters, stageGrid;
  DeviceBuffer rec, cellrec, pos32, packed;
  std::vector<std::complex<double>> hostSurf[2];
  CellList cl;
  bool ran = false;
  StageTimer<dpp::kStages> timer;  // option time_stages (uammd_dppoisson_stage_times)
  ~DPPoisson() {
    if (fct) uammd_fct_destroy(fct);
    if (bvp) uammd_bvp_destroy(bvp);
  }
};

template <class U> static int dpp_upload_surface(DPPoisson *h) {
  for (int wch = 0; wch < 2; ++wch) {
    std::vector<double> flat(2 * (size_t)h->nsys);
    for (int s = 0; s < h->nsys; ++s) { flat[2 * s] = h->hostSurf[wch][s].real(); flat[2 * s + 1] = h->hostSurf[wch][s].imag(); }
    if (int e = upload<U>(wch ? h->surfBot : h->surfTop, flat)) return e;
  }
  return 0;
}

template <class U> static ChebGrid<U> dpp_grid(const DPPoisson *h) {
  ChebGrid<U> g;
  g.nx = h->cfg.cells[0]; g.ny = h->cfg.cells[1]; g.nz = h->cfg.cells[2];
  g.support = h->par.support;
  g.Lx = (U)h->par.Lxy[0]; g.Ly = (U)h->par.Lxy[1]; g.span = (U)h->cfg.Htot;
  g.hx = (U)h->cfg.h; g.hy = (U)h->cfg.hy;
  g.invhx = (U)(1.0 / h->cfg.h); g.invhy = (U)(1.0 / h->cfg.hy);
  g.prefactor = (U)(1.0 / (h->cfg.gt * std::sqrt(2 * M_PI)));
  g.tau = (U)(-1.0 / (2.0 * h->cfg.gt * h->cfg.gt));
  g.rmax = (U)h->cfg.rmax;
  g.rcut = g.rmax * U(1.000001);
  g.zplane = (const U *)h->zplane.ptr;
  g.qw = (const U *)h->qw.ptr;
  return g;
}

template <class U> static int dpp_build(DPPoisson *h) {
  const auto &p = h->par;
  const auto &c = h->cfg;
  const int nx = c.cells[0], ny = c.cells[1], nz = c.cells[2], nsys = nx * ny;
  h->nsys = nsys;
  h->nz = nz;
  const double Hh = 0.5 * c.Htot;
  std::vector<double> zp, qw, ct(nz), cb(nz), k(nsys), kx(nsys), ky(nsys), tfi(nsys), tsi(nsys), bfi(nsys), bsi(nsys);
  dp::chebyshev_planes(nz, Hh, c.h, c.hy, zp, qw);
  for (int i = 0; i < nz; ++i) {
    ct[i] = std::cos(i * c.thetaTop);
    cb[i] = std::cos(i * c.thetaBot);
  }
  for (int s = 0; s < nsys; ++s) {
    dp::wave_vector(s, nx, ny, p.Lxy[0], p.Lxy[1], kx[s], ky[s], k[s]);
    dp::bvp_boundary_factors(k[s], Hh, tfi[s], tsi[s], bfi[s], bsi[s]);
  }
  int e = upload<U>(h->zplane, zp);
  if (!e) e = upload<U>(h->qw, qw);
  if (!e) e = upload<U>(h->cosTop, ct);
  if (!e) e = upload<U>(h->cosBot, cb);
  if (!e) e = upload<U>(h->kmod, k);
  if (!e) e = upload<U>(h->kxPaired, kx);
  if (!e) e = upload<U>(h->kyPaired, ky);
  if (e) return e;
  h->hostSurf[0].assign(nsys, 0.0);
  h->hostSurf[1].assign(nsys, 0.0);
  if (int e2 = dpp_upload_surface<U>(h)) return e2;
  {  // TabulatedFunction<real2> over r^2 in [0, rcut^2] (NearField.cuh:130-147): the abscissa is rounded to `real` before the closed forms
    std::vector<double> tab(2 * (size_t)c.ntable);
    const double rmaxT = c.rcut * c.rcut;
    for (int i = 0; i < c.ntable; ++i) {
      const double r2 = (double)(U)((i / (double)(c.ntable - 1)) * rmaxT);
      tab[2 * (size_t)i] = dpp::greens_near_potential(r2, c.split, p.gw, p.permitivity[2]);
      tab[2 * (size_t)i + 1] = dpp::greens_near_field(r2, c.split, p.gw, p.permitivity[2]);
    }
    if (int e2 = upload<U>(h->nearTable, tab)) return e2;
  }
  if (int e2 = uammd_fct_create(nx, ny, nz, h->doublePrecision, &h->fct)) return e2;
  if (int e2 = uammd_bvp_create(nsys, nz, Hh, k.data(), tfi.data(), tsi.data(), bfi.data(), bsi.data(), h->doublePrecision, &h->bvp)) return e2;
  const size_t fieldBytes = 2 * sizeof(U) * (size_t)nsys * nz;
  for (auto &f : h->field)
    if (int e2 = f.reserve(fieldBytes)) return e2;
  if (int e2 = h->mismatch.reserve(2 * sizeof(U) * (4 * (size_t)nsys + 2))) return e2;
  if (int e2 = h->k0mode.reserve(2 * sizeof(U) * 4 * (size_t)nz)) return e2;
  if (int e2 = h->counters.reserve(8 * sizeof(unsigned))) return e2;
  UH_CHECK(hipMemset(h->counters.ptr, 0, 8 * sizeof(unsigned)));
  UH_CHECK(hipMemset(h->k0mode.ptr, 0, 2 * sizeof(U) * 4 * (size_t)nz));
  UH_CHECK(hipMemset(h->mismatch.ptr, 0, 2 * sizeof(U) * (4 * (size_t)nsys + 2)));
  return 0;
}

template <class U> static U image_ratio(double wall, double inside) {  // spreadInterp.cuh:94-106, NearField.cuh:175-178
  return std::isinf(wall) ? U(1) : (U)((wall - inside) / (wall + inside));
}

// FarField::compute then NearField::compute (DPPoissonSlab.cuh:47-81); field may be null
template <class U>
static int dpp_run(DPPoisson *h, const void *d_pos, const void *d_charge, int N, void *d_force, void *d_energy, void *d_field, hipStream_t st) {
  using T2 = typename VecOf<U>::T2;
  using T4 = typename VecOf<U>::T4;
  const auto &p = h->par;
  const auto &c = h->cfg;
  const ChebGrid<U> g = dpp_grid<U>(h);
  const int nsys = h->nsys, nz = h->nz;
  const U half = (U)(0.5 * p.H);
  const U ratioTop = image_ratio<U>(p.permitivity[0], p.permitivity[2]), ratioBot = image_ratio<U>(p.permitivity[1], p.permitivity[2]);
  if (int e = h->rec.reserve(sizeof(T4) * (size_t)N)) return e;
  if (int e = h->cellrec.reserve(sizeof(int4) * (size_t)N)) return e;
  if (int e = h->pos32.reserve(sizeof(float4) * (size_t)N)) return e;
  if (int e = h->packed.reserve(sizeof(T4) * (size_t)N)) return e;
  T2 *B[6];
  for (int i = 0; i < 6; ++i) B[i] = (T2 *)h->field[i].ptr;
  const T4 *rec = (const T4 *)h->rec.ptr;
  const int4 *cellrec = (const int4 *)h->cellrec.ptr;
  h->timer.reset();
  auto mark = [&]() { return h->timer.mark(st); };
  if (int e = mark()) return e;
  // (1)
  UH_CHECK(hipMemsetAsync(h->counters.ptr, 0, 8 * sizeof(unsigned), st));
  hipLaunchKernelGGL((k_dpp_classify<U>), dim3((N + 255) / 256), dim3(256), 0, st, (const T4 *)d_pos, (const U *)d_charge, N, g, half,
                     (U)(2 * c.He), (T4 *)h->rec.ptr, (int4 *)h->cellrec.ptr, (float4 *)h->pos32.ptr, (unsigned *)h->counters.ptr);
  if (int e = mark()) return e;
  // (2, 3) one grid: real part the near-wall charges, imaginary part the rest and the images
  if (h->simpleSpread) {
    UH_CHECK(hipMemsetAsync(B[0], 0, sizeof(T2) * (size_t)nsys * nz, st));
    hipLaunchKernelGGL((k_dp_spread_simple<U, ChebGrid<U>, DppSource<U>>), dim3((N + 63) / 64), dim3(64), 0, st, rec, cellrec, N, g,
                       DppSource<U>{half, ratioTop, ratioBot}, (U *)B[0], (U *)nullptr);
  } else {
    hipLaunchKernelGGL((k_dpp_spread_owner<U>), dp_owner_grid(g.nx, g.ny, nz), dim3(64), 0, st, rec, cellrec, N, g, half, ratioTop, ratioBot, B[0]);
  }
  UH_CHECK(hipGetLastError());
  if (int e = mark()) return e;
  if (h->keepStages) {
    if (int e = h->stageGrid.reserve(sizeof(T2) * (size_t)nsys * nz)) return e;
    UH_CHECK(hipMemcpyAsync(h->stageGrid.ptr, B[0], sizeof(T2) * (size_t)nsys * nz, hipMemcpyDeviceToDevice, st));
  }
  auto fctRun = [&](bool planes, const T2 *in, T2 *out, int dir) { return fct_run<U>(h->fct, planes, in, out, dir, st); };
  if (int e = fctRun(true, B[0], B[1], UAMMD_FCT_FORWARD)) return e;  // spectrum in B1
  if (int e = mark()) return e;
  // (2)-(5): an in B0 (the grid is spent), outside in B2, inside in B3
  uammd_bvp_tables bt;
  if (int e = uammd_bvp_device_tables(h->bvp, &bt)) return e;
  const double Hh = 0.5 * c.Htot;
  const auto tables = uammd::BVP::device::Tables<U>::over((const U *)bt.d_tables, nsys, nz, (U)(Hh * Hh));
  DppWalls<U> walls{(U)p.permitivity[0], (U)p.permitivity[1], (U)p.permitivity[2], (U)p.H, c.metTop ? 1 : 0, c.metBot ? 1 : 0};
  hipLaunchKernelGGL((k_dpp_solve<U>), dim3((nsys + 63) / 64), dim3(64), 0, st, tables, (const T2 *)B[1], g.nx, g.ny, (U)(1.0 / p.permitivity[2]),
                     (U)(1.0 / Hh), (const U *)h->cosTop.ptr, (const U *)h->cosBot.ptr, (const T2 *)h->surfTop.ptr, (const T2 *)h->surfBot.ptr,
                     walls, B[0], B[2], B[3], (T2 *)h->mismatch.ptr);
  if (int e = mark()) return e;
  // (6) correction at the planes into B4, B5; to Chebyshev space in B0, B1
  DppCorrection corr{p.permitivity[0], p.permitivity[1], p.permitivity[2], p.H, c.He, c.kmax, c.metTop ? 1 : 0, c.metBot ? 1 : 0};
  const size_t total = (size_t)nsys * nz;
  hipLaunchKernelGGL((k_dpp_correction<U>), dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, (const T2 *)h->mismatch.ptr,
                     (const U *)h->kmod.ptr, (const U *)h->zplane.ptr, nsys, nz, corr, B[4], B[5]);
  UH_CHECK(hipGetLastError());
  if (int e = mark()) return e;
  if (int e = fctRun(false, B[4], B[0], UAMMD_FCT_FORWARD)) return e;
  if (int e = mark()) return e;
  if (int e = fctRun(false, B[5], B[1], UAMMD_FCT_FORWARD)) return e;
  if (int e = mark()) return e;
  // the four components, packed in B4 (Ex + i Ey) and B5 (Ez + i phi); inverse into B2 and B0
  hipLaunchKernelGGL((k_dpp_assemble<U>), dim3((nsys + 63) / 64), dim3(64), 0, st, (const T2 *)B[3], (const T2 *)B[0], (const T2 *)B[1], nsys, nz,
                     (U)(1.0 / Hh), (const U *)h->kxPaired.ptr, (const U *)h->kyPaired.ptr, B[4], B[5], (T2 *)h->k0mode.ptr);
  UH_CHECK(hipGetLastError());
  if (int e = mark()) return e;
  if (int e = fctRun(true, B[4], B[2], UAMMD_FCT_INVERSE)) return e;
  if (int e = mark()) return e;
  if (int e = fctRun(true, B[5], B[0], UAMMD_FCT_INVERSE)) return e;
  if (int e = mark()) return e;
  // (7)
  hipLaunchKernelGGL((k_dp_gather<U, ChebGrid<U>, 4, DppSink<U>, T4, U, T4>), dim3((N + 3) / 4), dim3(256), 0, st, rec, cellrec, N, g,
                     (const T2 *)B[2], (const T2 *)B[0], (T4 *)d_force, (U *)d_energy, (T4 *)d_field);
  UH_CHECK(hipGetLastError());
  if (int e = mark()) return e;
  h->ran = true;
  if (h->skipNear) return 0;
  // near field: the list on (Lx, Ly, H) periodic in x and y (NearField.cuh:232-252).  The list sorts a float copy, so its cells are a
  // hair wider than the cut-off and its box a hair taller than the slab (a charge exactly on a wall stays inside)
  const float rcl = (float)(c.rcut * 1.0001);
  const float L[3] = {(float)p.Lxy[0], (float)p.Lxy[1], (float)(p.H * 1.0001)}, rc3[3] = {rcl, rcl, rcl};
  const int per[3] = {1, 1, 0};
  int cd[3], gper[3];
  float gL[3];
  if (int e = uammd_celllist_create_grid(L, per, rc3, cd, gL, gper)) return e;
  if (int e = h->cl.update((const float4 *)h->pos32.ptr, N, gL, gper, cd, st)) return e;
  hipLaunchKernelGGL((k_dpp_pack_sorted<U>), dim3((N + 255) / 256), dim3(256), 0, st, rec, (const int *)h->cl.index.ptr, N, (T4 *)h->packed.ptr);
  if (int e = mark()) return e;
  NearTable<U> tab{(const T2 *)h->nearTable.ptr, c.ntable - 1, (U)(c.rcut * c.rcut), (U)(1.0 / (c.rcut * c.rcut)), (U)(1.0 / (c.ntable - 1))};
  hipLaunchKernelGGL((k_dpp_near<U>), dim3((N + 127) / 128), dim3(128), 0, st, (const T4 *)h->packed.ptr, (const float4 *)h->cl.sortPos.ptr,
                     (const int *)h->cl.index.ptr, cellrec, (const uint *)h->cl.cellStart.ptr, (const int *)h->cl.cellEnd.ptr, h->cl.validCell, N,
                     h->cl.grid, (U)p.Lxy[0], (U)p.Lxy[1], (U)p.H, (U)c.rcut, tab, ratioTop, ratioBot, (T4 *)d_force, (U *)d_energy, (T4 *)d_field);
  UH_CHECK(hipGetLastError());
  if (int e = mark()) return e;
  return 0;
}

static int dpp_entry(uammd_dppoisson *h_, bool wantDouble, const void *pos, const void *charge, int N, void *force, void *energy, void *field,
                     bool needField, int virial, void *stream, const char *who) {
  DPPoisson *h = reinterpret_cast<DPPoisson *>(h_);
  if (!h) { set_last_error("%s: null handle", who); return -1; }
  if (virial) { set_last_error("[Poisson] not implemented (%s: the virial)", who); return -3; }
  if (int e = dp_check_precision(h->doublePrecision, wantDouble, who)) return e;
  if (N < 0) { set_last_error("%s: numberParticles = %d", who, N); return -1; }
  if (N == 0) return 0;
  if (!pos || !charge || !force || !energy || (needField && !field)) { set_last_error("%s: null argument", who); return -1; }
  return wantDouble ? dpp_run<double>(h, pos, charge, N, force, energy, field, (hipStream_t)stream)
                    : dpp_run<float>(h, pos, charge, N, force, energy, field, (hipStream_t)stream);
}

}  // namespace uammd_hip

using namespace uammd_hip;

extern "C" {

int uammd_dppoisson_create(const uammd_dppoisson_parameters *par, int double_precision, uammd_dppoisson **out, uammd_dppoisson_info *info) {
  if (!par) { set_last_error("uammd_dppoisson_create: null argument"); return -1; }
  if (!out && !info) { set_last_error("uammd_dppoisson_create: null argument"); return -1; }
  dpp::Host cfg;
  if (int e = dpp::configure(*par, double_precision != 0, cfg)) return e;
  if (info) {
    for (int a = 0; a < 3; ++a) info->cells[a] = cfg.cells[a];
    info->He = cfg.He; info->gt = cfg.gt; info->h = cfg.h;
    info->support = par->support; info->supportZ = cfg.supportZ;
    info->nearFieldCutOff = cfg.rcut; info->nTable = cfg.ntable; info->kmax = cfg.kmax; info->split = cfg.split;
  }
  if (!out) return 0;  // host only: the configuration, nothing built
  DPPoisson *h = new (std::nothrow) DPPoisson();
  if (!h) { set_last_error("uammd_dppoisson_create: out of host memory"); return -3; }
  h->par = *par;
  h->cfg = cfg;
  h->doublePrecision = double_precision != 0;
  const int e = h->doublePrecision ? dpp_build<double>(h) : dpp_build<float>(h);
  if (e) { delete h; return e; }
  *out = reinterpret_cast<uammd_dppoisson *>(h);
  return 0;
}

int uammd_dppoisson_destroy(uammd_dppoisson *h) {
  delete reinterpret_cast<DPPoisson *>(h);
  return 0;
}

int uammd_dppoisson_set_option(uammd_dppoisson *h_, const char *name, int value) {
  DPPoisson *h = reinterpret_cast<DPPoisson *>(h_);
  if (!h || !name) { set_last_error("uammd_dppoisson_set_option: null argument"); return -1; }
  const std::string n(name);
  if (n == "simple_spread") { h->simpleSpread = value != 0; return 0; }
  if (n == "keep_stages") { h->keepStages = value != 0; return 0; }
  if (n == "skip_near_field") { h->skipNear = value != 0; return 0; }
  if (n == "time_stages") { h->timer.enable(value != 0); return 0; }
  set_last_error("uammd_dppoisson_set_option: unknown option %s", name);
  return -1;
}

// Host arrays of nx ny samples at x = (i / nx - 1/2) Lx, y = (j / ny - 1/2) Ly, element (i, j) at i + nx j; NULL means zeros.  The spectrum
// is normalised like the library's forward transform (divided by nx ny; the reference keeps it unnormalised like its grids).
int uammd_dppoisson_set_surface_values(uammd_dppoisson *h_, const double *top, const double *bottom) {
  DPPoisson *h = reinterpret_cast<DPPoisson *>(h_);
  if (!h) { set_last_error("uammd_dppoisson_set_surface_values: null handle"); return -1; }
  const int nx = h->cfg.cells[0], ny = h->cfg.cells[1];
  std::vector<std::complex<double>> wxt(nx), wyt(ny), rows((size_t)nx * ny);
  for (int a = 0; a < nx; ++a) wxt[a] = std::polar(1.0, -2 * M_PI * a / nx);
  for (int a = 0; a < ny; ++a) wyt[a] = std::polar(1.0, -2 * M_PI * a / ny);
  for (int wch = 0; wch < 2; ++wch) {
    const double *v = wch ? bottom : top;
    auto &spec = h->hostSurf[wch];
    spec.assign((size_t)nx * ny, 0.0);
    if (!v) continue;
    for (int j = 0; j < ny; ++j)  // along x
      for (int kxi = 0; kxi < nx; ++kxi) {
        std::complex<double> acc = 0;
        for (int i = 0; i < nx; ++i) acc += v[i + (size_t)nx * j] * wxt[(int)(((long long)i * kxi) % nx)];
        rows[kxi + (size_t)nx * j] = acc;
      }
    for (int kyi = 0; kyi < ny; ++kyi)  // along y
      for (int kxi = 0; kxi < nx; ++kxi) {
        std::complex<double> acc = 0;
        for (int j = 0; j < ny; ++j) acc += rows[kxi + (size_t)nx * j] * wyt[(int)(((long long)j * kyi) % ny)];
        spec[kxi + (size_t)nx * kyi] = acc / (double)((size_t)nx * ny);
      }
    // the samples are real: make the spectrum conjugate-symmetric to the last bit (the packed inverse transform relies on it)
    for (int j = 0; j < ny; ++j)
      for (int i = 0; i < nx; ++i) {
        const size_t s = i + (size_t)nx * j, sm = (i ? nx - i : 0) + (size_t)nx * (j ? ny - j : 0);
        if (s <= sm) {
          const std::complex<double> m = 0.5 * (spec[s] + std::conj(spec[sm]));
          spec[s] = m;
          spec[sm] = std::conj(m);
        }
      }
  }
  UH_CHECK(hipDeviceSynchronize());
  return h->doublePrecision ? dpp_upload_surface<double>(h) : dpp_upload_surface<float>(h);
}

// DPPoissonSlab::setSurfaceValuesZeroModeFourier (FarField.cuh:179-181): only the k = 0 entries change
int uammd_dppoisson_set_surface_zero_mode(uammd_dppoisson *h_, double top, double bottom) {
  DPPoisson *h = reinterpret_cast<DPPoisson *>(h_);
  if (!h) { set_last_error("uammd_dppoisson_set_surface_zero_mode: null handle"); return -1; }
  h->hostSurf[0][0] = top;
  h->hostSurf[1][0] = bottom;
  UH_CHECK(hipDeviceSynchronize());
  return h->doublePrecision ? dpp_upload_surface<double>(h) : dpp_upload_surface<float>(h);
}

int uammd_dppoisson_sum(uammd_dppoisson *h, const float *d_pos, const float *d_charge, int numberParticles, float *d_force, float *d_energy,
                        int virial, void *stream) {
  return dpp_entry(h, false, d_pos, d_charge, numberParticles, d_force, d_energy, nullptr, false, virial, stream, "uammd_dppoisson_sum");
}
int uammd_dppoisson_sum_f64(uammd_dppoisson *h, const double *d_pos, const double *d_charge, int numberParticles, double *d_force, double *d_energy,
                            int virial, void *stream) {
  return dpp_entry(h, true, d_pos, d_charge, numberParticles, d_force, d_energy, nullptr, false, virial, stream, "uammd_dppoisson_sum_f64");
}
int uammd_dppoisson_field_potential(uammd_dppoisson *h, const float *d_pos, const float *d_charge, int numberParticles, float *d_fieldPotential,
                                    float *d_force, float *d_energy, void *stream) {
  return dpp_entry(h, false, d_pos, d_charge, numberParticles, d_force, d_energy, d_fieldPotential, true, 0, stream,
                   "uammd_dppoisson_field_potential");
}
int uammd_dppoisson_field_potential_f64(uammd_dppoisson *h, const double *d_pos, const double *d_charge, int numberParticles,
                                        double *d_fieldPotential, double *d_force, double *d_energy, void *stream) {
  return dpp_entry(h, true, d_pos, d_charge, numberParticles, d_force, d_energy, d_fieldPotential, true, 0, stream,
                   "uammd_dppoisson_field_potential_f64");
}

// the corrected k = 0 column of the last call: nz x (Ex, Ey, Ez, phi) complex, as 8 nz host doubles (synchronises)
int uammd_dppoisson_get_k0_mode(uammd_dppoisson *h_, double *out) {
  DPPoisson *h = reinterpret_cast<DPPoisson *>(h_);
  if (!h || !out) { set_last_error("uammd_dppoisson_get_k0_mode: null argument"); return -1; }
  const size_t n = 8 * (size_t)h->nz;
  UH_CHECK(hipDeviceSynchronize());
  if (h->doublePrecision) {
    UH_CHECK(hipMemcpy(out, h->k0mode.ptr, n * sizeof(double), hipMemcpyDeviceToHost));
  } else {
    std::vector<float> tmp(n);
    UH_CHECK(hipMemcpy(tmp.data(), h->k0mode.ptr, n * sizeof(float), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < n; ++i) out[i] = tmp[i];
  }
  return 0;
}

// particles of the last call that lay outside the slab (synchronises)
int uammd_dppoisson_outside_count(uammd_dppoisson *h_, int *count) {
  DPPoisson *h = reinterpret_cast<DPPoisson *>(h_);
  if (!h || !count) { set_last_error("uammd_dppoisson_outside_count: null argument"); return -1; }
  unsigned c[8];
  UH_CHECK(hipDeviceSynchronize());
  UH_CHECK(hipMemcpy(c, h->counters.ptr, sizeof(c), hipMemcpyDeviceToHost));
  *count = (int)c[4];
  return 0;
}

// test hook: "grid_near" / "grid_all" (nx ny nz reals, needs option keep_stages) and "mismatch" (4 nsys + 2 complex: mP0, mPH, mE0, mEH per wave
// number, component c of wave number s at c nsys + s, then the k = 0 line A0, B0) of the last call, into device memory
int uammd_dppoisson_get_stage(uammd_dppoisson *h_, const char *name, void *d_out) {
  DPPoisson *h = reinterpret_cast<DPPoisson *>(h_);
  if (!h || !name || !d_out) { set_last_error("uammd_dppoisson_get_stage: null argument"); return -1; }
  if (!h->ran) { set_last_error("uammd_dppoisson_get_stage: nothing has run on this handle"); return -1; }
  UH_CHECK(hipDeviceSynchronize());  // the last run may have used any stream
  const std::string n(name);
  const size_t total = (size_t)h->nsys * h->nz;
  const size_t real = h->doublePrecision ? sizeof(double) : sizeof(float);
  if (n == "mismatch") {
    UH_CHECK(hipMemcpy(d_out, h->mismatch.ptr, 2 * real * (4 * (size_t)h->nsys + 2), hipMemcpyDeviceToDevice));
    return 0;
  }
  if (n == "grid_near" || n == "grid_all") {
    if (!h->keepStages || !h->stageGrid.ptr) { set_last_error("uammd_dppoisson_get_stage: set option keep_stages before the call"); return -1; }
    const int all = n == "grid_all";
    if (h->doublePrecision)
      hipLaunchKernelGGL((k_dpp_stage_grid<double>), dim3((unsigned)((total + 255) / 256)), dim3(256), 0, 0, (const double2 *)h->stageGrid.ptr, total, all,
                         (double *)d_out);
    else
      hipLaunchKernelGGL((k_dpp_stage_grid<float>), dim3((unsigned)((total + 255) / 256)), dim3(256), 0, 0, (const float2 *)h->stageGrid.ptr, total, all,
                         (float *)d_out);
    UH_CHECK(hipGetLastError());
    UH_CHECK(hipDeviceSynchronize());
    return 0;
  }
  set_last_error("uammd_dppoisson_get_stage: unknown stage %s", name);
  return -1;
}

// Milliseconds each stage of the last run took, from device events recorded between the stage launches while option time_stages is set
// (synchronises).  ms[13]: classify, spread, forward transform, solve (both systems, both at the walls, the mismatch), correction, z pass of
// d phi / dz, z pass of phi, assemble, inverse transform of (Ex, Ey), of (Ez, phi), gather, cell list + pack, near field; a stage that did
// not run (skip_near_field) reads 0.
int uammd_dppoisson_stage_times(uammd_dppoisson *h_, double *ms) {
  DPPoisson *h = reinterpret_cast<DPPoisson *>(h_);
  if (!h || !ms) { set_last_error("uammd_dppoisson_stage_times: null argument"); return -1; }
  return h->timer.times(ms, "uammd_dppoisson_stage_times");
}

}  // extern "C"
