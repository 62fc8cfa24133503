// Smoothed particle hydrodynamics for gfx950 (Interactor/SPH.cuh, SPH.cu, SPH/Kernel.cuh): the density and the force sums over an
// updated Verlet list.
//
//   rij = pbc(rj - ri), r = |rij|, vij = vj - vi, m = mass or 1; j runs over the list entries of i, i ITSELF INCLUDED
//   W(rij, h): q = r / h;  0 if q >= 2;  ((2 - q)^3 - [q <= 1] 4 (1 - q)^3) / (4 pi h^3)
//   G(rij, h): q = r (1/h);  0 if q >= 2;  c (3 r - 4 h) rij if q <= 1, else c (2 h - r)^2 rij;  c = -3 / (4 pi h^6)
//   rho_i = sum_j m_j W;  P_i = K (rho_i - rho0);  Pi_ij = -nu (vij . rij) / (r^2 + 0.001 h^2)
//   F_i += sum_j m_i m_j (P_i / rho_i^2 + P_j / rho_j^2 + Pi_ij) G
// G is the reference's formula as written, not the derivative of W.
//
// Shape.  The reference runs two generic list traversals with a transform between them and reads vel[index[j]],
// density[index[j]] and pressure[index[j]] per neighbour.  Here one lane owns one sorted particle in both passes, so a lane is the only
// writer of its rows: no atomics, and two sums of one state give the same bits.  Pass 1 walks the list, sums rho_i and leaves
// {v_i, P_i / rho_i^2} as ONE float4 row in list order (and m_i when masses exist), gathering the velocity from vel[groupIndex[i]] on the
// way.  Pass 2 then reads two 16-byte rows per listed neighbour, position and info, both indexed by the list entry itself.  Pass 2 needs
// every row of pass 1, hence two launches.  Both walks are k_lj_verlet's software pipeline: the entries of iteration k + 2 and the rows of
// iteration k + 1 are requested before the pairs of iteration k are evaluated.  The list holds pairs out to 1.08 x 2h; the excess falls
// out through q >= 2, where W and G reach zero continuously.
#include "verletlist.hpp"

namespace uammd_hip {

struct SPHParams {
  float h, invh, twoh;
  float wNorm;      // 1 / (4 pi h^3)
  float gNorm;      // -3 / (4 pi h^6)
  float minusNu;    // -viscosity
  float eps;        // 0.001 h^2
  float K, rho0;
};

constexpr int kSB = 128;  // lanes per workgroup
constexpr int kSU = 4;    // neighbours per pipeline stage

UH_D float sph_w(const real3f &rij, const SPHParams &p) {
  const float r = sqrtf(dot3(rij, rij));
  const float q = r / p.h;
  const float a = 2.0f - q, b = 1.0f - q;
  float w = a * a * a;
  w -= q <= 1.0f ? 4.0f * (b * b * b) : 0.0f;
  return q >= 2.0f ? 0.0f : w * p.wNorm;
}

// the list entries of rows k .. k + kSU - 1 of one particle; rows past its own count re-read its last one and carry no weight
// (a particle without a single neighbour, a NaN position, has no row 0: it gathers itself)
UH_D void sph_entries(const int *__restrict__ mine, int N, int nn, int l1, int id, int k, int (&j)[kSU]) {
#pragma unroll
  for (int u = 0; u < kSU; ++u) j[u] = nn > 0 ? mine[(size_t)min(k + u, l1) * N] : id;
}

// Pass 1.  rho_i in list order of the neighbours; out: info[id] = {v_i, P_i / rho_i^2}, sortMass[id], density / pressure in particle order
template <bool MASS>
__global__ void __launch_bounds__(kSB) k_sph_density(const float4 *__restrict__ sortPos, const int *__restrict__ groupIndex,
                                                     const int *__restrict__ neighbourList, const int *__restrict__ numberNeighbours, int N,
                                                     BoxT<float> box, SPHParams p, const float *__restrict__ vel,
                                                     const float *__restrict__ mass, float4 *__restrict__ info,
                                                     float *__restrict__ sortMass, float *__restrict__ density,
                                                     float *__restrict__ pressure) {
  const int id = (int)xcd_contiguous_block(blockIdx.x, gridDim.x) * kSB + threadIdx.x;
  if (id >= N) return;
  const int gi = groupIndex[id];
  const float4 pi = sortPos[id];
  const int nn = numberNeighbours[id];
  const int *mine = neighbourList + id;
  const int l1 = max(nn - 1, 0);
  const float vx = vel[3 * gi], vy = vel[3 * gi + 1], vz = vel[3 * gi + 2];
  int jb[kSU], jc[kSU];
  float4 cb[kSU];
  float mb[kSU];
  sph_entries(mine, N, nn, l1, id, 0, jb);
  sph_entries(mine, N, nn, l1, id, kSU, jc);
#pragma unroll
  for (int u = 0; u < kSU; ++u) {
    cb[u] = sortPos[jb[u]];
    if (MASS) mb[u] = mass[groupIndex[jb[u]]];
  }
  float rho = 0.0f;
  for (int k = 0; k < nn; k += kSU) {
    float4 c[kSU];
    float m[kSU];
    int jd[kSU];
#pragma unroll
    for (int u = 0; u < kSU; ++u) {
      c[u] = cb[u];
      if (MASS) m[u] = mb[u];
    }
    sph_entries(mine, N, nn, l1, id, k + 2 * kSU, jd);
#pragma unroll
    for (int u = 0; u < kSU; ++u) {
      cb[u] = sortPos[jc[u]];
      if (MASS) mb[u] = mass[groupIndex[jc[u]]];
    }
#pragma unroll
    for (int u = 0; u < kSU; ++u) jc[u] = jd[u];
#pragma unroll
    for (int u = 0; u < kSU; ++u) {
      const real3f rij = box.apply_pbc(real3f{c[u].x - pi.x, c[u].y - pi.y, c[u].z - pi.z});
      float w = sph_w(rij, p);
      if (MASS) w = m[u] * w;
      rho += k + u < nn ? w : 0.0f;
    }
  }
  const float P = p.K * (rho - p.rho0);
  info[id] = make_float4(vx, vy, vz, P / (rho * rho));
  if (MASS) sortMass[id] = mass[gi];
  if (density) density[gi] = rho;
  if (pressure) pressure[gi] = P;
}

// Pass 2.  Per listed neighbour one position row and one info row (and one mass when masses exist), accumulated in list order
template <bool MASS>
__global__ void __launch_bounds__(kSB) k_sph_force(const float4 *__restrict__ sortPos, const int *__restrict__ groupIndex,
                                                   const int *__restrict__ neighbourList, const int *__restrict__ numberNeighbours, int N,
                                                   BoxT<float> box, SPHParams p, const float4 *__restrict__ info,
                                                   const float *__restrict__ sortMass, float4 *__restrict__ force) {
  const int id = (int)xcd_contiguous_block(blockIdx.x, gridDim.x) * kSB + threadIdx.x;
  if (id >= N) return;
  const float4 pi = sortPos[id], vi = info[id];
  const float mi = MASS ? sortMass[id] : 1.0f;
  const int nn = numberNeighbours[id];
  const int *mine = neighbourList + id;
  const int l1 = max(nn - 1, 0);
  int jb[kSU], jc[kSU];
  float4 cb[kSU], ib[kSU];
  float mb[kSU];
  sph_entries(mine, N, nn, l1, id, 0, jb);
  sph_entries(mine, N, nn, l1, id, kSU, jc);
#pragma unroll
  for (int u = 0; u < kSU; ++u) {
    cb[u] = sortPos[jb[u]];
    ib[u] = info[jb[u]];
    if (MASS) mb[u] = sortMass[jb[u]];
  }
  float fx = 0.0f, fy = 0.0f, fz = 0.0f;
  for (int k = 0; k < nn; k += kSU) {
    float4 c[kSU], v[kSU];
    float m[kSU];
    int jd[kSU];
#pragma unroll
    for (int u = 0; u < kSU; ++u) {
      c[u] = cb[u];
      v[u] = ib[u];
      if (MASS) m[u] = mb[u];
    }
    sph_entries(mine, N, nn, l1, id, k + 2 * kSU, jd);
#pragma unroll
    for (int u = 0; u < kSU; ++u) {
      cb[u] = sortPos[jc[u]];
      ib[u] = info[jc[u]];
      if (MASS) mb[u] = sortMass[jc[u]];
    }
#pragma unroll
    for (int u = 0; u < kSU; ++u) jc[u] = jd[u];
#pragma unroll
    for (int u = 0; u < kSU; ++u) {
      const real3f rij = box.apply_pbc(real3f{c[u].x - pi.x, c[u].y - pi.y, c[u].z - pi.z});
      const real3f vij = real3f{v[u].x - vi.x, v[u].y - vi.y, v[u].z - vi.z};
      const float r2 = dot3(rij, rij);
      const float r = sqrtf(r2);
      const float q = r * p.invh;
      const float outer = p.twoh - r;
      const float g = p.gNorm * (q <= 1.0f ? fmaf(3.0f, r, -4.0f * p.h) : outer * outer);
      const float vis = p.minusNu * (dot3(vij, rij) / (r2 + p.eps));
      float s = vi.w + v[u].w + vis;
      if (MASS) s = (mi * m[u]) * s;
      s = (q >= 2.0f || k + u >= nn) ? 0.0f : s * g;
      fx = fmaf(s, rij.x, fx);
      fy = fmaf(s, rij.y, fy);
      fz = fmaf(s, rij.z, fz);
    }
  }
  const int gi = groupIndex[id];
  float4 f = force[gi];
  f.x += fx; f.y += fy; f.z += fz;
  force[gi] = f;
}

template <bool MASS>
static void sph_launch(VerletList *v, const BoxT<float> &box, const SPHParams &p, const float *vel, const float *mass, float4 *force,
                       float *density, float *pressure, hipStream_t st) {
  const int N = v->N;
  const dim3 grid((N + kSB - 1) / kSB), block(kSB);
  const float4 *sortPos = (const float4 *)v->sortPos.ptr;
  const int *index = (const int *)v->cl.index.ptr, *list = (const int *)v->neighbourList.ptr, *nn = (const int *)v->numberNeighbours.ptr;
  hipLaunchKernelGGL(k_sph_density<MASS>, grid, block, 0, st, sortPos, index, list, nn, N, box, p, vel, mass, (float4 *)v->sphInfo.ptr,
                     (float *)v->sphMass.ptr, density, pressure);
  hipLaunchKernelGGL(k_sph_force<MASS>, grid, block, 0, st, sortPos, index, list, nn, N, box, p, (const float4 *)v->sphInfo.ptr,
                     (const float *)v->sphMass.ptr, force);
}

}  // namespace uammd_hip

using namespace uammd_hip;

extern "C" {

int uammd_sph_sum_verletlist(uammd_verletlist *h, const float *d_vel, const float *d_mass, const float boxL[3], const int boxPeriodic[3],
                             float support, float viscosity, float gasStiffness, float restDensity, float *d_force, float *d_density,
                             float *d_pressure, void *stream) {
  if (!h || !d_vel || !d_force || !boxL || !boxPeriodic) { set_last_error("uammd_sph_sum_verletlist: null argument"); return -1; }
  if (!(support > 0)) { set_last_error("uammd_sph_sum_verletlist: needs support > 0"); return -1; }
  VerletList *v = reinterpret_cast<VerletList *>(h);
  const int N = v->N;
  if (N == 0) return 0;
  if (v->storedN != N || !(v->currentCutOff >= 2.0f * support)) {
    set_last_error("uammd_sph_sum_verletlist: the list was updated with cut-off %g, the kernel's support needs %g (2 x support)",
                   v->storedN == N ? v->currentCutOff : 0.0f, 2.0f * support);
    return -3;
  }
  hipStream_t st = (hipStream_t)stream;
  if (int e = v->sphInfo.reserve(sizeof(float4) * (size_t)N)) return e;   // grow only: nothing is allocated after the first sum of a size
  if (d_mass)
    if (int e = v->sphMass.reserve(sizeof(float) * (size_t)N)) return e;
  SPHParams p;
  const float hh = support;
  p.h = hh;
  p.invh = 1.0f / hh;
  p.twoh = 2.0f * hh;
  p.wNorm = 1.0f / (hh * hh * hh * 4.0f * (float)M_PI);
  const float invh3 = p.invh * p.invh * p.invh;
  p.gNorm = -(invh3 * invh3) * 3.0f / (4.0f * (float)M_PI);
  p.minusNu = -viscosity;
  p.eps = 0.001f * hh * hh;
  p.K = gasStiffness;
  p.rho0 = restDensity;
  const BoxT<float> box = make_box<float>(boxL, boxPeriodic);
  if (d_mass) sph_launch<true>(v, box, p, d_vel, d_mass, reinterpret_cast<float4 *>(d_force), d_density, d_pressure, st);
  else sph_launch<false>(v, box, p, d_vel, nullptr, reinterpret_cast<float4 *>(d_force), d_density, d_pressure, st);
  UH_CHECK(hipGetLastError());
  return 0;
}

}  // extern "C"
