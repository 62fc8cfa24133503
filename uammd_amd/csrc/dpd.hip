// Dissipative particle dynamics pair force for gfx950 (Interactor/Potential/DPD.cuh:121-152, ForceTransverser::compute), over a built
// cell list (PairForces.cu:55-68) and over all pairs (PairForces.cu:49-53, the box <= 3 rc fallback).
//
//   rij = pbc(ri - rj), vij = vi - vj, r = |rij|; nothing if r == 0 or 1/r <= 1/rc
//   wr = 1 - r/rc;  Fc = A wr / r;  Fd = -g wr^2 (rij . vij) / r^2;  Fr = xi sigma sqrt(g) wr / r
//   xi = Saru(ij, seed, step).gf(0, 1).x,  ij = min(i, j) + N max(i, j)  (particle indices; unsigned arithmetic: DESIGN.md 12)
//   F_i += (Fc + Fd + Fr) rij
//
// Shape.  One lane per particle in list order, so a lane is the only writer of its force row: no atomics, and two sums
// of the same state give the same bits.  At rho = 3, rc = 1 a particle sees 81 candidates in its 27 cells and keeps 12.6 of them, and
// an accepted pair costs ~10x a rejected one (three-word Saru seeding, two draws, log, sqrt, sin against a distance test).  Evaluating
// inside the candidate loop would run the generator for the whole wave whenever ANY lane accepts, i.e. on almost every candidate.  The
// walk is therefore split as in the LJ kernels: the distance test compacts the hits of each lane into a per-lane FIFO in LDS, and the
// wave drains the FIFOs together when one fills up and at the end of the walk — the generator then runs max-over-lanes(hits) times per
// wave instead of 81.  Velocities and keys are gathered ONCE per sum into list order (float4 {v, key} in a scratch array the handle
// owns), so that the drain reads one 16-byte row next to the position row instead of vel[index[j]].
#include "celllist.hpp"
#include "lj_common.hpp"
#include "saru.hpp"

namespace uammd_hip {

struct DPDParams {
  float invrc, rc2Filter;  // 1 / rc; rc^2 widened by a few ulp for the compaction (the exact 1/r <= 1/rc test decides in the drain)
  float A, gamma, sigmaSqrtGamma;
  uint seed, step, N;
};

// DPD.cuh:121-152 for one pair that has passed the coarse distance filter; ki, kj are the particles' indices (the generator's key)
UH_D void dpd_pair(float &fx, float &fy, float &fz, const real3f &rij, float r2, const real3f &vij, uint ki, uint kj, const DPDParams &p) {
  if (r2 == 0.0f) return;
  const float rmod = sqrtf(r2);
  const float invrmod = 1.0f / rmod;
  if (invrmod <= p.invrc) return;
  const float wr = 1.0f - rmod * p.invrc;
  const float Fc = p.A * wr * invrmod;
  const float Fd = -p.gamma * (wr * wr) * invrmod * invrmod * dot3(rij, vij);
  const uint lo = ki < kj ? ki : kj, hi = ki < kj ? kj : ki;
#if defined(UAMMD_DPD_NO_DRAW)   // diagnostic build (tools/time_dpd.py): what the kernel costs without the generator
  const float xi = 0.5f + 1e-9f * (float)(lo + p.N * hi);
#else
  Saru rng(lo + p.N * hi, p.seed, p.step);
  const float xi = rng.gf_fast_x(0.0f, 1.0f);
#endif
  const float Fr = xi * (p.sigmaSqrtGamma * wr * invrmod);
  const float f = Fc + Fd + Fr;
  fx = fmaf(f, rij.x, fx);
  fy = fmaf(f, rij.y, fy);
  fz = fmaf(f, rij.z, fz);
}

constexpr int kDB = 128;    // lanes per workgroup
constexpr int kDCap = 32;   // FIFO entries per lane (LDS: 16 KB per workgroup)

// velocities and keys into list order: out[s] = {vel[ori], ori}, ori = globalIndex[index[s]]
__global__ void __launch_bounds__(256) k_dpd_gather(const int *__restrict__ index, const int *__restrict__ globalIndex,
                                                    const float *__restrict__ vel, float4 *__restrict__ out, int N) {
  const int s = blockIdx.x * 256 + threadIdx.x;
  if (s >= N) return;
  const int gi = index[s];
  const int ori = globalIndex ? globalIndex[gi] : gi;
  out[s] = make_float4(vel[3 * ori], vel[3 * ori + 1], vel[3 * ori + 2], __uint_as_float((uint)ori));
}

UH_D void dpd_drain(float &fx, float &fy, float &fz, const uint *q, int &n, const float4 *__restrict__ P, const float4 *__restrict__ V,
                    const float4 &pi, const float4 &vi, const BoxT<float> &box, const DPDParams &p) {
  for (int k = 0; __any(k < n); ++k) {
    if (k < n) {
      const uint j = q[k * kDB];
      const float4 pj = P[j], vj = V[j];
      const real3f rij = box.apply_pbc(real3f{pi.x - pj.x, pi.y - pj.y, pi.z - pj.z});
      dpd_pair(fx, fy, fz, rij, dot3(rij, rij), real3f{vi.x - vj.x, vi.y - vj.y, vi.z - vj.z}, __float_as_uint(vi.w), __float_as_uint(vj.w), p);
    }
  }
  n = 0;
}

__global__ void __launch_bounds__(kDB) k_dpd_celllist(ListView cl, GridT<float> grid, BoxT<float> box, const float4 *__restrict__ sortVel,
                                                      DPDParams p, float4 *__restrict__ force) {
  __shared__ uint fifo[kDCap * kDB];
  const int id = (int)xcd_contiguous_block(blockIdx.x, gridDim.x) * kDB + threadIdx.x;
  if (id >= cl.N) return;   // (no workgroup barrier below: the wave-level votes only count the lanes that are left)
  const float4 pi = cl.sortPos[id], vi = sortVel[id];
  uint *q = fifo + threadIdx.x;
  int n = 0;
  float fx = 0.f, fy = 0.f, fz = 0.f;
  const int3 nc = grid.cellDim;
  const int npx = nc.x > 1 ? 3 : 1, npy = nc.y > 1 ? 3 : 1, npz = nc.z > 1 ? 3 : 1;
  const int3 celli = grid.getCell(real3f{pi.x, pi.y, pi.z});
  for (int cc = 0; cc < npx * npy * npz; ++cc) {
    int3 cellj = celli;
    if (npx > 1) cellj.x += cc % 3 - 1;
    if (npy > 1) cellj.y += (cc / npx) % 3 - 1;
    if (npz > 1) cellj.z += cc / (npx * npy) - 1;
    cellj.x = grid.pbc_x(cellj.x);
    cellj.y = grid.pbc_y(cellj.y);
    cellj.z = grid.pbc_z(cellj.z);
    // outside a non periodic box: no such cell
    const bool exists = !(cellj.x < 0 || cellj.x >= nc.x || cellj.y < 0 || cellj.y >= nc.y || cellj.z < 0 || cellj.z >= nc.z);
    int first = 0, last = 0;
    if (exists) {
      const int icellj = grid.getCellIndex(cellj);
      if (cl.cellRange) {
        const uint2 rg = cl.cellRange[icellj];
        first = (int)rg.x;
        last = (int)(rg.y & 0x7fffffffu);
      } else {
        const uint cs = cl.cellStart[icellj];
        if (cs >= cl.validCell) { first = (int)(cs - cl.validCell); last = cl.cellEnd[icellj]; }
      }
    }
    for (int j = first; __any(j < last); ++j) {
      if (j < last) {
        const float4 pj = cl.sortPos[j];
        const real3f rij = box.apply_pbc(real3f{pi.x - pj.x, pi.y - pj.y, pi.z - pj.z});
        if (dot3(rij, rij) < p.rc2Filter && j != id) { q[n * kDB] = (uint)j; ++n; }
      }
      if (__any(n == kDCap)) dpd_drain(fx, fy, fz, q, n, cl.sortPos, sortVel, pi, vi, box, p);
    }
  }
  dpd_drain(fx, fy, fz, q, n, cl.sortPos, sortVel, pi, vi, box, p);
  const uint ori = __float_as_uint(vi.w);
  float4 f = force[ori];
  f.x += fx; f.y += fy; f.z += fz;
  force[ori] = f;
}

// all pairs among the members (t -> globalIndex[t], or the identity), 128-particle tiles staged in LDS
__global__ void __launch_bounds__(kDB) k_dpd_nbody(const float4 *__restrict__ pos, const float *__restrict__ vel, int N, BoxT<float> box,
                                                   const int *__restrict__ globalIndex, DPDParams p, float4 *__restrict__ force) {
  __shared__ float4 tp[kDB], tv[kDB];
  const int t = blockIdx.x * kDB + threadIdx.x;
  const bool active = t < N;
  const int id = active ? (globalIndex ? globalIndex[t] : t) : 0;
  const float4 pi = active ? pos[id] : make_float4(0.f, 0.f, 0.f, 0.f);
  const real3f vi = active ? real3f{vel[3 * id], vel[3 * id + 1], vel[3 * id + 2]} : real3f{0.f, 0.f, 0.f};
  float fx = 0.f, fy = 0.f, fz = 0.f;
  for (int base = 0; base < N; base += kDB) {
    const int l = base + threadIdx.x;
    if (l < N) {
      const int jd = globalIndex ? globalIndex[l] : l;
      tp[threadIdx.x] = pos[jd];
      tv[threadIdx.x] = make_float4(vel[3 * jd], vel[3 * jd + 1], vel[3 * jd + 2], __uint_as_float((uint)jd));
    }
    __syncthreads();
    if (active) {
      const int cnt = min(kDB, N - base);
      for (int c = 0; c < cnt; ++c) {
        const float4 pj = tp[c], vj = tv[c];
        const real3f rij = box.apply_pbc(real3f{pi.x - pj.x, pi.y - pj.y, pi.z - pj.z});
        const float r2 = dot3(rij, rij);
        if (r2 < p.rc2Filter && base + c != t)
          dpd_pair(fx, fy, fz, rij, r2, real3f{vi.x - vj.x, vi.y - vj.y, vi.z - vj.z}, (uint)id, __float_as_uint(vj.w), p);
      }
    }
    __syncthreads();
  }
  if (active) {
    float4 f = force[id];
    f.x += fx; f.y += fy; f.z += fz;
    force[id] = f;
  }
}

static int dpd_params(const char *who, float cutOff, float A, float gamma, float sigma, unsigned long long seed, unsigned long long step,
                      int numberParticlesKey, DPDParams *p) {
  if (!(cutOff > 0) || !(gamma >= 0) || numberParticlesKey < 0) {
    set_last_error("%s: needs cutOff > 0, gamma >= 0 and numberParticlesKey >= 0", who);
    return -1;
  }
  p->invrc = 1.0f / cutOff;
  p->rc2Filter = cutOff * cutOff * 1.00001f;
  p->A = A;
  p->gamma = gamma;
  p->sigmaSqrtGamma = sigma * sqrtf(gamma);
  p->seed = (uint)seed;   // Saru's constructor takes 32-bit words (third_party/saruprng.cuh:222)
  p->step = (uint)step;
  p->N = (uint)numberParticlesKey;
  return 0;
}

}  // namespace uammd_hip

using namespace uammd_hip;

extern "C" {

int uammd_dpd_transverse_celllist(uammd_celllist *hh, const float *d_vel, const float boxL[3], const int boxPeriodic[3], float cutOff,
                                  float A, float gamma, float sigma, unsigned long long seed, unsigned long long step,
                                  int numberParticlesKey, float *d_force, const int *d_globalIndex, void *stream) {
  if (!hh || !d_vel || !d_force || !boxL || !boxPeriodic) { set_last_error("uammd_dpd_transverse_celllist: null argument"); return -1; }
  CellList *h = reinterpret_cast<CellList *>(hh);
  DPDParams p;
  if (int e = dpd_params("uammd_dpd_transverse_celllist", cutOff, A, gamma, sigma, seed, step, numberParticlesKey, &p)) return e;
  const int N = h->numberParticlesBuilt;
  if (N == 0) return 0;
  if (h->numOwned != 0x7fffffff) { set_last_error("uammd_dpd_transverse_celllist: lists with ghost particles (num_owned) are not supported"); return -3; }
  const GridT<float> &g = h->grid;
  // the walk visits the 27 cells around a particle: no edge of a direction with several cells may be shorter than the cut-off
  if ((g.cellDim.x > 1 && g.cellSize.x < 0.9999f * cutOff) || (g.cellDim.y > 1 && g.cellSize.y < 0.9999f * cutOff) || (g.cellDim.z > 1 && g.cellSize.z < 0.9999f * cutOff)) {
    set_last_error("uammd_dpd_transverse_celllist: the list's cells (%g, %g, %g) are smaller than the cut-off %g", g.cellSize.x, g.cellSize.y,
                   g.cellSize.z, cutOff);
    return -3;
  }
  hipStream_t st = (hipStream_t)stream;
  if (int e = h->dpdVel.reserve(sizeof(float4) * (size_t)N)) return e;   // grows only: nothing is allocated after the first sum of a size
  const BoxT<float> box = make_box<float>(boxL, boxPeriodic);
  ListView cl{};
  cl.cellStart = (const uint *)h->cellStart.ptr;
  cl.cellEnd = (const int *)h->cellEnd.ptr;
  cl.sortPos = (const float4 *)h->sortPos.ptr;
  cl.groupIndex = (const int *)h->index.ptr;
  cl.cellRange = h->haveCellOutside ? (const uint2 *)h->cellRange.ptr : nullptr;
  cl.validCell = h->validCell;
  cl.N = N;
  cl.numOwned = h->numOwned;
  hipLaunchKernelGGL(k_dpd_gather, dim3((N + 255) / 256), dim3(256), 0, st, cl.groupIndex, d_globalIndex, d_vel, (float4 *)h->dpdVel.ptr, N);
  hipLaunchKernelGGL(k_dpd_celllist, dim3((N + kDB - 1) / kDB), dim3(kDB), 0, st, cl, g, box, (const float4 *)h->dpdVel.ptr, p,
                     reinterpret_cast<float4 *>(d_force));
  UH_CHECK(hipGetLastError());
  return 0;
}

int uammd_dpd_transverse_nbody(const float *d_pos, const float *d_vel, int numberParticles, const float boxL[3], const int boxPeriodic[3],
                               float cutOff, float A, float gamma, float sigma, unsigned long long seed, unsigned long long step,
                               int numberParticlesKey, float *d_force, const int *d_globalIndex, void *stream) {
  if (!d_pos || !d_vel || !d_force || !boxL || !boxPeriodic) { set_last_error("uammd_dpd_transverse_nbody: null argument"); return -1; }
  DPDParams p;
  if (int e = dpd_params("uammd_dpd_transverse_nbody", cutOff, A, gamma, sigma, seed, step, numberParticlesKey, &p)) return e;
  if (numberParticles <= 0) return 0;
  const BoxT<float> box = make_box<float>(boxL, boxPeriodic);
  hipLaunchKernelGGL(k_dpd_nbody, dim3((numberParticles + kDB - 1) / kDB), dim3(kDB), 0, (hipStream_t)stream,
                     reinterpret_cast<const float4 *>(d_pos), d_vel, numberParticles, box, d_globalIndex, p, reinterpret_cast<float4 *>(d_force));
  UH_CHECK(hipGetLastError());
  return 0;
}

}  // extern "C"
