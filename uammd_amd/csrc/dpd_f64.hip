// DOUBLE_PRECISION build of the dissipative particle dynamics pair force for gfx950 (Interactor/Potential/DPD.cuh:121-152), over a built
// double-precision cell list (md_f64.hip) and over all pairs: the `_f64` entry points that dpd.hip has in single precision.
//
//   rij = pbc(ri - rj), vij = vi - vj, r = |rij|; nothing if r == 0 or 1/r <= 1/rc      (both tests exact, in double)
//   wr = 1 - r/rc;  Fc = A wr / r;  Fd = -g wr^2 (rij . vij) / r^2;  Fr = xi sigma sqrt(g) wr / r
//   xi = Saru(ij, seed, step).gf(0, 1).x,  ij = min(i, j) + N max(i, j)  (unsigned arithmetic, seed and step truncated to 32 bits)
//   F_i += (Fc + Fd + Fr) rij
// xi is Saru's SINGLE-precision Box-Muller x promoted to double, as the reference's double build draws it and as uammd_verletnvt_gj_f64
// treats its Gaussians; everything else is double.
//
// Shape: dpd.hip's.  Velocities and keys are gathered once per sum into list order (32-byte rows {v, key} in scratch the list handle
// owns); a lane per particle compacts its hits into a per-lane FIFO in LDS and the wave drains the FIFOs together, so the generator
// runs max-over-lanes(hits) times per wave.  A lane is the only writer of its force row: no atomics, the same bits run to run.
// LDS: 32 entries x 128 lanes x 4 bytes = 16 KB per workgroup of two waves: ten workgroups, five waves per SIMD, fit in a CU's 160 KB.
#include "md_f64.hpp"
#include "saru.hpp"

namespace uammd_hip {
namespace {

using namespace md64d;

struct DPDParams64 {
  double invrc, rc2Filter;  // 1 / rc; rc^2 widened by a few ulp for the compaction (the exact 1/r <= 1/rc test decides in the drain)
  double A, gamma, sigmaSqrtGamma;
  uint seed, step, N;
};

UH_D uint key_of(const double4 &v) { return (uint)__double_as_longlong(v.w); }
UH_D double key_as_double(uint k) { return __longlong_as_double((long long)k); }

// DPD.cuh:121-152 for one pair that has passed the coarse distance filter; ki, kj are the particles' indices (the generator's key)
UH_D void dpd_pair64(double &fx, double &fy, double &fz, const real3d &rij, double r2, const real3d &vij, uint ki, uint kj,
                     const DPDParams64 &p) {
  if (r2 == 0.0) return;
  const double rmod = sqrt(r2);
  const double invrmod = 1.0 / rmod;
  if (invrmod <= p.invrc) return;
  const double wr = 1.0 - rmod * p.invrc;
  const double Fc = p.A * wr * invrmod;
  const double Fd = -p.gamma * (wr * wr) * invrmod * invrmod * dot3(rij, vij);
  const uint lo = ki < kj ? ki : kj, hi = ki < kj ? kj : ki;
  Saru rng(lo + p.N * hi, p.seed, p.step);
  const double xi = (double)rng.gf(0.0f, 1.0f).x;
  const double Fr = xi * (p.sigmaSqrtGamma * wr * invrmod);
  const double f = Fc + Fd + Fr;
  fx = fma(f, rij.x, fx);
  fy = fma(f, rij.y, fy);
  fz = fma(f, rij.z, fz);
}

constexpr int kDB = 128;   // lanes per workgroup
constexpr int kDCap = 32;  // FIFO entries per lane (LDS: 16 KB per workgroup)

// velocities and keys into list order: out[s] = {vel[ori], ori}, ori = globalIndex[index[s]]
__global__ void __launch_bounds__(256) k64_dpd_gather(const int *__restrict__ index, const int *__restrict__ globalIndex,
                                                      const double *__restrict__ vel, double4 *__restrict__ out, int N) {
  const int s = blockIdx.x * 256 + threadIdx.x;
  if (s >= N) return;
  const int gi = index[s];
  const int ori = globalIndex ? globalIndex[gi] : gi;
  out[s] = make_double4(vel[3 * (size_t)ori], vel[3 * (size_t)ori + 1], vel[3 * (size_t)ori + 2], key_as_double((uint)ori));
}

UH_D void dpd_drain64(double &fx, double &fy, double &fz, const uint *q, int &n, const double4 *__restrict__ P, const double4 *__restrict__ V,
                      const double4 &pi, const double4 &vi, const BoxT<double> &box, const DPDParams64 &p) {
  for (int k = 0; __any(k < n); ++k) {
    if (k < n) {
      const uint j = q[k * kDB];
      const double4 pj = P[j], vj = V[j];
      const real3d rij = box.apply_pbc(real3d{pi.x - pj.x, pi.y - pj.y, pi.z - pj.z});
      dpd_pair64(fx, fy, fz, rij, dot3(rij, rij), real3d{vi.x - vj.x, vi.y - vj.y, vi.z - vj.z}, key_of(vi), key_of(vj), p);
    }
  }
  n = 0;
}

struct DPDView {
  const uint *cellStart;
  const int *cellEnd;
  const double4 *sortPos;
  const uint *sortHash;
  uint validCell, maxHash;
  int N;
};

__global__ void __launch_bounds__(kDB) k64_dpd_celllist(DPDView cl, GridT<double> grid, BoxT<double> box, const double4 *__restrict__ sortVel,
                                                        DPDParams64 p, double4 *__restrict__ force) {
  __shared__ uint fifo[kDCap * kDB];
  const int id = (int)xcd_contiguous_block(blockIdx.x, gridDim.x) * kDB + threadIdx.x;
  if (id >= cl.N) return;  // (no workgroup barrier below: the wave-level votes only count the lanes that are left)
  const uint key = cl.sortHash[id];
  if (key > cl.maxHash) return;  // a particle without a cell: nothing is computed for it
  const double4 pi = cl.sortPos[id], vi = sortVel[id];
  uint *q = fifo + threadIdx.x;
  int n = 0;
  double fx = 0.0, fy = 0.0, fz = 0.0;
  const int3 nc = grid.cellDim;
  const int npx = nc.x > 1 ? 3 : 1, npy = nc.y > 1 ? 3 : 1, npz = nc.z > 1 ? 3 : 1;
  const int3 celli = cell_of_key(key);
  for (int cc = 0; cc < npx * npy * npz; ++cc) {
    int3 cellj = celli;
    if (npx > 1) cellj.x += cc % 3 - 1;
    if (npy > 1) cellj.y += (cc / npx) % 3 - 1;
    if (npz > 1) cellj.z += cc / (npx * npy) - 1;
    cellj.x = grid.pbc_x(cellj.x);
    cellj.y = grid.pbc_y(cellj.y);
    cellj.z = grid.pbc_z(cellj.z);
    int first = 0, last = 0;
    if (in_grid(grid, cellj)) {  // outside a non periodic box: no such cell
      const int icellj = grid.getCellIndex(cellj);
      const uint cs = cl.cellStart[icellj];
      if (cs >= cl.validCell) { first = (int)(cs - cl.validCell); last = cl.cellEnd[icellj]; }
    }
    for (int j = first; __any(j < last); ++j) {
      if (j < last) {
        const double4 pj = cl.sortPos[j];
        const real3d rij = box.apply_pbc(real3d{pi.x - pj.x, pi.y - pj.y, pi.z - pj.z});
        if (dot3(rij, rij) < p.rc2Filter && j != id) { q[n * kDB] = (uint)j; ++n; }  // n < kDCap: a full FIFO was drained below
      }
      if (__any(n == kDCap)) dpd_drain64(fx, fy, fz, q, n, cl.sortPos, sortVel, pi, vi, box, p);
    }
  }
  dpd_drain64(fx, fy, fz, q, n, cl.sortPos, sortVel, pi, vi, box, p);
  const uint ori = key_of(vi);
  double4 f = force[ori];
  f.x += fx; f.y += fy; f.z += fz;
  force[ori] = f;
}

// all pairs among the members (t -> globalIndex[t], or the identity), 128-particle tiles staged in LDS
__global__ void __launch_bounds__(kDB) k64_dpd_nbody(const double4 *__restrict__ pos, const double *__restrict__ vel, int N, BoxT<double> box,
                                                     const int *__restrict__ globalIndex, DPDParams64 p, double4 *__restrict__ force) {
  __shared__ double4 tp[kDB], tv[kDB];
  const int t = blockIdx.x * kDB + threadIdx.x;
  const bool active = t < N;
  const int id = active ? (globalIndex ? globalIndex[t] : t) : 0;
  const double4 pi = active ? pos[id] : make_double4(0.0, 0.0, 0.0, 0.0);
  const real3d vi = active ? real3d{vel[3 * (size_t)id], vel[3 * (size_t)id + 1], vel[3 * (size_t)id + 2]} : real3d{0.0, 0.0, 0.0};
  double fx = 0.0, fy = 0.0, fz = 0.0;
  for (int base = 0; base < N; base += kDB) {
    const int l = base + threadIdx.x;
    if (l < N) {
      const int jd = globalIndex ? globalIndex[l] : l;
      tp[threadIdx.x] = pos[jd];
      tv[threadIdx.x] = make_double4(vel[3 * (size_t)jd], vel[3 * (size_t)jd + 1], vel[3 * (size_t)jd + 2], key_as_double((uint)jd));
    }
    __syncthreads();
    if (active) {
      const int cnt = min(kDB, N - base);
      for (int c = 0; c < cnt; ++c) {
        const double4 pj = tp[c], vj = tv[c];
        const real3d rij = box.apply_pbc(real3d{pi.x - pj.x, pi.y - pj.y, pi.z - pj.z});
        const double r2 = dot3(rij, rij);
        if (r2 < p.rc2Filter && base + c != t)
          dpd_pair64(fx, fy, fz, rij, r2, real3d{vi.x - vj.x, vi.y - vj.y, vi.z - vj.z}, (uint)id, key_of(vj), p);
      }
    }
    __syncthreads();
  }
  if (active) {
    double4 f = force[id];
    f.x += fx; f.y += fy; f.z += fz;
    force[id] = f;
  }
}

int dpd_params64(const char *who, double cutOff, double A, double gamma, double sigma, unsigned long long seed, unsigned long long step,
                 int numberParticlesKey, DPDParams64 *p) {
  if (!(cutOff > 0) || !(gamma >= 0) || numberParticlesKey < 0) {
    set_last_error("%s: needs cutOff > 0, gamma >= 0 and numberParticlesKey >= 0", who);
    return -1;
  }
  p->invrc = 1.0 / cutOff;
  p->rc2Filter = cutOff * cutOff * (1.0 + 0x1p-40);
  p->A = A;
  p->gamma = gamma;
  p->sigmaSqrtGamma = sigma * sqrt(gamma);
  p->seed = (uint)seed;  // Saru's constructor takes 32-bit words (third_party/saruprng.cuh:222)
  p->step = (uint)step;
  p->N = (uint)numberParticlesKey;
  return 0;
}

}  // namespace
}  // namespace uammd_hip

using namespace uammd_hip;

extern "C" {

int uammd_dpd_transverse_celllist_f64(uammd_celllist_f64 *hh, const double *d_vel, const double boxL[3], const int boxPeriodic[3],
                                      double cutOff, double A, double gamma, double sigma, unsigned long long seed, unsigned long long step,
                                      int numberParticlesKey, double *d_force, const int *d_globalIndex, void *stream) {
  if (!hh || !d_vel || !d_force || !boxL || !boxPeriodic) { set_last_error("uammd_dpd_transverse_celllist_f64: null argument"); return -1; }
  CellList64 *h = reinterpret_cast<CellList64 *>(hh);
  DPDParams64 p;
  if (int e = dpd_params64("uammd_dpd_transverse_celllist_f64", cutOff, A, gamma, sigma, seed, step, numberParticlesKey, &p)) return e;
  hipStream_t st = (hipStream_t)stream;
  if (int e = h->check_errors(st, false)) return e;
  const int N = h->N;
  if (N == 0) return 0;
  const GridT<double> &g = h->grid;
  // the walk visits the 27 cells around a particle: no edge of a direction with several cells may be shorter than the cut-off
  if ((g.cellDim.x > 1 && g.cellSize.x < 0.9999 * cutOff) || (g.cellDim.y > 1 && g.cellSize.y < 0.9999 * cutOff) ||
      (g.cellDim.z > 1 && g.cellSize.z < 0.9999 * cutOff)) {
    set_last_error("uammd_dpd_transverse_celllist_f64: the list's cells (%g, %g, %g) are smaller than the cut-off %g", g.cellSize.x, g.cellSize.y,
                   g.cellSize.z, cutOff);
    return -3;
  }
  const size_t bytes = 4 * sizeof(double) * (size_t)N;
  if (bytes != h->dpdRowsBytes) {  // the scratch follows the list's size
    if (int e = h->dpdRows.reserve(bytes)) return e;
    h->dpdRowsBytes = bytes;
  }
  const BoxT<double> box = make_box<double>(boxL, boxPeriodic);
  const DPDView cl{(const uint *)h->cellStart.ptr, (const int *)h->cellEnd.ptr, (const double4 *)h->sortPos.ptr, (const uint *)h->hash.ptr,
                   h->epoch.validCell, h->maxHash, N};
  hipLaunchKernelGGL(k64_dpd_gather, dim3((N + 255) / 256), dim3(256), 0, st, (const int *)h->index.ptr, d_globalIndex, d_vel,
                     (double4 *)h->dpdRows.ptr, N);
  hipLaunchKernelGGL(k64_dpd_celllist, dim3((N + kDB - 1) / kDB), dim3(kDB), 0, st, cl, g, box, (const double4 *)h->dpdRows.ptr, p,
                     reinterpret_cast<double4 *>(d_force));
  UH_CHECK(hipGetLastError());
  return 0;
}

int uammd_dpd_transverse_nbody_f64(const double *d_pos, const double *d_vel, int numberParticles, const double boxL[3], const int boxPeriodic[3],
                                   double cutOff, double A, double gamma, double sigma, unsigned long long seed, unsigned long long step,
                                   int numberParticlesKey, double *d_force, const int *d_globalIndex, void *stream) {
  if (!d_pos || !d_vel || !d_force || !boxL || !boxPeriodic) { set_last_error("uammd_dpd_transverse_nbody_f64: null argument"); return -1; }
  DPDParams64 p;
  if (int e = dpd_params64("uammd_dpd_transverse_nbody_f64", cutOff, A, gamma, sigma, seed, step, numberParticlesKey, &p)) return e;
  if (numberParticles <= 0) return 0;
  const BoxT<double> box = make_box<double>(boxL, boxPeriodic);
  hipLaunchKernelGGL(k64_dpd_nbody, dim3((numberParticles + kDB - 1) / kDB), dim3(kDB), 0, (hipStream_t)stream,
                     reinterpret_cast<const double4 *>(d_pos), d_vel, numberParticles, box, d_globalIndex, p, reinterpret_cast<double4 *>(d_force));
  UH_CHECK(hipGetLastError());
  return 0;
}

}  // extern "C"
