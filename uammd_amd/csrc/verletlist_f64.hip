// DOUBLE_PRECISION build of the Verlet (explicit neighbour) list for gfx950: the `_f64` entry points of the "Path A in double" block of
// include/uammd_hip.h that verletlist.hip has in single precision.
//
// What the reference does (behaviour matched against the -DDOUBLE_PRECISION oracle; NOT its implementation):
//   BasicNeighbourListBase::update / fillBasicNeighbourList      Interactor/NeighbourList/BasicList/BasicListBase.cuh:41-215
//   VerletListBase::update / needsRebuild / checkMaximumDrift     Interactor/NeighbourList/VerletList/VerletListBase.cuh:55-199
//   transverseWithNeighbourContainer                              Interactor/NeighbourList/common.cuh:10-34
// A cell list (md_f64.hip) of the STORED positions with radius multiplier * cutOff; for every sorted particle i the sorted indices j with
// |pbc(rj - ri)|^2 <= (multiplier * cutOff)^2 in double, i itself included, in the order of the 27-cell walk; entry k at
// neighbourList[k * N + i].  The host logic (rebuild decision, threshold, capacity, sizes) is verletlist_f64_host.hpp.
#include "md_f64.hpp"
#include "verletlist_f64_host.hpp"

namespace uammd_hip {
namespace {

using namespace md64d;

struct VerletList64 {
  uammd_celllist_f64 *cl = nullptr;  // BasicNeighbourListBase::cl, on the stored positions
  DeviceBuffer neighbourList, numberNeighbours, storedPos, sortPos, flags;
  vl64::State s;
  uint *hostFlag = nullptr;  // pinned: the drift counter and the largest neighbour count are read back here
  CellList64 *list() const { return reinterpret_cast<CellList64 *>(cl); }
  ~VerletList64() {
    if (hostFlag) (void)hipHostFree(hostFlag);
    if (cl) uammd_celllist_destroy_f64(cl);
  }
};

struct FillView {
  const uint *cellStart;
  const int *cellEnd;
  const double4 *sortPos;
  const uint *sortHash;
  const unsigned char *cellOutside;
  uint validCell, maxHash;
  int N;
};

// K7.  A lane per sorted particle walks its 27 cells in the reference's order.  Every neighbour is COUNTED; entry k is STORED only while
// k < capacity, the capacity this launch's buffer was sized for (vl64::may_store), so a fill cannot write past its buffer whatever the
// positions are.  The largest count goes to *largestCount: the host grows the capacity and fills again while it reaches the capacity
// (the reference's `nneigh >= max`).  The minimum image is skipped per neighbour cell for the whole wave where it is the identity, as in
// k64_lj (md_f64.hip).
__global__ void __launch_bounds__(128) k64_verlet_fill(FillView cl, GridT<double> grid, BoxT<double> box, double cutOff2, int capacity,
                                                       int *__restrict__ neighbourList, int *__restrict__ numberNeighbours,
                                                       int *__restrict__ largestCount) {
  const int id = (int)xcd_contiguous_block(blockIdx.x, gridDim.x) * 128 + threadIdx.x;
  if (id >= cl.N) return;
  const uint key = cl.sortHash[id];
  if (key > cl.maxHash) {  // a particle without a cell (NaN, outside a non-periodic box): no neighbours; the cell list's flag reports it
    numberNeighbours[id] = 0;
    return;
  }
  const double4 pi = cl.sortPos[id];
  const int3 n = grid.cellDim;
  const int npx = n.x > 1 ? 3 : 1, npy = n.y > 1 ? 3 : 1, npz = n.z > 1 ? 3 : 1;
  const int numberNeighbourCells = npx * npy * npz;
  const int3 celli = cell_of_key(key);
  const bool sameBox = box.boxSize.x == grid.box.boxSize.x && box.boxSize.y == grid.box.boxSize.y && box.boxSize.z == grid.box.boxSize.z &&
                       box.px() == grid.box.px() && box.py() == grid.box.py() && box.pz() == grid.box.pz();
  const bool smallGrid = n.x < 5 || n.y < 5 || n.z < 5 || !sameBox;
  const double hx = 0.5 * box.boxSize.x, hy = 0.5 * box.boxSize.y, hz = 0.5 * box.boxSize.z;
  const bool iOut = !(pi.x >= -hx && pi.x < hx && pi.y >= -hy && pi.y < hy && pi.z >= -hz && pi.z < hz);
  int *mine = neighbourList + id;
  int cnt = 0;
  for (int cc = 0; cc < numberNeighbourCells; ++cc) {
    int3 cellj = celli;
    if (npx > 1) cellj.x += cc % 3 - 1;
    if (npy > 1) cellj.y += (cc / npx) % 3 - 1;
    if (npz > 1) cellj.z += cc / (npx * npy) - 1;
    const int3 raw = cellj;
    cellj.x = grid.pbc_x(cellj.x);
    cellj.y = grid.pbc_y(cellj.y);
    cellj.z = grid.pbc_z(cellj.z);
    int first = 0, last = 0;
    bool needPBC = false;
    if (in_grid(grid, cellj)) {  // outside a non periodic box: no such cell
      const int icellj = grid.getCellIndex(cellj);
      const uint cs = cl.cellStart[icellj];
      if (cs >= cl.validCell) {
        first = (int)(cs - cl.validCell);
        last = cl.cellEnd[icellj];
        const bool wrapped = raw.x != cellj.x || raw.y != cellj.y || raw.z != cellj.z;
        needPBC = smallGrid || iOut || wrapped || cl.cellOutside[icellj] != 0;
      }
    }
    const bool wavePBC = __any(needPBC);
    for (int j = first; j < last; ++j) {
      const double4 pj = cl.sortPos[j];
      const double r2 = wavePBC ? lj_dist2_64<true>(box, pi, pj) : lj_dist2_64<false>(box, pi, pj);
      if (r2 <= cutOff2) {
        if (cnt < capacity) mine[(size_t)cnt * (size_t)cl.N] = j;
        ++cnt;
      }
    }
  }
  numberNeighbours[id] = cnt;
  if (cnt >= capacity) atomicMax(largestCount, cnt);
}

// K8.  Counts the particles that moved >= maxDistAllowed from their stored position.
__global__ void __launch_bounds__(256) k64_verlet_drift(const double4 *__restrict__ currentPos, const double4 *__restrict__ storedPos,
                                                        double maxDistAllowed, uint *__restrict__ counter, BoxT<double> box, int N) {
  const int id = blockIdx.x * 256 + threadIdx.x;
  bool over = false;
  if (id < N) {
    const double4 c = currentPos[id], s = storedPos[id];
    const real3d rij = box.apply_pbc(real3d{c.x - s.x, c.y - s.y, c.z - s.z});
    over = dot3(rij, rij) >= (maxDistAllowed * maxDistAllowed);
  }
  const unsigned long long m = __ballot(over);
  if ((threadIdx.x & 63) == 0 && m) atomicAdd(counter, (uint)__popcll(m));
}

__global__ void __launch_bounds__(256) k64_verlet_sortpos(const double4 *__restrict__ pos, const int *__restrict__ groupIndex,
                                                          double4 *__restrict__ sortPos, int N) {
  const int id = blockIdx.x * 256 + threadIdx.x;
  if (id < N) sortPos[id] = pos[groupIndex[id]];
}

// K6 over the list.  A lane per sorted particle: entry k of the 64 lanes of a wave is one coalesced 256-byte read of the list, then a
// gather of the neighbours' 32-byte rows.  Every listed pair goes through the full minimum image and md_f64's pair evaluation, in list
// order: force, energy and virial keep the oracle's FMA placement.  Two entries ahead, one row ahead, as k_lj_verlet (verletlist.hip);
// entries past the particle's own count re-read its last one and carry no weight, so nothing beyond numberNeighbours[i] is read.
template <bool NT1, bool WE, bool WV>
__global__ void __launch_bounds__(128) k64_lj_verlet(const double4 *__restrict__ sortPos, const int *__restrict__ groupIndex,
                                                     const int *__restrict__ neighbourList, const int *__restrict__ numberNeighbours, int N,
                                                     BoxT<double> box, const LJParams64 *__restrict__ tbl, int ntypes, Out64 out) {
  const int id = (int)xcd_contiguous_block(blockIdx.x, gridDim.x) * 128 + threadIdx.x;
  if (id >= N) return;
  const int gi = groupIndex[id];
  const int ori = out.globalIndex ? out.globalIndex[gi] : gi;
  const double4 pi = sortPos[id];
  const LJParams64 p1 = tbl[0];
  const int nn = numberNeighbours[id];
  const int *mine = neighbourList + id;
  Acc64 acc;
  const int l1 = max(nn - 1, 0);
  auto entries = [&](int k, int (&j)[2]) {
#pragma unroll
    for (int u = 0; u < 2; ++u) j[u] = nn > 0 ? mine[(size_t)min(k + u, l1) * (size_t)N] : id;
  };
  int jb[2], jc[2];
  double4 cb[2];
  entries(0, jb);
  entries(2, jc);
#pragma unroll
  for (int u = 0; u < 2; ++u) cb[u] = sortPos[jb[u]];
  for (int k = 0; k < nn; k += 2) {
    double4 c[2];
    int jd[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) c[u] = cb[u];
    entries(k + 4, jd);
#pragma unroll
    for (int u = 0; u < 2; ++u) cb[u] = sortPos[jc[u]];
#pragma unroll
    for (int u = 0; u < 2; ++u) jc[u] = jd[u];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      real3d r12;
      double fm, e;
      if (NT1) lj_eval64<true, WE>(box, p1, pi, c[u], r12, fm, e);
      else lj_eval64<true, WE>(box, lj_lookup64(tbl, ntypes, (int)pi.w, (int)c[u].w), pi, c[u], r12, fm, e);
      const bool live = k + u < nn;
      lj_acc64<WE, WV>(acc, r12, live ? fm : 0.0, live ? e : 0.0);
    }
  }
  write_out64(out, ori, acc);
}

template <bool NT1, bool WE, bool WV>
void launch_verlet64(VerletList64 *v, const BoxT<double> &box, const LJParams64 *tbl, int ntypes, const Out64 &out, hipStream_t st) {
  hipLaunchKernelGGL((k64_lj_verlet<NT1, WE, WV>), dim3((v->s.N + 127) / 128), dim3(128), 0, st, (const double4 *)v->sortPos.ptr,
                     (const int *)v->list()->index.ptr, (const int *)v->neighbourList.ptr, (const int *)v->numberNeighbours.ptr, v->s.N, box,
                     tbl, ntypes, out);
}

int read_flag(VerletList64 *v, int slot, hipStream_t st, uint *value) {
  UH_CHECK(hipMemcpyAsync(v->hostFlag, (const uint *)v->flags.ptr + slot, sizeof(uint), hipMemcpyDeviceToHost, st));
  UH_CHECK(hipStreamSynchronize(st));
  *value = *v->hostFlag;
  return 0;
}

// BasicNeighbourListBase::update (BasicListBase.cuh:132-142) on the stored positions
int rebuild64(VerletList64 *v, hipStream_t st) {
  const int N = v->s.N;
  const double rcut = vl64::list_radius(v->s);  // VerletListBase.cuh:153-156
  const double rc3[3] = {rcut, rcut, rcut};
  int cd[3], gper[3];
  double gL[3];
  if (int e = uammd_celllist_create_grid_f64(v->s.boxL, v->s.boxPeriodic, rc3, cd, gL, gper)) return e;
  if (int e = uammd_celllist_update_f64(v->cl, (const double *)v->storedPos.ptr, N, gL, gper, cd, st)) return e;
  CellList64 *c = v->list();
  const BoxT<double> box = make_box<double>(v->s.boxL, v->s.boxPeriodic);
  const FillView view{(const uint *)c->cellStart.ptr, (const int *)c->cellEnd.ptr, (const double4 *)c->sortPos.ptr, (const uint *)c->hash.ptr,
                      (const unsigned char *)c->cellOutside.ptr, c->epoch.validCell, c->maxHash, N};
  for (;;) {  // fillBasicNeighbourList: again with more slots while some particle reaches the capacity
    const int capacity = v->s.maxNeighboursPerParticle;
    const vl64::BufferBytes bytes = vl64::buffer_bytes(N, capacity);
    if (int e = v->numberNeighbours.reserve(bytes.numberNeighbours)) return e;
    if (int e = v->neighbourList.reserve(bytes.neighbourList)) return e;
    UH_CHECK(hipMemsetAsync((uint *)v->flags.ptr + 1, 0, sizeof(uint), st));
    hipLaunchKernelGGL(k64_verlet_fill, dim3((N + 127) / 128), dim3(128), 0, st, view, c->grid, box, rcut * rcut, capacity,
                       (int *)v->neighbourList.ptr, (int *)v->numberNeighbours.ptr, (int *)v->flags.ptr + 1);
    UH_CHECK(hipGetLastError());
    uint largest = 0;
    if (int e = read_flag(v, 1, st, &largest)) return e;
    if (!vl64::grow_capacity(v->s, (int)largest)) break;
  }
  return c->check_errors(st, false);  // (the read-back above synchronised the stream)
}

}  // namespace
}  // namespace uammd_hip

using namespace uammd_hip;

extern "C" {

int uammd_verletlist_create_f64(uammd_verletlist_f64 **out) {
  if (!out) { set_last_error("uammd_verletlist_create_f64: null argument"); return -1; }
  VerletList64 *v = new VerletList64();  // (device and pinned memory come with the first update that has particles)
  if (uammd_celllist_create_f64(&v->cl)) {
    delete v;
    return -2;
  }
  *out = reinterpret_cast<uammd_verletlist_f64 *>(v);
  return 0;
}

int uammd_verletlist_destroy_f64(uammd_verletlist_f64 *h) {
  delete reinterpret_cast<VerletList64 *>(h);
  return 0;
}

int uammd_verletlist_force_next_update_f64(uammd_verletlist_f64 *h) {
  if (!h) { set_last_error("uammd_verletlist_force_next_update_f64: null handle"); return -1; }
  reinterpret_cast<VerletList64 *>(h)->s.forceNextRebuild = true;
  return 0;
}

int uammd_verletlist_set_cutoff_multiplier_f64(uammd_verletlist_f64 *h, double newMultiplier) {
  if (const char *msg = vl64::check_multiplier(h, newMultiplier)) { set_last_error("%s", msg); return -1; }
  VerletList64 *v = reinterpret_cast<VerletList64 *>(h);
  v->s.forceNextRebuild = true;
  v->s.verletRadiusMultiplier = newMultiplier;
  return 0;
}

int uammd_verletlist_get_steps_since_last_update_f64(uammd_verletlist_f64 *h, int *steps) {
  if (!h || !steps) { set_last_error("uammd_verletlist_get_steps_since_last_update_f64: null argument"); return -1; }
  *steps = reinterpret_cast<VerletList64 *>(h)->s.stepsSinceLastUpdate - 1;  // VerletListBase.cuh:124
  return 0;
}

// VerletListBase::update (VerletListBase.cuh:107-117)
int uammd_verletlist_update_f64(uammd_verletlist_f64 *h, const double *d_pos, int numberParticles, const double L[3], const int periodic[3],
                                double cutOff, void *stream, int *rebuilt) {
  VerletList64 *v = reinterpret_cast<VerletList64 *>(h);
  if (const char *msg = vl64::check_update(h, d_pos, numberParticles, L, periodic, cutOff, v ? v->s.verletRadiusMultiplier : 1.0)) {
    set_last_error("%s", msg);
    return -1;
  }
  hipStream_t st = (hipStream_t)stream;
  const int N = numberParticles;
  if (rebuilt) *rebuilt = 0;
  if (N == 0) { v->s.N = 0; return 0; }
  if (!v->hostFlag) {
    UH_CHECK(hipHostMalloc((void **)&v->hostFlag, sizeof(uint)));
    if (int e = v->flags.reserve(vl64::buffer_bytes(0, 0).flags)) return e;
  }
  const BoxT<double> box = make_box<double>(L, periodic);
  bool rebuild = vl64::needs_rebuild(v->s, L, periodic, cutOff, N) == vl64::REBUILD;
  if (!rebuild) {  // isParticleDriftOverThreshold, :177-199
    UH_CHECK(hipMemsetAsync(v->flags.ptr, 0, sizeof(uint), st));
    hipLaunchKernelGGL(k64_verlet_drift, dim3((N + 255) / 256), dim3(256), 0, st, (const double4 *)d_pos, (const double4 *)v->storedPos.ptr,
                       vl64::drift_threshold(v->s.verletRadiusMultiplier, v->s.currentCutOff), (uint *)v->flags.ptr, box, N);
    UH_CHECK(hipGetLastError());
    uint moved = 0;
    if (int e = read_flag(v, 0, st, &moved)) return e;
    rebuild = moved > 0;
  }
  if (rebuild) {
    vl64::begin_rebuild(v->s, L, periodic, cutOff, N);
    const vl64::BufferBytes bytes = vl64::buffer_bytes(N, v->s.maxNeighboursPerParticle);
    if (int e = v->storedPos.reserve(bytes.storedPos)) return e;
    if (int e = v->sortPos.reserve(bytes.sortPos)) return e;
    UH_CHECK(hipMemcpyAsync(v->storedPos.ptr, d_pos, bytes.storedPos, hipMemcpyDeviceToDevice, st));  // storeCurrentPos
    if (int e = rebuild64(v, st)) {
      v->s.forceNextRebuild = true;  // nothing usable was built
      v->s.N = 0;
      return e;
    }
    if (rebuilt) *rebuilt = 1;
  }
  v->s.N = N;  // (an update with no particles in between left 0 here; the list of storedN particles is still the one in force)
  // updateSortedPositions, :140-151
  hipLaunchKernelGGL(k64_verlet_sortpos, dim3((N + 255) / 256), dim3(256), 0, st, (const double4 *)d_pos, (const int *)v->list()->index.ptr,
                     (double4 *)v->sortPos.ptr, N);
  UH_CHECK(hipGetLastError());
  vl64::end_update(v->s);
  return 0;
}

int uammd_verletlist_get_f64(uammd_verletlist_f64 *h, uammd_verletlist_data_f64 *out) {
  if (!h || !out) { set_last_error("uammd_verletlist_get_f64: null argument"); return -1; }
  VerletList64 *v = reinterpret_cast<VerletList64 *>(h);
  out->d_neighbourList = (const int *)v->neighbourList.ptr;
  out->d_numberNeighbours = (const int *)v->numberNeighbours.ptr;
  out->d_sortPos = (const double *)v->sortPos.ptr;
  out->d_groupIndex = (const int *)v->list()->index.ptr;
  out->particleStride = v->s.N;  // BasicListBase.cuh:163-166
  out->maxNeighboursPerParticle = v->s.maxNeighboursPerParticle;
  out->numberParticles = v->s.N;
  return 0;
}

int uammd_lj_transverse_verletlist_f64(uammd_verletlist_f64 *h, const uammd_lj_pair_parameters_f64 *d_paramTable, int ntypes,
                                       const double boxL[3], const int boxPeriodic[3], double *d_force, double *d_energy, double *d_virial,
                                       const int *d_globalIndex, void *stream) {
  if (!h || !d_paramTable || !boxL || !boxPeriodic || ntypes < 1) { set_last_error("uammd_lj_transverse_verletlist_f64: bad arguments"); return -1; }
  VerletList64 *v = reinterpret_cast<VerletList64 *>(h);
  if (v->s.N == 0) return 0;
  const BoxT<double> box = make_box<double>(boxL, boxPeriodic);
  const Out64 out{reinterpret_cast<double4 *>(d_force), d_energy, d_virial, d_globalIndex};
  const LJParams64 *tbl = reinterpret_cast<const LJParams64 *>(d_paramTable);
  hipStream_t st = (hipStream_t)stream;
  const bool nt1 = ntypes == 1, ev = d_energy != nullptr || d_virial != nullptr;
  if (nt1 && !ev) launch_verlet64<true, false, false>(v, box, tbl, ntypes, out, st);
  else if (nt1) launch_verlet64<true, true, true>(v, box, tbl, ntypes, out, st);
  else if (!ev) launch_verlet64<false, false, false>(v, box, tbl, ntypes, out, st);
  else launch_verlet64<false, true, true>(v, box, tbl, ntypes, out, st);
  UH_CHECK(hipGetLastError());
  return 0;
}

}  // extern "C"
