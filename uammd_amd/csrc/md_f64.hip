// DOUBLE_PRECISION build of path A for gfx950: the cell list, the Lennard-Jones traversal and the Verlet integrators with real = double
// (the `_f64` entry points of the "Path A in double" block of include/uammd_hip.h).  The reference makes `real` a build switch
// (global/defines.h:9-11,33-44); f64.hip is that build of path B, this file of the half the headline benchmark runs.
//
// What the reference does (behaviour matched bit for bit against the -DDOUBLE_PRECISION oracle; NOT its implementation):
//   assignHash, stable sort, reorder        utils/ParticleSorter.cuh:102-111,303-321,178-187
//   fillCellList, epoch trick               Interactor/NeighbourList/CellList/CellListBase.cuh:68-94,210-230
//   transverseWithNeighbourContainer        Interactor/NeighbourList/common.cuh:10-34 (27 cells, members in sorted order)
//   Radial<LJFunctor>                       Interactor/Potential/RadialPotential.cuh:107-127, Potential.cuh:37-82
//   NBody (boxes of at most 3 cut-offs)     Interactor/NBodyBase.cuh:46-116
//   VerletNVT / VerletNVE kernels           Integrator/VerletNVT/GronbechJensen.cu:28-62, Basic.cu:12-29,86-114,173-207, VerletNVE.cu:64-85
//
// Layout-generic on purpose, in the spirit of f64.hip: the build is hash -> rocPRIM's stable radix sort (uammd_sort_pairs) -> one kernel
// that gathers the 32-byte rows and fills the cell tables.  The counting-sort build, the LDS window ranks, the tile (MFMA) traversal, the
// fused MD step and the ghost / profiling hooks of the single-precision path are single precision only.
//
// The two traversal kernels share one shape, k_lj_general's (lj.hip): a lane per sorted particle SCANS its candidates (distance test only)
// and pushes the index of every hit into a per-lane FIFO in LDS; when some lane's FIFO is nearly full the wave DRAINS, every lane
// evaluating its queued pairs in FIFO order, so the double division and the force polynomial run on converged lanes and the sum keeps
// the reference's neighbour order.  GENERAL scans the double positions; SCAN32 scans a single-precision image of them with a widened
// cut-off (a strict superset, margins derived at scan32_threshold) and leaves the exact test to the drain: the same bits.
#include "md_f64.hpp"
#include "saru.hpp"

#include <cmath>

namespace uammd_hip {
namespace {

using md64::kPadRows;
using namespace md64d;  // the handle and the pair evaluation: md_f64.hpp
constexpr int kB = 256;
inline int nblk(long long n) { return (int)((n + kB - 1) / kB); }

// ---- cell list --------------------------------------------------------------------------------------------------------------------
// K1: hash = Morton(getCell(pos)), index = i.  A NaN or a particle outside a non-periodic box has no cell: it takes the key behind the
// last cell's (it sorts to the end, no table mentions it, the traversals skip it) and raises the flag.
__global__ void __launch_bounds__(kB) k64_hash(const double4 *__restrict__ pos, int N, GridT<double> grid, uint badKey,
                                               uint *__restrict__ hash, int *__restrict__ index, int *__restrict__ errorFlag) {
  const int i = blockIdx.x * kB + threadIdx.x;
  if (i >= N) return;
  const double4 p = pos[i];
  const int3 c = grid.getCell(real3d{p.x, p.y, p.z});
  uint h = morton_hash(c);
  if (!in_grid(grid, c) || !(p.x == p.x && p.y == p.y && p.z == p.z)) {  // (int)NaN is a valid-looking cell 0: test it by name
    errorFlag[0] = 1;
    h = badKey;
  }
  hash[i] = h;
  index[i] = i;
}

// The position folded into the list's box, on the side of the box its cell is on: Grid::getCell sends the index cellDim (a coordinate
// that rounds to +L/2) to cell 0, and the image follows it there.  What the single-precision image holds and what SCAN32 measures from.
UH_D real3d fold_to_cell(const GridT<double> &g, real3d r) {
  real3d p = g.box.apply_pbc(r);
  if (g.box.px() && (int)((p.x + 0.5 * g.box.boxSize.x) * g.invCellSize.x) == g.cellDim.x) p.x -= g.box.boxSize.x;
  if (g.box.py() && (int)((p.y + 0.5 * g.box.boxSize.y) * g.invCellSize.y) == g.cellDim.y) p.y -= g.box.boxSize.y;
  if (g.box.pz() && (int)((p.z + 0.5 * g.box.boxSize.z) * g.invCellSize.z) == g.cellDim.z) p.z -= g.box.boxSize.z;
  return p;
}

// K3 + K4 on the sorted (key, index) pairs: sortPos[id] = pos[index[id]], its single-precision image, and cellStart / cellEnd from the
// key boundaries (a sorted particle's cell is its key's: the same cell fillCellList recomputes from the position).  cellOutside[cell] = 1
// when some member is stored outside the primary box (the traversal then applies the minimum image to that cell's pairs).
__global__ void __launch_bounds__(kB) k64_reorder_fill(const double4 *__restrict__ pos, const int *__restrict__ index,
                                                       const uint *__restrict__ sortHash, int N, GridT<double> grid, uint validCell,
                                                       uint maxHash, double4 *__restrict__ sortPos, float4 *__restrict__ sortPos32,
                                                       uint *__restrict__ cellStart, int *__restrict__ cellEnd,
                                                       unsigned char *__restrict__ cellOutside) {
  const int id = blockIdx.x * kB + threadIdx.x;
  if (id >= N + kPadRows) return;
  if (id >= N) {  // the rows the traversals' grouped loads may touch behind the last particle
    sortPos[id] = make_double4(0.0, 0.0, 0.0, 0.0);
    sortPos32[id] = make_float4(0.f, 0.f, 0.f, 0.f);
    return;
  }
  const double4 p = pos[index[id]];
  sortPos[id] = p;
  const real3d pf = fold_to_cell(grid, real3d{p.x, p.y, p.z});
  sortPos32[id] = make_float4((float)pf.x, (float)pf.y, (float)pf.z, 0.f);
  const uint h = sortHash[id];
  if (h > maxHash) return;  // no cell
  const int icell = grid.getCellIndex(cell_of_key(h));
  const double hx = 0.5 * grid.box.boxSize.x, hy = 0.5 * grid.box.boxSize.y, hz = 0.5 * grid.box.boxSize.z;
  if (!(p.x >= -hx && p.x < hx && p.y >= -hy && p.y < hy && p.z >= -hz && p.z < hz)) cellOutside[icell] = 1;  // benign race: every writer stores 1
  const uint hPrev = id > 0 ? sortHash[id - 1] : 0u;
  if (id == 0 || hPrev != h) {
    cellStart[icell] = (uint)id + validCell;
    if (id > 0) cellEnd[grid.getCellIndex(cell_of_key(hPrev))] = id;
  }
  if (id == N - 1 || sortHash[id + 1] > maxHash) cellEnd[icell] = id + 1;
}

// ---- Lennard-Jones (the pair evaluation is in md_f64.hpp) ---------------------------------------------------------------------------
// The per-lane FIFO: entry t of lane l lives at queue[t * 128 + l]; its state is ONE 32-bit LDS address per lane (the next free entry),
// so that an append is a masked ds_write and an add (lj_scan of lj.hip).
using LdsU32 = __attribute__((address_space(3))) uint;
constexpr uint kQStep = 128 * sizeof(uint);
constexpr int kQCap64 = 24;       // FIFO depth of the cell-list kernels
constexpr int kQCapNBody64 = 32;  // ... of the all-pairs kernel

// what a drain needs besides the FIFO
template <bool NT1> struct PairCtx {
  const double4 *__restrict__ P;  // rows the queued indices refer to
  double4 pi;
  BoxT<double> box;
  LJParams64 p1;
  const LJParams64 *tbl;
  int ntypes;
};

template <bool PBC, bool NT1, bool WE, bool WV>
UH_D void lj_drain64(Acc64 &acc, uint q0, uint &qa, const PairCtx<NT1> &c) {
  const int n = (int)((qa - q0) / kQStep);
  for (int t = 0; t < n; t += 4) {
    uint jj[4];
    double4 r[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) jj[u] = *(const LdsU32 *)(uintptr_t)(q0 + (uint)min(t + u, n - 1) * kQStep);
#pragma unroll
    for (int u = 0; u < 4; ++u) r[u] = c.P[jj[u]];
    real3d d[4];
    double f[4], e[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (NT1) lj_eval64<PBC, WE>(c.box, c.p1, c.pi, r[u], d[u], f[u], e[u]);
      else lj_eval64<PBC, WE>(c.box, lj_lookup64(c.tbl, c.ntypes, (int)c.pi.w, (int)r[u].w), c.pi, r[u], d[u], f[u], e[u]);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {  // added in FIFO order; the clamped tail repeats the last pair with weight 0
      const bool live = t + u < n;
      lj_acc64<WE, WV>(acc, d[u], live ? f[u] : 0.0, live ? e[u] : 0.0);
    }
  }
  qa = q0;
}
template <bool NT1, bool WE, bool WV> UH_D void lj_drain64(bool pbc, Acc64 &acc, uint q0, uint &qa, const PairCtx<NT1> &c) {
  if (pbc) lj_drain64<true, NT1, WE, WV>(acc, q0, qa, c);
  else lj_drain64<false, NT1, WE, WV>(acc, q0, qa, c);
}

// Scans j in [jb, je) in order, four double rows per trip; rc2 = the table's largest squared cut-off (the drain applies the pair's own).
// !(r2 >= rc2) keeps NaN pairs, like the reference.  Rows past je are other particles or the padding behind the array, masked by u < rem.
template <bool PBC, int QCAP, bool NT1, bool WE, bool WV>
UH_D void lj_scan64(Acc64 &acc, uint q0, uint &qa, bool drainPBC, int jb, int je, double rc2, const PairCtx<NT1> &c) {
  for (int j = jb; j < je; j += 4) {
    if (__any(qa > q0 + (QCAP - 4) * kQStep)) lj_drain64<NT1, WE, WV>(drainPBC, acc, q0, qa, c);  // wave-uniform: some lane could not take 4 more
    const double4 *__restrict__ pj = c.P + j;
    double4 r[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) r[u] = pj[u];
    double d[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) d[u] = lj_dist2_64<PBC>(c.box, c.pi, r[u]);
    const int rem = je - j;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const bool hit = !(d[u] >= rc2) & (u < rem);
      if (hit) { *(LdsU32 *)(uintptr_t)qa = (uint)(j + u); qa += kQStep; }
    }
  }
}

// SCAN32's test.  The image holds x_j = fl32(X_j), X_j the member's position folded into the list's box (fold_to_cell); the lane holds
// x_i = fl32(X_i - k L), its own folded position moved by the whole box lengths k in {-1, 0, 1} that bring it next to the neighbour cell
// it is scanning (the neighbour cell's wrap).  On the grids SCAN32 runs on (md64::scan32_covers: the potential's box is the list's, every
// periodic direction has >= 5 cells) D = X_j - (X_i - k L) has |D_k| <= 2 cells <= 0.4 L, so it IS the minimum image the drain measures.
// With u = 2^-24 and M = max_k (L_k / 2 + cell_k) >= |X_j|, |X_i - k L|:
//   rounding of the two coordinates      |x_j - X_j|, |x_i - (X_i - k L)| <= u M
//   float subtraction d = fl(x_j - x_i)  |d - (x_j - x_i)| <= u |x_j - x_i| <= u (|D| + 2 u M)
//   so for a pair inside the cut-off     e := |d - D| <= u (2 M + rc) (1 + u)            per component, |D| < rc
//   sum of squares S = sum d_k^2         S <= |D|^2 + 2 sqrt(3) rc e + 3 e^2
//   its float evaluation (mul, 2 fma)    d32 <= S (1 + u)^3 <= S (1 + 3.01 u)
// The test is d32 < rc2 (1 + m) + a with m = 2^-21 = 8 u and a = 4 rc e: for e <= rc / 1024 (otherwise the threshold is +inf: every
// candidate is queued, still a superset) 2 sqrt(3) rc e + 3 e^2 <= 3.47 rc e and (|D|^2 + 3.47 rc e)(1 + 3.01 u) < rc2 (1 + 3.01 u) +
// 3.48 rc e.  What is left, 4.99 u rc2 + 0.52 rc e >= 0.52 rc u L, pays for the roundings on the double side (the fold, k L, and the
// drain's own r2 from the unfolded rows: a few 2^-53 |stored coordinate| each, below it for |stored coordinate| < 2^20 L) and for rounding
// the threshold to float, which is done upwards.  A pair the image lets through wrongly costs one masked evaluation and no bit.
UH_D float scan32_threshold(double rc2, double reachM) {
  const double u = 0x1p-24;
  const double rc = sqrt(rc2);
  const double e = u * (2.0 * reachM + rc) * (1.0 + 0x1p-20);
  const double thr = rc2 * (1.0 + 0x1p-21) + 4.0 * rc * e;
  float t = (float)thr;
  if ((double)t < thr) t = nextafterf(t, __builtin_inff());
  if (!(e <= rc * 0x1p-10)) t = __builtin_inff();
  return t;
}

// Eight rows of the image per trip: 16 bytes and single-precision arithmetic a candidate instead of 32 bytes at the double rate.
template <int QCAP, bool NT1, bool WE, bool WV>
UH_D void lj_scan32(Acc64 &acc, uint q0, uint &qa, bool drainPBC, const float4 *__restrict__ P32, int jb, int je, real3f xi, float thr,
                    const PairCtx<NT1> &c) {
  for (int j = jb; j < je; j += 8) {
    if (__any(qa > q0 + (QCAP - 8) * kQStep)) lj_drain64<NT1, WE, WV>(drainPBC, acc, q0, qa, c);
    const float4 *__restrict__ pj = P32 + j;
    float4 r[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) r[u] = pj[u];
    float d[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) d[u] = dot3(real3f{r[u].x - xi.x, r[u].y - xi.y, r[u].z - xi.z}, real3f{r[u].x - xi.x, r[u].y - xi.y, r[u].z - xi.z});
    const int rem = je - j;
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const bool hit = !(d[u] >= thr) & (u < rem);
      if (hit) { *(LdsU32 *)(uintptr_t)qa = (uint)(j + u); qa += kQStep; }
    }
  }
}

struct View64 {
  const uint *cellStart;
  const int *cellEnd;
  const double4 *sortPos;
  const float4 *sortPos32;
  const int *groupIndex;
  const uint *sortHash;
  const unsigned char *cellOutside;
  uint validCell, maxHash;
  int N;
};
// A lane per sorted particle, 128 lanes per workgroup.  The minimum image is the identity (offset 0, r + 0 L == r) for a pair whose two
// particles are stored inside the primary box and whose cells are direct (unwrapped) neighbours on a grid with >= 5 cells per direction
// built on the potential's box: then |d| <= 2 cells <= 0.4 L and floor(d (-1 / L) + 0.5) == 0 exactly.  It is skipped per neighbour cell
// for the whole wave, as in k_lj_general.  S32: reachM = max_k (L_k / 2 + cell_k) of the list's grid (scan32_threshold).
template <bool NT1, bool WE, bool WV, bool S32>
__global__ void __launch_bounds__(128) k64_lj(View64 cl, GridT<double> grid, BoxT<double> box, const LJParams64 *__restrict__ tbl, int ntypes,
                                              Out64 out, double reachM) {
  __shared__ uint gq[kQCap64 * 128];
  const int id = (int)xcd_contiguous_block(blockIdx.x, gridDim.x) * 128 + threadIdx.x;
  if (id >= cl.N) return;
  const uint key = cl.sortHash[id];
  if (key > cl.maxHash) return;  // a particle without a cell: nothing is computed for it
  const int gi = cl.groupIndex[id];
  const int ori = out.globalIndex ? out.globalIndex[gi] : gi;
  PairCtx<NT1> c{cl.sortPos, cl.sortPos[id], box, tbl[0], tbl, ntypes};
  const double4 &pi = c.pi;
  const double rc2 = NT1 ? c.p1.cutOff2 : lj_max_cutoff2_64(tbl, ntypes);
  const uint q0 = (uint)(uintptr_t)(LdsU32 *)(gq + threadIdx.x);
  uint qa = q0;
  Acc64 acc;

  const int3 n = grid.cellDim;
  const int npx = n.x > 1 ? 3 : 1, npy = n.y > 1 ? 3 : 1, npz = n.z > 1 ? 3 : 1;
  const int numberNeighbourCells = npx * npy * npz;
  const int3 celli = cell_of_key(key);
  const bool sameBox = box.boxSize.x == grid.box.boxSize.x && box.boxSize.y == grid.box.boxSize.y && box.boxSize.z == grid.box.boxSize.z &&
                       box.px() == grid.box.px() && box.py() == grid.box.py() && box.pz() == grid.box.pz();
  const bool smallGrid = n.x < 5 || n.y < 5 || n.z < 5 || !sameBox;
  const double hx = 0.5 * box.boxSize.x, hy = 0.5 * box.boxSize.y, hz = 0.5 * box.boxSize.z;
  const bool iOut = !(pi.x >= -hx && pi.x < hx && pi.y >= -hy && pi.y < hy && pi.z >= -hz && pi.z < hz);
  real3d pif{0.0, 0.0, 0.0};
  float thr = 0.f;
  if (S32) {
    pif = fold_to_cell(grid, real3d{pi.x, pi.y, pi.z});
    thr = scan32_threshold(rc2, reachM);
  }
  bool drainPBC = false;
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
    if (in_grid(grid, cellj)) {  // outside a non periodic box: no such cell (DESIGN.md "non-periodic neighbours")
      const int icellj = grid.getCellIndex(cellj);
      const uint cs = cl.cellStart[icellj];
      if (cs >= cl.validCell) {
        first = (int)(cs - cl.validCell);
        last = cl.cellEnd[icellj];
        const bool wrapped = raw.x != cellj.x || raw.y != cellj.y || raw.z != cellj.z;
        needPBC = smallGrid || iOut || wrapped || cl.cellOutside[icellj] != 0;
      }
    }
    if (__any(needPBC)) drainPBC = true;  // the full minimum image is exact for every pair already queued
    if (S32) {
      // the neighbour cell sits k = (raw - wrapped) / cellDim box lengths from where its members are stored
      const real3f xi{(float)(pif.x - (double)((raw.x - cellj.x) / n.x) * grid.box.boxSize.x),
                      (float)(pif.y - (double)((raw.y - cellj.y) / n.y) * grid.box.boxSize.y),
                      (float)(pif.z - (double)((raw.z - cellj.z) / n.z) * grid.box.boxSize.z)};
      lj_scan32<kQCap64, NT1, WE, WV>(acc, q0, qa, drainPBC, cl.sortPos32, first, last, xi, thr, c);
    } else if (drainPBC) {
      lj_scan64<true, kQCap64, NT1, WE, WV>(acc, q0, qa, true, first, last, rc2, c);
    } else {
      lj_scan64<false, kQCap64, NT1, WE, WV>(acc, q0, qa, false, first, last, rc2, c);
    }
  }
  lj_drain64<NT1, WE, WV>(drainPBC, acc, q0, qa, c);
  write_out64(out, ori, acc);
}

// All pairs, j ascending over the group (NBodyBase.cuh:79-110): 128-row tiles staged in LDS, rows in input order (k_lj_nbody).
template <bool NT1, bool WE, bool WV>
__global__ void __launch_bounds__(128) k64_lj_nbody(const double4 *__restrict__ pos, int N, BoxT<double> box, const LJParams64 *__restrict__ tbl,
                                                    int ntypes, Out64 out) {
  __shared__ double4 tile[128];
  __shared__ uint nq[kQCapNBody64 * 128];
  const int t = blockIdx.x * 128 + threadIdx.x;
  const bool active = t < N;
  const int id = active ? (out.globalIndex ? out.globalIndex[t] : t) : 0;
  PairCtx<NT1> c{tile, active ? pos[id] : make_double4(0.0, 0.0, 0.0, 0.0), box, tbl[0], tbl, ntypes};
  const double rc2 = NT1 ? c.p1.cutOff2 : lj_max_cutoff2_64(tbl, ntypes);
  const uint q0 = (uint)(uintptr_t)(LdsU32 *)(nq + threadIdx.x);
  uint qa = q0;
  Acc64 acc;
  const int numTiles = (N + 127) / 128;
  for (int tileIdx = 0; tileIdx < numTiles; ++tileIdx) {
    const int iload = tileIdx * 128 + threadIdx.x;
    // rows past N keep the previous tile's contents or are zero: the scan masks them (u < rem)
    tile[threadIdx.x] = iload < N ? pos[out.globalIndex ? out.globalIndex[iload] : iload] : make_double4(0.0, 0.0, 0.0, 0.0);
    __syncthreads();
    if (active) {
      const int cnt = min(128, N - tileIdx * 128);
      lj_scan64<true, kQCapNBody64, NT1, WE, WV>(acc, q0, qa, true, 0, cnt, rc2, c);
      lj_drain64<true, NT1, WE, WV>(acc, q0, qa, c);  // queue indices are tile-local
    }
    __syncthreads();
  }
  if (active) write_out64(out, id, acc);
}

// ---- integrators: one streaming kernel each, a lane per particle --------------------------------------------------------------------
// Saru is keyed exactly as in the single-precision kernels; the Gaussians are Saru's single-precision Box-Muller pair promoted to double,
// as the reference's double build draws them (third_party/saruprng.cuh:115-128 gf; uammd_bd_scheme_step_f64 does the same).
template <int STEP>
__global__ void __launch_bounds__(kB) k64_verletnvt_gj(double4 *__restrict__ pos, double *__restrict__ vel, double4 *__restrict__ force,
                                                       const double *__restrict__ mass, double defaultMass, const int *__restrict__ index,
                                                       int N, double dt, double friction, int is2D, double noiseAmplitude, uint stepNum,
                                                       uint seed) {
  const int id = blockIdx.x * kB + threadIdx.x;
  if (id >= N) return;
  const int i = index ? index[id] : id;
  const double invMass = 1.0 / (defaultMass > 0 ? defaultMass : mass[i]);
  real3d v{vel[3 * (size_t)i], vel[3 * (size_t)i + 1], vel[3 * (size_t)i + 2]};
  const double4 f = force[i];
  if (STEP == 1) {  // GronbechJensen.cu:36-57
    Saru rng((uint)id, stepNum, seed);
    noiseAmplitude *= 1.0 / sqrt(invMass);
    const float2 n01 = rng.gf(0.0f, (float)noiseAmplitude);
    double nx = n01.x, ny = n01.y, nz = 0.0;
    if (!is2D) nz = rng.gf(0.0f, (float)noiseAmplitude).x;
    const double gdthalfinvMass = friction * dt * 0.5;
    const double b = 1.0 / (1.0 + gdthalfinvMass);
    const double a = (1.0 - gdthalfinvMass) * b;
    double4 p = pos[i];
    const double bdt = b * dt;
    const double c = 0.5 * invMass * dt * b;
    p.x = fma(c, fma(dt, f.x, nx), fma(bdt, v.x, p.x));
    p.y = fma(c, fma(dt, f.y, ny), fma(bdt, v.y, p.y));
    p.z = fma(c, fma(dt, f.z, nz), fma(bdt, v.z, p.z));
    pos[i] = p;
    const double d = dt * 0.5 * invMass * a;
    const double e = b * invMass;
    v.x = fma(e, nx, fma(d, f.x, a * v.x));
    v.y = fma(e, ny, fma(d, f.y, a * v.y));
    v.z = fma(e, nz, fma(d, f.z, a * v.z));
    force[i] = make_double4(0.0, 0.0, 0.0, 0.0);
  } else {
    const double d = dt * 0.5 * invMass;
    v.x = fma(d, f.x, v.x);
    v.y = fma(d, f.y, v.y);
    v.z = fma(d, f.z, v.z);
  }
  if (is2D) v.z = 0.0;
  vel[3 * (size_t)i] = v.x; vel[3 * (size_t)i + 1] = v.y; vel[3 * (size_t)i + 2] = v.z;
}

template <int STEP>
__global__ void __launch_bounds__(kB) k64_verletnvt_basic(double4 *__restrict__ pos, double *__restrict__ vel, double4 *__restrict__ force,
                                                          const double *__restrict__ mass, double defaultMass,
                                                          const int *__restrict__ index, int N, double dt, double friction, int is2D,
                                                          double noiseAmplitude, uint stepNum, uint seed) {
  const int id = blockIdx.x * kB + threadIdx.x;
  if (id >= N) return;
  const int i = index ? index[id] : id;
  const double invMass = 1.0 / (defaultMass > 0 ? defaultMass : mass[i]);
  Saru rng((uint)(id + N * (STEP - 1)), stepNum, seed);  // Basic.cu:92
  noiseAmplitude *= (double)sqrtf((float)(0.5 * invMass));
  const float2 n01 = rng.gf(0.0f, (float)noiseAmplitude);
  const double nx = n01.x, ny = n01.y, nz = rng.gf(0.0f, (float)noiseAmplitude).x;
  real3d v{vel[3 * (size_t)i], vel[3 * (size_t)i + 1], vel[3 * (size_t)i + 2]};
  const double4 f = force[i];
  const double hdt = dt * 0.5;
  v.x = v.x + fma(fma(f.x, invMass, -(friction * v.x)), hdt, nx);
  v.y = v.y + fma(fma(f.y, invMass, -(friction * v.y)), hdt, ny);
  v.z = v.z + fma(fma(f.z, invMass, -(friction * v.z)), hdt, nz);
  if (is2D) v.z = 0.0;
  vel[3 * (size_t)i] = v.x; vel[3 * (size_t)i + 1] = v.y; vel[3 * (size_t)i + 2] = v.z;
  if (STEP == 1) {
    double4 p = pos[i];
    p.x = fma(v.x, dt, p.x);
    p.y = fma(v.y, dt, p.y);
    p.z = fma(v.z, dt, p.z);
    pos[i] = p;
    force[i] = make_double4(0.0, 0.0, 0.0, 0.0);
  }
}

// VerletNVE.cu:64-85: the mass array wins over defaultMass whenever it is there; forces are read only
template <int STEP>
__global__ void __launch_bounds__(kB) k64_verletnve(double4 *__restrict__ pos, double *__restrict__ vel, const double4 *__restrict__ force,
                                                    const double *__restrict__ mass, double defaultMass, const int *__restrict__ index, int N,
                                                    double dt, int is2D) {
  const int id = blockIdx.x * kB + threadIdx.x;
  if (id >= N) return;
  const int i = index ? index[id] : id;
  const double m = mass ? mass[i] : defaultMass;
  const double4 f = force[i];
  real3d v{vel[3 * (size_t)i], vel[3 * (size_t)i + 1], vel[3 * (size_t)i + 2]};
  v.x = v.x + (f.x / m) * dt * 0.5;
  v.y = v.y + (f.y / m) * dt * 0.5;
  v.z = v.z + (f.z / m) * dt * 0.5;
  if (is2D) v.z = 0.0;
  vel[3 * (size_t)i] = v.x; vel[3 * (size_t)i + 1] = v.y; vel[3 * (size_t)i + 2] = v.z;
  if (STEP == 1) {
    double4 p = pos[i];
    p.x = p.x + v.x * dt;
    p.y = p.y + v.y * dt;
    p.z = p.z + v.z * dt;
    pos[i] = p;
  }
}

// Basic.cu:12-29 (mass ignored, one look-up of the group iterator: k_initial_velocities); gd() = float uniforms and float libm, scaled in double
__global__ void __launch_bounds__(kB) k64_initial_velocities(double *__restrict__ vel, const int *__restrict__ index, double vamp, int is2D, int N,
                                                             uint seed) {
  const int id = blockIdx.x * kB + threadIdx.x;
  if (id >= N) return;
  Saru rng((uint)id, seed);
  const int i = index ? index[id] : id;
  auto gd = [&](double mean, double std, double &o0, double &o1) {
    const double pi2 = 2.0 * 3.14159265358979323846;
    double u0;
    do { u0 = rng.f(); } while (u0 <= 2.2250738585072014e-308);
    const double u1 = rng.f();
    const double r = sqrtf((float)(-2.0 * logf((float)u0)));
    const double theta = pi2 * u1;
    o0 = r * sinf((float)theta) * std + mean;
    o1 = r * cosf((float)theta) * std + mean;
  };
  double nx, ny, nz = 0.0, tmp;
  gd(0.0, vamp, nx, ny);
  if (!is2D) gd(0.0, vamp, nz, tmp);
  vel[3 * (size_t)i] = nx; vel[3 * (size_t)i + 1] = ny; vel[3 * (size_t)i + 2] = nz;
}

// Basic.cu:173-207: energy[i] += 0.5 m |v|^2
__global__ void __launch_bounds__(kB) k64_sum_kinetic_energy(const double *__restrict__ vel, double *__restrict__ energy,
                                                             const double *__restrict__ mass, double defaultMass, const int *__restrict__ index,
                                                             int N) {
  const int id = blockIdx.x * kB + threadIdx.x;
  if (id >= N) return;
  const int i = index ? index[id] : id;
  const double vx = vel[3 * (size_t)i], vy = vel[3 * (size_t)i + 1], vz = vel[3 * (size_t)i + 2];
  const double m = (defaultMass > 0.0 || !mass) ? defaultMass : mass[i];
  energy[i] += 0.5 * fma(vz, vz, fma(vy, vy, vx * vx)) * m;
}

// ---- host -------------------------------------------------------------------------------------------------------------------------
int update64(CellList64 *h, const double4 *d_pos, int N, const double L[3], const int periodic[3], const int cellDim[3], hipStream_t st) {
  if (!h->hostErr) {
    UH_CHECK(hipHostMalloc((void **)&h->hostErr, 64, hipHostMallocMapped));
    h->hostErr[0] = 0;
    UH_CHECK(hipHostGetDevicePointer((void **)&h->devErr, h->hostErr, 0));
  }
  if (int e = h->check_errors(st, false)) return e;  // raised by an earlier build
  const BoxT<double> box = make_box<double>(L, periodic);
  h->grid = make_grid<double>(box, make_int3(cellDim[0], cellDim[1], cellDim[2]));
  for (int k = 0; k < 3; ++k) { h->boxL[k] = L[k]; h->boxPeriodic[k] = periodic[k] != 0; }
  const GridT<double> &g = h->grid;
  const long long ncells = (long long)g.cellDim.x * g.cellDim.y * g.cellDim.z;
  const md64::BufferBytes bytes = md64::buffer_bytes(N, ncells);
  const bool cellsResized = h->nCellsAlloc != ncells;
  const bool needsClear = h->epoch.next(N);
  if (int e = h->cellStart.reserve(bytes.cellStart)) return e;
  if (int e = h->cellEnd.reserve(bytes.cellEnd)) return e;
  if (int e = h->cellOutside.reserve(bytes.cellOutside)) return e;
  if (int e = h->hash.reserve(bytes.hash)) return e;
  if (int e = h->index.reserve(bytes.index)) return e;
  if (int e = h->sortPos.reserve(bytes.sortPos)) return e;
  if (int e = h->sortPos32.reserve(bytes.sortPos32)) return e;
  if (cellsResized || needsClear) UH_CHECK(hipMemsetAsync(h->cellStart.ptr, 0, bytes.cellStart, st));
  UH_CHECK(hipMemsetAsync(h->cellOutside.ptr, 0, bytes.cellOutside, st));
  h->nCellsAlloc = ncells;
  h->N = N;
  h->maxHash = morton_hash(make_int3(g.cellDim.x - 1, g.cellDim.y - 1, g.cellDim.z - 1));  // ParticleSorter.cuh:161
  const uint badKey = h->maxHash + 1u;
  hipLaunchKernelGGL(k64_hash, dim3(nblk(N)), dim3(kB), 0, st, d_pos, N, g, badKey, (uint *)h->hash.ptr, (int *)h->index.ptr, h->devErr);
  UH_CHECK(hipGetLastError());
  // a stable sort of (key, index) on the key's bits: the order is the reference's for every particle with a cell, whatever the width
  if (int e = uammd_sort_pairs((uint *)h->hash.ptr, (int *)h->index.ptr, N, md64::sort_end_bit(badKey), (void *)st)) return e;
  hipLaunchKernelGGL(k64_reorder_fill, dim3(nblk((long long)N + kPadRows)), dim3(kB), 0, st, d_pos, (const int *)h->index.ptr,
                     (const uint *)h->hash.ptr, N, g, h->epoch.validCell, h->maxHash, (double4 *)h->sortPos.ptr, (float4 *)h->sortPos32.ptr,
                     (uint *)h->cellStart.ptr, (int *)h->cellEnd.ptr, (unsigned char *)h->cellOutside.ptr);
  UH_CHECK(hipGetLastError());
  return 0;
}

// AUTO: the scan over the single-precision image where it covers the grid, else GENERAL.  Measured at 1e6 particles, rho* = 0.8: 0.562 ms
// against GENERAL's 0.70 ms in each of three alternating runs, the same bits (profiles/md_f64_lj.md).
constexpr bool kAutoScan32 = true;

template <bool NT1, bool WE, bool WV>
void launch_celllist64(bool s32, const View64 &cl, const GridT<double> &g, const BoxT<double> &box, const LJParams64 *tbl, int ntypes,
                       const Out64 &out, double reachM, hipStream_t st) {
  const dim3 grid((cl.N + 127) / 128), block(128);
  if (s32) hipLaunchKernelGGL((k64_lj<NT1, WE, WV, true>), grid, block, 0, st, cl, g, box, tbl, ntypes, out, reachM);
  else hipLaunchKernelGGL((k64_lj<NT1, WE, WV, false>), grid, block, 0, st, cl, g, box, tbl, ntypes, out, reachM);
}
template <bool NT1, bool WE, bool WV>
void launch_nbody64(const double4 *pos, int N, const BoxT<double> &box, const LJParams64 *tbl, int ntypes, const Out64 &out, hipStream_t st) {
  hipLaunchKernelGGL((k64_lj_nbody<NT1, WE, WV>), dim3((N + 127) / 128), dim3(128), 0, st, pos, N, box, tbl, ntypes, out);
}

// the kernels are instantiated for forces alone and for forces + energy + virial (outputs that were not asked for are null: write_out64)
#define UH_DISPATCH_FEV64(FN, ...)                                                   \
  do {                                                                               \
    const bool nt1 = ntypes == 1, ev = d_energy != nullptr || d_virial != nullptr;   \
    if (nt1 && !ev) FN<true, false, false>(__VA_ARGS__);                             \
    else if (nt1) FN<true, true, true>(__VA_ARGS__);                                 \
    else if (!ev) FN<false, false, false>(__VA_ARGS__);                              \
    else FN<false, true, true>(__VA_ARGS__);                                         \
  } while (0)

inline int nb(int n) { return (n + kB - 1) / kB; }

}  // namespace
}  // namespace uammd_hip

using namespace uammd_hip;

extern "C" {

int uammd_celllist_create_f64(uammd_celllist_f64 **out) {
  if (!out) { set_last_error("uammd_celllist_create_f64: null output"); return -1; }
  *out = reinterpret_cast<uammd_celllist_f64 *>(new CellList64());
  return 0;
}
int uammd_celllist_destroy_f64(uammd_celllist_f64 *h) {
  delete reinterpret_cast<CellList64 *>(h);
  return 0;
}

int uammd_celllist_create_grid_f64(const double L[3], const int periodic[3], const double cutOff[3], int cellDim_out[3], double L_out[3],
                                   int periodic_out[3]) {
  if (!L || !periodic || !cutOff || !cellDim_out || !L_out || !periodic_out) { set_last_error("uammd_celllist_create_grid_f64: null argument"); return -1; }
  md64::create_grid(L, periodic, cutOff, cellDim_out, L_out, periodic_out);
  return 0;
}

int uammd_celllist_update_f64(uammd_celllist_f64 *hh, const double *d_pos, int numberParticles, const double L[3], const int periodic[3],
                              const int cellDim[3], void *stream) {
  if (const char *msg = md64::check_update(hh, d_pos, numberParticles, L, periodic, cellDim)) { set_last_error("%s", msg); return -2; }
  if (numberParticles == 0) return 0;
  return update64(reinterpret_cast<CellList64 *>(hh), reinterpret_cast<const double4 *>(d_pos), numberParticles, L, periodic, cellDim,
                  (hipStream_t)stream);
}

int uammd_celllist_get_f64(uammd_celllist_f64 *hh, uammd_celllist_data_f64 *out) {
  if (!hh || !out) { set_last_error("uammd_celllist_get_f64: null argument"); return -1; }
  CellList64 *h = reinterpret_cast<CellList64 *>(hh);
  if (int e = h->check_errors(nullptr, false)) return e;
  out->d_cellStart = (const unsigned int *)h->cellStart.ptr;
  out->d_cellEnd = (const int *)h->cellEnd.ptr;
  out->d_sortPos = (const double *)h->sortPos.ptr;
  out->d_groupIndex = (const int *)h->index.ptr;
  out->d_sortHash = (const unsigned int *)h->hash.ptr;
  out->cellDim[0] = h->grid.cellDim.x; out->cellDim[1] = h->grid.cellDim.y; out->cellDim[2] = h->grid.cellDim.z;
  for (int k = 0; k < 3; ++k) { out->boxSize[k] = h->boxL[k]; out->periodic[k] = h->boxPeriodic[k]; }
  out->VALID_CELL = h->epoch.validCell;
  out->numberParticles = h->N;
  return 0;
}

int uammd_celllist_check_errors_f64(uammd_celllist_f64 *hh, void *stream) {
  if (!hh) { set_last_error("uammd_celllist_check_errors_f64: null handle"); return -1; }
  return reinterpret_cast<CellList64 *>(hh)->check_errors((hipStream_t)stream, true);
}

int uammd_lj_process_pair_parameters_f64(double cutOff, double sigma, double epsilon, int shift, uammd_lj_pair_parameters_f64 *out) {
  if (!out) { set_last_error("uammd_lj_process_pair_parameters_f64: null output"); return -1; }
  double p[4];
  md64::process_pair_parameters(cutOff, sigma, epsilon, shift, p);
  out->cutOff2 = p[0]; out->sigma2 = p[1]; out->epsilonDivSigma2 = p[2]; out->shift = p[3];
  return 0;
}

int uammd_lj_transverse_celllist_f64(uammd_celllist_f64 *hh, const uammd_lj_pair_parameters_f64 *d_paramTable, int ntypes, const double boxL[3],
                                     const int boxPeriodic[3], double *d_force, double *d_energy, double *d_virial, const int *d_globalIndex,
                                     int algo, void *stream) {
  if (const char *msg = md64::check_transverse(hh, d_paramTable, ntypes, boxL, boxPeriodic, algo)) { set_last_error("%s", msg); return -1; }
  CellList64 *h = reinterpret_cast<CellList64 *>(hh);
  hipStream_t st = (hipStream_t)stream;
  if (int e = h->check_errors(st, false)) return e;
  if (h->N == 0) return 0;
  const GridT<double> &g = h->grid;
  const BoxT<double> box = make_box<double>(boxL, boxPeriodic);
  const int cellDim[3] = {g.cellDim.x, g.cellDim.y, g.cellDim.z};
  const bool covered = md64::scan32_covers(cellDim, h->boxL, h->boxPeriodic, boxL, boxPeriodic);
  const bool s32 = covered && (algo == UAMMD_LJ_ALGO_SCAN32 || (algo == UAMMD_LJ_ALGO_AUTO && kAutoScan32));
  const double reachM = fmax(0.5 * g.box.boxSize.x + g.cellSize.x, fmax(0.5 * g.box.boxSize.y + g.cellSize.y, 0.5 * g.box.boxSize.z + g.cellSize.z));
  const View64 cl{(const uint *)h->cellStart.ptr, (const int *)h->cellEnd.ptr, (const double4 *)h->sortPos.ptr, (const float4 *)h->sortPos32.ptr,
                  (const int *)h->index.ptr, (const uint *)h->hash.ptr, (const unsigned char *)h->cellOutside.ptr, h->epoch.validCell, h->maxHash,
                  h->N};
  const Out64 out{reinterpret_cast<double4 *>(d_force), d_energy, d_virial, d_globalIndex};
  const LJParams64 *tbl = reinterpret_cast<const LJParams64 *>(d_paramTable);
  UH_DISPATCH_FEV64(launch_celllist64, s32, cl, g, box, tbl, ntypes, out, reachM, st);
  UH_CHECK(hipGetLastError());
  return 0;
}

int uammd_lj_transverse_nbody_f64(const double *d_pos, int numberParticles, const uammd_lj_pair_parameters_f64 *d_paramTable, int ntypes,
                                  const double boxL[3], const int boxPeriodic[3], double *d_force, double *d_energy, double *d_virial,
                                  const int *d_globalIndex, void *stream) {
  if (!d_pos || !d_paramTable || !boxL || !boxPeriodic || ntypes < 1) { set_last_error("uammd_lj_transverse_nbody_f64: bad arguments"); return -1; }
  if (numberParticles <= 0) return 0;
  const BoxT<double> box = make_box<double>(boxL, boxPeriodic);
  const Out64 out{reinterpret_cast<double4 *>(d_force), d_energy, d_virial, d_globalIndex};
  const LJParams64 *tbl = reinterpret_cast<const LJParams64 *>(d_paramTable);
  UH_DISPATCH_FEV64(launch_nbody64, reinterpret_cast<const double4 *>(d_pos), numberParticles, box, tbl, ntypes, out, (hipStream_t)stream);
  UH_CHECK(hipGetLastError());
  return 0;
}

int uammd_verletnvt_gj_f64(int step, double *d_pos, double *d_vel, double *d_force, const double *d_mass, double defaultMass, const int *d_index,
                           int N, double dt, double friction, int is2D, double noiseAmplitude, unsigned int stepNum, unsigned int seed,
                           void *stream) {
  if (N <= 0) return 0;
  if (!d_pos || !d_vel || !d_force) { set_last_error("uammd_verletnvt_gj_f64: null argument"); return -1; }
  if (step != 1 && step != 2) { set_last_error("uammd_verletnvt_gj_f64: step must be 1 or 2"); return -1; }
  if (!d_mass && !(defaultMass > 0)) { set_last_error("uammd_verletnvt_gj_f64: no mass array and defaultMass <= 0"); return -1; }
  hipStream_t st = (hipStream_t)stream;
  if (step == 1)
    hipLaunchKernelGGL(k64_verletnvt_gj<1>, dim3(nb(N)), dim3(kB), 0, st, (double4 *)d_pos, d_vel, (double4 *)d_force, d_mass, defaultMass, d_index,
                       N, dt, friction, is2D, noiseAmplitude, stepNum, seed);
  else
    hipLaunchKernelGGL(k64_verletnvt_gj<2>, dim3(nb(N)), dim3(kB), 0, st, (double4 *)d_pos, d_vel, (double4 *)d_force, d_mass, defaultMass, d_index,
                       N, dt, friction, is2D, noiseAmplitude, stepNum, seed);
  UH_CHECK(hipGetLastError());
  return 0;
}

int uammd_verletnvt_basic_f64(int step, double *d_pos, double *d_vel, double *d_force, const double *d_mass, double defaultMass,
                              const int *d_index, int N, double dt, double friction, int is2D, double noiseAmplitude, unsigned int stepNum,
                              unsigned int seed, void *stream) {
  if (N <= 0) return 0;
  if (!d_pos || !d_vel || !d_force) { set_last_error("uammd_verletnvt_basic_f64: null argument"); return -1; }
  if (step != 1 && step != 2) { set_last_error("uammd_verletnvt_basic_f64: step must be 1 or 2"); return -1; }
  if (!d_mass && !(defaultMass > 0)) { set_last_error("uammd_verletnvt_basic_f64: no mass array and defaultMass <= 0"); return -1; }
  hipStream_t st = (hipStream_t)stream;
  if (step == 1)
    hipLaunchKernelGGL(k64_verletnvt_basic<1>, dim3(nb(N)), dim3(kB), 0, st, (double4 *)d_pos, d_vel, (double4 *)d_force, d_mass, defaultMass,
                       d_index, N, dt, friction, is2D, noiseAmplitude, stepNum, seed);
  else
    hipLaunchKernelGGL(k64_verletnvt_basic<2>, dim3(nb(N)), dim3(kB), 0, st, (double4 *)d_pos, d_vel, (double4 *)d_force, d_mass, defaultMass,
                       d_index, N, dt, friction, is2D, noiseAmplitude, stepNum, seed);
  UH_CHECK(hipGetLastError());
  return 0;
}

int uammd_verletnve_f64(int step, double *d_pos, double *d_vel, const double *d_force, const double *d_mass, double defaultMass,
                        const int *d_index, int N, double dt, int is2D, void *stream) {
  if (N <= 0) return 0;
  if (!d_pos || !d_vel || !d_force) { set_last_error("uammd_verletnve_f64: null argument"); return -1; }
  if (step != 1 && step != 2) { set_last_error("uammd_verletnve_f64: step must be 1 or 2"); return -1; }
  if (!d_mass && !(defaultMass > 0)) { set_last_error("uammd_verletnve_f64: no mass array and defaultMass <= 0"); return -1; }
  hipStream_t st = (hipStream_t)stream;
  if (step == 1)
    hipLaunchKernelGGL(k64_verletnve<1>, dim3(nb(N)), dim3(kB), 0, st, (double4 *)d_pos, d_vel, (const double4 *)d_force, d_mass, defaultMass,
                       d_index, N, dt, is2D);
  else
    hipLaunchKernelGGL(k64_verletnve<2>, dim3(nb(N)), dim3(kB), 0, st, (double4 *)d_pos, d_vel, (const double4 *)d_force, d_mass, defaultMass,
                       d_index, N, dt, is2D);
  UH_CHECK(hipGetLastError());
  return 0;
}

int uammd_verletnvt_initial_velocities_f64(double *d_vel, const int *d_index, double velAmplitude, int is2D, int N, unsigned int seed,
                                           void *stream) {
  if (N <= 0) return 0;
  if (!d_vel) { set_last_error("uammd_verletnvt_initial_velocities_f64: null argument"); return -1; }
  hipLaunchKernelGGL(k64_initial_velocities, dim3(nb(N)), dim3(kB), 0, (hipStream_t)stream, d_vel, d_index, velAmplitude, is2D, N, seed);
  UH_CHECK(hipGetLastError());
  return 0;
}

int uammd_sum_kinetic_energy_f64(const double *d_vel, double *d_energy, const double *d_mass, double defaultMass, const int *d_index, int N,
                                 void *stream) {
  if (N <= 0) return 0;
  if (!d_vel || !d_energy) { set_last_error("uammd_sum_kinetic_energy_f64: null argument"); return -1; }
  hipLaunchKernelGGL(k64_sum_kinetic_energy, dim3(nb(N)), dim3(kB), 0, (hipStream_t)stream, d_vel, d_energy, d_mass, defaultMass, d_index, N);
  UH_CHECK(hipGetLastError());
  return 0;
}

}  // extern "C"
