// Monte Carlo NVT on a checkerboard for gfx950 (Integrator/MonteCarlo/NVT/Anderson.cuh:47-119, Anderson.cu): one MC_NVT::Anderson step
// with Potential::LJ, the host draws (origin, subgrid order, seed) supplied by the caller.
//
//   shifted = pos + origin;  cell list of `shifted` on the MC grid (Anderson.cu:197-205);  sortPos = list.sortPos + (-origin) (:207-217)
//   per subgrid, in the caller's order (:219-231), per cell of it with rng = Saru(seed, step, icell), triesPerCell times (:302-349):
//     tried[icell]++;  i = first + int(rng.f() * nincell);  new = old + jump * (2 rng.f() - 1) per axis (z drawn and dropped in 2D)
//     getCell(new + origin) != cell -> next try, no further draw
//     dH = sum_j u(new, j) - sum_j u(old, j) over the 27 (9) cells, u = 0 at r2 == 0, the moved particle standing for itself
//     Z = rng.f();  accept if Z <= min(1, exp(-beta dH)):  sortPos[i] = new, accepted[icell]++
//   pos[groupIndex[k]] = sortPos[k] (Anderson.cuh:106-115)
// u is the PAIR energy: twice what Radial::Transverser::compute returns, which is the particle's half of it (Potential.cuh:47-65) —
// the reference puts the half into the Metropolis rule and so samples at 2 T.
//
// Shape.  The reference runs one thread per cell, every try walking ~27 cells of neighbours from global memory.  During
// a subgrid pass only a cell's own particles move and the other 26 cells belong to other subgrids, so here ONE WAVE owns a cell: it
// stages the rows of its 27 (9) cells in LDS once, every lane carries the same Saru state (the draws are wave-uniform without a
// broadcast), the lanes split the staged rows for the two energy sums, the sums are reduced in a fixed DPP order, the decision is
// wave-uniform and lane 0 updates the moved row in LDS.  After the last try the wave writes its own cell's rows back.  No atomics; two
// runs of one state give the same bits.  A neighbourhood above the staging capacity ("mc_stage_capacity") is walked in global memory
// instead, by the same wave.  k_mc_cell is the reference-shaped kernel ("mc_baseline" = 1): thread per cell, global memory.
// Every cell of the active subgrid is visited exactly once in 2D and 3D (the reference's launch does not: DESIGN.md 6).
#include "celllist.hpp"
#include "lj_common.hpp"
#include "saru.hpp"

#include <cstring>
#include <new>

namespace uammd_hip {

namespace mc {
int g_baseline = 0;          // "mc_baseline"
int g_stageCapacity = 512;   // "mc_stage_capacity": rows of LDS per wave (4 waves x (512 + 16) x 16 B = 33 KiB per workgroup)
constexpr int kMaxStageCapacity = 960;  // 4 x (960 + 16) x 16 B stays under the 64 KiB a launch gets without an attribute
constexpr int kWaves = 4;    // cells per workgroup
constexpr int kTab = 16;     // float4 rows after a wave's stage that hold its table: offsets at [0, 32), first rows at [32, 64)
}  // namespace mc

struct MCArgs {
  const uint *cellStart;
  const int *cellEnd;
  uint validCell;
  float4 *pos;  // list order, unshifted
  GridT<float> grid;
  BoxT<float> box;
  real3f origin;
  int3 off, half;  // the subgrid's offset and the number of its cells per axis
  int nsub, is2D, tries;
  float beta, jump;
  uint step, seed;
  const LJParams *tbl;
  int ntypes;
  uint *tried, *accepted;
  int cap;
};

struct MCAnderson {
  CellList cl;
  DeviceBuffer shifted, sortPos, counters, sums;
  int ncells = -1;
};

// half the pair energy, Radial::Transverser::compute (RadialPotential.cuh:107-118) with LJFunctor::energy
template <bool NT1>
UH_D float mc_pair(const BoxT<float> &box, const LJParams *__restrict__ tbl, int ntypes, const LJParams &p1, const float4 &ri, const float4 &rj) {
  const real3f r12 = box.apply_pbc(real3f{rj.x - ri.x, rj.y - ri.y, rj.z - ri.z});
  const float r2 = dot3(r12, r12);
  if (r2 == 0.0f) return 0.0f;
  const LJParams p = NT1 ? p1 : lj_lookup(tbl, ntypes, (int)ri.w, (int)rj.w);
  return lj_energy(r2, p);
}

UH_D int3 mc_cell_of(const MCArgs &a, int w) {
  int3 c;
  c.x = 2 * (w % a.half.x) + a.off.x;
  c.y = 2 * ((w / a.half.x) % a.half.y) + a.off.y;
  c.z = a.is2D ? 0 : 2 * (w / (a.half.x * a.half.y)) + a.off.z;
  return c;
}

// first row and number of rows of neighbour k of cell c (0 rows: empty, or past the edge of a non-periodic axis)
UH_D void mc_neighbour(const MCArgs &a, int3 c, int k, int &start, int &count) {
  start = count = 0;
  int3 n;
  n.x = a.grid.pbc_x(c.x + k % 3 - 1);
  n.y = a.grid.pbc_y(c.y + (k / 3) % 3 - 1);
  n.z = a.is2D ? c.z : a.grid.pbc_z(c.z + k / 9 - 1);
  if (n.x < 0 || n.x >= a.grid.cellDim.x || n.y < 0 || n.y >= a.grid.cellDim.y || n.z < 0 || n.z >= a.grid.cellDim.z) return;
  const int j = a.grid.getCellIndex(n);
  const uint cs = a.cellStart[j];
  if (cs < a.validCell) return;
  start = (int)(cs - a.validCell);
  count = a.cellEnd[j] - start;
}

struct MCTry {
  int idx;
  float4 old, nw;
  bool inCell;
};
// the draws of one try up to the cell test (Anderson.cu:325-336); Saru::f() can return 1: the pick is clamped to the cell's last row
UH_D MCTry mc_draw(const MCArgs &a, Saru &rng, int3 c, int nin, const float4 *rows) {
  MCTry t;
  t.idx = min((int)(rng.f() * nin), nin - 1);
  t.old = rows[t.idx];
  const float dx = a.jump * (2.0f * rng.f() - 1.0f);
  const float dy = a.jump * (2.0f * rng.f() - 1.0f);
  const float dz = a.jump * (2.0f * rng.f() - 1.0f);
  t.nw = make_float4(t.old.x + dx, t.old.y + dy, a.is2D ? t.old.z : t.old.z + dz, t.old.w);
  const int3 nc = a.grid.getCell(real3f{t.nw.x + a.origin.x, t.nw.y + a.origin.y, t.nw.z + a.origin.z});
  t.inCell = nc.x == c.x && nc.y == c.y && nc.z == c.z;
  return t;
}
UH_D bool mc_metropolis(const MCArgs &a, Saru &rng, float eOld, float eNew) {
  const float dH = 2.0f * (eNew - eOld);
  const float Z = rng.f();
  const float e = expf(-a.beta * dH);
  const float p = 1.0f < e ? 1.0f : e;  // uammd::min: a NaN is rejected
  return Z <= p;
}

UH_D void mc_wave_sync() {  // orders a wave's own LDS traffic (its lanes run in lockstep; no other wave shares these rows)
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

template <bool NT1>
__global__ void __launch_bounds__(64 * mc::kWaves) k_mc_wave(MCArgs a) {
  extern __shared__ float4 mcShared[];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int w = (int)blockIdx.x * mc::kWaves + wv;
  if (w >= a.nsub) return;
  float4 *stage = mcShared + (size_t)wv * (a.cap + mc::kTab);
  int *tab = reinterpret_cast<int *>(stage + a.cap);
  const int3 c = mc_cell_of(a, w);
  const int icell = a.grid.getCellIndex(c);
  const uint cs = a.cellStart[icell];
  if (cs < a.validCell) return;  // an empty cell draws nothing and counts nothing (Anderson.cu:316-318)
  const int first = (int)(cs - a.validCell);
  const int nin = a.cellEnd[icell] - first;
  if (nin <= 0) return;
  const int nn = a.is2D ? 9 : 27, ownK = a.is2D ? 4 : 13;
  int start = 0, count = 0;
  if (lane < nn) mc_neighbour(a, c, lane, start, count);
  const int incl = (int)wave_inclusive_scan((uint)count);
  const int total = __shfl(incl, 63);
  const int ownOff = __shfl(incl - count, ownK);
  if (lane < 32) {
    tab[lane] = lane < nn ? incl - count : total;
    tab[32 + lane] = start;
  }
  mc_wave_sync();
  // entry e of the neighbourhood -> its row in the list: the last cell whose offset is <= e
  auto row_of = [&](int e) {
    int k = 0;
    for (int q = 1; q < nn; ++q) k += e >= tab[q] ? 1 : 0;
    return tab[32 + k] + (e - tab[k]);
  };
  const bool staged = total <= a.cap;
  if (staged) {
    staged_copy<4, float4>(lane, total, 64, [&](int e) { return a.pos[row_of(e)]; }, [&](int e, const float4 &v) { stage[e] = v; });
    mc_wave_sync();
  }
  const LJParams p1 = a.tbl[0];
  Saru rng(a.seed, a.step, (uint)icell);
  uint accepted = 0;
  for (int t = 0; t < a.tries; ++t) {
    const MCTry tr = staged ? mc_draw(a, rng, c, nin, stage + ownOff) : mc_draw(a, rng, c, nin, a.pos + first);
    if (!tr.inCell) continue;
    const int moved = ownOff + tr.idx;
    float eOld = 0.0f, eNew = 0.0f;
    for (int e = lane; e < total; e += 64) {
      float4 pj = staged ? stage[e] : a.pos[row_of(e)];
      eOld += mc_pair<NT1>(a.box, a.tbl, a.ntypes, p1, tr.old, pj);
      if (e == moved) pj = tr.nw;
      eNew += mc_pair<NT1>(a.box, a.tbl, a.ntypes, p1, tr.nw, pj);
    }
    eOld = wave_total(eOld);
    eNew = wave_total(eNew);
    if (mc_metropolis(a, rng, eOld, eNew)) {
      ++accepted;
      if (staged) {
        if (lane == 0) stage[moved] = tr.nw;
        mc_wave_sync();
      } else {
        if (lane == 0) a.pos[first + tr.idx] = tr.nw;
        __threadfence();
      }
    }
  }
  if (staged)
    for (int j = lane; j < nin; j += 64) a.pos[first + j] = stage[ownOff + j];
  if (lane == 0) {
    a.tried[icell] += (uint)a.tries;
    a.accepted[icell] += accepted;
  }
}

// MCStepKernel's shape (Anderson.cu:302-349): one thread per cell of the subgrid, everything in global memory
template <bool NT1>
__global__ void __launch_bounds__(128) k_mc_cell(MCArgs a) {
  const int w = (int)blockIdx.x * 128 + threadIdx.x;
  if (w >= a.nsub) return;
  const int3 c = mc_cell_of(a, w);
  const int icell = a.grid.getCellIndex(c);
  const uint cs = a.cellStart[icell];
  if (cs < a.validCell) return;
  const int first = (int)(cs - a.validCell);
  const int nin = a.cellEnd[icell] - first;
  if (nin <= 0) return;
  const int nn = a.is2D ? 9 : 27;
  const LJParams p1 = a.tbl[0];
  Saru rng(a.seed, a.step, (uint)icell);
  uint accepted = 0;
  for (int t = 0; t < a.tries; ++t) {
    const MCTry tr = mc_draw(a, rng, c, nin, a.pos + first);
    if (!tr.inCell) continue;
    const int moved = first + tr.idx;
    float eOld = 0.0f, eNew = 0.0f;
    for (int k = 0; k < nn; ++k) {
      int start, count;
      mc_neighbour(a, c, k, start, count);
      for (int j = start; j < start + count; ++j) {
        float4 pj = a.pos[j];
        eOld += mc_pair<NT1>(a.box, a.tbl, a.ntypes, p1, tr.old, pj);
        if (j == moved) pj = tr.nw;
        eNew += mc_pair<NT1>(a.box, a.tbl, a.ntypes, p1, tr.nw, pj);
      }
    }
    if (mc_metropolis(a, rng, eOld, eNew)) {
      ++accepted;
      a.pos[moved] = tr.nw;
    }
  }
  a.tried[icell] += (uint)a.tries;
  a.accepted[icell] += accepted;
}

__global__ void __launch_bounds__(256) k_mc_shift(const float4 *__restrict__ in, float4 *__restrict__ out, int n, real3f o) {
  const int i = (int)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float4 p = in[i];
  out[i] = make_float4(p.x + o.x, p.y + o.y, p.z + o.z, p.w);
}
__global__ void __launch_bounds__(256) k_mc_scatter(const float4 *__restrict__ in, const int *__restrict__ index, float4 *__restrict__ out, int n) {
  const int i = (int)blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[index[i]] = in[i];
}
// sums[0] = sum tried, sums[1] = sum accepted; reset: the counters are zeroed behind the read
__global__ void __launch_bounds__(256) k_mc_sum(uint *__restrict__ tried, uint *__restrict__ accepted, int ncells, int reset,
                                                unsigned long long *__restrict__ sums) {
  __shared__ unsigned long long part[2][256];
  unsigned long long t = 0, ac = 0;
  for (int i = threadIdx.x; i < ncells; i += 256) {
    t += tried[i];
    ac += accepted[i];
    if (reset) tried[i] = accepted[i] = 0u;
  }
  part[0][threadIdx.x] = t;
  part[1][threadIdx.x] = ac;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) {
      part[0][threadIdx.x] += part[0][threadIdx.x + s];
      part[1][threadIdx.x] += part[1][threadIdx.x + s];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) { sums[0] = part[0][0]; sums[1] = part[1][0]; }
}

// Anderson_ns::checkGridValidity (Anderson.cu:67-73) plus what the checkerboard itself needs: even extents
static bool mc_grid_valid(const int cd[3]) {
  if (cd[0] < 3 || cd[1] < 3 || cd[2] == 2 || cd[2] < 1) return false;
  return cd[0] % 2 == 0 && cd[1] % 2 == 0 && (cd[2] == 1 || cd[2] % 2 == 0);
}

int mc_set_tunable(const char *name, int value) {
  if (!std::strcmp(name, "mc_baseline") && (value == 0 || value == 1)) { mc::g_baseline = value; return 0; }
  if (!std::strcmp(name, "mc_stage_capacity") && value >= 0 && value <= mc::kMaxStageCapacity) { mc::g_stageCapacity = value; return 0; }
  return -1;
}

}  // namespace uammd_hip

using namespace uammd_hip;

extern "C" {

int uammd_mc_anderson_create(uammd_mc_anderson **out) {
  if (!out) { set_last_error("uammd_mc_anderson_create: null argument"); return -1; }
  MCAnderson *h = new (std::nothrow) MCAnderson();
  if (!h) { set_last_error("uammd_mc_anderson_create: out of memory"); return -1; }
  *out = reinterpret_cast<uammd_mc_anderson *>(h);
  return 0;
}

int uammd_mc_anderson_destroy(uammd_mc_anderson *h) {
  delete reinterpret_cast<MCAnderson *>(h);
  return 0;
}

static int mc_counters_for(MCAnderson *h, int ncells, hipStream_t st) {
  if (h->ncells == ncells) return 0;
  if (int e = h->counters.reserve(2 * sizeof(uint) * (size_t)ncells)) return e;
  UH_CHECK(hipMemsetAsync(h->counters.ptr, 0, 2 * sizeof(uint) * (size_t)ncells, st));
  h->ncells = ncells;
  return 0;
}

int uammd_mc_anderson_step(uammd_mc_anderson *hh, float *d_pos, int numberParticles, const float boxL[3], const int boxPeriodic[3],
                           const int cellDim[3], const float origin[3], const int *subgridOrder, int numberSubgrids, int triesPerCell,
                           float beta, float jumpSize, unsigned int step, unsigned int seed,
                           const uammd_lj_pair_parameters *d_paramTable, int ntypes, void *stream) {
  if (!hh || !d_pos || !boxL || !boxPeriodic || !cellDim || !origin || !subgridOrder || !d_paramTable || ntypes < 1 || numberParticles < 0) {
    set_last_error("uammd_mc_anderson_step: null or bad argument");
    return -1;
  }
  if (!mc_grid_valid(cellDim)) {
    set_last_error("uammd_mc_anderson_step: invalid grid %d %d %d (needs even extents, x and y >= 3, z == 1 or z >= 4)", cellDim[0],
                   cellDim[1], cellDim[2]);
    return -1;
  }
  const bool is2D = cellDim[2] == 1;
  if (numberSubgrids != (is2D ? 4 : 8)) {
    set_last_error("uammd_mc_anderson_step: numberSubgrids must be %d for this grid, got %d", is2D ? 4 : 8, numberSubgrids);
    return -1;
  }
  for (int s = 0; s < numberSubgrids; ++s)
    if (subgridOrder[s] < 0 || subgridOrder[s] >= numberSubgrids) { set_last_error("uammd_mc_anderson_step: subgrid index out of range"); return -1; }
  MCAnderson *h = reinterpret_cast<MCAnderson *>(hh);
  hipStream_t st = (hipStream_t)stream;
  const int N = numberParticles;
  const int ncells = cellDim[0] * cellDim[1] * cellDim[2];
  if (int e = mc_counters_for(h, ncells, st)) return e;
  if (N == 0) return 0;
  if (int e = h->shifted.reserve(sizeof(float4) * (size_t)N)) return e;
  if (int e = h->sortPos.reserve(sizeof(float4) * (size_t)N)) return e;
  float4 *pos = reinterpret_cast<float4 *>(d_pos), *shifted = (float4 *)h->shifted.ptr, *sortPos = (float4 *)h->sortPos.ptr;
  const real3f o{origin[0], origin[1], is2D ? 0.0f : origin[2]};
  const dim3 gN((N + 255) / 256), bN(256);
  hipLaunchKernelGGL(k_mc_shift, gN, bN, 0, st, pos, shifted, N, o);
  if (int e = h->cl.update(shifted, N, boxL, boxPeriodic, cellDim, st)) return e;
  hipLaunchKernelGGL(k_mc_shift, gN, bN, 0, st, (const float4 *)h->cl.sortPos.ptr, sortPos, N, real3f{-1.0f * o.x, -1.0f * o.y, -1.0f * o.z});
  MCArgs a;
  a.cellStart = (const uint *)h->cl.cellStart.ptr;
  a.cellEnd = (const int *)h->cl.cellEnd.ptr;
  a.validCell = h->cl.validCell;
  a.pos = sortPos;
  a.grid = h->cl.grid;
  a.box = h->cl.grid.box;
  a.origin = o;
  a.half = make_int3(cellDim[0] / 2, cellDim[1] / 2, is2D ? 1 : cellDim[2] / 2);
  a.nsub = a.half.x * a.half.y * a.half.z;
  a.is2D = is2D ? 1 : 0;
  a.tries = triesPerCell;
  a.beta = beta;
  a.jump = jumpSize;
  a.step = step;
  a.seed = seed;
  a.tbl = reinterpret_cast<const LJParams *>(d_paramTable);
  a.ntypes = ntypes;
  a.tried = (uint *)h->counters.ptr;
  a.accepted = a.tried + ncells;
  a.cap = mc::g_stageCapacity;
  const size_t lds = sizeof(float4) * (size_t)mc::kWaves * (size_t)(a.cap + mc::kTab);
  for (int s = 0; s < numberSubgrids && triesPerCell > 0; ++s) {
    const int g = subgridOrder[s];  // offset3D (Anderson.cuh:93-100)
    a.off = make_int3(g & 1, (g >> 1) & 1, (g >> 2) & 1);
    if (mc::g_baseline) {
      const dim3 grid((a.nsub + 127) / 128), block(128);
      if (ntypes == 1) hipLaunchKernelGGL(k_mc_cell<true>, grid, block, 0, st, a);
      else hipLaunchKernelGGL(k_mc_cell<false>, grid, block, 0, st, a);
    } else {
      const dim3 grid((a.nsub + mc::kWaves - 1) / mc::kWaves), block(64 * mc::kWaves);
      if (ntypes == 1) hipLaunchKernelGGL(k_mc_wave<true>, grid, block, lds, st, a);
      else hipLaunchKernelGGL(k_mc_wave<false>, grid, block, lds, st, a);
    }
  }
  hipLaunchKernelGGL(k_mc_scatter, gN, bN, 0, st, (const float4 *)sortPos, (const int *)h->cl.index.ptr, pos, N);
  UH_CHECK(hipGetLastError());
  return 0;
}

int uammd_mc_anderson_counters(uammd_mc_anderson *hh, unsigned long long *tried, unsigned long long *accepted, int reset, void *stream) {
  if (!hh || !tried || !accepted) { set_last_error("uammd_mc_anderson_counters: null argument"); return -1; }
  MCAnderson *h = reinterpret_cast<MCAnderson *>(hh);
  *tried = *accepted = 0;
  if (h->ncells <= 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  if (int e = h->sums.reserve(2 * sizeof(unsigned long long))) return e;
  uint *t = (uint *)h->counters.ptr;
  hipLaunchKernelGGL(k_mc_sum, dim3(1), dim3(256), 0, st, t, t + h->ncells, h->ncells, reset, (unsigned long long *)h->sums.ptr);
  unsigned long long host[2] = {0, 0};
  UH_CHECK(hipMemcpyAsync(host, h->sums.ptr, sizeof(host), hipMemcpyDeviceToHost, st));
  UH_CHECK(hipStreamSynchronize(st));
  *tried = host[0];
  *accepted = host[1];
  return 0;
}

int uammd_mc_anderson_cell_counters(uammd_mc_anderson *hh, unsigned int *tried, unsigned int *accepted, void *stream) {
  if (!hh || !tried || !accepted) { set_last_error("uammd_mc_anderson_cell_counters: null argument"); return -1; }
  MCAnderson *h = reinterpret_cast<MCAnderson *>(hh);
  if (h->ncells <= 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  const uint *t = (const uint *)h->counters.ptr;
  UH_CHECK(hipMemcpyAsync(tried, t, sizeof(uint) * (size_t)h->ncells, hipMemcpyDeviceToHost, st));
  UH_CHECK(hipMemcpyAsync(accepted, t + h->ncells, sizeof(uint) * (size_t)h->ncells, hipMemcpyDeviceToHost, st));
  UH_CHECK(hipStreamSynchronize(st));
  return 0;
}

int uammd_mc_anderson_energy(uammd_mc_anderson *hh, const float *d_pos, int numberParticles, const float boxL[3], const int boxPeriodic[3],
                             const int cellDim[3], const uammd_lj_pair_parameters *d_paramTable, int ntypes, float *d_energy, void *stream) {
  if (!hh || !d_pos || !boxL || !boxPeriodic || !cellDim || !d_paramTable || !d_energy || ntypes < 1 || numberParticles < 0) {
    set_last_error("uammd_mc_anderson_energy: null or bad argument");
    return -1;
  }
  if (!mc_grid_valid(cellDim)) {
    set_last_error("uammd_mc_anderson_energy: invalid grid %d %d %d", cellDim[0], cellDim[1], cellDim[2]);
    return -1;
  }
  MCAnderson *h = reinterpret_cast<MCAnderson *>(hh);
  hipStream_t st = (hipStream_t)stream;
  if (numberParticles == 0) return 0;
  // Anderson::sumEnergy (Anderson.cu:377-400): origin 0, the list on the MC grid, energy zeroed, one traversal with energy only
  if (int e = h->cl.update(reinterpret_cast<const float4 *>(d_pos), numberParticles, boxL, boxPeriodic, cellDim, st)) return e;
  UH_CHECK(hipMemsetAsync(d_energy, 0, sizeof(float) * (size_t)numberParticles, st));
  return uammd_lj_transverse_celllist(reinterpret_cast<uammd_celllist *>(&h->cl), d_paramTable, ntypes, boxL, boxPeriodic, nullptr, d_energy,
                                      nullptr, nullptr, UAMMD_LJ_ALGO_AUTO, stream);
}

}  // extern "C"
