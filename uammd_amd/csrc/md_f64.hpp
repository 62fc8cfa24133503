// What the other double-precision files of path A (verletlist_f64.hip, bonded_f64.hip, dpd_f64.hip) need of md_f64.hip: the state behind the
// uammd_celllist_f64 handle and the device-side pieces of the Lennard-Jones traversal (the pair evaluation with the oracle's FMA
// placement, the output rows).  Declarations only: md_f64.hip includes this header and compiles to the same code as before.
#pragma once
#include "celllist.hpp"
#include "md_f64_host.hpp"

namespace uammd_hip {
namespace md64d {

struct CellList64 {
  DeviceBuffer hash, index, sortPos, sortPos32, cellStart, cellEnd, cellOutside;
  DeviceBuffer dpdRows;  // uammd_dpd_transverse_celllist_f64: {velocity, key} rows in list order (dpd_f64.hip)
  size_t dpdRowsBytes = 0;
  GridT<double> grid{};
  double boxL[3] = {0, 0, 0};
  int boxPeriodic[3] = {0, 0, 0};
  md64::ValidCell epoch;
  uint maxHash = 0;
  long long nCellsAlloc = -1;
  int N = 0;
  // NaN positions / particles outside a non-periodic box: raised by the kernels in host-mapped memory, looked at by the next call
  int *hostErr = nullptr, *devErr = nullptr;
  int check_errors(hipStream_t st, bool sync) {
    if (!hostErr) return 0;
    if (sync) UH_CHECK(hipStreamSynchronize(st));
    if (__atomic_load_n(hostErr, __ATOMIC_ACQUIRE)) {
      __atomic_store_n(hostErr, 0, __ATOMIC_RELEASE);
      set_last_error("CellList encountered NaN positions or particles outside a non-periodic box");  // CellListBase.cuh:262
      return -4;
    }
    return 0;
  }
  ~CellList64() {
    if (hostErr) (void)hipHostFree(hostErr);
  }
};

UH_D bool in_grid(const GridT<double> &g, int3 c) {
  return !(c.x < 0 || c.x >= g.cellDim.x || c.y < 0 || c.y >= g.cellDim.y || c.z < 0 || c.z >= g.cellDim.z);
}

UH_D int3 cell_of_key(uint h) { return make_int3((int)compact10(h), (int)compact10(h >> 1), (int)compact10(h >> 2)); }

// ---- Lennard-Jones ----------------------------------------------------------------------------------------------------------------
struct LJParams64 { double cutOff2, sigma2, epsilonDivSigma2, shift; };
struct Acc64 { double fx = 0.0, fy = 0.0, fz = 0.0, e = 0.0, v = 0.0; };

UH_D LJParams64 lj_lookup64(const LJParams64 *tbl, int ntypes, int ti, int tj) {  // ParameterHandler.cuh:41-60
  if (ti > tj) { const int t = ti; ti = tj; tj = t; }
  int typeIndex = ti + ntypes * tj;
  if (ti >= ntypes || tj >= ntypes) typeIndex = 0;
  return tbl[typeIndex];
}
UH_D double lj_max_cutoff2_64(const LJParams64 *tbl, int ntypes) {
  double m = 0.0;
  for (int t = 0; t < ntypes * ntypes; ++t) m = fmax(m, tbl[t].cutOff2);
  return m;
}

// One pair, branch free (lj_eval of lj_common.hpp in double): |f|/r and half the pair energy, both exactly 0 at r = 0 and from the
// cut-off on.  A masked pair adds fma(0, r12, acc) == acc: the same bits as skipping it.
template <bool PBC, bool WE>
UH_D void lj_eval64(const BoxT<double> &box, const LJParams64 &p, const double4 &ri, const double4 &rj, real3d &r12, double &fm, double &e) {
  r12 = real3d{rj.x - ri.x, rj.y - ri.y, rj.z - ri.z};
  if (PBC) r12 = box.apply_pbc(r12);
  const double r2 = dot3(r12, r12);
  const bool in = (r2 != 0.0) & !(r2 >= p.cutOff2);
  const double invr2 = p.sigma2 / r2;
  const double invr6 = invr2 * invr2 * invr2;
  const double f = p.epsilonDivSigma2 * fma(-48.0, invr6, 24.0) * invr6 * invr2;
  fm = in ? f : 0.0;
  if (WE) {
    const double E = fma(p.epsilonDivSigma2 * p.sigma2 * 4.0 * invr6, (invr6 - 1.0), -p.shift);
    e = in ? 0.5 * E : 0.0;
  } else
    e = 0.0;
}
template <bool WE, bool WV> UH_D void lj_acc64(Acc64 &a, const real3d &r12, double fm, double e) {
  if (WE) a.e += e;
  a.fx = fma(fm, r12.x, a.fx);
  a.fy = fma(fm, r12.y, a.fy);
  a.fz = fma(fm, r12.z, a.fz);
  if (WV) a.v += dot3(real3d{fm * r12.x, fm * r12.y, fm * r12.z}, r12);
}
template <bool PBC> UH_D double lj_dist2_64(const BoxT<double> &box, const double4 &ri, const double4 &rj) {
  real3d r12{rj.x - ri.x, rj.y - ri.y, rj.z - ri.z};
  if (PBC) r12 = box.apply_pbc(r12);
  return dot3(r12, r12);
}

struct Out64 {
  double4 *force;
  double *energy, *virial;
  const int *globalIndex;
};
UH_D void write_out64(const Out64 &o, int ori, const Acc64 &a) {
  if (o.force) {
    double4 f = o.force[ori];
    f.x += a.fx; f.y += a.fy; f.z += a.fz; f.w += 0.0;
    o.force[ori] = f;
  }
  if (o.energy) o.energy[ori] += a.e;
  if (o.virial) o.virial[ori] += a.v;
}

}  // namespace md64d
}  // namespace uammd_hip
