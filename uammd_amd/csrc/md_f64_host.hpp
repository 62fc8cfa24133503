// Host-only logic of the double-precision path A (md_f64.hip): the grid rule, the pair-parameter processing, the epoch rule of the cell
// tables, the sort width, the sizes of the handle's buffers and the argument checks.  Plain C++14, no HIP type: tests/cxx/md_f64_host.cpp
// runs it under the address and undefined-behaviour sanitizers.
//   CellList::createUpdateGrid                  Interactor/NeighbourList/CellList.cuh:100-126
//   CellListBase::updateCurrentValidCell        Interactor/NeighbourList/CellList/CellListBase.cuh:210-230
//   Sorter maxbit                               utils/ParticleSorter.cuh:93-100,264-266
//   LJFunctor::processPairParameters            Interactor/Potential/Potential.cuh:66-82
#pragma once
#include <cmath>
#include <cstddef>
#include <limits>

namespace uammd_hip {
namespace md64 {

// uammd_celllist_create_grid with double for float: cellDim = int3(L / cutOff) by C truncation, any dimension with <= 3 cells collapses to
// 1, a dimension of DBL_MAX or more becomes 64 cut-offs, an infinite one also non periodic
inline void create_grid(const double L_in[3], const int periodic_in[3], const double cutOff[3], int cellDim_out[3], double L_out[3],
                        int periodic_out[3]) {
  const double inf = std::numeric_limits<double>::max();
  for (int k = 0; k < 3; ++k) {
    double L = L_in[k];
    const bool inputPeriodic = periodic_in[k] && !(L == 0.0 || std::isinf(L));
    if (L >= inf) L = 64 * cutOff[k];
    L_out[k] = L;
    periodic_out[k] = (inputPeriodic && L < inf) ? 1 : 0;
    const double q = L / cutOff[k];
    int cd = (q > -2147483648.0 && q < 2147483647.0) ? (int)q : 0;  // Grid(Box, real3 minCellSize): C truncation (a NaN or a quotient
                                                                    // beyond int has no value in C: one cell)
    if (cd <= 3) cd = 1;
    cellDim_out[k] = cd;
  }
}

inline void process_pair_parameters(double cutOff, double sigma, double epsilon, int shift, double out[4]) {
  const double cutOff2 = cutOff * cutOff;
  const double sigma2 = sigma * sigma;
  out[0] = cutOff2;
  out[1] = sigma2;
  out[2] = epsilon / sigma2;
  if (shift) {
    const double invCutOff2 = sigma2 / cutOff2;
    const double invrc6 = invCutOff2 * invCutOff2 * invCutOff2;
    out[3] = epsilon * 4.0 * invrc6 * (invrc6 - 1.0);
  } else
    out[3] = 0.0;
}

// number of key bits the stable sort looks at: 32 - clz(maxKey), 0 for maxKey = 0
inline int sort_end_bit(unsigned maxKey) {
  int bits = 0;
  while (maxKey) { ++bits; maxKey >>= 1; }
  return bits;
}

// the epoch trick: cellStart holds start + VALID_CELL, so the table is cleared only when the epoch would overflow or N changed
struct ValidCell {
  unsigned validCell = 0;
  long long counter = -1;
  int lastN = -1;
  bool next(int numberParticles) {  // returns whether cellStart has to be zero-filled
    if (numberParticles != lastN) counter = -1;
    const bool uninit = counter < 0;
    const unsigned long long nextMax = (unsigned long long)numberParticles * (unsigned long long)(counter + 2);
    const unsigned long long maxStorable = (unsigned long long)std::numeric_limits<unsigned>::max() - 1ull;
    lastN = numberParticles;
    if (uninit || nextMax >= maxStorable) {
      validCell = (unsigned)numberParticles;
      counter = 1;
      return true;
    }
    counter++;
    validCell = (unsigned)numberParticles * (unsigned)counter;
    return false;
  }
};

constexpr int kPadRows = 8;  // rows past the last particle that the traversals' grouped loads may touch (masked)

// bytes of every buffer of a list of N particles on ncells cells
struct BufferBytes {
  size_t hash, index, sortPos, sortPos32, cellStart, cellEnd, cellOutside;
};
inline BufferBytes buffer_bytes(int N, long long ncells) {
  BufferBytes b;
  b.hash = sizeof(unsigned) * ((size_t)N + 1);
  b.index = sizeof(int) * ((size_t)N + 1);
  b.sortPos = 4 * sizeof(double) * ((size_t)N + kPadRows);
  b.sortPos32 = 4 * sizeof(float) * ((size_t)N + kPadRows);
  b.cellStart = sizeof(unsigned) * (size_t)ncells;
  b.cellEnd = sizeof(int) * (size_t)ncells;
  b.cellOutside = (size_t)ncells;
  return b;
}

// argument checks: the message of what is wrong, or nullptr
inline const char *check_update(const void *handle, const void *d_pos, int N, const double L[3], const int periodic[3], const int cellDim[3]) {
  if (!handle) return "uammd_celllist_update_f64: null handle";
  if (N < 0) return "uammd_celllist_update_f64: negative number of particles";
  if (N == 0) return nullptr;
  if (!d_pos || !L || !periodic || !cellDim) return "uammd_celllist_update_f64: null argument";
  if (cellDim[0] <= 0 || cellDim[1] <= 0 || cellDim[2] < 0 || cellDim[0] > 1024 || cellDim[1] > 1024 || cellDim[2] > 1024)
    return "CellList encountered an invalid grid and/or cutoff";  // (10 bits of Morton key per direction)
  for (int k = 0; k < 3; ++k)
    if (!(L[k] > 0.0 || (k == 2 && L[k] == 0.0)) || std::isinf(L[k])) return "CellList encountered an invalid grid and/or cutoff";
  if ((long long)cellDim[0] * cellDim[1] * (cellDim[2] ? cellDim[2] : 1) > (1ll << 30)) return "CellList: too many cells";
  return nullptr;
}

constexpr int kAlgoAuto = 0, kAlgoGeneral = 1, kAlgoScan32 = 11;
inline const char *check_transverse(const void *handle, const void *d_table, int ntypes, const double boxL[3], const int boxPeriodic[3], int algo) {
  if (!handle || !d_table || !boxL || !boxPeriodic) return "uammd_lj_transverse_celllist_f64: null argument";
  if (ntypes < 1) return "uammd_lj_transverse_celllist_f64: ntypes < 1";
  if (algo != kAlgoAuto && algo != kAlgoGeneral && algo != kAlgoScan32)
    return "uammd_lj_transverse_celllist_f64: unknown algorithm (AUTO, GENERAL and SCAN32 exist in double)";
  return nullptr;
}

// Does the single-precision image of the sorted positions cover this traversal?  It holds positions folded into the LIST's box and the
// scan replaces the minimum image by a shift per neighbour cell, which is the minimum image when the potential's box is the list's and
// every periodic direction has at least 5 cells (|d| <= 2 cells <= 0.4 L); a direction with one cell must be non periodic.
inline bool scan32_covers(const int cellDim[3], const double gridL[3], const int gridPeriodic[3], const double boxL[3], const int boxPeriodic[3]) {
  for (int k = 0; k < 3; ++k) {
    const bool gp = gridPeriodic[k] != 0, bp = boxPeriodic[k] != 0 && !(boxL[k] == 0.0 || std::isinf(boxL[k]));
    if (gp != bp) return false;
    if (gp && gridL[k] != boxL[k]) return false;
    if (gp && cellDim[k] < 5) return false;
  }
  return true;
}

}  // namespace md64
}  // namespace uammd_hip
