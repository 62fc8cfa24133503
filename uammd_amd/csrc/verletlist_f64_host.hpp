// Host-only logic of the double-precision Verlet list (verletlist_f64.hip): when the list is rebuilt, the drift threshold, how the
// capacity grows, the sizes of the handle's buffers and the argument checks.  Plain C++14, no HIP type: tests/cxx/verletlist_f64_host.cpp
// runs it under the address and undefined-behaviour sanitizers.
//   VerletListBase::update / needsRebuild / isParticleDriftOverThreshold   Interactor/NeighbourList/VerletList/VerletListBase.cuh:107-199
//   BasicNeighbourListBase::fillBasicNeighbourList (capacity 32, +32)      Interactor/NeighbourList/BasicList/BasicListBase.cuh:76-142
#pragma once
#include <cstddef>

namespace uammd_hip {
namespace vl64 {

constexpr int kInitialCapacity = 32;  // BasicListBase.cuh:127
constexpr int kCapacityStep = 32;

// what the list remembers between updates
struct State {
  int maxNeighboursPerParticle = kInitialCapacity;
  double verletRadiusMultiplier = 1.08;  // VerletListBase.cuh:101
  double currentCutOff = 0.0;
  double boxL[3] = {0, 0, 0};
  int boxPeriodic[3] = {0, 0, 0};
  bool haveBox = false;
  int storedN = -1;
  bool forceNextRebuild = true;
  int stepsSinceLastUpdate = 0;
  int N = 0;
};

enum Decision { KEEP_UNLESS_DRIFT = 0, REBUILD = 1 };

// (multiplier * cutOff - cutOff) / 2 in double (VerletListBase.cuh:181)
inline double drift_threshold(double multiplier, double cutOff) { return (multiplier * cutOff - cutOff) / 2.0; }

// needsRebuild up to the drift check (VerletListBase.cuh:158-175): REBUILD, or KEEP_UNLESS_DRIFT when only the particles' drift can still
// ask for a rebuild (the caller then runs the drift kernel and reads its counter back).  Consumes the forced rebuild.
inline Decision needs_rebuild(State &s, const double L[3], const int periodic[3], double cutOff, int N) {
  if (s.forceNextRebuild) {
    s.forceNextRebuild = false;
    return REBUILD;
  }
  if (!s.haveBox || L[0] != s.boxL[0] || L[1] != s.boxL[1] || L[2] != s.boxL[2] || (periodic[0] != 0) != (s.boxPeriodic[0] != 0) ||
      (periodic[1] != 0) != (s.boxPeriodic[1] != 0) || (periodic[2] != 0) != (s.boxPeriodic[2] != 0) || cutOff != s.currentCutOff ||
      N != s.storedN)
    return REBUILD;
  if (drift_threshold(s.verletRadiusMultiplier, s.currentCutOff) <= 1e-6) return REBUILD;  // :183
  return KEEP_UNLESS_DRIFT;
}

// what a rebuild records before the list is filled (VerletListBase.cuh:112-115,153-156)
inline void begin_rebuild(State &s, const double L[3], const int periodic[3], double cutOff, int N) {
  s.stepsSinceLastUpdate = 0;
  for (int k = 0; k < 3; ++k) { s.boxL[k] = L[k]; s.boxPeriodic[k] = periodic[k] != 0; }
  s.haveBox = true;
  s.currentCutOff = cutOff;
  s.N = N;
  s.storedN = N;
}
inline void end_update(State &s) { s.stepsSinceLastUpdate++; }
inline double list_radius(const State &s) { return s.currentCutOff * s.verletRadiusMultiplier; }

// The fill counts every neighbour of a particle and reports the largest count.  The reference retries with 32 more slots while some
// particle has `capacity` neighbours or more (BasicListBase.cuh:65-70,96-110); knowing the largest count, the capacity it ends at is
// reached in one step.  Returns whether the list has to be filled again.
inline bool grow_capacity(State &s, int largestCount) {
  bool grew = false;
  while (largestCount >= s.maxNeighboursPerParticle) {
    s.maxNeighboursPerParticle += kCapacityStep;
    grew = true;
  }
  return grew;
}

// bytes of the handle's buffers.  Entry k of sorted particle i is at k * N + i and the fill stores entries k < capacity only.
struct BufferBytes {
  size_t neighbourList, numberNeighbours, storedPos, sortPos, flags;
};
inline BufferBytes buffer_bytes(int N, int capacity) {
  BufferBytes b;
  b.neighbourList = sizeof(int) * (size_t)N * (size_t)capacity;
  b.numberNeighbours = sizeof(int) * (size_t)N;
  b.storedPos = 4 * sizeof(double) * (size_t)N;
  b.sortPos = 4 * sizeof(double) * (size_t)N;
  b.flags = 2 * sizeof(unsigned);  // [0] particles over the drift threshold, [1] largest neighbour count of the last fill
  return b;
}
// may the fill store entry k of sorted particle i?  (the one bound the fill kernel depends on; the kernel spells the same test)
inline bool may_store(int k, int i, int N, int capacity) { return k >= 0 && k < capacity && i >= 0 && i < N; }
inline size_t entry_offset(int k, int i, int N) { return (size_t)k * (size_t)N + (size_t)i; }

// argument checks: the message of what is wrong, or nullptr
inline const char *check_update(const void *handle, const void *d_pos, int N, const double *L, const int *periodic, double cutOff,
                                double multiplier) {
  if (!handle) return "uammd_verletlist_update_f64: null handle";
  if (N < 0) return "uammd_verletlist_update_f64: negative number of particles";
  if (!L || !periodic) return "uammd_verletlist_update_f64: null argument";
  if (N > 0 && !d_pos) return "uammd_verletlist_update_f64: null positions";
  if (!(cutOff > 0.0)) return "uammd_verletlist_update_f64: the cut-off must be positive";
  if (!(multiplier >= 1.0)) return "uammd_verletlist_update_f64: the cut-off multiplier must be at least 1";
  return nullptr;
}
inline const char *check_multiplier(const void *handle, double multiplier) {
  if (!handle) return "uammd_verletlist_set_cutoff_multiplier_f64: null handle";
  if (!(multiplier >= 1.0)) return "uammd_verletlist_set_cutoff_multiplier_f64: the cut-off multiplier must be at least 1";
  return nullptr;
}

}  // namespace vl64
}  // namespace uammd_hip
