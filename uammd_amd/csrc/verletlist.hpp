// Host-side state of one Verlet list (owned through the opaque uammd_verletlist handle): built in verletlist.hip, walked there by the
// LJ traversal and in sph.hip by the SPH sums.
#pragma once
#include "celllist.hpp"

namespace uammd_hip {

struct VerletList {
  CellList cl;  // BasicNeighbourListBase::cl
  DeviceBuffer neighbourList, numberNeighbours, storedPos, sortPos, flags;
  int maxNeighboursPerParticle = 32;      // BasicListBase.cuh:127
  float verletRadiusMultiplier = 1.08f;   // VerletListBase.cuh:101
  float currentCutOff = 0.0f;
  float boxL[3] = {0, 0, 0};
  int boxPeriodic[3] = {0, 0, 0};
  bool haveBox = false;
  int storedN = -1;
  bool forceNextRebuild = true;
  int stepsSinceLastUpdate = 0;
  int N = 0;
  DeviceBuffer sphInfo, sphMass;  // uammd_sph_sum_verletlist: {velocity, P / rho^2} and mass rows in list order (sph.hip); they only grow
  uint *hostFlag = nullptr;  // pinned: the drift / overflow flags are read back every update, as in the reference
  ~VerletList() {
    if (hostFlag) (void)hipHostFree(hostFlag);
  }
};

}  // namespace uammd_hip
