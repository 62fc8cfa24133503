// The same DPD fluid with a dissipation functor of the program's own (DPD.cuh: DPD_impl<DissipativeStrength>) on a VerletList: device code
// of the user's, so hipcc and the generic PairForces<MyPotential, NeighbourList> of device/PairForces.hip.hpp.  The functor answers the
// constant 4.5, so that the statistics are those of dpd_builtin.cpp.
#include "dpd_run.h"

struct PairwiseDissipation {
  uammd::real scale = 1;
  // i < j are the particles' indices, then their positions and velocities
  __device__ uammd::real dissipativeStrength(int i, int j, const uammd::real4 &pi, const uammd::real4 &pj, const uammd::real3 &vi,
                                             const uammd::real3 &vj) const {
    return uammd::real(4.5) * scale;
  }
};

int main(int argc, char *argv[]) {
  using DPD = uammd::Potential::DPD_impl<PairwiseDissipation>;
  DPD::Parameters par;
  par.gamma = PairwiseDissipation{};
  return runDPD<DPD, uammd::VerletList>(argc, argv, par);
}
