// The same run with a Lennard-Jones functor of the program's own: device code of the user's, so hipcc and the generic
// MC_NVT::Anderson<MyPotential> of device/Anderson.hip.hpp over Potential::Radial<UserLJ> (device/PairForces.hip.hpp).  The functor
// restates LJFunctor (Potential.cuh:25-83) operation for operation, so the positions are those of mc_builtin.cpp bit for bit.
#include "device/Anderson.hip.hpp"
#include "device/PairForces.hip.hpp"
#include "mc_run.h"

struct UserLJ {
  struct InputPairParameters { uammd::real cutOff, sigma, epsilon; bool shift = false; };
  struct PairParameters { uammd::real cutOff2, sigma2, epsilonDivSigma2, shift; };
  __device__ uammd::real force(uammd::real r2, PairParameters p) const {
    if (r2 >= p.cutOff2) return 0;
    const uammd::real invr2 = p.sigma2 / r2, invr6 = invr2 * invr2 * invr2;
    return p.epsilonDivSigma2 * fmaf(-48.0f, invr6, 24.0f) * invr6 * invr2;
  }
  __device__ uammd::real energy(uammd::real r2, PairParameters p) const {  // the particle's half of the pair
    if (r2 >= p.cutOff2) return 0;
    const uammd::real invr2 = p.sigma2 / r2, invr6 = invr2 * invr2 * invr2;
    return 0.5f * fmaf(p.epsilonDivSigma2 * p.sigma2 * 4.0f * invr6, invr6 - 1.0f, -p.shift);
  }
  static PairParameters processPairParameters(InputPairParameters in) {
    PairParameters p;
    p.cutOff2 = in.cutOff * in.cutOff;
    p.sigma2 = in.sigma * in.sigma;
    p.epsilonDivSigma2 = in.epsilon / p.sigma2;
    p.shift = 0;
    if (in.shift) {
      const uammd::real i2 = p.sigma2 / p.cutOff2, i6 = i2 * i2 * i2;
      p.shift = in.epsilon * 4.0f * i6 * (i6 - 1.0f);
    }
    return p;
  }
};

int main(int argc, char *argv[]) {
  using Pot = uammd::Potential::Radial<UserLJ>;
  return runMC<uammd::MC_NVT::Anderson<Pot>, Pot>(argc, argv);
}
