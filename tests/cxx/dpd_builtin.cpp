// A DPD fluid the way a user builds it from a plain C++14 translation unit (g++, the C ABI): VerletNVE + PairForces<Potential::DPD>
// (Integrator/VerletNVE.cuh, Interactor/Potential/DPD.cuh).  See dpd_run.h for the arguments and the line it prints;
// tests/test_gpu_dpd.py checks the momentum and the kinetic temperature.
#include "dpd_run.h"

int main(int argc, char *argv[]) {
  uammd::Potential::DPD::Parameters par;
  par.gamma = 4.5;
  return runDPD<uammd::Potential::DPD, uammd::CellList>(argc, argv, par);
}
