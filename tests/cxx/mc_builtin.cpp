// MC_NVT::Anderson<Potential::LJ> the way a user builds it from a plain C++14 translation unit (g++, the C ABI); the run is mc_run.h's.
#include "Integrator/MonteCarlo/NVT/Anderson.cuh"
#include "mc_run.h"

int main(int argc, char *argv[]) { return runMC<uammd::MC_NVT::Anderson<uammd::Potential::LJ>, uammd::Potential::LJ>(argc, argv); }
