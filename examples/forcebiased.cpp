// Force biased Monte Carlo (MC::ForceBiased, the Metropolized Euler-Maruyama scheme) of a Lennard-Jones fluid — the set-up of the
// reference's test/MC/ForceBiased/ForceBiased.cu with "integrator forcebiased", written against the same class names and compiled
// against the MI355X library with a plain C++14 compiler:
//   g++ -std=c++14 -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -I../include/uammd forcebiased.cpp \
//       -L../uammd_amd/lib -luammd_hip -L/opt/rocm/lib -lamdhip64 -o forcebiased
//   forcebiased [numberParticles] [density] [temperature] [calls]
// Prints the trial-weighted average of the potential energy per particle: forwardTime() returns at an acceptance, so the state a call
// starts from counts once for every trial that call took (Integrator/MonteCarlo/ForceBiased.cuh).
#include "uammd.cuh"
#include "Interactor/NeighbourList/CellList.cuh"
#include "Interactor/PairForces.cuh"
#include "Interactor/Potential/Potential.cuh"
#include "Integrator/MonteCarlo/ForceBiased.cuh"
#include <cstdio>
using namespace uammd;

int main(int argc, char *argv[]) {
  const int N = argc > 1 ? std::atoi(argv[1]) : 512;
  const double density = argc > 2 ? std::atof(argv[2]) : 0.6;
  const double temperature = argc > 3 ? std::atof(argv[3]) : 3.0;
  const int calls = argc > 4 ? std::atoi(argv[4]) : 2000;
  auto sys = std::make_shared<System>(argc, argv);
  sys->rng().setSeed(1234);
  auto pd = std::make_shared<ParticleData>(N, sys);
  const real3 boxSize = make_real3(std::cbrt(N / density));
  Box box(boxSize);
  {
    auto pos = pd->getPos(access::cpu, access::write);
    auto initial = initLatticeSC(boxSize, N);
    std::copy(initial.begin(), initial.end(), pos.begin());
  }
  MC::ForceBiased::Parameters par;
  par.beta = 1.0 / temperature;
  par.stepSize = 2e-4;
  par.acceptanceRatio = 0.5;
  auto mala = std::make_shared<MC::ForceBiased>(pd, par);
  using PairForces = PairForces<Potential::LJ, CellList>;
  auto pot = std::make_shared<Potential::LJ>();
  {
    Potential::LJ::InputPairParameters p;
    p.epsilon = 1.0; p.shift = false; p.sigma = 1; p.cutOff = 2.5 * p.sigma;
    pot->setPotParameters(0, 0, p);
  }
  PairForces::Parameters params;
  params.box = box;
  mala->addInteractor(std::make_shared<PairForces>(pd, params, pot));
  for (int i = 0; i < calls / 2; i++) mala->forwardTime();  // relaxation
  double sumU = 0, sumW = 0;
  for (int i = 0; i < calls; i++) {
    const double Ustart = mala->getCurrentEnergy();
    mala->forwardTime();
    sumU += Ustart * mala->getLastNumberOfTrials();
    sumW += mala->getLastNumberOfTrials();
  }
  // the energy the integrator carries is the sum of the per-particle energies of the configuration it holds
  double U = 0;
  {
    auto energy = pd->getEnergy(access::cpu, access::read);
    for (auto e : energy) U += e;
  }
  const double carried = mala->getCurrentEnergy();
  std::printf("N %d density %g T %g calls %d trials %llu U/N %.5f E %.5f stepSize %.4g acceptance %.3f\n", N, density, temperature, calls,
              mala->getTotalNumberOfTrials(), sumU / sumW / N, 1.5 * temperature + sumU / sumW / N, (double)mala->getCurrentStepSize(),
              (double)mala->getCurrentAcceptanceRatio());
  sys->finish();
  return std::abs(carried - U) <= 1e-5 * std::abs(U) + 1e-3 ? 0 : 1;
}
