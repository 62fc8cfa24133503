// Same include path as the reference's src/Integrator/MonteCarlo/ForceBiased.cuh: force biased Monte Carlo, the Metropolized
// Euler-Maruyama scheme of Bou-Rabee and Vanden-Eijnden [1], also known as MALA, on the C ABI — host code only, usable from plain g++
// (C++14).  It works with ANY interactor through Interactor::sum({force, energy}).
//
//   MC::ForceBiased::Parameters par;
//   par.beta = 1.0;              // inverse of temperature
//   par.stepSize = 0.0001;       // initial step size (optimized towards the target ratio)
//   par.acceptanceRatio = 0.5;   // desired ratio of accepted trials
//   auto mala = std::make_shared<MC::ForceBiased>(pd, par);
//   mala->addInteractor(myinteractor);
//   mala->forwardTime();         // tries new configurations until one is accepted
//   mala->getCurrentEnergy();  mala->getCurrentStepSize();  mala->getCurrentAcceptanceRatio();  mala->getLastNumberOfTrials();
//
// A trial: Y = X + h F(X) + sqrt(2 h / beta) xi (uammd_mc_forcebiased_propose, uammd_hip.h), force and energy zeroed, the interactors
// summed on Y, then uammd_mc_forcebiased_decide forms E_Y, T_XY and T_YX on the device, decides Z < exp(-beta ((E_Y - E_X) + (T_YX - T_XY)))
// and keeps Y or puts X back; uammd_mc_forcebiased_result is the one host synchronisation of the trial.  The host draws keep the
// reference's order: seed = sys->rng().next32() at construction, Z = sys->rng().uniform(0, 1) once per trial.
//
// Where this class departs from the reference:
//   * U = sum_i energy[i], NOT half of it.  Every interactor of this library deposits half of a pair's energy on each partner
//     (Potential::LJ::energy already returns the half), so the sum is U; the reference halves it a second time and so weighs
//     exp(-beta U / 2) against a drift built from the whole force.  getCurrentEnergy() returns U.  A user functor that deposits the WHOLE
//     pair energy on both partners double counts: deposit half.
//   * getLastNumberOfTrials() / getTotalNumberOfTrials().  forwardTime() returns only at an acceptance, so the states seen after each call
//     are NOT a Boltzmann sample on their own: the state a call STARTS from has to be weighted by the number of trials that call took.
//   * Parameters::maxTrials (default 1 000 000): that many consecutive rejections throw instead of looping for ever (on a NaN landscape
//     the reference never returns).  Positions and forces are then those of the stored configuration.
//   * a group other than "All" is refused (the reference indexes its stored arrays by group size but the particle arrays globally).
//   * the three sums and the acceptance exponent are in double (float thrust::reduce in the reference).
//
// [1] Pathwise Accuracy and Ergodicity of Metropolized Integrators for SDEs (2009).  N. Bou-Rabee and E. Vanden-Eijnden.
//     https://doi.org/10.1002/cpa.20306
#pragma once
#if defined(DOUBLE_PRECISION)
#error "ForceBiased.cuh: this module has a single-precision backend only on MI355X (uammd.h, PRECISION): build without -DDOUBLE_PRECISION"
#endif
#include "../../uammd.h"

namespace uammd {
namespace MC {
namespace forcebiased_ns {

class Optimize {  // ForceBiased.cuh:88-138
  int naccept;
  int ntry;
  int ncontrol;
  real jumpSize;
  real currentAcceptanceRatio = 0;
  const real targetRatio = 0.9;

  void adjustStepSize() {
    constexpr float updateRateIncrease = 1.02;
    constexpr float updateRateDecrease = 0.9;
    constexpr float minimumJumpSize = 1e-8;
    constexpr float maximumJumpSize = 2;
    const float ratio = naccept / (float)ntry;
    if (ratio > targetRatio && jumpSize < maximumJumpSize) {
      jumpSize *= updateRateIncrease;
    } else if (ratio < targetRatio && jumpSize > minimumJumpSize) {
      jumpSize *= updateRateDecrease;
    }
    ntry = naccept = 0;
    currentAcceptanceRatio = ratio;
  }

public:
  Optimize(real targetAcceptanceRatio, real initialStepSize = 1) : targetRatio(targetAcceptanceRatio) {
    naccept = 0;
    ntry = 0;
    ncontrol = 1000;
    jumpSize = initialStepSize;
  }
  void registerAccept() {
    naccept++;
    ntry++;
    if (ntry % ncontrol == 0) adjustStepSize();
  }
  void registerReject() {
    ntry++;
    if (ntry % ncontrol == 0) adjustStepSize();
  }
  real getStepSize() { return jumpSize; }
  real getCurrentAcceptanceRatio() { return currentAcceptanceRatio; }
};

}  // namespace forcebiased_ns

class ForceBiased : public Integrator {
public:
  struct Parameters {
    real beta = -1;              // inverse of temperature
    real stepSize = 0.1;         // initial step length (optimized according to the target acceptance ratio)
    real acceptanceRatio = 0.5;  // desired acceptance ratio
    int maxTrials = 1000000;     // consecutive rejections after which forwardTime() throws (not in the reference)
  };

  ForceBiased(shared_ptr<ParticleData> pd, Parameters par) : ForceBiased(std::make_shared<ParticleGroup>(pd, "All"), par) {}

  ForceBiased(shared_ptr<ParticleGroup> pg, Parameters par)  // ForceBiased.cuh:163-179
      : Integrator(pg, "MC::ForceBiased"), beta(par.beta), maxTrials(par.maxTrials), optimizeStepSize(par.acceptanceRatio, par.stepSize) {
    System::log<System::MESSAGE>("[MC::ForceBiased] Initialized");
    System::log<System::MESSAGE>("[MC::ForceBiased] Temperature: %g", 1.0 / beta);
    System::log<System::MESSAGE>("[MC::ForceBiased] Target acceptance ratio: %g", (double)par.acceptanceRatio);
    System::log<System::MESSAGE>("[MC::ForceBiased] Initial step size: %g", (double)par.stepSize);
    if (beta < 0 || par.stepSize <= 0 || par.acceptanceRatio <= 0) {
      System::log<System::ERROR>("[MC::ForceBiased] ERROR: parameters beta, stepSize and acceptanceRatio must be >=0");
      throw std::runtime_error("Invalid parameter");
    }
    if (maxTrials < 1) {
      System::log<System::ERROR>("[MC::ForceBiased] ERROR: maxTrials must be at least 1");
      throw std::runtime_error("Invalid parameter");
    }
    if (subgroup) {
      System::log<System::ERROR>("[MC::ForceBiased] ERROR: only the group of all particles is supported");
      throw std::runtime_error("[MC::ForceBiased] A group other than \"All\" is not supported");
    }
    this->seed = sys->rng().next32();
    detail::check(uammd_mc_forcebiased_create(&handle));
  }
  ~ForceBiased() { uammd_mc_forcebiased_destroy(handle); }
  ForceBiased(const ForceBiased &) = delete;

  real getCurrentEnergy() { return currentEnergy; }
  real getCurrentStepSize() { return optimizeStepSize.getStepSize(); }
  real getCurrentAcceptanceRatio() { return optimizeStepSize.getCurrentAcceptanceRatio(); }
  // trials the last forwardTime() took (the weight, in an average, of the state that call STARTED from) and since construction
  int getLastNumberOfTrials() { return lastTrials; }
  unsigned long long getTotalNumberOfTrials() { return totalTrials; }

  void forwardTime() override {  // ForceBiased.cuh:191-200
    System::log<System::DEBUG1>("[ForceBiased] Starting step %d", step);
    if (step == 0) firstStep();
    updateInteractors();
    lastTrials = 0;
    while (true) {
      lastTrials++;
      totalTrials++;
      if (tryNewStep()) return;
      if (lastTrials >= maxTrials) {
        System::log<System::ERROR>("[MC::ForceBiased] %d consecutive trials were rejected", lastTrials);
        throw std::runtime_error("[MC::ForceBiased] Too many consecutive trials were rejected (maxTrials)");
      }
    }
  }

private:
  real currentEnergy = 0;
  real beta;
  uint step = 0;
  uint seed;
  int maxTrials;
  int lastTrials = 0;
  unsigned long long totalTrials = 0;
  forcebiased_ns::Optimize optimizeStepSize;
  uammd_mc_forcebiased *handle = nullptr;

  void updateInteractors() {  // ForceBiased.cuh:203-209
    if (step == 0)
      for (auto &updatable : updatables) updatable->updateTemperature(1.0 / beta);
  }

  void firstStep() {  // ForceBiased.cuh:211-218
    System::log<System::DEBUG1>("[ForceBiased] First step");
    updateForceEnergyEstimation();
    auto pos = pd->getPos(access::gpu, access::read);
    auto force = pd->getForce(access::gpu, access::read);
    auto energy = pd->getEnergy(access::gpu, access::read);
    detail::check(uammd_mc_forcebiased_begin(handle, (const float *)pos.raw(), (const float *)force.raw(), energy.raw(), pd->getNumParticles(),
                                             nullptr));
  }

  // the two fills and the interactors of updateForceEnergyEstimation (ForceBiased.cuh:326-354); the sum itself is the library's
  void updateForceEnergyEstimation() {
    System::log<System::DEBUG2>("[MC::ForceBiased] Computing current force and energy");
    {
      auto force = pd->getForce(access::gpu, access::write);
      auto energy = pd->getEnergy(access::gpu, access::write);
      detail::check(uammd_fill_zero(force.raw(), sizeof(real4) * force.size(), nullptr));
      detail::check(uammd_fill_zero(energy.raw(), sizeof(real) * energy.size(), nullptr));
    }
    for (auto &inter : interactors) {
      Interactor::Computables c;
      c.force = true;
      c.energy = true;
      inter->sum(c, 0);
    }
  }

  bool tryNewStep() {  // ForceBiased.cuh:220-262
    step++;
    System::log<System::DEBUG2>("[ForceBiased] Propose next move");
    const real stepSize = optimizeStepSize.getStepSize();
    const int N = pd->getNumParticles();
    {
      auto pos = pd->getPos(access::gpu, access::readwrite);
      detail::check(uammd_mc_forcebiased_propose(handle, (float *)pos.raw(), N, stepSize, beta, step, seed, nullptr, nullptr));
    }
    updateForceEnergyEstimation();
    const real Z = sys->rng().uniform(0, 1);
    int accepted = 0;
    double record[6];
    {
      auto pos = pd->getPos(access::gpu, access::readwrite);
      auto force = pd->getForce(access::gpu, access::readwrite);
      auto energy = pd->getEnergy(access::gpu, access::read);
      detail::check(uammd_mc_forcebiased_decide(handle, (float *)pos.raw(), (float *)force.raw(), energy.raw(), N, stepSize, beta, (double)Z, nullptr));
      detail::check(uammd_mc_forcebiased_result(handle, &accepted, record, nullptr));
    }
    if (record[1] == (double)std::numeric_limits<real>::max())
      System::log<System::WARNING>("[MC::ForceBiased] Detected an infinite or NaN energy");
    currentEnergy = (real)record[5];
    if (accepted) optimizeStepSize.registerAccept();
    else optimizeStepSize.registerReject();
    return accepted != 0;
  }
};

}  // namespace MC
}  // namespace uammd
