// Same include path as the reference's src/Integrator/VerletNVE.cuh: the constant-energy velocity-Verlet integrator
// (Integrator/VerletNVE.cuh, VerletNVE.cu) on the C ABI — host code only, usable from plain g++ (C++14).
//
//   VerletNVE::Parameters par;
//   par.dt = 0.01; par.initVelocities = true; par.energy = 1.0;   // target energy per particle (ignored without initVelocities)
//   auto verlet = std::make_shared<VerletNVE>(pd, par);
//   verlet->addInteractor(pairForces);
//   verlet->forwardTime();
#pragma once
#if defined(DOUBLE_PRECISION)
#error "VerletNVE.cuh: this module has a single-precision backend only on MI355X (uammd.h, PRECISION): build without -DDOUBLE_PRECISION"
#endif
#include "../uammd.h"

namespace uammd {

class VerletNVE : public Integrator {
public:
  struct Parameters {  // VerletNVE.cuh:39-47
    real energy = 0;   // target energy per particle, ignored if initVelocities is false
    real dt = 0;
    bool is2D = false;
    bool initVelocities = true;  // modify the starting velocities to ensure the target energy
    real mass = -1;
  };
  VerletNVE(shared_ptr<ParticleData> pd, Parameters par) : VerletNVE(make_shared<ParticleGroup>(pd, "All"), par) {}
  VerletNVE(shared_ptr<ParticleGroup> pg, Parameters par)  // VerletNVE.cu:32-57
      : Integrator(pg, "VerletNVE"), dt(par.dt), energy(par.energy), is2D(par.is2D), initVelocities(par.initVelocities) {
    if (initVelocities) System::log<System::MESSAGE>("[VerletNVE] Target energy per particle: %g", (double)energy);
    else System::log<System::MESSAGE>("[VerletNVE] Not fixing an initial per particle energy.");
    System::log<System::MESSAGE>("[VerletNVE] Time step: %g", (double)dt);
    if (is2D) System::log<System::MESSAGE>("[VerletNVE] Working in 2D mode.");
    if (pd->isVelAllocated() && initVelocities)
      System::log<System::WARNING>("[VerletNVE] Velocity will be overwritten to ensure energy conservation!");
    defaultMass = par.mass;
    if (!pd->isMassAllocated() && defaultMass < 0) defaultMass = 1.0;
    detail::hipCheck(hipStreamCreate(&stream), "hipStreamCreate");
  }
  ~VerletNVE() { hipStreamDestroy(stream); }
  VerletNVE(const VerletNVE &) = delete;

  void forwardTime() override {  // VerletNVE.cu:174-188
    steps++;
    System::log<System::DEBUG1>("[VerletNVE] Performing integration step %d", steps);
    if (steps == 1) firstStepPreparation();
    callIntegrate(1);
    resetGroupForces(stream);
    for (auto &u : updatables) u->updateSimulationTime(steps * dt);
    sumForces();
    callIntegrate(2);
  }

  real sumEnergy() override {  // VerletNVE.cu:203-224: energy[i] += m |v|^2 / 2 with defaultMass whenever it is positive; returns 0
    auto vel = pd->getVel(access::gpu, access::read);
    auto e = pd->getEnergy(access::gpu, access::readwrite);
    auto mass = defaultMass > 0 ? property_ptr<real>() : pd->getMassIfAllocated(access::gpu, access::read);
    detail::check(uammd_sum_kinetic_energy((const float *)vel.raw(), e.raw(), mass.raw(), defaultMass, groupIndex(), groupSize(), nullptr));
    return 0;
  }

private:
  real dt, energy;
  bool is2D, initVelocities;
  real defaultMass;
  int steps = 0;
  hipStream_t stream = 0;

  void sumForces() {
    for (auto &f : interactors) { Interactor::Computables c; c.force = true; f->sum(c, stream); }
  }
  void callIntegrate(int step) {  // VerletNVE.cu:133-150; the mass array wins over defaultMass whenever it is allocated (:76)
    auto pos = pd->getPos(access::gpu, access::readwrite);
    auto vel = pd->getVel(access::gpu, access::readwrite);
    auto force = pd->getForce(access::gpu, access::read);
    auto mass = pd->getMassIfAllocated(access::gpu, access::read);
    detail::check(uammd_verletnve(step, (float *)pos.raw(), (float *)vel.raw(), (const float *)force.raw(), mass.raw(), defaultMass,
                                  groupIndex(), groupSize(), dt, is2D, (void *)stream));
  }
  void firstStepPreparation() {  // VerletNVE.cu:160-171
    if (initVelocities) initializeVelocities();
    resetGroupForces(stream);
    for (auto &u : updatables) u->updateTimeStep(dt);
    sumForces();
  }
  void initializeVelocities() {  // VerletNVE.cu:88-131: K = E - U / N per particle, |v| = sqrt(2 K / m) in a random direction
    const int n = groupSize();
    {
      auto e = pd->getEnergy(access::gpu, access::write);
      if (subgroup) detail::check(uammd_fill_zero_indexed(e.raw(), groupIndex(), n, (int)sizeof(real), nullptr));
      else detail::check(uammd_fill_zero(e.raw(), sizeof(real) * e.size(), nullptr));
    }
    for (auto &f : interactors) { Interactor::Computables c; c.energy = true; f->sum(c, 0); }
    detail::hipCheck(hipDeviceSynchronize(), "hipDeviceSynchronize");
    real U = 0;
    {
      auto e = pd->getEnergy(access::cpu, access::read);
      auto gindex = pg->getIndexIterator(access::cpu);
      for (int t = 0; t < n; ++t) U += e.raw()[gindex[t]];
    }
    U = U / n;
    const real K = energy - U;
    if (K < 0) {
      System::log<System::ERROR>("[VerletNVE] Cannot fix requested energy per particle. Requested E = U + K = %g, but U=%g", (double)energy, (double)U);
      throw std::runtime_error("[VerletNVE] Cannot fix energy");
    }
    System::log<System::MESSAGE>("Starting potential energy per particle: %g", (double)U);
    auto vel = pd->getVel(access::cpu, access::write);
    auto massPtr = pd->getMassIfAllocated(access::cpu, access::read);
    const real *mass = massPtr.raw();
    auto gindex = pg->getIndexIterator(access::cpu);
    for (int t = 0; t < n; ++t) {
      const int i = gindex[t];
      const auto g = sys->rng().gaussian3(0.0, 1.0);
      real3 dir = make_real3((real)g.x, (real)g.y, (real)g.z);
      dir = dir / std::sqrt(dot(dir, dir));
      const real m = mass ? mass[i] : defaultMass;
      vel.raw()[i] = make_real3((real)std::sqrt(2.0 * K / m) * dir);
    }
    System::log<System::MESSAGE>("Starting kinetic energy per particle: %g", (double)K);
  }
};

}  // namespace uammd
