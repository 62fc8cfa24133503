// Same include path as the reference's src/Interactor/SPH.cuh: smoothed particle hydrodynamics as an Interactor, to be used with a
// symplectic integrator without a thermostat (VerletNVE):
//
//   SPH::Parameters par;
//   par.box = box; par.support = 2.4; par.viscosity = 10; par.gasStiffness = 60; par.restDensity = 0.3;
//   verlet->addInteractor(std::make_shared<SPH>(pd, par));
//
// Per force evaluation, over a VerletList with cut-off 2 support (the list includes the particle itself, and the self term counts in the
// density), with m the mass property or 1:
//   rho_i = sum_j m_j W(rij, h);  P_i = gasStiffness (rho_i - restDensity)
//   F_i += sum_j m_i m_j (P_i / rho_i^2 + P_j / rho_j^2 - viscosity (vij . rij) / (r^2 + 0.001 h^2)) G(rij, h)
// W is the M4 cubic spline and G the "gradient" of SPH/Kernel.cuh as the reference writes it (uammd_hip.h).  Both sums run in
// the library through the C ABI (uammd_sph_sum_verletlist): host code only, plain g++ is enough.  The Computables are ignored, as in the
// reference: the force is always added and no energy or virial is produced.
#pragma once
#if defined(DOUBLE_PRECISION)
#error "SPH.cuh: this module has a single-precision backend only on MI355X (uammd.h, PRECISION): build without -DDOUBLE_PRECISION"
#endif
#include "../uammd.h"

namespace uammd {

class SPH : public Interactor {
public:
  using NeighbourList = VerletList;
  struct Parameters {  // SPH.cuh:45-52
    Box box;
    real support = 1.0;
    real viscosity = 50.0;
    real gasStiffness = 100.0;
    real restDensity = 0.4;
    shared_ptr<NeighbourList> nl = nullptr;
  };
  SPH(shared_ptr<ParticleGroup> pg, Parameters par)  // SPH.cu:45-53
      : Interactor(pg, "SPH/"), nl(par.nl), box(par.box), support(par.support), gasStiffness(par.gasStiffness),
        restDensity(par.restDensity), viscosity(par.viscosity) {
    System::log<System::MESSAGE>("[SPH] Initialized.");
    if (pg->getNumberParticles() != pd->getNumParticles()) System::log<System::CRITICAL>("[SPH] Not compatible with groups yet!.");
  }
  SPH(shared_ptr<ParticleData> pd, Parameters par) : SPH(std::make_shared<ParticleGroup>(pd, "All"), par) {}
  ~SPH() { System::log<System::MESSAGE>("[SPH] Destroyed."); }

  void sum(Computables, hipStream_t st = 0) override {  // SPH.cu:178-215
    System::log<System::DEBUG1>("[SPH] Summing forces");
    if (!nl) nl = std::make_shared<NeighbourList>(pg);
    const real rcut = real(2.0) * support;  // Kernel::M4CubicSpline::getCutOff
    nl->update(box, rcut, st);
    float L[3]; int per[3];
    box.toArrays(L, per);
    auto mass = pd->getMassIfAllocated(access::gpu, access::read);
    auto force = pd->getForce(access::gpu, access::readwrite);
    auto vel = pd->getVel(access::gpu, access::readwrite);
    detail::check(uammd_sph_sum_verletlist(nl->handle(), (const float *)vel.raw(), mass.raw(), L, per, support, viscosity, gasStiffness,
                                           restDensity, (float *)force.raw(), nullptr, nullptr, (void *)st));
  }

private:
  shared_ptr<NeighbourList> nl;
  Box box;
  real support;
  real gasStiffness;
  real restDensity;
  real viscosity;
};

}  // namespace uammd
