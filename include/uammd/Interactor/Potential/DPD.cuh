// Same include path as the reference's src/Interactor/Potential/DPD.cuh: the dissipative-particle-dynamics potential.  Used with a
// VerletNVE integrator through a PairForces interactor it gives a DPD simulation:
//
//   Potential::DPD::Parameters par;
//   par.cutOff = 1; par.dt = 0.01; par.gamma = 4.5; par.temperature = 1; par.A = 25;
//   auto dpd = std::make_shared<Potential::DPD>(par);
//   PairForces<Potential::DPD>::Parameters params; params.box = box;
//   verlet->addInteractor(std::make_shared<PairForces<Potential::DPD>>(pd, params, dpd));
//
// PairForces<Potential::DPD, CellList> (the default dissipation, a constant gamma) runs the library's kernel through the C ABI
// (uammd_dpd_transverse_celllist / _nbody): host code only, plain g++ is enough.  A user's dissipation functor
// (DPD_impl<MyDissipation>, with dissipativeStrength(i, j, pi, pj, vi, vj)) and the VerletList go through the generic
// PairForces<MyPotential, NL> of device/PairForces.hip.hpp, which needs hipcc as it needs nvcc in the reference.
//
// A deliberate departure: the reference's DPD.cuh offers getForceTransverser only, which its PairForces never asks for
// (PairForces.cu:28-37,75-76 want getTransverser and fall back to a null transverser), so that PairForces<Potential::DPD> sums nothing
// there.  Here getTransverser(Computables, Box, pd) hands out what the file plainly means: ForceTransverser::compute (:121-152).
#pragma once
#if defined(DOUBLE_PRECISION)
#error "DPD.cuh: this module has a single-precision backend only on MI355X (uammd.h, PRECISION): build without -DDOUBLE_PRECISION"
#endif
#include "../PairForces.cuh"
#include "../../third_party/saruprng.cuh"
#include <cmath>

namespace uammd {
namespace Potential {

struct DefaultDissipation {  // DPD.cuh:23-38
  real gamma;
  UAMMD_HOSTDEV DefaultDissipation() : DefaultDissipation(1.0) {}
  UAMMD_HOSTDEV DefaultDissipation(real gamma) : gamma(gamma) {}
  template <class... T> UAMMD_HOSTDEV real dissipativeStrength(T...) const { return gamma; }
};

template <class DissipativeStrength = DefaultDissipation> class DPD_impl : public ParameterUpdatable {
protected:
  int step;
  real rcut;
  DissipativeStrength gamma;  // dissipative force strength
  real temperature;
  real sigma;                 // random force strength without the sqrt(gamma): sqrt(2 kT) / sqrt(dt)
  real dt;
  real A;                     // maximum repulsion between a pair
  unsigned long long seed = 0;
  bool haveSeed = false;
  void updateSigma() { sigma = (real)(std::sqrt(2.0 * temperature) / std::sqrt((double)dt)); }
public:
  struct Parameters {  // DPD.cuh:52-58
    real cutOff = 1;
    real dt = 0;
    DissipativeStrength gamma;  // 1.0 by default
    real temperature = 0;
    real A = 1;
  };
  DPD_impl(Parameters par) : DPD_impl(nullptr, par) {}
  // (the system parameter is unused, as in the reference: kept for old programs)
  DPD_impl(shared_ptr<System>, Parameters par)
      : step(0), rcut(par.cutOff), gamma(par.gamma), temperature(par.temperature), dt(par.dt), A(par.A) {
    System::log<System::MESSAGE>("[Potential::DPD] Created");
    updateSigma();
    System::log<System::MESSAGE>("[Potential::DPD] Temperature: %f", (double)temperature);
    System::log<System::MESSAGE>("[Potential::DPD] Cut off: %f", (double)rcut);
    System::log<System::MESSAGE>("[Potential::DPD] aij: %f", (double)A);
  }
  ~DPD_impl() { System::log<System::MESSAGE>("[Potential::DPD] Destroyed"); }
  real getCutOff() { return rcut; }
  void updateTemperature(real newTemp) override { temperature = newTemp; updateSigma(); }  // :82-85
  void updateTimeStep(real newdt) override { dt = newdt; updateSigma(); }                   // :87-90

  // What one force evaluation needs (DPD.cuh:161-170): the seed is drawn once from pd->getSystem()->rng().next(), the step counter
  // advances once per request.
  struct Arguments { real rcut, A, sigma; DissipativeStrength gamma; unsigned long long seed, step; int N; };
  Arguments nextForceArguments(shared_ptr<ParticleData> pd) {
    if (!haveSeed) { seed = pd->getSystem()->rng().next(); haveSeed = true; }
    step++;
    return Arguments{rcut, A, sigma, gamma, seed, (unsigned long long)step, pd->getNumParticles()};
  }
  // Energy and virial are not defined for DPD (DPD.cuh:171-180): asking says so at CRITICAL and adds nothing
  static bool refuseEnergy(Interactor::Computables comp) {
    if (comp.energy || comp.virial) System::log<System::CRITICAL>("[DPD] No way of measuring energy in DPD");
    return !comp.force;
  }

#if defined(__HIPCC__)
  // DPD.cuh:92-159 as the generic traversals of device/PairForces.hip.hpp take it: compute / getInfo / set
  struct Transverser {
    real3 *vel;
    real4 *force;   // null: nothing is added (energy or virial alone was asked for)
    Box box;
    unsigned int seed, step;
    int N;
    real invrcut;
    DissipativeStrength gamma;
    real sigma, A;
    using returnInfo = real3;
    struct Info { real3 vel; int id; };
    __device__ returnInfo compute(const real4 &pi, const real4 &pj, const Info &infoi, const Info &infoj) {
      const real3 rij = box.apply_pbc(make_real3(pi) - make_real3(pj));
      const real3 vij = infoi.vel - infoj.vel;
      unsigned int i = (unsigned int)infoi.id, j = (unsigned int)infoj.id;
      if (i > j) { const unsigned int t = i; i = j; j = t; }
      const unsigned int ij = i + (unsigned int)N * j;   // (the reference's int product overflows for N > 46340: unsigned wraps the same way)
      Saru rng(ij, seed, step);
      const real rmod = sqrtf(dot(rij, rij));
      if (rmod == real(0)) return real3(0, 0, 0);
      const real invrmod = real(1.0) / rmod;
      if (invrmod <= invrcut) return real3(0, 0, 0);
      const real wr = real(1.0) - rmod * invrcut;
      const real Fc = A * wr * invrmod;
      const real wd = wr * wr;
      const real g = gamma.dissipativeStrength((int)i, (int)j, pi, pj, infoi.vel, infoj.vel);
      const real Fd = -g * wd * invrmod * invrmod * dot(rij, vij);
      const real Fr = rng.gf(real(0.0), sigma * sqrtf(g) * wr * invrmod).x;
      return (Fc + Fd + Fr) * rij;
    }
    __device__ Info getInfo(int pi) { return {vel[pi], pi}; }
    __device__ void set(int pi, const returnInfo &total) { if (force) force[pi] += make_real4(total, 0); }
  };
  Transverser getTransverser(Interactor::Computables comp, Box box, shared_ptr<ParticleData> pd) {
    const bool nothing = refuseEnergy(comp);
    auto vel = pd->getVel(access::gpu, access::read);
    real4 *f = nothing ? nullptr : pd->getForce(access::gpu, access::readwrite).raw();
    const Arguments a = nextForceArguments(pd);
    return Transverser{vel.raw(), f, box, (unsigned int)a.seed, (unsigned int)a.step, a.N, real(1.0) / a.rcut, a.gamma, a.sigma, a.A};
  }
#endif
};

using DPD = DPD_impl<>;
}  // namespace Potential

// ---- PairForces<Potential::DPD, CellList>: the library's kernel (PairForces.cu:43-78 with DPD.cuh:121-152) ----------------------------
template <> class PairForces<Potential::DPD, CellList> : public Interactor {
  Box box;
  shared_ptr<Potential::DPD> pot;
  shared_ptr<CellList> nl;
public:
  struct Parameters { Box box; shared_ptr<CellList> nl = nullptr; };
  PairForces(shared_ptr<ParticleData> pd, Parameters par, shared_ptr<Potential::DPD> pot)
      : Interactor(pd, "PairForces"), box(par.box), pot(pot), nl(par.nl) {}
  PairForces(shared_ptr<ParticleGroup> pg, Parameters par, shared_ptr<Potential::DPD> pot)
      : Interactor(pg, "PairForces"), box(par.box), pot(pot), nl(par.nl) {}
  // ParameterUpdatableDelegate<Potential> (PairForces.cuh:25,40-44): every update goes on to the potential
  void updateBox(Box b) override { box = b; pot->updateBox(b); }
  void updateTimeStep(real v) override { pot->updateTimeStep(v); }
  void updateSimulationTime(real v) override { pot->updateSimulationTime(v); }
  void updateTemperature(real v) override { pot->updateTemperature(v); }
  void updateViscosity(real v) override { pot->updateViscosity(v); }
  shared_ptr<Potential::DPD> getPotential() { return pot; }
  void sum(Computables comp, hipStream_t st = 0) override {
    const bool nothing = Potential::DPD::refuseEnergy(comp);
    const auto a = pot->nextForceArguments(pd);   // (the step advances once per transverser request, force or not: DPD.cuh:166)
    if (nothing) return;
    float L[3]; int per[3];
    box.toArrays(L, per);
    const real rcut = a.rcut;
    const bool useNL = !(box.boxSize.x <= 3 * rcut && box.boxSize.y <= 3 * rcut && box.boxSize.z <= 3 * rcut);
    const int *globalIndex = subgroup ? subgroup->getIndicesRawPtr(access::gpu) : nullptr;
    if (useNL) {
      if (!nl) nl = subgroup ? make_shared<CellList>(subgroup) : make_shared<CellList>(pd);
      nl->update(box, rcut, st);
    }
    auto vel = pd->getVel(access::gpu, access::read);
    auto force = pd->getForce(access::gpu, access::readwrite);
    if (useNL) {
      detail::check(uammd_dpd_transverse_celllist(nl->handle(), (const float *)vel.raw(), L, per, rcut, a.A, a.gamma.gamma, a.sigma, a.seed,
                                                  a.step, a.N, (float *)force.raw(), globalIndex, (void *)st));
    } else {
      const int n = subgroup ? subgroup->getNumberParticles() : pd->getNumParticles();
      auto pos = pd->getPos(access::gpu, access::read);
      detail::check(uammd_dpd_transverse_nbody((const float *)pos.raw(), (const float *)vel.raw(), n, L, per, rcut, a.A, a.gamma.gamma, a.sigma,
                                               a.seed, a.step, a.N, (float *)force.raw(), globalIndex, (void *)st));
    }
  }
};

}  // namespace uammd
