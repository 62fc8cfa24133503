// An SPH fluid the way a user builds it from a plain C++14 translation unit (g++, the C ABI): VerletNVE + SPH (Integrator/VerletNVE.cuh,
// Interactor/SPH.cuh) in the state of the reference's SPH example: an fcc lattice at number density 0.247 in a periodic cube, support 2.4,
// rest density 0.3, gas stiffness 60, viscosity 10, dt 0.01.  Particle i starts with velocity 0.05 (+-1, +-1, +-1), the signs being bits
// 0, 1 and 2 of i (no net momentum when N is a multiple of 8).
// Arguments: N steps.  One SPH::sum of the initial state, then `steps` steps.  Prints one line:
//   "sph N <N> sumAbsF <sum |F| of the first sum> weighted <sum (i % 17 + 1) F, three numbers> steps <steps> momentum <px> <py> <pz>
//    sumAbsV <sum |v| after the run> finite <0 | 1>"
// tests/test_gpu_sph.py compares the first sum with the Python layer's on the same input and checks the momentum.
#include "Integrator/VerletNVE.cuh"
#include "Interactor/SPH.cuh"
#include "uammd.h"
#include "utils/InitialConditions.cuh"

#include <cmath>
#include <cstdio>
#include <cstdlib>

int main(int argc, char *argv[]) {
  using namespace uammd;
  const int N = argc > 1 ? std::atoi(argv[1]) : 16000;
  const int steps = argc > 2 ? std::atoi(argv[2]) : 50;
  const real L = std::cbrt(N / 0.247);
  auto sys = std::make_shared<System>();
  auto pd = std::make_shared<ParticleData>(N, sys);
  {
    auto pos = pd->getPos(access::cpu, access::write);
    auto vel = pd->getVel(access::cpu, access::write);
    auto initial = initLattice(make_real3(L, L, L), N, fcc);
    for (int i = 0; i < N; ++i) {
      pos[i] = initial[i];
      pos[i].w = 0;
      vel[i] = make_real3(i & 1 ? 0.05f : -0.05f, i & 2 ? 0.05f : -0.05f, i & 4 ? 0.05f : -0.05f);
    }
  }
  SPH::Parameters par;
  par.box = Box(make_real3(L, L, L));
  par.support = 2.4;
  par.viscosity = 10;
  par.gasStiffness = 60;
  par.restDensity = 0.3;
  auto sph = std::make_shared<SPH>(pd, par);
  double sumAbsF = 0, wx = 0, wy = 0, wz = 0;
  {
    auto force = pd->getForce(access::cpu, access::write);
    for (int i = 0; i < N; ++i) force[i] = make_real4(0, 0, 0, 0);
  }
  sph->sum(Interactor::Computables{true, false, false, false}, 0);
  {
    auto force = pd->getForce(access::cpu, access::read);
    for (int i = 0; i < N; ++i) {
      const real4 f = force[i];
      sumAbsF += std::fabs((double)f.x) + std::fabs((double)f.y) + std::fabs((double)f.z);
      const double w = i % 17 + 1;
      wx += w * f.x; wy += w * f.y; wz += w * f.z;
    }
  }
  VerletNVE::Parameters vpar;
  vpar.dt = 0.01;
  vpar.initVelocities = false;
  auto verlet = std::make_shared<VerletNVE>(pd, vpar);
  verlet->addInteractor(sph);
  for (int s = 0; s < steps; ++s) verlet->forwardTime();
  double px = 0, py = 0, pz = 0, sumAbsV = 0;
  bool finite = true;
  {
    auto vel = pd->getVel(access::cpu, access::read);
    auto pos = pd->getPos(access::cpu, access::read);
    for (int i = 0; i < N; ++i) {
      const real3 v = vel[i];
      const real4 p = pos[i];
      px += v.x; py += v.y; pz += v.z;
      sumAbsV += std::sqrt((double)v.x * v.x + (double)v.y * v.y + (double)v.z * v.z);
      finite = finite && std::isfinite(v.x + v.y + v.z + p.x + p.y + p.z);
    }
  }
  std::printf("sph N %d sumAbsF %.9g weighted %.9g %.9g %.9g steps %d momentum %.9g %.9g %.9g sumAbsV %.9g finite %d\n", N, sumAbsF, wx, wy, wz,
              steps, px, py, pz, sumAbsV, finite ? 1 : 0);
  return 0;
}
