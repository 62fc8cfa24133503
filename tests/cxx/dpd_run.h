// Shared by dpd_builtin.cpp and dpd_user.hip: a DPD fluid (rho = 3, rc = 1, A = 25, gamma = 4.5, kT = 1, dt = 0.01) started from uniform
// random positions at rest, moved by VerletNVE with PairForces<Potential, NeighbourList> as its only interactor.
// Arguments: N steps measured.  The kinetic temperature sum m v^2 / (3 N) is averaged over the last `measured` steps in 20 blocks.
// Prints one line: "dpd N <N> temperature <mean> stderr <standard error of the 20 block means> momentum <px> <py> <pz>".
#pragma once
#include "Integrator/VerletNVE.cuh"
#include "Interactor/PairForces.cuh"
#include "Interactor/Potential/DPD.cuh"
#include "uammd.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

template <class Potential, class NeighbourList> int runDPD(int argc, char *argv[], typename Potential::Parameters dpdPar) {
  using namespace uammd;
  const int N = argc > 1 ? std::atoi(argv[1]) : 24000;
  const int steps = argc > 2 ? std::atoi(argv[2]) : 3000;
  const int measured = argc > 3 ? std::atoi(argv[3]) : 2000;
  const int blocks = 20;
  const real L = std::cbrt(N / 3.0);
  auto sys = std::make_shared<System>();
  auto pd = std::make_shared<ParticleData>(N, sys);
  {
    auto pos = pd->getPos(access::cpu, access::write);
    auto vel = pd->getVel(access::cpu, access::write);
    for (int i = 0; i < N; ++i) {
      pos[i] = make_real4(sys->rng().uniform(-0.5 * L, 0.5 * L), sys->rng().uniform(-0.5 * L, 0.5 * L), sys->rng().uniform(-0.5 * L, 0.5 * L), 0);
      vel[i] = make_real3(0, 0, 0);
    }
  }
  VerletNVE::Parameters par;
  par.dt = 0.01;
  par.initVelocities = false;
  auto verlet = std::make_shared<VerletNVE>(pd, par);
  dpdPar.cutOff = 1;
  dpdPar.dt = par.dt;
  dpdPar.temperature = 1;
  dpdPar.A = 25;
  using PF = PairForces<Potential, NeighbourList>;
  typename PF::Parameters pfPar;
  pfPar.box = Box(make_real3(L, L, L));
  verlet->addInteractor(std::make_shared<PF>(pd, pfPar, std::make_shared<Potential>(dpdPar)));
  std::vector<double> blockMean(blocks, 0.0);
  const int perBlock = measured / blocks;
  double px = 0, py = 0, pz = 0;
  for (int s = 0; s < steps; ++s) {
    verlet->forwardTime();
    const int m = s - (steps - perBlock * blocks);
    if (m >= 0 || s == steps - 1) {
      auto vel = pd->getVel(access::cpu, access::read);
      double v2 = 0;
      px = py = pz = 0;
      for (int i = 0; i < N; ++i) {
        const real3 v = vel[i];
        v2 += (double)v.x * v.x + (double)v.y * v.y + (double)v.z * v.z;
        px += v.x; py += v.y; pz += v.z;
      }
      if (m >= 0) blockMean[m / perBlock] += v2 / (3.0 * N) / perBlock;
    }
  }
  double mean = 0, var = 0;
  for (double b : blockMean) mean += b / blocks;
  for (double b : blockMean) var += (b - mean) * (b - mean) / (blocks - 1);
  std::printf("dpd N %d temperature %.9g stderr %.9g momentum %.9g %.9g %.9g\n", N, mean, std::sqrt(var / blocks), px, py, pz);
  return 0;
}
