// The run shared by mc_builtin.cpp (g++, MC_NVT::Anderson<Potential::LJ> on the C ABI) and mc_user.hip (hipcc, a functor of the program's
// own through device/Anderson.hip.hpp).
// Arguments: <positions: raw float32 x y z type rows> N L steps systemSeed saruSeed shift.  A periodic cube of edge L, rc = 2.5,
// sigma = epsilon = 1, T = 1.5, 10 tries per cell, jump 0.15, tuneSteps = steps (so the acceptance ratio is taken at the last step).
// Prints one line:
//   "mc N <N> steps <steps> hash <FNV-1a of the final position words, hex> ratio <acceptance ratio, %.9g> jump <step size, %.9g>"
// tests/test_mc_cxx.py compares it with the Python class's run from the same system seed: the host draws come from System::rng() in
// the same order on every front end, so the trajectories are the same bits.
#pragma once
#include "uammd.h"

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

template <class NVT, class Pot> int runMC(int argc, char *argv[]) {
  using namespace uammd;
  if (argc < 8) {
    std::fprintf(stderr, "usage: %s positions N L steps systemSeed saruSeed shift\n", argv[0]);
    return 2;
  }
  const int N = std::atoi(argv[2]);
  const real L = (real)std::atof(argv[3]);
  const int steps = std::atoi(argv[4]);
  const unsigned long long systemSeed = std::strtoull(argv[5], nullptr, 0);
  const int saruSeed = std::atoi(argv[6]);
  const bool shift = std::atoi(argv[7]) != 0;
  std::vector<float> in((size_t)4 * N);
  {
    FILE *f = std::fopen(argv[1], "rb");
    if (!f || std::fread(in.data(), sizeof(float), in.size(), f) != in.size()) {
      std::fprintf(stderr, "cannot read %d rows from %s\n", N, argv[1]);
      return 2;
    }
    std::fclose(f);
  }
  auto sys = std::make_shared<System>();
  sys->rng().setSeed(systemSeed);
  auto pd = std::make_shared<ParticleData>(N, sys);
  {
    auto pos = pd->getPos(access::cpu, access::write);
    for (int i = 0; i < N; ++i) pos[i] = make_real4(in[4 * i], in[4 * i + 1], in[4 * i + 2], in[4 * i + 3]);
  }
  auto pot = std::make_shared<Pot>();
  {
    typename Pot::InputPairParameters p;
    p.cutOff = 2.5;
    p.sigma = 1;
    p.epsilon = 1;
    p.shift = shift;
    pot->setPotParameters(0, 0, p);
  }
  typename NVT::Parameters par;
  par.box = Box(make_real3(L, L, L));
  par.temperature = 1.5;
  par.triesPerCell = 10;
  par.initialJumpSize = 0.15;
  par.tuneSteps = steps;
  par.seed = saruSeed;
  auto mc = std::make_shared<NVT>(pd, pot, par);
  for (int s = 0; s < steps; ++s) mc->forwardTime();
  std::uint64_t h = 1469598103934665603ull;
  {
    auto pos = pd->getPos(access::cpu, access::read);
    for (int i = 0; i < N; ++i) {
      const real4 p = pos[i];
      const float w[4] = {p.x, p.y, p.z, p.w};
      unsigned char b[16];
      std::memcpy(b, w, 16);
      for (unsigned char c : b) { h ^= c; h *= 1099511628211ull; }
    }
  }
  std::printf("mc N %d steps %d hash %016llx ratio %.9g jump %.9g\n", N, steps, (unsigned long long)h, (double)mc->getCurrentAcceptanceRatio(),
              (double)mc->getCurrentStepSize());
  return 0;
}
