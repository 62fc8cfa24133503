// The host side of MC::ForceBiased (Integrator/MonteCarlo/ForceBiased.cuh) without a GPU, for tests/test_forcebiased_cpu.py:
//   forcebiased_host optimize <target> <initialStep>   reads a line of '1' (accepted) and '0' (rejected) from stdin, drives
//                                                      forcebiased_ns::Optimize with it and prints step size and ratio after every try
//   forcebiased_host refusals                          the constructor's refusals, one line each
#include "uammd.cuh"
#include "Integrator/MonteCarlo/ForceBiased.cuh"
#include <cstdio>
#include <iostream>
#include <string>
using namespace uammd;

static int refused(const char *what, std::shared_ptr<ParticleData> pd, MC::ForceBiased::Parameters par) {
  try {
    MC::ForceBiased mala(pd, par);
  } catch (const std::runtime_error &e) {
    std::printf("%s: %s\n", what, e.what());
    return 0;
  }
  std::printf("%s: accepted\n", what);
  return 1;
}

int main(int argc, char *argv[]) {
  const std::string mode = argc > 1 ? argv[1] : "";
  if (mode == "optimize" && argc == 4) {
    MC::forcebiased_ns::Optimize opt((real)std::atof(argv[2]), (real)std::atof(argv[3]));
    std::string script;
    std::getline(std::cin, script);
    for (char c : script) {
      if (c == '1') opt.registerAccept();
      else if (c == '0') opt.registerReject();
      else continue;
      std::printf("%a %a\n", (double)opt.getStepSize(), (double)opt.getCurrentAcceptanceRatio());
    }
    return 0;
  }
  if (mode == "refusals") {
    System::maxLogLevel() = System::CRITICAL;
    auto sys = std::make_shared<System>();
    auto pd = std::make_shared<ParticleData>(8, sys);
    MC::ForceBiased::Parameters ok;
    ok.beta = 2.0;
    int bad = 0;
    MC::ForceBiased::Parameters par;  // beta = -1 by default
    bad += refused("default beta", pd, par);
    par = ok; par.stepSize = 0;
    bad += refused("stepSize 0", pd, par);
    par = ok; par.acceptanceRatio = 0;
    bad += refused("acceptanceRatio 0", pd, par);
    par = ok; par.maxTrials = 0;
    bad += refused("maxTrials 0", pd, par);
    sys->rng().setSeed(77);
    MC::ForceBiased mala(pd, ok);  // draws its seed: the generator moves by exactly one next32()
    Xorshift128plus r;
    r.setSeed(77);
    r.next32();
    std::printf("seed draw: %s\n", r.next() == sys->rng().next() ? "one next32" : "differs");
    std::printf("accessors: %g %g %g %d %llu\n", (double)mala.getCurrentEnergy(), (double)mala.getCurrentStepSize(),
                (double)mala.getCurrentAcceptanceRatio(), mala.getLastNumberOfTrials(), mala.getTotalNumberOfTrials());
    return bad;
  }
  std::fprintf(stderr, "usage: forcebiased_host optimize <target> <initialStep> | refusals\n");
  return 2;
}
