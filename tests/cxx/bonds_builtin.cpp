// BondedForces with the built-in kinds from a plain C++14 translation unit (g++, the C ABI): the four particles of
// tests/golden/bonds/init.pos with the Harmonic, Angular and Torsional bond files beside it, in a box of 32 (the reference's
// test/Bonds/data.main).  Prints, per kind and particle, "kind index fx fy fz energy virial"; tests/test_gpu_bonded.py checks the lines
// against its NumPy restatement.  With "errors" as the first argument it only reads a missing and a truncated bond file and prints the
// exception each one raised (no GPU needed).
#include "Interactor/AngularBondedForces.cuh"
#include "Interactor/BondedForces.cuh"
#include "Interactor/TorsionalBondedForces.cuh"
#include "uammd.h"

#include <cstdio>
#include <fstream>
#include <string>

using namespace uammd;

template <class BF> void run(const char *name, shared_ptr<ParticleData> pd, std::shared_ptr<BF> bf) {
  const int N = pd->getNumParticles();
  {
    auto f = pd->getForce(access::cpu, access::write);
    auto e = pd->getEnergy(access::cpu, access::write);
    auto v = pd->getVirial(access::cpu, access::write);
    for (int i = 0; i < N; ++i) { f[i] = make_real4(0); e[i] = 0; v[i] = 0; }
  }
  Interactor::Computables comp;
  comp.force = comp.energy = comp.virial = true;
  bf->sum(comp, 0);
  auto f = pd->getForce(access::cpu, access::read);
  auto e = pd->getEnergy(access::cpu, access::read);
  auto v = pd->getVirial(access::cpu, access::read);
  for (int i = 0; i < N; ++i) std::printf("%s %d %.9g %.9g %.9g %.9g %.9g\n", name, i, f[i].x, f[i].y, f[i].z, e[i], v[i]);
}

int main(int argc, char *argv[]) {
  const std::string arg = argc > 1 ? argv[1] : ".";
  if (arg == "errors") {
    try {
      BondedForces_ns::readBondFile<BondedType::Harmonic, 2>("/nonexistent/particles.bonds");
    } catch (std::ios_base::failure &) {
      std::printf("missing: ios_base::failure\n");
    } catch (std::runtime_error &) {
      std::printf("missing: runtime_error\n");
    }
    const std::string shortFile = argc > 2 ? argv[2] : "short.bonds";
    try {
      BondedForces_ns::readBondFile<BondedType::Harmonic, 2>(shortFile);
      std::printf("short: no exception\n");
    } catch (std::ios_base::failure &) {
      std::printf("short: ios_base::failure\n");
    } catch (std::runtime_error &) {
      std::printf("short: runtime_error\n");
    }
    return 0;
  }
  const std::string dir = arg;
  std::ifstream in(dir + "/init.pos");
  int N;
  in >> N;
  auto pd = std::make_shared<ParticleData>(N);
  {
    auto pos = pd->getPos(access::cpu, access::write);
    for (int i = 0; i < N; ++i) {
      real3 p;
      in >> p.x >> p.y >> p.z;
      pos[i] = make_real4(p.x, p.y, p.z, 0);
    }
  }
  const real3 L = make_real3(32);
  {
    using BF = BondedForces<BondedType::Harmonic, 2>;
    BF::Parameters par;
    par.file = dir + "/harmonic.bonds";
    run("harmonic", pd, std::make_shared<BF>(pd, par, std::make_shared<BondedType::Harmonic>(Box(L))));
  }
  {
    using BF = AngularBondedForces<AngularBondedForces_ns::AngularBond>;
    BF::Parameters par;
    par.file = dir + "/angular.bonds";
    run("angular", pd, std::make_shared<BF>(pd, par, std::make_shared<AngularBondedForces_ns::AngularBond>(L)));
  }
  {
    using BF = TorsionalBondedForces<TorsionalBondedForces_ns::TorsionalBond>;
    BF::Parameters par;
    par.file = dir + "/torsional.bonds";
    run("torsional", pd, std::make_shared<BF>(pd, par, std::make_shared<TorsionalBondedForces_ns::TorsionalBond>(L)));
  }
  return 0;
}
