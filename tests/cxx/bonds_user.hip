// BondedForces<UserBond, 2> with a bond kind of the program's own (device/BondedForces.hip.hpp, hipcc): a harmonic spring whose constant
// follows the simulation time through ParameterUpdatable (k * (1 + t)).  Two systems: chains of 100 beads (every row on the lane shape)
// and 600 particles with 100 random partners each (rows of ~200 entries: the wave shape).  Prints "set index id fx fy fz energy virial"
// per particle after a sum at t = 0.5; tests/test_gpu_bonded.py checks the lines against its NumPy restatement.
#include "Interactor/BondedForces.cuh"
#include "uammd.cuh"

#include <cstdio>
#include <fstream>
#include <random>

using namespace uammd;

struct UserBond : public ParameterUpdatable {
  Box box;
  real time = 0;
  UserBond(Box box) : box(box) {}
  struct BondInfo { real k, r0; };
  __device__ ComputeType compute(int bond_index, int ids[2], real3 pos[2], Interactor::Computables comp, BondInfo bi) {
    real3 r12 = box.apply_pbc(pos[1] - pos[0]);
    if (bond_index == ids[1]) r12 = real(-1.0) * r12;   // from this particle to the other one
    const real r2 = dot(r12, r12);
    if (r2 == real(0)) return ComputeType{};
    const real r = sqrt(r2);
    const real k = bi.k * (real(1.0) + time);
    ComputeType ct;
    ct.force = k * (r - bi.r0) / r * r12;
    ct.energy = comp.energy ? real(0.25) * k * (r - bi.r0) * (r - bi.r0) : real(0);
    ct.virial = comp.virial ? -dot(ct.force, r12) : real(0);
    return ct;
  }
  static BondInfo readBond(std::istream &in) {
    BondInfo bi;
    in >> bi.k >> bi.r0;
    return bi;
  }
  void updateSimulationTime(real t) override { time = t; }
};

void runSet(const char *name, int N, real L, const std::string &file, unsigned seed) {
  auto pd = std::make_shared<ParticleData>(N);
  {
    std::mt19937 gen(seed);
    std::uniform_real_distribution<float> u(-0.5f * L, 0.5f * L);
    auto pos = pd->getPos(access::cpu, access::write);
    auto f = pd->getForce(access::cpu, access::write);
    auto e = pd->getEnergy(access::cpu, access::write);
    auto v = pd->getVirial(access::cpu, access::write);
    for (int i = 0; i < N; ++i) { pos[i] = make_real4(u(gen), u(gen), u(gen), 0); f[i] = make_real4(0); e[i] = 0; v[i] = 0; }
  }
  pd->sortParticles();   // the rows must follow the reorder
  using BF = BondedForces<UserBond, 2>;
  BF::Parameters par;
  par.file = file;
  auto bf = std::make_shared<BF>(pd, par, std::make_shared<UserBond>(Box(make_real3(L))));
  bf->updateSimulationTime(0.5);
  Interactor::Computables comp;
  comp.force = comp.energy = comp.virial = true;
  bf->sum(comp, 0);
  auto pos = pd->getPos(access::cpu, access::read);
  auto f = pd->getForce(access::cpu, access::read);
  auto e = pd->getEnergy(access::cpu, access::read);
  auto v = pd->getVirial(access::cpu, access::read);
  auto id = pd->getId(access::cpu, access::read);
  for (int i = 0; i < N; ++i)
    std::printf("%s %d %.9g %.9g %.9g %.9g %.9g %.9g %.9g %.9g\n", name, id[i], pos[i].x, pos[i].y, pos[i].z, f[i].x, f[i].y, f[i].z, e[i], v[i]);
}

int main(int argc, char *argv[]) {
  const std::string dir = argc > 1 ? argv[1] : ".";
  {
    std::ofstream out(dir + "/chain.bonds");
    const int nc = 10, len = 100;
    out << nc * (len - 1) << "\n";
    for (int c = 0; c < nc; ++c)
      for (int j = 0; j + 1 < len; ++j) out << c * len + j << " " << c * len + j + 1 << " 2.5 0.7\n";
  }
  {
    std::ofstream out(dir + "/dense.bonds");
    std::mt19937 gen(7);
    std::uniform_int_distribution<int> pick(0, 599);
    const int n = 600, m = 100;
    out << n * m << "\n";
    for (int i = 0; i < n; ++i)
      for (int j = 0; j < m; ++j) {
        int p = pick(gen);
        if (p == i) p = (p + 1) % n;
        out << i << " " << p << " 1.5 2.0\n";
      }
  }
  runSet("chain", 1000, 40, dir + "/chain.bonds", 1);
  runSet("dense", 600, 12, dir + "/dense.bonds", 2);
  return 0;
}
