// The DPD pair force written as a USER potential (compute / getInfo / set, the formula of Interactor/Potential/DPD.cuh:121-152) and run
// through the generic PairForces<MyPotential, CellList> of device/PairForces.hip.hpp: how DPD could be run before the library had a
// kernel for it, and the baseline tools/time_dpd.py times the library's kernel against.  It uses nothing newer than the generic path, so
// it compiles against older headers of this project as well.
//   dpd_generic_baseline STATE REPS     STATE: int32 N, float32 L, N x float4 positions, N x float3 velocities (tools/time_dpd.py writes it)
// Prints one JSON line: ms per sum with the list rebuilt every time, and with the list kept.
#include "Interactor/PairForces.cuh"
#include "third_party/saruprng.cuh"
#include "uammd.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace uammd;

struct UserDPD {
  real rcut = 1, A = 25, gamma = 4.5, sigma = 14.142135f;
  int step = 0;
  real getCutOff() { return rcut; }
  struct Transverser {
    real3 *vel;
    real4 *force;
    Box box;
    unsigned int seed, step;
    int N;
    real invrcut, gamma, sigma, A;
    struct Info { real3 vel; int id; };
    __device__ real3 compute(const real4 &pi, const real4 &pj, const Info &infoi, const Info &infoj) {
      const real3 rij = box.apply_pbc(make_real3(pi) - make_real3(pj));
      const real3 vij = infoi.vel - infoj.vel;
      unsigned int i = infoi.id, j = infoj.id;
      if (i > j) { const unsigned int t = i; i = j; j = t; }
      Saru rng(i + (unsigned int)N * j, seed, step);
      const real rmod = sqrtf(dot(rij, rij));
      if (rmod == real(0)) return real3(0, 0, 0);
      const real invrmod = real(1.0) / rmod;
      if (invrmod <= invrcut) return real3(0, 0, 0);
      const real wr = real(1.0) - rmod * invrcut;
      const real Fc = A * wr * invrmod;
      const real Fd = -gamma * wr * wr * invrmod * invrmod * dot(rij, vij);
      const real Fr = rng.gf(real(0.0), sigma * sqrtf(gamma) * wr * invrmod).x;
      return (Fc + Fd + Fr) * rij;
    }
    __device__ Info getInfo(int pi) { return {vel[pi], pi}; }
    __device__ void set(int pi, const real3 &total) { force[pi] += make_real4(total, 0); }
  };
  Transverser getTransverser(Interactor::Computables, Box box, shared_ptr<ParticleData> pd) {
    auto vel = pd->getVel(access::gpu, access::read);
    auto force = pd->getForce(access::gpu, access::readwrite);
    step++;
    return Transverser{vel.raw(), force.raw(), box, 0x1234567u, (unsigned int)step, pd->getNumParticles(), real(1.0) / rcut, gamma, sigma, A};
  }
};

int main(int argc, char *argv[]) {
  if (argc < 3) { std::fprintf(stderr, "usage: %s STATE REPS\n", argv[0]); return 2; }
  std::FILE *f = std::fopen(argv[1], "rb");
  if (!f) { std::perror(argv[1]); return 2; }
  int N; float L;
  if (std::fread(&N, 4, 1, f) != 1 || std::fread(&L, 4, 1, f) != 1) return 2;
  std::vector<real4> p(N);
  std::vector<real3> v(N);
  if (std::fread(p.data(), sizeof(real4), N, f) != (size_t)N || std::fread(v.data(), sizeof(real3), N, f) != (size_t)N) return 2;
  std::fclose(f);
  const int reps = std::atoi(argv[2]);
  auto pd = std::make_shared<ParticleData>(N);
  {
    auto pos = pd->getPos(access::cpu, access::write);
    auto vel = pd->getVel(access::cpu, access::write);
    for (int i = 0; i < N; ++i) { pos[i] = p[i]; vel[i] = v[i]; }
  }
  using PF = PairForces<UserDPD, CellList>;
  PF::Parameters par;
  par.box = Box(make_real3(L, L, L));
  auto pf = std::make_shared<PF>(pd, par, std::make_shared<UserDPD>());
  Interactor::Computables comp;
  comp.force = true;
  hipEvent_t a, b;
  hipEventCreate(&a);
  hipEventCreate(&b);
  float ms[2];
  for (int rebuild = 1; rebuild >= 0; --rebuild) {
    for (int w = 0; w < 5; ++w) pf->sum(comp, 0);
    hipDeviceSynchronize();
    hipEventRecord(a, 0);
    for (int r = 0; r < reps; ++r) {
      if (rebuild) pd->getPos(access::gpu, access::readwrite);   // raises the position-write signal: the list is rebuilt
      pf->sum(comp, 0);
    }
    hipEventRecord(b, 0);
    hipEventSynchronize(b);
    hipEventElapsedTime(&ms[rebuild], a, b);
    ms[rebuild] /= reps;
  }
  std::printf("{\"N\": %d, \"reps\": %d, \"ms_sum_with_list_build\": %.5f, \"ms_sum_list_kept\": %.5f}\n", N, reps, ms[1], ms[0]);
  return 0;
}
