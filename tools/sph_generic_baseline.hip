// The two SPH sums written as USER Transversers (compute / getInfo / set / zero, from the formulas of include/uammd_hip.h) and run through
// the generic device::transverseList on the same VerletList, with a transform for the pressure between them: how SPH had to be run before
// the library had kernels for it, and the baseline tools/time_sph.py times the library against.
//   sph_generic_baseline STATE REPS   STATE: int32 N, float32 L, N x float4 positions, N x float3 velocities (tools/time_sph.py writes it)
// Prints one JSON line: ms per force evaluation (list update + two traversals + transform) with the list rebuilt every time and with the
// list kept, and sum |F| of one evaluation (to be compared with the library's).
#include "uammd.cuh"
#include "Interactor/NeighbourList/VerletList.cuh"
#include "device/Transverser.hip.hpp"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace uammd;

struct Spline {   // the M4 cubic spline and the "gradient" as the module's formulas state them
  real h;
  __device__ real W(real3 rij) const {
    const real q = sqrtf(dot(rij, rij)) / h;
    if (q >= real(2.0)) return 0;
    real w = (real(2.0) - q) * (real(2.0) - q) * (real(2.0) - q);
    if (q <= real(1.0)) w -= real(4.0) * (real(1.0) - q) * (real(1.0) - q) * (real(1.0) - q);
    return w * (real(1.0) / (h * h * h * real(4.0) * real(M_PI)));
  }
  __device__ real3 G(real3 rij) const {
    const real r = sqrtf(dot(rij, rij));
    const real invh = real(1.0) / h;
    const real q = r * invh;
    if (q >= real(2.0)) return make_real3(0, 0, 0);
    const real invh3 = invh * invh * invh;
    const real c = -invh3 * invh3 * real(3.0) / (real(4.0) * real(M_PI));
    if (q <= real(1.0)) return c * (real(3.0) * r - real(4.0) * h) * rij;
    return c * (real(2.0) * h - r) * (real(2.0) * h - r) * rij;
  }
};

struct Density {
  Spline k;
  Box box;
  real *density;
  __device__ real zero() { return 0; }
  __device__ real getInfo(int) { return real(1.0); }   // the mass (none allocated: 1)
  __device__ real compute(const real4 &ri, const real4 &rj, real, real mj) { return mj * k.W(box.apply_pbc(make_real3(rj) - make_real3(ri))); }
  __device__ void accumulate(real &total, const real &cur) { total += cur; }
  __device__ void set(int i, const real &total) { density[i] = total; }
};

struct Force {
  Spline k;
  Box box;
  real4 *force;
  real3 *vel;
  real *density, *pressure;
  real nu, eps;
  struct Info { real Pdivrho2, mass; real3 vel; };
  __device__ real3 zero() { return make_real3(0, 0, 0); }
  __device__ Info getInfo(int i) { const real rho = density[i]; return Info{pressure[i] / (rho * rho), real(1.0), vel[i]}; }
  __device__ real3 compute(const real4 &ri, const real4 &rj, const Info &a, const Info &b) {
    const real3 rij = box.apply_pbc(make_real3(rj) - make_real3(ri));
    const real3 vij = b.vel - a.vel;
    const real vis = -nu * (dot(vij, rij) / (dot(rij, rij) + eps));
    return a.mass * b.mass * (a.Pdivrho2 + b.Pdivrho2 + vis) * k.G(rij);
  }
  __device__ void accumulate(real3 &total, const real3 &cur) { total += cur; }
  __device__ void set(int i, const real3 &total) { force[i] += make_real4(total, 0); }
};

__global__ void pressureOf(const real *density, real *pressure, real K, real rho0, int N) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < N) pressure[i] = K * (density[i] - rho0);
}

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
  const real h = 2.4, K = 60, rho0 = 0.3, nu = 10;
  auto pd = std::make_shared<ParticleData>(N);
  {
    auto pos = pd->getPos(access::cpu, access::write);
    auto vel = pd->getVel(access::cpu, access::write);
    auto force = pd->getForce(access::cpu, access::write);
    for (int i = 0; i < N; ++i) { pos[i] = p[i]; vel[i] = v[i]; force[i] = make_real4(0, 0, 0, 0); }
  }
  const Box box(make_real3(L, L, L));
  VerletList nl(pd);
  real *density, *pressure;
  if (hipMalloc(&density, sizeof(real) * N) != hipSuccess || hipMalloc(&pressure, sizeof(real) * N) != hipSuccess) return 3;
  auto sum = [&]() {
    nl.update(box, real(2.0) * h, 0);
    auto vel = pd->getVel(access::gpu, access::read);
    auto force = pd->getForce(access::gpu, access::readwrite);
    Density d{Spline{h}, box, density};
    if (device::transverseList(nl.handle(), d, 0) != 0) std::exit(4);
    hipLaunchKernelGGL(pressureOf, dim3((N + 255) / 256), dim3(256), 0, 0, density, pressure, K, rho0, N);
    Force fr{Spline{h}, box, force.raw(), vel.raw(), density, pressure, nu, real(0.001) * h * h};
    if (device::transverseList(nl.handle(), fr, 0) != 0) std::exit(4);
  };
  sum();
  double sumAbsF = 0;
  {
    auto force = pd->getForce(access::cpu, access::read);
    for (int i = 0; i < N; ++i) sumAbsF += std::fabs((double)force[i].x) + std::fabs((double)force[i].y) + std::fabs((double)force[i].z);
  }
  hipEvent_t a, b;
  if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) return 3;
  float ms[2];
  for (int rebuild = 1; rebuild >= 0; --rebuild) {
    for (int w = 0; w < 5; ++w) sum();
    (void)hipDeviceSynchronize();
    (void)hipEventRecord(a, 0);
    for (int r = 0; r < reps; ++r) {
      if (rebuild) {   // the position-write signal makes the list look at the positions again; the handle is told to rebuild
        pd->getPos(access::gpu, access::readwrite);
        uammd_verletlist_force_next_update(nl.handle());
      }
      sum();
    }
    (void)hipEventRecord(b, 0);
    (void)hipEventSynchronize(b);
    (void)hipEventElapsedTime(&ms[rebuild], a, b);
    ms[rebuild] /= reps;
  }
  std::printf("{\"N\": %d, \"reps\": %d, \"ms_sum_with_list_build\": %.5f, \"ms_sum_list_kept\": %.5f, \"sum_abs_force\": %.9g}\n", N, reps, ms[1],
              ms[0], sumAbsF);
  return 0;
}
