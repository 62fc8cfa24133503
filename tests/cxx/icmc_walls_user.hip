// User-written walls for Hydro::ICM_Compressible_impl<Walls> (hipcc; device/ICM_Compressible.hip.hpp): Walls classes with the reference's
// applyBoundaryConditionZBottom / ZTop, written with the reference's index arithmetic on FluidPointers.  A 9 x 6 x 5 grid of unit cells,
// no particles.  Arguments: steps (default 20), output file.
//   (a) the rule of test/Hydro/ICM_Compressible/walltest.cu (an oscillating bottom wall, the top wall at rest) as a user class against the
//       same walls as icm_compressible::MovingWalls: prints "icmcu same <0|1>" — every value of rho, v and g has the same bits;
//   (b) a free-slip rule (tangential v_ghost = +v_adj, normal reflected): writes to the output file, as raw floats, the initial rho, v_x,
//       v_y, v_z and the final rho, v_x, v_y, v_z, g_x, g_y, g_z (staggered, n.x n.y n.z each) for tests/test_gpu_icm_compressible_walls.py
//       to compare with the restatement under the same rule.
#include "Integrator/Hydro/ICM_Compressible.cuh"
#include "uammd.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace uammd;
using FluidPointers = Hydro::icm_compressible::FluidPointers;

static real bottomVelocity(real t) { return real(0.04 * std::cos(2.0 * (double)t)); }

// walltest.cu's ICMWalls, every component written as 2 u - v (u = 0 where that wall does not move)
class UserWalls : public ParameterUpdatable {
  real bottomWallvx = bottomVelocity(0);

public:
  __host__ __device__ bool isEnabled() { return true; }

  __device__ void applyBoundaryConditionZBottom(FluidPointers fluid, int3 ghostCell, int3 n) const {
    const int ighost = ghostCell.x + (ghostCell.y + ghostCell.z * (n.y + 2)) * (n.x + 2);
    const int ighostZp1 = ghostCell.x + (ghostCell.y + (ghostCell.z + 1) * (n.y + 2)) * (n.x + 2);
    const real rho = fluid.density[ighostZp1];
    fluid.density[ighost] = rho;
    fluid.velocityX[ighost] = 2 * bottomWallvx - fluid.velocityX[ighostZp1];
    fluid.velocityY[ighost] = 2 * real(0) - fluid.velocityY[ighostZp1];
    fluid.velocityZ[ighost] = 2 * real(0) - fluid.velocityZ[ighostZp1];
    fluid.momentumX[ighost] = 2 * bottomWallvx * rho - fluid.momentumX[ighostZp1];
    fluid.momentumY[ighost] = 2 * real(0) * rho - fluid.momentumY[ighostZp1];
    fluid.momentumZ[ighost] = 2 * real(0) * rho - fluid.momentumZ[ighostZp1];
    fluid.density[ighostZp1] = -1;  // a write to the interior plane: dropped
  }

  __device__ void applyBoundaryConditionZTop(FluidPointers fluid, int3 ghostCell, int3 n) const {
    const int ighost = ghostCell.x + (ghostCell.y + ghostCell.z * (n.y + 2)) * (n.x + 2);
    const int ighostZm1 = ghostCell.x + (ghostCell.y + (ghostCell.z - 1) * (n.y + 2)) * (n.x + 2);
    const real rho = fluid.density[ighostZm1];
    fluid.density[ighost] = rho;
    fluid.velocityX[ighost] = 2 * real(0) - fluid.velocityX[ighostZm1];
    fluid.velocityY[ighost] = 2 * real(0) - fluid.velocityY[ighostZm1];
    fluid.velocityZ[ighost] = 2 * real(0) - fluid.velocityZ[ighostZm1];
    fluid.momentumX[ighost] = 2 * real(0) * rho - fluid.momentumX[ighostZm1];
    fluid.momentumY[ighost] = 2 * real(0) * rho - fluid.momentumY[ighostZm1];
    fluid.momentumZ[ighost] = 2 * real(0) * rho - fluid.momentumZ[ighostZm1];
  }

  void updateSimulationTime(real t) override { bottomWallvx = bottomVelocity(t); }
};

struct BuiltinWalls : public Hydro::icm_compressible::MovingWalls {
  BuiltinWalls() : MovingWalls(make_real2(bottomVelocity(0), 0), make_real2(0, 0)) {}
  void updateSimulationTime(real t) override { setVelocities(make_real2(bottomVelocity(t), 0), make_real2(0, 0)); }
};

// free slip: the tangential velocity continued evenly, the normal one reflected
class FreeSlip : public ParameterUpdatable {
  __device__ static void apply(FluidPointers fluid, int ighost, int iadj) {
    fluid.density[ighost] = fluid.density[iadj];
    fluid.velocityX[ighost] = fluid.velocityX[iadj];
    fluid.velocityY[ighost] = fluid.velocityY[iadj];
    fluid.velocityZ[ighost] = -fluid.velocityZ[iadj];
    fluid.momentumX[ighost] = fluid.momentumX[iadj];
    fluid.momentumY[ighost] = fluid.momentumY[iadj];
    fluid.momentumZ[ighost] = -fluid.momentumZ[iadj];
  }

public:
  static constexpr bool isEnabled() { return true; }
  __device__ void applyBoundaryConditionZBottom(FluidPointers fluid, int3 c, int3 n) const {
    apply(fluid, c.x + (c.y + c.z * (n.y + 2)) * (n.x + 2), c.x + (c.y + (c.z + 1) * (n.y + 2)) * (n.x + 2));
  }
  __device__ void applyBoundaryConditionZTop(FluidPointers fluid, int3 c, int3 n) const {
    apply(fluid, c.x + (c.y + c.z * (n.y + 2)) * (n.x + 2), c.x + (c.y + (c.z - 1) * (n.y + 2)) * (n.x + 2));
  }
};

static std::vector<real> toHost(const real *d, size_t n) {
  std::vector<real> h(n);
  if (hipMemcpy(h.data(), d, sizeof(real) * n, hipMemcpyDeviceToHost) != hipSuccess) std::exit(3);
  return h;
}

// rho, v_x, v_y, v_z (staggered) and, with momentum, g_x, g_y, g_z appended to out
template <class ICM> static void fields(ICM &icm, bool momentum, std::vector<real> &out) {
  const int3 n = icm.getGridSize();
  const size_t nc = (size_t)n.x * n.y * n.z;
  auto density = icm.getCurrentDensity();
  auto v = icm.getCurrentStaggeredVelocity();
  auto g = icm.getCurrentMomentum();
  const real *src[7] = {density.data().get(), v.x(), v.y(), v.z(), g.x(), g.y(), g.z()};
  for (int f = 0; f < (momentum ? 7 : 4); ++f) {
    const std::vector<real> a = toHost(src[f], nc);
    out.insert(out.end(), a.begin(), a.end());
  }
}

template <class Walls> static std::vector<real> run(std::shared_ptr<ParticleData> pd, int steps, std::vector<real> *initial) {
  using ICM = Hydro::ICM_Compressible_impl<Walls>;
  typename ICM::Parameters par;
  par.shearViscosity = 1.3;
  par.bulkViscosity = 0.7;
  par.speedOfSound = 4;
  par.dt = 0.05;
  par.boxSize = make_real3(9, 6, 5);
  par.cellDim = make_int3(9, 6, 5);
  par.seed = 77;
  par.initialDensity = [](real3 r) { return real(1 + 0.05 * std::sin(2 * M_PI * (double)r.x / 9) * std::cos(0.7 * (double)r.z)); };
  par.initialVelocityX = [](real3 r) { return real(0.05 * std::sin(2 * M_PI * (double)r.y / 6) * std::cos(0.5 * (double)r.z)); };
  par.initialVelocityY = [](real3 r) { return real(0.03 * std::cos(2 * M_PI * (double)r.x / 9 + 0.4) * std::sin(0.6 * (double)r.z + 0.4)); };
  par.initialVelocityZ = [](real3 r) { return real(0.02 * std::cos(2 * M_PI * (double)r.x / 9) * std::cos(0.4 * (double)r.z - 0.4)); };
  par.walls = std::make_shared<Walls>();
  ICM icm(pd, par);
  if (initial) fields(icm, false, *initial);
  for (int s = 0; s < steps; ++s) icm.forwardTime();
  std::vector<real> out;
  fields(icm, true, out);
  return out;
}

int main(int argc, char *argv[]) {
  const int steps = argc > 1 ? std::atoi(argv[1]) : 20;
  auto sys = std::make_shared<System>();
  auto pd = std::make_shared<ParticleData>(0, sys);
  const std::vector<real> builtin = run<BuiltinWalls>(pd, steps, nullptr);
  const std::vector<real> user = run<UserWalls>(pd, steps, nullptr);
  const bool same = builtin.size() == user.size() && std::memcmp(builtin.data(), user.data(), sizeof(real) * user.size()) == 0;
  double moved = 0;
  for (size_t i = 270; i < 2 * 270 && i < user.size(); ++i) moved = std::fmax(moved, std::fabs((double)user[i]));
  std::printf("icmcu same %d values %zu max|v_x| %.6g\n", (int)same, user.size(), moved);
  std::vector<real> all;
  const std::vector<real> slip = run<FreeSlip>(pd, steps, &all);
  all.insert(all.end(), slip.begin(), slip.end());
  if (argc > 2) {
    FILE *f = std::fopen(argv[2], "wb");
    if (!f || std::fwrite(all.data(), sizeof(real), all.size(), f) != all.size()) { std::printf("icmcu: cannot write %s\n", argv[2]); return 2; }
    std::fclose(f);
  }
  std::printf("icmcu freeslip values %zu\n", all.size());
  return same ? 0 : 1;
}
