// Device side of user-written walls for Hydro::ICM_Compressible_impl<Walls> (hipcc translation units; pulled in by
// Integrator/Hydro/ICM_Compressible.cuh).  Replaces updateGhostCellsWallsD (ICM_Compressible/GhostCells.cuh:84-112) for a Walls class with
//   __device__ void applyBoundaryConditionZBottom(FluidPointers fluid, int3 ghostCell, int3 n) const;
//   __device__ void applyBoundaryConditionZTop(FluidPointers fluid, int3 ghostCell, int3 n) const;
// The library keeps no (n + 2)^3 ghost grid; it hands out the four planes a rule touches (uammd_icmc_wall_planes_get, uammd_hip.h): per
// field the bottom ghost plane, the bottom adjacent layer, the top adjacent layer and the top ghost plane, each (n.x + 2)(n.y + 2) floats
// with periodic x / y border columns.  The FluidPointers a rule receives are offset so that the reference's own index
//   x + (y + z (n.y + 2)) (n.x + 2)
// lands in those planes for z in {0, 1} at the bottom and z in {n.z, n.z + 1} at the top; any other z is out of bounds.  A rule may read
// the adjacent interior plane and write the ghost plane.  WRITES TO THE INTERIOR PLANE ARE DROPPED: only the ghost planes are copied back.
// The ghost planes arrive holding their periodic images in z, as the reference's do when its rule runs.
#pragma once
#include <cstdint>

namespace uammd {
namespace Hydro {
namespace icm_compressible {

// every (i, j) of the ghost grid, x / y border columns included, both walls; the walls object by value, as in the reference
template <class Walls>
__global__ void userWallFillD(FluidPointers bottom, FluidPointers top, Walls walls, int3 n) {
  const int id = blockIdx.x * blockDim.x + threadIdx.x;
  const int gx = n.x + 2, gy = n.y + 2;
  if (id >= gx * gy) return;
  const int i = id % gx, j = id / gx;
  walls.applyBoundaryConditionZBottom(bottom, make_int3(i, j, 0), n);
  walls.applyBoundaryConditionZTop(top, make_int3(i, j, n.z + 1), n);
}

// field f, plane k of the packed planes lies at planes + (4 f + k) P; the fields are rho, g_x, g_y, g_z, v_x, v_y, v_z
inline FluidPointers wallPlanePointers(real *planes, int3 n, bool top) {
  const std::intptr_t P = (std::intptr_t)(n.x + 2) * (n.y + 2);
  const std::intptr_t shift = top ? (2 - (std::intptr_t)n.z) * P : 0;  // z = n.z -> plane 2, z = n.z + 1 -> plane 3
  auto field = [&](int f) {
    return reinterpret_cast<real *>(reinterpret_cast<std::intptr_t>(planes) + (std::intptr_t)sizeof(real) * (4 * f * P + shift));
  };
  FluidPointers p;
  p.density = field(0);
  p.momentumX = field(1); p.momentumY = field(2); p.momentumZ = field(3);
  p.velocityX = field(4); p.velocityY = field(5); p.velocityZ = field(6);
  return p;
}

template <class Walls> void callUserWallFill(real *planes, Walls &walls, int3 n) {
  const int threads = 128, cells = (n.x + 2) * (n.y + 2);
  hipLaunchKernelGGL(userWallFillD<Walls>, dim3((cells + threads - 1) / threads), dim3(threads), 0, 0, wallPlanePointers(planes, n, false),
                     wallPlanePointers(planes, n, true), walls, n);
  uammd::detail::hipCheck(hipGetLastError(), "userWallFillD");
}

}  // namespace icm_compressible
}  // namespace Hydro
}  // namespace uammd
