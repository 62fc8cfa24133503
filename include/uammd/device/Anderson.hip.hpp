// Anderson.hip.hpp — MC_NVT::Anderson<AnyPotential> for hipcc translation units (MI355X / gfx950): the checkerboard Monte Carlo of
// Integrator/MonteCarlo/NVT/Anderson.cuh with a potential of the program's own, anything with
//   real getCutOff();   Transverser getTransverser(Interactor::Computables{false, true, false}, Box, shared_ptr<ParticleData>);
// whose Transverser::compute(...) returns an object with an `energy` member, the particle's half of the pair (Potential::Radial<Functor>
// of device/PairForces.hip.hpp is one).  A functor cannot cross the C ABI, so this is compiled with the user's code, as in the reference.
//
//   using NVT = uammd::MC_NVT::Anderson<uammd::Potential::Radial<MyFunctor>>;
//   auto mc = std::make_shared<NVT>(pd, pot, par);   mc->forwardTime();
//
// A correctness path, not a tuned one: one wave per cell of the active subgrid walks the list's cells in global memory through the
// Transverser adaptor of Transverser.hip.hpp.  Host draws, step arithmetic, counters and the deviations are those of
// Anderson<Potential::LJ> (one host side, Anderson_ns::HostSide of Anderson.cuh): with a functor that restates LJFunctor the
// positions are the same bits.
#ifndef UAMMD_MI355X_ANDERSON_HIP_HPP
#define UAMMD_MI355X_ANDERSON_HIP_HPP

#include "../Integrator/MonteCarlo/NVT/Anderson.cuh"
#include "../third_party/saruprng.cuh"
#include "ForceEnergyVirial.hpp"
#include "Transverser.hip.hpp"

#include <array>

namespace uammd {
namespace MC_NVT {
namespace Anderson_ns {

struct StepArgs {
  uammd_celllist_data list;
  real4 *pos;  // list order, unshifted
  float3 L, minusInvL, invCellSize, origin;
  int3 off, half;
  int nsub, is2D, tries;
  real beta, jump;
  uint step, seed;
  uint *tried, *accepted;
};

__device__ inline int3 cellOf(const StepArgs &a, float3 r) {  // Grid::getCell (utils/Grid.cuh:50-71)
  const float px = r.x + floorf(fmaf(r.x, a.minusInvL.x, 0.5f)) * a.L.x, py = r.y + floorf(fmaf(r.y, a.minusInvL.y, 0.5f)) * a.L.y,
              pz = r.z + floorf(fmaf(r.z, a.minusInvL.z, 0.5f)) * a.L.z;
  int3 c = make_int3((int)((px + 0.5f * a.L.x) * a.invCellSize.x), (int)((py + 0.5f * a.L.y) * a.invCellSize.y),
                     a.is2D ? 0 : (int)((pz + 0.5f * a.L.z) * a.invCellSize.z));
  if (c.x == a.list.cellDim[0]) c.x = 0;
  if (c.y == a.list.cellDim[1]) c.y = 0;
  if (c.z == a.list.cellDim[2]) c.z = 0;
  return c;
}
__device__ inline int wrapCell(int c, int n, bool periodic) { return !periodic ? c : (c < 0 ? c + n : (c >= n ? c - n : c)); }
__device__ inline real waveSum(real x) {  // fixed order: the same bits on every run
  for (int m = 32; m > 0; m >>= 1) x += __shfl_xor(x, m);
  return x;
}

template <class Transverser> __global__ void __launch_bounds__(256) stepKernel(Transverser tr, StepArgs a) {
  const int lane = threadIdx.x & 63;
  const int w = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (w >= a.nsub) return;
  const int cx = a.list.cellDim[0], cy = a.list.cellDim[1], cz = a.list.cellDim[2];
  int3 c;
  c.x = 2 * (w % a.half.x) + a.off.x;
  c.y = 2 * ((w / a.half.x) % a.half.y) + a.off.y;
  c.z = a.is2D ? 0 : 2 * (w / (a.half.x * a.half.y)) + a.off.z;
  const int icell = c.x + cx * (c.y + cy * c.z);
  const unsigned cs = a.list.d_cellStart[icell];
  if (cs < a.list.VALID_CELL) return;
  const int first = (int)(cs - a.list.VALID_CELL), nin = a.list.d_cellEnd[icell] - first;
  if (nin <= 0) return;
  const int nn = a.is2D ? 9 : 27;
  Saru rng(a.seed, a.step, icell);
  uint accepted = 0;
  for (int t = 0; t < a.tries; ++t) {
    const int i = first + min((int)(rng.f() * nin), nin - 1);
    const real4 oldPos = a.pos[i];
    const real dx = a.jump * (real(2.0) * rng.f() - real(1.0));
    const real dy = a.jump * (real(2.0) * rng.f() - real(1.0));
    const real dz = a.jump * (real(2.0) * rng.f() - real(1.0));
    const real4 newPos = make_real4(oldPos.x + dx, oldPos.y + dy, a.is2D ? oldPos.z : oldPos.z + dz, oldPos.w);
    const int3 nc = cellOf(a, make_float3(newPos.x + a.origin.x, newPos.y + a.origin.y, newPos.z + a.origin.z));
    if (nc.x != c.x || nc.y != c.y || nc.z != c.z) continue;
    const int gi = a.list.d_groupIndex[i];
    device::detail::Adaptor<Transverser> adaptor;
    adaptor.load(tr, gi);
    real eOld = 0, eNew = 0;
    for (int k = 0; k < nn; ++k) {
      const int nx = wrapCell(c.x + k % 3 - 1, cx, a.minusInvL.x != 0.0f), ny = wrapCell(c.y + (k / 3) % 3 - 1, cy, a.minusInvL.y != 0.0f),
                nz = a.is2D ? c.z : wrapCell(c.z + k / 9 - 1, cz, a.minusInvL.z != 0.0f);
      if (nx < 0 || nx >= cx || ny < 0 || ny >= cy || nz < 0 || nz >= cz) continue;
      const int jc = nx + cx * (ny + cy * nz);
      const unsigned js = a.list.d_cellStart[jc];
      if (js < a.list.VALID_CELL) continue;
      const int j0 = (int)(js - a.list.VALID_CELL), j1 = a.list.d_cellEnd[jc];
      for (int j = j0 + lane; j < j1; j += 64) {
        real4 pj = a.pos[j];
        const int gj = a.list.d_groupIndex[j];
        eOld += adaptor.compute(tr, gj, oldPos, pj).energy;
        if (j == i) pj = newPos;
        eNew += adaptor.compute(tr, gj, newPos, pj).energy;
      }
    }
    const real dH = real(2.0) * (waveSum(eNew) - waveSum(eOld));  // the whole pair energy
    const real Z = rng.f();
    const real e = expf(-a.beta * dH);
    const real p = real(1.0) < e ? real(1.0) : e;
    if (Z <= p) {
      ++accepted;
      if (lane == 0) a.pos[i] = newPos;
      __threadfence();
    }
  }
  if (lane == 0) {
    a.tried[icell] += (uint)a.tries;
    a.accepted[icell] += accepted;
  }
}

__global__ void shiftKernel(const real4 *in, real4 *out, int n, float3 o) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = make_real4(in[i].x + o.x, in[i].y + o.y, in[i].z + o.z, in[i].w);
}
__global__ void scatterKernel(const real4 *in, const int *index, real4 *out, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[index[i]] = in[i];
}
}  // namespace Anderson_ns

template <class Pot> class Anderson : public Anderson_ns::HostSide {
public:
  Anderson(shared_ptr<ParticleData> pd, shared_ptr<Pot> pot, Parameters in_par) : Anderson_ns::HostSide(pd, in_par, pot->getCutOff()), pot(pot) {
    detail::check(uammd_celllist_create(&list));
    resetCounters();
  }
  ~Anderson() { uammd_celllist_destroy(list); }
  Anderson(const Anderson &) = delete;

  void updateSimulationBox(Box newBox) {
    setGrid(newBox, pot->getCutOff());
    resetCounters();
  }

  void forwardTime() override {
    beginStep();
    const std::array<int, 8> shuffled = drawSubgridOrder();
    const int N = pd->getNumParticles();
    const int ncells = cellDim.x * cellDim.y * cellDim.z;
    float L[3];
    int per[3];
    box.toArrays(L, per);
    const int cd[3] = {cellDim.x, cellDim.y, cellDim.z};
    shifted.resize(N);
    sortPos.resize(N);
    auto tr = pot->getTransverser(Interactor::Computables{false, true, false, false}, box, pd);
    auto pos = pd->getPos(access::gpu, access::readwrite);
    const float3 o = make_float3(currentOrigin.x, currentOrigin.y, currentOrigin.z);
    const dim3 gN((N + 255) / 256), bN(256);
    hipLaunchKernelGGL(Anderson_ns::shiftKernel, gN, bN, 0, 0, (const real4 *)pos.raw(), shifted.d, N, o);
    detail::check(uammd_celllist_update(list, (const float *)shifted.d, N, L, per, cd, nullptr));
    Anderson_ns::StepArgs a;
    detail::check(uammd_celllist_get(list, &a.list));
    hipLaunchKernelGGL(Anderson_ns::shiftKernel, gN, bN, 0, 0, (const real4 *)a.list.d_sortPos, sortPos.d, N,
                       make_float3(-1.0f * o.x, -1.0f * o.y, -1.0f * o.z));
    a.pos = sortPos.d;
    a.L = make_float3(L[0], L[1], L[2]);
    a.minusInvL = make_float3(per[0] ? -1.0f / L[0] : 0.0f, per[1] ? -1.0f / L[1] : 0.0f, per[2] && L[2] != 0 ? -1.0f / L[2] : 0.0f);
    a.invCellSize = make_float3(1.0f / cellSize.x, 1.0f / cellSize.y, is2D ? 0.0f : 1.0f / cellSize.z);
    a.origin = o;
    a.half = make_int3(cellDim.x / 2, cellDim.y / 2, is2D ? 1 : cellDim.z / 2);
    a.nsub = a.half.x * a.half.y * a.half.z;
    a.is2D = is2D;
    a.tries = par.triesPerCell;
    a.beta = 1.0 / par.temperature;
    a.jump = jumpSize;
    a.step = (uint)steps;
    a.seed = (uint)seed;
    a.tried = counters.d;
    a.accepted = counters.d + ncells;
    for (int s = 0; s < numberSubGrids() && a.tries > 0; ++s) {
      const int g = shuffled[s];
      a.off = make_int3(g & 1, (g >> 1) & 1, (g >> 2) & 1);
      hipLaunchKernelGGL((Anderson_ns::stepKernel<decltype(tr)>), dim3((a.nsub + 3) / 4), dim3(256), 0, 0, tr, a);
    }
    hipLaunchKernelGGL(Anderson_ns::scatterKernel, gN, bN, 0, 0, (const real4 *)sortPos.d, a.list.d_groupIndex, pos.raw(), N);
    detail::hipCheck(hipGetLastError(), "MC_NVT::Anderson step");
    if (isTuneStep()) {
      std::vector<uint> h(2 * (size_t)ncells);
      detail::hipCheck(hipMemcpy(h.data(), counters.d, sizeof(uint) * h.size(), hipMemcpyDeviceToHost), "hipMemcpy");
      resetCounters();
      uint tried = 0, accepted = 0;
      for (int k = 0; k < ncells; ++k) { tried += h[k]; accepted += h[ncells + k]; }
      tune(tried, accepted);
    }
  }

  real sumEnergy() override {  // Anderson.cu:377-400
    currentOrigin = real3();
    const int N = pd->getNumParticles();
    float L[3];
    int per[3];
    box.toArrays(L, per);
    const int cd[3] = {cellDim.x, cellDim.y, cellDim.z};
    {
      auto pos = pd->getPos(access::gpu, access::read);
      detail::check(uammd_celllist_update(list, (const float *)pos.raw(), N, L, per, cd, nullptr));
      auto energy = pd->getEnergy(access::gpu, access::write);
      detail::check(uammd_fill_zero(energy.raw(), sizeof(real) * (size_t)N, nullptr));
    }
    auto tr = pot->getTransverser(Interactor::Computables{false, true, false, false}, box, pd);
    if (device::transverseList(list, tr, 0, nullptr) != 0) throw cuda_generic_error("MC_NVT::Anderson: traversal failed", -1);
    return 0;
  }

private:
  shared_ptr<Pot> pot;
  void resetCounters() {
    const size_t ncells = (size_t)cellDim.x * cellDim.y * cellDim.z;
    counters.resize(2 * ncells);
    detail::hipCheck(hipMemset(counters.d, 0, sizeof(uint) * 2 * ncells), "hipMemset");
  }
  uammd_celllist *list = nullptr;
  detail::DeviceArray<real4> shifted, sortPos;
  detail::DeviceArray<uint> counters;
};

}  // namespace MC_NVT
}  // namespace uammd
#endif
