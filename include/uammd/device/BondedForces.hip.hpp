// BondedForces.hip.hpp — BondedForces<BondType, N> for a USER BondType (reference: src/Interactor/BondedForces.cu:187-276): the bond
// functor is device code, compiled by hipcc with the user's translation unit as it is by nvcc in the reference
// (examples/interaction_modules/Bonds.cu `HarmonicBond`).
//
// The same layout and traversal shapes as the library's kernels for the built-in kinds (uammd_amd/csrc/bonded.hip): CSR
// rows (one per particle with bonds, ascending id), each row's entries in registration order, the members of every entry in CURRENT
// index space (memb[k][e], refreshed after ParticleData reorders), the BondInfo next to them.  Rows with at most `waveThreshold` entries
// take one lane each and sum in registration order; longer rows take one wave, the lanes' partial sums meeting in a fixed xor-shuffle
// tree.  No atomics: the same bits on every run.  compute() gets bond_index and ids[] as current indices, -1 for a fixed point.
#ifndef UAMMD_MI355X_BONDEDFORCES_HIP_HPP
#define UAMMD_MI355X_BONDEDFORCES_HIP_HPP

#include "../Interactor/BondedForces.cuh"
#include <hip/hip_runtime.h>

namespace uammd {
namespace BondedForces_ns {
constexpr int waveThreshold = 32;  // the library's default "bonded_wave_threshold"

inline __device__ void accumulate(ComputeType &acc, const ComputeType &c) {  // BondedForces.cu:236-238
  acc.force = acc.force + c.force;
  acc.virial += c.virial;
  acc.energy += c.energy;
}
inline __device__ real waveSum(real v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

template <int N, class BondType, class BondInfo>
__device__ ComputeType entry(BondType &bt, int self, int e, int stride, const int *memb, const BondInfo *info, const real4 *pos, const real4 *fp,
                             Interactor::Computables comp) {
  int ids[N];
  real3 p[N];
  for (int k = 0; k < N; ++k) {
    const int j = memb[k * stride + e];
    p[k] = make_real3(j < 0 ? fp[-j - 1] : pos[j]);
    ids[k] = j < 0 ? -1 : j;
  }
  return bt.compute(self, ids, p, comp, info[e]);
}

inline __device__ void store(int i, const ComputeType &ct, Interactor::Computables comp, real4 *force, real *energy, real *virial) {
  if (comp.force) force[i] += make_real4(ct.force);
  if (comp.energy) energy[i] += ct.energy;
  if (comp.virial) virial[i] += ct.virial;
}

template <int N, class BondType, class BondInfo>
__global__ void __launch_bounds__(256) bondsLane(BondType bt, const int *list, int n, const int *rowIndex, const int *rowStart, const int *memb,
                                                 int stride, const BondInfo *info, const real4 *pos, const real4 *fp, Interactor::Computables comp,
                                                 real4 *force, real *energy, real *virial) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  const int r = list[t], self = rowIndex[r];
  ComputeType acc{};
  for (int e = rowStart[r]; e < rowStart[r + 1]; ++e) accumulate(acc, entry<N>(bt, self, e, stride, memb, info, pos, fp, comp));
  store(self, acc, comp, force, energy, virial);
}

template <int N, class BondType, class BondInfo>
__global__ void __launch_bounds__(256) bondsWave(BondType bt, const int *list, int n, const int *rowIndex, const int *rowStart, const int *memb,
                                                 int stride, const BondInfo *info, const real4 *pos, const real4 *fp, Interactor::Computables comp,
                                                 real4 *force, real *energy, real *virial) {
  const int w = blockIdx.x * (blockDim.x / 64) + threadIdx.x / 64, lane = threadIdx.x % 64;
  if (w >= n) return;  // (a whole wave)
  const int r = list[w], self = rowIndex[r];
  ComputeType acc{};
  for (int e = rowStart[r] + lane; e < rowStart[r + 1]; e += 64) accumulate(acc, entry<N>(bt, self, e, stride, memb, info, pos, fp, comp));
  ComputeType s;
  s.force = make_real3(waveSum(acc.force.x), waveSum(acc.force.y), waveSum(acc.force.z));
  s.energy = waveSum(acc.energy);
  s.virial = waveSum(acc.virial);
  if (lane == 0) store(self, s, comp, force, energy, virial);
}

template <int N>
__global__ void bondsRefresh(const int *ids, int nentries, const int *rowId, int nrows, const int *id2index, int *memb, int *rowIndex) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t < nentries)
    for (int k = 0; k < N; ++k) {
      const int id = ids[k * nentries + t];
      memb[k * nentries + t] = id < 0 ? id : id2index[id];
    }
  if (t < nrows) rowIndex[t] = id2index[rowId[t]];
}

template <class BondType, int N> class DeviceBackend {
  using BondInfo = typename BondType::BondInfo;
  int nrows = 0, nentries = 0, nLane = 0, nWave = 0, maxId = -1;
  detail::DeviceArray<int> rowStart, rowId, rowIndex, entryIds, memb, laneRows, waveRows;
  detail::DeviceArray<BondInfo> info;
  detail::DeviceArray<real4> fixedPoints;
  template <class T> static void upload(detail::DeviceArray<T> &d, const std::vector<T> &h) {
    d.resize(h.size() ? h.size() : 1);
    if (h.size()) detail::hipCheck(hipMemcpy(d.d, h.data(), sizeof(T) * h.size(), hipMemcpyHostToDevice), "hipMemcpy");
  }
public:
  DeviceBackend(const BondSet<BondInfo, N> &set, const BondType &) {
    const int nb = (int)set.ids.size();
    std::vector<int> flat;
    for (auto &b : set.ids) flat.insert(flat.end(), b.begin(), b.end());
    int nr = 0, ne = 0;
    detail::check(uammd_bonded_build_rows(N, nb, flat.data(), &nr, &ne, nullptr, nullptr, nullptr));  // BondProcessor / buildBondList
    std::vector<int> rid(nr), rs(nr + 1), eb(ne);
    detail::check(uammd_bonded_build_rows(N, nb, flat.data(), &nr, &ne, rid.data(), rs.data(), eb.data()));
    nrows = nr;
    nentries = ne;
    maxId = nr ? rid.back() : -1;
    std::vector<int> ids((size_t)N * ne);
    std::vector<BondInfo> inf(ne);
    for (int e = 0; e < ne; ++e) {
      for (int k = 0; k < N; ++k) ids[(size_t)k * ne + e] = set.ids[eb[e]][k];
      inf[e] = set.info[eb[e]];
    }
    std::vector<int> lane, wave;
    for (int r = 0; r < nr; ++r) (rs[r + 1] - rs[r] > waveThreshold ? wave : lane).push_back(r);
    nLane = (int)lane.size();
    nWave = (int)wave.size();
    upload(rowStart, rs); upload(rowId, rid); upload(entryIds, ids); upload(info, inf); upload(laneRows, lane); upload(waveRows, wave);
    upload(fixedPoints, set.fixedPoints);
    rowIndex.resize(nr ? nr : 1);
    memb.resize(ids.size() ? ids.size() : 1);
  }
  void refresh(const int *d_id2index, int numberParticles, hipStream_t st) {
    if (maxId >= numberParticles) throw std::runtime_error("[BondedForces] a bond names a particle that does not exist");
    const int n = std::max(nrows, nentries);
    if (n == 0) return;
    hipLaunchKernelGGL((bondsRefresh<N>), dim3((n + 255) / 256), dim3(256), 0, st, entryIds.d, nentries, rowId.d, nrows, d_id2index, memb.d, rowIndex.d);
    detail::hipCheck(hipGetLastError(), "BondedForces");
  }
  void sum(BondType &bt, const real4 *pos, real4 *force, real *energy, real *virial, hipStream_t st) {
    Interactor::Computables comp;
    comp.force = force != nullptr;
    comp.energy = energy != nullptr;
    comp.virial = virial != nullptr;
    if (nLane)
      hipLaunchKernelGGL((bondsLane<N, BondType, BondInfo>), dim3((nLane + 255) / 256), dim3(256), 0, st, bt, laneRows.d, nLane, rowIndex.d, rowStart.d,
                         memb.d, nentries, info.d, pos, fixedPoints.d, comp, force, energy, virial);
    if (nWave)
      hipLaunchKernelGGL((bondsWave<N, BondType, BondInfo>), dim3((nWave + 3) / 4), dim3(256), 0, st, bt, waveRows.d, nWave, rowIndex.d, rowStart.d,
                         memb.d, nentries, info.d, pos, fixedPoints.d, comp, force, energy, virial);
    detail::hipCheck(hipGetLastError(), "BondedForces");
  }
};
}  // namespace BondedForces_ns
}  // namespace uammd
#endif
