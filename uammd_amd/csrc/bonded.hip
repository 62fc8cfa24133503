// BondedForces / AngularBondedForces / TorsionalBondedForces (reference: src/Interactor/BondedForces.{cuh,cu},
// AngularBondedForces.cuh, TorsionalBondedForces.cuh): bonds of 2, 3 or 4 particles with the built-in kinds Harmonic, FENE (plus
// fixed-point bonds), Angular, Torsional and FourierLAMMPS.
//
// Ownership is the reference's: every particle that has bonds sums, in registration order, the contribution of each bond it belongs to
// and adds it to its own force / energy / virial.  No atomics; the result is the same bits on every run.
//
// Storage: CSR, one row per particle with bonds (rows in ascending id, as the reference's std::set), the row's entries
// are the bonds it is a member of in registration order (BondProcessor::registerBond, BondedForces.cu:43-57).  The entries are SoA: the
// current index of each member (memb[k][e], refreshed from the ids when ParticleData reorders), then the BondInfo (float2).  Fixed points
// are real4 rows, taken when a member index is negative (-(j+1) -> fixedPoints[j]).
//
// Two traversal shapes, chosen per row from its length when the set is uploaded:
//   lane per row  — rows with at most `threshold` entries (chains: 1-4 entries), summed in registration order;
//   wave per row  — longer rows: the 64 lanes of a wave stride the row, the partial sums meet in a fixed DPP tree (wave_sum_to_last).
// The reference-shaped baseline (thread per row, AoS entries, id2index looked up on every step, BondedForces.cu:191-243) stays
// selectable through uammd_hip_set_tunable("bonded_baseline", 1) for measurement.
#include "celllist.hpp"

#include <algorithm>
#include <atomic>
#include <cstring>
#include <vector>

namespace uammd_hip {

namespace bonded {

std::atomic<int> g_baseline{0};
std::atomic<int> g_waveThreshold{32};  // entries per row above which a row takes the wave shape (measured)

struct V3 { float x, y, z; };
UH_D V3 v3(float4 p) { return {p.x, p.y, p.z}; }
UH_D V3 operator+(V3 a, V3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
UH_D V3 operator-(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
UH_D V3 operator*(float s, V3 a) { return {s * a.x, s * a.y, s * a.z}; }
UH_D V3 operator*(V3 a, float s) { return {a.x * s, a.y * s, a.z * s}; }
// utils/vector.cuh of the reference: dot and cross as written there (no contraction: the library builds with -ffp-contract=off)
UH_D float dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
UH_D V3 cross(V3 a, V3 b) { return {a.y * b.z - a.z * b.y, (-a.x * b.z + a.z * b.x), a.x * b.y - a.y * b.x}; }
UH_D V3 pbc(const BoxT<float> &box, V3 r) {
  const vec3<float> q = box.apply_pbc(vec3<float>{r.x, r.y, r.z});
  return {q.x, q.y, q.z};
}

struct Comp { bool force, energy, virial; };
struct CT { V3 force; float virial, energy; };  // ComputeType, BondedForces.cuh:46-50
UH_D CT zero_ct() { return CT{{0.f, 0.f, 0.f}, 0.f, 0.f}; }

enum Kind { HARMONIC = 0, FENE = 1, ANGULAR = 2, TORSIONAL = 3, FOURIER = 4 };
template <int K> struct Members { static constexpr int value = K <= FENE ? 2 : (K == ANGULAR ? 3 : 4); };

// ---- the kinds: the reference's arithmetic, line for line ----------------------------------------------------------------------
// Harmonic: BondedForces.cuh:57-78 (harmonicBond) and :98-107 (Harmonic::compute). BondInfo {k, r0}.
// FENE:     BondedForces.cuh:119-138 (feneBond) and :149-158 (FENE::compute).      BondInfo {r0, k}.
template <int K> UH_D CT compute_pair(int self, const int *ids, const V3 *pos, Comp comp, float2 bi, const BoxT<float> &box) {
  V3 ri = pos[0], rj = pos[1];
  if (self == ids[0]) { const V3 t = ri; ri = rj; rj = t; }
  const V3 r12 = pbc(box, rj - ri);
  const float r2 = dot(r12, r12);
  CT ct;
  if (K == HARMONIC) {
    const float k = bi.x, r0 = bi.y;
    const float invr = rsqrtf(r2);
    const float f = -k * (1.0f - r0 * invr);
    ct.force = f * r12;
    const float d = 1.0f / invr - r0;
    ct.energy = comp.energy ? (0.25f * k * (d * d)) : 0.0f;
    ct.virial = comp.virial ? dot(ct.force, r12) : 0.0f;
  } else {
    const float r0 = bi.x, k = bi.y, r02 = r0 * r0;
    const float f = -r02 * k / (r02 - r2);
    ct.force = f * r12;
    ct.energy = comp.energy ? (-0.25f * k * r02 * logf(1.0f - r2 / r02)) : 0.0f;
    ct.virial = comp.virial ? dot(ct.force, r12) : 0.0f;
  }
  return (r2 == 0.0f) ? zero_ct() : ct;
}

// Angular: AngularBondedForces.cuh:66-127.  BondInfo {ang0, k}.  No energy, no virial (the reference leaves them 0).
UH_D CT compute_angular(int self, const int *ids, const V3 *pos, Comp, float2 bi, const BoxT<float> &box) {
  const float ang0 = bi.x, kspring = bi.y;
  const V3 rij = pbc(box, pos[1] - pos[0]);
  const float rij2 = dot(rij, rij);
  const float invsqrij = rsqrtf(rij2);
  const V3 rjk = pbc(box, pos[2] - pos[1]);
  const float rjk2 = dot(rjk, rjk);
  const float invsqrjk = rsqrtf(rjk2);
  const float a2 = invsqrij * invsqrjk;
  float cijk = dot(rij, rjk) * a2;
  if (cijk > 1.0f) cijk = 1.0f;
  else if (cijk < -1.0f) cijk = -1.0f;
  float ampli;
  CT ct = zero_ct();
  if (ang0 == 0.0f) {
    ampli = -2.0f * kspring;
  } else {
    const float theta = acosf(cijk);
    if (theta == 0.0f) return zero_ct();
    const float sinthetao2 = sinf(0.5f * theta);
    ampli = -2.0f * kspring * (sinthetao2 - sinf(ang0 * 0.5f)) / sinthetao2;
  }
  const float a11 = ampli * cijk / rij2;
  const float a12 = ampli * a2;
  const float a22 = ampli * cijk / rjk2;
  if (self == ids[0]) ct.force = a12 * rjk - a11 * rij;
  else if (self == ids[1]) ct.force = -1.0f * ((-a11 - a12) * rij + (a12 + a22) * rjk);
  else if (self == ids[2]) ct.force = -1.0f * (a12 * rij - a22 * rjk);
  return ct;
}

// Torsional: TorsionalBondedForces.cuh:60-108.  BondInfo {phi0, k}.  Force only.  DELIBERATE DEVIATION: the reference
// compares the particle against ids[1], ids[2], ids[3] and then the out-of-bounds ids[4], so member 0 gets the force meant for member 1
// and so on and the net force of a bond is not zero; here members 0..3 get -fj, fm+fj-fk, fn+fk-fm, -fn (the intended mapping).
UH_D CT compute_torsional(int self, const int *ids, const V3 *pos, Comp, float2 bi, const BoxT<float> &box) {
  const float phi0 = bi.x, k = bi.y;
  const V3 rjk = pbc(box, pos[1] - pos[0]);
  const V3 rkm = pbc(box, pos[2] - pos[1]);
  const V3 rmn = pbc(box, pos[3] - pos[2]);
  V3 njkm = cross(rjk, rkm);
  V3 nkmn = cross(rkm, rmn);
  const float n2 = dot(njkm, njkm);
  const float nn2 = dot(nkmn, nkmn);
  if (n2 > 0 && nn2 > 0) {
    const float invn = rsqrtf(n2);
    const float invnn = rsqrtf(nn2);
    const float cosphi = dot(njkm, nkmn) * invn * invnn;
    float Fmod = 0;
    const float phi = acosf(cosphi);
    if (cosphi * cosphi <= 1 && phi * phi > 0) Fmod = -k * (phi - phi0) / sinf(phi);
    njkm = njkm * invn;
    nkmn = nkmn * invnn;
    CT ct = zero_ct();
    const V3 v1 = (nkmn - cosphi * njkm) * invn;
    const V3 fj = Fmod * cross(v1, rkm);
    if (self == ids[0]) { ct.force = -1.0f * fj; return ct; }
    const V3 v2 = (njkm - cosphi * nkmn) * invnn;
    const V3 fk = Fmod * cross(v2, rmn);
    const V3 fm = Fmod * cross(v1, rjk);
    if (self == ids[1]) { ct.force = fm + fj - fk; return ct; }
    const V3 fn = Fmod * cross(v2, rkm);
    if (self == ids[2]) { ct.force = fn + fk - fm; return ct; }
    if (self == ids[3]) { ct.force = -1.0f * fn; return ct; }
  }
  return zero_ct();
}

// FourierLAMMPS: TorsionalBondedForces.cuh:121-207 (compute, signOfPhi).  BondInfo {phi0, kdih}.  U = kdih (1 + cos(phi - phi0)), a
// quarter per member; the virial per member as written there.
UH_D float sign_of_phi(V3 r12, V3 r23, V3 r34) {
  const V3 ru23 = r23 * rsqrtf(dot(r23, r23));
  const V3 uloc1 = r12 * rsqrtf(dot(r12, r12));
  const V3 uloc2 = ru23 - dot(uloc1, ru23) * uloc1;
  const V3 uloc3 = cross(uloc1, uloc2);
  return (dot(r34, uloc3) < 0) ? -1.0f : 1.0f;
}
UH_D CT compute_fourier(int self, const int *ids, const V3 *pos, Comp comp, float2 bi, const BoxT<float> &box) {
  const float phi0 = bi.x, kdih = bi.y;
  const V3 r12 = pbc(box, pos[1] - pos[0]);
  const V3 r23 = pbc(box, pos[2] - pos[1]);
  const V3 r34 = pbc(box, pos[3] - pos[2]);
  const V3 v123 = cross(r12, r23);
  const V3 v234 = cross(r23, r34);
  const float v123q = dot(v123, v123);
  const float v234q = dot(v234, v234);
  CT ct = zero_ct();
  if (v123q < 1e-15f || v234q < 1e-15f) return ct;
  if (comp.energy) {
    const float cosPhi = fmaxf(-1.0f, fminf(1.0f, dot(v123, v234) * rsqrtf(v123q) * rsqrtf(v234q)));
    const float dphi = sign_of_phi(r12, r23, r34) * acosf(cosPhi) - phi0;
    ct.energy = 0.25f * kdih * (1 + cosf(dphi));
  }
  if (!comp.force && !comp.virial) return ct;
  const float invsqv123 = rsqrtf(v123q);
  const float invsqv234 = rsqrtf(v234q);
  const float cosPhi = fmaxf(-1.0f, fminf(1.0f, dot(v123, v234) * invsqv123 * invsqv234));
  const float phi = sign_of_phi(r12, r23, r34) * acosf(cosPhi);
  if (fabsf(phi) < 1e-10f || float(M_PI) - fabsf(phi) < 1e-10f) return ct;
  const float pref = -kdih * sinf(phi - phi0) / sinf(phi);
  const V3 vu234 = v234 * invsqv234;
  const V3 vu123 = v123 * invsqv123;
  const V3 w1 = (vu234 - cosPhi * vu123) * invsqv123;
  const V3 w2 = (vu123 - cosPhi * vu234) * invsqv234;
  if (self == ids[0]) {
    ct.force = pref * cross(w1, r23);
    ct.virial = comp.virial ? dot(ct.force, r23) : 0;
  } else if (self == ids[1]) {
    const V3 r13 = pbc(box, pos[2] - pos[0]);
    const V3 c34 = cross(w2, r34);
    const V3 c13 = cross(w1, r13);
    ct.force = pref * (c34 - c13);
    ct.virial = comp.virial ? (dot(pref * c34, r34) - dot(pref * c13, r13)) : 0;
  } else if (self == ids[2]) {
    const V3 r24 = pbc(box, pos[3] - pos[1]);
    const V3 c12 = cross(w1, r12);
    const V3 c24 = cross(w2, r24);
    ct.force = pref * (c12 - c24);
    ct.virial = comp.virial ? (dot(pref * c12, r12) - dot(pref * c24, r24)) : 0;
  } else if (self == ids[3]) {
    ct.force = pref * cross(w2, r23);
    ct.virial = comp.virial ? dot(ct.force, r23) : 0;
  }
  return ct;
}

template <int K> UH_D CT compute(int self, const int *ids, const V3 *pos, Comp comp, float2 bi, const BoxT<float> &box) {
  if (K == HARMONIC || K == FENE) return compute_pair<K>(self, ids, pos, comp, bi, box);
  if (K == ANGULAR) return compute_angular(self, ids, pos, comp, bi, box);
  if (K == TORSIONAL) return compute_torsional(self, ids, pos, comp, bi, box);
  return compute_fourier(self, ids, pos, comp, bi, box);
}

UH_D void accumulate(CT &acc, const CT &c) {  // BondedForces.cu:236-238: force, virial, energy
  acc.force = acc.force + c.force;
  acc.virial += c.virial;
  acc.energy += c.energy;
}

struct Outputs { float4 *force; float *energy, *virial; };

UH_D void store(const Outputs &o, Comp comp, int i, const CT &ct) {  // BondedForces.cu:240-245
  if (comp.force) {
    float4 f = o.force[i];
    f.x += ct.force.x; f.y += ct.force.y; f.z += ct.force.z;
    o.force[i] = f;
  }
  if (comp.energy) o.energy[i] += ct.energy;
  if (comp.virial) o.virial[i] += ct.virial;
}

// the entries in current-index space: memb[k * stride + e] (negative: fixed point -(j+1)), info[e]
struct Rows {
  const int *rowIndex, *rowStart, *memb;
  const float2 *info;
  const float4 *fixedPoints;
  int stride;
};

template <int K> UH_D CT entry(const Rows &R, int e, int self, const float4 *__restrict__ pos, Comp comp, const BoxT<float> &box) {
  constexpr int NP = Members<K>::value;
  int ids[NP];
  V3 p[NP];
#pragma unroll
  for (int k = 0; k < NP; ++k) ids[k] = R.memb[k * R.stride + e];
  const float2 bi = R.info[e];
#pragma unroll
  for (int k = 0; k < NP; ++k) {
    const int j = ids[k];
    p[k] = v3(j < 0 ? R.fixedPoints[-j - 1] : pos[j]);
    ids[k] = j < 0 ? -1 : j;  // (the reference hands -1 for a fixed point, BondedForces.cu:225-229)
  }
  return compute<K>(self, ids, p, comp, bi, box);
}

// lane per row: each lane walks its row in registration order
template <int K>
__global__ void __launch_bounds__(256) k_lane(Rows R, const int *__restrict__ list, int n, const float4 *__restrict__ pos, Comp comp,
                                              BoxT<float> box, Outputs o) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  const int r = list[t];
  const int self = R.rowIndex[r];
  const int first = R.rowStart[r], last = R.rowStart[r + 1];
  CT acc = zero_ct();
  for (int e = first; e < last; ++e) accumulate(acc, entry<K>(R, e, self, pos, comp, box));
  store(o, comp, self, acc);
}

// wave per row: lane l takes entries first + l, first + l + 64, ...; the partial sums meet in wave_sum_to_last (fixed DPP order)
template <int K>
__global__ void __launch_bounds__(256) k_wave(Rows R, const int *__restrict__ list, int n, const float4 *__restrict__ pos, Comp comp,
                                              BoxT<float> box, Outputs o) {
  const int w = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (w >= n) return;  // (whole waves leave together: the DPP tree below runs with all 64 lanes)
  const int r = list[w];
  const int self = R.rowIndex[r];
  const int first = R.rowStart[r], last = R.rowStart[r + 1];
  CT acc = zero_ct();
  for (int e = first + lane; e < last; e += 64) accumulate(acc, entry<K>(R, e, self, pos, comp, box));
  CT s;
  s.force.x = comp.force ? wave_sum_to_last(acc.force.x) : 0.f;
  s.force.y = comp.force ? wave_sum_to_last(acc.force.y) : 0.f;
  s.force.z = comp.force ? wave_sum_to_last(acc.force.z) : 0.f;
  s.energy = comp.energy ? wave_sum_to_last(acc.energy) : 0.f;
  s.virial = comp.virial ? wave_sum_to_last(acc.virial) : 0.f;
  if (lane == 63) store(o, comp, self, s);
}

// the reference's shape: thread per row, AoS entries in id space, id2index looked up on every step (BondedForces.cu:191-246)
template <int NP> struct __align__(16) AosBond { int ids[NP]; float2 info; };

template <int K>
__global__ void __launch_bounds__(128) k_baseline(const AosBond<Members<K>::value> *__restrict__ bonds, const int *__restrict__ rowStart,
                                                  const int *__restrict__ rowId, const int *__restrict__ id2index, const float4 *fixedPoints,
                                                  int n, const float4 *__restrict__ pos, Comp comp, BoxT<float> box, Outputs o) {
  constexpr int NP = Members<K>::value;
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  const int self = id2index[rowId[t]];
  CT acc = zero_ct();
  for (int b = rowStart[t]; b < rowStart[t + 1]; ++b) {
    const AosBond<NP> bond = bonds[b];
    int ids[NP];
    V3 p[NP];
#pragma unroll
    for (int k = 0; k < NP; ++k) {
      const int j = bond.ids[k];
      ids[k] = j < 0 ? -1 : id2index[j];
      p[k] = v3(j < 0 ? fixedPoints[-j - 1] : pos[ids[k]]);
    }
    accumulate(acc, compute<K>(self, ids, p, comp, bond.info, box));
  }
  store(o, comp, self, acc);
}

// ids (id space, AoS) -> current indices (SoA), and each row's own index
template <int NP>
__global__ void __launch_bounds__(256) k_refresh(const AosBond<NP> *__restrict__ bonds, int nentries, const int *__restrict__ rowId, int nrows,
                                                 const int *__restrict__ id2index, int *memb, int *rowIndex) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t < nentries) {
    const AosBond<NP> b = bonds[t];
#pragma unroll
    for (int k = 0; k < NP; ++k) memb[k * nentries + t] = b.ids[k] < 0 ? b.ids[k] : id2index[b.ids[k]];
  }
  if (t < nrows) rowIndex[t] = id2index[rowId[t]];
}

int members_of(int kind) { return kind <= FENE ? 2 : (kind == ANGULAR ? 3 : 4); }

// BondProcessor + buildBondList (BondedForces.cu:35-74, :109-137): rows = the particles with bonds in ascending id (std::set), each row the
// bonds it is a member of in registration order.  Negative ids (fixed points) register nothing.
void build_rows(int ppb, int nbonds, const int *ids, std::vector<int> &rowId, std::vector<int> &rowStart, std::vector<int> &entryBond) {
  int maxId = -1;
  for (long i = 0; i < (long)nbonds * ppb; ++i) maxId = std::max(maxId, ids[i]);
  std::vector<int> count(maxId + 1, 0);
  for (long i = 0; i < (long)nbonds * ppb; ++i)
    if (ids[i] >= 0) count[ids[i]]++;
  rowId.clear();
  rowStart.assign(1, 0);
  std::vector<int> slot(maxId + 1, -1);
  for (int p = 0; p <= maxId; ++p)
    if (count[p]) {
      slot[p] = rowStart.back();
      rowId.push_back(p);
      rowStart.push_back(rowStart.back() + count[p]);
    }
  entryBond.assign(rowStart.back(), 0);
  for (int b = 0; b < nbonds; ++b)
    for (int k = 0; k < ppb; ++k) {
      const int id = ids[(long)b * ppb + k];
      if (id >= 0) entryBond[slot[id]++] = b;
    }
}

struct Handle {
  int kind = -1, ppb = 0, nbonds = 0, nrows = 0, nentries = 0, nfixed = 0, maxId = -1;
  BoxT<float> box;
  std::vector<int> rowLength;                 // host: entries per row (for the shape split)
  int threshold = -1, nLane = 0, nWave = 0;   // the split in force
  bool refreshed = false;
  DeviceBuffer aos, rowStart, rowId, fixedPoints, memb, info, rowIndex, laneRows, waveRows, id2index;
};

template <int NP> int upload_aos(Handle &h, const int *ids, const float *info, const std::vector<int> &entryBond) {
  std::vector<AosBond<NP>> a(h.nentries);
  std::vector<float2> inf(h.nentries);
  for (int e = 0; e < h.nentries; ++e) {
    const int b = entryBond[e];
    for (int k = 0; k < NP; ++k) a[e].ids[k] = ids[(long)b * NP + k];
    a[e].info = make_float2(info[2l * b], info[2l * b + 1]);
    inf[e] = a[e].info;
  }
  if (h.nentries == 0) return 0;
  if (h.aos.reserve(sizeof(AosBond<NP>) * h.nentries) || h.info.reserve(sizeof(float2) * h.nentries) ||
      h.memb.reserve(sizeof(int) * NP * (size_t)h.nentries))
    return -1;
  UH_CHECK(hipMemcpy(h.aos.ptr, a.data(), sizeof(AosBond<NP>) * h.nentries, hipMemcpyHostToDevice));
  UH_CHECK(hipMemcpy(h.info.ptr, inf.data(), sizeof(float2) * h.nentries, hipMemcpyHostToDevice));
  return 0;
}

int split_rows(Handle &h) {
  const int T = g_waveThreshold.load();
  if (T == h.threshold) return 0;
  std::vector<int> lane, wave;
  for (int r = 0; r < h.nrows; ++r) (h.rowLength[r] > T ? wave : lane).push_back(r);
  h.nLane = (int)lane.size();
  h.nWave = (int)wave.size();
  if (h.laneRows.reserve(sizeof(int) * (lane.size() + 1)) || h.waveRows.reserve(sizeof(int) * (wave.size() + 1))) return -1;
  if (!lane.empty()) UH_CHECK(hipMemcpy(h.laneRows.ptr, lane.data(), sizeof(int) * lane.size(), hipMemcpyHostToDevice));
  if (!wave.empty()) UH_CHECK(hipMemcpy(h.waveRows.ptr, wave.data(), sizeof(int) * wave.size(), hipMemcpyHostToDevice));
  h.threshold = T;
  return 0;
}

template <int K> int launch_sum(Handle &h, const float4 *pos, Outputs o, Comp comp, hipStream_t st) {
  constexpr int NP = Members<K>::value;
  const float4 *fp = reinterpret_cast<const float4 *>(h.fixedPoints.ptr);
  if (g_baseline.load()) {
    hipLaunchKernelGGL(k_baseline<K>, dim3((h.nrows + 127) / 128), dim3(128), 0, st, reinterpret_cast<const AosBond<NP> *>(h.aos.ptr),
                       (const int *)h.rowStart.ptr, (const int *)h.rowId.ptr, (const int *)h.id2index.ptr, fp, h.nrows, pos, comp, h.box, o);
    UH_CHECK(hipGetLastError());
    return 0;
  }
  if (split_rows(h)) return -1;
  Rows R{(const int *)h.rowIndex.ptr, (const int *)h.rowStart.ptr, (const int *)h.memb.ptr, (const float2 *)h.info.ptr, fp, h.nentries};
  if (h.nLane)
    hipLaunchKernelGGL(k_lane<K>, dim3((h.nLane + 255) / 256), dim3(256), 0, st, R, (const int *)h.laneRows.ptr, h.nLane, pos, comp, h.box, o);
  if (h.nWave)
    hipLaunchKernelGGL(k_wave<K>, dim3((h.nWave + 3) / 4), dim3(256), 0, st, R, (const int *)h.waveRows.ptr, h.nWave, pos, comp, h.box, o);
  UH_CHECK(hipGetLastError());
  return 0;
}

}  // namespace bonded

// uammd_hip_set_tunable's bonded switches (lj.hip): 0 = handled
int bonded_set_tunable(const char *name, int value) {
  if (!std::strcmp(name, "bonded_baseline") && (value == 0 || value == 1)) { bonded::g_baseline = value; return 0; }
  if (!std::strcmp(name, "bonded_wave_threshold") && value >= 0) { bonded::g_waveThreshold = value; return 0; }
  return -1;
}

}  // namespace uammd_hip

using namespace uammd_hip;
using namespace uammd_hip::bonded;

extern "C" {

int uammd_bonded_create(uammd_bonded **out) {
  if (!out) { set_last_error("uammd_bonded_create: null argument"); return -1; }
  *out = reinterpret_cast<uammd_bonded *>(new Handle());
  return 0;
}

int uammd_bonded_destroy(uammd_bonded *h) {
  delete reinterpret_cast<Handle *>(h);
  return 0;
}

int uammd_bonded_build_rows(int particlesPerBond, int nbonds, const int *ids, int *nrows, int *nentries, int *rowId, int *rowStart,
                            int *entryBond) {
  if (particlesPerBond < 2 || particlesPerBond > 4 || nbonds < 0 || (nbonds > 0 && !ids) || !nrows || !nentries) {
    set_last_error("uammd_bonded_build_rows: bad arguments");
    return -1;
  }
  std::vector<int> rid, rs, eb;
  build_rows(particlesPerBond, nbonds, ids, rid, rs, eb);
  *nrows = (int)rid.size();
  *nentries = (int)eb.size();
  if (rowId) std::copy(rid.begin(), rid.end(), rowId);
  if (rowStart) std::copy(rs.begin(), rs.end(), rowStart);
  if (entryBond) std::copy(eb.begin(), eb.end(), entryBond);
  return 0;
}

int uammd_bonded_upload(uammd_bonded *hh, int kind, int nbonds, const int *ids, const float *info, int nfixed, const float *fixedPoints,
                        const float L[3], const int periodic[3]) {
  Handle *h = reinterpret_cast<Handle *>(hh);
  if (!h || kind < HARMONIC || kind > FOURIER || nbonds < 0 || nfixed < 0 || (nbonds > 0 && (!ids || !info)) || (nfixed > 0 && !fixedPoints) ||
      !L || !periodic) {
    set_last_error("uammd_bonded_upload: bad arguments");
    return -1;
  }
  const int ppb = members_of(kind);
  for (long i = 0; i < (long)nbonds * ppb; ++i) {
    const int id = ids[i];
    if (id < -nfixed || (id < 0 && ppb != 2)) {
      set_last_error("uammd_bonded_upload: bond %ld refers to fixed point %d, there are %d", i / ppb, -id - 1, nfixed);
      return -1;
    }
  }
  std::vector<int> rid, rs, eb;
  build_rows(ppb, nbonds, ids, rid, rs, eb);
  h->kind = kind;
  h->ppb = ppb;
  h->nbonds = nbonds;
  h->nfixed = nfixed;
  h->nrows = (int)rid.size();
  h->nentries = (int)eb.size();
  h->maxId = rid.empty() ? -1 : rid.back();
  h->box = make_box<float>(L, periodic);
  h->rowLength.resize(h->nrows);
  for (int r = 0; r < h->nrows; ++r) h->rowLength[r] = rs[r + 1] - rs[r];
  h->threshold = -1;
  h->refreshed = false;
  int rc = ppb == 2 ? upload_aos<2>(*h, ids, info, eb) : ppb == 3 ? upload_aos<3>(*h, ids, info, eb) : upload_aos<4>(*h, ids, info, eb);
  if (rc) return rc;
  if (h->rowStart.reserve(sizeof(int) * (h->nrows + 1)) || h->rowId.reserve(sizeof(int) * (h->nrows + 1)) ||
      h->rowIndex.reserve(sizeof(int) * (h->nrows + 1)) || h->fixedPoints.reserve(sizeof(float4) * (nfixed + 1)))
    return -1;
  UH_CHECK(hipMemcpy(h->rowStart.ptr, rs.data(), sizeof(int) * (h->nrows + 1), hipMemcpyHostToDevice));
  if (h->nrows) UH_CHECK(hipMemcpy(h->rowId.ptr, rid.data(), sizeof(int) * h->nrows, hipMemcpyHostToDevice));
  if (nfixed) UH_CHECK(hipMemcpy(h->fixedPoints.ptr, fixedPoints, sizeof(float4) * nfixed, hipMemcpyHostToDevice));
  return 0;
}

int uammd_bonded_refresh(uammd_bonded *hh, const int *d_id2index, int numberParticles, void *stream) {
  Handle *h = reinterpret_cast<Handle *>(hh);
  if (!h || h->kind < 0 || numberParticles < 0 || (numberParticles > 0 && !d_id2index)) {
    set_last_error("uammd_bonded_refresh: bad arguments (no bond set uploaded?)");
    return -1;
  }
  if (h->maxId >= numberParticles) {
    set_last_error("uammd_bonded_refresh: a bond names particle %d, there are %d particles", h->maxId, numberParticles);
    return -1;
  }
  hipStream_t st = (hipStream_t)stream;
  if (numberParticles) {
    if (h->id2index.reserve(sizeof(int) * numberParticles)) return -1;
    UH_CHECK(hipMemcpyAsync(h->id2index.ptr, d_id2index, sizeof(int) * numberParticles, hipMemcpyDeviceToDevice, st));
  }
  const int n = std::max(h->nentries, h->nrows);
  if (n) {
    const int *rid = (const int *)h->rowId.ptr;
    int *memb = (int *)h->memb.ptr, *ri = (int *)h->rowIndex.ptr;
    const int *i2i = (const int *)h->id2index.ptr;
    if (h->ppb == 2)
      hipLaunchKernelGGL(k_refresh<2>, dim3((n + 255) / 256), dim3(256), 0, st, (const AosBond<2> *)h->aos.ptr, h->nentries, rid, h->nrows, i2i, memb, ri);
    else if (h->ppb == 3)
      hipLaunchKernelGGL(k_refresh<3>, dim3((n + 255) / 256), dim3(256), 0, st, (const AosBond<3> *)h->aos.ptr, h->nentries, rid, h->nrows, i2i, memb, ri);
    else
      hipLaunchKernelGGL(k_refresh<4>, dim3((n + 255) / 256), dim3(256), 0, st, (const AosBond<4> *)h->aos.ptr, h->nentries, rid, h->nrows, i2i, memb, ri);
    UH_CHECK(hipGetLastError());
  }
  h->refreshed = true;
  return 0;
}

int uammd_bonded_sum(uammd_bonded *hh, const float *d_pos, float *d_force, float *d_energy, float *d_virial, void *stream) {
  Handle *h = reinterpret_cast<Handle *>(hh);
  if (!h || h->kind < 0 || !h->refreshed) {
    set_last_error("uammd_bonded_sum: no bond set uploaded and refreshed on this handle");
    return -1;
  }
  const Comp comp{d_force != nullptr, d_energy != nullptr, d_virial != nullptr};
  if (h->nrows == 0 || (!comp.force && !comp.energy && !comp.virial)) return 0;
  if (!d_pos) { set_last_error("uammd_bonded_sum: null positions"); return -1; }
  const float4 *pos = reinterpret_cast<const float4 *>(d_pos);
  const Outputs o{reinterpret_cast<float4 *>(d_force), d_energy, d_virial};
  hipStream_t st = (hipStream_t)stream;
  switch (h->kind) {
    case HARMONIC: return launch_sum<HARMONIC>(*h, pos, o, comp, st);
    case FENE: return launch_sum<FENE>(*h, pos, o, comp, st);
    case ANGULAR: return launch_sum<ANGULAR>(*h, pos, o, comp, st);
    case TORSIONAL: return launch_sum<TORSIONAL>(*h, pos, o, comp, st);
    default: return launch_sum<FOURIER>(*h, pos, o, comp, st);
  }
}

int uammd_bonded_get_shape(uammd_bonded *hh, int *rows, int *entries, int *laneRows, int *waveRows) {
  Handle *h = reinterpret_cast<Handle *>(hh);
  if (!h) { set_last_error("uammd_bonded_get_shape: null handle"); return -1; }
  if (h->kind >= 0 && split_rows(*h)) return -1;
  if (rows) *rows = h->nrows;
  if (entries) *entries = h->nentries;
  if (laneRows) *laneRows = h->nLane;
  if (waveRows) *waveRows = h->nWave;
  return 0;
}

}  // extern "C"
