// DOUBLE_PRECISION build of BondedForces / AngularBondedForces / TorsionalBondedForces for gfx950: the `_f64` entry points that bonded.hip
// has in single precision (reference: src/Interactor/BondedForces.{cuh,cu}, AngularBondedForces.cuh, TorsionalBondedForces.cuh).
//
// The same five kinds with the same BondInfo order, the same CSR layout (rows in ascending id, entries in registration order, SoA member
// indices, a negative index -(j+1) reads fixedPoints[j]) and the same two shapes: lane per row up to `bonded_wave_threshold` entries, wave
// per row above with the fixed DPP tree for the wave's sum.  No atomics: the same bits run to run.  The arithmetic is the reference's line
// by line with real = double; where the single-precision kernel uses a hardware approximation (rsqrtf) this one divides: 1.0 / sqrt(r2).
// uammd_bonded_build_rows has no precision and is shared with bonded.hip, as is the wave threshold.
#include "celllist.hpp"

#include <algorithm>
#include <atomic>
#include <vector>

namespace uammd_hip {

namespace bonded {
extern std::atomic<int> g_waveThreshold;  // bonded.hip
void build_rows(int ppb, int nbonds, const int *ids, std::vector<int> &rowId, std::vector<int> &rowStart, std::vector<int> &entryBond);
}  // namespace bonded

namespace bonded64 {

struct V3 { double x, y, z; };
UH_D V3 v3(double4 p) { return {p.x, p.y, p.z}; }
UH_D V3 operator+(V3 a, V3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
UH_D V3 operator-(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
UH_D V3 operator*(double s, V3 a) { return {s * a.x, s * a.y, s * a.z}; }
UH_D V3 operator*(V3 a, double s) { return {a.x * s, a.y * s, a.z * s}; }
// utils/vector.cuh of the reference: dot and cross as written there (no contraction: the library builds with -ffp-contract=off)
UH_D double dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
UH_D V3 cross(V3 a, V3 b) { return {a.y * b.z - a.z * b.y, (-a.x * b.z + a.z * b.x), a.x * b.y - a.y * b.x}; }
UH_D V3 pbc(const BoxT<double> &box, V3 r) {
  const vec3<double> q = box.apply_pbc(vec3<double>{r.x, r.y, r.z});
  return {q.x, q.y, q.z};
}
UH_D double rsqrt_(double x) { return 1.0 / sqrt(x); }

struct Comp { bool force, energy, virial; };
struct CT { V3 force; double virial, energy; };  // ComputeType, BondedForces.cuh:46-50
UH_D CT zero_ct() { return CT{{0.0, 0.0, 0.0}, 0.0, 0.0}; }

enum Kind { HARMONIC = 0, FENE = 1, ANGULAR = 2, TORSIONAL = 3, FOURIER = 4 };
template <int K> struct Members { static constexpr int value = K <= FENE ? 2 : (K == ANGULAR ? 3 : 4); };

// Harmonic: BondedForces.cuh:57-78, :98-107.  BondInfo {k, r0}.   FENE: BondedForces.cuh:119-138, :149-158.  BondInfo {r0, k}.
template <int K> UH_D CT compute_pair(int self, const int *ids, const V3 *pos, Comp comp, double2 bi, const BoxT<double> &box) {
  V3 ri = pos[0], rj = pos[1];
  if (self == ids[0]) { const V3 t = ri; ri = rj; rj = t; }
  const V3 r12 = pbc(box, rj - ri);
  const double r2 = dot(r12, r12);
  CT ct;
  if (K == HARMONIC) {
    const double k = bi.x, r0 = bi.y;
    const double invr = rsqrt_(r2);
    const double f = -k * (1.0 - r0 * invr);
    ct.force = f * r12;
    const double d = 1.0 / invr - r0;
    ct.energy = comp.energy ? (0.25 * k * (d * d)) : 0.0;
    ct.virial = comp.virial ? dot(ct.force, r12) : 0.0;
  } else {
    const double r0 = bi.x, k = bi.y, r02 = r0 * r0;
    const double f = -r02 * k / (r02 - r2);
    ct.force = f * r12;
    ct.energy = comp.energy ? (-0.25 * k * r02 * log(1.0 - r2 / r02)) : 0.0;
    ct.virial = comp.virial ? dot(ct.force, r12) : 0.0;
  }
  return (r2 == 0.0) ? zero_ct() : ct;
}

// Angular: AngularBondedForces.cuh:66-127.  BondInfo {ang0, k}.  No energy, no virial (the reference leaves them 0).
UH_D CT compute_angular(int self, const int *ids, const V3 *pos, Comp, double2 bi, const BoxT<double> &box) {
  const double ang0 = bi.x, kspring = bi.y;
  const V3 rij = pbc(box, pos[1] - pos[0]);
  const double rij2 = dot(rij, rij);
  const double invsqrij = rsqrt_(rij2);
  const V3 rjk = pbc(box, pos[2] - pos[1]);
  const double rjk2 = dot(rjk, rjk);
  const double invsqrjk = rsqrt_(rjk2);
  const double a2 = invsqrij * invsqrjk;
  double cijk = dot(rij, rjk) * a2;
  if (cijk > 1.0) cijk = 1.0;
  else if (cijk < -1.0) cijk = -1.0;
  double ampli;
  CT ct = zero_ct();
  if (ang0 == 0.0) {
    ampli = -2.0 * kspring;
  } else {
    const double theta = acos(cijk);
    if (theta == 0.0) return zero_ct();
    const double sinthetao2 = sin(0.5 * theta);
    ampli = -2.0 * kspring * (sinthetao2 - sin(ang0 * 0.5)) / sinthetao2;
  }
  const double a11 = ampli * cijk / rij2;
  const double a12 = ampli * a2;
  const double a22 = ampli * cijk / rjk2;
  if (self == ids[0]) ct.force = a12 * rjk - a11 * rij;
  else if (self == ids[1]) ct.force = -1.0 * ((-a11 - a12) * rij + (a12 + a22) * rjk);
  else if (self == ids[2]) ct.force = -1.0 * (a12 * rij - a22 * rjk);
  return ct;
}

// Torsional: TorsionalBondedForces.cuh:60-108.  BondInfo {phi0, k}.  Force only, with the intended member mapping.
UH_D CT compute_torsional(int self, const int *ids, const V3 *pos, Comp, double2 bi, const BoxT<double> &box) {
  const double phi0 = bi.x, k = bi.y;
  const V3 rjk = pbc(box, pos[1] - pos[0]);
  const V3 rkm = pbc(box, pos[2] - pos[1]);
  const V3 rmn = pbc(box, pos[3] - pos[2]);
  V3 njkm = cross(rjk, rkm);
  V3 nkmn = cross(rkm, rmn);
  const double n2 = dot(njkm, njkm);
  const double nn2 = dot(nkmn, nkmn);
  if (n2 > 0 && nn2 > 0) {
    const double invn = rsqrt_(n2);
    const double invnn = rsqrt_(nn2);
    const double cosphi = dot(njkm, nkmn) * invn * invnn;
    double Fmod = 0;
    const double phi = acos(cosphi);
    if (cosphi * cosphi <= 1 && phi * phi > 0) Fmod = -k * (phi - phi0) / sin(phi);
    njkm = njkm * invn;
    nkmn = nkmn * invnn;
    CT ct = zero_ct();
    const V3 v1 = (nkmn - cosphi * njkm) * invn;
    const V3 fj = Fmod * cross(v1, rkm);
    if (self == ids[0]) { ct.force = -1.0 * fj; return ct; }
    const V3 v2 = (njkm - cosphi * nkmn) * invnn;
    const V3 fk = Fmod * cross(v2, rmn);
    const V3 fm = Fmod * cross(v1, rjk);
    if (self == ids[1]) { ct.force = fm + fj - fk; return ct; }
    const V3 fn = Fmod * cross(v2, rkm);
    if (self == ids[2]) { ct.force = fn + fk - fm; return ct; }
    if (self == ids[3]) { ct.force = -1.0 * fn; return ct; }
  }
  return zero_ct();
}

// FourierLAMMPS: TorsionalBondedForces.cuh:121-207 (compute, signOfPhi).  BondInfo {phi0, kdih}.
UH_D double sign_of_phi(V3 r12, V3 r23, V3 r34) {
  const V3 ru23 = r23 * rsqrt_(dot(r23, r23));
  const V3 uloc1 = r12 * rsqrt_(dot(r12, r12));
  const V3 uloc2 = ru23 - dot(uloc1, ru23) * uloc1;
  const V3 uloc3 = cross(uloc1, uloc2);
  return (dot(r34, uloc3) < 0) ? -1.0 : 1.0;
}
UH_D CT compute_fourier(int self, const int *ids, const V3 *pos, Comp comp, double2 bi, const BoxT<double> &box) {
  const double phi0 = bi.x, kdih = bi.y;
  const V3 r12 = pbc(box, pos[1] - pos[0]);
  const V3 r23 = pbc(box, pos[2] - pos[1]);
  const V3 r34 = pbc(box, pos[3] - pos[2]);
  const V3 v123 = cross(r12, r23);
  const V3 v234 = cross(r23, r34);
  const double v123q = dot(v123, v123);
  const double v234q = dot(v234, v234);
  CT ct = zero_ct();
  if (v123q < 1e-15 || v234q < 1e-15) return ct;
  const double invsqv123 = rsqrt_(v123q);
  const double invsqv234 = rsqrt_(v234q);
  const double cosPhi = fmax(-1.0, fmin(1.0, dot(v123, v234) * invsqv123 * invsqv234));
  const double phi = sign_of_phi(r12, r23, r34) * acos(cosPhi);
  if (comp.energy) ct.energy = 0.25 * kdih * (1 + cos(phi - phi0));
  if (!comp.force && !comp.virial) return ct;
  if (fabs(phi) < 1e-10 || M_PI - fabs(phi) < 1e-10) return ct;
  const double pref = -kdih * sin(phi - phi0) / sin(phi);
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

template <int K> UH_D CT compute(int self, const int *ids, const V3 *pos, Comp comp, double2 bi, const BoxT<double> &box) {
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

struct Outputs { double4 *force; double *energy, *virial; };

UH_D void store(const Outputs &o, Comp comp, int i, const CT &ct) {  // BondedForces.cu:240-245
  if (comp.force) {
    double4 f = o.force[i];
    f.x += ct.force.x; f.y += ct.force.y; f.z += ct.force.z;
    o.force[i] = f;
  }
  if (comp.energy) o.energy[i] += ct.energy;
  if (comp.virial) o.virial[i] += ct.virial;
}

// the entries in current-index space: memb[k * stride + e] (negative: fixed point -(j+1)), info[e]
struct Rows {
  const int *rowIndex, *rowStart, *memb;
  const double2 *info;
  const double4 *fixedPoints;
  int stride;
};

template <int K> UH_D CT entry(const Rows &R, int e, int self, const double4 *__restrict__ pos, Comp comp, const BoxT<double> &box) {
  constexpr int NP = Members<K>::value;
  int ids[NP];
  V3 p[NP];
#pragma unroll
  for (int k = 0; k < NP; ++k) ids[k] = R.memb[k * R.stride + e];
  const double2 bi = R.info[e];
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
__global__ void __launch_bounds__(256) k64_lane(Rows R, const int *__restrict__ list, int n, const double4 *__restrict__ pos, Comp comp,
                                                BoxT<double> box, Outputs o) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  const int r = list[t];
  const int self = R.rowIndex[r];
  const int first = R.rowStart[r], last = R.rowStart[r + 1];
  CT acc = zero_ct();
  for (int e = first; e < last; ++e) accumulate(acc, entry<K>(R, e, self, pos, comp, box));
  store(o, comp, self, acc);
}

// wave_sum_to_last (device_common.hpp) for a double: the same DPP tree, each move carrying the two halves of the value
template <int CTRL, int ROWS, bool BOUND> UH_D double dpp_move64(double v) {
  const long long b = __builtin_bit_cast(long long, v);
  const int lo = __builtin_amdgcn_update_dpp(0, (int)(b & 0xffffffffll), CTRL, ROWS, 0xf, BOUND);
  const int hi = __builtin_amdgcn_update_dpp(0, (int)(b >> 32), CTRL, ROWS, 0xf, BOUND);
  return __builtin_bit_cast(double, ((long long)hi << 32) | (long long)(unsigned int)lo);
}
UH_D double wave_sum_to_last64(double x) {
  x += dpp_move64<0xB1, 0xf, true>(x);    // quad_perm [1, 0, 3, 2]
  x += dpp_move64<0x4E, 0xf, true>(x);    // quad_perm [2, 3, 0, 1]
  x += dpp_move64<0x141, 0xf, true>(x);   // row_half_mirror: eight lanes
  x += dpp_move64<0x140, 0xf, true>(x);   // row_mirror: the row of sixteen
  x += dpp_move64<0x142, 0xa, false>(x);  // row_bcast:15 into rows 1 and 3
  x += dpp_move64<0x143, 0xc, false>(x);  // row_bcast:31 into rows 2 and 3
  return x;
}

// wave per row: lane l takes entries first + l, first + l + 64, ...; the partial sums meet in the fixed DPP tree
template <int K>
__global__ void __launch_bounds__(256) k64_wave(Rows R, const int *__restrict__ list, int n, const double4 *__restrict__ pos, Comp comp,
                                                BoxT<double> box, Outputs o) {
  const int w = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (w >= n) return;  // (whole waves leave together: the DPP tree below runs with all 64 lanes)
  const int r = list[w];
  const int self = R.rowIndex[r];
  const int first = R.rowStart[r], last = R.rowStart[r + 1];
  CT acc = zero_ct();
  for (int e = first + lane; e < last; e += 64) accumulate(acc, entry<K>(R, e, self, pos, comp, box));
  CT s;
  s.force.x = comp.force ? wave_sum_to_last64(acc.force.x) : 0.0;
  s.force.y = comp.force ? wave_sum_to_last64(acc.force.y) : 0.0;
  s.force.z = comp.force ? wave_sum_to_last64(acc.force.z) : 0.0;
  s.energy = comp.energy ? wave_sum_to_last64(acc.energy) : 0.0;
  s.virial = comp.virial ? wave_sum_to_last64(acc.virial) : 0.0;
  if (lane == 63) store(o, comp, self, s);
}

// ids (id space, member-major SoA) -> current indices, and each row's own index
__global__ void __launch_bounds__(256) k64_refresh(const int *__restrict__ membId, int nwords, const int *__restrict__ rowId, int nrows,
                                                   const int *__restrict__ id2index, int *memb, int *rowIndex) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t < nwords) {
    const int id = membId[t];
    memb[t] = id < 0 ? id : id2index[id];
  }
  if (t < nrows) rowIndex[t] = id2index[rowId[t]];
}

int members_of(int kind) { return kind <= FENE ? 2 : (kind == ANGULAR ? 3 : 4); }

struct Handle {
  int kind = -1, ppb = 0, nbonds = 0, nrows = 0, nentries = 0, nfixed = 0, maxId = -1;
  BoxT<double> box;
  std::vector<int> rowLength;                 // host: entries per row (for the shape split)
  int threshold = -1, nLane = 0, nWave = 0;   // the split in force
  bool refreshed = false;
  DeviceBuffer membId, rowStart, rowId, fixedPoints, memb, info, rowIndex, laneRows, waveRows, id2index;
};

int split_rows(Handle &h) {
  const int T = bonded::g_waveThreshold.load();
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

template <int K> int launch_sum(Handle &h, const double4 *pos, Outputs o, Comp comp, hipStream_t st) {
  if (split_rows(h)) return -1;
  Rows R{(const int *)h.rowIndex.ptr, (const int *)h.rowStart.ptr, (const int *)h.memb.ptr, (const double2 *)h.info.ptr,
         (const double4 *)h.fixedPoints.ptr, h.nentries};
  if (h.nLane)
    hipLaunchKernelGGL(k64_lane<K>, dim3((h.nLane + 255) / 256), dim3(256), 0, st, R, (const int *)h.laneRows.ptr, h.nLane, pos, comp, h.box, o);
  if (h.nWave)
    hipLaunchKernelGGL(k64_wave<K>, dim3((h.nWave + 3) / 4), dim3(256), 0, st, R, (const int *)h.waveRows.ptr, h.nWave, pos, comp, h.box, o);
  UH_CHECK(hipGetLastError());
  return 0;
}

}  // namespace bonded64
}  // namespace uammd_hip

using namespace uammd_hip;
using namespace uammd_hip::bonded64;

extern "C" {

int uammd_bonded_create_f64(uammd_bonded_f64 **out) {
  if (!out) { set_last_error("uammd_bonded_create_f64: null argument"); return -1; }
  *out = reinterpret_cast<uammd_bonded_f64 *>(new Handle());
  return 0;
}

int uammd_bonded_destroy_f64(uammd_bonded_f64 *h) {
  delete reinterpret_cast<Handle *>(h);
  return 0;
}

int uammd_bonded_upload_f64(uammd_bonded_f64 *hh, int kind, int nbonds, const int *ids, const double *info, int nfixed,
                            const double *fixedPoints, const double L[3], const int periodic[3]) {
  Handle *h = reinterpret_cast<Handle *>(hh);
  if (!h || kind < HARMONIC || kind > FOURIER || nbonds < 0 || nfixed < 0 || (nbonds > 0 && (!ids || !info)) || (nfixed > 0 && !fixedPoints) ||
      !L || !periodic) {
    set_last_error("uammd_bonded_upload_f64: bad arguments");
    return -1;
  }
  const int ppb = members_of(kind);
  for (long i = 0; i < (long)nbonds * ppb; ++i) {
    const int id = ids[i];
    if (id < -nfixed || (id < 0 && ppb != 2)) {
      set_last_error("uammd_bonded_upload_f64: bond %ld refers to fixed point %d, there are %d", i / ppb, -id - 1, nfixed);
      return -1;
    }
  }
  std::vector<int> rid, rs, eb;
  bonded::build_rows(ppb, nbonds, ids, rid, rs, eb);
  const int nrows = (int)rid.size(), nentries = (int)eb.size();
  // member-major ids and the BondInfo of every entry
  std::vector<int> membId((size_t)ppb * nentries);
  std::vector<double> inf(2 * (size_t)nentries);
  for (int e = 0; e < nentries; ++e) {
    const int b = eb[e];
    for (int k = 0; k < ppb; ++k) membId[(size_t)k * nentries + e] = ids[(long)b * ppb + k];
    inf[2 * (size_t)e] = info[2l * b];
    inf[2 * (size_t)e + 1] = info[2l * b + 1];
  }
  h->kind = -1;  // (nothing usable until every buffer below is in place)
  h->refreshed = false;
  if (h->membId.reserve(sizeof(int) * (membId.size() + 1)) || h->memb.reserve(sizeof(int) * (membId.size() + 1)) ||
      h->info.reserve(sizeof(double) * (inf.size() + 2)) || h->rowStart.reserve(sizeof(int) * (nrows + 1)) ||
      h->rowId.reserve(sizeof(int) * (nrows + 1)) || h->rowIndex.reserve(sizeof(int) * (nrows + 1)) ||
      h->fixedPoints.reserve(4 * sizeof(double) * (nfixed + 1)))
    return -1;
  if (nentries) {
    UH_CHECK(hipMemcpy(h->membId.ptr, membId.data(), sizeof(int) * membId.size(), hipMemcpyHostToDevice));
    UH_CHECK(hipMemcpy(h->info.ptr, inf.data(), sizeof(double) * inf.size(), hipMemcpyHostToDevice));
  }
  UH_CHECK(hipMemcpy(h->rowStart.ptr, rs.data(), sizeof(int) * (nrows + 1), hipMemcpyHostToDevice));
  if (nrows) UH_CHECK(hipMemcpy(h->rowId.ptr, rid.data(), sizeof(int) * nrows, hipMemcpyHostToDevice));
  if (nfixed) UH_CHECK(hipMemcpy(h->fixedPoints.ptr, fixedPoints, 4 * sizeof(double) * nfixed, hipMemcpyHostToDevice));
  h->ppb = ppb;
  h->nbonds = nbonds;
  h->nfixed = nfixed;
  h->nrows = nrows;
  h->nentries = nentries;
  h->maxId = rid.empty() ? -1 : rid.back();
  h->box = make_box<double>(L, periodic);
  h->rowLength.resize(nrows);
  for (int r = 0; r < nrows; ++r) h->rowLength[r] = rs[r + 1] - rs[r];
  h->threshold = -1;
  h->kind = kind;
  return 0;
}

int uammd_bonded_refresh_f64(uammd_bonded_f64 *hh, const int *d_id2index, int numberParticles, void *stream) {
  Handle *h = reinterpret_cast<Handle *>(hh);
  if (!h || h->kind < 0 || numberParticles < 0 || (numberParticles > 0 && !d_id2index)) {
    set_last_error("uammd_bonded_refresh_f64: bad arguments (no bond set uploaded?)");
    return -1;
  }
  if (h->maxId >= numberParticles) {  // the sum would read positions out of range
    set_last_error("uammd_bonded_refresh_f64: a bond names particle %d, there are %d particles", h->maxId, numberParticles);
    return -1;
  }
  hipStream_t st = (hipStream_t)stream;
  if (numberParticles) {
    if (h->id2index.reserve(sizeof(int) * numberParticles)) return -1;
    UH_CHECK(hipMemcpyAsync(h->id2index.ptr, d_id2index, sizeof(int) * numberParticles, hipMemcpyDeviceToDevice, st));
  }
  const int nwords = h->ppb * h->nentries;
  const int n = std::max(nwords, h->nrows);
  if (n) {
    hipLaunchKernelGGL(k64_refresh, dim3((n + 255) / 256), dim3(256), 0, st, (const int *)h->membId.ptr, nwords, (const int *)h->rowId.ptr,
                       h->nrows, (const int *)h->id2index.ptr, (int *)h->memb.ptr, (int *)h->rowIndex.ptr);
    UH_CHECK(hipGetLastError());
  }
  h->refreshed = true;
  return 0;
}

int uammd_bonded_sum_f64(uammd_bonded_f64 *hh, const double *d_pos, double *d_force, double *d_energy, double *d_virial, void *stream) {
  Handle *h = reinterpret_cast<Handle *>(hh);
  if (!h || h->kind < 0 || !h->refreshed) {
    set_last_error("uammd_bonded_sum_f64: no bond set uploaded and refreshed on this handle");
    return -1;
  }
  const Comp comp{d_force != nullptr, d_energy != nullptr, d_virial != nullptr};
  if (h->nrows == 0 || (!comp.force && !comp.energy && !comp.virial)) return 0;
  if (!d_pos) { set_last_error("uammd_bonded_sum_f64: null positions"); return -1; }
  const double4 *pos = reinterpret_cast<const double4 *>(d_pos);
  const Outputs o{reinterpret_cast<double4 *>(d_force), d_energy, d_virial};
  hipStream_t st = (hipStream_t)stream;
  switch (h->kind) {
    case HARMONIC: return launch_sum<HARMONIC>(*h, pos, o, comp, st);
    case FENE: return launch_sum<FENE>(*h, pos, o, comp, st);
    case ANGULAR: return launch_sum<ANGULAR>(*h, pos, o, comp, st);
    case TORSIONAL: return launch_sum<TORSIONAL>(*h, pos, o, comp, st);
    default: return launch_sum<FOURIER>(*h, pos, o, comp, st);
  }
}

int uammd_bonded_get_shape_f64(uammd_bonded_f64 *hh, int *rows, int *entries, int *laneRows, int *waveRows) {
  Handle *h = reinterpret_cast<Handle *>(hh);
  if (!h) { set_last_error("uammd_bonded_get_shape_f64: null handle"); return -1; }
  if (h->kind >= 0 && split_rows(*h)) return -1;
  if (rows) *rows = h->nrows;
  if (entries) *entries = h->nentries;
  if (laneRows) *laneRows = h->nLane;
  if (waveRows) *waveRows = h->nWave;
  return 0;
}

}  // extern "C"
