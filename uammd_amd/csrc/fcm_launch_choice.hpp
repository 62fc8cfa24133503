// Which kernel instantiation a spread or a gather of the FCM handle (fcm.hip) launches, and on how many workgroups, decided on the host:
// plain C++14, no HIP header, no environment.  fcm.hip reads the switches once, fills the inputs, and launches what it is told
// (fcm_run_spread_tile, fcm_run_gather); uammd_fcm_probe's `info` reports the same choice.  tests/cxx/fcm_launch_choice.cpp replays
// tests/golden/fcm_launch_choice.json (recorded through the probe before the choices moved here) and enumerates the inputs against the
// kernels' own limits, under the sanitizers.
#pragma once
#include <cstddef>

namespace uammd_hip {

struct FcmInt3 { int x, y, z; };

// The environment's A/B switches, read by fcm.hip once per process.
struct FcmSwitches {
  int gatherHalf = 1;       // UAMMD_FCM_GATHER_HALF: 0 k_fcm_gather_half off, 1 on cache-resident grids, 2 also on grids read from HBM
  bool noSpec = false;      // UAMMD_FCM_NO_SPEC set: no speculative first round of the spread
  bool specDense = false;   // UAMMD_FCM_SPEC_DENSE set: the speculative round with four waves per tile too
  bool packedInter = true;  // UAMMD_FCM_PACKED_INTER=0: the gather's grid as float4 everywhere
  bool noTile9 = false;     // UAMMD_FCM_NO_TILE9 set: no 9-node tile edge
  bool noPlaneFft = false;  // UAMMD_FCM_NO_PLANE_FFT set: the x / y transforms by rows and lines only
  bool slots = true;        // UAMMD_FCM_SLOTS=0: a new handle's option "slots" starts off
};

// ---- tiles -------------------------------------------------------------------------------------------------------------------------------
constexpr int kTile = 8;      // the tile edge that the kernels' LDS / matrix layouts are sized for
constexpr int kTileMax = 9;   // the spread's second instantiation (108 = 12 x 9, ...)
// The tile-owned spread/gather needs every axis to divide into >= 3 tiles of edge T and a stencil that reaches the adjacent tiles only
// (a particle is binned by ITS cell and its stencil reaches support / 2 (+ 1 with the shift of even supports) nodes either way: it stays
// within the adjacent tiles when support <= 2 (T - 1)).  The tile edge T is chosen per axis: the largest divisor of the axis in 4..8
// that satisfies this — 8 for power-of-two grids, 6 for the 108^3 grid of the PSE far field at psi = 0.5, 5 for 100, 7 for 84.  The
// kernels' LDS / matrix layouts are sized for 8; a shorter tile leaves rows and columns unused (and unwritten).
inline bool fcm_tiles_usable(const int cells[3], const int support[3], bool only8, const FcmSwitches &sw, FcmInt3 *tdim) {
  int T[3];
  for (int a = 0; a < 3; ++a) {
    T[a] = 0;
    // 8 where it divides the axis; then 9 (the spread's second instantiation: 108, 162, 180, 198, 270 ...) before the shorter edges
    const int order[6] = {8, 9, 7, 6, 5, 4};
    for (int k = 0; k < (only8 ? 1 : 6); ++k) {
      const int t = order[k];
      if (t == 9 && sw.noTile9) continue;
      if (cells[a] % t == 0 && cells[a] / t >= 3 && support[a] <= 2 * (t - 1)) { T[a] = t; break; }
    }
    if (!T[a]) return false;
  }
  *tdim = FcmInt3{T[0], T[1], T[2]};
  return true;
}
// option "tile_gather": k_fcm_gather_tile's staged window is loaded in aligned x pairs and is 16 nodes wide — an even tile edge along x,
// edge + support - 1 <= 16; elsewhere the option is accepted and the global gather runs
inline bool fcm_tile_gather_fits(FcmInt3 tdim, FcmInt3 support) {
  return tdim.x % 2 == 0 && tdim.x + support.x - 1 <= 16 && tdim.y + support.y - 1 <= 16 && tdim.z + support.z - 1 <= 16;
}

// ---- spread (k_fcm_spread_tile<W, SLOTS, E, SPEC>) ------------------------------------------------------------------------------------------
#ifndef UAMMD_SP_WORDS   // (A/B builds: tools/variants_fcm.sh — 6144 words / 4 candidates per thread: within 1 % of these at C4 and 108^3)
#define UAMMD_SP_WORDS 6144
#endif
constexpr int kSpWeightWordsMax = UAMMD_SP_WORDS;

struct FcmSpreadInputs {
  int N;
  FcmInt3 ntiles, support, tdim;
  int wavesOption;   // option "spread_waves": 0 = by the tiles' population, 2, 4
  bool slots;        // this solve reads the slot layout
  int cap;           // its records per tile (FcmPrep::cap)
  bool allowSpec;    // false: the slab, which instantiates no speculative round
  FcmSwitches sw;
};
struct FcmSpreadChoice {
  int waves;        // W: waves per tile
  int edge;         // E: kTile or kTileMax
  int weightWords;  // LDS budget of phase B in words: 24 (27 with E = 9) per listed particle
  bool spec;        // SPEC
  int listEntries;  // particles that one chunk of a tile's list holds
};
// dynamic LDS: float wts[weightWords + 32] | entry list[64 waves + 1]   (a list never holds more entries than the workgroup has threads;
// +1: phase C reads 8 words per 5-word entry); the waves' private tiles of the final sum alias the same block.  Two-wave tiles with
// 129 entries instead of 257: 15.6 KB per workgroup, ten of them on a CU — as many as the registers allow — instead of nine.
inline size_t fcm_spread_lds_bytes(const FcmSpreadChoice &c, size_t entryBytes) {
  const size_t a = sizeof(float) * (size_t)(c.weightWords + 32) + entryBytes * (64 * c.waves + 1),
               b = sizeof(float) * c.waves * 3 * c.edge * c.edge * c.edge;
  return a > b ? a : b;
}
inline FcmSpreadChoice fcm_choose_spread(const FcmSpreadInputs &in) {
  const FcmInt3 s = in.support, t = in.tdim;
  FcmSpreadChoice c{};
  const double perTile = (double)in.N / ((double)in.ntiles.x * in.ntiles.y * in.ntiles.z);
  const double listed = perTile * (1.0 + (s.x - 1) / (double)t.x) * (1.0 + (s.y - 1) / (double)t.y) * (1.0 + (s.z - 1) / (double)t.z);
  // two waves per tile where a tile lists few particles (measured at C5, ~26 listed: see DESIGN 5.4), four otherwise
  c.waves = (in.wavesOption == 2 || in.wavesOption == 4) ? in.wavesOption : listed > 48.0 ? 4 : 2;
  c.edge = (t.x > kTile || t.y > kTile || t.z > kTile) ? kTileMax : kTile;
  const int full = c.edge == kTileMax ? 256 * 3 * kTileMax : kSpWeightWordsMax;   // (256 listed particles either way)
  c.weightWords = listed > 64.0 ? full : full / 2;
  c.listEntries = c.weightWords / (3 * c.edge) < 64 * c.waves ? c.weightWords / (3 * c.edge) : 64 * c.waves;
  // (SPEC: see the kernel — two waves per tile, exactly eight source tiles, slots deep enough)
  const bool eight = (s.x - 2 + t.x) / t.x == 1 && (s.y - 2 + t.y) / t.y == 1 && (s.z - 2 + t.z) / t.z == 1;
  // (dense tiles, four waves, 8 x 32 slots: measured at C4 with no gain — 0.1578 / 0.1580 / 0.1593 against 0.1578 / 0.1589 / 0.1594 ms —
  // since the records' round trip hides behind the other tiles' matrix steps there; kept behind UAMMD_FCM_SPEC_DENSE=1 for A/B runs)
  // (the round lists up to one record per thread at once: the list and its weights must hold a workgroup's worth — capEntries >= 64 W)
  c.spec = in.allowSpec && !in.sw.noSpec && in.slots && eight && in.cap >= 8 * c.waves && c.weightWords / (3 * c.edge) >= 64 * c.waves &&
           (c.waves == 2 || in.sw.specDense);
  return c;
}

// ---- gather ---------------------------------------------------------------------------------------------------------------------------------
// (16 waves = 16 consecutive tile-sorted particles per workgroup, to share their lines in the CU's L1: 48.7 against 47.1 us)
constexpr int kGatherWaves = 4;
// the forms, as UAMMD_FCM_GATHER_* of include/uammd_hip.h (tied by a static_assert in fcm.hip)
enum FcmGatherForm { kFcmGatherAtomic = 0, kFcmGatherTile = 1, kFcmGatherPrep = 2, kFcmGatherInter = 3, kFcmGatherCol = 4, kFcmGatherHalf = 5 };

struct FcmGatherInputs {
  bool tiles;         // the tile-prepared stencils exist: the grid allows them and option "atomic_spread" is off
  bool interGather;   // option "interleaved_gather"
  bool tileGather;    // option "tile_gather", where it fits (fcm_tile_gather_fits)
  FcmInt3 support, cells;
  int perWave;        // option "gather_per_wave": 1, 2, 4; negative (test hook): k_fcm_gather_inter with that many particles per wave
  bool customFFT;     // the solve's own inverse x transform writes the interleaved grid (so it may be written packed)
  bool packedGiven;   // uammd_fcm_probe: the caller's packed grid
  FcmSwitches sw;
};
struct FcmGatherChoice {
  int form;               // FcmGatherForm
  int rs;                 // R of k_fcm_gather_inter<R, P, PK>, S of k_fcm_gather_half<S, SZMAX>, else 0
  int P;                  // particles per wave of the three interleaved forms, else 0
  int szmax;              // SZMAX of k_fcm_gather_col<P, SZMAX> and k_fcm_gather_half<S, SZMAX>, else 0
  bool readsInterleaved;  // inter, col, half: the inverse x transform (or k_fcm_interleave) writes the interleaved grid
  bool packed;            // that grid holds 12 bytes per node: k_fcm_gather_inter<R, P, true>
  // workgroups of the interleaved forms: kGatherWaves waves of P particles each
  int blocks(int N) const { return (N + kGatherWaves * P - 1) / (kGatherWaves * P); }
};
inline FcmGatherChoice fcm_choose_gather(const FcmGatherInputs &in) {
  const FcmInt3 s = in.support;
  const bool small = s.x <= 6 && s.y <= 6 && s.z <= 6;
  if (!in.tiles) return FcmGatherChoice{kFcmGatherAtomic, 0, 0, 0, false, false};
  if (small && in.tileGather) return FcmGatherChoice{kFcmGatherTile, 0, 0, 0, false, false};
  if (!in.interGather) return FcmGatherChoice{kFcmGatherPrep, 0, 0, 0, false, false};
  const size_t nodes = (size_t)in.cells.x * in.cells.y * in.cells.z, nodeBytes = 16;   // (a float4 per node)
  const int rounds = (s.x * s.y * s.z + 63) / 64;   // of 64 stencil nodes
  const int R = rounds <= 1 ? 1 : rounds <= 2 ? 2 : rounds <= 4 ? 4 : 8;
  // The grid with 12 bytes per node: where the float4 grid would not stay in the Infinity Cache between the inverse x pass and the
  // gather (> 128 MB: the same bound as for the cache-resident forms below).  The float4 forms do not apply to it.
  if (in.packedGiven || (in.customFFT && in.sw.packedInter && nodes * nodeBytes > ((size_t)128 << 20) && in.perWave >= 0)) {
    // (P as instantiated: up to two rounds always two particles per wave.  It used to be 4 with option "gather_per_wave" = 4 there
    // as well, and a grid sized for four per wave under a kernel that takes two left half of the particles ungathered — supports 3, 4, 5
    // on a packed grid: tests/test_gpu_fcm_stages.py, test_gather_forms[packed-1-2-per-wave-4] and [packed-2-2-per-wave-4])
    const int P = rounds <= 2 ? 2 : rounds <= 4 ? (in.perWave >= 4 ? 4 : 2) : 1;
    return FcmGatherChoice{kFcmGatherInter, R, P, 0, true, true};
  }
  if (in.sw.gatherHalf == 2 && in.perWave >= 0 && s.x == 6 && s.y == 6 && s.z <= 8 && nodes * nodeBytes < ((size_t)1 << 32))
    return FcmGatherChoice{kFcmGatherHalf, 6, 2, s.z <= 6 ? 6 : 8, true, false};
  // the column form where the float4 grid stays in the 256 MB Infinity Cache (C4: 39.5 -> 32.9 us; at C5, a 268 MB grid read from HBM,
  // its six partly filled loads per particle lose to the four full ones: 126 against 112 us)
  if (in.perWave >= 0 && s.x <= 8 && s.y <= 8 && s.z <= 8 && nodes * nodeBytes <= ((size_t)128 << 20)) {
    // (P = 2: 32.9 / 33.5 / 36.4 us with 2 / 3 / 4 particles per wave at C4)
    if (s.x == 6 && s.y == 6 && in.sw.gatherHalf != 0) return FcmGatherChoice{kFcmGatherHalf, 6, 2, s.z <= 6 ? 6 : 8, true, false};
    if (s.x == 7 && s.y == 7 && in.sw.gatherHalf != 0) return FcmGatherChoice{kFcmGatherHalf, 7, 2, s.z <= 7 ? 7 : 8, true, false};
    return FcmGatherChoice{kFcmGatherCol, 0, 2, s.z <= 6 ? 6 : 8, true, false};
  }
  const int perWave = in.perWave < 0 ? -in.perWave : in.perWave;  // (test hook: a negative value asks for k_fcm_gather_inter)
  // (measured at C4, support 6: 47.3 / 40.2 / 40.8 us with 1 / 2 / 4 particles per wave)
  const int P = (rounds <= 4 && perWave >= 2) ? (perWave >= 4 ? 4 : 2) : 1;
  return FcmGatherChoice{kFcmGatherInter, R, P, 0, true, false};
}

}  // namespace uammd_hip
