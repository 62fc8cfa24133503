// CPU test of the FCM launch choices (uammd_amd/csrc/fcm_launch_choice.hpp): a stand-alone program over that header alone, built with the
// address and undefined-behaviour sanitizers by tests/test_fcm_launch_choice_cpu.py.
//   replay      rows on stdin, made from tests/golden/fcm_launch_choice.json (what uammd_fcm_probe's info said on the GPU before the
//               choices moved into the header): the header gives the recorded choice for every row
//   enumerate   every combination of the inputs in the ranges below against invariants G1 .. G7, S1 .. S3, T1, which come from the
//               kernels' own limits (named next to each, by kernel of csrc/fcm.hip)
#include "../../uammd_amd/csrc/fcm_launch_choice.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>

using namespace uammd_hip;

static long failures = 0;
#define CHECK(cond, ...)                                  \
  do {                                                    \
    if (!(cond)) {                                        \
      if (failures++ < 20) {                              \
        std::printf("BROKEN %s: ", #cond);               \
        std::printf(__VA_ARGS__);                         \
        std::printf("\n");                               \
      }                                                   \
    }                                                     \
  } while (0)

// ---- replay --------------------------------------------------------------------------------------------------------------------------
// gather cx cy cz sx sy sz atomic_spread interleaved_gather tile_gather gather_per_wave packed | form R P SZMAX saidPacked   (form -1: the probe
//        refused the packed grid, because the options do not select a gather that reads an interleaved grid)
// spread cx cy cz sx sy sz spread_waves slots cap N | tiles waves edge spec tx ty tz listEntries
static int replay() {
  char kind[16];
  long rows = 0;
  const FcmSwitches sw;   // (recorded with no switch set)
  while (std::scanf("%15s", kind) == 1) {
    int c[3], s[3];
    if (std::scanf("%d %d %d %d %d %d", &c[0], &c[1], &c[2], &s[0], &s[1], &s[2]) != 6) return 2;
    FcmInt3 tdim{0, 0, 0};
    const bool usable = fcm_tiles_usable(c, s, false, sw, &tdim);
    const FcmInt3 cells{c[0], c[1], c[2]}, support{s[0], s[1], s[2]};
    if (!std::strcmp(kind, "gather")) {
      int atomic, inter, tileGather, perWave, packed, form, R, P, szmax, said;
      if (std::scanf("%d %d %d %d %d | %d %d %d %d %d", &atomic, &inter, &tileGather, &perWave, &packed, &form, &R, &P, &szmax, &said) != 10) return 2;
      // (a gather probe is stage 3 of the solve: the real grids are the caller's, the solve's own FFT does not run)
      const FcmGatherChoice g = fcm_choose_gather(FcmGatherInputs{usable && !atomic, inter != 0, tileGather && usable && fcm_tile_gather_fits(tdim, support),
                                                                  support, cells, perWave, false, packed != 0, sw});
      if (form < 0) CHECK(!g.readsInterleaved, "row %ld: refused by the probe, chosen form %d", rows, g.form);
      else
        CHECK(g.form == form && g.rs == R && g.P == P && g.szmax == szmax && (g.form == kFcmGatherInter && packed) == (said != 0) &&
                  g.packed == (packed != 0),
              "row %ld: cells %d %d %d support %d %d %d per wave %d packed %d: recorded %d %d %d %d, chosen %d %d %d %d", rows, c[0], c[1], c[2], s[0],
              s[1], s[2], perWave, packed, form, R, P, szmax, g.form, g.rs, g.P, g.szmax);
    } else if (!std::strcmp(kind, "spread")) {
      int wavesOpt, slots, cap, N, tiles, waves, edge, spec, t[3], listEntries;
      if (std::scanf("%d %d %d %d | %d %d %d %d %d %d %d %d", &wavesOpt, &slots, &cap, &N, &tiles, &waves, &edge, &spec, &t[0], &t[1], &t[2],
                     &listEntries) != 12) return 2;
      CHECK(usable == (tiles != 0), "row %ld: tiles", rows);
      if (usable) {
        const FcmSpreadChoice p = fcm_choose_spread(FcmSpreadInputs{N, FcmInt3{c[0] / tdim.x, c[1] / tdim.y, c[2] / tdim.z}, support, tdim, wavesOpt,
                                                                    slots != 0, cap, true, sw});
        CHECK(tdim.x == t[0] && tdim.y == t[1] && tdim.z == t[2] && p.waves == waves && p.edge == edge && p.spec == (spec != 0) &&
                  p.listEntries == listEntries,
              "row %ld: cells %d %d %d support %d N %d waves option %d slots %d cap %d: recorded W %d E %d spec %d list %d, chosen %d %d %d %d", rows,
              c[0], c[1], c[2], s[0], N, wavesOpt, slots, cap, waves, edge, spec, listEntries, p.waves, p.edge, (int)p.spec, p.listEntries);
      }
    } else
      return 2;
    rows++;
  }
  std::printf("replayed %ld rows: %ld differ\n", rows, failures);
  return failures ? 1 : 0;
}

// ---- enumeration -----------------------------------------------------------------------------------------------------------------------
static const int kCells[] = {16, 20, 24, 27, 32, 64, 108, 128, 200, 208, 256, 648};
static const int kNCells = sizeof(kCells) / sizeof(kCells[0]);

// the (R, P, packed) that fcm.hip instantiates k_fcm_gather_inter for
static bool inter_instantiated(int R, int P, bool packed) {
  if (packed) return (R == 1 && P == 2) || (R == 2 && P == 2) || (R == 4 && (P == 2 || P == 4)) || (R == 8 && P == 1);
  return ((R == 1 || R == 2 || R == 4) && (P == 1 || P == 2 || P == 4)) || (R == 8 && P == 1);
}

static void gather_invariants(const FcmGatherInputs &in, const FcmGatherChoice &g) {
  const FcmInt3 s = in.support;
  const unsigned long long nodes = (unsigned long long)in.cells.x * in.cells.y * in.cells.z;
  const bool interleaved = g.form == kFcmGatherInter || g.form == kFcmGatherCol || g.form == kFcmGatherHalf;
  // G7: without tile-prepared stencils only k_fcm_ibm<false> can run (every other gather reads FcmPrep::origin / weights)
  if (!in.tiles) CHECK(g.form == kFcmGatherAtomic, "form %d", g.form);
  CHECK(g.form >= kFcmGatherAtomic && g.form <= kFcmGatherHalf, "form %d", g.form);
  // G6: the three kernels that take `const float4 *gi`; k_fcm_gather_tile's LDS window is sized for supports <= 6 (its kGtW = 16 nodes)
  CHECK(g.readsInterleaved == interleaved, "form %d", g.form);
  if (g.form == kFcmGatherTile) CHECK(s.x <= 6 && s.y <= 6 && s.z <= 6 && in.tileGather, "support %d %d %d", s.x, s.y, s.z);
  if (g.form == kFcmGatherPrep) CHECK(!in.interGather, "prep");
  if (!interleaved) {
    CHECK(g.rs == 0 && g.P == 0 && g.szmax == 0 && !g.packed, "form %d", g.form);
    return;
  }
  // G1: slot0 = (block * kGatherWaves + wave) * P in all three kernels, `if (slot0 >= N) return`: every particle has a wave, no workgroup is idle
  CHECK((g.P == 1 || g.P == 2 || g.P == 4) && g.rs >= 0 && g.rs <= 8, "R %d P %d", g.rs, g.P);
  if (!((g.P == 1 || g.P == 2 || g.P == 4) && g.rs >= 0 && g.rs <= 8)) return;
  static bool sized[6][9][5][2];   // (blocks(N) reads the choice alone: once per distinct choice)
  bool &done = sized[g.form][g.rs][g.P][g.packed];
  for (int N = 1; N <= 4097 && !done; ++N) {
    const long long b = g.blocks(N);
    if (!(b * kGatherWaves * g.P >= N && (b - 1) * kGatherWaves * g.P < N)) {
      CHECK(false, "G1: form %d R %d P %d packed %d N %d blocks %lld", g.form, g.rs, g.P, (int)g.packed, N, b);
      break;
    }
  }
  done = true;
  if (g.form == kFcmGatherCol || g.form == kFcmGatherHalf) {
    // G2: k_fcm_gather_col / k_fcm_gather_half address a node as (uint)(base + planeNodes * z) << 4: byte offsets in 32 bits
    CHECK(nodes * 16 < (1ull << 32), "nodes %llu", nodes);
    CHECK(!g.packed && g.P == 2, "P %d", g.P);   // (both take float4 nodes; fcm.hip instantiates col<2, *>, half pairs two particles per wave)
  }
  if (g.form == kFcmGatherCol) {
    // G2: k_fcm_gather_col: lane = column (lane & 7, lane >> 3), float4 g[P][SZMAX]
    CHECK(s.x <= 8 && s.y <= 8 && s.z <= g.szmax && (g.szmax == 6 || g.szmax == 8) && g.rs == 0, "support %d %d %d SZMAX %d", s.x, s.y, s.z, g.szmax);
  }
  if (g.form == kFcmGatherHalf) {
    // G3: k_fcm_gather_half<S, SZMAX>: static_assert(R > 0 && 2 * S + SZMAX <= 32), float4 g[SZMAX], the weights of a particle in one half wave
    const int S = g.rs;
    CHECK(s.x == S && s.y == S && (S == 6 || S == 7) && s.z <= g.szmax && 2 * S + g.szmax <= 32 && (g.szmax == S || g.szmax == 8),
          "support %d %d %d S %d SZMAX %d", s.x, s.y, s.z, S, g.szmax);
    CHECK(in.sw.gatherHalf != 0, "half with the switch at 0");
  }
  if (g.form == kFcmGatherInter) {
    // G4: k_fcm_gather_inter<R, P>: R < 8 unrolls R rounds of 64 nodes once; R = 8 loops over chunks of 8 rounds; float4 v[P][R] in registers
    const int vol = s.x * s.y * s.z;
    if (g.rs < 8) CHECK(64 * g.rs >= vol, "R %d for %d nodes", g.rs, vol);
    CHECK(g.P == 1 || g.rs <= 4, "R %d P %d", g.rs, g.P);
    CHECK(inter_instantiated(g.rs, g.P, g.packed), "R %d P %d packed %d", g.rs, g.P, (int)g.packed);
    CHECK(g.szmax == 0, "SZMAX %d", g.szmax);
  }
  // G5: only k_fcm_gather_inter<R, P, true> reads 12-byte nodes
  if (g.packed) CHECK(g.form == kFcmGatherInter && inter_instantiated(g.rs, g.P, true), "form %d R %d P %d", g.form, g.rs, g.P);
  if (in.packedGiven) CHECK(g.packed, "a packed grid given to form %d", g.form);
}

static void enumerate_gather(long *count) {
  const int halfModes[] = {0, 1, 2};
  for (int sx = 1; sx <= 16; ++sx)
    for (int sy = 1; sy <= 16; ++sy)
      for (int sz = 1; sz <= 16; ++sz)
        for (int ci = 0; ci < kNCells; ++ci)     // (the choice reads the product of the cells only: cubic grids and two with unequal axes)
          for (int shape = 0; shape < 3; ++shape) {
            const int n = kCells[ci];
            const FcmInt3 cells = shape == 0 ? FcmInt3{n, n, n} : shape == 1 ? FcmInt3{n, kCells[(ci + 1) % kNCells], kCells[(ci + 5) % kNCells]}
                                                                             : FcmInt3{kCells[(ci + 7) % kNCells], n, n};
            for (int perWave = -4; perWave <= 4; ++perWave)
              for (int bits = 0; bits < 32; ++bits)
                for (int hm = 0; hm < 3; ++hm)
                  for (int pk = 0; pk < 2; ++pk) {
                    FcmSwitches sw;
                    sw.gatherHalf = halfModes[hm];
                    sw.packedInter = pk != 0;
                    const FcmGatherInputs in{(bits & 1) != 0, (bits & 2) != 0, (bits & 4) != 0, FcmInt3{sx, sy, sz}, cells, perWave, (bits & 8) != 0,
                                             (bits & 16) != 0, sw};
                    gather_invariants(in, fcm_choose_gather(in));
                    ++*count;
                  }
          }
}

static void enumerate_tiles(long *count) {
  for (int i = 0; i < kNCells; ++i)
    for (int j = 0; j < kNCells; ++j)
      for (int k = 0; k < kNCells; k += (i == j ? 1 : 5))
        for (int sx = 1; sx <= 16; ++sx)
          for (int sy = 1; sy <= 16; sy += (i == j ? 1 : 3))
            for (int sz = 1; sz <= 16; sz += (i == j ? 1 : 3))
              for (int only8 = 0; only8 < 2; ++only8)
                for (int no9 = 0; no9 < 2; ++no9) {
                  const int c[3] = {kCells[i], kCells[j], kCells[k]}, s[3] = {sx, sy, sz};
                  FcmSwitches sw;
                  sw.noTile9 = no9 != 0;
                  FcmInt3 t{-1, -1, -1};
                  const bool usable = fcm_tiles_usable(c, s, only8 != 0, sw, &t);
                  ++*count;
                  const int td[3] = {t.x, t.y, t.z};
                  bool any = true;
                  for (int a = 0; a < 3; ++a) {
                    // T1: k_fcm_spread_tile: ">= 3 tiles per axis, so a source tile appears at exactly ONE of the steps 0, -1, -2"; stencil_tile:
                    // support <= 2 (edge - 1) <= cells, one wrap; the kernel's E is 8 or 9
                    bool axis = false;
                    for (int e = 4; e <= 9; ++e) {
                      const bool ok = c[a] % e == 0 && c[a] / e >= 3 && s[a] <= 2 * (e - 1) && !(e == 9 && no9) && !(only8 && e != 8);
                      axis = axis || ok;
                      if (usable && e == 8 && ok) CHECK(td[a] == 8, "axis %d of %d cells: edge %d where 8 qualifies", a, c[a], td[a]);
                    }
                    any = any && axis;
                    if (usable) {
                      CHECK(td[a] >= 4 && td[a] <= 9 && c[a] % td[a] == 0 && c[a] / td[a] >= 3 && s[a] <= 2 * (td[a] - 1), "axis %d: %d cells edge %d support %d", a,
                            c[a], td[a], s[a]);
                      CHECK(!(no9 && td[a] == 9) && !(only8 && td[a] != 8), "axis %d: edge %d", a, td[a]);
                    }
                  }
                  CHECK(usable == any, "cells %d %d %d support %d %d %d: usable %d, an edge qualifies on every axis %d", c[0], c[1], c[2], sx, sy, sz, (int)usable, (int)any);
                  if (!usable) CHECK(t.x == -1 && t.y == -1 && t.z == -1, "tdim written for an unusable grid");
                }
}

static void enumerate_spread(long *count) {
  const int Ns[] = {1, 100, 1000, 20000, 200000, 1000000, 2000000};
  const int caps[] = {0, 8, 15, 16, 31, 32, 40, 56, 64};
  const int extra[3][3] = {{20, 24, 28}, {24, 27, 28}, {108, 108, 64}};
  for (int g = 0; g < kNCells + 3; ++g)
    for (int sx = 1; sx <= 16; ++sx)
      for (int sy = 1; sy <= 16; ++sy)
        for (int sz = 1; sz <= 16; ++sz) {
          if (!(sx == sy && sy == sz) && !(sx % 3 == 1 && sy % 3 == 2 && sz % 3 == 0)) continue;   // (every cubic support, and 5 x 5 x 5 others)
          for (int geo = 0; geo < 4; ++geo) {
            const int n = g < kNCells ? kCells[g] : 0;
            const int c[3] = {n ? n : extra[g - kNCells][0], n ? n : extra[g - kNCells][1], n ? n : extra[g - kNCells][2]}, s[3] = {sx, sy, sz};
            FcmSwitches sw;
            sw.noTile9 = (geo & 1) != 0;
            FcmInt3 t{0, 0, 0};
            if (!fcm_tiles_usable(c, s, (geo & 2) != 0, sw, &t)) continue;
            const FcmInt3 nt{c[0] / t.x, c[1] / t.y, c[2] / t.z};
            for (int Ni = 0; Ni < 7; ++Ni)
              for (int opt = 0; opt <= 4; opt += 2)
                for (int ci = 0; ci < 9; ++ci)
                  for (int bits = 0; bits < 16; ++bits) {
                    FcmSwitches w = sw;
                    w.noSpec = (bits & 1) != 0;
                    w.specDense = (bits & 2) != 0;
                    const FcmSpreadInputs in{Ns[Ni], nt, FcmInt3{sx, sy, sz}, t, opt, (bits & 4) != 0, caps[ci], (bits & 8) != 0, w};
                    const FcmSpreadChoice p = fcm_choose_spread(in);
                    ++*count;
                    // S1: k_fcm_spread_tile<W, SLOTS, E, SPEC> is instantiated for W in {2, 4} and E in {kTile, kTileMax}; its layouts hold E nodes per axis
                    CHECK(p.waves == 2 || p.waves == 4, "W %d", p.waves);
                    CHECK(p.edge == ((t.x > 8 || t.y > 8 || t.z > 8) ? 9 : 8), "E %d for tiles %d %d %d", p.edge, t.x, t.y, t.z);
                    if (opt) CHECK(p.waves == opt, "W %d asked %d", p.waves, opt);
                    // (phase B: 3 E weight words per listed particle; a list never holds more entries than the workgroup has threads)
                    CHECK(p.weightWords % (3 * p.edge) == 0 && p.listEntries >= 1 && p.listEntries <= 64 * p.waves && p.listEntries * 3 * p.edge <= p.weightWords,
                          "words %d entries %d", p.weightWords, p.listEntries);
                    // (a workgroup's dynamic LDS holds the final tile sum and stays within a CU's 160 KB; 20 = sizeof(SpEntry))
                    CHECK(fcm_spread_lds_bytes(p, 20) <= 160 * 1024 && fcm_spread_lds_bytes(p, 20) >= sizeof(float) * p.waves * 3 * p.edge * p.edge * p.edge, "lds");
                    // S2: SPEC: static_assert(!SPEC || SLOTS); the round requests kSpecSlots = 8 W slots of each of EIGHT source tiles and lists up to one
                    // record per thread at once (list and weights hold 64 W entries)
                    if (p.spec) {
                      const bool eight = (sx - 2 + t.x) / t.x == 1 && (sy - 2 + t.y) / t.y == 1 && (sz - 2 + t.z) / t.z == 1;
                      CHECK(in.slots && eight && in.cap >= 8 * p.waves && p.listEntries >= 64 * p.waves && (p.waves == 2 || w.specDense) && !w.noSpec,
                            "spec: slots %d eight %d cap %d W %d entries %d", (int)in.slots, (int)eight, in.cap, p.waves, p.listEntries);
                    }
                    // S3: the slab instantiates no SPEC kernel
                    if (!in.allowSpec) CHECK(!p.spec, "spec on the slab");
                  }
          }
        }
}

int main(int argc, char **argv) {
  if (argc >= 2 && !std::strcmp(argv[1], "replay")) return replay();
  if (argc >= 2 && !std::strcmp(argv[1], "enumerate")) {
    long g = 0, t = 0, s = 0;
    enumerate_gather(&g);
    enumerate_tiles(&t);
    enumerate_spread(&s);
    std::printf("enumerated %ld gather inputs, %ld tile geometries, %ld spread inputs: %s (%ld broken)\n", g, t, s,
                failures ? "INVARIANTS BROKEN" : "invariants hold", failures);
    return failures ? 1 : 0;
  }
  std::fprintf(stderr, "usage: fcm_launch_choice replay < rows | enumerate\n");
  return 2;
}
