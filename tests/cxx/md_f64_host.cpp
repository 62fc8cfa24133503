// Stand-alone program over uammd_amd/csrc/md_f64_host.hpp alone (the host logic of the double-precision path A), built with
// -fsanitize=address,undefined by tests/test_md_f64_cpu.py.  It drives
//   - the grid rule on ordinary, collapsed, infinite, zero and NaN boxes,
//   - the pair-parameter processing,
//   - the epoch rule over sequences of builds, up to the overflow of the 32-bit cell entries,
//   - the sort width,
//   - the argument checks with every pointer missing in turn,
//   - the buffer sizes: a host model of the build's three kernels (keys, stable sort, gather + cell tables, padding rows included) and of a
//     traversal's grouped loads writes and reads heap blocks of exactly buffer_bytes(), so an entry too few is a sanitizer report.
// Prints "md_f64_host: ok" and returns 0 when every expectation holds.
#include "../../uammd_amd/csrc/md_f64_host.hpp"

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <numeric>
#include <vector>

using namespace uammd_hip::md64;

static int failures = 0;
#define EXPECT(cond)                                                        \
  do {                                                                      \
    if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } \
  } while (0)

static void grid(double Lx, double Ly, double Lz, int px, int py, int pz, double rc, int cd[3], double Lo[3], int po[3]) {
  const double L[3] = {Lx, Ly, Lz}, c[3] = {rc, rc, rc};
  const int p[3] = {px, py, pz};
  create_grid(L, p, c, cd, Lo, po);
}

static void test_grid() {
  int cd[3], po[3];
  double Lo[3];
  grid(16, 16, 16, 1, 1, 1, 2.5, cd, Lo, po);
  EXPECT(cd[0] == 6 && cd[1] == 6 && cd[2] == 6 && po[0] && po[1] && po[2] && Lo[0] == 16);
  grid(107.7217345, 107.7217345, 107.7217345, 1, 1, 1, 2.5, cd, Lo, po);
  EXPECT(cd[0] == 43 && cd[2] == 43);
  grid(30, 30, 9, 1, 1, 1, 2.5, cd, Lo, po);
  EXPECT(cd[0] == 12 && cd[1] == 12 && cd[2] == 1 && po[2] == 1);
  grid(7, 7, 7, 1, 1, 1, 2.5, cd, Lo, po);
  EXPECT(cd[0] == 1 && cd[1] == 1 && cd[2] == 1);
  const double inf = std::numeric_limits<double>::infinity(), big = std::numeric_limits<double>::max();
  grid(40, inf, 40, 1, 1, 1, 2.5, cd, Lo, po);
  EXPECT(cd[1] == 64 && Lo[1] == 160.0 && po[1] == 0 && po[0] == 1);
  grid(40, big, 40, 1, 1, 1, 2.5, cd, Lo, po);
  EXPECT(cd[1] == 64 && Lo[1] == 160.0 && po[1] == 1);
  grid(40, 40, 0, 1, 1, 1, 2.5, cd, Lo, po);
  EXPECT(cd[2] == 1 && po[2] == 0);
  grid(std::nan(""), 40, 40, 1, 1, 1, 2.5, cd, Lo, po);  // no int value: one cell, no undefined conversion
  EXPECT(cd[0] == 1);
  grid(1e300, 40, 40, 1, 1, 1, 1e-300, cd, Lo, po);
  EXPECT(cd[0] == 1);
  grid(40, 40, 40, 1, 1, 1, 0.0, cd, Lo, po);  // L / 0 = inf
  EXPECT(cd[0] == 1);
}

static void test_params() {
  double p[4];
  process_pair_parameters(2.5, 1.0, 1.0, 0, p);
  EXPECT(p[0] == 6.25 && p[1] == 1.0 && p[2] == 1.0 && p[3] == 0.0);
  process_pair_parameters(2.5, 1.0, 1.0, 1, p);
  const double i6 = (1.0 / 6.25) * (1.0 / 6.25) * (1.0 / 6.25);
  EXPECT(p[3] == 4.0 * i6 * (i6 - 1.0));
  process_pair_parameters(0.0, 0.0, 1.0, 1, p);  // 0 / 0: NaN in, NaN out, nothing else
  EXPECT(p[0] == 0.0 && p[3] != p[3]);
}

static void test_epoch() {
  ValidCell e;
  EXPECT(e.next(1000) && e.validCell == 1000u);
  EXPECT(!e.next(1000) && e.validCell == 2000u);
  EXPECT(!e.next(1000) && e.validCell == 3000u);
  EXPECT(e.next(999) && e.validCell == 999u);  // another N: cleared
  EXPECT(e.next(0) && e.validCell == 0u);
  ValidCell big;
  const int N = 1 << 30;
  EXPECT(big.next(N) && big.validCell == (unsigned)N);
  EXPECT(!big.next(N) && big.validCell == 2u * (unsigned)N);  // entries up to 3N - 1 < 2^32 - 1
  EXPECT(big.next(N) && big.validCell == (unsigned)N);        // 4N would not fit: cleared, back to N
  // entries never wrap: id + validCell stays below 2^32 - 1 over a long run
  ValidCell r;
  const int M = 700000000;
  for (int k = 0; k < 50; ++k) {
    r.next(M);
    EXPECT((unsigned long long)r.validCell + (unsigned long long)M - 1ull < 0xFFFFFFFFull);
  }
  EXPECT(sort_end_bit(0u) == 0 && sort_end_bit(1u) == 1 && sort_end_bit(255u) == 8 && sort_end_bit(256u) == 9 && sort_end_bit(0xFFFFFFFFu) == 32);
}

static void test_checks() {
  int h = 0;
  double pos[4] = {0, 0, 0, 0};
  const double L[3] = {10, 10, 10}, L0[3] = {10, 10, 0}, Lbad[3] = {10, -1, 10}, Linf[3] = {10, std::numeric_limits<double>::infinity(), 10};
  const int per[3] = {1, 1, 1}, cd[3] = {4, 4, 4}, cd0[3] = {0, 4, 4}, cdBig[3] = {1025, 4, 4}, cd2[3] = {4, 4, 0};
  EXPECT(check_update(&h, pos, 1, L, per, cd) == nullptr);
  EXPECT(check_update(&h, pos, 1, L0, per, cd2) == nullptr);
  EXPECT(check_update(&h, nullptr, 0, nullptr, nullptr, nullptr) == nullptr);  // N = 0: a no-op, nothing is looked at
  EXPECT(check_update(nullptr, pos, 1, L, per, cd) != nullptr);
  EXPECT(check_update(&h, nullptr, 1, L, per, cd) != nullptr);
  EXPECT(check_update(&h, pos, 1, nullptr, per, cd) != nullptr);
  EXPECT(check_update(&h, pos, 1, L, nullptr, cd) != nullptr);
  EXPECT(check_update(&h, pos, 1, L, per, nullptr) != nullptr);
  EXPECT(check_update(&h, pos, -1, L, per, cd) != nullptr);
  EXPECT(check_update(&h, pos, 1, L, per, cd0) != nullptr);
  EXPECT(check_update(&h, pos, 1, L, per, cdBig) != nullptr);
  EXPECT(check_update(&h, pos, 1, Lbad, per, cd) != nullptr);
  EXPECT(check_update(&h, pos, 1, Linf, per, cd) != nullptr);
  EXPECT(check_transverse(&h, pos, 1, L, per, kAlgoAuto) == nullptr);
  EXPECT(check_transverse(&h, pos, 3, L, per, kAlgoGeneral) == nullptr);
  EXPECT(check_transverse(&h, pos, 1, L, per, kAlgoScan32) == nullptr);
  EXPECT(check_transverse(&h, pos, 1, L, per, 8) != nullptr);  // the tile kernel is single precision only
  EXPECT(check_transverse(&h, pos, 0, L, per, kAlgoAuto) != nullptr);
  EXPECT(check_transverse(nullptr, pos, 1, L, per, kAlgoAuto) != nullptr);
  EXPECT(check_transverse(&h, nullptr, 1, L, per, kAlgoAuto) != nullptr);
  EXPECT(check_transverse(&h, pos, 1, nullptr, per, kAlgoAuto) != nullptr);
  EXPECT(check_transverse(&h, pos, 1, L, nullptr, kAlgoAuto) != nullptr);
  const int c6[3] = {6, 6, 6}, c4[3] = {6, 4, 6}, c1[3] = {6, 6, 1}, np[3] = {1, 1, 0};
  const double L2[3] = {10, 10, 11};
  EXPECT(scan32_covers(c6, L, per, L, per));
  EXPECT(!scan32_covers(c4, L, per, L, per));
  EXPECT(!scan32_covers(c1, L, per, L, per));
  EXPECT(scan32_covers(c1, L, np, L, np));     // one cell, non periodic
  EXPECT(scan32_covers(c1, L, np, L2, np));    // ... where the side does not matter
  EXPECT(!scan32_covers(c6, L, per, L2, per)); // another box
  EXPECT(!scan32_covers(c6, L, per, L, np));
}

// ---- a host model of the build on blocks of exactly buffer_bytes() ---------------------------------------------------------------------
static unsigned spread10(unsigned i) {
  unsigned x = i & 0x3ffu;
  x = (x | x << 16) & 0x30000ffu;
  x = (x | x << 8) & 0x300f00fu;
  x = (x | x << 4) & 0x30c30c3u;
  x = (x | x << 2) & 0x9249249u;
  return x;
}
static unsigned compact10(unsigned x) {
  x &= 0x9249249u;
  x = (x | x >> 2) & 0x30c30c3u;
  x = (x | x >> 4) & 0x300f00fu;
  x = (x | x >> 8) & 0x30000ffu;
  x = (x | x >> 16) & 0x3ffu;
  return x;
}
static unsigned morton(int cx, int cy, int cz) { return spread10((unsigned)cx) | (spread10((unsigned)cy) << 1) | (spread10((unsigned)cz) << 2); }

static void model_build(int N, const int cd[3], unsigned seed, int nBad) {
  const long long ncells = (long long)cd[0] * cd[1] * cd[2];
  const BufferBytes b = buffer_bytes(N, ncells);
  unsigned *hash = (unsigned *)std::malloc(b.hash);
  int *index = (int *)std::malloc(b.index);
  double *sortPos = (double *)std::malloc(b.sortPos);
  float *sortPos32 = (float *)std::malloc(b.sortPos32);
  unsigned *cellStart = (unsigned *)std::calloc(1, b.cellStart ? b.cellStart : 1);
  int *cellEnd = (int *)std::calloc(1, b.cellEnd ? b.cellEnd : 1);
  unsigned char *cellOutside = (unsigned char *)std::calloc(1, b.cellOutside ? b.cellOutside : 1);
  std::vector<double> pos(4 * (size_t)N);
  ValidCell epoch;
  epoch.next(N);
  epoch.next(N);
  const unsigned maxHash = morton(cd[0] - 1, cd[1] - 1, cd[2] - 1), badKey = maxHash + 1u;
  unsigned s = seed;
  auto rnd = [&]() { s = s * 1664525u + 1013904223u; return s >> 8; };
  for (int i = 0; i < N; ++i) {  // K1
    const int cx = (int)(rnd() % (unsigned)cd[0]), cy = (int)(rnd() % (unsigned)cd[1]), cz = (int)(rnd() % (unsigned)cd[2]);
    for (int k = 0; k < 4; ++k) pos[4 * (size_t)i + k] = i + 0.25 * k;
    hash[i] = i < nBad ? badKey : morton(cx, cy, cz);
    index[i] = i;
  }
  std::vector<int> order(N);  // K2: a stable sort of (key, index) on sort_end_bit(badKey) bits
  std::iota(order.begin(), order.end(), 0);
  const int bits = sort_end_bit(badKey);
  const unsigned mask = bits >= 32 ? 0xFFFFFFFFu : ((1u << bits) - 1u);
  std::stable_sort(order.begin(), order.end(), [&](int a, int c) { return (hash[a] & mask) < (hash[c] & mask); });
  {
    std::vector<unsigned> h2(N);
    for (int i = 0; i < N; ++i) h2[i] = hash[order[i]];
    for (int i = 0; i < N; ++i) { hash[i] = h2[i]; index[i] = order[i]; }
  }
  for (int id = 0; id < N + kPadRows; ++id) {  // K3 + K4, thread by thread
    if (id >= N) {
      for (int k = 0; k < 4; ++k) { sortPos[4 * (size_t)id + k] = 0.0; sortPos32[4 * (size_t)id + k] = 0.f; }
      continue;
    }
    for (int k = 0; k < 4; ++k) {
      sortPos[4 * (size_t)id + k] = pos[4 * (size_t)index[id] + k];
      sortPos32[4 * (size_t)id + k] = (float)pos[4 * (size_t)index[id] + k];
    }
    const unsigned h = hash[id];
    if (h > maxHash) continue;
    auto lin = [&](unsigned key) { return (long long)compact10(key) + cd[0] * ((long long)compact10(key >> 1) + (long long)cd[1] * compact10(key >> 2)); };
    const long long icell = lin(h);
    EXPECT(icell >= 0 && icell < ncells);
    cellOutside[icell] = 1;
    const unsigned hPrev = id > 0 ? hash[id - 1] : 0u;
    if (id == 0 || hPrev != h) {
      cellStart[icell] = (unsigned)id + epoch.validCell;
      if (id > 0) cellEnd[lin(hPrev)] = id;
    }
    if (id == N - 1 || hash[id + 1] > maxHash) cellEnd[icell] = id + 1;
  }
  // what the tables must say: every particle with a cell inside its cell's range, the ranges disjoint and covering them all
  long long covered = 0;
  for (long long c = 0; c < ncells; ++c) {
    if (cellStart[c] < epoch.validCell) continue;
    const int first = (int)(cellStart[c] - epoch.validCell), last = cellEnd[c];
    EXPECT(first < last && last <= N - nBad);
    covered += last - first;
    // a traversal's grouped loads: 4 double rows / 8 image rows from every group's first row
    for (int j = first; j < last; j += 4) { volatile double x = sortPos[4 * ((size_t)j + 3) + 3]; (void)x; }
    for (int j = first; j < last; j += 8) { volatile float x = sortPos32[4 * ((size_t)j + 7) + 3]; (void)x; }
  }
  EXPECT(covered == N - nBad);
  for (int id = 0; id + 1 < N; ++id) EXPECT(hash[id] <= hash[id + 1]);
  std::free(hash); std::free(index); std::free(sortPos); std::free(sortPos32); std::free(cellStart); std::free(cellEnd); std::free(cellOutside);
}

int main() {
  test_grid();
  test_params();
  test_epoch();
  test_checks();
  const int grids[][3] = {{1, 1, 1}, {6, 6, 6}, {13, 8, 18}, {12, 12, 1}, {16, 1, 16}, {5, 7, 64}};
  const int sizes[] = {1, 2, 7, 8, 9, 129, 1000};
  unsigned seed = 1;
  for (const auto &g : grids)
    for (int N : sizes)
      for (int nBad : {0, 1, N}) model_build(N, g, seed++, std::min(nBad, N));
  if (failures) { std::printf("md_f64_host: %d expectations FAILED\n", failures); return 1; }
  std::printf("md_f64_host: ok\n");
  return 0;
}
