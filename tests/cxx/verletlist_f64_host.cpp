// Stand-alone program over uammd_amd/csrc/verletlist_f64_host.hpp alone (the host logic of the double-precision Verlet list), built with
// -fsanitize=address,undefined by tests/test_md2_f64_cpu.py.  It drives
//   - the rebuild decision over every sequence of {nothing, box, periodicity, cut-off, N, forced, multiplier} changes up to length four,
//     against a model written from the reference's needsRebuild,
//   - the threshold rule (multiplier 1 rebuilds on every update),
//   - the capacity growth against the reference's retry loop,
//   - the buffer sizes: a host model of the fill (count every neighbour, store below the capacity) and of the traversal's reads on heap
//     blocks of exactly buffer_bytes(), so an entry too few is a sanitizer report,
//   - the argument checks.
// Prints "verletlist_f64_host: ok" and returns 0 when every expectation holds.
#include "../../uammd_amd/csrc/verletlist_f64_host.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace uammd_hip::vl64;

static int failures = 0;
#define EXPECT(cond)                                                        \
  do {                                                                      \
    if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } \
  } while (0)

// ---- rebuild decisions ------------------------------------------------------------------------------------------------------------
struct Input {
  double L[3];
  int periodic[3];
  double cutOff;
  int N;
};
// the reference's needsRebuild, restated independently: what it remembers is exactly the input of the last rebuild
struct Model {
  bool have = false, forced = true;
  Input last{};
  double multiplier = 1.08;
  bool decide(const Input &in) {  // true = rebuild without looking at the drift
    if (forced) { forced = false; return true; }
    if (!have) return true;
    if (std::memcmp(in.L, last.L, sizeof in.L) != 0) return true;
    for (int k = 0; k < 3; ++k)
      if (in.periodic[k] != last.periodic[k]) return true;
    if (in.cutOff != last.cutOff || in.N != last.N) return true;
    return (multiplier * last.cutOff - last.cutOff) / 2.0 <= 1e-6;
  }
};

enum Change { NONE, BOX, PERIODIC, CUTOFF, NUMBER, FORCED, MULTIPLIER_ONE, MULTIPLIER_BACK, DRIFTED, NCHANGES };

static void run_sequence(const int *seq, int len) {
  State s;
  Model m;
  Input in{{10.0, 11.0, 12.0}, {1, 1, 1}, 2.5, 100};
  int expectedSteps = 0;
  for (int t = -1; t < len; ++t) {  // t = -1: the first update of a fresh list
    bool drift = false;
    if (t >= 0) switch (seq[t]) {
        case BOX: in.L[1] += 0.5; break;
        case PERIODIC: in.periodic[2] = !in.periodic[2]; break;
        case CUTOFF: in.cutOff *= 1.1; break;
        case NUMBER: in.N += 7; break;
        case FORCED: s.forceNextRebuild = true; m.forced = true; break;
        case MULTIPLIER_ONE: s.forceNextRebuild = true; s.verletRadiusMultiplier = 1.0; m.forced = true; m.multiplier = 1.0; break;
        case MULTIPLIER_BACK: s.forceNextRebuild = true; s.verletRadiusMultiplier = 1.08; m.forced = true; m.multiplier = 1.08; break;
        case DRIFTED: drift = true; break;
        default: break;
      }
    const bool want = m.decide(in);
    const Decision d = needs_rebuild(s, in.L, in.periodic, in.cutOff, in.N);
    EXPECT((d == REBUILD) == want);
    const bool rebuild = d == REBUILD || drift;
    if (rebuild) {
      begin_rebuild(s, in.L, in.periodic, in.cutOff, in.N);
      m.have = true;
      m.last = in;
      expectedSteps = 0;
      EXPECT(s.storedN == in.N && s.N == in.N && s.currentCutOff == in.cutOff && s.haveBox && s.stepsSinceLastUpdate == 0);
      EXPECT(list_radius(s) == in.cutOff * s.verletRadiusMultiplier);
    }
    end_update(s);
    ++expectedSteps;
    EXPECT(s.stepsSinceLastUpdate == expectedSteps);
    EXPECT(!s.forceNextRebuild);
  }
}

static void test_rebuild_sequences() {
  int seq[4];
  long count = 0;
  for (int len = 0; len <= 4; ++len) {
    long total = 1;
    for (int k = 0; k < len; ++k) total *= NCHANGES;
    for (long c = 0; c < total; ++c) {
      long r = c;
      for (int k = 0; k < len; ++k) { seq[k] = (int)(r % NCHANGES); r /= NCHANGES; }
      run_sequence(seq, len);
      ++count;
    }
  }
  EXPECT(count == 1 + 9 + 81 + 729 + 6561);
}

static void test_threshold() {
  EXPECT(drift_threshold(1.08, 2.5) == (1.08 * 2.5 - 2.5) / 2.0);
  EXPECT(drift_threshold(1.08, 2.5) > 0.09 && drift_threshold(1.08, 2.5) < 0.11);
  EXPECT(drift_threshold(1.0, 2.5) == 0.0);
  State s;
  const double L[3] = {9, 9, 9};
  const int p[3] = {1, 1, 1};
  s.verletRadiusMultiplier = 1.0;
  for (int t = 0; t < 5; ++t) {  // multiplier 1: threshold 0 <= 1e-6, every update rebuilds
    EXPECT(needs_rebuild(s, L, p, 2.5, 10) == REBUILD);
    begin_rebuild(s, L, p, 2.5, 10);
    end_update(s);
  }
  s.verletRadiusMultiplier = 1.0 + 1e-6;  // (1e-6 * 2.5) / 2 = 1.25e-6 > 1e-6: the drift decides
  EXPECT(needs_rebuild(s, L, p, 2.5, 10) == KEEP_UNLESS_DRIFT);
  s.verletRadiusMultiplier = 1.0 + 7e-7;  // 8.75e-7 <= 1e-6
  EXPECT(needs_rebuild(s, L, p, 2.5, 10) == REBUILD);
}

static void test_capacity() {
  for (int largest = 0; largest < 400; ++largest) {
    State s;
    int ref = kInitialCapacity;  // the reference: fill, and while some particle has >= capacity neighbours, capacity += 32
    while (largest >= ref) ref += kCapacityStep;
    const bool grew = grow_capacity(s, largest);
    EXPECT(s.maxNeighboursPerParticle == ref && grew == (ref != kInitialCapacity));
    EXPECT(largest < s.maxNeighboursPerParticle && s.maxNeighboursPerParticle % 32 == 0);
    EXPECT(!grow_capacity(s, largest));  // a second look at the same count changes nothing
  }
  State s;
  EXPECT(!grow_capacity(s, 31) && s.maxNeighboursPerParticle == 32);
  EXPECT(grow_capacity(s, 32) && s.maxNeighboursPerParticle == 64);
  EXPECT(grow_capacity(s, 95) && s.maxNeighboursPerParticle == 96);
  EXPECT(grow_capacity(s, 300) && s.maxNeighboursPerParticle == 320);
}

// A host model of fill + traversal on blocks of exactly the handle's sizes: particle i has counts[i] neighbours.
static void model_fill(int N, const std::vector<int> &counts) {
  State s;
  s.N = N;
  for (int pass = 0;; ++pass) {
    EXPECT(pass < 2);  // one refill at the most
    const int capacity = s.maxNeighboursPerParticle;
    const BufferBytes b = buffer_bytes(N, capacity);
    EXPECT(b.neighbourList == sizeof(int) * (size_t)N * capacity && b.storedPos == 32 * (size_t)N && b.sortPos == 32 * (size_t)N);
    EXPECT(b.flags == 8);
    int *list = (int *)std::malloc(b.neighbourList ? b.neighbourList : 1);
    int *nn = (int *)std::malloc(b.numberNeighbours ? b.numberNeighbours : 1);
    std::memset(list, 0xff, b.neighbourList);
    int largest = 0;
    for (int i = 0; i < N; ++i) {
      int cnt = 0;
      for (int c = 0; c < counts[i]; ++c) {
        if (may_store(cnt, i, N, capacity)) list[entry_offset(cnt, i, N)] = c;
        EXPECT(may_store(cnt, i, N, capacity) == (cnt < capacity));
        ++cnt;
      }
      nn[i] = cnt;
      if (cnt >= capacity && cnt > largest) largest = cnt;
    }
    if (!grow_capacity(s, largest)) {
      long sum = 0;
      for (int i = 0; i < N; ++i) {  // the traversal: entries k < numberNeighbours[i], nothing else
        EXPECT(nn[i] == counts[i] && nn[i] < capacity);
        for (int k = 0; k < nn[i]; ++k) sum += list[entry_offset(k, i, N)] == k;
        if (nn[i] < capacity) EXPECT(list[entry_offset(nn[i], i, N)] == -1);  // never written
      }
      long want = 0;
      for (int i = 0; i < N; ++i) want += counts[i];
      EXPECT(sum == want);
      std::free(list);
      std::free(nn);
      break;
    }
    std::free(list);
    std::free(nn);
  }
}

static void test_sizes() {
  model_fill(0, {});
  model_fill(1, {1});
  model_fill(1, {31});
  model_fill(1, {32});
  model_fill(3, {5, 95, 96});
  std::vector<int> c(257);
  for (int i = 0; i < 257; ++i) c[i] = 1 + (i * 37) % 301;
  model_fill(257, c);
  EXPECT(!may_store(-1, 0, 4, 32) && !may_store(32, 0, 4, 32) && !may_store(0, 4, 4, 32) && !may_store(0, -1, 4, 32) && may_store(31, 3, 4, 32));
  EXPECT(entry_offset(95, 6399, 6400) == (size_t)95 * 6400 + 6399);
  EXPECT(buffer_bytes(70000000, 64).neighbourList == (size_t)4 * 70000000 * 64);  // beyond 2^32 bytes: sized in size_t
}

static void test_checks() {
  const double L[3] = {9, 9, 9};
  const int p[3] = {1, 1, 1};
  int dummy = 0;
  EXPECT(check_update(nullptr, &dummy, 4, L, p, 2.5, 1.08) != nullptr);
  EXPECT(std::strstr(check_update(nullptr, &dummy, 4, L, p, 2.5, 1.08), "null handle"));
  EXPECT(check_update(&dummy, &dummy, -1, L, p, 2.5, 1.08) != nullptr);
  EXPECT(check_update(&dummy, nullptr, 4, L, p, 2.5, 1.08) != nullptr);
  EXPECT(check_update(&dummy, &dummy, 4, nullptr, p, 2.5, 1.08) != nullptr);
  EXPECT(check_update(&dummy, &dummy, 4, L, nullptr, 2.5, 1.08) != nullptr);
  EXPECT(std::strstr(check_update(&dummy, &dummy, 4, L, p, 0.0, 1.08), "positive"));
  EXPECT(std::strstr(check_update(&dummy, &dummy, 4, L, p, -1.0, 1.08), "positive"));
  EXPECT(check_update(&dummy, &dummy, 4, L, p, std::strtod("nan", nullptr), 1.08) != nullptr);
  EXPECT(std::strstr(check_update(&dummy, &dummy, 4, L, p, 2.5, 0.99), "multiplier"));
  EXPECT(check_update(&dummy, &dummy, 4, L, p, 2.5, 1.0) == nullptr);
  EXPECT(check_update(&dummy, nullptr, 0, L, p, 2.5, 1.08) == nullptr);  // N = 0 needs no positions
  EXPECT(check_multiplier(nullptr, 1.08) != nullptr && check_multiplier(&dummy, 0.5) != nullptr && check_multiplier(&dummy, 1.0) == nullptr);
  EXPECT(check_multiplier(&dummy, std::strtod("nan", nullptr)) != nullptr);
}

int main() {
  test_rebuild_sequences();
  test_threshold();
  test_capacity();
  test_sizes();
  test_checks();
  if (failures) {
    std::printf("verletlist_f64_host: %d expectation(s) failed\n", failures);
    return 1;
  }
  std::printf("verletlist_f64_host: ok\n");
  return 0;
}
