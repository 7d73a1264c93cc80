// The planning of hmj_window_device (hashmergejoin_amd/csrc/hmj_winplan.h) on its own: the geometry and the carry levels for
// every boundary size, what every function writes, and the cut of a call's functions into launches.  No HIP, no library:
// tests/test_winplan_cpu.py builds this file with g++, plain and under AddressSanitizer + UBSan, and runs both.  The
// program prints the kernels' constants P, G and T, which that test compares with the literals of tests/test_window_gpu.py.
#include <cstdio>
#include <initializer_list>

#include "../../hashmergejoin_amd/csrc/hmj_winplan.h"

using namespace hmj_host;

static int failures = 0;
#define CHECK(cond)                                                     \
  do {                                                                  \
    if (!(cond)) {                                                      \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);     \
      failures++;                                                       \
    }                                                                   \
  } while (0)

static void check_grid(uint64_t n) {
  const WinGrid g = win_grid(n);
  CHECK(g.words * 64 >= n && (n == 0 || (g.words - 1) * 64 < n));
  CHECK(g.ranges * kWinRange >= n && (n == 0 || (g.ranges - 1) * kWinRange < n));
  CHECK(g.ranges * kWinChunks >= g.words);
  CHECK(g.tiles * kWinCarryTile >= g.ranges && (g.ranges == 0 || (g.tiles - 1) * kWinCarryTile < g.ranges));
  // every wave of a walk has a range or lies behind the rows; the same for the words
  CHECK((uint64_t)g.walk_blocks * (kWinThreads / 64) >= g.ranges && (g.ranges == 0 || ((uint64_t)g.walk_blocks - 1) * (kWinThreads / 64) < g.ranges));
  CHECK((uint64_t)g.word_blocks * (kWinThreads / 64) >= g.words && (g.words == 0 || ((uint64_t)g.word_blocks - 1) * (kWinThreads / 64) < g.words));
  // the levels: nothing to carry into the only range; one tile needs no totals; the top scan holds every total
  CHECK(g.levels <= kWinTopLevel);
  CHECK((g.levels == 0) == (g.ranges <= 1));
  CHECK((g.levels == kWinTopLevel) == (g.tiles > 1));
  if (g.levels == kWinTopLevel) {
    CHECK(g.top_per >= 1 && g.top_per <= kWinCarryPer);
    CHECK((uint64_t)g.top_per * kWinTopThreads >= g.tiles);
  } else {
    CHECK(g.top_per == 0);
  }
}

static void check_chunks(const uint32_t* ops, uint32_t n_fns) {
  WinChunk chunks[HMJ_MAX_WINDOW_FNS];
  const uint32_t n = win_chunks(ops, n_fns, chunks);
  CHECK(n <= n_fns && (n_fns == 0 || n >= 1));
  uint32_t seen[HMJ_MAX_WINDOW_FNS] = {0};
  uint32_t last_cls = WIN_CLASS_RANK;
  for (uint32_t q = 0; q < n; q++) {
    CHECK(chunks[q].k >= 1 && chunks[q].k <= kWinLaunch);
    CHECK(chunks[q].cls >= last_cls);  // the ranking launches first
    last_cls = chunks[q].cls;
    for (uint32_t a = 0; a < chunks[q].k; a++) {
      const uint32_t f = chunks[q].fn[a];
      CHECK(f < n_fns);
      if (f >= n_fns) continue;
      CHECK(win_class(ops[f]) == chunks[q].cls);
      CHECK(a == 0 || chunks[q].fn[a - 1] < f);  // the call's order inside a launch
      seen[f]++;
    }
  }
  for (uint32_t f = 0; f < n_fns; f++) CHECK(seen[f] == 1);
}

int main() {
  const uint64_t P = kWinRange, G = kWinGroup, T = kWinCarryTile;
  std::printf("P %llu\nG %llu\nT %llu\n", (unsigned long long)P, (unsigned long long)G, (unsigned long long)T);
  CHECK(P == 64 * kWinChunks && G == P * (kWinThreads / 64) && T == kWinThreads * kWinCarryPer);
  const uint64_t sizes[] = {0, 1, 2, 63, 64, 65, P - 1, P, P + 1, G - 1, G, G + 1, 5000, 3 * G + 5, P * T - 1, P * T, P * T + 1,
                            (1ull << 20), (1ull << 22) + 77, (1ull << 24), (1ull << 26), (1ull << 31) + 1, kWinMaxRows - 1, kWinMaxRows};
  for (uint64_t n : sizes) check_grid(n);
  CHECK(win_grid(0).levels == 0 && win_grid(P).levels == 0 && win_grid(P + 1).levels == 1);
  CHECK(win_grid(P * T).levels == 1 && win_grid(P * T + 1).levels == kWinTopLevel);
  const WinGrid big = win_grid((1ull << 22) + 77);
  std::printf("levels(2^22+77) %u\ntop %u\n", big.levels, kWinTopLevel);
  CHECK(big.levels == kWinTopLevel && big.tiles == 5 && big.top_per == 1);
  CHECK(win_grid(kWinMaxRows).top_per == 4);

  // what a function writes
  for (uint32_t type = HMJ_TYPE_I8; type <= HMJ_TYPE_F64; type++) {
    for (uint32_t op = HMJ_WIN_ROW_NUMBER; op <= HMJ_WIN_CUM_COUNT; op++) CHECK(win_out_type(type, op) == HMJ_TYPE_U64 && win_never_null(op));
    const uint32_t sum = type >= HMJ_TYPE_F32 ? HMJ_TYPE_F64 : (type <= HMJ_TYPE_I64 ? HMJ_TYPE_I64 : HMJ_TYPE_U64);
    CHECK(win_out_type(type, HMJ_WIN_CUM_SUM) == sum && win_out_width(type, HMJ_WIN_CUM_SUM) == 8);
    for (uint32_t op : {HMJ_WIN_CUM_MIN, HMJ_WIN_CUM_MAX, HMJ_WIN_LAG, HMJ_WIN_LEAD}) {
      CHECK(win_out_type(type, op) == type && win_out_width(type, op) == width_of(type) && !win_never_null(op));
    }
  }
  for (uint32_t op = 0; op <= HMJ_WIN_LEAD; op++) {
    CHECK(win_known_op(op));
    CHECK(win_reads_values(op) == (op >= HMJ_WIN_CUM_SUM));
    CHECK(win_reads_validity(op) == (op >= HMJ_WIN_CUM_COUNT));
    CHECK((win_class(op) == WIN_CLASS_SCAN) == (op >= HMJ_WIN_CUM_COUNT && op <= HMJ_WIN_CUM_MAX));
  }
  CHECK(!win_known_op(HMJ_WIN_LEAD + 1) && !win_known_op(~0u));

  // the launches: every function once, for every op alone, all ops in turn up to the cap, and one class only
  uint32_t ops[HMJ_MAX_WINDOW_FNS];
  for (uint32_t n_fns = 1; n_fns <= HMJ_MAX_WINDOW_FNS; n_fns++) {
    for (uint32_t shift = 0; shift < 9; shift++) {
      for (uint32_t f = 0; f < n_fns; f++) ops[f] = (f * 5 + shift) % 9;
      check_chunks(ops, n_fns);
    }
    for (uint32_t f = 0; f < n_fns; f++) ops[f] = HMJ_WIN_CUM_SUM;
    check_chunks(ops, n_fns);
    for (uint32_t f = 0; f < n_fns; f++) ops[f] = HMJ_WIN_LAG;
    check_chunks(ops, n_fns);
  }
  WinChunk chunks[HMJ_MAX_WINDOW_FNS];
  const uint32_t six[6] = {HMJ_WIN_CUM_SUM, HMJ_WIN_CUM_SUM, HMJ_WIN_CUM_SUM, HMJ_WIN_CUM_SUM, HMJ_WIN_CUM_SUM, HMJ_WIN_CUM_SUM};
  CHECK(win_chunks(six, 6, chunks) == 2 && chunks[0].k == 4 && chunks[1].k == 2 && chunks[1].fn[0] == 4);  // the 5th of 6 opens a launch

  if (failures) {
    std::printf("%d checks failed\n", failures);
    return 1;
  }
  std::printf("all window plan cases passed\n");
  return 0;
}
