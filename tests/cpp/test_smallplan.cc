// The planning arithmetic of the ordered small-build join and of the device sort (hashmergejoin_amd/csrc/hmj_smallplan.h) on
// its own: the rank-run cut and level, the cost model's gate, the varying digits of a mask, the LSD digit split, the device
// sort's MSD window and the digits of both chains of slab passes.  No HIP, no library: tests/test_smallplan_cpu.py builds
// this file with g++, plain and under AddressSanitizer + UBSan, and runs both.
#include <cmath>
#include <cstdio>

#include "../../hashmergejoin_amd/csrc/hmj_smallplan.h"

using namespace hmj_host;

static int failures = 0;
#define CHECK(cond)                                                     \
  do {                                                                  \
    if (!(cond)) {                                                      \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);     \
      failures++;                                                       \
    }                                                                   \
  } while (0)

static bool near(double a, double b) { return std::fabs(a - b) <= 1e-12 * std::fabs(b); }

// what hmj_create fills in: gtable.hip's rank_sort_max_run for the levels -1 .. 2; every other knob at hmj_ctx's default
static LdsSortKnobs lds_knobs() {
  LdsSortKnobs k;
  k.max_run[0] = 512;
  k.max_run[1] = 2048;
  k.max_run[2] = 4096;
  k.max_run[3] = 8192;
  return k;
}
static RankRunKnobs run_knobs(int max_cut) {
  RankRunKnobs k;
  k.max_cut = max_cut;
  k.lds = lds_knobs();
  return k;
}

// {n_build, n_probe, max_cut, fits, tb, level}: tests/test_gpu_join.py's restatement, for every (nb, npb) of
// test_ordered_small_build_side_sorts_rank_payload_composites (max_cut = 10) and of
// test_rank_runs_in_the_larger_workgroup_shapes (max_cut = 0), generated with
//   r = _rank_runs_cut(nb, npb, max_cut=mc); (nb, npb, mc, r is not None, r[0] if r else 0, r[1] if r else 0)
static const long long kRankRuns[][6] = {
    {1, 5000, 10, 0, 0, 0},
    {7, 70000, 10, 1, 3, 0},
    {1000, 300001, 10, 1, 0, -1},
    {5000, 700000, 10, 1, 0, -1},
    {60000, 8388608, 10, 1, 0, -1},
    {1000, 200000, 10, 1, 0, -1},
    {1000, 400001, 10, 1, 0, 0},
    {3000, 4500000, 10, 1, 0, 0},
    {3001, 1500000, 10, 1, 0, 0},
    {4000, 1200000, 10, 1, 0, -1},
    {300, 5000, 10, 0, 0, 0},
    {2000, 700000, 10, 1, 0, 0},
    {2000, 600001, 10, 1, 0, -1},
    {1500, 500000, 10, 1, 0, -1},
    {3000, 400000, 10, 1, 0, -1},
    {4000, 2200001, 10, 1, 0, 0},
    {300, 4194304, 10, 1, 4, 0},
    {300, 4194227, 10, 1, 4, 0},
    {500, 3000001, 10, 1, 2, 0},
    {37, 1048576, 10, 1, 5, 0},
    {300, 4194304, 10, 1, 4, 0},
    {100, 2097152, 10, 1, 4, 0},
    {300000, 8388608, 10, 1, -1, -1},
    {300001, 8388613, 10, 1, -1, -1},
    {600000, 16777216, 10, 1, -2, -1},
    {280000, 5000000, 10, 1, -1, -1},
    {300, 1048576, 0, 1, 0, 1},
    {200, 1048897, 0, 1, 0, 2},
    {310, 1048576, 0, 1, 0, 1},
    {150, 1048576, 0, 1, 0, 2},
    {100, 1048576, 0, 0, 0, 0},
};

static void test_rank_runs_fit() {
  for (const auto& r : kRankRuns) {
    int tb = 99, level = 99;
    const bool fit = rank_runs_fit(run_knobs((int)r[2]), (uint64_t)r[0], (uint64_t)r[1], &tb, &level);
    CHECK(fit == (r[3] != 0));
    if (fit) CHECK(tb == r[4] && level == r[5]);
    if (!fit || tb != r[4] || level != r[5]) std::printf("  rank_runs_fit(%lld, %lld, max_cut %lld) -> %d (%d, %d)\n", r[0], r[1], r[2], (int)fit, tb, level);
  }
  // the switches: no rank runs, no slab passes
  int tb, level;
  RankRunKnobs off = run_knobs(10);
  off.rank_runs_mode = false;
  CHECK(!rank_runs_fit(off, 7, 70000, &tb, &level) && tb == 0 && level == 0);
  off = run_knobs(10);
  off.slab_mode = false;
  CHECK(!rank_runs_fit(off, 7, 70000, &tb, &level));
  // without the wave shape a whole run of ~300 rows takes the 256-thread workgroup
  RankRunKnobs no_wave = run_knobs(10);
  no_wave.rank_runs_wave = false;
  CHECK(rank_runs_fit(no_wave, 1000, 300001, &tb, &level) && tb == 0 && level == 0);
  CHECK(rank_runs_rested(0, 0, 3) && !rank_runs_rested(1, 0, 0) && rank_runs_rested(0, 5, 0) && rank_runs_rested(0, 5, -1) && !rank_runs_rested(0, 5, 2));
}

// the four shapes of the gate loop of test_ordered_small_build_side_sorts_rank_payload_composites, default executor: a
// fan-out below 128 is not eligible; fan-outs of 300 and 140 over joins too small to repay the fixed cost are refused by the
// model; thousands of rows per key over 2^23 probe rows are admitted.  gtable_sort_cooldown is not the gate's to read.
static void test_gate() {
  SmallOrderedKnobs k;
  k.runs = run_knobs(10);
  const OrderedCostModel m;
  const struct {
    uint64_t nb, np;
    SmallGate want;
  } cases[4] = {{50000, 600000, SmallGate::NotEligible}, {1000, 300000, SmallGate::RefusedByModel},
                {60000, 1u << 23, SmallGate::RefusedByModel}, {1000, 1u << 23, SmallGate::Eligible}};
  for (const auto& cs : cases) {
    SmallOrderedCooldowns cool;
    const SmallGateResult g = small_ordered_gate(k, m, cs.nb, cs.np, true, cool);
    CHECK(g.verdict == cs.want);
    int tb = 0, level = 0;
    const bool fit = rank_runs_fit(k.runs, cs.nb, cs.np, &tb, &level);
    if (g.verdict != SmallGate::NotEligible) CHECK(g.fit == fit && g.run_tb == tb && g.run_level == level);
    cool.gtable_sort = 5;
    CHECK(small_ordered_gate(k, m, cs.nb, cs.np, true, cool).verdict == cs.want);
    CHECK(small_ordered_gate(k, m, cs.nb, cs.np, false, cool).verdict == SmallGate::NotEligible);  // not an ordered join
  }
  // the model switched off (HMJ_GTABLE_SORT_FANOUT=1): every fan-out from 1 on is eligible
  k.gtable_sort_fanout = 1;
  for (const auto& cs : cases) CHECK(small_ordered_gate(k, m, cs.nb, cs.np, true, SmallOrderedCooldowns()).verdict == SmallGate::Eligible);
  k.available = false;
  CHECK(small_ordered_gate(k, m, 1000, 1u << 23, true, SmallOrderedCooldowns()).verdict == SmallGate::NotEligible);
}

static void test_varying_digits() {
  CHECK(varying_digits(0) == 0);
  CHECK(varying_digits(~0ull) == 0xFFu);
  for (int d = 0; d < 8; d++)
    for (int b = 0; b < 8; b += 7) CHECK(varying_digits(1ull << (8 * d + b)) == (1u << d));  // the lowest and the highest bit of digit d
  CHECK(varying_digits(0x0000FF0000000100ull) == ((1u << 1) | (1u << 5)));
}

static void test_lsd_split() {
  for (int total = 1; total <= 64; total++) {
    const int passes = lsd_passes(total, 9);
    CHECK(passes == (total + 8) / 9);  // minimal: one pass fewer holds at most 9 (passes - 1) < total bits
    CHECK(9 * (passes - 1) < total);
    int sum = 0;
    for (int i = 0; i < passes; i++) {
      const int bits = lsd_digit_bits(total, passes, i);
      CHECK(bits >= 1 && bits <= 9);
      if (i) CHECK(bits <= lsd_digit_bits(total, passes, i - 1));  // the earlier passes take the extra bit
      sum += bits;
    }
    CHECK(sum == total);
  }
}

// n = 2^22 + 4099 rows, the context's defaults (window of at most 18 bits, partitions of at most 1200 rows on average, levels
// 0 .. 2).  Derived on paper from the loop: the window widens bit by bit until n * dens / 2^TB <= 1200.
static void test_sort_msd_window() {
  const uint64_t n = (1ull << 22) + 4099;
  const LdsSortKnobs lds = lds_knobs();
  // uniform 64-bit keys: the sample sees every bit vary, nothing exact is known.  hi = 64, dens = 1; n / 2^11 = 2050 > 1200,
  // n / 2^12 = 1025: TB = 12; 1025 + 8 * 32.02 + 24 = 1305 <= 2048: level 0
  SortMsdWindow w = sort_msd_window(n, ~0ull, ~0ull, 0, ~0ull, 18, 1200.0, 2, lds, 9);
  CHECK(w.ok && w.hi == 64 && w.TB == 12 && w.level == 0 && w.dens == 1.0 && near(w.mean, (double)n / 4096.0));
  // 63-bit keys: the sample never saw bit 63 vary -> half of the top digit is in use, dens = 2: one more bit, TB = 13
  w = sort_msd_window(n, ~0ull, ~0ull >> 1, 0, ~0ull, 18, 1200.0, 2, lds, 9);
  CHECK(w.ok && w.hi == 64 && w.TB == 13 && w.level == 0 && w.dens == 2.0 && near(w.mean, 2.0 * (double)n / 8192.0));
  // a permutation of 0 .. n - 1: exact, the keys differ in bits 0 .. 22 -> hi = 23.  The values of the top TB bits in use:
  // ((n - 1) >> (23 - TB)) + 1 -- TB = 12: 2051, mean n / 2051 = 2047 > 1200; TB = 13: 4101, mean 1023.75: TB = 13, level 0
  w = sort_msd_window(n, (1ull << 23) - 1, 0, 0, n - 1, 18, 1200.0, 2, lds, 9);
  CHECK(w.ok && w.hi == 23 && w.TB == 13 && w.level == 0 && near(w.dens, 8192.0 / 4101.0) && near(w.mean, (double)n / 4101.0));
  // a window capped at 9 bits: partitions of 8200 rows outgrow the largest sort (8200 + 8 * 90.6 + 24 > 8192)
  w = sort_msd_window(n, ~0ull, ~0ull, 0, ~0ull, 9, 1200.0, 2, lds, 9);
  CHECK(!w.ok && w.TB == 9 && w.level == 3);
  // ... at 10 bits they take the 1024-thread sort, which a context held to level 1 does not have
  w = sort_msd_window(n, ~0ull, ~0ull, 0, ~0ull, 10, 1200.0, 2, lds, 9);
  CHECK(w.ok && w.TB == 10 && w.level == 2);
  CHECK(!sort_msd_window(n, ~0ull, ~0ull, 0, ~0ull, 10, 1200.0, 1, lds, 9).ok);
  // one distinct key, two distinct keys in bit 0: no window of two bits
  CHECK(!sort_msd_window(n, 0, 0, 5, 5, 18, 1200.0, 2, lds, 9).ok);
  w = sort_msd_window(n, 1, 1, 4, 5, 18, 1200.0, 2, lds, 9);
  CHECK(!w.ok && w.TB == 0 && w.hi == 1);
}

static void test_chain_digits() {
  // the device sort on a permutation of 0 .. n - 1, n = 2^22 + 77: exact, bits 0 .. 22 differ -> digits of 8 + 8 + 7 bits; the
  // top one holds (n - 1) >> 16 = 64, so 65 of its 128 values
  const uint64_t n = (1ull << 22) + 77;
  ChainDigit dg[8];
  int nd = sort_chain_digits((1ull << 23) - 1, 0, 0, n - 1, dg);
  CHECK(nd == 3);
  CHECK(dg[0].shift == 0 && dg[0].bits == 8 && dg[0].dens == 1.0);
  CHECK(dg[1].shift == 8 && dg[1].bits == 8 && dg[1].dens == 1.0);
  CHECK(dg[2].shift == 16 && dg[2].bits == 7 && near(dg[2].dens, 128.0 / 65.0));
  // sampled only, 63-bit keys: eight digits of eight bits, the top one half full
  nd = sort_chain_digits(~0ull, ~0ull >> 1, 0, ~0ull, dg);
  CHECK(nd == 8);
  for (int d = 0; d < 8; d++) CHECK(dg[d].shift == 8 * d && dg[d].bits == 8 && dg[d].dens == (d == 7 ? 2.0 : 1.0));
  // exact, digits 1 and 6 with a gap inside digit 6 (bits 48 .. 50 and 55: 4 of 8 bits vary, 200 of the 256 values between
  // the extremes)
  nd = sort_chain_digits(0x008700000000FF00ull, 0, 0, 0x00C7000000000000ull, dg);
  CHECK(nd == 2 && dg[0].shift == 8 && dg[0].bits == 8 && dg[1].shift == 48 && dg[1].bits == 8 && dg[1].dens == 16.0);
  // the composite sort: 1000 build rows (10 rank bits) under payloads that are the same permutation (23 range bits): 33 bits
  // in four passes of 9 + 8 + 8 + 8; bit 22, the range's top, lies in the third digit, the rank's top bits in the last
  int passes = composite_chain_digits(10, 23, 0, n - 1, 1000, 9, dg);
  CHECK(passes == 4);
  const int shifts[4] = {0, 9, 17, 25}, bits[4] = {9, 8, 8, 8};
  for (int i = 0; i < 4; i++) CHECK(dg[i].shift == shifts[i] && dg[i].bits == bits[i]);
  CHECK(dg[0].dens == 1.0 && dg[1].dens == 1.0 && near(dg[2].dens, 8388608.0 / (double)n) && near(dg[3].dens, 1.024));
  // one build row, payloads of one value: nothing to sort on
  CHECK(composite_chain_digits(0, 0, 7, 7, 1, 9, dg) == 0);
}

static void test_lds_sort() {
  const LdsSortKnobs lds = lds_knobs();
  CHECK(lds.at(-1) == 512 && lds.at(0) == 2048 && lds.at(2) == 8192 && lds.at(3) == 8192);
  CHECK(lds_sort_fits(1681.0, 2048) && !lds_sort_fits(1700.0, 2048));  // 1681 + 8 * 41 + 24 = 2033
  CHECK(lds_sort_level(300.0, -1, 2, lds.max_run) == -1 && lds_sort_level(300.0, 0, 2, lds.max_run) == 0);
  CHECK(lds_sort_level(3500.0, 0, 2, lds.max_run) == 1 && lds_sort_level(5200.0, 0, 2, lds.max_run) == 2);
  CHECK(lds_sort_level(5200.0, 0, 1, lds.max_run) == 2 && lds_sort_level(9000.0, -1, 2, lds.max_run) == 3);  // none: max_level + 1
}

int main() {
  test_lds_sort();
  test_rank_runs_fit();
  test_gate();
  test_varying_digits();
  test_lsd_split();
  test_sort_msd_window();
  test_chain_digits();
  if (failures) {
    std::printf("%d checks failed\n", failures);
    return 1;
  }
  std::printf("all small-plan cases passed\n");
  return 0;
}
