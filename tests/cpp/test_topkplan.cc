// The planning of hmj_top_k_device (hashmergejoin_amd/csrc/hmj_topkplan.h) on its own: the pick of the threshold digit
// against a brute-force count over drawn histograms, the digit schedule, the saturating arithmetic of the cut at the uint64
// limits, and the workspace sizes at the largest row count.  No HIP, no library: tests/test_topkplan_cpu.py builds this file
// with g++, plain and under AddressSanitizer + UBSan, and runs both.
#include <cstdio>
#include <vector>

#include "../../hashmergejoin_amd/csrc/hmj_topkplan.h"

using namespace hmj_host;

static int failures = 0;
#define CHECK(cond)                                                     \
  do {                                                                  \
    if (!(cond)) {                                                      \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);     \
      failures++;                                                       \
    }                                                                   \
  } while (0)

static uint64_t rng_state = 0x2545F4914F6CDD1Dull;
static uint64_t draw() {  // xorshift64*
  rng_state ^= rng_state >> 12;
  rng_state ^= rng_state << 25;
  rng_state ^= rng_state >> 27;
  return rng_state * 0x2545F4914F6CDD1Dull;
}

// the pick by counting: the rows are the bins' digits written out in order; row k_rest - 1 (0-based) is the cut's last
static void check_pick(const std::vector<uint64_t>& hist, uint64_t k_rest, uint64_t tie_limit) {
  uint64_t total = 0;
  for (uint64_t h : hist) total += h;
  const TopkPick p = topk_pick(hist.data(), (uint32_t)hist.size(), k_rest, tie_limit);
  if (k_rest == 0 || k_rest > total) {
    CHECK(p.stop == TOPK_BAD);
    return;
  }
  uint32_t digit = 0;
  uint64_t below = 0, seen = 0;
  for (uint32_t d = 0; d < hist.size(); d++) {  // the digit of the k_rest-th smallest row
    if (seen + hist[d] >= k_rest) {
      digit = d;
      below = seen;
      break;
    }
    seen += hist[d];
  }
  CHECK(p.digit == digit && p.below == below && p.tie == hist[digit] && p.k_rest == k_rest - below);
  CHECK(p.k_rest >= 1 && p.k_rest <= p.tie && p.tie >= 1);
  CHECK(p.below + p.k_rest == k_rest);  // the cut is kept: definite rows + what the tie set still owes
  if (p.k_rest == p.tie) CHECK(p.stop == TOPK_STOP_WHOLE);
  else if (p.tie <= tie_limit) CHECK(p.stop == TOPK_STOP_FITS);
  else CHECK(p.stop == TOPK_GO);
}

static void check_picks() {
  for (int it = 0; it < 400; it++) {
    const uint32_t bins = it % 7 == 0 ? kTopkBins : 1u << (1 + draw() % kTopkDigitBits);
    std::vector<uint64_t> hist(bins, 0);
    const int shape = it % 4;
    if (shape == 0) {  // one full bin
      hist[draw() % bins] = 1 + draw() % 100000;
    } else {
      for (uint32_t d = 0; d < bins; d++)  // shape 1: mostly empty bins; 2: small counts; 3: counts near 2^32
        hist[d] = shape == 1 ? (draw() % 8 == 0 ? draw() % 50 : 0) : (shape == 2 ? draw() % 5 : draw() % (1ull << 21));
    }
    uint64_t total = 0;
    for (uint64_t h : hist) total += h;
    check_pick(hist, 0, 4);
    check_pick(hist, total + 1, 4);
    if (!total) continue;
    check_pick(hist, 1, 4);
    check_pick(hist, total, 4);
    uint64_t seen = 0;
    int done = 0;
    for (uint32_t d = 0; d < bins && done < 6; d++) {  // both ends of a bucket, K' == the bucket, and the middle
      if (!hist[d]) continue;
      for (uint64_t tie_limit : {(uint64_t)1, hist[d], hist[d] - 1, (uint64_t)1 << 40}) {
        check_pick(hist, seen + 1, tie_limit);
        check_pick(hist, seen + hist[d], tie_limit);
        check_pick(hist, seen + (hist[d] + 1) / 2, tie_limit);
      }
      seen += hist[d];
      done++;
    }
    for (int q = 0; q < 8; q++) check_pick(hist, 1 + draw() % total, draw() % 3 ? draw() % 64 : 0);
  }
  std::vector<uint64_t> edge(kTopkBins, 0xFFFFFFFFull / kTopkBins);  // bins that add up to the largest row count
  check_pick(edge, 0xFFFFFFFFull / kTopkBins * kTopkBins, 1);
}

static void check_digits() {
  const TopkDigit f = topk_first_digit();
  CHECK(f.width == kTopkDigitBits && f.shift + f.width == 64);
  // OR words 0, 1, 2^63 and all ones, from every decided boundary
  for (uint32_t lo = 0; lo <= 64; lo++) {
    CHECK(topk_next_digit(0, lo).width == 0);
    const TopkDigit one = topk_next_digit(1, lo);
    if (lo == 0) CHECK(one.width == 0);
    else CHECK(one.width == 1 && one.shift == 0);
    const TopkDigit top = topk_next_digit(1ull << 63, lo);
    if (lo == 64) CHECK(top.width == kTopkDigitBits && top.shift == 64 - kTopkDigitBits);
    else CHECK(top.width == 0);
    const TopkDigit all = topk_next_digit(~0ull, lo);
    const uint32_t want = lo < kTopkDigitBits ? lo : kTopkDigitBits;
    CHECK(all.width == want && (want == 0 || all.shift + all.width == lo));
  }
  // a word is walked in at most 8 levels, every varying bit once, no shared bit as the top of a digit
  for (int it = 0; it < 2000; it++) {
    uint64_t varying = draw() & draw();
    if (it % 5 == 0) varying &= (1ull << (draw() % 64)) - 1;
    uint32_t lo = f.shift, levels = 1;
    uint64_t covered = ~0ull << f.shift;
    for (;;) {
      const TopkDigit d = topk_next_digit(varying, lo);
      if (!d.width) break;
      CHECK(d.width <= kTopkDigitBits && d.shift + d.width <= lo);
      CHECK((varying >> (d.shift + d.width - 1)) & 1ull);                       // the digit's top bit varies
      CHECK(!(topk_bits_from(varying, d.shift + d.width) & ((1ull << lo) - 1)));  // nothing varies between it and lo
      covered |= ((d.width == 64 ? 0 : (1ull << d.width)) - 1) << d.shift;
      lo = d.shift;
      levels++;
    }
    CHECK(levels <= 8 && levels <= 1 + (64 - kTopkDigitBits + kTopkDigitBits - 1) / kTopkDigitBits);
    CHECK((varying & ~covered) == 0);
  }
  CHECK(topk_bits_from(~0ull, 64) == 0 && topk_bits_from(~0ull, 0) == ~0ull && topk_bits_from(0xFFull, 4) == 0xF0ull);
}

static void check_cut() {
  const uint64_t M = UINT64_MAX, H = 1ull << 63;
  CHECK(topk_cut(10, 0, 3) == 3 && topk_n_out(10, 0, 3) == 3);
  CHECK(topk_cut(10, 8, 3) == 10 && topk_n_out(10, 8, 3) == 2);
  CHECK(topk_cut(10, 10, 3) == 10 && topk_n_out(10, 10, 3) == 0);
  CHECK(topk_cut(10, 11, M) == 10 && topk_n_out(10, 11, M) == 0);
  CHECK(topk_cut(10, M, M) == 10 && topk_n_out(10, M, M) == 0);
  CHECK(topk_cut(10, 1, M) == 10 && topk_n_out(10, 1, M) == 9);
  CHECK(topk_cut(10, H, H) == 10 && topk_n_out(10, H, H) == 0);  // 2^63 + 2^63 wraps to 0 in 64 bits
  CHECK(topk_cut(M, H, H) == M && topk_n_out(M, H, H) == H - 1);  // the sum saturates one short of 2^64
  CHECK(topk_cut(M, H, H - 1) == M && topk_n_out(M, H, H - 1) == H - 1);
  CHECK(topk_cut(M, M - 1, 1) == M && topk_n_out(M, M - 1, 1) == 1);
  CHECK(topk_cut(M, M, 1) == M && topk_n_out(M, M, 1) == 0);
  CHECK(topk_cut(M, 0, M) == M && topk_n_out(M, 0, M) == M);
  CHECK(topk_cut(0, 0, M) == 0 && topk_n_out(0, M, M) == 0 && topk_cut(5, 0, 0) == 0 && topk_n_out(5, 0, 0) == 0);
  for (int it = 0; it < 20000; it++) {  // against 128-bit arithmetic
    const uint64_t pick[8] = {0, 1, 2, draw() % 100, H, M, M - 1, draw()};
    const uint64_t n = pick[draw() % 8], o = pick[draw() % 8], k = pick[draw() % 8];
    const unsigned __int128 sum = (unsigned __int128)o + k;
    const uint64_t K = sum < n ? (uint64_t)sum : n;
    const uint64_t lo = o < n ? o : n;
    CHECK(topk_cut(n, o, k) == K);
    CHECK(topk_n_out(n, o, k) == K - (lo < K ? lo : K));
  }
  CHECK(topk_auto_full(kTopkAutoMinRows - 1, 1) && !topk_auto_full(kTopkAutoMinRows, 1));
  CHECK(topk_auto_full(1ull << 24, (1ull << 24) / kTopkAutoShare + 1) && !topk_auto_full(1ull << 24, (1ull << 24) / kTopkAutoShare));
  CHECK(topk_tie_limit(0) == kTopkDefaultTieRows && topk_tie_limit(1) == 1 && topk_tie_limit(M) == M);
}

static void check_sizes() {
  for (uint64_t n : {(uint64_t)1, (uint64_t)2, (uint64_t)255, (uint64_t)256, (uint64_t)257, (uint64_t)4097, kTopkMaxRows}) {
    const TopkSizes s = topk_sizes(n, 23);
    CHECK(s.tiles * kTopkThreads >= n && (s.tiles - 1) * kTopkThreads < n);
    CHECK(s.words * 64 == s.tiles * kTopkThreads);  // a ballot word for every wave of every tile, the last tile's too
    CHECK(s.acc == (23 + (uint64_t)kTopkBins) * 8 && s.ballots == s.words * 8 && s.blk == s.tiles * 8 && s.blk_off == s.blk + 8);
    CHECK(s.map == n * 8 && s.map / 8 == n);
    CHECK(topk_list_bytes(n) / 16 == n && topk_word_bytes(n) / 8 == n);
  }
  const TopkSizes big = topk_sizes(kTopkMaxRows, 23);
  CHECK(big.tiles == (1ull << 24) && big.tiles < (1ull << 32));  // a grid's x extent and launch_scan_u64's count hold it
  CHECK(big.map == 0x7FFFFFFF8ull && topk_list_bytes(kTopkMaxRows) == 0xFFFFFFFF0ull);
}

int main() {
  check_picks();
  check_digits();
  check_cut();
  check_sizes();
  std::printf("digit_bits %u\nbins %u\n", kTopkDigitBits, kTopkBins);
  if (failures) {
    std::printf("%d checks failed\n", failures);
    return 1;
  }
  std::printf("all top-k plan cases passed\n");
  return 0;
}
