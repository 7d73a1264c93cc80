// Pure host planning of hmj_top_k_device (topk.hip; include/hmj.h): the saturating arithmetic of the cut, the AUTO rule,
// the digit schedule of a stream word, the pick of the threshold digit from a level's histogram, and the workspace sizes.
// No HIP call and no hmj_ctx: the header compiles with a plain C++ compiler (tests/cpp/test_topkplan.cc runs it under
// sanitizers).  Internal header.
#pragma once
#include <cstdint>

namespace hmj_host {

// The geometry.  A level histograms one digit of kTopkDigitBits bits of a 64-bit stream word: kTopkBins u32 bins in LDS
// (8 KB) per workgroup of kTopkThreads lanes, one lane per row of a tile.
constexpr uint32_t kTopkDigitBits = 11;
constexpr uint32_t kTopkBins = 1u << kTopkDigitBits;
constexpr uint32_t kTopkThreads = 256;
constexpr uint64_t kTopkMaxRows = 0xFFFFFFFFull;
static_assert(kTopkDigitBits >= 8 && kTopkDigitBits <= 16, "a word is decided in at most 8 levels; the bins fit LDS");

// AUTO takes the full ORDER BY when the cut K exceeds n / kTopkAutoShare (the candidates' ordering and the emit phase
// approach the full sort) and below kTopkAutoMinRows rows (the levels, the mark, the scan and the final ordering are a
// fixed cost of launches and read-backs).  A tie set of more than kTopkDefaultTieRows rows is narrowed by a further level
// before the final ordering sorts it (max_tie_rows == 0).  The share is set from tools/bench_top_k.py's recorded sweep, the
// largest measured K / n at which SELECT beat hmj_order_by_device in every shape; the other two are not measured (DESIGN.md
// "Top-k").
constexpr uint64_t kTopkAutoMinRows = 1ull << 23;
constexpr uint64_t kTopkAutoShare = 256;
constexpr uint64_t kTopkDefaultTieRows = 1ull << 14;

// K = min(n, offset + k) without wrapping, and the entries the call writes: min(k, n - min(n, offset))
inline uint64_t topk_cut(uint64_t n, uint64_t offset, uint64_t k) {
  const uint64_t sum = offset > UINT64_MAX - k ? UINT64_MAX : offset + k;
  return sum < n ? sum : n;
}
inline uint64_t topk_n_out(uint64_t n, uint64_t offset, uint64_t k) {
  const uint64_t rest = n - (offset < n ? offset : n);
  return k < rest ? k : rest;
}
inline bool topk_auto_full(uint64_t n, uint64_t K) { return n < kTopkAutoMinRows || K > n / kTopkAutoShare; }
inline uint64_t topk_tie_limit(uint64_t max_tie_rows) { return max_tie_rows ? max_tie_rows : kTopkDefaultTieRows; }

// The digit schedule of one window (a 64-bit stream word).  `varying`: the bits in which the window's rows differ (the OR
// of w ^ w_first, known behind the window's first level); lo: the bits at and above lo are decided (64: none).  The next
// digit ends at the highest varying bit below lo -- bits that every row shares are never walked -- and is up to
// kTopkDigitBits wide.  width == 0: nothing varies below lo, the window is used up.  The first level of a window runs
// before `varying` is known, on the top kTopkDigitBits bits: topk_first_digit.
struct TopkDigit {
  uint32_t shift, width;  // the digit is (w >> shift) & ((1 << width) - 1)
};
inline TopkDigit topk_first_digit() { return TopkDigit{64u - kTopkDigitBits, kTopkDigitBits}; }
inline TopkDigit topk_next_digit(uint64_t varying, uint32_t lo) {
  const uint64_t below = lo >= 64 ? varying : (varying & ((1ull << lo) - 1ull));
  if (!below) return TopkDigit{0, 0};
  const uint32_t top = 64u - (uint32_t)__builtin_clzll(below);  // one past the highest varying bit
  const uint32_t width = top < kTopkDigitBits ? top : kTopkDigitBits;
  return TopkDigit{top - width, width};
}
// the bits of w at and above bit `from` (from == 64: none, 0)
inline uint64_t topk_bits_from(uint64_t w, uint32_t from) { return from >= 64 ? 0ull : (w >> from) << from; }

// The pick.  hist: the level's bins (rows of the current tie set by digit), their sum the tie set's size; k_rest: how many
// of the tie set's rows the cut still takes, 1 <= k_rest <= that size.  digit: the bin that holds the k_rest-th row;
// below: the rows in smaller bins -- definite from here on --; tie: the digit's bin, the new tie set; k_rest - below of it
// are still to take.  Selection stops where the new tie set is at most tie_limit rows (FITS), or all of it is taken
// (WHOLE: nothing is tied with the cut any more); the caller stops where the window has no digit left.
enum : uint32_t { TOPK_GO = 0, TOPK_STOP_FITS = 1, TOPK_STOP_WHOLE = 2, TOPK_BAD = 3 };
struct TopkPick {
  uint32_t digit, stop;
  uint64_t below, tie, k_rest;
};
inline TopkPick topk_pick(const uint64_t* hist, uint32_t bins, uint64_t k_rest, uint64_t tie_limit) {
  TopkPick p{0, TOPK_BAD, 0, 0, 0};
  if (k_rest == 0) return p;
  uint64_t below = 0;
  for (uint32_t d = 0; d < bins; d++) {
    const uint64_t h = hist[d];
    if (h >= k_rest - below) {  // (below < k_rest here: no wrap)
      p.digit = d;
      p.below = below;
      p.tie = h;
      p.k_rest = k_rest - below;
      p.stop = p.k_rest == h ? TOPK_STOP_WHOLE : (h <= tie_limit ? TOPK_STOP_FITS : TOPK_GO);
      return p;
    }
    below += h;
  }
  return p;  // the bins hold fewer than k_rest rows: TOPK_BAD
}

// The workspace of a call of n rows, in bytes (n <= kTopkMaxRows: nothing wraps in 64 bits).  acc_words: the u64 counters
// in front of the bins, which follow them in one buffer so that a level has one read-back.
struct TopkSizes {
  uint64_t words, tiles;            // ballot words (one per wave of every tile), tiles ceil(n / kTopkThreads)
  uint64_t acc, ballots, blk, blk_off, map;
};
inline TopkSizes topk_sizes(uint64_t n, uint32_t acc_words) {
  TopkSizes s{};
  s.tiles = (n + kTopkThreads - 1) / kTopkThreads;
  s.words = s.tiles * (kTopkThreads / 64);
  s.acc = ((uint64_t)acc_words + kTopkBins) * 8;
  s.ballots = s.words * 8;  // one buffer per class
  s.blk = s.tiles * 8;
  s.blk_off = (s.tiles + 1) * 8;
  s.map = n * 8;
  return s;
}
// a list of m {word, row} rows; the words a list-mode window gathers
inline uint64_t topk_list_bytes(uint64_t m) { return m * 16; }
inline uint64_t topk_word_bytes(uint64_t m) { return m * 8; }

}  // namespace hmj_host
