// Pure host planning of hmj_window_device (window.hip; include/hmj.h): the geometry of its kernels over n sorted positions,
// the levels of its carry, what every function writes, and how the functions of a call are cut into launches.  No HIP call
// and no hmj_ctx: the header compiles with a plain C++ compiler (tests/cpp/test_winplan.cc runs it under sanitizers).
// Internal header.
#pragma once
#include <cstdint>

#include "hmj_args.h"

namespace hmj_host {

// The geometry.  A wave walks kWinChunks chunks of 64 sorted positions -- its RANGE, the unit of one carry aggregate --, a
// workgroup is kWinThreads / 64 waves.  The carry scans the ranges' aggregates in tiles of kWinCarryTile (one workgroup, a
// lane owning kWinCarryPer consecutive aggregates), and the tiles' totals in one workgroup of kWinTopThreads lanes, each
// owning top_per <= kWinCarryPer consecutive totals.
constexpr uint32_t kWinThreads = 256;
constexpr uint32_t kWinChunks = 8;
constexpr uint32_t kWinRange = 64 * kWinChunks;                        // P: positions per wave (512)
constexpr uint32_t kWinGroup = kWinRange * (kWinThreads / 64);         // G: positions per workgroup of a walk (2048)
constexpr uint32_t kWinCarryPer = 8;
constexpr uint32_t kWinCarryTile = kWinThreads * kWinCarryPer;         // T: aggregates per carry tile (2048)
constexpr uint32_t kWinTopThreads = 1024;
constexpr uint32_t kWinTopLevel = 2;                                   // the carry's highest level
constexpr uint32_t kWinLaunch = 4;                                     // functions per launch: the slots of an aggregate
constexpr uint64_t kWinMaxRows = 0xFFFFFFFFull;

struct WinGrid {
  uint64_t words;        // ballot words: ceil(n / 64)
  uint64_t ranges;       // carry aggregates: ceil(n / P)
  uint64_t tiles;        // carry tiles: ceil(ranges / T)
  uint32_t levels;       // 0: one range, nothing is carried; 1: one tile; 2: tiles and the scan of their totals
  uint32_t top_per;      // totals per lane of the top scan (0 below level 2)
  uint32_t walk_blocks;  // workgroups of a kernel with one wave per range
  uint32_t word_blocks;  // workgroups of a kernel with one wave per word (one lane per position)
};
inline WinGrid win_grid(uint64_t n) {
  WinGrid g{};
  g.words = (n + 63) / 64;
  g.ranges = (n + kWinRange - 1) / kWinRange;
  g.tiles = (g.ranges + kWinCarryTile - 1) / kWinCarryTile;
  g.levels = g.ranges <= 1 ? 0u : (g.tiles <= 1 ? 1u : kWinTopLevel);
  g.top_per = g.levels == kWinTopLevel ? (uint32_t)((g.tiles + kWinTopThreads - 1) / kWinTopThreads) : 0u;
  g.walk_blocks = (uint32_t)((g.ranges + kWinThreads / 64 - 1) / (kWinThreads / 64));
  g.word_blocks = (uint32_t)((g.words + kWinThreads / 64 - 1) / (kWinThreads / 64));
  return g;
}

// What a function is to the kernels.  The ranking functions and LAG / LEAD follow from the head ballots and one gather
// (window_rank_kernel); the cumulative ones are scanned and carried (window_scan_kernel).
enum : uint32_t { WIN_CLASS_RANK = 0, WIN_CLASS_SCAN = 1 };
inline bool win_known_op(uint32_t op) { return op <= HMJ_WIN_LEAD; }
inline uint32_t win_class(uint32_t op) { return op >= HMJ_WIN_CUM_COUNT && op <= HMJ_WIN_CUM_MAX ? WIN_CLASS_SCAN : WIN_CLASS_RANK; }
// reads the source column's values (its data must be there); CUM_COUNT reads the bitmap only
inline bool win_reads_values(uint32_t op) { return op >= HMJ_WIN_CUM_SUM; }
inline bool win_reads_validity(uint32_t op) { return op >= HMJ_WIN_CUM_COUNT; }
// the HMJ_TYPE_* of the output column
inline uint32_t win_out_type(uint32_t type, uint32_t op) {
  if (op <= HMJ_WIN_CUM_COUNT) return HMJ_TYPE_U64;
  if (op == HMJ_WIN_CUM_SUM) return type >= HMJ_TYPE_F32 ? HMJ_TYPE_F64 : (type <= HMJ_TYPE_I64 ? HMJ_TYPE_I64 : HMJ_TYPE_U64);
  return type;  // CUM_MIN, CUM_MAX, LAG, LEAD
}
inline uint32_t win_out_width(uint32_t type, uint32_t op) { return width_of(win_out_type(type, op)); }
// a slot can never be NULL
inline bool win_never_null(uint32_t op) { return op <= HMJ_WIN_CUM_COUNT; }

// The launches of a call: the functions of one class in the order of the call, kWinLaunch at a time; first every launch of
// the ranking class, then every launch of the scan class.  A function's result does not depend on its launch or slot.
struct WinChunk {
  uint32_t cls, k;
  uint32_t fn[kWinLaunch];  // indices into the call's fns
};
// out: room for HMJ_MAX_WINDOW_FNS chunks; returns how many were made
inline uint32_t win_chunks(const uint32_t* ops, uint32_t n_fns, WinChunk* out) {
  uint32_t n = 0;
  for (uint32_t cls = WIN_CLASS_RANK; cls <= WIN_CLASS_SCAN; cls++) {
    bool open = false;
    for (uint32_t f = 0; f < n_fns; f++) {
      if (win_class(ops[f]) != cls) continue;
      if (!open || out[n - 1].k == kWinLaunch) {
        out[n].cls = cls;
        out[n].k = 0;
        for (uint32_t s = 0; s < kWinLaunch; s++) out[n].fn[s] = 0;
        n++;
        open = true;
      }
      out[n - 1].fn[out[n - 1].k++] = f;
    }
  }
  return n;
}

}  // namespace hmj_host
