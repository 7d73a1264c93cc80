// Selection (hmj_filter_device; include/hmj.h): a predicate in conjunctive normal form over typed and string columns,
// evaluated at n positions, to the row map the takes consume and an optional Arrow bitmap.  Nothing in the reference
// corresponds: its iterator hands out (key, rval, sval) triples (hashjoin.h:183-191) and knows no predicates.  Two phases
// with one counter read-back between them; no workgroup ever waits on another:
//   filter_eval_kernel<K>     one lane per position, block b = positions [256 b, 256 b + 256) with slot b; a workgroup walks
//                             kEvalBlocks consecutive blocks (no grid-stride: the blocks' numbers are the indices of their
//                             slots), kEvalWide of them at a time, so a wave covers 64 consecutive positions that start at
//                             a multiple of 64 and a lane has kEvalWide loads in flight at every step.  The terms are kernel
//                             arguments (the term loop is fully unrolled with a `t < k` guard, K = 1, 2, 4, 8 or 16), the
//                             string literals are copied to LDS.  A lane loads the entry of each of the first kMapSlots
//                             distinct maps once (a term on a later map loads its own entry), tests it once per term
//                             (HMJ_TAKE_NO_ROW, >= n_src) and walks the terms with a running clause maximum and predicate
//                             minimum under FALSE < UNKNOWN < TRUE.  Every comparison is a three-way result c in {-1, 0, 1,
//                             2 = unordered} against each literal, and the op reads c: integers in their signedness, floats
//                             as doubles (f32 -> f64 is exact and keeps NaN and the zeros), strings bytewise and then by
//                             length, 8 bytes at a time (EQ / NE test the length first; at most literal-length bytes of a
//                             row are read).  The wave's ballot of TRUE is one mask word, stored by one lane; the popcounts
//                             of TRUE (low half) and UNKNOWN (high half) go to the block's slot, the error counters take
//                             one atomic per workgroup.
//   filter_scan_tiles_kernel  the slots' exclusive scan inside tiles of kScanTile slots, in place, and every tile's total.
//   filter_scan_top_kernel    one workgroup: the exclusive scan of the tile totals; the grand total goes to the counters.
//   -- the host reads the counters back: a bad call stops here, n_out and n_unknown are known --
//   filter_write_kernel       the same geometry as the evaluation: a wave reads, for all of its workgroup's blocks at once, its
//                             own mask word and those of the waves in front of it in the block, ranks the set bits of its
//                             word behind theirs, adds the block's base (tile base + slot) and stores position i at
//                             row_map_out[base + rank].
// The call owns its FilterWs (hmj_ctx.h: five DevBufs, the literals' host copy, four events) and touches nothing else of the
// ctx: no result column, no prepared build side, no grouping, no plan, timing or memo.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdio>
#include <cstring>

#include "hmj_entry.h"

using hmj::u32;
using hmj::u64;
using namespace hmj_host;

namespace {

typedef unsigned char u8;
typedef long long i64;

constexpr int FL_THREADS = 256;
constexpr int FL_WAVES = FL_THREADS / 64;
constexpr int kEvalBlocks = 8;                      // consecutive blocks of 256 positions per workgroup of the evaluation and the write
constexpr int kEvalWide = 4;                        // ... of which a lane evaluates this many together (loads in flight per lane)
constexpr int kScanPer = 8;                         // slots per lane of the tile scan
constexpr u32 kScanTile = FL_THREADS * kScanPer;    // workgroup slots per workgroup of the tile scan (2048)
constexpr int kTopThreads = 1024;                   // the top scan: one workgroup over <= 2^24 / kScanTile = 8192 tile totals
constexpr int kMapSlots = 4;                        // distinct maps whose entry a lane holds in registers
constexpr u32 kLitLds = HMJ_MAX_FILTER_LITERAL_BYTES + 8 * 2 * HMJ_MAX_FILTER_TERMS;  // every literal starts at a multiple of 8
constexpr u64 kNoRow = HMJ_TAKE_NO_ROW;
constexpr u32 kString = HMJ_FILTER_LARGE_STRING;
// FilterWs::acc slots (u64).  The first FA_N_RED are ballot popcounts of the evaluation: map entries >= n_src that are not
// HMJ_TAKE_NO_ROW, read valid string rows whose offsets decrease / end behind chars_bytes; FA_TOTAL is the scan's grand
// total, TRUE positions in the low half and UNKNOWN positions in the high half (both at most n <= 2^32 - 1: no carry).
// FA_SAFE: 16 bytes that stay 0, where a lane without a row points its loads (load_or).
enum { FA_BAD_MAP = 0, FA_BAD_DEC, FA_BAD_END, FA_N_RED, FA_TOTAL = FA_N_RED, FA_SAFE, FA_N = FA_SAFE + 2 };
enum : u32 { V_FALSE = 0, V_UNKNOWN = 1, V_TRUE = 2 };
// FilterTerms::slot beyond the register slots 0 .. kMapSlots - 1
enum : u32 { SLOT_OWN = kMapSlots, SLOT_IDENTITY = kMapSlots + 1 };

// The terms of a call, passed to the kernel by value.  lit0 / lit1: a fixed column's literals widened to 64 bits (signed:
// sign-extended, f32: as the double's bits), a string column's as {offset in the LDS literal block, length << 32}.
template <int K>
struct FilterTerms {
  const void* data[K];
  const u64* offsets[K];
  u64 chars_bytes[K];
  const u8* vbits[K];  // NULL: the column holds no NULL
  u64 voff[K];
  u64 n_src[K];
  const u64* map[K];  // the term's own map (read where slot == SLOT_OWN)
  u64 lit0[K], lit1[K];
  const u64* slot_map[kMapSlots];
  u8 type[K], op[K], neg[K], slot[K], last[K];  // last: the term closes its clause
  u32 k, n_slots;
};

__device__ __forceinline__ u64 load8(const u8* p) {  // any alignment
  u64 v;
  __builtin_memcpy(&v, p, 8);
  return v;
}

// *p where the lane has something to load, else a value from `safe` (16 readable bytes, aligned to 16) that the caller
// discards: the load itself is unconditional, so the U loads of a step leave together instead of each waiting in a branch of
// its own, and a lane without a row still reads nothing of the column.
template <class V>
__device__ __forceinline__ V load_or(const V* p, bool ok, const void* safe) {
  return *(ok ? p : reinterpret_cast<const V*>(safe));
}

// Three-way comparison of the m bytes at s (a row's, any alignment) with the m bytes at l (the literal's): -1, 0 or 1 as
// unsigned bytes order them.  8 bytes at a time; the last word overlaps the one before it (bytes already found equal).
// Reads exactly [s, s + m) and [l, l + m).
__device__ __forceinline__ int cmp_bytes(const u8* s, const u8* l, u32 m) {
  u32 k = 0;
  if (m >= 8u) {
    for (;;) {
      const u64 a = load8(s + k), b = load8(l + k);
      if (a != b) {
        const u32 sh = (u32)__builtin_ctzll(a ^ b) & ~7u;  // little-endian: the lowest differing byte is the first
        return ((a >> sh) & 0xFFu) < ((b >> sh) & 0xFFu) ? -1 : 1;
      }
      if (k + 8u >= m) return 0;
      k = k + 16u <= m ? k + 8u : m - 8u;
    }
  }
  for (; k < m; k++)
    if (s[k] != l[k]) return s[k] < l[k] ? -1 : 1;
  return 0;
}

// TRUE / FALSE of an op on the three-way results against its literals (2: unordered, a NaN on either side)
__device__ __forceinline__ bool op_result(u32 op, int c0, int c1) {
  switch (op) {
    case HMJ_FILTER_EQ:
    case HMJ_FILTER_STARTS_WITH:
    case HMJ_FILTER_ENDS_WITH: return c0 == 0;
    case HMJ_FILTER_NE: return c0 != 0;
    case HMJ_FILTER_LT: return c0 == -1;
    case HMJ_FILTER_LE: return c0 == -1 || c0 == 0;
    case HMJ_FILTER_GT: return c0 == 1;
    case HMJ_FILTER_GE: return c0 == 1 || c0 == 0;
    default: return (c0 == 1 || c0 == 0) && (c1 == -1 || c1 == 0);  // BETWEEN: lit0 <= x && x <= lit1
  }
}

// a valid value `a` of a fixed column against a literal, both widened as FilterTerms describes (type: uniform)
__device__ __forceinline__ int cmp_fixed(u32 type, u64 a, u64 l) {
  if (type <= HMJ_TYPE_I64) return (i64)a < (i64)l ? -1 : ((i64)a > (i64)l ? 1 : 0);
  if (type <= HMJ_TYPE_U64) return a < l ? -1 : (a > l ? 1 : 0);
  const double x = __longlong_as_double((i64)a), y = __longlong_as_double((i64)l);
  return x < y ? -1 : (x > y ? 1 : (x == y ? 0 : 2));
}

// The predicate at the U positions i[u] of one lane (in[u]: i[u] < n; a position past n reads nothing and is not counted),
// term by term for all U at once: every step of a term -- the map entries, the validity bytes, the values or the string
// offsets -- is U independent loads issued back to back before the first of them is used, so a lane keeps U loads in flight
// where a walk position by position kept one (measured: one 4-byte load per lane in flight held an I32 term to 1 TB/s).  A
// map entry is compared with n_src before anything is loaded through it, and a string row's two offsets are compared with
// each other and with chars_bytes before an address is formed from them: such a position raises its flag and the caller
// makes it UNKNOWN.  Under a NULL slot nothing is loaded: no value, no offsets, no bytes.
template <int K, int U>
__device__ __forceinline__ void eval_positions(const FilterTerms<K>& T, const u8* s_lit, const void* safe, const u64 (&i)[U],
                                               const bool (&in)[U], u32 (&pred)[U], bool (&bad_map)[U], bool (&bad_dec)[U],
                                               bool (&bad_end)[U]) {
  u64 rows[kMapSlots][U];
#pragma unroll
  for (int s = 0; s < kMapSlots; s++) {
#pragma unroll
    for (int u = 0; u < U; u++) rows[s][u] = kNoRow;
    if (s < (int)T.n_slots) {  // (uniform)
#pragma unroll
      for (int u = 0; u < U; u++) rows[s][u] = load_or(T.slot_map[s] + i[u], in[u], safe);
#pragma unroll
      for (int u = 0; u < U; u++) rows[s][u] = in[u] ? rows[s][u] : kNoRow;
    }
  }
  u32 cl[U];
#pragma unroll
  for (int u = 0; u < U; u++) {
    pred[u] = V_TRUE;
    cl[u] = V_FALSE;
    bad_map[u] = bad_dec[u] = bad_end[u] = false;
  }
#pragma unroll
  for (int t = 0; t < K; t++) {
    if (t < (int)T.k) {
      const u32 type = T.type[t], op = T.op[t], sl = T.slot[t];  // (uniform)
      u64 r[U];
      bool valid[U];
      u32 v[U];
      if (sl == SLOT_OWN) {  // (uniform)
#pragma unroll
        for (int u = 0; u < U; u++) r[u] = load_or(T.map[t] + i[u], in[u], safe);
#pragma unroll
        for (int u = 0; u < U; u++) r[u] = in[u] ? r[u] : kNoRow;
      } else {
#pragma unroll
        for (int u = 0; u < U; u++) {
          if (sl == SLOT_IDENTITY) r[u] = in[u] ? i[u] : kNoRow;  // (n_src >= n)
          else r[u] = sl == 0 ? rows[0][u] : (sl == 1 ? rows[1][u] : (sl == 2 ? rows[2][u] : rows[3][u]));
        }
      }
#pragma unroll
      for (int u = 0; u < U; u++) {
        valid[u] = r[u] < T.n_src[t];  // (n_src <= 2^32-1: never HMJ_TAKE_NO_ROW)
        bad_map[u] |= in[u] && !valid[u] && r[u] != kNoRow;
      }
      if (T.vbits[t]) {  // (uniform)
        u32 vb[U];
#pragma unroll
        for (int u = 0; u < U; u++) vb[u] = load_or(T.vbits[t] + ((T.voff[t] + r[u]) >> 3), valid[u], safe);
#pragma unroll
        for (int u = 0; u < U; u++) valid[u] = valid[u] && ((vb[u] >> ((T.voff[t] + r[u]) & 7)) & 1u);
      }
      if (op == HMJ_FILTER_IS_NULL || op == HMJ_FILTER_IS_NOT_NULL) {
#pragma unroll
        for (int u = 0; u < U; u++) v[u] = valid[u] == (op == HMJ_FILTER_IS_NOT_NULL) ? V_TRUE : V_FALSE;
      } else if (type == kString) {
        u64 b[U], e[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
          b[u] = load_or(T.offsets[t] + r[u], valid[u], safe);
          e[u] = load_or(T.offsets[t] + r[u] + 1, valid[u], safe);
        }
        const bool exact = op == HMJ_FILTER_EQ || op == HMJ_FILTER_NE;
        const bool part = op == HMJ_FILTER_STARTS_WITH || op == HMJ_FILTER_ENDS_WITH;
        const int nl = op == HMJ_FILTER_BETWEEN ? 2 : 1;
#pragma unroll
        for (int u = 0; u < U; u++) {
          const bool dec = valid[u] && e[u] < b[u], end = valid[u] && !dec && e[u] > T.chars_bytes[t];
          bad_dec[u] |= dec;
          bad_end[u] |= end;
          const bool ok = valid[u] && !dec && !end;
          int c0 = 2, c1 = 2;
          if (ok) {
            const u8* s = reinterpret_cast<const u8*>(T.data[t]) + b[u];
            const u64 len = e[u] - b[u];
#pragma unroll 1
            for (int j = 0; j < nl; j++) {
              const u64 lw = j ? T.lit1[t] : T.lit0[t];
              const u8* l = s_lit + (u32)lw;
              const u64 llen = lw >> 32;  // (<= HMJ_MAX_FILTER_LITERAL_BYTES)
              const u8* p = s;
              u32 m;
              bool skip = false;
              if (exact || part) {  // the length first: EQ needs it equal, a prefix or suffix needs the row to hold it
                skip = exact ? len != llen : len < llen;
                m = (u32)llen;
                if (op == HMJ_FILTER_ENDS_WITH && !skip) p = s + (len - llen);
              } else {
                m = (u32)(len < llen ? len : llen);
              }
              int c = skip ? 1 : cmp_bytes(p, l, m);
              if (!exact && !part && c == 0) c = len < llen ? -1 : (len > llen ? 1 : 0);
              if (j) c1 = c;
              else c0 = c;
            }
          }
          v[u] = ok ? (op_result(op, c0, c1) ? V_TRUE : V_FALSE) : V_UNKNOWN;
        }
      } else {
        u64 a[U];
        switch (type) {  // (uniform)
#define HMJ_FILTER_LOAD(ctype, widen)                                                                                       \
  _Pragma("unroll") for (int u = 0; u < U; u++) a[u] = widen load_or(reinterpret_cast<const ctype*>(T.data[t]) + r[u], valid[u], safe); \
  break
          case HMJ_TYPE_I8: HMJ_FILTER_LOAD(signed char, (u64)(i64));
          case HMJ_TYPE_I16: HMJ_FILTER_LOAD(short, (u64)(i64));
          case HMJ_TYPE_I32: HMJ_FILTER_LOAD(int, (u64)(i64));
          case HMJ_TYPE_U8: HMJ_FILTER_LOAD(u8, (u64));
          case HMJ_TYPE_U16: HMJ_FILTER_LOAD(unsigned short, (u64));
          case HMJ_TYPE_U32: HMJ_FILTER_LOAD(u32, (u64));
          case HMJ_TYPE_F32:
#pragma unroll
            for (int u = 0; u < U; u++)
              a[u] = (u64)__double_as_longlong((double)load_or(reinterpret_cast<const float*>(T.data[t]) + r[u], valid[u], safe));
            break;
          default: HMJ_FILTER_LOAD(u64, );  // I64, U64, F64
#undef HMJ_FILTER_LOAD
        }
#pragma unroll
        for (int u = 0; u < U; u++) {
          const int c0 = cmp_fixed(type, a[u], T.lit0[t]);
          const int c1 = op == HMJ_FILTER_BETWEEN ? cmp_fixed(type, a[u], T.lit1[t]) : 0;
          v[u] = valid[u] ? (op_result(op, c0, c1) ? V_TRUE : V_FALSE) : V_UNKNOWN;
        }
      }
#pragma unroll
      for (int u = 0; u < U; u++) {
        if (T.neg[t]) v[u] = V_TRUE - v[u];  // swaps TRUE and FALSE, leaves UNKNOWN
        cl[u] = v[u] > cl[u] ? v[u] : cl[u];
        if (T.last[t]) {
          pred[u] = cl[u] < pred[u] ? cl[u] : pred[u];
          cl[u] = V_FALSE;
        }
      }
    }
  }
}

// Workgroup g covers the kEvalBlocks consecutive blocks of 256 positions from block kEvalBlocks g on, kEvalWide blocks at a
// time: a lane evaluates its position of each of them together (eval_positions), and the literals are staged once.  Block b =
// positions [256 b, 256 b + 256) has slot b; every ballot is taken with all 64 lanes active (lanes past n contribute the
// padding zeros, and a block at or behind nblk lies past n).
template <int K>
__global__ __launch_bounds__(FL_THREADS) void filter_eval_kernel(FilterTerms<K> T, const u8* __restrict__ lit_dev, u32 lit_bytes, u64 n,
                                                                 u32 nblk, u64* __restrict__ mask, u64* __restrict__ blk,
                                                                 u64* __restrict__ acc) {
  static_assert(kEvalBlocks % kEvalWide == 0, "whole groups of blocks");
  __shared__ __attribute__((aligned(8))) u8 s_lit[kLitLds];
  __shared__ u32 red[kEvalBlocks][FL_WAVES][2];
  __shared__ u32 err[FL_WAVES][FA_N_RED];
  if (lit_bytes) {  // (uniform; a multiple of 8, at most kLitLds)
    for (u32 k = threadIdx.x * 8u; k < lit_bytes; k += FL_THREADS * 8u)
      *reinterpret_cast<u64*>(s_lit + k) = *reinterpret_cast<const u64*>(lit_dev + k);
    __syncthreads();
  }
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const u64 b0 = (u64)blockIdx.x * kEvalBlocks;
  u32 n_map = 0, n_dec = 0, n_end = 0;  // (wave-uniform: popcounts over the workgroup's blocks)
#pragma unroll 1
  for (int c = 0; c < kEvalBlocks; c += kEvalWide) {
    if (b0 + c >= nblk) break;  // (uniform)
    u64 i[kEvalWide];
    bool in[kEvalWide], bad_map[kEvalWide], bad_dec[kEvalWide], bad_end[kEvalWide];
    u32 pred[kEvalWide];
#pragma unroll
    for (int u = 0; u < kEvalWide; u++) {
      i[u] = (b0 + c + u) * FL_THREADS + threadIdx.x;
      in[u] = i[u] < n;
    }
    eval_positions<K, kEvalWide>(T, s_lit, acc + FA_SAFE, i, in, pred, bad_map, bad_dec, bad_end);
#pragma unroll
    for (int u = 0; u < kEvalWide; u++) {
      if (bad_map[u] || bad_dec[u] || bad_end[u]) pred[u] = V_UNKNOWN;
      const u64 m = __ballot(in[u] && pred[u] == V_TRUE);
      const u32 n_unk = (u32)__builtin_popcountll(__ballot(in[u] && pred[u] == V_UNKNOWN));
      n_map += (u32)__builtin_popcountll(__ballot(bad_map[u]));
      n_dec += (u32)__builtin_popcountll(__ballot(bad_dec[u]));
      n_end += (u32)__builtin_popcountll(__ballot(bad_end[u]));
      if (lane == 0) {
        if (in[u]) mask[i[u] >> 6] = m;
        red[c + u][wv][0] = (u32)__builtin_popcountll(m);
        red[c + u][wv][1] = n_unk;
      }
    }
  }
  if (lane == 0) {
    err[wv][FA_BAD_MAP] = n_map;
    err[wv][FA_BAD_DEC] = n_dec;
    err[wv][FA_BAD_END] = n_end;
  }
  __syncthreads();
  if (threadIdx.x < kEvalBlocks) {  // the slots of the workgroup's blocks
    if (b0 + threadIdx.x < nblk) {
      u64 tr = 0, un = 0;
      for (int k = 0; k < FL_WAVES; k++) {
        tr += red[threadIdx.x][k][0];
        un += red[threadIdx.x][k][1];
      }
      blk[b0 + threadIdx.x] = tr | (un << 32);
    }
  } else if (threadIdx.x >= 64 && threadIdx.x < 64 + FA_N_RED) {
    u64 t = 0;
    for (int k = 0; k < FL_WAVES; k++) t += err[k][threadIdx.x - 64];
    if (t) atomicAdd(&acc[threadIdx.x - 64], t);
  }
}

// Tile t = slots [t kScanTile, min(+ kScanTile, nblk)): their exclusive scan in place, their total to tile_tot[t].  The two
// halves of a slot never carry into each other (see FA_TOTAL), so one 64-bit scan scans both counts.
__global__ __launch_bounds__(FL_THREADS) void filter_scan_tiles_kernel(u64* __restrict__ blk, u32 nblk, u64* __restrict__ tile_tot) {
  __shared__ u64 wtot[FL_WAVES];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const u64 base = (u64)blockIdx.x * kScanTile + (u64)threadIdx.x * kScanPer;
  u64 v[kScanPer], sum = 0;
#pragma unroll
  for (int j = 0; j < kScanPer; j++) {
    v[j] = base + j < nblk ? blk[base + j] : 0ull;
    sum += v[j];
  }
  const u64 incl = hmj::wave_incl_scan_u64(sum, lane);
  if (lane == 63) wtot[wv] = incl;
  __syncthreads();
  u64 carry = 0, all = 0;
#pragma unroll
  for (int k = 0; k < FL_WAVES; k++) {
    if (k < wv) carry += wtot[k];
    all += wtot[k];
  }
  u64 run = carry + incl - sum;
#pragma unroll
  for (int j = 0; j < kScanPer; j++) {
    if (base + j < nblk) blk[base + j] = run;
    run += v[j];
  }
  if (threadIdx.x == 0) tile_tot[blockIdx.x] = all;
}

// One workgroup: tile_off[0 .. ntile] = the exclusive scan of tile_tot[0 .. ntile), and the grand total to the counters.
// A lane owns `per` consecutive tiles (ntile <= kTopThreads * per).
__global__ __launch_bounds__(kTopThreads) void filter_scan_top_kernel(const u64* __restrict__ tile_tot, u32 ntile, u32 per,
                                                                      u64* __restrict__ tile_off, u64* __restrict__ acc) {
  __shared__ u64 wtot[kTopThreads / 64];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const u64 base = (u64)threadIdx.x * per;
  u64 sum = 0;
  for (u32 j = 0; j < per; j++)
    if (base + j < ntile) sum += tile_tot[base + j];
  const u64 incl = hmj::wave_incl_scan_u64(sum, lane);
  if (lane == 63) wtot[wv] = incl;
  __syncthreads();
  u64 carry = 0, all = 0;
  for (int k = 0; k < kTopThreads / 64; k++) {
    if (k < wv) carry += wtot[k];
    all += wtot[k];
  }
  u64 run = carry + incl - sum;
  for (u32 j = 0; j < per; j++) {
    if (base + j < ntile) {
      tile_off[base + j] = run;
      run += tile_tot[base + j];
    }
  }
  if (threadIdx.x == 0) {
    tile_off[ntile] = all;
    acc[FA_TOTAL] = all;
  }
}

// The same geometry: workgroup g writes the TRUE positions of blocks kEvalBlocks g .. + kEvalBlocks - 1.  Block b is mask words
// 4 b .. 4 b + 3 (bits at and behind n are 0); the TRUE positions in front of it are the low half of tile base + slot (the
// blocks of a workgroup share a scan tile: kScanTile is a multiple of kEvalBlocks).  Lane l < kEvalBlocks of every wave prepares
// block l for its wave -- the wave's own mask word and the first output index of its bits: the block's base plus the bits of
// the waves in front of it -- so the loads of all blocks are in flight together; the values then reach the wave as scalars, and
// a lane's work per block is one bit test, one count and one store.
__global__ __launch_bounds__(FL_THREADS) void filter_write_kernel(const u64* __restrict__ mask, const u64* __restrict__ blk,
                                                                  const u64* __restrict__ tile_off, u64 n, u32 nblk,
                                                                  u64* __restrict__ out) {
  static_assert(kEvalBlocks <= 64 && kScanTile % kEvalBlocks == 0, "one lane per block of the workgroup, one tile");
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const u64 b0 = (u64)blockIdx.x * kEvalBlocks, nwords = (n + 63) / 64;
  const u64 tile_base = tile_off[b0 / kScanTile];
  u64 mine_l = 0;
  u32 start_l = 0;
  if (lane < kEvalBlocks && b0 + lane < nblk) {
    const u64 b = b0 + lane;
    u32 before = 0;
#pragma unroll
    for (int k = 0; k < FL_WAVES; k++) {
      if (k <= wv && b * FL_WAVES + k < nwords) {
        const u64 w = mask[b * FL_WAVES + k];
        if (k < wv) before += (u32)__builtin_popcountll(w);
        else mine_l = w;
      }
    }
    start_l = (u32)(tile_base + blk[b]) + before;  // (< n_out <= 2^32 - 1 wherever the wave has a bit)
  }
#pragma unroll
  for (int c = 0; c < kEvalBlocks; c++) {
    const u64 mine = (u64)(u32)__builtin_amdgcn_readlane((int)(u32)mine_l, c) |
                     ((u64)(u32)__builtin_amdgcn_readlane((int)(u32)(mine_l >> 32), c) << 32);
    if (mine == 0) continue;  // (uniform; a block at or behind nblk has no set bit)
    const u32 start = (u32)__builtin_amdgcn_readlane((int)start_l, c);
    if ((mine >> lane) & 1ull)
      out[(u64)start + (u32)__builtin_popcountll(mine & ((1ull << lane) - 1ull))] = (b0 + c) * FL_THREADS + threadIdx.x;
  }
}

// ---- host side -----------------------------------------------------------------------------------------------------------
const char* const kOpNames[] = {"EQ", "NE", "LT", "LE", "GT", "GE", "BETWEEN", "IS_NULL", "IS_NOT_NULL", "STARTS_WITH", "ENDS_WITH"};

bool reads_literal(u32 op) { return op != HMJ_FILTER_IS_NULL && op != HMJ_FILTER_IS_NOT_NULL; }
u32 n_literals(u32 op) { return !reads_literal(op) ? 0u : (op == HMJ_FILTER_BETWEEN ? 2u : 1u); }

int term_fail(hmj_ctx* c, u32 k, const char* what) {
  char msg[224];
  std::snprintf(msg, sizeof(msg), "hmj_filter_device: term %u: %s", k, what);
  return fail(c, HMJ_E_ARG, msg);
}

int check_filter_args(hmj_ctx* c, const hmj_filter_term* terms, u32 n_terms, u64 n, const u64* out, const u64* mask_out,
                      const hmj_filter_opts* opts) {
  char msg[224];
  if (!terms || !opts) return fail(c, HMJ_E_ARG, "hmj_filter_device: terms / opts is NULL");
  if (opts->struct_size < offsetof(hmj_filter_opts, reserved2) + sizeof(opts->reserved2))
    return fail(c, HMJ_E_ARG, "hmj_filter_opts.struct_size too small");
  if (opts->reserved || opts->reserved2) return fail(c, HMJ_E_ARG, "hmj_filter_opts: reserved / reserved2 must be 0");
  if (n_terms < 1 || n_terms > HMJ_MAX_FILTER_TERMS) {
    std::snprintf(msg, sizeof(msg), "hmj_filter_device: n_terms must be in 1..%d", HMJ_MAX_FILTER_TERMS);
    return fail(c, HMJ_E_ARG, msg);
  }
  if (n > 0xFFFFFFFFull) return fail(c, HMJ_E_ARG, "hmj_filter_device: too many positions (at most 2^32-1)");
  if (n > 0 && !out) return fail(c, HMJ_E_ARG, "hmj_filter_device: row_map_out is NULL");
  if ((uintptr_t)out & 7u) return fail(c, HMJ_E_ARG, "hmj_filter_device: row_map_out is not aligned to 8 bytes");
  if ((uintptr_t)mask_out & 7u) return fail(c, HMJ_E_ARG, "hmj_filter_device: mask_out is not aligned to 8 bytes");
  u64 lit_bytes = 0;
  for (u32 k = 0; k < n_terms; k++) {
    const hmj_filter_term& t = terms[k];
    const bool str = t.type == kString;
    if (t.type > HMJ_TYPE_F64 && !str) return term_fail(c, k, "unknown type (HMJ_TYPE_* or HMJ_FILTER_LARGE_STRING)");
    if (t.op > HMJ_FILTER_ENDS_WITH) return term_fail(c, k, "unknown op");
    if (t.flags & ~HMJ_FILTER_NOT) return term_fail(c, k, "unknown flag bits (HMJ_FILTER_NOT)");
    if (t.reserved) return term_fail(c, k, "reserved must be 0");
    if (!str && (t.op == HMJ_FILTER_STARTS_WITH || t.op == HMJ_FILTER_ENDS_WITH)) {
      std::snprintf(msg, sizeof(msg), "%s is a string-only op, the column is fixed-width", kOpNames[t.op]);
      return term_fail(c, k, msg);
    }
    if (k > 0 && t.clause < terms[k - 1].clause) return term_fail(c, k, "clause ids must not decrease along terms");
    if (t.n_src > 0xFFFFFFFFull) return term_fail(c, k, "too many rows (n_src at most 2^32-1)");
    if ((uintptr_t)t.row_map & 7u) return term_fail(c, k, "row_map is not aligned to 8 bytes");
    if (!t.row_map && t.n_src < n) return term_fail(c, k, "n_src < n without a row_map");
    if (validity_overflows(t.validity, t.n_src)) return term_fail(c, k, "validity bit_offset + n_src overflows 64 bits");
    const bool rows = n > 0 && t.n_src > 0;  // the call may read a row of the column
    if (str) {
      if (rows && !t.offsets) return term_fail(c, k, "offsets are NULL");
      if ((uintptr_t)t.offsets & 7u) return term_fail(c, k, "offsets are not aligned to 8 bytes");
      if (!t.data && t.chars_bytes) return term_fail(c, k, "chars are NULL with chars_bytes > 0");
      for (u32 j = 0; j < n_literals(t.op); j++) {
        if (!t.str_lit[j] && t.str_len[j]) return term_fail(c, k, "a string literal is NULL with a length > 0");
        if (t.str_len[j] > HMJ_MAX_FILTER_LITERAL_BYTES) lit_bytes = HMJ_MAX_FILTER_LITERAL_BYTES + 1ull;
        else lit_bytes += t.str_len[j];
      }
    } else {
      const u32 w = width_of(t.type);
      if (t.offsets) return term_fail(c, k, "offsets set on a fixed-width column");
      if (rows && !t.data) return term_fail(c, k, "data is NULL");
      if ((uintptr_t)t.data & (uintptr_t)(w - 1)) return term_fail(c, k, "data is not aligned to the type's width");
      for (u32 j = 0; j < n_literals(t.op); j++)
        if (w < 8 && (t.lit[j] >> (8 * w))) return term_fail(c, k, "a literal's bits do not fit the type's width");
    }
  }
  if (lit_bytes > HMJ_MAX_FILTER_LITERAL_BYTES) {
    std::snprintf(msg, sizeof(msg), "hmj_filter_device: the string literals hold more than HMJ_MAX_FILTER_LITERAL_BYTES (%d) bytes",
                  HMJ_MAX_FILTER_LITERAL_BYTES);
    return fail(c, HMJ_E_ARG, msg);
  }
  // An output the kernels write must not be something they read, nor the other output.  Address ranges only; n == 0 writes
  // nothing.
  if (n == 0) return HMJ_OK;
  const Range outs[2] = {range_of(out, 8 * n), range_of(mask_out, 8 * ((n + 63) / 64))};
  if (overlap(outs[0], outs[1])) return fail(c, HMJ_E_ARG, "hmj_filter_device: row_map_out and mask_out overlap");
  for (u32 k = 0; k < n_terms; k++) {
    const hmj_filter_term& t = terms[k];
    const bool str = t.type == kString;
    const Range in[4] = {range_of(t.data, str ? t.chars_bytes : t.n_src * width_of(t.type)),
                         str ? range_of(t.offsets, 8 * (t.n_src + 1)) : Range{0, 0}, range_of(t.row_map, 8 * n),
                         validity_range(t.validity, t.n_src)};
    if (first_overlap(outs, 2, in, 4)) return term_fail(c, k, "row_map_out or mask_out overlaps the column's values, offsets, bitmap or row_map");
  }
  return HMJ_OK;
}

// a fixed column's literal as the kernel compares it
u64 widen_literal(u32 type, u64 bits) {
  switch (type) {
    case HMJ_TYPE_I8: return (u64)(i64)(signed char)bits;
    case HMJ_TYPE_I16: return (u64)(i64)(short)bits;
    case HMJ_TYPE_I32: return (u64)(i64)(int)bits;
    case HMJ_TYPE_F32: {
      const u32 b = (u32)bits;
      float f;
      std::memcpy(&f, &b, 4);
      const double d = (double)f;
      u64 r;
      std::memcpy(&r, &d, 8);
      return r;
    }
    default: return bits;
  }
}

template <int K>
int launch_eval(hmj_ctx* c, const hmj_filter_term* terms, u32 n_terms, const u64* lit_word, u32 lit_bytes, u64 n, u32 nblk, u64* mask,
                u64* blk, u64* acc) {
  FilterTerms<K> T;
  std::memset(&T, 0, sizeof(T));
  T.k = n_terms;
  for (u32 k = 0; k < n_terms; k++) {
    const hmj_filter_term& t = terms[k];
    const bool str = t.type == kString;
    T.data[k] = t.data;
    T.offsets[k] = (const u64*)t.offsets;
    T.chars_bytes[k] = t.chars_bytes;
    T.vbits[k] = (const u8*)t.validity.bits;
    T.voff[k] = t.validity.bit_offset;
    T.n_src[k] = t.n_src;
    T.map[k] = (const u64*)t.row_map;
    T.lit0[k] = str ? lit_word[2 * k] : widen_literal(t.type, t.lit[0]);
    T.lit1[k] = str ? lit_word[2 * k + 1] : widen_literal(t.type, t.lit[1]);
    T.type[k] = (u8)t.type;
    T.op[k] = (u8)t.op;
    T.neg[k] = (u8)(t.flags & HMJ_FILTER_NOT);
    T.last[k] = (u8)(k + 1 == n_terms || terms[k + 1].clause != t.clause);
    if (!t.row_map) {
      T.slot[k] = (u8)SLOT_IDENTITY;
    } else {  // the first kMapSlots distinct maps are loaded once per lane; a term on a later one loads its own entry
      u32 s = 0;
      while (s < T.n_slots && T.slot_map[s] != (const u64*)t.row_map) s++;
      if (s == T.n_slots && s < (u32)kMapSlots) T.slot_map[T.n_slots++] = (const u64*)t.row_map;
      T.slot[k] = (u8)(s < (u32)kMapSlots ? s : (u32)SLOT_OWN);
    }
  }
  hipLaunchKernelGGL(filter_eval_kernel<K>, dim3((nblk + kEvalBlocks - 1) / kEvalBlocks), dim3(FL_THREADS), 0, c->stream, T,
                     (const u8*)c->filter_ws.lit.p, lit_bytes, n, nblk, mask, blk, acc);
  HIP_TRY(hipGetLastError());
  return HMJ_OK;
}

int filter_rows(hmj_ctx* c, const hmj_filter_term* terms, u32 n_terms, u64 n, u64* out, u64* mask_out, hmj_filter_opts* o) {
  const u32 nblk = (u32)((n + FL_THREADS - 1) / FL_THREADS);
  const u32 ntile = (nblk + kScanTile - 1) / kScanTile;
  const u32 per = (ntile + kTopThreads - 1) / kTopThreads;
  FilterWs& ws = c->filter_ws;
  RC_TRY(ensure_dev(c, ws.acc, FA_N * sizeof(u64)));
  RC_TRY(ensure_dev(c, ws.blk, (size_t)nblk * sizeof(u64)));
  RC_TRY(ensure_dev(c, ws.tile, (2 * (size_t)ntile + 1) * sizeof(u64)));
  if (!mask_out) RC_TRY(ensure_dev(c, ws.mask, (size_t)((n + 63) / 64) * sizeof(u64)));
  u64* acc = (u64*)ws.acc.p;
  u64* blk = (u64*)ws.blk.p;
  u64* tile_tot = (u64*)ws.tile.p;
  u64* tile_off = tile_tot + ntile;  // ntile + 1
  u64* mask = mask_out ? mask_out : (u64*)ws.mask.p;
  // the string literals: one block, every literal at a multiple of 8, copied to the device and from there to LDS
  u64 lit_word[2 * HMJ_MAX_FILTER_TERMS] = {0};
  std::vector<u8>& lits = ws.lit_host;
  lits.clear();
  for (u32 k = 0; k < n_terms; k++) {
    if (terms[k].type != kString) continue;
    for (u32 j = 0; j < n_literals(terms[k].op); j++) {
      const u64 len = terms[k].str_len[j];
      lit_word[2 * k + j] = (u64)lits.size() | (len << 32);
      if (len) lits.insert(lits.end(), (const u8*)terms[k].str_lit[j], (const u8*)terms[k].str_lit[j] + len);
      lits.resize((lits.size() + 7) & ~(size_t)7, 0);
    }
  }
  const u32 lit_bytes = (u32)lits.size();  // (<= kLitLds: at most 4096 bytes in at most 32 literals)
  if (lit_bytes) {
    RC_TRY(ensure_dev(c, ws.lit, kLitLds));
    HIP_TRY(hipMemcpyAsync(ws.lit.p, lits.data(), lit_bytes, hipMemcpyHostToDevice, c->stream));
  }
  HIP_TRY(hipMemsetAsync(acc, 0, FA_N * sizeof(u64), c->stream));
  RC_TRY(ws.ev.record(c, 0));
  if (n_terms <= 1) RC_TRY(launch_eval<1>(c, terms, n_terms, lit_word, lit_bytes, n, nblk, mask, blk, acc));
  else if (n_terms <= 2) RC_TRY(launch_eval<2>(c, terms, n_terms, lit_word, lit_bytes, n, nblk, mask, blk, acc));
  else if (n_terms <= 4) RC_TRY(launch_eval<4>(c, terms, n_terms, lit_word, lit_bytes, n, nblk, mask, blk, acc));
  else if (n_terms <= 8) RC_TRY(launch_eval<8>(c, terms, n_terms, lit_word, lit_bytes, n, nblk, mask, blk, acc));
  else RC_TRY(launch_eval<HMJ_MAX_FILTER_TERMS>(c, terms, n_terms, lit_word, lit_bytes, n, nblk, mask, blk, acc));
  hipLaunchKernelGGL(filter_scan_tiles_kernel, dim3(ntile), dim3(FL_THREADS), 0, c->stream, blk, nblk, tile_tot);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(filter_scan_top_kernel, dim3(1), dim3(kTopThreads), 0, c->stream, (const u64*)tile_tot, ntile, per, tile_off, acc);
  HIP_TRY(hipGetLastError());
  RC_TRY(ws.ev.record(c, 1));
  // the one synchronisation before the write phase: a bad call stops here
  u64 h[FA_N];
  RC_TRY(read_back(c, acc, h, sizeof(h)));
  if (h[FA_BAD_MAP] || h[FA_BAD_DEC] || h[FA_BAD_END]) {
    char msg[288];
    std::snprintf(msg, sizeof(msg),
                  "hmj_filter_device: %llu row_map entries are >= n_src and not HMJ_TAKE_NO_ROW; %llu read rows have bad string "
                  "offsets (%llu with offsets[r + 1] < offsets[r], %llu that end behind chars_bytes)",
                  h[FA_BAD_MAP], h[FA_BAD_DEC] + h[FA_BAD_END], h[FA_BAD_DEC], h[FA_BAD_END]);
    return fail(c, HMJ_E_ARG, msg);
  }
  o->n_out = h[FA_TOTAL] & 0xFFFFFFFFull;
  o->n_unknown = h[FA_TOTAL] >> 32;
  if (c->profiling) o->ms_eval = ws.ev.ms(0, 1);
  if (o->n_out == 0) return HMJ_OK;
  RC_TRY(ws.ev.record(c, 2));
  hipLaunchKernelGGL(filter_write_kernel, dim3((nblk + kEvalBlocks - 1) / kEvalBlocks), dim3(FL_THREADS), 0, c->stream, (const u64*)mask,
                     (const u64*)blk, (const u64*)tile_off, n, nblk, out);
  HIP_TRY(hipGetLastError());
  RC_TRY(ws.ev.record(c, 3));
  HIP_TRY(hipStreamSynchronize(c->stream));
  if (c->profiling) o->ms_write = ws.ev.ms(2, 3);
  return HMJ_OK;
}

}  // namespace

extern "C" {

int hmj_filter_device(hmj_ctx* c, const hmj_filter_term* terms, uint32_t n_terms, uint64_t n, uint64_t* row_map_out, uint64_t* mask_out,
                      hmj_filter_opts* opts) {
  if (!c) return HMJ_E_ARG;
  RC_TRY(check_filter_args(c, terms, n_terms, n, (const u64*)row_map_out, (const u64*)mask_out, opts));
  // the out fields of opts go to a full-size copy first; the caller gets the prefix its struct_size holds
  hmj_filter_opts o;
  opts_prefix_in(&o, opts);
  opts_clear_out(&o, opts, offsetof(hmj_filter_opts, n_out));
  if (n > 0) {
    HIP_TRY(hipSetDevice(c->device));
    RC_TRY(filter_rows(c, terms, n_terms, n, (u64*)row_map_out, (u64*)mask_out, &o));
  }
  opts_prefix_out(opts, o);
  return HMJ_OK;
}

}  // extern "C"
