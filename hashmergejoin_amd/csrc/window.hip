// Window functions over ordered partitions (hmj_window_device; include/hmj.h): ROW_NUMBER, RANK, DENSE_RANK, running
// COUNT / SUM / MIN / MAX, LAG and LEAD for every row of one OVER (PARTITION BY ... ORDER BY ...) clause.  Nothing in the
// reference corresponds.  The order is hmj_order_by_device's map (or the identity without keys); everything behind it runs
// on sorted positions, geometry and launches as hmj_winplan.h plans them.  No workgroup ever waits on another:
//   window_heads_kernel   a wave walks kWinChunks chunks of 64 positions: a lane gathers row map[j]'s fixed-width keys once and
//                         takes row map[j - 1]'s from the lane below (__shfl_up; lane 0 gathers its own), strings are read
//                         in place; the rows compare column by column (validity, then value; strings by length, then
//                         bytes); the ballots
//                         of "partition head" and "peer head" are one word each per chunk; partitions and peer groups are
//                         popcounts, one atomic per workgroup and counter.  The wave stores the aggregate of its range's
//                         position state, four slots: partition heads (sum), peer heads since the last partition head (sum,
//                         cut at a partition head), last partition head and last peer head (position + 1, max).
//   window_carry_kernel   the exclusive segmented scan of aggregates {accumulator, valid count, saw a head}, four slots each
//                         with its own operation: b follows a, a head in b selects b, else the accumulators combine.  One
//                         workgroup per tile; a lane owns `per` consecutive aggregates, a __shfl_up scan joins the lanes of a
//                         wave, the waves are joined in order: the shape depends on the index alone.  Run over the ranges'
//                         aggregates in place (tile totals out), then once over the totals.
//   window_state_kernel   one wave per chunk: the carry into the chunk's range, walked over the range's earlier words, is
//                         the chunk's state {partition heads in front, dense rank carried in, last partition head, last peer
//                         head}; the last position of every partition gives its length: the longest by a wave maximum, one
//                         atomic per workgroup.
//   window_rank_kernel    one lane per position, up to kWinLaunch functions: ROW_NUMBER, RANK and DENSE_RANK from the
//                         chunk's state and the bits below the lane; LAG / LEAD test the partition of position j -+ offset
//                         (its chunk's state and word) and gather one value.
//   window_scan_kernel    up to kWinLaunch cumulative functions, a wave per range: map entry and head word loaded once for all
//                         functions, every gather issued before the segmented scan of the chunk, the chunks joined in order.
//                         WRITE = false stores the range's aggregates for the carry; WRITE = true starts from the carried
//                         value and writes the outputs.
// The writing kernels store a wave's ballot of "valid" as one bitmap word and count NULLs by popcount, one atomic per
// workgroup and function.  The call owns its WindowWs (hmj_ctx.h) and calls hmj_order_by_device for the order; it touches
// nothing else of the ctx.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdio>
#include <cstring>

#include "hmj_entry.h"
#include "hmj_winplan.h"

using hmj::u32;
using hmj::u64;
using namespace hmj_host;

namespace {

typedef unsigned char u8;

constexpr int WN_THREADS = (int)kWinThreads;
constexpr int WN_WAVES = WN_THREADS / 64;
constexpr int kChunks = (int)kWinChunks;
constexpr int kLaunch = (int)kWinLaunch;
constexpr u64 kSign = 1ull << 63;
constexpr u32 kString = HMJ_ORDER_LARGE_STRING;
// WindowWs::acc slots (u64): partitions, peer groups, the longest partition, then the NULL slots of every function
enum { WA_PARTS = 0, WA_PEERS, WA_MAXLEN, WA_NULLS, WA_N = WA_NULLS + HMJ_MAX_WINDOW_FNS };

// how two accumulators combine (groupagg.hip's four operations, restated: that file keeps its own)
enum { CK_ADD_U = 0, CK_ADD_D, CK_MIN, CK_MAX };
__host__ __device__ __forceinline__ u32 comb_kind(u32 type, u32 op) {
  if (op == HMJ_WIN_CUM_MIN) return CK_MIN;
  if (op == HMJ_WIN_CUM_MAX) return CK_MAX;
  if (op == HMJ_WIN_CUM_SUM && type >= HMJ_TYPE_F32) return CK_ADD_D;
  return CK_ADD_U;  // integer sums; CUM_COUNT (its accumulator stays 0)
}
// -0.0 is the identity of the double add (x + -0.0 == x for every x, -0.0 included)
__device__ __forceinline__ u64 comb_identity(u32 kind) { return kind == CK_ADD_D ? kSign : kind == CK_MIN ? ~0ull : 0ull; }
__device__ __forceinline__ u64 comb(u32 kind, u64 a, u64 b) {
  switch (kind) {  // (uniform)
    case CK_ADD_U: return a + b;
    case CK_ADD_D: return (u64)__double_as_longlong(__longlong_as_double((long long)a) + __longlong_as_double((long long)b));
    case CK_MIN: return a < b ? a : b;
    default: return a > b ? a : b;
  }
}

// One aggregate: what a run of consecutive positions contributes.  head: a partition head lies in the run, and acc / cnt
// describe the positions from the run's last head on.
struct __attribute__((aligned(16))) WinAgg {
  u64 acc;
  u32 cnt, head;
};
__device__ __forceinline__ WinAgg agg_identity(u32 kind) { return WinAgg{comb_identity(kind), 0u, 0u}; }
// a: the earlier positions, b: the later ones.  A head in b SELECTS b: nothing of a reaches the result.
__device__ __forceinline__ WinAgg agg_join(u32 kind, const WinAgg& a, const WinAgg& b) {
  const u64 t = comb(kind, a.acc, b.acc);
  return WinAgg{b.head ? b.acc : t, b.head ? b.cnt : a.cnt + b.cnt, a.head | b.head};
}
__device__ __forceinline__ WinAgg agg_shfl_up(const WinAgg& v, int d) {
  return WinAgg{__shfl_up(v.acc, d, 64), __shfl_up(v.cnt, d, 64), __shfl_up(v.head, d, 64)};
}
__device__ __forceinline__ WinAgg agg_lane(const WinAgg& v, int l) {
  return WinAgg{__shfl(v.acc, l, 64), __shfl(v.cnt, l, 64), __shfl(v.head, l, 64)};
}
// inclusive scan over the lanes of a wave
__device__ __forceinline__ WinAgg agg_wave_scan(u32 kind, WinAgg v, int lane) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const WinAgg p = agg_shfl_up(v, d);
    const WinAgg t = agg_join(kind, p, v);
    if (lane >= d) v = t;
  }
  return v;
}

__device__ __forceinline__ u64 lanes_through(int lane) { return lane == 63 ? ~0ull : ((2ull << lane) - 1ull); }
__device__ __forceinline__ u64 uniform64(u64 v) {
  return ((u64)(u32)__builtin_amdgcn_readfirstlane((int)(u32)(v >> 32)) << 32) | (u64)(u32)__builtin_amdgcn_readfirstlane((int)(u32)v);
}
__device__ __forceinline__ u64 wave_id() { return uniform64(((u64)blockIdx.x * WN_THREADS + threadIdx.x) >> 6); }
__device__ __forceinline__ u64 load8(const u8* p) {  // any alignment
  u64 v;
  __builtin_memcpy(&v, p, 8);
  return v;
}

// A value as loaded, by the width of its type: zero-extended bits
__device__ __forceinline__ u64 load_bits(const void* __restrict__ p, u32 type, u64 r) {
  switch (width_of(type)) {  // (uniform)
    case 1: return reinterpret_cast<const u8*>(p)[r];
    case 2: return reinterpret_cast<const unsigned short*>(p)[r];
    case 4: return reinterpret_cast<const u32*>(p)[r];
    default: return reinterpret_cast<const u64*>(p)[r];
  }
}
__device__ __forceinline__ void store_bits(void* __restrict__ p, u32 width, u64 j, u64 o) {
  switch (width) {  // (uniform)
    case 1: reinterpret_cast<u8*>(p)[j] = (u8)o; break;
    case 2: reinterpret_cast<unsigned short*>(p)[j] = (unsigned short)o; break;
    case 4: reinterpret_cast<u32*>(p)[j] = (u32)o; break;
    default: reinterpret_cast<u64*>(p)[j] = o;
  }
}
// The accumulator a loaded value starts as (hmj_group_agg_device's rules).  SUM: integers extended to 64 bits in their
// signedness, floats as double; MIN / MAX: a u64 key whose unsigned order is the type's order -- signed integers biased by
// 2^63, floats by the sign-flip mapping on their own bits (F32 on 32 bits), a NaN on the losing side (~0 for MIN, 0 for MAX:
// no number's key is either).
__device__ __forceinline__ u64 acc_start(u64 bits, u32 type, u32 op) {
  const bool order = op == HMJ_WIN_CUM_MIN || op == HMJ_WIN_CUM_MAX;  // (uniform)
  if (type == HMJ_TYPE_F64) {
    if (!order) return bits;
    if ((bits & ~kSign) > 0x7ff0000000000000ull) return op == HMJ_WIN_CUM_MIN ? ~0ull : 0ull;
    return (bits >> 63) ? ~bits : (bits | kSign);
  }
  if (type == HMJ_TYPE_F32) {
    const u32 b = (u32)bits;
    if (!order) return (u64)__double_as_longlong((double)__uint_as_float(b));
    if ((b & 0x7fffffffu) > 0x7f800000u) return op == HMJ_WIN_CUM_MIN ? ~0ull : 0ull;
    return (u64)((b >> 31) ? ~b : (b | 0x80000000u));
  }
  const bool is_signed = type <= HMJ_TYPE_I64;
  const u32 up = is_signed ? 64u - 8u * width_of(type) : 0u;
  const u64 x = (u64)((long long)(bits << up) >> up);
  return order && is_signed ? (x ^ kSign) : x;
}
// ... and the output value of an accumulator with at least one valid value behind it
__device__ __forceinline__ u64 acc_finish(u64 k, u32 type, u32 op) {
  if (op == HMJ_WIN_CUM_SUM) return k;
  if (type == HMJ_TYPE_F64) return k == (op == HMJ_WIN_CUM_MIN ? ~0ull : 0ull) ? 0x7ff8000000000000ull : (k >> 63) ? (k ^ kSign) : ~k;
  if (type == HMJ_TYPE_F32) {
    const u32 k32 = (u32)k;
    return k == (op == HMJ_WIN_CUM_MIN ? ~0ull : 0ull) ? 0x7fc00000u : (k32 >> 31) ? (k32 ^ 0x80000000u) : (u32)~k32;
  }
  return type <= HMJ_TYPE_I64 ? (k ^ kSign) : k;
}

// ---- heads ---------------------------------------------------------------------------------------------------------------
// The key columns of the call, by value.  Columns [0, n_part) decide partitions, the rest peers.
struct WinKeys {
  const void* data[HMJ_MAX_ORDER_COLS];
  const u64* offsets[HMJ_MAX_ORDER_COLS];
  const u8* vbits[HMJ_MAX_ORDER_COLS];  // NULL: the column holds no NULL
  u64 voff[HMJ_MAX_ORDER_COLS];
  u32 type[HMJ_MAX_ORDER_COLS];
  u32 k, n_part;
};

// rows a and b differ in string column c under the ORDER BY's equality: two NULL slots are equal, a NULL slot differs from
// every string, strings compare by length and then by bytes.  Nothing under a NULL slot is read beyond its bitmap bit.
__device__ __forceinline__ bool col_differs(const WinKeys& K, int c, u64 a, u64 b) {
  if (K.vbits[c]) {  // (uniform)
    const u32 va = hmj::valid_bit(K.vbits[c], K.voff[c] + a), vb = hmj::valid_bit(K.vbits[c], K.voff[c] + b);
    if (!va || !vb) return va != vb;
  }
  const u64 a0 = K.offsets[c][a], a1 = K.offsets[c][a + 1], b0 = K.offsets[c][b], b1 = K.offsets[c][b + 1];
  const u64 len = a1 - a0;
  if (len != b1 - b0) return true;
  const u8* p = reinterpret_cast<const u8*>(K.data[c]) + a0;
  const u8* q = reinterpret_cast<const u8*>(K.data[c]) + b0;
  u64 i = 0;
  for (; i + 8 <= len; i += 8)
    if (load8(p + i) != load8(q + i)) return true;
  for (; i < len; i++)
    if (p[i] != q[i]) return true;
  return false;
}

// Row r's value in fixed-width column c as the bits equality compares: every NaN all ones, 0 under a NULL slot (v = 0),
// whose value bytes are not read.
__device__ __forceinline__ u64 key_bits(const WinKeys& K, int c, u64 r, u32& v) {
  v = K.vbits[c] ? hmj::valid_bit(K.vbits[c], K.voff[c] + r) : 1u;
  if (!v) return 0;
  const u32 type = K.type[c];
  const u64 x = load_bits(K.data[c], type, r);
  if (type == HMJ_TYPE_F64 && (x & ~kSign) > 0x7ff0000000000000ull) return ~0ull;
  if (type == HMJ_TYPE_F32 && (x & 0x7fffffffull) > 0x7f800000ull) return ~0ull;
  return x;
}

// the slots of the position state's aggregate, and how each is carried
enum { PS_PARTS = 0, PS_DENSE, PS_PLAST, PS_GLAST };
constexpr u32 kPosKinds = CK_ADD_U | (CK_ADD_U << 8) | (CK_MAX << 16) | (CK_MAX << 24);
__host__ __device__ __forceinline__ u32 kind_of(u32 kinds, int s) { return (kinds >> (8 * s)) & 0xffu; }

// what the words in front of a chunk leave it: folded over one more word
struct PosState {
  u64 parts, dense, plast, glast;  // plast / glast: position + 1; 0: none yet
};
__device__ __forceinline__ void pos_fold(PosState& s, u64 word, u64 pm, u64 gm) {
  s.parts += (u64)__builtin_popcountll(pm);
  if (pm) {
    const int last = 63 - __builtin_clzll(pm);
    s.dense = (u64)__builtin_popcountll(gm >> last);  // (a partition head is a peer head)
    s.plast = word * 64 + (u64)last + 1;
  } else {
    s.dense += (u64)__builtin_popcountll(gm);
  }
  if (gm) s.glast = word * 64 + (u64)(63 - __builtin_clzll(gm)) + 1;
}

__global__ __launch_bounds__(WN_THREADS) void window_heads_kernel(WinKeys K, const u64* __restrict__ map, u64 n, u64* __restrict__ phw,
                                                                  u64* __restrict__ ghw, WinAgg* __restrict__ rec, u64* __restrict__ acc) {
  __shared__ u32 red[WN_WAVES][2];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const u64 nwords = (n + 63) >> 6;
  const u64 r = wave_id();
  const u64 w0 = r * (u64)kChunks;
  const u64 w1 = w0 + (u64)kChunks < nwords ? w0 + (u64)kChunks : nwords;
  PosState s{0, 0, 0, 0};
  bool anyp = false;
  u64 peers = 0;
  for (u64 ch = w0; ch < w1; ch++) {  // (wave-uniform; empty for a wave behind the rows)
    const u64 j = ch * 64 + (u64)lane;
    const bool in = j < n;
    // A row's fixed-width keys are gathered once, by the lane of its position; the row in front is the lane below (lane 0
    // gathers its own).  Strings are compared in place.  Every lane takes part in the shuffles; what a lane without a
    // position or without a row in front computes is dropped.
    const u64 cur = map[in ? j : 0];
    u64 prev = __shfl_up(cur, 1, 64);
    const bool first = lane == 0 && in && j > 0;
    if (first) prev = map[j - 1];
    bool pd = false, gd = false;
#pragma unroll
    for (int c = 0; c < HMJ_MAX_ORDER_COLS; c++) {
      if (c < (int)K.k) {  // (uniform, like the column's type)
        bool d;
        if (K.type[c] == kString) {
          d = in && j > 0 && !pd && !gd && col_differs(K, c, prev, cur);
        } else {
          u32 v;
          const u64 x = key_bits(K, c, cur, v);
          u64 xp = __shfl_up(x, 1, 64);
          u32 vp = __shfl_up(v, 1, 64);
          if (first) xp = key_bits(K, c, prev, vp);
          d = v != vp || x != xp;
        }
        if (c < (int)K.n_part) pd = pd || d;
        else gd = gd || d;
      }
    }
    const bool ph = in && (j == 0 || pd);
    bool gh = in && gd;
    gh = gh || ph;
    const u64 pm = __ballot(ph), gm = __ballot(gh);
    if (lane == 0) {
      phw[ch] = pm;
      ghw[ch] = gm;
    }
    anyp = anyp || pm != 0;
    peers += (u64)__builtin_popcountll(gm);
    pos_fold(s, ch, pm, gm);
  }
  if (lane == 0) {
    if (w0 < nwords) {
      rec[r * kLaunch + PS_PARTS] = WinAgg{s.parts, 0u, 0u};
      rec[r * kLaunch + PS_DENSE] = WinAgg{s.dense, 0u, anyp ? 1u : 0u};
      rec[r * kLaunch + PS_PLAST] = WinAgg{s.plast, 0u, 0u};
      rec[r * kLaunch + PS_GLAST] = WinAgg{s.glast, 0u, 0u};
    }
    red[wv][0] = (u32)s.parts;
    red[wv][1] = (u32)peers;
  }
  __syncthreads();
  if (threadIdx.x < 2) {
    u64 t = 0;
    for (int k = 0; k < WN_WAVES; k++) t += red[k][threadIdx.x];
    if (t) atomicAdd(&acc[WA_PARTS + threadIdx.x], t);
  }
}

// ---- carry ---------------------------------------------------------------------------------------------------------------
// Workgroup b: aggregates [b THREADS per, + THREADS per) of `count`, kLaunch slots each (rec[i * kLaunch + s]), replaced by
// their exclusive scan inside the workgroup's tile; the tile's total goes to totals[b * kLaunch + s] (totals == NULL: the
// top scan, nobody reads it).  per <= kWinCarryPer.  A slot no function uses is scanned like the others (its aggregates
// are zeros).
template <int THREADS>
__global__ __launch_bounds__(THREADS) void window_carry_kernel(WinAgg* __restrict__ rec, u64 count, u32 per, u32 kinds,
                                                               WinAgg* __restrict__ totals) {
  __shared__ WinAgg wt[THREADS / 64];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const u64 base = ((u64)blockIdx.x * THREADS + threadIdx.x) * (u64)per;
#pragma unroll 1
  for (int s = 0; s < kLaunch; s++) {
    const u32 kind = kind_of(kinds, s);
    WinAgg v[kWinCarryPer];
    WinAgg sum = agg_identity(kind);
#pragma unroll
    for (int k = 0; k < (int)kWinCarryPer; k++) {
      v[k] = agg_identity(kind);
      if (k < (int)per && base + k < count) v[k] = rec[(base + k) * kLaunch + s];
      sum = agg_join(kind, sum, v[k]);
    }
    const WinAgg incl = agg_wave_scan(kind, sum, lane);
    if (lane == 63) wt[wv] = incl;
    WinAgg run = agg_shfl_up(incl, 1);
    if (lane == 0) run = agg_identity(kind);
    __syncthreads();
    WinAgg front = agg_identity(kind), all = agg_identity(kind);
    for (int k = 0; k < THREADS / 64; k++) {
      const WinAgg t = wt[k];
      if (k < wv) front = agg_join(kind, front, t);
      all = agg_join(kind, all, t);
    }
    run = agg_join(kind, front, run);
#pragma unroll
    for (int k = 0; k < (int)kWinCarryPer; k++) {
      if (k < (int)per && base + k < count) {
        rec[(base + k) * kLaunch + s] = run;
        run = agg_join(kind, run, v[k]);
      }
    }
    if (threadIdx.x == 0 && totals) totals[(u64)blockIdx.x * kLaunch + s] = all;
    __syncthreads();  // wt is reused by the next slot
  }
}

// what is carried into range r in slot s (wave-uniform loads)
__device__ __forceinline__ WinAgg carry_in(const WinAgg* __restrict__ rec, const WinAgg* __restrict__ top, u32 levels, u64 r, int s,
                                           u32 kind) {
  if (levels == 0) return agg_identity(kind);
  const WinAgg x = rec[r * kLaunch + s];
  if (levels == 1) return x;
  return agg_join(kind, top[(r / kWinCarryTile) * kLaunch + s], x);
}

// ---- the positions' state ------------------------------------------------------------------------------------------------
// state[w] = {partition heads in front of word w, peer heads since the last partition head in front of w, the last
// partition head in front of w, the last peer head in front of w} (positions; word 0 holds position 0, a head of both kinds,
// so its last two are never read).
__global__ __launch_bounds__(WN_THREADS) void window_state_kernel(const u64* __restrict__ phw, const u64* __restrict__ ghw, u64 n,
                                                                  const WinAgg* __restrict__ rec, const WinAgg* __restrict__ top, u32 levels,
                                                                  uint4* __restrict__ state, u64* __restrict__ acc) {
  __shared__ u32 red[WN_WAVES];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const u64 nwords = (n + 63) >> 6;
  const u64 w = wave_id();
  u32 longest = 0;
  if (w < nwords) {  // (wave-uniform)
    const u64 r = w / (u64)kChunks;
    PosState s;
    s.parts = carry_in(rec, top, levels, r, PS_PARTS, CK_ADD_U).acc;
    s.dense = carry_in(rec, top, levels, r, PS_DENSE, CK_ADD_U).acc;
    s.plast = carry_in(rec, top, levels, r, PS_PLAST, CK_MAX).acc;
    s.glast = carry_in(rec, top, levels, r, PS_GLAST, CK_MAX).acc;
    for (u64 k = r * (u64)kChunks; k < w; k++) pos_fold(s, k, phw[k], ghw[k]);
    if (lane == 0) state[w] = make_uint4((u32)s.parts, (u32)s.dense, s.plast ? (u32)(s.plast - 1) : 0u, s.glast ? (u32)(s.glast - 1) : 0u);
    // the last position of a partition knows the partition's length
    const u64 j = w * 64 + (u64)lane;
    const u64 pm = phw[w];
    if (j < n) {
      bool last = j + 1 == n;
      if (!last) last = lane < 63 ? ((pm >> (lane + 1)) & 1ull) != 0 : (phw[w + 1] & 1ull) != 0;
      if (last) {
        const u64 mp = pm & lanes_through(lane);
        const u64 ps = mp ? w * 64 + (u64)(63 - __builtin_clzll(mp)) : s.plast - 1;
        longest = (u32)(j - ps + 1);
      }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
      const u32 t = __shfl_xor(longest, o, 64);
      longest = t > longest ? t : longest;
    }
  }
  if (lane == 0) red[wv] = longest;
  __syncthreads();
  if (threadIdx.x == 0) {
    u32 m = 0;
    for (int k = 0; k < WN_WAVES; k++) m = red[k] > m ? red[k] : m;
    if (m) atomicMax(&acc[WA_MAXLEN], (u64)m);
  }
}

// a position's place in its partition, from its chunk's state and the bits at and below its lane
struct WinPos {
  u64 ps, gs;     // first position of the partition, of the peer group
  u32 dense, pid; // dense rank; partition heads at or in front of the position
};
__device__ __forceinline__ WinPos pos_of(const uint4& st, u64 pm, u64 gm, u64 w, int lane) {
  const u64 mp = pm & lanes_through(lane), mg = gm & lanes_through(lane);
  WinPos p;
  const int pl = mp ? 63 - __builtin_clzll(mp) : 0;
  p.ps = mp ? w * 64 + (u64)pl : (u64)st.z;
  p.gs = mg ? w * 64 + (u64)(63 - __builtin_clzll(mg)) : (u64)st.w;
  p.dense = mp ? (u32)__builtin_popcountll(mg >> pl) : st.y + (u32)__builtin_popcountll(mg);
  p.pid = st.x + (u32)__builtin_popcountll(mp);
  return p;
}

// ---- the functions ---------------------------------------------------------------------------------------------------------
// One launch of functions, by value; every loop over them is fully unrolled with an `a < k` guard.
struct WinFns {
  const void* src[kLaunch];
  const u8* vbits[kLaunch];  // NULL: the source column holds no NULL
  u64 voff[kLaunch];
  u64 offset[kLaunch];
  void* dst[kLaunch];
  u64* dval[kLaunch];  // NULL: no output bitmap wanted
  u32 type[kLaunch], op[kLaunch], ow[kLaunch];
  u32 fn[kLaunch];  // the function's index in the call: its NULL counter
  u32 k;
};

// the NULL counters of a launch: popcounts per wave, one atomic per workgroup and function
template <int K>
__device__ __forceinline__ void count_nulls(const WinFns& F, const u32 (&nulls)[K], u32 (*red)[kLaunch], u64* __restrict__ acc) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if (lane == 0) {
#pragma unroll
    for (int a = 0; a < kLaunch; a++) red[wv][a] = 0;
#pragma unroll
    for (int a = 0; a < K; a++) red[wv][a] = nulls[a];
  }
  __syncthreads();
  if (threadIdx.x < F.k) {
    u64 t = 0;
    for (int k = 0; k < WN_WAVES; k++) t += red[k][threadIdx.x];
    if (t) atomicAdd(&acc[WA_NULLS + F.fn[threadIdx.x]], t);
  }
}

// One wave per chunk of 64 positions that starts at a multiple of 64: a ballot is one bitmap word (lanes past n give the
// padding zeros).
template <int K>
__global__ __launch_bounds__(WN_THREADS) void window_rank_kernel(WinFns F, const u64* __restrict__ map, u64 n, const u64* __restrict__ phw,
                                                                 const u64* __restrict__ ghw, const uint4* __restrict__ state,
                                                                 u64* __restrict__ acc) {
  __shared__ u32 red[WN_WAVES][kLaunch];
  const int lane = threadIdx.x & 63;
  const u64 nwords = (n + 63) >> 6;
  const u64 w = wave_id();
  u32 nulls[K];
#pragma unroll
  for (int a = 0; a < K; a++) nulls[a] = 0;
  if (w < nwords) {  // (wave-uniform)
    const u64 j = w * 64 + (u64)lane;
    const bool in = j < n;
    const u32 n_in = (u32)__builtin_popcountll(__ballot(in));
    const WinPos P = pos_of(state[w], phw[w], ghw[w], w, lane);
#pragma unroll
    for (int a = 0; a < K; a++) {
      if (a >= (int)F.k) continue;
      const u32 op = F.op[a], type = F.type[a];  // (uniform)
      bool ok = in;
      u64 o = 0;
      if (op == HMJ_WIN_ROW_NUMBER) {
        o = j - P.ps + 1;
      } else if (op == HMJ_WIN_RANK) {
        o = P.gs - P.ps + 1;
      } else if (op == HMJ_WIN_DENSE_RANK) {
        o = (u64)P.dense;
      } else {
        const u64 off = F.offset[a];
        u64 jj = j;
        if (op == HMJ_WIN_LAG) {
          ok = in && off <= j - P.ps;
          jj = ok ? j - off : j;
        } else {
          ok = in && off <= n - 1 - j;  // (j + off cannot wrap behind this)
          jj = ok ? j + off : j;
          if (ok) {  // the same partition: as many partition heads at or in front of jj
            const u64 w2 = jj >> 6;
            ok = state[w2].x + (u32)__builtin_popcountll(phw[w2] & lanes_through((int)(jj & 63))) == P.pid;
          }
        }
        if (ok) {
          const u64 row = map[jj];
          if (F.vbits[a]) ok = hmj::valid_bit(F.vbits[a], F.voff[a] + row) != 0;
          if (ok) o = load_bits(F.src[a], type, row);
        }
      }
      if (!ok) o = 0;  // the bytes of a NULL slot are 0
      if (in) store_bits(F.dst[a], F.ow[a], j, o);
      const u64 m = __ballot(ok);
      if (F.dval[a] && lane == 0) F.dval[a][w] = m;
      nulls[a] += n_in - (u32)__builtin_popcountll(m);
    }
  }
  count_nulls<K>(F, nulls, red, acc);
}

// One wave per range.  WRITE = false: the range's aggregates to rec (all kLaunch slots; zeros where the launch has no
// function).  WRITE = true: the walk again from the carried value, outputs written.
template <int K, bool WRITE>
__global__ __launch_bounds__(WN_THREADS) void window_scan_kernel(WinFns F, const u64* __restrict__ map, u64 n, const u64* __restrict__ phw,
                                                                 WinAgg* __restrict__ rec, const WinAgg* __restrict__ top, u32 levels,
                                                                 u64* __restrict__ acc) {
  __shared__ u32 red[WN_WAVES][kLaunch];
  const int lane = threadIdx.x & 63;
  const u64 nwords = (n + 63) >> 6;
  const u64 r = wave_id();
  const u64 w0 = r * (u64)kChunks;
  const u64 w1 = w0 + (u64)kChunks < nwords ? w0 + (u64)kChunks : nwords;
  u32 kind[K], nulls[K];
  WinAgg run[K];
#pragma unroll
  for (int a = 0; a < K; a++) {
    kind[a] = a < (int)F.k ? comb_kind(F.type[a], F.op[a]) : (u32)CK_ADD_U;
    nulls[a] = 0;
    run[a] = agg_identity(kind[a]);
    if (WRITE && w0 < nwords && a < (int)F.k) run[a] = carry_in(rec, top, levels, r, a, kind[a]);
  }
  for (u64 ch = w0; ch < w1; ch++) {  // (wave-uniform)
    const u64 j = ch * 64 + (u64)lane;
    const bool in = j < n;
    const u32 n_in = (u32)__builtin_popcountll(__ballot(in));
    // a lane without a position loads what position 0 loads and drops it: no gather sits under a divergent branch
    const u64 row = map[in ? j : 0];
    const u32 head = (u32)((phw[ch] >> lane) & 1ull);
    u64 bits[K];
    bool bit[K];
#pragma unroll
    for (int a = 0; a < K; a++) {  // every gather of the position
      bits[a] = 0;
      bit[a] = true;
      if (a < (int)F.k) {  // (uniform)
        if (F.op[a] != HMJ_WIN_CUM_COUNT) bits[a] = load_bits(F.src[a], F.type[a], row);
        if (F.vbits[a]) bit[a] = hmj::valid_bit(F.vbits[a], F.voff[a] + row) != 0;
      }
    }
#pragma unroll
    for (int a = 0; a < K; a++) {
      if (a >= (int)F.k) continue;
      const u32 op = F.op[a], type = F.type[a];  // (uniform)
      const bool ok = in && bit[a];
      WinAgg v;  // what lies under a NULL slot goes nowhere
      v.acc = ok && op != HMJ_WIN_CUM_COUNT ? acc_start(bits[a], type, op) : comb_identity(kind[a]);
      v.cnt = ok ? 1u : 0u;
      v.head = in ? head : 0u;
      v = agg_join(kind[a], run[a], agg_wave_scan(kind[a], v, lane));
      if (WRITE) {
        const bool valid = in && (op == HMJ_WIN_CUM_COUNT || v.cnt != 0);
        const u64 o = !valid ? 0ull : (op == HMJ_WIN_CUM_COUNT ? (u64)v.cnt : acc_finish(v.acc, type, op));
        if (in) store_bits(F.dst[a], F.ow[a], j, o);
        const u64 m = __ballot(valid);
        if (F.dval[a] && lane == 0) F.dval[a][ch] = m;
        nulls[a] += n_in - (u32)__builtin_popcountll(m);
      }
      run[a] = agg_lane(v, 63);  // (lanes past n hold identities: lane 63 has the chunk's whole result)
    }
  }
  if (!WRITE) {
    if (lane == 0 && w0 < nwords) {
#pragma unroll
      for (int a = 0; a < kLaunch; a++) {
        WinAgg z{0, 0, 0};
        if (a < K && a < (int)F.k) z = run[a < K ? a : 0];
        rec[r * kLaunch + a] = z;
      }
    }
  } else {
    count_nulls<K>(F, nulls, red, acc);
  }
}

__global__ __launch_bounds__(WN_THREADS) void window_identity_kernel(u64* __restrict__ map, u64 n) {
  const u64 j = (u64)blockIdx.x * WN_THREADS + threadIdx.x;
  if (j < n) map[j] = j;
}

// ---- host side -----------------------------------------------------------------------------------------------------------
int fn_fail(hmj_ctx* c, u32 a, const char* what) {
  char msg[224];
  std::snprintf(msg, sizeof(msg), "hmj_window_device: function %u: %s", a, what);
  return fail(c, HMJ_E_ARG, msg);
}

int check_window_args(hmj_ctx* c, const hmj_order_col* keys, u32 n_keys, u64 n, const hmj_window_fn* fns, u32 n_fns,
                      const hmj_window_dst* dst, const u64* map_out, const hmj_window_opts* opts) {
  char msg[224];
  if (!fns || !dst || !opts) return fail(c, HMJ_E_ARG, "hmj_window_device: fns / dst / opts is NULL");
  if (opts->struct_size < offsetof(hmj_window_opts, reserved) + sizeof(opts->reserved))
    return fail(c, HMJ_E_ARG, "hmj_window_opts.struct_size too small");
  if (opts->reserved) return fail(c, HMJ_E_ARG, "hmj_window_opts: reserved must be 0");
  if (n_keys > HMJ_MAX_ORDER_COLS) {
    std::snprintf(msg, sizeof(msg), "hmj_window_device: n_keys must be in 0..%d", HMJ_MAX_ORDER_COLS);
    return fail(c, HMJ_E_ARG, msg);
  }
  if (n_keys > 0 && !keys) return fail(c, HMJ_E_ARG, "hmj_window_device: keys is NULL with n_keys > 0");
  if (opts->n_partition_cols > n_keys) return fail(c, HMJ_E_ARG, "hmj_window_device: n_partition_cols is greater than n_keys");
  if (n_fns < 1 || n_fns > HMJ_MAX_WINDOW_FNS) {
    std::snprintf(msg, sizeof(msg), "hmj_window_device: n_fns must be in 1..%d", HMJ_MAX_WINDOW_FNS);
    return fail(c, HMJ_E_ARG, msg);
  }
  if (n > kWinMaxRows) return fail(c, HMJ_E_ARG, "hmj_window_device: too many rows (at most 2^32-1)");
  for (u32 a = 0; a < n_fns; a++) {
    if (!win_known_op(fns[a].op)) return fn_fail(c, a, "unknown op (HMJ_WIN_*)");
    if (fns[a].type > HMJ_TYPE_F64) return fn_fail(c, a, "unknown type (HMJ_TYPE_*)");
  }
  if (n == 0) return HMJ_OK;  // nothing is read or written
  if (!map_out) return fail(c, HMJ_E_ARG, "hmj_window_device: row_map_out is NULL");
  if ((uintptr_t)map_out & 7u) return fail(c, HMJ_E_ARG, "hmj_window_device: row_map_out is not aligned to 8 bytes");
  for (u32 a = 0; a < n_fns; a++) {
    const hmj_window_fn& f = fns[a];
    const hmj_window_dst& d = dst[a];
    const u32 w = width_of(f.type), ow = win_out_width(f.type, f.op);
    if (win_reads_values(f.op)) {
      if (!f.data) return fn_fail(c, a, "source data is NULL");
      if ((uintptr_t)f.data & (uintptr_t)(w - 1)) return fn_fail(c, a, "source data is not aligned to its width");
    }
    if (win_reads_validity(f.op) && validity_overflows(f.validity, n)) return fn_fail(c, a, "validity bit_offset + n overflows 64 bits");
    if (!d.data) return fn_fail(c, a, "destination data is NULL");
    if ((uintptr_t)d.data & (uintptr_t)(ow - 1)) return fn_fail(c, a, "destination data is not aligned to its width");
    if ((uintptr_t)d.validity & 7u) return fn_fail(c, a, "destination validity is not aligned to 8 bytes");
  }
  // A destination the kernels write must not be something they read, nor another destination: address ranges only (the
  // extent of a string column's chars is known on the device only and is not checked, as in hmj_order_by_device).
  constexpr int kMaxIn = 2 * HMJ_MAX_WINDOW_FNS + 3 * HMJ_MAX_ORDER_COLS, kMaxOut = 2 * HMJ_MAX_WINDOW_FNS + 1;
  Range in[kMaxIn], out[kMaxOut];
  int n_in = 0;
  for (u32 a = 0; a < n_fns; a++) {
    const hmj_window_fn& f = fns[a];
    in[n_in++] = win_reads_values(f.op) ? range_of(f.data, n * width_of(f.type)) : Range{0, 0};
    in[n_in++] = win_reads_validity(f.op) ? validity_range(f.validity, n) : Range{0, 0};
    out[2 * a] = range_of(dst[a].data, n * win_out_width(f.type, f.op));
    out[2 * a + 1] = range_of(dst[a].validity, 8 * ((n + 63) / 64));
  }
  out[2 * n_fns] = range_of(map_out, 8 * n);
  for (u32 k = 0; k < n_keys; k++) {
    const hmj_order_col& col = keys[k];
    const bool str = col.type == kString;
    in[n_in++] = str || col.type > HMJ_TYPE_F64 ? Range{0, 0} : range_of(col.data, n * width_of(col.type));
    in[n_in++] = str ? range_of(col.offsets, 8 * (n + 1)) : Range{0, 0};
    in[n_in++] = validity_overflows(col.validity, n) ? Range{0, 0} : validity_range(col.validity, n);
  }
  const int n_out = 2 * (int)n_fns + 1;
  if (OverlapHit h = first_overlap(out, n_out, in, n_in)) {
    if (h.out == 2 * (int)n_fns) return fail(c, HMJ_E_ARG, "hmj_window_device: row_map_out overlaps a source column, a key column or a bitmap");
    return fn_fail(c, (u32)h.out / 2, "the destination overlaps a source column, a key column or a bitmap");
  }
  if (OverlapHit h = first_overlap(out, n_out, out, n_out)) {
    if (h.out == 2 * (int)n_fns) return fail(c, HMJ_E_ARG, "hmj_window_device: row_map_out overlaps a destination");
    return fn_fail(c, (u32)h.out / 2, "the destination overlaps another destination or row_map_out");
  }
  return HMJ_OK;
}

// the scan of the aggregates in ws.rec (exclusive, in place) under the plan's levels
int launch_carry(hmj_ctx* c, const WinGrid& g, u32 kinds) {
  WindowWs& ws = c->window_ws;
  if (g.levels == 0) return HMJ_OK;
  WinAgg* rec = (WinAgg*)ws.rec.p;
  WinAgg* top = (WinAgg*)ws.top.p;
  hipLaunchKernelGGL(window_carry_kernel<WN_THREADS>, dim3((u32)g.tiles), dim3(WN_THREADS), 0, c->stream, rec, g.ranges, kWinCarryPer, kinds,
                     g.levels == kWinTopLevel ? top : (WinAgg*)nullptr);
  HIP_TRY(hipGetLastError());
  if (g.levels == kWinTopLevel) {
    hipLaunchKernelGGL(window_carry_kernel<(int)kWinTopThreads>, dim3(1), dim3(kWinTopThreads), 0, c->stream, top, g.tiles, g.top_per, kinds,
                       (WinAgg*)nullptr);
    HIP_TRY(hipGetLastError());
  }
  return HMJ_OK;
}

template <int K>
int launch_fns(hmj_ctx* c, const WinGrid& g, const WinFns& F, u32 cls, const u64* map, u64 n) {
  WindowWs& ws = c->window_ws;
  const u64 *phw = (const u64*)ws.phw.p, *ghw = (const u64*)ws.ghw.p;
  u64* acc = (u64*)ws.acc.p;
  const dim3 B(WN_THREADS);
  if (cls == WIN_CLASS_RANK) {
    hipLaunchKernelGGL(window_rank_kernel<K>, dim3(g.word_blocks), B, 0, c->stream, F, map, n, phw, ghw, (const uint4*)ws.state.p, acc);
    HIP_TRY(hipGetLastError());
    return HMJ_OK;
  }
  WinAgg* rec = (WinAgg*)ws.rec.p;
  const WinAgg* top = (const WinAgg*)ws.top.p;
  if (g.levels > 0) {
    hipLaunchKernelGGL((window_scan_kernel<K, false>), dim3(g.walk_blocks), B, 0, c->stream, F, map, n, phw, rec, top, g.levels, acc);
    HIP_TRY(hipGetLastError());
    u32 kinds = 0;
    for (u32 a = 0; a < F.k; a++) kinds |= comb_kind(F.type[a], F.op[a]) << (8 * a);
    RC_TRY(launch_carry(c, g, kinds));
  }
  hipLaunchKernelGGL((window_scan_kernel<K, true>), dim3(g.walk_blocks), B, 0, c->stream, F, map, n, phw, rec, top, g.levels, acc);
  HIP_TRY(hipGetLastError());
  return HMJ_OK;
}

int window_rows(hmj_ctx* c, const hmj_order_col* keys, u32 n_keys, u64 n, const hmj_window_fn* fns, u32 n_fns, hmj_window_dst* dst, u64* map,
                hmj_window_opts* o) {
  const WinGrid g = win_grid(n);
  WindowWs& ws = c->window_ws;
  RC_TRY(ensure_dev(c, ws.acc, WA_N * sizeof(u64)));
  RC_TRY(ensure_dev(c, ws.phw, (size_t)g.words * sizeof(u64)));
  RC_TRY(ensure_dev(c, ws.ghw, (size_t)g.words * sizeof(u64)));
  RC_TRY(ensure_dev(c, ws.state, (size_t)g.words * sizeof(uint4)));
  RC_TRY(ensure_dev(c, ws.rec, (size_t)g.ranges * kLaunch * sizeof(WinAgg)));
  RC_TRY(ensure_dev(c, ws.top, (size_t)g.tiles * kLaunch * sizeof(WinAgg)));
  u64* acc = (u64*)ws.acc.p;
  const dim3 B(WN_THREADS);
  RC_TRY(ws.ev.record(c, 0));
  if (n_keys > 0) {  // the order, and every check of the keys: hmj_order_by_device's own
    hmj_order_opts oo;
    std::memset(&oo, 0, sizeof(oo));
    oo.struct_size = sizeof(oo);
    RC_TRY(hmj_order_by_device(c, keys, n_keys, n, (uint64_t*)map, &oo));
    o->n_rounds = oo.n_rounds;
  } else {
    hipLaunchKernelGGL(window_identity_kernel, dim3((u32)((n + WN_THREADS - 1) / WN_THREADS)), B, 0, c->stream, map, n);
    HIP_TRY(hipGetLastError());
  }
  RC_TRY(ws.ev.record(c, 1));
  HIP_TRY(hipMemsetAsync(acc, 0, WA_N * sizeof(u64), c->stream));
  WinKeys K;
  std::memset(&K, 0, sizeof(K));
  K.k = n_keys;
  K.n_part = o->n_partition_cols;
  for (u32 k = 0; k < n_keys; k++) {
    K.data[k] = keys[k].data;
    K.offsets[k] = (const u64*)keys[k].offsets;
    K.vbits[k] = (const u8*)keys[k].validity.bits;
    K.voff[k] = keys[k].validity.bit_offset;
    K.type[k] = keys[k].type;
  }
  hipLaunchKernelGGL(window_heads_kernel, dim3(g.walk_blocks), B, 0, c->stream, K, (const u64*)map, n, (u64*)ws.phw.p, (u64*)ws.ghw.p,
                     (WinAgg*)ws.rec.p, acc);
  HIP_TRY(hipGetLastError());
  RC_TRY(launch_carry(c, g, kPosKinds));
  hipLaunchKernelGGL(window_state_kernel, dim3(g.word_blocks), B, 0, c->stream, (const u64*)ws.phw.p, (const u64*)ws.ghw.p, n,
                     (const WinAgg*)ws.rec.p, (const WinAgg*)ws.top.p, g.levels, (uint4*)ws.state.p, acc);
  HIP_TRY(hipGetLastError());
  RC_TRY(ws.ev.record(c, 2));
  u32 ops[HMJ_MAX_WINDOW_FNS];
  WinChunk chunks[HMJ_MAX_WINDOW_FNS];
  for (u32 a = 0; a < n_fns; a++) ops[a] = fns[a].op;
  const u32 n_chunks = win_chunks(ops, n_fns, chunks);
  for (u32 q = 0; q < n_chunks; q++) {
    const WinChunk& ch = chunks[q];
    WinFns F;
    std::memset(&F, 0, sizeof(F));
    F.k = ch.k;
    for (u32 a = 0; a < ch.k; a++) {
      const hmj_window_fn& f = fns[ch.fn[a]];
      F.src[a] = f.data;
      F.vbits[a] = win_reads_validity(f.op) ? (const u8*)f.validity.bits : nullptr;
      F.voff[a] = f.validity.bit_offset;
      F.offset[a] = f.offset;
      F.dst[a] = dst[ch.fn[a]].data;
      F.dval[a] = (u64*)dst[ch.fn[a]].validity;
      F.type[a] = f.type;
      F.op[a] = f.op;
      F.ow[a] = win_out_width(f.type, f.op);
      F.fn[a] = ch.fn[a];
    }
    if (F.k <= 1) RC_TRY(launch_fns<1>(c, g, F, ch.cls, (const u64*)map, n));
    else if (F.k <= 2) RC_TRY(launch_fns<2>(c, g, F, ch.cls, (const u64*)map, n));
    else RC_TRY(launch_fns<kLaunch>(c, g, F, ch.cls, (const u64*)map, n));
  }
  RC_TRY(ws.ev.record(c, 3));
  u64 h[WA_N];
  RC_TRY(read_back(c, acc, h, sizeof(h)));
  o->n_partitions = h[WA_PARTS];
  o->n_peer_groups = h[WA_PEERS];
  o->max_partition_rows = h[WA_MAXLEN];
  for (u32 a = 0; a < n_fns; a++) dst[a].null_count = h[WA_NULLS + a];
  if (c->profiling) {
    o->ms_order = ws.ev.ms(0, 1);
    o->ms_heads = ws.ev.ms(1, 2);
    o->ms_scan = ws.ev.ms(2, 3);
  }
  return HMJ_OK;
}

}  // namespace

extern "C" {

int hmj_window_device(hmj_ctx* c, const hmj_order_col* keys, uint32_t n_keys, uint64_t n, const hmj_window_fn* fns, uint32_t n_fns,
                      hmj_window_dst* dst, uint64_t* row_map_out, hmj_window_opts* opts) {
  if (!c) return HMJ_E_ARG;
  RC_TRY(check_window_args(c, keys, n_keys, n, fns, n_fns, dst, (const u64*)row_map_out, opts));
  // the out fields of opts go to a full-size copy first; the caller gets the prefix its struct_size holds
  hmj_window_opts o;
  opts_prefix_in(&o, opts);
  opts_clear_out(&o, opts, offsetof(hmj_window_opts, n_partitions));
  if (n == 0) {
    for (u32 a = 0; a < n_fns; a++) dst[a].null_count = 0;
  } else {
    HIP_TRY(hipSetDevice(c->device));
    RC_TRY(window_rows(c, keys, n_keys, n, fns, n_fns, dst, (u64*)row_map_out, &o));
  }
  opts_prefix_out(opts, o);
  return HMJ_OK;
}

}  // extern "C"
