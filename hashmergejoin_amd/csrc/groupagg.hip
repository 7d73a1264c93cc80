// Typed value columns aggregated over a grouping (hmj_group_agg_device; include/hmj.h): what turns the group columns of
// hmj_group_cols_device / hmj_group_mixed_device into a query result -- SUM / MIN / MAX / MEAN / COUNT of up to HMJ_MAX_AGGS
// NULL-aware columns of ten value types.  Nothing in the reference corresponds.  The call reads what a materialising group
// call left in GroupWs (hmj_ctx.h) -- sorted: the {key64, row} rows, a group one contiguous run ascending by row; flags: one
// head ballot per 64 sorted positions; blk_off: the heads in front of every 256 positions; start: the groups' first
// positions and n behind the last -- and writes nothing of it.  Three kernels per launch chunk of up to kAggLaunch
// aggregates, in the idiom of hmj_group.h's group_agg_kernel and take.hip's cols_take_kernel:
//   agg_walk_kernel     a wave walks kWalkChunks chunks of 64 sorted positions.  rows[i].y and the flags word are loaded
//                       once for all aggregates of the launch; every gather of a position -- the value, and the validity
//                       byte where the column has a bitmap -- is issued before the scan.  Per aggregate a lane holds a 64-bit
//                       accumulator and a valid count (the counts are popcounts of the ballot of "valid": only the
//                       accumulators are scanned); which of four operations combines two accumulators (u64 add, double
//                       add, unsigned min, unsigned max) follows from type and op, MIN / MAX running on an order-preserving
//                       u64 key.  The head bits cut a chunk into segments, an inclusive segmented __shfl_up scan leaves a
//                       segment's result in its last lane, the chunk's last segment is carried (wave-uniform) into the next
//                       chunk.  A group inside the wave's range is stored to its slots by one lane; the group open at the
//                       left end of the range goes to the wave's left partial slot, the one still carried at the right end
//                       to its right partial slot.  No atomics.
//   agg_combine_kernel  one wave per walk wave whose right partial slot holds a group g: g's partials are that slot and the
//                       left slots of the following waves through the wave of g's last position (start[g + 1] - 1).  They
//                       are taken strided over the 64 lanes, each lane combining its own in ascending order, then a shuffle
//                       tree: the shape depends on the number of partials alone.  Lane 0 stores g's slots.
//   agg_finish_kernel   one lane per group: MEAN divides, MIN / MAX map back, a group without a valid value gives a NULL slot
//                       with value bytes 0; a wave's ballot is one word of the output bitmap (one lane stores it), NULLs
//                       are counted by popcount, one atomic per workgroup and aggregate.
// The host checks the arguments (address ranges included), loops over the launch chunks and reads the NULL counters back
// once.  The call owns its AggWs (hmj_ctx.h: three DevBufs, two events) and touches nothing else of the ctx.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdio>
#include <cstring>

#include "hmj_entry.h"

using hmj::u32;
using hmj::u64;
using namespace hmj_host;

namespace {

constexpr int GA_THREADS = 256;
constexpr int GA_WAVES = GA_THREADS / 64;
constexpr int kAggLaunch = 4;    // aggregates per launch
constexpr int kWalkChunks = 8;   // chunks of 64 positions a wave walks: the partial slots are per 512 positions
constexpr int kHeadBlock = 256;  // positions per entry of blk_off (group_heads_kernel's workgroup, hmj_group.h)
constexpr u64 kNoGroup = ~0ull;
constexpr u64 kSign = 1ull << 63;

// how two accumulators combine
enum { CK_ADD_U = 0, CK_ADD_D, CK_MIN, CK_MAX };
__host__ __device__ __forceinline__ u32 comb_kind(u32 type, u32 op) {
  if (op == HMJ_AGG_MIN) return CK_MIN;
  if (op == HMJ_AGG_MAX) return CK_MAX;
  if (op == HMJ_AGG_MEAN || (op == HMJ_AGG_SUM && type >= HMJ_TYPE_F32)) return CK_ADD_D;
  return CK_ADD_U;  // integer sums; HMJ_AGG_COUNT (its accumulator stays 0)
}
// -0.0 is the identity of the double add (x + -0.0 == x for every x, -0.0 included)
__device__ __forceinline__ u64 comb_identity(u32 kind) { return kind == CK_ADD_D ? kSign : kind == CK_MIN ? ~0ull : 0ull; }
// a: the earlier positions' accumulator, b: the later ones'
__device__ __forceinline__ u64 comb(u32 kind, u64 a, u64 b) {
  switch (kind) {  // (uniform)
    case CK_ADD_U: return a + b;
    case CK_ADD_D: return (u64)__double_as_longlong(__longlong_as_double((long long)a) + __longlong_as_double((long long)b));
    case CK_MIN: return a < b ? a : b;
    default: return a > b ? a : b;
  }
}

// A value as loaded: integers extended to 64 bits in their signedness, floats as their bits (F32 zero-extended).  The load
// is typed by the value's width; a signed integer is extended by a shift pair (uniform shift counts).
template <class T>
__device__ __forceinline__ u64 agg_raw(const void* __restrict__ p, u64 r) {
  return (u64) reinterpret_cast<const T*>(p)[r];
}
__device__ __forceinline__ u64 agg_load(const void* __restrict__ p, u32 type, u64 r) {
  u64 x;
  switch (width_of(type)) {  // (uniform)
    case 1: x = agg_raw<unsigned char>(p, r); break;
    case 2: x = agg_raw<unsigned short>(p, r); break;
    case 4: x = agg_raw<u32>(p, r); break;
    default: x = agg_raw<u64>(p, r);
  }
  const u32 up = type <= HMJ_TYPE_I64 ? 64u - 8u * width_of(type) : 0u;
  return (u64)((long long)(x << up) >> up);
}
// The accumulator a loaded value starts as.  SUM: the extended integer, floats as double; MEAN: every type as double;
// MIN / MAX: a u64 key whose unsigned order is the type's order -- signed integers biased by 2^63, floats by the sign-flip
// mapping on their own bits (F32 on 32 bits), a NaN mapped behind every number's key on the losing side (~0 for MIN, 0 for
// MAX: no number's key is either).
__device__ __forceinline__ u64 agg_start(u64 raw, u32 type, u32 op) {
  const bool order = op == HMJ_AGG_MIN || op == HMJ_AGG_MAX;  // (else SUM or MEAN; all uniform)
  if (type == HMJ_TYPE_F64) {
    if (!order) return raw;
    if ((raw & ~kSign) > 0x7ff0000000000000ull) return op == HMJ_AGG_MIN ? ~0ull : 0ull;
    return (raw >> 63) ? ~raw : (raw | kSign);
  }
  if (type == HMJ_TYPE_F32) {
    const u32 b = (u32)raw;
    if (!order) return (u64)__double_as_longlong((double)__uint_as_float(b));
    if ((b & 0x7fffffffu) > 0x7f800000u) return op == HMJ_AGG_MIN ? ~0ull : 0ull;
    return (u64)((b >> 31) ? ~b : (b | 0x80000000u));
  }
  const bool is_signed = type <= HMJ_TYPE_I64;
  if (op == HMJ_AGG_MEAN) return (u64)__double_as_longlong(is_signed ? (double)(long long)raw : (double)raw);
  return order && is_signed ? (raw ^ kSign) : raw;
}

// One launch chunk of aggregates, passed to the kernels by value -- what the walk reads and what the finish writes apart, so
// that neither kernel holds the other's pointers in scalar registers; every loop over them is fully unrolled with an
// `a < k` guard, so the members are read from the kernel arguments at constant offsets.
// desc: HMJ_TYPE_* | HMJ_AGG_* << 8 | dup << 16.  dup bit 0: the source column and type of the aggregate in front (SUM and MIN
// of one column): its loaded value is reused; dup bit 1: its bitmap and bit_offset: its validity bit is reused.
struct AggIn {
  const void* src[kAggLaunch];
  const unsigned char* vbits[kAggLaunch];  // NULL: the source column holds no NULL
  u64 voff[kAggLaunch];
  u32 desc[kAggLaunch];
  u32 k;
};
struct AggOut {
  void* dst[kAggLaunch];
  u64* dval[kAggLaunch];  // NULL: no output bitmap wanted
  u32 desc[kAggLaunch];
  u32 ow[kAggLaunch];  // bytes of an output value
  u32 k;
};
__host__ __device__ __forceinline__ u32 desc_type(u32 d) { return d & 0xffu; }
__host__ __device__ __forceinline__ u32 desc_op(u32 d) { return (d >> 8) & 0xffu; }
__host__ __device__ __forceinline__ u32 desc_dup(u32 d) { return d >> 16; }
// The chunk's slots.  Per group g the K accumulators of a K-aggregate launch side by side (acc[g * K + a]), behind all of
// them the K valid counts (cnt[g * K + a]); per walk wave w its left-open and its right-open group's partials, {accumulator,
// valid count} pairs at part[(w * 2 + side) * K + a]; behind the partials rgrp[w], the group of wave w's right slot or
// kNoGroup.  Everything of one group or wave lies at constant offsets from one address: the kernels hold two base pointers.
struct AggSlots {
  u64* grp;
  ulonglong2* part;
  u64 ng, waves;
  template <int K>
  __device__ u64* gacc(u64 g) const { return grp + g * (u64)K; }
  template <int K>
  __device__ u32* gcnt(u64 g) const { return (u32*)(grp + ng * (u64)K) + g * (u64)K; }
  template <int K>
  __device__ ulonglong2* slot(u64 w, int side) const { return part + (w * 2 + (u64)side) * (u64)K; }
  __device__ u64* rgrp() const { return (u64*)(part + waves * (u64)(2 * kAggLaunch)); }
  static size_t grp_bytes(u64 ng) { return (size_t)kAggLaunch * ng * (sizeof(u64) + sizeof(u32)); }
  static size_t part_bytes(u64 waves) { return (size_t)waves * (2 * kAggLaunch * sizeof(ulonglong2) + sizeof(u64)); }
};

__device__ __forceinline__ u64 lanes_through(int lane) { return lane == 63 ? ~0ull : ((2ull << lane) - 1ull); }
__device__ __forceinline__ u64 uniform64(u64 v) {
  return ((u64)(u32)__builtin_amdgcn_readfirstlane((int)(u32)(v >> 32)) << 32) | (u64)(u32)__builtin_amdgcn_readfirstlane((int)(u32)v);
}

enum { PUT_GROUP = 0, PUT_LEFT, PUT_RIGHT };
template <int K>
__device__ __forceinline__ void agg_put(const AggSlots& S, u32 k, int where, u64 at, const u64 (&v)[K], const u32 (&c)[K]) {
  if (where == PUT_GROUP && at >= S.ng) return;
#pragma unroll
  for (int a = 0; a < K; a++) {
    if (a >= (int)k) continue;
    if (where == PUT_GROUP) {
      S.gacc<K>(at)[a] = v[a];
      S.gcnt<K>(at)[a] = c[a];
    } else {
      S.slot<K>(at, where == PUT_LEFT ? 0 : 1)[a] = make_ulonglong2(v[a], (u64)c[a]);
    }
  }
}

// The walk of group_agg_kernel (hmj_group.h; the comment there explains segments, carry and what decides where a result
// goes -- the ballots alone, the same in every lane), with K accumulators and counts per lane and partial slots in place of
// the atomics: a group open at the left end of the wave's range goes to the wave's left slot when it ends (or at the end of
// the range, when it fills it), the group carried at the right end to the right slot -- always, also at the end of the
// rows, so that every group either lies strictly inside one wave's range and is stored here, or has a right slot in the
// wave of its head and is stored by agg_combine_kernel.  Grid: one wave per kWalkChunks chunks.
template <int K>
__global__ __launch_bounds__(GA_THREADS) void agg_walk_kernel(AggIn T, AggSlots S, const ulonglong2* __restrict__ rows, u64 n,
                                                              const u64* __restrict__ flags, const u64* __restrict__ blk_off) {
  const int lane = threadIdx.x & 63;
  const u64 nchunk = (n + 63) >> 6;
  const u64 w = uniform64(((u64)blockIdx.x * GA_THREADS + threadIdx.x) >> 6);
  const u64 c0 = w * (u64)kWalkChunks;
  if (c0 >= nchunk) return;  // (wave-uniform)
  const u64 c1 = c0 + (u64)kWalkChunks < nchunk ? c0 + (u64)kWalkChunks : nchunk;
  constexpr u64 kPer = kHeadBlock / 64;  // flags words per entry of blk_off
  u64 heads = blk_off[c0 / kPer];        // heads in front of chunk c0
  for (u64 k = (c0 / kPer) * kPer; k < c0; k++) heads += (u64)__builtin_popcountll(flags[k]);
  u32 kind[K];
  u64 cv[K];
  u32 cc[K];
#pragma unroll
  for (int a = 0; a < K; a++) {
    kind[a] = a < (int)T.k ? comb_kind(desc_type(T.desc[a]), desc_op(T.desc[a])) : (u32)CK_ADD_U;
    cv[a] = comb_identity(kind[a]);
    cc[a] = 0;
  }
  bool have = false, left_open = false;  // the carried group: heads - 1
  for (u64 ch = c0; ch < c1; ch++) {
    const u64 i0 = ch << 6;
    const u32 cnt = n - i0 < 64ull ? (u32)(n - i0) : 64u;  // the chunk's positions
    const bool active = (u32)lane < cnt;
    const u64 m = flags[ch];
    const bool head0 = m & 1ull;
    const u64 below = (m | 1ull) & lanes_through(lane);
    const int seg = 63 - __builtin_clzll(below);  // the lane's segment starts here
    // a lane without a row loads what row 0 loads and drops it: no gather sits under a divergent branch
    const u64 r0 = rows[active ? i0 + (u64)lane : i0].y;
    const bool row = active && r0 < n;
    const u64 r = row ? r0 : 0ull;
    const u64 mine = lanes_through(lane) & (~0ull << seg);  // the lanes of the segment up to this one
    const u64 rest = m & ~1ull;                             // heads behind lane 0
    const u64 closing = ~0ull << (rest ? 63 - __builtin_clzll(rest) : 0);  // the lanes of the chunk's last segment
    u64 v[K], raw[K];
    bool bit[K];
    u32 c[K], lc[K];  // lc: the valid values of the chunk's last segment (wave-uniform)
#pragma unroll
    for (int a = 0; a < K; a++) {  // every gather of the position
      raw[a] = 0;
      bit[a] = true;
      if (a < (int)T.k) {  // (uniform, like the tests of T below)
        if (a > 0 && (desc_dup(T.desc[a]) & 1u)) raw[a] = raw[a > 0 ? a - 1 : 0];
        else if (desc_op(T.desc[a]) != HMJ_AGG_COUNT) raw[a] = agg_load(T.src[a], desc_type(T.desc[a]), r);
        if (a > 0 && (desc_dup(T.desc[a]) & 2u)) {
          bit[a] = bit[a > 0 ? a - 1 : 0];
        } else if (T.vbits[a]) {
          bit[a] = hmj::valid_bit(T.vbits[a], T.voff[a] + r);
        }
      }
    }
#pragma unroll
    for (int a = 0; a < K; a++) {
      const bool ok = row && a < (int)T.k && bit[a];
      const u64 x = a < (int)T.k && desc_op(T.desc[a]) != HMJ_AGG_COUNT ? agg_start(raw[a], desc_type(T.desc[a]), desc_op(T.desc[a])) : 0ull;
      v[a] = ok ? x : comb_identity(kind[a]);  // what lies under a NULL slot goes nowhere
      const u64 vm = __ballot(ok);              // the counts need no scan: popcounts of the ballot
      c[a] = (u32)__builtin_popcountll(vm & mine);
      lc[a] = (u32)__builtin_popcountll(vm & closing);
    }
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const bool take = lane - d >= seg;
#pragma unroll
      for (int a = 0; a < K; a++) {
        const u64 pv = __shfl_up(v[a], d, 64);
        const u64 t = comb(kind[a], pv, v[a]);
        v[a] = take ? t : v[a];
      }
    }
    if (have && head0) {  // the carried group ended with the chunk before: closed on the right
      if (lane == 0) agg_put<K>(S, T.k, left_open ? PUT_LEFT : PUT_GROUP, left_open ? w : heads - 1, cv, cc);
      have = false;
    }
    const int tail = (int)cnt - 1;
    if (rest) {
      const int e0 = __builtin_ctzll(rest) - 1;  // the first segment's last lane
      const bool last = lane < tail && ((m >> (lane + 1)) & 1ull);
      if (last) {
        const u64 g = heads + (u64)__builtin_popcountll(m & lanes_through(lane)) - 1;  // (heads >= 1 where lane 0 is no head)
        if (lane == e0 && !head0) {  // continues the carried group, or the group open at the left end of the range
          u64 tv[K];
          u32 tc[K];
#pragma unroll
          for (int a = 0; a < K; a++) {
            tv[a] = comb(kind[a], cv[a], v[a]);
            tc[a] = cc[a] + c[a];
          }
          const bool left = have ? left_open : true;
          agg_put<K>(S, T.k, left ? PUT_LEFT : PUT_GROUP, left ? w : g, tv, tc);
        } else {
          agg_put<K>(S, T.k, PUT_GROUP, g, v, c);
        }
      }
#pragma unroll
      for (int a = 0; a < K; a++) {  // the last segment starts at a head of this chunk
        cv[a] = __shfl(v[a], tail, 64);
        cc[a] = lc[a];
      }
      have = true;
      left_open = false;
    } else {  // one segment
#pragma unroll
      for (int a = 0; a < K; a++) {
        const u64 tv = __shfl(v[a], tail, 64);
        const u32 tc = lc[a];
        if (have) {  // (lane 0 is no head: the carried group goes on)
          cv[a] = comb(kind[a], cv[a], tv);
          cc[a] += tc;
        } else {
          cv[a] = tv;
          cc[a] = tc;
        }
      }
      if (!have) {
        have = true;
        left_open = !head0;
      }
    }
    heads += (u64)__builtin_popcountll(m);
  }
  // (have: the range holds at least one chunk)  One group fills the range: its left slot; else the right-open group
  if (lane == 0) {
    agg_put<K>(S, T.k, left_open ? PUT_LEFT : PUT_RIGHT, w, cv, cc);
    S.rgrp()[w] = left_open ? kNoGroup : heads - 1;
  }
}

// Grid: the walk's, one wave per walk wave w.  A wave without a right-open group has nothing to do.  Group g = rgrp[w]
// has its head in wave w and the last position of w's range; it ends in wave wl = (start[g + 1] - 1) / 512, and the waves
// between hold nothing else: partial 0 is w's right slot, partial j > 0 the left slot of wave w + j.
template <int K>
__global__ __launch_bounds__(GA_THREADS) void agg_combine_kernel(AggOut T, AggSlots S, const u64* __restrict__ start, u64 n) {
  const int lane = threadIdx.x & 63;
  const u64 w = uniform64(((u64)blockIdx.x * GA_THREADS + threadIdx.x) >> 6);
  if (w >= S.waves) return;  // (wave-uniform, like every return here)
  const u64 g = uniform64(S.rgrp()[w]);
  if (g >= S.ng) return;
  const u64 e = uniform64(start[g + 1]);
  if (e == 0 || e > n) return;
  const u64 wl = (e - 1) / (u64)(64 * kWalkChunks);
  if (wl < w || wl >= S.waves) return;
  const u64 parts = wl - w + 1;
#pragma unroll
  for (int a = 0; a < K; a++) {
    if (a >= (int)T.k) continue;
    const u32 kind = comb_kind(desc_type(T.desc[a]), desc_op(T.desc[a]));
    u64 v = comb_identity(kind);
    u32 c = 0;
    for (u64 j = (u64)lane; j < parts; j += 64) {
      const ulonglong2 x = j ? S.slot<K>(w + j, 0)[a] : S.slot<K>(w, 1)[a];
      v = comb(kind, v, x.x);
      c += (u32)x.y;
    }
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {  // lane l: the partials of lanes l .. l + 2o - 1
      const u64 pv = __shfl_down(v, o, 64);
      const u32 pc = __shfl_down(c, o, 64);
      v = comb(kind, v, pv);
      c += pc;
    }
    if (lane == 0) {
      S.gacc<K>(g)[a] = v;
      S.gcnt<K>(g)[a] = c;
    }
  }
}

// Grid-stride over waves as cols_take_kernel: `base` stays a multiple of 64 and the loop condition wave-uniform, so a
// wave's ballot of "valid" is one word of the output bitmap (lanes past ng contribute the padding zeros).
template <int K>
__global__ __launch_bounds__(GA_THREADS) void agg_finish_kernel(AggOut T, AggSlots S, u64* __restrict__ acc_nulls) {
  __shared__ u32 red[GA_WAVES][kAggLaunch];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  u32 nulls[K];  // (wave-uniform: popcounts)
#pragma unroll
  for (int a = 0; a < K; a++) nulls[a] = 0;
  const u64 stride = (u64)gridDim.x * GA_THREADS;
  for (u64 base = (u64)blockIdx.x * GA_THREADS + (u64)(wv * 64); base < S.ng; base += stride) {
    const u64 g = base + (u64)lane;
    const bool in = g < S.ng;
    const u32 n_in = (u32)__builtin_popcountll(__ballot(in));
    u64 acc[K];
    u32 cnt[K];
#pragma unroll
    for (int a = 0; a < K; a++) {
      acc[a] = 0;
      cnt[a] = 0;
      if (a < (int)T.k && in) {
        acc[a] = S.gacc<K>(g)[a];
        cnt[a] = S.gcnt<K>(g)[a];
      }
    }
#pragma unroll
    for (int a = 0; a < K; a++) {
      if (a >= (int)T.k) continue;
      const u32 op = desc_op(T.desc[a]), type = desc_type(T.desc[a]);  // (uniform)
      const bool ok = in && (op == HMJ_AGG_COUNT || cnt[a] != 0);
      const u64 k = acc[a];
      u64 o;
      if (op == HMJ_AGG_COUNT) {
        o = (u64)cnt[a];
      } else if (op == HMJ_AGG_SUM) {
        o = k;
      } else if (op == HMJ_AGG_MEAN) {
        o = (u64)__double_as_longlong(__longlong_as_double((long long)k) / (double)(cnt[a] ? cnt[a] : 1u));
      } else if (type == HMJ_TYPE_F64) {
        o = k == (op == HMJ_AGG_MIN ? ~0ull : 0ull) ? 0x7ff8000000000000ull : (k >> 63) ? (k ^ kSign) : ~k;
      } else if (type == HMJ_TYPE_F32) {
        const u32 k32 = (u32)k;
        o = k == (op == HMJ_AGG_MIN ? ~0ull : 0ull) ? 0x7fc00000u : (k32 >> 31) ? (k32 ^ 0x80000000u) : ~k32;
      } else if (type <= HMJ_TYPE_I64) {
        o = k ^ kSign;
      } else {
        o = k;
      }
      if (!ok) o = 0;  // the bytes of a NULL slot are 0
      if (in) {
        switch (T.ow[a]) {  // (uniform)
          case 1: reinterpret_cast<unsigned char*>(T.dst[a])[g] = (unsigned char)o; break;
          case 2: reinterpret_cast<unsigned short*>(T.dst[a])[g] = (unsigned short)o; break;
          case 4: reinterpret_cast<u32*>(T.dst[a])[g] = (u32)o; break;
          default: reinterpret_cast<u64*>(T.dst[a])[g] = o;
        }
      }
      const u64 m = __ballot(ok);
      if (T.dval[a] && lane == 0) T.dval[a][base >> 6] = m;
      nulls[a] += n_in - (u32)__builtin_popcountll(m);
    }
  }
  if (lane == 0) {
#pragma unroll
    for (int a = 0; a < kAggLaunch; a++) red[wv][a] = 0;
#pragma unroll
    for (int a = 0; a < K; a++) red[wv][a] = nulls[a];
  }
  __syncthreads();
  if (threadIdx.x < kAggLaunch) {
    u64 t = 0;
    for (int k = 0; k < GA_WAVES; k++) t += red[k][threadIdx.x];
    if (t) atomicAdd(&acc_nulls[threadIdx.x], t);
  }
}

// ---- host side -----------------------------------------------------------------------------------------------------------
u32 out_width_of(u32 type, u32 op) { return op == HMJ_AGG_MIN || op == HMJ_AGG_MAX ? width_of(type) : 8u; }

int check_agg_args(hmj_ctx* c, const hmj_agg_src* src, u32 n_aggs, u64 n_rows, const hmj_agg_dst* dst, const hmj_group_agg_opts* opts) {
  char msg[192];
  if (!src || !dst || !opts) return fail(c, HMJ_E_ARG, "hmj_group_agg_device: src / dst / opts is NULL");
  if (opts->struct_size < offsetof(hmj_group_agg_opts, reserved) + sizeof(opts->reserved))
    return fail(c, HMJ_E_ARG, "hmj_group_agg_opts.struct_size too small");
  if (opts->reserved) return fail(c, HMJ_E_ARG, "hmj_group_agg_opts: reserved must be 0");
  if (n_aggs < 1 || n_aggs > HMJ_MAX_AGGS) {
    std::snprintf(msg, sizeof(msg), "hmj_group_agg_device: n_aggs must be in 1..%d", HMJ_MAX_AGGS);
    return fail(c, HMJ_E_ARG, msg);
  }
  const GroupWs& ws = c->grp_ws;
  if (!ws.live)
    return fail(c, HMJ_E_ARG, "hmj_group_agg_device: no live grouping (the last group call must have returned HMJ_OK with HMJ_MATERIALIZE)");
  if (n_rows != ws.live_rows) {
    std::snprintf(msg, sizeof(msg), "hmj_group_agg_device: n_rows is %llu, the live grouping has %llu rows", (unsigned long long)n_rows,
                  (unsigned long long)ws.live_rows);
    return fail(c, HMJ_E_ARG, msg);
  }
  const u64 ng = ws.live_groups;
  for (u32 a = 0; a < n_aggs; a++) {
    const hmj_agg_src& s = src[a];
    const hmj_agg_dst& d = dst[a];
    if (s.type > HMJ_TYPE_F64) {
      std::snprintf(msg, sizeof(msg), "hmj_group_agg_device: aggregate %u has unknown type %u", a, s.type);
      return fail(c, HMJ_E_ARG, msg);
    }
    if (s.op > HMJ_AGG_MEAN) {
      std::snprintf(msg, sizeof(msg), "hmj_group_agg_device: aggregate %u has unknown op %u", a, s.op);
      return fail(c, HMJ_E_ARG, msg);
    }
    const u32 w = width_of(s.type), ow = out_width_of(s.type, s.op);
    if (n_rows > 0 && !s.data && s.op != HMJ_AGG_COUNT) {
      std::snprintf(msg, sizeof(msg), "hmj_group_agg_device: aggregate %u: source data is NULL", a);
      return fail(c, HMJ_E_ARG, msg);
    }
    if (n_rows > 0 && ((uintptr_t)s.data & (uintptr_t)(w - 1))) {
      std::snprintf(msg, sizeof(msg), "hmj_group_agg_device: aggregate %u: source data is not aligned to its width (%u)", a, w);
      return fail(c, HMJ_E_ARG, msg);
    }
    if (validity_overflows(s.validity, n_rows)) {
      std::snprintf(msg, sizeof(msg), "hmj_group_agg_device: aggregate %u: validity bit_offset + n_rows overflows 64 bits", a);
      return fail(c, HMJ_E_ARG, msg);
    }
    if (ng > 0 && !d.data) {
      std::snprintf(msg, sizeof(msg), "hmj_group_agg_device: aggregate %u: destination data is NULL", a);
      return fail(c, HMJ_E_ARG, msg);
    }
    if ((uintptr_t)d.data & (uintptr_t)(ow - 1)) {
      std::snprintf(msg, sizeof(msg), "hmj_group_agg_device: aggregate %u: destination data is not aligned to its width (%u)", a, ow);
      return fail(c, HMJ_E_ARG, msg);
    }
    if ((uintptr_t)d.validity & 7u) {
      std::snprintf(msg, sizeof(msg), "hmj_group_agg_device: aggregate %u: destination validity is not aligned to 8 bytes", a);
      return fail(c, HMJ_E_ARG, msg);
    }
  }
  // A destination the kernels write must not be something they read, nor another destination: address ranges only, as
  // hmj_take_cols_device checks them; without groups nothing is written.
  if (ng == 0) return HMJ_OK;
  Range in[2 * HMJ_MAX_AGGS], out[2 * HMJ_MAX_AGGS];
  for (u32 a = 0; a < n_aggs; a++) {
    in[2 * a] = range_of(src[a].data, n_rows * width_of(src[a].type));
    in[2 * a + 1] = validity_range(src[a].validity, n_rows);
    out[2 * a] = range_of(dst[a].data, ng * out_width_of(src[a].type, src[a].op));
    out[2 * a + 1] = range_of(dst[a].validity, 8 * ((ng + 63) / 64));
  }
  for (u32 a = 0; a < n_aggs; a++) {
    if (first_overlap(out + 2 * a, 2, in, 2 * (int)n_aggs) || first_overlap(out + 2 * a, 2, out, 2 * (int)n_aggs)) {
      std::snprintf(msg, sizeof(msg), "hmj_group_agg_device: aggregate %u: the destination overlaps a source column, a source bitmap or another destination",
                    a);
      return fail(c, HMJ_E_ARG, msg);
    }
  }
  return HMJ_OK;
}

template <int K>
int launch_chunk(hmj_ctx* c, const AggIn& T, const AggOut& O, const AggSlots& S, u64 n, u64* acc_nulls) {
  const GroupWs& ws = c->grp_ws;
  const dim3 walk((u32)((S.waves + GA_WAVES - 1) / GA_WAVES)), B(GA_THREADS);
  hipLaunchKernelGGL(agg_walk_kernel<K>, walk, B, 0, c->stream, T, S, (const ulonglong2*)ws.sorted.p, n, (const u64*)ws.flags.p,
                     (const u64*)ws.blk_off.p);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(agg_combine_kernel<K>, walk, B, 0, c->stream, O, S, (const u64*)ws.start.p, n);
  HIP_TRY(hipGetLastError());
  const u64 need = (S.ng + GA_THREADS - 1) / GA_THREADS, most = (u64)c->num_cus * 16;
  hipLaunchKernelGGL(agg_finish_kernel<K>, dim3((u32)(need < most ? need : most)), B, 0, c->stream, O, S, acc_nulls);
  HIP_TRY(hipGetLastError());
  return HMJ_OK;
}

int group_agg(hmj_ctx* c, const hmj_agg_src* src, u32 n_aggs, u64 n, hmj_agg_dst* dst, hmj_group_agg_opts* o) {
  const u64 ng = c->grp_ws.live_groups;
  const u64 waves = ((n + 63) / 64 + kWalkChunks - 1) / kWalkChunks;
  AggWs& ws = c->agg_ws;
  RC_TRY(ensure_dev(c, ws.acc, HMJ_MAX_AGGS * sizeof(u64)));
  RC_TRY(ensure_dev(c, ws.grp, AggSlots::grp_bytes(ng)));
  RC_TRY(ensure_dev(c, ws.part, AggSlots::part_bytes(waves)));
  u64* acc = (u64*)ws.acc.p;
  AggSlots S;
  S.ng = ng;
  S.waves = waves;
  S.grp = (u64*)ws.grp.p;
  S.part = (ulonglong2*)ws.part.p;
  HIP_TRY(hipMemsetAsync(acc, 0, HMJ_MAX_AGGS * sizeof(u64), c->stream));
  RC_TRY(ws.ev.record(c, 0));
  for (u32 a0 = 0; a0 < n_aggs; a0 += kAggLaunch) {
    AggIn T;
    AggOut O;
    std::memset(&T, 0, sizeof(T));
    std::memset(&O, 0, sizeof(O));
    T.k = O.k = n_aggs - a0 < (u32)kAggLaunch ? n_aggs - a0 : (u32)kAggLaunch;
    for (u32 a = 0; a < T.k; a++) {
      const hmj_agg_src& s = src[a0 + a];
      T.src[a] = s.data;
      T.vbits[a] = (const unsigned char*)s.validity.bits;
      T.voff[a] = s.validity.bit_offset;
      O.dst[a] = dst[a0 + a].data;
      O.dval[a] = (u64*)dst[a0 + a].validity;
      O.ow[a] = out_width_of(s.type, s.op);
      u32 dup = 0;
      if (a > 0) {
        const hmj_agg_src& p = src[a0 + a - 1];
        const bool counts = s.op == HMJ_AGG_COUNT || p.op == HMJ_AGG_COUNT;  // (COUNT loads nothing)
        dup = (!counts && s.data == p.data && s.type == p.type ? 1u : 0u) |
              (s.validity.bits && s.validity.bits == p.validity.bits && s.validity.bit_offset == p.validity.bit_offset ? 2u : 0u);
      }
      T.desc[a] = O.desc[a] = s.type | (s.op << 8) | (dup << 16);
    }
    if (T.k <= 1) RC_TRY(launch_chunk<1>(c, T, O, S, n, acc + a0));
    else if (T.k <= 2) RC_TRY(launch_chunk<2>(c, T, O, S, n, acc + a0));
    else RC_TRY(launch_chunk<kAggLaunch>(c, T, O, S, n, acc + a0));
  }
  RC_TRY(ws.ev.record(c, 1));
  u64 h[HMJ_MAX_AGGS];
  RC_TRY(read_back(c, acc, h, sizeof(h)));
  for (u32 a = 0; a < n_aggs; a++) dst[a].null_count = h[a];
  if (c->profiling) o->ms_agg = ws.ev.ms(0, 1);
  return HMJ_OK;
}

}  // namespace

extern "C" {

int hmj_group_agg_device(hmj_ctx* c, const hmj_agg_src* src, uint32_t n_aggs, uint64_t n_rows, hmj_agg_dst* dst,
                         hmj_group_agg_opts* opts) {
  if (!c) return HMJ_E_ARG;
  RC_TRY(check_agg_args(c, src, n_aggs, n_rows, dst, opts));
  // the out fields of opts go to a full-size copy first; the caller gets the prefix its struct_size holds
  hmj_group_agg_opts o;
  opts_prefix_in(&o, opts);
  opts_clear_out(&o, opts, offsetof(hmj_group_agg_opts, n_groups));
  o.n_groups = c->grp_ws.live_groups;
  if (n_rows == 0 || o.n_groups == 0) {
    for (u32 a = 0; a < n_aggs; a++) dst[a].null_count = 0;
  } else {
    HIP_TRY(hipSetDevice(c->device));
    RC_TRY(group_agg(c, src, n_aggs, n_rows, dst, &o));
  }
  opts_prefix_out(opts, o);
  return HMJ_OK;
}

}  // extern "C"
