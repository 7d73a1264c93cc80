// String-key join on the device (hmj_hash_str_device, hmj_join_str_device; include/hmj.h).  The reference joins
// std::string keys through the same operator template (hashjoin.h:29 KeyValVec, hashjoin_bench.cc:109-143): it orders
// rows by std::hash of the key and breaks ties on the key (radix_hash.h:86-109).  Here:
//   1. str_hash_kernel   libstdc++'s _Hash_bytes of every key -> {hash, row} rows (16 bytes, what the u64 join takes);
//                        a wave's 64 keys are one contiguous byte span, staged in LDS with 16-byte loads;
//   2. the u64 join      join_device on those rows, HMJ_MATERIALIZE (+ HMJ_ORDERED): pairs of equal hash (hash, r_row, s_row);
//   3. str_verify_*      one lane per pair: lengths, then bytes, 8 at a time; survivors compacted (stable) with their
//                        payloads, or only counted / summed in the count modes;
//   4. collision order   ordered joins only: runs of equal hash whose build keys differ are sorted by key bytes in one
//                        workgroup each (a run beyond kRunCap rows is HMJ_E_UNSUPPORTED).
// The join kinds (hmj_join_kind_str_device) reuse 1, 3 and 4 and add (see join_str_kind below):
//   str_rep_verify_kernel  one lane per (representative, row) pair of a first-wins {hash,row} join: equal keys mark the
//                          row (one byte per row), different keys put it on the ambiguous list;
//   str_sweep_*_kernel     one lane per row of a relation: the rows its mark selects, counted / summed, then written in
//                          row order (stable) with their payload or the kind's fill;
//   str_sort_rows_kernel / str_gather_kernel   ordered kinds: (hash, index) rows for the u64 sort, columns gathered.
// NULL keys (validity bitmaps, calls that pass one only): str_valid_count_kernel counts the rows that have a key per
// workgroup, one scan places them, and str_hash_valid_kernel writes two arrays per relation: the dense rows the sweeps walk
// by row index (a NULL-key row: hash 0, row HMJ_STR_NO_ROW) and the compacted rows of the valid rows, which are all the u64
// joins see.  Row indices stay the caller's, so verification, marks and gathers are unchanged; ordered results emit the
// NULL-key rows into a tail behind the rows that are sorted (DESIGN.md "NULL keys on string keys").
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>

#include "hmj_ctx.h"

using hmj::u32;
using hmj::u64;
using namespace hmj_host;

namespace {

#define HIP_TRY(expr)                                           \
  do {                                                          \
    hipError_t _e = (expr);                                     \
    if (_e != hipSuccess) return fail(c, HMJ_E_HIP, #expr, _e); \
  } while (0)
#define RC_TRY(expr)                   \
  do {                                 \
    const int _rc = (expr);            \
    if (_rc != HMJ_OK) return _rc;     \
  } while (0)

constexpr u64 kMul = 0xc6a4a7935bd1e995ull;
constexpr u64 kSeed = 0xc70f6907ull;
constexpr int SH_THREADS = 256;
constexpr int SH_WAVES = SH_THREADS / 64;
constexpr int SH_STAGE = 4096;  // LDS bytes a wave stages its 64 keys in; a longer span: per-lane reads from global memory
constexpr int SV_THREADS = 256;
constexpr int kRunCap = 1024;  // rows of one mixed run the collision sort holds (one workgroup)
constexpr u64 kListCap = 1ull << 22;  // mismatching adjacent rows the collision search records
constexpr u64 kNoRow = ~0ull;         // HMJ_STR_NO_ROW
// str_acc slots (u64): [0] first row with decreasing offsets (~0 = none), [1] keys with bytes but chars == NULL,
// [2] mismatch list length, [3] error bits (1 = a mixed run beyond kRunCap, 2 = list overflow), [4] ambiguous rows and
// [5] pairs whose keys differ (join kinds), [8..15] ACC_* sums
enum { SA_BAD_ROW = 0, SA_NULL_CHARS, SA_LIST_N, SA_ERR, SA_AMB_N, SA_DIFF, SA_ACC = 8, SA_N = 16 };

__device__ __forceinline__ u64 shift_mix(u64 v) { return v ^ (v >> 47); }

// Reads the key bytes at byte position `pos` as little-endian 64-bit words through aligned 8-byte loads (word q = bytes
// [8q, 8q + 8) of the address space the loader LD sees).  A load never reaches beyond the 8-byte-aligned words that
// hold key bytes, so no load crosses into a page the key does not touch.
template <class LD>
struct KeyReader {
  LD ld;
  u64 q;     // aligned word holding the next byte
  u32 s;     // bit offset of the next byte in that word
  u64 cur;   // word q (valid when it holds key bytes)
  u64 left;  // key bytes not yet read
  __device__ __forceinline__ KeyReader(LD l, u64 pos, u64 len) : ld(l), q(pos >> 3), s((u32)(pos & 7) * 8u), cur(0), left(len) {
    if (len) cur = ld(q);
  }
  // the next 8 bytes (left >= 8)
  __device__ __forceinline__ u64 word() {
    u64 d;
    left -= 8;
    if (s == 0) {
      d = cur;
      q++;
      if (left) cur = ld(q);
    } else {
      const u64 nx = ld(q + 1);
      d = (cur >> s) | (nx << (64 - s));
      cur = nx;
      q++;
    }
    return d;
  }
  // the last 1..7 bytes (left < 8), zero-extended
  __device__ __forceinline__ u64 tail() {
    const u32 t = (u32)left;
    u64 d = cur >> s;
    if (s + 8u * t > 64u) d |= ld(q + 1) << (64 - s);
    left = 0;
    return d & ((1ull << (8u * t)) - 1ull);
  }
};
struct GlobalLd {
  __device__ __forceinline__ u64 operator()(u64 q) const { return *reinterpret_cast<const u64*>(q << 3); }
};
struct LdsLd {
  const u64* w;
  __device__ __forceinline__ u64 operator()(u64 q) const { return w[q]; }
};

// libstdc++ _Hash_bytes (64-bit size_t), i.e. std::hash<std::string>
template <class LD>
__device__ __forceinline__ u64 hash_bytes(LD ld, u64 pos, u64 len) {
  KeyReader<LD> rd(ld, pos, len);
  u64 h = kSeed ^ (len * kMul);
  for (u64 k = len >> 3; k; k--) {
    const u64 d = shift_mix(rd.word() * kMul) * kMul;
    h = (h ^ d) * kMul;
  }
  if (len & 7) h = (h ^ rd.tail()) * kMul;
  return shift_mix(shift_mix(h) * kMul);
}

__device__ __forceinline__ u64 fold_bits(u64 h, u32 bits) { return bits ? h >> (64 - bits) : h; }

// Per wave: 64 consecutive keys, bytes [offsets[i0], offsets[i0 + 64]).  Staged in LDS when the span's aligned 16-byte
// blocks fit SH_STAGE, else read per lane from global memory.  rows: out = {hash, row} x n, else bare hashes.  vals != NULL: their sum goes to acc[SA_ACC + ACC_SUM_P].
__global__ __launch_bounds__(SH_THREADS) void str_hash_kernel(const unsigned char* __restrict__ chars, const u64* __restrict__ offsets,
                                                              u64 n, u32 hash_bits, u64* __restrict__ out, int rows,
                                                              const u64* __restrict__ vals, u64* __restrict__ acc) {
  __shared__ u64 stage[SH_WAVES][SH_STAGE / 8 + 2];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const u64 i0 = ((u64)blockIdx.x * SH_WAVES + (u64)w) * 64ull;
  const u64 i = i0 + (u64)lane;
  const bool active = i < n;
  const u64 iend = i0 + 64 < n ? i0 + 64 : n;
  u64 o0 = 0, o1 = 0, s0 = 0, s1 = 0;
  if (i0 < n) {
    const u64 a = offsets[active ? i : n];
    const u64 e = offsets[iend];
    const u64 nxt = __shfl_down(a, 1, 64);
    o0 = a;
    o1 = lane == 63 ? e : nxt;
    if (i + 1 == iend) o1 = e;
    s0 = __shfl(a, 0, 64);
    s1 = e;
  }
  const bool bad = active && o1 < o0;
  const u64 bad_mask = __ballot(bad);
  if (bad_mask && lane == (int)__builtin_ctzll(bad_mask)) atomicMin(&acc[SA_BAD_ROW], i);
  const bool ok_wave = i0 < n && !bad_mask && s1 >= s0;
  if (ok_wave && !chars && s1 > s0 && lane == 0) atomicAdd(&acc[SA_NULL_CHARS], 1ull);
  const bool usable = ok_wave && (chars || s1 == s0);
  // stage the wave's span: 16-byte aligned loads covering [chars + s0, chars + s1)
  const uintptr_t b0 = usable ? ((uintptr_t)(chars + s0) & ~(uintptr_t)15) : 0;
  const u64 span_bytes = usable && s1 > s0 ? (u64)(((uintptr_t)(chars + s1) + 15) & ~(uintptr_t)15) - (u64)b0 : 0;
  const bool staged = usable && span_bytes <= (u64)SH_STAGE;
  if (staged) {
    const uint4* src = reinterpret_cast<const uint4*>(b0);
    uint4* dst = reinterpret_cast<uint4*>(&stage[w][0]);
    for (u32 k = (u32)lane; k < (u32)(span_bytes >> 4); k += 64) dst[k] = src[k];
  }
  if (vals && i0 < n) {
    const u64 vs = hmj::wave_sum_u64(active ? vals[i] : 0ull);
    if (lane == 0) atomicAdd(&acc[SA_ACC + hmj::ACC_SUM_P], vs);
  }
  __syncthreads();
  if (!usable || !active) return;
  const u64 len = o1 - o0;
  u64 h;
  if (staged) {
    h = hash_bytes(LdsLd{&stage[w][0]}, (u64)((uintptr_t)(chars + o0) - b0), len);
  } else {
    h = hash_bytes(GlobalLd{}, (u64)(uintptr_t)(chars + o0), len);
  }
  h = fold_bits(h, hash_bits);
  if (rows) {
    reinterpret_cast<ulonglong2*>(out)[i] = make_ulonglong2(h, i);
  } else {
    out[i] = h;
  }
}

// ---- NULL keys (validity bitmaps) ------------------------------------------------------------------------------------------
// One relation's Arrow validity bitmap (coljoin.hip's ColValid for the one key column a string relation has): row i has a
// key iff bit off + i (least-significant bit first) is set.  Only calls that pass a bitmap reach the two kernels below.
struct StrValid {
  const unsigned char* bits;
  u64 off;
};
__device__ __forceinline__ bool row_valid(const StrValid& V, u64 i) {
  const u64 b = V.off + i;
  return (V.bits[b >> 3] >> (b & 7)) & 1u;
}

// Pass 1 over the bitmap alone: one lane per row (eight lanes share a byte, a wave reads 8-9 consecutive bytes); the valid
// rows of workgroup b -- the 256 rows str_hash_valid_kernel's workgroup b hashes -- go to blk_cnt[b].
__global__ __launch_bounds__(SH_THREADS) void str_valid_count_kernel(StrValid V, u64 n, u64* __restrict__ blk_cnt) {
  __shared__ u32 wcnt[SH_WAVES];
  const u64 i = (u64)blockIdx.x * SH_THREADS + threadIdx.x;
  const bool ok = i < n && row_valid(V, i);
  const u64 m = __ballot(ok);
  if ((threadIdx.x & 63) == 0) wcnt[threadIdx.x >> 6] = (u32)__builtin_popcountll(m);
  __syncthreads();
  if (threadIdx.x == 0) {
    u64 t = 0;
    for (int k = 0; k < SH_WAVES; k++) t += wcnt[k];
    blk_cnt[blockIdx.x] = t;
  }
}

// Pass 2, str_hash_kernel for a relation with a bitmap: the same wave spans, staging and offset checks (a NULL slot's
// offsets must not decrease either, and its bytes are staged with the span; a NULL lane hashes nothing).  dense (NULL: not
// wanted): row i gets {hash, i}, a NULL-key row {0, HMJ_STR_NO_ROW} -- what the sweeps walk by row index.  comp: the valid
// rows' {hash, i}, workgroup b's at blk_off[b] in row order (the wave's ballot places a lane inside its wave, the per-wave
// counts in LDS the wave inside its workgroup); cap: rows comp holds.  No lane leaves before the second barrier: a lane
// that is inactive, NULL or in a wave whose offsets are unusable only takes no part in the ballot's count.  Such a wave
// reports its row as str_hash_kernel does and compacts nothing, so the rows behind it land in front of their places --
// inside comp, and in a call that fails.
__global__ __launch_bounds__(SH_THREADS) void str_hash_valid_kernel(const unsigned char* __restrict__ chars, const u64* __restrict__ offsets,
                                                                    u64 n, u32 hash_bits, StrValid V, u64* __restrict__ dense,
                                                                    u64* __restrict__ comp, u64 cap, const u64* __restrict__ blk_off,
                                                                    const u64* __restrict__ vals, u64* __restrict__ acc) {
  __shared__ u64 stage[SH_WAVES][SH_STAGE / 8 + 2];
  __shared__ u32 wcnt[SH_WAVES];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const u64 i0 = ((u64)blockIdx.x * SH_WAVES + (u64)w) * 64ull;
  const u64 i = i0 + (u64)lane;
  const bool active = i < n;
  const u64 iend = i0 + 64 < n ? i0 + 64 : n;
  u64 o0 = 0, o1 = 0, s0 = 0, s1 = 0;
  if (i0 < n) {
    const u64 a = offsets[active ? i : n];
    const u64 e = offsets[iend];
    const u64 nxt = __shfl_down(a, 1, 64);
    o0 = a;
    o1 = lane == 63 ? e : nxt;
    if (i + 1 == iend) o1 = e;
    s0 = __shfl(a, 0, 64);
    s1 = e;
  }
  const bool bad = active && o1 < o0;
  const u64 bad_mask = __ballot(bad);
  if (bad_mask && lane == (int)__builtin_ctzll(bad_mask)) atomicMin(&acc[SA_BAD_ROW], i);
  const bool ok_wave = i0 < n && !bad_mask && s1 >= s0;
  if (ok_wave && !chars && s1 > s0 && lane == 0) atomicAdd(&acc[SA_NULL_CHARS], 1ull);
  const bool usable = ok_wave && (chars || s1 == s0);
  const uintptr_t b0 = usable ? ((uintptr_t)(chars + s0) & ~(uintptr_t)15) : 0;
  const u64 span_bytes = usable && s1 > s0 ? (u64)(((uintptr_t)(chars + s1) + 15) & ~(uintptr_t)15) - (u64)b0 : 0;
  const bool staged = usable && span_bytes <= (u64)SH_STAGE;
  if (staged) {
    const uint4* src = reinterpret_cast<const uint4*>(b0);
    uint4* dst = reinterpret_cast<uint4*>(&stage[w][0]);
    for (u32 k = (u32)lane; k < (u32)(span_bytes >> 4); k += 64) dst[k] = src[k];
  }
  if (vals && i0 < n) {  // (every row's payload, NULL-key rows included)
    const u64 vs = hmj::wave_sum_u64(active ? vals[i] : 0ull);
    if (lane == 0) atomicAdd(&acc[SA_ACC + hmj::ACC_SUM_P], vs);
  }
  const bool ok = usable && active && row_valid(V, active ? i : 0);
  __syncthreads();
  u64 h = 0;
  if (ok) {
    const u64 len = o1 - o0;
    if (staged) {
      h = hash_bytes(LdsLd{&stage[w][0]}, (u64)((uintptr_t)(chars + o0) - b0), len);
    } else {
      h = hash_bytes(GlobalLd{}, (u64)(uintptr_t)(chars + o0), len);
    }
    h = fold_bits(h, hash_bits);
  }
  if (dense && active) reinterpret_cast<ulonglong2*>(dense)[i] = make_ulonglong2(h, ok ? i : kNoRow);
  const u64 m = __ballot(ok);
  if (lane == 0) wcnt[w] = (u32)__builtin_popcountll(m);
  __syncthreads();
  if (ok) {
    u64 pos = blk_off[blockIdx.x] + hmj::popc_below(m);
    for (int k = 0; k < w; k++) pos += wcnt[k];
    if (pos < cap) reinterpret_cast<ulonglong2*>(comp)[pos] = make_ulonglong2(h, i);
  }
}

// Lexicographic comparison of two keys as std::string::operator< compares them (unsigned bytes, then length).
__device__ __forceinline__ int key_cmp(const unsigned char* ca, const u64* oa, u64 ra, const unsigned char* cb, const u64* ob, u64 rb) {
  const u64 pa = oa[ra], la = oa[ra + 1] - pa, pb = ob[rb], lb = ob[rb + 1] - pb;
  const u64 m = la < lb ? la : lb;
  KeyReader<GlobalLd> A(GlobalLd{}, (u64)(uintptr_t)(ca + pa), m), B(GlobalLd{}, (u64)(uintptr_t)(cb + pb), m);
  while (A.left) {
    const u64 x = A.left >= 8 ? A.word() : A.tail();
    const u64 y = B.left >= 8 ? B.word() : B.tail();
    if (x != y) {
      const u32 sh = (u32)__builtin_ctzll(x ^ y) & ~7u;
      return ((x >> sh) & 0xFF) < ((y >> sh) & 0xFF) ? -1 : 1;
    }
  }
  return la < lb ? -1 : la > lb ? 1 : 0;
}
__device__ __forceinline__ bool key_eq(const unsigned char* ca, const u64* oa, u64 ra, const unsigned char* cb, const u64* ob, u64 rb) {
  if (oa[ra + 1] - oa[ra] != ob[rb + 1] - ob[rb]) return false;
  return key_cmp(ca, oa, ra, cb, ob, rb) == 0;
}

struct StrSide {
  const unsigned char* chars;
  const u64* offsets;
  const u64* vals;
};

// The join kinds' result rows: a row's key is the build key when r_row is present, else the probe key (rr == NULL: no
// r_row column, every row a probe row).
struct KeyRef {
  const unsigned char* chars;
  const u64* offsets;
  u64 row;
};
__device__ __forceinline__ KeyRef key_of(const StrSide& R, const StrSide& S, u64 r, u64 s) {
  return r != kNoRow ? KeyRef{R.chars, R.offsets, r} : KeyRef{S.chars, S.offsets, s};
}
__device__ __forceinline__ KeyRef row_key(const StrSide& R, const StrSide& S, const u64* rr, const u64* sr, u64 i) {
  return key_of(R, S, rr ? rr[i] : kNoRow, sr ? sr[i] : kNoRow);
}
__device__ __forceinline__ bool same_key(const KeyRef& a, const KeyRef& b) {
  return (a.offsets == b.offsets && a.row == b.row) || key_eq(a.chars, a.offsets, a.row, b.chars, b.offsets, b.row);
}

// Pass 1 of the verification.  MAT: one ballot word per wave (flags) and the survivors per workgroup (blk_cnt).
// Count modes (!MAT): counts, sums and checksums of the survivors straight into acc.  MARK (outer join kinds): the
// survivors' build and probe rows are marked (one byte per row; every writer stores 1).
template <bool MAT, bool MARK = false>
__global__ __launch_bounds__(SV_THREADS) void str_verify_kernel(const u64* __restrict__ hk, const u64* __restrict__ rr,
                                                                const u64* __restrict__ sr, u64 np, StrSide R, StrSide S,
                                                                u64* __restrict__ flags, u64* __restrict__ blk_cnt,
                                                                u64* __restrict__ acc, int checksum,
                                                                unsigned char* __restrict__ mark_r, unsigned char* __restrict__ mark_s) {
  __shared__ u64 red[8];
  if (threadIdx.x < 8) red[threadIdx.x] = 0;
  __syncthreads();  // (wave 0 zeroes red[]; every wave's lane 0 adds to red[0] below)
  const u64 j = (u64)blockIdx.x * SV_THREADS + threadIdx.x;
  bool keep = false;
  u64 r = 0, s = 0;
  if (j < np) {
    r = rr[j];
    s = sr[j];
    keep = key_eq(R.chars, R.offsets, r, S.chars, S.offsets, s);
    if (MARK && keep) {
      mark_r[r] = 1;
      mark_s[s] = 1;
    }
  }
  if (MAT) {
    const u64 m = __ballot(keep);
    const int lane = threadIdx.x & 63;
    if (lane == 0) {
      flags[j >> 6] = m;
      if (m) atomicAdd(&red[0], (u64)__builtin_popcountll(m));
    }
    __syncthreads();
    if (threadIdx.x == 0) blk_cnt[blockIdx.x] = red[0];
  } else {
    u64 v[6] = {0, 0, 0, 0, 0, 0};
    if (keep) {
      const u64 rv = R.vals[r], sv = S.vals[s];
      v[hmj::ACC_N] = 1;
      v[hmj::ACC_SUM_R] = rv;
      v[hmj::ACC_SUM_S] = sv;
      if (checksum) {
        const u64 t = hmj::tmix(hk[j], rv, sv);
        v[hmj::ACC_XOR] = t;
        v[hmj::ACC_MIX] = t;
      }
    }
    __syncthreads();
    hmj::block_accumulate(red, acc + SA_ACC, v, 1u << hmj::ACC_XOR);
  }
}

// Pass 2: the survivors of workgroup b go, in pair order, to rows [blk_off[b], ..) of the five result columns.
__global__ __launch_bounds__(SV_THREADS) void str_compact_kernel(const u64* __restrict__ hk, const u64* __restrict__ rr,
                                                                 const u64* __restrict__ sr, u64 np, StrSide R, StrSide S,
                                                                 const u64* __restrict__ flags, const u64* __restrict__ blk_off,
                                                                 u64* __restrict__ o_hash, u64* __restrict__ o_r, u64* __restrict__ o_s,
                                                                 u64* __restrict__ o_rv, u64* __restrict__ o_sv, u64* __restrict__ acc,
                                                                 int checksum) {
  __shared__ u64 red[8];
  if (threadIdx.x < 8) red[threadIdx.x] = 0;
  const u64 j = (u64)blockIdx.x * SV_THREADS + threadIdx.x;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  u64 v[6] = {0, 0, 0, 0, 0, 0};
  if (j < np) {
    const u64 m = flags[j >> 6];
    if ((m >> lane) & 1ull) {
      u64 pos = blk_off[blockIdx.x] + hmj::popc_below(m);
      const u64 f0 = ((u64)blockIdx.x * SV_THREADS) >> 6;
      for (int k = 0; k < w; k++) pos += (u64)__builtin_popcountll(flags[f0 + (u64)k]);
      const u64 h = hk[j], r = rr[j], s = sr[j];
      const u64 rv = R.vals[r], sv = S.vals[s];
      o_hash[pos] = h;
      o_r[pos] = r;
      o_s[pos] = s;
      o_rv[pos] = rv;
      o_sv[pos] = sv;
      v[hmj::ACC_SUM_R] = rv;
      v[hmj::ACC_SUM_S] = sv;
      if (checksum) {
        const u64 t = hmj::tmix(h, rv, sv);
        v[hmj::ACC_XOR] = t;
        v[hmj::ACC_MIX] = t;
      }
    }
  }
  __syncthreads();
  hmj::block_accumulate(red, acc + SA_ACC, v, 1u << hmj::ACC_XOR);
}

// Collision search (ordered): row i whose hash equals row i-1's but whose build key differs is recorded.  MIXED (join
// kinds): the rows' keys are row_key's (sr, S: the probe side).
template <bool MIXED = false>
__global__ __launch_bounds__(SV_THREADS) void str_mismatch_kernel(const u64* __restrict__ hk, const u64* __restrict__ rr, u64 n,
                                                                  StrSide R, u64* __restrict__ list, u64* __restrict__ acc,
                                                                  const u64* __restrict__ sr, StrSide S) {
  const u64 i = (u64)blockIdx.x * SV_THREADS + threadIdx.x + 1;
  if (i >= n) return;
  if (hk[i] != hk[i - 1]) return;
  if constexpr (MIXED) {
    if (same_key(row_key(R, S, rr, sr, i - 1), row_key(R, S, rr, sr, i))) return;
  } else {
    const u64 a = rr[i - 1], b = rr[i];
    if (a == b || key_eq(R.chars, R.offsets, a, R.chars, R.offsets, b)) return;
  }
  const u64 k = atomicAdd(&acc[SA_LIST_N], 1ull);
  if (k < kListCap) list[k] = i;
  else atomicOr(&acc[SA_ERR], 2ull);
}

// One lane per recorded row i: its run [s, e) of equal hash (binary searches on the ascending hash column).  The lane whose
// i is the FIRST mismatch of its run leads it (runs[2k], runs[2k + 1] = s, e); the others write an empty run.  A separate
// launch from the sort, so that no leader test reads rows another workgroup is moving.  MIXED as str_mismatch_kernel.
template <bool MIXED = false>
__global__ __launch_bounds__(SV_THREADS) void str_run_leader_kernel(const u64* __restrict__ hk, const u64* __restrict__ rr, u64 n,
                                                                    StrSide R, const u64* __restrict__ list, u64* __restrict__ runs,
                                                                    u64* __restrict__ acc, const u64* __restrict__ sr, StrSide S) {
  const u64 cnt = acc[SA_LIST_N] < kListCap ? acc[SA_LIST_N] : kListCap;
  for (u64 k = (u64)blockIdx.x * SV_THREADS + threadIdx.x; k < cnt; k += (u64)gridDim.x * SV_THREADS) {
    const u64 i = list[k], h = hk[i];
    u64 lo = 0, hi = i;  // first row with hash h
    while (lo < hi) {
      const u64 mid = (lo + hi) >> 1;
      if (hk[mid] < h) lo = mid + 1;
      else hi = mid;
    }
    const u64 s = lo;
    lo = i + 1;
    hi = n;  // first row past the run
    while (lo < hi) {
      const u64 mid = (lo + hi) >> 1;
      if (hk[mid] <= h) lo = mid + 1;
      else hi = mid;
    }
    const u64 e = lo;
    runs[2 * k] = 0;
    runs[2 * k + 1] = 0;
    if (e - s > (u64)kRunCap) {
      atomicOr(&acc[SA_ERR], 1ull);
      continue;
    }
    bool first = true;
    for (u64 t = s + 1; t < i && first; t++) {
      if constexpr (MIXED) {
        if (!same_key(row_key(R, S, rr, sr, t - 1), row_key(R, S, rr, sr, t))) first = false;
      } else {
        const u64 a = rr[t - 1], b = rr[t];
        if (a != b && !key_eq(R.chars, R.offsets, a, R.chars, R.offsets, b)) first = false;
      }
    }
    if (first) {
      runs[2 * k] = s;
      runs[2 * k + 1] = e;
    }
  }
}

// One workgroup per led run: rows sorted stably by build key bytes (rank = rows with a smaller key + rows before it with
// the same key), written back in place.  All rows of a run share the hash, so only r_row, s_row, rval, sval move.
// MIXED: by row_key (S: the probe side); a NULL column is absent (read as HMJ_STR_NO_ROW / 0, not written).
template <bool MIXED = false>
__global__ __launch_bounds__(SV_THREADS) void str_run_sort_kernel(const u64* __restrict__ runs, StrSide R, u64* __restrict__ o_r,
                                                                  u64* __restrict__ o_s, u64* __restrict__ o_rv,
                                                                  u64* __restrict__ o_sv, const u64* __restrict__ acc, StrSide S) {
  __shared__ u64 col[4][kRunCap];
  __shared__ u32 rank[kRunCap];
  const u64 cnt = acc[SA_LIST_N] < kListCap ? acc[SA_LIST_N] : kListCap;
  for (u64 k = blockIdx.x; k < cnt; k += gridDim.x) {
    const u64 s = runs[2 * k], e = runs[2 * k + 1];
    if (e <= s) continue;  // (uniform: not a leader)
    const u32 L = (u32)(e - s);
    for (u32 t = threadIdx.x; t < L; t += SV_THREADS) {
      if constexpr (MIXED) {
        col[0][t] = o_r ? o_r[s + t] : kNoRow;
        col[1][t] = o_s ? o_s[s + t] : kNoRow;
        col[2][t] = o_rv ? o_rv[s + t] : 0ull;
        col[3][t] = o_sv ? o_sv[s + t] : 0ull;
      } else {
        col[0][t] = o_r[s + t];
        col[1][t] = o_s[s + t];
        col[2][t] = o_rv[s + t];
        col[3][t] = o_sv[s + t];
      }
    }
    __syncthreads();
    for (u32 t = threadIdx.x; t < L; t += SV_THREADS) {
      u32 rk = 0;
      if constexpr (MIXED) {
        const KeyRef me = key_of(R, S, col[0][t], col[1][t]);
        for (u32 o = 0; o < L; o++) {
          const KeyRef other = key_of(R, S, col[0][o], col[1][o]);
          const int c = (other.offsets == me.offsets && other.row == me.row)
                            ? 0
                            : key_cmp(other.chars, other.offsets, other.row, me.chars, me.offsets, me.row);
          rk += (c < 0 || (c == 0 && o < t)) ? 1u : 0u;
        }
      } else {
        const u64 me = col[0][t];
        for (u32 o = 0; o < L; o++) {
          const u64 other = col[0][o];
          const int c = other == me ? 0 : key_cmp(R.chars, R.offsets, other, R.chars, R.offsets, me);
          rk += (c < 0 || (c == 0 && o < t)) ? 1u : 0u;
        }
      }
      rank[t] = rk;
    }
    __syncthreads();
    for (u32 t = threadIdx.x; t < L; t += SV_THREADS) {
      const u64 d = s + rank[t];
      if constexpr (MIXED) {
        if (o_r) o_r[d] = col[0][t];
        if (o_s) o_s[d] = col[1][t];
        if (o_rv) o_rv[d] = col[2][t];
        if (o_sv) o_sv[d] = col[3][t];
      } else {
        o_r[d] = col[0][t];
        o_s[d] = col[1][t];
        o_rv[d] = col[2][t];
        o_sv[d] = col[3][t];
      }
    }
    __syncthreads();
  }
}

// ---- join kinds --------------------------------------------------------------------------------------------------------
// One lane per pair of a first-wins {hash,row} join: row krow[j] of the side asked about (K) against row orow[j] of the
// other side (O), the one representative of its hash there.  Equal keys mark the K row (every writer stores 1).  Different
// keys: the pair counts in acc[SA_DIFF] and, when amb != NULL, the K row goes on the ambiguous list as a {hash, row} row
// (one counter add per wave) -- another O row of the same hash may still hold its key.
__global__ __launch_bounds__(SV_THREADS) void str_rep_verify_kernel(const u64* __restrict__ hk, const u64* __restrict__ orow,
                                                                    const u64* __restrict__ krow, u64 np, StrSide O, StrSide K,
                                                                    unsigned char* __restrict__ mark, u64* __restrict__ amb,
                                                                    u64* __restrict__ acc) {
  const u64 j = (u64)blockIdx.x * SV_THREADS + threadIdx.x;
  const int lane = threadIdx.x & 63;
  bool diff = false;
  u64 k = 0;
  if (j < np) {
    k = krow[j];
    if (key_eq(O.chars, O.offsets, orow[j], K.chars, K.offsets, k)) mark[k] = 1;
    else diff = true;
  }
  const u64 m = __ballot(diff);
  if (!m) return;
  u64 base = 0;
  if (lane == 0) {
    atomicAdd(&acc[SA_DIFF], (u64)__builtin_popcountll(m));
    if (amb) base = atomicAdd(&acc[SA_AMB_N], (u64)__builtin_popcountll(m));
  }
  base = __shfl(base, 0, 64);
  if (amb && diff) reinterpret_cast<ulonglong2*>(amb)[base + hmj::popc_below(m)] = make_ulonglong2(hk[j], k);
}

// A relation's rows as the kinds emit them: row i ({hash, i} in rows) is selected when (mark[i] != 0) == want.  probe: the
// row goes out as (hash, NO_ROW, i, fill, vals[i]), else as (hash, i, NO_ROW, vals[i], fill); NULL columns are not written.
// nulls (ordered results of a relation with a validity bitmap, whose NULL-key rows carry HMJ_STR_NO_ROW in rows): 0 = every
// selected row, 1 = only those with a key, 2 = only the NULL-key rows.
struct Sweep {
  const u64* rows;
  const unsigned char* mark;
  const u64* vals;
  u64 n, fill;
  u32 want, probe, nulls;
};
__device__ __forceinline__ bool sweep_sel(const Sweep& W, u64 i) {
  if (i >= W.n || (W.mark[i] != 0) != (W.want != 0)) return false;
  if (W.nulls == 0) return true;  // (uniform)
  return (W.rows[2 * i + 1] == kNoRow) == (W.nulls == 2);
}
__device__ __forceinline__ void sweep_vals(const Sweep& W, u64 i, u64& rv, u64& sv) {
  const u64 v = W.vals[i];
  rv = W.probe ? W.fill : v;
  sv = W.probe ? v : W.fill;
}

// Sweep pass 1.  MAT: selected rows per workgroup (blk_cnt).  Count modes: count, sums and checksums into acc.
template <bool MAT>
__global__ __launch_bounds__(SV_THREADS) void str_sweep_count_kernel(Sweep W, u64* __restrict__ blk_cnt, u64* __restrict__ acc,
                                                                     int checksum) {
  __shared__ u64 red[8];
  if (threadIdx.x < 8) red[threadIdx.x] = 0;
  __syncthreads();
  const u64 i = (u64)blockIdx.x * SV_THREADS + threadIdx.x;
  const bool sel = sweep_sel(W, i);
  if (MAT) {
    const u64 m = __ballot(sel);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(&red[0], (u64)__builtin_popcountll(m));
    __syncthreads();
    if (threadIdx.x == 0) blk_cnt[blockIdx.x] = red[0];
  } else {
    u64 v[6] = {0, 0, 0, 0, 0, 0};
    if (sel) {
      const u64 h = W.rows[2 * i];
      u64 rv, sv;
      sweep_vals(W, i, rv, sv);
      v[hmj::ACC_N] = 1;
      v[hmj::ACC_SUM_R] = rv;
      v[hmj::ACC_SUM_S] = sv;
      if (checksum) {
        const u64 t = hmj::tmix(h, rv, sv);
        v[hmj::ACC_XOR] = t;
        v[hmj::ACC_MIX] = t;
      }
    }
    hmj::block_accumulate(red, acc + SA_ACC, v, 1u << hmj::ACC_XOR);
  }
}

// Sweep pass 2: the selected rows of workgroup b go, in row order, to rows [blk_off[b], ..) of the result columns; count,
// sums and checksums into acc.
__global__ __launch_bounds__(SV_THREADS) void str_sweep_emit_kernel(Sweep W, const u64* __restrict__ blk_off, u64* __restrict__ o_hash,
                                                                    u64* __restrict__ o_r, u64* __restrict__ o_s, u64* __restrict__ o_rv,
                                                                    u64* __restrict__ o_sv, u64* __restrict__ acc, int checksum) {
  __shared__ u64 red[8];
  __shared__ u32 wcnt[SV_THREADS / 64];
  if (threadIdx.x < 8) red[threadIdx.x] = 0;
  const u64 i = (u64)blockIdx.x * SV_THREADS + threadIdx.x;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const bool sel = sweep_sel(W, i);
  const u64 m = __ballot(sel);
  if (lane == 0) wcnt[w] = (u32)__builtin_popcountll(m);
  __syncthreads();
  u64 v[6] = {0, 0, 0, 0, 0, 0};
  if (sel) {
    u64 pos = blk_off[blockIdx.x] + hmj::popc_below(m);
    for (int k = 0; k < w; k++) pos += wcnt[k];
    const u64 h = W.rows[2 * i];
    u64 rv, sv;
    sweep_vals(W, i, rv, sv);
    o_hash[pos] = h;
    if (o_r) o_r[pos] = W.probe ? kNoRow : i;
    if (o_s) o_s[pos] = W.probe ? i : kNoRow;
    if (o_rv) o_rv[pos] = rv;
    if (o_sv) o_sv[pos] = sv;
    v[hmj::ACC_N] = 1;
    v[hmj::ACC_SUM_R] = rv;
    v[hmj::ACC_SUM_S] = sv;
    if (checksum) {
      const u64 t = hmj::tmix(h, rv, sv);
      v[hmj::ACC_XOR] = t;
      v[hmj::ACC_MIX] = t;
    }
  }
  hmj::block_accumulate(red, acc + SA_ACC, v, 1u << hmj::ACC_XOR);
}

// Ordered kinds: (hash, index) rows for the stable u64 sort, then the five columns gathered in the sorted order.
__global__ __launch_bounds__(SV_THREADS) void str_sort_rows_kernel(const u64* __restrict__ hk, u64 n, u64* __restrict__ rows) {
  const u64 i = (u64)blockIdx.x * SV_THREADS + threadIdx.x;
  if (i < n) reinterpret_cast<ulonglong2*>(rows)[i] = make_ulonglong2(hk[i], i);
}
__global__ __launch_bounds__(SV_THREADS) void str_gather_kernel(const u64* __restrict__ sorted, u64 n, const u64* __restrict__ i_r,
                                                                const u64* __restrict__ i_s, const u64* __restrict__ i_rv,
                                                                const u64* __restrict__ i_sv, u64* __restrict__ o_hash,
                                                                u64* __restrict__ o_r, u64* __restrict__ o_s, u64* __restrict__ o_rv,
                                                                u64* __restrict__ o_sv) {
  const u64 j = (u64)blockIdx.x * SV_THREADS + threadIdx.x;
  if (j >= n) return;
  const ulonglong2 e = reinterpret_cast<const ulonglong2*>(sorted)[j];
  const u64 p = e.y;
  o_hash[j] = e.x;
  if (o_r) o_r[j] = i_r[p];
  if (o_s) o_s[j] = i_s[p];
  if (o_rv) o_rv[j] = i_rv[p];
  if (o_sv) o_sv[j] = i_sv[p];
}

}  // namespace

namespace {

constexpr int kStrJoinMemoKind = 15;  // workload_signature kind of the inner {hash,row} join (u64 joins 0, sorts 1, kinds 3..9,
                                      // string kinds 10..13, inner multi-column join 14, multi-column kinds 16..19)
constexpr u64 kNone = ~0ull;

int check_str_rel(hmj_ctx* c, const hmj_str_rel* r, const char* name) {
  char msg[128];
  if (!r) {
    std::snprintf(msg, sizeof(msg), "the %s relation is NULL", name);
    return fail(c, HMJ_E_ARG, msg);
  }
  if (r->n > 0xFFFFFFFFull) {
    std::snprintf(msg, sizeof(msg), "too many rows in the %s relation (at most 2^32-1)", name);
    return fail(c, HMJ_E_ARG, msg);
  }
  if (r->n > 0 && (!r->offsets || !r->vals)) {
    std::snprintf(msg, sizeof(msg), "%s relation: offsets / vals is NULL", name);
    return fail(c, HMJ_E_ARG, msg);
  }
  return HMJ_OK;
}

// acc: three blocks of SA_N words -- [0] build side's hashing, [1] probe side's hashing, [2] verification / collisions
int acc_reset(hmj_ctx* c, u64* acc) {
  HIP_TRY(hipMemsetAsync(acc, 0, 3 * SA_N * sizeof(u64), c->stream));
  HIP_TRY(hipMemsetAsync(acc + SA_BAD_ROW, 0xFF, sizeof(u64), c->stream));
  HIP_TRY(hipMemsetAsync(acc + SA_N + SA_BAD_ROW, 0xFF, sizeof(u64), c->stream));
  return HMJ_OK;
}

int launch_hash(hmj_ctx* c, const void* chars, const u64* offsets, u64 n, u32 bits, u64* out, bool rows, const u64* vals, u64* acc) {
  if (!n) return HMJ_OK;
  const u64 grid = (n + SH_THREADS - 1) / SH_THREADS;
  hipLaunchKernelGGL(str_hash_kernel, dim3((u32)grid), dim3(SH_THREADS), 0, c->stream, (const unsigned char*)chars, offsets, n, bits,
                     out, rows ? 1 : 0, vals, acc);
  HIP_TRY(hipGetLastError());
  return HMJ_OK;
}

// NULL keys: the {hash,row} rows of both relations in a call with bitmaps (VB / VP: NULL where a relation has none; such a
// relation goes through str_hash_kernel as always, and its dense rows are its join rows).  A relation with a bitmap: its
// valid rows counted per workgroup and scanned (str_vblk: nblk counts, then nblk + 1 offsets, the build side's first), then
// hashed into cmp (room for every row: no read-back between the passes) and, if `dense`, into the row-indexed str_rows_*.
// rows[2] / tot[2]: what the u64 joins take, and where on the device the number of those rows stands (NULL: every row).
int launch_hashes_valid(hmj_ctx* c, const hmj_str_rel* R, const hmj_str_rel* S, const StrValid* VB, const StrValid* VP, u32 bits, bool dense,
                        bool sum_probe, u64* acc, const void** rows, const u64** tot) {
  const hmj_str_rel* rel[2] = {R, S};
  const StrValid* V[2] = {VB, VP};
  DevBuf* plain[2] = {&c->str_rows_r, &c->str_rows_s};
  DevBuf* cmp[2] = {&c->str_cmp_r, &c->str_cmp_s};
  u64 nblk[2];
  for (int k = 0; k < 2; k++) nblk[k] = V[k] && rel[k]->n ? (rel[k]->n + SH_THREADS - 1) / SH_THREADS : 0;
  RC_TRY(ensure_dev(c, c->str_vblk, (2 * (nblk[0] + nblk[1]) + 2) * sizeof(u64)));
  u64* vblk = (u64*)c->str_vblk.p;
  for (int k = 0; k < 2; k++) {
    const u64 n = rel[k]->n;
    const u64* vals = k == 1 && sum_probe ? (const u64*)rel[k]->vals : nullptr;
    rows[k] = plain[k]->p;
    tot[k] = nullptr;
    if (!nblk[k]) {
      RC_TRY(launch_hash(c, rel[k]->chars, (const u64*)rel[k]->offsets, n, bits, (u64*)plain[k]->p, true, vals, acc + k * SA_N));
      continue;
    }
    u64 *cnt = vblk + (k ? 2 * nblk[0] + 1 : 0), *off = cnt + nblk[k];
    RC_TRY(ensure_dev(c, *cmp[k], 16 * n));
    hipLaunchKernelGGL(str_valid_count_kernel, dim3((u32)nblk[k]), dim3(SH_THREADS), 0, c->stream, *V[k], n, cnt);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hmj::launch_scan_u64(cnt, off, (u32)nblk[k], c->stream));
    hipLaunchKernelGGL(str_hash_valid_kernel, dim3((u32)nblk[k]), dim3(SH_THREADS), 0, c->stream, (const unsigned char*)rel[k]->chars,
                       (const u64*)rel[k]->offsets, n, bits, *V[k], dense ? (u64*)plain[k]->p : nullptr, (u64*)cmp[k]->p, n,
                       (const u64*)off, vals, acc + k * SA_N);
    HIP_TRY(hipGetLastError());
    rows[k] = cmp[k]->p;
    tot[k] = off + nblk[k];
  }
  return HMJ_OK;
}

// the hash kernel's verdict on one relation's offsets (h: its acc block, read back)
int hash_errors(hmj_ctx* c, const u64* h, const char* name) {
  char msg[160];
  if (h[SA_BAD_ROW] != kNone) {
    std::snprintf(msg, sizeof(msg), "%s relation: offsets decrease at row %llu (offsets[%llu] < offsets[%llu])", name,
                  (unsigned long long)h[SA_BAD_ROW], (unsigned long long)h[SA_BAD_ROW] + 1, (unsigned long long)h[SA_BAD_ROW]);
    return fail(c, HMJ_E_ARG, msg);
  }
  if (h[SA_NULL_CHARS]) {
    std::snprintf(msg, sizeof(msg), "%s relation: chars is NULL but keys have bytes", name);
    return fail(c, HMJ_E_ARG, msg);
  }
  return HMJ_OK;
}

int read_back(hmj_ctx* c, const void* dev, void* host, size_t bytes) {
  HIP_TRY(hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return HMJ_OK;
}

int record(hmj_ctx* c, int k) {
  if (!c->profiling) return HMJ_OK;
  if (!c->str_ev[k]) HIP_TRY(hipEventCreate(&c->str_ev[k]));
  HIP_TRY(hipEventRecord(c->str_ev[k], c->stream));
  return HMJ_OK;
}
float elapsed(hmj_ctx* c, int a, int b) {
  float ms = 0.f;
  if (c->str_ev[a] && c->str_ev[b] && hipEventElapsedTime(&ms, c->str_ev[a], c->str_ev[b]) != hipSuccess) {
    (void)hipGetLastError();
    ms = 0.f;
  }
  return ms;
}

// VB / VP: the relations' validity bitmaps, NULL where a relation has none (both NULL: the call without NULL keys, all
// hmj_join_str_device makes -- hmj_str_join_opts carries no bitmap; the INNER kind of hmj_join_kind_str_device passes its
// own).  n_null (with bitmaps): the NULL-key rows of the build and the probe side.
int join_str(hmj_ctx* c, const hmj_str_rel* R, const hmj_str_rel* S, uint32_t flags, hmj_str_join_opts* opts, hmj_str_result* out,
             const StrValid* VB = nullptr, const StrValid* VP = nullptr, u64* n_null = nullptr) {
  u64 nb = R->n, np = S->n;
  const u32 bits = opts->hash_bits;
  if (flags & HMJ_ORDERED) flags |= HMJ_MATERIALIZE;
  const bool mat = flags & HMJ_MATERIALIZE, ordered = flags & HMJ_ORDERED, checksum = flags & HMJ_CHECKSUM;
  c->prep.valid = false;  // like any other call, a string join discards a prepared build side
  RC_TRY(ensure_dev(c, c->str_acc, 3 * SA_N * sizeof(u64)));
  RC_TRY(ensure_dev(c, c->str_rows_r, 16 * (nb ? nb : 1)));
  RC_TRY(ensure_dev(c, c->str_rows_s, 16 * (np ? np : 1)));
  u64* acc = (u64*)c->str_acc.p;
  u64 h[3 * SA_N];
  // 1. {hash, row} rows of both relations (+ the probe payloads' sum)
  RC_TRY(record(c, 0));
  RC_TRY(acc_reset(c, acc));
  const void* rows[2] = {c->str_rows_r.p, c->str_rows_s.p};  // the rows the u64 join takes
  u64 nv[2] = {nb, np};                                       // ... and how many: the rows that have a key
  if (!VB && !VP) {
    RC_TRY(launch_hash(c, R->chars, (const u64*)R->offsets, nb, bits, (u64*)c->str_rows_r.p, true, nullptr, acc));
    RC_TRY(launch_hash(c, S->chars, (const u64*)S->offsets, np, bits, (u64*)c->str_rows_s.p, true, (flags & HMJ_SUM_PROBE) ? (const u64*)S->vals : nullptr,
                       acc + SA_N));
    RC_TRY(record(c, 1));
  } else {  // NULL keys: only the rows that have a key are joined (the inner join walks no relation by row: no dense rows)
    const u64* tot[2];
    RC_TRY(launch_hashes_valid(c, R, S, VB, VP, bits, false, flags & HMJ_SUM_PROBE, acc, rows, tot));
    RC_TRY(record(c, 1));
    for (int k = 0; k < 2; k++)
      if (tot[k]) HIP_TRY(hipMemcpyAsync(&nv[k], tot[k], sizeof(u64), hipMemcpyDeviceToHost, c->stream));
  }
  RC_TRY(read_back(c, acc, h, sizeof(h)));
  RC_TRY(hash_errors(c, h, "build"));
  RC_TRY(hash_errors(c, h + SA_N, "probe"));
  if (nv[0] > nb || nv[1] > np) return fail(c, HMJ_E_HIP, "string join: more valid rows counted than the relation holds");
  if (n_null) {
    n_null[0] = nb - nv[0];
    n_null[1] = np - nv[1];
  }
  nb = nv[0];  // from here on: the rows that have a key (every row in a call without bitmaps)
  np = nv[1];
  if (flags & HMJ_SUM_PROBE) out->sum_probe_all = h[SA_N + SA_ACC + hmj::ACC_SUM_P];
  if (nb == 0 || np == 0) {  // (nothing to join: no plan either)
    std::memset(&c->plan, 0, sizeof(c->plan));
    c->plan.struct_size = sizeof(c->plan);
    std::memset(&c->timing, 0, sizeof(c->timing));
    for (int k = 2; k < 5; k++) RC_TRY(record(c, k));
    return HMJ_OK;
  }
  // 2. the u64 join of the {hash, row} rows: pairs of equal hash as (hash, r_row, s_row), ordered by them if asked
  hmj_result inner;
  spans_reset(c);
  const int st = span_begin(c, K_TOTAL, -1);
  c->memo_kind = kStrJoinMemoKind;
  int rc = join_device(c, rows[0], nb, rows[1], np, HMJ_MATERIALIZE | (flags & HMJ_ORDERED), &inner, false);
  c->memo_kind = 0;
  span_end(c, st);
  if (c->profiling) {
    (void)hipStreamSynchronize(c->stream);
    spans_collect(c);
  }
  if (rc != HMJ_OK) return rc;
  RC_TRY(record(c, 2));
  const u64 n_pairs = inner.n_matches;
  opts->n_hash_pairs = n_pairs;
  // 3. key verification, payload gather, stable compaction (or the count modes' reduction)
  const StrSide RS{(const unsigned char*)R->chars, (const u64*)R->offsets, (const u64*)R->vals},
      SS{(const unsigned char*)S->chars, (const u64*)S->offsets, (const u64*)S->vals};
  const u64 *ik = (const u64*)inner.key, *ir = (const u64*)inner.rval, *is = (const u64*)inner.sval;
  const u64 nblk = (n_pairs + SV_THREADS - 1) / SV_THREADS;
  if (nblk > 0xFFFFFFFFull) return fail(c, HMJ_E_UNSUPPORTED, "string join: more than 2^40 pairs of equal hash");
  u64* acc_v = acc + 2 * SA_N;
  u64 n_out = 0;
  if (n_pairs && mat) {
    RC_TRY(ensure_dev(c, c->str_flags, nblk * (SV_THREADS / 64) * sizeof(u64)));
    RC_TRY(ensure_dev(c, c->str_blk, nblk * sizeof(u64)));
    RC_TRY(ensure_dev(c, c->str_blk_off, (nblk + 1) * sizeof(u64)));
    DevBuf* cols[5] = {&c->str_hash, &c->str_rrow, &c->str_srow, &c->str_rval, &c->str_sval};
    for (DevBuf* b : cols) RC_TRY(ensure_dev(c, *b, n_pairs * sizeof(u64)));
    hipLaunchKernelGGL(str_verify_kernel<true>, dim3((u32)nblk), dim3(SV_THREADS), 0, c->stream, ik, ir, is,
                       n_pairs, RS, SS, (u64*)c->str_flags.p, (u64*)c->str_blk.p, acc_v, 0, nullptr, nullptr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hmj::launch_scan_u64((const u64*)c->str_blk.p, (u64*)c->str_blk_off.p, (u32)nblk, c->stream));
    hipLaunchKernelGGL(str_compact_kernel, dim3((u32)nblk), dim3(SV_THREADS), 0, c->stream, ik, ir, is, n_pairs,
                       RS, SS, (const u64*)c->str_flags.p, (const u64*)c->str_blk_off.p, (u64*)c->str_hash.p, (u64*)c->str_rrow.p,
                       (u64*)c->str_srow.p, (u64*)c->str_rval.p, (u64*)c->str_sval.p, acc_v, checksum ? 1 : 0);
    HIP_TRY(hipGetLastError());
    RC_TRY(read_back(c, (const u64*)c->str_blk_off.p + nblk, &n_out, sizeof(u64)));
  } else if (n_pairs) {
    hipLaunchKernelGGL(str_verify_kernel<false>, dim3((u32)nblk), dim3(SV_THREADS), 0, c->stream, ik, ir, is,
                       n_pairs, RS, SS, nullptr, nullptr, acc_v, checksum ? 1 : 0, nullptr, nullptr);
    HIP_TRY(hipGetLastError());
  }
  RC_TRY(record(c, 3));
  // 4. ordered: runs of equal hash with different build keys, sorted by key bytes
  if (ordered && n_out > 1) {
    const u64 cap = n_out < kListCap ? n_out : kListCap;
    RC_TRY(ensure_dev(c, c->str_list, cap * sizeof(u64)));
    RC_TRY(ensure_dev(c, c->str_runs, 2 * cap * sizeof(u64)));
    const u64 g = (n_out - 1 + SV_THREADS - 1) / SV_THREADS;
    hipLaunchKernelGGL(str_mismatch_kernel<false>, dim3((u32)g), dim3(SV_THREADS), 0, c->stream, (const u64*)c->str_hash.p,
                       (const u64*)c->str_rrow.p, n_out, RS, (u64*)c->str_list.p, acc_v, nullptr, StrSide{});
    HIP_TRY(hipGetLastError());
    const u64 gl = (cap + SV_THREADS - 1) / SV_THREADS;
    hipLaunchKernelGGL(str_run_leader_kernel<false>, dim3((u32)(gl < 1024 ? gl : 1024)), dim3(SV_THREADS), 0, c->stream,
                       (const u64*)c->str_hash.p, (const u64*)c->str_rrow.p, n_out, RS, (const u64*)c->str_list.p,
                       (u64*)c->str_runs.p, acc_v, nullptr, StrSide{});
    HIP_TRY(hipGetLastError());
    const u64 gs = cap < (u64)(4 * c->num_cus) ? cap : (u64)(4 * c->num_cus);
    hipLaunchKernelGGL(str_run_sort_kernel<false>, dim3((u32)gs), dim3(SV_THREADS), 0, c->stream, (const u64*)c->str_runs.p, RS,
                       (u64*)c->str_rrow.p, (u64*)c->str_srow.p, (u64*)c->str_rval.p, (u64*)c->str_sval.p, (const u64*)acc_v,
                       StrSide{});
    HIP_TRY(hipGetLastError());
  }
  RC_TRY(record(c, 4));
  RC_TRY(read_back(c, acc_v, h, SA_N * sizeof(u64)));
  if (h[SA_ERR] & 1) return fail(c, HMJ_E_UNSUPPORTED, "string join: a run of equal hash with several distinct keys holds more than 1024 rows");
  if (h[SA_ERR] & 2) return fail(c, HMJ_E_UNSUPPORTED, "string join: more than 2^22 adjacent rows of equal hash with different keys");
  const u64* a = h + SA_ACC;
  out->n_matches = mat ? n_out : a[hmj::ACC_N];
  out->sum_r = a[hmj::ACC_SUM_R];
  out->sum_s = a[hmj::ACC_SUM_S];
  if (checksum) {
    out->xor_fold = a[hmj::ACC_XOR];
    out->mix_sum = a[hmj::ACC_MIX];
  }
  if (mat) {
    out->hash = (const uint64_t*)c->str_hash.p;
    out->r_row = (const uint64_t*)c->str_rrow.p;
    out->s_row = (const uint64_t*)c->str_srow.p;
    out->rval = (const uint64_t*)c->str_rval.p;
    out->sval = (const uint64_t*)c->str_sval.p;
  }
  opts->n_collisions = n_pairs - out->n_matches;
  return HMJ_OK;
}

// ---- join kinds (hmj_join_kind_str_device) -------------------------------------------------------------------------
// workload_signature kinds of the {hash,row} joins the kinds run (u64 joins 0, sorts 1, u64 kinds 3..9, inner multi-column
// join 14, inner string join 15, multi-column kinds 16..19): none of them teaches a join of another entry anything
constexpr int kMemoProbeRep = 10;  // first-wins join, probe rows against build representatives (probe SEMI / ANTI)
constexpr int kMemoBuildRep = 11;  // ... build rows against probe representatives (BUILD_SEMI / BUILD_ANTI)
constexpr int kMemoAmbiguous = 12; // the ambiguous rows against every row of their hash on the other side
constexpr int kMemoPairs = 13;     // the outer kinds' pair join
constexpr int kKindAccBlocks = 5;  // acc: [0] / [1] hashing, [2] verification, [3] probe sweep, [4] build sweep

int memo_join(hmj_ctx* c, const void* Rr, u64 nr, const void* Sr, u64 ns, uint32_t flags, int memo, hmj_result* out) {
  spans_reset(c);
  const int st = span_begin(c, K_TOTAL, -1);
  c->memo_kind = memo;
  const int rc = join_device(c, Rr, nr, Sr, ns, flags, out, false);
  c->memo_kind = 0;
  span_end(c, st);
  if (c->profiling) {
    (void)hipStreamSynchronize(c->stream);
    spans_collect(c);
  }
  return rc;
}

u64 blocks_of(u64 n) { return (n + SV_THREADS - 1) / SV_THREADS; }

// VB / VP: as join_str; o->n_build_null / n_probe_null are filled in a call with bitmaps.
int join_str_kind(hmj_ctx* c, const hmj_str_rel* R, const hmj_str_rel* S, uint32_t flags, hmj_str_kind_opts* o, hmj_str_result* out,
                  const StrValid* VB = nullptr, const StrValid* VP = nullptr) {
  const u64 nb = R->n, np = S->n;
  const u32 bits = o->hash_bits, kind = o->kind;
  if (flags & HMJ_ORDERED) flags |= HMJ_MATERIALIZE;
  const bool mat = flags & HMJ_MATERIALIZE, ordered = flags & HMJ_ORDERED, checksum = flags & HMJ_CHECKSUM;
  const bool bside = o->side == HMJ_KIND_BUILD_SIDE;
  // semi / anti of either side (HMJ_JOIN_SEMI == HMJ_BUILD_SEMI, HMJ_JOIN_ANTI == HMJ_BUILD_ANTI), else an outer kind
  const bool semi_anti = kind == HMJ_JOIN_SEMI || kind == HMJ_JOIN_ANTI;
  const bool sweep_p = bside ? kind == HMJ_FULL_OUTER : true;
  const bool sweep_b = bside;
  c->prep.valid = false;  // like any other call, a string join discards a prepared build side
  std::memset(&c->plan, 0, sizeof(c->plan));
  c->plan.struct_size = sizeof(c->plan);
  std::memset(&c->timing, 0, sizeof(c->timing));
  RC_TRY(ensure_dev(c, c->str_acc, kKindAccBlocks * SA_N * sizeof(u64)));
  RC_TRY(ensure_dev(c, c->str_rows_r, 16 * (nb ? nb : 1)));
  RC_TRY(ensure_dev(c, c->str_rows_s, 16 * (np ? np : 1)));
  RC_TRY(ensure_dev(c, c->str_mark_r, nb ? nb : 1));
  RC_TRY(ensure_dev(c, c->str_mark_s, np ? np : 1));
  u64* acc = (u64*)c->str_acc.p;
  u64* acc_v = acc + 2 * SA_N;
  u64 h[kKindAccBlocks * SA_N];
  // 1. {hash, row} rows of both relations (+ the probe payloads' sum), marks cleared
  RC_TRY(record(c, 0));
  HIP_TRY(hipMemsetAsync(acc, 0, kKindAccBlocks * SA_N * sizeof(u64), c->stream));
  HIP_TRY(hipMemsetAsync(acc + SA_BAD_ROW, 0xFF, sizeof(u64), c->stream));
  HIP_TRY(hipMemsetAsync(acc + SA_N + SA_BAD_ROW, 0xFF, sizeof(u64), c->stream));
  // (NULL keys: the dense rows stay indexed by row for the sweeps; the u64 joins take only the rows that have a key)
  const void* rows[2] = {c->str_rows_r.p, c->str_rows_s.p};
  u64 nv[2] = {nb, np};
  if (!VB && !VP) {
    RC_TRY(launch_hash(c, R->chars, (const u64*)R->offsets, nb, bits, (u64*)c->str_rows_r.p, true, nullptr, acc));
    RC_TRY(launch_hash(c, S->chars, (const u64*)S->offsets, np, bits, (u64*)c->str_rows_s.p, true,
                       (flags & HMJ_SUM_PROBE) ? (const u64*)S->vals : nullptr, acc + SA_N));
  } else {
    const u64* tot[2];
    RC_TRY(launch_hashes_valid(c, R, S, VB, VP, bits, true, flags & HMJ_SUM_PROBE, acc, rows, tot));
    for (int k = 0; k < 2; k++)
      if (tot[k]) HIP_TRY(hipMemcpyAsync(&nv[k], tot[k], sizeof(u64), hipMemcpyDeviceToHost, c->stream));
  }
  if (nb) HIP_TRY(hipMemsetAsync(c->str_mark_r.p, 0, nb, c->stream));
  if (np) HIP_TRY(hipMemsetAsync(c->str_mark_s.p, 0, np, c->stream));
  RC_TRY(record(c, 1));
  RC_TRY(read_back(c, acc, h, 2 * SA_N * sizeof(u64)));
  RC_TRY(hash_errors(c, h, "build"));
  RC_TRY(hash_errors(c, h + SA_N, "probe"));
  const u64 nvb = nv[0], nvp = nv[1];  // the rows that have a key
  if (nvb > nb || nvp > np) return fail(c, HMJ_E_HIP, "string join: more valid rows counted than the relation holds");
  if (VB || VP) {
    o->n_build_null = nb - nvb;
    o->n_probe_null = np - nvp;
  }
  if (flags & HMJ_SUM_PROBE) out->sum_probe_all = h[SA_N + SA_ACC + hmj::ACC_SUM_P];
  const StrSide RS{(const unsigned char*)R->chars, (const u64*)R->offsets, (const u64*)R->vals},
      SS{(const unsigned char*)S->chars, (const u64*)S->offsets, (const u64*)S->vals};
  unsigned char *mark_r = (unsigned char*)c->str_mark_r.p, *mark_s = (unsigned char*)c->str_mark_s.p;
  // 2. + 3. the {hash,row} join(s) and the key verification, which marks the rows that have a partner
  u64 n_pairs = 0;
  hmj_result inner;
  std::memset(&inner, 0, sizeof(inner));
  if (semi_anti) {
    // every row of the side asked about (K) meets the FIRST row of its hash on the other side (O), in row order
    const u64 nK = bside ? nvb : nvp, nO = bside ? nvp : nvb;
    const void *rowsK = bside ? rows[0] : rows[1], *rowsO = bside ? rows[1] : rows[0];
    const StrSide &KS = bside ? RS : SS, &OS = bside ? SS : RS;
    unsigned char* mark = bside ? mark_r : mark_s;
    if (nK && nO) {
      hmj_result rep;
      RC_TRY(memo_join(c, rowsO, nO, rowsK, nK, HMJ_MATERIALIZE | HMJ_FIRST_WINS, bside ? kMemoBuildRep : kMemoProbeRep, &rep));
      RC_TRY(record(c, 2));
      n_pairs = rep.n_matches;  // <= nK
      if (n_pairs) {
        RC_TRY(ensure_dev(c, c->str_amb, 16 * n_pairs));
        hipLaunchKernelGGL(str_rep_verify_kernel, dim3((u32)blocks_of(n_pairs)), dim3(SV_THREADS), 0, c->stream, (const u64*)rep.key,
                           (const u64*)rep.rval, (const u64*)rep.sval, n_pairs, OS, KS, mark, (u64*)c->str_amb.p, acc_v);
        HIP_TRY(hipGetLastError());
        RC_TRY(read_back(c, acc_v, h, SA_N * sizeof(u64)));
        const u64 n_amb = h[SA_AMB_N];
        if (n_amb) {  // (a real hash collision: a representative's key differs from the row's)
          hmj_result all;
          RC_TRY(memo_join(c, rowsO, nO, c->str_amb.p, n_amb, HMJ_MATERIALIZE, kMemoAmbiguous, &all));
          n_pairs += all.n_matches;
          if (all.n_matches) {
            hipLaunchKernelGGL(str_rep_verify_kernel, dim3((u32)blocks_of(all.n_matches)), dim3(SV_THREADS), 0, c->stream,
                               (const u64*)all.key, (const u64*)all.rval, (const u64*)all.sval, all.n_matches, OS, KS, mark,
                               nullptr, acc_v);
            HIP_TRY(hipGetLastError());
          }
        }
      }
    } else {
      RC_TRY(record(c, 2));
    }
  } else if (nvb && nvp) {
    RC_TRY(memo_join(c, rows[0], nvb, rows[1], nvp, HMJ_MATERIALIZE | (flags & HMJ_ORDERED), kMemoPairs, &inner));
    RC_TRY(record(c, 2));
    n_pairs = inner.n_matches;
  } else {
    RC_TRY(record(c, 2));
  }
  if (blocks_of(n_pairs) > 0xFFFFFFFFull) return fail(c, HMJ_E_UNSUPPORTED, "string join: more than 2^40 pairs of equal hash");
  o->n_hash_pairs = n_pairs;
  // result rows: the verified pairs (outer kinds), then the probe sweep's rows, then the build sweep's
  const u64 nblk_v = semi_anti ? 0 : blocks_of(n_pairs);
  const u64 nblk_p = sweep_p ? blocks_of(np) : 0, nblk_b = sweep_b ? blocks_of(nb) : 0;
  // ordered, NULL keys: the sweeps above take the rows that have a key, and a second launch per relation puts its NULL-key
  // rows (never marked: only the kinds that take unmarked rows emit them) into a tail behind everything that is sorted --
  // the build side's in r_row order, then the probe side's in s_row order
  const u32 want = kind == HMJ_JOIN_SEMI ? 1u : 0u;
  const bool split_b = ordered && VB, split_p = ordered && VP;
  const u64 nblk_tb = split_b && sweep_b && !want && nvb < nb ? blocks_of(nb) : 0;
  const u64 nblk_tp = split_p && sweep_p && !want && nvp < np ? blocks_of(np) : 0;
  const u64 nblk_m = nblk_v + nblk_p + nblk_b;  // workgroups of the rows that have a key
  const u64 nblk = nblk_m + nblk_tb + nblk_tp;
  if (nblk > 0xFFFFFFFFull) return fail(c, HMJ_E_UNSUPPORTED, "string join: more than 2^40 pairs of equal hash");
  const u64 cap = (semi_anti ? 0 : n_pairs) + (sweep_p ? np : 0) + (sweep_b ? nb : 0);
  DevBuf* cols[5] = {&c->str_hash, &c->str_rrow, &c->str_srow, &c->str_rval, &c->str_sval};
  if (mat) {
    RC_TRY(ensure_dev(c, c->str_flags, (nblk_v ? nblk_v : 1) * (SV_THREADS / 64) * sizeof(u64)));
    RC_TRY(ensure_dev(c, c->str_blk, (nblk ? nblk : 1) * sizeof(u64)));
    RC_TRY(ensure_dev(c, c->str_blk_off, (nblk + 1) * sizeof(u64)));
    for (DevBuf* b : cols) RC_TRY(ensure_dev(c, *b, (cap ? cap : 1) * sizeof(u64)));
  }
  const u64 *ik = (const u64*)inner.key, *ir = (const u64*)inner.rval, *is = (const u64*)inner.sval;
  if (nblk_v && mat) {
    hipLaunchKernelGGL((str_verify_kernel<true, true>), dim3((u32)nblk_v), dim3(SV_THREADS), 0, c->stream, ik, ir, is, n_pairs, RS,
                       SS, (u64*)c->str_flags.p, (u64*)c->str_blk.p, acc_v, 0, mark_r, mark_s);
    HIP_TRY(hipGetLastError());
  } else if (nblk_v) {
    hipLaunchKernelGGL((str_verify_kernel<false, true>), dim3((u32)nblk_v), dim3(SV_THREADS), 0, c->stream, ik, ir, is, n_pairs, RS,
                       SS, nullptr, nullptr, acc_v, checksum ? 1 : 0, mark_r, mark_s);
    HIP_TRY(hipGetLastError());
  }
  RC_TRY(record(c, 3));
  // 4. the sweeps: SEMI / BUILD_SEMI take the marked rows, every other kind the unmarked ones
  const u64 pfill = !semi_anti && (!bside || kind == HMJ_FULL_OUTER) ? o->probe_fill : 0ull;
  const u64 bfill = !semi_anti && bside ? o->build_fill : 0ull;
  const Sweep WP{(const u64*)c->str_rows_s.p, mark_s, SS.vals, np, pfill, want, 1u, split_p ? 1u : 0u};
  const Sweep WB{(const u64*)c->str_rows_r.p, mark_r, RS.vals, nb, bfill, want, 0u, split_b ? 1u : 0u};
  Sweep TP = WP, TB = WB;  // the tails' sweeps
  TP.nulls = TB.nulls = 2u;
  u64* acc_p = acc + 3 * SA_N;
  u64* acc_b = acc + 4 * SA_N;
  u64 n_out = 0, n_in = 0, n_main = 0;  // result rows; of those, verified pairs (materialising); rows in front of the NULL-key tail
  u64* oc[5] = {(u64*)c->str_hash.p, (u64*)c->str_rrow.p, (u64*)c->str_srow.p, (u64*)c->str_rval.p, (u64*)c->str_sval.p};
  if (semi_anti && !bside) oc[1] = oc[3] = nullptr;  // (hash, s_row, sval)
  if (semi_anti && bside) oc[2] = oc[4] = nullptr;   // (hash, r_row, rval)
  if (mat) {
    u64* blk = (u64*)c->str_blk.p;
    const u64* blk_off = (const u64*)c->str_blk_off.p;
    if (nblk_p)
      hipLaunchKernelGGL(str_sweep_count_kernel<true>, dim3((u32)nblk_p), dim3(SV_THREADS), 0, c->stream, WP, blk + nblk_v, nullptr, 0);
    if (nblk_b)
      hipLaunchKernelGGL(str_sweep_count_kernel<true>, dim3((u32)nblk_b), dim3(SV_THREADS), 0, c->stream, WB, blk + nblk_v + nblk_p,
                         nullptr, 0);
    if (nblk_tb)
      hipLaunchKernelGGL(str_sweep_count_kernel<true>, dim3((u32)nblk_tb), dim3(SV_THREADS), 0, c->stream, TB, blk + nblk_m, nullptr, 0);
    if (nblk_tp)
      hipLaunchKernelGGL(str_sweep_count_kernel<true>, dim3((u32)nblk_tp), dim3(SV_THREADS), 0, c->stream, TP, blk + nblk_m + nblk_tb,
                         nullptr, 0);
    HIP_TRY(hipGetLastError());
    if (nblk) HIP_TRY(hmj::launch_scan_u64(blk, (u64*)c->str_blk_off.p, (u32)nblk, c->stream));
    if (nblk_v) {
      hipLaunchKernelGGL(str_compact_kernel, dim3((u32)nblk_v), dim3(SV_THREADS), 0, c->stream, ik, ir, is, n_pairs, RS, SS,
                         (const u64*)c->str_flags.p, blk_off, oc[0], oc[1], oc[2], oc[3], oc[4], acc_v, checksum ? 1 : 0);
    }
    if (nblk_p)
      hipLaunchKernelGGL(str_sweep_emit_kernel, dim3((u32)nblk_p), dim3(SV_THREADS), 0, c->stream, WP, blk_off + nblk_v, oc[0], oc[1],
                         oc[2], oc[3], oc[4], acc_p, checksum ? 1 : 0);
    if (nblk_b)
      hipLaunchKernelGGL(str_sweep_emit_kernel, dim3((u32)nblk_b), dim3(SV_THREADS), 0, c->stream, WB, blk_off + nblk_v + nblk_p,
                         oc[0], oc[1], oc[2], oc[3], oc[4], acc_b, checksum ? 1 : 0);
    if (nblk_tb)
      hipLaunchKernelGGL(str_sweep_emit_kernel, dim3((u32)nblk_tb), dim3(SV_THREADS), 0, c->stream, TB, blk_off + nblk_m, oc[0], oc[1],
                         oc[2], oc[3], oc[4], acc_b, checksum ? 1 : 0);
    if (nblk_tp)
      hipLaunchKernelGGL(str_sweep_emit_kernel, dim3((u32)nblk_tp), dim3(SV_THREADS), 0, c->stream, TP, blk_off + nblk_m + nblk_tb,
                         oc[0], oc[1], oc[2], oc[3], oc[4], acc_p, checksum ? 1 : 0);
    HIP_TRY(hipGetLastError());
    if (nblk) {
      HIP_TRY(hipMemcpyAsync(&n_in, blk_off + nblk_v, sizeof(u64), hipMemcpyDeviceToHost, c->stream));
      if (nblk > nblk_m) HIP_TRY(hipMemcpyAsync(&n_main, blk_off + nblk_m, sizeof(u64), hipMemcpyDeviceToHost, c->stream));
      RC_TRY(read_back(c, blk_off + nblk, &n_out, sizeof(u64)));
      if (nblk == nblk_m) n_main = n_out;  // (no tail)
      if (n_main > n_out || n_out > cap) return fail(c, HMJ_E_HIP, "string join: the sweeps' offsets exceed the result's capacity");
    }
  } else {
    if (nblk_p)
      hipLaunchKernelGGL(str_sweep_count_kernel<false>, dim3((u32)nblk_p), dim3(SV_THREADS), 0, c->stream, WP, nullptr, acc_p,
                         checksum ? 1 : 0);
    if (nblk_b)
      hipLaunchKernelGGL(str_sweep_count_kernel<false>, dim3((u32)nblk_b), dim3(SV_THREADS), 0, c->stream, WB, nullptr, acc_b,
                         checksum ? 1 : 0);
    HIP_TRY(hipGetLastError());
  }
  RC_TRY(record(c, 4));
  // 5. ordered: a stable sort of (hash, index) rows, the columns gathered in that order, then runs of equal hash with
  // several keys sorted by key bytes.  (Outer kinds without unmatched rows are already in (hash, r_row, s_row) order.)
  // NULL keys: only the n_main rows in front of the tail are sorted; the tail is already in its order and is copied behind.
  if (ordered && n_main > 1) {
    if (n_main > n_in) {
      RC_TRY(ensure_dev(c, c->str_ord, 32 * n_main));
      u64* ord = (u64*)c->str_ord.p;
      hipLaunchKernelGGL(str_sort_rows_kernel, dim3((u32)blocks_of(n_main)), dim3(SV_THREADS), 0, c->stream, oc[0], n_main, ord);
      HIP_TRY(hipGetLastError());
      const hmj_plan_desc plan = c->plan;  // (the sort is not a join: hmj_last_plan / hmj_last_timing keep describing the last one)
      const hmj_timing timing = c->timing;
      const int rc = hmj_sort_u64_device(c, ord, n_main, ord + 2 * n_main);
      c->plan = plan;
      c->timing = timing;
      if (rc != HMJ_OK) return rc;
      DevBuf* kc[5] = {&c->str_khash, &c->str_krrow, &c->str_ksrow, &c->str_krval, &c->str_ksval};
      u64* nc[5];
      for (int k = 0; k < 5; k++) {
        nc[k] = nullptr;
        if (!oc[k]) continue;
        RC_TRY(ensure_dev(c, *kc[k], n_out * sizeof(u64)));
        nc[k] = (u64*)kc[k]->p;
      }
      hipLaunchKernelGGL(str_gather_kernel, dim3((u32)blocks_of(n_main)), dim3(SV_THREADS), 0, c->stream, (const u64*)(ord + 2 * n_main),
                         n_main, oc[1], oc[2], oc[3], oc[4], nc[0], nc[1], nc[2], nc[3], nc[4]);
      HIP_TRY(hipGetLastError());
      for (int k = 0; k < 5; k++) {
        if (nc[k] && n_out > n_main)
          HIP_TRY(hipMemcpyAsync(nc[k] + n_main, oc[k] + n_main, (n_out - n_main) * sizeof(u64), hipMemcpyDeviceToDevice, c->stream));
        oc[k] = nc[k];
      }
    }
    const u64 lcap = n_main < kListCap ? n_main : kListCap;
    RC_TRY(ensure_dev(c, c->str_list, lcap * sizeof(u64)));
    RC_TRY(ensure_dev(c, c->str_runs, 2 * lcap * sizeof(u64)));
    hipLaunchKernelGGL(str_mismatch_kernel<true>, dim3((u32)blocks_of(n_main - 1)), dim3(SV_THREADS), 0, c->stream, (const u64*)oc[0],
                       (const u64*)oc[1], n_main, RS, (u64*)c->str_list.p, acc_v, (const u64*)oc[2], SS);
    HIP_TRY(hipGetLastError());
    const u64 gl = blocks_of(lcap);
    hipLaunchKernelGGL(str_run_leader_kernel<true>, dim3((u32)(gl < 1024 ? gl : 1024)), dim3(SV_THREADS), 0, c->stream,
                       (const u64*)oc[0], (const u64*)oc[1], n_main, RS, (const u64*)c->str_list.p, (u64*)c->str_runs.p, acc_v,
                       (const u64*)oc[2], SS);
    HIP_TRY(hipGetLastError());
    const u64 gs = lcap < (u64)(4 * c->num_cus) ? lcap : (u64)(4 * c->num_cus);
    hipLaunchKernelGGL(str_run_sort_kernel<true>, dim3((u32)gs), dim3(SV_THREADS), 0, c->stream, (const u64*)c->str_runs.p, RS, oc[1],
                       oc[2], oc[3], oc[4], (const u64*)acc_v, SS);
    HIP_TRY(hipGetLastError());
  }
  RC_TRY(record(c, 5));
  RC_TRY(read_back(c, acc_v, h + 2 * SA_N, 3 * SA_N * sizeof(u64)));
  const u64 *av = h + 2 * SA_N, *ap = h + 3 * SA_N, *ab = h + 4 * SA_N;
  if (av[SA_ERR] & 1) return fail(c, HMJ_E_UNSUPPORTED, "string join: a run of equal hash with several distinct keys holds more than 1024 rows");
  if (av[SA_ERR] & 2) return fail(c, HMJ_E_UNSUPPORTED, "string join: more than 2^22 adjacent rows of equal hash with different keys");
  // the sweeps count their rows in their acc blocks; the verified pairs: the scan (materialising) or acc (count modes)
  const u64 n_p = ap[SA_ACC + hmj::ACC_N], n_b = ab[SA_ACC + hmj::ACC_N];
  if (!mat) n_in = av[SA_ACC + hmj::ACC_N];
  out->n_matches = n_in + n_p + n_b;
  out->sum_r = av[SA_ACC + hmj::ACC_SUM_R] + ap[SA_ACC + hmj::ACC_SUM_R] + ab[SA_ACC + hmj::ACC_SUM_R];
  out->sum_s = av[SA_ACC + hmj::ACC_SUM_S] + ap[SA_ACC + hmj::ACC_SUM_S] + ab[SA_ACC + hmj::ACC_SUM_S];
  if (checksum) {
    out->xor_fold = av[SA_ACC + hmj::ACC_XOR] ^ ap[SA_ACC + hmj::ACC_XOR] ^ ab[SA_ACC + hmj::ACC_XOR];
    out->mix_sum = av[SA_ACC + hmj::ACC_MIX] + ap[SA_ACC + hmj::ACC_MIX] + ab[SA_ACC + hmj::ACC_MIX];
  }
  if (mat) {
    out->hash = (const uint64_t*)oc[0];
    out->r_row = (const uint64_t*)oc[1];
    out->s_row = (const uint64_t*)oc[2];
    out->rval = (const uint64_t*)oc[3];
    out->sval = (const uint64_t*)oc[4];
  }
  o->n_collisions = semi_anti ? av[SA_DIFF] : n_pairs - n_in;
  // the counters the u64 entry of the kind fills
  hmj_kind_counts& k = o->counts;
  std::memset(&k, 0, sizeof(k));
  if (!bside) {
    k.n_probe_unmatched = kind == HMJ_JOIN_SEMI ? np - n_p : n_p;
    k.n_probe_matched = np - k.n_probe_unmatched;
  } else {
    k.n_build_unmatched = kind == HMJ_BUILD_SEMI ? nb - n_b : n_b;
    k.n_build_matched = nb - k.n_build_unmatched;
    if (kind == HMJ_FULL_OUTER) {
      k.n_probe_unmatched = n_p;
      k.n_probe_matched = np - n_p;
    }
  }
  return HMJ_OK;
}

// The validity bitmaps of a hmj_str_kind_opts whose struct_size covers them, as the kernels take them; *pb / *pp stay NULL
// for a relation without a bitmap (bits == NULL).
int opts_validity(hmj_ctx* c, const hmj_str_kind_opts* opts, const hmj_str_rel* build, const hmj_str_rel* probe, StrValid* VB, StrValid* VP,
                  const StrValid** pb, const StrValid** pp) {
  *pb = *pp = nullptr;
  if (opts->struct_size < offsetof(hmj_str_kind_opts, probe_validity) + sizeof(opts->probe_validity)) return HMJ_OK;
  const hmj_validity* v[2] = {&opts->build_validity, &opts->probe_validity};
  const hmj_str_rel* rel[2] = {build, probe};
  StrValid* V[2] = {VB, VP};
  const StrValid** pv[2] = {pb, pp};
  for (int k = 0; k < 2; k++) {
    if (!v[k]->bits) continue;
    if (v[k]->bit_offset > UINT64_MAX - rel[k]->n) {
      char msg[128];
      std::snprintf(msg, sizeof(msg), "%s relation: validity bit_offset + n overflows 64 bits", k ? "probe" : "build");
      return fail(c, HMJ_E_ARG, msg);
    }
    V[k]->bits = (const unsigned char*)v[k]->bits;
    V[k]->off = v[k]->bit_offset;
    *pv[k] = V[k];
  }
  return HMJ_OK;
}
// The out fields of a full-size copy o of the caller's opts are cleared from `counts` on; the in fields that lie behind them
// (the validity bitmaps) are the caller's again, as far as its struct_size holds them.
void clear_out_fields(hmj_str_kind_opts* o, const hmj_str_kind_opts* opts) {
  using T = hmj_str_kind_opts;
  std::memset(&o->counts, 0, sizeof(T) - offsetof(T, counts));
  const size_t lo = offsetof(T, build_validity), hi = offsetof(T, n_build_null);
  const size_t have = opts->struct_size < hi ? opts->struct_size : hi;
  if (have > lo) std::memcpy((char*)o + lo, (const char*)opts + lo, have - lo);
}

}  // namespace

extern "C" {

int hmj_hash_str_device(hmj_ctx* c, const void* chars, const uint64_t* offsets, uint64_t n, uint32_t hash_bits, uint64_t* hash_out_dev) {
  if (!c) return HMJ_E_ARG;
  if (n > 0xFFFFFFFFull) return fail(c, HMJ_E_ARG, "too many rows (at most 2^32-1)");
  if (hash_bits > 63) return fail(c, HMJ_E_ARG, "hash_bits > 63");
  if (n > 0 && (!offsets || !hash_out_dev)) return fail(c, HMJ_E_ARG, "offsets / hash_out_dev is NULL");
  c->prep.valid = false;  // like any other call, hashing discards a prepared build side
  if (n == 0) return HMJ_OK;
  HIP_TRY(hipSetDevice(c->device));
  RC_TRY(ensure_dev(c, c->str_acc, 3 * SA_N * sizeof(u64)));
  u64* acc = (u64*)c->str_acc.p;
  RC_TRY(acc_reset(c, acc));
  RC_TRY(launch_hash(c, chars, (const u64*)offsets, n, hash_bits, (u64*)hash_out_dev, false, nullptr, acc));
  u64 h[SA_N];
  RC_TRY(read_back(c, acc, h, sizeof(h)));
  return hash_errors(c, h, "the");
}

int hmj_join_str_device(hmj_ctx* c, const hmj_str_rel* build, const hmj_str_rel* probe, uint32_t flags, hmj_str_join_opts* opts,
                        hmj_str_result* out) {
  if (!c) return HMJ_E_ARG;
  if (!opts || !out) return fail(c, HMJ_E_ARG, "opts / out is NULL");
  if (opts->struct_size < offsetof(hmj_str_join_opts, hash_bits) + sizeof(opts->hash_bits))
    return fail(c, HMJ_E_ARG, "hmj_str_join_opts.struct_size too small");
  if (opts->hash_bits > 63) return fail(c, HMJ_E_ARG, "hash_bits > 63");
  if (flags & HMJ_FIRST_WINS) return fail(c, HMJ_E_ARG, "HMJ_FIRST_WINS is not defined for string joins");
  RC_TRY(check_str_rel(c, build, "build"));
  RC_TRY(check_str_rel(c, probe, "probe"));
  std::memset(out, 0, sizeof(*out));
  HIP_TRY(hipSetDevice(c->device));
  // the out fields of opts go to a full-size copy first; the caller gets the prefix its struct_size holds
  hmj_str_join_opts o;
  std::memset(&o, 0, sizeof(o));
  std::memcpy(&o, opts, opts->struct_size < sizeof(o) ? opts->struct_size : sizeof(o));
  const int rc = join_str(c, build, probe, flags, &o, out);
  if (rc != HMJ_OK) return rc;
  if (c->profiling) {
    (void)hipStreamSynchronize(c->stream);
    o.ms_hash = elapsed(c, 0, 1);
    o.ms_join = elapsed(c, 1, 2);
    o.ms_verify = elapsed(c, 2, 3);
    o.ms_order = elapsed(c, 3, 4);
  }
  const uint32_t room = opts->struct_size < sizeof(o) ? opts->struct_size : (uint32_t)sizeof(o);
  o.struct_size = opts->struct_size;
  std::memcpy(opts, &o, room);
  return HMJ_OK;
}

int hmj_join_kind_str_device(hmj_ctx* c, const hmj_str_rel* build, const hmj_str_rel* probe, uint32_t flags, hmj_str_kind_opts* opts,
                             hmj_str_result* out) {
  if (!c) return HMJ_E_ARG;
  if (!opts || !out) return fail(c, HMJ_E_ARG, "opts / out is NULL");
  if (opts->struct_size < offsetof(hmj_str_kind_opts, build_fill) + sizeof(opts->build_fill))
    return fail(c, HMJ_E_ARG, "hmj_str_kind_opts.struct_size too small");
  if (opts->side > HMJ_KIND_BUILD_SIDE) return fail(c, HMJ_E_ARG, "unknown join side");
  if (opts->side == HMJ_KIND_PROBE_SIDE ? opts->kind > HMJ_JOIN_PROBE_OUTER : (opts->kind < HMJ_BUILD_SEMI || opts->kind > HMJ_FULL_OUTER))
    return fail(c, HMJ_E_ARG, "unknown join kind");
  if (opts->hash_bits > 63) return fail(c, HMJ_E_ARG, "hash_bits > 63");
  if (flags & HMJ_FIRST_WINS) return fail(c, HMJ_E_ARG, "HMJ_FIRST_WINS is not defined for string joins");
  RC_TRY(check_str_rel(c, build, "build"));
  RC_TRY(check_str_rel(c, probe, "probe"));
  StrValid VB, VP;
  const StrValid *vb, *vp;
  RC_TRY(opts_validity(c, opts, build, probe, &VB, &VP, &vb, &vp));
  std::memset(out, 0, sizeof(*out));
  HIP_TRY(hipSetDevice(c->device));
  // the out fields of opts go to a full-size copy first; the caller gets the prefix its struct_size holds
  hmj_str_kind_opts o;
  std::memset(&o, 0, sizeof(o));
  std::memcpy(&o, opts, opts->struct_size < sizeof(o) ? opts->struct_size : sizeof(o));
  clear_out_fields(&o, opts);
  if (o.side == HMJ_KIND_PROBE_SIDE && o.kind == HMJ_JOIN_INNER) {  // exactly the inner string join
    hmj_str_join_opts jo;
    std::memset(&jo, 0, sizeof(jo));
    jo.struct_size = sizeof(jo);
    jo.hash_bits = o.hash_bits;
    u64 n_null[2] = {0, 0};
    RC_TRY(join_str(c, build, probe, flags, &jo, out, vb, vp, n_null));
    o.n_build_null = n_null[0];
    o.n_probe_null = n_null[1];
    o.n_hash_pairs = jo.n_hash_pairs;
    o.n_collisions = jo.n_collisions;
    if (c->profiling) {
      (void)hipStreamSynchronize(c->stream);
      o.ms_hash = elapsed(c, 0, 1);
      o.ms_join = elapsed(c, 1, 2);
      o.ms_verify = elapsed(c, 2, 3);
      o.ms_order = elapsed(c, 3, 4);
    }
  } else {
    RC_TRY(join_str_kind(c, build, probe, flags, &o, out, vb, vp));
    if (c->profiling) {
      (void)hipStreamSynchronize(c->stream);
      o.ms_hash = elapsed(c, 0, 1);
      o.ms_join = elapsed(c, 1, 2);
      o.ms_verify = elapsed(c, 2, 3);
      o.ms_emit = elapsed(c, 3, 4);
      o.ms_order = elapsed(c, 4, 5);
    }
  }
  const uint32_t room = opts->struct_size < sizeof(o) ? opts->struct_size : (uint32_t)sizeof(o);
  o.struct_size = opts->struct_size;
  std::memcpy(opts, &o, room);
  return HMJ_OK;
}

}  // extern "C"
