// Mixed keys on the device (hmj_join_mixed_device; include/hmj.h): the key is a tuple whose columns are Arrow large_string
// columns and fixed-width columns in any order (ON a.name = b.name AND a.day = b.day).  Nothing in the reference
// corresponds: its operator is a template over ONE Key with std::hash<Key> (hashjoin.h:33-56).  The call is the
// multi-column join's hashed form with a third key policy:
//   1. mix_key_kernel   every row -> {key64, row}: the multi-column join's mix64 chain over per-column 64-bit values, a
//                       fixed column contributing its zero-extended value and a string column libstdc++'s _Hash_bytes of
//                       its bytes (hash_bytes, hmj_strkey.h) -- the wave's byte span staged in LDS as str_hash_kernel
//                       stages it, the stage reused by the next string column.  One pass over every key column, one
//                       16-byte store per row.  The offsets of every string column are checked here (no decrease);
//   2. ... 5.           hmj_tuplejoin.h's tuple_join / tuple_join_kind, instantiated on MixPolicy: the u64 join(s) of the
//                       rows, verification, marks, sweeps, the ordered kinds' sort and the collision sort, all of them
//                       hmj_keyjoin.h's kernels on MixSide.
// The key policy (key_eq / key_cmp / payload on MixSide) compares fixed columns as coljoin.hip does and string columns
// as strjoin.hip does (bytes_cmp: aligned 8-byte loads that never leave the words holding key bytes).
// NULL-equals-NULL matching (HMJ_NULL_EQUAL with a bitmap): mix_key_kernel<false, true> keys every row, and the sequence
// runs on MixNeSide / MixNePolicy, whose key_eq / key_cmp read the bitmaps before any value, length or byte.
// Grouping (hmj_group_mixed_device): one relation's {key64, row} rows from mix_key_kernel<false, NE>, then hmj_group.h's
// group_rows on MixSide (no bitmap) / MixNeSide (some column has one), with MixGroupCheck reading the key kernel's verdict on
// the offsets back before any kernel compares tuples (DESIGN.md "Grouping rows by string and mixed keys").
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdio>
#include <cstring>
#include <type_traits>

#include "hmj_tuplejoin.h"
#include "hmj_group.h"
#include "hmj_strkey.h"

namespace {

constexpr int MK_THREADS = KJ_THREADS;  // workgroup b keys rows [256 b, 256 b + 256): the rows valid_count_kernel counted for it
constexpr int MK_WAVES = MK_THREADS / 64;
constexpr int MK_STAGE = 4096;  // LDS bytes a wave stages the 64 keys of one string column in (str_hash_kernel's SH_STAGE)

// One relation's key columns and payloads, passed to the kernels by value.  Column c is a string column when w[c] == 0
// (p[c]: its chars, off[c]: its n + 1 offsets), else a fixed-width column of w[c] bytes (p[c]: its values, off[c] NULL).
// Every loop over the columns is fully unrolled with a `c < k` guard, so the arrays are read at constant offsets.
struct MixSide {
  const void* p[kMaxCols];
  const u64* off[kMaxCols];
  u32 w[kMaxCols];
  u32 k;
  const u64* vals;  // NULL: the payload of row i is i
};
__device__ __forceinline__ u64 payload(const MixSide& A, u64 i) { return A.vals ? A.vals[i] : i; }

// The key policy of the shared kernels (hmj_keyjoin.h).  Both sides have the same column count, types and widths, so where
// a lane chooses its side at run time the first lane's are every lane's: the choice only selects the pointers.
// key_eq: all fixed columns, then every string column's length, then bytes -- a pair that differs in a cheap column never
// touches chars.
__device__ __forceinline__ bool key_eq(const MixSide& A, u64 a, const MixSide& B, u64 b) {
  bool eq = true;
  const int k = uniform(A.k);
#pragma unroll
  for (int c = 0; c < kMaxCols; c++) {
    const u32 w = uniform(A.w[c]);
    if (c < k && w && eq) eq = col_load(A.p[c], w, a) == col_load(B.p[c], w, b);
  }
#pragma unroll
  for (int c = 0; c < kMaxCols; c++) {
    const u32 w = uniform(A.w[c]);
    if (c < k && !w && eq) eq = A.off[c][a + 1] - A.off[c][a] == B.off[c][b + 1] - B.off[c][b];
  }
#pragma unroll
  for (int c = 0; c < kMaxCols; c++) {
    const u32 w = uniform(A.w[c]);
    if (c < k && !w && eq) {
      const u64 pa = A.off[c][a], pb = B.off[c][b], len = A.off[c][a + 1] - pa;
      eq = bytes_cmp((const unsigned char*)A.p[c] + pa, len, (const unsigned char*)B.p[c] + pb, len) == 0;
    }
  }
  return eq;
}
// strictly column by column: fixed columns as unsigned integers, string columns as std::string::operator<
__device__ __forceinline__ int key_cmp(const MixSide& A, u64 a, const MixSide& B, u64 b) {
  int r = 0;
  const int k = uniform(A.k);
#pragma unroll
  for (int c = 0; c < kMaxCols; c++) {
    const u32 w = uniform(A.w[c]);
    if (c < k && r == 0) {
      if (w) {
        const u64 x = col_load(A.p[c], w, a), y = col_load(B.p[c], w, b);
        if (x != y) r = x < y ? -1 : 1;
      } else {
        const u64 pa = A.off[c][a], la = A.off[c][a + 1] - pa, pb = B.off[c][b], lb = B.off[c][b + 1] - pb;
        r = bytes_cmp((const unsigned char*)A.p[c] + pa, la, (const unsigned char*)B.p[c] + pb, lb);
      }
    }
  }
  return r;
}

// NULL-equals-NULL matching (HMJ_NULL_EQUAL, calls that pass a bitmap only): the relation with its validity bitmaps.  A
// NULL slot is a value of its own that equals only the NULL slot of the same column -- not the valid empty string -- and
// sorts behind every valid value; neither the value nor the offsets under it are read.  The bitmap pointers are the lane's
// own where a lane chooses its side at run time; count, types and widths stay the first lane's.
struct MixNeSide {
  MixSide s;
  ColValid v;
};
__device__ __forceinline__ u64 payload(const MixNeSide& A, u64 i) { return payload(A.s, i); }
// key_eq: the validity of every column first, then MixSide's order over the columns valid on both sides
__device__ __forceinline__ bool key_eq(const MixNeSide& A, u64 a, const MixNeSide& B, u64 b) {
  bool eq = true;
  const int k = uniform(A.s.k);
  u32 nulls = 0;  // the columns NULL on both sides
#pragma unroll
  for (int c = 0; c < kMaxCols; c++) {
    if (c < k && eq) {
      const bool na = slot_null(A.v, c, a), nb = slot_null(B.v, c, b);
      eq = na == nb;
      if (na) nulls |= 1u << c;
    }
  }
#pragma unroll
  for (int c = 0; c < kMaxCols; c++) {
    const u32 w = uniform(A.s.w[c]);
    if (c < k && w && eq && !((nulls >> c) & 1u)) eq = col_load(A.s.p[c], w, a) == col_load(B.s.p[c], w, b);
  }
#pragma unroll
  for (int c = 0; c < kMaxCols; c++) {
    const u32 w = uniform(A.s.w[c]);
    if (c < k && !w && eq && !((nulls >> c) & 1u)) eq = A.s.off[c][a + 1] - A.s.off[c][a] == B.s.off[c][b + 1] - B.s.off[c][b];
  }
#pragma unroll
  for (int c = 0; c < kMaxCols; c++) {
    const u32 w = uniform(A.s.w[c]);
    if (c < k && !w && eq && !((nulls >> c) & 1u)) {
      const u64 pa = A.s.off[c][a], pb = B.s.off[c][b], len = A.s.off[c][a + 1] - pa;
      eq = bytes_cmp((const unsigned char*)A.s.p[c] + pa, len, (const unsigned char*)B.s.p[c] + pb, len) == 0;
    }
  }
  return eq;
}
// strictly column by column, NULLS LAST in each: two NULL slots tie
__device__ __forceinline__ int key_cmp(const MixNeSide& A, u64 a, const MixNeSide& B, u64 b) {
  int r = 0;
  const int k = uniform(A.s.k);
#pragma unroll
  for (int c = 0; c < kMaxCols; c++) {
    const u32 w = uniform(A.s.w[c]);
    if (c < k && r == 0) {
      const bool na = slot_null(A.v, c, a), nb = slot_null(B.v, c, b);
      if (na || nb) {
        r = (int)na - (int)nb;
      } else if (w) {
        const u64 x = col_load(A.s.p[c], w, a), y = col_load(B.s.p[c], w, b);
        if (x != y) r = x < y ? -1 : 1;
      } else {
        const u64 pa = A.s.off[c][a], la = A.s.off[c][a + 1] - pa, pb = B.s.off[c][b], lb = B.s.off[c][b + 1] - pb;
        r = bytes_cmp((const unsigned char*)A.s.p[c] + pa, la, (const unsigned char*)B.s.p[c] + pb, lb);
      }
    }
  }
  return r;
}

// What the key kernel reports per relation (err: 2 * kMaxCols words): [c] the first row of column c whose offsets decrease
// (~0: none), [kMaxCols + c] the waves of column c that hold key bytes under chars == NULL.
// NE: kNullWords more words behind them, from [kErrWords]: the rows with a NULL slot (count_null_rows).
constexpr int kErrWords = 2 * kMaxCols;

// One lane per row, workgroup b keys rows [256 b, 256 b + 256).  The columns are walked in a fully unrolled loop whose
// branches depend on kernel arguments only, so every barrier is reached by every lane of the workgroup; no lane returns
// before the last one.  A fixed column: one coalesced load per wave.  A string column, as str_hash_kernel: the wave reads
// its 65 offsets (none past offsets[n]), checks that they do not decrease, stages its byte span [offsets[i0],
// offsets[i0 + 64)) in its own MK_STAGE bytes of LDS with aligned 16-byte loads when the span's aligned blocks fit (else:
// per-lane reads from global memory), and every lane hashes its key.  The next string column reuses the stage behind a
// barrier.  A wave whose offsets are unusable in some column reports it in err and its rows' keys mean nothing: the call
// fails on the host before anything reads them.
// VALID == false: out[i] = {key64, i}.  VALID: cols_key_valid_kernel's outputs -- dense (NULL: not wanted): {key64, i}, a
// NULL-key row {0, HMJ_COLS_NO_ROW}; comp: the valid rows' {key64, i}, workgroup b's at blk_off[b] in row order; cap: rows
// comp holds.  A NULL-key lane hashes no bytes.  sum_probe: every row's payload (NULL-key rows too) into acc[KA_SUM_P].
// NE (HMJ_NULL_EQUAL; with VALID == false, whose dense output it keeps): every row has a key.  A column's validity bits of
// the wave's rows are one or two aligned 8-byte words, loaded once per wave (wave_valid_word; the branch on the column's
// bitmap pointer depends on kernel arguments only).  A NULL slot contributes v_c = 0: a fixed value is not loaded, a
// string's bytes are not hashed (the wave still stages its span and still checks the slot's offsets); the row's NULL
// columns (m: bit c for column c) are mixed in behind the last column.  The rows with m != 0 are counted into the words
// from err[kErrWords], one atomic per workgroup (count_null_rows).
template <bool VALID, bool NE = false>
__global__ __launch_bounds__(MK_THREADS) void mix_key_kernel(MixSide A, ColValid V, u64 n, u32 hash_bits, u64* __restrict__ out,
                                                             u64* __restrict__ comp, u64 cap, const u64* __restrict__ blk_off,
                                                             int sum_probe, u64* __restrict__ acc, u64* __restrict__ err) {
  __shared__ __align__(16) u64 stage[MK_WAVES][MK_STAGE / 8 + 2];
  __shared__ u64 red[MK_WAVES];
  __shared__ u32 wcnt[MK_WAVES];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const u64 i0 = ((u64)blockIdx.x * MK_WAVES + (u64)w) * 64ull;
  const u64 i = i0 + (u64)lane;
  const bool active = i < n;
  const u64 iend = i0 + 64 < n ? i0 + 64 : n;
  bool ok = active;  // the row has a key
  if (VALID) ok = active && row_valid(V, active ? i : 0);
  const u32 cnt = (u32)(iend > i0 ? iend - i0 : 0);  // rows of this wave
  u64 m = 0;                                         // NE: the row's NULL columns
  bool wave_ok = true;  // every string column of this wave had usable offsets
  bool staged_before = false;
  u64 h = (u64)A.k;
#pragma unroll
  for (int c = 0; c < kMaxCols; c++) {
    if (c < (int)A.k) {  // (kernel arguments: uniform over the grid)
      u64 v = 0;
      bool null = false;
      if (NE && V.bits[c] && cnt) null = !((wave_valid_word(V.bits[c], V.off[c], uniform64(i0), uniform(cnt)) >> lane) & 1ull);
      if (NE && null) m |= 1ull << c;
      if (A.w[c]) {
        if (active && !null) v = col_load(A.p[c], A.w[c], i);
      } else {
        const unsigned char* chars = (const unsigned char*)A.p[c];
        const u64* offsets = A.off[c];
        if (staged_before) __syncthreads();  // the previous string column's readers are done with the stage
        staged_before = true;
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
        if (bad_mask && lane == (int)__builtin_ctzll(bad_mask)) atomicMin(&err[c], i);
        const bool ok_wave = i0 < n && !bad_mask && s1 >= s0;
        if (ok_wave && !chars && s1 > s0 && lane == 0) atomicAdd(&err[kMaxCols + c], 1ull);
        const bool usable = ok_wave && (chars || s1 == s0);
        // stage the wave's span: 16-byte aligned loads covering [chars + s0, chars + s1)
        const uintptr_t b0 = usable ? ((uintptr_t)(chars + s0) & ~(uintptr_t)15) : 0;
        const u64 span_bytes = usable && s1 > s0 ? (u64)(((uintptr_t)(chars + s1) + 15) & ~(uintptr_t)15) - (u64)b0 : 0;
        const bool staged = usable && span_bytes <= (u64)MK_STAGE;
        if (staged) {
          const uint4* src = reinterpret_cast<const uint4*>(b0);
          uint4* dst = reinterpret_cast<uint4*>(&stage[w][0]);
          for (u32 q = (u32)lane; q < (u32)(span_bytes >> 4); q += 64) dst[q] = src[q];
        }
        __syncthreads();
        if (!usable) wave_ok = false;
        if (usable && ok && !null) {
          const u64 len = o1 - o0;
          if (staged) v = hash_bytes(LdsLd{&stage[w][0]}, (u64)((uintptr_t)(chars + o0) - b0), len);
          else v = hash_bytes(GlobalLd{}, (u64)(uintptr_t)(chars + o0), len);
        }
      }
      h = hmj::mix64(h + v + kGolden);
    }
  }
  if (NE && m) h = hmj::mix64(h + m + kGolden);
  h = fold_bits(h, hash_bits);
  if (NE) {
    const u64 with_null = __ballot(active && m != 0);
    if (lane == 0) wcnt[w] = (u32)__builtin_popcountll(with_null);
  }
  u64 sum = 0;
  if (sum_probe && active) sum = payload(A, i);
  if (sum_probe) {  // (uniform)
    sum = hmj::wave_sum_u64(sum);
    if (lane == 0) red[w] = sum;
  }
  if (!VALID) {
    if (active) reinterpret_cast<ulonglong2*>(out)[i] = make_ulonglong2(h, i);
    __syncthreads();
    if (NE && threadIdx.x == 0) {
      u64 t = 0;
      for (int q = 0; q < MK_WAVES; q++) t += wcnt[q];
      count_null_rows(err + kErrWords, t);
    }
  } else {
    ok = ok && wave_ok;
    const u64 key = ok ? h : 0ull;
    if (out && active) reinterpret_cast<ulonglong2*>(out)[i] = make_ulonglong2(key, ok ? i : kNoRow);
    const u64 m = __ballot(ok);
    if (lane == 0) wcnt[w] = (u32)__builtin_popcountll(m);
    __syncthreads();
    if (ok) {
      u64 pos = blk_off[blockIdx.x] + hmj::popc_below(m);
      for (int q = 0; q < w; q++) pos += wcnt[q];
      if (pos < cap) reinterpret_cast<ulonglong2*>(comp)[pos] = make_ulonglong2(key, i);
    }
  }
  if (sum_probe && threadIdx.x == 0) {
    u64 t = 0;
    for (int q = 0; q < MK_WAVES; q++) t += red[q];
    if (t) atomicAdd(&acc[KA_SUM_P], t);
  }
}

// ---- host side -----------------------------------------------------------------------------------------------------------
constexpr KeyJoinNames kNames{"mixed-key join", "key64", "tuples"};
constexpr u64 kNone = ~0ull;

// NE: the policy of HMJ_NULL_EQUAL calls that pass a bitmap -- MixNeSide, the NE key kernel, kNullWords more report words
// per relation.  The driver runs its no-bitmap path (every row has a key), so key_valid is never reached.  The {key64,row} joins
// keep the entry's memo kinds: what they learn about a relation's key64 distribution holds with and without the flag.
template <bool NE>
struct MixPolicyT {
  using Side = typename std::conditional<NE, MixNeSide, MixSide>::type;
  using Self = MixPolicyT<NE>;
  static constexpr bool kCanPack = false;     // the key is always hashed
  static constexpr int kRelWords = kErrWords + (NE ? kNullWords : 0);  // the key kernel's report on one relation
  static constexpr int kAccExtra = 2 * kRelWords;             // the build relation's, then the probe relation's
  // workload_signature kinds of the {key64,row} joins (u64 joins 0, sorts 1, kinds 3..9, string joins 10..13 and 15,
  // multi-column joins 14 and 16..19): mixed joins teach no other entry anything
  static constexpr int kMemoInner = 20;      // the inner join
  static constexpr int kMemoProbeRep = 21;   // first-wins join, probe rows against build representatives (probe SEMI / ANTI)
  static constexpr int kMemoBuildRep = 22;   // ... build rows against probe representatives (BUILD_SEMI / BUILD_ANTI)
  static constexpr int kMemoAmbiguous = 23;  // the ambiguous rows against every row of their key64 on the other side
  static constexpr int kMemoPairs = 24;      // the outer kinds' pair join
  static const KeyJoinNames& names() { return kNames; }
  static KeyJoinWs& ws(hmj_ctx* c) { return c->mix_ws; }
  static u64* err_of(hmj_ctx* c, int rel) { return tuple_acc_extra<Self>(c) + rel * kRelWords; }
  static int keys_begin(hmj_ctx* c) {
    u64* e = tuple_acc_extra<Self>(c);  // (the driver cleared the words)
    HIP_TRY(hipMemsetAsync(e, 0xFF, kMaxCols * sizeof(u64), c->stream));
    HIP_TRY(hipMemsetAsync(e + kRelWords, 0xFF, kMaxCols * sizeof(u64), c->stream));
    return HMJ_OK;
  }
  // The key kernels' verdict on both relations' string columns: the build relation first, the lowest-numbered column first.
  static int keys_check(hmj_ctx* c, TupleCall* call) {
    u64 e[kAccExtra];
    RC_TRY(read_back(c, tuple_acc_extra<Self>(c), e, sizeof(e)));
    if (NE) {
      call->n_build_null = null_rows_of(e + kErrWords);
      call->n_probe_null = null_rows_of(e + kRelWords + kErrWords);
    }
    char msg[192];
    for (int rel = 0; rel < 2; rel++) {
      const u64* r = e + rel * kRelWords;
      const char* name = rel ? "probe" : "build";
      for (int k = 0; k < kMaxCols; k++) {
        if (r[k] != kNone) {
          std::snprintf(msg, sizeof(msg), "%s relation: column %d: offsets decrease at row %llu (offsets[%llu] < offsets[%llu])", name, k,
                        (unsigned long long)r[k], (unsigned long long)r[k] + 1, (unsigned long long)r[k]);
          return fail(c, HMJ_E_ARG, msg);
        }
        if (r[kMaxCols + k]) {
          std::snprintf(msg, sizeof(msg), "%s relation: column %d: data is NULL but keys have bytes", name, k);
          return fail(c, HMJ_E_ARG, msg);
        }
      }
    }
    return HMJ_OK;
  }
  static int key(hmj_ctx* c, const Side& A, int rel, u64 n, const TupleCall& call, u64* out, bool sum_probe, u64* acc) {
    if (!n) return HMJ_OK;
    if constexpr (NE)
      hipLaunchKernelGGL((mix_key_kernel<false, true>), dim3((u32)blocks_of(n)), dim3(MK_THREADS), 0, c->stream, A.s, A.v, n, call.bits, out,
                         nullptr, 0ull, nullptr, sum_probe ? 1 : 0, acc, err_of(c, rel));
    else
      hipLaunchKernelGGL(mix_key_kernel<false>, dim3((u32)blocks_of(n)), dim3(MK_THREADS), 0, c->stream, A, ColValid{}, n, call.bits, out,
                         nullptr, 0ull, nullptr, sum_probe ? 1 : 0, acc, err_of(c, rel));
    HIP_TRY(hipGetLastError());
    return HMJ_OK;
  }
  static int key_valid(hmj_ctx* c, const Side& A, const ColValid& V, int rel, u64 n, const TupleCall& call, u64 nblk, u64* dense, u64* comp,
                       u64 cap, const u64* off, bool sum_probe, u64* acc) {
    if constexpr (NE) {
      return fail(c, HMJ_E_HIP, "mixed-key join: the NULL-equals-NULL form compacts no rows");
    } else {
      hipLaunchKernelGGL(mix_key_kernel<true>, dim3((u32)nblk), dim3(MK_THREADS), 0, c->stream, A, V, n, call.bits, dense, comp, cap, off,
                         sum_probe ? 1 : 0, acc, err_of(c, rel));
      HIP_TRY(hipGetLastError());
      return HMJ_OK;
    }
  }
};
using MixPolicy = MixPolicyT<false>;
using MixNePolicy = MixPolicyT<true>;

int check_mixed_rel(hmj_ctx* c, const hmj_mixed_rel* r, const char* name) {
  char msg[160];
  if (!r) {
    std::snprintf(msg, sizeof(msg), "the %s relation is NULL", name);
    return fail(c, HMJ_E_ARG, msg);
  }
  if (r->n_cols < 1 || r->n_cols > HMJ_MAX_KEY_COLS) {
    std::snprintf(msg, sizeof(msg), "%s relation: n_cols must be in 1..%d", name, HMJ_MAX_KEY_COLS);
    return fail(c, HMJ_E_ARG, msg);
  }
  if (!r->cols) {
    std::snprintf(msg, sizeof(msg), "%s relation: cols is NULL", name);
    return fail(c, HMJ_E_ARG, msg);
  }
  if (r->reserved) {
    std::snprintf(msg, sizeof(msg), "%s relation: reserved must be 0", name);
    return fail(c, HMJ_E_ARG, msg);
  }
  if (r->n > 0xFFFFFFFFull) {
    std::snprintf(msg, sizeof(msg), "too many rows in the %s relation (at most 2^32-1)", name);
    return fail(c, HMJ_E_ARG, msg);
  }
  for (u32 k = 0; k < r->n_cols; k++) {
    const hmj_mixed_col& col = r->cols[k];
    if (col.type == HMJ_KEY_FIXED) {
      if (col.width != 1 && col.width != 2 && col.width != 4 && col.width != 8) {
        std::snprintf(msg, sizeof(msg), "%s relation: column %u has width %u (1, 2, 4 or 8)", name, k, col.width);
        return fail(c, HMJ_E_ARG, msg);
      }
      if (col.offsets) {
        std::snprintf(msg, sizeof(msg), "%s relation: column %u: a fixed-width column has offsets", name, k);
        return fail(c, HMJ_E_ARG, msg);
      }
      if (r->n > 0 && !col.data) {
        std::snprintf(msg, sizeof(msg), "%s relation: column %u: data is NULL", name, k);
        return fail(c, HMJ_E_ARG, msg);
      }
      if (r->n > 0 && ((uintptr_t)col.data & (uintptr_t)(col.width - 1))) {
        std::snprintf(msg, sizeof(msg), "%s relation: column %u: data is not aligned to its width (%u)", name, k, col.width);
        return fail(c, HMJ_E_ARG, msg);
      }
    } else if (col.type == HMJ_KEY_LARGE_STRING) {
      if (col.width) {
        std::snprintf(msg, sizeof(msg), "%s relation: column %u: a string column has width %u (must be 0)", name, k, col.width);
        return fail(c, HMJ_E_ARG, msg);
      }
      if (r->n > 0 && !col.offsets) {
        std::snprintf(msg, sizeof(msg), "%s relation: column %u: offsets is NULL", name, k);
        return fail(c, HMJ_E_ARG, msg);
      }
      if ((uintptr_t)col.offsets & 7u) {
        std::snprintf(msg, sizeof(msg), "%s relation: column %u: offsets is not aligned to 8 bytes", name, k);
        return fail(c, HMJ_E_ARG, msg);
      }
    } else {
      std::snprintf(msg, sizeof(msg), "%s relation: column %u has unknown type %u", name, k, col.type);
      return fail(c, HMJ_E_ARG, msg);
    }
    if (col.validity.bits && col.validity.bit_offset > UINT64_MAX - r->n) {
      std::snprintf(msg, sizeof(msg), "%s relation: column %u: validity bit_offset + n overflows 64 bits", name, k);
      return fail(c, HMJ_E_ARG, msg);
    }
  }
  return HMJ_OK;
}

// The relation as the kernels take it; *any: at least one column has a validity bitmap.
MixSide side_of(const hmj_mixed_rel* r, ColValid* V, bool* any) {
  MixSide A;
  std::memset(&A, 0, sizeof(A));
  std::memset(V, 0, sizeof(*V));
  A.k = V->k = r->n_cols;
  *any = false;
  for (u32 k = 0; k < r->n_cols; k++) {
    const hmj_mixed_col& col = r->cols[k];
    A.p[k] = col.data;
    A.off[k] = col.type == HMJ_KEY_LARGE_STRING ? (const u64*)col.offsets : nullptr;
    A.w[k] = col.type == HMJ_KEY_LARGE_STRING ? 0u : col.width;
    if (col.validity.bits) {
      V->bits[k] = (const unsigned char*)col.validity.bits;
      V->off[k] = col.validity.bit_offset;
      *any = true;
    }
  }
  A.vals = (const u64*)r->vals;
  return A;
}

// ---- grouping (hmj_group_mixed_device; kernels and the driver, group_rows: hmj_group.h) ------------------------------------
constexpr KeyJoinNames kGroupNames{"mixed-key grouping", "key64", "tuples"};

// group_rows' Check for this key shape: the key kernel's report on the one relation, laid out as MixPolicyT lays out a
// relation's (kErrWords offset-error words, preset as keys_begin presets them; NE: kNullWords behind them).  key_eq / key_cmp
// follow a string column's offsets into its chars, so decreasing offsets must end the call before any of them runs.
template <bool NE>
struct MixGroupCheck {
  static constexpr int kWords = kErrWords + (NE ? kNullWords : 0);
  int begin(hmj_ctx* c, u64* e) const {  // (group_rows cleared the words)
    HIP_TRY(hipMemsetAsync(e, 0xFF, kMaxCols * sizeof(u64), c->stream));
    return HMJ_OK;
  }
  int check(hmj_ctx* c, const u64* e, hmj_group_opts* o) const {
    char msg[192];
    for (int k = 0; k < kMaxCols; k++) {  // the lowest-numbered column first, keys_check's wording
      if (e[k] != kNone) {
        std::snprintf(msg, sizeof(msg), "grouped relation: column %d: offsets decrease at row %llu (offsets[%llu] < offsets[%llu])", k,
                      (unsigned long long)e[k], (unsigned long long)e[k] + 1, (unsigned long long)e[k]);
        return fail(c, HMJ_E_ARG, msg);
      }
      if (e[kMaxCols + k]) {
        std::snprintf(msg, sizeof(msg), "grouped relation: column %d: data is NULL but keys have bytes", k);
        return fail(c, HMJ_E_ARG, msg);
      }
    }
    if (NE) o->n_null = null_rows_of(e + kErrWords);
    return HMJ_OK;
  }
};

}  // namespace

extern "C" {

int hmj_join_mixed_device(hmj_ctx* c, const hmj_mixed_rel* build, const hmj_mixed_rel* probe, uint32_t flags, hmj_mixed_opts* opts,
                          hmj_cols_result* out) {
  if (!c) return HMJ_E_ARG;
  if (!opts || !out) return fail(c, HMJ_E_ARG, "opts / out is NULL");
  if (opts->struct_size < offsetof(hmj_mixed_opts, build_fill) + sizeof(opts->build_fill))
    return fail(c, HMJ_E_ARG, "hmj_mixed_opts.struct_size too small");
  if (opts->side > HMJ_KIND_BUILD_SIDE) return fail(c, HMJ_E_ARG, "unknown join side");
  if (opts->side == HMJ_KIND_PROBE_SIDE ? opts->kind > HMJ_JOIN_PROBE_OUTER : (opts->kind < HMJ_BUILD_SEMI || opts->kind > HMJ_FULL_OUTER))
    return fail(c, HMJ_E_ARG, "unknown join kind");
  if (opts->hash_bits > 63) return fail(c, HMJ_E_ARG, "hash_bits > 63");
  if (flags & HMJ_FIRST_WINS) return fail(c, HMJ_E_ARG, "HMJ_FIRST_WINS is not defined for mixed-key joins");
  RC_TRY(check_mixed_rel(c, build, "build"));
  RC_TRY(check_mixed_rel(c, probe, "probe"));
  if (build->n_cols != probe->n_cols) return fail(c, HMJ_E_ARG, "build and probe relations have different n_cols");
  for (u32 k = 0; k < build->n_cols; k++) {
    const hmj_mixed_col &b = build->cols[k], &p = probe->cols[k];
    if (b.type != p.type || b.width != p.width) {
      char msg[160];
      std::snprintf(msg, sizeof(msg), "column %u has type %u, width %u on the build side and type %u, width %u on the probe side", k, b.type,
                    b.width, p.type, p.width);
      return fail(c, HMJ_E_ARG, msg);
    }
  }
  ColValid VB, VP;
  bool any_b, any_p;
  const MixSide RS = side_of(build, &VB, &any_b), SS = side_of(probe, &VP, &any_p);
  std::memset(out, 0, sizeof(*out));
  HIP_TRY(hipSetDevice(c->device));
  TupleCall call;
  call.hashed = true;
  call.bits = opts->hash_bits;
  call.side = opts->side;
  call.kind = opts->kind;
  call.probe_fill = opts->probe_fill;
  call.build_fill = opts->build_fill;
  const bool inner = opts->side == HMJ_KIND_PROBE_SIDE && opts->kind == HMJ_JOIN_INNER;
  // NULL-equals-NULL matching needs a bitmap to differ from the call without the flag, which is what runs when there is none
  const bool null_equal = (flags & HMJ_NULL_EQUAL) && (any_b || any_p);
  flags &= ~HMJ_NULL_EQUAL;
  if (null_equal) {
    const MixNeSide RN{RS, VB}, SN{SS, VP};  // (a relation without a bitmap: its ColValid holds no pointer)
    if (inner) RC_TRY(tuple_join<MixNePolicy>(c, RN, build->n, SN, probe->n, flags, &call, out, nullptr, nullptr));
    else RC_TRY(tuple_join_kind<MixNePolicy>(c, RN, build->n, SN, probe->n, flags, &call, out, nullptr, nullptr));
  } else if (inner) {
    RC_TRY(tuple_join<MixPolicy>(c, RS, build->n, SS, probe->n, flags, &call, out, any_b ? &VB : nullptr, any_p ? &VP : nullptr));
  } else {
    RC_TRY(tuple_join_kind<MixPolicy>(c, RS, build->n, SS, probe->n, flags, &call, out, any_b ? &VB : nullptr, any_p ? &VP : nullptr));
  }
  // the out fields go to a full-size copy first; the caller gets the prefix its struct_size holds
  hmj_mixed_opts o;
  opts_prefix_in(&o, opts);
  opts_clear_out(&o, opts, offsetof(hmj_mixed_opts, counts));
  o.counts = call.counts;
  o.n_key_pairs = call.n_key_pairs;
  o.n_collisions = call.n_collisions;
  o.n_build_null = call.n_build_null;
  o.n_probe_null = call.n_probe_null;
  fill_kind_ms(c, o, o.ms_key, c->mix_ws.ev, !inner);
  opts_prefix_out(opts, o);
  return HMJ_OK;
}

int hmj_group_mixed_device(hmj_ctx* c, const hmj_mixed_rel* rel, uint32_t flags, hmj_group_opts* opts, hmj_group_result* out) {
  if (!c) return HMJ_E_ARG;
  c->grp_ws.live = false;  // hmj_group_agg_device's binding ends here, whatever becomes of this call
  if (!opts || !out) return fail(c, HMJ_E_ARG, "opts / out is NULL");
  if (opts->struct_size < offsetof(hmj_group_opts, validity) + sizeof(opts->validity))
    return fail(c, HMJ_E_ARG, "hmj_group_opts.struct_size too small");
  if (opts->hash_bits > 63) return fail(c, HMJ_E_ARG, "hash_bits > 63");
  if (flags & HMJ_FIRST_WINS) return fail(c, HMJ_E_ARG, "HMJ_FIRST_WINS is not defined for grouping");
  if (flags & HMJ_CHECKSUM) return fail(c, HMJ_E_ARG, "HMJ_CHECKSUM is not defined for grouping");
  if (flags & HMJ_SUM_PROBE) return fail(c, HMJ_E_ARG, "HMJ_SUM_PROBE is not defined for grouping");
  const uint32_t all = HMJ_GROUP_COUNT | HMJ_GROUP_SUM | HMJ_GROUP_MIN | HMJ_GROUP_MAX | HMJ_GROUP_ROW_MAP;
  if (opts->want & ~all) return fail(c, HMJ_E_ARG, "hmj_group_opts.want has unknown bits");
  if (opts->reserved) return fail(c, HMJ_E_ARG, "hmj_group_opts.reserved must be 0");
  if (opts->validity) return fail(c, HMJ_E_ARG, "hmj_group_opts.validity must be NULL for mixed keys: the bitmaps are in the columns");
  RC_TRY(check_mixed_rel(c, rel, "grouped"));
  ColValid V;
  bool any = false;
  const MixSide A = side_of(rel, &V, &any);
  if (flags & HMJ_ORDERED) flags |= HMJ_MATERIALIZE;  // (HMJ_NULL_EQUAL: implied, ignored)
  const bool mat = flags & HMJ_MATERIALIZE;
  std::memset(out, 0, sizeof(*out));
  HIP_TRY(hipSetDevice(c->device));
  c->prep.valid = false;  // like any other call, this one discards a prepared build side
  // the out fields of opts go to a full-size copy first; the caller gets the prefix its struct_size holds
  hmj_group_opts o;
  opts_prefix_in(&o, opts);
  opts_clear_out(&o, opts, offsetof(hmj_group_opts, n_null));
  o.form = HMJ_COLS_HASHED;  // (force_hashed: ignored)
  const u32 bits = o.hash_bits;
  const u64 n = rel->n;
  out->n_rows = n;
  if (n) {
    const dim3 G((u32)blocks_of(n)), T(MK_THREADS);
    if (any) {
      const MixNeSide N{A, V};
      auto key = [&](hmj_ctx* c, u64* rows, u64* acc) {
        hipLaunchKernelGGL((mix_key_kernel<false, true>), G, T, 0, c->stream, N.s, N.v, n, bits, rows, nullptr, 0ull, nullptr, 0, acc, acc + GA_N);
        HIP_TRY(hipGetLastError());
        return (int)HMJ_OK;
      };
      RC_TRY(group_rows(c, kGroupNames, N, n, true, mat, key, MixGroupCheck<true>{}, &o, out));
    } else {
      auto key = [&](hmj_ctx* c, u64* rows, u64* acc) {
        hipLaunchKernelGGL(mix_key_kernel<false>, G, T, 0, c->stream, A, ColValid{}, n, bits, rows, nullptr, 0ull, nullptr, 0, acc, acc + GA_N);
        HIP_TRY(hipGetLastError());
        return (int)HMJ_OK;
      };
      RC_TRY(group_rows(c, kGroupNames, A, n, true, mat, key, MixGroupCheck<false>{}, &o, out));
    }
    fill_group_ms(c, o);
  }
  opts_prefix_out(opts, o);
  c->grp_ws.live = mat;  // the live grouping of hmj_group_agg_device
  c->grp_ws.live_rows = n;
  c->grp_ws.live_groups = out->n_groups;
  return HMJ_OK;
}

}  // extern "C"
