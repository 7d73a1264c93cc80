// Multi-column fixed-width keys on the device (hmj_join_cols_device; include/hmj.h).  Nothing in the reference
// corresponds: its operator is a template over ONE Key with std::hash<Key> (hashjoin.h:33-56).  The structure is the
// string join's (strjoin.hip) with the byte walks replaced by column loads; what the two share -- every kernel and launch
// sequence named below without a cols_ prefix -- lives in hmj_keyjoin.h and is instantiated here on ColSide.  This file
// holds the key kernels, the packed form's gather and the key policy (key_eq / key_cmp / payload on ColSide); the launch
// sequence of the stages below is hmj_tuplejoin.h's (tuple_join / tuple_join_kind), shared with the mixed-key join
// (mixjoin.hip) and instantiated here on ColPolicy:
//   1. cols_key_kernel    k columns (struct of arrays, one device pointer each) -> {key64, row} rows (16 bytes, what the
//                         u64 join takes).  PACKED (widths sum to <= 8 bytes): key64 is the tuple itself, column 0 in the
//                         most significant position, so equal key64 IS equal tuples and ascending key64 IS tuple order.
//                         HASHED: key64 = a mix64 chain over the columns (hash_bits applied);
//   2. the u64 join       join_device on those rows, HMJ_MATERIALIZE (+ HMJ_ORDERED): (key64, r_row, s_row);
//   3. PACKED             cols_gather_kernel: payloads gathered (or only reduced in the count modes); no verification;
//      HASHED             verify_kernel, one lane per pair: columns compared one by one with early exit; survivors
//                         compacted (stable) with their payloads, or only counted / summed in the count modes;
//   4. collision order    HASHED + ordered only: runs of equal key64 whose build tuples differ are sorted by the tuple
//                         (column by column, unsigned) in one workgroup each (a run beyond kRunCap rows is
//                         HMJ_E_UNSUPPORTED).
// The join kinds (hmj_join_kind_cols_device) are the string kinds' design (join_str_kind, strjoin.hip):
//   semi / anti           the {key64,row} rows joined first-wins, the side asked about as the probe side: one pair per row.
//                         rep_verify_kernel marks the rows whose tuples are equal (PACKED: every pair, no column load) and
//                         lists the others, which are joined with every row of their key64 and verified again;
//   outer kinds           the pair join above; the MARK variants of cols_gather_kernel / verify_kernel mark both rows of
//                         every result pair;
//   sweeps                sweep_count_kernel / sweep_emit_kernel: one lane per row of a relation, the rows its mark
//                         selects emitted stably in row order behind the pairs (one scan over all per-workgroup counts);
//   order                 (key64, index) rows through the stable u64 sort, one gather, and -- HASHED only -- the collision
//                         sort's MIXED variants (a row's tuple is its build row's, or its probe row's where there is none).
// NULL keys (validity bitmaps, calls that pass one only): valid_count_kernel counts the rows whose key columns are all
// valid per workgroup, one scan places them, and cols_key_valid_kernel writes two arrays per relation: the dense rows the
// sweeps walk by row index (a NULL-key row: key64 0, row HMJ_COLS_NO_ROW) and the compacted rows of the valid rows, which are
// all the u64 joins see -- so a NULL-key row is never paired and never marked.  Ordered kinds: the sweeps emit the NULL-key
// rows into a tail behind the rows that are sorted (DESIGN.md "NULL keys (validity bitmaps)").
// NULL-equals-NULL matching (HMJ_NULL_EQUAL with a bitmap): none of that -- cols_key_ne_kernel gives every row a key (a NULL
// slot hashes as 0, the row's NULL-column mask is mixed in last), and the sequence above runs in its hashed form on
// ColNeSide / ColNePolicy, whose key_eq / key_cmp read the bitmaps (DESIGN.md "NULL-equals-NULL matching").
// Grouping (hmj_group_cols_device): one relation's {key64, row} rows from the key kernels above (cols_key_ne_kernel where a
// bitmap is passed: NULLs of a column form one group), hmj_sort_u64_device, then hmj_group.h's kernels on ColSide /
// ColNeSide -- collision sort, group heads, group columns, aggregates (group_rows, hmj_group.h; DESIGN.md "Grouping rows by
// multi-column keys").
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdio>
#include <cstring>

#include "hmj_tuplejoin.h"
#include "hmj_group.h"

namespace {

constexpr int CJ_THREADS = KJ_THREADS;  // the key kernels' workgroup: valid_count_kernel counts the rows of one of cols_key_valid_kernel
constexpr int CJ_WAVES = CJ_THREADS / 64;

// One relation's key columns and payloads, passed to the kernels by value.  Every loop over the columns is fully unrolled
// with a `c < k` guard, so p[c] / w[c] are read from the kernel arguments at constant offsets.
struct ColSide {
  const void* p[kMaxCols];
  u32 w[kMaxCols];
  u32 k;
  const u64* vals;  // NULL: the payload of row i is i
};

__device__ __forceinline__ u64 payload(const ColSide& A, u64 i) { return A.vals ? A.vals[i] : i; }

// The key policy of the shared kernels (hmj_keyjoin.h).  Both sides have the same column count and widths, so where a lane
// chooses its side at run time (the join kinds' mixed rows) the first lane's count and widths are every lane's: the choice
// only selects the column pointers, and col_load's switch stays a scalar branch.
__device__ __forceinline__ bool key_eq(const ColSide& A, u64 a, const ColSide& B, u64 b) {
  bool eq = true;
  const int k = uniform(A.k);
#pragma unroll
  for (int c = 0; c < kMaxCols; c++) {
    const u32 w = uniform(A.w[c]);
    if (c < k && eq) eq = col_load(A.p[c], w, a) == col_load(B.p[c], w, b);
  }
  return eq;
}
// column by column as unsigned integers
__device__ __forceinline__ int key_cmp(const ColSide& A, u64 a, const ColSide& B, u64 b) {
  int r = 0;
  const int k = uniform(A.k);
#pragma unroll
  for (int c = 0; c < kMaxCols; c++) {
    const u32 w = uniform(A.w[c]);
    if (c < k && r == 0) {
      const u64 x = col_load(A.p[c], w, a), y = col_load(B.p[c], w, b);
      if (x != y) r = x < y ? -1 : 1;
    }
  }
  return r;
}

// NULL-equals-NULL matching (HMJ_NULL_EQUAL, calls that pass a bitmap only): the relation with its validity bitmaps.  A
// NULL slot is a value of its own that equals only the NULL slot of the same column and sorts behind every valid value;
// what lies under it is never loaded.  Where a lane chooses its side at run time the bitmap pointers are the lane's own
// (a per-lane branch); count and widths stay the first lane's.
struct ColNeSide {
  ColSide s;
  ColValid v;
};
__device__ __forceinline__ u64 payload(const ColNeSide& A, u64 i) { return payload(A.s, i); }
__device__ __forceinline__ bool key_eq(const ColNeSide& A, u64 a, const ColNeSide& B, u64 b) {
  bool eq = true;
  const int k = uniform(A.s.k);
#pragma unroll
  for (int c = 0; c < kMaxCols; c++) {
    const u32 w = uniform(A.s.w[c]);
    if (c < k && eq) {
      const bool na = slot_null(A.v, c, a), nb = slot_null(B.v, c, b);
      if (na || nb) eq = na && nb;
      else eq = col_load(A.s.p[c], w, a) == col_load(B.s.p[c], w, b);
    }
  }
  return eq;
}
// column by column, NULLS LAST in each: two NULL slots tie
__device__ __forceinline__ int key_cmp(const ColNeSide& A, u64 a, const ColNeSide& B, u64 b) {
  int r = 0;
  const int k = uniform(A.s.k);
#pragma unroll
  for (int c = 0; c < kMaxCols; c++) {
    const u32 w = uniform(A.s.w[c]);
    if (c < k && r == 0) {
      const bool na = slot_null(A.v, c, a), nb = slot_null(B.v, c, b);
      if (na || nb) {
        r = (int)na - (int)nb;
      } else {
        const u64 x = col_load(A.s.p[c], w, a), y = col_load(B.s.p[c], w, b);
        if (x != y) r = x < y ? -1 : 1;
      }
    }
  }
  return r;
}

// Grid-stride, one row per lane and step: per column a wave reads 64 consecutive values (coalesced), and writes 64 rows of
// {key64, row} as one kilobyte.  sum_probe: the payloads' sum goes to acc[KA_SUM_P], one atomic per workgroup.
template <bool HASHED>
__global__ __launch_bounds__(CJ_THREADS) void cols_key_kernel(ColSide A, u64 n, u32 hash_bits, u64* __restrict__ out, int sum_probe,
                                                              u64* __restrict__ acc) {
  __shared__ u64 red[CJ_WAVES];
  u64 sum = 0;
  for (u64 i = (u64)blockIdx.x * CJ_THREADS + threadIdx.x; i < n; i += (u64)gridDim.x * CJ_THREADS) {
    u64 key = HASHED ? (u64)A.k : 0ull;
#pragma unroll
    for (int c = 0; c < kMaxCols; c++) {
      if (c < (int)A.k) {
        const u64 v = col_load(A.p[c], A.w[c], i);
        if (HASHED) key = hmj::mix64(key + v + kGolden);
        else key = A.w[c] == 8 ? v : ((key << (8u * A.w[c])) | v);  // (an 8-byte column is the whole packed key)
      }
    }
    if (HASHED) key = fold_bits(key, hash_bits);
    reinterpret_cast<ulonglong2*>(out)[i] = make_ulonglong2(key, i);
    if (sum_probe) sum += payload(A, i);
  }
  if (sum_probe) {  // (uniform)
    sum = hmj::wave_sum_u64(sum);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
      u64 t = 0;
      for (int k = 0; k < CJ_WAVES; k++) t += red[k];
      if (t) atomicAdd(&acc[KA_SUM_P], t);
    }
  }
}

// ---- NULL keys (validity bitmaps: ColValid / row_valid, hmj_tuplejoin.h) ------------------------------------------------
// Pass 2, cols_key_kernel for a relation with bitmaps: one lane per row, one workgroup per 256 rows (blk_off is indexed by
// workgroup).  dense (NULL: not wanted): row i gets {key64, i}, a NULL-key row {0, HMJ_COLS_NO_ROW} -- what the sweeps walk
// by row index.  comp: the valid rows' {key64, i}, workgroup b's at blk_off[b] in row order (the wave's ballot places a lane
// inside its wave, the per-wave counts in LDS the wave inside its workgroup); cap: rows comp holds.  The values under a
// NULL slot may be loaded; the key made of them is dropped.  sum_probe as cols_key_kernel (every row, NULL-key rows too).
template <bool HASHED>
__global__ __launch_bounds__(CJ_THREADS) void cols_key_valid_kernel(ColSide A, ColValid V, u64 n, u32 hash_bits, u64* __restrict__ dense,
                                                                    u64* __restrict__ comp, u64 cap, const u64* __restrict__ blk_off,
                                                                    int sum_probe, u64* __restrict__ acc) {
  __shared__ u64 red[CJ_WAVES];
  __shared__ u32 wcnt[CJ_WAVES];
  const u64 i = (u64)blockIdx.x * CJ_THREADS + threadIdx.x;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  bool ok = false;
  u64 key = 0, sum = 0;
  if (i < n) {
    ok = row_valid(V, i);
    u64 h = HASHED ? (u64)A.k : 0ull;
#pragma unroll
    for (int c = 0; c < kMaxCols; c++) {
      if (c < (int)A.k) {
        const u64 v = col_load(A.p[c], A.w[c], i);
        if (HASHED) h = hmj::mix64(h + v + kGolden);
        else h = A.w[c] == 8 ? v : ((h << (8u * A.w[c])) | v);
      }
    }
    if (HASHED) h = fold_bits(h, hash_bits);
    key = ok ? h : 0ull;
    if (dense) reinterpret_cast<ulonglong2*>(dense)[i] = make_ulonglong2(key, ok ? i : kNoRow);
    if (sum_probe) sum = payload(A, i);
  }
  const u64 m = __ballot(ok);
  if (lane == 0) wcnt[w] = (u32)__builtin_popcountll(m);
  if (sum_probe) {  // (uniform)
    sum = hmj::wave_sum_u64(sum);
    if (lane == 0) red[w] = sum;
  }
  __syncthreads();
  if (ok) {
    u64 pos = blk_off[blockIdx.x] + hmj::popc_below(m);
    for (int k = 0; k < w; k++) pos += wcnt[k];
    if (pos < cap) reinterpret_cast<ulonglong2*>(comp)[pos] = make_ulonglong2(key, i);
  }
  if (sum_probe && threadIdx.x == 0) {
    u64 t = 0;
    for (int k = 0; k < CJ_WAVES; k++) t += red[k];
    if (t) atomicAdd(&acc[KA_SUM_P], t);
  }
}

// ---- NULL-equals-NULL matching (HMJ_NULL_EQUAL) ----------------------------------------------------------------------------
// cols_key_kernel for a call that matches NULL slots with NULL slots (always HASHED): every row gets a key, so there is
// nothing to count, scan or compact -- one dense {key64, row} row per row, as without bitmaps.  Grid-stride by waves: a
// wave keys the 64 consecutive rows from i0 (a multiple of 64, wave-uniform), and reads a column's 64 validity bits as one
// or two aligned 8-byte words (wave_valid_word).  A NULL slot contributes v_c = 0 and is not loaded; the row's NULL columns
// (m: bit c for column c) are mixed in behind the last column, so a row without NULLs has exactly cols_key_kernel's key64.
// n_null: the relation's kNullWords words for the rows with m != 0 (count_null_rows: one atomic per workgroup).  sum_probe as
// cols_key_kernel.
__global__ __launch_bounds__(CJ_THREADS) void cols_key_ne_kernel(ColSide A, ColValid V, u64 n, u32 hash_bits, u64* __restrict__ out,
                                                                 int sum_probe, u64* __restrict__ acc, u64* __restrict__ n_null) {
  __shared__ u64 red[CJ_WAVES];
  __shared__ u32 nred[CJ_WAVES];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  u64 sum = 0;
  u32 nulls = 0;  // rows of this wave's steps with a NULL slot (the same in every lane)
  for (u64 i0 = uniform64((u64)blockIdx.x * CJ_THREADS + (u64)(w * 64)); i0 < n; i0 += (u64)gridDim.x * CJ_THREADS) {
    const u32 cnt = n - i0 < 64ull ? (u32)(n - i0) : 64u;
    const u64 i = i0 + (u64)lane;
    const bool active = (u32)lane < cnt;
    u64 key = (u64)A.k, m = 0;
#pragma unroll
    for (int c = 0; c < kMaxCols; c++) {
      if (c < (int)A.k) {
        bool null = false;
        if (V.bits[c]) null = !((wave_valid_word(V.bits[c], V.off[c], i0, cnt) >> lane) & 1ull);  // (uniform branch)
        u64 v = 0;
        if (active && !null) v = col_load(A.p[c], A.w[c], i);
        if (null) m |= 1ull << c;
        key = hmj::mix64(key + v + kGolden);
      }
    }
    if (m) key = hmj::mix64(key + m + kGolden);
    key = fold_bits(key, hash_bits);
    if (active) {
      reinterpret_cast<ulonglong2*>(out)[i] = make_ulonglong2(key, i);
      if (sum_probe) sum += payload(A, i);
    }
    nulls += (u32)__builtin_popcountll(__ballot(active && m != 0));
  }
  if (sum_probe) sum = hmj::wave_sum_u64(sum);  // (uniform)
  if (lane == 0) {
    red[w] = sum;
    nred[w] = nulls;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    u64 t = 0, tn = 0;
    for (int k = 0; k < CJ_WAVES; k++) {
      t += red[k];
      tn += nred[k];
    }
    if (sum_probe && t) atomicAdd(&acc[KA_SUM_P], t);
    count_null_rows(n_null, tn);
  }
}

// What the MARK variant of cols_gather_kernel writes besides the payloads (outer join kinds): one mark byte per row of each
// relation (every writer stores 1), and -- materialising -- the pair's key64 / r_row / s_row into the kinds' result columns
// and the rows of each workgroup (blk_cnt), which the one scan over pairs and sweeps takes.
struct PairMark {
  unsigned char *mark_r, *mark_s;
  u64 *o_key, *o_r, *o_s, *blk_cnt;
};

// PACKED: every pair of the u64 join is a result row.  MAT: rval / sval gathered; always: count, sums, checksums into acc.
// MARK: see PairMark; nothing is compared, so every pair marks.
template <bool MAT, bool MARK = false>
__global__ __launch_bounds__(CJ_THREADS) void cols_gather_kernel(const u64* __restrict__ kk, const u64* __restrict__ rr,
                                                                 const u64* __restrict__ sr, u64 np, const u64* __restrict__ rvals,
                                                                 const u64* __restrict__ svals, u64* __restrict__ o_rv,
                                                                 u64* __restrict__ o_sv, u64* __restrict__ acc, int checksum,
                                                                 PairMark M) {
  __shared__ u64 red[8];
  if (threadIdx.x < 8) red[threadIdx.x] = 0;
  const u64 j = (u64)blockIdx.x * CJ_THREADS + threadIdx.x;
  u64 v[6] = {0, 0, 0, 0, 0, 0};
  if (MAT && MARK && threadIdx.x == 0) {
    const u64 left = np - (u64)blockIdx.x * CJ_THREADS;
    M.blk_cnt[blockIdx.x] = left < (u64)CJ_THREADS ? left : (u64)CJ_THREADS;
  }
  if (j < np) {
    const u64 r = rr[j], s = sr[j];
    const u64 rv = rvals ? rvals[r] : r, sv = svals ? svals[s] : s;
    if (MAT) {
      o_rv[j] = rv;
      o_sv[j] = sv;
    }
    if (MARK) {
      M.mark_r[r] = 1;
      M.mark_s[s] = 1;
      if (MAT) {
        M.o_key[j] = kk[j];
        M.o_r[j] = r;
        M.o_s[j] = s;
      }
    }
    v[hmj::ACC_N] = 1;
    v[hmj::ACC_SUM_R] = rv;
    v[hmj::ACC_SUM_S] = sv;
    if (checksum) {
      const u64 t = hmj::tmix(kk[j], rv, sv);
      v[hmj::ACC_XOR] = t;
      v[hmj::ACC_MIX] = t;
    }
  }
  __syncthreads();
  hmj::block_accumulate(red, acc + KA_ACC, v, 1u << hmj::ACC_XOR);
}

// ---- host side -----------------------------------------------------------------------------------------------------------
constexpr KeyJoinNames kNames{"multi-column join", "key64", "tuples"};

int check_cols_rel(hmj_ctx* c, const hmj_cols_rel* r, const char* name) {
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
    const hmj_key_col& col = r->cols[k];
    if (col.width != 1 && col.width != 2 && col.width != 4 && col.width != 8) {
      std::snprintf(msg, sizeof(msg), "%s relation: column %u has width %u (1, 2, 4 or 8)", name, k, col.width);
      return fail(c, HMJ_E_ARG, msg);
    }
    if (col.reserved) {
      std::snprintf(msg, sizeof(msg), "%s relation: column %u: reserved must be 0", name, k);
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
  }
  return HMJ_OK;
}

ColSide side_of(const hmj_cols_rel* r) {
  ColSide A;
  std::memset(&A, 0, sizeof(A));
  A.k = r->n_cols;
  for (u32 k = 0; k < r->n_cols; k++) {
    A.p[k] = r->cols[k].data;
    A.w[k] = r->cols[k].width;
  }
  A.vals = (const u64*)r->vals;
  return A;
}

int launch_key(hmj_ctx* c, const ColSide& A, u64 n, bool hashed, u32 bits, u64* out, bool sum_probe, u64* acc) {
  if (!n) return HMJ_OK;
  const u64 need = blocks_of(n), most = (u64)c->num_cus * 16;
  const dim3 grid((u32)(need < most ? need : most));
  if (hashed)
    hipLaunchKernelGGL(cols_key_kernel<true>, grid, dim3(CJ_THREADS), 0, c->stream, A, n, bits, out, sum_probe ? 1 : 0, acc);
  else
    hipLaunchKernelGGL(cols_key_kernel<false>, grid, dim3(CJ_THREADS), 0, c->stream, A, n, bits, out, sum_probe ? 1 : 0, acc);
  HIP_TRY(hipGetLastError());
  return HMJ_OK;
}

// ---- NULL keys: calls with validity bitmaps ---------------------------------------------------------------------------
// The bitmaps of one relation as the kernels take them.  *any: at least one column has one (else the call is today's).
int valid_of(hmj_ctx* c, const hmj_validity* v, const hmj_cols_rel* r, const char* name, ColValid* V, bool* any) {
  std::memset(V, 0, sizeof(*V));
  V->k = r->n_cols;
  *any = false;
  if (!v) return HMJ_OK;
  for (u32 k = 0; k < r->n_cols; k++) {
    if (!v[k].bits) continue;
    if (v[k].bit_offset > UINT64_MAX - r->n) {
      char msg[128];
      std::snprintf(msg, sizeof(msg), "%s relation: column %u: validity bit_offset + n overflows 64 bits", name, k);
      return fail(c, HMJ_E_ARG, msg);
    }
    V->bits[k] = (const unsigned char*)v[k].bits;
    V->off[k] = v[k].bit_offset;
    *any = true;
  }
  return HMJ_OK;
}

// The multi-column join's side of the driver (hmj_tuplejoin.h): its key kernels and the packed form's gather.
struct ColPolicy {
  using Side = ColSide;
  static constexpr bool kCanPack = true;
  static constexpr int kAccExtra = 0;
  // workload_signature kinds of the {key64,row} joins (u64 joins 0, sorts 1, kinds 3..9, string kinds 10..13, inner string
  // join 15, mixed-key joins 20..24): none of them teaches a join of another entry anything
  static constexpr int kMemoInner = 14;      // the inner join
  static constexpr int kMemoProbeRep = 16;   // first-wins join, probe rows against build representatives (probe SEMI / ANTI)
  static constexpr int kMemoBuildRep = 17;   // ... build rows against probe representatives (BUILD_SEMI / BUILD_ANTI)
  static constexpr int kMemoAmbiguous = 18;  // the ambiguous rows against every row of their key64 on the other side
  static constexpr int kMemoPairs = 19;      // the outer kinds' pair join
  static const KeyJoinNames& names() { return kNames; }
  static KeyJoinWs& ws(hmj_ctx* c) { return c->col_ws; }
  static int keys_begin(hmj_ctx*) { return HMJ_OK; }
  static int keys_check(hmj_ctx*, TupleCall*) { return HMJ_OK; }
  static int key(hmj_ctx* c, const ColSide& A, int, u64 n, const TupleCall& call, u64* out, bool sum_probe, u64* acc) {
    return launch_key(c, A, n, call.hashed, call.bits, out, sum_probe, acc);
  }
  static int key_valid(hmj_ctx* c, const ColSide& A, const ColValid& V, int, u64 n, const TupleCall& call, u64 nblk, u64* dense, u64* comp,
                       u64 cap, const u64* off, bool sum_probe, u64* acc) {
    if (call.hashed)
      hipLaunchKernelGGL(cols_key_valid_kernel<true>, dim3((u32)nblk), dim3(CJ_THREADS), 0, c->stream, A, V, n, call.bits, dense, comp, cap,
                         off, sum_probe ? 1 : 0, acc);
    else
      hipLaunchKernelGGL(cols_key_valid_kernel<false>, dim3((u32)nblk), dim3(CJ_THREADS), 0, c->stream, A, V, n, call.bits, dense, comp, cap,
                         off, sum_probe ? 1 : 0, acc);
    HIP_TRY(hipGetLastError());
    return HMJ_OK;
  }
  // packed: every pair is a result row (o_rv / o_sv: the payload columns, materialising); mark: the outer kinds' PairMark
  static int gather(hmj_ctx* c, bool mat, bool mark, u64 nblk, const u64* kk, const u64* rr, const u64* sr, u64 n_pairs, const ColSide& RS,
                    const ColSide& SS, u64* o_rv, u64* o_sv, u64* acc, bool checksum, unsigned char* mark_r, unsigned char* mark_s, u64* o_key,
                    u64* o_r, u64* o_s, u64* blk) {
    const PairMark M{mark_r, mark_s, o_key, o_r, o_s, blk};
    const dim3 G((u32)nblk), T(CJ_THREADS);
    const int cs = checksum ? 1 : 0;
    if (mat && mark)
      hipLaunchKernelGGL((cols_gather_kernel<true, true>), G, T, 0, c->stream, kk, rr, sr, n_pairs, RS.vals, SS.vals, o_rv, o_sv, acc, cs, M);
    else if (mark)
      hipLaunchKernelGGL((cols_gather_kernel<false, true>), G, T, 0, c->stream, kk, rr, sr, n_pairs, RS.vals, SS.vals, nullptr, nullptr, acc,
                         cs, M);
    else if (mat)
      hipLaunchKernelGGL(cols_gather_kernel<true>, G, T, 0, c->stream, kk, rr, sr, n_pairs, RS.vals, SS.vals, o_rv, o_sv, acc, cs, M);
    else
      hipLaunchKernelGGL(cols_gather_kernel<false>, G, T, 0, c->stream, kk, rr, sr, n_pairs, RS.vals, SS.vals, nullptr, nullptr, acc, cs, M);
    HIP_TRY(hipGetLastError());
    return HMJ_OK;
  }
};

// HMJ_NULL_EQUAL with a bitmap on either side: the hashed form on ColNeSide.  The driver runs its no-bitmap path (every row
// has a key; VB == VP == NULL in tuple_join / tuple_join_kind), so key_valid is never reached.  The {key64,row} joins are
// the hashed column join's, under its memo kinds: what they learn about a relation's key64 distribution holds for both.
struct ColNePolicy {
  using Side = ColNeSide;
  static constexpr bool kCanPack = false;
  static constexpr int kAccExtra = 2 * kNullWords;  // the key kernels' counts of rows with a NULL slot: build, probe
  static constexpr int kMemoInner = ColPolicy::kMemoInner, kMemoProbeRep = ColPolicy::kMemoProbeRep;
  static constexpr int kMemoBuildRep = ColPolicy::kMemoBuildRep, kMemoAmbiguous = ColPolicy::kMemoAmbiguous;
  static constexpr int kMemoPairs = ColPolicy::kMemoPairs;
  static const KeyJoinNames& names() { return kNames; }
  static KeyJoinWs& ws(hmj_ctx* c) { return c->col_ws; }
  static int keys_begin(hmj_ctx*) { return HMJ_OK; }  // (the driver cleared the counts)
  static int keys_check(hmj_ctx* c, TupleCall* call) {
    u64 nn[kAccExtra];
    RC_TRY(read_back(c, tuple_acc_extra<ColNePolicy>(c), nn, sizeof(nn)));
    call->n_build_null = null_rows_of(nn);
    call->n_probe_null = null_rows_of(nn + kNullWords);
    return HMJ_OK;
  }
  static int key(hmj_ctx* c, const ColNeSide& A, int rel, u64 n, const TupleCall& call, u64* out, bool sum_probe, u64* acc) {
    if (!n) return HMJ_OK;
    const u64 need = blocks_of(n), most = (u64)c->num_cus * 16;
    hipLaunchKernelGGL(cols_key_ne_kernel, dim3((u32)(need < most ? need : most)), dim3(CJ_THREADS), 0, c->stream, A.s, A.v, n, call.bits, out,
                       sum_probe ? 1 : 0, acc, tuple_acc_extra<ColNePolicy>(c) + rel * kNullWords);
    HIP_TRY(hipGetLastError());
    return HMJ_OK;
  }
  static int key_valid(hmj_ctx* c, const ColNeSide&, const ColValid&, int, u64, const TupleCall&, u64, u64*, u64*, u64, const u64*, bool, u64*) {
    return fail(c, HMJ_E_HIP, "multi-column join: the NULL-equals-NULL form compacts no rows");
  }
};
// V == NULL: the relation has no bitmap (no NULL slot)
ColNeSide ne_side_of(const hmj_cols_rel* r, const ColValid* V) {
  ColNeSide A;
  std::memset(&A, 0, sizeof(A));
  A.s = side_of(r);
  if (V) A.v = *V;
  A.v.k = r->n_cols;
  return A;
}

bool cols_hashed(const hmj_cols_rel* R, uint32_t force_hashed) {
  u32 total = 0;
  for (u32 k = 0; k < R->n_cols; k++) total += R->cols[k].width;
  return total > 8 || force_hashed;
}

// VB / VP: the relations' validity bitmaps, NULL where a relation has none (both NULL: the call without NULL keys, all
// hmj_join_cols_device makes -- hmj_cols_join_opts carries no bitmaps; the INNER kind of hmj_join_kind_cols_device passes
// its own).  n_null (with bitmaps): the NULL-key rows of the build and the probe side.  null_equal (with a bitmap): NULL
// slots match NULL slots -- the hashed form on ColNeSide, the bitmaps inside the sides.
int join_cols(hmj_ctx* c, const hmj_cols_rel* R, const hmj_cols_rel* S, uint32_t flags, hmj_cols_join_opts* opts, hmj_cols_result* out,
              const ColValid* VB = nullptr, const ColValid* VP = nullptr, u64* n_null = nullptr, bool null_equal = false) {
  TupleCall call;
  call.hashed = null_equal || cols_hashed(R, opts->force_hashed);
  call.bits = call.hashed ? opts->hash_bits : 0;
  if (R->n && S->n) opts->form = call.hashed ? HMJ_COLS_HASHED : HMJ_COLS_PACKED;
  if (null_equal) RC_TRY(tuple_join<ColNePolicy>(c, ne_side_of(R, VB), R->n, ne_side_of(S, VP), S->n, flags, &call, out, nullptr, nullptr));
  else RC_TRY(tuple_join<ColPolicy>(c, side_of(R), R->n, side_of(S), S->n, flags, &call, out, VB, VP));
  if (n_null && (VB || VP)) {
    n_null[0] = call.n_build_null;
    n_null[1] = call.n_probe_null;
  }
  opts->n_key_pairs = call.n_key_pairs;
  opts->n_collisions = call.n_collisions;
  return HMJ_OK;
}

int join_cols_kind(hmj_ctx* c, const hmj_cols_rel* R, const hmj_cols_rel* S, uint32_t flags, hmj_cols_kind_opts* o, hmj_cols_result* out,
                   const ColValid* VB, const ColValid* VP, bool null_equal) {
  TupleCall call;
  call.hashed = null_equal || cols_hashed(R, o->force_hashed);
  call.bits = call.hashed ? o->hash_bits : 0;
  call.side = o->side;
  call.kind = o->kind;
  call.probe_fill = o->probe_fill;
  call.build_fill = o->build_fill;
  o->form = call.hashed ? HMJ_COLS_HASHED : HMJ_COLS_PACKED;
  if (null_equal)
    RC_TRY(tuple_join_kind<ColNePolicy>(c, ne_side_of(R, VB), R->n, ne_side_of(S, VP), S->n, flags, &call, out, nullptr, nullptr));
  else RC_TRY(tuple_join_kind<ColPolicy>(c, side_of(R), R->n, side_of(S), S->n, flags, &call, out, VB, VP));
  o->n_build_null = call.n_build_null;
  o->n_probe_null = call.n_probe_null;
  o->n_key_pairs = call.n_key_pairs;
  o->n_collisions = call.n_collisions;
  o->counts = call.counts;
  return HMJ_OK;
}

// what hmj_join_cols_device and hmj_join_kind_cols_device both reject (after ctx / opts / out and struct_size)
int check_cols_args(hmj_ctx* c, const hmj_cols_rel* build, const hmj_cols_rel* probe, uint32_t flags, uint32_t hash_bits) {
  if (hash_bits > 63) return fail(c, HMJ_E_ARG, "hash_bits > 63");
  if (flags & HMJ_FIRST_WINS) return fail(c, HMJ_E_ARG, "HMJ_FIRST_WINS is not defined for multi-column joins");
  RC_TRY(check_cols_rel(c, build, "build"));
  RC_TRY(check_cols_rel(c, probe, "probe"));
  if (build->n_cols != probe->n_cols) return fail(c, HMJ_E_ARG, "build and probe relations have different n_cols");
  for (u32 k = 0; k < build->n_cols; k++) {
    if (build->cols[k].width != probe->cols[k].width) {
      char msg[128];
      std::snprintf(msg, sizeof(msg), "column %u has width %u on the build side and %u on the probe side", k, build->cols[k].width,
                    probe->cols[k].width);
      return fail(c, HMJ_E_ARG, msg);
    }
  }
  return HMJ_OK;
}

// The validity arrays of a hmj_cols_kind_opts whose struct_size covers them, as the kernels take them; *pb / *pp stay NULL
// for a relation without a bitmap.
int opts_validity(hmj_ctx* c, const hmj_cols_kind_opts* opts, const hmj_cols_rel* build, const hmj_cols_rel* probe, ColValid* VB, ColValid* VP,
                  const ColValid** pb, const ColValid** pp) {
  *pb = *pp = nullptr;
  if (opts->struct_size < offsetof(hmj_cols_kind_opts, probe_validity) + sizeof(opts->probe_validity)) return HMJ_OK;
  bool any_b = false, any_p = false;
  RC_TRY(valid_of(c, opts->build_validity, build, "build", VB, &any_b));
  RC_TRY(valid_of(c, opts->probe_validity, probe, "probe", VP, &any_p));
  if (any_b) *pb = VB;
  if (any_p) *pp = VP;
  return HMJ_OK;
}

// ---- grouping (hmj_group_cols_device; kernels and the driver, group_rows: hmj_group.h) ------------------------------------
constexpr KeyJoinNames kGroupNames{"multi-column grouping", "key64", "tuples"};

}  // namespace

extern "C" {

int hmj_join_cols_device(hmj_ctx* c, const hmj_cols_rel* build, const hmj_cols_rel* probe, uint32_t flags, hmj_cols_join_opts* opts,
                         hmj_cols_result* out) {
  if (!c) return HMJ_E_ARG;
  if (!opts || !out) return fail(c, HMJ_E_ARG, "opts / out is NULL");
  if (opts->struct_size < offsetof(hmj_cols_join_opts, force_hashed) + sizeof(opts->force_hashed))
    return fail(c, HMJ_E_ARG, "hmj_cols_join_opts.struct_size too small");
  RC_TRY(check_cols_args(c, build, probe, flags, opts->hash_bits));
  std::memset(out, 0, sizeof(*out));
  HIP_TRY(hipSetDevice(c->device));
  // the out fields of opts go to a full-size copy first; the caller gets the prefix its struct_size holds
  hmj_cols_join_opts o;
  opts_prefix_in(&o, opts);
  opts_clear_out(&o, opts, offsetof(hmj_cols_join_opts, form));
  const int rc = join_cols(c, build, probe, flags, &o, out);
  if (rc != HMJ_OK) return rc;
  fill_join_ms(c, o, o.ms_key, c->col_ws.ev);
  opts_prefix_out(opts, o);
  return HMJ_OK;
}

int hmj_join_kind_cols_device(hmj_ctx* c, const hmj_cols_rel* build, const hmj_cols_rel* probe, uint32_t flags, hmj_cols_kind_opts* opts,
                              hmj_cols_result* out) {
  if (!c) return HMJ_E_ARG;
  if (!opts || !out) return fail(c, HMJ_E_ARG, "opts / out is NULL");
  if (opts->struct_size < offsetof(hmj_cols_kind_opts, build_fill) + sizeof(opts->build_fill))
    return fail(c, HMJ_E_ARG, "hmj_cols_kind_opts.struct_size too small");
  if (opts->side > HMJ_KIND_BUILD_SIDE) return fail(c, HMJ_E_ARG, "unknown join side");
  if (opts->side == HMJ_KIND_PROBE_SIDE ? opts->kind > HMJ_JOIN_PROBE_OUTER : (opts->kind < HMJ_BUILD_SEMI || opts->kind > HMJ_FULL_OUTER))
    return fail(c, HMJ_E_ARG, "unknown join kind");
  RC_TRY(check_cols_args(c, build, probe, flags, opts->hash_bits));
  ColValid VB, VP;
  const ColValid *vb, *vp;
  RC_TRY(opts_validity(c, opts, build, probe, &VB, &VP, &vb, &vp));
  // NULL-equals-NULL matching needs a bitmap to differ from the call without the flag, which is what runs when there is none
  const bool null_equal = (flags & HMJ_NULL_EQUAL) && (vb || vp);
  flags &= ~HMJ_NULL_EQUAL;
  std::memset(out, 0, sizeof(*out));
  HIP_TRY(hipSetDevice(c->device));
  // the out fields of opts go to a full-size copy first; the caller gets the prefix its struct_size holds
  hmj_cols_kind_opts o;
  opts_prefix_in(&o, opts);
  o.form = 0;
  // (out fields: form, and from `counts` on; the validity arrays behind them are in fields)
  opts_clear_out(&o, opts, offsetof(hmj_cols_kind_opts, counts), offsetof(hmj_cols_kind_opts, build_validity), offsetof(hmj_cols_kind_opts, n_build_null));
  const bool inner = o.side == HMJ_KIND_PROBE_SIDE && o.kind == HMJ_JOIN_INNER;  // exactly the inner multi-column join
  if (inner) {
    hmj_cols_join_opts jo;
    std::memset(&jo, 0, sizeof(jo));
    jo.struct_size = sizeof(jo);
    jo.hash_bits = o.hash_bits;
    jo.force_hashed = o.force_hashed;
    u64 n_null[2] = {0, 0};
    RC_TRY(join_cols(c, build, probe, flags, &jo, out, vb, vp, n_null, null_equal));
    o.n_build_null = n_null[0];
    o.n_probe_null = n_null[1];
    u32 total = 0;  // (the inner entry leaves form 0 when a side is empty; here it is always filled)
    for (u32 k = 0; k < build->n_cols; k++) total += build->cols[k].width;
    o.form = total > 8 || o.force_hashed || null_equal ? HMJ_COLS_HASHED : HMJ_COLS_PACKED;
    o.n_key_pairs = jo.n_key_pairs;
    o.n_collisions = jo.n_collisions;
  } else {
    RC_TRY(join_cols_kind(c, build, probe, flags, &o, out, vb, vp, null_equal));
  }
  fill_kind_ms(c, o, o.ms_key, c->col_ws.ev, !inner);
  opts_prefix_out(opts, o);
  return HMJ_OK;
}

int hmj_group_cols_device(hmj_ctx* c, const hmj_cols_rel* rel, uint32_t flags, hmj_group_opts* opts, hmj_group_result* out) {
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
  RC_TRY(check_cols_rel(c, rel, "grouped"));
  ColValid V;
  bool any = false;
  RC_TRY(valid_of(c, opts->validity, rel, "grouped", &V, &any));
  if (flags & HMJ_ORDERED) flags |= HMJ_MATERIALIZE;  // (HMJ_NULL_EQUAL: implied, ignored)
  const bool mat = flags & HMJ_MATERIALIZE;
  std::memset(out, 0, sizeof(*out));
  HIP_TRY(hipSetDevice(c->device));
  c->prep.valid = false;  // like any other call, this one discards a prepared build side
  // the out fields of opts go to a full-size copy first; the caller gets the prefix its struct_size holds
  hmj_group_opts o;
  opts_prefix_in(&o, opts);
  opts_clear_out(&o, opts, offsetof(hmj_group_opts, n_null));
  const bool hashed = any || cols_hashed(rel, o.force_hashed);
  const u32 bits = hashed ? o.hash_bits : 0;
  o.form = hashed ? HMJ_COLS_HASHED : HMJ_COLS_PACKED;
  const u64 n = rel->n;
  out->n_rows = n;
  if (n) {
    const u64 need = blocks_of(n), most = (u64)c->num_cus * 16;
    if (any) {
      const ColNeSide A = ne_side_of(rel, &V);
      auto key = [&](hmj_ctx* c, u64* rows, u64* acc) {
        hipLaunchKernelGGL(cols_key_ne_kernel, dim3((u32)(need < most ? need : most)), dim3(CJ_THREADS), 0, c->stream, A.s, A.v, n, bits, rows, 0,
                           acc, acc + GA_NULL);
        HIP_TRY(hipGetLastError());
        return (int)HMJ_OK;
      };
      RC_TRY(group_rows(c, kGroupNames, A, n, true, mat, key, GroupNoCheck{}, &o, out));
    } else {
      const ColSide A = side_of(rel);
      auto key = [&](hmj_ctx* c, u64* rows, u64* acc) { return launch_key(c, A, n, hashed, bits, rows, false, acc); };
      RC_TRY(group_rows(c, kGroupNames, A, n, hashed, mat, key, GroupNoCheck{}, &o, out));
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
