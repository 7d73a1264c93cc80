// Multi-column fixed-width keys on the device (hmj_join_cols_device; include/hmj.h).  Nothing in the reference
// corresponds: its operator is a template over ONE Key with std::hash<Key> (hashjoin.h:33-56).  The structure is the
// string join's (strjoin.hip) with the byte walks replaced by column loads:
//   1. cols_key_kernel    k columns (struct of arrays, one device pointer each) -> {key64, row} rows (16 bytes, what the
//                         u64 join takes).  PACKED (widths sum to <= 8 bytes): key64 is the tuple itself, column 0 in the
//                         most significant position, so equal key64 IS equal tuples and ascending key64 IS tuple order.
//                         HASHED: key64 = a mix64 chain over the columns (hash_bits applied);
//   2. the u64 join       join_device on those rows, HMJ_MATERIALIZE (+ HMJ_ORDERED): (key64, r_row, s_row);
//   3. PACKED             cols_gather_kernel: payloads gathered (or only reduced in the count modes); no verification;
//      HASHED             cols_verify_kernel, one lane per pair: columns compared one by one with early exit; survivors
//                         compacted (stable) with their payloads, or only counted / summed in the count modes;
//   4. collision order    HASHED + ordered only: runs of equal key64 whose build tuples differ are sorted by the tuple
//                         (column by column, unsigned) in one workgroup each (a run beyond kRunCap rows is
//                         HMJ_E_UNSUPPORTED).
// The join kinds (hmj_join_kind_cols_device) are the string kinds' design (join_str_kind, strjoin.hip) on these kernels:
//   semi / anti           the {key64,row} rows joined first-wins, the side asked about as the probe side: one pair per row.
//                         cols_rep_verify_kernel marks the rows whose tuples are equal (PACKED: every pair, no column load) and
//                         lists the others, which are joined with every row of their key64 and verified again;
//   outer kinds           the pair join above; the MARK variants of cols_gather_kernel / cols_verify_kernel mark both rows of
//                         every result pair;
//   sweeps                cols_sweep_count_kernel / cols_sweep_emit_kernel: one lane per row of a relation, the rows its mark
//                         selects emitted stably in row order behind the pairs (one scan over all per-workgroup counts);
//   order                 (key64, index) rows through the stable u64 sort, one gather, and -- HASHED only -- the collision
//                         sort's MIXED variants (a row's tuple is its build row's, or its probe row's where there is none).
// NULL keys (validity bitmaps, calls that pass one only): cols_valid_count_kernel counts the rows whose key columns are all
// valid per workgroup, one scan places them, and cols_key_valid_kernel writes two arrays per relation: the dense rows the
// sweeps walk by row index (a NULL-key row: key64 0, row HMJ_COLS_NO_ROW) and the compacted rows of the valid rows, which are
// all the u64 joins see -- so a NULL-key row is never paired and never marked.  Ordered kinds: the sweeps emit the NULL-key
// rows into a tail behind the rows that are sorted (DESIGN.md "NULL keys (validity bitmaps)").
#include <hip/hip_runtime.h>

#include <cstddef>
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

#define RC_TRY(expr)               \
  do {                             \
    const int _rc = (expr);        \
    if (_rc != HMJ_OK) return _rc; \
  } while (0)

constexpr int CJ_THREADS = 256;
constexpr int CJ_WAVES = CJ_THREADS / 64;
constexpr int kMaxCols = HMJ_MAX_KEY_COLS;
constexpr int kRunCap = 1024;         // rows of one mixed run the collision sort holds (one workgroup)
constexpr u64 kListCap = 1ull << 22;  // mismatching adjacent rows the collision search records
constexpr u64 kGolden = 0x9E3779B97F4A7C15ull;
// col_acc slots (u64): [0] mismatch list length, [1] error bits (1 = a mixed run beyond kRunCap, 2 = list overflow),
// [2] sum of the probe payloads (HMJ_SUM_PROBE), [3] join kinds: pairs of a representative join whose tuples differ,
// [4] join kinds: length of the ambiguous list, [8..15] ACC_* sums
enum { CA_LIST_N = 0, CA_ERR, CA_SUM_P, CA_DIFF, CA_AMB_N, CA_ACC = 8, CA_N = 16 };
constexpr u64 kNoRow = HMJ_COLS_NO_ROW;

// One relation's key columns and payloads, passed to the kernels by value.  Every loop over the columns is fully unrolled
// with a `c < k` guard, so p[c] / w[c] are read from the kernel arguments at constant offsets.
struct ColSide {
  const void* p[kMaxCols];
  u32 w[kMaxCols];
  u32 k;
  const u64* vals;  // NULL: the payload of row i is i
};

// column value of row i, zero-extended (w is uniform: a scalar branch)
__device__ __forceinline__ u64 col_load(const void* p, u32 w, u64 i) {
  switch (w) {
    case 1: return (u64) reinterpret_cast<const unsigned char*>(p)[i];
    case 2: return (u64) reinterpret_cast<const unsigned short*>(p)[i];
    case 4: return (u64) reinterpret_cast<const u32*>(p)[i];
    default: return reinterpret_cast<const u64*>(p)[i];
  }
}
__device__ __forceinline__ u64 payload(const ColSide& A, u64 i) { return A.vals ? A.vals[i] : i; }
__device__ __forceinline__ u64 fold_bits(u64 h, u32 bits) { return bits ? h >> (64 - bits) : h; }

__device__ __forceinline__ bool tuple_eq(const ColSide& A, u64 a, const ColSide& B, u64 b) {
  bool eq = true;
#pragma unroll
  for (int c = 0; c < kMaxCols; c++)
    if (c < (int)A.k && eq) eq = col_load(A.p[c], A.w[c], a) == col_load(B.p[c], A.w[c], b);
  return eq;
}
// rows a and b of one relation, column by column as unsigned integers
__device__ __forceinline__ int tuple_cmp(const ColSide& A, u64 a, u64 b) {
  int r = 0;
#pragma unroll
  for (int c = 0; c < kMaxCols; c++) {
    if (c < (int)A.k && r == 0) {
      const u64 x = col_load(A.p[c], A.w[c], a), y = col_load(A.p[c], A.w[c], b);
      if (x != y) r = x < y ? -1 : 1;
    }
  }
  return r;
}

// The join kinds' result rows: a row's tuple is its build row's when r_row is present, else its probe row's (a NULL row
// column: every row is of the other side).  Both sides have the same widths, so only the column pointer is selected.
struct TupRef {
  bool from_r;
  u64 row;
};
__device__ __forceinline__ TupRef tup_of(u64 r, u64 s) { return r != kNoRow ? TupRef{true, r} : TupRef{false, s}; }
__device__ __forceinline__ TupRef row_tup(const u64* rr, const u64* sr, u64 i) {
  return tup_of(rr ? rr[i] : kNoRow, sr ? sr[i] : kNoRow);
}
__device__ __forceinline__ int tup_cmp(const ColSide& R, const ColSide& S, const TupRef& a, const TupRef& b) {
  int r = 0;
  if (a.from_r == b.from_r && a.row == b.row) return 0;
#pragma unroll
  for (int c = 0; c < kMaxCols; c++) {
    if (c < (int)R.k && r == 0) {
      const u64 x = col_load(a.from_r ? R.p[c] : S.p[c], R.w[c], a.row), y = col_load(b.from_r ? R.p[c] : S.p[c], R.w[c], b.row);
      if (x != y) r = x < y ? -1 : 1;
    }
  }
  return r;
}
__device__ __forceinline__ bool same_tup(const ColSide& R, const ColSide& S, const TupRef& a, const TupRef& b) {
  if (a.from_r == b.from_r && a.row == b.row) return true;
  bool eq = true;
#pragma unroll
  for (int c = 0; c < kMaxCols; c++)
    if (c < (int)R.k && eq)
      eq = col_load(a.from_r ? R.p[c] : S.p[c], R.w[c], a.row) == col_load(b.from_r ? R.p[c] : S.p[c], R.w[c], b.row);
  return eq;
}

// Grid-stride, one row per lane and step: per column a wave reads 64 consecutive values (coalesced), and writes 64 rows of
// {key64, row} as one kilobyte.  sum_probe: the payloads' sum goes to acc[CA_SUM_P], one atomic per workgroup.
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
      if (t) atomicAdd(&acc[CA_SUM_P], t);
    }
  }
}

// ---- NULL keys (validity bitmaps) ------------------------------------------------------------------------------------------
// One relation's Arrow validity bitmaps, passed by value like ColSide: bits[c] == NULL: column c holds no NULL.  Row i is
// valid in column c iff bit off[c] + i (least-significant bit first) is set; a row is a NULL-key row when any column's is not.
struct ColValid {
  const unsigned char* bits[kMaxCols];
  u64 off[kMaxCols];
  u32 k;
};
__device__ __forceinline__ bool row_valid(const ColValid& V, u64 i) {
  bool ok = true;
#pragma unroll
  for (int c = 0; c < kMaxCols; c++) {
    if (c < (int)V.k && V.bits[c]) {  // (uniform)
      const u64 b = V.off[c] + i;
      ok = ok && ((V.bits[c][b >> 3] >> (b & 7)) & 1u);
    }
  }
  return ok;
}

// Pass 1 over the bitmaps alone: one lane per row (eight lanes share a byte, a wave reads 8-9 consecutive bytes per
// column); the valid rows of workgroup b go to blk_cnt[b].
__global__ __launch_bounds__(CJ_THREADS) void cols_valid_count_kernel(ColValid V, u64 n, u64* __restrict__ blk_cnt) {
  __shared__ u32 wcnt[CJ_WAVES];
  const u64 i = (u64)blockIdx.x * CJ_THREADS + threadIdx.x;
  const bool ok = i < n && row_valid(V, i);
  const u64 m = __ballot(ok);
  if ((threadIdx.x & 63) == 0) wcnt[threadIdx.x >> 6] = (u32)__builtin_popcountll(m);
  __syncthreads();
  if (threadIdx.x == 0) {
    u64 t = 0;
    for (int k = 0; k < CJ_WAVES; k++) t += wcnt[k];
    blk_cnt[blockIdx.x] = t;
  }
}

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
    if (t) atomicAdd(&acc[CA_SUM_P], t);
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
  hmj::block_accumulate(red, acc + CA_ACC, v, 1u << hmj::ACC_XOR);
}

// HASHED, pass 1 of the verification.  MAT: one ballot word per wave (flags) and the survivors per workgroup (blk_cnt).
// Count modes (!MAT): counts, sums and checksums of the survivors straight into acc.  MARK (outer join kinds): the
// survivors' build and probe rows are marked (one byte per row; every writer stores 1).
template <bool MAT, bool MARK = false>
__global__ __launch_bounds__(CJ_THREADS) void cols_verify_kernel(const u64* __restrict__ kk, const u64* __restrict__ rr,
                                                                 const u64* __restrict__ sr, u64 np, ColSide R, ColSide S,
                                                                 u64* __restrict__ flags, u64* __restrict__ blk_cnt,
                                                                 u64* __restrict__ acc, int checksum,
                                                                 unsigned char* __restrict__ mark_r, unsigned char* __restrict__ mark_s) {
  __shared__ u64 red[8];
  if (threadIdx.x < 8) red[threadIdx.x] = 0;
  __syncthreads();  // (wave 0 zeroes red[]; every wave's lane 0 adds to red[0] below)
  const u64 j = (u64)blockIdx.x * CJ_THREADS + threadIdx.x;
  bool keep = false;
  u64 r = 0, s = 0;
  if (j < np) {
    r = rr[j];
    s = sr[j];
    keep = tuple_eq(R, r, S, s);
    if (MARK && keep) {
      mark_r[r] = 1;
      mark_s[s] = 1;
    }
  }
  if (MAT) {
    const u64 m = __ballot(keep);
    if ((threadIdx.x & 63) == 0) {
      flags[j >> 6] = m;
      if (m) atomicAdd(&red[0], (u64)__builtin_popcountll(m));
    }
    __syncthreads();
    if (threadIdx.x == 0) blk_cnt[blockIdx.x] = red[0];
  } else {
    u64 v[6] = {0, 0, 0, 0, 0, 0};
    if (keep) {
      const u64 rv = payload(R, r), sv = payload(S, s);
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
    hmj::block_accumulate(red, acc + CA_ACC, v, 1u << hmj::ACC_XOR);
  }
}

// Pass 2: the survivors of workgroup b go, in pair order, to rows [blk_off[b], ..) of the five result columns.
__global__ __launch_bounds__(CJ_THREADS) void cols_compact_kernel(const u64* __restrict__ kk, const u64* __restrict__ rr,
                                                                  const u64* __restrict__ sr, u64 np, ColSide R, ColSide S,
                                                                  const u64* __restrict__ flags, const u64* __restrict__ blk_off,
                                                                  u64* __restrict__ o_key, u64* __restrict__ o_r, u64* __restrict__ o_s,
                                                                  u64* __restrict__ o_rv, u64* __restrict__ o_sv, u64* __restrict__ acc,
                                                                  int checksum) {
  __shared__ u64 red[8];
  if (threadIdx.x < 8) red[threadIdx.x] = 0;
  const u64 j = (u64)blockIdx.x * CJ_THREADS + threadIdx.x;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  u64 v[6] = {0, 0, 0, 0, 0, 0};
  if (j < np) {
    const u64 m = flags[j >> 6];
    if ((m >> lane) & 1ull) {
      u64 pos = blk_off[blockIdx.x] + hmj::popc_below(m);
      const u64 f0 = ((u64)blockIdx.x * CJ_THREADS) >> 6;
      for (int k = 0; k < w; k++) pos += (u64)__builtin_popcountll(flags[f0 + (u64)k]);
      const u64 h = kk[j], r = rr[j], s = sr[j];
      const u64 rv = payload(R, r), sv = payload(S, s);
      o_key[pos] = h;
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
  hmj::block_accumulate(red, acc + CA_ACC, v, 1u << hmj::ACC_XOR);
}

// Collision search (ordered): row i whose key64 equals row i-1's but whose build tuple differs is recorded.  MIXED (join
// kinds): the rows' tuples are row_tup's (sr, S: the probe side).
template <bool MIXED = false>
__global__ __launch_bounds__(CJ_THREADS) void cols_mismatch_kernel(const u64* __restrict__ kk, const u64* __restrict__ rr, u64 n,
                                                                   ColSide R, u64* __restrict__ list, u64* __restrict__ acc,
                                                                   const u64* __restrict__ sr, ColSide S) {
  const u64 i = (u64)blockIdx.x * CJ_THREADS + threadIdx.x + 1;
  if (i >= n) return;
  if (kk[i] != kk[i - 1]) return;
  if constexpr (MIXED) {
    if (same_tup(R, S, row_tup(rr, sr, i - 1), row_tup(rr, sr, i))) return;
  } else {
    const u64 a = rr[i - 1], b = rr[i];
    if (a == b || tuple_eq(R, a, R, b)) return;
  }
  const u64 k = atomicAdd(&acc[CA_LIST_N], 1ull);
  if (k < kListCap) list[k] = i;
  else atomicOr(&acc[CA_ERR], 2ull);
}

// One lane per recorded row i: its run [s, e) of equal key64 (binary searches on the ascending key64 column).  The lane
// whose i is the FIRST mismatch of its run leads it (runs[2k], runs[2k + 1] = s, e); the others write an empty run.  A
// separate launch from the sort, so that no leader test reads rows another workgroup is moving.  MIXED as
// cols_mismatch_kernel.
template <bool MIXED = false>
__global__ __launch_bounds__(CJ_THREADS) void cols_run_leader_kernel(const u64* __restrict__ kk, const u64* __restrict__ rr, u64 n,
                                                                     ColSide R, const u64* __restrict__ list, u64* __restrict__ runs,
                                                                     u64* __restrict__ acc, const u64* __restrict__ sr, ColSide S) {
  const u64 cnt = acc[CA_LIST_N] < kListCap ? acc[CA_LIST_N] : kListCap;
  for (u64 k = (u64)blockIdx.x * CJ_THREADS + threadIdx.x; k < cnt; k += (u64)gridDim.x * CJ_THREADS) {
    const u64 i = list[k], h = kk[i];
    u64 lo = 0, hi = i;  // first row with key64 h
    while (lo < hi) {
      const u64 mid = (lo + hi) >> 1;
      if (kk[mid] < h) lo = mid + 1;
      else hi = mid;
    }
    const u64 s = lo;
    lo = i + 1;
    hi = n;  // first row past the run
    while (lo < hi) {
      const u64 mid = (lo + hi) >> 1;
      if (kk[mid] <= h) lo = mid + 1;
      else hi = mid;
    }
    const u64 e = lo;
    runs[2 * k] = 0;
    runs[2 * k + 1] = 0;
    if (e - s > (u64)kRunCap) {
      atomicOr(&acc[CA_ERR], 1ull);
      continue;
    }
    bool first = true;
    for (u64 t = s + 1; t < i && first; t++) {
      if constexpr (MIXED) {
        if (!same_tup(R, S, row_tup(rr, sr, t - 1), row_tup(rr, sr, t))) first = false;
      } else {
        const u64 a = rr[t - 1], b = rr[t];
        if (a != b && !tuple_eq(R, a, R, b)) first = false;
      }
    }
    if (first) {
      runs[2 * k] = s;
      runs[2 * k + 1] = e;
    }
  }
}

// One workgroup per led run: rows sorted stably by build tuple (rank = rows with a smaller tuple + rows before it with
// the same tuple), written back in place.  All rows of a run share key64, so only r_row, s_row, rval, sval move.
// MIXED: by row_tup (S: the probe side); a NULL column is absent (read as HMJ_COLS_NO_ROW / 0, not written).
template <bool MIXED = false>
__global__ __launch_bounds__(CJ_THREADS) void cols_run_sort_kernel(const u64* __restrict__ runs, ColSide R, u64* __restrict__ o_r,
                                                                   u64* __restrict__ o_s, u64* __restrict__ o_rv,
                                                                   u64* __restrict__ o_sv, const u64* __restrict__ acc, ColSide S) {
  __shared__ u64 col[4][kRunCap];
  __shared__ u32 rank[kRunCap];
  const u64 cnt = acc[CA_LIST_N] < kListCap ? acc[CA_LIST_N] : kListCap;
  for (u64 k = blockIdx.x; k < cnt; k += gridDim.x) {
    const u64 s = runs[2 * k], e = runs[2 * k + 1];
    if (e <= s) continue;  // (uniform: not a leader)
    const u32 L = (u32)(e - s);
    for (u32 t = threadIdx.x; t < L; t += CJ_THREADS) {
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
    for (u32 t = threadIdx.x; t < L; t += CJ_THREADS) {
      u32 rk = 0;
      if constexpr (MIXED) {
        const TupRef me = tup_of(col[0][t], col[1][t]);
        for (u32 o = 0; o < L; o++) {
          const int cm = tup_cmp(R, S, tup_of(col[0][o], col[1][o]), me);
          rk += (cm < 0 || (cm == 0 && o < t)) ? 1u : 0u;
        }
      } else {
        const u64 me = col[0][t];
        for (u32 o = 0; o < L; o++) {
          const u64 other = col[0][o];
          const int cm = other == me ? 0 : tuple_cmp(R, other, me);
          rk += (cm < 0 || (cm == 0 && o < t)) ? 1u : 0u;
        }
      }
      rank[t] = rk;
    }
    __syncthreads();
    for (u32 t = threadIdx.x; t < L; t += CJ_THREADS) {
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
// One lane per pair of a first-wins {key64,row} join: row krow[j] of the side asked about (K) against row orow[j] of the
// other side (O), the one representative of its key64 there.  PACKED: equal key64 is equal tuples, so the pair marks its K
// row without loading a column.  HASHED: equal tuples mark the K row (every writer stores 1); different tuples count in
// acc[CA_DIFF] and, when amb != NULL, the K row goes on the ambiguous list as a {key64, row} row (one counter add per wave)
// -- another O row of the same key64 may still hold its tuple.
template <bool HASHED>
__global__ __launch_bounds__(CJ_THREADS) void cols_rep_verify_kernel(const u64* __restrict__ kk, const u64* __restrict__ orow,
                                                                     const u64* __restrict__ krow, u64 np, ColSide O, ColSide K,
                                                                     unsigned char* __restrict__ mark, u64* __restrict__ amb,
                                                                     u64* __restrict__ acc) {
  const u64 j = (u64)blockIdx.x * CJ_THREADS + threadIdx.x;
  bool diff = false;
  u64 k = 0;
  if (j < np) {
    k = krow[j];
    if (!HASHED || tuple_eq(O, orow[j], K, k)) mark[k] = 1;
    else diff = true;
  }
  if (!HASHED) return;
  const u64 m = __ballot(diff);
  if (!m) return;  // (wave-uniform)
  u64 base = 0;
  if ((threadIdx.x & 63) == 0) {
    atomicAdd(&acc[CA_DIFF], (u64)__builtin_popcountll(m));
    if (amb) base = atomicAdd(&acc[CA_AMB_N], (u64)__builtin_popcountll(m));
  }
  base = __shfl(base, 0, 64);
  if (amb && diff) reinterpret_cast<ulonglong2*>(amb)[base + hmj::popc_below(m)] = make_ulonglong2(kk[j], k);
}

// A relation's rows as the kinds emit them: row i ({key64, i} in rows) is selected when (mark[i] != 0) == want.  probe: the
// row goes out as (key64, NO_ROW, i, fill, payload), else as (key64, i, NO_ROW, payload, fill); NULL columns are not
// written.  vals == NULL: the payload of row i is i.  nulls (ordered results of a relation with validity bitmaps, whose
// NULL-key rows carry HMJ_COLS_NO_ROW in rows): 0 = every selected row, 1 = only those with a key, 2 = only the NULL-key rows.
struct ColSweep {
  const u64* rows;
  const unsigned char* mark;
  const u64* vals;
  u64 n, fill;
  u32 want, probe, nulls;
};
__device__ __forceinline__ bool sweep_sel(const ColSweep& W, u64 i) {
  if (i >= W.n || (W.mark[i] != 0) != (W.want != 0)) return false;
  if (W.nulls == 0) return true;  // (uniform)
  return (W.rows[2 * i + 1] == kNoRow) == (W.nulls == 2);
}
__device__ __forceinline__ void sweep_vals(const ColSweep& W, u64 i, u64& rv, u64& sv) {
  const u64 v = W.vals ? W.vals[i] : i;
  rv = W.probe ? W.fill : v;
  sv = W.probe ? v : W.fill;
}

// Sweep pass 1.  MAT: selected rows per workgroup (blk_cnt).  Count modes: count, sums and checksums into acc.
template <bool MAT>
__global__ __launch_bounds__(CJ_THREADS) void cols_sweep_count_kernel(ColSweep W, u64* __restrict__ blk_cnt, u64* __restrict__ acc,
                                                                      int checksum) {
  __shared__ u64 red[8];
  if (threadIdx.x < 8) red[threadIdx.x] = 0;
  __syncthreads();
  const u64 i = (u64)blockIdx.x * CJ_THREADS + threadIdx.x;
  const bool sel = sweep_sel(W, i);
  if (MAT) {
    const u64 m = __ballot(sel);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(&red[0], (u64)__builtin_popcountll(m));
    __syncthreads();
    if (threadIdx.x == 0) blk_cnt[blockIdx.x] = red[0];
  } else {
    u64 v[6] = {0, 0, 0, 0, 0, 0};
    if (sel) {
      u64 rv, sv;
      sweep_vals(W, i, rv, sv);
      v[hmj::ACC_N] = 1;
      v[hmj::ACC_SUM_R] = rv;
      v[hmj::ACC_SUM_S] = sv;
      if (checksum) {
        const u64 t = hmj::tmix(W.rows[2 * i], rv, sv);
        v[hmj::ACC_XOR] = t;
        v[hmj::ACC_MIX] = t;
      }
    }
    hmj::block_accumulate(red, acc + CA_ACC, v, 1u << hmj::ACC_XOR);
  }
}

// Sweep pass 2: the selected rows of workgroup b go, in row order, to rows [blk_off[b], ..) of the result columns (the
// wave's ballot places a lane inside its wave, the per-wave counts in LDS place the wave inside the workgroup); count, sums
// and checksums into acc.
__global__ __launch_bounds__(CJ_THREADS) void cols_sweep_emit_kernel(ColSweep W, const u64* __restrict__ blk_off, u64* __restrict__ o_key,
                                                                     u64* __restrict__ o_r, u64* __restrict__ o_s, u64* __restrict__ o_rv,
                                                                     u64* __restrict__ o_sv, u64* __restrict__ acc, int checksum) {
  __shared__ u64 red[8];
  __shared__ u32 wcnt[CJ_WAVES];
  if (threadIdx.x < 8) red[threadIdx.x] = 0;
  const u64 i = (u64)blockIdx.x * CJ_THREADS + threadIdx.x;
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
    o_key[pos] = h;
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
  hmj::block_accumulate(red, acc + CA_ACC, v, 1u << hmj::ACC_XOR);
}

// Ordered kinds: (key64, index) rows for the stable u64 sort, then the result columns gathered in the sorted order.
__global__ __launch_bounds__(CJ_THREADS) void cols_sort_rows_kernel(const u64* __restrict__ kk, u64 n, u64* __restrict__ rows) {
  const u64 i = (u64)blockIdx.x * CJ_THREADS + threadIdx.x;
  if (i < n) reinterpret_cast<ulonglong2*>(rows)[i] = make_ulonglong2(kk[i], i);
}
__global__ __launch_bounds__(CJ_THREADS) void cols_order_gather_kernel(const u64* __restrict__ sorted, u64 n, const u64* __restrict__ i_r,
                                                                       const u64* __restrict__ i_s, const u64* __restrict__ i_rv,
                                                                       const u64* __restrict__ i_sv, u64* __restrict__ o_key,
                                                                       u64* __restrict__ o_r, u64* __restrict__ o_s,
                                                                       u64* __restrict__ o_rv, u64* __restrict__ o_sv) {
  const u64 j = (u64)blockIdx.x * CJ_THREADS + threadIdx.x;
  if (j >= n) return;
  const ulonglong2 e = reinterpret_cast<const ulonglong2*>(sorted)[j];
  const u64 p = e.y;
  o_key[j] = e.x;
  if (o_r) o_r[j] = i_r[p];
  if (o_s) o_s[j] = i_s[p];
  if (o_rv) o_rv[j] = i_rv[p];
  if (o_sv) o_sv[j] = i_sv[p];
}

// ---- host side -----------------------------------------------------------------------------------------------------------
constexpr int kColsJoinMemoKind = 14;  // workload_signature kind of the inner {key64,row} join (u64 joins 0, sorts 1, kinds
                                       // 3..9, string kinds 10..13, inner string join 15, multi-column kinds 16..19)

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

u64 blocks_of(u64 n) { return (n + CJ_THREADS - 1) / CJ_THREADS; }

int launch_key(hmj_ctx* c, const ColSide& A, u64 n, bool hashed, u32 bits, u64* out, bool sum_probe, u64* acc) {
  if (!n) return HMJ_OK;
  const u64 need = (n + CJ_THREADS - 1) / CJ_THREADS, most = (u64)c->num_cus * 16;
  const dim3 grid((u32)(need < most ? need : most));
  if (hashed)
    hipLaunchKernelGGL(cols_key_kernel<true>, grid, dim3(CJ_THREADS), 0, c->stream, A, n, bits, out, sum_probe ? 1 : 0, acc);
  else
    hipLaunchKernelGGL(cols_key_kernel<false>, grid, dim3(CJ_THREADS), 0, c->stream, A, n, bits, out, sum_probe ? 1 : 0, acc);
  HIP_TRY(hipGetLastError());
  return HMJ_OK;
}

int read_back(hmj_ctx* c, const void* dev, void* host, size_t bytes) {
  HIP_TRY(hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
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

// The {key64,row} rows of one relation in a call with bitmaps.  dense: the relation's row-indexed rows (NULL: not wanted);
// *rows / *n_valid: what the u64 joins take.  A relation with a bitmap: its valid rows counted per workgroup (vblk: nblk
// counts, then nblk + 1 offsets), the total read back, the valid rows compacted into cmp.  A relation without one goes
// through cols_key_kernel as always, and its dense rows are its join rows.
int launch_key_valid(hmj_ctx* c, const ColSide& A, const ColValid& V, bool has, u64 n, bool hashed, u32 bits, u64* dense, u64* plain,
                     DevBuf& cmp, u64* vblk, bool sum_probe, u64* acc, const void** rows, u64* n_valid) {
  *rows = plain;
  *n_valid = n;
  if (!has || !n) return launch_key(c, A, n, hashed, bits, plain, sum_probe, acc);
  const u64 nblk = blocks_of(n);
  if (nblk > 0xFFFFFFFFull) return fail(c, HMJ_E_ARG, "multi-column join: too many rows");
  u64 *cnt = vblk, *off = vblk + nblk;
  hipLaunchKernelGGL(cols_valid_count_kernel, dim3((u32)nblk), dim3(CJ_THREADS), 0, c->stream, V, n, cnt);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hmj::launch_scan_u64(cnt, off, (u32)nblk, c->stream));
  u64 nv = 0;
  RC_TRY(read_back(c, off + nblk, &nv, sizeof(u64)));
  if (nv > n) return fail(c, HMJ_E_HIP, "multi-column join: more valid rows counted than the relation holds");
  RC_TRY(ensure_dev(c, cmp, 16 * (nv ? nv : 1)));
  if (hashed)
    hipLaunchKernelGGL(cols_key_valid_kernel<true>, dim3((u32)nblk), dim3(CJ_THREADS), 0, c->stream, A, V, n, bits, dense, (u64*)cmp.p, nv,
                       (const u64*)off, sum_probe ? 1 : 0, acc);
  else
    hipLaunchKernelGGL(cols_key_valid_kernel<false>, dim3((u32)nblk), dim3(CJ_THREADS), 0, c->stream, A, V, n, bits, dense, (u64*)cmp.p, nv,
                       (const u64*)off, sum_probe ? 1 : 0, acc);
  HIP_TRY(hipGetLastError());
  *rows = cmp.p;
  *n_valid = nv;
  return HMJ_OK;
}

// Both relations' {key64,row} rows in a call with bitmaps (the block counts of both sides share col_vblk).
int launch_keys_valid(hmj_ctx* c, const ColSide& RS, const ColSide& SS, const ColValid* VB, const ColValid* VP, u64 nb, u64 np,
                      bool hashed, u32 bits, bool dense, bool sum_probe, u64* acc, const void** rows_r, u64* nvb, const void** rows_s,
                      u64* nvp) {
  const u64 kb = VB ? blocks_of(nb) : 0, kp = VP ? blocks_of(np) : 0;
  RC_TRY(ensure_dev(c, c->col_vblk, (2 * (kb + kp) + 2) * sizeof(u64)));
  u64* vblk = (u64*)c->col_vblk.p;
  const ColValid none{};
  u64 *plain_r = (u64*)c->col_rows_r.p, *plain_s = (u64*)c->col_rows_s.p;
  RC_TRY(launch_key_valid(c, RS, VB ? *VB : none, VB != nullptr, nb, hashed, bits, dense ? plain_r : nullptr, plain_r, c->col_cmp_r, vblk,
                          false, acc, rows_r, nvb));
  RC_TRY(launch_key_valid(c, SS, VP ? *VP : none, VP != nullptr, np, hashed, bits, dense ? plain_s : nullptr, plain_s, c->col_cmp_s,
                          vblk + 2 * kb + 1, sum_probe, acc, rows_s, nvp));
  return HMJ_OK;
}

int record(hmj_ctx* c, int k) {
  if (!c->profiling) return HMJ_OK;
  if (!c->col_ev[k]) HIP_TRY(hipEventCreate(&c->col_ev[k]));
  HIP_TRY(hipEventRecord(c->col_ev[k], c->stream));
  return HMJ_OK;
}
float elapsed(hmj_ctx* c, int a, int b) {
  float ms = 0.f;
  if (c->col_ev[a] && c->col_ev[b] && hipEventElapsedTime(&ms, c->col_ev[a], c->col_ev[b]) != hipSuccess) {
    (void)hipGetLastError();
    ms = 0.f;
  }
  return ms;
}

// VB / VP: the relations' validity bitmaps, NULL where a relation has none (both NULL: the call without NULL keys, all
// hmj_join_cols_device makes -- hmj_cols_join_opts carries no bitmaps; the INNER kind of hmj_join_kind_cols_device passes
// its own).  n_null (with bitmaps): the NULL-key rows of the build and the probe side.
int join_cols(hmj_ctx* c, const hmj_cols_rel* R, const hmj_cols_rel* S, uint32_t flags, hmj_cols_join_opts* opts, hmj_cols_result* out,
              const ColValid* VB = nullptr, const ColValid* VP = nullptr, u64* n_null = nullptr) {
  const u64 nb = R->n, np = S->n;
  u32 total = 0;
  for (u32 k = 0; k < R->n_cols; k++) total += R->cols[k].width;
  const bool hashed = total > 8 || opts->force_hashed;
  const u32 bits = hashed ? opts->hash_bits : 0;
  if (flags & HMJ_ORDERED) flags |= HMJ_MATERIALIZE;
  const bool mat = flags & HMJ_MATERIALIZE, ordered = flags & HMJ_ORDERED, checksum = flags & HMJ_CHECKSUM;
  c->prep.valid = false;  // like any other call, a multi-column join discards a prepared build side
  RC_TRY(ensure_dev(c, c->col_acc, CA_N * sizeof(u64)));
  RC_TRY(ensure_dev(c, c->col_rows_r, 16 * (nb ? nb : 1)));
  RC_TRY(ensure_dev(c, c->col_rows_s, 16 * (np ? np : 1)));
  u64* acc = (u64*)c->col_acc.p;
  u64 h[CA_N];
  const ColSide RS = side_of(R), SS = side_of(S);
  // 1. {key64, row} rows of both relations (+ the probe payloads' sum)
  RC_TRY(record(c, 0));
  HIP_TRY(hipMemsetAsync(acc, 0, CA_N * sizeof(u64), c->stream));
  const void *rows_r = c->col_rows_r.p, *rows_s = c->col_rows_s.p;  // the rows the u64 join takes
  u64 nvb = nb, nvp = np;                                           // ... and how many: the rows that have a key
  if (!VB && !VP) {
    RC_TRY(launch_key(c, RS, nb, hashed, bits, (u64*)c->col_rows_r.p, false, acc));
    RC_TRY(launch_key(c, SS, np, hashed, bits, (u64*)c->col_rows_s.p, flags & HMJ_SUM_PROBE, acc));
  } else {  // NULL keys: only the rows that have a key are joined (the inner join walks no relation by row: no dense rows)
    RC_TRY(launch_keys_valid(c, RS, SS, VB, VP, nb, np, hashed, bits, false, flags & HMJ_SUM_PROBE, acc, &rows_r, &nvb, &rows_s, &nvp));
    if (n_null) {
      n_null[0] = nb - nvb;
      n_null[1] = np - nvp;
    }
    if (nb && np) opts->form = hashed ? HMJ_COLS_HASHED : HMJ_COLS_PACKED;
  }
  RC_TRY(record(c, 1));
  if (nvb == 0 || nvp == 0) {  // (nothing to join: no plan either)
    std::memset(&c->plan, 0, sizeof(c->plan));
    c->plan.struct_size = sizeof(c->plan);
    std::memset(&c->timing, 0, sizeof(c->timing));
    for (int k = 2; k < 5; k++) RC_TRY(record(c, k));
    if (flags & HMJ_SUM_PROBE) {
      RC_TRY(read_back(c, acc, h, sizeof(h)));
      out->sum_probe_all = h[CA_SUM_P];
    }
    return HMJ_OK;
  }
  opts->form = hashed ? HMJ_COLS_HASHED : HMJ_COLS_PACKED;
  // 2. the u64 join of the {key64, row} rows: pairs of equal key64 as (key64, r_row, s_row), ordered by them if asked
  hmj_result inner;
  spans_reset(c);
  const int st = span_begin(c, K_TOTAL, -1);
  c->memo_kind = kColsJoinMemoKind;
  const int rc = join_device(c, rows_r, nvb, rows_s, nvp, HMJ_MATERIALIZE | (flags & HMJ_ORDERED), &inner, false);
  c->memo_kind = 0;
  span_end(c, st);
  if (c->profiling) {
    (void)hipStreamSynchronize(c->stream);
    spans_collect(c);
  }
  if (rc != HMJ_OK) return rc;
  RC_TRY(record(c, 2));
  const u64 n_pairs = inner.n_matches;
  opts->n_key_pairs = n_pairs;
  const u64 *ik = (const u64*)inner.key, *ir = (const u64*)inner.rval, *is = (const u64*)inner.sval;
  const u64 nblk = (n_pairs + CJ_THREADS - 1) / CJ_THREADS;
  if (nblk > 0xFFFFFFFFull) return fail(c, HMJ_E_UNSUPPORTED, "multi-column join: more than 2^40 pairs of equal key64");
  u64 n_out = 0;
  if (!hashed) {
    // 3a. packed: every pair is a result row; payloads gathered, or only reduced
    if (n_pairs && mat) {
      RC_TRY(ensure_dev(c, c->col_rval, n_pairs * sizeof(u64)));
      RC_TRY(ensure_dev(c, c->col_sval, n_pairs * sizeof(u64)));
      hipLaunchKernelGGL(cols_gather_kernel<true>, dim3((u32)nblk), dim3(CJ_THREADS), 0, c->stream, ik, ir, is, n_pairs, RS.vals,
                         SS.vals, (u64*)c->col_rval.p, (u64*)c->col_sval.p, acc, checksum ? 1 : 0, PairMark{});
      HIP_TRY(hipGetLastError());
    } else if (n_pairs) {
      hipLaunchKernelGGL(cols_gather_kernel<false>, dim3((u32)nblk), dim3(CJ_THREADS), 0, c->stream, ik, ir, is, n_pairs, RS.vals,
                         SS.vals, nullptr, nullptr, acc, checksum ? 1 : 0, PairMark{});
      HIP_TRY(hipGetLastError());
    }
    n_out = n_pairs;
    RC_TRY(record(c, 3));
  } else {
    // 3b. hashed: tuple verification, payload gather, stable compaction (or the count modes' reduction)
    if (n_pairs && mat) {
      RC_TRY(ensure_dev(c, c->col_flags, nblk * CJ_WAVES * sizeof(u64)));
      RC_TRY(ensure_dev(c, c->col_blk, nblk * sizeof(u64)));
      RC_TRY(ensure_dev(c, c->col_blk_off, (nblk + 1) * sizeof(u64)));
      DevBuf* cols[5] = {&c->col_key, &c->col_rrow, &c->col_srow, &c->col_rval, &c->col_sval};
      for (DevBuf* b : cols) RC_TRY(ensure_dev(c, *b, n_pairs * sizeof(u64)));
      hipLaunchKernelGGL(cols_verify_kernel<true>, dim3((u32)nblk), dim3(CJ_THREADS), 0, c->stream, ik, ir, is, n_pairs, RS, SS,
                         (u64*)c->col_flags.p, (u64*)c->col_blk.p, acc, 0, nullptr, nullptr);
      HIP_TRY(hipGetLastError());
      HIP_TRY(hmj::launch_scan_u64((const u64*)c->col_blk.p, (u64*)c->col_blk_off.p, (u32)nblk, c->stream));
      hipLaunchKernelGGL(cols_compact_kernel, dim3((u32)nblk), dim3(CJ_THREADS), 0, c->stream, ik, ir, is, n_pairs, RS, SS,
                         (const u64*)c->col_flags.p, (const u64*)c->col_blk_off.p, (u64*)c->col_key.p, (u64*)c->col_rrow.p,
                         (u64*)c->col_srow.p, (u64*)c->col_rval.p, (u64*)c->col_sval.p, acc, checksum ? 1 : 0);
      HIP_TRY(hipGetLastError());
      RC_TRY(read_back(c, (const u64*)c->col_blk_off.p + nblk, &n_out, sizeof(u64)));
    } else if (n_pairs) {
      hipLaunchKernelGGL(cols_verify_kernel<false>, dim3((u32)nblk), dim3(CJ_THREADS), 0, c->stream, ik, ir, is, n_pairs, RS, SS,
                         nullptr, nullptr, acc, checksum ? 1 : 0, nullptr, nullptr);
      HIP_TRY(hipGetLastError());
    }
    RC_TRY(record(c, 3));
    // 4. ordered: runs of equal key64 with different build tuples, sorted by the tuple
    if (ordered && n_out > 1) {
      const u64 cap = n_out < kListCap ? n_out : kListCap;
      RC_TRY(ensure_dev(c, c->col_list, cap * sizeof(u64)));
      RC_TRY(ensure_dev(c, c->col_runs, 2 * cap * sizeof(u64)));
      const u64 g = (n_out - 1 + CJ_THREADS - 1) / CJ_THREADS;
      hipLaunchKernelGGL(cols_mismatch_kernel<false>, dim3((u32)g), dim3(CJ_THREADS), 0, c->stream, (const u64*)c->col_key.p,
                         (const u64*)c->col_rrow.p, n_out, RS, (u64*)c->col_list.p, acc, nullptr, ColSide{});
      HIP_TRY(hipGetLastError());
      const u64 gl = (cap + CJ_THREADS - 1) / CJ_THREADS;
      hipLaunchKernelGGL(cols_run_leader_kernel<false>, dim3((u32)(gl < 1024 ? gl : 1024)), dim3(CJ_THREADS), 0, c->stream,
                         (const u64*)c->col_key.p, (const u64*)c->col_rrow.p, n_out, RS, (const u64*)c->col_list.p,
                         (u64*)c->col_runs.p, acc, nullptr, ColSide{});
      HIP_TRY(hipGetLastError());
      const u64 gs = cap < (u64)(4 * c->num_cus) ? cap : (u64)(4 * c->num_cus);
      hipLaunchKernelGGL(cols_run_sort_kernel<false>, dim3((u32)gs), dim3(CJ_THREADS), 0, c->stream, (const u64*)c->col_runs.p, RS,
                         (u64*)c->col_rrow.p, (u64*)c->col_srow.p, (u64*)c->col_rval.p, (u64*)c->col_sval.p, (const u64*)acc,
                         ColSide{});
      HIP_TRY(hipGetLastError());
    }
  }
  RC_TRY(record(c, 4));
  RC_TRY(read_back(c, acc, h, sizeof(h)));
  if (h[CA_ERR] & 1)
    return fail(c, HMJ_E_UNSUPPORTED, "multi-column join: a run of equal key64 with several distinct tuples holds more than 1024 rows");
  if (h[CA_ERR] & 2)
    return fail(c, HMJ_E_UNSUPPORTED, "multi-column join: more than 2^22 adjacent rows of equal key64 with different tuples");
  const u64* a = h + CA_ACC;
  out->n_matches = (hashed && mat) ? n_out : a[hmj::ACC_N];
  out->sum_r = a[hmj::ACC_SUM_R];
  out->sum_s = a[hmj::ACC_SUM_S];
  if (checksum) {
    out->xor_fold = a[hmj::ACC_XOR];
    out->mix_sum = a[hmj::ACC_MIX];
  }
  if (flags & HMJ_SUM_PROBE) out->sum_probe_all = h[CA_SUM_P];
  if (mat && !hashed) {
    out->key64 = (const uint64_t*)ik;
    out->r_row = (const uint64_t*)ir;
    out->s_row = (const uint64_t*)is;
    out->rval = (const uint64_t*)c->col_rval.p;
    out->sval = (const uint64_t*)c->col_sval.p;
  } else if (mat) {
    out->key64 = (const uint64_t*)c->col_key.p;
    out->r_row = (const uint64_t*)c->col_rrow.p;
    out->s_row = (const uint64_t*)c->col_srow.p;
    out->rval = (const uint64_t*)c->col_rval.p;
    out->sval = (const uint64_t*)c->col_sval.p;
  }
  opts->n_collisions = n_pairs - out->n_matches;
  return HMJ_OK;
}

// ---- join kinds (hmj_join_kind_cols_device) --------------------------------------------------------------------------
// workload_signature kinds of the {key64,row} joins the kinds run: none of them teaches a join of another entry anything
constexpr int kMemoProbeRep = 16;   // first-wins join, probe rows against build representatives (probe SEMI / ANTI)
constexpr int kMemoBuildRep = 17;   // ... build rows against probe representatives (BUILD_SEMI / BUILD_ANTI)
constexpr int kMemoAmbiguous = 18;  // the ambiguous rows against every row of their key64 on the other side
constexpr int kMemoPairs = 19;      // the outer kinds' pair join
constexpr int kKindAccBlocks = 3;   // acc: [0] keys, verification, collision search, [1] probe sweep, [2] build sweep

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

int join_cols_kind(hmj_ctx* c, const hmj_cols_rel* R, const hmj_cols_rel* S, uint32_t flags, hmj_cols_kind_opts* o, hmj_cols_result* out,
                   const ColValid* VB, const ColValid* VP) {
  const u64 nb = R->n, np = S->n;
  const u32 kind = o->kind;
  u32 total = 0;
  for (u32 k = 0; k < R->n_cols; k++) total += R->cols[k].width;
  const bool hashed = total > 8 || o->force_hashed;
  const u32 bits = hashed ? o->hash_bits : 0;
  if (flags & HMJ_ORDERED) flags |= HMJ_MATERIALIZE;
  const bool mat = flags & HMJ_MATERIALIZE, ordered = flags & HMJ_ORDERED, checksum = flags & HMJ_CHECKSUM;
  const bool bside = o->side == HMJ_KIND_BUILD_SIDE;
  // semi / anti of either side (HMJ_JOIN_SEMI == HMJ_BUILD_SEMI, HMJ_JOIN_ANTI == HMJ_BUILD_ANTI), else an outer kind
  const bool semi_anti = kind == HMJ_JOIN_SEMI || kind == HMJ_JOIN_ANTI;
  const bool sweep_p = bside ? kind == HMJ_FULL_OUTER : true;
  const bool sweep_b = bside;
  c->prep.valid = false;  // like any other call, a multi-column join discards a prepared build side
  std::memset(&c->plan, 0, sizeof(c->plan));
  c->plan.struct_size = sizeof(c->plan);
  std::memset(&c->timing, 0, sizeof(c->timing));
  RC_TRY(ensure_dev(c, c->col_acc, kKindAccBlocks * CA_N * sizeof(u64)));
  RC_TRY(ensure_dev(c, c->col_rows_r, 16 * (nb ? nb : 1)));
  RC_TRY(ensure_dev(c, c->col_rows_s, 16 * (np ? np : 1)));
  RC_TRY(ensure_dev(c, c->col_mark_r, nb ? nb : 1));
  RC_TRY(ensure_dev(c, c->col_mark_s, np ? np : 1));
  u64* acc = (u64*)c->col_acc.p;
  u64 *acc_p = acc + CA_N, *acc_b = acc + 2 * CA_N;
  u64 h[kKindAccBlocks * CA_N];
  const ColSide RS = side_of(R), SS = side_of(S);
  unsigned char *mark_r = (unsigned char*)c->col_mark_r.p, *mark_s = (unsigned char*)c->col_mark_s.p;
  // 1. {key64, row} rows of both relations (+ the probe payloads' sum), marks cleared
  RC_TRY(record(c, 0));
  HIP_TRY(hipMemsetAsync(acc, 0, kKindAccBlocks * CA_N * sizeof(u64), c->stream));
  // (NULL keys: the dense rows stay indexed by row for the sweeps; the u64 joins take only the rows that have a key)
  const void *rows_r = c->col_rows_r.p, *rows_s = c->col_rows_s.p;
  u64 nvb = nb, nvp = np;
  if (!VB && !VP) {
    RC_TRY(launch_key(c, RS, nb, hashed, bits, (u64*)c->col_rows_r.p, false, acc));
    RC_TRY(launch_key(c, SS, np, hashed, bits, (u64*)c->col_rows_s.p, flags & HMJ_SUM_PROBE, acc));
  } else {
    RC_TRY(launch_keys_valid(c, RS, SS, VB, VP, nb, np, hashed, bits, true, flags & HMJ_SUM_PROBE, acc, &rows_r, &nvb, &rows_s, &nvp));
    o->n_build_null = nb - nvb;
    o->n_probe_null = np - nvp;
  }
  if (nb) HIP_TRY(hipMemsetAsync(mark_r, 0, nb, c->stream));
  if (np) HIP_TRY(hipMemsetAsync(mark_s, 0, np, c->stream));
  RC_TRY(record(c, 1));
  o->form = hashed ? HMJ_COLS_HASHED : HMJ_COLS_PACKED;
  // 2. + 3. the {key64,row} join(s) and the tuple verification, which marks the rows that have a partner
  u64 n_pairs = 0;
  hmj_result inner;
  std::memset(&inner, 0, sizeof(inner));
  if (semi_anti) {
    // every row of the side asked about (K) meets the FIRST row of its key64 on the other side (O), in row order
    const u64 nK = bside ? nvb : nvp, nO = bside ? nvp : nvb;
    const void *rowsK = bside ? rows_r : rows_s, *rowsO = bside ? rows_s : rows_r;
    const ColSide &KS = bside ? RS : SS, &OS = bside ? SS : RS;
    unsigned char* mark = bside ? mark_r : mark_s;
    if (nK && nO) {
      hmj_result rep;
      RC_TRY(memo_join(c, rowsO, nO, rowsK, nK, HMJ_MATERIALIZE | HMJ_FIRST_WINS, bside ? kMemoBuildRep : kMemoProbeRep, &rep));
      RC_TRY(record(c, 2));
      n_pairs = rep.n_matches;  // <= nK
      if (n_pairs && !hashed) {
        hipLaunchKernelGGL(cols_rep_verify_kernel<false>, dim3((u32)blocks_of(n_pairs)), dim3(CJ_THREADS), 0, c->stream,
                           (const u64*)rep.key, (const u64*)rep.rval, (const u64*)rep.sval, n_pairs, OS, KS, mark, nullptr, acc);
        HIP_TRY(hipGetLastError());
      } else if (n_pairs) {
        RC_TRY(ensure_dev(c, c->col_amb, 16 * n_pairs));
        hipLaunchKernelGGL(cols_rep_verify_kernel<true>, dim3((u32)blocks_of(n_pairs)), dim3(CJ_THREADS), 0, c->stream,
                           (const u64*)rep.key, (const u64*)rep.rval, (const u64*)rep.sval, n_pairs, OS, KS, mark,
                           (u64*)c->col_amb.p, acc);
        HIP_TRY(hipGetLastError());
        RC_TRY(read_back(c, acc, h, CA_N * sizeof(u64)));
        const u64 n_amb = h[CA_AMB_N];
        if (n_amb) {  // (a collision: a representative's tuple differs from the row's)
          hmj_result all;
          RC_TRY(memo_join(c, rowsO, nO, c->col_amb.p, n_amb, HMJ_MATERIALIZE, kMemoAmbiguous, &all));
          n_pairs += all.n_matches;
          if (blocks_of(all.n_matches) > 0xFFFFFFFFull)
            return fail(c, HMJ_E_UNSUPPORTED, "multi-column join: more than 2^40 pairs of equal key64");
          if (all.n_matches) {
            hipLaunchKernelGGL(cols_rep_verify_kernel<true>, dim3((u32)blocks_of(all.n_matches)), dim3(CJ_THREADS), 0, c->stream,
                               (const u64*)all.key, (const u64*)all.rval, (const u64*)all.sval, all.n_matches, OS, KS, mark, nullptr,
                               acc);
            HIP_TRY(hipGetLastError());
          }
        }
      }
    } else {
      RC_TRY(record(c, 2));
    }
  } else if (nvb && nvp) {
    RC_TRY(memo_join(c, rows_r, nvb, rows_s, nvp, HMJ_MATERIALIZE | (flags & HMJ_ORDERED), kMemoPairs, &inner));
    RC_TRY(record(c, 2));
    n_pairs = inner.n_matches;
  } else {
    RC_TRY(record(c, 2));
  }
  if (blocks_of(n_pairs) > 0xFFFFFFFFull) return fail(c, HMJ_E_UNSUPPORTED, "multi-column join: more than 2^40 pairs of equal key64");
  o->n_key_pairs = n_pairs;
  // result rows: the pairs (outer kinds), then the probe sweep's rows, then the build sweep's
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
  if (nblk > 0xFFFFFFFFull) return fail(c, HMJ_E_UNSUPPORTED, "multi-column join: more than 2^40 pairs of equal key64");
  const u64 cap = (semi_anti ? 0 : n_pairs) + (sweep_p ? np : 0) + (sweep_b ? nb : 0);
  DevBuf* cols[5] = {&c->col_key, &c->col_rrow, &c->col_srow, &c->col_rval, &c->col_sval};
  if (mat) {
    RC_TRY(ensure_dev(c, c->col_flags, (nblk_v ? nblk_v : 1) * CJ_WAVES * sizeof(u64)));
    RC_TRY(ensure_dev(c, c->col_blk, (nblk ? nblk : 1) * sizeof(u64)));
    RC_TRY(ensure_dev(c, c->col_blk_off, (nblk + 1) * sizeof(u64)));
    for (DevBuf* b : cols) RC_TRY(ensure_dev(c, *b, (cap ? cap : 1) * sizeof(u64)));
  }
  u64* oc[5] = {(u64*)c->col_key.p, (u64*)c->col_rrow.p, (u64*)c->col_srow.p, (u64*)c->col_rval.p, (u64*)c->col_sval.p};
  if (semi_anti && !bside) oc[1] = oc[3] = nullptr;  // (key64, s_row, sval)
  if (semi_anti && bside) oc[2] = oc[4] = nullptr;   // (key64, r_row, rval)
  const u64 *ik = (const u64*)inner.key, *ir = (const u64*)inner.rval, *is = (const u64*)inner.sval;
  u64* blk = (u64*)c->col_blk.p;
  if (nblk_v && !hashed) {  // packed: every pair is a result row and marks its two rows
    const PairMark M{mark_r, mark_s, oc[0], oc[1], oc[2], blk};
    if (mat)
      hipLaunchKernelGGL((cols_gather_kernel<true, true>), dim3((u32)nblk_v), dim3(CJ_THREADS), 0, c->stream, ik, ir, is, n_pairs,
                         RS.vals, SS.vals, oc[3], oc[4], acc, checksum ? 1 : 0, M);
    else
      hipLaunchKernelGGL((cols_gather_kernel<false, true>), dim3((u32)nblk_v), dim3(CJ_THREADS), 0, c->stream, ik, ir, is, n_pairs,
                         RS.vals, SS.vals, nullptr, nullptr, acc, checksum ? 1 : 0, M);
    HIP_TRY(hipGetLastError());
  } else if (nblk_v) {  // hashed: the surviving pairs mark theirs
    if (mat)
      hipLaunchKernelGGL((cols_verify_kernel<true, true>), dim3((u32)nblk_v), dim3(CJ_THREADS), 0, c->stream, ik, ir, is, n_pairs, RS,
                         SS, (u64*)c->col_flags.p, blk, acc, 0, mark_r, mark_s);
    else
      hipLaunchKernelGGL((cols_verify_kernel<false, true>), dim3((u32)nblk_v), dim3(CJ_THREADS), 0, c->stream, ik, ir, is, n_pairs, RS,
                         SS, nullptr, nullptr, acc, checksum ? 1 : 0, mark_r, mark_s);
    HIP_TRY(hipGetLastError());
  }
  RC_TRY(record(c, 3));
  // 4. the sweeps: SEMI / BUILD_SEMI take the marked rows, every other kind the unmarked ones
  const u64 pfill = !semi_anti && (!bside || kind == HMJ_FULL_OUTER) ? o->probe_fill : 0ull;
  const u64 bfill = !semi_anti && bside ? o->build_fill : 0ull;
  const ColSweep WP{(const u64*)c->col_rows_s.p, mark_s, SS.vals, np, pfill, want, 1u, split_p ? 1u : 0u};
  const ColSweep WB{(const u64*)c->col_rows_r.p, mark_r, RS.vals, nb, bfill, want, 0u, split_b ? 1u : 0u};
  ColSweep TP = WP, TB = WB;  // the tails' sweeps
  TP.nulls = TB.nulls = 2u;
  u64 n_out = 0, n_in = 0, n_main = 0;  // result rows; of those, pairs (materialising); rows in front of the NULL-key tail
  if (mat) {
    const u64* blk_off = (const u64*)c->col_blk_off.p;
    if (nblk_p)
      hipLaunchKernelGGL(cols_sweep_count_kernel<true>, dim3((u32)nblk_p), dim3(CJ_THREADS), 0, c->stream, WP, blk + nblk_v, nullptr, 0);
    if (nblk_b)
      hipLaunchKernelGGL(cols_sweep_count_kernel<true>, dim3((u32)nblk_b), dim3(CJ_THREADS), 0, c->stream, WB, blk + nblk_v + nblk_p,
                         nullptr, 0);
    if (nblk_tb)
      hipLaunchKernelGGL(cols_sweep_count_kernel<true>, dim3((u32)nblk_tb), dim3(CJ_THREADS), 0, c->stream, TB, blk + nblk_m, nullptr, 0);
    if (nblk_tp)
      hipLaunchKernelGGL(cols_sweep_count_kernel<true>, dim3((u32)nblk_tp), dim3(CJ_THREADS), 0, c->stream, TP, blk + nblk_m + nblk_tb,
                         nullptr, 0);
    HIP_TRY(hipGetLastError());
    if (nblk) HIP_TRY(hmj::launch_scan_u64(blk, (u64*)c->col_blk_off.p, (u32)nblk, c->stream));
    if (nblk_v && hashed)
      hipLaunchKernelGGL(cols_compact_kernel, dim3((u32)nblk_v), dim3(CJ_THREADS), 0, c->stream, ik, ir, is, n_pairs, RS, SS,
                         (const u64*)c->col_flags.p, blk_off, oc[0], oc[1], oc[2], oc[3], oc[4], acc, checksum ? 1 : 0);
    if (nblk_p)
      hipLaunchKernelGGL(cols_sweep_emit_kernel, dim3((u32)nblk_p), dim3(CJ_THREADS), 0, c->stream, WP, blk_off + nblk_v, oc[0], oc[1],
                         oc[2], oc[3], oc[4], acc_p, checksum ? 1 : 0);
    if (nblk_b)
      hipLaunchKernelGGL(cols_sweep_emit_kernel, dim3((u32)nblk_b), dim3(CJ_THREADS), 0, c->stream, WB, blk_off + nblk_v + nblk_p,
                         oc[0], oc[1], oc[2], oc[3], oc[4], acc_b, checksum ? 1 : 0);
    if (nblk_tb)
      hipLaunchKernelGGL(cols_sweep_emit_kernel, dim3((u32)nblk_tb), dim3(CJ_THREADS), 0, c->stream, TB, blk_off + nblk_m, oc[0], oc[1],
                         oc[2], oc[3], oc[4], acc_b, checksum ? 1 : 0);
    if (nblk_tp)
      hipLaunchKernelGGL(cols_sweep_emit_kernel, dim3((u32)nblk_tp), dim3(CJ_THREADS), 0, c->stream, TP, blk_off + nblk_m + nblk_tb,
                         oc[0], oc[1], oc[2], oc[3], oc[4], acc_p, checksum ? 1 : 0);
    HIP_TRY(hipGetLastError());
    if (nblk) {
      HIP_TRY(hipMemcpyAsync(&n_in, blk_off + nblk_v, sizeof(u64), hipMemcpyDeviceToHost, c->stream));
      HIP_TRY(hipMemcpyAsync(&n_main, blk_off + nblk_m, sizeof(u64), hipMemcpyDeviceToHost, c->stream));
      RC_TRY(read_back(c, blk_off + nblk, &n_out, sizeof(u64)));
      if (n_main > n_out || n_out > cap) return fail(c, HMJ_E_HIP, "multi-column join: the sweeps' offsets exceed the result's capacity");
    }
  } else {
    if (nblk_p)
      hipLaunchKernelGGL(cols_sweep_count_kernel<false>, dim3((u32)nblk_p), dim3(CJ_THREADS), 0, c->stream, WP, nullptr, acc_p,
                         checksum ? 1 : 0);
    if (nblk_b)
      hipLaunchKernelGGL(cols_sweep_count_kernel<false>, dim3((u32)nblk_b), dim3(CJ_THREADS), 0, c->stream, WB, nullptr, acc_b,
                         checksum ? 1 : 0);
    HIP_TRY(hipGetLastError());
  }
  RC_TRY(record(c, 4));
  // 5. ordered: a stable sort of (key64, index) rows, the columns gathered in that order; hashed: then runs of equal key64
  // with several tuples sorted by tuple.  (Outer kinds without unmatched rows are already in (key64, r_row, s_row) order;
  // packed: equal key64 is equal tuples, so there is no collision to search for.)
  // NULL keys: only the n_main rows in front of the tail are sorted; the tail is already in its order and is copied behind.
  if (ordered && n_main > 1) {
    if (n_main > n_in) {
      RC_TRY(ensure_dev(c, c->col_ord, 32 * n_main));
      u64* ord = (u64*)c->col_ord.p;
      hipLaunchKernelGGL(cols_sort_rows_kernel, dim3((u32)blocks_of(n_main)), dim3(CJ_THREADS), 0, c->stream, oc[0], n_main, ord);
      HIP_TRY(hipGetLastError());
      const hmj_plan_desc plan = c->plan;  // (the sort is not a join: hmj_last_plan / hmj_last_timing keep describing the last one)
      const hmj_timing timing = c->timing;
      const int rc = hmj_sort_u64_device(c, ord, n_main, ord + 2 * n_main);
      c->plan = plan;
      c->timing = timing;
      if (rc != HMJ_OK) return rc;
      DevBuf* kc[5] = {&c->col_kkey, &c->col_krrow, &c->col_ksrow, &c->col_krval, &c->col_ksval};
      u64* nc[5];
      for (int k = 0; k < 5; k++) {
        nc[k] = nullptr;
        if (!oc[k]) continue;
        RC_TRY(ensure_dev(c, *kc[k], n_out * sizeof(u64)));
        nc[k] = (u64*)kc[k]->p;
      }
      hipLaunchKernelGGL(cols_order_gather_kernel, dim3((u32)blocks_of(n_main)), dim3(CJ_THREADS), 0, c->stream,
                         (const u64*)(ord + 2 * n_main), n_main, oc[1], oc[2], oc[3], oc[4], nc[0], nc[1], nc[2], nc[3], nc[4]);
      HIP_TRY(hipGetLastError());
      for (int k = 0; k < 5; k++) {
        if (nc[k] && n_out > n_main)
          HIP_TRY(hipMemcpyAsync(nc[k] + n_main, oc[k] + n_main, (n_out - n_main) * sizeof(u64), hipMemcpyDeviceToDevice, c->stream));
        oc[k] = nc[k];
      }
    }
    if (hashed) {
      const u64 lcap = n_main < kListCap ? n_main : kListCap;
      RC_TRY(ensure_dev(c, c->col_list, lcap * sizeof(u64)));
      RC_TRY(ensure_dev(c, c->col_runs, 2 * lcap * sizeof(u64)));
      hipLaunchKernelGGL(cols_mismatch_kernel<true>, dim3((u32)blocks_of(n_main - 1)), dim3(CJ_THREADS), 0, c->stream, (const u64*)oc[0],
                         (const u64*)oc[1], n_main, RS, (u64*)c->col_list.p, acc, (const u64*)oc[2], SS);
      HIP_TRY(hipGetLastError());
      const u64 gl = blocks_of(lcap);
      hipLaunchKernelGGL(cols_run_leader_kernel<true>, dim3((u32)(gl < 1024 ? gl : 1024)), dim3(CJ_THREADS), 0, c->stream,
                         (const u64*)oc[0], (const u64*)oc[1], n_main, RS, (const u64*)c->col_list.p, (u64*)c->col_runs.p, acc,
                         (const u64*)oc[2], SS);
      HIP_TRY(hipGetLastError());
      const u64 gs = lcap < (u64)(4 * c->num_cus) ? lcap : (u64)(4 * c->num_cus);
      hipLaunchKernelGGL(cols_run_sort_kernel<true>, dim3((u32)gs), dim3(CJ_THREADS), 0, c->stream, (const u64*)c->col_runs.p, RS, oc[1],
                         oc[2], oc[3], oc[4], (const u64*)acc, SS);
      HIP_TRY(hipGetLastError());
    }
  }
  RC_TRY(record(c, 5));
  RC_TRY(read_back(c, acc, h, sizeof(h)));
  if (h[CA_ERR] & 1)
    return fail(c, HMJ_E_UNSUPPORTED, "multi-column join: a run of equal key64 with several distinct tuples holds more than 1024 rows");
  if (h[CA_ERR] & 2)
    return fail(c, HMJ_E_UNSUPPORTED, "multi-column join: more than 2^22 adjacent rows of equal key64 with different tuples");
  // the sweeps count their rows in their acc blocks; the pairs: the scan (materialising) or acc (count modes)
  const u64 *av = h + CA_ACC, *ap = h + CA_N + CA_ACC, *ab = h + 2 * CA_N + CA_ACC;
  const u64 n_p = ap[hmj::ACC_N], n_b = ab[hmj::ACC_N];
  if (!mat) n_in = av[hmj::ACC_N];
  out->n_matches = n_in + n_p + n_b;
  out->sum_r = av[hmj::ACC_SUM_R] + ap[hmj::ACC_SUM_R] + ab[hmj::ACC_SUM_R];
  out->sum_s = av[hmj::ACC_SUM_S] + ap[hmj::ACC_SUM_S] + ab[hmj::ACC_SUM_S];
  if (checksum) {
    out->xor_fold = av[hmj::ACC_XOR] ^ ap[hmj::ACC_XOR] ^ ab[hmj::ACC_XOR];
    out->mix_sum = av[hmj::ACC_MIX] + ap[hmj::ACC_MIX] + ab[hmj::ACC_MIX];
  }
  if (flags & HMJ_SUM_PROBE) out->sum_probe_all = h[CA_SUM_P];
  if (mat) {
    out->key64 = (const uint64_t*)oc[0];
    out->r_row = (const uint64_t*)oc[1];
    out->s_row = (const uint64_t*)oc[2];
    out->rval = (const uint64_t*)oc[3];
    out->sval = (const uint64_t*)oc[4];
  }
  o->n_collisions = semi_anti ? h[CA_DIFF] : n_pairs - n_in;
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
// The out fields of a full-size copy o of the caller's opts are cleared from `first_out` on; the in fields that lie behind
// them (the validity arrays) are the caller's again, as far as its struct_size holds them.
void clear_out_fields(hmj_cols_kind_opts* o, const hmj_cols_kind_opts* opts, size_t first_out) {
  using T = hmj_cols_kind_opts;
  std::memset((char*)o + first_out, 0, sizeof(T) - first_out);
  const size_t lo = offsetof(T, build_validity), hi = offsetof(T, n_build_null);
  const size_t have = opts->struct_size < hi ? opts->struct_size : hi;
  if (have > lo) std::memcpy((char*)o + lo, (const char*)opts + lo, have - lo);
}

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
  std::memset(&o, 0, sizeof(o));
  std::memcpy(&o, opts, opts->struct_size < sizeof(o) ? opts->struct_size : sizeof(o));
  std::memset(&o.form, 0, sizeof(o) - offsetof(hmj_cols_join_opts, form));
  const int rc = join_cols(c, build, probe, flags, &o, out);
  if (rc != HMJ_OK) return rc;
  if (c->profiling) {
    (void)hipStreamSynchronize(c->stream);
    o.ms_key = elapsed(c, 0, 1);
    o.ms_join = elapsed(c, 1, 2);
    o.ms_verify = elapsed(c, 2, 3);
    o.ms_order = elapsed(c, 3, 4);
  }
  const uint32_t room = opts->struct_size < sizeof(o) ? opts->struct_size : (uint32_t)sizeof(o);
  o.struct_size = opts->struct_size;
  std::memcpy(opts, &o, room);
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
  std::memset(out, 0, sizeof(*out));
  HIP_TRY(hipSetDevice(c->device));
  // the out fields of opts go to a full-size copy first; the caller gets the prefix its struct_size holds
  hmj_cols_kind_opts o;
  std::memset(&o, 0, sizeof(o));
  std::memcpy(&o, opts, opts->struct_size < sizeof(o) ? opts->struct_size : sizeof(o));
  o.form = 0;
  clear_out_fields(&o, opts, offsetof(hmj_cols_kind_opts, counts));
  if (o.side == HMJ_KIND_PROBE_SIDE && o.kind == HMJ_JOIN_INNER) {  // exactly the inner multi-column join
    hmj_cols_join_opts jo;
    std::memset(&jo, 0, sizeof(jo));
    jo.struct_size = sizeof(jo);
    jo.hash_bits = o.hash_bits;
    jo.force_hashed = o.force_hashed;
    u64 n_null[2] = {0, 0};
    RC_TRY(join_cols(c, build, probe, flags, &jo, out, vb, vp, n_null));
    o.n_build_null = n_null[0];
    o.n_probe_null = n_null[1];
    u32 total = 0;  // (the inner entry leaves form 0 when a side is empty; here it is always filled)
    for (u32 k = 0; k < build->n_cols; k++) total += build->cols[k].width;
    o.form = total > 8 || o.force_hashed ? HMJ_COLS_HASHED : HMJ_COLS_PACKED;
    o.n_key_pairs = jo.n_key_pairs;
    o.n_collisions = jo.n_collisions;
    if (c->profiling) {
      (void)hipStreamSynchronize(c->stream);
      o.ms_key = elapsed(c, 0, 1);
      o.ms_join = elapsed(c, 1, 2);
      o.ms_verify = elapsed(c, 2, 3);
      o.ms_order = elapsed(c, 3, 4);
    }
  } else {
    RC_TRY(join_cols_kind(c, build, probe, flags, &o, out, vb, vp));
    if (c->profiling) {
      (void)hipStreamSynchronize(c->stream);
      o.ms_key = elapsed(c, 0, 1);
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
