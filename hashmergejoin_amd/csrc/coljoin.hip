// Multi-column fixed-width keys on the device (hmj_join_cols_device; include/hmj.h).  Nothing in the reference
// corresponds: its operator is a template over ONE Key with std::hash<Key> (hashjoin.h:33-56).  The structure is the
// string join's (strjoin.hip) with the byte walks replaced by column loads; what the two share -- every kernel and launch
// sequence named below without a cols_ prefix -- lives in hmj_keyjoin.h and is instantiated here on ColSide.  This file
// holds the key kernels, the packed form's gather, the key policy (key_eq / key_cmp / payload on ColSide) and stages 1-3:
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
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdio>
#include <cstring>

#include "hmj_keyjoin.h"

namespace {

constexpr int CJ_THREADS = KJ_THREADS;  // the key kernels' workgroup: valid_count_kernel counts the rows of one of cols_key_valid_kernel
constexpr int CJ_WAVES = CJ_THREADS / 64;
constexpr int kMaxCols = HMJ_MAX_KEY_COLS;
constexpr u64 kGolden = 0x9E3779B97F4A7C15ull;

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

// The key policy of the shared kernels (hmj_keyjoin.h).  Both sides have the same column count and widths, so where a lane
// chooses its side at run time (the join kinds' mixed rows) the first lane's count and widths are every lane's: the choice
// only selects the column pointers, and col_load's switch stays a scalar branch.
__device__ __forceinline__ u32 uniform(u32 v) { return __builtin_amdgcn_readfirstlane(v); }
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
  hipLaunchKernelGGL(valid_count_kernel<ColValid>, dim3((u32)nblk), dim3(CJ_THREADS), 0, c->stream, V, n, cnt);
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

// Both relations' {key64,row} rows in a call with bitmaps (the block counts of both sides share vblk).
int launch_keys_valid(hmj_ctx* c, const ColSide& RS, const ColSide& SS, const ColValid* VB, const ColValid* VP, u64 nb, u64 np,
                      bool hashed, u32 bits, bool dense, bool sum_probe, u64* acc, const void** rows_r, u64* nvb, const void** rows_s,
                      u64* nvp) {
  KeyJoinWs& ws = c->col_ws;
  const u64 kb = VB ? blocks_of(nb) : 0, kp = VP ? blocks_of(np) : 0;
  RC_TRY(ensure_dev(c, ws.vblk, (2 * (kb + kp) + 2) * sizeof(u64)));
  u64* vblk = (u64*)ws.vblk.p;
  const ColValid none{};
  u64 *plain_r = (u64*)ws.rows_r.p, *plain_s = (u64*)ws.rows_s.p;
  RC_TRY(launch_key_valid(c, RS, VB ? *VB : none, VB != nullptr, nb, hashed, bits, dense ? plain_r : nullptr, plain_r, ws.cmp_r, vblk,
                          false, acc, rows_r, nvb));
  RC_TRY(launch_key_valid(c, SS, VP ? *VP : none, VP != nullptr, np, hashed, bits, dense ? plain_s : nullptr, plain_s, ws.cmp_s,
                          vblk + 2 * kb + 1, sum_probe, acc, rows_s, nvp));
  return HMJ_OK;
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
  KeyJoinWs& ws = c->col_ws;
  RC_TRY(ensure_dev(c, ws.acc, KA_N * sizeof(u64)));
  RC_TRY(ensure_dev(c, ws.rows_r, 16 * (nb ? nb : 1)));
  RC_TRY(ensure_dev(c, ws.rows_s, 16 * (np ? np : 1)));
  u64* acc = (u64*)ws.acc.p;
  u64 h[KA_N];
  const ColSide RS = side_of(R), SS = side_of(S);
  // 1. {key64, row} rows of both relations (+ the probe payloads' sum)
  RC_TRY(record(c, ws.ev, 0));
  HIP_TRY(hipMemsetAsync(acc, 0, KA_N * sizeof(u64), c->stream));
  const void *rows_r = ws.rows_r.p, *rows_s = ws.rows_s.p;  // the rows the u64 join takes
  u64 nvb = nb, nvp = np;                                           // ... and how many: the rows that have a key
  if (!VB && !VP) {
    RC_TRY(launch_key(c, RS, nb, hashed, bits, (u64*)ws.rows_r.p, false, acc));
    RC_TRY(launch_key(c, SS, np, hashed, bits, (u64*)ws.rows_s.p, flags & HMJ_SUM_PROBE, acc));
  } else {  // NULL keys: only the rows that have a key are joined (the inner join walks no relation by row: no dense rows)
    RC_TRY(launch_keys_valid(c, RS, SS, VB, VP, nb, np, hashed, bits, false, flags & HMJ_SUM_PROBE, acc, &rows_r, &nvb, &rows_s, &nvp));
    if (n_null) {
      n_null[0] = nb - nvb;
      n_null[1] = np - nvp;
    }
    if (nb && np) opts->form = hashed ? HMJ_COLS_HASHED : HMJ_COLS_PACKED;
  }
  RC_TRY(record(c, ws.ev, 1));
  if (nvb == 0 || nvp == 0) {  // (nothing to join: no plan either)
    std::memset(&c->plan, 0, sizeof(c->plan));
    c->plan.struct_size = sizeof(c->plan);
    std::memset(&c->timing, 0, sizeof(c->timing));
    for (int k = 2; k < 5; k++) RC_TRY(record(c, ws.ev, k));
    if (flags & HMJ_SUM_PROBE) {
      RC_TRY(read_back(c, acc, h, sizeof(h)));
      out->sum_probe_all = h[KA_SUM_P];
    }
    return HMJ_OK;
  }
  opts->form = hashed ? HMJ_COLS_HASHED : HMJ_COLS_PACKED;
  // 2. the u64 join of the {key64, row} rows: pairs of equal key64 as (key64, r_row, s_row), ordered by them if asked
  hmj_result inner;
  RC_TRY(memo_join(c, rows_r, nvb, rows_s, nvp, HMJ_MATERIALIZE | (flags & HMJ_ORDERED), kColsJoinMemoKind, &inner));
  RC_TRY(record(c, ws.ev, 2));
  const u64 n_pairs = inner.n_matches;
  opts->n_key_pairs = n_pairs;
  const u64 *ik = (const u64*)inner.key, *ir = (const u64*)inner.rval, *is = (const u64*)inner.sval;
  const u64 nblk = blocks_of(n_pairs);
  if (nblk > 0xFFFFFFFFull) return too_many_pairs(c, kNames);
  u64 n_out = 0;
  if (!hashed) {
    // 3a. packed: every pair is a result row; payloads gathered, or only reduced
    if (n_pairs && mat) {
      RC_TRY(ensure_dev(c, ws.rval, n_pairs * sizeof(u64)));
      RC_TRY(ensure_dev(c, ws.sval, n_pairs * sizeof(u64)));
      hipLaunchKernelGGL(cols_gather_kernel<true>, dim3((u32)nblk), dim3(CJ_THREADS), 0, c->stream, ik, ir, is, n_pairs, RS.vals,
                         SS.vals, (u64*)ws.rval.p, (u64*)ws.sval.p, acc, checksum ? 1 : 0, PairMark{});
      HIP_TRY(hipGetLastError());
    } else if (n_pairs) {
      hipLaunchKernelGGL(cols_gather_kernel<false>, dim3((u32)nblk), dim3(CJ_THREADS), 0, c->stream, ik, ir, is, n_pairs, RS.vals,
                         SS.vals, nullptr, nullptr, acc, checksum ? 1 : 0, PairMark{});
      HIP_TRY(hipGetLastError());
    }
    n_out = n_pairs;
    RC_TRY(record(c, ws.ev, 3));
  } else {
    // 3b. hashed: tuple verification, payload gather, stable compaction (or the count modes' reduction)
    if (n_pairs && mat) {
      RC_TRY(ensure_dev(c, ws.flags, nblk * CJ_WAVES * sizeof(u64)));
      RC_TRY(ensure_dev(c, ws.blk, nblk * sizeof(u64)));
      RC_TRY(ensure_dev(c, ws.blk_off, (nblk + 1) * sizeof(u64)));
      DevBuf* cols[5] = {&ws.key, &ws.rrow, &ws.srow, &ws.rval, &ws.sval};
      for (DevBuf* b : cols) RC_TRY(ensure_dev(c, *b, n_pairs * sizeof(u64)));
      hipLaunchKernelGGL((verify_kernel<ColSide, true>), dim3((u32)nblk), dim3(CJ_THREADS), 0, c->stream, ik, ir, is, n_pairs, RS, SS,
                         (u64*)ws.flags.p, (u64*)ws.blk.p, acc, 0, nullptr, nullptr);
      HIP_TRY(hipGetLastError());
      HIP_TRY(hmj::launch_scan_u64((const u64*)ws.blk.p, (u64*)ws.blk_off.p, (u32)nblk, c->stream));
      hipLaunchKernelGGL(compact_kernel<ColSide>, dim3((u32)nblk), dim3(CJ_THREADS), 0, c->stream, ik, ir, is, n_pairs, RS, SS,
                         (const u64*)ws.flags.p, (const u64*)ws.blk_off.p, (u64*)ws.key.p, (u64*)ws.rrow.p,
                         (u64*)ws.srow.p, (u64*)ws.rval.p, (u64*)ws.sval.p, acc, checksum ? 1 : 0);
      HIP_TRY(hipGetLastError());
      RC_TRY(read_back(c, (const u64*)ws.blk_off.p + nblk, &n_out, sizeof(u64)));
    } else if (n_pairs) {
      hipLaunchKernelGGL((verify_kernel<ColSide, false>), dim3((u32)nblk), dim3(CJ_THREADS), 0, c->stream, ik, ir, is, n_pairs, RS, SS,
                         nullptr, nullptr, acc, checksum ? 1 : 0, nullptr, nullptr);
      HIP_TRY(hipGetLastError());
    }
    RC_TRY(record(c, ws.ev, 3));
    // 4. ordered: runs of equal key64 with different build tuples, sorted by the tuple
    if (ordered && n_out > 1) {
      u64* cols[5] = {(u64*)ws.key.p, (u64*)ws.rrow.p, (u64*)ws.srow.p, (u64*)ws.rval.p, (u64*)ws.sval.p};
      RC_TRY(order_collisions<false>(c, ws, RS, ColSide{}, cols, n_out, acc));
    }
  }
  RC_TRY(record(c, ws.ev, 4));
  RC_TRY(read_back(c, acc, h, sizeof(h)));
  RC_TRY(collision_errors(c, kNames, h[KA_ERR]));
  const u64* a = h + KA_ACC;
  out->n_matches = (hashed && mat) ? n_out : a[hmj::ACC_N];
  out->sum_r = a[hmj::ACC_SUM_R];
  out->sum_s = a[hmj::ACC_SUM_S];
  if (checksum) {
    out->xor_fold = a[hmj::ACC_XOR];
    out->mix_sum = a[hmj::ACC_MIX];
  }
  if (flags & HMJ_SUM_PROBE) out->sum_probe_all = h[KA_SUM_P];
  if (mat && !hashed) {
    out->key64 = (const uint64_t*)ik;
    out->r_row = (const uint64_t*)ir;
    out->s_row = (const uint64_t*)is;
    out->rval = (const uint64_t*)ws.rval.p;
    out->sval = (const uint64_t*)ws.sval.p;
  } else if (mat) {
    out->key64 = (const uint64_t*)ws.key.p;
    out->r_row = (const uint64_t*)ws.rrow.p;
    out->s_row = (const uint64_t*)ws.srow.p;
    out->rval = (const uint64_t*)ws.rval.p;
    out->sval = (const uint64_t*)ws.sval.p;
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

int join_cols_kind(hmj_ctx* c, const hmj_cols_rel* R, const hmj_cols_rel* S, uint32_t flags, hmj_cols_kind_opts* o, hmj_cols_result* out,
                   const ColValid* VB, const ColValid* VP) {
  const u64 nb = R->n, np = S->n;
  const u32 kind = o->kind;
  u32 total = 0;
  for (u32 k = 0; k < R->n_cols; k++) total += R->cols[k].width;
  const bool hashed = total > 8 || o->force_hashed;
  const u32 bits = hashed ? o->hash_bits : 0;
  if (flags & HMJ_ORDERED) flags |= HMJ_MATERIALIZE;
  const bool mat = flags & HMJ_MATERIALIZE, checksum = flags & HMJ_CHECKSUM;
  const bool bside = o->side == HMJ_KIND_BUILD_SIDE;
  // semi / anti of either side (HMJ_JOIN_SEMI == HMJ_BUILD_SEMI, HMJ_JOIN_ANTI == HMJ_BUILD_ANTI), else an outer kind
  const bool semi_anti = kind == HMJ_JOIN_SEMI || kind == HMJ_JOIN_ANTI;
  c->prep.valid = false;  // like any other call, a multi-column join discards a prepared build side
  KeyJoinWs& ws = c->col_ws;
  std::memset(&c->plan, 0, sizeof(c->plan));
  c->plan.struct_size = sizeof(c->plan);
  std::memset(&c->timing, 0, sizeof(c->timing));
  RC_TRY(ensure_dev(c, ws.acc, kKindAccBlocks * KA_N * sizeof(u64)));
  RC_TRY(ensure_dev(c, ws.rows_r, 16 * (nb ? nb : 1)));
  RC_TRY(ensure_dev(c, ws.rows_s, 16 * (np ? np : 1)));
  RC_TRY(ensure_dev(c, ws.mark_r, nb ? nb : 1));
  RC_TRY(ensure_dev(c, ws.mark_s, np ? np : 1));
  u64* acc = (u64*)ws.acc.p;
  u64 *acc_p = acc + KA_N, *acc_b = acc + 2 * KA_N;
  u64 h[kKindAccBlocks * KA_N];
  const ColSide RS = side_of(R), SS = side_of(S);
  unsigned char *mark_r = (unsigned char*)ws.mark_r.p, *mark_s = (unsigned char*)ws.mark_s.p;
  // 1. {key64, row} rows of both relations (+ the probe payloads' sum), marks cleared
  RC_TRY(record(c, ws.ev, 0));
  HIP_TRY(hipMemsetAsync(acc, 0, kKindAccBlocks * KA_N * sizeof(u64), c->stream));
  // (NULL keys: the dense rows stay indexed by row for the sweeps; the u64 joins take only the rows that have a key)
  const void *rows_r = ws.rows_r.p, *rows_s = ws.rows_s.p;
  u64 nvb = nb, nvp = np;
  if (!VB && !VP) {
    RC_TRY(launch_key(c, RS, nb, hashed, bits, (u64*)ws.rows_r.p, false, acc));
    RC_TRY(launch_key(c, SS, np, hashed, bits, (u64*)ws.rows_s.p, flags & HMJ_SUM_PROBE, acc));
  } else {
    RC_TRY(launch_keys_valid(c, RS, SS, VB, VP, nb, np, hashed, bits, true, flags & HMJ_SUM_PROBE, acc, &rows_r, &nvb, &rows_s, &nvp));
    o->n_build_null = nb - nvb;
    o->n_probe_null = np - nvp;
  }
  if (nb) HIP_TRY(hipMemsetAsync(mark_r, 0, nb, c->stream));
  if (np) HIP_TRY(hipMemsetAsync(mark_s, 0, np, c->stream));
  RC_TRY(record(c, ws.ev, 1));
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
      RC_TRY(record(c, ws.ev, 2));
      n_pairs = rep.n_matches;  // <= nK
      if (n_pairs && !hashed) {
        hipLaunchKernelGGL((rep_verify_kernel<ColSide, false>), dim3((u32)blocks_of(n_pairs)), dim3(CJ_THREADS), 0, c->stream,
                           (const u64*)rep.key, (const u64*)rep.rval, (const u64*)rep.sval, n_pairs, OS, KS, mark, nullptr, acc);
        HIP_TRY(hipGetLastError());
      } else if (n_pairs) {
        RC_TRY(ensure_dev(c, ws.amb, 16 * n_pairs));
        hipLaunchKernelGGL((rep_verify_kernel<ColSide, true>), dim3((u32)blocks_of(n_pairs)), dim3(CJ_THREADS), 0, c->stream,
                           (const u64*)rep.key, (const u64*)rep.rval, (const u64*)rep.sval, n_pairs, OS, KS, mark,
                           (u64*)ws.amb.p, acc);
        HIP_TRY(hipGetLastError());
        RC_TRY(read_back(c, acc, h, KA_N * sizeof(u64)));
        const u64 n_amb = h[KA_AMB_N];
        if (n_amb) {  // (a collision: a representative's tuple differs from the row's)
          hmj_result all;
          RC_TRY(memo_join(c, rowsO, nO, ws.amb.p, n_amb, HMJ_MATERIALIZE, kMemoAmbiguous, &all));
          n_pairs += all.n_matches;
          if (blocks_of(all.n_matches) > 0xFFFFFFFFull) return too_many_pairs(c, kNames);
          if (all.n_matches) {
            hipLaunchKernelGGL((rep_verify_kernel<ColSide, true>), dim3((u32)blocks_of(all.n_matches)), dim3(CJ_THREADS), 0, c->stream,
                               (const u64*)all.key, (const u64*)all.rval, (const u64*)all.sval, all.n_matches, OS, KS, mark, nullptr,
                               acc);
            HIP_TRY(hipGetLastError());
          }
        }
      }
    } else {
      RC_TRY(record(c, ws.ev, 2));
    }
  } else if (nvb && nvp) {
    RC_TRY(memo_join(c, rows_r, nvb, rows_s, nvp, HMJ_MATERIALIZE | (flags & HMJ_ORDERED), kMemoPairs, &inner));
    RC_TRY(record(c, ws.ev, 2));
    n_pairs = inner.n_matches;
  } else {
    RC_TRY(record(c, ws.ev, 2));
  }
  o->n_key_pairs = n_pairs;
  KindRows k;
  RC_TRY(kind_rows(c, ws, kNames, o->side, kind, flags, nb, np, nvb, nvp, VB != nullptr, VP != nullptr, n_pairs, &k));
  const u64* pairs[3] = {(const u64*)inner.key, (const u64*)inner.rval, (const u64*)inner.sval};
  u64* blk = (u64*)ws.blk.p;
  if (k.nblk_v && !hashed) {  // packed: every pair is a result row and marks its two rows
    const PairMark M{mark_r, mark_s, k.oc[0], k.oc[1], k.oc[2], blk};
    if (mat)
      hipLaunchKernelGGL((cols_gather_kernel<true, true>), dim3((u32)k.nblk_v), dim3(CJ_THREADS), 0, c->stream, pairs[0], pairs[1],
                         pairs[2], n_pairs, RS.vals, SS.vals, k.oc[3], k.oc[4], acc, checksum ? 1 : 0, M);
    else
      hipLaunchKernelGGL((cols_gather_kernel<false, true>), dim3((u32)k.nblk_v), dim3(CJ_THREADS), 0, c->stream, pairs[0], pairs[1],
                         pairs[2], n_pairs, RS.vals, SS.vals, nullptr, nullptr, acc, checksum ? 1 : 0, M);
    HIP_TRY(hipGetLastError());
  } else if (k.nblk_v) {  // hashed: the surviving pairs mark theirs
    if (mat)
      hipLaunchKernelGGL((verify_kernel<ColSide, true, true>), dim3((u32)k.nblk_v), dim3(CJ_THREADS), 0, c->stream, pairs[0], pairs[1],
                         pairs[2], n_pairs, RS, SS, (u64*)ws.flags.p, blk, acc, 0, mark_r, mark_s);
    else
      hipLaunchKernelGGL((verify_kernel<ColSide, false, true>), dim3((u32)k.nblk_v), dim3(CJ_THREADS), 0, c->stream, pairs[0], pairs[1],
                         pairs[2], n_pairs, RS, SS, nullptr, nullptr, acc, checksum ? 1 : 0, mark_r, mark_s);
    HIP_TRY(hipGetLastError());
  }
  RC_TRY(record(c, ws.ev, 3));
  // 4. the sweeps (hashed: the pairs' survivors compacted in front of them), 5. ordered: the sort by key64, then -- hashed
  // only: packed, equal key64 is equal tuples, so there is no collision to search for -- runs of equal key64 with several
  // tuples sorted by tuple
  RC_TRY(kind_sweeps(c, ws, kNames, k, RS, SS, o->probe_fill, o->build_fill, hashed, pairs, acc, acc_p, acc_b));
  RC_TRY(record(c, ws.ev, 4));
  RC_TRY(kind_order(c, ws, k, RS, SS, hashed, acc));
  RC_TRY(record(c, ws.ev, 5));
  RC_TRY(read_back(c, acc, h, sizeof(h)));
  RC_TRY(collision_errors(c, kNames, h[KA_ERR]));
  kind_report(k, h + KA_ACC, h + KA_N + KA_ACC, h + 2 * KA_N + KA_ACC, out, &o->counts);
  if (flags & HMJ_SUM_PROBE) out->sum_probe_all = h[KA_SUM_P];
  if (mat) out->key64 = (const uint64_t*)k.oc[0];
  o->n_collisions = semi_anti ? h[KA_DIFF] : n_pairs - k.n_in;
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
    o.ms_key = elapsed(c->col_ws.ev, 0, 1);
    o.ms_join = elapsed(c->col_ws.ev, 1, 2);
    o.ms_verify = elapsed(c->col_ws.ev, 2, 3);
    o.ms_order = elapsed(c->col_ws.ev, 3, 4);
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
      o.ms_key = elapsed(c->col_ws.ev, 0, 1);
      o.ms_join = elapsed(c->col_ws.ev, 1, 2);
      o.ms_verify = elapsed(c->col_ws.ev, 2, 3);
      o.ms_order = elapsed(c->col_ws.ev, 3, 4);
    }
  } else {
    RC_TRY(join_cols_kind(c, build, probe, flags, &o, out, vb, vp));
    if (c->profiling) {
      (void)hipStreamSynchronize(c->stream);
      o.ms_key = elapsed(c->col_ws.ev, 0, 1);
      o.ms_join = elapsed(c->col_ws.ev, 1, 2);
      o.ms_verify = elapsed(c->col_ws.ev, 2, 3);
      o.ms_emit = elapsed(c->col_ws.ev, 3, 4);
      o.ms_order = elapsed(c->col_ws.ev, 4, 5);
    }
  }
  const uint32_t room = opts->struct_size < sizeof(o) ? opts->struct_size : (uint32_t)sizeof(o);
  o.struct_size = opts->struct_size;
  std::memcpy(opts, &o, room);
  return HMJ_OK;
}

}  // extern "C"
