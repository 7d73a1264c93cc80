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
// [2] sum of the probe payloads (HMJ_SUM_PROBE), [8..15] ACC_* sums
enum { CA_LIST_N = 0, CA_ERR, CA_SUM_P, CA_ACC = 8, CA_N = 16 };

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

// PACKED: every pair of the u64 join is a result row.  MAT: rval / sval gathered; always: count, sums, checksums into acc.
template <bool MAT>
__global__ __launch_bounds__(CJ_THREADS) void cols_gather_kernel(const u64* __restrict__ kk, const u64* __restrict__ rr,
                                                                 const u64* __restrict__ sr, u64 np, const u64* __restrict__ rvals,
                                                                 const u64* __restrict__ svals, u64* __restrict__ o_rv,
                                                                 u64* __restrict__ o_sv, u64* __restrict__ acc, int checksum) {
  __shared__ u64 red[8];
  if (threadIdx.x < 8) red[threadIdx.x] = 0;
  const u64 j = (u64)blockIdx.x * CJ_THREADS + threadIdx.x;
  u64 v[6] = {0, 0, 0, 0, 0, 0};
  if (j < np) {
    const u64 r = rr[j], s = sr[j];
    const u64 rv = rvals ? rvals[r] : r, sv = svals ? svals[s] : s;
    if (MAT) {
      o_rv[j] = rv;
      o_sv[j] = sv;
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
// Count modes (!MAT): counts, sums and checksums of the survivors straight into acc.
template <bool MAT>
__global__ __launch_bounds__(CJ_THREADS) void cols_verify_kernel(const u64* __restrict__ kk, const u64* __restrict__ rr,
                                                                 const u64* __restrict__ sr, u64 np, ColSide R, ColSide S,
                                                                 u64* __restrict__ flags, u64* __restrict__ blk_cnt,
                                                                 u64* __restrict__ acc, int checksum) {
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

// Collision search (ordered): row i whose key64 equals row i-1's but whose build tuple differs is recorded.
__global__ __launch_bounds__(CJ_THREADS) void cols_mismatch_kernel(const u64* __restrict__ kk, const u64* __restrict__ rr, u64 n,
                                                                   ColSide R, u64* __restrict__ list, u64* __restrict__ acc) {
  const u64 i = (u64)blockIdx.x * CJ_THREADS + threadIdx.x + 1;
  if (i >= n) return;
  if (kk[i] != kk[i - 1]) return;
  const u64 a = rr[i - 1], b = rr[i];
  if (a == b || tuple_eq(R, a, R, b)) return;
  const u64 k = atomicAdd(&acc[CA_LIST_N], 1ull);
  if (k < kListCap) list[k] = i;
  else atomicOr(&acc[CA_ERR], 2ull);
}

// One lane per recorded row i: its run [s, e) of equal key64 (binary searches on the ascending key64 column).  The lane
// whose i is the FIRST mismatch of its run leads it (runs[2k], runs[2k + 1] = s, e); the others write an empty run.  A
// separate launch from the sort, so that no leader test reads rows another workgroup is moving.
__global__ __launch_bounds__(CJ_THREADS) void cols_run_leader_kernel(const u64* __restrict__ kk, const u64* __restrict__ rr, u64 n,
                                                                     ColSide R, const u64* __restrict__ list, u64* __restrict__ runs,
                                                                     u64* __restrict__ acc) {
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
      const u64 a = rr[t - 1], b = rr[t];
      if (a != b && !tuple_eq(R, a, R, b)) first = false;
    }
    if (first) {
      runs[2 * k] = s;
      runs[2 * k + 1] = e;
    }
  }
}

// One workgroup per led run: rows sorted stably by build tuple (rank = rows with a smaller tuple + rows before it with
// the same tuple), written back in place.  All rows of a run share key64, so only r_row, s_row, rval, sval move.
__global__ __launch_bounds__(CJ_THREADS) void cols_run_sort_kernel(const u64* __restrict__ runs, ColSide R, u64* __restrict__ o_r,
                                                                   u64* __restrict__ o_s, u64* __restrict__ o_rv,
                                                                   u64* __restrict__ o_sv, const u64* __restrict__ acc) {
  __shared__ u64 col[4][kRunCap];
  __shared__ u32 rank[kRunCap];
  const u64 cnt = acc[CA_LIST_N] < kListCap ? acc[CA_LIST_N] : kListCap;
  for (u64 k = blockIdx.x; k < cnt; k += gridDim.x) {
    const u64 s = runs[2 * k], e = runs[2 * k + 1];
    if (e <= s) continue;  // (uniform: not a leader)
    const u32 L = (u32)(e - s);
    for (u32 t = threadIdx.x; t < L; t += CJ_THREADS) {
      col[0][t] = o_r[s + t];
      col[1][t] = o_s[s + t];
      col[2][t] = o_rv[s + t];
      col[3][t] = o_sv[s + t];
    }
    __syncthreads();
    for (u32 t = threadIdx.x; t < L; t += CJ_THREADS) {
      u32 rk = 0;
      const u64 me = col[0][t];
      for (u32 o = 0; o < L; o++) {
        const u64 other = col[0][o];
        const int cm = other == me ? 0 : tuple_cmp(R, other, me);
        rk += (cm < 0 || (cm == 0 && o < t)) ? 1u : 0u;
      }
      rank[t] = rk;
    }
    __syncthreads();
    for (u32 t = threadIdx.x; t < L; t += CJ_THREADS) {
      const u64 d = s + rank[t];
      o_r[d] = col[0][t];
      o_s[d] = col[1][t];
      o_rv[d] = col[2][t];
      o_sv[d] = col[3][t];
    }
    __syncthreads();
  }
}

// ---- host side -----------------------------------------------------------------------------------------------------------
constexpr int kColsJoinMemoKind = 14;  // workload_signature kind of the inner {key64,row} join (u64 joins 0, sorts 1, kinds
                                       // 3..9, string kinds 10..13, inner string join 15)

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

int join_cols(hmj_ctx* c, const hmj_cols_rel* R, const hmj_cols_rel* S, uint32_t flags, hmj_cols_join_opts* opts, hmj_cols_result* out) {
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
  RC_TRY(launch_key(c, RS, nb, hashed, bits, (u64*)c->col_rows_r.p, false, acc));
  RC_TRY(launch_key(c, SS, np, hashed, bits, (u64*)c->col_rows_s.p, flags & HMJ_SUM_PROBE, acc));
  RC_TRY(record(c, 1));
  if (nb == 0 || np == 0) {  // (nothing to join: no plan either)
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
  const int rc = join_device(c, c->col_rows_r.p, nb, c->col_rows_s.p, np, HMJ_MATERIALIZE | (flags & HMJ_ORDERED), &inner, false);
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
                         SS.vals, (u64*)c->col_rval.p, (u64*)c->col_sval.p, acc, checksum ? 1 : 0);
      HIP_TRY(hipGetLastError());
    } else if (n_pairs) {
      hipLaunchKernelGGL(cols_gather_kernel<false>, dim3((u32)nblk), dim3(CJ_THREADS), 0, c->stream, ik, ir, is, n_pairs, RS.vals,
                         SS.vals, nullptr, nullptr, acc, checksum ? 1 : 0);
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
                         (u64*)c->col_flags.p, (u64*)c->col_blk.p, acc, 0);
      HIP_TRY(hipGetLastError());
      HIP_TRY(hmj::launch_scan_u64((const u64*)c->col_blk.p, (u64*)c->col_blk_off.p, (u32)nblk, c->stream));
      hipLaunchKernelGGL(cols_compact_kernel, dim3((u32)nblk), dim3(CJ_THREADS), 0, c->stream, ik, ir, is, n_pairs, RS, SS,
                         (const u64*)c->col_flags.p, (const u64*)c->col_blk_off.p, (u64*)c->col_key.p, (u64*)c->col_rrow.p,
                         (u64*)c->col_srow.p, (u64*)c->col_rval.p, (u64*)c->col_sval.p, acc, checksum ? 1 : 0);
      HIP_TRY(hipGetLastError());
      RC_TRY(read_back(c, (const u64*)c->col_blk_off.p + nblk, &n_out, sizeof(u64)));
    } else if (n_pairs) {
      hipLaunchKernelGGL(cols_verify_kernel<false>, dim3((u32)nblk), dim3(CJ_THREADS), 0, c->stream, ik, ir, is, n_pairs, RS, SS,
                         nullptr, nullptr, acc, checksum ? 1 : 0);
      HIP_TRY(hipGetLastError());
    }
    RC_TRY(record(c, 3));
    // 4. ordered: runs of equal key64 with different build tuples, sorted by the tuple
    if (ordered && n_out > 1) {
      const u64 cap = n_out < kListCap ? n_out : kListCap;
      RC_TRY(ensure_dev(c, c->col_list, cap * sizeof(u64)));
      RC_TRY(ensure_dev(c, c->col_runs, 2 * cap * sizeof(u64)));
      const u64 g = (n_out - 1 + CJ_THREADS - 1) / CJ_THREADS;
      hipLaunchKernelGGL(cols_mismatch_kernel, dim3((u32)g), dim3(CJ_THREADS), 0, c->stream, (const u64*)c->col_key.p,
                         (const u64*)c->col_rrow.p, n_out, RS, (u64*)c->col_list.p, acc);
      HIP_TRY(hipGetLastError());
      const u64 gl = (cap + CJ_THREADS - 1) / CJ_THREADS;
      hipLaunchKernelGGL(cols_run_leader_kernel, dim3((u32)(gl < 1024 ? gl : 1024)), dim3(CJ_THREADS), 0, c->stream,
                         (const u64*)c->col_key.p, (const u64*)c->col_rrow.p, n_out, RS, (const u64*)c->col_list.p,
                         (u64*)c->col_runs.p, acc);
      HIP_TRY(hipGetLastError());
      const u64 gs = cap < (u64)(4 * c->num_cus) ? cap : (u64)(4 * c->num_cus);
      hipLaunchKernelGGL(cols_run_sort_kernel, dim3((u32)gs), dim3(CJ_THREADS), 0, c->stream, (const u64*)c->col_runs.p, RS,
                         (u64*)c->col_rrow.p, (u64*)c->col_srow.p, (u64*)c->col_rval.p, (u64*)c->col_sval.p, (const u64*)acc);
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

}  // namespace

extern "C" {

int hmj_join_cols_device(hmj_ctx* c, const hmj_cols_rel* build, const hmj_cols_rel* probe, uint32_t flags, hmj_cols_join_opts* opts,
                         hmj_cols_result* out) {
  if (!c) return HMJ_E_ARG;
  if (!opts || !out) return fail(c, HMJ_E_ARG, "opts / out is NULL");
  if (opts->struct_size < offsetof(hmj_cols_join_opts, force_hashed) + sizeof(opts->force_hashed))
    return fail(c, HMJ_E_ARG, "hmj_cols_join_opts.struct_size too small");
  if (opts->hash_bits > 63) return fail(c, HMJ_E_ARG, "hash_bits > 63");
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

}  // extern "C"
