// What the string-key join (strjoin.hip), the multi-column key join (coljoin.hip) and the mixed-key join (mixjoin.hip)
// share: all turn a relation into
// {key64, row} rows (a hash of the key, or the packed tuple), run the u64 join on those rows and then work on pairs and
// rows of equal key64.  Everything here is that second half, once, as templates over the relation-side struct of the
// including file (StrSide, ColSide, MixSide).  Internal header: its contents are local to the file that includes it.
//
// The key policy is the Side struct itself, with three overloads the including file keeps next to it:
//   bool key_eq(const Side& A, u64 a, const Side& B, u64 b)    row a of A and row b of B hold the same key
//   int  key_cmp(const Side& A, u64 a, const Side& B, u64 b)   -1 / 0 / 1 in the order the ordered results take
//   u64  payload(const Side& A, u64 row)                       the row's payload
// Kernels (KJ_THREADS lanes per workgroup):
//   valid_count_kernel                   rows that have a key, per workgroup (validity bitmaps; row_valid overload)
//   verify_kernel / compact_kernel       one lane per pair: keys compared, survivors compacted stably with their payloads
//   mismatch_kernel / run_leader_kernel / run_sort_kernel   the collision order (order_collisions below)
//   rep_verify_kernel                    the kinds' first-wins pairs: marks, and the ambiguous list
//   sweep_count_kernel / sweep_emit_kernel   the kinds' rows of one relation, selected by their marks
//   sort_rows_kernel / order_gather_kernel   the ordered kinds: (key64, index) rows for the u64 sort, columns gathered
// Host side: the launch sequences around them that both joins run (order_collisions, kind_sweeps, kind_order) and the
// small helpers of both (memo_join, blocks_of, collision_errors, kind_counts; read_back and the phase events: hmj_entry.h).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>

#include "hmj_entry.h"

namespace {

using hmj::u32;
using hmj::u64;
using namespace hmj_host;

constexpr int KJ_THREADS = 256;
constexpr int KJ_WAVES = KJ_THREADS / 64;
constexpr int kRunCap = 1024;         // rows of one mixed run the collision sort holds (one workgroup)
constexpr u64 kListCap = 1ull << 22;  // mismatching adjacent rows the collision search records
constexpr u64 kNoRow = ~0ull;
static_assert(kNoRow == HMJ_STR_NO_ROW && kNoRow == HMJ_COLS_NO_ROW, "one marker for a row without a partner");

// One accumulator block (u64 slots; a call owns several and says which one a stage adds to): [2] mismatch list length,
// [3] error bits (1 = a mixed run beyond kRunCap, 2 = list overflow), [4] ambiguous rows and [5] pairs whose keys differ
// (join kinds), [6] sum of the probe payloads (key kernels), [8..15] ACC_* sums.  [0] and [1] index the string hash kernels'
// report words of one relation instead: first row with decreasing offsets (~0 = none), keys with bytes but chars == NULL
enum { KA_BAD_ROW = 0, KA_NULL_CHARS, KA_LIST_N, KA_ERR, KA_AMB_N, KA_DIFF, KA_SUM_P, KA_ACC = 8, KA_N = 16 };

// What a caller's error messages call itself, its key64 and its keys.
struct KeyJoinNames {
  const char *join, *key64, *keys;
};

__device__ __forceinline__ u64 fold_bits(u64 h, u32 bits) { return bits ? h >> (64 - bits) : h; }

// A result row's key.  MIXED (join kinds): the build row's when r_row is present, else the probe row's (a NULL row column:
// every row is of the other side).  !MIXED: always the build row's.
struct RowRef {
  bool from_r;
  u64 row;
};
template <bool MIXED>
__device__ __forceinline__ RowRef row_of(u64 r, u64 s) {
  return !MIXED || r != kNoRow ? RowRef{true, r} : RowRef{false, s};
}
template <bool MIXED>
__device__ __forceinline__ RowRef row_ref(const u64* rr, const u64* sr, u64 i) {
  if constexpr (MIXED) return row_of<true>(rr ? rr[i] : kNoRow, sr ? sr[i] : kNoRow);
  else return RowRef{true, rr[i]};
}
// (the same row of the same side is equal without loading its key)
template <class Side>
__device__ __forceinline__ bool same_key(const Side& R, const Side& S, const RowRef& a, const RowRef& b) {
  if (a.from_r == b.from_r && a.row == b.row) return true;
  return key_eq(a.from_r ? R : S, a.row, b.from_r ? R : S, b.row);
}
template <class Side>
__device__ __forceinline__ int ref_cmp(const Side& R, const Side& S, const RowRef& a, const RowRef& b) {
  if (a.from_r == b.from_r && a.row == b.row) return 0;
  return key_cmp(a.from_r ? R : S, a.row, b.from_r ? R : S, b.row);
}

// NULL keys, pass 1 over the bitmaps alone: one lane per row (eight lanes share a byte, a wave reads 8-9 consecutive bytes
// per bitmap); the valid rows of workgroup b -- the KJ_THREADS rows workgroup b of the caller's second pass keys -- go to
// blk_cnt[b].
template <class Valid>
__global__ __launch_bounds__(KJ_THREADS) void valid_count_kernel(Valid V, u64 n, u64* __restrict__ blk_cnt) {
  __shared__ u32 wcnt[KJ_WAVES];
  const u64 i = (u64)blockIdx.x * KJ_THREADS + threadIdx.x;
  const bool ok = i < n && row_valid(V, i);
  const u64 m = __ballot(ok);
  if ((threadIdx.x & 63) == 0) wcnt[threadIdx.x >> 6] = (u32)__builtin_popcountll(m);
  __syncthreads();
  if (threadIdx.x == 0) {
    u64 t = 0;
    for (int k = 0; k < KJ_WAVES; k++) t += wcnt[k];
    blk_cnt[blockIdx.x] = t;
  }
}

// Pass 1 of the verification.  MAT: one ballot word per wave (flags) and the survivors per workgroup (blk_cnt).
// Count modes (!MAT): counts, sums and checksums of the survivors straight into acc.  MARK (outer join kinds): the
// survivors' build and probe rows are marked (one byte per row; every writer stores 1).
template <class Side, bool MAT, bool MARK = false>
__global__ __launch_bounds__(KJ_THREADS) void verify_kernel(const u64* __restrict__ kk, const u64* __restrict__ rr,
                                                            const u64* __restrict__ sr, u64 np, Side R, Side S, u64* __restrict__ flags,
                                                            u64* __restrict__ blk_cnt, u64* __restrict__ acc, int checksum,
                                                            unsigned char* __restrict__ mark_r, unsigned char* __restrict__ mark_s) {
  __shared__ u64 red[8];
  if (threadIdx.x < 8) red[threadIdx.x] = 0;
  __syncthreads();  // (wave 0 zeroes red[]; every wave's lane 0 adds to red[0] below)
  const u64 j = (u64)blockIdx.x * KJ_THREADS + threadIdx.x;
  bool keep = false;
  u64 r = 0, s = 0;
  if (j < np) {
    r = rr[j];
    s = sr[j];
    keep = key_eq(R, r, S, s);
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
    hmj::block_accumulate(red, acc + KA_ACC, v, 1u << hmj::ACC_XOR);
  }
}

// Pass 2: the survivors of workgroup b go, in pair order, to rows [blk_off[b], ..) of the five result columns.
template <class Side>
__global__ __launch_bounds__(KJ_THREADS) void compact_kernel(const u64* __restrict__ kk, const u64* __restrict__ rr,
                                                             const u64* __restrict__ sr, u64 np, Side R, Side S,
                                                             const u64* __restrict__ flags, const u64* __restrict__ blk_off,
                                                             u64* __restrict__ o_key, u64* __restrict__ o_r, u64* __restrict__ o_s,
                                                             u64* __restrict__ o_rv, u64* __restrict__ o_sv, u64* __restrict__ acc,
                                                             int checksum) {
  __shared__ u64 red[8];
  if (threadIdx.x < 8) red[threadIdx.x] = 0;
  const u64 j = (u64)blockIdx.x * KJ_THREADS + threadIdx.x;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  u64 v[6] = {0, 0, 0, 0, 0, 0};
  if (j < np) {
    const u64 m = flags[j >> 6];
    if ((m >> lane) & 1ull) {
      u64 pos = blk_off[blockIdx.x] + hmj::popc_below(m);
      const u64 f0 = ((u64)blockIdx.x * KJ_THREADS) >> 6;
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
  hmj::block_accumulate(red, acc + KA_ACC, v, 1u << hmj::ACC_XOR);
}

// Collision search (ordered): row i whose key64 equals row i-1's but whose key differs is recorded.  The rows' keys are
// row_ref<MIXED>'s (sr, S: the probe side, read by the join kinds only).
template <class Side, bool MIXED>
__global__ __launch_bounds__(KJ_THREADS) void mismatch_kernel(const u64* __restrict__ kk, const u64* __restrict__ rr, u64 n, Side R,
                                                              u64* __restrict__ list, u64* __restrict__ acc,
                                                              const u64* __restrict__ sr, Side S) {
  const u64 i = (u64)blockIdx.x * KJ_THREADS + threadIdx.x + 1;
  if (i >= n) return;
  if (kk[i] != kk[i - 1]) return;
  if (same_key(R, S, row_ref<MIXED>(rr, sr, i - 1), row_ref<MIXED>(rr, sr, i))) return;
  const u64 k = atomicAdd(&acc[KA_LIST_N], 1ull);
  if (k < kListCap) list[k] = i;
  else atomicOr(&acc[KA_ERR], 2ull);
}

// One lane per recorded row i: its run [s, e) of equal key64 (binary searches on the ascending key64 column).  The lane
// whose i is the FIRST mismatch of its run leads it (runs[2k], runs[2k + 1] = s, e); the others write an empty run.  A
// separate launch from the sort, so that no leader test reads rows another workgroup is moving.  MIXED as mismatch_kernel.
template <class Side, bool MIXED>
__global__ __launch_bounds__(KJ_THREADS) void run_leader_kernel(const u64* __restrict__ kk, const u64* __restrict__ rr, u64 n, Side R,
                                                                const u64* __restrict__ list, u64* __restrict__ runs,
                                                                u64* __restrict__ acc, const u64* __restrict__ sr, Side S) {
  const u64 cnt = acc[KA_LIST_N] < kListCap ? acc[KA_LIST_N] : kListCap;
  for (u64 k = (u64)blockIdx.x * KJ_THREADS + threadIdx.x; k < cnt; k += (u64)gridDim.x * KJ_THREADS) {
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
      atomicOr(&acc[KA_ERR], 1ull);
      continue;
    }
    bool first = true;
    for (u64 t = s + 1; t < i && first; t++)
      if (!same_key(R, S, row_ref<MIXED>(rr, sr, t - 1), row_ref<MIXED>(rr, sr, t))) first = false;
    if (first) {
      runs[2 * k] = s;
      runs[2 * k + 1] = e;
    }
  }
}

// One workgroup per led run: rows sorted stably by key (rank = rows with a smaller key + rows before it with the same
// key), written back in place.  All rows of a run share key64, so only r_row, s_row, rval, sval move.  MIXED: by
// row_of<true> (S: the probe side); a NULL column is absent (read as kNoRow / 0, not written).
template <class Side, bool MIXED>
__global__ __launch_bounds__(KJ_THREADS) void run_sort_kernel(const u64* __restrict__ runs, Side R, u64* __restrict__ o_r,
                                                              u64* __restrict__ o_s, u64* __restrict__ o_rv, u64* __restrict__ o_sv,
                                                              const u64* __restrict__ acc, Side S) {
  __shared__ u64 col[4][kRunCap];
  __shared__ u32 rank[kRunCap];
  const u64 cnt = acc[KA_LIST_N] < kListCap ? acc[KA_LIST_N] : kListCap;
  for (u64 k = blockIdx.x; k < cnt; k += gridDim.x) {
    const u64 s = runs[2 * k], e = runs[2 * k + 1];
    if (e <= s) continue;  // (uniform: not a leader)
    const u32 L = (u32)(e - s);
    for (u32 t = threadIdx.x; t < L; t += KJ_THREADS) {
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
    for (u32 t = threadIdx.x; t < L; t += KJ_THREADS) {
      u32 rk = 0;
      const RowRef me = row_of<MIXED>(col[0][t], col[1][t]);
      for (u32 o = 0; o < L; o++) {
        const int cm = ref_cmp(R, S, row_of<MIXED>(col[0][o], col[1][o]), me);
        rk += (cm < 0 || (cm == 0 && o < t)) ? 1u : 0u;
      }
      rank[t] = rk;
    }
    __syncthreads();
    for (u32 t = threadIdx.x; t < L; t += KJ_THREADS) {
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
// other side (O), the one representative of its key64 there.  !COMPARE (a key64 that IS the key): the pair marks its K row
// without loading a key.  COMPARE: equal keys mark the K row (every writer stores 1); different keys count in acc[KA_DIFF]
// and, when amb != NULL, the K row goes on the ambiguous list as a {key64, row} row (one counter add per wave) -- another
// O row of the same key64 may still hold its key.
template <class Side, bool COMPARE>
__global__ __launch_bounds__(KJ_THREADS) void rep_verify_kernel(const u64* __restrict__ kk, const u64* __restrict__ orow,
                                                                const u64* __restrict__ krow, u64 np, Side O, Side K,
                                                                unsigned char* __restrict__ mark, u64* __restrict__ amb,
                                                                u64* __restrict__ acc) {
  const u64 j = (u64)blockIdx.x * KJ_THREADS + threadIdx.x;
  bool diff = false;
  u64 k = 0;
  if (j < np) {
    k = krow[j];
    if (!COMPARE || key_eq(O, orow[j], K, k)) mark[k] = 1;
    else diff = true;
  }
  if (!COMPARE) return;
  const u64 m = __ballot(diff);
  if (!m) return;  // (wave-uniform)
  u64 base = 0;
  if ((threadIdx.x & 63) == 0) {
    atomicAdd(&acc[KA_DIFF], (u64)__builtin_popcountll(m));
    if (amb) base = atomicAdd(&acc[KA_AMB_N], (u64)__builtin_popcountll(m));
  }
  base = __shfl(base, 0, 64);
  if (amb && diff) reinterpret_cast<ulonglong2*>(amb)[base + hmj::popc_below(m)] = make_ulonglong2(kk[j], k);
}

// A relation's rows as the kinds emit them: row i ({key64, i} in rows) is selected when (mark[i] != 0) == want.  probe: the
// row goes out as (key64, NO_ROW, i, fill, payload), else as (key64, i, NO_ROW, payload, fill); NULL columns are not
// written.  nulls (ordered results of a relation with a validity bitmap, whose NULL-key rows carry kNoRow in rows): 0 =
// every selected row, 1 = only those with a key, 2 = only the NULL-key rows.
template <class Side>
struct Sweep {
  const u64* rows;
  const unsigned char* mark;
  Side rel;
  u64 n, fill;
  u32 want, probe, nulls;
};
template <class Side>
__device__ __forceinline__ bool sweep_sel(const Sweep<Side>& W, u64 i) {
  if (i >= W.n || (W.mark[i] != 0) != (W.want != 0)) return false;
  if (W.nulls == 0) return true;  // (uniform)
  return (W.rows[2 * i + 1] == kNoRow) == (W.nulls == 2);
}
template <class Side>
__device__ __forceinline__ void sweep_vals(const Sweep<Side>& W, u64 i, u64& rv, u64& sv) {
  const u64 v = payload(W.rel, i);
  rv = W.probe ? W.fill : v;
  sv = W.probe ? v : W.fill;
}

// Sweep pass 1.  MAT: selected rows per workgroup (blk_cnt).  Count modes: count, sums and checksums into acc.
template <class Side, bool MAT>
__global__ __launch_bounds__(KJ_THREADS) void sweep_count_kernel(Sweep<Side> W, u64* __restrict__ blk_cnt, u64* __restrict__ acc,
                                                                 int checksum) {
  __shared__ u64 red[8];
  if (threadIdx.x < 8) red[threadIdx.x] = 0;
  __syncthreads();
  const u64 i = (u64)blockIdx.x * KJ_THREADS + threadIdx.x;
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
    hmj::block_accumulate(red, acc + KA_ACC, v, 1u << hmj::ACC_XOR);
  }
}

// Sweep pass 2: the selected rows of workgroup b go, in row order, to rows [blk_off[b], ..) of the result columns (the
// wave's ballot places a lane inside its wave, the per-wave counts in LDS place the wave inside the workgroup); count, sums
// and checksums into acc.
template <class Side>
__global__ __launch_bounds__(KJ_THREADS) void sweep_emit_kernel(Sweep<Side> W, const u64* __restrict__ blk_off, u64* __restrict__ o_key,
                                                                u64* __restrict__ o_r, u64* __restrict__ o_s, u64* __restrict__ o_rv,
                                                                u64* __restrict__ o_sv, u64* __restrict__ acc, int checksum) {
  __shared__ u64 red[8];
  __shared__ u32 wcnt[KJ_WAVES];
  if (threadIdx.x < 8) red[threadIdx.x] = 0;
  const u64 i = (u64)blockIdx.x * KJ_THREADS + threadIdx.x;
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
  hmj::block_accumulate(red, acc + KA_ACC, v, 1u << hmj::ACC_XOR);
}

// Ordered kinds: (key64, index) rows for the stable u64 sort, then the result columns gathered in the sorted order.
__global__ __launch_bounds__(KJ_THREADS) void sort_rows_kernel(const u64* __restrict__ kk, u64 n, u64* __restrict__ rows) {
  const u64 i = (u64)blockIdx.x * KJ_THREADS + threadIdx.x;
  if (i < n) reinterpret_cast<ulonglong2*>(rows)[i] = make_ulonglong2(kk[i], i);
}
__global__ __launch_bounds__(KJ_THREADS) void order_gather_kernel(const u64* __restrict__ sorted, u64 n, const u64* __restrict__ i_r,
                                                                  const u64* __restrict__ i_s, const u64* __restrict__ i_rv,
                                                                  const u64* __restrict__ i_sv, u64* __restrict__ o_key,
                                                                  u64* __restrict__ o_r, u64* __restrict__ o_s, u64* __restrict__ o_rv,
                                                                  u64* __restrict__ o_sv) {
  const u64 j = (u64)blockIdx.x * KJ_THREADS + threadIdx.x;
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
u64 blocks_of(u64 n) { return (n + KJ_THREADS - 1) / KJ_THREADS; }

// join_device on {key64,row} rows under a workload_signature kind of its own (memo), with its spans collected.
// hmj_set_key_prefix_bits describes the CALLER'S u64 relations; key64 is a hash or a packed tuple, about which the caller
// promised nothing (a hint would place the partition window as if key64 shared those top bits: partitions would stop
// being key ranges, and an ordered result is not sorted again).  So this join samples its own keys, and the hint is put
// back for the caller's next u64 join on every way out.
// memo_kind is set for the duration of join_device only and is 0 again before anything else runs: hmj_sort_u64_device keys
// its memo by memo_kind when it is non-zero (hmj_order_by_device's sorts), so the sorts the key joins and group_rows reach
// (kind_order, hmj_group.h) must find it 0 to stay under the plain sort's kind 1.
int memo_join(hmj_ctx* c, const void* Rr, u64 nr, const void* Sr, u64 ns, uint32_t flags, int memo, hmj_result* out) {
  spans_reset(c);
  const int st = span_begin(c, K_TOTAL, -1);
  c->memo_kind = memo;
  const int hint = c->prefix_bits;
  c->prefix_bits = -1;
  const int rc = join_device(c, Rr, nr, Sr, ns, flags, out, false);
  c->prefix_bits = hint;
  c->memo_kind = 0;
  span_end(c, st);
  if (c->profiling) {
    (void)hipStreamSynchronize(c->stream);
    spans_collect(c);
  }
  return rc;
}

int too_many_pairs(hmj_ctx* c, const KeyJoinNames& nm) {
  char msg[160];
  std::snprintf(msg, sizeof(msg), "%s: more than 2^40 pairs of equal %s", nm.join, nm.key64);
  return fail(c, HMJ_E_UNSUPPORTED, msg);
}

// Collision order: runs of equal key64 (col[0], n rows, ascending) whose keys differ are sorted by key, each in one
// workgroup.  col: key64, r_row, s_row, rval, sval; MIXED: the kinds' rows (NULL columns absent; S: the probe side).
// Failures are bits in acc[KA_ERR], which the caller reads back with its sums (collision_errors).
template <bool MIXED, class Side>
int order_collisions(hmj_ctx* c, KeyJoinWs& ws, const Side& R, const Side& S, u64* const col[5], u64 n, u64* acc) {
  const u64 cap = n < kListCap ? n : kListCap;
  RC_TRY(ensure_dev(c, ws.list, cap * sizeof(u64)));
  RC_TRY(ensure_dev(c, ws.runs, 2 * cap * sizeof(u64)));
  u64 *list = (u64*)ws.list.p, *runs = (u64*)ws.runs.p;
  hipLaunchKernelGGL((mismatch_kernel<Side, MIXED>), dim3((u32)blocks_of(n - 1)), dim3(KJ_THREADS), 0, c->stream, (const u64*)col[0],
                     (const u64*)col[1], n, R, list, acc, (const u64*)col[2], S);
  HIP_TRY(hipGetLastError());
  const u64 gl = blocks_of(cap);
  hipLaunchKernelGGL((run_leader_kernel<Side, MIXED>), dim3((u32)(gl < 1024 ? gl : 1024)), dim3(KJ_THREADS), 0, c->stream,
                     (const u64*)col[0], (const u64*)col[1], n, R, (const u64*)list, runs, acc, (const u64*)col[2], S);
  HIP_TRY(hipGetLastError());
  const u64 gs = cap < (u64)(4 * c->num_cus) ? cap : (u64)(4 * c->num_cus);
  hipLaunchKernelGGL((run_sort_kernel<Side, MIXED>), dim3((u32)gs), dim3(KJ_THREADS), 0, c->stream, (const u64*)runs, R, col[1], col[2],
                     col[3], col[4], (const u64*)acc, S);
  HIP_TRY(hipGetLastError());
  return HMJ_OK;
}
int collision_errors(hmj_ctx* c, const KeyJoinNames& nm, u64 err) {
  char msg[192];
  if (err & 1) {
    std::snprintf(msg, sizeof(msg), "%s: a run of equal %s with several distinct %s holds more than 1024 rows", nm.join, nm.key64, nm.keys);
    return fail(c, HMJ_E_UNSUPPORTED, msg);
  }
  if (err & 2) {
    std::snprintf(msg, sizeof(msg), "%s: more than 2^22 adjacent rows of equal %s with different %s", nm.join, nm.key64, nm.keys);
    return fail(c, HMJ_E_UNSUPPORTED, msg);
  }
  return HMJ_OK;
}

// ---- the join kinds' result rows ---------------------------------------------------------------------------------------
// The verified pairs (outer kinds), then the probe sweep's rows, then the build sweep's.  Ordered, NULL keys: those sweeps
// take the rows that have a key, and a second launch per relation puts its NULL-key rows (never marked: only the kinds that
// take unmarked rows emit them) into a tail behind everything that is sorted -- the build side's in r_row order, then the
// probe side's in s_row order.
struct KindRows {
  u32 kind, want;  // want: the sweeps take the marked rows (SEMI / BUILD_SEMI), else the unmarked ones
  bool bside, semi_anti, mat, ordered, checksum, split_b, split_p;
  u64 nb, np, n_pairs;
  u64 nblk_v, nblk_p, nblk_b, nblk_tb, nblk_tp, nblk_m, nblk;  // workgroups: pairs, sweeps, tails; nblk_m: all in front of the tail
  u64 cap;                                                     // rows the result columns hold
  u64* oc[5];                                                  // key64, r_row, s_row, rval, sval (NULL: the kind has no such column)
  u64 n_out = 0, n_in = 0, n_main = 0;  // result rows; of those, verified pairs (materialising); rows in front of the tail
};

// Sizes a kind's result and allocates what the pairs' verification and the sweeps write (mat only).  has_vb / has_vp: the
// relation has a validity bitmap; nvb / nvp: its rows that have a key.
int kind_rows(hmj_ctx* c, KeyJoinWs& ws, const KeyJoinNames& nm, u32 side, u32 kind, uint32_t flags, u64 nb, u64 np, u64 nvb, u64 nvp,
              bool has_vb, bool has_vp, u64 n_pairs, KindRows* out) {
  KindRows& k = *out;
  if (blocks_of(n_pairs) > 0xFFFFFFFFull) return too_many_pairs(c, nm);
  k.kind = kind;
  k.want = kind == HMJ_JOIN_SEMI ? 1u : 0u;
  k.bside = side == HMJ_KIND_BUILD_SIDE;
  // semi / anti of either side (HMJ_JOIN_SEMI == HMJ_BUILD_SEMI, HMJ_JOIN_ANTI == HMJ_BUILD_ANTI), else an outer kind
  k.semi_anti = kind == HMJ_JOIN_SEMI || kind == HMJ_JOIN_ANTI;
  k.mat = flags & HMJ_MATERIALIZE;
  k.ordered = flags & HMJ_ORDERED;
  k.checksum = flags & HMJ_CHECKSUM;
  k.nb = nb;
  k.np = np;
  k.n_pairs = n_pairs;
  const bool sweep_p = k.bside ? kind == HMJ_FULL_OUTER : true, sweep_b = k.bside;
  k.split_b = k.ordered && has_vb;
  k.split_p = k.ordered && has_vp;
  k.nblk_v = k.semi_anti ? 0 : blocks_of(n_pairs);
  k.nblk_p = sweep_p ? blocks_of(np) : 0;
  k.nblk_b = sweep_b ? blocks_of(nb) : 0;
  k.nblk_tb = k.split_b && sweep_b && !k.want && nvb < nb ? blocks_of(nb) : 0;
  k.nblk_tp = k.split_p && sweep_p && !k.want && nvp < np ? blocks_of(np) : 0;
  k.nblk_m = k.nblk_v + k.nblk_p + k.nblk_b;
  k.nblk = k.nblk_m + k.nblk_tb + k.nblk_tp;
  if (k.nblk > 0xFFFFFFFFull) return too_many_pairs(c, nm);
  k.cap = (k.semi_anti ? 0 : n_pairs) + (sweep_p ? np : 0) + (sweep_b ? nb : 0);
  DevBuf* cols[5] = {&ws.key, &ws.rrow, &ws.srow, &ws.rval, &ws.sval};
  if (k.mat) {
    RC_TRY(ensure_dev(c, ws.flags, (k.nblk_v ? k.nblk_v : 1) * KJ_WAVES * sizeof(u64)));
    RC_TRY(ensure_dev(c, ws.blk, (k.nblk ? k.nblk : 1) * sizeof(u64)));
    RC_TRY(ensure_dev(c, ws.blk_off, (k.nblk + 1) * sizeof(u64)));
    for (DevBuf* b : cols) RC_TRY(ensure_dev(c, *b, (k.cap ? k.cap : 1) * sizeof(u64)));
  }
  for (int i = 0; i < 5; i++) k.oc[i] = (u64*)cols[i]->p;
  if (k.semi_anti && !k.bside) k.oc[1] = k.oc[3] = nullptr;  // (key64, s_row, sval)
  if (k.semi_anti && k.bside) k.oc[2] = k.oc[4] = nullptr;   // (key64, r_row, rval)
  return HMJ_OK;
}

// The sweeps: SEMI / BUILD_SEMI take the marked rows, every other kind the unmarked ones.  Materialising: the sweeps'
// per-workgroup counts join the pairs' in ws.blk (written by the caller's verification), one scan places them all, the
// pairs are compacted (compact: the caller's verification left ballots in ws.flags; pairs: key64 / r_row / s_row of the
// u64 join) and the sweeps emit behind them; k.n_in / n_main / n_out are read back.  Count modes: the sweeps reduce into
// their acc blocks.  acc_v / acc_p / acc_b: the blocks the pairs, the probe sweep and the build sweep add to.
template <class Side>
int kind_sweeps(hmj_ctx* c, KeyJoinWs& ws, const KeyJoinNames& nm, KindRows& k, const Side& R, const Side& S, u64 probe_fill,
                u64 build_fill, bool compact, const u64* const pairs[3], u64* acc_v, u64* acc_p, u64* acc_b) {
  const u64 pfill = !k.semi_anti && (!k.bside || k.kind == HMJ_FULL_OUTER) ? probe_fill : 0ull;
  const u64 bfill = !k.semi_anti && k.bside ? build_fill : 0ull;
  const Sweep<Side> WP{(const u64*)ws.rows_s.p, (const unsigned char*)ws.mark_s.p, S, k.np, pfill, k.want, 1u, k.split_p ? 1u : 0u};
  const Sweep<Side> WB{(const u64*)ws.rows_r.p, (const unsigned char*)ws.mark_r.p, R, k.nb, bfill, k.want, 0u, k.split_b ? 1u : 0u};
  Sweep<Side> TP = WP, TB = WB;  // the tails' sweeps
  TP.nulls = TB.nulls = 2u;
  const int cs = k.checksum ? 1 : 0;
  const dim3 T(KJ_THREADS);
  u64* const* oc = k.oc;
  if (!k.mat) {
    if (k.nblk_p) hipLaunchKernelGGL((sweep_count_kernel<Side, false>), dim3((u32)k.nblk_p), T, 0, c->stream, WP, nullptr, acc_p, cs);
    if (k.nblk_b) hipLaunchKernelGGL((sweep_count_kernel<Side, false>), dim3((u32)k.nblk_b), T, 0, c->stream, WB, nullptr, acc_b, cs);
    HIP_TRY(hipGetLastError());
    return HMJ_OK;
  }
  u64* blk = (u64*)ws.blk.p;
  const u64* blk_off = (const u64*)ws.blk_off.p;
  // where each launch's workgroups stand in blk / blk_off
  const u64 at_p = k.nblk_v, at_b = at_p + k.nblk_p, at_tb = k.nblk_m, at_tp = at_tb + k.nblk_tb;
  if (k.nblk_p) hipLaunchKernelGGL((sweep_count_kernel<Side, true>), dim3((u32)k.nblk_p), T, 0, c->stream, WP, blk + at_p, nullptr, 0);
  if (k.nblk_b) hipLaunchKernelGGL((sweep_count_kernel<Side, true>), dim3((u32)k.nblk_b), T, 0, c->stream, WB, blk + at_b, nullptr, 0);
  if (k.nblk_tb) hipLaunchKernelGGL((sweep_count_kernel<Side, true>), dim3((u32)k.nblk_tb), T, 0, c->stream, TB, blk + at_tb, nullptr, 0);
  if (k.nblk_tp) hipLaunchKernelGGL((sweep_count_kernel<Side, true>), dim3((u32)k.nblk_tp), T, 0, c->stream, TP, blk + at_tp, nullptr, 0);
  HIP_TRY(hipGetLastError());
  if (k.nblk) HIP_TRY(hmj::launch_scan_u64(blk, (u64*)ws.blk_off.p, (u32)k.nblk, c->stream));
  if (k.nblk_v && compact)
    hipLaunchKernelGGL(compact_kernel<Side>, dim3((u32)k.nblk_v), T, 0, c->stream, pairs[0], pairs[1], pairs[2], k.n_pairs, R, S,
                       (const u64*)ws.flags.p, blk_off, oc[0], oc[1], oc[2], oc[3], oc[4], acc_v, cs);
  if (k.nblk_p)
    hipLaunchKernelGGL(sweep_emit_kernel<Side>, dim3((u32)k.nblk_p), T, 0, c->stream, WP, blk_off + at_p, oc[0], oc[1], oc[2], oc[3],
                       oc[4], acc_p, cs);
  if (k.nblk_b)
    hipLaunchKernelGGL(sweep_emit_kernel<Side>, dim3((u32)k.nblk_b), T, 0, c->stream, WB, blk_off + at_b, oc[0], oc[1], oc[2], oc[3],
                       oc[4], acc_b, cs);
  if (k.nblk_tb)
    hipLaunchKernelGGL(sweep_emit_kernel<Side>, dim3((u32)k.nblk_tb), T, 0, c->stream, TB, blk_off + at_tb, oc[0], oc[1], oc[2], oc[3],
                       oc[4], acc_b, cs);
  if (k.nblk_tp)
    hipLaunchKernelGGL(sweep_emit_kernel<Side>, dim3((u32)k.nblk_tp), T, 0, c->stream, TP, blk_off + at_tp, oc[0], oc[1], oc[2], oc[3],
                       oc[4], acc_p, cs);
  HIP_TRY(hipGetLastError());
  if (k.nblk) {
    HIP_TRY(hipMemcpyAsync(&k.n_in, blk_off + k.nblk_v, sizeof(u64), hipMemcpyDeviceToHost, c->stream));
    if (k.nblk > k.nblk_m) HIP_TRY(hipMemcpyAsync(&k.n_main, blk_off + k.nblk_m, sizeof(u64), hipMemcpyDeviceToHost, c->stream));
    RC_TRY(read_back(c, blk_off + k.nblk, &k.n_out, sizeof(u64)));
    if (k.nblk == k.nblk_m) k.n_main = k.n_out;  // (no tail)
    if (k.n_main > k.n_out || k.n_out > k.cap) {
      char msg[128];
      std::snprintf(msg, sizeof(msg), "%s: the sweeps' offsets exceed the result's capacity", nm.join);
      return fail(c, HMJ_E_HIP, msg);
    }
  }
  return HMJ_OK;
}

// Ordered kinds: a stable sort of (key64, index) rows, the columns gathered in that order (k.oc then names the sorted
// columns), then -- collide: a key64 that is not the key itself -- runs of equal key64 with several keys sorted by key.
// (Outer kinds without unmatched rows are already in (key64, r_row, s_row) order.)  NULL keys: only the n_main rows in front
// of the tail are sorted; the tail is already in its order and is copied behind.
template <class Side>
int kind_order(hmj_ctx* c, KeyJoinWs& ws, KindRows& k, const Side& R, const Side& S, bool collide, u64* acc_v) {
  if (!k.ordered || k.n_main <= 1) return HMJ_OK;
  const u64 n_main = k.n_main, n_out = k.n_out;
  u64** oc = k.oc;
  if (n_main > k.n_in) {
    RC_TRY(ensure_dev(c, ws.ord, 32 * n_main));
    u64* ord = (u64*)ws.ord.p;
    hipLaunchKernelGGL(sort_rows_kernel, dim3((u32)blocks_of(n_main)), dim3(KJ_THREADS), 0, c->stream, oc[0], n_main, ord);
    HIP_TRY(hipGetLastError());
    const hmj_plan_desc plan = c->plan;  // (the sort is not a join: hmj_last_plan / hmj_last_timing keep describing the last one)
    const hmj_timing timing = c->timing;
    const int rc = hmj_sort_u64_device(c, ord, n_main, ord + 2 * n_main);
    c->plan = plan;
    c->timing = timing;
    if (rc != HMJ_OK) return rc;
    DevBuf* kc[5] = {&ws.kkey, &ws.krrow, &ws.ksrow, &ws.krval, &ws.ksval};
    u64* nc[5];
    for (int i = 0; i < 5; i++) {
      nc[i] = nullptr;
      if (!oc[i]) continue;
      RC_TRY(ensure_dev(c, *kc[i], n_out * sizeof(u64)));
      nc[i] = (u64*)kc[i]->p;
    }
    hipLaunchKernelGGL(order_gather_kernel, dim3((u32)blocks_of(n_main)), dim3(KJ_THREADS), 0, c->stream, (const u64*)(ord + 2 * n_main),
                       n_main, oc[1], oc[2], oc[3], oc[4], nc[0], nc[1], nc[2], nc[3], nc[4]);
    HIP_TRY(hipGetLastError());
    for (int i = 0; i < 5; i++) {
      if (nc[i] && n_out > n_main)
        HIP_TRY(hipMemcpyAsync(nc[i] + n_main, oc[i] + n_main, (n_out - n_main) * sizeof(u64), hipMemcpyDeviceToDevice, c->stream));
      oc[i] = nc[i];
    }
  }
  if (collide) RC_TRY(order_collisions<true>(c, ws, R, S, oc, n_main, acc_v));
  return HMJ_OK;
}

// What a kind call reports once its acc blocks are back on the host (av / ap / ab: the KA_ACC sums of the pairs, the probe
// sweep and the build sweep): the result's count, sums and columns, and the counters the u64 entry of the kind fills.
// The result's key64 column is set by the caller.
void kind_report(KindRows& k, const u64* av, const u64* ap, const u64* ab, hmj_cols_result* out, hmj_kind_counts* counts) {
  // the sweeps count their rows in their acc blocks; the pairs: the scan (materialising) or acc (count modes)
  const u64 n_p = ap[hmj::ACC_N], n_b = ab[hmj::ACC_N];
  if (!k.mat) k.n_in = av[hmj::ACC_N];
  out->n_matches = k.n_in + n_p + n_b;
  out->sum_r = av[hmj::ACC_SUM_R] + ap[hmj::ACC_SUM_R] + ab[hmj::ACC_SUM_R];
  out->sum_s = av[hmj::ACC_SUM_S] + ap[hmj::ACC_SUM_S] + ab[hmj::ACC_SUM_S];
  if (k.checksum) {
    out->xor_fold = av[hmj::ACC_XOR] ^ ap[hmj::ACC_XOR] ^ ab[hmj::ACC_XOR];
    out->mix_sum = av[hmj::ACC_MIX] + ap[hmj::ACC_MIX] + ab[hmj::ACC_MIX];
  }
  if (k.mat) {
    out->r_row = (const uint64_t*)k.oc[1];
    out->s_row = (const uint64_t*)k.oc[2];
    out->rval = (const uint64_t*)k.oc[3];
    out->sval = (const uint64_t*)k.oc[4];
  }
  std::memset(counts, 0, sizeof(*counts));
  if (!k.bside) {
    counts->n_probe_unmatched = k.kind == HMJ_JOIN_SEMI ? k.np - n_p : n_p;
    counts->n_probe_matched = k.np - counts->n_probe_unmatched;
  } else {
    counts->n_build_unmatched = k.kind == HMJ_BUILD_SEMI ? k.nb - n_b : n_b;
    counts->n_build_matched = k.nb - counts->n_build_unmatched;
    if (k.kind == HMJ_FULL_OUTER) {
      counts->n_probe_unmatched = n_p;
      counts->n_probe_matched = k.np - n_p;
    }
  }
}

}  // namespace
