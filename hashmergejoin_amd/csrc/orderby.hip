// Ordering rows by typed, string and mixed keys (hmj_order_by_device; include/hmj.h): a stable multi-column ORDER BY that
// returns a row map for hmj_take_cols_device / hmj_take_str_device.  Nothing in the reference corresponds beyond its u64
// sort, which the call uses (hmj_sort_u64_device).  Every row has an order-preserving byte stream (stream_window, hmj_order.h)
// whose memcmp order is the requested order; the rows are sorted by that stream, up to eight bytes of it per round:
//   order_key_kernel      round 0, one lane per row (workgroups walk tiles of 256 rows, grid-stride, as the heads and mark
//                         kernels do): checks the string columns' offsets (no decrease, no bytes under
//                         chars == NULL) before it follows any of them, writes {first 8 stream bytes, row} and reduces the
//                         longest stream S (one atomic per workgroup).
//   order_heads_kernel    behind a round's stable sort, one lane per sorted row: a head is a row whose word differs from its
//                         predecessor's; a wave's ballot is one word of head bits (group_heads_kernel's idiom).  The row goes
//                         to its position of the map.
//   order_mark_kernel     a row is ACTIVE when its segment holds several rows and its stream is longer than the bytes
//                         consumed; the stream is prefix-free, so the rows of a segment agree on that.  Ballots of active
//                         rows and of active segments' heads; both counts of a workgroup in the halves of one word, so that
//                         one scan places rows and ranks segments.  Rows of a segment that is exhausted are the tied rows.
//   order_compact_kernel  the active rows, in order, as {position, row} with their segment's rank.
//   order_refine_kernel   rounds >= 1, one lane per active row: the next b stream bytes under the s bits of the segment's
//                         rank.  One stable sort of these words sorts every segment at once (segments are contiguous and
//                         the compaction keeps their order); heads, marks and the compaction then run over the active rows
//                         only.  Resolved rows are never read or written again.
// The host loop is bounded by 1 + ceil(max(0, S - 8) / 4) rounds (every round consumes at least four bytes).  No device-side
// spin, no inline assembly; the counters (longest stream, heads, tied rows) take one atomic per workgroup, the offsets'
// verdict one per wave and column, and only in a wave that holds an offending row.  hmj_top_k_device (topk.hip) shares the
// stream, the argument checks and the refinement loop (order_refine_rows) through hmj_order.h.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdio>
#include <cstring>

#include "hmj_entry.h"
#include "hmj_order.h"

using hmj::u32;
using hmj::u64;
using namespace hmj_host;

using namespace hmj_order;

namespace {

constexpr int kMemoOrder = 25;  // workload_signature kind of the call's sorts (mixjoin.hip lists the others)

// Round 0.  A workgroup walks tiles of OB_THREADS rows, one lane per row (grid-stride: a grid of a few workgroups per CU
// keeps the counters at one atomic per workgroup -- one per tile put 2^16 atomics of a 2^24-row call on one address, which
// cost more than the kernel's memory traffic); no lane leaves the loop before the ballots of stream_window.
__global__ __launch_bounds__(OB_THREADS) void order_key_kernel(OrdCols T, u64 n, ulonglong2* __restrict__ rows, u64* __restrict__ acc) {
  __shared__ u64 red[OB_WAVES];
  const u64 tiles = (n + OB_THREADS - 1) / OB_THREADS;
  u64 best = 0;
  for (u64 tile = blockIdx.x; tile < tiles; tile += gridDim.x) {  // (uniform over the workgroup)
    const u64 i = tile * OB_THREADS + threadIdx.x;
    const bool active = i < n;
    u64 len = 0;
    const u64 word = stream_window<true>(T, active ? i : 0, active, 0, 8, len, acc);
    if (active) {
      rows[i] = make_ulonglong2(word, i);
      best = len > best ? len : best;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const u64 t = __shfl_xor(best, o, 64);
    best = t > best ? t : best;
  }
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = best;
  __syncthreads();
  if (threadIdx.x == 0) {
    u64 t = 0;
    for (int k = 0; k < OB_WAVES; k++) t = red[k] > t ? red[k] : t;
    atomicMax(&acc[OA_MAXLEN], t);
  }
}

// Rounds >= 1.  One lane per active row: word = segment rank << (64 - s) | the next b stream bytes, b = (64 - s) / 8 <= 8.
__global__ __launch_bounds__(OB_THREADS) void order_refine_kernel(OrdCols T, const ulonglong2* __restrict__ lst, const u32* __restrict__ rank,
                                                                  u64 m, u64 n, u64 cursor, u32 b, u32 s, ulonglong2* __restrict__ rows) {
  const u64 k = (u64)blockIdx.x * OB_THREADS + threadIdx.x;
  if (k >= m) return;
  const u64 r = lst[k].y;
  u64 len = 0, w = 0;
  if (r < n) w = stream_window<false>(T, r, true, cursor, b, len, nullptr);
  const u64 top = s ? (u64)rank[k] << (64u - s) : 0ull;
  rows[k] = make_ulonglong2(top | (w >> s), r);
}

// Tiles of OB_THREADS sorted rows of the round, one lane per row k < m, grid-stride as order_key_kernel; lst == NULL
// (round 0): row k sits at position k.  flags: one ballot word per wave of a tile; acc[OA_HEADS]: the round's heads.
__global__ __launch_bounds__(OB_THREADS) void order_heads_kernel(const ulonglong2* __restrict__ sorted, u64 m, u64 n,
                                                                 const ulonglong2* __restrict__ lst, u64* __restrict__ map,
                                                                 u64* __restrict__ flags, u64* __restrict__ acc) {
  __shared__ u32 wcnt[OB_WAVES];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const u64 tiles = (m + OB_THREADS - 1) / OB_THREADS;
  u32 heads = 0;  // (wave-uniform: popcounts of ballots)
  for (u64 tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const u64 k = tile * OB_THREADS + threadIdx.x;
    ulonglong2 e = make_ulonglong2(0, 0);
    if (k < m) e = sorted[k];
    u64 pk = __shfl_up(e.x, 1, 64);  // (every lane of the wave takes part)
    if (lane == 0 && k > 0 && k < m) pk = sorted[k - 1].x;
    const bool head = k < m && (k == 0 || e.x != pk);
    if (k < m) {
      const u64 at = lst ? lst[k].x : k;
      if (at < n) map[at] = e.y;
    }
    const u64 mk = __ballot(head);
    if (lane == 0) flags[k >> 6] = mk;
    heads += (u32)__builtin_popcountll(mk);
  }
  if (lane == 0) wcnt[w] = heads;
  __syncthreads();
  if (threadIdx.x == 0) {
    u64 t = 0;
    for (int q = 0; q < OB_WAVES; q++) t += wcnt[q];
    if (t) atomicAdd(&acc[OA_HEADS], t);
  }
}

// Tiles of OB_THREADS sorted rows of the round, grid-stride as above.  Row k's segment has several rows unless k and k + 1
// are both heads (behind the last row a head is implied); `consumed`: the stream bytes the rounds so far have sorted by;
// fixed_len != 0: every stream has this length (no string column).  blk[t]: active rows | active segments << 32 of tile t
// (order_compact_kernel's workgroup t); acc[OA_TIED]: rows of segments that are exhausted.
__global__ __launch_bounds__(OB_THREADS) void order_mark_kernel(OrdCols T, const ulonglong2* __restrict__ sorted, u64 m, u64 n,
                                                                const u64* __restrict__ flags, u64 consumed, u64 fixed_len,
                                                                u64* __restrict__ act, u64* __restrict__ acth, u64* __restrict__ blk,
                                                                u64* __restrict__ acc) {
  __shared__ u32 wa[OB_WAVES], wh[OB_WAVES], wt[OB_WAVES];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const u64 tiles = (m + OB_THREADS - 1) / OB_THREADS;
  u32 tied = 0;  // (wave-uniform)
  for (u64 tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const u64 k = tile * OB_THREADS + threadIdx.x;
    bool head = false, several = false, more = false;
    if (k < m) {
      head = (flags[k >> 6] >> lane) & 1ull;
      const bool next_head = k + 1 >= m || ((flags[(k + 1) >> 6] >> ((k + 1) & 63)) & 1ull);
      several = !(head && next_head);
      if (several) {
        u64 len = fixed_len;
        if (!fixed_len) {
          const u64 r = sorted[k].y;
          len = 0;
          if (r < n) (void)stream_window<false>(T, r, true, 0, 0, len, nullptr);
        }
        more = len > consumed;
      }
    }
    const u64 ma = __ballot(several && more), mh = __ballot(several && more && head), mt = __ballot(several && !more);
    tied += (u32)__builtin_popcountll(mt);
    if (lane == 0) {
      act[k >> 6] = ma;
      acth[k >> 6] = mh;
      wa[w] = (u32)__builtin_popcountll(ma);
      wh[w] = (u32)__builtin_popcountll(mh);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      u64 a = 0, h = 0;
      for (int q = 0; q < OB_WAVES; q++) {
        a += wa[q];
        h += wh[q];
      }
      blk[tile] = a | (h << 32);
    }
    __syncthreads();  // (the next tile's counts go to the same words)
  }
  if (lane == 0) wt[w] = tied;
  __syncthreads();
  if (threadIdx.x == 0) {
    u64 t = 0;
    for (int q = 0; q < OB_WAVES; q++) t += wt[q];
    if (t) atomicAdd(&acc[OA_TIED], t);
  }
}

// One lane per sorted row of the round (the grid of order_mark_kernel): active row k goes to slot blk_off's low half + the
// active rows in front of it in its workgroup, with rank = active segments' heads at or in front of it - 1.  cap: the slots.
__global__ __launch_bounds__(OB_THREADS) void order_compact_kernel(const ulonglong2* __restrict__ sorted, u64 m,
                                                                   const ulonglong2* __restrict__ lst, const u64* __restrict__ act,
                                                                   const u64* __restrict__ acth, const u64* __restrict__ blk_off,
                                                                   ulonglong2* __restrict__ lst_out, u32* __restrict__ rank_out, u64 cap) {
  const u64 k = (u64)blockIdx.x * OB_THREADS + threadIdx.x;
  if (k >= m) return;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const u64 ma = act[k >> 6];
  if (!((ma >> lane) & 1ull)) return;
  const u64 mh = acth[k >> 6];
  const u64 base = blk_off[blockIdx.x];
  const u64 f0 = ((u64)blockIdx.x * OB_THREADS) >> 6;
  const u64 through = lane == 63 ? ~0ull : ((2ull << lane) - 1ull);
  u64 a = (base & 0xffffffffull) + (u64)__builtin_popcountll(ma & (through >> 1));
  u64 h = (base >> 32) + (u64)__builtin_popcountll(mh & through);
  for (int q = 0; q < w; q++) {
    a += (u64)__builtin_popcountll(act[f0 + (u64)q]);
    h += (u64)__builtin_popcountll(acth[f0 + (u64)q]);
  }
  if (a >= cap || h == 0) return;  // (an active row follows its segment's head: never taken)
  lst_out[a] = make_ulonglong2(lst ? lst[k].x : k, sorted[k].y);
  rank_out[a] = (u32)(h - 1);
}

// ---- host side -----------------------------------------------------------------------------------------------------------
u64 blocks_of(u64 n) { return (n + OB_THREADS - 1) / OB_THREADS; }

// the stable u64 sort of a round; it is not a join: hmj_last_plan / hmj_last_timing keep describing the last one
int sort_round(hmj_ctx* c, const void* in, u64 m, void* out) {
  const hmj_plan_desc plan = c->plan;
  const hmj_timing timing = c->timing;
  c->memo_kind = kMemoOrder;
  const int rc = hmj_sort_u64_device(c, in, m, out);
  c->memo_kind = 0;
  c->plan = plan;
  c->timing = timing;
  return rc;
}

}  // namespace

namespace hmj_order {

void order_cols_of(const hmj_order_col* cols, u32 n_cols, OrdCols* T, u64* fixed_len) {
  std::memset(T, 0, sizeof(*T));
  T->k = n_cols;
  u64 len = 0;
  bool strings = false;
  for (u32 k = 0; k < n_cols; k++) {
    T->p[k] = cols[k].data;
    T->off[k] = (const u64*)cols[k].offsets;
    T->vb[k] = (const unsigned char*)cols[k].validity.bits;
    T->voff[k] = cols[k].validity.bit_offset;
    T->type[k] = cols[k].type;
    T->flags[k] = cols[k].flags;
    if (cols[k].type == HMJ_ORDER_LARGE_STRING) strings = true;
    else len += (T->vb[k] ? 1u : 0u) + width_of(cols[k].type);
  }
  *fixed_len = strings ? 0 : len;
}

int order_check_cols(hmj_ctx* c, const hmj_order_col* cols, u32 n_cols, u64 n, const u64* map, u64 map_entries) {
  char msg[192];
  if (n_cols < 1 || n_cols > HMJ_MAX_ORDER_COLS) {
    std::snprintf(msg, sizeof(msg), "hmj_order_by_device: n_cols must be in 1..%d", HMJ_MAX_ORDER_COLS);
    return fail(c, HMJ_E_ARG, msg);
  }
  if (n > 0xFFFFFFFFull) return fail(c, HMJ_E_ARG, "hmj_order_by_device: more than 2^32 - 1 rows");
  if (map_entries > 0 && !map) return fail(c, HMJ_E_ARG, "hmj_order_by_device: row_map_out is NULL");
  if (map_entries > 0 && ((uintptr_t)map & 7u)) return fail(c, HMJ_E_ARG, "hmj_order_by_device: row_map_out is not aligned to 8 bytes");
  for (u32 k = 0; k < n_cols; k++) {
    const hmj_order_col& s = cols[k];
    const bool str = s.type == HMJ_ORDER_LARGE_STRING;
    if (!str && s.type > HMJ_TYPE_F64) {
      std::snprintf(msg, sizeof(msg), "hmj_order_by_device: column %u has unknown type %u", k, s.type);
      return fail(c, HMJ_E_ARG, msg);
    }
    if (s.flags & ~(HMJ_ORDER_DESC | HMJ_ORDER_NULLS_FIRST)) {
      std::snprintf(msg, sizeof(msg), "hmj_order_by_device: column %u has unknown flag bits 0x%x", k, s.flags);
      return fail(c, HMJ_E_ARG, msg);
    }
    if (str) {
      if (!s.offsets) {
        std::snprintf(msg, sizeof(msg), "hmj_order_by_device: column %u: offsets is NULL", k);
        return fail(c, HMJ_E_ARG, msg);
      }
      if ((uintptr_t)s.offsets & 7u) {
        std::snprintf(msg, sizeof(msg), "hmj_order_by_device: column %u: offsets is not aligned to 8 bytes", k);
        return fail(c, HMJ_E_ARG, msg);
      }
    } else {
      const u32 w = width_of(s.type);
      if (s.offsets) {
        std::snprintf(msg, sizeof(msg), "hmj_order_by_device: column %u: offsets set on a fixed-width column", k);
        return fail(c, HMJ_E_ARG, msg);
      }
      if (n > 0 && !s.data) {
        std::snprintf(msg, sizeof(msg), "hmj_order_by_device: column %u: data is NULL", k);
        return fail(c, HMJ_E_ARG, msg);
      }
      if (n > 0 && ((uintptr_t)s.data & (uintptr_t)(w - 1))) {
        std::snprintf(msg, sizeof(msg), "hmj_order_by_device: column %u: data is not aligned to its width (%u)", k, w);
        return fail(c, HMJ_E_ARG, msg);
      }
    }
    if (validity_overflows(s.validity, n)) {
      std::snprintf(msg, sizeof(msg), "hmj_order_by_device: column %u: validity bit_offset + n overflows 64 bits", k);
      return fail(c, HMJ_E_ARG, msg);
    }
  }
  // The map must not be something the kernels read: address ranges, as hmj_take_cols_device checks them.  The extent of a
  // string column's chars is known on the device only.
  if (n == 0 || map_entries == 0) return HMJ_OK;
  const Range out = range_of(map, 8 * map_entries);
  for (u32 k = 0; k < n_cols; k++) {
    const hmj_order_col& s = cols[k];
    const bool str = s.type == HMJ_ORDER_LARGE_STRING;
    const Range in[2] = {str ? range_of(s.offsets, 8 * (n + 1)) : range_of(s.data, n * width_of(s.type)), validity_range(s.validity, n)};
    if (first_overlap(&out, 1, in, 2)) {
      std::snprintf(msg, sizeof(msg), "hmj_order_by_device: column %u: row_map_out overlaps the column's values, offsets or bitmap", k);
      return fail(c, HMJ_E_ARG, msg);
    }
  }
  return HMJ_OK;
}

int order_offsets_verdict(hmj_ctx* c, const u64* h) {
  char msg[192];
  for (int k = 0; k < kMaxCols; k++) {  // the lowest-numbered column first, the mixed-key join's wording
    if (h[OA_ERR + k] != kNone) {
      std::snprintf(msg, sizeof(msg), "ordered relation: column %d: offsets decrease at row %llu (offsets[%llu] < offsets[%llu])", k,
                    (unsigned long long)h[OA_ERR + k], (unsigned long long)h[OA_ERR + k] + 1, (unsigned long long)h[OA_ERR + k]);
      return fail(c, HMJ_E_ARG, msg);
    }
    if (h[OA_NODATA + k]) {
      std::snprintf(msg, sizeof(msg), "ordered relation: column %d: data is NULL but keys have bytes", k);
      return fail(c, HMJ_E_ARG, msg);
    }
  }
  return HMJ_OK;
}

int order_rows(hmj_ctx* c, const OrdCols& T, u64 fixed_len, u64 n, u64* map, hmj_order_opts* o) {
  OrderWs& ws = c->ord_ws;
  const u64 nblk = blocks_of(n);
  RC_TRY(ensure_dev(c, ws.acc, OA_N * sizeof(u64)));
  RC_TRY(ensure_dev(c, ws.rows, 16 * n));
  u64* acc = (u64*)ws.acc.p;
  const u64 most = (u64)c->num_cus * 8;  // workgroups of the grid-stride kernels
  u64 h[OA_N];
  // round 0: {first 8 stream bytes, row}; the key kernel's verdict on its input before anything else follows an offset
  RC_TRY(ws.ev.record(c, 0));
  HIP_TRY(hipMemsetAsync(acc, 0, OA_N * sizeof(u64), c->stream));
  HIP_TRY(hipMemsetAsync(acc + OA_ERR, 0xFF, kMaxCols * sizeof(u64), c->stream));
  hipLaunchKernelGGL(order_key_kernel, dim3((u32)(nblk < most ? nblk : most)), dim3(OB_THREADS), 0, c->stream, T, n, (ulonglong2*)ws.rows.p, acc);
  HIP_TRY(hipGetLastError());
  RC_TRY(ws.ev.record(c, 1));
  RC_TRY(read_back(c, acc, h, sizeof(h)));
  RC_TRY(order_offsets_verdict(c, h));
  return order_refine_rows(c, T, fixed_len, h[OA_MAXLEN], n, n, map, o);
}

int order_refine_rows(hmj_ctx* c, const OrdCols& T, u64 fixed_len, u64 S, u64 n_rows, u64 m0, u64* map, hmj_order_opts* o) {
  OrderWs& ws = c->ord_ws;
  const u64 nblk = blocks_of(m0);
  RC_TRY(ensure_dev(c, ws.acc, OA_N * sizeof(u64)));
  RC_TRY(ensure_dev(c, ws.sorted, 16 * m0));
  RC_TRY(ensure_dev(c, ws.heads, (nblk * OB_WAVES + 1) * sizeof(u64)));
  RC_TRY(ensure_dev(c, ws.act, nblk * OB_WAVES * sizeof(u64)));
  RC_TRY(ensure_dev(c, ws.acth, nblk * OB_WAVES * sizeof(u64)));
  RC_TRY(ensure_dev(c, ws.blk, nblk * sizeof(u64)));
  RC_TRY(ensure_dev(c, ws.blk_off, (nblk + 1) * sizeof(u64)));
  u64* acc = (u64*)ws.acc.p;
  ulonglong2* rows = (ulonglong2*)ws.rows.p;
  ulonglong2* sorted = (ulonglong2*)ws.sorted.p;
  const dim3 B(OB_THREADS);
  const u64 most = (u64)c->num_cus * 8;  // workgroups of the grid-stride kernels
  u64 h[2];
  const u64 bound = 1 + (S > 8 ? (S - 8 + 3) / 4 : 0);
  u64 m = m0, consumed = 0, heads = 0, segs = 0, tied = 0;
  u32 b = 8, rounds = 0;
  int cur = -1;  // the list of the round's rows; -1: every row, at its position
  for (;;) {
    RC_TRY(sort_round(c, rows, m, sorted));
    rounds++;
    if (rounds == 1) RC_TRY(ws.ev.record(c, 2));
    consumed += b;
    const u64 mblk = blocks_of(m);
    const dim3 G((u32)mblk), W((u32)(mblk < most ? mblk : most));
    const ulonglong2* lst = cur < 0 ? nullptr : (const ulonglong2*)ws.lst[cur].p;
    HIP_TRY(hipMemsetAsync(acc, 0, 2 * sizeof(u64), c->stream));  // OA_HEADS, OA_TIED
    hipLaunchKernelGGL(order_heads_kernel, W, B, 0, c->stream, (const ulonglong2*)sorted, m, m0, lst, map, (u64*)ws.heads.p, acc);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(order_mark_kernel, W, B, 0, c->stream, T, (const ulonglong2*)sorted, m, n_rows, (const u64*)ws.heads.p, consumed, fixed_len,
                       (u64*)ws.act.p, (u64*)ws.acth.p, (u64*)ws.blk.p, acc);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hmj::launch_scan_u64((const u64*)ws.blk.p, (u64*)ws.blk_off.p, (u32)mblk, c->stream));
    u64 tot = 0;
    HIP_TRY(hipMemcpyAsync(&tot, (const u64*)ws.blk_off.p + mblk, sizeof(u64), hipMemcpyDeviceToHost, c->stream));
    RC_TRY(read_back(c, acc, h, 2 * sizeof(u64)));
    heads += h[OA_HEADS];
    tied += h[OA_TIED];
    const u64 m2 = tot & 0xffffffffull, nseg = tot >> 32;
    if (m2 > m || 2 * nseg > m2 || (m2 && !nseg)) return fail(c, HMJ_E_HIP, "hmj_order_by_device: the active rows' count is not consistent");
    if (m2 == 0) break;
    if ((u64)rounds >= bound) return fail(c, HMJ_E_HIP, "hmj_order_by_device: refinement did not converge");
    segs += nseg;
    const int nxt = cur == 0 ? 1 : 0;
    RC_TRY(ensure_dev(c, ws.lst[nxt], 16 * m2));
    RC_TRY(ensure_dev(c, ws.rank[nxt], sizeof(u32) * m2));
    hipLaunchKernelGGL(order_compact_kernel, G, B, 0, c->stream, (const ulonglong2*)sorted, m, lst, (const u64*)ws.act.p, (const u64*)ws.acth.p,
                       (const u64*)ws.blk_off.p, (ulonglong2*)ws.lst[nxt].p, (u32*)ws.rank[nxt].p, m2);
    HIP_TRY(hipGetLastError());
    const u32 s = nseg > 1 ? 64u - (u32)__builtin_clzll(nseg - 1) : 0u;  // bits of a segment's rank (<= 31: 2 nseg <= m2 < 2^32)
    b = (64u - s) / 8u;
    hipLaunchKernelGGL(order_refine_kernel, dim3((u32)blocks_of(m2)), B, 0, c->stream, T, (const ulonglong2*)ws.lst[nxt].p, (const u32*)ws.rank[nxt].p,
                       m2, n_rows, consumed, b, s, rows);
    HIP_TRY(hipGetLastError());
    if (rounds == 1) RC_TRY(ws.ev.record(c, 3));
    m = m2;
    cur = nxt;
  }
  if (rounds == 1) RC_TRY(ws.ev.record(c, 3));
  RC_TRY(ws.ev.record(c, 4));
  if (heads < segs + 1 || heads - segs > m0) return fail(c, HMJ_E_HIP, "hmj_order_by_device: the heads' count is not in 1..n");
  o->n_distinct = heads - segs;  // every active segment of a round was counted as a head of the round before
  o->n_tied_rows = tied;
  o->n_rounds = rounds;
  if (c->profiling) {
    HIP_TRY(hipStreamSynchronize(c->stream));
    o->ms_key = ws.ev.ms(0, 1);
    o->ms_sort = ws.ev.ms(1, 2);
    o->ms_map = ws.ev.ms(2, 3);
    o->ms_refine = ws.ev.ms(3, 4);
  }
  return HMJ_OK;
}

}  // namespace hmj_order

extern "C" {

int hmj_order_by_device(hmj_ctx* c, const hmj_order_col* cols, uint32_t n_cols, uint64_t n, uint64_t* row_map_out,
                        hmj_order_opts* opts) {
  if (!c) return HMJ_E_ARG;
  if (!cols || !opts) return fail(c, HMJ_E_ARG, "hmj_order_by_device: cols / opts is NULL");
  if (opts->struct_size < offsetof(hmj_order_opts, reserved2) + sizeof(opts->reserved2))
    return fail(c, HMJ_E_ARG, "hmj_order_opts.struct_size too small");
  if (opts->reserved || opts->reserved2) return fail(c, HMJ_E_ARG, "hmj_order_opts: reserved must be 0");
  RC_TRY(order_check_cols(c, cols, n_cols, n, (const u64*)row_map_out, n));
  // the out fields of opts go to a full-size copy first; the caller gets the prefix its struct_size holds
  hmj_order_opts o;
  opts_prefix_in(&o, opts);
  opts_clear_out(&o, opts, offsetof(hmj_order_opts, n_distinct));
  if (n > 0) {
    HIP_TRY(hipSetDevice(c->device));
    c->prep.valid = false;  // (as hmj_sort_u64_device, which a call of one row does not reach)
    if (n == 1) {
      HIP_TRY(hipMemsetAsync(row_map_out, 0, sizeof(u64), c->stream));
      HIP_TRY(hipStreamSynchronize(c->stream));
      o.n_distinct = 1;
    } else {
      OrdCols T;
      u64 fixed_len = 0;
      order_cols_of(cols, n_cols, &T, &fixed_len);
      RC_TRY(order_rows(c, T, fixed_len, n, (u64*)row_map_out, &o));
    }
  }
  opts_prefix_out(opts, o);
  return HMJ_OK;
}

}  // extern "C"
