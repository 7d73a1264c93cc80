// ORDER BY ... LIMIT k [OFFSET o] (hmj_top_k_device; include/hmj.h): entries offset .. offset + k of the map that
// hmj_order_by_device would return, without sorting the rows the cut rejects.  Nothing in the reference corresponds.  The
// rows' order is the memcmp order of their byte streams (stream_window, hmj_order.h), so the K = min(n, offset + k) smallest
// rows are found by a radix selection over the stream, eight bytes -- one WINDOW -- at a time:
//   topk_hist_kernel   a LEVEL: one lane per row of the window's population (every row in window 0, the tie list behind
//                      it; workgroups walk tiles of 256 rows, grid-stride).  A row whose word agrees with the threshold
//                      prefix decided so far counts into an LDS histogram of the level's digit (2048 bins; a wave whose
//                      matching lanes share one bin adds their popcount once); a workgroup flushes its non-zero bins with
//                      one global atomic each.  A window's first level also reduces the OR and the AND of the words -- the
//                      bits that vary --, and the call's first level checks the string columns' offsets before it follows
//                      any of them and reduces the longest stream S.  The host picks the threshold digit (hmj_topkplan.h).
//   topk_mark_kernel   ballots of "below the threshold" and "tied with it", both counts of a tile in the halves of one
//                      word (order_mark_kernel's idiom), the tied rows' stream length (they agree on it: the stream is
//                      prefix-free); hmj::launch_scan_u64 places the tiles.
//   topk_write_kernel  the rows below the threshold go to the candidates, the tied rows behind them or -- a whole window
//                      decided, bytes left, more ties than max_tie_rows -- to the tie list of the next window; each class
//                      in ascending row order, as {first stream word, row}.  Tied rows whose stream is used up are equal
//                      in every column: only the first K' of them by row index are written.
//   topk_gather_kernel a window behind the first: the tie list's next eight stream bytes (order_refine_kernel's form, s = 0).
// Rows with equal whole keys fall into the same class at every level and every list keeps ascending row order, so the
// refinement loop of orderby.hip (order_refine_rows), whose sorts are stable, orders the candidates exactly as the full
// ORDER BY orders them.  No device-side spin, no inline assembly; atomics on counters and histogram bins only.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdio>
#include <cstring>

#include "hmj_entry.h"
#include "hmj_order.h"
#include "hmj_topkplan.h"

using namespace hmj_order;
using namespace hmj_host;

namespace {

static_assert(kTopkThreads == (uint32_t)OB_THREADS, "the tiles of the top-k kernels are ORDER BY's");

// acc words behind ORDER BY's (the offsets' verdict and OA_MAXLEN are written by stream_window<true> and level 0): the OR
// and the AND of a window's words, the stream length of the rows tied with the threshold; the bins follow.
enum { TA_OR = OA_N, TA_AND, TA_TIELEN, TA_N };

// A level.  LIST: row k's word is words[k]; else row k's first eight stream bytes.  FIRST: the window's first level.
// above: the bits of a word at and above this one must equal prefix's (64: no bit is decided yet).
template <bool LIST, bool FIRST>
__global__ __launch_bounds__(OB_THREADS) void topk_hist_kernel(OrdCols T, u64 m, const u64* __restrict__ words, u64 prefix, u32 above,
                                                               u32 shift, u32 width, u64* __restrict__ acc) {
  __shared__ u32 bins[kTopkBins];
  __shared__ u64 red[3][OB_WAVES];
  for (u32 b = threadIdx.x; b < kTopkBins; b += OB_THREADS) bins[b] = 0;
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const u64 tiles = (m + OB_THREADS - 1) / OB_THREADS;
  const u32 dmask = (1u << width) - 1u;
  u64 best = 0, any = 0, all = ~0ull;
  for (u64 tile = blockIdx.x; tile < tiles; tile += gridDim.x) {  // (uniform over the workgroup)
    const u64 i = tile * OB_THREADS + threadIdx.x;
    const bool active = i < m;
    u64 len = 0, w = 0;
    if (LIST) {
      if (active) w = words[i];
    } else {
      w = stream_window<FIRST>(T, active ? i : 0, active, 0, 8, len, acc);
    }
    if (FIRST && active) {
      best = len > best ? len : best;
      any |= w;
      all &= w;
    }
    const bool match = active && (above >= 64u || (w >> above) == (prefix >> above));
    const u32 d = (u32)(w >> shift) & dmask;
    const u64 mask = __ballot(match);
    if (mask) {  // (wave-uniform)
      const int leader = (int)__builtin_ctzll(mask);
      const u32 d0 = __shfl(d, leader, 64);
      const u64 same = __ballot(match && d == d0);
      if (same == mask) {
        if (lane == leader) atomicAdd(&bins[d0], (u32)__builtin_popcountll(mask));
      } else if (match) {
        atomicAdd(&bins[d], 1u);
      }
    }
  }
  __syncthreads();
  u64* hist = acc + TA_N;
  for (u32 b = threadIdx.x; b < kTopkBins; b += OB_THREADS) {
    const u32 v = bins[b];
    if (v) atomicAdd(&hist[b], (u64)v);
  }
  if (FIRST) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const u64 t = __shfl_xor(best, o, 64);
      best = t > best ? t : best;
      any |= __shfl_xor(any, o, 64);
      all &= __shfl_xor(all, o, 64);
    }
    if (lane == 0) {
      red[0][threadIdx.x >> 6] = best;
      red[1][threadIdx.x >> 6] = any;
      red[2][threadIdx.x >> 6] = all;
    }
    __syncthreads();
    if (threadIdx.x == 0 && (u64)blockIdx.x < tiles) {  // (a workgroup without a tile has seen no word)
      u64 t = 0, o = 0, a = ~0ull;
      for (int k = 0; k < OB_WAVES; k++) {
        t = red[0][k] > t ? red[0][k] : t;
        o |= red[1][k];
        a &= red[2][k];
      }
      if (!LIST) atomicMax(&acc[OA_MAXLEN], t);
      atomicOr(&acc[TA_OR], o);
      atomicAnd(&acc[TA_AND], a);
    }
  }
}

// words[k]: bytes [cursor, cursor + 8) of the stream of the tie list's row k
__global__ __launch_bounds__(OB_THREADS) void topk_gather_kernel(OrdCols T, const ulonglong2* __restrict__ lst, u64 m, u64 n, u64 cursor,
                                                                 u64* __restrict__ words) {
  const u64 k = (u64)blockIdx.x * OB_THREADS + threadIdx.x;
  if (k >= m) return;
  const u64 r = lst[k].y;
  u64 len = 0, w = 0;
  if (r < n) w = stream_window<false>(T, r, true, cursor, 8, len, nullptr);
  words[k] = w;
}

// Tiles of OB_THREADS rows of the window's population, grid-stride.  A row is BELOW when the bits of its word at and above
// lo are smaller than prefix's, TIED when they are equal (lo <= 63).  fb / ft: one ballot word per wave of a tile;
// blk[t]: below | tied << 32 of tile t; acc[TA_TIELEN]: the stream length of the tied rows.
template <bool LIST>
__global__ __launch_bounds__(OB_THREADS) void topk_mark_kernel(OrdCols T, u64 m, u64 n, const ulonglong2* __restrict__ lst,
                                                               const u64* __restrict__ words, u64 prefix, u32 lo, u64* __restrict__ fb,
                                                               u64* __restrict__ ft, u64* __restrict__ blk, u64* __restrict__ acc) {
  __shared__ u32 wb[OB_WAVES], wt[OB_WAVES];
  __shared__ u64 wl[OB_WAVES];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const u64 tiles = (m + OB_THREADS - 1) / OB_THREADS;
  const u64 ph = prefix >> lo;
  u64 best = 0;
  for (u64 tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const u64 i = tile * OB_THREADS + threadIdx.x;
    const bool active = i < m;
    u64 len = 0, w = 0;
    if (LIST) {
      if (active) w = words[i];
    } else if (active) {
      w = stream_window<false>(T, i, true, 0, 8, len, nullptr);
    }
    const u64 hi = w >> lo;
    const bool below = active && hi < ph, tied = active && hi == ph;
    if (LIST && tied) {
      const u64 r = lst[i].y;
      if (r < n) (void)stream_window<false>(T, r, true, 0, 0, len, nullptr);
    }
    if (tied) best = len > best ? len : best;
    const u64 mb = __ballot(below), mt = __ballot(tied);
    if (lane == 0) {
      fb[i >> 6] = mb;
      ft[i >> 6] = mt;
      wb[wv] = (u32)__builtin_popcountll(mb);
      wt[wv] = (u32)__builtin_popcountll(mt);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      u64 b = 0, t = 0;
      for (int q = 0; q < OB_WAVES; q++) {
        b += wb[q];
        t += wt[q];
      }
      blk[tile] = b | (t << 32);
    }
    __syncthreads();  // (the next tile's counts go to the same words)
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const u64 t = __shfl_xor(best, o, 64);
    best = t > best ? t : best;
  }
  if (lane == 0) wl[wv] = best;
  __syncthreads();
  if (threadIdx.x == 0) {
    u64 t = 0;
    for (int q = 0; q < OB_WAVES; q++) t = wl[q] > t ? wl[q] : t;
    if (t) atomicMax(&acc[TA_TIELEN], t);
  }
}

// One lane per row of the population (workgroup t: tile t of topk_mark_kernel).  A row below the threshold goes to
// dst_below[its rank among them] (cap_below slots), a tied row to dst_tied[its rank] while that is below tie_limit; the
// word of a written row is its first stream word -- recomputed in column mode, the list entry's own in list mode.
template <bool LIST>
__global__ __launch_bounds__(OB_THREADS) void topk_write_kernel(OrdCols T, u64 m, const ulonglong2* __restrict__ lst, const u64* __restrict__ fb,
                                                                const u64* __restrict__ ft, const u64* __restrict__ blk_off,
                                                                ulonglong2* __restrict__ dst_below, u64 cap_below,
                                                                ulonglong2* __restrict__ dst_tied, u64 tie_limit) {
  const u64 i = (u64)blockIdx.x * OB_THREADS + threadIdx.x;
  if (i >= m) return;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const u64 mb = fb[i >> 6], mt = ft[i >> 6];
  const bool below = (mb >> lane) & 1ull, tied = (mt >> lane) & 1ull;
  if (!below && !tied) return;
  const u64* __restrict__ f = below ? fb : ft;
  const u64 base = blk_off[blockIdx.x];
  const u64 f0 = ((u64)blockIdx.x * OB_THREADS) >> 6;
  u64 at = (below ? (base & 0xffffffffull) : (base >> 32)) + (u64)__builtin_popcountll((below ? mb : mt) & ((1ull << lane) - 1ull));
  for (int q = 0; q < wv; q++) at += (u64)__builtin_popcountll(f[f0 + (u64)q]);
  if (at >= (below ? cap_below : tie_limit)) return;
  ulonglong2 e;
  if (LIST) {
    e = lst[i];
  } else {
    u64 len = 0;
    e = make_ulonglong2(stream_window<false>(T, i, true, 0, 8, len, nullptr), i);
  }
  (below ? dst_below : dst_tied)[at] = e;
}

// ---- host side -----------------------------------------------------------------------------------------------------------
u64 blocks_of(u64 n) { return (n + OB_THREADS - 1) / OB_THREADS; }

template <bool LIST>
void launch_hist(hmj_ctx* c, bool first, dim3 W, const OrdCols& T, u64 m, const u64* words, u64 prefix, u32 above, TopkDigit d, u64* acc) {
  if (first)
    hipLaunchKernelGGL((topk_hist_kernel<LIST, true>), W, dim3(OB_THREADS), 0, c->stream, T, m, words, prefix, above, d.shift, d.width, acc);
  else
    hipLaunchKernelGGL((topk_hist_kernel<LIST, false>), W, dim3(OB_THREADS), 0, c->stream, T, m, words, prefix, above, d.shift, d.width, acc);
}

// The SELECT plan: the candidates into OrderWs::rows, their count in *n_cand; S: the longest stream.  Event 1 falls behind
// the first window's levels: the marks, the writes and every later window are the emit phase.
int select_rows(hmj_ctx* c, const OrdCols& T, u64 n, u64 K, hmj_top_k_opts* o, u64* n_cand, u64* S_out) {
  TopkWs& ws = c->topk_ws;
  const TopkSizes sz = topk_sizes(n, TA_N);
  RC_TRY(ensure_dev(c, ws.acc, sz.acc));
  RC_TRY(ensure_dev(c, ws.below, sz.ballots));
  RC_TRY(ensure_dev(c, ws.tied, sz.ballots));
  RC_TRY(ensure_dev(c, ws.blk, sz.blk));
  RC_TRY(ensure_dev(c, ws.blk_off, sz.blk_off));
  u64* acc = (u64*)ws.acc.p;
  const dim3 B(OB_THREADS);
  const u64 most = (u64)c->num_cus * 8;  // workgroups of the grid-stride kernels
  const u64 tie_limit = topk_tie_limit(o->max_tie_rows);
  uint64_t h[TA_N + kTopkBins];  // a level's read-back
  u64 k_rest = K, definite = 0, pop = n, S = 0;
  u32 levels = 0, window = 0;
  int cur = -1;  // the tie list of the window; -1: every row
  for (;;) {
    const u64 mblk = blocks_of(pop);
    const dim3 G((u32)mblk), W((u32)(mblk < most ? mblk : most));
    const ulonglong2* lst = cur < 0 ? nullptr : (const ulonglong2*)ws.tie[cur].p;
    const u64* words = nullptr;
    if (cur >= 0) {
      RC_TRY(ensure_dev(c, ws.words, topk_word_bytes(pop)));
      hipLaunchKernelGGL(topk_gather_kernel, G, B, 0, c->stream, T, lst, pop, n, 8ull * window, (u64*)ws.words.p);
      HIP_TRY(hipGetLastError());
      words = (const u64*)ws.words.p;
    }
    // the levels of this window
    u64 prefix = 0, varying = 0, common = 0, win_below = 0, tie = pop;
    u32 lo = 64, stop = TOPK_GO;
    TopkDigit d = topk_first_digit();
    for (bool first = true;; first = false) {
      if (first) {
        HIP_TRY(hipMemsetAsync(acc, 0, sz.acc, c->stream));
        HIP_TRY(hipMemsetAsync(acc + OA_ERR, 0xFF, kMaxCols * sizeof(u64), c->stream));
        HIP_TRY(hipMemsetAsync(acc + TA_AND, 0xFF, sizeof(u64), c->stream));
      } else {
        HIP_TRY(hipMemsetAsync(acc + TA_N, 0, kTopkBins * sizeof(u64), c->stream));
      }
      const u32 above = d.shift + d.width;
      if (cur < 0) launch_hist<false>(c, first, W, T, pop, words, prefix, above, d, acc);
      else launch_hist<true>(c, first, W, T, pop, words, prefix, above, d, acc);
      HIP_TRY(hipGetLastError());
      RC_TRY(read_back(c, acc, h, sz.acc));
      levels++;
      if (first) {
        if (cur < 0) {  // the verdict on the input before anything else follows an offset
          RC_TRY(order_offsets_verdict(c, (const u64*)h));
          S = h[OA_MAXLEN];
        }
        varying = h[TA_OR] ^ h[TA_AND];
        common = h[TA_AND];
      }
      u64 sum = 0;
      for (u32 b = 0; b < (1u << d.width); b++) sum += h[TA_N + b];
      const TopkPick p = topk_pick(h + TA_N, 1u << d.width, k_rest, tie_limit);
      if (sum != tie || p.stop == TOPK_BAD) return fail(c, HMJ_E_HIP, "hmj_top_k_device: a level's histogram does not add up to its tie set");
      prefix |= (u64)p.digit << d.shift;
      lo = d.shift;
      win_below += p.below;
      k_rest = p.k_rest;
      tie = p.tie;
      stop = p.stop;
      if (stop != TOPK_GO) break;
      const TopkDigit nx = topk_next_digit(varying, lo);
      if (!nx.width) break;
      // the bits between the next digit and the decided ones are shared by every row of the window
      prefix |= topk_bits_from(common, nx.shift + nx.width) & ((1ull << lo) - 1ull);
      d = nx;
    }
    const bool decided = lo == 0 || !topk_next_digit(varying, lo).width;  // no row of the tie set differs below lo
    if (decided && lo) {
      prefix |= common & ((1ull << lo) - 1ull);
      lo = 0;
    }
    if (window == 0) RC_TRY(ws.ev.record(c, 1));
    // the classes of this window's population
    if (cur < 0)
      hipLaunchKernelGGL(topk_mark_kernel<false>, W, B, 0, c->stream, T, pop, n, lst, words, prefix, lo, (u64*)ws.below.p, (u64*)ws.tied.p,
                         (u64*)ws.blk.p, acc);
    else
      hipLaunchKernelGGL(topk_mark_kernel<true>, W, B, 0, c->stream, T, pop, n, lst, words, prefix, lo, (u64*)ws.below.p, (u64*)ws.tied.p,
                         (u64*)ws.blk.p, acc);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hmj::launch_scan_u64((const u64*)ws.blk.p, (u64*)ws.blk_off.p, (u32)mblk, c->stream));
    u64 tot = 0, tielen = 0;
    HIP_TRY(hipMemcpyAsync(&tot, (const u64*)ws.blk_off.p + mblk, sizeof(u64), hipMemcpyDeviceToHost, c->stream));
    RC_TRY(read_back(c, acc + TA_TIELEN, &tielen, sizeof(u64)));
    const u64 nb = tot & 0xffffffffull, nt = tot >> 32;
    if (nb != win_below || nt != tie || k_rest > nt) return fail(c, HMJ_E_HIP, "hmj_top_k_device: the marked rows do not match the histograms");
    const u64 consumed = 8ull * (window + 1);
    const bool exhausted = decided && tielen <= consumed;  // the tied rows are equal in every column
    const bool last = stop != TOPK_GO || exhausted;
    const u64 tie_write = exhausted ? k_rest : nt;
    if (window == 0) RC_TRY(ensure_dev(c, c->ord_ws.rows, topk_list_bytes(nb + (last ? tie_write : nt))));
    ulonglong2* cand = (ulonglong2*)c->ord_ws.rows.p + definite;
    ulonglong2* dst_tied = cand + nb;
    int nxt = cur;
    if (!last) {
      if (consumed >= S) return fail(c, HMJ_E_HIP, "hmj_top_k_device: ties with stream bytes left behind the longest stream");
      nxt = cur == 0 ? 1 : 0;
      RC_TRY(ensure_dev(c, ws.tie[nxt], topk_list_bytes(nt)));
      dst_tied = (ulonglong2*)ws.tie[nxt].p;
    }
    if (cur < 0)
      hipLaunchKernelGGL(topk_write_kernel<false>, G, B, 0, c->stream, T, pop, lst, (const u64*)ws.below.p, (const u64*)ws.tied.p,
                         (const u64*)ws.blk_off.p, cand, nb, dst_tied, tie_write);
    else
      hipLaunchKernelGGL(topk_write_kernel<true>, G, B, 0, c->stream, T, pop, lst, (const u64*)ws.below.p, (const u64*)ws.tied.p,
                         (const u64*)ws.blk_off.p, cand, nb, dst_tied, tie_write);
    HIP_TRY(hipGetLastError());
    definite += nb;
    if (last) {
      o->n_tie_rows = stop == TOPK_STOP_WHOLE ? 0 : nt;
      definite += tie_write;
      break;
    }
    pop = nt;
    cur = nxt;
    window++;
  }
  if (definite < K || definite > n) return fail(c, HMJ_E_HIP, "hmj_top_k_device: the candidates' count is not in K..n");
  o->n_levels = levels;
  *n_cand = definite;
  *S_out = S;
  return HMJ_OK;
}

}  // namespace

extern "C" {

int hmj_top_k_device(hmj_ctx* c, const hmj_order_col* cols, uint32_t n_cols, uint64_t n, uint64_t k, uint64_t* row_map_out,
                     hmj_top_k_opts* opts) {
  if (!c) return HMJ_E_ARG;
  if (!cols || !opts) return fail(c, HMJ_E_ARG, "hmj_top_k_device: cols / opts is NULL");
  if (opts->struct_size < offsetof(hmj_top_k_opts, max_tie_rows) + sizeof(opts->max_tie_rows))
    return fail(c, HMJ_E_ARG, "hmj_top_k_opts.struct_size too small");
  // the out fields of opts go to a full-size copy first; the caller gets the prefix its struct_size holds
  hmj_top_k_opts o;
  opts_prefix_in(&o, opts);
  if (o.plan > HMJ_TOPK_FULL) return fail(c, HMJ_E_ARG, "hmj_top_k_opts: unknown plan");
  if (o.reserved) return fail(c, HMJ_E_ARG, "hmj_top_k_opts: reserved must be 0");
  opts_clear_out(&o, opts, offsetof(hmj_top_k_opts, n_out));
  const u64 K = topk_cut(n, o.offset, k), n_out = topk_n_out(n, o.offset, k);
  RC_TRY(order_check_cols(c, cols, n_cols, n, (const u64*)row_map_out, n_out));
  if (n_out > 0) {
    HIP_TRY(hipSetDevice(c->device));
    c->prep.valid = false;  // (as hmj_order_by_device)
    TopkWs& ws = c->topk_ws;
    o.n_out = n_out;
    if (n == 1) {
      HIP_TRY(hipMemsetAsync(row_map_out, 0, sizeof(u64), c->stream));
      HIP_TRY(hipStreamSynchronize(c->stream));
      o.n_candidates = 1;
    } else {
      OrdCols T;
      u64 fixed_len = 0;
      order_cols_of(cols, n_cols, &T, &fixed_len);
      hmj_order_opts oo;
      std::memset(&oo, 0, sizeof(oo));
      const bool full = o.plan == HMJ_TOPK_FULL || (o.plan == HMJ_TOPK_AUTO && topk_auto_full(n, K));
      u64 n_cand = n;
      RC_TRY(ws.ev.record(c, 0));
      if (full) {
        RC_TRY(ensure_dev(c, ws.map, topk_sizes(n, TA_N).map));
        RC_TRY(ws.ev.record(c, 1));
        RC_TRY(ws.ev.record(c, 2));
        RC_TRY(order_rows(c, T, fixed_len, n, (u64*)ws.map.p, &oo));
      } else {
        u64 S = 0;
        RC_TRY(select_rows(c, T, n, K, &o, &n_cand, &S));
        RC_TRY(ws.ev.record(c, 2));
        RC_TRY(ensure_dev(c, ws.map, topk_sizes(n_cand, TA_N).map));
        if (n_cand == 1) {  // (nothing to sort)
          HIP_TRY(hipMemcpyAsync(ws.map.p, (const char*)c->ord_ws.rows.p + 8, sizeof(u64), hipMemcpyDeviceToDevice, c->stream));
        } else {
          RC_TRY(order_refine_rows(c, T, fixed_len, S, n, n_cand, (u64*)ws.map.p, &oo));
        }
      }
      HIP_TRY(hipMemcpyAsync(row_map_out, (const u64*)ws.map.p + o.offset, 8 * n_out, hipMemcpyDeviceToDevice, c->stream));
      RC_TRY(ws.ev.record(c, 3));
      HIP_TRY(hipStreamSynchronize(c->stream));
      o.n_candidates = n_cand;
      o.plan_taken = full ? HMJ_TOPK_FULL : HMJ_TOPK_SELECT;
      o.n_rounds = oo.n_rounds;
      if (c->profiling) {
        o.ms_select = ws.ev.ms(0, 1);
        o.ms_emit = ws.ev.ms(1, 2);
        o.ms_order = ws.ev.ms(2, 3);
      }
    }
  }
  opts_prefix_out(opts, o);
  return HMJ_OK;
}

}  // extern "C"
