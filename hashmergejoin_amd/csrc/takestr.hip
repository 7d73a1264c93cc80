// One Arrow large_string / large_binary column taken through a row map (hmj_take_str_device; include/hmj.h): the sibling of
// take.hip for variable-width values -- what turns a string join's r_row / s_row back into its key strings.  Nothing in the
// reference corresponds (its iterator hands out (key, rval, sval) triples, hashjoin.h:183-191).  Two phases, three kernels:
//   str_take_offsets_kernel   one lane per output row, one workgroup per 256 consecutive rows (no grid-stride: the workgroup
//                             number is the index of its total).  The lane loads the map entry and tests it once
//                             (HMJ_TAKE_NO_ROW, >= n_src), gathers offsets[r], offsets[r + 1] and the validity byte together,
//                             and checks the row (decreasing offsets, an end behind chars_bytes) before its length counts.  A
//                             wave covers 64 rows that start at a multiple of 64: its ballot of "valid" is one bitmap word,
//                             the counts are ballot popcounts (one atomicAdd per workgroup and counter).  The workgroup's
//                             exclusive scan of the lengths goes to dst->offsets, its total to TakeStrWs::blk.
//   (hmj::launch_scan_u64 over the totals, as hmj_keyjoin.h places its per-workgroup counts)
//   str_take_place_kernel     streaming: adds every workgroup's base to its 256 offsets, writes offsets[n_out] and the total.
//   -- the host reads the counters back: a bad call stops here, a sizing call is complete --
//   str_take_bytes_kernel     balanced by output BYTES: a workgroup owns a tile of kTileBytes output bytes, finds the rows
//                             that intersect it by binary search in the final offsets and stages their output starts and
//                             source starts in LDS (up to kStageRows rows; beyond, lanes read both from global memory).  A
//                             lane produces one aligned 16-byte piece: for every run of the piece inside one row it reads
//                             the source bytes as one or two ALIGNED 16-byte granules (only granules that hold a byte of
//                             the row), shifts them into place and ORs them into the piece, which leaves in one 16-byte
//                             store.  The column's last piece is stored bytewise when it is short, so nothing at or behind
//                             total_bytes is written.
// The call owns its TakeStrWs (hmj_ctx.h: two DevBufs, four events) and touches nothing else of the ctx.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdio>
#include <cstring>

#include "hmj_entry.h"

using hmj::u32;
using hmj::u64;
using namespace hmj_host;

namespace {

typedef unsigned __int128 u128;
typedef unsigned char u8;

constexpr int TS_THREADS = 256;
constexpr int TS_WAVES = TS_THREADS / 64;
constexpr u32 kTileBytes = TS_THREADS * 16;  // output bytes per workgroup of the bytes phase: one 16-byte piece per lane
constexpr u32 kStageRows = 1024;             // rows of a tile whose starts are staged in LDS (16 KiB)
constexpr u64 kNoRow = HMJ_TAKE_NO_ROW;
// TakeStrWs::acc slots (u64).  The first TS_N_RED are ballot popcounts of the offsets phase: map entries equal to
// HMJ_TAKE_NO_ROW, map entries >= n_src that are not, taken valid rows whose offsets decrease / end behind chars_bytes, NULL
// output slots; TS_TOTAL is offsets[n_out].
enum { TS_NO_ROW = 0, TS_BAD_MAP, TS_BAD_DEC, TS_BAD_END, TS_NULLS, TS_N_RED, TS_TOTAL = TS_N_RED, TS_N };

// ---- offsets phase ---------------------------------------------------------------------------------------------------------
// Workgroup b covers rows [256 b, 256 b + 256); every ballot is taken with all 64 lanes active (lanes past n_out contribute
// the padding zeros).  A map entry is compared with n_src before anything is loaded through it, and the two offsets are
// compared with each other and with chars_bytes before a length is formed from them: a bad lane writes a NULL slot of length
// 0.  The offsets under a NULL source slot are loaded with the validity byte (one round trip, not two) and not looked at.
__global__ __launch_bounds__(TS_THREADS) void str_take_offsets_kernel(const u64* __restrict__ offsets, u64 chars_bytes,
                                                                      const u8* __restrict__ vbits, u64 voff,
                                                                      const u64* __restrict__ row_map, u64 n_out, u64 n_src,
                                                                      u64* __restrict__ out_off, u64* __restrict__ out_val,
                                                                      u64* __restrict__ blk_tot, u64* __restrict__ acc) {
  __shared__ u64 wtot[TS_WAVES];
  __shared__ u32 red[TS_WAVES][TS_N_RED];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const u64 i = (u64)blockIdx.x * TS_THREADS + threadIdx.x;
  const bool in = i < n_out;
  const u64 r = in ? row_map[i] : kNoRow;
  const bool have = r < n_src;  // (n_src <= 2^32-1: never HMJ_TAKE_NO_ROW)
  u64 b = 0, e = 0;
  bool ok = have;
  if (have) {
    b = offsets[r];
    e = offsets[r + 1];
    if (vbits) ok = hmj::valid_bit(vbits, voff + r);  // (uniform)
  }
  const bool dec = ok && e < b, end = ok && !dec && e > chars_bytes;
  ok = ok && !dec && !end;
  const u64 len = ok ? e - b : 0ull;
  const u64 incl = hmj::wave_incl_scan_u64(len, lane);
  const u64 m = __ballot(ok);
  const u32 n_no = (u32)__builtin_popcountll(__ballot(in && r == kNoRow));
  const u32 n_map = (u32)__builtin_popcountll(__ballot(in && !have && r != kNoRow));
  const u32 n_dec = (u32)__builtin_popcountll(__ballot(dec));
  const u32 n_end = (u32)__builtin_popcountll(__ballot(end));
  const u32 n_in = (u32)__builtin_popcountll(__ballot(in));
  if (lane == 0) {
    if (out_val && in) out_val[i >> 6] = m;
    red[wv][TS_NO_ROW] = n_no;
    red[wv][TS_BAD_MAP] = n_map;
    red[wv][TS_BAD_DEC] = n_dec;
    red[wv][TS_BAD_END] = n_end;
    red[wv][TS_NULLS] = n_in - (u32)__builtin_popcountll(m);
  }
  if (lane == 63) wtot[wv] = incl;
  __syncthreads();
  u64 carry = 0, all = 0;
#pragma unroll
  for (int k = 0; k < TS_WAVES; k++) {
    if (k < wv) carry += wtot[k];
    all += wtot[k];
  }
  if (in) out_off[i] = carry + incl - len;
  if (threadIdx.x == 0) blk_tot[blockIdx.x] = all;
  if (threadIdx.x < TS_N_RED) {
    u64 t = 0;
    for (int k = 0; k < TS_WAVES; k++) t += red[k][threadIdx.x];
    if (t) atomicAdd(&acc[threadIdx.x], t);
  }
}

// The same geometry: workgroup b adds blk_off[b] (the exclusive scan of the totals) to its 256 offsets.
__global__ __launch_bounds__(TS_THREADS) void str_take_place_kernel(u64* __restrict__ out_off, u64 n_out,
                                                                    const u64* __restrict__ blk_off, u32 nblk, u64* __restrict__ acc) {
  const u64 i = (u64)blockIdx.x * TS_THREADS + threadIdx.x;
  if (i < n_out) out_off[i] += blk_off[blockIdx.x];
  if (i == 0) {
    const u64 total = blk_off[nblk];
    out_off[n_out] = total;
    acc[TS_TOTAL] = total;
  }
}

// ---- bytes phase -----------------------------------------------------------------------------------------------------------
__device__ __forceinline__ u128 load_granule(const u8* p) {  // p aligned to 16
  const ulonglong2 t = *reinterpret_cast<const ulonglong2*>(p);
  return (u128)t.x | ((u128)t.y << 64);
}

// The n bytes (1..16) at `a`, any alignment, in the low bytes of the result, zeros above.  Reads the aligned granule that
// holds a[0] and, only when a[n - 1] lies in the next one, that one too: no granule without a byte of [a, a + n).
__device__ __forceinline__ u128 fetch_bytes(const u8* a, u32 n) {
  const u32 sh = (u32)((uintptr_t)a & 15u);
  const u8* base = a - sh;
  u128 v = load_granule(base) >> (8u * sh);
  if (sh + n > 16u) v |= load_granule(base + 16) << (8u * (16u - sh));  // (sh > 0 here)
  if (n < 16u) v &= ((u128)1 << (8u * n)) - 1;
  return v;
}

// The largest k in [l, h) with start(k) <= q; the caller guarantees start(l) <= q < start(h).
template <class F>
__device__ __forceinline__ u64 last_start_at_or_below(F start, u64 l, u64 h, u64 q) {
  while (h - l > 1) {
    const u64 mid = l + (h - l) / 2;
    if (start(mid) <= q) l = mid;
    else h = mid;
  }
  return l;
}

// Tile t = output bytes [t kTileBytes, min(+ kTileBytes, total)).  out_off: the n_out + 1 final output offsets (offsets[0]
// = 0, offsets[n_out] = total > 0, never decreasing).  A row with bytes is a valid taken row whose source offsets the
// offsets phase has checked: only such rows' map entries and source offsets are read here.
__global__ __launch_bounds__(TS_THREADS) void str_take_bytes_kernel(const u8* __restrict__ chars, const u64* __restrict__ src_off,
                                                                    const u64* __restrict__ row_map, const u64* __restrict__ out_off,
                                                                    u64 n_out, u64 total, u8* __restrict__ dst) {
  __shared__ u64 s_out[kStageRows + 1];
  __shared__ u64 s_src[kStageRows];
  __shared__ u64 s_edge[2];
  const u64 t0 = (u64)blockIdx.x * kTileBytes;
  const u64 t1 = t0 + kTileBytes < total ? t0 + kTileBytes : total;
  auto g_out = [&](u64 row) { return out_off[row]; };
  if (threadIdx.x == 0 || threadIdx.x == 64)  // the rows that hold the tile's first and last byte (two waves, side by side)
    s_edge[threadIdx.x >> 6] = last_start_at_or_below(g_out, 0, n_out, threadIdx.x == 0 ? t0 : t1 - 1);
  __syncthreads();
  const u64 lo = s_edge[0], cnt = s_edge[1] - lo + 1;  // rows lo .. lo + cnt - 1 intersect the tile (empty ones between them included)
  const bool staged = cnt <= kStageRows;               // (uniform)
  if (staged) {
    for (u32 k = threadIdx.x; k < (u32)cnt; k += TS_THREADS) {
      const u64 s = out_off[lo + k], e = out_off[lo + k + 1];
      s_out[k] = s;
      if (k + 1 == (u32)cnt) s_out[cnt] = e;
      s_src[k] = e > s ? src_off[row_map[lo + k]] : 0ull;
    }
    __syncthreads();
  }
  const u64 p = t0 + 16ull * threadIdx.x;  // this lane's piece
  if (p >= t1) return;
  const u32 n = t1 - p < 16 ? (u32)(t1 - p) : 16u;
  auto out_start = [&](u64 k) { return staged ? s_out[k] : out_off[lo + k]; };
  auto src_start = [&](u64 k) { return staged ? s_src[k] : src_off[row_map[lo + k]]; };
  u64 k = last_start_at_or_below(out_start, 0, cnt, p);  // the row of the piece's first byte
  u128 v = 0;
  u32 j = 0;
  for (;;) {
    const u64 q = p + j, s = out_start(k), e = out_start(k + 1);  // s <= q < e
    const u32 seg = e - q < (u64)(n - j) ? (u32)(e - q) : n - j;
    v |= fetch_bytes(chars + src_start(k) + (q - s), seg) << (8u * j);
    j += seg;
    if (j >= n) break;
    k++;  // the next row starts at p + j; where it is empty, search for the row that holds that byte
    if (out_start(k + 1) <= p + j) k = last_start_at_or_below(out_start, k, cnt, p + j);
  }
  if (n == 16u) {
    *reinterpret_cast<ulonglong2*>(dst + p) = make_ulonglong2((u64)v, (u64)(v >> 64));
  } else {  // the column's last piece: nothing at or behind total_bytes is written
    for (u32 t = 0; t < n; t++) dst[p + t] = (u8)(v >> (8u * t));
  }
}

// ---- host side -----------------------------------------------------------------------------------------------------------
int check_take_str_args(hmj_ctx* c, const hmj_take_str_src* src, u64 n_src, const u64* row_map, u64 n_out, const hmj_take_str_dst* dst,
                        const hmj_take_str_opts* opts) {
  if (!src || !dst || !opts) return fail(c, HMJ_E_ARG, "hmj_take_str_device: src / dst / opts is NULL");
  if (opts->struct_size < offsetof(hmj_take_str_opts, reserved) + sizeof(opts->reserved))
    return fail(c, HMJ_E_ARG, "hmj_take_str_opts.struct_size too small");
  if (opts->reserved) return fail(c, HMJ_E_ARG, "hmj_take_str_opts: reserved must be 0");
  if (n_out > 0xFFFFFFFFull || n_src > 0xFFFFFFFFull) return fail(c, HMJ_E_ARG, "hmj_take_str_device: too many rows (at most 2^32-1)");
  if (n_out > 0 && !row_map) return fail(c, HMJ_E_ARG, "hmj_take_str_device: row_map is NULL");
  if ((uintptr_t)row_map & 7u) return fail(c, HMJ_E_ARG, "hmj_take_str_device: row_map is not aligned to 8 bytes");
  if (n_src > 0 && !src->offsets) return fail(c, HMJ_E_ARG, "hmj_take_str_device: source offsets are NULL");
  if ((uintptr_t)src->offsets & 7u) return fail(c, HMJ_E_ARG, "hmj_take_str_device: source offsets are not aligned to 8 bytes");
  if (!src->chars && src->chars_bytes) return fail(c, HMJ_E_ARG, "hmj_take_str_device: source chars are NULL with chars_bytes > 0");
  if (validity_overflows(src->validity, n_src))
    return fail(c, HMJ_E_ARG, "hmj_take_str_device: validity bit_offset + n_src overflows 64 bits");
  if (n_out > 0 && !dst->offsets) return fail(c, HMJ_E_ARG, "hmj_take_str_device: destination offsets are NULL");
  if ((uintptr_t)dst->offsets & 7u) return fail(c, HMJ_E_ARG, "hmj_take_str_device: destination offsets are not aligned to 8 bytes");
  if ((uintptr_t)dst->validity & 7u) return fail(c, HMJ_E_ARG, "hmj_take_str_device: destination validity is not aligned to 8 bytes");
  if ((uintptr_t)dst->chars & 15u) return fail(c, HMJ_E_ARG, "hmj_take_str_device: destination chars are not aligned to 16 bytes");
  // A destination the kernels write must not be something they read, nor another destination.  Address ranges only;
  // n_out == 0 writes nothing.
  if (n_out == 0) return HMJ_OK;
  const Range in[4] = {range_of(row_map, 8 * n_out), range_of(src->offsets, 8 * (n_src + 1)), range_of(src->chars, src->chars_bytes),
                       validity_range(src->validity, n_src)};
  const Range out[3] = {range_of(dst->offsets, 8 * (n_out + 1)), range_of(dst->validity, 8 * ((n_out + 63) / 64)),
                        range_of(dst->chars, dst->chars_capacity)};
  for (int a = 0; a < 3; a++) {
    if (first_overlap(out + a, 1, in, 4))
      return fail(c, HMJ_E_ARG, "hmj_take_str_device: a destination overlaps the row map, the source offsets, chars or bitmap");
    if (first_overlap(out + a, 1, out + a + 1, 2 - a)) return fail(c, HMJ_E_ARG, "hmj_take_str_device: two destinations overlap");
  }
  return HMJ_OK;
}

int take_str(hmj_ctx* c, const hmj_take_str_src* src, u64 n_src, const u64* row_map, u64 n_out, hmj_take_str_dst* dst,
             hmj_take_str_opts* o) {
  const u32 nblk = (u32)((n_out + TS_THREADS - 1) / TS_THREADS);
  TakeStrWs& ws = c->takestr_ws;
  RC_TRY(ensure_dev(c, ws.acc, TS_N * sizeof(u64)));
  RC_TRY(ensure_dev(c, ws.blk, (2 * (size_t)nblk + 1) * sizeof(u64)));
  u64* acc = (u64*)ws.acc.p;
  u64* blk_tot = (u64*)ws.blk.p;
  u64* blk_off = blk_tot + nblk;  // nblk + 1
  const u64* src_off = (const u64*)src->offsets;
  u64* out_off = (u64*)dst->offsets;
  u64* out_val = (u64*)dst->validity;
  HIP_TRY(hipMemsetAsync(acc, 0, TS_N * sizeof(u64), c->stream));
  RC_TRY(ws.ev.record(c, 0));
  hipLaunchKernelGGL(str_take_offsets_kernel, dim3(nblk), dim3(TS_THREADS), 0, c->stream, src_off, src->chars_bytes,
                     (const u8*)src->validity.bits, src->validity.bit_offset, row_map, n_out, n_src, out_off, out_val, blk_tot,
                     acc);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hmj::launch_scan_u64(blk_tot, blk_off, nblk, c->stream));
  hipLaunchKernelGGL(str_take_place_kernel, dim3(nblk), dim3(TS_THREADS), 0, c->stream, out_off, n_out, blk_off, nblk, acc);
  HIP_TRY(hipGetLastError());
  RC_TRY(ws.ev.record(c, 1));
  // the one synchronisation before the bytes phase: a bad call stops here, a sizing call is complete
  u64 h[TS_N];
  RC_TRY(read_back(c, acc, h, sizeof(h)));
  char msg[224];
  if (h[TS_BAD_MAP]) {
    std::snprintf(msg, sizeof(msg), "hmj_take_str_device: %llu row_map entries are >= n_src (%llu) and not HMJ_TAKE_NO_ROW", h[TS_BAD_MAP],
                  n_src);
    return fail(c, HMJ_E_ARG, msg);
  }
  if (h[TS_BAD_DEC] || h[TS_BAD_END]) {
    std::snprintf(msg, sizeof(msg),
                  "hmj_take_str_device: %llu taken rows have bad source offsets (%llu with offsets[r + 1] < offsets[r], %llu that end "
                  "behind chars_bytes = %llu)",
                  h[TS_BAD_DEC] + h[TS_BAD_END], h[TS_BAD_DEC], h[TS_BAD_END], (u64)src->chars_bytes);
    return fail(c, HMJ_E_ARG, msg);
  }
  const u64 total = h[TS_TOTAL];
  dst->null_count = h[TS_NULLS];
  dst->total_bytes = total;
  o->n_no_row = h[TS_NO_ROW];
  if (c->profiling) o->ms_offsets = ws.ev.ms(0, 1);
  if (!dst->chars) return HMJ_OK;  // the sizing call
  if (dst->chars_capacity < total) {
    std::snprintf(msg, sizeof(msg), "hmj_take_str_device: chars_capacity (%llu) is smaller than total_bytes (%llu)",
                  (u64)dst->chars_capacity, total);
    return fail(c, HMJ_E_ARG, msg);
  }
  if (total == 0) return HMJ_OK;
  const u64 tiles = (total + kTileBytes - 1) / kTileBytes;
  if (tiles > 0x7FFFFFFFull) return fail(c, HMJ_E_ARG, "hmj_take_str_device: more output bytes than one launch covers (2^43)");
  RC_TRY(ws.ev.record(c, 2));
  hipLaunchKernelGGL(str_take_bytes_kernel, dim3((u32)tiles), dim3(TS_THREADS), 0, c->stream, (const u8*)src->chars, src_off, row_map,
                     out_off, n_out, total, (u8*)dst->chars);
  HIP_TRY(hipGetLastError());
  RC_TRY(ws.ev.record(c, 3));
  HIP_TRY(hipStreamSynchronize(c->stream));
  if (c->profiling) o->ms_chars = ws.ev.ms(2, 3);
  return HMJ_OK;
}

}  // namespace

extern "C" {

int hmj_take_str_device(hmj_ctx* c, const hmj_take_str_src* src, uint64_t n_src, const uint64_t* row_map, uint64_t n_out,
                        hmj_take_str_dst* dst, hmj_take_str_opts* opts) {
  if (!c) return HMJ_E_ARG;
  RC_TRY(check_take_str_args(c, src, n_src, (const u64*)row_map, n_out, dst, opts));
  // the out fields of opts go to a full-size copy first; the caller gets the prefix its struct_size holds
  hmj_take_str_opts o;
  opts_prefix_in(&o, opts);
  opts_clear_out(&o, opts, offsetof(hmj_take_str_opts, n_no_row));
  int rc = HMJ_OK;
  if (n_out == 0) {
    dst->null_count = 0;
    dst->total_bytes = 0;
  } else {
    HIP_TRY(hipSetDevice(c->device));
    rc = take_str(c, src, n_src, (const u64*)row_map, n_out, dst, &o);
  }
  if (rc == HMJ_OK) opts_prefix_out(opts, o);
  return rc;
}

}  // extern "C"
