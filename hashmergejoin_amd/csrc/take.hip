// Fixed-width columns taken through a row map (hmj_take_cols_device; include/hmj.h): what turns a join's r_row / s_row back
// into Arrow columns.  Nothing in the reference corresponds: its iterator hands out (key, rval, sval) triples
// (hashjoin.h:183-191) and knows no columns.  One kernel, in the idiom of coljoin.hip:
//   cols_take_kernel      one lane per output row, up to kTakeChunk columns per launch (descriptors by value, the column loop
//                         unrolled with a `c < k` guard like ColSide; instantiated for 1, 2, 4 and 8 columns).  The map
//                         entry is loaded once per row, one grid-stride step ahead, and tested once for all columns
//                         (HMJ_TAKE_NO_ROW, >= n_src); every gather of the row -- the value, and the validity
//                         byte where the column has a bitmap -- is issued before the first store.  A wave covers 64
//                         consecutive rows that start at a multiple of 64, so its ballot of "valid" IS one word of the output
//                         bitmap: one lane stores it (no atomics, no read-modify-write; lanes past n_out contribute the
//                         padding zeros).  Null counts per column, the HMJ_TAKE_NO_ROW entries and the out-of-range entries
//                         are ballot popcounts, summed over the four waves in LDS, one atomicAdd per workgroup and counter.
// The host checks the arguments (address ranges included), loops over chunks of kTakeChunk columns and reads the counters
// back once.  The call owns its TakeWs (hmj_ctx.h: the counters, two events) and touches nothing else of the ctx: no result
// column, no prepared build side, no plan, timing or memo.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdio>
#include <cstring>

#include "hmj_entry.h"

using hmj::u32;
using hmj::u64;
using namespace hmj_host;

namespace {

constexpr int TK_THREADS = 256;
constexpr int TK_WAVES = TK_THREADS / 64;
constexpr int kTakeChunk = 8;  // columns per launch
constexpr u64 kNoRow = HMJ_TAKE_NO_ROW;
// TakeWs::acc slots (u64): [0] map entries equal to HMJ_TAKE_NO_ROW, [1] map entries >= n_src that are not, [2 + c] NULL slots
// of output column c (all columns of the call: one read-back)
enum { TA_NO_ROW = 0, TA_BAD, TA_NULLS = 2, TA_N = TA_NULLS + HMJ_MAX_TAKE_COLS };

// One chunk of columns, passed to the kernel by value.  Every loop over the columns is fully unrolled with a `c < k` guard,
// so the members are read from the kernel arguments at constant offsets.
struct TakeCols {
  const void* src[kTakeChunk];
  const unsigned char* vbits[kTakeChunk];  // NULL: the source column holds no NULL
  u64 voff[kTakeChunk];
  void* dst[kTakeChunk];
  u64* dval[kTakeChunk];  // NULL: no output bitmap wanted
  u32 w[kTakeChunk];
  u32 k;
};

// Grid-stride over waves: gridDim.x * TK_THREADS is a multiple of 256, so `base` (the wave's first row) stays a multiple
// of 64 and the loop condition is wave-uniform -- every ballot below is taken with all 64 lanes active.  count_map: this
// launch counts the map's HMJ_TAKE_NO_ROW and out-of-range entries (the first chunk of a call only).  An entry >= n_src is
// compared before anything is loaded through it: its lane loads nothing and writes a NULL slot.
// K (1, 2, 4 or kTakeChunk): the columns the body is unrolled for, T.k <= K.  The registers a lane holds grow with K (two
// 64-bit values, a flag and a counter per column), so a call of one or two columns runs at twice the occupancy of the
// 8-column body.  The next step's map entry is loaded before this step's gathers: the one load whose address is known
// ahead does not sit in the dependent chain map -> gather -> store.
template <int K>
__global__ __launch_bounds__(TK_THREADS) void cols_take_kernel(TakeCols T, const u64* __restrict__ row_map, u64 n_out, u64 n_src,
                                                               u64* __restrict__ acc, u64* __restrict__ acc_nulls, int count_map) {
  __shared__ u32 red[TK_WAVES][kTakeChunk + 2];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  u32 nulls[K];  // (wave-uniform: popcounts)
#pragma unroll
  for (int c = 0; c < K; c++) nulls[c] = 0;
  u32 n_no = 0, n_bad = 0;
  const u64 stride = (u64)gridDim.x * TK_THREADS;
  u64 base = (u64)blockIdx.x * TK_THREADS + (u64)(wv * 64);
  u64 r_next = base + (u64)lane < n_out ? row_map[base + (u64)lane] : kNoRow;
  for (; base < n_out; base += stride) {
    const u64 i = base + (u64)lane;
    const bool in = i < n_out;
    const u64 r = r_next;  // (kNoRow past n_out)
    r_next = i + stride < n_out ? row_map[i + stride] : kNoRow;
    const bool have = r < n_src;  // (n_src <= 2^32-1: never HMJ_TAKE_NO_ROW)
    u64 lo[K], hi[K];
    bool ok[K];
#pragma unroll
    for (int c = 0; c < K; c++) {  // every gather of the row
      lo[c] = 0;
      hi[c] = 0;
      ok[c] = have;
      if (c < (int)T.k && have) {
        switch (T.w[c]) {  // (uniform)
          case 1: lo[c] = (u64) reinterpret_cast<const unsigned char*>(T.src[c])[r]; break;
          case 2: lo[c] = (u64) reinterpret_cast<const unsigned short*>(T.src[c])[r]; break;
          case 4: lo[c] = (u64) reinterpret_cast<const u32*>(T.src[c])[r]; break;
          case 8: lo[c] = reinterpret_cast<const u64*>(T.src[c])[r]; break;
          default: {
            const ulonglong2 t = reinterpret_cast<const ulonglong2*>(T.src[c])[r];
            lo[c] = t.x;
            hi[c] = t.y;
          }
        }
        if (T.vbits[c]) {  // (uniform)
          ok[c] = hmj::valid_bit(T.vbits[c], T.voff[c] + r);
        }
      }
    }
    const u32 n_in = (u32)__builtin_popcountll(__ballot(in));
#pragma unroll
    for (int c = 0; c < K; c++) {  // the stores
      if (c < (int)T.k) {
        const u64 m = __ballot(ok[c]);
        if (in) {
          const u64 a = ok[c] ? lo[c] : 0ull, b = ok[c] ? hi[c] : 0ull;  // the bytes of a NULL slot are 0
          switch (T.w[c]) {
            case 1: reinterpret_cast<unsigned char*>(T.dst[c])[i] = (unsigned char)a; break;
            case 2: reinterpret_cast<unsigned short*>(T.dst[c])[i] = (unsigned short)a; break;
            case 4: reinterpret_cast<u32*>(T.dst[c])[i] = (u32)a; break;
            case 8: reinterpret_cast<u64*>(T.dst[c])[i] = a; break;
            default: reinterpret_cast<ulonglong2*>(T.dst[c])[i] = make_ulonglong2(a, b);
          }
        }
        if (T.dval[c] && lane == 0) T.dval[c][base >> 6] = m;
        nulls[c] += n_in - (u32)__builtin_popcountll(m);
      }
    }
    if (count_map) {  // (uniform)
      n_no += (u32)__builtin_popcountll(__ballot(in && r == kNoRow));
      n_bad += (u32)__builtin_popcountll(__ballot(in && !have && r != kNoRow));
    }
  }
  if (lane == 0) {
#pragma unroll
    for (int c = 0; c < kTakeChunk; c++) red[wv][c] = 0;
#pragma unroll
    for (int c = 0; c < K; c++) red[wv][c] = nulls[c];
    red[wv][kTakeChunk] = n_no;
    red[wv][kTakeChunk + 1] = n_bad;
  }
  __syncthreads();
  if (threadIdx.x < kTakeChunk + 2) {
    u64 t = 0;
    for (int k = 0; k < TK_WAVES; k++) t += red[k][threadIdx.x];
    if (t) {
      if (threadIdx.x < kTakeChunk) atomicAdd(&acc_nulls[threadIdx.x], t);
      else atomicAdd(&acc[threadIdx.x == kTakeChunk ? TA_NO_ROW : TA_BAD], t);
    }
  }
}

// ---- host side -----------------------------------------------------------------------------------------------------------
int check_take_args(hmj_ctx* c, const hmj_take_src* src, u32 n_cols, u64 n_src, const u64* row_map, u64 n_out, const hmj_take_dst* dst,
                    const hmj_take_opts* opts) {
  char msg[192];
  if (!src || !dst || !opts) return fail(c, HMJ_E_ARG, "hmj_take_cols_device: src / dst / opts is NULL");
  if (opts->struct_size < offsetof(hmj_take_opts, reserved) + sizeof(opts->reserved))
    return fail(c, HMJ_E_ARG, "hmj_take_opts.struct_size too small");
  if (opts->reserved) return fail(c, HMJ_E_ARG, "hmj_take_opts: reserved must be 0");
  if (n_cols < 1 || n_cols > HMJ_MAX_TAKE_COLS) {
    std::snprintf(msg, sizeof(msg), "hmj_take_cols_device: n_cols must be in 1..%d", HMJ_MAX_TAKE_COLS);
    return fail(c, HMJ_E_ARG, msg);
  }
  if (n_out > 0xFFFFFFFFull || n_src > 0xFFFFFFFFull) return fail(c, HMJ_E_ARG, "hmj_take_cols_device: too many rows (at most 2^32-1)");
  if (n_out > 0 && !row_map) return fail(c, HMJ_E_ARG, "hmj_take_cols_device: row_map is NULL");
  if ((uintptr_t)row_map & 7u) return fail(c, HMJ_E_ARG, "hmj_take_cols_device: row_map is not aligned to 8 bytes");
  for (u32 k = 0; k < n_cols; k++) {
    const hmj_take_src& s = src[k];
    const hmj_take_dst& d = dst[k];
    const u32 w = s.width;
    if (w != 1 && w != 2 && w != 4 && w != 8 && w != 16) {
      std::snprintf(msg, sizeof(msg), "hmj_take_cols_device: column %u has width %u (1, 2, 4, 8 or 16)", k, w);
      return fail(c, HMJ_E_ARG, msg);
    }
    if (s.reserved) {
      std::snprintf(msg, sizeof(msg), "hmj_take_cols_device: column %u: reserved must be 0", k);
      return fail(c, HMJ_E_ARG, msg);
    }
    if (n_src > 0 && !s.data) {
      std::snprintf(msg, sizeof(msg), "hmj_take_cols_device: column %u: source data is NULL", k);
      return fail(c, HMJ_E_ARG, msg);
    }
    if (n_src > 0 && ((uintptr_t)s.data & (uintptr_t)(w - 1))) {
      std::snprintf(msg, sizeof(msg), "hmj_take_cols_device: column %u: source data is not aligned to its width (%u)", k, w);
      return fail(c, HMJ_E_ARG, msg);
    }
    if (validity_overflows(s.validity, n_src)) {
      std::snprintf(msg, sizeof(msg), "hmj_take_cols_device: column %u: validity bit_offset + n_src overflows 64 bits", k);
      return fail(c, HMJ_E_ARG, msg);
    }
    if (n_out > 0 && !d.data) {
      std::snprintf(msg, sizeof(msg), "hmj_take_cols_device: column %u: destination data is NULL", k);
      return fail(c, HMJ_E_ARG, msg);
    }
    if (n_out > 0 && ((uintptr_t)d.data & (uintptr_t)(w - 1))) {
      std::snprintf(msg, sizeof(msg), "hmj_take_cols_device: column %u: destination data is not aligned to its width (%u)", k, w);
      return fail(c, HMJ_E_ARG, msg);
    }
    if ((uintptr_t)d.validity & 7u) {
      std::snprintf(msg, sizeof(msg), "hmj_take_cols_device: column %u: destination validity is not aligned to 8 bytes", k);
      return fail(c, HMJ_E_ARG, msg);
    }
  }
  // A destination the kernel writes must not be something it reads: the map, or any source column or source bitmap of the
  // call (a later chunk's source included).  Address ranges only; n_out == 0 writes nothing.
  if (n_out == 0) return HMJ_OK;
  Range in[1 + 2 * HMJ_MAX_TAKE_COLS] = {range_of(row_map, 8 * n_out)};
  for (u32 j = 0; j < n_cols; j++) {
    in[1 + 2 * j] = range_of(src[j].data, n_src * src[j].width);
    in[2 + 2 * j] = validity_range(src[j].validity, n_src);
  }
  for (u32 k = 0; k < n_cols; k++) {
    const Range out[2] = {range_of(dst[k].data, n_out * src[k].width), range_of(dst[k].validity, 8 * ((n_out + 63) / 64))};
    if (first_overlap(out, 2, in, 1 + 2 * (int)n_cols)) {
      std::snprintf(msg, sizeof(msg), "hmj_take_cols_device: column %u: the destination overlaps the row map or a source column", k);
      return fail(c, HMJ_E_ARG, msg);
    }
  }
  return HMJ_OK;
}

int take_cols(hmj_ctx* c, const hmj_take_src* src, u32 n_cols, u64 n_src, const u64* row_map, u64 n_out, hmj_take_dst* dst,
              hmj_take_opts* o) {
  TakeWs& ws = c->take_ws;
  RC_TRY(ensure_dev(c, ws.acc, TA_N * sizeof(u64)));
  u64* acc = (u64*)ws.acc.p;
  HIP_TRY(hipMemsetAsync(acc, 0, TA_N * sizeof(u64), c->stream));
  RC_TRY(ws.ev.record(c, 0));
  const u64 need = (n_out + TK_THREADS - 1) / TK_THREADS, most = (u64)c->num_cus * 16;
  const dim3 grid((u32)(need < most ? need : most));
  for (u32 k0 = 0; k0 < n_cols; k0 += kTakeChunk) {
    TakeCols T;
    std::memset(&T, 0, sizeof(T));
    T.k = n_cols - k0 < (u32)kTakeChunk ? n_cols - k0 : (u32)kTakeChunk;
    for (u32 k = 0; k < T.k; k++) {
      const hmj_take_src& s = src[k0 + k];
      T.src[k] = s.data;
      T.vbits[k] = (const unsigned char*)s.validity.bits;
      T.voff[k] = s.validity.bit_offset;
      T.dst[k] = dst[k0 + k].data;
      T.dval[k] = (u64*)dst[k0 + k].validity;
      T.w[k] = s.width;
    }
    u64* acc_nulls = acc + TA_NULLS + k0;
    const int count_map = k0 == 0 ? 1 : 0;
    if (T.k <= 1)
      hipLaunchKernelGGL(cols_take_kernel<1>, grid, dim3(TK_THREADS), 0, c->stream, T, row_map, n_out, n_src, acc, acc_nulls, count_map);
    else if (T.k <= 2)
      hipLaunchKernelGGL(cols_take_kernel<2>, grid, dim3(TK_THREADS), 0, c->stream, T, row_map, n_out, n_src, acc, acc_nulls, count_map);
    else if (T.k <= 4)
      hipLaunchKernelGGL(cols_take_kernel<4>, grid, dim3(TK_THREADS), 0, c->stream, T, row_map, n_out, n_src, acc, acc_nulls, count_map);
    else
      hipLaunchKernelGGL(cols_take_kernel<kTakeChunk>, grid, dim3(TK_THREADS), 0, c->stream, T, row_map, n_out, n_src, acc, acc_nulls,
                         count_map);
    HIP_TRY(hipGetLastError());
  }
  RC_TRY(ws.ev.record(c, 1));
  u64 h[TA_N];
  RC_TRY(read_back(c, acc, h, sizeof(h)));
  if (h[TA_BAD]) {
    char msg[192];
    std::snprintf(msg, sizeof(msg), "hmj_take_cols_device: %llu row_map entries are >= n_src (%llu) and not HMJ_TAKE_NO_ROW", h[TA_BAD],
                  n_src);
    return fail(c, HMJ_E_ARG, msg);
  }
  for (u32 k = 0; k < n_cols; k++) dst[k].null_count = h[TA_NULLS + k];
  o->n_no_row = h[TA_NO_ROW];
  if (c->profiling) o->ms_take = ws.ev.ms(0, 1);
  return HMJ_OK;
}

}  // namespace

extern "C" {

int hmj_take_cols_device(hmj_ctx* c, const hmj_take_src* src, uint32_t n_cols, uint64_t n_src, const uint64_t* row_map, uint64_t n_out,
                         hmj_take_dst* dst, hmj_take_opts* opts) {
  if (!c) return HMJ_E_ARG;
  RC_TRY(check_take_args(c, src, n_cols, n_src, (const u64*)row_map, n_out, dst, opts));
  // the out fields of opts go to a full-size copy first; the caller gets the prefix its struct_size holds
  hmj_take_opts o;
  opts_prefix_in(&o, opts);
  opts_clear_out(&o, opts, offsetof(hmj_take_opts, n_no_row));
  if (n_out == 0) {
    for (u32 k = 0; k < n_cols; k++) dst[k].null_count = 0;
  } else {
    HIP_TRY(hipSetDevice(c->device));
    RC_TRY(take_cols(c, src, n_cols, n_src, (const u64*)row_map, n_out, dst, &o));
  }
  opts_prefix_out(opts, o);
  return HMJ_OK;
}

}  // extern "C"
