// What hmj_order_by_device (orderby.hip) shares with hmj_top_k_device (topk.hip): the key columns as the kernels take them,
// the order-preserving byte stream of a row (stream_window), the words of its offsets' verdict, and the host functions of
// orderby.hip that the top-k entry calls -- the argument checks of the key columns, the whole ORDER BY of n rows, and the
// refinement loop over a list of {word, row} rows.  Both files compile the device functions.  Internal header.
#pragma once
#include <hip/hip_runtime.h>

#include "hmj_entry.h"

namespace hmj_order {

using hmj::u32;
using hmj::u64;
using hmj_host::width_of;

constexpr int OB_THREADS = 256;
constexpr int OB_WAVES = OB_THREADS / 64;
constexpr int kMaxCols = HMJ_MAX_ORDER_COLS;
constexpr u64 kNone = ~0ull;

// acc words: heads and tied rows of a round (cleared per round), the longest stream, and the report of the kernel that
// checks the offsets -- per column the first row whose offsets decrease (~0: none) and the waves that hold key bytes under
// chars == NULL
enum { OA_HEADS = 0, OA_TIED, OA_MAXLEN, OA_ERR, OA_NODATA = OA_ERR + kMaxCols, OA_N = OA_NODATA + kMaxCols };

// The key columns, passed to the kernels by value; every loop over them is fully unrolled with a `c < k` guard.
struct OrdCols {
  const void* p[kMaxCols];            // values, or a string column's chars
  const u64* off[kMaxCols];           // string columns: n + 1 offsets
  const unsigned char* vb[kMaxCols];  // NULL: the column holds no NULL
  u64 voff[kMaxCols];
  u32 type[kMaxCols], flags[kMaxCols];
  u32 k;
};

// A valid fixed-width value as an unsigned integer of its own width whose order is the type's: signed integers with the
// sign bit flipped; floats negative -> complement, else sign bit set, every NaN all ones (above +inf's key).
__device__ __forceinline__ u64 enc_fixed(const void* __restrict__ p, u32 type, u64 r) {
  const u32 w = width_of(type);
  u64 x;
  switch (w) {  // (uniform)
    case 1: x = reinterpret_cast<const unsigned char*>(p)[r]; break;
    case 2: x = reinterpret_cast<const unsigned short*>(p)[r]; break;
    case 4: x = reinterpret_cast<const u32*>(p)[r]; break;
    default: x = reinterpret_cast<const u64*>(p)[r];
  }
  if (type <= HMJ_TYPE_I64) return x ^ (1ull << (8u * w - 1u));
  if (type == HMJ_TYPE_F32) {
    const u32 b = (u32)x;
    if ((b & 0x7fffffffu) > 0x7f800000u) return 0xffffffffull;
    return (u64)((b >> 31) ? ~b : (b | 0x80000000u));
  }
  if (type == HMJ_TYPE_F64) {
    if ((x & ~(1ull << 63)) > 0x7ff0000000000000ull) return ~0ull;
    return (x >> 63) ? ~x : (x | (1ull << 63));
  }
  return x;
}

// Bytes [cursor, cursor + nb) of row r's stream, the first one in the top byte of the result, zeros behind the stream's
// end (nb <= 8; nb == 0: the length alone); len: the stream's length.  Per column: a marker byte when the column has a
// bitmap (the NULL side as flagged), then
//   fixed   the key of enc_fixed big-endian, complemented under HMJ_ORDER_DESC; zeros under a NULL slot (no load);
//   string  nothing under a NULL slot (no byte is read); else max(1, ceil(len / 7)) blocks of 7 data bytes, zero padded,
//           and a control byte -- 0xFF: the string continues, else the data bytes of this block, 0..7 -- all eight
//           complemented under HMJ_ORDER_DESC.  Prefix-free, and ordered as (bytes, then length): a shorter string meets
//           the longer one's 0xFF with its count, or its zero padding with equal data and a smaller count.
// CHECK (order_key_kernel, topk_hist_kernel's level 0; every lane of the wave calls, `active` says which hold a row): a
// string column's offsets are tested before a byte is read, a row that fails reads none and is reported in acc.
template <bool CHECK>
__device__ __forceinline__ u64 stream_window(const OrdCols& T, u64 r, bool active, u64 cursor, u32 nb, u64& len, u64* __restrict__ acc) {
  const int lane = threadIdx.x & 63;
  u64 pos = 0, out = 0;
  u32 cnt = 0;
#pragma unroll
  for (int c = 0; c < kMaxCols; c++) {
    if (c < (int)T.k) {  // (kernel arguments: uniform, like every test of T's type, flags and bitmap pointer)
      const u32 bm = T.vb[c] ? 1u : 0u;
      bool valid = active;
      if (bm && active) valid = hmj::valid_bit(T.vb[c], T.voff[c] + r);
      const u32 inv = (T.flags[c] & HMJ_ORDER_DESC) ? 0xFFu : 0u;
      const u32 marker = ((T.flags[c] & HMJ_ORDER_NULLS_FIRST) != 0) == valid ? 1u : 0u;
      u64 L;
      if (T.type[c] != HMJ_ORDER_LARGE_STRING) {
        const u32 w = width_of(T.type[c]);
        L = (u64)(bm + w);
        if (active && cnt < nb && cursor < pos + L) {
          const u64 x = valid ? enc_fixed(T.p[c], T.type[c], r) : 0ull;
          for (u32 j = cursor > pos ? (u32)(cursor - pos) : 0u; j < (u32)L && cnt < nb; j++) {
            u32 byte = marker;
            if (!bm || j) {
              byte = (u32)(x >> (8u * (w - 1u - (j - bm)))) & 0xFFu;
              if (valid) byte ^= inv;
            }
            out |= (u64)byte << (56u - 8u * cnt);
            cnt++;
          }
        }
      } else {
        const unsigned char* chars = (const unsigned char*)T.p[c];
        u64 o0 = 0, o1 = 0;
        if (active) {
          o0 = T.off[c][r];
          o1 = T.off[c][r + 1];
        }
        bool usable = true;
        if (CHECK) {
          const bool bad = active && o1 < o0;
          const u64 bad_mask = __ballot(bad);
          if (bad_mask && lane == (int)__builtin_ctzll(bad_mask)) atomicMin(&acc[OA_ERR + c], r);
          const bool nodata = valid && !bad && !chars && o1 > o0;  // (a NULL slot holds no key bytes, whatever its offsets span)
          const u64 nd_mask = __ballot(nodata);
          if (nd_mask && lane == (int)__builtin_ctzll(nd_mask)) atomicAdd(&acc[OA_NODATA + c], 1ull);
          usable = !bad && !nodata;
        }
        const u64 slen = usable && o1 > o0 ? o1 - o0 : 0ull;
        const u64 blocks = slen ? (slen + 6) / 7 : 1ull;
        L = (u64)bm + (valid ? 8ull * blocks : 0ull);
        if (active && cnt < nb && cursor < pos + L) {
          for (u64 j = cursor > pos ? cursor - pos : 0ull; j < L && cnt < nb; j++) {
            u32 byte = marker;
            if (!bm || j) {
              const u64 q = j - bm, blk = q >> 3;
              const u32 in = (u32)(q & 7);
              if (in < 7) {
                const u64 at = blk * 7 + in;
                byte = at < slen ? (u32)chars[o0 + at] : 0u;
              } else {
                byte = blk + 1 < blocks ? 0xFFu : (u32)(slen - blk * 7);
              }
              byte ^= inv;
            }
            out |= (u64)byte << (56u - 8u * cnt);
            cnt++;
          }
        }
      }
      pos += L;
    }
  }
  len = pos;
  return out;
}

// ---- host side: defined in orderby.hip -------------------------------------------------------------------------------------
// cols as the kernels take them; fixed_len: the length every stream has, 0 with a string column among them
void order_cols_of(const hmj_order_col* cols, u32 n_cols, OrdCols* T, u64* fixed_len);
// hmj_order_by_device's checks of n_cols, n, the map (map_entries of them; looked at with map_entries > 0) and every
// column, in that entry's order and wording
int order_check_cols(hmj_ctx* c, const hmj_order_col* cols, u32 n_cols, u64 n, const u64* map, u64 map_entries);
// the verdict on the offsets, read back into h[OA_N] behind the first kernel that computed a stream
int order_offsets_verdict(hmj_ctx* c, const u64* h);
// The whole ORDER BY of n >= 2 rows into map (n entries): the key kernel, its verdict, then order_refine_rows.
int order_rows(hmj_ctx* c, const OrdCols& T, u64 fixed_len, u64 n, u64* map, hmj_order_opts* o);
// The rounds.  OrderWs::rows holds m {first 8 stream bytes, row} rows, row ids below n_rows, in an order that keeps rows of
// equal streams in ascending row index; S: the longest stream.  map gets m entries, positions below m: the rows in order.
int order_refine_rows(hmj_ctx* c, const OrdCols& T, u64 fixed_len, u64 S, u64 n_rows, u64 m, u64* map, hmj_order_opts* o);

}  // namespace hmj_order
