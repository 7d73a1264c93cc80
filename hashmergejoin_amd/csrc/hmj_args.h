// Pure host helpers of the entries' argument checks and of their size-versioned opts: address ranges, Arrow validity
// bitmaps' byte spans, the width of a HMJ_TYPE_*, and the prefix copies between a caller's opts and the library's full-size
// copy.  No HIP call and no hmj_ctx: the header compiles with a plain C++ compiler (tests/cpp/test_entry_args.cc runs it
// under sanitizers).  Internal header.
#pragma once
#include <cstdint>
#include <cstring>

#include "../../include/hmj.h"

#ifdef __HIPCC__
#define HMJ_ARGS_FN __host__ __device__ __forceinline__
#else
#define HMJ_ARGS_FN inline
#endif

namespace hmj_host {

// bytes of a value of a fixed HMJ_TYPE_* (I8 .. I64, U8 .. U64, F32, F64)
HMJ_ARGS_FN uint32_t width_of(uint32_t type) { return type >= HMJ_TYPE_F32 ? 4u << (type - HMJ_TYPE_F32) : 1u << (type & 3u); }

// address ranges, for the host checks of the entries that write caller-owned columns
struct Range {
  uintptr_t lo, hi;  // [lo, hi); empty when lo == hi
};
inline Range range_of(const void* p, uint64_t bytes) { return Range{(uintptr_t)p, (uintptr_t)p + (uintptr_t)(p ? bytes : 0)}; }
inline bool overlap(const Range& a, const Range& b) { return a.lo < a.hi && b.lo < b.hi && a.lo < b.hi && b.lo < a.hi; }

// the bytes of a bitmap that hold the bits of rows 0 .. n - 1; empty without a bitmap or without rows
inline Range validity_range(const hmj_validity& v, uint64_t n) {
  if (!v.bits || n == 0) return Range{0, 0};
  return range_of((const unsigned char*)v.bits + (v.bit_offset >> 3), ((v.bit_offset & 7) + n + 7) / 8);
}
// bit_offset + n does not fit 64 bits (a column without a bitmap has no offset to overflow)
inline bool validity_overflows(const hmj_validity& v, uint64_t n) { return v.bits && v.bit_offset > UINT64_MAX - n; }

// The first pair (outs[out], ins[in]) that overlaps, in the order out-major; out < 0: none.  A range is not compared with
// itself, so the outputs of a call can be checked against each other: first_overlap(outs, n, outs, n).  The entry makes its
// own message of the pair.
struct OverlapHit {
  int out, in;
  explicit operator bool() const { return out >= 0; }
};
inline OverlapHit first_overlap(const Range* outs, int n_outs, const Range* ins, int n_ins) {
  for (int a = 0; a < n_outs; a++)
    for (int b = 0; b < n_ins; b++)
      if (&outs[a] != &ins[b] && overlap(outs[a], ins[b])) return OverlapHit{a, b};
  return OverlapHit{-1, -1};
}

// ---- size-versioned opts -------------------------------------------------------------------------------------------------
// Every opts struct T starts with uint32_t struct_size, the sizeof(T) of the caller's header.  An entry works on a full-size
// copy and hands back the prefix the caller's struct holds; no byte at or behind min(struct_size, sizeof(T)) of the
// caller's struct is read or written.
template <class T>
inline size_t opts_room(const T* caller) {
  return caller->struct_size < sizeof(T) ? caller->struct_size : sizeof(T);
}
// full: zeros, then the caller's prefix
template <class T>
inline void opts_prefix_in(T* full, const T* caller) {
  std::memset(full, 0, sizeof(T));
  std::memcpy(full, caller, opts_room(caller));
}
// The out fields of the full-size copy are cleared: every byte from first_out on.  In fields that lie behind out fields --
// bytes [in_lo, in_hi), the validity arrays a later header version appended -- are the caller's again, as far as its
// struct_size holds them.
template <class T>
inline void opts_clear_out(T* full, const T* caller, size_t first_out, size_t in_lo = 0, size_t in_hi = 0) {
  std::memset((char*)full + first_out, 0, sizeof(T) - first_out);
  const size_t have = caller->struct_size < in_hi ? caller->struct_size : in_hi;
  if (have > in_lo) std::memcpy((char*)full + in_lo, (const char*)caller + in_lo, have - in_lo);
}
// the caller gets the prefix its struct_size holds; its struct_size stays what it was
template <class T>
inline void opts_prefix_out(T* caller, const T& full) {
  const uint32_t size = caller->struct_size;
  std::memcpy(caller, &full, opts_room(caller));
  caller->struct_size = size;
}

}  // namespace hmj_host
