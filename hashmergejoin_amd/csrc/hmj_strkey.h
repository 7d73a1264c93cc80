// What the string-key join (strjoin.hip) and the mixed-key join (mixjoin.hip) share on key BYTES: the aligned reader, its
// two loaders, libstdc++'s _Hash_bytes and the comparison of two byte strings.  Internal header, included after
// hmj_keyjoin.h; its contents are local to the file that includes it.
#pragma once
#include "hmj_keyjoin.h"

namespace {

constexpr u64 kMul = 0xc6a4a7935bd1e995ull;
constexpr u64 kSeed = 0xc70f6907ull;
__device__ __forceinline__ u64 shift_mix(u64 v) { return v ^ (v >> 47); }

// Reads the key bytes at byte position `pos` as little-endian 64-bit words through aligned 8-byte loads (word q = bytes
// [8q, 8q + 8) of the address space the loader LD sees).  A load never reaches beyond the 8-byte-aligned words that
// hold key bytes, so no load crosses into a page the key does not touch.
template <class LD>
struct KeyReader {
  LD ld;
  u64 q;     // aligned word holding the next byte
  u32 s;     // bit offset of the next byte in that word
  u64 cur;   // word q (valid when it holds key bytes)
  u64 left;  // key bytes not yet read
  __device__ __forceinline__ KeyReader(LD l, u64 pos, u64 len) : ld(l), q(pos >> 3), s((u32)(pos & 7) * 8u), cur(0), left(len) {
    if (len) cur = ld(q);
  }
  // the next 8 bytes (left >= 8)
  __device__ __forceinline__ u64 word() {
    u64 d;
    left -= 8;
    if (s == 0) {
      d = cur;
      q++;
      if (left) cur = ld(q);
    } else {
      const u64 nx = ld(q + 1);
      d = (cur >> s) | (nx << (64 - s));
      cur = nx;
      q++;
    }
    return d;
  }
  // the last 1..7 bytes (left < 8), zero-extended
  __device__ __forceinline__ u64 tail() {
    const u32 t = (u32)left;
    u64 d = cur >> s;
    if (s + 8u * t > 64u) d |= ld(q + 1) << (64 - s);
    left = 0;
    return d & ((1ull << (8u * t)) - 1ull);
  }
};
struct GlobalLd {
  __device__ __forceinline__ u64 operator()(u64 q) const { return *reinterpret_cast<const u64*>(q << 3); }
};
struct LdsLd {
  const u64* w;
  __device__ __forceinline__ u64 operator()(u64 q) const { return w[q]; }
};

// libstdc++ _Hash_bytes (64-bit size_t), i.e. std::hash<std::string>
template <class LD>
__device__ __forceinline__ u64 hash_bytes(LD ld, u64 pos, u64 len) {
  KeyReader<LD> rd(ld, pos, len);
  u64 h = kSeed ^ (len * kMul);
  for (u64 k = len >> 3; k; k--) {
    const u64 d = shift_mix(rd.word() * kMul) * kMul;
    h = (h ^ d) * kMul;
  }
  if (len & 7) h = (h ^ rd.tail()) * kMul;
  return shift_mix(shift_mix(h) * kMul);
}

// Lexicographic comparison of two byte strings (a: la bytes, b: lb bytes) as std::string::operator< compares them
// (unsigned bytes, then length).
__device__ __forceinline__ int bytes_cmp(const unsigned char* a, u64 la, const unsigned char* b, u64 lb) {
  const u64 m = la < lb ? la : lb;
  KeyReader<GlobalLd> X(GlobalLd{}, (u64)(uintptr_t)a, m), Y(GlobalLd{}, (u64)(uintptr_t)b, m);
  while (X.left) {
    const u64 x = X.left >= 8 ? X.word() : X.tail();
    const u64 y = Y.left >= 8 ? Y.word() : Y.tail();
    if (x != y) {
      const u32 sh = (u32)__builtin_ctzll(x ^ y) & ~7u;
      return ((x >> sh) & 0xFF) < ((y >> sh) & 0xFF) ? -1 : 1;
    }
  }
  return la < lb ? -1 : la > lb ? 1 : 0;
}

}  // namespace
