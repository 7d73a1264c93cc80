// String-key join on the device (hmj_hash_str_device, hmj_join_str_device; include/hmj.h).  The reference joins
// std::string keys through the same operator template (hashjoin.h:29 KeyValVec, hashjoin_bench.cc:109-143): it orders
// rows by std::hash of the key and breaks ties on the key (radix_hash.h:86-109).  Here:
//   1. str_hash_kernel   libstdc++'s _Hash_bytes of every key -> {hash, row} rows (16 bytes, what the u64 join takes);
//                        a wave's 64 keys are one contiguous byte span, staged in LDS with 16-byte loads;
//   2. the u64 join      join_device on those rows, HMJ_MATERIALIZE (+ HMJ_ORDERED): pairs of equal hash (hash, r_row, s_row);
//   3. verify_kernel     one lane per pair: lengths, then bytes, 8 at a time; survivors compacted (stable) with their
//                        payloads, or only counted / summed in the count modes;
//   4. collision order   ordered joins only: runs of equal hash whose build keys differ are sorted by key bytes in one
//                        workgroup each (a run beyond kRunCap rows is HMJ_E_UNSUPPORTED).
// Steps 2 to 4 and everything the join kinds add to them -- rep_verify_kernel, the sweeps, the ordered kinds' sort and
// gather -- are hmj_tuplejoin.h's driver (tuple_join / tuple_join_kind) on hmj_keyjoin.h's kernels, shared with the
// multi-column and the mixed-key join and instantiated here on StrPolicy / StrSide; this file holds the hash kernels, the
// key policy (key_eq / key_cmp / payload on StrSide), StrPolicy (how the driver keys a relation and where the hash kernels
// report on its offsets) and the entries.  The byte reader, _Hash_bytes and the byte comparison are hmj_strkey.h's, shared
// with the mixed-key join (mixjoin.hip).
// NULL keys (validity bitmaps, calls that pass one only): the driver's valid_count_kernel counts the rows that have a key per
// workgroup, one scan places them, and str_hash_valid_kernel writes two arrays per relation: the dense rows the sweeps walk
// by row index (a NULL-key row: hash 0, row HMJ_STR_NO_ROW) and the compacted rows of the valid rows, which are all the u64
// joins see.  Row indices stay the caller's, so verification, marks and gathers are unchanged; ordered results emit the
// NULL-key rows into a tail behind the rows that are sorted (DESIGN.md "NULL keys on string keys").
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>

#include "hmj_tuplejoin.h"
#include "hmj_strkey.h"

namespace {

constexpr int SH_THREADS = 256;
constexpr int SH_WAVES = SH_THREADS / 64;
constexpr int SH_STAGE = 4096;  // LDS bytes a wave stages its 64 keys in; a longer span: per-lane reads from global memory
static_assert(SH_THREADS == KJ_THREADS, "valid_count_kernel counts the rows of one workgroup of str_hash_valid_kernel");

// Per wave: 64 consecutive keys, bytes [offsets[i0], offsets[i0 + 64]).  Staged in LDS when the span's aligned 16-byte
// blocks fit SH_STAGE, else read per lane from global memory.  rows: out = {hash, row} x n, else bare hashes.  vals != NULL: their sum goes to
// acc[KA_SUM_P] of the call's block.  err: the relation's report words -- err[KA_BAD_ROW]: its first row whose offsets decrease
// (preset ~0), err[KA_NULL_CHARS]: its waves that hold key bytes under chars == NULL.
__global__ __launch_bounds__(SH_THREADS) void str_hash_kernel(const unsigned char* __restrict__ chars, const u64* __restrict__ offsets,
                                                              u64 n, u32 hash_bits, u64* __restrict__ out, int rows,
                                                              const u64* __restrict__ vals, u64* __restrict__ acc,
                                                              u64* __restrict__ err) {
  __shared__ u64 stage[SH_WAVES][SH_STAGE / 8 + 2];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const u64 i0 = ((u64)blockIdx.x * SH_WAVES + (u64)w) * 64ull;
  const u64 i = i0 + (u64)lane;
  const bool active = i < n;
  const u64 iend = i0 + 64 < n ? i0 + 64 : n;
  u64 o0 = 0, o1 = 0, s0 = 0, s1 = 0;
  if (i0 < n) {
    const u64 a = offsets[active ? i : n];
    const u64 e = offsets[iend];
    const u64 nxt = __shfl_down(a, 1, 64);
    o0 = a;
    o1 = lane == 63 ? e : nxt;
    if (i + 1 == iend) o1 = e;
    s0 = __shfl(a, 0, 64);
    s1 = e;
  }
  const bool bad = active && o1 < o0;
  const u64 bad_mask = __ballot(bad);
  if (bad_mask && lane == (int)__builtin_ctzll(bad_mask)) atomicMin(&err[KA_BAD_ROW], i);
  const bool ok_wave = i0 < n && !bad_mask && s1 >= s0;
  if (ok_wave && !chars && s1 > s0 && lane == 0) atomicAdd(&err[KA_NULL_CHARS], 1ull);
  const bool usable = ok_wave && (chars || s1 == s0);
  // stage the wave's span: 16-byte aligned loads covering [chars + s0, chars + s1)
  const uintptr_t b0 = usable ? ((uintptr_t)(chars + s0) & ~(uintptr_t)15) : 0;
  const u64 span_bytes = usable && s1 > s0 ? (u64)(((uintptr_t)(chars + s1) + 15) & ~(uintptr_t)15) - (u64)b0 : 0;
  const bool staged = usable && span_bytes <= (u64)SH_STAGE;
  if (staged) {
    const uint4* src = reinterpret_cast<const uint4*>(b0);
    uint4* dst = reinterpret_cast<uint4*>(&stage[w][0]);
    for (u32 k = (u32)lane; k < (u32)(span_bytes >> 4); k += 64) dst[k] = src[k];
  }
  if (vals && i0 < n) {
    const u64 vs = hmj::wave_sum_u64(active ? vals[i] : 0ull);
    if (lane == 0) atomicAdd(&acc[KA_SUM_P], vs);
  }
  __syncthreads();
  if (!usable || !active) return;
  const u64 len = o1 - o0;
  u64 h;
  if (staged) {
    h = hash_bytes(LdsLd{&stage[w][0]}, (u64)((uintptr_t)(chars + o0) - b0), len);
  } else {
    h = hash_bytes(GlobalLd{}, (u64)(uintptr_t)(chars + o0), len);
  }
  h = fold_bits(h, hash_bits);
  if (rows) {
    reinterpret_cast<ulonglong2*>(out)[i] = make_ulonglong2(h, i);
  } else {
    out[i] = h;
  }
}

// ---- NULL keys (validity bitmaps) ------------------------------------------------------------------------------------------
// One relation's Arrow validity bitmap as the kernel below takes it (column 0 of the ColValid the entry builds and the
// driver's pass 1, valid_count_kernel, reads): row i has a key iff bit off + i (least-significant bit first) is set.
struct StrValid {
  const unsigned char* bits;
  u64 off;
};
__device__ __forceinline__ bool row_valid(const StrValid& V, u64 i) {
  const u64 b = V.off + i;
  return (V.bits[b >> 3] >> (b & 7)) & 1u;
}

// Pass 2, str_hash_kernel for a relation with a bitmap: the same wave spans, staging and offset checks (a NULL slot's
// offsets must not decrease either, and its bytes are staged with the span; a NULL lane hashes nothing).  dense (NULL: not
// wanted): row i gets {hash, i}, a NULL-key row {0, HMJ_STR_NO_ROW} -- what the sweeps walk by row index.  comp: the valid
// rows' {hash, i}, workgroup b's at blk_off[b] in row order (the wave's ballot places a lane inside its wave, the per-wave
// counts in LDS the wave inside its workgroup); cap: rows comp holds.  No lane leaves before the second barrier: a lane
// that is inactive, NULL or in a wave whose offsets are unusable only takes no part in the ballot's count.  Such a wave
// reports its row as str_hash_kernel does and compacts nothing, so the rows behind it land in front of their places --
// inside comp, and in a call that fails.
__global__ __launch_bounds__(SH_THREADS) void str_hash_valid_kernel(const unsigned char* __restrict__ chars, const u64* __restrict__ offsets,
                                                                    u64 n, u32 hash_bits, StrValid V, u64* __restrict__ dense,
                                                                    u64* __restrict__ comp, u64 cap, const u64* __restrict__ blk_off,
                                                                    const u64* __restrict__ vals, u64* __restrict__ acc,
                                                                    u64* __restrict__ err) {
  __shared__ u64 stage[SH_WAVES][SH_STAGE / 8 + 2];
  __shared__ u32 wcnt[SH_WAVES];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const u64 i0 = ((u64)blockIdx.x * SH_WAVES + (u64)w) * 64ull;
  const u64 i = i0 + (u64)lane;
  const bool active = i < n;
  const u64 iend = i0 + 64 < n ? i0 + 64 : n;
  u64 o0 = 0, o1 = 0, s0 = 0, s1 = 0;
  if (i0 < n) {
    const u64 a = offsets[active ? i : n];
    const u64 e = offsets[iend];
    const u64 nxt = __shfl_down(a, 1, 64);
    o0 = a;
    o1 = lane == 63 ? e : nxt;
    if (i + 1 == iend) o1 = e;
    s0 = __shfl(a, 0, 64);
    s1 = e;
  }
  const bool bad = active && o1 < o0;
  const u64 bad_mask = __ballot(bad);
  if (bad_mask && lane == (int)__builtin_ctzll(bad_mask)) atomicMin(&err[KA_BAD_ROW], i);
  const bool ok_wave = i0 < n && !bad_mask && s1 >= s0;
  if (ok_wave && !chars && s1 > s0 && lane == 0) atomicAdd(&err[KA_NULL_CHARS], 1ull);
  const bool usable = ok_wave && (chars || s1 == s0);
  const uintptr_t b0 = usable ? ((uintptr_t)(chars + s0) & ~(uintptr_t)15) : 0;
  const u64 span_bytes = usable && s1 > s0 ? (u64)(((uintptr_t)(chars + s1) + 15) & ~(uintptr_t)15) - (u64)b0 : 0;
  const bool staged = usable && span_bytes <= (u64)SH_STAGE;
  if (staged) {
    const uint4* src = reinterpret_cast<const uint4*>(b0);
    uint4* dst = reinterpret_cast<uint4*>(&stage[w][0]);
    for (u32 k = (u32)lane; k < (u32)(span_bytes >> 4); k += 64) dst[k] = src[k];
  }
  if (vals && i0 < n) {  // (every row's payload, NULL-key rows included)
    const u64 vs = hmj::wave_sum_u64(active ? vals[i] : 0ull);
    if (lane == 0) atomicAdd(&acc[KA_SUM_P], vs);
  }
  const bool ok = usable && active && row_valid(V, active ? i : 0);
  __syncthreads();
  u64 h = 0;
  if (ok) {
    const u64 len = o1 - o0;
    if (staged) {
      h = hash_bytes(LdsLd{&stage[w][0]}, (u64)((uintptr_t)(chars + o0) - b0), len);
    } else {
      h = hash_bytes(GlobalLd{}, (u64)(uintptr_t)(chars + o0), len);
    }
    h = fold_bits(h, hash_bits);
  }
  if (dense && active) reinterpret_cast<ulonglong2*>(dense)[i] = make_ulonglong2(h, ok ? i : kNoRow);
  const u64 m = __ballot(ok);
  if (lane == 0) wcnt[w] = (u32)__builtin_popcountll(m);
  __syncthreads();
  if (ok) {
    u64 pos = blk_off[blockIdx.x] + hmj::popc_below(m);
    for (int k = 0; k < w; k++) pos += wcnt[k];
    if (pos < cap) reinterpret_cast<ulonglong2*>(comp)[pos] = make_ulonglong2(h, i);
  }
}

// One relation as the shared kernels take it (hmj_keyjoin.h), with its key policy.
struct StrSide {
  const unsigned char* chars;
  const u64* offsets;
  const u64* vals;
};

// Lexicographic comparison of two keys as std::string::operator< compares them (bytes_cmp, hmj_strkey.h).
__device__ __forceinline__ int key_cmp(const StrSide& A, u64 ra, const StrSide& B, u64 rb) {
  const u64 pa = A.offsets[ra], la = A.offsets[ra + 1] - pa, pb = B.offsets[rb], lb = B.offsets[rb + 1] - pb;
  return bytes_cmp(A.chars + pa, la, B.chars + pb, lb);
}
__device__ __forceinline__ bool key_eq(const StrSide& A, u64 ra, const StrSide& B, u64 rb) {
  if (A.offsets[ra + 1] - A.offsets[ra] != B.offsets[rb + 1] - B.offsets[rb]) return false;
  return key_cmp(A, ra, B, rb) == 0;
}
__device__ __forceinline__ u64 payload(const StrSide& A, u64 row) { return A.vals[row]; }

// ---- host side -----------------------------------------------------------------------------------------------------------
constexpr KeyJoinNames kNames{"string join", "hash", "keys"};
constexpr u64 kNone = ~0ull;

int check_str_rel(hmj_ctx* c, const hmj_str_rel* r, const char* name) {
  char msg[128];
  if (!r) {
    std::snprintf(msg, sizeof(msg), "the %s relation is NULL", name);
    return fail(c, HMJ_E_ARG, msg);
  }
  if (r->n > 0xFFFFFFFFull) {
    std::snprintf(msg, sizeof(msg), "too many rows in the %s relation (at most 2^32-1)", name);
    return fail(c, HMJ_E_ARG, msg);
  }
  if (r->n > 0 && (!r->offsets || !r->vals)) {
    std::snprintf(msg, sizeof(msg), "%s relation: offsets / vals is NULL", name);
    return fail(c, HMJ_E_ARG, msg);
  }
  return HMJ_OK;
}

// err: the relation's report words (err[KA_BAD_ROW] preset to ~0, err[KA_NULL_CHARS] to 0)
int launch_hash(hmj_ctx* c, const void* chars, const u64* offsets, u64 n, u32 bits, u64* out, bool rows, const u64* vals, u64* acc, u64* err) {
  if (!n) return HMJ_OK;
  const u64 grid = (n + SH_THREADS - 1) / SH_THREADS;
  hipLaunchKernelGGL(str_hash_kernel, dim3((u32)grid), dim3(SH_THREADS), 0, c->stream, (const unsigned char*)chars, offsets, n, bits,
                     out, rows ? 1 : 0, vals, acc, err);
  HIP_TRY(hipGetLastError());
  return HMJ_OK;
}

// the hash kernel's verdict on one relation's offsets (h: its report words, read back)
int hash_errors(hmj_ctx* c, const u64* h, const char* name) {
  char msg[160];
  if (h[KA_BAD_ROW] != kNone) {
    std::snprintf(msg, sizeof(msg), "%s relation: offsets decrease at row %llu (offsets[%llu] < offsets[%llu])", name,
                  (unsigned long long)h[KA_BAD_ROW], (unsigned long long)h[KA_BAD_ROW] + 1, (unsigned long long)h[KA_BAD_ROW]);
    return fail(c, HMJ_E_ARG, msg);
  }
  if (h[KA_NULL_CHARS]) {
    std::snprintf(msg, sizeof(msg), "%s relation: chars is NULL but keys have bytes", name);
    return fail(c, HMJ_E_ARG, msg);
  }
  return HMJ_OK;
}

// The string join as hmj_tuplejoin.h's driver takes it: a tuple of one string column whose key64 is always the hash.
struct StrPolicy {
  using Side = StrSide;
  static constexpr bool kCanPack = false;
  static constexpr int kRelWords = 2;  // the hash kernels' report on one relation: [KA_BAD_ROW], [KA_NULL_CHARS]
  static_assert(KA_BAD_ROW < kRelWords && KA_NULL_CHARS < kRelWords, "the report words of one relation");
  static constexpr int kAccExtra = 2 * kRelWords;  // the build relation's, then the probe relation's
  // workload_signature kinds of the {hash,row} joins (u64 joins 0, sorts 1, u64 kinds 3..9, multi-column joins 14 and
  // 16..19, mixed joins 20..24): none of them teaches a join of another entry anything
  static constexpr int kMemoInner = 15;      // the inner join
  static constexpr int kMemoProbeRep = 10;   // first-wins join, probe rows against build representatives (probe SEMI / ANTI)
  static constexpr int kMemoBuildRep = 11;   // ... build rows against probe representatives (BUILD_SEMI / BUILD_ANTI)
  static constexpr int kMemoAmbiguous = 12;  // the ambiguous rows against every row of their hash on the other side
  static constexpr int kMemoPairs = 13;      // the outer kinds' pair join
  static const KeyJoinNames& names() { return kNames; }
  static KeyJoinWs& ws(hmj_ctx* c) { return c->str_ws; }
  static u64* err_of(hmj_ctx* c, int rel) { return tuple_acc_extra<StrPolicy>(c) + rel * kRelWords; }
  static int keys_begin(hmj_ctx* c) {
    u64* e = tuple_acc_extra<StrPolicy>(c);  // (the driver cleared the words)
    HIP_TRY(hipMemsetAsync(e + KA_BAD_ROW, 0xFF, sizeof(u64), c->stream));
    HIP_TRY(hipMemsetAsync(e + kRelWords + KA_BAD_ROW, 0xFF, sizeof(u64), c->stream));
    return HMJ_OK;
  }
  static int keys_check(hmj_ctx* c, TupleCall*) {
    u64 e[kAccExtra];
    RC_TRY(read_back(c, tuple_acc_extra<StrPolicy>(c), e, sizeof(e)));
    RC_TRY(hash_errors(c, e, "build"));
    return hash_errors(c, e + kRelWords, "probe");
  }
  static int key(hmj_ctx* c, const StrSide& A, int rel, u64 n, const TupleCall& call, u64* out, bool sum_probe, u64* acc) {
    return launch_hash(c, A.chars, A.offsets, n, call.bits, out, true, sum_probe ? A.vals : nullptr, acc, err_of(c, rel));
  }
  static int key_valid(hmj_ctx* c, const StrSide& A, const ColValid& V, int rel, u64 n, const TupleCall& call, u64 nblk, u64* dense, u64* comp,
                       u64 cap, const u64* off, bool sum_probe, u64* acc) {
    hipLaunchKernelGGL(str_hash_valid_kernel, dim3((u32)nblk), dim3(SH_THREADS), 0, c->stream, A.chars, A.offsets, n, call.bits,
                       StrValid{V.bits[0], V.off[0]}, dense, comp, cap, off, sum_probe ? A.vals : nullptr, acc, err_of(c, rel));
    HIP_TRY(hipGetLastError());
    return HMJ_OK;
  }
};

// One call of either entry on the driver: the probe side's INNER is tuple_join, every other kind tuple_join_kind.  The driver
// fills a hmj_cols_result, whose fields are hmj_str_result's (key64: hash).
int run_join(hmj_ctx* c, const hmj_str_rel* R, const hmj_str_rel* S, uint32_t flags, bool inner, TupleCall* call, hmj_str_result* out,
             const ColValid* VB, const ColValid* VP) {
  const StrSide RS{(const unsigned char*)R->chars, (const u64*)R->offsets, (const u64*)R->vals},
      SS{(const unsigned char*)S->chars, (const u64*)S->offsets, (const u64*)S->vals};
  hmj_cols_result r;
  std::memset(&r, 0, sizeof(r));
  if (inner) RC_TRY(tuple_join<StrPolicy>(c, RS, R->n, SS, S->n, flags, call, &r, VB, VP));
  else RC_TRY(tuple_join_kind<StrPolicy>(c, RS, R->n, SS, S->n, flags, call, &r, VB, VP));
  *out = hmj_str_result{r.n_matches, r.sum_r, r.sum_s, r.xor_fold, r.mix_sum, r.sum_probe_all, r.key64, r.r_row, r.s_row, r.rval, r.sval};
  return HMJ_OK;
}

// The validity bitmaps of a hmj_str_kind_opts whose struct_size covers them, as the kernels take them; *pb / *pp stay NULL
// for a relation without a bitmap (bits == NULL).
int opts_validity(hmj_ctx* c, const hmj_str_kind_opts* opts, const hmj_str_rel* build, const hmj_str_rel* probe, ColValid* VB, ColValid* VP,
                  const ColValid** pb, const ColValid** pp) {
  *pb = *pp = nullptr;
  if (opts->struct_size < offsetof(hmj_str_kind_opts, probe_validity) + sizeof(opts->probe_validity)) return HMJ_OK;
  const hmj_validity* v[2] = {&opts->build_validity, &opts->probe_validity};
  const hmj_str_rel* rel[2] = {build, probe};
  ColValid* V[2] = {VB, VP};
  const ColValid** pv[2] = {pb, pp};
  for (int k = 0; k < 2; k++) {
    if (!v[k]->bits) continue;
    if (v[k]->bit_offset > UINT64_MAX - rel[k]->n) {
      char msg[128];
      std::snprintf(msg, sizeof(msg), "%s relation: validity bit_offset + n overflows 64 bits", k ? "probe" : "build");
      return fail(c, HMJ_E_ARG, msg);
    }
    *V[k] = ColValid{};
    V[k]->bits[0] = (const unsigned char*)v[k]->bits;
    V[k]->off[0] = v[k]->bit_offset;
    V[k]->k = 1;
    *pv[k] = V[k];
  }
  return HMJ_OK;
}

}  // namespace

extern "C" {

int hmj_hash_str_device(hmj_ctx* c, const void* chars, const uint64_t* offsets, uint64_t n, uint32_t hash_bits, uint64_t* hash_out_dev) {
  if (!c) return HMJ_E_ARG;
  if (n > 0xFFFFFFFFull) return fail(c, HMJ_E_ARG, "too many rows (at most 2^32-1)");
  if (hash_bits > 63) return fail(c, HMJ_E_ARG, "hash_bits > 63");
  if (n > 0 && (!offsets || !hash_out_dev)) return fail(c, HMJ_E_ARG, "offsets / hash_out_dev is NULL");
  c->prep.valid = false;  // like any other call, hashing discards a prepared build side
  if (n == 0) return HMJ_OK;
  HIP_TRY(hipSetDevice(c->device));
  // (the report words of a join's build relation; no payloads, so nothing is added to acc)
  RC_TRY(ensure_dev(c, c->str_ws.acc, tuple_acc_bytes<StrPolicy>()));
  u64* err = StrPolicy::err_of(c, 0);
  HIP_TRY(hipMemsetAsync(err, 0, StrPolicy::kRelWords * sizeof(u64), c->stream));
  HIP_TRY(hipMemsetAsync(err + KA_BAD_ROW, 0xFF, sizeof(u64), c->stream));
  RC_TRY(launch_hash(c, chars, (const u64*)offsets, n, hash_bits, (u64*)hash_out_dev, false, nullptr, (u64*)c->str_ws.acc.p, err));
  u64 h[StrPolicy::kRelWords];
  RC_TRY(read_back(c, err, h, sizeof(h)));
  return hash_errors(c, h, "the");
}

int hmj_join_str_device(hmj_ctx* c, const hmj_str_rel* build, const hmj_str_rel* probe, uint32_t flags, hmj_str_join_opts* opts,
                        hmj_str_result* out) {
  if (!c) return HMJ_E_ARG;
  if (!opts || !out) return fail(c, HMJ_E_ARG, "opts / out is NULL");
  if (opts->struct_size < offsetof(hmj_str_join_opts, hash_bits) + sizeof(opts->hash_bits))
    return fail(c, HMJ_E_ARG, "hmj_str_join_opts.struct_size too small");
  if (opts->hash_bits > 63) return fail(c, HMJ_E_ARG, "hash_bits > 63");
  if (flags & HMJ_FIRST_WINS) return fail(c, HMJ_E_ARG, "HMJ_FIRST_WINS is not defined for string joins");
  RC_TRY(check_str_rel(c, build, "build"));
  RC_TRY(check_str_rel(c, probe, "probe"));
  std::memset(out, 0, sizeof(*out));
  HIP_TRY(hipSetDevice(c->device));
  // the out fields of opts go to a full-size copy first; the caller gets the prefix its struct_size holds
  hmj_str_join_opts o;
  opts_prefix_in(&o, opts);
  TupleCall call;  // (hmj_str_join_opts carries no bitmap: the call without NULL keys)
  call.bits = o.hash_bits;
  RC_TRY(run_join(c, build, probe, flags, true, &call, out, nullptr, nullptr));
  o.n_hash_pairs = call.n_key_pairs;
  o.n_collisions = call.n_collisions;
  fill_join_ms(c, o, o.ms_hash, c->str_ws.ev);
  opts_prefix_out(opts, o);
  return HMJ_OK;
}

int hmj_join_kind_str_device(hmj_ctx* c, const hmj_str_rel* build, const hmj_str_rel* probe, uint32_t flags, hmj_str_kind_opts* opts,
                             hmj_str_result* out) {
  if (!c) return HMJ_E_ARG;
  if (!opts || !out) return fail(c, HMJ_E_ARG, "opts / out is NULL");
  if (opts->struct_size < offsetof(hmj_str_kind_opts, build_fill) + sizeof(opts->build_fill))
    return fail(c, HMJ_E_ARG, "hmj_str_kind_opts.struct_size too small");
  if (opts->side > HMJ_KIND_BUILD_SIDE) return fail(c, HMJ_E_ARG, "unknown join side");
  if (opts->side == HMJ_KIND_PROBE_SIDE ? opts->kind > HMJ_JOIN_PROBE_OUTER : (opts->kind < HMJ_BUILD_SEMI || opts->kind > HMJ_FULL_OUTER))
    return fail(c, HMJ_E_ARG, "unknown join kind");
  if (opts->hash_bits > 63) return fail(c, HMJ_E_ARG, "hash_bits > 63");
  if (flags & HMJ_FIRST_WINS) return fail(c, HMJ_E_ARG, "HMJ_FIRST_WINS is not defined for string joins");
  if (flags & HMJ_NULL_EQUAL)
    return fail(c, HMJ_E_ARG, "HMJ_NULL_EQUAL is not taken by the string kinds: call hmj_join_mixed_device with one string column");
  RC_TRY(check_str_rel(c, build, "build"));
  RC_TRY(check_str_rel(c, probe, "probe"));
  ColValid VB, VP;
  const ColValid *vb, *vp;
  RC_TRY(opts_validity(c, opts, build, probe, &VB, &VP, &vb, &vp));
  std::memset(out, 0, sizeof(*out));
  HIP_TRY(hipSetDevice(c->device));
  // the out fields of opts go to a full-size copy first; the caller gets the prefix its struct_size holds
  hmj_str_kind_opts o;
  opts_prefix_in(&o, opts);
  // (out fields from `counts` on; the validity bitmaps behind them are in fields)
  opts_clear_out(&o, opts, offsetof(hmj_str_kind_opts, counts), offsetof(hmj_str_kind_opts, build_validity), offsetof(hmj_str_kind_opts, n_build_null));
  TupleCall call;
  call.bits = o.hash_bits;
  call.side = o.side;
  call.kind = o.kind;
  call.probe_fill = o.probe_fill;
  call.build_fill = o.build_fill;
  const bool inner = o.side == HMJ_KIND_PROBE_SIDE && o.kind == HMJ_JOIN_INNER;  // exactly the inner string join
  RC_TRY(run_join(c, build, probe, flags, inner, &call, out, vb, vp));
  o.counts = call.counts;
  o.n_hash_pairs = call.n_key_pairs;
  o.n_collisions = call.n_collisions;
  o.n_build_null = call.n_build_null;
  o.n_probe_null = call.n_probe_null;
  fill_kind_ms(c, o, o.ms_hash, c->str_ws.ev, !inner);
  opts_prefix_out(opts, o);
  return HMJ_OK;
}

}  // extern "C"
