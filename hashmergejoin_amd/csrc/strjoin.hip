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
// Steps 3 and 4 and everything the join kinds add to them -- rep_verify_kernel, the sweeps, the ordered kinds' sort and
// gather -- are hmj_keyjoin.h's kernels and launch sequences, shared with the multi-column join and instantiated here on
// StrSide; this file holds the hash kernels, the key policy (key_eq / key_cmp / payload on StrSide) and stages 1-3 of the
// calls.  The byte reader, _Hash_bytes and the byte comparison are hmj_strkey.h's, shared with the mixed-key join (mixjoin.hip).
// NULL keys (validity bitmaps, calls that pass one only): valid_count_kernel counts the rows that have a key per
// workgroup, one scan places them, and str_hash_valid_kernel writes two arrays per relation: the dense rows the sweeps walk
// by row index (a NULL-key row: hash 0, row HMJ_STR_NO_ROW) and the compacted rows of the valid rows, which are all the u64
// joins see.  Row indices stay the caller's, so verification, marks and gathers are unchanged; ordered results emit the
// NULL-key rows into a tail behind the rows that are sorted (DESIGN.md "NULL keys on string keys").
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>

#include "hmj_keyjoin.h"
#include "hmj_strkey.h"

namespace {

constexpr int SH_THREADS = 256;
constexpr int SH_WAVES = SH_THREADS / 64;
constexpr int SH_STAGE = 4096;  // LDS bytes a wave stages its 64 keys in; a longer span: per-lane reads from global memory
static_assert(SH_THREADS == KJ_THREADS, "valid_count_kernel counts the rows of one workgroup of str_hash_valid_kernel");

// Per wave: 64 consecutive keys, bytes [offsets[i0], offsets[i0 + 64]).  Staged in LDS when the span's aligned 16-byte
// blocks fit SH_STAGE, else read per lane from global memory.  rows: out = {hash, row} x n, else bare hashes.  vals != NULL: their sum goes to acc[KA_ACC + ACC_SUM_P].
__global__ __launch_bounds__(SH_THREADS) void str_hash_kernel(const unsigned char* __restrict__ chars, const u64* __restrict__ offsets,
                                                              u64 n, u32 hash_bits, u64* __restrict__ out, int rows,
                                                              const u64* __restrict__ vals, u64* __restrict__ acc) {
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
  if (bad_mask && lane == (int)__builtin_ctzll(bad_mask)) atomicMin(&acc[KA_BAD_ROW], i);
  const bool ok_wave = i0 < n && !bad_mask && s1 >= s0;
  if (ok_wave && !chars && s1 > s0 && lane == 0) atomicAdd(&acc[KA_NULL_CHARS], 1ull);
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
    if (lane == 0) atomicAdd(&acc[KA_ACC + hmj::ACC_SUM_P], vs);
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
// One relation's Arrow validity bitmap (coljoin.hip's ColValid for the one key column a string relation has): row i has a
// key iff bit off + i (least-significant bit first) is set.  Only calls that pass a bitmap reach valid_count_kernel (hmj_keyjoin.h, pass 1) and the kernel below.
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
                                                                    const u64* __restrict__ vals, u64* __restrict__ acc) {
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
  if (bad_mask && lane == (int)__builtin_ctzll(bad_mask)) atomicMin(&acc[KA_BAD_ROW], i);
  const bool ok_wave = i0 < n && !bad_mask && s1 >= s0;
  if (ok_wave && !chars && s1 > s0 && lane == 0) atomicAdd(&acc[KA_NULL_CHARS], 1ull);
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
    if (lane == 0) atomicAdd(&acc[KA_ACC + hmj::ACC_SUM_P], vs);
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
constexpr int kStrJoinMemoKind = 15;  // workload_signature kind of the inner {hash,row} join (u64 joins 0, sorts 1, kinds 3..9,
                                      // string kinds 10..13, inner multi-column join 14, multi-column kinds 16..19)
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

// acc: three blocks of KA_N words -- [0] build side's hashing, [1] probe side's hashing, [2] verification / collisions
int acc_reset(hmj_ctx* c, u64* acc) {
  HIP_TRY(hipMemsetAsync(acc, 0, 3 * KA_N * sizeof(u64), c->stream));
  HIP_TRY(hipMemsetAsync(acc + KA_BAD_ROW, 0xFF, sizeof(u64), c->stream));
  HIP_TRY(hipMemsetAsync(acc + KA_N + KA_BAD_ROW, 0xFF, sizeof(u64), c->stream));
  return HMJ_OK;
}

int launch_hash(hmj_ctx* c, const void* chars, const u64* offsets, u64 n, u32 bits, u64* out, bool rows, const u64* vals, u64* acc) {
  if (!n) return HMJ_OK;
  const u64 grid = (n + SH_THREADS - 1) / SH_THREADS;
  hipLaunchKernelGGL(str_hash_kernel, dim3((u32)grid), dim3(SH_THREADS), 0, c->stream, (const unsigned char*)chars, offsets, n, bits,
                     out, rows ? 1 : 0, vals, acc);
  HIP_TRY(hipGetLastError());
  return HMJ_OK;
}

// NULL keys: the {hash,row} rows of both relations in a call with bitmaps (VB / VP: NULL where a relation has none; such a
// relation goes through str_hash_kernel as always, and its dense rows are its join rows).  A relation with a bitmap: its
// valid rows counted per workgroup and scanned (vblk: nblk counts, then nblk + 1 offsets, the build side's first), then
// hashed into cmp (room for every row: no read-back between the passes) and, if `dense`, into the row-indexed rows_r / rows_s.
// rows[2] / tot[2]: what the u64 joins take, and where on the device the number of those rows stands (NULL: every row).
int launch_hashes_valid(hmj_ctx* c, const hmj_str_rel* R, const hmj_str_rel* S, const StrValid* VB, const StrValid* VP, u32 bits, bool dense,
                        bool sum_probe, u64* acc, const void** rows, const u64** tot) {
  const hmj_str_rel* rel[2] = {R, S};
  const StrValid* V[2] = {VB, VP};
  KeyJoinWs& ws = c->str_ws;
  DevBuf* plain[2] = {&ws.rows_r, &ws.rows_s};
  DevBuf* cmp[2] = {&ws.cmp_r, &ws.cmp_s};
  u64 nblk[2];
  for (int k = 0; k < 2; k++) nblk[k] = V[k] && rel[k]->n ? (rel[k]->n + SH_THREADS - 1) / SH_THREADS : 0;
  RC_TRY(ensure_dev(c, ws.vblk, (2 * (nblk[0] + nblk[1]) + 2) * sizeof(u64)));
  u64* vblk = (u64*)ws.vblk.p;
  for (int k = 0; k < 2; k++) {
    const u64 n = rel[k]->n;
    const u64* vals = k == 1 && sum_probe ? (const u64*)rel[k]->vals : nullptr;
    rows[k] = plain[k]->p;
    tot[k] = nullptr;
    if (!nblk[k]) {
      RC_TRY(launch_hash(c, rel[k]->chars, (const u64*)rel[k]->offsets, n, bits, (u64*)plain[k]->p, true, vals, acc + k * KA_N));
      continue;
    }
    u64 *cnt = vblk + (k ? 2 * nblk[0] + 1 : 0), *off = cnt + nblk[k];
    RC_TRY(ensure_dev(c, *cmp[k], 16 * n));
    hipLaunchKernelGGL(valid_count_kernel<StrValid>, dim3((u32)nblk[k]), dim3(SH_THREADS), 0, c->stream, *V[k], n, cnt);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hmj::launch_scan_u64(cnt, off, (u32)nblk[k], c->stream));
    hipLaunchKernelGGL(str_hash_valid_kernel, dim3((u32)nblk[k]), dim3(SH_THREADS), 0, c->stream, (const unsigned char*)rel[k]->chars,
                       (const u64*)rel[k]->offsets, n, bits, *V[k], dense ? (u64*)plain[k]->p : nullptr, (u64*)cmp[k]->p, n,
                       (const u64*)off, vals, acc + k * KA_N);
    HIP_TRY(hipGetLastError());
    rows[k] = cmp[k]->p;
    tot[k] = off + nblk[k];
  }
  return HMJ_OK;
}

// the hash kernel's verdict on one relation's offsets (h: its acc block, read back)
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

// VB / VP: the relations' validity bitmaps, NULL where a relation has none (both NULL: the call without NULL keys, all
// hmj_join_str_device makes -- hmj_str_join_opts carries no bitmap; the INNER kind of hmj_join_kind_str_device passes its
// own).  n_null (with bitmaps): the NULL-key rows of the build and the probe side.
int join_str(hmj_ctx* c, const hmj_str_rel* R, const hmj_str_rel* S, uint32_t flags, hmj_str_join_opts* opts, hmj_str_result* out,
             const StrValid* VB = nullptr, const StrValid* VP = nullptr, u64* n_null = nullptr) {
  u64 nb = R->n, np = S->n;
  const u32 bits = opts->hash_bits;
  if (flags & HMJ_ORDERED) flags |= HMJ_MATERIALIZE;
  const bool mat = flags & HMJ_MATERIALIZE, ordered = flags & HMJ_ORDERED, checksum = flags & HMJ_CHECKSUM;
  c->prep.valid = false;  // like any other call, a string join discards a prepared build side
  KeyJoinWs& ws = c->str_ws;
  RC_TRY(ensure_dev(c, ws.acc, 3 * KA_N * sizeof(u64)));
  RC_TRY(ensure_dev(c, ws.rows_r, 16 * (nb ? nb : 1)));
  RC_TRY(ensure_dev(c, ws.rows_s, 16 * (np ? np : 1)));
  u64* acc = (u64*)ws.acc.p;
  u64 h[3 * KA_N];
  // 1. {hash, row} rows of both relations (+ the probe payloads' sum)
  RC_TRY(record(c, ws.ev, 0));
  RC_TRY(acc_reset(c, acc));
  const void* rows[2] = {ws.rows_r.p, ws.rows_s.p};  // the rows the u64 join takes
  u64 nv[2] = {nb, np};                                       // ... and how many: the rows that have a key
  if (!VB && !VP) {
    RC_TRY(launch_hash(c, R->chars, (const u64*)R->offsets, nb, bits, (u64*)ws.rows_r.p, true, nullptr, acc));
    RC_TRY(launch_hash(c, S->chars, (const u64*)S->offsets, np, bits, (u64*)ws.rows_s.p, true, (flags & HMJ_SUM_PROBE) ? (const u64*)S->vals : nullptr,
                       acc + KA_N));
    RC_TRY(record(c, ws.ev, 1));
  } else {  // NULL keys: only the rows that have a key are joined (the inner join walks no relation by row: no dense rows)
    const u64* tot[2];
    RC_TRY(launch_hashes_valid(c, R, S, VB, VP, bits, false, flags & HMJ_SUM_PROBE, acc, rows, tot));
    RC_TRY(record(c, ws.ev, 1));
    for (int k = 0; k < 2; k++)
      if (tot[k]) HIP_TRY(hipMemcpyAsync(&nv[k], tot[k], sizeof(u64), hipMemcpyDeviceToHost, c->stream));
  }
  RC_TRY(read_back(c, acc, h, sizeof(h)));
  RC_TRY(hash_errors(c, h, "build"));
  RC_TRY(hash_errors(c, h + KA_N, "probe"));
  if (nv[0] > nb || nv[1] > np) return fail(c, HMJ_E_HIP, "string join: more valid rows counted than the relation holds");
  if (n_null) {
    n_null[0] = nb - nv[0];
    n_null[1] = np - nv[1];
  }
  nb = nv[0];  // from here on: the rows that have a key (every row in a call without bitmaps)
  np = nv[1];
  if (flags & HMJ_SUM_PROBE) out->sum_probe_all = h[KA_N + KA_ACC + hmj::ACC_SUM_P];
  if (nb == 0 || np == 0) {  // (nothing to join: no plan either)
    std::memset(&c->plan, 0, sizeof(c->plan));
    c->plan.struct_size = sizeof(c->plan);
    std::memset(&c->timing, 0, sizeof(c->timing));
    for (int k = 2; k < 5; k++) RC_TRY(record(c, ws.ev, k));
    return HMJ_OK;
  }
  // 2. the u64 join of the {hash, row} rows: pairs of equal hash as (hash, r_row, s_row), ordered by them if asked
  hmj_result inner;
  RC_TRY(memo_join(c, rows[0], nb, rows[1], np, HMJ_MATERIALIZE | (flags & HMJ_ORDERED), kStrJoinMemoKind, &inner));
  RC_TRY(record(c, ws.ev, 2));
  const u64 n_pairs = inner.n_matches;
  opts->n_hash_pairs = n_pairs;
  // 3. key verification, payload gather, stable compaction (or the count modes' reduction)
  const StrSide RS{(const unsigned char*)R->chars, (const u64*)R->offsets, (const u64*)R->vals},
      SS{(const unsigned char*)S->chars, (const u64*)S->offsets, (const u64*)S->vals};
  const u64 *ik = (const u64*)inner.key, *ir = (const u64*)inner.rval, *is = (const u64*)inner.sval;
  const u64 nblk = blocks_of(n_pairs);
  if (nblk > 0xFFFFFFFFull) return too_many_pairs(c, kNames);
  u64* acc_v = acc + 2 * KA_N;
  u64 n_out = 0;
  if (n_pairs && mat) {
    RC_TRY(ensure_dev(c, ws.flags, nblk * KJ_WAVES * sizeof(u64)));
    RC_TRY(ensure_dev(c, ws.blk, nblk * sizeof(u64)));
    RC_TRY(ensure_dev(c, ws.blk_off, (nblk + 1) * sizeof(u64)));
    DevBuf* cols[5] = {&ws.key, &ws.rrow, &ws.srow, &ws.rval, &ws.sval};
    for (DevBuf* b : cols) RC_TRY(ensure_dev(c, *b, n_pairs * sizeof(u64)));
    hipLaunchKernelGGL((verify_kernel<StrSide, true>), dim3((u32)nblk), dim3(KJ_THREADS), 0, c->stream, ik, ir, is, n_pairs, RS, SS, (u64*)ws.flags.p, (u64*)ws.blk.p, acc_v, 0, nullptr, nullptr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hmj::launch_scan_u64((const u64*)ws.blk.p, (u64*)ws.blk_off.p, (u32)nblk, c->stream));
    hipLaunchKernelGGL(compact_kernel<StrSide>, dim3((u32)nblk), dim3(KJ_THREADS), 0, c->stream, ik, ir, is, n_pairs, RS, SS, (const u64*)ws.flags.p, (const u64*)ws.blk_off.p, (u64*)ws.key.p, (u64*)ws.rrow.p,
                       (u64*)ws.srow.p, (u64*)ws.rval.p, (u64*)ws.sval.p, acc_v, checksum ? 1 : 0);
    HIP_TRY(hipGetLastError());
    RC_TRY(read_back(c, (const u64*)ws.blk_off.p + nblk, &n_out, sizeof(u64)));
  } else if (n_pairs) {
    hipLaunchKernelGGL((verify_kernel<StrSide, false>), dim3((u32)nblk), dim3(KJ_THREADS), 0, c->stream, ik, ir, is, n_pairs, RS, SS, nullptr, nullptr, acc_v, checksum ? 1 : 0, nullptr, nullptr);
    HIP_TRY(hipGetLastError());
  }
  RC_TRY(record(c, ws.ev, 3));
  // 4. ordered: runs of equal hash with different build keys, sorted by key bytes
  if (ordered && n_out > 1) {
    u64* cols[5] = {(u64*)ws.key.p, (u64*)ws.rrow.p, (u64*)ws.srow.p, (u64*)ws.rval.p, (u64*)ws.sval.p};
    RC_TRY(order_collisions<false>(c, ws, RS, StrSide{}, cols, n_out, acc_v));
  }
  RC_TRY(record(c, ws.ev, 4));
  RC_TRY(read_back(c, acc_v, h, KA_N * sizeof(u64)));
  RC_TRY(collision_errors(c, kNames, h[KA_ERR]));
  const u64* a = h + KA_ACC;
  out->n_matches = mat ? n_out : a[hmj::ACC_N];
  out->sum_r = a[hmj::ACC_SUM_R];
  out->sum_s = a[hmj::ACC_SUM_S];
  if (checksum) {
    out->xor_fold = a[hmj::ACC_XOR];
    out->mix_sum = a[hmj::ACC_MIX];
  }
  if (mat) {
    out->hash = (const uint64_t*)ws.key.p;
    out->r_row = (const uint64_t*)ws.rrow.p;
    out->s_row = (const uint64_t*)ws.srow.p;
    out->rval = (const uint64_t*)ws.rval.p;
    out->sval = (const uint64_t*)ws.sval.p;
  }
  opts->n_collisions = n_pairs - out->n_matches;
  return HMJ_OK;
}

// ---- join kinds (hmj_join_kind_str_device) -------------------------------------------------------------------------
// workload_signature kinds of the {hash,row} joins the kinds run (u64 joins 0, sorts 1, u64 kinds 3..9, inner multi-column
// join 14, inner string join 15, multi-column kinds 16..19): none of them teaches a join of another entry anything
constexpr int kMemoProbeRep = 10;  // first-wins join, probe rows against build representatives (probe SEMI / ANTI)
constexpr int kMemoBuildRep = 11;  // ... build rows against probe representatives (BUILD_SEMI / BUILD_ANTI)
constexpr int kMemoAmbiguous = 12; // the ambiguous rows against every row of their hash on the other side
constexpr int kMemoPairs = 13;     // the outer kinds' pair join
constexpr int kKindAccBlocks = 5;  // acc: [0] / [1] hashing, [2] verification, [3] probe sweep, [4] build sweep

// VB / VP: as join_str; o->n_build_null / n_probe_null are filled in a call with bitmaps.
int join_str_kind(hmj_ctx* c, const hmj_str_rel* R, const hmj_str_rel* S, uint32_t flags, hmj_str_kind_opts* o, hmj_str_result* out,
                  const StrValid* VB = nullptr, const StrValid* VP = nullptr) {
  const u64 nb = R->n, np = S->n;
  const u32 bits = o->hash_bits, kind = o->kind;
  if (flags & HMJ_ORDERED) flags |= HMJ_MATERIALIZE;
  const bool mat = flags & HMJ_MATERIALIZE, checksum = flags & HMJ_CHECKSUM;
  const bool bside = o->side == HMJ_KIND_BUILD_SIDE;
  // semi / anti of either side (HMJ_JOIN_SEMI == HMJ_BUILD_SEMI, HMJ_JOIN_ANTI == HMJ_BUILD_ANTI), else an outer kind
  const bool semi_anti = kind == HMJ_JOIN_SEMI || kind == HMJ_JOIN_ANTI;
  c->prep.valid = false;  // like any other call, a string join discards a prepared build side
  KeyJoinWs& ws = c->str_ws;
  std::memset(&c->plan, 0, sizeof(c->plan));
  c->plan.struct_size = sizeof(c->plan);
  std::memset(&c->timing, 0, sizeof(c->timing));
  RC_TRY(ensure_dev(c, ws.acc, kKindAccBlocks * KA_N * sizeof(u64)));
  RC_TRY(ensure_dev(c, ws.rows_r, 16 * (nb ? nb : 1)));
  RC_TRY(ensure_dev(c, ws.rows_s, 16 * (np ? np : 1)));
  RC_TRY(ensure_dev(c, ws.mark_r, nb ? nb : 1));
  RC_TRY(ensure_dev(c, ws.mark_s, np ? np : 1));
  u64* acc = (u64*)ws.acc.p;
  u64* acc_v = acc + 2 * KA_N;
  u64 h[kKindAccBlocks * KA_N];
  // 1. {hash, row} rows of both relations (+ the probe payloads' sum), marks cleared
  RC_TRY(record(c, ws.ev, 0));
  HIP_TRY(hipMemsetAsync(acc, 0, kKindAccBlocks * KA_N * sizeof(u64), c->stream));
  HIP_TRY(hipMemsetAsync(acc + KA_BAD_ROW, 0xFF, sizeof(u64), c->stream));
  HIP_TRY(hipMemsetAsync(acc + KA_N + KA_BAD_ROW, 0xFF, sizeof(u64), c->stream));
  // (NULL keys: the dense rows stay indexed by row for the sweeps; the u64 joins take only the rows that have a key)
  const void* rows[2] = {ws.rows_r.p, ws.rows_s.p};
  u64 nv[2] = {nb, np};
  if (!VB && !VP) {
    RC_TRY(launch_hash(c, R->chars, (const u64*)R->offsets, nb, bits, (u64*)ws.rows_r.p, true, nullptr, acc));
    RC_TRY(launch_hash(c, S->chars, (const u64*)S->offsets, np, bits, (u64*)ws.rows_s.p, true,
                       (flags & HMJ_SUM_PROBE) ? (const u64*)S->vals : nullptr, acc + KA_N));
  } else {
    const u64* tot[2];
    RC_TRY(launch_hashes_valid(c, R, S, VB, VP, bits, true, flags & HMJ_SUM_PROBE, acc, rows, tot));
    for (int k = 0; k < 2; k++)
      if (tot[k]) HIP_TRY(hipMemcpyAsync(&nv[k], tot[k], sizeof(u64), hipMemcpyDeviceToHost, c->stream));
  }
  if (nb) HIP_TRY(hipMemsetAsync(ws.mark_r.p, 0, nb, c->stream));
  if (np) HIP_TRY(hipMemsetAsync(ws.mark_s.p, 0, np, c->stream));
  RC_TRY(record(c, ws.ev, 1));
  RC_TRY(read_back(c, acc, h, 2 * KA_N * sizeof(u64)));
  RC_TRY(hash_errors(c, h, "build"));
  RC_TRY(hash_errors(c, h + KA_N, "probe"));
  const u64 nvb = nv[0], nvp = nv[1];  // the rows that have a key
  if (nvb > nb || nvp > np) return fail(c, HMJ_E_HIP, "string join: more valid rows counted than the relation holds");
  if (VB || VP) {
    o->n_build_null = nb - nvb;
    o->n_probe_null = np - nvp;
  }
  if (flags & HMJ_SUM_PROBE) out->sum_probe_all = h[KA_N + KA_ACC + hmj::ACC_SUM_P];
  const StrSide RS{(const unsigned char*)R->chars, (const u64*)R->offsets, (const u64*)R->vals},
      SS{(const unsigned char*)S->chars, (const u64*)S->offsets, (const u64*)S->vals};
  unsigned char *mark_r = (unsigned char*)ws.mark_r.p, *mark_s = (unsigned char*)ws.mark_s.p;
  // 2. + 3. the {hash,row} join(s) and the key verification, which marks the rows that have a partner
  u64 n_pairs = 0;
  hmj_result inner;
  std::memset(&inner, 0, sizeof(inner));
  if (semi_anti) {
    // every row of the side asked about (K) meets the FIRST row of its hash on the other side (O), in row order
    const u64 nK = bside ? nvb : nvp, nO = bside ? nvp : nvb;
    const void *rowsK = bside ? rows[0] : rows[1], *rowsO = bside ? rows[1] : rows[0];
    const StrSide &KS = bside ? RS : SS, &OS = bside ? SS : RS;
    unsigned char* mark = bside ? mark_r : mark_s;
    if (nK && nO) {
      hmj_result rep;
      RC_TRY(memo_join(c, rowsO, nO, rowsK, nK, HMJ_MATERIALIZE | HMJ_FIRST_WINS, bside ? kMemoBuildRep : kMemoProbeRep, &rep));
      RC_TRY(record(c, ws.ev, 2));
      n_pairs = rep.n_matches;  // <= nK
      if (n_pairs) {
        RC_TRY(ensure_dev(c, ws.amb, 16 * n_pairs));
        hipLaunchKernelGGL((rep_verify_kernel<StrSide, true>), dim3((u32)blocks_of(n_pairs)), dim3(KJ_THREADS), 0, c->stream, (const u64*)rep.key,
                           (const u64*)rep.rval, (const u64*)rep.sval, n_pairs, OS, KS, mark, (u64*)ws.amb.p, acc_v);
        HIP_TRY(hipGetLastError());
        RC_TRY(read_back(c, acc_v, h, KA_N * sizeof(u64)));
        const u64 n_amb = h[KA_AMB_N];
        if (n_amb) {  // (a real hash collision: a representative's key differs from the row's)
          hmj_result all;
          RC_TRY(memo_join(c, rowsO, nO, ws.amb.p, n_amb, HMJ_MATERIALIZE, kMemoAmbiguous, &all));
          n_pairs += all.n_matches;
          if (all.n_matches) {
            hipLaunchKernelGGL((rep_verify_kernel<StrSide, true>), dim3((u32)blocks_of(all.n_matches)), dim3(KJ_THREADS), 0, c->stream,
                               (const u64*)all.key, (const u64*)all.rval, (const u64*)all.sval, all.n_matches, OS, KS, mark,
                               nullptr, acc_v);
            HIP_TRY(hipGetLastError());
          }
        }
      }
    } else {
      RC_TRY(record(c, ws.ev, 2));
    }
  } else if (nvb && nvp) {
    RC_TRY(memo_join(c, rows[0], nvb, rows[1], nvp, HMJ_MATERIALIZE | (flags & HMJ_ORDERED), kMemoPairs, &inner));
    RC_TRY(record(c, ws.ev, 2));
    n_pairs = inner.n_matches;
  } else {
    RC_TRY(record(c, ws.ev, 2));
  }
  o->n_hash_pairs = n_pairs;
  KindRows k;
  RC_TRY(kind_rows(c, ws, kNames, o->side, kind, flags, nb, np, nvb, nvp, VB != nullptr, VP != nullptr, n_pairs, &k));
  const u64* pairs[3] = {(const u64*)inner.key, (const u64*)inner.rval, (const u64*)inner.sval};
  if (k.nblk_v && mat) {
    hipLaunchKernelGGL((verify_kernel<StrSide, true, true>), dim3((u32)k.nblk_v), dim3(KJ_THREADS), 0, c->stream, pairs[0], pairs[1],
                       pairs[2], n_pairs, RS, SS, (u64*)ws.flags.p, (u64*)ws.blk.p, acc_v, 0, mark_r, mark_s);
    HIP_TRY(hipGetLastError());
  } else if (k.nblk_v) {
    hipLaunchKernelGGL((verify_kernel<StrSide, false, true>), dim3((u32)k.nblk_v), dim3(KJ_THREADS), 0, c->stream, pairs[0], pairs[1],
                       pairs[2], n_pairs, RS, SS, nullptr, nullptr, acc_v, checksum ? 1 : 0, mark_r, mark_s);
    HIP_TRY(hipGetLastError());
  }
  RC_TRY(record(c, ws.ev, 3));
  // 4. the sweeps, 5. ordered: the sort by hash, then runs of equal hash with several keys sorted by key bytes
  u64 *acc_p = acc + 3 * KA_N, *acc_b = acc + 4 * KA_N;
  RC_TRY(kind_sweeps(c, ws, kNames, k, RS, SS, o->probe_fill, o->build_fill, true, pairs, acc_v, acc_p, acc_b));
  RC_TRY(record(c, ws.ev, 4));
  RC_TRY(kind_order(c, ws, k, RS, SS, true, acc_v));
  RC_TRY(record(c, ws.ev, 5));
  RC_TRY(read_back(c, acc_v, h + 2 * KA_N, 3 * KA_N * sizeof(u64)));
  const u64 *av = h + 2 * KA_N, *ap = h + 3 * KA_N, *ab = h + 4 * KA_N;
  RC_TRY(collision_errors(c, kNames, av[KA_ERR]));
  kind_report(k, av + KA_ACC, ap + KA_ACC, ab + KA_ACC, out, &o->counts);
  if (mat) out->hash = (const uint64_t*)k.oc[0];
  o->n_collisions = semi_anti ? av[KA_DIFF] : n_pairs - k.n_in;
  return HMJ_OK;
}

// The validity bitmaps of a hmj_str_kind_opts whose struct_size covers them, as the kernels take them; *pb / *pp stay NULL
// for a relation without a bitmap (bits == NULL).
int opts_validity(hmj_ctx* c, const hmj_str_kind_opts* opts, const hmj_str_rel* build, const hmj_str_rel* probe, StrValid* VB, StrValid* VP,
                  const StrValid** pb, const StrValid** pp) {
  *pb = *pp = nullptr;
  if (opts->struct_size < offsetof(hmj_str_kind_opts, probe_validity) + sizeof(opts->probe_validity)) return HMJ_OK;
  const hmj_validity* v[2] = {&opts->build_validity, &opts->probe_validity};
  const hmj_str_rel* rel[2] = {build, probe};
  StrValid* V[2] = {VB, VP};
  const StrValid** pv[2] = {pb, pp};
  for (int k = 0; k < 2; k++) {
    if (!v[k]->bits) continue;
    if (v[k]->bit_offset > UINT64_MAX - rel[k]->n) {
      char msg[128];
      std::snprintf(msg, sizeof(msg), "%s relation: validity bit_offset + n overflows 64 bits", k ? "probe" : "build");
      return fail(c, HMJ_E_ARG, msg);
    }
    V[k]->bits = (const unsigned char*)v[k]->bits;
    V[k]->off = v[k]->bit_offset;
    *pv[k] = V[k];
  }
  return HMJ_OK;
}
// The out fields of a full-size copy o of the caller's opts are cleared from `counts` on; the in fields that lie behind them
// (the validity bitmaps) are the caller's again, as far as its struct_size holds them.
void clear_out_fields(hmj_str_kind_opts* o, const hmj_str_kind_opts* opts) {
  using T = hmj_str_kind_opts;
  std::memset(&o->counts, 0, sizeof(T) - offsetof(T, counts));
  const size_t lo = offsetof(T, build_validity), hi = offsetof(T, n_build_null);
  const size_t have = opts->struct_size < hi ? opts->struct_size : hi;
  if (have > lo) std::memcpy((char*)o + lo, (const char*)opts + lo, have - lo);
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
  RC_TRY(ensure_dev(c, c->str_ws.acc, 3 * KA_N * sizeof(u64)));
  u64* acc = (u64*)c->str_ws.acc.p;
  RC_TRY(acc_reset(c, acc));
  RC_TRY(launch_hash(c, chars, (const u64*)offsets, n, hash_bits, (u64*)hash_out_dev, false, nullptr, acc));
  u64 h[KA_N];
  RC_TRY(read_back(c, acc, h, sizeof(h)));
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
  std::memset(&o, 0, sizeof(o));
  std::memcpy(&o, opts, opts->struct_size < sizeof(o) ? opts->struct_size : sizeof(o));
  const int rc = join_str(c, build, probe, flags, &o, out);
  if (rc != HMJ_OK) return rc;
  if (c->profiling) {
    (void)hipStreamSynchronize(c->stream);
    o.ms_hash = elapsed(c->str_ws.ev, 0, 1);
    o.ms_join = elapsed(c->str_ws.ev, 1, 2);
    o.ms_verify = elapsed(c->str_ws.ev, 2, 3);
    o.ms_order = elapsed(c->str_ws.ev, 3, 4);
  }
  const uint32_t room = opts->struct_size < sizeof(o) ? opts->struct_size : (uint32_t)sizeof(o);
  o.struct_size = opts->struct_size;
  std::memcpy(opts, &o, room);
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
  StrValid VB, VP;
  const StrValid *vb, *vp;
  RC_TRY(opts_validity(c, opts, build, probe, &VB, &VP, &vb, &vp));
  std::memset(out, 0, sizeof(*out));
  HIP_TRY(hipSetDevice(c->device));
  // the out fields of opts go to a full-size copy first; the caller gets the prefix its struct_size holds
  hmj_str_kind_opts o;
  std::memset(&o, 0, sizeof(o));
  std::memcpy(&o, opts, opts->struct_size < sizeof(o) ? opts->struct_size : sizeof(o));
  clear_out_fields(&o, opts);
  if (o.side == HMJ_KIND_PROBE_SIDE && o.kind == HMJ_JOIN_INNER) {  // exactly the inner string join
    hmj_str_join_opts jo;
    std::memset(&jo, 0, sizeof(jo));
    jo.struct_size = sizeof(jo);
    jo.hash_bits = o.hash_bits;
    u64 n_null[2] = {0, 0};
    RC_TRY(join_str(c, build, probe, flags, &jo, out, vb, vp, n_null));
    o.n_build_null = n_null[0];
    o.n_probe_null = n_null[1];
    o.n_hash_pairs = jo.n_hash_pairs;
    o.n_collisions = jo.n_collisions;
    if (c->profiling) {
      (void)hipStreamSynchronize(c->stream);
      o.ms_hash = elapsed(c->str_ws.ev, 0, 1);
      o.ms_join = elapsed(c->str_ws.ev, 1, 2);
      o.ms_verify = elapsed(c->str_ws.ev, 2, 3);
      o.ms_order = elapsed(c->str_ws.ev, 3, 4);
    }
  } else {
    RC_TRY(join_str_kind(c, build, probe, flags, &o, out, vb, vp));
    if (c->profiling) {
      (void)hipStreamSynchronize(c->stream);
      o.ms_hash = elapsed(c->str_ws.ev, 0, 1);
      o.ms_join = elapsed(c->str_ws.ev, 1, 2);
      o.ms_verify = elapsed(c->str_ws.ev, 2, 3);
      o.ms_emit = elapsed(c->str_ws.ev, 3, 4);
      o.ms_order = elapsed(c->str_ws.ev, 4, 5);
    }
  }
  const uint32_t room = opts->struct_size < sizeof(o) ? opts->struct_size : (uint32_t)sizeof(o);
  o.struct_size = opts->struct_size;
  std::memcpy(opts, &o, room);
  return HMJ_OK;
}

}  // extern "C"
