// The driver of the keyed joins: the string-key join (strjoin.hip, a tuple of one string column), the multi-column join of
// fixed-width columns (coljoin.hip) and the mixed-key join of string and fixed-width columns (mixjoin.hip).  All three turn
// every row into a {key64, row} row, run the u64 join on those rows and finish on hmj_keyjoin.h's kernels; tuple_join (the
// inner join) and tuple_join_kind (the join kinds) are that sequence once, as templates over a policy P the including file
// defines:
//   P::Side                    the relation-side struct with its key_eq / key_cmp / payload overloads (hmj_keyjoin.h)
//   P::kCanPack                the key may be the packed tuple itself (the call says so: TupleCall::hashed == false)
//   P::kAccExtra               u64 words the key kernels own behind the call's accumulator blocks (tuple_acc_extra)
//   P::kMemoInner / kMemoProbeRep / kMemoBuildRep / kMemoAmbiguous / kMemoPairs   workload_signature kinds of the u64 joins
//   P::names() / P::ws(c)      what error messages call the join; the workspace of the entry
//   P::key(c, A, rel, n, call, out, sum_probe, acc)                          {key64,row} rows of a relation without bitmaps
//   P::key_valid(c, A, V, rel, n, call, nblk, dense, comp, cap, off, sum_probe, acc)   ... of one with bitmaps (pass 2)
//   P::keys_begin(c) / P::keys_check(c, call)   before the first key kernel (the call's blocks and P's words are zero:
//                                         presets the words that start elsewhere) / behind the last: where a key kernel
//                                         that checks its input (string offsets) reports, and where the NULL-equals-NULL
//                                         key kernels' counts of rows with NULL slots reach call->n_*_null; the plain
//                                         fixed-width policy does nothing in either
//   P::gather(...)             kCanPack only: the packed form's payload gather
// A relation with bitmaps is keyed in one sequence for every policy (launch_key_valid: count, scan, key_valid with room for
// every row; keys_end reads the valid-row totals once, behind the key phase).
// Also here: what the key kernels share -- col_load, the per-column validity bitmaps (ColValid / row_valid, and for the
// NULL-equals-NULL policies slot_null / wave_valid_word), kGolden.
// Internal header: its contents are local to the file that includes it.
#pragma once
#include "hmj_keyjoin.h"

namespace {

constexpr int kMaxCols = HMJ_MAX_KEY_COLS;
constexpr u64 kGolden = 0x9E3779B97F4A7C15ull;
constexpr int kKindAccBlocks = 3;  // acc: [0] keys, verification, collision search, [1] probe sweep, [2] build sweep

__device__ __forceinline__ u32 uniform(u32 v) { return __builtin_amdgcn_readfirstlane(v); }

// column value of row i, zero-extended (w is uniform: a scalar branch)
__device__ __forceinline__ u64 col_load(const void* p, u32 w, u64 i) {
  switch (w) {
    case 1: return (u64) reinterpret_cast<const unsigned char*>(p)[i];
    case 2: return (u64) reinterpret_cast<const unsigned short*>(p)[i];
    case 4: return (u64) reinterpret_cast<const u32*>(p)[i];
    default: return reinterpret_cast<const u64*>(p)[i];
  }
}

// ---- NULL keys (validity bitmaps) ------------------------------------------------------------------------------------------
// One relation's Arrow validity bitmaps, passed by value like the Side: bits[c] == NULL: column c holds no NULL.  Row i is
// valid in column c iff bit off[c] + i (least-significant bit first) is set; a row is a NULL-key row when any column's is not.
struct ColValid {
  const unsigned char* bits[kMaxCols];
  u64 off[kMaxCols];
  u32 k;
};
__device__ __forceinline__ bool row_valid(const ColValid& V, u64 i) {
  bool ok = true;
#pragma unroll
  for (int c = 0; c < kMaxCols; c++) {
    if (c < (int)V.k && V.bits[c]) {  // (uniform)
      const u64 b = V.off[c] + i;
      ok = ok && ((V.bits[c][b >> 3] >> (b & 7)) & 1u);
    }
  }
  return ok;
}

// NULL-equals-NULL matching (HMJ_NULL_EQUAL): a NULL slot is a value of its own, so the bitmaps are read per column.
// slot_null: row i is NULL in column c (one lane, any row: the comparisons of the shared kernels).
__device__ __forceinline__ bool slot_null(const ColValid& V, int c, u64 i) {
  const unsigned char* bits = V.bits[c];
  if (!bits) return false;
  const u64 b = V.off[c] + i;
  return !((bits[b >> 3] >> (b & 7)) & 1u);
}
// The validity bits of rows [i0, i0 + cnt) of one column (1 <= cnt <= 64; row i0 + j at bit j; the bits from cnt on mean
// nothing), for a wave that keys 64 consecutive rows: every argument is wave-uniform, so the one or two aligned 8-byte words
// that hold the bits are loaded once per wave.  Only words that hold a wanted bit are read -- an aligned word that shares a
// byte with the bitmap lies in the bitmap's pages, as bytes_cmp's words do (hmj_strkey.h).
__device__ __forceinline__ u64 wave_valid_word(const unsigned char* bits, u64 off, u64 i0, u32 cnt) {
  const u64 b0 = off + i0;
  const uintptr_t at = (uintptr_t)bits + (uintptr_t)(b0 >> 3), base = at & ~(uintptr_t)7;
  const u32 sh = (u32)((at - base) << 3) + (u32)(b0 & 7);  // 0..63: the first wanted bit inside the first word
  const u64* wp = reinterpret_cast<const u64*>(base);
  u64 word = wp[0] >> sh;
  if (sh + cnt > 64u) word |= wp[1] << (64u - sh);  // (sh > 0 here)
  return word;
}
__device__ __forceinline__ u64 uniform64(u64 v) {
  return ((u64)uniform((u32)(v >> 32)) << 32) | (u64)uniform((u32)v);
}
// Where the NULL-equals-NULL key kernels count a relation's rows with a NULL slot: one atomic per workgroup, spread by
// workgroup index over kNullSlots words that lie kNullStride words (one 128-byte line) apart -- one word takes about 88
// atomics per microsecond, which 65536 workgroups of a 2^24-row relation would wait 0.7 ms for.  The host adds the slots up.
constexpr int kNullSlots = 32, kNullStride = 16;
constexpr int kNullWords = kNullSlots * kNullStride;
__device__ __forceinline__ void count_null_rows(u64* __restrict__ slots, u64 t) {
  if (t) atomicAdd(&slots[(blockIdx.x & (u32)(kNullSlots - 1)) * kNullStride], t);
}
inline u64 null_rows_of(const u64* slots) {
  u64 t = 0;
  for (int k = 0; k < kNullSlots; k++) t += slots[k * kNullStride];
  return t;
}

// ---- host side -----------------------------------------------------------------------------------------------------------
// One call as the driver sees it.  in: the join key's form, the kind and its fills; out: what the entries report.
struct TupleCall {
  bool hashed = true;  // key64 is the hash chain (false: the packed tuple; P::kCanPack only)
  u32 bits = 0;        // hash_bits (hashed only)
  u32 side = 0, kind = 0;
  u64 probe_fill = 0, build_fill = 0;
  u64 n_key_pairs = 0, n_collisions = 0, n_build_null = 0, n_probe_null = 0;
  hmj_kind_counts counts{};
};

// the words P's key kernels own in the workspace's accumulator: behind the call's blocks, cleared with them
template <class P>
u64* tuple_acc_extra(hmj_ctx* c) {
  return (u64*)P::ws(c).acc.p + kKindAccBlocks * KA_N;
}
template <class P>
constexpr size_t tuple_acc_bytes() {
  return (kKindAccBlocks * KA_N + P::kAccExtra) * sizeof(u64);
}

// The {key64,row} rows of one relation (rel: 0 build, 1 probe) in a call with bitmaps.  dense: the relation's row-indexed
// rows (NULL: not wanted); *rows: what the u64 joins take; *tot: where on the device the number of those rows stands (NULL:
// every row).  A relation with a bitmap: its valid rows counted per workgroup (vblk: nblk counts, then nblk + 1 offsets) and
// compacted into cmp, which has room for every row: nothing is read back between the passes (keys_end fetches the totals).
// A relation without one goes through P::key as always, and its dense rows are its join rows.
template <class P>
int launch_key_valid(hmj_ctx* c, const typename P::Side& A, const ColValid& V, bool has, int rel, u64 n, const TupleCall& call, u64* dense,
                     u64* plain, DevBuf& cmp, u64* vblk, bool sum_probe, u64* acc, const void** rows, const u64** tot) {
  *rows = plain;
  *tot = nullptr;
  if (!has || !n) return P::key(c, A, rel, n, call, plain, sum_probe, acc);
  const u64 nblk = blocks_of(n);
  char msg[96];
  std::snprintf(msg, sizeof(msg), "%s: too many rows", P::names().join);
  if (nblk > 0xFFFFFFFFull) return fail(c, HMJ_E_ARG, msg);
  u64 *cnt = vblk, *off = vblk + nblk;
  RC_TRY(ensure_dev(c, cmp, 16 * n));
  hipLaunchKernelGGL(valid_count_kernel<ColValid>, dim3((u32)nblk), dim3(KJ_THREADS), 0, c->stream, V, n, cnt);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hmj::launch_scan_u64(cnt, off, (u32)nblk, c->stream));
  RC_TRY(P::key_valid(c, A, V, rel, n, call, nblk, dense, (u64*)cmp.p, n, (const u64*)off, sum_probe, acc));
  *rows = cmp.p;
  *tot = off + nblk;
  return HMJ_OK;
}

// Both relations' {key64,row} rows in a call with bitmaps (the block counts of both sides share vblk).
template <class P>
int launch_keys_valid(hmj_ctx* c, const typename P::Side& RS, const typename P::Side& SS, const ColValid* VB, const ColValid* VP, u64 nb,
                      u64 np, const TupleCall& call, bool dense, bool sum_probe, u64* acc, const void** rows_r, const u64** tot_b,
                      const void** rows_s, const u64** tot_p) {
  KeyJoinWs& ws = P::ws(c);
  const u64 kb = VB ? blocks_of(nb) : 0, kp = VP ? blocks_of(np) : 0;
  RC_TRY(ensure_dev(c, ws.vblk, (2 * (kb + kp) + 2) * sizeof(u64)));
  u64* vblk = (u64*)ws.vblk.p;
  const ColValid none{};
  u64 *plain_r = (u64*)ws.rows_r.p, *plain_s = (u64*)ws.rows_s.p;
  RC_TRY(launch_key_valid<P>(c, RS, VB ? *VB : none, VB != nullptr, 0, nb, call, dense ? plain_r : nullptr, plain_r, ws.cmp_r, vblk,
                             false, acc, rows_r, tot_b));
  RC_TRY(launch_key_valid<P>(c, SS, VP ? *VP : none, VP != nullptr, 1, np, call, dense ? plain_s : nullptr, plain_s, ws.cmp_s,
                             vblk + 2 * kb + 1, sum_probe, acc, rows_s, tot_p));
  return HMJ_OK;
}

// Behind the key phase: P's verdict on its input, then -- a call with bitmaps (tot_b / tot_p as launch_key_valid left
// them) -- the rows of each relation that have a key, into *nvb / *nvp and call->n_*_null.  The totals' copies are queued
// in front of keys_check, so a policy that reads its report words back fetches them in the same synchronisation.
template <class P>
int keys_end(hmj_ctx* c, TupleCall* call, bool bitmaps, const u64* tot_b, const u64* tot_p, u64 nb, u64 np, u64* nvb, u64* nvp) {
  if (tot_b) HIP_TRY(hipMemcpyAsync(nvb, tot_b, sizeof(u64), hipMemcpyDeviceToHost, c->stream));
  if (tot_p) HIP_TRY(hipMemcpyAsync(nvp, tot_p, sizeof(u64), hipMemcpyDeviceToHost, c->stream));
  const int rc = P::keys_check(c, call);
  if (tot_b || tot_p) HIP_TRY(hipStreamSynchronize(c->stream));  // (the totals are on the host whatever keys_check did)
  RC_TRY(rc);
  if (!bitmaps) return HMJ_OK;
  char msg[96];
  std::snprintf(msg, sizeof(msg), "%s: more valid rows counted than the relation holds", P::names().join);
  if (*nvb > nb || *nvp > np) return fail(c, HMJ_E_HIP, msg);
  call->n_build_null = nb - *nvb;
  call->n_probe_null = np - *nvp;
  return HMJ_OK;
}

// The inner join.  RS / SS: the relations (nb / np rows); VB / VP: their validity bitmaps, NULL where a relation has none
// (both NULL: the call without NULL keys).  call: form in, n_key_pairs / n_collisions / n_*_null out.
template <class P>
int tuple_join(hmj_ctx* c, const typename P::Side& RS, u64 nb, const typename P::Side& SS, u64 np, uint32_t flags, TupleCall* call,
               hmj_cols_result* out, const ColValid* VB, const ColValid* VP) {
  using Side = typename P::Side;
  const bool hashed = call->hashed;
  if (flags & HMJ_ORDERED) flags |= HMJ_MATERIALIZE;
  const bool mat = flags & HMJ_MATERIALIZE, ordered = flags & HMJ_ORDERED, checksum = flags & HMJ_CHECKSUM;
  c->prep.valid = false;  // like any other call, the join discards a prepared build side
  KeyJoinWs& ws = P::ws(c);
  RC_TRY(ensure_dev(c, ws.acc, tuple_acc_bytes<P>()));
  RC_TRY(ensure_dev(c, ws.rows_r, 16 * (nb ? nb : 1)));
  RC_TRY(ensure_dev(c, ws.rows_s, 16 * (np ? np : 1)));
  u64* acc = (u64*)ws.acc.p;
  u64 h[KA_N];
  // 1. {key64, row} rows of both relations (+ the probe payloads' sum)
  RC_TRY(ws.ev.record(c, 0));
  HIP_TRY(hipMemsetAsync(acc, 0, tuple_acc_bytes<P>(), c->stream));
  RC_TRY(P::keys_begin(c));
  const void *rows_r = ws.rows_r.p, *rows_s = ws.rows_s.p;  // the rows the u64 join takes
  u64 nvb = nb, nvp = np;                                   // ... and how many: the rows that have a key
  const u64 *tot_b = nullptr, *tot_p = nullptr;
  if (!VB && !VP) {
    RC_TRY(P::key(c, RS, 0, nb, *call, (u64*)ws.rows_r.p, false, acc));
    RC_TRY(P::key(c, SS, 1, np, *call, (u64*)ws.rows_s.p, flags & HMJ_SUM_PROBE, acc));
  } else {  // NULL keys: only the rows that have a key are joined (the inner join walks no relation by row: no dense rows)
    RC_TRY(launch_keys_valid<P>(c, RS, SS, VB, VP, nb, np, *call, false, flags & HMJ_SUM_PROBE, acc, &rows_r, &tot_b, &rows_s, &tot_p));
  }
  RC_TRY(ws.ev.record(c, 1));
  RC_TRY(keys_end<P>(c, call, VB || VP, tot_b, tot_p, nb, np, &nvb, &nvp));
  if (nvb == 0 || nvp == 0) {  // (nothing to join: no plan either)
    std::memset(&c->plan, 0, sizeof(c->plan));
    c->plan.struct_size = sizeof(c->plan);
    std::memset(&c->timing, 0, sizeof(c->timing));
    for (int k = 2; k < 5; k++) RC_TRY(ws.ev.record(c, k));
    if (flags & HMJ_SUM_PROBE) {
      RC_TRY(read_back(c, acc, h, sizeof(h)));
      out->sum_probe_all = h[KA_SUM_P];
    }
    return HMJ_OK;
  }
  // 2. the u64 join of the {key64, row} rows: pairs of equal key64 as (key64, r_row, s_row), ordered by them if asked
  hmj_result inner;
  RC_TRY(memo_join(c, rows_r, nvb, rows_s, nvp, HMJ_MATERIALIZE | (flags & HMJ_ORDERED), P::kMemoInner, &inner));
  RC_TRY(ws.ev.record(c, 2));
  const u64 n_pairs = inner.n_matches;
  call->n_key_pairs = n_pairs;
  const u64 *ik = (const u64*)inner.key, *ir = (const u64*)inner.rval, *is = (const u64*)inner.sval;
  const u64 nblk = blocks_of(n_pairs);
  if (nblk > 0xFFFFFFFFull) return too_many_pairs(c, P::names());
  u64 n_out = 0;
  if (!hashed) {
    // 3a. packed: every pair is a result row; payloads gathered, or only reduced
    if constexpr (P::kCanPack) {
      if (n_pairs && mat) {
        RC_TRY(ensure_dev(c, ws.rval, n_pairs * sizeof(u64)));
        RC_TRY(ensure_dev(c, ws.sval, n_pairs * sizeof(u64)));
      }
      if (n_pairs)
        RC_TRY(P::gather(c, mat, false, nblk, ik, ir, is, n_pairs, RS, SS, mat ? (u64*)ws.rval.p : nullptr, mat ? (u64*)ws.sval.p : nullptr, acc,
                         checksum, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr));
    }
    n_out = n_pairs;
    RC_TRY(ws.ev.record(c, 3));
  } else {
    // 3b. hashed: tuple verification, payload gather, stable compaction (or the count modes' reduction)
    if (n_pairs && mat) {
      RC_TRY(ensure_dev(c, ws.flags, nblk * KJ_WAVES * sizeof(u64)));
      RC_TRY(ensure_dev(c, ws.blk, nblk * sizeof(u64)));
      RC_TRY(ensure_dev(c, ws.blk_off, (nblk + 1) * sizeof(u64)));
      DevBuf* cols[5] = {&ws.key, &ws.rrow, &ws.srow, &ws.rval, &ws.sval};
      for (DevBuf* b : cols) RC_TRY(ensure_dev(c, *b, n_pairs * sizeof(u64)));
      hipLaunchKernelGGL((verify_kernel<Side, true>), dim3((u32)nblk), dim3(KJ_THREADS), 0, c->stream, ik, ir, is, n_pairs, RS, SS,
                         (u64*)ws.flags.p, (u64*)ws.blk.p, acc, 0, nullptr, nullptr);
      HIP_TRY(hipGetLastError());
      HIP_TRY(hmj::launch_scan_u64((const u64*)ws.blk.p, (u64*)ws.blk_off.p, (u32)nblk, c->stream));
      hipLaunchKernelGGL(compact_kernel<Side>, dim3((u32)nblk), dim3(KJ_THREADS), 0, c->stream, ik, ir, is, n_pairs, RS, SS,
                         (const u64*)ws.flags.p, (const u64*)ws.blk_off.p, (u64*)ws.key.p, (u64*)ws.rrow.p,
                         (u64*)ws.srow.p, (u64*)ws.rval.p, (u64*)ws.sval.p, acc, checksum ? 1 : 0);
      HIP_TRY(hipGetLastError());
      RC_TRY(read_back(c, (const u64*)ws.blk_off.p + nblk, &n_out, sizeof(u64)));
    } else if (n_pairs) {
      hipLaunchKernelGGL((verify_kernel<Side, false>), dim3((u32)nblk), dim3(KJ_THREADS), 0, c->stream, ik, ir, is, n_pairs, RS, SS,
                         nullptr, nullptr, acc, checksum ? 1 : 0, nullptr, nullptr);
      HIP_TRY(hipGetLastError());
    }
    RC_TRY(ws.ev.record(c, 3));
    // 4. ordered: runs of equal key64 with different build tuples, sorted by the tuple
    if (ordered && n_out > 1) {
      u64* cols[5] = {(u64*)ws.key.p, (u64*)ws.rrow.p, (u64*)ws.srow.p, (u64*)ws.rval.p, (u64*)ws.sval.p};
      RC_TRY(order_collisions<false>(c, ws, RS, Side{}, cols, n_out, acc));
    }
  }
  RC_TRY(ws.ev.record(c, 4));
  RC_TRY(read_back(c, acc, h, sizeof(h)));
  RC_TRY(collision_errors(c, P::names(), h[KA_ERR]));
  const u64* a = h + KA_ACC;
  out->n_matches = (hashed && mat) ? n_out : a[hmj::ACC_N];
  out->sum_r = a[hmj::ACC_SUM_R];
  out->sum_s = a[hmj::ACC_SUM_S];
  if (checksum) {
    out->xor_fold = a[hmj::ACC_XOR];
    out->mix_sum = a[hmj::ACC_MIX];
  }
  if (flags & HMJ_SUM_PROBE) out->sum_probe_all = h[KA_SUM_P];
  if (mat && !hashed) {
    out->key64 = (const uint64_t*)ik;
    out->r_row = (const uint64_t*)ir;
    out->s_row = (const uint64_t*)is;
    out->rval = (const uint64_t*)ws.rval.p;
    out->sval = (const uint64_t*)ws.sval.p;
  } else if (mat) {
    out->key64 = (const uint64_t*)ws.key.p;
    out->r_row = (const uint64_t*)ws.rrow.p;
    out->s_row = (const uint64_t*)ws.srow.p;
    out->rval = (const uint64_t*)ws.rval.p;
    out->sval = (const uint64_t*)ws.sval.p;
  }
  call->n_collisions = n_pairs - out->n_matches;
  return HMJ_OK;
}

// ---- join kinds ----------------------------------------------------------------------------------------------------------
// Every kind but the probe side's INNER (which is tuple_join).  call: form, side, kind and fills in; counts, n_key_pairs,
// n_collisions and n_*_null out.
template <class P>
int tuple_join_kind(hmj_ctx* c, const typename P::Side& RS, u64 nb, const typename P::Side& SS, u64 np, uint32_t flags, TupleCall* o,
                    hmj_cols_result* out, const ColValid* VB, const ColValid* VP) {
  using Side = typename P::Side;
  const u32 kind = o->kind;
  const bool hashed = o->hashed;
  if (flags & HMJ_ORDERED) flags |= HMJ_MATERIALIZE;
  const bool mat = flags & HMJ_MATERIALIZE, checksum = flags & HMJ_CHECKSUM;
  const bool bside = o->side == HMJ_KIND_BUILD_SIDE;
  // semi / anti of either side (HMJ_JOIN_SEMI == HMJ_BUILD_SEMI, HMJ_JOIN_ANTI == HMJ_BUILD_ANTI), else an outer kind
  const bool semi_anti = kind == HMJ_JOIN_SEMI || kind == HMJ_JOIN_ANTI;
  c->prep.valid = false;  // like any other call, the join discards a prepared build side
  KeyJoinWs& ws = P::ws(c);
  std::memset(&c->plan, 0, sizeof(c->plan));
  c->plan.struct_size = sizeof(c->plan);
  std::memset(&c->timing, 0, sizeof(c->timing));
  RC_TRY(ensure_dev(c, ws.acc, tuple_acc_bytes<P>()));
  RC_TRY(ensure_dev(c, ws.rows_r, 16 * (nb ? nb : 1)));
  RC_TRY(ensure_dev(c, ws.rows_s, 16 * (np ? np : 1)));
  RC_TRY(ensure_dev(c, ws.mark_r, nb ? nb : 1));
  RC_TRY(ensure_dev(c, ws.mark_s, np ? np : 1));
  u64* acc = (u64*)ws.acc.p;
  u64 *acc_p = acc + KA_N, *acc_b = acc + 2 * KA_N;
  u64 h[kKindAccBlocks * KA_N];
  unsigned char *mark_r = (unsigned char*)ws.mark_r.p, *mark_s = (unsigned char*)ws.mark_s.p;
  // 1. {key64, row} rows of both relations (+ the probe payloads' sum), marks cleared
  RC_TRY(ws.ev.record(c, 0));
  HIP_TRY(hipMemsetAsync(acc, 0, tuple_acc_bytes<P>(), c->stream));
  RC_TRY(P::keys_begin(c));
  // (NULL keys: the dense rows stay indexed by row for the sweeps; the u64 joins take only the rows that have a key)
  const void *rows_r = ws.rows_r.p, *rows_s = ws.rows_s.p;
  u64 nvb = nb, nvp = np;
  const u64 *tot_b = nullptr, *tot_p = nullptr;
  if (!VB && !VP) {
    RC_TRY(P::key(c, RS, 0, nb, *o, (u64*)ws.rows_r.p, false, acc));
    RC_TRY(P::key(c, SS, 1, np, *o, (u64*)ws.rows_s.p, flags & HMJ_SUM_PROBE, acc));
  } else {
    RC_TRY(launch_keys_valid<P>(c, RS, SS, VB, VP, nb, np, *o, true, flags & HMJ_SUM_PROBE, acc, &rows_r, &tot_b, &rows_s, &tot_p));
  }
  if (nb) HIP_TRY(hipMemsetAsync(mark_r, 0, nb, c->stream));
  if (np) HIP_TRY(hipMemsetAsync(mark_s, 0, np, c->stream));
  RC_TRY(ws.ev.record(c, 1));
  RC_TRY(keys_end<P>(c, o, VB || VP, tot_b, tot_p, nb, np, &nvb, &nvp));
  // 2. + 3. the {key64,row} join(s) and the tuple verification, which marks the rows that have a partner
  u64 n_pairs = 0;
  hmj_result inner;
  std::memset(&inner, 0, sizeof(inner));
  if (semi_anti) {
    // every row of the side asked about (K) meets the FIRST row of its key64 on the other side (O), in row order
    const u64 nK = bside ? nvb : nvp, nO = bside ? nvp : nvb;
    const void *rowsK = bside ? rows_r : rows_s, *rowsO = bside ? rows_s : rows_r;
    const Side &KS = bside ? RS : SS, &OS = bside ? SS : RS;
    unsigned char* mark = bside ? mark_r : mark_s;
    if (nK && nO) {
      hmj_result rep;
      RC_TRY(memo_join(c, rowsO, nO, rowsK, nK, HMJ_MATERIALIZE | HMJ_FIRST_WINS, bside ? P::kMemoBuildRep : P::kMemoProbeRep, &rep));
      RC_TRY(ws.ev.record(c, 2));
      n_pairs = rep.n_matches;  // <= nK
      if (n_pairs && !hashed) {
        hipLaunchKernelGGL((rep_verify_kernel<Side, false>), dim3((u32)blocks_of(n_pairs)), dim3(KJ_THREADS), 0, c->stream,
                           (const u64*)rep.key, (const u64*)rep.rval, (const u64*)rep.sval, n_pairs, OS, KS, mark, nullptr, acc);
        HIP_TRY(hipGetLastError());
      } else if (n_pairs) {
        RC_TRY(ensure_dev(c, ws.amb, 16 * n_pairs));
        hipLaunchKernelGGL((rep_verify_kernel<Side, true>), dim3((u32)blocks_of(n_pairs)), dim3(KJ_THREADS), 0, c->stream,
                           (const u64*)rep.key, (const u64*)rep.rval, (const u64*)rep.sval, n_pairs, OS, KS, mark,
                           (u64*)ws.amb.p, acc);
        HIP_TRY(hipGetLastError());
        RC_TRY(read_back(c, acc, h, KA_N * sizeof(u64)));
        const u64 n_amb = h[KA_AMB_N];
        if (n_amb) {  // (a collision: a representative's tuple differs from the row's)
          hmj_result all;
          RC_TRY(memo_join(c, rowsO, nO, ws.amb.p, n_amb, HMJ_MATERIALIZE, P::kMemoAmbiguous, &all));
          n_pairs += all.n_matches;
          if (blocks_of(all.n_matches) > 0xFFFFFFFFull) return too_many_pairs(c, P::names());
          if (all.n_matches) {
            hipLaunchKernelGGL((rep_verify_kernel<Side, true>), dim3((u32)blocks_of(all.n_matches)), dim3(KJ_THREADS), 0, c->stream,
                               (const u64*)all.key, (const u64*)all.rval, (const u64*)all.sval, all.n_matches, OS, KS, mark, nullptr,
                               acc);
            HIP_TRY(hipGetLastError());
          }
        }
      }
    } else {
      RC_TRY(ws.ev.record(c, 2));
    }
  } else if (nvb && nvp) {
    RC_TRY(memo_join(c, rows_r, nvb, rows_s, nvp, HMJ_MATERIALIZE | (flags & HMJ_ORDERED), P::kMemoPairs, &inner));
    RC_TRY(ws.ev.record(c, 2));
    n_pairs = inner.n_matches;
  } else {
    RC_TRY(ws.ev.record(c, 2));
  }
  o->n_key_pairs = n_pairs;
  KindRows k;
  RC_TRY(kind_rows(c, ws, P::names(), o->side, kind, flags, nb, np, nvb, nvp, VB != nullptr, VP != nullptr, n_pairs, &k));
  const u64* pairs[3] = {(const u64*)inner.key, (const u64*)inner.rval, (const u64*)inner.sval};
  u64* blk = (u64*)ws.blk.p;
  if (k.nblk_v && !hashed) {  // packed: every pair is a result row and marks its two rows
    if constexpr (P::kCanPack)
      RC_TRY(P::gather(c, mat, true, k.nblk_v, pairs[0], pairs[1], pairs[2], n_pairs, RS, SS, mat ? k.oc[3] : nullptr,
                       mat ? k.oc[4] : nullptr, acc, checksum, mark_r, mark_s, k.oc[0], k.oc[1], k.oc[2], blk));
  } else if (k.nblk_v) {  // hashed: the surviving pairs mark theirs
    if (mat)
      hipLaunchKernelGGL((verify_kernel<Side, true, true>), dim3((u32)k.nblk_v), dim3(KJ_THREADS), 0, c->stream, pairs[0], pairs[1],
                         pairs[2], n_pairs, RS, SS, (u64*)ws.flags.p, blk, acc, 0, mark_r, mark_s);
    else
      hipLaunchKernelGGL((verify_kernel<Side, false, true>), dim3((u32)k.nblk_v), dim3(KJ_THREADS), 0, c->stream, pairs[0], pairs[1],
                         pairs[2], n_pairs, RS, SS, nullptr, nullptr, acc, checksum ? 1 : 0, mark_r, mark_s);
    HIP_TRY(hipGetLastError());
  }
  RC_TRY(ws.ev.record(c, 3));
  // 4. the sweeps (hashed: the pairs' survivors compacted in front of them), 5. ordered: the sort by key64, then -- hashed
  // only: packed, equal key64 is equal tuples, so there is no collision to search for -- runs of equal key64 with several
  // tuples sorted by tuple
  RC_TRY(kind_sweeps(c, ws, P::names(), k, RS, SS, o->probe_fill, o->build_fill, hashed, pairs, acc, acc_p, acc_b));
  RC_TRY(ws.ev.record(c, 4));
  RC_TRY(kind_order(c, ws, k, RS, SS, hashed, acc));
  RC_TRY(ws.ev.record(c, 5));
  RC_TRY(read_back(c, acc, h, sizeof(h)));
  RC_TRY(collision_errors(c, P::names(), h[KA_ERR]));
  kind_report(k, h + KA_ACC, h + KA_N + KA_ACC, h + 2 * KA_N + KA_ACC, out, &o->counts);
  if (flags & HMJ_SUM_PROBE) out->sum_probe_all = h[KA_SUM_P];
  if (mat) out->key64 = (const uint64_t*)k.oc[0];
  o->n_collisions = semi_anti ? h[KA_DIFF] : n_pairs - k.n_in;
  return HMJ_OK;
}

}  // namespace
