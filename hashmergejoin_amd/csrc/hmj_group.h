// Grouping rows by key (hmj_group_cols_device, coljoin.hip; hmj_group_mixed_device, mixjoin.hip): what follows the key
// kernel and the stable u64 sort of the {key64, row} rows -- the collision sort on 16-byte rows, the group heads, the group
// columns and the aggregates -- as templates over the relation-side struct of the including file, with hmj_keyjoin.h's key
// policy (key_eq / key_cmp / payload overloads next to the Side), and group_rows, the host sequence of both entries behind
// their argument checks.  Internal header: its contents are local to the file that includes it.
// Kernels (KJ_THREADS lanes per workgroup; `rows` are the sorted {key64, row} rows, n of them):
//   group_mismatch_kernel / group_run_leader_kernel / group_run_sort_kernel   hashed keys: runs of equal key64 that hold
//                          several keys are sorted by (key, row), each in one workgroup (hmj_keyjoin.h's collision order on
//                          16-byte rows).  Afterwards the rows of one group are contiguous and ascending by row.
//   group_heads_kernel     one lane per sorted position: a head is a position whose key differs from its predecessor's.  A
//                          wave's ballot is 64 head bits (flags, one word per wave); heads per workgroup go to blk_cnt.
//   group_emit_kernel      group index = heads at or in front of a position - 1.  A head writes key64 / first_row / start and
//                          clears its aggregate slots; every position writes group_of_row[row].
//   group_count_kernel     one lane per group: count = start[g + 1] - start[g]; the largest count by one atomic per workgroup.
//   group_agg_kernel       sum / min / max of the payloads: a segmented scan by the head bits inside each wave; a group that
//                          lies inside one wave's range is stored, one that crosses it is finished by one atomic per wave.
#pragma once
#include "hmj_tuplejoin.h"

namespace {

// acc words of a group call behind hmj_keyjoin.h's KA_LIST_N / KA_ERR: heads that follow a row of equal key64, the largest
// group's rows; from GA_NULL on the column key kernel's kNullWords words (count_null_rows); behind GA_N the words of
// group_rows' Check, if any
enum { GA_COLL = KA_ACC, GA_MAXC = KA_ACC + 1, GA_NULL = KA_N, GA_N = KA_N + kNullWords };

// Row i of the sorted rows whose key64 equals row i-1's but whose key differs is recorded (mismatch_kernel's test).
template <class Side>
__global__ __launch_bounds__(KJ_THREADS) void group_mismatch_kernel(const ulonglong2* __restrict__ rows, u64 n, Side A,
                                                                    u64* __restrict__ list, u64* __restrict__ acc) {
  const u64 i = (u64)blockIdx.x * KJ_THREADS + threadIdx.x + 1;
  if (i >= n) return;
  const ulonglong2 a = rows[i - 1], b = rows[i];
  if (a.x != b.x) return;
  if (key_eq(A, a.y, A, b.y)) return;
  const u64 k = atomicAdd(&acc[KA_LIST_N], 1ull);
  if (k < kListCap) list[k] = i;
  else atomicOr(&acc[KA_ERR], 2ull);
}

// run_leader_kernel on 16-byte rows: the recorded row that is the first mismatch of its run [s, e) of equal key64 leads it;
// a run beyond kRunCap rows raises acc[KA_ERR] bit 0.  A launch of its own, so that no leader test reads rows that a sort
// is moving.
template <class Side>
__global__ __launch_bounds__(KJ_THREADS) void group_run_leader_kernel(const ulonglong2* __restrict__ rows, u64 n, Side A,
                                                                      const u64* __restrict__ list, u64* __restrict__ runs,
                                                                      u64* __restrict__ acc) {
  const u64 cnt = acc[KA_LIST_N] < kListCap ? acc[KA_LIST_N] : kListCap;
  for (u64 k = (u64)blockIdx.x * KJ_THREADS + threadIdx.x; k < cnt; k += (u64)gridDim.x * KJ_THREADS) {
    const u64 i = list[k];
    runs[2 * k] = 0;
    runs[2 * k + 1] = 0;
    if (i == 0 || i >= n) continue;  // (never recorded)
    const u64 h = rows[i].x;
    u64 lo = 0, hi = i;  // first row with key64 h
    while (lo < hi) {
      const u64 mid = (lo + hi) >> 1;
      if (rows[mid].x < h) lo = mid + 1;
      else hi = mid;
    }
    const u64 s = lo;
    lo = i + 1;
    hi = n;  // first row past the run
    while (lo < hi) {
      const u64 mid = (lo + hi) >> 1;
      if (rows[mid].x <= h) lo = mid + 1;
      else hi = mid;
    }
    const u64 e = lo;
    if (e - s > (u64)kRunCap) {
      atomicOr(&acc[KA_ERR], 1ull);
      continue;
    }
    bool first = true;
    for (u64 t = s + 1; t < i && first; t++)
      if (!key_eq(A, rows[t - 1].y, A, rows[t].y)) first = false;
    if (first) {
      runs[2 * k] = s;
      runs[2 * k + 1] = e;
    }
  }
}

// One workgroup per led run: its rows sorted by (key, row) in place.  The run arrives ascending by row (the u64 sort is
// stable), so rank = rows with a smaller key + rows in front with the same key keeps the rows of one key ascending.
template <class Side>
__global__ __launch_bounds__(KJ_THREADS) void group_run_sort_kernel(const u64* __restrict__ runs, Side A, ulonglong2* __restrict__ rows,
                                                                    const u64* __restrict__ acc) {
  __shared__ u64 row[kRunCap];
  __shared__ u32 rank[kRunCap];
  const u64 cnt = acc[KA_LIST_N] < kListCap ? acc[KA_LIST_N] : kListCap;
  for (u64 k = blockIdx.x; k < cnt; k += gridDim.x) {
    const u64 s = runs[2 * k], e = runs[2 * k + 1];
    if (e <= s || e - s > (u64)kRunCap) continue;  // (uniform: not a leader)
    const u32 L = (u32)(e - s);
    const u64 h = rows[s].x;
    for (u32 t = threadIdx.x; t < L; t += KJ_THREADS) row[t] = rows[s + t].y;
    __syncthreads();
    for (u32 t = threadIdx.x; t < L; t += KJ_THREADS) {
      u32 rk = 0;
      const u64 me = row[t];
      for (u32 o = 0; o < L; o++) {
        const int cm = o == t ? 0 : key_cmp(A, row[o], A, me);
        rk += (cm < 0 || (cm == 0 && o < t)) ? 1u : 0u;
      }
      rank[t] = rk;
    }
    __syncthreads();
    for (u32 t = threadIdx.x; t < L; t += KJ_THREADS) rows[s + rank[t]] = make_ulonglong2(h, row[t]);
    __syncthreads();
  }
}

// One lane per sorted position, one workgroup per KJ_THREADS positions.  Position i is a head when i == 0, key64[i] !=
// key64[i - 1], or -- HASHED -- the two rows' keys differ (both rows' columns are gathered).  Position i - 1's row comes from
// the neighbouring lane; lane 0 of a wave loads it.  flags: one ballot word per wave of the grid (0 behind n); blk_cnt: heads
// per workgroup; acc[GA_COLL]: heads that follow a row of equal key64.
template <class Side, bool HASHED>
__global__ __launch_bounds__(KJ_THREADS) void group_heads_kernel(const ulonglong2* __restrict__ rows, u64 n, Side A,
                                                                 u64* __restrict__ flags, u64* __restrict__ blk_cnt,
                                                                 u64* __restrict__ acc) {
  __shared__ u32 wcnt[KJ_WAVES], wcol[KJ_WAVES];
  const u64 i = (u64)blockIdx.x * KJ_THREADS + threadIdx.x;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  ulonglong2 e = make_ulonglong2(0, 0);
  if (i < n) e = rows[i];
  u64 pk = __shfl_up(e.x, 1, 64), pr = __shfl_up(e.y, 1, 64);  // (every lane of the wave takes part)
  if (lane == 0 && i > 0 && i < n) {
    const ulonglong2 p = rows[i - 1];
    pk = p.x;
    pr = p.y;
  }
  bool head = false, coll = false;
  if (i < n) {
    if (i == 0 || e.x != pk) head = true;
    else if (HASHED && !key_eq(A, pr, A, e.y)) head = coll = true;
  }
  const u64 m = __ballot(head), mc = __ballot(coll);
  if (lane == 0) {
    flags[i >> 6] = m;
    wcnt[w] = (u32)__builtin_popcountll(m);
    wcol[w] = (u32)__builtin_popcountll(mc);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    u64 t = 0, tc = 0;
    for (int k = 0; k < KJ_WAVES; k++) {
      t += wcnt[k];
      tc += wcol[k];
    }
    blk_cnt[blockIdx.x] = t;
    if (tc) atomicAdd(&acc[GA_COLL], tc);
  }
}

// The heads in front of the wave of position i (a multiple of 64 behind its workgroup's first position): the workgroup's
// offset plus the ballots of its earlier waves.
__device__ __forceinline__ u64 group_wave_base(const u64* __restrict__ flags, const u64* __restrict__ blk_off, int w) {
  u64 g = blk_off[blockIdx.x];
  const u64 f0 = ((u64)blockIdx.x * KJ_THREADS) >> 6;
  for (int k = 0; k < w; k++) g += (u64)__builtin_popcountll(flags[f0 + (u64)k]);
  return g;
}
__device__ __forceinline__ u64 lanes_through(int lane) { return lane == 63 ? ~0ull : ((2ull << lane) - 1ull); }

// One lane per sorted position (the grid of group_heads_kernel).  NULL columns are not written.  sum / mn / mx: the
// aggregate slots, cleared to the identity of their operation for group_agg_kernel.  start has ng + 1 entries.
__global__ __launch_bounds__(KJ_THREADS) void group_emit_kernel(const ulonglong2* __restrict__ rows, u64 n, u64 ng,
                                                                const u64* __restrict__ flags, const u64* __restrict__ blk_off,
                                                                u64* __restrict__ key, u64* __restrict__ first,
                                                                u64* __restrict__ start, u64* __restrict__ sum, u64* __restrict__ mn,
                                                                u64* __restrict__ mx, u64* __restrict__ gmap) {
  const u64 i = (u64)blockIdx.x * KJ_THREADS + threadIdx.x;
  if (i == 0) start[ng] = n;
  if (i >= n) return;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const u64 m = flags[i >> 6];
  const u64 at = group_wave_base(flags, blk_off, w) + (u64)__builtin_popcountll(m & lanes_through(lane));
  if (at == 0 || at > ng) return;  // (position 0 is always a head: never taken)
  const u64 g = at - 1;
  const ulonglong2 e = rows[i];
  if ((m >> lane) & 1ull) {
    start[g] = i;
    if (key) key[g] = e.x;
    if (first) first[g] = e.y;
    if (sum) sum[g] = 0ull;
    if (mn) mn[g] = ~0ull;
    if (mx) mx[g] = 0ull;
  }
  if (gmap && e.y < n) gmap[e.y] = g;
}

// One lane per group: its rows, and the largest group's into acc[GA_MAXC].
__global__ __launch_bounds__(KJ_THREADS) void group_count_kernel(const u64* __restrict__ start, u64 ng, u64* __restrict__ count,
                                                                 u64* __restrict__ acc) {
  __shared__ u64 red[KJ_WAVES];
  const u64 g = (u64)blockIdx.x * KJ_THREADS + threadIdx.x;
  u64 cnt = 0;
  if (g < ng) {
    cnt = start[g + 1] - start[g];
    if (count) count[g] = cnt;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const u64 t = __shfl_xor(cnt, o, 64);
    cnt = t > cnt ? t : cnt;
  }
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) {
    u64 t = 0;
    for (int k = 0; k < KJ_WAVES; k++) t = red[k] > t ? red[k] : t;
    if (t) atomicMax(&acc[GA_MAXC], t);
  }
}

// A group's partial result goes to its slots: added atomically where other waves may hold rows of the group, stored where
// the caller holds them all.
__device__ __forceinline__ void group_put(bool atomic, u64 g, u64 ng, u64 s, u64 lo, u64 hi, u64* __restrict__ sum, u64* __restrict__ mn,
                                          u64* __restrict__ mx) {
  if (g >= ng) return;
  if (atomic) {
    if (sum && s) atomicAdd(&sum[g], s);
    if (mn) atomicMin(&mn[g], lo);
    if (mx && hi) atomicMax(&mx[g], hi);
  } else {
    if (sum) sum[g] = s;
    if (mn) mn[g] = lo;
    if (mx) mx[g] = hi;
  }
}

// v = payload(A, row) of every sorted position, reduced per group.  A wave walks kAggChunks consecutive chunks of 64
// positions (one flags word each).  Inside a chunk the head bits cut the 64 lanes into segments; lane 0 starts one whether
// it is a head or not.  An inclusive segmented scan (six __shfl_up steps; a lane takes its partner's value only when the
// partner lies in its segment) leaves every segment's result in its last lane.  A segment between two heads of one chunk is
// its whole group: its last lane stores it.  The chunk's last segment is carried in (wave-uniform) registers into the next
// chunk, whose first segment continues it unless lane 0 is a head there; the carry is put down when its group ends.  What
// is stored and what is added atomically is decided from the ballots alone, the same in every lane: a group that was open
// at the left end of the wave's range (its first chunk's lane 0 is no head) or is still carried at the right end may hold
// rows of other waves -- one atomic per operation on the slots group_emit_kernel cleared; every other group lies inside the
// range and is stored.  No lane reads what another wave wrote.
constexpr int kAggChunks = 8;
template <class Side>
__global__ __launch_bounds__(KJ_THREADS) void group_agg_kernel(const ulonglong2* __restrict__ rows, u64 n, u64 ng, Side A,
                                                               const u64* __restrict__ flags, const u64* __restrict__ blk_off,
                                                               u64* __restrict__ sum, u64* __restrict__ mn, u64* __restrict__ mx) {
  const int lane = threadIdx.x & 63;
  const u64 nchunk = (n + 63) >> 6;
  const u64 c0 = uniform64((((u64)blockIdx.x * KJ_THREADS + threadIdx.x) >> 6) * (u64)kAggChunks);
  if (c0 >= nchunk) return;  // (wave-uniform)
  const u64 c1 = c0 + (u64)kAggChunks < nchunk ? c0 + (u64)kAggChunks : nchunk;
  // heads in front of chunk c0: its workgroup's offset in group_heads_kernel's grid plus the ballots of the chunks before it
  u64 heads = blk_off[c0 / KJ_WAVES];
  for (u64 k = (c0 / KJ_WAVES) * KJ_WAVES; k < c0; k++) heads += (u64)__builtin_popcountll(flags[k]);
  bool have = false, left_open = false;  // the carried group: heads - 1
  u64 cs = 0, clo = ~0ull, chi = 0;
  for (u64 ch = c0; ch < c1; ch++) {
    const u64 i0 = ch << 6;
    const u32 cnt = n - i0 < 64ull ? (u32)(n - i0) : 64u;  // the chunk's positions
    const bool active = (u32)lane < cnt;
    const u64 m = flags[ch];
    const bool head0 = m & 1ull;
    const u64 below = (m | 1ull) & lanes_through(lane);
    const int seg = 63 - __builtin_clzll(below);  // the lane's segment starts here
    u64 v = 0;
    if (active) {
      const u64 r = rows[i0 + (u64)lane].y;
      if (r < n) v = payload(A, r);
    }
    u64 s = v, lo = active ? v : ~0ull, hi = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const u64 ps = __shfl_up(s, d, 64), pl = __shfl_up(lo, d, 64), ph = __shfl_up(hi, d, 64);
      if (lane - d >= seg) {
        s += ps;
        lo = pl < lo ? pl : lo;
        hi = ph > hi ? ph : hi;
      }
    }
    if (have && head0) {  // the carried group ended with the chunk before: closed on the right
      if (lane == 0) group_put(left_open, heads - 1, ng, cs, clo, chi, sum, mn, mx);
      have = false;
    }
    const u64 rest = m & ~1ull;  // heads behind lane 0
    const int tail = (int)cnt - 1;
    if (rest) {
      const int e0 = __builtin_ctzll(rest) - 1;  // the first segment's last lane
      const bool last = lane < tail && ((m >> (lane + 1)) & 1ull);
      if (last) {
        const u64 g = heads + (u64)__builtin_popcountll(m & lanes_through(lane)) - 1;  // (heads >= 1 where lane 0 is no head)
        if (lane == e0 && !head0) {  // continues the carried group, or the group open at the left end of the range
          const u64 ts = s + cs, tl = clo < lo ? clo : lo, th = chi > hi ? chi : hi;
          group_put(have ? left_open : true, g, ng, ts, tl, th, sum, mn, mx);
        } else {
          group_put(false, g, ng, s, lo, hi, sum, mn, mx);
        }
      }
      cs = __shfl(s, tail, 64);  // the last segment starts at a head of this chunk
      clo = __shfl(lo, tail, 64);
      chi = __shfl(hi, tail, 64);
      have = true;
      left_open = false;
    } else {  // one segment
      const u64 ts = __shfl(s, tail, 64), tl = __shfl(lo, tail, 64), th = __shfl(hi, tail, 64);
      if (have) {  // (lane 0 is no head: the carried group goes on)
        cs += ts;
        clo = tl < clo ? tl : clo;
        chi = th > chi ? th : chi;
      } else {
        cs = ts;
        clo = tl;
        chi = th;
        have = true;
        left_open = !head0;
      }
    }
    heads += (u64)__builtin_popcountll(m);
  }
  if (have && lane == 0) group_put(true, heads - 1, ng, cs, clo, chi, sum, mn, mx);  // open on the right, always
}

// ---- host side -----------------------------------------------------------------------------------------------------------
// What a key kernel that checks its input adds to group_rows: kWords report words behind the call's GA_N accumulator words
// (cleared with them), begin() to preset them before the key kernel, and check() on their host copy -- behind the key
// kernel and the u64 sort, which reads key64 and row only, and in front of the first kernel that compares tuples.  A check
// that fails ends the call; one that passes may fill o->n_null.  GroupNoCheck: fixed-width columns, whose key kernels
// report nothing -- no word, no launch and no round trip is added.
struct GroupNoCheck {
  static constexpr int kWords = 0;
  int begin(hmj_ctx*, u64*) const { return HMJ_OK; }
  int check(hmj_ctx*, const u64*, hmj_group_opts*) const { return HMJ_OK; }
};

// What a group entry does behind its argument checks.  A: the relation as the kernels of steps 3-6 take it (a Side without
// bitmaps, or its NULL-equals-NULL form with them, always hashed); key: launches the key kernel of that form into the rows
// it is given (acc: the call's accumulator, the Check's words from acc + GA_N).
// o: hash_bits / force_hashed / want in, n_null / n_collisions out.
template <class Side, class KeyFn, class Check>
int group_rows(hmj_ctx* c, const KeyJoinNames& nm, const Side& A, u64 n, bool hashed, bool mat, KeyFn key, const Check& chk, hmj_group_opts* o,
               hmj_group_result* out) {
  GroupWs& ws = c->grp_ws;
  const u32 want = mat ? o->want : 0u;
  const u64 nblk = blocks_of(n);
  constexpr size_t acc_words = (size_t)GA_N + (size_t)Check::kWords;
  RC_TRY(ensure_dev(c, ws.acc, acc_words * sizeof(u64)));
  RC_TRY(ensure_dev(c, ws.rows, 16 * n));
  RC_TRY(ensure_dev(c, ws.sorted, 16 * n));
  RC_TRY(ensure_dev(c, ws.flags, nblk * KJ_WAVES * sizeof(u64)));
  RC_TRY(ensure_dev(c, ws.blk, nblk * sizeof(u64)));
  RC_TRY(ensure_dev(c, ws.blk_off, (nblk + 1) * sizeof(u64)));
  u64* acc = (u64*)ws.acc.p;
  ulonglong2* rows = (ulonglong2*)ws.sorted.p;
  const dim3 G((u32)nblk), T(KJ_THREADS);
  u64 h[GA_N];
  // 1. {key64, row} rows
  RC_TRY(ws.ev.record(c, 0));
  HIP_TRY(hipMemsetAsync(acc, 0, acc_words * sizeof(u64), c->stream));
  if constexpr (Check::kWords != 0) RC_TRY(chk.begin(c, acc + GA_N));
  RC_TRY(key(c, (u64*)ws.rows.p, acc));
  RC_TRY(ws.ev.record(c, 1));
  // 2. the stable u64 sort: rows of one key64 contiguous and ascending by row
  {
    const hmj_plan_desc plan = c->plan;  // (the sort is not a join: hmj_last_plan / hmj_last_timing keep describing the last one)
    const hmj_timing timing = c->timing;
    const int rc = hmj_sort_u64_device(c, ws.rows.p, n, ws.sorted.p);
    c->plan = plan;
    c->timing = timing;
    if (rc != HMJ_OK) return rc;
  }
  RC_TRY(ws.ev.record(c, 2));
  // the key kernel's verdict on its input, before any kernel follows a row into the key columns
  if constexpr (Check::kWords != 0) {
    u64 e[Check::kWords];
    RC_TRY(read_back(c, acc + GA_N, e, sizeof(e)));
    RC_TRY(chk.check(c, e, o));
  }
  // 3. hashed: runs of equal key64 that hold several tuples, sorted by (tuple, row)
  bool mixed = false;  // some run of equal key64 holds several tuples
  if (hashed && n > 1) {
    const u64 cap = n < kListCap ? n : kListCap;
    RC_TRY(ensure_dev(c, ws.list, cap * sizeof(u64)));
    RC_TRY(ensure_dev(c, ws.runs, 2 * cap * sizeof(u64)));
    hipLaunchKernelGGL(group_mismatch_kernel<Side>, dim3((u32)blocks_of(n - 1)), T, 0, c->stream, (const ulonglong2*)rows, n, A,
                       (u64*)ws.list.p, acc);
    HIP_TRY(hipGetLastError());
    RC_TRY(read_back(c, acc, h, KA_N * sizeof(u64)));
    RC_TRY(collision_errors(c, nm, h[KA_ERR]));
    mixed = h[KA_LIST_N] != 0;
    if (mixed) {
      const u64 gl = blocks_of(h[KA_LIST_N]), gs = h[KA_LIST_N] < (u64)(4 * c->num_cus) ? h[KA_LIST_N] : (u64)(4 * c->num_cus);
      hipLaunchKernelGGL(group_run_leader_kernel<Side>, dim3((u32)(gl < 1024 ? gl : 1024)), T, 0, c->stream, (const ulonglong2*)rows, n, A,
                         (const u64*)ws.list.p, (u64*)ws.runs.p, acc);
      HIP_TRY(hipGetLastError());
      hipLaunchKernelGGL(group_run_sort_kernel<Side>, dim3((u32)gs), T, 0, c->stream, (const u64*)ws.runs.p, A, rows, (const u64*)acc);
      HIP_TRY(hipGetLastError());
      RC_TRY(read_back(c, acc, h, KA_N * sizeof(u64)));
      RC_TRY(collision_errors(c, nm, h[KA_ERR]));
    }
  }
  // 4. heads: one ballot word per wave, heads per workgroup, one scan; n_groups comes back to size the group columns.  The
  // tuples are compared only where the collision search found a mismatch: without one, equal key64 is equal tuples.
  if (mixed) hipLaunchKernelGGL((group_heads_kernel<Side, true>), G, T, 0, c->stream, (const ulonglong2*)rows, n, A, (u64*)ws.flags.p,
                                 (u64*)ws.blk.p, acc);
  else hipLaunchKernelGGL((group_heads_kernel<Side, false>), G, T, 0, c->stream, (const ulonglong2*)rows, n, A, (u64*)ws.flags.p,
                          (u64*)ws.blk.p, acc);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hmj::launch_scan_u64((const u64*)ws.blk.p, (u64*)ws.blk_off.p, (u32)nblk, c->stream));
  u64 ng = 0;
  RC_TRY(read_back(c, (const u64*)ws.blk_off.p + nblk, &ng, sizeof(u64)));
  if (ng < 1 || ng > n) {
    char msg[128];
    std::snprintf(msg, sizeof(msg), "%s: the heads' count is not in 1..n", nm.join);
    return fail(c, HMJ_E_HIP, msg);
  }
  // 5. the group columns (count-only calls: start alone, for max_count)
  RC_TRY(ensure_dev(c, ws.start, (ng + 1) * sizeof(u64)));
  struct Col {
    DevBuf* b;
    bool on;
    u64 rows;
    u64* p;
  } cols[7] = {{&ws.key, mat, ng, nullptr},
               {&ws.first, mat, ng, nullptr},
               {&ws.count, (want & HMJ_GROUP_COUNT) != 0, ng, nullptr},
               {&ws.sum, (want & HMJ_GROUP_SUM) != 0, ng, nullptr},
               {&ws.min, (want & HMJ_GROUP_MIN) != 0, ng, nullptr},
               {&ws.max, (want & HMJ_GROUP_MAX) != 0, ng, nullptr},
               {&ws.gmap, (want & HMJ_GROUP_ROW_MAP) != 0, n, nullptr}};
  for (Col& k : cols) {
    if (!k.on) continue;
    RC_TRY(ensure_dev(c, *k.b, k.rows * sizeof(u64)));
    k.p = (u64*)k.b->p;
  }
  hipLaunchKernelGGL(group_emit_kernel, G, T, 0, c->stream, (const ulonglong2*)rows, n, ng, (const u64*)ws.flags.p, (const u64*)ws.blk_off.p,
                     cols[0].p, cols[1].p, (u64*)ws.start.p, cols[3].p, cols[4].p, cols[5].p, cols[6].p);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(group_count_kernel, dim3((u32)blocks_of(ng)), T, 0, c->stream, (const u64*)ws.start.p, ng, cols[2].p, acc);
  HIP_TRY(hipGetLastError());
  RC_TRY(ws.ev.record(c, 3));
  // 6. sum / min / max of the payloads
  if (want & (HMJ_GROUP_SUM | HMJ_GROUP_MIN | HMJ_GROUP_MAX)) {
    const u64 waves = ((n + 63) / 64 + kAggChunks - 1) / kAggChunks;  // a wave walks kAggChunks chunks of 64 positions
    hipLaunchKernelGGL(group_agg_kernel<Side>, dim3((u32)((waves + KJ_WAVES - 1) / KJ_WAVES)), T, 0, c->stream, (const ulonglong2*)rows, n, ng, A, (const u64*)ws.flags.p,
                       (const u64*)ws.blk_off.p, cols[3].p, cols[4].p, cols[5].p);
    HIP_TRY(hipGetLastError());
  }
  RC_TRY(ws.ev.record(c, 4));
  RC_TRY(read_back(c, acc, h, sizeof(h)));
  RC_TRY(collision_errors(c, nm, h[KA_ERR]));
  if constexpr (Check::kWords == 0) o->n_null = null_rows_of(h + GA_NULL);  // (else: the Check's words hold the count)
  o->n_collisions = h[GA_COLL];
  out->n_groups = ng;
  out->max_count = h[GA_MAXC];
  out->key64 = (const uint64_t*)cols[0].p;
  out->first_row = (const uint64_t*)cols[1].p;
  out->count = (const uint64_t*)cols[2].p;
  out->sum = (const uint64_t*)cols[3].p;
  out->min = (const uint64_t*)cols[4].p;
  out->max = (const uint64_t*)cols[5].p;
  out->group_of_row = (const uint64_t*)cols[6].p;
  return HMJ_OK;
}

}  // namespace
