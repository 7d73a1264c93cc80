// The planning arithmetic of the ordered join of a small build side (api.hip, try_small_build_ordered) and of
// hmj_sort_u64_device: the cost model and its gate, the rank-run cut and level, the MSD window of the device sort, the
// digits of the chains of slab passes.  Pure functions of sizes, key masks and knobs: no HIP call and no hmj_ctx, so the
// header compiles with a plain C++ compiler (tests/cpp/test_smallplan.cc runs it under sanitizers).  What the functions need
// of a context comes in as small knob structs that api.hip fills.  Internal header.
#pragma once
#include <cmath>
#include <cstdint>

namespace hmj_host {

// The constants of the cost model that chooses, for an ordered join of a small build side under a long probe side, between
// the partitioned one-pass ordered write and the forms that order through the key's rank (api.hip, try_small_build_ordered).
// ALL of them are fits to sweeps on MI355X boxes (profiles/r04i_*, r04l_*, r04p_*, r04u_*, r05k_*): ms per join =
// fixed + ns_per_row * probe rows / 10^6 (+ per-run term).  One struct, so that a port to another part re-measures one place
// (they were literals in three functions); HMJ_ORDERED_MODEL="name=value,..." overrides single fields at
// hmj_create (developer builds).
struct OrderedCostModel {
  // partitioned one-pass ordered write at fan-out f (probe rows per build row)
  double part_fixed_ms = 0.15;
  double part_ns = 0.030, part_ns_per_f = 0.00023;                // whole-run ranking: linear in the run (f < 24, or cheaper than the buckets)
  double part_bucket_ns = 0.043, part_bucket_ns_per_f = 0.0001;  // (build rank, payload position) buckets from f = 24; + per f beyond 128
  double part_epilogue_ns = 0.25;                                 // f > 700: runs beyond the kernel's partitions, write + order epilogue
  // (rank, payload) composites sorted by global LSD passes
  double comp_fixed_ms = 0.65;
  double comp_ns_chain = 0.060, comp_ns_exact = 0.072;  // passes as a chain of slab passes / exact passes
  double comp_ns_wide = 0.145;                          // rank and payload as two words (payloads spanning > 64 - rank bits)
  double comp_ns_beyond_l2 = 0.02;                      // + where the key -> rank table leaves an XCD's L2
  // rank runs: two slab passes on the rank + an LDS sort per run
  double runs_fixed_ms = 0.25, runs_ns = 0.0215, runs_ns_per_run = 7.5;
  double runs_ns_per_log2_build = 0.0023;  // ... + this per probe row and doubling of the build side beyond 2^14 rows (the rank table and the build rows leave the L2: 2^14 / 2^18 / 2^20 x 2^28 rows 8.5 / 11.0 / 12.6 ms)
  double runs_wave_ns_per_run = 1.2, runs_wave_ns = 0.007;  // partitions of <= 512 rows, one wave each: per partition, and on top of runs_ns per row (profiles/r05aa_*)
  double runs_range_ns = 0.0;    // cut runs: the range of the payloads comes from a sample of ~2^17 rows (a pass over all of them cost 0.003)
};

// The most probe rows ANY of P partitions is expected to hold in a foreign-key join: a partition gets N ~ Poisson(lam)
// build keys (lam = avg_np / f) and about f probe rows for each.  N's upper quantile at 0.05 / P is found by summing
// the Poisson tail (the normal approximation "mean + 5 sigma" is 15 % short at lam = 8: fan-out 256 was planned into
// partitions that did not fit, and the whole join fell back to the two-step ordered form); the rows-per-key noise is
// added in quadrature.
inline double fk_probe_rows_hi(double avg_np, double f, double P) {
  if (avg_np <= 0.0 || f <= 0.0) return 0.0;
  const double lam = avg_np / f, p_tail = 0.05 / (P > 1.0 ? P : 1.0);
  const double step = lam > 256.0 ? std::floor(std::sqrt(lam) / 8.0) : 1.0;
  double k = std::floor(lam);
  for (const double k_end = lam + 40.0 * std::sqrt(lam) + 100.0; k < k_end; k += step) {
    const double lp = -lam + (k + 1.0) * std::log(lam) - std::lgamma(k + 2.0);  // log P(N = k + 1)
    if (std::exp(lp) / (1.0 - lam / (k + 2.0)) <= p_tail) break;                // (geometric bound on P(N > k))
  }
  const double z = (k - lam) / std::sqrt(lam), from_keys = (k - lam) * f, from_rows = z * std::sqrt(avg_np);
  return avg_np + std::sqrt(from_keys * from_keys + from_rows * from_rows);
}

// ns per probe row of the partitioned one-pass ordered foreign-key write at fan-out f (profiles/r04u_side_fk_payload_buckets.txt);
// slab_max_bits: the digit width of a slab pass (hmj_dev.h, SLAB_MAX_BITS) -- two of them make the finest plan there is
inline double ordered_part_ns(const OrderedCostModel& m, double f, double n_probe, int slab_max_bits) {
  if (f > 700.0) return m.part_epilogue_ns;  // (runs beyond the kernel's partitions: write + order epilogue)
  // ... and so are a few keys too many in one partition of the finest plan there is (18 bits): 2^19 x 2^28 rows -- two keys
  // of 512 probe rows per partition on average, twelve in the fullest of 2^18 -- overflowed the write's 6144-row shape,
  // the exact path took over with the order epilogue: 137 ms, against 19 ms on the composites and 15 ms for 2^20 x 2^28
  // (profiles/r05s_*).  The plan's own estimate of the fullest partition (fk_probe_rows_hi) says when.
  const double P18 = (double)(1u << (2 * slab_max_bits));
  if (fk_probe_rows_hi(n_probe / P18, f, P18) > 6144.0) return m.part_epilogue_ns;
  const double lin = m.part_ns + m.part_ns_per_f * f;
  if (f < 24.0) return lin;
  const double bucketed = m.part_bucket_ns + (f > 128.0 ? m.part_bucket_ns_per_f * (f - 128.0) : 0.0);
  return lin < bucketed ? lin : bucketed;
}

// ---- one workgroup's LDS sort of a partition (gtable.hip) ----------------------------------------------------------------
// The most rows a partition may hold at level -1 (one wave) and 0 / 1 / 2 (workgroups of 256 / 512 / 1024 threads):
// gtable.hip's rank_sort_max_run, 512 / 2048 / 4096 / 8192; filled once per context.
struct LdsSortKnobs {
  int max_run[4] = {0, 0, 0, 0};
  int at(int level) const { return max_run[(level < -1 ? -1 : level > 2 ? 2 : level) + 1]; }
};
// partitions that average `mean` rows fit a sort of at most max_run rows with room for their spread: mean + 8 sigma of a
// Poisson count, and a little
inline bool lds_sort_fits(double mean, int max_run) { return mean + 8.0 * std::sqrt(mean) + 24.0 <= (double)max_run; }
// the first of the levels first_level .. max_level whose sort holds such partitions (the smallest shape is the fastest: most
// sorters per CU); max_level + 1 where none does
inline int lds_sort_level(double mean, int first_level, int max_level, const int max_run[4]) {
  int lv = first_level;
  while (lv <= max_level && !lds_sort_fits(mean, max_run[(lv > 2 ? 2 : lv) + 1])) lv++;
  return lv;
}

// bit d: some bit of the 8-bit digit d of the mask is set (the digits in which keys differ)
inline uint32_t varying_digits(uint64_t mask) {
  uint32_t d = 0;
  for (int i = 0; i < 8; i++) d |= ((mask >> (8 * i)) & 0xFFu) ? (1u << i) : 0u;
  return d;
}

// Stable LSD passes over the low `total` bits of a word, digits of at most max_bits bits: as few passes as hold them, the
// bits spread evenly, the earlier passes take the extra bit.
inline int lsd_passes(int total, int max_bits) { return (total + max_bits - 1) / max_bits; }
inline int lsd_digit_bits(int total, int passes, int i) { return total / passes + (i < total % passes ? 1 : 0); }

// ---- the rank-run form ---------------------------------------------------------------------------------------------------
struct RankRunKnobs {
  bool rank_runs_mode = true, slab_mode = true, rank_runs_wave = true;
  int max_level = 2, max_group = 3, max_cut = 10;  // hmj_ctx: rank_runs_max_level / _max_group / _max_cut
  int chunk_rows = 64;                             // hmj_dev.h, RANK_PASS_CHUNK_ROWS
  int slab_max_bits = 9;                           // hmj_dev.h, SLAB_MAX_BITS
  LdsSortKnobs lds;
};
// The rank-run form (gtable.hip): every partition of probe rows must fit one workgroup's LDS sort with room for its
// spread (mean + 8 sigma of a run of a uniform foreign key), both digits of the partition number must be slab passes, and
// the partitions must be long enough for a workgroup each to pay.  A partition is a rank's whole run up to fan-outs of
// ~1700 (*tb = 0); beyond, a run is cut into 2^tb partitions by the position of the payload in the payloads' range.
inline bool rank_runs_fit(const RankRunKnobs& k, uint64_t n_build, uint64_t n_probe, int* tb, int* level) {
  *tb = 0;
  *level = 0;
  if (!k.rank_runs_mode || !k.slab_mode || n_build < 4 || n_probe > 0xFFFFFFFFull ||
      n_probe < (1u << 16))  // (a slab pass wants a few dozen tiles of rows)
    return false;
  const int rank_bits = 64 - __builtin_clzll(n_build - 1), max_bits = 2 * k.slab_max_bits;
  if (rank_bits < 2) return false;
  const double f0 = (double)n_probe / (double)n_build;
  if (f0 < 16.0) return false;
  if (rank_bits > max_bits) {
    // more ranks than two slab passes tell apart: 2^gb consecutive ranks to a partition (*tb = -gb), sorted there by (rank's
    // low bits, payload) as one word -- where 2^gb runs still fit one workgroup's sort
    const int gb = rank_bits - max_bits;
    if (gb > k.max_group) return false;
    const int lv = lds_sort_level(f0 * (double)(1u << gb), k.rank_runs_wave ? -1 : 0, k.max_level, k.lds.max_run);
    if (lv > k.max_level) return false;
    *tb = -gb;
    *level = lv;
    return true;
  }
  // the smallest workgroup shape (the fastest: most sorters per CU) whose cut stays within two slab passes; the wave
  // shape (level -1: 512 rows) only for whole runs -- cutting a run further to reach it would only add partitions
  if (k.rank_runs_wave && lds_sort_fits(f0, k.lds.at(-1))) {
    *level = -1;
    return true;
  }
  for (int lv = 0; lv <= k.max_level; lv++) {
    double f = f0;
    int t = 0;
    while (!lds_sort_fits(f, k.lds.at(lv))) {
      f *= 0.5;
      t++;
    }
    if (rank_bits + t > max_bits || t > k.max_cut) continue;
    if (t > 0) {
      // Payloads that grow with the row's position (row ids, timestamps): a worker of pass A reads `places` chunks from all
      // over the probe side (radix.hip, slab_a_body's strided form), each inside ONE piece; the fullest of its slabs must
      // still be within a slab's capacity (slab_geometry: mean + 8 sqrt(mean) + 24), or the attempt is known to overflow.
      const int TB = rank_bits + t, ba = TB - TB / 2;
      const double tile = ba > 8 ? 4096.0 : 2048.0, tiles = std::ceil((double)n_probe / tile), tpw = std::ceil(tiles / 2048.0);
      const double rpw = tpw * tile, places = rpw / (double)k.chunk_rows, pieces = (double)(1u << t);
      const double skew = places >= pieces ? std::ceil(places / pieces) / (places / pieces) : pieces / places;
      const double mean = rpw / (double)(1u << ba);
      if (skew * mean + 4.0 * std::sqrt(skew * mean) > mean + 8.0 * std::sqrt(mean) + 24.0) return false;
    }
    *tb = t;
    *level = lv;
    return true;
  }
  return false;
}
// (what a workload's memo says on top: the form rests after it gave up; cut runs exist only with the lookup inside pass A)
inline bool rank_runs_rested(int rank_runs_cooldown, int rank_lookup_cooldown, int tb) {
  return rank_runs_cooldown == 0 && (tb <= 0 || rank_lookup_cooldown == 0);
}

// ---- the gate of the ordered small-build join ----------------------------------------------------------------------------
struct SmallOrderedKnobs {
  bool available = true;  // the path's switches are on and nothing of the context rules it out (a forced plan, a prepared
                          // build side, rows still arriving, a prepare-only call)
  uint64_t gtable_max_rows = 1ull << 17;
  uint32_t gtable_sort_fanout = 128;
  bool chain_mode = true;  // the composites' passes may be a chain of slab passes (gtable_sort_slab && slab_mode) ...
  uint64_t gtable_sort_slab_min = 1ull << 25;  // ... from this many probe rows on
  RankRunKnobs runs;
};
// What the workload's memo holds of this path, by value: the gate decrements nothing.  gtable_sort is the caller's to test,
// AFTER the model has admitted the join, and only then to decrement: the gate does not read it.
struct SmallOrderedCooldowns {
  int gtable_sort = 0, gtable_sort_slab = 0, rank_runs = 0, rank_lookup = 0;
};
enum class SmallGate { NotEligible, RefusedByModel, Eligible };
struct SmallGateResult {
  SmallGate verdict = SmallGate::NotEligible;
  int run_tb = 0, run_level = 0;  // rank_runs_fit's cut and level ...
  bool fit = false;               // ... and its verdict, before the memo's say (rank_runs_rested)
  double part_ns = 0.0;           // ordered_part_ns of the join (Eligible: the wide-payload test wants it again)
};
// Which is faster is a matter of fan-out AND size (profiles/r04i_*, r04l_*: both paths over a grid of sizes).  This path:
// ~0.65 ms of dependent launches and read-backs + 0.06-0.09 ns per probe row (below).  The
// partitioned one-pass ordered write: ~0.15 ms + (0.030 + 0.00023 f) ns per row up to fan-out ~200, 0.00041 f ns beyond
// (the plan changes), and from ~700 rows per key on it declines (runs beyond its capacity) and the write + order
// epilogue takes over at 0.25 ns per row and more.  HMJ_GTABLE_SORT_FANOUT=1 (the experiments) skips the model.
inline SmallGateResult small_ordered_gate(const SmallOrderedKnobs& k, const OrderedCostModel& m, uint64_t n_build, uint64_t n_probe,
                                          bool ordered, SmallOrderedCooldowns cool) {
  SmallGateResult g;
  if (!k.available || !ordered || n_build == 0 || n_build > 16 * k.gtable_max_rows || n_probe > 0xFFFFFFFFull ||
      n_probe < (uint64_t)k.gtable_sort_fanout * n_build)
    return g;
  const double f = (double)n_probe / (double)n_build, rows = (double)n_probe * 1e-6;
  // (later in round 4 the one-pass write learned to rank inside (build rank, payload position) buckets from fan-out 24 on:
  //  0.043 ns per row up to fan-out ~130, + 0.0001 per further probe row per key -- 2^18 x 2^26: 7.5 -> 3.9 ms, 2^20 x 2^28:
  //  29.3 -> 15.8 -- so this path is now for fan-outs beyond ~500 and for runs the kernel's partitions cannot hold)
  g.part_ns = ordered_part_ns(m, f, (double)n_probe, k.runs.slab_max_bits);
  // (round 4, later: 0.060 where the composites' passes are the chain of slab passes below, 0.072 on exact passes, + 0.02
  //  where the table leaves the L2 -- profiles/r04p_side_rank_sort_slab_chain.txt)
  const bool chain = k.chain_mode && cool.gtable_sort_slab == 0 && n_probe >= k.gtable_sort_slab_min;
  // (round 5: runs that fit one workgroup's LDS sort -- fan-out up to ~1700 -- are partitioned by rank with two slab passes
  //  and sorted run by run, rank_runs_fit, whatever the payloads' width;
  //  measured over 2^12 ... 2^18 build x 2^22 ... 2^28 probe rows, profiles/r05k_sweep_ordered_small_build.txt: 0.25 ms of
  //  launches and read-backs + 0.0215 ns per probe row + 7.5 ns per RUN -- a workgroup's load -> sort -> store chain per key.
  //  Longer runs are cut into 2^tb pieces by the position of the payload in the payloads' range.  Row ids and timestamps
  //  are monotone in the row's POSITION, so a worker of a slab pass that reads one contiguous range of the probe side sees
  //  one piece only and its slab for that digit overflows, whichever digit the piece bits go into: the pass with the
  //  lookup reads 4 KiB chunks from all over the relation instead (radix.hip, RankXform::kStrided); + one pass over the
  //  payloads for their range)
  g.fit = rank_runs_fit(k.runs, n_build, n_probe, &g.run_tb, &g.run_level);
  const bool runs = g.fit && rank_runs_rested(cool.rank_runs, cool.rank_lookup, g.run_tb);
  // (2^20 ... 2^21 build rows: the rank-run form only -- there for the joins whose fullest 18-bit partition outgrows the
  //  one-pass ordered write: 2^21 x 2^29 rows took 166 ms on the exact path with the order epilogue, profiles/r05y_*)
  const double P18 = (double)(1u << (2 * k.runs.slab_max_bits));
  if (n_build > 8 * k.gtable_max_rows && (!runs || fk_probe_rows_hi((double)n_probe / P18, f, P18) <= 6144.0)) return g;
  const double rank_ns = (chain ? m.comp_ns_chain : m.comp_ns_exact) + (n_build > k.gtable_max_rows ? m.comp_ns_beyond_l2 : 0.0);
  const double n_parts = g.run_tb >= 0 ? (double)(n_build << g.run_tb) : (double)(n_build >> -g.run_tb);
  const double lb = std::log2((double)n_build) - 14.0;
  const bool wave = g.run_level < 0;
  const double rank_ms = runs ? m.runs_fixed_ms + (m.runs_ns + (wave ? m.runs_wave_ns : 0.0) + (g.run_tb > 0 ? m.runs_range_ns : 0.0) +
                                                  (lb > 0.0 ? lb * m.runs_ns_per_log2_build : 0.0)) * rows +
                                    (wave ? m.runs_wave_ns_per_run : m.runs_ns_per_run) * n_parts * 1e-6
                              : m.comp_fixed_ms + rank_ns * rows;
  g.verdict = (k.gtable_sort_fanout > 1 && rank_ms >= m.part_fixed_ms + g.part_ns * rows) ? SmallGate::RefusedByModel : SmallGate::Eligible;
  return g;
}
// Payloads too wide for one word beside the rank: ten passes instead of four or five, about 1.6 x the time per row (the
// rank-run form does not care) -- a wide-payload join needs twice the fan-out to take this path
inline bool wide_composites_refused(const OrderedCostModel& m, uint64_t n_probe, double part_ns) {
  const double rows = (double)n_probe * 1e-6;
  return m.comp_fixed_ms + m.comp_ns_wide * rows >= m.part_fixed_ms + part_ns * rows;
}

// ---- chains of slab passes (api.hip, slab_chain) -------------------------------------------------------------------------
// One digit of a chain: bits [shift, shift + bits) of the key word; dens >= 1 says how much fuller than the mean the values
// in use of the digit are (slab_chain sizes its slabs by it).
struct ChainDigit {
  int shift, bits;
  double dens;
};
// The composite sort's chain: the low rank_bits + range_bits bits of {rank, payload - svmin}, split as lsd_digit_bits does.
// The digits that hold the payload range's and the rank's top bits are sized for how much of their range is in use.
inline int composite_chain_digits(int rank_bits, int range_bits, uint64_t svmin, uint64_t svmax, uint32_t nb, int max_bits, ChainDigit dg[8]) {
  const int total = rank_bits + range_bits, passes = lsd_passes(total, max_bits);
  const double dens_range = range_bits ? std::ldexp(1.0, range_bits) / ((double)(svmax - svmin) + 1.0) : 1.0;
  const double dens_rank = rank_bits ? std::ldexp(1.0, rank_bits) / (double)nb : 1.0;
  int shift = 0;
  for (int i = 0; i < passes; i++) {
    dg[i].shift = shift;
    dg[i].bits = lsd_digit_bits(total, passes, i);
    dg[i].dens = 1.0;
    if (range_bits && shift <= range_bits - 1 && range_bits - 1 < shift + dg[i].bits) dg[i].dens *= dens_range;
    if (rank_bits && i == passes - 1) dg[i].dens *= dens_rank;
    shift += dg[i].bits;
  }
  return passes;
}
// The device sort's chain, one digit per varying 8-bit digit of the keys.  exact: `diff` holds every bit in which keys differ
// (digits are trimmed to them).  Otherwise the sample saw all eight digits vary and `sdiff` holds the bits IT saw varying:
// every digit keeps its eight bits (a bit the sample missed must still be sorted on), but a bit of a digit that (as far as the
// sample tells) never varies halves the values in use, so the rows crowd into the others -- 63-bit keys fill half of the top
// digit -- and the slabs are sized for that.
inline int sort_chain_digits(uint64_t diff, uint64_t sdiff, uint64_t kmin, uint64_t kmax, ChainDigit dg[8]) {
  const bool exact = diff != ~0ull || sdiff == ~0ull;
  int nd = 0;
  for (int d = 0; d < 8; d++) {
    const uint32_t sub = (uint32_t)((exact ? diff : sdiff) >> (8 * d)) & 0xFFu;
    if (exact && !sub) continue;
    const int lo = exact ? __builtin_ctz(sub) : 0, hi = exact ? 31 - __builtin_clz(sub) : 7;
    dg[nd].shift = 8 * d + lo;
    dg[nd].bits = hi - lo + 1;
    dg[nd].dens = std::ldexp(1.0, dg[nd].bits - __builtin_popcount(sub));
    nd++;
  }
  if (exact && diff != ~0ull && nd) {  // (kmin / kmax are the keys' extremes, all bits above the top digit agree)
    const ChainDigit& t = dg[nd - 1];
    const uint64_t in_use = (kmax >> t.shift) - (kmin >> t.shift) + 1;
    const double dt = std::ldexp(1.0, t.bits) / (double)in_use;
    if (dt > dg[nd - 1].dens) dg[nd - 1].dens = dt;
  }
  return nd;
}

// ---- the device sort's MSD window ----------------------------------------------------------------------------------------
// The key bits [hi - TB, hi) that two slab passes partition the rows on.  The window's top is the highest bit in which keys
// differ (diff != ~0: exact, with the extremes kmin / kmax), or bit 63 when only the sample's mask sdiff is known; it is the
// narrowest whose partitions average <= target_mean rows, counting that the keys may fill only part of it (dens).  ok: the
// window exists, pass A's digit is a slab pass's, and a level of the LDS sort up to max_level holds the partitions.
struct SortMsdWindow {
  int TB = 0, hi = 64, level = 0;
  double dens = 1.0, mean = 0.0;
  bool ok = false;
};
inline SortMsdWindow sort_msd_window(uint64_t n, uint64_t diff, uint64_t sdiff, uint64_t kmin, uint64_t kmax, int max_bits, double target_mean,
                                     int max_level, const LdsSortKnobs& lds, int slab_max_bits) {
  SortMsdWindow w;
  const bool exact = diff != ~0ull;
  const int hi = exact ? (diff ? 64 - __builtin_clzll(diff) : 0) : 64;  // keys agree in every bit from `hi` up
  // how much of the window's top digit is in use: exact -> from the extremes; sampled -> a top bit the sample never saw
  // varying halves it (63-bit keys)
  // the narrowest window whose partitions average <= 1200 rows, counting that the keys may fill only part of it
  int TB = 1;
  double dens = 1.0, mean = (double)n;
  do {
    TB++;
    if (TB > hi) break;
    if (exact) {
      const uint64_t in_use = (kmax >> (hi - TB)) - (kmin >> (hi - TB)) + 1;
      dens = std::ldexp(1.0, TB) / (double)in_use;
    } else if (sdiff != ~0ull) {
      dens = std::ldexp(1.0, __builtin_clzll(sdiff));  // (the sample's top varying bit is below bit 63)
      if (dens > 64.0) dens = 64.0;
    }
    mean = dens * (double)n / std::ldexp(1.0, TB);
    // (a 17th / 18th bit makes a pass a 9-bit pass -- 1.95 / 2.17 ms per 2^28 rows against 1.5 / 1.6 -- and is only worth
    //  partitions beyond the 512-thread sort's comfort: 2^27 / 2^28 rows 3.43 / 7.06 -> 3.32 / 6.84 ms, profiles/r05ad_*)
  } while (TB < max_bits && mean > (TB >= 16 ? 2.0 : 1.0) * target_mean);
  if (TB > hi) TB = 0;
  // (beyond 4.5 * 10^8 rows the 2^18 partitions outgrow the 256-thread sort: 512 / 1024 threads hold 4096 / 8192 rows)
  w.TB = TB;
  w.hi = hi;
  w.dens = dens;
  w.mean = mean;
  w.level = lds_sort_level(mean, 0, max_level, lds.max_run);
  w.ok = TB >= 2 && TB - TB / 2 <= slab_max_bits && w.level <= max_level;
  return w;
}

}  // namespace hmj_host
