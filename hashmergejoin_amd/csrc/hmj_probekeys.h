// The key-only probe side of a plain count join (api.hip run_slab_join; radix.hip's key-row slab passes; probe.hip's PKEYS
// kernel and its pilot): which probe rows the pilot samples, and whether a join attempts the path, pilots first, or skips it.
//
// A count join returns n_matches, sum_r and sum_s.  The first two need the probe KEYS only; sum_s needs a probe payload only
// for a probe row that does not meet exactly one build row.  When every probe row meets exactly one -- the foreign-key join
// against a unique dimension key with referential integrity -- sum_s is the plain sum of all probe payloads mod 2^64, which
// pass A adds up while it reads the rows anyway, and the probe side travels through the slab passes as 8-byte keys: 48
// instead of 80 bytes per probe row.  The probe kernel counts every probe row's hits and reports any count but one; the
// driver then redoes the probe side with whole rows (the build slabs stay).  The pilot keeps a one-shot caller whose join is
// not of that kind from paying for a wasted pass.
//
// Pure functions: no HIP call, no hmj_ctx -- the header compiles with a plain C++ compiler (tests/cpp/test_probekeys.cc)
// and, for the sample rule, inside the pilot kernel.  Internal header.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define HMJ_PK_HD __host__ __device__
#else
#define HMJ_PK_HD
#endif

namespace hmj_host {

#ifndef HMJ_PROBE_KEYS_DEFAULT
#define HMJ_PROBE_KEYS_DEFAULT -1
#endif
constexpr int kProbeKeysModeDefault = HMJ_PROBE_KEYS_DEFAULT;  // -1 pilot first, 0 off, 1 attempt unasked (HMJ_PROBE_KEYS = 2 / 0 / 1)
constexpr uint32_t kProbeKeysPilotRows = 4096;  // K: probe rows the pilot looks up, one wave each
// Probe rows from which the path is attempted (HMJ_PROBE_KEYS_MIN_LOG2): the smallest size at which a workload's FIRST join
// -- pilot and its host sync included -- was not slower than the join without the path (tools/exp_probe_keys_pilot.py,
// 2^k x 2^k rows, ms with pilot / without the path: 2^23 0.467 / 0.432, 2^24 0.710 / 0.683, 2^25 1.149 / 1.198, 2^26 2.073 / 2.254).
constexpr int kProbeKeysMinLog2Default = 25;
constexpr int kProbeKeysMinLog2Floor = 16;      // ... what the switch accepts
constexpr int kProbeKeysCooldown = 8;           // joins of the workload that keep whole rows after the probe said no
constexpr int kProbeKeysDirtyJoins = 64;        // joins of the workload that keep whole rows, silently, after the PILOT said no
constexpr int kProbeKeysMaxPassBits = 8;        // digit width of the key-row slab kernels (the 512-thread shape)

// Rows sampled from a probe side of np rows: K, or all of them where there are fewer.
HMJ_PK_HD inline uint32_t probe_keys_sample_count(uint64_t np) { return np < kProbeKeysPilotRows ? (uint32_t)np : kProbeKeysPilotRows; }
// Index of sample i (i < probe_keys_sample_count(np)): floor(i * np / K) for np >= K -- strictly increasing because the
// step np / K is at least one -- and i itself below.
HMJ_PK_HD inline uint64_t probe_keys_sample_index(uint32_t i, uint64_t np) {
  return np < kProbeKeysPilotRows ? (uint64_t)i : (uint64_t)i * np / kProbeKeysPilotRows;
}

// What a workload has taught the context (WorkloadMemo, hmj_ctx.h) and what the environment says.
struct ProbeKeysState {
  int mode;       // HMJ_PROBE_KEYS: 0 never, 1 always attempt (no pilot), -1 (the switch: 2): pilot unless the memo knows
  int min_log2;   // HMJ_PROBE_KEYS_MIN_LOG2
  int cooldown;   // > 0: the probe kernel said no within the last kProbeKeysCooldown joins of this workload
  bool clean;     // the workload's last key-only join was verified clean
  bool dirty;     // the workload's last pilot met a probe row without exactly one build row (asked again after kProbeKeysDirtyJoins)
};
// The join itself: what run_slab_join knows when it has decided to take the slab path.
struct ProbeKeysJoin {
  uint32_t flags;      // HMJ_* mode flags of the call (0: the plain count join)
  uint64_t np;         // probe rows
  int pass_bits[2];    // digit widths of slab passes A and B
  bool prepare_only;   // hmj_prepare_build: there is no probe side
  bool arriving;       // the probe rows are still arriving over the links (exchange join)
};
enum class ProbeKeysVerdict {
  SkipShape,    // not a join the path exists for: nothing is recorded
  SkipOff,      // HMJ_PROBE_KEYS=0
  SkipCooling,  // the workload is cooling: HMJ_REFUSED_PROBE_KEYS_COOLING
  SkipDirty,    // the workload's last pilot said no: whole rows, no pilot, nothing recorded in the plan
  Pilot,        // run the pilot after the build side's passes; attempt if it is clean
  Attempt       // attempt without a pilot (the memo says clean, or HMJ_PROBE_KEYS=1)
};
inline ProbeKeysVerdict probe_keys_decide(const ProbeKeysState& s, const ProbeKeysJoin& j) {
  if (j.flags != 0 || j.prepare_only || j.arriving || j.np == 0) return ProbeKeysVerdict::SkipShape;
  if (j.pass_bits[0] < 1 || j.pass_bits[0] > kProbeKeysMaxPassBits || j.pass_bits[1] < 1 || j.pass_bits[1] > kProbeKeysMaxPassBits)
    return ProbeKeysVerdict::SkipShape;
  if (s.min_log2 < 0 || s.min_log2 > 63 || j.np < (1ull << s.min_log2)) return ProbeKeysVerdict::SkipShape;
  if (s.mode == 0) return ProbeKeysVerdict::SkipOff;
  if (s.cooldown > 0) return ProbeKeysVerdict::SkipCooling;  // (also under HMJ_PROBE_KEYS=1: the probe kernel has spoken)
  if (s.mode == 1 || s.clean) return ProbeKeysVerdict::Attempt;
  if (s.dirty) return ProbeKeysVerdict::SkipDirty;
  return ProbeKeysVerdict::Pilot;
}

// Slab capacity of the key-row passes: the Tup passes' capacity rounded up to whole 128-byte lines of 16 keys, so that every
// slab starts on a line.  The buffers are sized for 16-byte rows of the unrounded capacity (cap >= 8), so nothing grows.
HMJ_PK_HD inline uint32_t probe_keys_slab_cap(uint32_t cap) { return (cap + 15u) & ~15u; }

}  // namespace hmj_host
