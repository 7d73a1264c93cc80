// The key-only probe side's host arithmetic (hashmergejoin_amd/csrc/hmj_probekeys.h) on its own: which probe rows the pilot
// samples, whether a join attempts the path, pilots first or skips it, and the slab capacity of key rows.  No HIP, no
// library: tests/test_probekeys_cpu.py builds this file with g++, plain and under AddressSanitizer + UBSan, and runs both.
#include <cstdint>
#include <cstdio>
#include <initializer_list>

#include "../../hashmergejoin_amd/csrc/hmj_probekeys.h"

using namespace hmj_host;

static int failures = 0;
#define CHECK(cond)                                                     \
  do {                                                                  \
    if (!(cond)) {                                                      \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);     \
      failures++;                                                       \
    }                                                                   \
  } while (0)

// indices in range and strictly increasing, for probe sides below, at, just above and far above K, multiples of K or not
static void test_sample_rule() {
  const uint64_t K = kProbeKeysPilotRows;
  const uint64_t sizes[] = {1, 2, 63, K - 1, K, K + 1, 2 * K - 1, 2 * K, 3 * K + 7, (1ull << 22), (1ull << 22) + 1, (1ull << 22) + 2047,
                            (1ull << 22) + 4097, (1ull << 26) + 12345, (1ull << 28), 500000000ull, (1ull << 32) - 17, (1ull << 40) + 3};
  for (uint64_t np : sizes) {
    const uint32_t cnt = probe_keys_sample_count(np);
    CHECK(cnt == (np < K ? np : K));
    uint64_t prev = 0;
    for (uint32_t i = 0; i < cnt; i++) {
      const uint64_t idx = probe_keys_sample_index(i, np);
      CHECK(idx < np);
      CHECK(i == 0 ? idx == 0 : idx > prev);
      prev = idx;
    }
    if (np >= K) {
      CHECK(probe_keys_sample_index(1, np) == np / K);                    // floor(i * np / K)
      CHECK(probe_keys_sample_index((uint32_t)K - 1, np) == (K - 1) * np / K);
      CHECK(probe_keys_sample_index((uint32_t)K - 1, np) < np - 1 || np == K);  // the last row is never sampled beyond np = K
    } else {
      CHECK(probe_keys_sample_index(cnt - 1, np) == np - 1);              // every row
    }
  }
  CHECK(probe_keys_sample_count(0) == 0);
  // rows the GPU tests plant an unmatched row at
  CHECK(probe_keys_sample_index(1, 1ull << 22) == 1024 && probe_keys_sample_index(0, 1ull << 22) == 0);
}

static ProbeKeysJoin join_of(uint64_t np, int ba = 8, int bb = 8) { return ProbeKeysJoin{0u, np, {ba, bb}, false, false}; }

static void test_decision() {
  typedef ProbeKeysVerdict V;
  const uint64_t big = 1ull << 28;
  const ProbeKeysState fresh{-1, kProbeKeysMinLog2Default, 0, false, false};
  CHECK(kProbeKeysMinLog2Default > 23);  // the suite's 2^22 / 2^23-row joins stay on whole rows by default
  // a workload nothing is known about: pilot; known clean: attempt; known dirty (the pilot said no): skip silently
  CHECK(probe_keys_decide(fresh, join_of(big)) == V::Pilot);
  CHECK(probe_keys_decide(ProbeKeysState{-1, 24, 0, true, false}, join_of(big)) == V::Attempt);
  CHECK(probe_keys_decide(ProbeKeysState{-1, 24, 0, false, true}, join_of(big)) == V::SkipDirty);
  CHECK(probe_keys_decide(ProbeKeysState{-1, 24, 0, true, true}, join_of(big)) == V::Attempt);  // (a verified join outranks an older pilot)
  // cooling outranks everything but "off", also the forced mode
  for (int mode : {-1, 1})
    for (int clean = 0; clean < 2; clean++) CHECK(probe_keys_decide(ProbeKeysState{mode, 24, 3, clean != 0, false}, join_of(big)) == V::SkipCooling);
  CHECK(probe_keys_decide(ProbeKeysState{0, 24, 3, true, false}, join_of(big)) == V::SkipOff);
  CHECK(probe_keys_decide(ProbeKeysState{0, 24, 0, true, false}, join_of(big)) == V::SkipOff);
  // forced: no pilot, whatever the memo says
  CHECK(probe_keys_decide(ProbeKeysState{1, 24, 0, false, false}, join_of(big)) == V::Attempt);
  CHECK(probe_keys_decide(ProbeKeysState{1, 24, 0, false, true}, join_of(big)) == V::Attempt);
  // the threshold: np >= 2^min_log2
  CHECK(probe_keys_decide(fresh, join_of((1ull << kProbeKeysMinLog2Default) - 1)) == V::SkipShape);
  CHECK(probe_keys_decide(fresh, join_of(1ull << kProbeKeysMinLog2Default)) == V::Pilot);
  CHECK(probe_keys_decide(ProbeKeysState{-1, 24, 0, false, false}, join_of((1ull << 24) - 1)) == V::SkipShape);
  CHECK(probe_keys_decide(ProbeKeysState{-1, 24, 0, false, false}, join_of(1ull << 24)) == V::Pilot);
  CHECK(probe_keys_decide(ProbeKeysState{-1, 22, 0, false, false}, join_of(1ull << 22)) == V::Pilot);
  CHECK(probe_keys_decide(ProbeKeysState{1, 22, 0, false, false}, join_of((1ull << 22) - 1)) == V::SkipShape);
  CHECK(probe_keys_decide(ProbeKeysState{-1, -1, 0, false, false}, join_of(big)) == V::SkipShape);
  CHECK(probe_keys_decide(ProbeKeysState{-1, 64, 0, false, false}, join_of(big)) == V::SkipShape);
  // not the plain count join, no probe side, rows still arriving, pass widths the key kernels do not have: nothing is
  // recorded, whatever the switches and the memo say
  for (int mode : {-1, 0, 1}) {
    const ProbeKeysState s{mode, 24, mode == 0 ? 0 : 2, true, false};
    for (uint32_t flags : {1u, 2u, 4u, 8u, 0x10u, 0x3u}) {
      ProbeKeysJoin j = join_of(big);
      j.flags = flags;
      CHECK(probe_keys_decide(s, j) == V::SkipShape);
    }
    ProbeKeysJoin j = join_of(big);
    j.prepare_only = true;
    CHECK(probe_keys_decide(s, j) == V::SkipShape);
    j = join_of(big);
    j.arriving = true;
    CHECK(probe_keys_decide(s, j) == V::SkipShape);
    CHECK(probe_keys_decide(s, join_of(0)) == V::SkipShape);
    CHECK(probe_keys_decide(s, join_of(big, 9, 8)) == V::SkipShape);  // the 17-bit plan of 5 * 10^8 rows keeps whole rows
    CHECK(probe_keys_decide(s, join_of(big, 8, 9)) == V::SkipShape);
    CHECK(probe_keys_decide(s, join_of(big, 0, 8)) == V::SkipShape);
  }
  CHECK(probe_keys_decide(fresh, join_of(big, 1, 1)) == V::Pilot);
  CHECK(probe_keys_decide(fresh, join_of(big, kProbeKeysMaxPassBits, kProbeKeysMaxPassBits)) == V::Pilot);
}

static void test_slab_cap() {
  for (uint32_t cap = 8; cap < 5000; cap += 8) {  // (the Tup passes' capacities are multiples of 8 rows)
    const uint32_t k = probe_keys_slab_cap(cap);
    CHECK(k % 16 == 0 && k >= cap && k < cap + 16);
    CHECK((uint64_t)k * 8 <= (uint64_t)cap * 16);  // key slabs fit the buffers sized for 16-byte rows
  }
}

int main() {
  test_sample_rule();
  test_decision();
  test_slab_cap();
  if (failures) {
    std::printf("%d checks failed\n", failures);
    return 1;
  }
  std::printf("all probe-keys cases passed\n");
  return 0;
}
