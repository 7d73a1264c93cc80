// The pure host helpers of the entries (hashmergejoin_amd/csrc/hmj_args.h) on their own: widths, validity byte spans, range
// overlap, and the prefix copies of the size-versioned opts.  No HIP, no library: tests/test_entry_args_cpu.py builds this
// file with g++, plain and under AddressSanitizer + UBSan, and runs both.  A caller's opts struct is allocated at exactly its
// struct_size bytes, so that the sanitizer sees any byte touched behind it.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../hashmergejoin_amd/csrc/hmj_args.h"

using namespace hmj_host;

static int failures = 0;
#define CHECK(cond)                                                     \
  do {                                                                  \
    if (!(cond)) {                                                      \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);     \
      failures++;                                                       \
    }                                                                   \
  } while (0)

// out lies between the size and an in field that a later header version appended
struct TestOpts {
  uint32_t struct_size;
  uint32_t out;
  uint64_t in_behind;
};

// n bytes the compiler knows nothing about, every byte 0xAB
static void* raw_bytes(size_t n) {
  volatile size_t m = n;
  void* p = std::malloc(m);
  std::memset(p, 0xAB, m);
  return p;
}

static void test_width_of() {
  const uint32_t types[10] = {HMJ_TYPE_I8, HMJ_TYPE_I16, HMJ_TYPE_I32, HMJ_TYPE_I64, HMJ_TYPE_U8,
                              HMJ_TYPE_U16, HMJ_TYPE_U32, HMJ_TYPE_U64, HMJ_TYPE_F32, HMJ_TYPE_F64};
  const uint32_t want[10] = {1, 2, 4, 8, 1, 2, 4, 8, 4, 8};
  for (int k = 0; k < 10; k++) CHECK(width_of(types[k]) == want[k]);
}

static void test_validity() {
  unsigned char bits[8] = {0};
  const uint64_t offs[4] = {0, 7, 8, 9}, ns[3] = {1, 8, 9};
  // (offset 9 with 9 rows: bits 9 .. 17 lie in bytes 1 and 2 -- two bytes, what ((9 & 7) + 9 + 7) / 8 gives)
  const uint64_t want[4][3] = {{1, 1, 2}, {1, 2, 2}, {1, 1, 2}, {1, 2, 2}};
  for (int a = 0; a < 4; a++) {
    for (int b = 0; b < 3; b++) {
      const hmj_validity v = {bits, offs[a]};
      const Range r = validity_range(v, ns[b]);
      CHECK(r.lo == (uintptr_t)bits + offs[a] / 8);
      CHECK(r.hi - r.lo == want[a][b]);
    }
  }
  const hmj_validity none = {nullptr, 5}, some = {bits, 5};
  CHECK(validity_range(none, 9).lo == validity_range(none, 9).hi);
  CHECK(validity_range(some, 0).lo == validity_range(some, 0).hi);
  const uint64_t n = 1000;
  const hmj_validity edge = {bits, UINT64_MAX - n}, past = {bits, UINT64_MAX - n + 1}, past_none = {nullptr, UINT64_MAX - n + 1};
  CHECK(!validity_overflows(edge, n));
  CHECK(validity_overflows(past, n));
  CHECK(!validity_overflows(past_none, n));
}

static void test_overlap() {
  unsigned char buf[64];
  const Range a = range_of(buf, 16), b = range_of(buf + 16, 16), c = range_of(buf + 15, 2), empty = range_of(buf + 4, 0),
              null = range_of(nullptr, 16);
  CHECK(!overlap(a, b) && !overlap(b, a));  // touching
  CHECK(overlap(a, c) && overlap(c, b));
  CHECK(overlap(a, a));
  CHECK(!overlap(empty, a) && !overlap(a, empty) && !overlap(empty, empty));  // an empty range lies inside a
  CHECK(null.lo == null.hi && !overlap(null, a));
  const Range outs[2] = {a, b}, ins[3] = {empty, null, c};
  OverlapHit h = first_overlap(outs, 2, ins, 3);
  CHECK(h && h.out == 0 && h.in == 2);
  h = first_overlap(outs + 1, 1, ins, 3);
  CHECK(h && h.out == 0 && h.in == 2);
  CHECK(!first_overlap(outs, 2, ins, 2));
  CHECK(!first_overlap(outs, 2, outs, 2));  // no range against itself
  const Range twice[2] = {a, c};
  h = first_overlap(twice, 2, twice, 2);
  CHECK(h && h.out == 0 && h.in == 1);
}

// One round trip as an entry makes it, with the caller's struct in exactly `size` bytes.
static void round_trip(uint32_t size) {
  TestOpts* caller = (TestOpts*)raw_bytes(size);
  caller->struct_size = size;
  const bool has_out = size >= offsetof(TestOpts, out) + sizeof(uint32_t);
  const bool has_in = size >= offsetof(TestOpts, in_behind) + sizeof(uint64_t);
  if (has_out) caller->out = 0x11111111u;
  if (has_in) caller->in_behind = 0x2222222222222222ull;

  TestOpts full;
  std::memset(&full, 0xCD, sizeof(full));
  opts_prefix_in(&full, caller);
  CHECK(full.struct_size == size);
  CHECK(full.out == (has_out ? 0x11111111u : 0u));
  CHECK(full.in_behind == (has_in ? 0x2222222222222222ull : 0ull));  // zeros behind the caller's prefix

  opts_clear_out(&full, caller, offsetof(TestOpts, out), offsetof(TestOpts, in_behind), sizeof(TestOpts));
  CHECK(full.struct_size == size);
  CHECK(full.out == 0);  // an out field comes back cleared
  CHECK(full.in_behind == (has_in ? 0x2222222222222222ull : 0ull));  // the in field behind it is the caller's again

  full.out = 77;
  full.struct_size = 0xFFFFFFFFu;  // whatever the entry left there
  opts_prefix_out(caller, full);
  CHECK(caller->struct_size == size);  // survives
  if (has_out) CHECK(caller->out == 77);
  if (has_in) CHECK(caller->in_behind == 0x2222222222222222ull);
  const unsigned char* tail = (const unsigned char*)caller;
  for (uint32_t k = sizeof(TestOpts); k < size; k++) CHECK(tail[k] == 0xAB);  // nothing behind sizeof(T) is written
  std::free(caller);
}

static void test_prefix_copies() {
  round_trip(sizeof(uint32_t) + sizeof(uint32_t));  // an older header: smaller than the struct
  round_trip(sizeof(TestOpts));
  round_trip(sizeof(TestOpts) + 8);  // a newer header: larger
  // the clear without in fields behind the out fields: everything from first_out on
  TestOpts caller = {sizeof(TestOpts), 5, 6}, full;
  opts_prefix_in(&full, &caller);
  opts_clear_out(&full, &caller, offsetof(TestOpts, out));
  CHECK(full.struct_size == sizeof(TestOpts) && full.out == 0 && full.in_behind == 0);
}

int main() {
  test_width_of();
  test_validity();
  test_overlap();
  test_prefix_copies();
  if (failures) {
    std::printf("%d checks failed\n", failures);
    return 1;
  }
  std::printf("all entry argument cases passed\n");
  return 0;
}
