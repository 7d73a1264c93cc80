// Host-only test of the C++ drop-in operator (include/hashmergejoin_hip.hpp) linked against tests/cpp/hmj_abi_stub.cc
// instead of libhmj_hip.so, so that it runs under AddressSanitizer, UBSan and ThreadSanitizer on any machine
// (tests/test_dropin_host_cpu.py).  Every expected result comes from tests/cpp/dropin_checks.h's brute-force joins; the
// stub is never its own check.  Covered: every join class and input kind at sizes from 0 x 0 to 2^17 x 2^17 on 8 threads,
// copies / moves / assignments / clear() / a destroyed source, exceptions thrown by the caller's key and payload types,
// errors of every status-returning ABI call, and two threads joining at once.
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <deque>
#include <stdexcept>
#include <string>
#include <thread>
#include <tuple>
#include <utility>
#include <vector>

#include "dropin_checks.h"
#include "hashmergejoin_hip.hpp"

extern "C" void hmj_stub_fail(int nth_call, int code);

using namespace dropin_checks;

typedef std::vector<std::pair<uint64_t, uint64_t>> U64Vec;
typedef std::deque<std::pair<uint64_t, uint64_t>> U64Deque;
typedef std::vector<std::pair<std::string, uint64_t>> StrVec;

static int g_fails = 0;
static void expect(bool good, const std::string& what) {
  if (!good) {
    std::printf("FAIL %s\n", what.c_str());
    g_fails++;
  }
}

struct Size {
  std::size_t nr, ns;
  unsigned threads;
};
// below 65536 rows hmj_detail::parallel_ranges starts no threads; 2^17 rows on 8 threads split every pass.  Largest first:
// the threaded passes and the pair-by-pair path are reached before any smaller case can stop the run.
static const Size kSizes[] = {{1u << 17, 1u << 17, 8}, {1000, 900, 2}, {1, 1, 1}, {5, 0, 1}, {0, 5, 1}, {0, 0, 1}};

static std::string tag(const char* what, const Size& z) {
  return std::string(what) + " " + std::to_string(z.nr) + "x" + std::to_string(z.ns) + " threads=" + std::to_string(z.threads);
}

// row i's key number: unique (offset + i) when domain == 0, else drawn from [0, domain) with repeats
static uint64_t key_no(std::size_t i, uint64_t offset, uint64_t domain, uint64_t salt) {
  return domain ? mix64(i * 0x9E37ull + salt) % domain : offset + i;
}
// std::string keys, a third of them too long for the string's inline buffer (their characters live on the heap)
static std::string str_key(uint64_t x) { return (x % 3 == 0 ? "a-key-long-enough-for-the-heap-" : "k") + std::to_string(x); }

// ---- uint64_t keys: the native operator (the GPU joins the caller's rows as they are) ----------------------------------
static void native_case(const Size& z, bool dup) {
  U64Vec r(z.nr), s(z.ns);
  for (std::size_t i = 0; i < z.nr; i++) r[i] = std::make_pair(mix64(key_no(i, 0, dup ? z.nr / 3 + 1 : 0, 1)), 1000 * i + 7);
  for (std::size_t i = 0; i < z.ns; i++) s[i] = std::make_pair(mix64(key_no(i, z.nr / 2, dup ? z.ns / 5 + 1 : 0, 2)), 3 * i + 1);
  const std::vector<Row3> want = native_rows(r.begin(), r.end(), s.begin(), s.end());
  const U64Vec o_r = {{5, 1}, {5, 2}, {6, 3}}, o_s = {{5, 9}, {6, 8}};
  const std::string t = tag(dup ? "native, duplicate keys" : "native, unique keys", z);
  typedef HashMergeJoin<U64Vec::const_iterator, U64Vec::const_iterator> J;
  g_fails += value_semantics<J>(
      t.c_str(), [&]() { return J(r.cbegin(), r.cend(), s.cbegin(), s.cend(), z.threads); },
      [&]() { return J(o_r.cbegin(), o_r.cend(), o_s.cbegin(), o_s.cend()); }, [&](J& j) { return native_ok(j, want); });
  // a std::deque is not contiguous: its rows are staged
  const U64Deque rd(r.begin(), r.end()), sd(s.begin(), s.end());
  const U64Deque o_rd(o_r.begin(), o_r.end()), o_sd(o_s.begin(), o_s.end());
  typedef HashMergeJoin<U64Deque::const_iterator, U64Deque::const_iterator> D;
  g_fails += value_semantics<D>(
      (t + " (std::deque)").c_str(), [&]() { return D(rd.cbegin(), rd.cend(), sd.cbegin(), sd.cend(), z.threads); },
      [&]() { return D(o_rd.cbegin(), o_rd.cend(), o_sd.cbegin(), o_sd.cend()); }, [&](D& j) { return native_ok(j, want); });
  // the count / sum reduction
  uint64_t want_sum = 0;
  for (const Row3& w : want) want_sum += std::get<1>(w) + std::get<2>(w);
  uint64_t n = 0, n2 = 0;
  const uint64_t sum = hash_merge_join_sum(r.begin(), r.end(), s.begin(), s.end(), &n);
  const uint64_t sum2 = hash_merge_join_sum(rd.begin(), rd.end(), sd.begin(), sd.end(), &n2);
  expect(n == want.size() && sum == want_sum && n2 == want.size() && sum2 == want_sum, t + ": hash_merge_join_sum");
}

// ---- hashed keys: HashMergeJoin<non-native key> ----------------------------------------------------------------------
template <typename Rel>
static void hashed_case(const char* what, const Size& z, const Rel& r, const Rel& s, const Rel& o_r, const Rel& o_s) {
  typedef typename Rel::value_type::first_type Key;
  std::vector<Key> rk, sk;
  std::vector<uint64_t> rh;
  for (const auto& row : r) {
    rk.push_back(row.first);
    rh.push_back((uint64_t)std::hash<Key>()(row.first));
  }
  for (const auto& row : s) sk.push_back(row.first);
  const std::vector<RowPair> want = hashed_pairs(rk, rh, sk);
  typedef HashMergeJoin<typename Rel::const_iterator, typename Rel::const_iterator> J;
  static_assert(!hmj_detail::is_hmj_relation_iter<typename Rel::const_iterator>::value, "the hashed operator");
  g_fails += value_semantics<J>(
      tag(what, z).c_str(), [&]() { return J(r.cbegin(), r.cend(), s.cbegin(), s.cend(), z.threads); },
      [&]() { return J(o_r.cbegin(), o_r.cend(), o_s.cbegin(), o_s.cend()); },
      [&](J& j) {
        return hashed_ok(j, want, [&](std::size_t i) { return &r[i].first; }, [&](std::size_t i) { return r[i].second; },
                         [&](std::size_t q) { return s[q].second; });
      });
}

static void string_case(const Size& z, bool repeats) {
  StrVec r(z.nr), s(z.ns);
  const uint64_t dom = z.nr / 2 + 1;
  // unique: r holds 0..nr-1 shuffled (7919 is prime to every size here), s holds nr/2 .. nr/2+ns-1
  for (std::size_t i = 0; i < z.nr; i++) r[i] = std::make_pair(str_key(repeats ? key_no(i, 0, dom, 3) : (i * 7919) % z.nr), 10 * i);
  for (std::size_t i = 0; i < z.ns; i++) s[i] = std::make_pair(str_key(key_no(i, z.nr / 2, repeats ? dom : 0, 4)), 5 * i + 2);
  const StrVec o_r = {{"x", 1}, {"y", 2}}, o_s = {{"y", 3}, {"x", 4}, {"x", 5}};
  hashed_case(repeats ? "std::string keys, repeats on both sides" : "std::string keys, unique", z, r, s, o_r, o_s);
}

template <unsigned Mod>
static void colliding_case(const Size& z) {
  typedef std::vector<std::pair<ModKey<Mod>, uint64_t>> Rel;
  Rel r(z.nr), s(z.ns);
  const uint64_t dom = z.nr + z.nr / 2 + 1;
  for (std::size_t i = 0; i < z.nr; i++) r[i] = std::make_pair(ModKey<Mod>{mix64(key_no(i, 0, dom, 5))}, 10 * i + 1);
  for (std::size_t i = 0; i < z.ns; i++) s[i] = std::make_pair(ModKey<Mod>{mix64(key_no(i, 0, dom, 6))}, 10 * i + 2);
  const Rel o_r = {{ModKey<Mod>{1}, 1}, {ModKey<Mod>{1 + Mod}, 2}}, o_s = {{ModKey<Mod>{1 + Mod}, 3}};
  hashed_case(("keys whose std::hash is v % " + std::to_string(Mod)).c_str(), z, r, s, o_r, o_s);
}

// ---- HashMergeJoin2: pre-hashed std::tuple<hash, key, value> rows ------------------------------------------------------
template <typename Buf, typename MakeRow>
static void prehashed_case(const char* what, const Size& z, MakeRow row) {
  typedef typename std::tuple_element<1, typename Buf::value_type>::type Key;
  Buf r, s, o_r, o_s;
  for (std::size_t i = 0; i < z.nr; i++) r.push_back(row(key_no(i, 0, z.nr / 2 + 1, 7), 10 * i));
  for (std::size_t i = 0; i < z.ns; i++) s.push_back(row(key_no(i, 0, z.nr / 2 + 1, 8), 10 * i + 3));
  for (uint64_t i = 0; i < 4; i++) o_r.push_back(row(i, i)), o_s.push_back(row(3 - i, i));
  // the ctor leaves both buffers stably sorted by hash: the rows the operator's results point at
  Buf rs(r), ss(s);
  auto by_hash = [](const typename Buf::value_type& a, const typename Buf::value_type& b) { return std::get<0>(a) < std::get<0>(b); };
  std::stable_sort(rs.begin(), rs.end(), by_hash);
  std::stable_sort(ss.begin(), ss.end(), by_hash);
  std::vector<Key> rk, sk;
  std::vector<uint64_t> rh;
  for (const auto& t : rs) rk.push_back(std::get<1>(t)), rh.push_back((uint64_t)std::get<0>(t));
  for (const auto& t : ss) sk.push_back(std::get<1>(t));
  const std::vector<RowPair> want = hashed_pairs(rk, rh, sk);
  typedef HashMergeJoin2<typename Buf::iterator, typename Buf::iterator> J;
  g_fails += value_semantics<J>(
      tag(what, z).c_str(), [&]() { return J(r.begin(), r.end(), s.begin(), s.end(), z.threads); },
      [&]() { return J(o_r.begin(), o_r.end(), o_s.begin(), o_s.end()); },
      [&](J& j) {
        return hashed_ok(j, want, [&](std::size_t i) { return &std::get<1>(r[i]); },
                         [&](std::size_t i) { return std::get<2>(r[i]); }, [&](std::size_t q) { return std::get<2>(s[q]); });
      });
  expect(r == rs && s == ss, tag(what, z) + ": caller buffers stably sorted by hash");
}

// ---- exceptions from the caller's types ------------------------------------------------------------------------------
// A key / payload type that counts its live objects and, once armed, throws from the armed operations on every call from
// the n-th on (so that with 8 threads several shares throw at once).
struct BoomError : std::runtime_error {
  BoomError() : std::runtime_error("boom") {}
};
struct Boom {
  enum { HASH = 1, EQ = 2, LESS = 4, COPY = 8 };
  static std::atomic<long> live, countdown;
  static std::atomic<int> armed;
  static void tick(int op) {
    if ((armed.load(std::memory_order_relaxed) & op) && countdown.fetch_sub(1) <= 1) throw BoomError();
  }
  uint64_t v = 0;
  Boom() { live++; }
  explicit Boom(uint64_t x) : v(x) { live++; }
  Boom(const Boom& o) : v(o.v) { live++; }
  Boom& operator=(const Boom& o) {
    tick(COPY);
    v = o.v;
    return *this;
  }
  ~Boom() { live--; }
  bool operator==(const Boom& o) const {
    tick(EQ);
    return v == o.v;
  }
  bool operator<(const Boom& o) const {
    tick(LESS);
    return v < o.v;
  }
};
std::atomic<long> Boom::live(0), Boom::countdown(0);
std::atomic<int> Boom::armed(0);
namespace std {
template <>
struct hash<Boom> {
  size_t operator()(const Boom& b) const {
    Boom::tick(Boom::HASH);
    return (size_t)mix64(b.v);
  }
};
}  // namespace std

static void exception_case(int op, unsigned threads) {
  typedef std::vector<std::pair<Boom, Boom>> Rel;
  const std::size_t n = threads > 1 ? 1u << 17 : 1u << 12;  // (every armed operation runs at least n / 2 times)
  const bool repeats = op == Boom::LESS;  // operator< orders the groups of a repeated hash only
  Rel r, s;
  for (std::size_t i = 0; i < n; i++) {
    r.push_back(std::make_pair(Boom(i), Boom(10 * i)));
    s.push_back(std::make_pair(Boom(repeats ? (i * 7) % (n / 2) : n / 2 + i), Boom(10 * i + 1)));
  }
  const long live = Boom::live.load();
  const std::string t = "exception from " + std::string(op == Boom::HASH ? "std::hash" : op == Boom::EQ ? "operator==" : op == Boom::LESS ? "operator<" : "payload copy") +
                        ", threads=" + std::to_string(threads);
  typedef HashMergeJoin<Rel::const_iterator, Rel::const_iterator> J;
  bool caught = false;
  Boom::countdown = 1000;
  Boom::armed = op;
  try {
    J j(r.cbegin(), r.cend(), s.cbegin(), s.cend(), threads);
  } catch (const BoomError&) {
    caught = true;
  }
  Boom::armed = 0;
  expect(caught, t + ": the exception reached the caller");
  expect(Boom::live.load() == live, t + ": no object leaked");
  // a later join on the same thread succeeds
  std::vector<Boom> rk, sk;
  std::vector<uint64_t> rh;
  for (const auto& row : r) rk.push_back(row.first), rh.push_back((uint64_t)std::hash<Boom>()(row.first));
  for (const auto& row : s) sk.push_back(row.first);
  const std::vector<RowPair> want = hashed_pairs(rk, rh, sk);
  J j(r.cbegin(), r.cend(), s.cbegin(), s.cend(), threads);
  expect(hashed_ok(j, want, [&](std::size_t i) { return &r[i].first; }, [&](std::size_t i) { return r[i].second; },
                   [&](std::size_t q) { return s[q].second; }),
         t + ": the next join");
}

static void prehashed_exception_case(unsigned threads) {
  typedef std::vector<std::tuple<std::size_t, Boom, uint64_t>> Buf;
  const std::size_t n = threads > 1 ? 1u << 17 : 1u << 12;
  Buf r, s;
  for (std::size_t i = 0; i < n; i++) {  // (hash = key / 2: pairs of different keys to drop, and n / 2 equal-key pairs)
    r.push_back(std::make_tuple((std::size_t)(i / 2), Boom(i), (uint64_t)i));
    s.push_back(std::make_tuple((std::size_t)((n / 2 + i) / 2), Boom(n / 2 + i), (uint64_t)i));
  }
  const long live = Boom::live.load();
  typedef HashMergeJoin2<Buf::iterator, Buf::iterator> J;
  bool caught = false;
  Boom::countdown = 1000;
  Boom::armed = Boom::EQ;
  try {
    J j(r.begin(), r.end(), s.begin(), s.end(), threads);
  } catch (const BoomError&) {
    caught = true;
  }
  Boom::armed = 0;
  const std::string t = "HashMergeJoin2, exception from operator==, threads=" + std::to_string(threads);
  expect(caught, t + ": the exception reached the caller");
  expect(Boom::live.load() == live, t + ": no object leaked");
  J j(r.begin(), r.end(), s.begin(), s.end(), threads);
  expect(j.size() == n / 2, t + ": the next join");
}

// ---- errors of the C ABI ---------------------------------------------------------------------------------------------
template <typename Fn>
static void error_case(const char* call, int nth, int code, Fn join) {
  hmj_stub_fail(nth, code);
  std::string msg;
  try {
    join();
  } catch (const std::runtime_error& e) {
    msg = e.what();
  }
  hmj_stub_fail(0, 0);
  expect(msg.find(hmj_strerror(code)) != std::string::npos && msg.find(call) != std::string::npos,
         std::string("an error of ") + call + " surfaces as std::runtime_error with hmj_strerror's text (got \"" + msg + "\")");
  bool ok = true;
  try {
    join();
  } catch (const std::exception&) {
    ok = false;
  }
  expect(ok, std::string("a join after an error of ") + call);
}

static void error_cases() {
  const U64Vec r = {{1, 10}, {2, 20}, {3, 30}}, s = {{2, 7}, {3, 8}, {4, 9}};
  const StrVec rs = {{"a", 1}, {"b", 2}}, ss = {{"b", 3}};
  typedef std::vector<std::tuple<std::size_t, uint64_t, uint64_t>> Buf;
  typedef std::vector<std::tuple<std::size_t, std::string, uint64_t>> SBuf;
  Buf br = {std::make_tuple(3, 3, 0), std::make_tuple(1, 1, 1)}, bs = {std::make_tuple(1, 1, 5)};
  SBuf sr = {std::make_tuple(9, "z", 0), std::make_tuple(2, "y", 1)}, sq = {std::make_tuple(2, "y", 4)};
  auto native = [&]() { HashMergeJoin<U64Vec::const_iterator, U64Vec::const_iterator> j(r.begin(), r.end(), s.begin(), s.end()); };
  auto hashed = [&]() { HashMergeJoin<StrVec::const_iterator, StrVec::const_iterator> j(rs.begin(), rs.end(), ss.begin(), ss.end()); };
  native();  // this thread's ctx exists from here on: hmj_create is not among the next calls
  // status calls per join: native and hashed: hmj_set_host_threads, hmj_join_u64_rows; the sum: hmj_join_u64;
  // HashMergeJoin2: the sort of each buffer (hmj_sort_rows_by_u64_host / hmj_argsort_u64_host), then the two join calls
  error_case("hmj_set_host_threads", 1, HMJ_E_ARG, native);
  error_case("hmj_join_u64_rows", 2, HMJ_E_OOM, native);
  error_case("hmj_join_u64_rows", 2, HMJ_E_HIP, hashed);
  error_case("hmj_join_u64", 1, HMJ_E_NODEV, [&]() { (void)hash_merge_join_sum(r.begin(), r.end(), s.begin(), s.end()); });
  error_case("hmj_sort_rows_by_u64_host", 1, HMJ_E_UNSUPPORTED,
             [&]() { HashMergeJoin2<Buf::iterator, Buf::iterator> j(br.begin(), br.end(), bs.begin(), bs.end()); });
  error_case("hmj_argsort_u64_host", 1, HMJ_E_OOM,
             [&]() { HashMergeJoin2<SBuf::iterator, SBuf::iterator> j(sr.begin(), sr.end(), sq.begin(), sq.end()); });
  error_case("hmj_join_u64_rows", 3, HMJ_E_HIP,
             [&]() { HashMergeJoin2<Buf::iterator, Buf::iterator> j(br.begin(), br.end(), bs.begin(), bs.end()); });
  // hmj_create: the first join of a new thread creates that thread's ctx
  std::string msg;
  std::thread t([&]() {
    hmj_stub_fail(1, HMJ_E_NODEV);
    try {
      native();
    } catch (const std::runtime_error& e) {
      msg = e.what();
    }
    hmj_stub_fail(0, 0);
    try {
      native();
    } catch (const std::exception&) {
      msg += " / the next join failed";
    }
  });
  t.join();
  expect(msg.find("hmj_create") != std::string::npos && msg.find(hmj_strerror(HMJ_E_NODEV)) != std::string::npos &&
             msg.find("next join") == std::string::npos,
         "an error of hmj_create surfaces and the thread's next join succeeds (got \"" + msg + "\")");
}

// ---- two threads at once, each with its own ctx and scratch buffer -----------------------------------------------------
static void two_threads_case() {
  struct Out {
    hmj_ctx* ctx = nullptr;
    const uint64_t* scratch = nullptr;
    bool ok = false;
  } out[2];
  auto work = [](int id, Out* o) {
    const std::size_t n = 1u << 17;
    StrVec r(n), s(n);
    U64Vec a(n), b(n);
    for (std::size_t i = 0; i < n; i++) {
      r[i] = std::make_pair(str_key(mix64(i + id) % n), i);
      s[i] = std::make_pair(str_key((i * 5 + id) % n), i);
      a[i] = std::make_pair(mix64(i * 3 + id), i);
      b[i] = std::make_pair(mix64(i + id), i);
    }
    std::vector<std::string> rk, sk;
    std::vector<uint64_t> rh;
    for (const auto& row : r) rk.push_back(row.first), rh.push_back((uint64_t)std::hash<std::string>()(row.first));
    for (const auto& row : s) sk.push_back(row.first);
    const std::vector<RowPair> want = hashed_pairs(rk, rh, sk);
    const std::vector<Row3> want_n = native_rows(a.begin(), a.end(), b.begin(), b.end());
    bool ok = true;
    for (int it = 0; it < 2; it++) {
      HashMergeJoin<StrVec::const_iterator, StrVec::const_iterator> j(r.cbegin(), r.cend(), s.cbegin(), s.cend(), 4);
      ok = ok && hashed_ok(j, want, [&](std::size_t i) { return &r[i].first; }, [&](std::size_t i) { return r[i].second; },
                           [&](std::size_t q) { return s[q].second; });
      HashMergeJoin<U64Vec::const_iterator, U64Vec::const_iterator> k(a.cbegin(), a.cend(), b.cbegin(), b.cend(), 4);
      ok = ok && native_ok(k, want_n);
    }
    o->ok = ok;
    o->ctx = hmj_detail::thread_ctx();
    o->scratch = hmj_detail::hash_scratch(1);
  };
  std::thread t0(work, 0, &out[0]), t1(work, 1, &out[1]);
  t0.join();
  t1.join();
  expect(out[0].ok && out[1].ok, "two threads joining at once");
  expect(out[0].ctx != out[1].ctx && out[0].scratch != out[1].scratch, "each thread has its own ctx and scratch buffer");
}

int main() {
  typedef std::vector<std::tuple<std::size_t, uint64_t, uint64_t>> Buf;
  typedef std::vector<std::tuple<std::size_t, std::string, uint64_t>> SBuf;
  for (const Size& z : kSizes) {
    string_case(z, true);
    string_case(z, false);
    native_case(z, false);
    native_case(z, true);
    const bool big = z.nr > 65536;
    if (big)
      colliding_case<32749>(z);  // (v % 7 would pair up 2^34 / 7 rows)
    else
      colliding_case<7>(z);
    const uint64_t mod = big ? 65521 : 997;
    prehashed_case<Buf>("HashMergeJoin2, hash = key % 997 (65521 at 2^17 rows)", z, [mod](uint64_t k, uint64_t v) {
      return std::make_tuple((std::size_t)(k % mod), k, v);
    });
    prehashed_case<SBuf>("HashMergeJoin2, std::string keys", z, [](uint64_t k, uint64_t v) {
      const std::string key = str_key(k);
      return std::make_tuple(std::hash<std::string>()(key), key, v);
    });
  }
  for (unsigned threads : {1u, 8u})
    for (int op : {(int)Boom::HASH, (int)Boom::EQ, (int)Boom::LESS, (int)Boom::COPY}) exception_case(op, threads);
  prehashed_exception_case(1);
  prehashed_exception_case(8);
  error_cases();
  two_threads_case();
  std::printf(g_fails ? "FAILED (%d)\n" : "all host drop-in cases passed\n", g_fails);
  return g_fails ? 1 : 0;
}
