// dropin_checks.h -- what the C++ drop-in operator (include/hashmergejoin_hip.hpp) must yield, computed here by brute force
// over std::multimap / std::map and never by the code under test, and the value-semantics walk every join class goes
// through.  Shared by the host-only test against the ABI stub (test_dropin_host.cc) and the GPU test (test_dropin.cc).
#ifndef HMJ_DROPIN_CHECKS_H
#define HMJ_DROPIN_CHECKS_H

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <functional>
#include <map>
#include <tuple>
#include <utility>
#include <vector>

namespace dropin_checks {

inline uint64_t mix64(uint64_t x) {  // splitmix64's finaliser
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

// A key whose std::hash sends every key to one of Mod values, so that different keys share a hash: the operator must drop
// the pairs of different keys the GPU pairs up and order each hash group by key.
template <unsigned Mod>
struct ModKey {
  uint64_t v;
  bool operator==(const ModKey& o) const { return v == o.v; }
  bool operator<(const ModKey& o) const { return v < o.v; }
};

typedef std::tuple<uint64_t, uint64_t, uint64_t> Row3;
typedef std::pair<std::size_t, std::size_t> RowPair;

// uint64_t keys: (key, r payload, s payload) of every pair of equal keys, ascending -- the native operator's order
template <typename RIt, typename SIt>
std::vector<Row3> native_rows(RIt rb, RIt re, SIt sb, SIt se) {
  std::multimap<uint64_t, uint64_t> m;
  for (RIt i = rb; i != re; ++i) m.insert(std::make_pair((uint64_t)i->first, (uint64_t)i->second));
  std::vector<Row3> v;
  for (SIt j = sb; j != se; ++j) {
    auto range = m.equal_range(j->first);
    for (auto it = range.first; it != range.second; ++it) v.push_back(Row3(j->first, it->second, (uint64_t)j->second));
  }
  std::sort(v.begin(), v.end());
  return v;
}

// hashed keys: (r row, s row) of every pair of equal keys in the order (hash, key, r row, s row); rh[i] is r row i's hash
template <typename Key>
std::vector<RowPair> hashed_pairs(const std::vector<Key>& rk, const std::vector<uint64_t>& rh, const std::vector<Key>& sk) {
  std::map<Key, std::vector<std::size_t>> rows;
  for (std::size_t i = 0; i < rk.size(); i++) rows[rk[i]].push_back(i);
  std::vector<RowPair> v;
  for (std::size_t j = 0; j < sk.size(); j++) {
    auto it = rows.find(sk[j]);
    if (it != rows.end())
      for (std::size_t i : it->second) v.push_back(RowPair(i, j));
  }
  std::sort(v.begin(), v.end(), [&](const RowPair& a, const RowPair& b) {
    if (rh[a.first] != rh[b.first]) return rh[a.first] < rh[b.first];
    if (rk[a.first] < rk[b.first]) return true;
    if (rk[b.first] < rk[a.first]) return false;
    return a < b;
  });
  return v;
}

// a native join yields exactly `want`, in order
template <typename J>
bool native_ok(J& j, const std::vector<Row3>& want) {
  if (j.size() != want.size()) return false;
  std::size_t k = 0;
  for (auto t : j) {
    if (k >= want.size() || Row3(*std::get<0>(t), (uint64_t)*std::get<1>(t), (uint64_t)*std::get<2>(t)) != want[k]) return false;
    k++;
  }
  return k == want.size();
}

// a hashed join yields the pairs `want`, in order: the key is the caller's r row's own (its address, key_at(i)), the
// payloads are those of r row i and s row j (rv_at(i), sv_at(j))
template <typename J, typename KeyAt, typename RvAt, typename SvAt>
bool hashed_ok(J& j, const std::vector<RowPair>& want, KeyAt key_at, RvAt rv_at, SvAt sv_at) {
  if (j.size() != want.size()) return false;
  std::size_t k = 0;
  for (auto t : j) {
    if (k >= want.size() || std::get<0>(t) != key_at(want[k].first) || !(*std::get<1>(t) == rv_at(want[k].first)) ||
        !(*std::get<2>(t) == sv_at(want[k].second)))
      return false;
    k++;
  }
  return k == want.size();
}

template <typename J>
bool empty_ok(J& j) {
  return j.size() == 0 && j.begin() == j.end();
}

// Every way a join object is copied, moved, assigned and cleared.  make() builds the join under test, other() a different
// non-empty join of the same type, ok(j) checks one object's rows.  A copy must stay whole after its source is cleared,
// reassigned or destroyed; a moved-from object is empty or still whole.  Returns the number of failed steps.
template <typename J, typename Make, typename Other, typename Ok>
int value_semantics(const char* what, Make make, Other other, Ok ok) {
  int fails = 0;
  auto expect = [&](bool good, const char* step) {
    if (!good) {
      std::printf("FAIL %s: %s\n", what, step);
      fails++;
    }
  };
  J* a = new J(make());
  expect(ok(*a), "constructed");
  J b(*a);
  delete a;
  expect(ok(b), "copy-construct, then the source destroyed");
  J c(b);
  b.clear();
  expect(ok(c), "copy-construct, then clear() on the source");
  expect(empty_ok(b), "clear()");
  J d(other());
  d = c;
  c = other();
  expect(ok(d), "copy-assign into a non-empty object, then the source reassigned");
  J e(std::move(d));
  expect(ok(e), "move-construct");
  expect(empty_ok(d) || ok(d), "moved-from object (move-construct)");
  J f(other());
  f = std::move(e);
  expect(ok(f), "move-assign");
  expect(empty_ok(e) || ok(e), "moved-from object (move-assign)");
  J& same = f;
  f = same;
  expect(ok(f), "self-assignment");
  J g;
  expect(empty_ok(g), "default-constructed");
  g = make();
  expect(ok(g), "j = Class(...)");
  {
    J h(g);
    g = J();
    expect(ok(h), "copy, then the source assigned an empty join");
    expect(empty_ok(g), "assigned an empty join");
  }
  return fails;
}

}  // namespace dropin_checks

namespace std {
template <unsigned Mod>
struct hash<dropin_checks::ModKey<Mod>> {
  size_t operator()(const dropin_checks::ModKey<Mod>& k) const { return (size_t)(k.v % Mod); }
};
}  // namespace std

#endif
