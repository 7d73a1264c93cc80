// hmj_abi_stub.cc -- a host-only implementation of the ten calls of hmj.h that include/hashmergejoin_hip.hpp makes,
// so that the drop-in operator can be built and run under AddressSanitizer / ThreadSanitizer without a GPU
// (tests/cpp/test_dropin_host.cc, tests/test_dropin_host_cpu.py).  Test infrastructure only: no product target links it.
//
//   hmj_create / hmj_destroy / hmj_strerror / hmj_last_error / hmj_set_host_threads
//   hmj_join_u64_rows + hmj_rows_free    sort-merge equi-join, full cross product per key, rows in (key, rval, sval)
//                                        order (HMJ_ORDERED, hmj.h); every column its own heap allocation
//   hmj_join_u64                         the same join, count and sums only
//   hmj_sort_rows_by_u64_host            stable in-place sort of fixed-size rows on a u64 field
//   hmj_argsort_u64_host                 stable argsort of strided u64 keys
//
// hmj_stub_fail(nth, code): the nth status-returning call from now on (1 = the next one) returns `code` instead of doing
// its work; nth = 0 disarms.  A ctx used by two threads at once is reported and aborts the process (hmj.h: an hmj_ctx is
// not thread-safe).
#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "hmj.h"

struct hmj_ctx {
  std::atomic<int> busy{0};
  int host_threads = 8;
  std::string last_error;
};
struct hmj_rows {
  std::vector<uint64_t> key, rval, sval;
};

namespace {

std::atomic<long> g_fail_countdown{0};
std::atomic<int> g_fail_code{0};

// one status-returning call: true if this is the call hmj_stub_fail picked
bool injected(int* code) {
  long left = g_fail_countdown.load();
  while (left > 0)
    if (g_fail_countdown.compare_exchange_weak(left, left - 1)) {
      if (left == 1) {
        *code = g_fail_code.load();
        return true;
      }
      return false;
    }
  return false;
}

struct Use {  // marks the ctx busy for the duration of one call
  hmj_ctx* c;
  explicit Use(hmj_ctx* ctx) : c(ctx) {
    if (c && c->busy.exchange(1)) {
      std::fprintf(stderr, "hmj_abi_stub: hmj_ctx %p used by two threads at once\n", (void*)c);
      std::abort();
    }
  }
  ~Use() {
    if (c) c->busy.store(0);
  }
};

int fail(hmj_ctx* c, int code, const char* what) {
  if (c) c->last_error = what;
  return code;
}

struct Row {
  uint64_t key, val;
};
std::vector<Row> load(const void* p, uint64_t n) {
  std::vector<Row> v(n);
  if (n) std::memcpy(v.data(), p, n * sizeof(Row));
  return v;
}

// every (build row, probe row) pair of equal keys, ascending (key, rval, sval)
template <typename Emit>
void merge_join(const void* build, uint64_t nb, const void* probe, uint64_t np, Emit emit) {
  std::vector<Row> b = load(build, nb), p = load(probe, np);
  auto by_key_val = [](const Row& x, const Row& y) { return x.key != y.key ? x.key < y.key : x.val < y.val; };
  std::sort(b.begin(), b.end(), by_key_val);
  std::sort(p.begin(), p.end(), by_key_val);
  std::size_t i = 0, j = 0;
  while (i < b.size() && j < p.size()) {
    if (b[i].key < p[j].key) {
      i++;
    } else if (p[j].key < b[i].key) {
      j++;
    } else {
      std::size_t ie = i, je = j;
      while (ie < b.size() && b[ie].key == b[i].key) ie++;
      while (je < p.size() && p[je].key == p[j].key) je++;
      for (std::size_t x = i; x < ie; x++)
        for (std::size_t y = j; y < je; y++) emit(b[x].key, b[x].val, p[y].val);
      i = ie;
      j = je;
    }
  }
}

bool bad_relation(const void* p, uint64_t n) { return (n && !p) || n > 0xFFFFFFFFull; }

// a stable order of n u64 keys at `keys + i * stride`
std::vector<uint32_t> stable_order(const unsigned char* keys, uint64_t n, uint32_t stride) {
  std::vector<uint64_t> k(n);
  for (uint64_t i = 0; i < n; i++) std::memcpy(&k[i], keys + i * stride, 8);
  std::vector<uint32_t> perm(n);
  for (uint64_t i = 0; i < n; i++) perm[i] = (uint32_t)i;
  std::stable_sort(perm.begin(), perm.end(), [&](uint32_t a, uint32_t b) { return k[a] < k[b]; });
  return perm;
}

}  // namespace

extern "C" void hmj_stub_fail(int nth_call, int code) {
  g_fail_code.store(code);
  g_fail_countdown.store(nth_call > 0 ? nth_call : 0);
}

int hmj_create(hmj_ctx** out, int) {
  int code;
  if (injected(&code)) return code;
  if (!out) return HMJ_E_ARG;
  *out = new hmj_ctx;
  return HMJ_OK;
}

void hmj_destroy(hmj_ctx* ctx) {
  { Use u(ctx); }
  delete ctx;
}

const char* hmj_strerror(int code) {
  switch (code) {
    case HMJ_OK: return "ok";
    case HMJ_E_ARG: return "invalid argument";
    case HMJ_E_NODEV: return "no usable HIP device";
    case HMJ_E_OOM: return "out of device or pinned host memory";
    case HMJ_E_HIP: return "HIP runtime error";
    case HMJ_E_UNSUPPORTED: return "unsupported flag combination for this input";
    default: return "unknown error";
  }
}

const char* hmj_last_error(hmj_ctx* ctx) { return ctx ? ctx->last_error.c_str() : ""; }

int hmj_set_host_threads(hmj_ctx* ctx, int n) {
  Use u(ctx);
  int code;
  if (injected(&code)) return fail(ctx, code, "injected failure in hmj_set_host_threads");
  if (!ctx || n < 0 || n > 64) return HMJ_E_ARG;
  ctx->host_threads = n;
  return HMJ_OK;
}

int hmj_join_u64_rows(hmj_ctx* ctx, const void* build, uint64_t nb, const void* probe, uint64_t np, uint32_t flags,
                      hmj_result* out, hmj_rows** rows) {
  Use u(ctx);
  int code;
  if (injected(&code)) return fail(ctx, code, "injected failure in hmj_join_u64_rows");
  if (!ctx || !out || !rows || bad_relation(build, nb) || bad_relation(probe, np))
    return fail(ctx, HMJ_E_ARG, "hmj_join_u64_rows: bad argument");
  (void)flags;  // always materialised and ordered
  hmj_rows* r = new hmj_rows;
  std::memset(out, 0, sizeof(*out));
  merge_join(build, nb, probe, np, [&](uint64_t k, uint64_t rv, uint64_t sv) {
    r->key.push_back(k);
    r->rval.push_back(rv);
    r->sval.push_back(sv);
    out->sum_r += rv;
    out->sum_s += sv;
  });
  // exactly n words per column, so that a read past the end is caught too
  r->key.shrink_to_fit();
  r->rval.shrink_to_fit();
  r->sval.shrink_to_fit();
  out->n_matches = r->key.size();
  out->key = r->key.data();
  out->rval = r->rval.data();
  out->sval = r->sval.data();
  *rows = r;
  return HMJ_OK;
}

void hmj_rows_free(hmj_rows* rows) { delete rows; }

int hmj_join_u64(hmj_ctx* ctx, const void* build, uint64_t nb, const void* probe, uint64_t np, uint32_t flags,
                 hmj_result* out) {
  Use u(ctx);
  int code;
  if (injected(&code)) return fail(ctx, code, "injected failure in hmj_join_u64");
  if (!ctx || !out || bad_relation(build, nb) || bad_relation(probe, np) || (flags & (HMJ_MATERIALIZE | HMJ_ORDERED)))
    return fail(ctx, HMJ_E_ARG, "hmj_join_u64: bad argument (the stub joins count / sum only)");
  std::memset(out, 0, sizeof(*out));
  merge_join(build, nb, probe, np, [&](uint64_t, uint64_t rv, uint64_t sv) {
    out->n_matches++;
    out->sum_r += rv;
    out->sum_s += sv;
  });
  return HMJ_OK;
}

int hmj_sort_rows_by_u64_host(hmj_ctx* ctx, void* rows_host, uint64_t n, uint32_t row_bytes, uint32_t key_offset) {
  Use u(ctx);
  int code;
  if (injected(&code)) return fail(ctx, code, "injected failure in hmj_sort_rows_by_u64_host");
  if (!ctx || bad_relation(rows_host, n) || row_bytes % 8 || row_bytes < 16 || row_bytes > 64 || key_offset % 8 ||
      key_offset + 8 > row_bytes)
    return fail(ctx, HMJ_E_ARG, "hmj_sort_rows_by_u64_host: bad argument");
  unsigned char* base = static_cast<unsigned char*>(rows_host);
  const std::vector<uint32_t> perm = stable_order(base + key_offset, n, row_bytes);
  std::vector<unsigned char> tmp((std::size_t)n * row_bytes);
  for (uint64_t i = 0; i < n; i++) std::memcpy(&tmp[i * row_bytes], base + (std::size_t)perm[i] * row_bytes, row_bytes);
  if (n) std::memcpy(base, tmp.data(), tmp.size());
  return HMJ_OK;
}

int hmj_argsort_u64_host(hmj_ctx* ctx, const void* keys_host, uint64_t n, uint32_t stride_bytes, uint32_t* perm_out) {
  Use u(ctx);
  int code;
  if (injected(&code)) return fail(ctx, code, "injected failure in hmj_argsort_u64_host");
  if (!ctx || bad_relation(keys_host, n) || (n && !perm_out) || stride_bytes < 8)
    return fail(ctx, HMJ_E_ARG, "hmj_argsort_u64_host: bad argument");
  const std::vector<uint32_t> perm = stable_order(static_cast<const unsigned char*>(keys_host), n, stride_bytes);
  if (n) std::memcpy(perm_out, perm.data(), n * sizeof(uint32_t));
  return HMJ_OK;
}
