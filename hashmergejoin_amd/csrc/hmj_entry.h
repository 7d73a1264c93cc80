// What the body of an entry shares with every other entry and needs the ctx for: recording its phase events, reading its
// counters back, and filling the ms_* fields of the join and group opts.  Internal header.
#pragma once
#include "hmj_ctx.h"

namespace hmj_host {

template <int N>
int PhaseEvents<N>::record(hmj_ctx* c, int k) {
  if (!c->profiling) return HMJ_OK;
  if (!ev[k]) HIP_TRY(hipEventCreate(&ev[k]));
  HIP_TRY(hipEventRecord(ev[k], c->stream));
  return HMJ_OK;
}

// counters to the host; the stream is idle when this returns
inline int read_back(hmj_ctx* c, const void* dev, void* host, size_t bytes) {
  HIP_TRY(hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return HMJ_OK;
}

// The phase times of a key join (profiling only): events 0..3 bound key, join and verify; behind them the inner join
// orders, a kind emits and then orders.  ms_first: the opts family's name of the key phase, o.ms_hash or o.ms_key.
template <class Opts>
void fill_join_ms(hmj_ctx* c, Opts& o, float& ms_first, PhaseEvents<6>& ev, bool with_emit = false) {
  if (!c->profiling) return;
  (void)hipStreamSynchronize(c->stream);
  ms_first = ev.ms(0, 1);
  o.ms_join = ev.ms(1, 2);
  o.ms_verify = ev.ms(2, 3);
  o.ms_order = with_emit ? ev.ms(4, 5) : ev.ms(3, 4);
}
template <class Opts>
void fill_kind_ms(hmj_ctx* c, Opts& o, float& ms_first, PhaseEvents<6>& ev, bool with_emit) {
  fill_join_ms(c, o, ms_first, ev, with_emit);
  if (c->profiling && with_emit) o.ms_emit = ev.ms(3, 4);
}
inline void fill_group_ms(hmj_ctx* c, hmj_group_opts& o) {
  if (!c->profiling) return;
  (void)hipStreamSynchronize(c->stream);
  PhaseEvents<5>& ev = c->grp_ws.ev;
  o.ms_key = ev.ms(0, 1);
  o.ms_sort = ev.ms(1, 2);
  o.ms_groups = ev.ms(2, 3);
  o.ms_agg = ev.ms(3, 4);
}

}  // namespace hmj_host
