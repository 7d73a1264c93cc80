#!/usr/bin/env python3
"""Time grouping by multi-column keys on the device (hmj_group_cols_device) beside its floor and its yardsticks.  One JSON line.

  Shapes: [4,4] (the packed form) and [8,4,2] (the hashed form), 2^24 and 2^26 rows; the rows draw their tuple from 2^4,
  2^12 or 2^20 distinct tuples, or are all distinct.  Two calls per input: COUNT only (HMJ_MATERIALIZE, want = COUNT) and
  everything (want = COUNT | SUM | MIN | MAX | ROW_MAP over a random payload column).  Per input:

  count_ms / all_ms   median of --reps device-timed calls (HIP events around the call) after --warmup, profiling off
  phases_ms           median hmj_group_opts ms_key / ms_sort / ms_groups / ms_agg of the everything call (profiling on,
                      separate calls)
  sort_floor_ms       hmj_sort_u64_device on the pre-built {key64,row} rows, same process, timed the same way: the floor a
                      design that sorts cannot beat
  take_ms             hmj_take_cols_device of the payload column through a random map of n rows: the yardstick of the
                      aggregate's 8-byte gather
  torch_unique_ms     torch.unique(..., return_inverse=True, return_counts=True) on the same keys: the packed u64 key for
                      [4,4], dim=0 over the three columns for [8,4,2] (null where torch runs out of memory)

  There is no gate.  The inputs are drawn on the device; the tool checks n_groups against torch.unique and the key64 it
  builds for the floor against cols_key64 on a sample.

    python tools/bench_group_cols.py [--reps 20] [--warmup 3] [--log2 24 26]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPES = (("4_4", [4, 4]), ("8_4_2", [8, 4, 2]))


def signed(x):
    return x - (1 << 64) if x >= (1 << 63) else x


def timed(torch, fn, reps, warmup):
    out = None
    for _ in range(warmup):
        out = fn()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), out


def lsr(x, k):
    """Logical right shift of int64 tensors holding uint64 bits."""
    return (x >> k) & ((1 << (64 - k)) - 1)


def mix64(x):
    x = x ^ lsr(x, 30)
    x = x * signed(0xBF58476D1CE4E5B9)
    x = x ^ lsr(x, 27)
    x = x * signed(0x94D049BB133111EB)
    return x ^ lsr(x, 31)


def columns_of(torch, ids, widths):
    """bench_join_cols.py's columns, on the device (int64 ids; signed dtypes of the widths, compared bit for bit)."""
    if widths == [4, 4]:
        return [((ids >> 12) * 2654435761).to(torch.int32), ids.to(torch.int32)]
    return [ids * signed(0x9E3779B97F4A7C15), (ids % 36500).to(torch.int32), (ids & 0xFFFF).to(torch.int16)]


def key64_of(torch, cols, widths):
    """cols_key64 on the device: the packed tuple for [4,4], the hash chain for [8,4,2]."""
    u = [c.to(torch.int64) & ((1 << (8 * w)) - 1) if w < 8 else c for c, w in zip(cols, widths)]
    if sum(widths) <= 8:
        key = torch.zeros_like(u[0])
        for v, w in zip(u, widths):
            key = (key << (8 * w)) | v
        return key
    h = torch.full_like(u[0], len(widths))
    for v in u:
        h = mix64(h + v + signed(0x9E3779B97F4A7C15))
    return h


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--log2", type=int, nargs="+", default=[24, 26])
    args = ap.parse_args()
    import torch

    import hashmergejoin_amd as H

    assert torch.cuda.is_available(), "bench_group_cols needs a GPU"
    ex = H.Executor(0)
    out = {"tool": "bench_group_cols", "reps": args.reps, "warmup": args.warmup, "device": torch.cuda.get_device_name(0)}
    everything = H.HMJ_GROUP_COUNT | H.HMJ_GROUP_SUM | H.HMJ_GROUP_MIN | H.HMJ_GROUP_MAX | H.HMJ_GROUP_ROW_MAP
    gen = torch.Generator(device="cuda")
    for lg in args.log2:
        n = 1 << lg
        for name, widths in SHAPES:
            for dl in (4, 12, 20, None):
                gen.manual_seed(lg * 100 + (dl or 99))
                if dl is None:
                    ids = torch.randperm(n, device="cuda", generator=gen)
                else:
                    ids = torch.randint(0, 1 << dl, (n,), device="cuda", generator=gen)
                cols = columns_of(torch, ids, widths)
                vals = torch.randint(-(1 << 63), (1 << 63) - 1, (n,), device="cuda", generator=gen)
                key = key64_of(torch, cols, widths)
                sample = [c[:1000].cpu().numpy() for c in cols]
                assert np.array_equal(key[:1000].cpu().numpy().view(np.uint64), H.cols_key64(sample, widths)), "key64 of the floor"
                rows = torch.stack([key, torch.arange(n, device="cuda")], 1).contiguous()
                rmap = torch.randperm(n, device="cuda", generator=gen)
                del ids
                ex.set_profiling(False)
                count_ms, (res, info) = timed(torch, lambda: ex.group_cols_device(cols, None, None, H.HMJ_MATERIALIZE, H.HMJ_GROUP_COUNT),
                                              args.reps, args.warmup)
                all_ms, (res, info) = timed(torch, lambda: ex.group_cols_device(cols, vals, None, H.HMJ_MATERIALIZE, everything),
                                            args.reps, args.warmup)
                n_groups, max_count = int(res.n_groups), int(res.max_count)
                ex.set_profiling(True)
                ph = {k: [] for k in ("ms_key", "ms_sort", "ms_groups", "ms_agg")}
                for _ in range(max(5, args.reps // 2)):
                    _, inf = ex.group_cols_device(cols, vals, None, H.HMJ_MATERIALIZE, everything)
                    for k in ph:
                        ph[k].append(inf[k])
                ex.set_profiling(False)
                ex.release_result()
                floor_ms, _ = timed(torch, lambda: ex.sort_device(rows), args.reps, args.warmup)
                take_ms, _ = timed(torch, lambda: ex.take_cols_device([vals], rmap, want_validity=False), args.reps, args.warmup)
                del rows, rmap
                torch.cuda.empty_cache()
                row = {"form": "packed" if info["form"] == H.HMJ_COLS_PACKED else "hashed", "n_groups": n_groups, "max_count": max_count,
                       "n_collisions": info["n_collisions"], "count_ms": round(count_ms, 4), "all_ms": round(all_ms, 4),
                       "phases_ms": {k: round(statistics.median(v), 4) for k, v in ph.items()}, "sort_floor_ms": round(floor_ms, 4),
                       "take_ms": round(take_ms, 4), "count_vs_floor": round(count_ms / floor_ms, 3)}
                try:
                    if sum(widths) <= 8:
                        fn = lambda: torch.unique(key, return_inverse=True, return_counts=True)
                    else:
                        wide = torch.stack([c.to(torch.int64) for c in cols], 1).contiguous()
                        fn = lambda: torch.unique(wide, dim=0, return_inverse=True, return_counts=True)
                    t_ms, (u, _, _) = timed(torch, fn, args.reps, args.warmup)
                    assert u.shape[0] == n_groups, (u.shape[0], n_groups)
                    row["torch_unique_ms"] = round(t_ms, 4)
                    row["all_vs_torch_unique"] = round(all_ms / t_ms, 3)
                    del u
                except torch.OutOfMemoryError:
                    row["torch_unique_ms"] = None
                wide = None
                out["%s_2^%d_distinct_%s" % (name, lg, "all" if dl is None else "2^%d" % dl)] = row
                del cols, vals, key
                torch.cuda.empty_cache()
    ex.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
