#!/usr/bin/env python3
"""Time hmj_group_agg_device -- typed columns aggregated over a grouping -- beside the group call's own aggregate kernel and
the take yardstick.  One JSON line.

  Inputs: 2^24 and 2^26 rows grouped by one uint64 key column (packed form, unordered) that draws its key from 2^4, 2^12 or
  2^20 distinct keys, or is all distinct.  Per input, all in one process on one ctx:

  (a) u64_sum_min_max   one U64 column under SUM + MIN + MAX through the new entry: agg_ms (median hmj_group_agg_opts.ms_agg,
                        profiling on) and call_ms (median wall time of the call, HIP events around it, profiling off), beside
                        group_ms_agg -- hmj_group_opts.ms_agg of hmj_group_cols_device with want = SUM | MIN | MAX over the
                        same column: group_agg_kernel doing the same reduction with one atomic per wave boundary.  The
                        three output columns are compared with the group call's (inputs up to 2^20 groups).
  (b) four_columns      I32 SUM, F64 MEAN, I64 MIN and F32 SUM: one call of four against four calls of one (agg_ms summed).
  (c) the 2^4-group rows are the giant-group case: their waves all hand partials to the combine step; nothing else differs.
  (d) take_ms           hmj_take_cols_device of the same four columns through a random map of n rows, no bitmaps: what
                        gathering these bytes once costs.

  There is no gate.

    python tools/bench_group_agg.py [--reps 10] [--warmup 2] [--log2 24 26]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


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


def agg_ms(ex, aggs, reps, warmup):
    """Median ms_agg of the call (profiling on)."""
    ex.set_profiling(True)
    ms = []
    for k in range(warmup + reps):
        _, info = ex.group_agg_device(aggs, want_validity=False)
        if k >= warmup:
            ms.append(info["ms_agg"])
    ex.set_profiling(False)
    return statistics.median(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--log2", type=int, nargs="+", default=[24, 26])
    args = ap.parse_args()
    import torch

    import hashmergejoin_amd as H

    assert torch.cuda.is_available(), "bench_group_agg needs a GPU"
    ex = H.Executor(0)
    out = {"tool": "bench_group_agg", "reps": args.reps, "warmup": args.warmup, "device": torch.cuda.get_device_name(0)}
    gen = torch.Generator(device="cuda")
    S, MN, MX, ME = H.HMJ_AGG_SUM, H.HMJ_AGG_MIN, H.HMJ_AGG_MAX, H.HMJ_AGG_MEAN
    smm = H.HMJ_GROUP_SUM | H.HMJ_GROUP_MIN | H.HMJ_GROUP_MAX
    for lg in args.log2:
        n = 1 << lg
        for dl in (4, 12, 20, None):
            gen.manual_seed(lg * 100 + (dl or 99))
            if dl is None:
                ids = torch.randperm(n, device="cuda", generator=gen)
            else:
                ids = torch.randint(0, 1 << dl, (n,), device="cuda", generator=gen)
            key = ids * -7046029254386353131  # (0x9E3779B97F4A7C15: odd, so distinct ids stay distinct)
            del ids
            vals = torch.randint(-(1 << 63), (1 << 63) - 1, (n,), device="cuda", generator=gen)
            u64 = vals.view(torch.uint64)
            i32 = torch.randint(-(1 << 31), (1 << 31) - 1, (n,), device="cuda", generator=gen, dtype=torch.int32)
            f64 = torch.randn(n, device="cuda", generator=gen, dtype=torch.float64)
            f32 = torch.randn(n, device="cuda", generator=gen, dtype=torch.float32)
            # the parent's kernel on the same reduction, then the live grouping every call below aggregates over
            ex.set_profiling(True)
            parent = []
            for k in range(args.warmup + args.reps):
                res, info = ex.group_cols_device([key], vals, None, H.HMJ_MATERIALIZE, smm)
                if k >= args.warmup:
                    parent.append(info["ms_agg"])
            ex.set_profiling(False)
            n_groups, max_count = int(res.n_groups), int(res.max_count)
            three = [(S, u64, None), (MN, u64, None), (MX, u64, None)]
            a_ms = agg_ms(ex, three, args.reps, args.warmup)
            a_call, (got, _) = timed(torch, lambda: ex.group_agg_device(three, want_validity=False), args.reps, args.warmup)
            same = None
            if n_groups <= 1 << 20:
                cols = ex.group_rows_to_numpy(res)
                same = all(np.array_equal(got[k][0].cpu().numpy(), cols[name]) for k, name in enumerate(("sum", "min", "max")))
                assert same, "the new entry and the group call disagree"
            four = [(S, i32, None), (ME, f64, None), (MN, vals, None), (S, f32, None)]
            b_one = agg_ms(ex, four, args.reps, args.warmup)
            b_four = sum(agg_ms(ex, [a], args.reps, args.warmup) for a in four)
            b_call, _ = timed(torch, lambda: ex.group_agg_device(four, want_validity=False), args.reps, args.warmup)
            rmap = torch.randperm(n, device="cuda", generator=gen)
            take_ms, _ = timed(torch, lambda: ex.take_cols_device([i32, f64, vals, f32], rmap, want_validity=False), args.reps, args.warmup)
            del rmap
            ex.release_result()
            out["2^%d_distinct_%s" % (lg, "all" if dl is None else "2^%d" % dl)] = {
                "n_groups": n_groups, "max_count": max_count,
                "u64_sum_min_max": {"agg_ms": round(a_ms, 4), "call_ms": round(a_call, 4), "group_ms_agg": round(statistics.median(parent), 4),
                                    "agg_vs_group": round(a_ms / statistics.median(parent), 3), "same_as_group_call": same},
                "four_columns": {"one_call_agg_ms": round(b_one, 4), "four_calls_agg_ms": round(b_four, 4), "call_ms": round(b_call, 4)},
                "take_ms": round(take_ms, 4), "four_vs_take": round(b_one / take_ms, 3)}
            del key, vals, u64, i32, f64, f32, got
            torch.cuda.empty_cache()
    ex.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
