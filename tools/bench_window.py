#!/usr/bin/env python3
"""Time window functions over ordered partitions (hmj_window_device) beside their floor and their yardsticks.  One JSON line.

  Inputs: 2^24 and 2^26 rows, keys (I32 partition key, I64 order key); the rows draw their partition from 2^4, 2^12 or 2^20
  values, or are all distinct ("distinct"), or share one ("one").  Three function sets per input: ROW_NUMBER alone;
  CUM_SUM(I64); ROW_NUMBER + RANK + CUM_SUM(F64) + LAG(I32) in one call.  Per input and set:

  call_ms             median of --reps device-timed calls (HIP events around the call) after --warmup, profiling off
  phases_ms           median hmj_window_opts ms_order / ms_heads / ms_scan (profiling on, separate calls), and
                      heads_scan_ms = ms_heads + ms_scan: what the call adds to its ORDER BY
  order_by_ms         hmj_order_by_device on the same keys, same process, timed the same way: the call's floor, which
                      ms_order should match
  take_ms             hmj_take_cols_device of the set's source columns through the call's own row_map_out: the gather any
                      implementation pays (null for ROW_NUMBER alone, which reads no source)
  torch_ms            CUM_SUM(I64) only: the same result composed from torch ops -- a stable sort of the (partition, order)
                      composite, a gather, cumsum, and the partition's base taken back out through a cummax of the heads
                      (null where torch runs out of memory)

  There is no gate.  The inputs are drawn on the device; the tool checks CUM_SUM(I64) against the torch composition and
  ROW_NUMBER's last entry per partition against the partition sizes.  It needs a GPU: there is no fallback.

    python tools/bench_window.py [--reps 10] [--warmup 2] [--log2 24 26]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PARTITIONS = (("2^4", 4), ("2^12", 12), ("2^20", 20), ("distinct", None), ("one", 0))
SETS = ("row_number", "cum_sum_i64", "four")


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


def torch_cum_sum(torch, k, t, x):
    """CUM_SUM(x) OVER (PARTITION BY k ORDER BY t) in sorted order, and the order, from torch ops (t in [0, 2^31))."""
    comp = (k.to(torch.int64) << 32) | t
    comp, perm = torch.sort(comp, stable=True)
    xs = x[perm]
    cs = torch.cumsum(xs, 0)
    head = torch.ones_like(comp, dtype=torch.bool)
    head[1:] = (comp[1:] >> 32) != (comp[:-1] >> 32)
    pos = torch.arange(len(comp), device=comp.device)
    start = torch.cummax(torch.where(head, pos, torch.zeros_like(pos)), 0)[0]
    return cs - (cs - xs)[start], perm


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--log2", type=int, nargs="+", default=[24, 26])
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench_window.py needs a GPU")
    import hashmergejoin_amd as H

    ex = H.Executor(0)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(20261021)
    results = []
    for lg in args.log2:
        n = 1 << lg
        t = torch.randint(0, 1 << 31, (n,), device="cuda", generator=gen, dtype=torch.int64)
        x64 = torch.randint(-(1 << 40), 1 << 40, (n,), device="cuda", generator=gen, dtype=torch.int64)
        f64 = torch.randn(n, device="cuda", generator=gen, dtype=torch.float64)
        x32 = torch.randint(-(1 << 30), 1 << 30, (n,), device="cuda", generator=gen, dtype=torch.int32)
        for pname, bits in PARTITIONS:
            if bits is None:
                k = torch.randperm(n, device="cuda", generator=gen).to(torch.int32)
            elif bits == 0:
                k = torch.zeros(n, device="cuda", dtype=torch.int32)
            else:
                k = torch.randint(0, 1 << min(bits, lg), (n,), device="cuda", generator=gen, dtype=torch.int32)
            keys = [(k, 0), (t, 0)]
            order_ms, _ = timed(torch, lambda: ex.order_by_device(keys), args.reps, args.warmup)
            for sname in SETS:
                fns = {"row_number": [(H.HMJ_WIN_ROW_NUMBER, None)], "cum_sum_i64": [(H.HMJ_WIN_CUM_SUM, x64)],
                       "four": [(H.HMJ_WIN_ROW_NUMBER, None), (H.HMJ_WIN_RANK, None), (H.HMJ_WIN_CUM_SUM, f64),
                                (H.HMJ_WIN_LAG, x32, None, 0, 1)]}[sname]
                sources = [f[1] for f in fns if f[1] is not None]
                call = lambda: ex.window_device(keys, 1, fns, want_validity=True)  # noqa: E731
                call_ms, (rmap, outs, info) = timed(torch, call, args.reps, args.warmup)
                ex.set_profiling(True)
                phases = [call()[2] for _ in range(max(3, args.reps // 2))]
                ex.set_profiling(False)
                ph = {p: statistics.median(i[p] for i in phases) for p in ("ms_order", "ms_heads", "ms_scan")}
                take_ms = None
                if sources:
                    take_ms, _ = timed(torch, lambda: ex.take_cols_device(sources, rmap), args.reps, args.warmup)
                torch_ms, checked = None, "partition sizes"
                if sname == "cum_sum_i64":
                    try:
                        torch_ms, (want, perm) = timed(torch, lambda: torch_cum_sum(torch, k, t, x64), max(3, args.reps // 2), 1)
                        assert torch.equal(perm, rmap), "the torch composition orders the rows differently"  # (both sorts are stable)
                        assert torch.equal(want, outs[0][0]), "CUM_SUM(I64) differs from the torch composition"
                        checked = "torch composition"
                        del want, perm
                    except torch.cuda.OutOfMemoryError:
                        torch.cuda.empty_cache()
                elif sname == "row_number":
                    assert int(outs[0][0].view(torch.int64).max()) == info["max_partition_rows"]
                results.append({"log2_rows": lg, "partitions": pname, "set": sname, "n_partitions": info["n_partitions"],
                                "max_partition_rows": info["max_partition_rows"], "call_ms": round(call_ms, 3),
                                "phases_ms": {p: round(v, 3) for p, v in ph.items()},
                                "heads_scan_ms": round(ph["ms_heads"] + ph["ms_scan"], 3), "order_by_ms": round(order_ms, 3),
                                "take_ms": None if take_ms is None else round(take_ms, 3),
                                "torch_ms": None if torch_ms is None else round(torch_ms, 3), "checked": checked})
                del rmap, outs
            del k, keys
            torch.cuda.empty_cache()
    ex.close()
    print(json.dumps({"tool": "bench_window", "device": torch.cuda.get_device_name(0), "reps": args.reps, "warmup": args.warmup,
                      "results": results}))


if __name__ == "__main__":
    main()
