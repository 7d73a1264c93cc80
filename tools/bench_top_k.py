#!/usr/bin/env python3
"""Time ORDER BY ... LIMIT k on the device (hmj_top_k_device) beside its yardsticks.  One JSON line.

  Shapes, at 2^24 and 2^26 rows: the seven of tools/bench_order_by.py.  Per shape:

  order_by_ms         median of --reps device-timed hmj_order_by_device calls on the same columns: the way to a top-k before
                      this entry, and the yardstick
  and per K in 1, 10, 1000, 2^16, 2^20, n/8, n/2 (offset 0), under "K=<k>":
  select_ms, full_ms, auto_ms   median of --reps device-timed calls (HIP events around the call) after --warmup, profiling
                      off, the plan pinned or left to the library; auto_plan: the plan AUTO took
  phases_ms, n_levels, n_candidates, n_tie_rows, n_rounds   the SELECT plan's ms_select / ms_emit / ms_order (profiling on,
                      separate calls) and its counters
  torch_topk_ms       torch.topk(largest=False) on the same column (single numeric columns, K <= 2^20; U64 as the int64 of the
                      same bits)
  model_bytes, copy_ms  the byte model of the SELECT plan -- every level and the mark read the key columns once, the
                      candidates cost an ORDER BY's 150 bytes each -- and a device copy that moves as many bytes

  There is no gate.  The inputs are drawn on the device; the SELECT map is checked against the FULL map in every cell.

    python tools/bench_top_k.py [--reps 10] [--warmup 2] [--log2 24 26]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_order_by import MIN64, device_bitmap, fixed_strings, timed  # noqa: E402

ORDER_BYTES_PER_ROW = 150  # DESIGN.md "Ordering rows (ORDER BY)": what a full ORDER BY moves per row
COPY_CAP = 1 << 30


def draw_shape(torch, H, gen, shape, n):
    """-> (cols as Executor.order_by_device takes them, the int64 column torch.topk orders alike or None, key bytes per row)."""
    key = torch.randint(MIN64, (1 << 63) - 1, (n,), device="cuda", generator=gen)
    if shape == "u64":
        return [(key.view(torch.uint64), 0)], key ^ MIN64, 8
    if shape == "i32":
        col = torch.randint(-(1 << 31), (1 << 31) - 1, (n,), device="cuda", generator=gen, dtype=torch.int32)
        return [(col, 0)], col, 4
    if shape == "f64":
        col = torch.randn(n, device="cuda", generator=gen, dtype=torch.float64) * 1e6
        return [(col, 0)], col, 8
    if shape == "i32x200_i64":
        a = torch.randint(0, 200, (n,), device="cuda", generator=gen, dtype=torch.int32)
        return [(a, 0), (key, 0)], None, 12
    del key
    if shape == "str22_unique":
        return [(fixed_strings(torch, gen, n, 22), 0)], None, 8 + 22
    if shape == "str_prefix16":
        return [(fixed_strings(torch, gen, n, 22, prefix=16), 0)], None, 8 + 22
    strings = fixed_strings(torch, gen, n, 16)
    valid = torch.rand(n, device="cuda", generator=gen) >= 0.1
    b = torch.randint(-(1 << 31), (1 << 31) - 1, (n,), device="cuda", generator=gen, dtype=torch.int32)
    return [(strings, 0, device_bitmap(torch, valid), 0), (b, H.HMJ_ORDER_DESC)], None, 8 + 16 + 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--log2", type=int, nargs="+", default=[24, 26])
    ap.add_argument("--shapes", nargs="+", default=["u64", "i32", "f64", "i32x200_i64", "str22_unique", "str_prefix16", "str16_i32desc_nulls"])
    args = ap.parse_args()
    import torch

    import hashmergejoin_amd as H

    assert torch.cuda.is_available(), "bench_top_k needs a GPU"
    ex = H.Executor(0)
    out = {"tool": "bench_top_k", "reps": args.reps, "warmup": args.warmup, "device": torch.cuda.get_device_name(0)}
    gen = torch.Generator(device="cuda")
    src = torch.empty(COPY_CAP, dtype=torch.uint8, device="cuda")
    dst = torch.empty(COPY_CAP, dtype=torch.uint8, device="cuda")
    for lg in args.log2:
        n = 1 << lg
        for shape in args.shapes:
            name = "%s_2^%d" % (shape, lg)
            try:
                gen.manual_seed(lg * 100 + len(shape))
                cols, sortable, key_bytes = draw_shape(torch, H, gen, shape, n)
                ex.set_profiling(False)
                order_ms, _ = timed(torch, lambda: ex.order_by_device(cols), args.reps, args.warmup)
                row = {"order_by_ms": round(order_ms, 4)}
                for K in (1, 10, 1000, 1 << 16, 1 << 20, n // 8, n // 2):
                    cell = {}
                    maps = {}
                    for plan in ("select", "full", "auto"):
                        ms, (rmap, info) = timed(torch, lambda: ex.top_k_device(cols, K, plan=plan), args.reps, args.warmup)
                        cell[plan + "_ms"] = round(ms, 4)
                        maps[plan] = rmap
                        if plan == "auto":
                            cell["auto_plan"] = "select" if info["plan_taken"] == H.HMJ_TOPK_SELECT else "full"
                    assert torch.equal(maps["select"], maps["full"]) and torch.equal(maps["auto"], maps["full"]), (name, K)
                    del maps, rmap
                    ex.set_profiling(True)
                    ph = {k: [] for k in ("ms_select", "ms_emit", "ms_order")}
                    for _ in range(3):
                        _, info = ex.top_k_device(cols, K, plan="select")
                        for k in ph:
                            ph[k].append(info[k])
                    ex.set_profiling(False)
                    cell["phases_ms"] = {k: round(statistics.median(v), 4) for k, v in ph.items()}
                    for k in ("n_levels", "n_candidates", "n_tie_rows", "n_rounds"):
                        cell[k] = info[k]
                    cell["select_vs_order_by"] = round(cell["select_ms"] / order_ms, 3)
                    if sortable is not None and K <= 1 << 20:  # (beyond, torch.topk is a full sort: bench_order_by.py has it)
                        t_ms, _ = timed(torch, lambda: torch.topk(sortable, K, largest=False), args.reps, args.warmup)
                        cell["torch_topk_ms"] = round(t_ms, 4)
                    model = (info["n_levels"] + 1) * key_bytes * n + ORDER_BYTES_PER_ROW * info["n_candidates"]
                    half = min(model // 2, COPY_CAP)
                    c_ms, _ = timed(torch, lambda: dst[:half].copy_(src[:half]), args.reps, args.warmup)
                    cell["model_bytes"] = model
                    cell["copy_ms"] = round(c_ms * (model / 2) / max(half, 1), 4)  # (scaled where the model exceeds the buffers)
                    row["K=%d" % K] = cell
                out[name] = row
                print("%s: order_by %.3f ms" % (name, order_ms), file=sys.stderr, flush=True)
                del cols, sortable
                torch.cuda.empty_cache()
            except Exception as e:  # keep what was measured: the line is printed at the end
                out[name] = {"error": str(e).splitlines()[0][:200]}
                ex.close()
                print(json.dumps(out))
                raise
    ex.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
