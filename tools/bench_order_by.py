#!/usr/bin/env python3
"""Time ORDER BY on the device (hmj_order_by_device) beside its floor and its yardsticks.  One JSON line.

  Shapes, at 2^24 and 2^26 rows: one U64 column; one I32 column; one F64 column; (I32 with 200 distinct values, I64); one
  22-byte string column, unique; one string column with a 16-byte shared prefix; (16-byte string, I32 DESC) with 10 % NULLs
  in the string column (the strings are unique, so the I32 decides among the NULL rows only).  Per shape:

  order_ms            median of --reps device-timed calls (HIP events around the call) after --warmup, profiling off
  phases_ms, n_rounds median hmj_order_opts ms_key / ms_sort / ms_refine / ms_map (profiling on, separate calls)
  sort_floor_ms       hmj_sort_u64_device on pre-built {key, row} rows of the same n, same process, timed the same way: the
                      key is the column's order-preserving u64 where the key has at most 8 bytes (the floor of any
                      single-column key of that width), random 64-bit keys otherwise
  torch_sort_ms       torch.sort(stable=True) on the same column (U64 as the int64 of the same bits; single fixed columns)
  group_ordered_ms    string shapes: the ordered COUNT call of hmj_group_mixed_device on the same column(s) -- hash order,
                      not value order: what a caller had before this entry

  There is no gate.  The inputs are drawn on the device; single fixed columns are checked against torch.sort.

    python tools/bench_order_by.py [--reps 10] [--warmup 2] [--log2 24 26]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
MIN64 = -(1 << 63)


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


def fixed_strings(torch, gen, n, length, prefix=0):
    """n strings of `length` bytes as (chars uint8 [n * length], offsets int64 [n + 1]): random lower-case letters, the
    first `prefix` bytes shared."""
    body = torch.randint(97, 123, (n, length), device="cuda", generator=gen, dtype=torch.uint8)
    if prefix:
        body[:, :prefix] = body[0, :prefix].clone()
    return body.reshape(-1).contiguous(), torch.arange(n + 1, device="cuda", dtype=torch.int64) * length


def device_bitmap(torch, valid):
    """pack_validity on the device, bit offset 0."""
    n = valid.shape[0]
    pad = (-n) % 8
    bits = torch.cat([valid, torch.zeros(pad, dtype=torch.bool, device=valid.device)]).reshape(-1, 8).to(torch.int32)
    weights = torch.tensor([1, 2, 4, 8, 16, 32, 64, 128], device=valid.device, dtype=torch.int32)
    return (bits * weights).sum(1).to(torch.uint8).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--log2", type=int, nargs="+", default=[24, 26])
    args = ap.parse_args()
    import torch

    import hashmergejoin_amd as H

    assert torch.cuda.is_available(), "bench_order_by needs a GPU"
    ex = H.Executor(0)
    out = {"tool": "bench_order_by", "reps": args.reps, "warmup": args.warmup, "device": torch.cuda.get_device_name(0)}
    gen = torch.Generator(device="cuda")
    for lg in args.log2:
        n = 1 << lg
        for shape in ("u64", "i32", "f64", "i32x200_i64", "str22_unique", "str_prefix16", "str16_i32desc_nulls"):
            try:
                gen.manual_seed(lg * 100 + len(shape))
                key = torch.randint(MIN64, (1 << 63) - 1, (n,), device="cuda", generator=gen)  # the floor's keys unless set below
                sortable, strings = None, None
                if shape == "u64":
                    col = key.clone()  # the floor sorts the very same keys
                    cols, sortable = [(col.view(torch.uint64), 0)], col ^ MIN64  # (int64 whose order is the uint64 order)
                elif shape == "i32":
                    col = torch.randint(-(1 << 31), (1 << 31) - 1, (n,), device="cuda", generator=gen, dtype=torch.int32)
                    cols, sortable = [(col, 0)], col
                    key = (col.to(torch.int64) + (1 << 31)) << 32
                elif shape == "f64":
                    col = torch.randn(n, device="cuda", generator=gen, dtype=torch.float64) * 1e6
                    cols, sortable = [(col, 0)], col
                    bits = col.view(torch.int64)
                    key = torch.where(bits < 0, ~bits, bits ^ MIN64)
                elif shape == "i32x200_i64":
                    a = torch.randint(0, 200, (n,), device="cuda", generator=gen, dtype=torch.int32)
                    cols = [(a, 0), (key.clone(), 0)]
                elif shape == "str22_unique":
                    strings = fixed_strings(torch, gen, n, 22)
                    cols = [(strings, 0)]
                elif shape == "str_prefix16":
                    strings = fixed_strings(torch, gen, n, 22, prefix=16)
                    cols = [(strings, 0)]
                else:
                    strings = fixed_strings(torch, gen, n, 16)
                    valid = torch.rand(n, device="cuda", generator=gen) >= 0.1
                    b = torch.randint(-(1 << 31), (1 << 31) - 1, (n,), device="cuda", generator=gen, dtype=torch.int32)
                    cols = [(strings, 0, device_bitmap(torch, valid), 0), (b, H.HMJ_ORDER_DESC)]
                    del valid
                rows = torch.stack([key, torch.arange(n, device="cuda")], 1).contiguous()
                del key
                ex.set_profiling(False)
                order_ms, (rmap, info) = timed(torch, lambda: ex.order_by_device(cols), args.reps, args.warmup)
                if sortable is not None:
                    assert torch.equal(sortable[rmap], torch.sort(sortable, stable=True).values), shape
                del rmap
                ex.set_profiling(True)
                ph = {k: [] for k in ("ms_key", "ms_sort", "ms_refine", "ms_map")}
                for _ in range(max(3, args.reps // 2)):
                    _, inf = ex.order_by_device(cols)
                    for k in ph:
                        ph[k].append(inf[k])
                ex.set_profiling(False)
                floor_ms, _ = timed(torch, lambda: ex.sort_device(rows), args.reps, args.warmup)
                del rows
                row = {"n_rounds": info["n_rounds"], "n_distinct": info["n_distinct"], "n_tied_rows": info["n_tied_rows"],
                       "order_ms": round(order_ms, 4), "phases_ms": {k: round(statistics.median(v), 4) for k, v in ph.items()},
                       "sort_floor_ms": round(floor_ms, 4), "order_vs_floor": round(order_ms / floor_ms, 3)}
                if sortable is not None:
                    t_ms, _ = timed(torch, lambda: torch.sort(sortable, stable=True), args.reps, args.warmup)
                    row["torch_sort_ms"] = round(t_ms, 4)
                if strings is not None:
                    gcols = [strings] + ([cols[1][0]] if len(cols) > 1 else [])
                    g_ms, _ = timed(torch, lambda: ex.group_mixed_device(gcols, flags=H.HMJ_ORDERED, want=H.HMJ_GROUP_COUNT), args.reps, args.warmup)
                    row["group_ordered_ms"] = round(g_ms, 4)
                    ex.release_result()
                out["%s_2^%d" % (shape, lg)] = row
                del cols, sortable, strings
                torch.cuda.empty_cache()
            except Exception as e:  # keep what was measured: the line is printed at the end
                out["%s_2^%d" % (shape, lg)] = {"error": str(e).splitlines()[0][:200]}
                ex.close()
                print(json.dumps(out))
                raise
    ex.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
