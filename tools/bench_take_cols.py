#!/usr/bin/env python3
"""Time hmj_take_cols_device (fixed-width columns through a row map) against torch's gather and a device copy.  One JSON line.

  Maps, per output size 2^24 and 2^26: the identity, a random permutation (n_src = n_out), and -- at 2^24 rows -- r_row of the
  HMJ_ORDERED result of a 2^22 x 2^24 foreign-key multi-column join ([4,4] keys; sorted by key, so every build row repeats
  about four times in a row), read straight from the result's device pointer.
  Per map: widths 4 and 8; one column per call, four columns per call (`fused4`) and the same four columns as four
  one-column calls (`four_calls`); without bitmaps, and with a source bitmap (10 % NULL) and an output bitmap per column.

  ms            median of --reps calls after --warmup, HIP events around the whole call: the launches, the read-back of the
                counts, and the output tensors taken from torch's caching allocator
  kernel_ms     median hmj_take_opts.ms_take (profiling on, separate calls): the launches alone
  GBps          algorithmic bytes / kernel_ms; the bytes per row are 8 (map) + per column 2 * width (value read and written)
                + 1/8 (output bitmap) + 1/8 (source bitmap), the bitmap terms only with bitmaps
  index_select_ms   torch.index_select of the same tensors through the same map into preallocated outputs, in the same process,
                timed the same way (one call per column; it knows nothing of validity, so it is the baseline of the runs
                without bitmaps)
  copy_ms       a device-to-device copy of the output's size (torch copy_): the floor of any kernel that writes the output

  No ratio is a gate: the gather is uncoalesced by nature (identity excepted), and the numbers are there to be read.

    python tools/bench_take_cols.py [--reps 20] [--warmup 3] [--log2 24 26]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--log2", type=int, nargs="+", default=[24, 26])
    args = ap.parse_args()
    import torch

    import hashmergejoin_amd as H
    from hashmergejoin_amd.join import _memcpy_d2d

    assert torch.cuda.is_available(), "bench_take_cols needs a GPU"
    ex = H.Executor(0)
    out = {"tool": "bench_take_cols", "reps": args.reps, "warmup": args.warmup, "null_frac": 0.1}
    dtypes = {4: torch.int32, 8: torch.int64}

    def kernel_ms(fn):
        ex.set_profiling(True)
        ms = [fn()[2]["ms_take"] for _ in range(max(5, args.reps // 2))]
        ex.set_profiling(False)
        return statistics.median(ms)

    def bench_map(tag, row_map, n_src):
        """row_map: an int64 device tensor without HMJ_TAKE_NO_ROW (index_select reads it too)."""
        n = row_map.shape[0]
        rng = np.random.default_rng(n_src % 1000003)
        bitmaps = [H.pack_validity(rng.random(n_src) >= 0.1, 0, "cuda") for _ in range(4)]
        for w in (4, 8):
            src = [torch.randint(-2 ** 31, 2 ** 31 - 1, (n_src,), dtype=dtypes[w], device="cuda") for _ in range(4)]
            dst = [torch.empty(n, dtype=dtypes[w], device="cuda") for _ in range(4)]
            other = torch.empty(n, dtype=dtypes[w], device="cuda")
            row = {}
            copy1, _ = timed(torch, lambda: dst[0].copy_(other), args.reps, args.warmup)
            sel1, _ = timed(torch, lambda: torch.index_select(src[0], 0, row_map, out=dst[0]), args.reps, args.warmup)
            sel4, _ = timed(torch, lambda: [torch.index_select(s, 0, row_map, out=d) for s, d in zip(src, dst)], args.reps, args.warmup)
            got, _, _ = ex.take_cols_device(src[:1], row_map, want_validity=False)
            assert torch.equal(got[0], dst[0])
            del got
            for bm in (False, True):
                valid = (lambda k: [(bitmaps[c], 0) for c in range(k)]) if bm else (lambda k: None)
                per_row = lambda k: 8 + k * (2 * w + (0.25 if bm else 0.0))
                calls = (("one", 1, lambda: ex.take_cols_device(src[:1], row_map, valid=valid(1), want_validity=bm)),
                         ("fused4", 4, lambda: ex.take_cols_device(src, row_map, valid=valid(4), want_validity=bm)))
                for name, k, fn in calls:
                    ms, _ = timed(torch, fn, args.reps, args.warmup)
                    km = kernel_ms(fn)
                    row["%s%s" % (name, "_bitmaps" if bm else "")] = {
                        "ms": round(ms, 4), "kernel_ms": round(km, 4), "bytes_per_row": per_row(k),
                        "GBps": round(per_row(k) * n / km / 1e6, 1)}
                four = lambda: [ex.take_cols_device([s], row_map, valid=None if not bm else [(b, 0)], want_validity=bm)
                                for s, b in zip(src, bitmaps)]
                ms, _ = timed(torch, four, args.reps, args.warmup)
                row["four_calls%s" % ("_bitmaps" if bm else "")] = {"ms": round(ms, 4)}
            row.update({"index_select_ms": round(sel1, 4), "index_select_x4_ms": round(sel4, 4), "copy_ms": round(copy1, 4),
                        "copy_x4_ms": round(4 * copy1, 4), "n_out": n, "n_src": n_src})
            out["%s_w%d" % (tag, w)] = row
            del src, dst, other
            torch.cuda.empty_cache()

    for lg in args.log2:
        n = 1 << lg
        bench_map("identity_2^%d" % lg, torch.arange(n, dtype=torch.int64, device="cuda"), n)
        bench_map("permutation_2^%d" % lg, torch.randperm(n, dtype=torch.int64, device="cuda"), n)
        if lg == 24:  # the ordered result of a 2^22 x 2^24 foreign-key join on two int32 columns
            nb = 1 << 22
            ids = torch.randperm(nb, dtype=torch.int64, device="cuda")
            fk = ids[torch.randint(0, nb, (n,), device="cuda")]
            key = lambda t: [(t >> 12).to(torch.int32) * 40503, t.to(torch.int32)]
            res, _ = ex.join_cols_device(key(ids), None, key(fk), None, H.HMJ_ORDERED)
            assert int(res.n_matches) == n
            r_row = torch.empty(n, dtype=torch.int64, device="cuda")
            _memcpy_d2d(torch, r_row, res.r_row, 8 * n)
            src = torch.arange(nb, dtype=torch.int64, device="cuda")
            got, _, info = ex.take_cols_device([src], (res.r_row, n), want_validity=False)  # straight from the result
            assert torch.equal(got[0], r_row) and info["n_no_row"] == 0
            del got, src, ids, fk
            bench_map("fk_join_r_row_2^24", r_row, nb)
            ex.release_result()
        torch.cuda.empty_cache()
    ex.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
