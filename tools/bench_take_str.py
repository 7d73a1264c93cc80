#!/usr/bin/env python3
"""Time hmj_take_str_device (one Arrow large_string column through a row map) against a device copy of the output bytes and
against the same take composed from torch ops.  One JSON line.

  Shapes: 10^6 and 2^24 rows of about 22 bytes (18..26: the keys of BASELINE configs[0]), 2^24 rows of 8 bytes, 2^20 rows of
  1 KiB.  Maps, n_out = n_src: the identity, a random permutation, and -- for the 22-byte shapes -- r_row of the HMJ_ORDERED
  result of the string join of the column with a permutation of itself, read straight from the result's device pointer.
  Each without bitmaps, and with a source bitmap (10 % NULL) and an output bitmap.

  ms            median of --reps calls after --warmup, HIP events around Executor.take_str_device with the capacity known (one
                call of the entry: both phases, the read-back between them, the output tensors from torch's allocator)
  two_call_ms   the same with capacity=None: the sizing call, an allocation of exactly total_bytes, the full call
  ms_offsets, ms_chars   medians of hmj_take_str_opts' phase times (profiling on, separate calls)
  GBps          algorithmic bytes / (ms_offsets + ms_chars); per output row 8 (map) + 16 (two source offsets gathered) + 24
                (the output offsets written, read and written again by the placing kernel) + 2 * its bytes, + 1/4 with bitmaps
  copy_ms       a device-to-device copy of total_bytes (torch copy_): the floor of anything that writes the output's chars
  torch_ms      the same take from torch ops into fresh tensors -- gathered lengths, cumsum, repeat_interleave, index_select
                on the chars --, checked equal to the entry's output; it knows nothing of validity, so it is the yardstick
                of the runs without bitmaps (null where the shape exceeds --torch-max-bytes)

  No ratio is a gate: the numbers are there to be read.

    python tools/bench_take_str.py [--reps 10] [--warmup 2] [--shapes keys22_1e6 keys22_2^24 w8_2^24 kib_2^20]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"keys22_1e6": (10 ** 6, 18, 26), "keys22_2^24": (1 << 24, 18, 26), "w8_2^24": (1 << 24, 8, 8), "kib_2^20": (1 << 20, 1024, 1024)}


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
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shapes", nargs="+", default=list(SHAPES), choices=list(SHAPES))
    ap.add_argument("--torch-max-bytes", type=int, default=1 << 31)
    args = ap.parse_args()
    import torch

    import hashmergejoin_amd as H
    from hashmergejoin_amd.join import _memcpy_d2d

    assert torch.cuda.is_available(), "bench_take_str needs a GPU"
    ex = H.Executor(0)
    out = {"tool": "bench_take_str", "reps": args.reps, "warmup": args.warmup, "null_frac": 0.1}

    def torch_take(chars, offsets, row_map):
        starts = offsets[:-1].index_select(0, row_map)
        lens = offsets[1:].index_select(0, row_map) - starts
        out_off = torch.zeros(row_map.shape[0] + 1, dtype=torch.int64, device="cuda")
        torch.cumsum(lens, 0, out=out_off[1:])
        total = int(out_off[-1])
        row_of = torch.repeat_interleave(torch.arange(row_map.shape[0], device="cuda"), lens, output_size=total)
        idx = torch.arange(total, device="cuda") - out_off[:-1].index_select(0, row_of) + starts.index_select(0, row_of)
        return chars.index_select(0, idx), out_off

    def bench_map(tag, chars, offsets, row_map, bitmap):
        """row_map: an int64 device tensor without HMJ_TAKE_NO_ROW (the torch composition reads it too)."""
        n = row_map.shape[0]
        row = {"n_out": n, "n_src": offsets.shape[0] - 1}
        got_c, got_o, _, info = ex.take_str_device(chars, offsets, row_map, want_validity=False)
        total = info["total_bytes"]
        row["total_bytes"] = total
        a, b = torch.empty(total, dtype=torch.uint8, device="cuda"), torch.empty(total, dtype=torch.uint8, device="cuda")
        row["copy_ms"] = round(timed(torch, lambda: a.copy_(b), args.reps, args.warmup)[0], 4)
        del a, b
        row["torch_ms"] = None
        if total <= args.torch_max_bytes:
            ms, (t_c, t_o) = timed(torch, lambda: torch_take(chars, offsets, row_map), args.reps, args.warmup)
            assert torch.equal(t_c, got_c) and torch.equal(t_o, got_o)
            row["torch_ms"] = round(ms, 4)
            del t_c, t_o
        del got_c, got_o
        torch.cuda.empty_cache()
        for bm in (False, True):
            valid = (bitmap, 0) if bm else None
            one = lambda: ex.take_str_device(chars, offsets, row_map, valid=valid, want_validity=bm, capacity=total)
            two = lambda: ex.take_str_device(chars, offsets, row_map, valid=valid, want_validity=bm)
            ms1, got = timed(torch, one, args.reps, args.warmup)
            ms2, _ = timed(torch, two, args.reps, args.warmup)
            ex.set_profiling(True)
            infos = [one()[3] for _ in range(max(5, args.reps // 2))]
            ex.set_profiling(False)
            mo, mc = statistics.median(i["ms_offsets"] for i in infos), statistics.median(i["ms_chars"] for i in infos)
            algo = n * (48 + (0.25 if bm else 0.0)) + 2 * got[3]["total_bytes"]
            row["bitmaps" if bm else "plain"] = {"ms": round(ms1, 4), "two_call_ms": round(ms2, 4), "ms_offsets": round(mo, 4),
                                                 "ms_chars": round(mc, 4), "total_bytes": got[3]["total_bytes"],
                                                 "null_count": got[3]["null_count"], "GBps": round(algo / (mo + mc) / 1e6, 1)}
            del got
        out[tag] = row
        torch.cuda.empty_cache()

    for name in args.shapes:
        n, lo, hi = SHAPES[name]
        gen = torch.Generator(device="cuda").manual_seed(n + lo)
        lens = torch.randint(lo, hi + 1, (n,), dtype=torch.int64, device="cuda", generator=gen)
        offsets = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
        torch.cumsum(lens, 0, out=offsets[1:])
        chars = torch.randint(0, 256, (int(offsets[-1]),), dtype=torch.uint8, device="cuda", generator=gen)
        bitmap = H.pack_validity(np.random.default_rng(n).random(n) >= 0.1, 0, "cuda")
        bench_map(name + "_identity", chars, offsets, torch.arange(n, dtype=torch.int64, device="cuda"), bitmap)
        perm = torch.randperm(n, dtype=torch.int64, device="cuda", generator=gen)
        bench_map(name + "_permutation", chars, offsets, perm, bitmap)
        if name.startswith("keys22"):  # the ordered result of the column joined with a permutation of itself
            p_chars, p_off = torch_take(chars, offsets, perm)
            vals = torch.arange(n, dtype=torch.int64, device="cuda")
            res, _ = ex.join_str_device((chars, offsets, vals), (p_chars, p_off, vals), H.HMJ_ORDERED)
            m = int(res.n_matches)
            assert m >= n
            r_row = torch.empty(m, dtype=torch.int64, device="cuda")
            _memcpy_d2d(torch, r_row, res.r_row, 8 * m)
            got = ex.take_str_device(chars, offsets, (res.r_row, m), want_validity=False)  # straight from the result
            want = torch_take(chars, offsets, r_row)
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and got[3]["n_no_row"] == 0
            del got, want, p_chars, p_off
            ex.release_result()
            bench_map(name + "_join_r_row", chars, offsets, r_row, bitmap)
        del chars, offsets, lens, perm
        torch.cuda.empty_cache()
    ex.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
