#!/usr/bin/env python3
"""Time grouping by string and mixed keys on the device (hmj_group_mixed_device) beside its floors and yardsticks.  One JSON
line, also written to --out.

  Shapes over 2^24 rows: one string column of 16-byte keys (s16), one of 64-byte keys whose first 48 bytes are shared
  (s64: a compare walks the whole prefix), and (16-byte string, 4-byte integer) tuples (s16_4).  The rows draw their key
  from 2^4, 2^12 or 2^20 distinct keys, or are all distinct.  Two calls per input: COUNT only (HMJ_MATERIALIZE, want =
  COUNT) and everything (want = COUNT | SUM | MIN | MAX | ROW_MAP over a random payload column).  Per input:

  count_ms / all_ms   median of --reps device-timed calls (HIP events around the call) after --warmup, profiling off
  phases_ms           median hmj_group_opts ms_key / ms_sort / ms_groups / ms_agg of the everything call (profiling on,
                      separate calls)
  key_floor_ms        ms_key of hmj_join_mixed_device with the same relation as the build side and one probe row: the
                      hashing floor (one pass over every key byte)
  sort_floor_ms       hmj_sort_u64_device on the pre-built {key64,row} rows, same process, timed the same way
  take_str_ms         hmj_take_str_device of the string key column through a random map of n rows (capacity given: one call)

  There is no gate.  The inputs are built on the device; the tool checks n_groups against the number of distinct ids and
  the key64 it rebuilds for the sort floor against mixed_key64 on a sample.

    python tools/bench_group_mixed.py [--reps 20] [--warmup 3] [--log2 24] [--out profiles/group_mixed_bench.json]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.bench_group_cols import mix64, timed  # noqa: E402

SHAPES = ("s16", "s64", "s16_4")
PREFIX = b"shared-prefix-of-forty-eight-bytes-0123456789abcd"[:48]


def string_column(torch, ids, width):
    """Fixed-length keys, injective in the id: 16 letters from the nibbles of mix64(id), behind PREFIX for 64-byte keys."""
    n = ids.shape[0]
    h = mix64(ids)
    tail = torch.stack([((h >> (4 * j)) & 15) + 97 for j in range(16)], 1).to(torch.uint8)
    if width == 64:
        head = torch.tensor(list(PREFIX), dtype=torch.uint8, device=ids.device).expand(n, 48)
        tail = torch.cat([head, tail], 1)
    return tail.contiguous().reshape(-1), torch.arange(n + 1, device=ids.device, dtype=torch.int64) * width


def columns_of(torch, ids, shape):
    if shape == "s16":
        return [string_column(torch, ids, 16)]
    if shape == "s64":
        return [string_column(torch, ids, 64)]
    return [string_column(torch, ids >> 3, 16), (ids & 7).to(torch.int32)]


def host_sample(cols, k):
    out = []
    for c in cols:
        if isinstance(c, tuple):
            off = c[1][:k + 1].cpu().numpy()
            raw = c[0][:int(off[-1])].cpu().numpy().tobytes()
            out.append([raw[off[i]:off[i + 1]] for i in range(k)])
        else:
            out.append(c[:k].cpu().numpy())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--log2", type=int, nargs="+", default=[24])
    ap.add_argument("--shapes", nargs="+", default=list(SHAPES))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    import hashmergejoin_amd as H

    assert torch.cuda.is_available(), "bench_group_mixed needs a GPU"
    ex = H.Executor(0)
    out = {"tool": "bench_group_mixed", "reps": args.reps, "warmup": args.warmup, "device": torch.cuda.get_device_name(0)}
    everything = H.HMJ_GROUP_COUNT | H.HMJ_GROUP_SUM | H.HMJ_GROUP_MIN | H.HMJ_GROUP_MAX | H.HMJ_GROUP_ROW_MAP
    gen = torch.Generator(device="cuda")
    for lg in args.log2:
        n = 1 << lg
        for shape in args.shapes:
            for dl in (4, 12, 20, None):
                gen.manual_seed(lg * 100 + (dl or 99))
                if dl is None:
                    ids = torch.randperm(n, device="cuda", generator=gen)
                else:
                    ids = torch.randint(0, 1 << dl, (n,), device="cuda", generator=gen)
                distinct = int(torch.unique(ids).shape[0])
                cols = columns_of(torch, ids, shape)
                del ids
                vals = torch.randint(-(1 << 63), (1 << 63) - 1, (n,), device="cuda", generator=gen)
                rmap = torch.randperm(n, device="cuda", generator=gen)
                ex.set_profiling(False)
                count_ms, (res, info) = timed(torch, lambda: ex.group_mixed_device(cols, None, None, H.HMJ_MATERIALIZE, H.HMJ_GROUP_COUNT),
                                              args.reps, args.warmup)
                all_ms, (res, info) = timed(torch, lambda: ex.group_mixed_device(cols, vals, None, H.HMJ_MATERIALIZE, everything),
                                            args.reps, args.warmup)
                n_groups, max_count = int(res.n_groups), int(res.max_count)
                assert n_groups == distinct, (n_groups, distinct)
                # every row's key64, for the sort floor: its group's key64 through the row map
                got = ex.group_rows_to_numpy(res)
                key = torch.from_numpy(got["key64"].view(np.int64)).cuda()[torch.from_numpy(got["group_of_row"].view(np.int64)).cuda()]
                del got
                assert np.array_equal(key[:1000].cpu().numpy().view(np.uint64), H.mixed_key64(host_sample(cols, 1000))), "key64 of the floor"
                rows = torch.stack([key, torch.arange(n, device="cuda")], 1).contiguous()
                del key
                ex.set_profiling(True)
                ph = {k: [] for k in ("ms_key", "ms_sort", "ms_groups", "ms_agg")}
                for _ in range(max(5, args.reps // 2)):
                    _, inf = ex.group_mixed_device(cols, vals, None, H.HMJ_MATERIALIZE, everything)
                    for k in ph:
                        ph[k].append(inf[k])
                one = [(c[0], c[1][:2].contiguous()) if isinstance(c, tuple) else c[:1].contiguous() for c in cols]
                kf = []
                for _ in range(args.warmup + max(5, args.reps // 2)):
                    _, jinf = ex.join_mixed_device(cols, None, one, None, H.HMJ_KIND_PROBE_SIDE, H.HMJ_JOIN_INNER, 0)
                    kf.append(jinf["ms_key"])
                kf = kf[args.warmup:]
                ex.set_profiling(False)
                ex.release_result()
                floor_ms, _ = timed(torch, lambda: ex.sort_device(rows), args.reps, args.warmup)
                chars, offs = cols[0]
                take_ms, _ = timed(torch, lambda: ex.take_str_device(chars, offs, rmap, want_validity=False, capacity=chars.numel()),
                                   args.reps, args.warmup)
                row = {"n_groups": n_groups, "max_count": max_count, "n_collisions": info["n_collisions"], "count_ms": round(count_ms, 4),
                       "all_ms": round(all_ms, 4), "phases_ms": {k: round(statistics.median(v), 4) for k, v in ph.items()},
                       "key_floor_ms": round(statistics.median(kf), 4), "sort_floor_ms": round(floor_ms, 4), "take_str_ms": round(take_ms, 4),
                       "count_vs_floors": round(count_ms / (statistics.median(kf) + floor_ms), 3)}
                out["%s_2^%d_distinct_%s" % (shape, lg, "all" if dl is None else "2^%d" % dl)] = row
                del cols, vals, rows, rmap, chars, offs, one
                torch.cuda.empty_cache()
    ex.close()
    line = json.dumps(out)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
