#!/usr/bin/env python3
"""Time the multi-column key join on the device (hmj_join_cols_device) against its floor.  One JSON line.

  Shapes: [4,4] (two int32 columns: the packed form) and [8,4,2] (the hashed form), 2^24 x 2^24 and 2^26 x 2^26 rows, unique
  tuples on the build side, the probe side a permutation of them; count mode and HMJ_ORDERED.  Per shape, size and mode:

  ms           median of --reps device-timed joins (HIP events around the call) after --warmup, profiling off
  floor_ms     hmj_join_u64_device with the same flags, in the same process and timed the same way, on pre-built {key64,row}
               rows -- the rows the key kernel writes (cols_key64 on the host).  What the column handling adds is ms - floor_ms.
  phases_ms    median hmj_cols_join_opts ms_key / ms_join / ms_verify / ms_order (profiling on, separate joins)
  key_kernel   both relations' key kernels: ms_key, their algorithmic bytes -- T + 16 per row (T = the widths' sum read, one
               {key64,row} row written) -- and the share of the 8 TB/s HBM peak that is.  ms_key spans two launches and, with
               HMJ_SUM_PROBE off, nothing else.

  --kinds: the join kinds (hmj_join_kind_cols_device) instead.  Same shapes and sizes, but every second probe tuple is one the
  build side does not hold; probe SEMI, probe ANTI and FULL_OUTER in count mode, each beside the inner count join
  (hmj_join_cols_device) of the same relations in the same process, timed the same way: ms, inner_ms, ms / inner_ms.

  --nulls FRAC: NULL keys (validity bitmaps) instead.  Same shapes and sizes, the --kinds relations.  In one process and on
  the same rows the inner count join -- with --kinds also probe SEMI, probe ANTI and FULL_OUTER in count mode -- is timed
  three ways: plain_ms (no bitmap: the call as it was), all_valid_ms (a bitmap of ones on column 1 of both sides: what the
  feature itself costs -- a pass over the bitmaps, a scan, a read-back and the compacted {key64,row} rows) and nulls_ms (FRAC
  of the rows of each side NULL in column 1).

  --null-equal: NULL-equals-NULL matching (HMJ_NULL_EQUAL) instead.  Same shapes and sizes, the --kinds relations with 10 %
  of the slots of one column NULL on each side -- column 0 of [4,4] and column 1 of [8,4,2]: the other columns keep the
  tuples distinct, so NULL slots add matches (the same id NULL on both sides) without piling rows up on one tuple.  In one process and on the same rows the inner count join -- with --kinds also
  probe SEMI, probe ANTI and FULL_OUTER in count mode -- runs once under SQL semantics (sql_ms: the call without the flag,
  the yardstick) and once under the flag (null_equal_ms); ms_key and ms_verify of both from separate calls with profiling
  on.  Under SQL semantics [4,4] keeps its packed form; under the flag every call with a bitmap is hashed.  No gate.

    python tools/bench_join_cols.py [--reps 20] [--warmup 3] [--log2 24 26] [--kinds] [--nulls FRAC] [--null-equal]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_TBPS = 8.0
SHAPES = (("4_4", [4, 4]), ("8_4_2", [8, 4, 2]))


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


def columns_of(ids, widths):
    if widths == [4, 4]:  # (tenant, id): the id alone is distinct
        return [(ids >> np.uint64(12)).astype(np.uint32) * np.uint32(2654435761), ids.astype(np.uint32)]
    # (id scattered over 64 bits, day, flag)
    return [ids * np.uint64(0x9E3779B97F4A7C15), (ids % np.uint64(36500)).astype(np.uint32), (ids & np.uint64(0xFFFF)).astype(np.uint16)]


def make_columns(n, widths, seed, miss_half=False):
    """n distinct tuples over `widths` (numpy, unsigned) and a permutation of them for the probe side.  miss_half: every
    second probe tuple is built from an id the build side does not hold (id + n)."""
    rng = np.random.default_rng(seed)
    ids = rng.permutation(n).astype(np.uint64)
    probe_ids = ids[rng.permutation(n)]
    if miss_half:
        probe_ids[::2] += np.uint64(n)
    return columns_of(ids, widths), columns_of(probe_ids, widths)


def bench_kinds(torch, H, ex, args, dev, out):
    kinds = (("semi", H.HMJ_KIND_PROBE_SIDE, H.HMJ_JOIN_SEMI), ("anti", H.HMJ_KIND_PROBE_SIDE, H.HMJ_JOIN_ANTI),
             ("full_outer", H.HMJ_KIND_BUILD_SIDE, H.HMJ_FULL_OUTER))
    for lg in args.log2:
        n = 1 << lg
        for name, widths in SHAPES:
            bc, pc = make_columns(n, widths, lg, miss_half=True)
            B, P = [dev(c) for c in bc], [dev(c) for c in pc]
            del bc, pc
            ex.set_profiling(False)
            inner_ms, (res, info) = timed(torch, lambda: ex.join_cols_device(B, None, P, None, 0), args.reps, args.warmup)
            assert int(res.n_matches) == n // 2
            row = {"form": "packed" if info["form"] == H.HMJ_COLS_PACKED else "hashed", "inner_ms": round(inner_ms, 4)}
            for kname, side, kind in kinds:
                ms, (res, inf) = timed(torch, lambda: ex.join_kind_cols_device(B, None, P, None, side, kind, 0), args.reps, args.warmup)
                assert int(res.n_matches) == (n // 2 if kind != H.HMJ_FULL_OUTER else n + n // 2) and inf["n_collisions"] == 0
                assert (inf["n_probe_matched"], inf["n_probe_unmatched"]) == (n // 2, n // 2)
                row[kname] = {"ms": round(ms, 4), "vs_inner": round(ms / inner_ms, 3), "n_key_pairs": inf["n_key_pairs"],
                              "path": ex.last_plan()["path"]}
            out["kinds_%s_2^%d_count" % (name, lg)] = row
            del B, P
            ex.release_result()
            torch.cuda.empty_cache()


def bench_nulls(torch, H, ex, args, dev, out):
    calls = [("inner", None, None)]
    if args.kinds:
        calls += [("semi", H.HMJ_KIND_PROBE_SIDE, H.HMJ_JOIN_SEMI), ("anti", H.HMJ_KIND_PROBE_SIDE, H.HMJ_JOIN_ANTI),
                  ("full_outer", H.HMJ_KIND_BUILD_SIDE, H.HMJ_FULL_OUTER)]
    out["nulls_frac"] = args.nulls
    for lg in args.log2:
        n = 1 << lg
        for name, widths in SHAPES:
            bc, pc = make_columns(n, widths, lg, miss_half=True)
            B, P = [dev(c) for c in bc], [dev(c) for c in pc]
            del bc, pc
            rng = np.random.default_rng(lg + 1)
            k = len(widths)
            on_col1 = lambda t: [None, t] + [None] * (k - 2)
            ones = H.pack_validity(np.ones(n, bool), 0, "cuda")
            mb, mp = rng.random(n) >= args.nulls, rng.random(n) >= args.nulls
            variants = (("plain_ms", None, None), ("all_valid_ms", on_col1(ones), on_col1(ones)),
                        ("nulls_ms", on_col1(H.pack_validity(mb, 0, "cuda")), on_col1(H.pack_validity(mp, 0, "cuda"))))
            ex.set_profiling(False)
            for cname, side, kind in calls:
                row = {}
                for vname, vb, vp in variants:
                    if kind is None:
                        fn = lambda: ex.join_cols_device(B, None, P, None, 0, build_valid=vb, probe_valid=vp)
                    else:
                        fn = lambda: ex.join_kind_cols_device(B, None, P, None, side, kind, 0, build_valid=vb, probe_valid=vp)
                    ms, (res, inf) = timed(torch, fn, args.reps, args.warmup)
                    row[vname] = round(ms, 4)
                    if vname != "nulls_ms":
                        assert (inf["n_build_null"], inf["n_probe_null"]) == (0, 0)
                        row["n_matches"] = int(res.n_matches)
                    else:
                        assert (inf["n_build_null"], inf["n_probe_null"]) == (int((~mb).sum()), int((~mp).sum()))
                        row["n_matches_nulls"] = int(res.n_matches)
                    row["form"] = "packed" if inf["form"] == H.HMJ_COLS_PACKED else "hashed"
                row["all_valid_vs_plain"] = round(row["all_valid_ms"] / row["plain_ms"], 3)
                row["nulls_vs_plain"] = round(row["nulls_ms"] / row["plain_ms"], 3)
                out["nulls_%s_%s_2^%d_count" % (cname, name, lg)] = row
            del B, P, ones, variants
            ex.release_result()
            torch.cuda.empty_cache()


def bench_null_equal(torch, H, ex, args, dev, out, frac=0.1):
    calls = [("inner", H.HMJ_KIND_PROBE_SIDE, H.HMJ_JOIN_INNER)]
    if args.kinds:
        calls += [("semi", H.HMJ_KIND_PROBE_SIDE, H.HMJ_JOIN_SEMI), ("anti", H.HMJ_KIND_PROBE_SIDE, H.HMJ_JOIN_ANTI),
                  ("full_outer", H.HMJ_KIND_BUILD_SIDE, H.HMJ_FULL_OUTER)]
    out["null_slots_frac"] = frac
    for lg in args.log2:
        n = 1 << lg
        for name, widths in SHAPES:
            bc, pc = make_columns(n, widths, lg, miss_half=True)
            B, P = [dev(c) for c in bc], [dev(c) for c in pc]
            del bc, pc
            rng = np.random.default_rng(lg + 2)
            mb, mp = rng.random(n) >= frac, rng.random(n) >= frac
            col = 0 if len(widths) == 2 else 1
            on_col = lambda m: [H.pack_validity(m, 0, "cuda") if c == col else None for c in range(len(widths))]
            vb, vp = on_col(mb), on_col(mp)
            for cname, side, kind in calls:
                row = {}
                for vname, flag in (("sql", 0), ("null_equal", H.HMJ_NULL_EQUAL)):
                    fn = lambda: ex.join_kind_cols_device(B, None, P, None, side, kind, flag, build_valid=vb, probe_valid=vp)
                    ex.set_profiling(False)
                    ms, (res, inf) = timed(torch, fn, args.reps, args.warmup)
                    assert (inf["n_build_null"], inf["n_probe_null"]) == (int((~mb).sum()), int((~mp).sum()))
                    ex.set_profiling(True)
                    ph = [fn()[1] for _ in range(max(5, args.reps // 2))]
                    ex.set_profiling(False)
                    row[vname + "_ms"] = round(ms, 4)
                    row[vname] = {"form": "packed" if inf["form"] == H.HMJ_COLS_PACKED else "hashed", "n_matches": int(res.n_matches),
                                  "ms_key": round(statistics.median(p["ms_key"] for p in ph), 4),
                                  "ms_verify": round(statistics.median(p["ms_verify"] for p in ph), 4)}
                row["null_equal_vs_sql"] = round(row["null_equal_ms"] / row["sql_ms"], 3)
                out["null_equal_%s_%s_2^%d_count" % (cname, name, lg)] = row
            del B, P, vb, vp
            ex.release_result()
            torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--log2", type=int, nargs="+", default=[24, 26])
    ap.add_argument("--kinds", action="store_true", help="time probe SEMI / ANTI / FULL_OUTER beside the inner count join")
    ap.add_argument("--nulls", type=float, default=None, metavar="FRAC",
                    help="time the plain call, the call with all-valid bitmaps and the call with FRAC of the rows NULL-keyed")
    ap.add_argument("--null-equal", action="store_true",
                    help="time each call under SQL semantics and under HMJ_NULL_EQUAL on the same rows with 10 %% NULL slots")
    args = ap.parse_args()
    import torch

    import hashmergejoin_amd as H

    assert torch.cuda.is_available(), "bench_join_cols needs a GPU"
    ex = H.Executor(0)
    out = {"tool": "bench_join_cols", "reps": args.reps, "warmup": args.warmup, "hbm_peak_TBps": HBM_TBPS}

    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(a).view("i%d" % a.dtype.itemsize)).cuda()

    if args.null_equal:
        bench_null_equal(torch, H, ex, args, dev, out)
        ex.close()
        print(json.dumps(out))
        return
    if args.nulls is not None:
        bench_nulls(torch, H, ex, args, dev, out)
        ex.close()
        print(json.dumps(out))
        return
    if args.kinds:
        bench_kinds(torch, H, ex, args, dev, out)
        ex.close()
        print(json.dumps(out))
        return

    for lg in args.log2:
        n = 1 << lg
        for name, widths in SHAPES:
            bc, pc = make_columns(n, widths, lg)
            rows = np.arange(n, dtype=np.uint64)
            Bu = dev(np.stack([H.cols_key64(bc, widths), rows], 1))
            Pu = dev(np.stack([H.cols_key64(pc, widths), rows], 1))
            B, P = [dev(c) for c in bc], [dev(c) for c in pc]
            del bc, pc
            for mode, flags in (("count", 0), ("ordered", H.HMJ_ORDERED)):
                ex.set_profiling(False)
                ms, (res, info) = timed(torch, lambda: ex.join_cols_device(B, None, P, None, flags), args.reps, args.warmup)
                path = ex.last_plan()["path"]
                floor, u = timed(torch, lambda: ex.join_device(Bu, Pu, flags), args.reps, args.warmup)
                floor_path = ex.last_plan()["path"]
                assert int(res.n_matches) == n == int(u.n_matches) and (int(res.sum_r), int(res.sum_s)) == (int(u.sum_r), int(u.sum_s))
                ex.set_profiling(True)
                ph = {k: [] for k in ("ms_key", "ms_join", "ms_verify", "ms_order")}
                for _ in range(max(5, args.reps // 2)):
                    _, inf = ex.join_cols_device(B, None, P, None, flags)
                    for k in ph:
                        ph[k].append(inf[k])
                ex.set_profiling(False)
                med = {k: statistics.median(v) for k, v in ph.items()}
                byts = 2 * n * (sum(widths) + 16)
                out["%s_2^%d_%s" % (name, lg, mode)] = {
                    "form": "packed" if info["form"] == H.HMJ_COLS_PACKED else "hashed", "ms": round(ms, 4), "floor_ms": round(floor, 4),
                    "added_ms": round(ms - floor, 4), "phases_ms": {k: round(v, 4) for k, v in med.items()},
                    "key_kernel": {"ms": round(med["ms_key"], 4), "bytes": byts, "TBps": round(byts / med["ms_key"] / 1e9, 3),
                                   "share_of_hbm_peak": round(byts / med["ms_key"] / 1e9 / HBM_TBPS, 3)},
                    "n_matches": int(res.n_matches), "n_collisions": info["n_collisions"], "path": path, "floor_path": floor_path}
            del B, P, Bu, Pu
            ex.release_result()
            torch.cuda.empty_cache()
    ex.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
