#!/usr/bin/env python3
"""Time the join kinds (hmj_join_kind_u64_device, and the build-side kinds of hmj_join_build_kind_u64_device) beside the
inner join of the same relations, in the same process.

One JSON line per (shape, kind, mode): median ms of >= --reps joins after --warmup (HIP events, hmj_last_timing.ms_total),
the median phase split, the path bits, and the achieved GB/s of the probe phase against its algorithmic bytes
(16 * (n_build + n_probe) read; materialising: + 16 B per result row for semi / anti, 24 B for inner / outer, written; the
build-side kinds add the sweep's 16 * n_build + n_build / 8 per pass, and their write pass reads both sides again only where
the walk writes rows -- build outer, full outer).
Relations come from the device generators (hmj_gen_build / hmj_gen_probe), so every probe row but every miss_mod-th has
exactly one build row.

    python tools/bench_join_kinds.py [--reps 20] [--warmup 3] [--shapes 28x28m0,26x26m4,...] [--kinds full_outer,...]

--exchange times the distributed form instead (hmj_exchange_join_kind_u64_device beside hmj_exchange_join_u64_device): one
rank running the whole exchange path over RCCL self send/recv (dist.init_comm_single(ex, self_exchange=True), the route
HMJ_FORCE_DIST=1 takes), count mode, default shapes 26x26m4,28x28m4.  One JSON line per (shape, kind): the median
wall-clock ms of a step (the call is synchronous: it returns after the final reduction), the median summed kernel ms of
its round joins (hmj_exchange_info.ms_kernels, profiling on), rounds and round joins.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = "28x28m0,28x28m4,26x26m0,26x26m4,16x26m0"
EXCHANGE_SHAPES = "26x26m4,28x28m4"
PHASES = ("ms_partition_build", "ms_partition_probe", "ms_probe_count", "ms_out_scan", "ms_probe_write", "ms_order")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shapes", default=SHAPES)
    ap.add_argument("--kinds", default="", help="comma-separated kind names to time beside the inner join (default: all)")
    ap.add_argument("--exchange", action="store_true", help="time the one-rank exchange path (RCCL self send/recv) instead")
    a = ap.parse_args()
    if a.exchange:
        return main_exchange(a)
    import torch

    import hashmergejoin_amd as H

    ex = H.Executor(0)
    ex.set_profiling(True)
    # (name, kind, build-side kind): the build-side kinds go through hmj_join_build_kind_u64_device
    kinds = (("inner", H.HMJ_JOIN_INNER, False), ("semi", H.HMJ_JOIN_SEMI, False), ("anti", H.HMJ_JOIN_ANTI, False),
             ("probe_outer", H.HMJ_JOIN_PROBE_OUTER, False), ("build_semi", H.HMJ_BUILD_SEMI, True),
             ("build_anti", H.HMJ_BUILD_ANTI, True), ("build_outer", H.HMJ_BUILD_OUTER, True),
             ("full_outer", H.HMJ_FULL_OUTER, True))
    if a.kinds:
        kinds = tuple(k for k in kinds if k[0] in a.kinds.split(",") or k[0] == "inner")
    modes = (("count", 0), ("materialize", H.HMJ_MATERIALIZE))
    for shape in a.shapes.split(","):
        lb, rest = shape.split("x")
        lp, miss = rest.split("m")
        nb, npb, miss = 1 << int(lb), 1 << int(lp), int(miss)
        bd, pd = ex.gen_build(nb), ex.gen_probe(npb, nb, miss_mod=miss)
        torch.cuda.synchronize()
        inner_ms = {}
        for mname, mflag in modes:
            for kname, kind, bkind in kinds:
                ts = []
                for i in range(a.warmup + a.reps):
                    if bkind:
                        r, cnt = ex.join_build_kind_device(bd, pd, kind, mflag)
                    else:
                        r, cnt = ex.join_kind_device(bd, pd, kind, mflag)
                    if i >= a.warmup:
                        ts.append(ex.last_timing())
                n_rows = int(r.n_matches)
                ms = statistics.median(t["ms_total"] for t in ts)
                ph = {k: round(statistics.median(t[k] for t in ts), 4) for k in PHASES}
                # build-side kinds: + the sweep (16 B per build row + its bit), once per pass; build semi / anti
                # need no walk in the write pass
                sweep = (16 * nb + nb // 8) if bkind else 0
                semi_anti = kind in ((H.HMJ_BUILD_SEMI, H.HMJ_BUILD_ANTI) if bkind else (H.HMJ_JOIN_SEMI, H.HMJ_JOIN_ANTI))
                if mflag:
                    probe_ms = ph["ms_probe_count"] + ph["ms_out_scan"] + ph["ms_probe_write"]
                    row_bytes = 16 if semi_anti else 24
                    probe_bytes = 16 * (nb + npb) + row_bytes * n_rows
                    if bkind:
                        probe_bytes += 2 * sweep + (0 if semi_anti else 16 * (nb + npb))
                else:
                    probe_ms = ph["ms_probe_count"]
                    probe_bytes = 16 * (nb + npb) + sweep
                if kind == H.HMJ_JOIN_INNER:
                    inner_ms[mname] = ms
                line = {"shape": "2^%s x 2^%s" % (lb, lp), "miss_mod": miss, "kind": kname, "mode": mname,
                        "ms_median": round(ms, 4), "x_inner": round(ms / inner_ms[mname], 3) if inner_ms.get(mname) else None,
                        "n_rows": n_rows, "n_probe_matched": cnt["n_probe_matched"], "phases": ph,
                        "path": hex(ts[-1]["path"]), "radix_bits": ts[-1]["radix_bits"],
                        "probe_GBps": round(probe_bytes / (probe_ms * 1e6), 1) if probe_ms > 0 else None,
                        "probe_bytes": probe_bytes, "reps": a.reps}
                print(json.dumps(line), flush=True)
        del bd, pd
        ex.release_result()
        torch.cuda.empty_cache()
    ex.close()


def main_exchange(a):
    import time

    import torch

    import hashmergejoin_amd as H
    from hashmergejoin_amd import dist as hdist

    ex = H.Executor(0)
    hdist.init_comm_single(ex, self_exchange=True, timeout_s=120.0)
    ex.set_profiling(True)
    P, B = H.HMJ_KIND_PROBE_SIDE, H.HMJ_KIND_BUILD_SIDE
    kinds = (("inner", P, H.HMJ_JOIN_INNER), ("semi", P, H.HMJ_JOIN_SEMI), ("anti", P, H.HMJ_JOIN_ANTI),
             ("probe_outer", P, H.HMJ_JOIN_PROBE_OUTER), ("build_semi", B, H.HMJ_BUILD_SEMI), ("build_anti", B, H.HMJ_BUILD_ANTI),
             ("build_outer", B, H.HMJ_BUILD_OUTER), ("full_outer", B, H.HMJ_FULL_OUTER))
    if a.kinds:
        kinds = tuple(k for k in kinds if k[0] in a.kinds.split(",") or k[0] == "inner")
    shapes = a.shapes if a.shapes != SHAPES else EXCHANGE_SHAPES
    for shape in shapes.split(","):
        lb, rest = shape.split("x")
        lp, miss = rest.split("m")
        nb, npb, miss = 1 << int(lb), 1 << int(lp), int(miss)
        bd, pd = ex.gen_build(nb), ex.gen_probe(npb, nb, miss_mod=miss)
        torch.cuda.synchronize()
        inner_ms = None
        for kname, side, kind in kinds:
            walls, infos = [], []
            for i in range(a.warmup + a.reps):
                t0 = time.perf_counter()
                if kind == H.HMJ_JOIN_INNER and side == P:
                    loc, glob = ex.exchange_join(bd, pd, 0)  # (the inner exchange step itself)
                    cnt = {"global": {}}
                else:
                    loc, glob, cnt = ex.exchange_join_kind(bd, pd, side, kind, 0)
                t1 = time.perf_counter()
                if i >= a.warmup:
                    walls.append((t1 - t0) * 1e3)
                    infos.append(ex.last_exchange_info())
            ms = statistics.median(walls)
            if kname == "inner":
                inner_ms = ms
            line = {"exchange": "one rank, RCCL self send/recv", "shape": "2^%s x 2^%s" % (lb, lp), "miss_mod": miss,
                    "kind": kname, "ms_median": round(ms, 3), "x_inner": round(ms / inner_ms, 3) if inner_ms else None,
                    "ms_kernels_median": round(statistics.median(i["ms_kernels"] for i in infos), 3),
                    "rounds": infos[-1]["rounds_probe"], "round_joins": infos[-1]["n_subjoins"],
                    "owner_mode": infos[-1]["owner_mode"], "n_rows": int(glob.n_matches), "counts": cnt["global"],
                    "reps": a.reps}
            print(json.dumps(line), flush=True)
        del bd, pd
        torch.cuda.empty_cache()
    ex.close()


if __name__ == "__main__":
    main()
