#!/usr/bin/env python3
"""Time the mixed-key join on the device (hmj_join_mixed_device) on a (string of ~22 bytes, int32) key.  One JSON line, no gate.

  Sizes: 2^24 x 2^24 rows ("synthetic-key-%08d" strings, 22 bytes each, as tools/bench_join_str.py makes them; the probe side a
  permutation of the build side) and 10^6 x 10^6 rows (two create_strvec(10^6) relations over tests/golden/words.txt, seeds 1
  and 2, as bench_join_str.py's configs0).  The int32 column is a function of the string, so equal strings are equal tuples
  and the tuples are as unique as the strings.  Kinds: inner count, inner ordered, probe SEMI and FULL_OUTER (count mode).

  Per size and kind, in one process and on the same rows:
  ms           median of --reps device-timed calls (HIP events around the call) after --warmup, profiling off
  str_ms       hmj_join_kind_str_device on the string column alone, same kind and flags, timed the same way
  cols_ms      hmj_join_kind_cols_device on a hashed [8,4] key (the row's id scattered over 64 bits, the same int32 column)
  phases_ms    median hmj_mixed_opts ms_key / ms_join / ms_verify / ms_emit / ms_order (profiling on, separate calls)

  key_kernel (per size, from the inner count calls with profiling on; median, min and max of the repetitions):
  ms_key       both relations' mix_key_kernel launches -- with HMJ_SUM_PROBE off nothing else lies between the two events
  bytes        the kernel's algorithmic bytes over both relations: the chars + 8 per row of offsets + 4 per row of the int32
               column read, 16 per row of {key64,row} written -- and the share of the 8 TB/s HBM peak that is at ms_key
  yardstick    ms_hash of the string join + ms_key of the column join in this same run: together they read what the mixed
               key kernel reads (the column join 8 bytes a row more: its id column) and write the rows twice

  --null-equal: NULL-equals-NULL matching (HMJ_NULL_EQUAL) instead.  The same relations with 10 % of the int32 column's
  slots NULL on each side (the strings keep the tuples distinct); per size and kind the call runs once under SQL semantics (sql_ms: the call without the flag, the
  yardstick) and once under the flag (null_equal_ms) in this one process, with ms_key and ms_verify of both from separate
  calls with profiling on.  No gate.

    python tools/bench_join_mixed.py [--reps 20] [--warmup 3] [--sizes 2^24 10^6] [--null-equal]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
HBM_TBPS = 8.0

from bench_join_str import synthetic_keys, timed  # noqa: E402


def spread(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


def relations(torch, H, size):
    """(build, probe): per side (chars, offsets, day int32, id int64) device tensors."""
    if size == "10^6":
        from oracle.pyoracle import create_strvec

        words = open(os.path.join(ROOT, "tests", "golden", "words.txt")).read().split("\n")
        words = words[:-1] if words[-1] == "" else words
        ids = {}
        out = []
        for seed in (1, 2):
            keys = [k.encode("utf-8") if isinstance(k, str) else bytes(k) for k, _ in create_strvec(10 ** 6, words, seed)]
            c, o = H.pack_strings(keys, device="cuda")
            idv = np.array([ids.setdefault(k, len(ids)) for k in keys], np.uint64)
            out.append((c, o, idv))
        return [(c, o, torch.from_numpy((idv % np.uint64(36500)).astype(np.int32)).cuda(),
                 torch.from_numpy((idv * np.uint64(0x9E3779B97F4A7C15)).view(np.int64)).cuda()) for c, o, idv in out]
    n = 1 << 24
    c, o = synthetic_keys(n)
    width = len(c) // n
    ids = np.arange(n, dtype=np.uint64)
    perm = np.random.default_rng(24).permutation(n)
    out = []
    for order in (None, perm):
        m, idv = (c.reshape(n, width), ids) if order is None else (c.reshape(n, width)[order], ids[order])
        out.append((torch.from_numpy(np.ascontiguousarray(m).reshape(-1)).cuda(), torch.from_numpy(o).cuda(),
                    torch.from_numpy((idv % np.uint64(36500)).astype(np.int32)).cuda(),
                    torch.from_numpy((idv * np.uint64(0x9E3779B97F4A7C15)).view(np.int64)).cuda()))
    return out


def bench_null_equal(torch, H, ex, args, kinds, out, frac=0.1):
    out["null_slots_frac"] = frac
    for size in args.sizes:
        (bc, bo, bday, bid), (pc, po, pday, pid) = relations(torch, H, size)
        nb, np_ = bday.shape[0], pday.shape[0]
        rng = np.random.default_rng(7)
        mb, mp = rng.random(nb) >= frac, rng.random(np_) >= frac
        vb, vp = [None, H.pack_validity(mb, 0, "cuda")], [None, H.pack_validity(mp, 0, "cuda")]
        rec = {"n_build": nb, "n_probe": np_}
        for name, side, kind, flags in kinds:
            row = {}
            for vname, flag in (("sql", 0), ("null_equal", H.HMJ_NULL_EQUAL)):
                fn = lambda: ex.join_mixed_device([(bc, bo), bday], None, [(pc, po), pday], None, side, kind, flags | flag, build_valid=vb,
                                                  probe_valid=vp)
                ex.set_profiling(False)
                ms, (res, inf) = timed(torch, fn, args.reps, args.warmup)
                assert (inf["n_build_null"], inf["n_probe_null"]) == (int((~mb).sum()), int((~mp).sum()))
                ex.set_profiling(True)
                ph = [fn()[1] for _ in range(max(5, args.reps // 2))]
                ex.set_profiling(False)
                row[vname + "_ms"] = round(ms, 4)
                row[vname] = {"n_matches": int(res.n_matches), "ms_key": round(statistics.median(p["ms_key"] for p in ph), 4),
                              "ms_verify": round(statistics.median(p["ms_verify"] for p in ph), 4)}
            row["null_equal_vs_sql"] = round(row["null_equal_ms"] / row["sql_ms"], 3)
            rec[name] = row
        out[size] = rec
        del bc, bo, bday, bid, pc, po, pday, pid, vb, vp
        ex.release_result()
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sizes", nargs="+", default=["2^24", "10^6"], choices=["2^24", "10^6"])
    ap.add_argument("--null-equal", action="store_true",
                    help="time each call under SQL semantics and under HMJ_NULL_EQUAL on the same rows with 10 %% NULL int32 slots")
    args = ap.parse_args()
    import torch

    import hashmergejoin_amd as H

    ex = H.Executor(0)
    out = {"tool": "bench_join_mixed", "reps": args.reps, "warmup": args.warmup}
    P, B = H.HMJ_KIND_PROBE_SIDE, H.HMJ_KIND_BUILD_SIDE
    kinds = (("inner_count", P, H.HMJ_JOIN_INNER, 0), ("inner_ordered", P, H.HMJ_JOIN_INNER, H.HMJ_ORDERED),
             ("semi", P, H.HMJ_JOIN_SEMI, 0), ("full_outer", B, H.HMJ_FULL_OUTER, 0))
    if args.null_equal:
        bench_null_equal(torch, H, ex, args, kinds, out)
        ex.close()
        print(json.dumps(out))
        return
    for size in args.sizes:
        (bc, bo, bday, bid), (pc, po, pday, pid) = relations(torch, H, size)
        nb, np_ = bday.shape[0], pday.shape[0]
        bvals, pvals = torch.arange(nb, dtype=torch.int64, device="cuda"), torch.arange(np_, dtype=torch.int64, device="cuda")
        mixed = lambda s, k, f: ex.join_mixed_device([(bc, bo), bday], None, [(pc, po), pday], None, s, k, f)
        strj = lambda s, k, f: ex.join_kind_str_device((bc, bo, bvals), (pc, po, pvals), s, k, f)
        colj = lambda s, k, f: ex.join_kind_cols_device([bid, bday], None, [pid, pday], None, s, k, f)
        rec = {"n_build": nb, "n_probe": np_, "avg_key_bytes": round((bc.numel() + pc.numel()) / (nb + np_), 2)}
        for name, side, kind, flags in kinds:
            ex.set_profiling(False)
            ms, (res, _) = timed(torch, lambda: mixed(side, kind, flags), args.reps, args.warmup)
            ms_s, (res_s, _) = timed(torch, lambda: strj(side, kind, flags), args.reps, args.warmup)
            ms_c, (res_c, _) = timed(torch, lambda: colj(side, kind, flags), args.reps, args.warmup)
            assert int(res.n_matches) == int(res_s.n_matches) == int(res_c.n_matches), name
            ex.set_profiling(True)
            ph = {k: [] for k in ("ms_key", "ms_join", "ms_verify", "ms_emit", "ms_order")}
            hs, kc = [], []
            for _ in range(args.reps):
                inf = mixed(side, kind, flags)[1]
                for k in ph:
                    ph[k].append(inf[k])
                if name == "inner_count":
                    hs.append(strj(side, kind, flags)[1]["ms_hash"])
                    kc.append(colj(side, kind, flags)[1]["ms_key"])
            ex.set_profiling(False)
            rec[name] = {"ms": round(ms, 4), "str_ms": round(ms_s, 4), "cols_ms": round(ms_c, 4), "n_matches": int(res.n_matches),
                         "phases_ms": {k: round(statistics.median(v), 4) for k, v in ph.items()}}
            if name == "inner_count":
                byts = bc.numel() + pc.numel() + (8 + 4 + 16) * (nb + np_)
                mk = statistics.median(ph["ms_key"])
                rec["key_kernel"] = {"ms_key": spread(ph["ms_key"]), "bytes": byts, "TBps": round(byts / mk / 1e9, 3),
                                     "share_of_8TBps": round(byts / mk / 1e9 / HBM_TBPS, 3),
                                     "yardstick": {"str_ms_hash": spread(hs), "cols_ms_key": spread(kc),
                                                   "sum_of_medians": round(statistics.median(hs) + statistics.median(kc), 4)}}
        out[size] = rec
        del bc, bo, bday, bid, pc, po, pday, pid, bvals, pvals
    ex.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
