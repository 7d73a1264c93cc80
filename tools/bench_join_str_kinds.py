#!/usr/bin/env python3
"""Time the string-key join kinds on the device (hmj_join_kind_str_device) beside the inner string join.  One JSON line.

  configs0     BASELINE configs[0]'s relations (two create_strvec(10^6) over tests/golden/words.txt, seeds 1 and 2);
  synth_2^24   2^24 x 2^24 synthetic keys "synthetic-key-%08d", a quarter of the probe keys missing (probe key i + 2^22).
For each relation pair and each kind x {count, materialise, ordered}: the median (and min / max) of --reps device-timed
joins (HIP events around the call) after --warmup, and the median phase times (hmj_str_kind_opts ms_hash / ms_join /
ms_verify / ms_emit / ms_order, profiling on, --phase-reps joins).  "inner" is hmj_join_str_device in the same run.  For
kernel-only times run it under `rocprofv3 --kernel-trace --stats`.

--nulls F (NULL keys, validity bitmaps): every call runs three ways on the same rows in the same process -- plain (no
bitmap; the entry above), "<name>@valid" with all-valid bitmaps on both sides, and "<name>@nulls" with a fraction F of
NULL-key rows on each side (seeded) -- and the entries gain n_build_null / n_probe_null.  With bitmaps "inner" is the INNER
kind of hmj_join_kind_str_device, which is where the inner join of nullable keys lives.

    python tools/bench_join_str_kinds.py [--reps 10] [--warmup 2] [--phase-reps 3] [--skip-configs0] [--skip-synth]
                                         [--nulls F] [--kinds inner,semi,...] [--modes count,mat,ordered]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_join_str import synthetic_keys  # noqa: E402

KINDS = (("inner", 0, 0), ("semi", 0, 1), ("anti", 0, 2), ("probe_outer", 0, 3), ("build_semi", 1, 1), ("build_anti", 1, 2),
         ("build_outer", 1, 3), ("full_outer", 1, 4))
PHASES = ("ms_hash", "ms_join", "ms_verify", "ms_emit", "ms_order")


def timed_all(torch, fn, reps, warmup):
    """Every repetition's device time (ms) and the last result."""
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
    return ms, out


def validity_ways(H, nb, np_, frac):
    """name suffix -> keywords of the call: plain, all-valid bitmaps, a fraction `frac` of NULL-key rows per side."""
    ways = [("", {})]
    if frac is None:
        return ways
    rng = np.random.default_rng(20240)
    ones = lambda n: (H.pack_validity(np.ones(n, bool), 0, "cuda"), 0)
    some = lambda n, off: (H.pack_validity(rng.random(n) >= frac, off, "cuda"), off)
    ways.append(("@valid", {"build_valid": ones(nb), "probe_valid": ones(np_)}))
    ways.append(("@nulls", {"build_valid": some(nb, 3), "probe_valid": some(np_, 0)}))
    return ways


def bench_pair(H, torch, ex, B, P, args):
    out = {}
    modes = [m for m in (("count", 0), ("mat", H.HMJ_MATERIALIZE), ("ordered", H.HMJ_ORDERED)) if m[0] in args.modes]
    ways = validity_ways(H, int(B[2].shape[0]), int(P[2].shape[0]), args.nulls)
    for kname, side, kind in KINDS:
        if kname not in args.kinds:
            continue
        for mname, flags in modes:
            for suffix, kw in ways:
                if kname == "inner" and not kw:  # the inner entry itself
                    call = lambda: ex.join_str_device(B, P, flags)
                    prof = None
                else:
                    call = lambda: ex.join_kind_str_device(B, P, side, kind, flags, probe_fill=1, build_fill=2, **kw)
                    prof = call
                ex.set_profiling(False)
                ms, (res, info) = timed_all(torch, call, args.reps, args.warmup)
                e = {"ms": round(statistics.median(ms), 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4),
                     "n": int(res.n_matches), "n_hash_pairs": info["n_hash_pairs"]}
                for k in ("n_build_null", "n_probe_null"):
                    if k in info:
                        e[k] = info[k]
                ex.set_profiling(True)
                ph = {k: [] for k in PHASES}
                for _ in range(args.phase_reps):
                    _, inf = call()
                    for k in PHASES:
                        if k in inf:
                            ph[k].append(inf[k])
                ex.set_profiling(False)
                e["phases_ms"] = {k: round(statistics.median(v), 4) for k, v in ph.items() if v}
                out["%s_%s%s" % (kname, mname, suffix)] = e
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--phase-reps", type=int, default=3)
    ap.add_argument("--skip-configs0", action="store_true")
    ap.add_argument("--skip-synth", action="store_true")
    ap.add_argument("--nulls", type=float, default=None, metavar="F",
                    help="also run every call with all-valid bitmaps and with a fraction F of NULL-key rows per side")
    ap.add_argument("--kinds", default=",".join(k for k, _, _ in KINDS), help="comma-separated subset of the kinds")
    ap.add_argument("--modes", default="count,mat,ordered", help="comma-separated subset of count, mat, ordered")
    args = ap.parse_args()
    args.kinds, args.modes = args.kinds.split(","), args.modes.split(",")
    if args.nulls is not None and not 0.0 <= args.nulls <= 1.0:
        ap.error("--nulls takes a fraction in [0, 1]")
    import torch

    import hashmergejoin_amd as H

    ex = H.Executor(0)
    out = {"tool": "bench_join_str_kinds", "reps": args.reps, "warmup": args.warmup, "nulls": args.nulls}
    if not args.skip_configs0:
        from oracle.pyoracle import create_strvec

        words = open(os.path.join(ROOT, "tests", "golden", "words.txt")).read().split("\n")
        words = words[:-1] if words[-1] == "" else words
        rels = []
        for seed in (1, 2):
            pairs = create_strvec(10 ** 6, words, seed)
            c, o = H.pack_strings([k for k, _ in pairs], device="cuda")
            rels.append((c, o, torch.tensor([v for _, v in pairs], dtype=torch.int64, device="cuda")))
        out["configs0"] = bench_pair(H, torch, ex, rels[0], rels[1], args)
        del rels
    if not args.skip_synth:
        n = 1 << 24
        c, o = synthetic_keys(n + n // 4)
        chars, offs = torch.from_numpy(c).cuda(), torch.from_numpy(o).cuda()
        w = int(o[1])  # (fixed-width keys)
        B = (chars[: n * w], offs[: n + 1], torch.arange(n, dtype=torch.int64, device="cuda"))
        P = (chars[(n // 4) * w:], offs[n // 4:] - offs[n // 4], torch.arange(n, dtype=torch.int64, device="cuda"))
        out["synth_2^24"] = bench_pair(H, torch, ex, B, P, args)
        del B, P, chars, offs
    ex.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
