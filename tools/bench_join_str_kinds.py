#!/usr/bin/env python3
"""Time the string-key join kinds on the device (hmj_join_kind_str_device) beside the inner string join.  One JSON line.

  configs0     BASELINE configs[0]'s relations (two create_strvec(10^6) over tests/golden/words.txt, seeds 1 and 2);
  synth_2^24   2^24 x 2^24 synthetic keys "synthetic-key-%08d", a quarter of the probe keys missing (probe key i + 2^22).
For each relation pair and each kind x {count, materialise, ordered}: the median of --reps device-timed joins (HIP events
around the call) after --warmup, and the median phase times (hmj_str_kind_opts ms_hash / ms_join / ms_verify / ms_emit /
ms_order, profiling on, --phase-reps joins).  "inner" is hmj_join_str_device in the same run.  For kernel-only times run it
under `rocprofv3 --kernel-trace --stats`.

    python tools/bench_join_str_kinds.py [--reps 10] [--warmup 2] [--phase-reps 3] [--skip-configs0] [--skip-synth]
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

from bench_join_str import synthetic_keys, timed  # noqa: E402

KINDS = (("semi", 0, 1), ("anti", 0, 2), ("probe_outer", 0, 3), ("build_semi", 1, 1), ("build_anti", 1, 2),
         ("build_outer", 1, 3), ("full_outer", 1, 4))
PHASES = ("ms_hash", "ms_join", "ms_verify", "ms_emit", "ms_order")


def bench_pair(H, torch, ex, B, P, args):
    out = {}
    modes = (("count", 0), ("mat", H.HMJ_MATERIALIZE), ("ordered", H.HMJ_ORDERED))
    for mname, flags in modes:
        ex.set_profiling(False)
        ms, (res, _) = timed(torch, lambda: ex.join_str_device(B, P, flags), args.reps, args.warmup)
        out["inner_" + mname] = {"ms": round(ms, 4), "n": int(res.n_matches)}
    for kname, side, kind in KINDS:
        for mname, flags in modes:
            ex.set_profiling(False)
            ms, (res, info) = timed(torch, lambda: ex.join_kind_str_device(B, P, side, kind, flags, probe_fill=1, build_fill=2),
                                    args.reps, args.warmup)
            ex.set_profiling(True)
            ph = {k: [] for k in PHASES}
            for _ in range(args.phase_reps):
                _, inf = ex.join_kind_str_device(B, P, side, kind, flags, probe_fill=1, build_fill=2)
                for k in PHASES:
                    ph[k].append(inf[k])
            ex.set_profiling(False)
            out["%s_%s" % (kname, mname)] = {"ms": round(ms, 4), "n": int(res.n_matches), "n_hash_pairs": info["n_hash_pairs"],
                                             "phases_ms": {k: round(statistics.median(v), 4) for k, v in ph.items()}}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--phase-reps", type=int, default=3)
    ap.add_argument("--skip-configs0", action="store_true")
    ap.add_argument("--skip-synth", action="store_true")
    args = ap.parse_args()
    import torch

    import hashmergejoin_amd as H

    ex = H.Executor(0)
    out = {"tool": "bench_join_str_kinds", "reps": args.reps, "warmup": args.warmup}
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
