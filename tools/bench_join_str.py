#!/usr/bin/env python3
"""Time the string-key join on the device (hmj_join_str_device) and its hash kernel (hmj_hash_str_device).  One JSON line.

  configs0_*   BASELINE configs[0]'s relations (two create_strvec(10^6) over tests/golden/words.txt, seeds 1 and 2), ordered
               and count mode: median of --reps device-timed joins (HIP events around the call) after --warmup, and the
               median phase times (hmj_str_join_opts ms_hash / ms_join / ms_verify / ms_order, profiling on).  Compare with
               bench.py's extra.configs0_strgen_1M_ms (the C++ drop-in, which hashes and verifies on the host).
  hash_2^k     synthetic keys "synthetic-key-%08d" (22 bytes each), 2^24 and 2^26 of them: hash kernel time (events around
               hmj_hash_str_device) and its algorithmic bytes -- chars + 8 (n + 1) read, 8 n (bare hashes) written; the {hash,row}
               rows of a join write 16 n.  For kernel-only times run it under `rocprofv3 --kernel-trace --stats`.
  verify_2^24  a 2^24 x 2^24 materialising join of those keys: ms_verify and the verification's algorithmic bytes -- per pair
               24 B of (hash, r_row, s_row) + 32 B of offsets + both keys read in pass 1; per survivor 24 B + 16 B of payloads read
               and 40 B written in pass 2.

    python tools/bench_join_str.py [--reps 20] [--warmup 3] [--skip-configs0] [--hash-only]
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


def synthetic_keys(n):
    """chars / offsets (numpy) of "synthetic-key-%08d" % i, i < n (22 bytes each for n <= 10^8)."""
    prefix = np.frombuffer(b"synthetic-key-", np.uint8)
    width = len(prefix) + 8
    m = np.empty((n, width), np.uint8)
    m[:, : len(prefix)] = prefix
    v = np.arange(n, dtype=np.int64)
    for p in range(8):
        m[:, width - 1 - p] = ord("0") + (v // 10 ** p) % 10
    return m.reshape(-1), np.arange(n + 1, dtype=np.int64) * width


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
    ap.add_argument("--skip-configs0", action="store_true")
    ap.add_argument("--hash-only", action="store_true", help="the hash kernel at 2^24 and 2^26 only (for a kernel trace)")
    args = ap.parse_args()
    import torch

    import hashmergejoin_amd as H

    ex = H.Executor(0)
    out = {"tool": "bench_join_str", "reps": args.reps, "warmup": args.warmup}
    if not args.hash_only and not args.skip_configs0:
        from oracle.pyoracle import create_strvec

        words = open(os.path.join(ROOT, "tests", "golden", "words.txt")).read().split("\n")
        words = words[:-1] if words[-1] == "" else words
        rels = []
        for seed in (1, 2):
            pairs = create_strvec(10 ** 6, words, seed)
            c, o = H.pack_strings([k for k, _ in pairs], device="cuda")
            rels.append((c, o, torch.tensor([v for _, v in pairs], dtype=torch.int64, device="cuda")))
        for name, flags in (("ordered", H.HMJ_ORDERED), ("count", 0)):
            ex.set_profiling(False)
            ms, (res, info) = timed(torch, lambda: ex.join_str_device(rels[0], rels[1], flags), args.reps, args.warmup)
            ex.set_profiling(True)
            ph = {k: [] for k in ("ms_hash", "ms_join", "ms_verify", "ms_order")}
            for _ in range(max(5, args.reps // 2)):
                _, inf = ex.join_str_device(rels[0], rels[1], flags)
                for k in ph:
                    ph[k].append(inf[k])
            ex.set_profiling(False)
            out["configs0_" + name] = {"ms": round(ms, 4), "n_matches": int(res.n_matches),
                                       "sum": (int(res.sum_r) + int(res.sum_s)) & ((1 << 64) - 1),
                                       "phases_ms": {k: round(statistics.median(v), 4) for k, v in ph.items()},
                                       "path": ex.last_plan()["path"], "key_bytes": int(rels[0][1][-1]) + int(rels[1][1][-1])}
        del rels
    for lg in (24, 26):
        n = 1 << lg
        c, o = synthetic_keys(n)
        chars, offs = torch.from_numpy(c).cuda(), torch.from_numpy(o).cuda()
        ms, _ = timed(torch, lambda: ex.hash_str_device(chars, offs), args.reps, args.warmup)
        byts = len(c) + 8 * (n + 1) + 8 * n
        out["hash_2^%d" % lg] = {"ms": round(ms, 4), "avg_key_bytes": len(c) / n, "bytes": byts,
                                 "TBps": round(byts / ms / 1e9, 3), "share_of_8TBps": round(byts / ms / 1e9 / HBM_TBPS, 3)}
        if lg == 24 and not args.hash_only:
            vals = torch.arange(n, dtype=torch.int64, device="cuda")
            rel = (chars, offs, vals)
            ex.set_profiling(True)
            ph = []
            for _ in range(max(5, args.reps // 2)):
                res, inf = ex.join_str_device(rel, rel, H.HMJ_MATERIALIZE)
                ph.append(inf)
            ex.set_profiling(False)
            mv = statistics.median(p["ms_verify"] for p in ph)
            kl = len(c) / n
            vb = int(n * (24 + 32 + 2 * kl) + int(res.n_matches) * (24 + 16 + 40))
            out["verify_2^24"] = {"ms_verify": round(mv, 4), "bytes": vb, "TBps": round(vb / mv / 1e9, 3),
                                  "ms_hash": round(statistics.median(p["ms_hash"] for p in ph), 4),
                                  "ms_join": round(statistics.median(p["ms_join"] for p in ph), 4)}
            del vals, rel
        del chars, offs
    ex.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
