#!/usr/bin/env python3
"""What the key-only probe side's pilot costs, and from which size the path pays (hmj_probekeys.h, HMJ_PROBE_KEYS_MIN_LOG2).

Plain count joins of 2^k x 2^k rows on one warm context, the workload's memo forgotten before every join, so that every
join is a workload's FIRST: with the path on, each one pilots (4096 sampled probe rows + one host sync) and then runs the
key-only passes (clean probe side) or whole rows (--miss m: every m-th probe row has no build row, the pilot declines).
Run the same command on the commit before the path existed for the other half of the comparison: there the loop times the
plain join.  One JSON line per size: median and minimum wall-clock ms per join (stream synchronised) and the path taken.

  python3 tools/exp_probe_keys_pilot.py [--sizes 23,24,25,26] [--miss 0] [--reps 9]"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402,F401  (before the library: one HIP runtime per process)

import hashmergejoin_amd as H  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--sizes", default="23,24,25,26")
ap.add_argument("--miss", type=int, default=0)
ap.add_argument("--reps", type=int, default=9)
args = ap.parse_args()

os.environ.setdefault("HMJ_SLAB_MIN_LOG2", "22")
os.environ.setdefault("HMJ_PROBE_KEYS_MIN_LOG2", "22")  # (ignored by a library without the path)
os.environ.setdefault("HMJ_PROBE_KEYS", "2")  # pilot first, whatever the library's default
ex = H.Executor(0)
keys_bit = getattr(H, "HMJ_PATH_PROBE_KEYS", 0)
for k in [int(s) for s in args.sizes.split(",")]:
    n = 1 << k
    b, p = ex.gen_build(n), ex.gen_probe(n, n, miss_mod=args.miss)
    for _ in range(3):  # allocations, placement, code objects
        r = ex.join_device(b, p, 0)
    ms = []
    for _ in range(args.reps):
        ex.forget_workloads()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = ex.join_device(b, p, 0)
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    plan = ex.last_plan()
    warm = []
    for _ in range(args.reps):  # the workload's later joins: no pilot either way
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = ex.join_device(b, p, 0)
        torch.cuda.synchronize()
        warm.append((time.perf_counter() - t0) * 1e3)
    print(json.dumps({"log2n": k, "miss_mod": args.miss, "n_matches": int(r.n_matches),
                      "first_join_ms_median": round(statistics.median(ms), 4), "first_join_ms_min": round(min(ms), 4),
                      "later_join_ms_median": round(statistics.median(warm), 4), "later_join_ms_min": round(min(warm), 4),
                      "first_path": hex(plan["path"]), "first_key_only": bool(plan["path"] & keys_bit),
                      "later_key_only": bool(ex.last_plan()["path"] & keys_bit), "slab": bool(plan["path"] & H.HMJ_PATH_SLAB)}), flush=True)
    del b, p
ex.close()
