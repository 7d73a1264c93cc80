#!/usr/bin/env python3
"""Time WHERE on the device (hmj_filter_device) beside two yardsticks.  One JSON line.

  Cases, at 2^24 and 2^26 rows: one I32 column `x < lit` at selectivity 1 %, 50 % and 99 %; three clauses over (I32, F64 with
  10 % NULLs, I64); 22-byte strings EQ (the literal is one of the rows) and STARTS_WITH (a two-letter prefix); the 50 % I32
  term through a random row map.  Per case:

  filter_ms           median of --reps device-timed calls (HIP events around the call) after --warmup, profiling off
  phases_ms           median hmj_filter_opts ms_eval / ms_write (profiling on, separate calls)
  torch_ms            the same predicate composed from torch ops ending in torch.nonzero, same process, timed the same way
  copy_ms             one device copy that moves the bytes DESIGN.md's byte model counts for the case (the columns once, n / 8
                      bytes of mask written and read, 8 bytes per passing row; a map adds its 8 n): a tensor of half that
                      many bytes copied once, so read + written = the model's bytes
  vs_torch, vs_copy   filter_ms / torch_ms, filter_ms / copy_ms

  There is no gate.  The inputs are drawn on the device; every case's map is checked against the torch result.

    python tools/bench_filter.py [--reps 10] [--warmup 2] [--log2 24 26]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.bench_order_by import device_bitmap, fixed_strings, timed  # noqa: E402

CASES = ("i32_lt_1pct", "i32_lt_50pct", "i32_lt_99pct", "three_clauses", "str22_eq", "str22_starts_with", "i32_lt_50pct_random_map")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--log2", type=int, nargs="+", default=[24, 26])
    args = ap.parse_args()
    import torch

    import hashmergejoin_amd as H

    assert torch.cuda.is_available(), "bench_filter needs a GPU"
    ex = H.Executor(0)
    out = {"tool": "bench_filter", "reps": args.reps, "warmup": args.warmup, "device": torch.cuda.get_device_name(0)}
    gen = torch.Generator(device="cuda")
    for lg in args.log2:
        n = 1 << lg
        for case in CASES:
            try:
                gen.manual_seed(lg * 100 + len(case))
                col_bytes = 0
                if case.startswith("i32_lt"):
                    x = torch.randint(0, 100, (n,), device="cuda", generator=gen, dtype=torch.int32)
                    lit = {"1pct": 1, "50pct": 50, "99pct": 99}[case.split("_")[2]]
                    col_bytes = 4 * n
                    if case.endswith("random_map"):
                        rmap_in = torch.randint(0, n, (n,), device="cuda", generator=gen, dtype=torch.int64)
                        terms = [{"column": x, "op": H.HMJ_FILTER_LT, "lit": lit, "row_map": rmap_in}]
                        col_bytes += 8 * n
                        ref = lambda: torch.nonzero(x[rmap_in] < lit).reshape(-1)  # noqa: E731
                    else:
                        terms = [{"column": x, "op": H.HMJ_FILTER_LT, "lit": lit}]
                        ref = lambda: torch.nonzero(x < lit).reshape(-1)  # noqa: E731
                elif case == "three_clauses":
                    a = torch.randint(0, 100, (n,), device="cuda", generator=gen, dtype=torch.int32)
                    b = torch.randn(n, device="cuda", generator=gen, dtype=torch.float64)
                    c = torch.randint(-(1 << 40), 1 << 40, (n,), device="cuda", generator=gen, dtype=torch.int64)
                    valid = torch.rand(n, device="cuda", generator=gen) >= 0.1
                    bits = device_bitmap(torch, valid)
                    terms = [{"column": a, "op": H.HMJ_FILTER_LT, "lit": 70, "clause": 0},
                             {"column": b, "op": H.HMJ_FILTER_GT, "lit": -0.5, "valid": bits, "clause": 1},
                             {"column": c, "op": H.HMJ_FILTER_GE, "lit": 0, "clause": 2}]
                    col_bytes = (4 + 8 + 8) * n + n // 8
                    ref = lambda: torch.nonzero((a < 70) & (b > -0.5) & valid & (c >= 0)).reshape(-1)  # noqa: E731
                else:
                    chars, offsets = fixed_strings(torch, gen, n, 22)
                    body = chars.reshape(n, 22)
                    k = 22 if case == "str22_eq" else 2
                    lit_t = body[n // 3, :k].clone()
                    lit = bytes(lit_t.cpu().numpy().tobytes())
                    op = H.HMJ_FILTER_EQ if case == "str22_eq" else H.HMJ_FILTER_STARTS_WITH
                    terms = [{"column": (chars, offsets), "op": op, "lit": lit}]
                    col_bytes = (22 + 8) * n
                    ref = lambda: torch.nonzero((body[:, :k] == lit_t).all(1)).reshape(-1)  # noqa: E731
                ex.set_profiling(False)
                filter_ms, (rmap, _, info) = timed(torch, lambda: ex.filter_device(terms), args.reps, args.warmup)
                torch_ms, want = timed(torch, ref, args.reps, args.warmup)
                assert torch.equal(rmap, want), case
                del rmap, want
                ex.set_profiling(True)
                ph = {k: [] for k in ("ms_eval", "ms_write")}
                for _ in range(max(3, args.reps // 2)):
                    _, _, inf = ex.filter_device(terms)
                    for k in ph:
                        ph[k].append(inf[k])
                ex.set_profiling(False)
                model_bytes = col_bytes + 2 * (n // 8) + 8 * info["n_out"]
                src = torch.empty(model_bytes // 2, dtype=torch.uint8, device="cuda")
                dst = torch.empty_like(src)
                copy_ms, _ = timed(torch, lambda: dst.copy_(src), args.reps, args.warmup)
                del src, dst
                out["%s_2^%d" % (case, lg)] = {"n_out": info["n_out"], "n_unknown": info["n_unknown"], "filter_ms": round(filter_ms, 4),
                                               "phases_ms": {k: round(statistics.median(v), 4) for k, v in ph.items()},
                                               "torch_ms": round(torch_ms, 4), "model_bytes": model_bytes, "copy_ms": round(copy_ms, 4),
                                               "vs_torch": round(filter_ms / torch_ms, 3), "vs_copy": round(filter_ms / copy_ms, 3)}
                del terms, ref
                torch.cuda.empty_cache()
            except Exception as e:  # keep what was measured: the line is printed at the end
                out["%s_2^%d" % (case, lg)] = {"error": str(e).splitlines()[0][:200]}
                ex.close()
                print(json.dumps(out))
                raise
    ex.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
