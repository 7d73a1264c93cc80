"""bench.py on the GPU: --steps sets the timed steps, and --dump-outputs writes what the timed join returned -- its
counts and sums, and with --materialize its rows (all, or the fixed hash sample) -- checked against the CPU oracle."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def run_bench(out_dir, log2n, *extra):
    p = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1",
                        "--log2n", str(log2n), "--steps", "3", "--warmup", "1", "--no-extra", "--no-cpu", "--no-traffic",
                        "--dump-outputs", str(out_dir)] + list(extra), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=400)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    lines = [l for l in p.stdout.decode().splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout.decode()
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["warmup"] == 1 and d["ms_per_step"] > 0, d
    return d


def from_limbs(a):
    a = np.asarray(a)
    assert a.dtype == np.float64 and a.shape[-1] == 4
    return sum(a[..., i].astype(np.uint64) << np.uint64(48 - 16 * i) for i in range(4))


def check_counts(out_dir, n, ck):
    for k, want in (("n_matches", n), ("sum_r", ck["sum_r"]), ("sum_s", ck["sum_s"])):
        assert int(from_limbs(np.load(os.path.join(out_dir, k + ".npy")))) == want, k


def test_dump_outputs_count_mode(oracle, tmp_path):
    n = 1 << 18
    d = run_bench(tmp_path, 18)
    ck, _ = oracle.equijoin(oracle.gen_build(n), oracle.gen_probe(n, n))
    check_counts(tmp_path, n, ck)
    assert sorted(os.listdir(tmp_path)) == ["n_matches.npy", "sum_r.npy", "sum_s.npy"]
    assert d["dump_outputs"]["shapes"] == {"n_matches": [4], "sum_r": [4], "sum_s": [4]}


def test_dump_outputs_materialized_rows_are_the_fixed_sample(oracle, tmp_path):
    import importlib.util

    spec = importlib.util.spec_from_file_location("hmj_bench", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    n = 1 << 20  # > DUMP_ROWS_MAX: sampled
    assert n > bench.DUMP_ROWS_MAX
    run_bench(tmp_path, 20, "--materialize")
    ck, rows = oracle.equijoin(oracle.gen_build(n), oracle.gen_probe(n, n))
    check_counts(tmp_path, n, ck)
    # the sample restated on the host: top b bits of key * 0x9E3779B97F4A7C15 (mod 2^64) zero, sorted by (key, rval, sval)
    b = max(1, (n // bench.DUMP_ROWS_TARGET - 1).bit_length())
    with np.errstate(over="ignore"):
        h = rows[:, 0] * np.uint64(0x9E3779B97F4A7C15)
    want = rows[(h >> np.uint64(64 - b)) == 0]
    want = want[np.lexsort((want[:, 2], want[:, 1], want[:, 0]))]
    got = from_limbs(np.load(os.path.join(tmp_path, "rows.npy")))
    assert 0 < len(want) <= bench.DUMP_ROWS_MAX and np.array_equal(got, want)
