"""The key-only probe side of plain count joins on the slab path (hashmergejoin_amd/csrc/hmj_probekeys.h; HMJ_PATH_PROBE_KEYS).

When every probe row meets exactly one build row, the probe side goes through the slab passes as 8-byte keys, pass A adds up
the payloads, and the probe kernel verifies the premise row by row; a pilot over 4096 sampled probe rows decides whether the
passes are started at all, and a probe row the pilot missed makes the join redo its probe side with whole rows.  Every case
here compares (n_matches, sum_r, sum_s) with the CPU oracle AND with the same join on an executor created under
HMJ_PROBE_KEYS=0, and asserts on hmj_last_plan / hmj_timing which form produced the result.  Executors are created under
HMJ_SLAB_MIN_LOG2=22 HMJ_PROBE_KEYS_MIN_LOG2=22 so that 2^22 rows per side reach the path."""
import os
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 1 << 22
# (HMJ_PROBE_KEYS=2: pilot first, whatever the library's default)
ENV = {"HMJ_SLAB_MIN_LOG2": "22", "HMJ_PROBE_KEYS_MIN_LOG2": "22", "HMJ_PROBE_KEYS": "2"}
PLAN_FIELDS = ("path", "radix_bits", "radix_passes", "pass_bits", "key_prefix_bits", "key_window_low", "n_partitions", "probe_items",
               "attempts", "refused", "cooling", "workload")


def _executor(extra=None):
    import hashmergejoin_amd as H

    env = dict(ENV, **(extra or {}))
    os.environ.update(env)
    try:
        return H.Executor(0)
    finally:
        for k in env:
            del os.environ[k]


@pytest.fixture(scope="module")
def H():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import hashmergejoin_amd as H

    return H


@pytest.fixture(scope="module")
def ex_off(H):
    e = _executor({"HMJ_PROBE_KEYS": "0"})  # today's path, whole rows: the second reference of every case
    yield e
    e.close()


@pytest.fixture
def make_ex(H):
    made = []

    def make(extra=None):
        made.append(_executor(extra))
        return made[-1]

    yield make
    for e in made:
        e.close()


def to_dev(a):
    import torch

    a = np.ascontiguousarray(a, np.uint64).reshape(-1, 2)
    return torch.from_numpy(a.view(np.int64).copy()).cuda()


def sums(r):
    return int(r.n_matches), int(r.sum_r), int(r.sum_s)


def want_of(oracle, B, P):
    ck, _ = oracle.equijoin(B, P, cap=0)
    return ck["n_matches"], ck["sum_r"], ck["sum_s"]


def pilot_samples(n_probe):
    """The pilot's sample rule, restated from the header: K rows at floor(i * np / K) (all rows where np < K)."""
    src = open(os.path.join(ROOT, "hashmergejoin_amd", "csrc", "hmj_probekeys.h")).read()
    K = int(re.search(r"kProbeKeysPilotRows\s*=\s*(\d+)", src).group(1))
    assert "(uint64_t)i * np / kProbeKeysPilotRows" in src
    return {i * n_probe // K for i in range(min(K, n_probe))}


def one_to_one(oracle, n):
    return oracle.gen_build(n), oracle.gen_probe(n, n)


def join_both(ex, ex_off, B, P):
    """The join on `ex` and on the HMJ_PROBE_KEYS=0 executor: (sums, plan, timing) of the first, sums of the second."""
    b, p = to_dev(B), to_dev(P)
    got = sums(ex.join_device(b, p, 0))
    plan, t = ex.last_plan(), ex.last_timing()
    off = sums(ex_off.join_device(b, p, 0))
    return got, plan, t, off


def test_clean_workload_joined_three_times(H, oracle, ex_off, make_ex):
    L, ex = H._lib, make_ex()
    B, P = one_to_one(oracle, N)
    want = want_of(oracle, B, P)
    assert want == (N, int(B[:, 1].sum(dtype=np.uint64)), int(P[:, 1].sum(dtype=np.uint64)))  # the generators' closed form
    b, p = to_dev(B), to_dev(P)
    assert sums(ex_off.join_device(b, p, 0)) == want
    plans = []
    for _ in range(3):  # the first join pilots, the others start from the workload's memo
        assert sums(ex.join_device(b, p, 0)) == want
        plans.append(ex.last_plan())
        t = ex.last_timing()
        assert plans[-1]["path"] & H.HMJ_PATH_PROBE_KEYS and plans[-1]["path"] & H.HMJ_PATH_SLAB, plans[-1]
        assert plans[-1]["attempts"] == 1 and plans[-1]["cooling"] == 0, plans[-1]
        assert t["path"] == plans[-1]["path"]
        assert t["bytes_scatter"] == 2 * 32 * N + 24 * N + 16 * N and t["bytes_probe_count"] == 16 * N + 8 * N, t
    for k in PLAN_FIELDS:
        assert plans[0][k] == plans[1][k] == plans[2][k], (k, plans)
    assert not plans[0]["refused"] & (L.HMJ_REFUSED_PROBE_KEYS_GAVE_UP | L.HMJ_REFUSED_PROBE_KEYS_COOLING)


@pytest.mark.parametrize("extra", [1, 2047, 2049, 4097])
def test_ragged_sizes_around_the_tiles(H, oracle, ex_off, make_ex, extra):
    # one row, one row short of / past the 2048 rows a pass-A worker's range is made of, one past a 4096-key tile
    n = N + extra
    B, P = one_to_one(oracle, n)
    want = want_of(oracle, B, P)
    got, plan, _, off = join_both(make_ex(), ex_off, B, P)
    assert got == want == off
    assert plan["path"] & H.HMJ_PATH_PROBE_KEYS and plan["attempts"] == 1, plan


def test_several_tiles_per_worker(H, ex_off, make_ex):
    # 2^24 + 4097 rows: a pass-A worker owns 8192 rows -- two 4096-row tiles, so lines are carried from tile to tile under the
    # prefetch -- and the A-slabs hold ~32 keys, so pass B's gather takes its few-slab-starts branches, not only the walk.
    # Device generators and their closed forms (unique build keys with payload = row number; the probe side meets each once).
    n = (1 << 24) + 4097
    ex = make_ex()
    b, p = ex.gen_build(n), ex.gen_probe(n, n)
    want = (n, (n * (n - 1) // 2) % (1 << 64), int(p[:, 1].sum().item()) % (1 << 64))
    for _ in range(2):  # with the pilot, then from the memo
        assert sums(ex.join_device(b, p, 0)) == want
        plan, t = ex.last_plan(), ex.last_timing()
        assert plan["path"] & H.HMJ_PATH_PROBE_KEYS and plan["attempts"] == 1 and plan["cooling"] == 0, plan
        assert t["bytes_scatter"] == (2 * 32 + 24 + 16) * n and t["bytes_probe_count"] == 24 * n, t
    assert sums(ex_off.join_device(b, p, 0)) == want
    assert not ex_off.last_plan()["path"] & H.HMJ_PATH_PROBE_KEYS


def test_payload_sum_wraps(H, oracle, ex_off, make_ex):
    B, P = one_to_one(oracle, N)
    P[:, 1] = (P[:, 1] * np.uint64(0x9E3779B97F4A7C15)) | np.uint64(1 << 63)  # every payload >= 2^63: the total wraps 2^21 times
    want = want_of(oracle, B, P)
    assert want[2] == int(P[:, 1].sum(dtype=np.uint64)) and sum(int(v) for v in P[:1000, 1]) >= 1 << 64
    got, plan, _, off = join_both(make_ex(), ex_off, B, P)
    assert got == want == off
    assert plan["path"] & H.HMJ_PATH_PROBE_KEYS, plan


def _absent_key(B):
    k = np.uint64(0x5EED0000DEADBEEF)
    while (B[:, 0] == k).any():
        k += np.uint64(1)
    return k


def _gave_up_then_cools(H, ex, ex_off, oracle, B, P):
    L = H._lib
    want = want_of(oracle, B, P)
    got, plan, t, off = join_both(ex, ex_off, B, P)
    assert got == want == off  # exact: the probe side was redone with whole rows
    assert not plan["path"] & H.HMJ_PATH_PROBE_KEYS and plan["path"] & H.HMJ_PATH_SLAB, plan
    assert plan["refused"] & L.HMJ_REFUSED_PROBE_KEYS_GAVE_UP and plan["cooling"] & L.HMJ_COOL_PROBE_KEYS, plan
    assert plan["attempts"] == 1, plan  # the redo is not a new plan
    n_b, n_p = len(B), len(P)
    assert t["bytes_scatter"] == 2 * 32 * n_b + (24 + 16) * n_p + 2 * 32 * n_p, t  # build, key passes, whole-row passes
    assert t["bytes_probe_count"] == 16 * n_b + 8 * n_p + 16 * (n_b + n_p), t
    got, plan, t, _ = join_both(ex, ex_off, B, P)  # the workload's next join does not attempt the path
    assert got == want
    assert not plan["path"] & H.HMJ_PATH_PROBE_KEYS and plan["refused"] & L.HMJ_REFUSED_PROBE_KEYS_COOLING, plan
    assert not plan["refused"] & L.HMJ_REFUSED_PROBE_KEYS_GAVE_UP and plan["attempts"] == 1, plan
    assert t["bytes_scatter"] == 2 * 32 * (n_b + n_p), t


@pytest.mark.parametrize("where", ["index_1", "last_row_of_a_ragged_tile"])
def test_one_unmatched_probe_row_the_pilot_does_not_sample(H, oracle, ex_off, make_ex, where):
    n = N if where == "index_1" else N + 2047  # (the last worker's last tile holds 2047 rows)
    idx = 1 if where == "index_1" else n - 1
    assert idx not in pilot_samples(n)
    B, P = one_to_one(oracle, n)
    P[idx, 0] = _absent_key(B)
    _gave_up_then_cools(H, make_ex(), ex_off, oracle, B, P)


def test_one_duplicated_build_key_whose_probe_rows_are_not_sampled(H, oracle, ex_off, make_ex):
    B, P = one_to_one(oracle, N)
    sampled = pilot_samples(N)
    order = np.argsort(P[:, 0], kind="stable")
    pos = order[np.searchsorted(P[:, 0][order], B[:, 0])]  # probe row of every build key
    assert np.array_equal(P[pos, 0], B[:, 0])
    free = [i for i in range(64) if int(pos[i]) not in sampled]
    i, j = free[0], free[1]
    B[j, 0] = B[i, 0]  # probe row pos[i] now meets two build rows, probe row pos[j] none
    _gave_up_then_cools(H, make_ex(), ex_off, oracle, B, P)


def test_every_tenth_probe_row_unmatched_stops_at_the_pilot(H, oracle, ex_off, make_ex):
    L = H._lib
    B, P = oracle.gen_build(N), oracle.gen_probe(N, N, miss_mod=10)
    want = want_of(oracle, B, P)
    assert want[0] < N
    ex = make_ex()
    for _ in range(2):  # (the second join: the workload remembers the pilot's answer; still nothing cools)
        got, plan, t, off = join_both(ex, ex_off, B, P)
        assert got == want == off
        assert t["bytes_scatter"] == 4 * 32 * N and t["bytes_probe_count"] == 16 * 2 * N, t  # no key-only pass was launched
        assert not plan["path"] & H.HMJ_PATH_PROBE_KEYS and plan["path"] & H.HMJ_PATH_SLAB and plan["attempts"] == 1, plan
        assert not plan["cooling"] & L.HMJ_COOL_PROBE_KEYS, plan
        assert not plan["refused"] & (L.HMJ_REFUSED_PROBE_KEYS_GAVE_UP | L.HMJ_REFUSED_PROBE_KEYS_COOLING), plan


def test_foreign_key_shape_on_the_two_sided_slab_path(H, oracle, ex_off, make_ex):
    # every build key is met by two probe rows, every probe row meets one build row: 2^22 x 2^23 stays on the two-sided slab path
    nb, npb = N, 1 << 23
    B, P = oracle.gen_build(nb), oracle.gen_probe(npb, nb)
    want = want_of(oracle, B, P)
    assert want[0] == npb and want[2] == int(P[:, 1].sum(dtype=np.uint64))
    got, plan, t, off = join_both(make_ex(), ex_off, B, P)
    assert got == want == off
    assert plan["path"] & H.HMJ_PATH_SLAB and not plan["path"] & H.HMJ_PATH_SLAB_PROBE, plan
    assert plan["path"] & H.HMJ_PATH_PROBE_KEYS and plan["attempts"] == 1, plan
    assert t["bytes_probe_count"] == 16 * nb + 8 * npb, t


def test_switched_off_plans_as_before(H, oracle, make_ex):
    L = H._lib
    B, P = one_to_one(oracle, N)
    ex0 = make_ex({"HMJ_PROBE_KEYS": "0"})  # (an executor of its own: the plan must not depend on what the shared one has seen)
    got, plan, t, off = join_both(make_ex(), ex0, B, P)
    p0, t0 = ex0.last_plan(), ex0.last_timing()
    assert got == off == want_of(oracle, B, P)
    new_refused = L.HMJ_REFUSED_PROBE_KEYS_GAVE_UP | L.HMJ_REFUSED_PROBE_KEYS_COOLING
    assert not p0["path"] & H.HMJ_PATH_PROBE_KEYS and not p0["refused"] & new_refused and not p0["cooling"] & L.HMJ_COOL_PROBE_KEYS
    assert p0["path"] == plan["path"] & ~H.HMJ_PATH_PROBE_KEYS and p0["path"] & H.HMJ_PATH_SLAB, (p0, plan)
    for k in PLAN_FIELDS[1:]:  # everything but the path bit is what the key-only join reports too
        assert p0[k] == plan[k], (k, p0, plan)
    assert t0["bytes_scatter"] == 4 * 32 * N and t0["bytes_probe_count"] == 16 * 2 * N, t0


def test_forced_slab_overflow_ends_on_the_exact_path(H, oracle, make_ex):
    # the hot-key relations of test_gpu_join.py: half the rows in one radix digit, a slab overflows
    L = H._lib
    keys = oracle.gen_build(N)[:, 0]
    hot = keys.copy()
    hot[: N // 2] = (hot[: N // 2] & np.uint64((1 << 50) - 1)) | np.uint64(0xABC << 52)
    B = np.stack([hot, np.arange(N, dtype=np.uint64)], 1)
    P = np.stack([hot[::-1].copy(), np.arange(N, dtype=np.uint64) + np.uint64(9)], 1)
    want = want_of(oracle, B, P)
    for extra in (None, {"HMJ_PROBE_KEYS": "1"}):  # with the pilot in front, and with the key-only passes started unasked
        got, plan, _, off = join_both(make_ex(extra), make_ex({"HMJ_PROBE_KEYS": "0"}), B, P)  # (the overflow cools a workload: no shared executor)
        assert got == want == off
        assert plan["attempts"] == 2 and plan["path"] & H.HMJ_PATH_EXACT and not plan["path"] & H.HMJ_PATH_PROBE_KEYS, plan
        assert plan["refused"] & L.HMJ_REFUSED_SLAB_OVERFLOW and plan["cooling"] & L.HMJ_COOL_SLAB, plan
