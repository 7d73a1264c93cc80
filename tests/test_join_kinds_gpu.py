"""GPU checks of the join kinds (hmj_join_kind_u64_device): semi, anti and probe-side outer joins against numpy
expectations computed here (test_join_kinds_cpu.expect_kind), the reference's partitioned probe loop against the compiled
reference's record (golden.json), and the planner's isolation of kind joins from inner joins."""
import json
import os

import numpy as np
import pytest

from test_join_kinds_cpu import ANTI, M64, OUTER, SEMI, expect_kind

pytestmark = pytest.mark.gpu
VAL_XOR = 0x9E3779B97F4A7C15
KINDS = (SEMI, ANTI, OUTER)


@pytest.fixture(scope="module")
def H():
    import hashmergejoin_amd as H

    return H


@pytest.fixture(scope="module")
def ex(H):
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    e = H.Executor(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def G(golden_dir):
    with open(os.path.join(golden_dir, "golden.json")) as f:
        return json.load(f)["cases"]


def to_dev(a):
    import torch

    a = np.ascontiguousarray(a, np.uint64).reshape(-1, 2)
    return torch.from_numpy(a.view(np.int64).copy()).cuda()


def to_np(t):
    return t.cpu().numpy().view(np.uint64).reshape(-1, 2)


def sort_rows(a):
    return a[np.lexsort(tuple(a[:, k] for k in reversed(range(a.shape[1]))))] if len(a) else a


def got_rows(ex, r, kind):
    if kind == OUTER:
        return ex.columns_to_numpy(r, host=False)
    assert not r.rval, "semi / anti results have no rval column"
    return ex.probe_rows_to_numpy(r)


def check_kind(ex, H, B, P, bd, pd, kind, modes=(0, None, None), first=False, fill=0, want=None):
    """Every mode in `modes` (0 = count, HMJ_MATERIALIZE, HMJ_ORDERED) against numpy: rows, checks, both counters."""
    rows, ck, matched = want or expect_kind(B, P, kind, first_wins=first, fill=fill)
    for mode in modes:
        if mode is None:
            continue
        fl = mode | H.HMJ_CHECKSUM | (H.HMJ_FIRST_WINS if first else 0)
        r, cnt = ex.join_kind_device(bd, pd, kind, fl, outer_fill=fill)
        assert r.checks() == ck, (kind, mode, first)
        assert cnt == {"n_probe_matched": matched, "n_probe_unmatched": len(P) - matched}, (kind, mode)
        if mode:
            got = got_rows(ex, r, kind)
            assert np.array_equal(got if mode & H.HMJ_ORDERED else sort_rows(got), rows), (kind, mode, first)
    return rows, ck, matched


# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log2n", [10, 16, 20])
@pytest.mark.parametrize("miss", [0, 3, 1])
def test_exact_rows_for_every_kind(ex, H, log2n, miss):
    n = 1 << log2n
    modes = (0, H.HMJ_MATERIALIZE, H.HMJ_ORDERED)
    # unique keys, then every build key met by two probe rows (duplicate probe keys)
    for npb in (n, 2 * n):
        bd, pd = ex.gen_build(n), ex.gen_probe(npb, n, miss_mod=miss)
        B, P = to_np(bd), to_np(pd)
        for kind in KINDS:
            check_kind(ex, H, B, P, bd, pd, kind, modes, fill=0xABCD)
        check_kind(ex, H, B, P, bd, pd, OUTER, modes, first=True)
        if miss == 1:  # every probe row misses
            assert expect_kind(B, P, SEMI)[2] == 0
    ex.release_result()


def test_duplicate_build_keys(ex, H, golden_dir, G):
    for c in G["dup_partitioned"]:
        z = np.load(os.path.join(golden_dir, c["file"]))
        B, P = z["build"], z["probe"]
        bd, pd = to_dev(B), to_dev(P)
        modes = (0, H.HMJ_MATERIALIZE, H.HMJ_ORDERED)
        for kind in KINDS:
            check_kind(ex, H, B, P, bd, pd, kind, modes, fill=5)
        check_kind(ex, H, B, P, bd, pd, OUTER, modes, first=True)
        for kind in (SEMI, ANTI):  # first-wins does not change semi / anti
            want = expect_kind(B, P, kind)
            check_kind(ex, H, B, P, bd, pd, kind, (0, H.HMJ_ORDERED), first=True, want=want)


def test_the_reference_partitioned_probe_loop(ex, H, G, golden_dir):
    # hashjoin_bench.cc:92-96 visits every probe row and adds r.second + s_tables[i][r.first] (first insert wins, a miss
    # reads 0): PROBE_OUTER | FIRST_WINS with fill 0, row by row -- its sum is the compiled reference's record
    for c in G["gen_join"]:
        nb, npb, miss = c["n_build"], c["n_probe"], c["miss_mod"]
        bd, pd = ex.gen_build(nb), ex.gen_probe(npb, nb, miss_mod=miss)
        r, cnt = ex.join_kind_device(bd, pd, H.HMJ_JOIN_PROBE_OUTER, H.HMJ_FIRST_WINS, outer_fill=0)
        assert int(r.n_matches) == npb
        assert (int(r.sum_r) + int(r.sum_s)) & M64 == c["psum_T1_bits10"][0]
        assert cnt["n_probe_matched"] + cnt["n_probe_unmatched"] == npb
    for c in G["dup_partitioned"]:
        z = np.load(os.path.join(golden_dir, c["file"]))
        r, cnt = ex.join_kind_device(to_dev(z["build"]), to_dev(z["probe"]), H.HMJ_JOIN_PROBE_OUTER,
                                     H.HMJ_FIRST_WINS | H.HMJ_MATERIALIZE)
        assert int(r.n_matches) == len(z["probe"])
        assert (int(r.sum_r) + int(r.sum_s)) & M64 == c["psum"]
        assert cnt["n_probe_matched"] == int(np.isin(z["probe"][:, 0], z["build"][:, 0]).sum())


@pytest.mark.parametrize("bits", [0, 4])
def test_chunked_build_tables(ex, H, oracle, bits):
    # few radix bits: build partitions far beyond one LDS table (5120 rows) -- hits are marked in the bitmap chunk by
    # chunk and the unmatched rows emitted after the last one (an answer emitted per chunk would repeat rows)
    nb, npb = 200000, 150000
    B, P = oracle.gen_build(nb), oracle.gen_probe(npb, nb, miss_mod=4)
    Bd = np.concatenate([B, B[: nb // 2] ^ np.array([0, 1], np.uint64)])  # half the keys twice: row lists span chunks
    ex.set_radix_bits(bits)
    try:
        for Bx in (B, Bd):
            bd, pd = to_dev(Bx), to_dev(P)
            for kind in KINDS:
                check_kind(ex, H, Bx, P, bd, pd, kind, (0, H.HMJ_MATERIALIZE), fill=3)
            check_kind(ex, H, Bx, P, bd, pd, OUTER, (0, H.HMJ_MATERIALIZE), first=True)
            # the inner part of the outer join is the oracle's equijoin
            r, _ = ex.join_kind_device(bd, pd, H.HMJ_JOIN_PROBE_OUTER, H.HMJ_MATERIALIZE, outer_fill=3)
            got = ex.columns_to_numpy(r, host=False)
            _, inner = oracle.equijoin(Bx, P)
            hit = np.isin(got[:, 0], Bx[:, 0])
            assert np.array_equal(sort_rows(got[hit]), inner)
            t = ex.last_plan()
            assert t["path"] & H.HMJ_PATH_CHUNKED_BUILD, t
    finally:
        ex.set_radix_bits(None)
    ex.release_result()


def test_hot_probe_key_is_split(ex, H):
    nb = npb = 1 << 22
    bd = ex.gen_build(nb)
    B = to_np(bd)
    P = to_np(ex.gen_probe(npb, nb, miss_mod=3)).copy()
    hot = np.random.default_rng(7).random(npb) < 0.3
    P[hot, 0] = B[12345, 0]
    pd = to_dev(P)
    ex.set_profiling(True)
    try:
        for kind in KINDS:
            check_kind(ex, H, B, P, bd, pd, kind, (0, H.HMJ_MATERIALIZE), fill=1)
            assert ex.last_timing()["path"] & H.HMJ_PATH_SPLIT, kind
    finally:
        ex.set_profiling(False)
    ex.release_result()


def test_hot_build_key_is_not_cut_into_build_slices(ex, H):
    # thousands of copies of one build key: the inner join's enumerating modes cut that partition into build slices;
    # an outer join must not (a probe row would meet its key's rows in several work items)
    n = 1 << 16
    B = to_np(ex.gen_build(n)).copy()
    hot = np.stack([np.full(6000, B[3, 0], np.uint64), np.arange(6000, dtype=np.uint64) + 10**9], 1)
    B = np.concatenate([B, hot])
    P = to_np(ex.gen_probe(2 * n, n, miss_mod=3))
    bd, pd = to_dev(B), to_dev(P)
    check_kind(ex, H, B, P, bd, pd, OUTER, (0, H.HMJ_MATERIALIZE, H.HMJ_ORDERED), fill=9)
    for kind in (SEMI, ANTI):
        check_kind(ex, H, B, P, bd, pd, kind, (0, H.HMJ_MATERIALIZE))
    ex.release_result()


def test_edge_inputs(ex, H):
    import torch

    empty = torch.empty((0, 2), dtype=torch.int64, device="cuda:0")
    P = np.array([[5, 50], [7, 70], [5, 51]], np.uint64)
    B = np.array([[5, 1]], np.uint64)
    cases = [(np.zeros((0, 2), np.uint64), P, empty, to_dev(P)), (B, np.zeros((0, 2), np.uint64), to_dev(B), empty),
             (np.zeros((0, 2), np.uint64), np.zeros((0, 2), np.uint64), empty, empty)]
    for Bx, Px, bd, pd in cases:
        for kind in KINDS:
            check_kind(ex, H, Bx, Px, bd, pd, kind, (0, H.HMJ_MATERIALIZE, H.HMJ_ORDERED), fill=4)
    # n_build == 0: ANTI is the whole probe side, OUTER every probe row with the fill
    r, cnt = ex.join_kind_device(empty, to_dev(P), H.HMJ_JOIN_PROBE_OUTER, H.HMJ_ORDERED, outer_fill=4)
    assert ex.columns_to_numpy(r, host=False).tolist() == [[5, 4, 50], [5, 4, 51], [7, 4, 70]]
    assert cnt == {"n_probe_matched": 0, "n_probe_unmatched": 3}
    with pytest.raises(H.HmjError) as ei:  # an unknown kind
        ex.join_kind_device(to_dev(B), to_dev(P), 4)
    assert ei.value.code == -1


def test_key_sets_that_stress_partitioning(ex, H):
    rng = np.random.default_rng(11)
    n = 1 << 20
    # build keys in a quarter of the key range under uniform probe keys: the dense-build plan, most build partitions
    # empty of build rows -- their probe rows are the anti join's answer
    Bk = rng.integers(0, 1 << 62, n, dtype=np.uint64)
    B = np.stack([Bk, np.arange(n, dtype=np.uint64)], 1)
    Pk = rng.integers(0, 1 << 63, n, dtype=np.uint64) * np.uint64(2) + np.uint64(1)
    Pk[::3] = Bk[: len(Pk[::3])]
    P = np.stack([Pk, np.arange(n, dtype=np.uint64) ^ np.uint64(VAL_XOR)], 1)
    bd, pd = to_dev(B), to_dev(P)
    rows, _, matched = check_kind(ex, H, B, P, bd, pd, ANTI, (0, H.HMJ_MATERIALIZE))
    assert len(rows) > n // 2 and matched >= len(Pk[::3])
    check_kind(ex, H, B, P, bd, pd, OUTER, (0, H.HMJ_ORDERED), fill=2)
    # dense small-integer keys (the shared prefix is skipped, the window placed under it)
    B = np.stack([np.arange(n, dtype=np.uint64), np.arange(n, dtype=np.uint64) * np.uint64(3)], 1)
    P = np.stack([rng.integers(0, 2 * n, n, dtype=np.uint64), np.arange(n, dtype=np.uint64)], 1)
    bd, pd = to_dev(B), to_dev(P)
    for kind in KINDS:
        check_kind(ex, H, B, P, bd, pd, kind, (0, H.HMJ_MATERIALIZE, H.HMJ_ORDERED), fill=2)
    # ... and a few probe keys outside the sampled prefix (none at a sampled position, every n / 2048 + 1-th row): the
    # ordered join finds them and plans again
    P2 = P.copy()
    outliers = [1000, 300001, 777778]
    assert all(j % (n // 2048 + 1) for j in outliers)
    P2[outliers, 0] = np.uint64(1 << 63) + np.arange(3, dtype=np.uint64)
    pd2 = to_dev(P2)
    for kind in KINDS:
        check_kind(ex, H, B, P2, bd, pd2, kind, (H.HMJ_ORDERED,), fill=2)
        assert ex.last_plan()["refused"] & H._lib.HMJ_REFUSED_PREFIX_VIOLATED or ex.last_plan()["attempts"] == 1
    ex.forget_workloads()
    ex.join_kind_device(bd, pd2, ANTI, H.HMJ_ORDERED)
    assert ex.last_plan()["refused"] & H._lib.HMJ_REFUSED_PREFIX_VIOLATED, ex.last_plan()
    ex.release_result()


FORBIDDEN = ("GLOBAL_TABLE", "LDS_TABLE", "SLAB_ONE_PASS", "UNIQ_WRITE", "SORTED_WRITE", "SORTED_FK", "SORTED_FK_HALF",
             "SORTED_FK_WIDE", "ORDER_BY_RANK_SORT", "RANK_RUNS", "ORDERED_EXPANSION", "KEY_RANGES", "PREPARED")


def test_planner_isolation(H):
    bad = 0
    for name in FORBIDDEN:
        bad |= getattr(H._lib, "HMJ_PATH_" + name)
    exf, exk = H.Executor(0), H.Executor(0)
    try:
        bd, pd = exf.gen_build(1 << 8), exf.gen_probe(1 << 22, 1 << 8, miss_mod=3)
        B, P = to_np(bd), to_np(pd)
        modes = (0, H.HMJ_MATERIALIZE, H.HMJ_ORDERED)
        # inner joins on a fresh ctx: what they plan when nothing else ran
        fresh = []
        for _ in range(2):
            for m in modes:
                exf.join_device(bd, pd, m)
                fresh.append(exf.last_plan())
        got = []
        for _ in range(2):
            for m in modes:
                for kind in KINDS:
                    r, _ = exk.join_kind_device(bd, pd, kind, m)
                    p = exk.last_plan()
                    assert not p["path"] & bad, (kind, m, hex(p["path"]))
                exk.join_device(bd, pd, m)
                got.append(exk.last_plan())
        assert got == fresh
        exk.prepare_build(bd, 1 << 22)  # a kind join discards a prepared build side
        exk.join_kind_device(bd, pd, SEMI, 0)
        assert not exk.last_plan()["path"] & H.HMJ_PATH_PREPARED
        check_kind(exk, H, B, P, bd, pd, ANTI, (0, H.HMJ_MATERIALIZE))
    finally:
        exf.close()
        exk.close()


def test_inner_through_the_kind_entry_is_the_inner_join(ex, H):
    bd, pd = ex.gen_build(1 << 16), ex.gen_probe(1 << 17, 1 << 16, miss_mod=3)
    for fl in (H.HMJ_CHECKSUM, H.HMJ_MATERIALIZE | H.HMJ_CHECKSUM, H.HMJ_ORDERED | H.HMJ_CHECKSUM):
        a = ex.join_device(bd, pd, fl)
        ra, pa = ex.columns_to_numpy(a, host=False) if fl != H.HMJ_CHECKSUM else None, ex.last_plan()
        b, cnt = ex.join_kind_device(bd, pd, H.HMJ_JOIN_INNER, fl)
        assert b.checks() == a.checks() and ex.last_plan()["path"] == pa["path"]
        assert cnt == {"n_probe_matched": 0, "n_probe_unmatched": 0}
        if ra is not None:
            rb = ex.columns_to_numpy(b, host=False)
            assert np.array_equal(sort_rows(ra), sort_rows(rb))


def test_full_size_semi_and_anti(ex, H):
    # 2^26 x 2^26, miss_mod 4: probe row j misses iff j % 4 == 0, its payload is j ^ VAL_XOR
    n = 1 << 26
    bd, pd = ex.gen_build(n), ex.gen_probe(n, n, miss_mod=4)
    s_hit = s_miss = 0
    for j0 in range(0, n, 1 << 24):
        j = np.arange(j0, j0 + (1 << 24), dtype=np.uint64)
        v = j ^ np.uint64(VAL_XOR)
        miss = (j % np.uint64(4)) == 0
        s_miss += int(v[miss].sum(dtype=np.uint64))
        s_hit += int(v[~miss].sum(dtype=np.uint64))
    for kind, want_n, want_s in ((SEMI, n - n // 4, s_hit & M64), (ANTI, n // 4, s_miss & M64)):
        for fl in (0, H.HMJ_CHECKSUM):
            r, cnt = ex.join_kind_device(bd, pd, kind, fl)
            assert (int(r.n_matches), int(r.sum_r), int(r.sum_s)) == (want_n, 0, want_s), kind
            assert cnt == {"n_probe_matched": n - n // 4, "n_probe_unmatched": n // 4}
    del bd, pd
    ex.release_result()
