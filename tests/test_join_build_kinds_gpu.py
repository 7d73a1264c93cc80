"""GPU checks of the build-side join kinds (hmj_join_build_kind_u64_device): build semi, build anti, build outer and full
outer joins against numpy expectations computed here (test_join_build_kinds_cpu.expect_build_kind), invariants between
the kinds, and the planner's isolation of these joins from inner joins."""
import json
import os

import numpy as np
import pytest

from test_join_build_kinds_cpu import BANTI, BOUTER, BSEMI, FULL, expect_build_kind
from test_join_kinds_cpu import M64, expect_kind

pytestmark = pytest.mark.gpu
VAL_XOR = 0x9E3779B97F4A7C15
KINDS = (BSEMI, BANTI, BOUTER, FULL)


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
    if kind in (BOUTER, FULL):
        return ex.columns_to_numpy(r, host=False)
    assert not r.sval, "build semi / anti results have no sval column"
    return ex.build_rows_to_numpy(r)


def check_bkind(ex, H, B, P, bd, pd, kind, modes=(0, None, None), flags=0, bf=0, pf=0, want=None):
    """Every mode in `modes` (0 = count, HMJ_MATERIALIZE, HMJ_ORDERED) against numpy: rows, checks, all four counters."""
    rows, ck, cnt = want or expect_build_kind(B, P, kind, build_fill=bf, probe_fill=pf)
    for mode in modes:
        if mode is None:
            continue
        r, got_cnt = ex.join_build_kind_device(bd, pd, kind, mode | H.HMJ_CHECKSUM | flags, build_fill=bf, probe_fill=pf)
        assert r.checks() == ck, (kind, mode)
        assert got_cnt == cnt, (kind, mode)
        if mode:
            got = got_rows(ex, r, kind)
            assert np.array_equal(got if mode & H.HMJ_ORDERED else sort_rows(got), rows), (kind, mode)
    return rows, ck, cnt


def all_modes(H):
    return (0, H.HMJ_MATERIALIZE, H.HMJ_ORDERED)


# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log2n", [10, 16, 20])
@pytest.mark.parametrize("miss", [0, 3, 1])
def test_exact_rows_for_every_build_kind(ex, H, log2n, miss):
    n = 1 << log2n
    # probe side as long as, twice and a third of the build side (the last leaves build rows unmatched even with miss 0)
    for npb in (n, 2 * n, n // 3):
        bd, pd = ex.gen_build(n), ex.gen_probe(npb, n, miss_mod=miss)
        B, P = to_np(bd), to_np(pd)
        for kind in KINDS:
            _, _, cnt = check_bkind(ex, H, B, P, bd, pd, kind, all_modes(H), bf=0x5EED, pf=0xABCD)
        if npb < n:
            assert cnt["n_build_unmatched"] >= n - npb
    ex.release_result()


def test_duplicate_keys(ex, H, golden_dir, G):
    for c in G["dup_partitioned"]:
        z = np.load(os.path.join(golden_dir, c["file"]))
        B, P = z["build"], z["probe"]
        bd, pd = to_dev(B), to_dev(P)
        for kind in KINDS:
            check_bkind(ex, H, B, P, bd, pd, kind, all_modes(H), bf=6, pf=5)
        for kind in (BSEMI, BANTI):  # first-wins does not change build semi / anti
            want = expect_build_kind(B, P, kind)
            check_bkind(ex, H, B, P, bd, pd, kind, (0, H.HMJ_ORDERED), flags=H.HMJ_FIRST_WINS, want=want)
        for kind in (BOUTER, FULL):  # ... and is an argument error with the outer kinds
            with pytest.raises(H.HmjError) as ei:
                ex.join_build_kind_device(bd, pd, kind, H.HMJ_FIRST_WINS)
            assert ei.value.code == -1


@pytest.mark.parametrize("bits", [0, 4])
def test_chunked_build_tables(ex, H, oracle, bits):
    # few radix bits: build partitions far beyond one LDS table (5120 rows); every table marks its own build rows
    nb, npb = 200000, 150000
    B, P = oracle.gen_build(nb), oracle.gen_probe(npb, nb, miss_mod=4)
    Bd = np.concatenate([B, B[: nb // 2] ^ np.array([0, 1], np.uint64)])  # half the keys twice: row lists span chunks
    ex.set_radix_bits(bits)
    try:
        for Bx in (B, Bd):
            bd, pd = to_dev(Bx), to_dev(P)
            for kind in KINDS:
                check_bkind(ex, H, Bx, P, bd, pd, kind, (0, H.HMJ_MATERIALIZE), bf=3, pf=4)
                assert ex.last_plan()["path"] & H.HMJ_PATH_CHUNKED_BUILD, kind
    finally:
        ex.set_radix_bits(None)
    ex.release_result()


def test_hot_probe_key_is_split(ex, H):
    # one probe key on 30 % of the rows: its partition is cut into probe slices, and several workgroups mark its build rows
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
            check_bkind(ex, H, B, P, bd, pd, kind, (0, H.HMJ_MATERIALIZE), bf=1, pf=2)
            assert ex.last_timing()["path"] & H.HMJ_PATH_SPLIT, kind
    finally:
        ex.set_profiling(False)
    ex.release_result()


def test_hot_build_key(ex, H):
    # thousands of copies of one build key: each copy is one build semi (or anti) row, and in the build outer join each
    # copy pairs with every probe row of its key
    n = 1 << 16
    B = to_np(ex.gen_build(n)).copy()
    hot_key = B[3, 0]
    hot = np.stack([np.full(6000, hot_key, np.uint64), np.arange(6000, dtype=np.uint64) + 10**9], 1)
    B = np.concatenate([B, hot])
    P = to_np(ex.gen_probe(2 * n, n, miss_mod=3))
    bd, pd = to_dev(B), to_dev(P)
    hot_probe = int((P[:, 0] == hot_key).sum())
    assert hot_probe > 0
    rows, _, _ = check_bkind(ex, H, B, P, bd, pd, BOUTER, all_modes(H), bf=9)
    assert int((rows[:, 0] == hot_key).sum()) == 6001 * hot_probe
    rows, _, _ = check_bkind(ex, H, B, P, bd, pd, BSEMI, (0, H.HMJ_MATERIALIZE))
    assert int((rows[:, 0] == hot_key).sum()) == 6001 and len(np.unique(rows[rows[:, 0] == hot_key, 1])) == 6001
    # the same key, unmatched (the probe rows of that key removed): every copy is a build anti row, once
    P2 = P[P[:, 0] != hot_key]
    pd2 = to_dev(P2)
    rows, _, _ = check_bkind(ex, H, B, P2, bd, pd2, BANTI, (0, H.HMJ_MATERIALIZE, H.HMJ_ORDERED))
    assert int((rows[:, 0] == hot_key).sum()) == 6001
    check_bkind(ex, H, B, P2, bd, pd2, FULL, (0, H.HMJ_MATERIALIZE), bf=9, pf=8)
    ex.release_result()


def test_disjoint_key_ranges(ex, H):
    # build keys in the lower half of the key range, probe keys in the upper half, and a few thousand shared keys: whole
    # partitions hold build rows and no probe rows (all of them build anti / outer rows), and the reverse
    rng = np.random.default_rng(5)
    n = 1 << 18
    Bk = rng.integers(0, 1 << 63, n, dtype=np.uint64)
    Pk = rng.integers(0, 1 << 63, n, dtype=np.uint64) | np.uint64(1 << 63)
    Pk[::64] = Bk[::64]
    B = np.stack([Bk, np.arange(n, dtype=np.uint64)], 1)
    P = np.stack([Pk, np.arange(n, dtype=np.uint64) ^ np.uint64(VAL_XOR)], 1)
    bd, pd = to_dev(B), to_dev(P)
    for kind in KINDS:
        check_bkind(ex, H, B, P, bd, pd, kind, all_modes(H), bf=11, pf=12)
    ex.release_result()


def test_key_sets_that_stress_partitioning(ex, H):
    rng = np.random.default_rng(11)
    n = 1 << 20
    # build keys in a quarter of the key range under uniform probe keys: the dense-build plan
    Bk = rng.integers(0, 1 << 62, n, dtype=np.uint64)
    B = np.stack([Bk, np.arange(n, dtype=np.uint64)], 1)
    Pk = rng.integers(0, 1 << 63, n, dtype=np.uint64) * np.uint64(2) + np.uint64(1)
    Pk[::3] = Bk[: len(Pk[::3])]
    P = np.stack([Pk, np.arange(n, dtype=np.uint64) ^ np.uint64(VAL_XOR)], 1)
    bd, pd = to_dev(B), to_dev(P)
    for kind in (BANTI, FULL):
        check_bkind(ex, H, B, P, bd, pd, kind, (0, H.HMJ_ORDERED), bf=2, pf=3)
    # dense small-integer keys (the shared prefix is skipped, the window placed under it)
    B = np.stack([np.arange(n, dtype=np.uint64), np.arange(n, dtype=np.uint64) * np.uint64(3)], 1)
    P = np.stack([rng.integers(0, 2 * n, n, dtype=np.uint64), np.arange(n, dtype=np.uint64)], 1)
    bd, pd = to_dev(B), to_dev(P)
    for kind in KINDS:
        check_bkind(ex, H, B, P, bd, pd, kind, all_modes(H), bf=2, pf=3)
    # ... and a few keys outside the sampled prefix (none at a sampled position, every n / 2048 + 1-th row), on the probe
    # side and then on the build side: the ordered join finds them and plans again
    outliers = [1000, 300001, 777778]
    assert all(j % (n // 2048 + 1) for j in outliers)
    P2 = P.copy()
    P2[outliers, 0] = np.uint64(1 << 63) + np.arange(3, dtype=np.uint64)
    B2 = B.copy()
    B2[outliers, 0] = np.uint64(1 << 63) + np.arange(10, 13, dtype=np.uint64)
    for Bx, Px in ((B, P2), (B2, P)):
        bdx, pdx = to_dev(Bx), to_dev(Px)
        for kind in KINDS:
            check_bkind(ex, H, Bx, Px, bdx, pdx, kind, (H.HMJ_ORDERED,), bf=2, pf=3)
            assert ex.last_plan()["refused"] & H._lib.HMJ_REFUSED_PREFIX_VIOLATED or ex.last_plan()["attempts"] == 1
        ex.forget_workloads()
        ex.join_build_kind_device(bdx, pdx, BANTI, H.HMJ_ORDERED)
        assert ex.last_plan()["refused"] & H._lib.HMJ_REFUSED_PREFIX_VIOLATED, ex.last_plan()
    ex.release_result()


def test_empty_sides_and_argument_errors(ex, H):
    import ctypes as C

    import torch

    empty = torch.empty((0, 2), dtype=torch.int64, device="cuda:0")
    P = np.array([[5, 50], [7, 70], [5, 51]], np.uint64)
    B = np.array([[5, 1], [6, 2], [6, 3]], np.uint64)
    none = np.zeros((0, 2), np.uint64)
    for Bx, Px, bd, pd in [(none, P, empty, to_dev(P)), (B, none, to_dev(B), empty), (none, none, empty, empty)]:
        for kind in KINDS:
            check_bkind(ex, H, Bx, Px, bd, pd, kind, all_modes(H), bf=4, pf=3)
    # n_probe == 0: build anti, build outer and full outer return every build row
    r, cnt = ex.join_build_kind_device(to_dev(B), empty, FULL, H.HMJ_ORDERED, build_fill=4)
    assert ex.columns_to_numpy(r, host=False).tolist() == [[5, 1, 4], [6, 2, 4], [6, 3, 4]]
    assert cnt == {"n_build_matched": 0, "n_build_unmatched": 3, "n_probe_matched": 0, "n_probe_unmatched": 0}
    r, _ = ex.join_build_kind_device(to_dev(B), empty, BANTI, H.HMJ_ORDERED)
    assert ex.build_rows_to_numpy(r).tolist() == [[5, 1], [6, 2], [6, 3]]
    # n_build == 0: full outer returns every probe row with the fill
    r, cnt = ex.join_build_kind_device(empty, to_dev(P), FULL, H.HMJ_ORDERED, probe_fill=3)
    assert ex.columns_to_numpy(r, host=False).tolist() == [[5, 3, 50], [5, 3, 51], [7, 3, 70]]
    assert cnt == {"n_build_matched": 0, "n_build_unmatched": 0, "n_probe_matched": 0, "n_probe_unmatched": 3}
    for kind in (0, 5):  # unknown kinds
        with pytest.raises(H.HmjError) as ei:
            ex.join_build_kind_device(to_dev(B), to_dev(P), kind)
        assert ei.value.code == -1
    # struct_size too small for the fields the kind reads (build semi reads only the kind)
    bd, pd = to_dev(B), to_dev(P)
    for kind, size, ok in ((BSEMI, 8, True), (BOUTER, 8, False), (BOUTER, 16, True), (FULL, 16, False), (FULL, 24, True),
                           (BSEMI, 4, False)):
        opts = H.BuildJoinOpts()
        opts.struct_size = size
        opts.kind = kind
        res = H.JoinResult()
        rc = ex.L.hmj_join_build_kind_u64_device(ex.h, C.c_void_p(bd.data_ptr()), len(B), C.c_void_p(pd.data_ptr()), len(P),
                                                 0, C.byref(opts), C.byref(res))
        assert (rc == 0) == ok and (ok or rc == -1), (kind, size, rc)
        if ok:  # the counters beyond struct_size are left alone
            assert opts.n_build_matched == 0 and int(res.n_matches) == expect_build_kind(B, P, kind)[1]["n_matches"]


def test_invariants_between_the_kinds(ex, H):
    n = 1 << 16
    bd, pd = ex.gen_build(n), ex.gen_probe(n // 2, n, miss_mod=3)
    B, P = to_np(bd), to_np(pd)
    # build semi rows and build anti rows partition the build rows
    rs, _ = ex.join_build_kind_device(bd, pd, BSEMI, H.HMJ_MATERIALIZE)
    semi = ex.build_rows_to_numpy(rs)
    ra, _ = ex.join_build_kind_device(bd, pd, BANTI, H.HMJ_MATERIALIZE)
    anti = ex.build_rows_to_numpy(ra)
    assert np.array_equal(sort_rows(np.concatenate([semi, anti])), sort_rows(B))
    # full outer = inner + unmatched probe rows + unmatched build rows; its unmatched probe rows are the anti join's
    inner = ex.join_device(bd, pd, 0)
    n_inner = int(inner.n_matches)
    rf, cnt = ex.join_build_kind_device(bd, pd, FULL, H.HMJ_MATERIALIZE, build_fill=1 << 60, probe_fill=1 << 61)
    assert int(rf.n_matches) == n_inner + cnt["n_probe_unmatched"] + cnt["n_build_unmatched"]
    assert cnt["n_build_unmatched"] == len(anti)
    full = ex.columns_to_numpy(rf, host=False)
    pmiss = full[~np.isin(full[:, 0], B[:, 0])]
    assert (pmiss[:, 1] == np.uint64(1 << 61)).all()
    rp, _ = ex.join_kind_device(bd, pd, H.HMJ_JOIN_ANTI, H.HMJ_MATERIALIZE)
    assert np.array_equal(sort_rows(pmiss[:, [0, 2]]), sort_rows(ex.probe_rows_to_numpy(rp)))
    bmiss = full[~np.isin(full[:, 0], P[:, 0])]
    assert np.array_equal(sort_rows(bmiss[:, :2]), sort_rows(anti)) and (bmiss[:, 2] == np.uint64(1 << 60)).all()
    assert expect_kind(B, P, H.HMJ_JOIN_ANTI)[2] == cnt["n_probe_matched"]
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
        modes = all_modes(H)
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
                    exk.join_build_kind_device(bd, pd, kind, m)
                    p = exk.last_plan()
                    assert not p["path"] & bad, (kind, m, hex(p["path"]))
                exk.join_device(bd, pd, m)
                got.append(exk.last_plan())
        assert got == fresh
        exk.prepare_build(bd, 1 << 22)  # a build kind join discards a prepared build side
        exk.join_build_kind_device(bd, pd, BSEMI, 0)
        assert not exk.last_plan()["path"] & H.HMJ_PATH_PREPARED
        check_bkind(exk, H, B, P, bd, pd, FULL, (0, H.HMJ_MATERIALIZE), bf=1, pf=2)
    finally:
        exf.close()
        exk.close()


def test_full_size_full_outer(ex, H):
    # 2^26 x 2^26, miss_mod 4: probe row j misses iff j % 4 == 0 (payload j ^ VAL_XOR); the others hit build row
    # (A j + B) mod n, a bijection of the rows, so the n / 4 build rows the missing j map to are unmatched.  Every build row
    # value (its index) occurs once over pairs and unmatched build rows, every probe payload once over pairs and unmatched
    # probe rows: sum_r = n (n - 1) / 2 + probe_fill n / 4, sum_s = sum_j (j ^ VAL_XOR) + build_fill n / 4.
    n = 1 << 26
    bf, pf = 77, 1 << 40
    bd, pd = ex.gen_build(n), ex.gen_probe(n, n, miss_mod=4)
    s_all = 0
    for j0 in range(0, n, 1 << 24):
        j = np.arange(j0, j0 + (1 << 24), dtype=np.uint64)
        s_all += int((j ^ np.uint64(VAL_XOR)).sum(dtype=np.uint64))
    # rows: 3n/4 pairs + n/4 unmatched probe rows + n/4 unmatched build rows
    want = (3 * n // 4 + n // 4 + n // 4, (n * (n - 1) // 2 + pf * (n // 4)) & M64, (s_all + bf * (n // 4)) & M64)
    r, cnt = ex.join_build_kind_device(bd, pd, FULL, 0, build_fill=bf, probe_fill=pf)
    assert (int(r.n_matches), int(r.sum_r), int(r.sum_s)) == want
    assert cnt == {"n_build_matched": n - n // 4, "n_build_unmatched": n // 4,
                   "n_probe_matched": n - n // 4, "n_probe_unmatched": n // 4}
    del bd, pd
    ex.release_result()
