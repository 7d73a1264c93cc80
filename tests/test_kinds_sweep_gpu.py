"""Randomized and plan-crossing GPU checks of every join kind, u64 and string: a seeded sweep of all nine u64 variants over
the cases of test_kinds_sweep_cpu.draw_u64_case (sizes at the thread-ownership, bitmap-word, sweep-tile and table-capacity
edges, five key distributions, forced radix bits), a ledger of the plan features the default seed reaches, the plan
features crossed with HMJ_ORDERED by name (chunked build tables, split hot partitions, both at once, first-wins beyond
65 535 rows, a one-partition size grid), a seeded sweep of the string join and its eight (side, kind) pairs, and the
identities between the kinds at 2^22 + 5 and 2^24 rows with duplicate keys on both sides, anchored to torch reductions.
Every comparison is exact; the expectations are numpy's (expect_kind, expect_build_kind) and pure Python's (kind_brute)."""
import os
import time

import numpy as np
import pytest

from test_join_str_cpu import M64, str_hash
from test_join_str_gpu import brute, checks_of, rel, unordered
from test_join_str_kinds_cpu import ALL_KINDS, INNER, PROBE
from test_join_str_kinds_gpu import check_kind as check_str_kind
from test_kinds_sweep_cpu import (SEVEN, STR_ITERS, STR_SEED, U64_ITERS, U64_SEED, VARIANTS, draw_str_case, draw_u64_case,
                                  expect_variant, str_tag)

pytestmark = pytest.mark.gpu
WITH_FIRST_OUTER = SEVEN[:3] + [VARIANTS[3]] + SEVEN[3:]  # the seven kinds and first-wins PROBE_OUTER


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


def to_dev(a):
    import torch

    a = np.ascontiguousarray(a, np.uint64).reshape(-1, 2)
    return torch.from_numpy(a.view(np.int64).copy()).cuda()


def sort_rows(a):
    return a[np.lexsort(tuple(a[:, k] for k in reversed(range(a.shape[1]))))] if len(a) else a


def mode_name(H, flags):
    return "ordered" if flags & H.HMJ_ORDERED else "materialize" if flags & H.HMJ_MATERIALIZE else "count"


def run_variant(ex, H, bd, pd, variant, flags, fills):
    _, family, kind, first = variant
    fl = flags | (H.HMJ_FIRST_WINS if first else 0)
    if family == "probe":
        return ex.join_kind_device(bd, pd, kind, fl, outer_fill=fills[0])
    return ex.join_build_kind_device(bd, pd, kind, fl, build_fill=fills[1], probe_fill=fills[0])


def check_variant(ex, H, B, P, bd, pd, variant, flags, fills, tag, want=None):
    """One variant in one mode against numpy: checks, counters, sum_probe_all, the columns hmj.h states for the kind, rows
    (as a sequence under HMJ_ORDERED, after a lexicographic sort otherwise).  Returns last_plan()."""
    name, family, kind, first = variant
    rows, ck, counters = want or expect_variant(B, P, variant, fills)
    tag = tag + (name, flags)
    r, cnt = run_variant(ex, H, bd, pd, variant, flags, fills)
    plan = ex.last_plan()
    assert int(r.n_matches) == ck["n_matches"], (tag, int(r.n_matches), ck["n_matches"])
    assert (int(r.sum_r), int(r.sum_s)) == (ck["sum_r"], ck["sum_s"]), tag
    if flags & H.HMJ_CHECKSUM:
        assert r.checks() == ck, tag
    assert cnt == counters, (tag, cnt, counters)
    if flags & H.HMJ_SUM_PROBE:
        assert int(r.sum_probe_all) == int(P[:, 1].sum(dtype=np.uint64)), tag
    if flags & (H.HMJ_MATERIALIZE | H.HMJ_ORDERED):
        two = rows.shape[1] == 2  # SEMI / ANTI: (key, sval), no rval column; BUILD_SEMI / BUILD_ANTI: (key, rval), no sval
        if len(rows):
            assert r.key, tag
            assert bool(r.rval) == (not two or family == "build"), tag
            assert bool(r.sval) == (not two or family == "probe"), tag
        got = (ex.columns_to_numpy(r, host=False) if not two else
               ex.probe_rows_to_numpy(r) if family == "probe" else ex.build_rows_to_numpy(r))
        assert got.shape == rows.shape, (tag, got.shape, rows.shape)
        if flags & H.HMJ_ORDERED:
            assert np.array_equal(got, rows), (tag, np.flatnonzero(np.any(got != rows, axis=1))[:5])
        else:
            assert np.array_equal(sort_rows(got), rows), tag
    return plan


def path_names(H, path):
    names = {getattr(H._lib, n): n[9:] for n in dir(H._lib) if n.startswith("HMJ_PATH_")}
    return "|".join(sorted(names.get(1 << b, hex(1 << b)) for b in range(32) if path >> b & 1))


# What the default seed and iteration count reach, per (entry family, mode): the HMJ_PATH_* bits seen on any join, and
# whether a join planned again ("replanned": attempts > 1), met a key outside the sampled prefix ("prefix_violated") or gave a
# partition to several work items ("sliced": probe_items > n_partitions).  Observed on an MI355X; a planner change that
# routes the sweep around one of these turns the test red.  (More may be reached: this is the minimum.)
COVERAGE = {
    ("probe", "count"): ("CHUNKED_BUILD|EXACT|HOT_KEY_HINT|PRESORTED|WINDOW", ["sliced"]),
    ("probe", "materialize"): ("CHUNKED_BUILD|EXACT|HOT_KEY_HINT|PRESORTED|SPLIT|WINDOW", ["sliced"]),
    ("probe", "ordered"): ("EXACT|HOT_KEY_HINT|PRESORTED", []),
    ("build", "count"): ("CHUNKED_BUILD|EXACT|HOT_KEY_HINT|PRESORTED|WINDOW", ["sliced"]),
    ("build", "materialize"): ("CHUNKED_BUILD|EXACT|HOT_KEY_HINT|PRESORTED|SPLIT|WINDOW", ["sliced"]),
    ("build", "ordered"): ("EXACT|HOT_KEY_HINT|PRESORTED", []),
}
# (the default seed's ordered cases reach neither chunked tables nor slices nor a split: the directed crossings below do)


def test_u64_sweep_of_every_kind(H):
    default = "HMJ_STRESS_ITERS" not in os.environ and "HMJ_STRESS_SEED" not in os.environ
    iters = int(os.environ.get("HMJ_STRESS_ITERS", U64_ITERS))
    rng = np.random.default_rng(int(os.environ.get("HMJ_STRESS_SEED", U64_SEED)))
    modes = [H.HMJ_CHECKSUM, H.HMJ_MATERIALIZE | H.HMJ_CHECKSUM, H.HMJ_ORDERED | H.HMJ_CHECKSUM]
    ledger, drawn = {}, set()
    ex = H.Executor(0)  # its own: nothing but this sweep's kind joins has run on it when the inner joins below plan
    try:
        for it in range(iters):
            B, P, fills, ctag = draw_u64_case(rng)
            nb, npb = len(B), len(P)
            forced = int(rng.integers(0, H.plan(max(nb, 1))[0] + 3)) if rng.random() < 0.3 else None
            m = int(rng.integers(0, 3))
            flags = modes[m] | (H.HMJ_SUM_PROBE if rng.integers(0, 3) == 0 else 0)
            drawn.add(modes[m] & ~H.HMJ_CHECKSUM)
            tag = (it,) + ctag + (forced,)
            bd, pd = to_dev(B), to_dev(P)
            t0 = time.perf_counter()
            if forced is not None:
                ex.set_radix_bits(forced)
            try:
                for v in VARIANTS:
                    p = check_variant(ex, H, B, P, bd, pd, v, flags, fills, tag)
                    e = ledger.setdefault((v[1], mode_name(H, flags)), {"path": 0, "events": set()})
                    e["path"] |= p["path"]
                    e["events"] |= {name for name, on in (("replanned", p["attempts"] > 1),
                                                          ("prefix_violated", p["refused"] & H._lib.HMJ_REFUSED_PREFIX_VIOLATED),
                                                          ("sliced", p["probe_items"] > p["n_partitions"])) if on}
            except AssertionError:
                if os.environ.get("HMJ_STRESS_DUMP"):  # keep the first failing case's relations
                    np.save(os.path.join(os.environ["HMJ_STRESS_DUMP"], "fail_kinds_B.npy"), B)
                    np.save(os.path.join(os.environ["HMJ_STRESS_DUMP"], "fail_kinds_P.npy"), P)
                raise
            finally:
                if forced is not None:
                    ex.set_radix_bits(None)
            if iters > U64_ITERS:  # offline runs: progress (pytest -s)
                print("kinds stress", tag, hex(flags), "%.2f s" % (time.perf_counter() - t0), flush=True)
        seen = {k: (path_names(H, e["path"]), sorted(e["events"])) for k, e in sorted(ledger.items())}
        print("coverage ledger:", seen, flush=True)
        if default:
            for key, (names, events) in COVERAGE.items():
                bits = 0
                for n in filter(None, names.split("|")):
                    bits |= getattr(H._lib, "HMJ_PATH_" + n)
                assert key in ledger and ledger[key]["path"] & bits == bits and set(events) <= ledger[key]["events"], (key, seen)
        # the sweep has taught inner joins nothing: they plan on this ctx as on a fresh one
        fresh = H.Executor(0)
        try:
            for mflags in sorted(drawn):
                ex.join_device(bd, pd, mflags)
                fresh.join_device(bd, pd, mflags)
                assert ex.last_plan() == fresh.last_plan(), (mflags, ex.last_plan(), fresh.last_plan())
        finally:
            fresh.close()
    finally:
        ex.close()


# ---------------------------------------------------------------------------------------------
def crossing(ex, H, B, P, variants, mode_list, fills, tag, plan_check):
    bd, pd = to_dev(B), to_dev(P)
    for v in variants:
        want = expect_variant(B, P, v, fills)
        for mode in mode_list:
            p = check_variant(ex, H, B, P, bd, pd, v, mode | H.HMJ_CHECKSUM, fills, tag, want=want)
            plan_check(p, (tag, v[0], mode))
    ex.release_result()


@pytest.mark.parametrize("bits", [0, 4])
def test_ordered_rows_from_chunked_build_tables(ex, H, oracle, bits):
    # the ordered epilogue over a partition's walk rows followed by its swept build rows, where the build partition is many
    # LDS tables (200 000 rows in 1 or 16 partitions of 5120-row tables) and row lists span tables
    nb, npb = 200000, 150000
    B, P = oracle.gen_build(nb), oracle.gen_probe(npb, nb, miss_mod=4)
    Bd = np.concatenate([B, B[: nb // 2] ^ np.array([0, 1], np.uint64)])

    def chunked(p, tag):
        assert p["path"] & H.HMJ_PATH_CHUNKED_BUILD and p["n_partitions"] == 1 << bits, (tag, p)

    ex.set_radix_bits(bits)
    try:
        for name, Bx in (("unique", B), ("half twice", Bd)):
            crossing(ex, H, Bx, P, WITH_FIRST_OUTER, (H.HMJ_ORDERED,), (3, 4), (bits, name), chunked)
    finally:
        ex.set_radix_bits(None)


def test_ordered_rows_from_a_split_hot_partition(ex, H):
    # 30 % of the probe rows on one build key: that partition is cut into probe slices, several workgroups mark its build
    # rows, and the ordered epilogue sorts a partition whose rows came from many work items
    nb = npb = 1 << 22
    B = ex.gen_build(nb).cpu().numpy().view(np.uint64).reshape(-1, 2)
    P = ex.gen_probe(npb, nb, miss_mod=3).cpu().numpy().view(np.uint64).reshape(-1, 2).copy()
    P[np.random.default_rng(7).random(npb) < 0.3, 0] = B[12345, 0]

    def split(p, tag):
        assert p["path"] & H.HMJ_PATH_SPLIT and p["probe_items"] > p["n_partitions"], (tag, p)

    crossing(ex, H, B, P, WITH_FIRST_OUTER, (H.HMJ_ORDERED,), (1, 2), ("split",), split)


def test_chunked_build_partitions_probed_by_several_work_items(ex, H, oracle):
    # 16 forced partitions of ~98 000 build rows (about twenty 5120-row tables each, half the keys twice) under 2^21 probe
    # rows, 30 % of them on one key: with so few partitions the planner gives each several probe slices (Q > 1), or -- where
    # the key sample saw the hot key -- one item each and the split step cuts the hot partition.  Either way several
    # workgroups walk the same build partition's tables and mark the same bitmap words.
    nb, npb = 1 << 20, 1 << 21
    B = oracle.gen_build(nb)
    B = np.concatenate([B, B[: nb // 2] ^ np.array([0, 1], np.uint64)])
    P = oracle.gen_probe(npb, nb, miss_mod=3)
    P[np.random.default_rng(8).random(npb) < 0.3, 0] = B[4321, 0]

    def chunked_and_sliced(p, tag):
        assert p["path"] & H.HMJ_PATH_CHUNKED_BUILD and p["n_partitions"] == 16, (tag, p)
        assert p["probe_items"] > p["n_partitions"] or p["path"] & H.HMJ_PATH_SPLIT, (tag, p)

    ex.set_radix_bits(4)
    try:
        crossing(ex, H, B, P, SEVEN, (0, H.HMJ_MATERIALIZE, H.HMJ_ORDERED), (5, 6), ("chunked x sliced",), chunked_and_sliced)
    finally:
        ex.set_radix_bits(None)


@pytest.mark.parametrize("bits", [0, 1])
def test_first_wins_outer_in_a_partition_of_more_than_65535_rows(ex, H, oracle, bits):
    # first-wins keeps the POSITION of a key's first row in its partition (test_gpu_join.py: position 65535 once collided
    # with the 16-bit "no entry" marker).  The same relations for the kinds, and with every build key twice in shuffled
    # input order, so that the first row of a key is not its only row
    nb = 70000
    B, P = oracle.gen_build(nb), oracle.gen_probe(nb, nb)
    B2 = np.concatenate([B, B ^ np.array([0, 1], np.uint64)])[np.random.default_rng(9).permutation(2 * nb)]

    def planned(p, tag):
        assert p["n_partitions"] == 1 << bits, (tag, p)

    ex.set_radix_bits(bits)
    try:
        for name, Bx in (("unique", B), ("twice", B2)):
            variants = [VARIANTS[3], VARIANTS[0], VARIANTS[1], VARIANTS[4]]  # outer | first-wins, semi, anti, semi | first-wins
            crossing(ex, H, Bx, P, variants, (0, H.HMJ_ORDERED), (7, 0), (bits, name), planned)
    finally:
        ex.set_radix_bits(None)


GRID = [1, 31, 32, 33, 1023, 1024, 1025, 4095, 4096, 4097, 5119, 5120, 5121]


@pytest.mark.parametrize("bits", [0, 1])
def test_partition_size_grid(ex, H, bits):
    # one partition (forced 0 bits): the partition size IS the relation size, so these sizes are the kernels' own edges -- a
    # row's bit owned by thread j mod 1024, 32 rows per bitmap word, 64 rows folded per mark, 1024 rows per sweep tile, 5120
    # rows per LDS table -- on both sides, all pairs.  Two partitions (1 bit): the second one starts wherever the first one
    # ends, so a wave's 64 row bits straddle three bitmap words (with one partition every wave starts at a word boundary).
    rng = np.random.default_rng(10 + bits)
    ex.set_radix_bits(bits)
    try:
        for nb in GRID:
            keys = rng.permutation(2 * nb)[: nb - nb // 4].astype(np.uint64)  # from a random half of 0 .. 2 nb
            kb = np.concatenate([keys, keys[::3][: nb // 4]])  # ... every third one twice: nb rows in all
            assert len(kb) == nb
            if bits:  # (the radix digit is taken from the keys' top bits: spread the small integers over them)
                kb = kb * np.uint64(0x9E3779B97F4A7C15)
            B = np.stack([rng.permutation(kb), rng.integers(0, 1 << 62, size=nb, dtype=np.uint64)], 1)
            for npb in GRID:
                kp = rng.integers(0, 2 * nb, size=npb, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15 if bits else 1)
                P = np.stack([kp, rng.integers(0, 1 << 62, size=npb, dtype=np.uint64)], 1)
                bd, pd = to_dev(B), to_dev(P)
                for v in SEVEN:
                    want = expect_variant(B, P, v, (11, 12))
                    for mode in (0, H.HMJ_ORDERED):
                        p = check_variant(ex, H, B, P, bd, pd, v, mode | H.HMJ_CHECKSUM, (11, 12), (bits, nb, npb), want=want)
                        assert p["n_partitions"] == 1 << bits, (nb, npb, p)
    finally:
        ex.set_radix_bits(None)
    ex.release_result()


# ---------------------------------------------------------------------------------------------
def test_string_sweep_of_the_join_and_every_kind(H, ex):
    default = "HMJ_STRESS_ITERS" not in os.environ and "HMJ_STRESS_SEED" not in os.environ
    iters = int(os.environ.get("HMJ_STRESS_ITERS", STR_ITERS))
    rng = np.random.default_rng(int(os.environ.get("HMJ_STRESS_SEED", STR_SEED)))
    modes = [H.HMJ_CHECKSUM, H.HMJ_MATERIALIZE | H.HMJ_CHECKSUM, H.HMJ_ORDERED | H.HMJ_CHECKSUM]
    pf, bf = 0x1111222233334444, 0xAAAA0000BBBB0001
    ambiguous_round = mixed_sort = 0
    for it in range(iters):
        c = draw_str_case(rng)
        flags = modes[int(rng.integers(0, 3))] | (H.HMJ_SUM_PROBE if rng.integers(0, 3) == 0 else 0)
        bk, bv, pk, pv, bits = c["bk"], c["bv"], c["pk"], c["pv"], c["hash_bits"]
        tag = (it,) + str_tag(c) + (flags,)
        t0 = time.perf_counter()
        B, P = rel(H, bk, bv, c["shift_b"], c["base_b"]), rel(H, pk, pv, c["shift_p"], c["base_p"])
        for (chars, offs, _), keys in ((B, bk), (P, pk)):
            got = ex.hash_str_device(chars, offs, hash_bits=bits).cpu().numpy().view(np.uint64)
            assert [int(x) for x in got] == [str_hash(k, bits) for k in keys], tag
        want, coll = brute(bk, bv, pk, pv, bits)
        res, info = ex.join_str_device(B, P, flags, hash_bits=bits)
        assert res.checks() == checks_of(want), tag
        assert (info["n_collisions"], info["n_hash_pairs"]) == (coll, len(want) + coll), (tag, info, coll, len(want))
        if flags & H.HMJ_SUM_PROBE:
            assert int(res.sum_probe_all) == sum(pv) & M64, tag
        inner = ex.str_rows_to_numpy(res) if flags & (H.HMJ_MATERIALIZE | H.HMJ_ORDERED) else None
        if flags & H.HMJ_ORDERED:
            assert np.array_equal(inner, want), tag
        elif inner is not None:
            assert np.array_equal(unordered(inner), unordered(want)), tag
        else:
            assert not res.hash, tag
        for side, kind in ALL_KINDS:
            try:
                kres, kinfo = check_str_kind(H, ex, B, P, bk, bv, pk, pv, side, kind, flags, bits, pf, bf)
            except AssertionError as e:
                raise AssertionError((tag, side, kind)) from e
            if (side, kind) == (PROBE, INNER):  # the inner kind is the inner string join, row for row
                assert (kinfo["n_collisions"], kinfo["n_hash_pairs"]) == (coll, len(want) + coll), tag
                if inner is not None:
                    krows = ex.str_kind_rows_to_numpy(kres)
                    assert np.array_equal(krows, inner) if flags & H.HMJ_ORDERED else \
                        np.array_equal(unordered(krows), unordered(inner)), tag
            elif kind in (1, 2):  # semi / anti of either side (HMJ_JOIN_SEMI == HMJ_BUILD_SEMI, ..._ANTI likewise)
                ambiguous_round += kinfo["n_collisions"] > 0
            else:  # the three outer kinds
                mixed_sort += bool(c["mixed_run"] and flags & H.HMJ_ORDERED)
        if iters > STR_ITERS:
            print("str kinds stress", tag, "%.2f s" % (time.perf_counter() - t0), flush=True)
    print("string sweep: semi / anti joins with collisions %d, ordered outer joins with a mixed run %d" %
          (ambiguous_round, mixed_sort), flush=True)
    if default:
        assert ambiguous_round > 0, "no semi / anti join met a collision: the ambiguous-rows round never ran"
        assert mixed_sort > 0, "no ordered outer join sorted a run with keys of both relations"
    ex.release_result()


# ---------------------------------------------------------------------------------------------
def _i64(x):
    return int(x) & M64


def torch_anchor(torch, bd, pd):
    """n, sum_r, sum_s of the inner join and the matched-row counts of both sides, from torch's unique / searchsorted /
    index_add on the device (64-bit sums wrap as the library's do): nothing of the library is involved."""
    kb, vb, kp, vp = (c.contiguous() for c in (bd[:, 0], bd[:, 1], pd[:, 0], pd[:, 1]))
    ub, inv, cb = torch.unique(kb, return_inverse=True, return_counts=True)
    sb = torch.zeros(len(ub), dtype=torch.int64, device=kb.device).index_add_(0, inv, vb)
    idx = torch.searchsorted(ub, kp).clamp(max=len(ub) - 1)
    hit = ub[idx] == kp
    up, cp = torch.unique(kp, return_counts=True)
    bhit = up[torch.searchsorted(up, kb).clamp(max=len(up) - 1)] == kb
    j = torch.searchsorted(up, ub).clamp(max=len(up) - 1)
    both = up[j] == ub
    return {"n_matches": int(cb[idx][hit].sum()), "sum_r": _i64(sb[idx][hit].sum()), "sum_s": _i64((vp[hit] * cb[idx][hit]).sum()),
            "n_probe_matched": int(hit.sum()), "n_build_matched": int(bhit.sum()), "sum_probe_all": _i64(vp.sum()),
            "hottest": int((cb[both] * cp[j][both]).max())}  # one key's build copies x probe rows, the largest


def kind_identities(ex, H, bd, pd, tag):
    import torch

    nb, npb = bd.shape[0], pd.shape[0]
    fl = H.HMJ_CHECKSUM | H.HMJ_SUM_PROBE
    anchor = torch_anchor(torch, bd, pd)
    # kind joins cut no build slices: one work item walks a hot build key's row list for each of its probe rows
    assert anchor["hottest"] < 1 << 26, (tag, anchor)
    inner = ex.join_device(bd, pd, fl).checks()
    assert {k: inner[k] for k in ("n_matches", "sum_r", "sum_s")} == {k: anchor[k] for k in ("n_matches", "sum_r", "sum_s")}, tag
    res, cnt = {}, {}
    for name, kind in (("SEMI", H.HMJ_JOIN_SEMI), ("ANTI", H.HMJ_JOIN_ANTI), ("PROBE_OUTER", H.HMJ_JOIN_PROBE_OUTER)):
        r, cnt[name] = ex.join_kind_device(bd, pd, kind, fl)
        res[name] = dict(r.checks(), sum_probe_all=int(r.sum_probe_all))
    for name, kind in (("BUILD_SEMI", H.HMJ_BUILD_SEMI), ("BUILD_ANTI", H.HMJ_BUILD_ANTI), ("BUILD_OUTER", H.HMJ_BUILD_OUTER),
                       ("FULL_OUTER", H.HMJ_FULL_OUTER)):
        r, cnt[name] = ex.join_build_kind_device(bd, pd, kind, fl)
        res[name] = dict(r.checks(), sum_probe_all=int(r.sum_probe_all))

    def add(*names):
        parts = [inner if n == "INNER" else res[n] for n in names]
        out = {k: sum(p[k] for p in parts) & M64 for k in ("n_matches", "sum_r", "sum_s", "mix_sum")}
        out["xor_fold"] = 0
        for p in parts:
            out["xor_fold"] ^= p["xor_fold"]
        return out

    def five(name):
        return {k: res[name][k] for k in ("n_matches", "sum_r", "sum_s", "mix_sum", "xor_fold")}

    pm, bm = anchor["n_probe_matched"], anchor["n_build_matched"]
    for name in res:
        assert res[name]["sum_probe_all"] == anchor["sum_probe_all"], (tag, name)
    assert res["SEMI"]["n_matches"] == pm and res["ANTI"]["n_matches"] == npb - pm, tag
    assert (res["SEMI"]["sum_s"] + res["ANTI"]["sum_s"]) & M64 == anchor["sum_probe_all"], tag
    assert res["SEMI"]["sum_r"] == res["ANTI"]["sum_r"] == 0, tag
    assert five("PROBE_OUTER") == add("INNER", "ANTI"), tag
    assert res["BUILD_SEMI"]["n_matches"] == bm and res["BUILD_ANTI"]["n_matches"] == nb - bm, tag
    assert (res["BUILD_SEMI"]["sum_r"] + res["BUILD_ANTI"]["sum_r"]) & M64 == _i64(bd[:, 1].sum()), tag
    assert res["BUILD_SEMI"]["sum_s"] == res["BUILD_ANTI"]["sum_s"] == 0, tag
    assert five("BUILD_OUTER") == add("INNER", "BUILD_ANTI"), tag
    assert five("FULL_OUTER") == add("INNER", "ANTI", "BUILD_ANTI"), tag
    probe_cnt = {"n_probe_matched": pm, "n_probe_unmatched": npb - pm}
    build_cnt = {"n_build_matched": bm, "n_build_unmatched": nb - bm}
    for name in ("SEMI", "ANTI", "PROBE_OUTER"):
        assert cnt[name] == probe_cnt, (tag, name, cnt[name])
    for name in ("BUILD_SEMI", "BUILD_ANTI", "BUILD_OUTER"):
        assert cnt[name] == dict(build_cnt, n_probe_matched=0, n_probe_unmatched=0), (tag, name, cnt[name])
    assert cnt["FULL_OUTER"] == dict(build_cnt, **probe_cnt), (tag, cnt["FULL_OUTER"])
    assert 0 < pm < npb and 0 < bm < nb, (tag, pm, bm)  # both anti joins have rows: the identities are not vacuous
    print("kind identities", tag, "hottest key: copies x probe rows =", anchor["hottest"], flush=True)


@pytest.mark.parametrize("n", [(1 << 22) + 5, 1 << 24])
def test_kind_identities_with_duplicates_on_both_sides(ex, H, n):
    # about 4 x 4 rows per key (domain n / 4, both sides uniform over it, Poisson(4) copies): no key has more than a few
    # dozen rows on a side, so copies x probe rows of one key stays below 2^10 (kind_identities asserts < 2^26)
    from test_join_build_kinds_cpu import FULL, expect_build_kind

    bd = ex.gen_uniform_domain(n, n // 4, zseed=0x7654321)
    pd = ex.gen_uniform_domain(n, n // 4, zseed=0x1357911)
    kind_identities(ex, H, bd, pd, ("uniform", n))
    if n < 1 << 24:
        B, P = (t.cpu().numpy().view(np.uint64).reshape(-1, 2) for t in (bd, pd))
        rows, ck, counters = expect_build_kind(B, P, FULL, build_fill=21, probe_fill=22)
        r, cnt = ex.join_build_kind_device(bd, pd, FULL, H.HMJ_ORDERED | H.HMJ_CHECKSUM, build_fill=21, probe_fill=22)
        assert r.checks() == ck and cnt == counters
        assert np.array_equal(ex.columns_to_numpy(r, host=False), rows)
    del bd, pd
    ex.release_result()


def test_kind_identities_with_a_skewed_build_side(ex, H):
    # Zipf(0.9) build keys over 2^20 values under uniform probe keys over the same values: sum k^-0.9 over 2^20 values is
    # about 30.6, so the hottest build key has about 137 000 copies (3.3 % of 2^22 + 5 rows), and a key has 4 probe rows on
    # average (a dozen or so at most): copies x probe rows of one key is about 2^21, far below the 2^26 allowed
    import torch

    from test_gpu_join import _zipf_thresholds

    n, dom = (1 << 22) + 5, 1 << 20
    thr_d = torch.from_numpy(_zipf_thresholds(dom).view(np.int64).copy()).cuda()
    bd = ex.gen_from_cdf(n, thr_d)
    pd = ex.gen_uniform_domain(n, dom, zseed=0x1357911)
    kind_identities(ex, H, bd, pd, ("zipf", n))
    del bd, pd
    ex.release_result()
