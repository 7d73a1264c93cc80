"""GPU checks of the string-key join kinds (hmj_join_kind_str_device) against the pure-Python brute force of
test_join_str_kinds_cpu.py: every kind in the count, materialising and ordered modes on duplicates and misses, forced hash
collisions (a representative whose key differs while another row of its hash matches), the duplicate bound of semi / anti,
the inner kind against hmj_join_str_device, the reference's string relations, edge keys, empty sides, errors and the
planner's isolation of the kinds' workloads."""
import ctypes as C
import json
import os
import random

import numpy as np
import pytest

from test_join_str_cpu import M64, str_hash
from test_join_str_gpu import _dup_relations, decimal_keys, rel
from test_join_str_kinds_cpu import (ALL_KINDS, ANTI, BUILD, BUILD_ANTI, BUILD_OUTER, BUILD_SEMI, FULL_OUTER, INNER, NO_ROW,
                                     PROBE, PROBE_OUTER, SEMI, kind_brute, tmix_checks)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HMJ_E_ARG = -1
PFILL, BFILL = 0x1111222233334444, 0xAAAA0000BBBB0001


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


def unordered(rows):
    return rows[np.lexsort(rows.T[::-1])] if len(rows) else rows


def modes(H):
    return (0, H.HMJ_MATERIALIZE | H.HMJ_CHECKSUM, H.HMJ_ORDERED | H.HMJ_CHECKSUM | H.HMJ_SUM_PROBE)


def check_kind(H, ex, B, P, bk, bv, pk, pv, side, kind, flags, bits=0, pfill=PFILL, bfill=BFILL):
    """One kind join against the brute force: rows (sorted unless ordered), sums, checksums, counters, absent columns."""
    want, counts = kind_brute(bk, bv, pk, pv, side, kind, bits, pfill, bfill)
    res, info = ex.join_kind_str_device(B, P, side, kind, flags, hash_bits=bits, probe_fill=pfill, build_fill=bfill)
    ck = tmix_checks(want)
    got_ck = res.checks()
    tag = (side, kind, flags, bits)
    if flags & H.HMJ_CHECKSUM:
        assert got_ck == ck, tag
    else:
        assert (got_ck["n_matches"], got_ck["sum_r"], got_ck["sum_s"]) == (ck["n_matches"], ck["sum_r"], ck["sum_s"]), tag
    if flags & H.HMJ_SUM_PROBE:
        assert int(res.sum_probe_all) == sum(pv) & M64, tag
    if kind != INNER or side != PROBE:
        assert {k: info[k] for k in counts} == counts, (tag, info, counts)
    if flags & (H.HMJ_MATERIALIZE | H.HMJ_ORDERED):
        got = ex.str_kind_rows_to_numpy(res)
        if flags & H.HMJ_ORDERED:
            assert np.array_equal(got, want), tag
        else:
            assert np.array_equal(unordered(got), unordered(want)), tag
        if len(want):
            semi_anti = kind in (SEMI, ANTI)
            assert bool(res.r_row) == bool(res.rval) == (not semi_anti or side == BUILD), tag
            assert bool(res.s_row) == bool(res.sval) == (not semi_anti or side == PROBE), tag
    else:
        assert not res.hash, tag
    return res, info


# ---------------------------------------------------------------------------------------------
def test_every_kind_on_duplicates_and_misses(H, ex):
    rng = random.Random(21)
    bk, bv, pk, pv = _dup_relations(rng, 300)
    B, P = rel(H, bk, bv, 3, 11), rel(H, pk, pv, 5, 0)
    for side, kind in ALL_KINDS:
        for flags in modes(H):
            _, info = check_kind(H, ex, B, P, bk, bv, pk, pv, side, kind, flags)
            assert info["n_collisions"] == 0


def _same_hash_keys(bits, count):
    """`count` different keys whose top `bits` hash bits agree."""
    by = {}
    i = 0
    while True:
        k = b"c%d" % i
        h = str_hash(k, bits)
        by.setdefault(h, []).append(k)
        if len(by[h]) == count:
            return by[h]
        i += 1


@pytest.mark.parametrize("bits", [6, 8, 12])
def test_forced_collisions(H, ex, bits):
    # a representative whose key differs: build [kA, kB] and probe [kC, kB] share one hash.  Probe row 1 meets kA first
    # and must still find kB; build row 1 meets kC first and must still find kB.
    kA, kB, kC = _same_hash_keys(bits, 3)
    bk, bv, pk, pv = [kA, kB], [5, 6], [kC, kB], [7, 8]
    B, P = rel(H, bk, bv), rel(H, pk, pv)
    res, info = ex.join_kind_str_device(B, P, PROBE, SEMI, H.HMJ_ORDERED, hash_bits=bits)
    assert ex.str_kind_rows_to_numpy(res).tolist() == [[str_hash(kB, bits), NO_ROW, 1, 0, 8]]
    assert info["n_collisions"] > 0 and info["n_probe_matched"] == 1
    res, info = ex.join_kind_str_device(B, P, BUILD, BUILD_SEMI, H.HMJ_ORDERED, hash_bits=bits)
    assert ex.str_kind_rows_to_numpy(res).tolist() == [[str_hash(kB, bits), 1, NO_ROW, 6, 0]]
    assert info["n_collisions"] > 0 and info["n_build_matched"] == 1
    for side, kind in ALL_KINDS:
        check_kind(H, ex, B, P, bk, bv, pk, pv, side, kind, H.HMJ_ORDERED | H.HMJ_CHECKSUM, bits)
    # random relations: many keys per hash value, every kind and mode
    rng = random.Random(bits)
    bk, bv, pk, pv = _dup_relations(rng, {6: 60, 8: 150, 12: 400}[bits], 12)
    B, P = rel(H, bk, bv, 1, 0), rel(H, pk, pv, 0, 4)
    for side, kind in ALL_KINDS:
        for flags in modes(H):
            _, info = check_kind(H, ex, B, P, bk, bv, pk, pv, side, kind, flags, bits)
            assert info["n_collisions"] > 0, (side, kind, flags)


def test_semi_anti_never_form_the_cross_product(H, ex):
    """64 keys x 2000 copies on each side: the inner join has 2.56e8 pairs; semi / anti compare one pair per row."""
    import torch

    n_keys, copies = 64, 2000
    rng = np.random.default_rng(3)
    kb = rng.permutation(np.repeat(np.arange(n_keys), copies))
    kp = rng.permutation(np.repeat(np.arange(n_keys) + n_keys // 2, copies))  # half the probe keys are missing
    cb, ob = decimal_keys(0, 2 * n_keys)

    def side_of(k):
        lo, hi = ob[k], ob[k + 1]
        lens = hi - lo
        offs = np.zeros(len(k) + 1, np.int64)
        np.cumsum(lens, out=offs[1:])
        idx = np.repeat(lo - offs[:-1], lens) + np.arange(offs[-1])
        return (torch.from_numpy(cb[idx]).cuda(), torch.from_numpy(offs).cuda(),
                torch.arange(len(k), dtype=torch.int64, device="cuda"))

    B, P = side_of(kb), side_of(kp)
    n = n_keys * copies
    for side, kind, rows, hit in ((PROBE, SEMI, 2, kp < n_keys), (PROBE, ANTI, 2, kp >= n_keys),
                                  (BUILD, BUILD_SEMI, 1, kb >= n_keys // 2), (BUILD, BUILD_ANTI, 1, kb < n_keys // 2)):
        for flags in (0, H.HMJ_MATERIALIZE):
            res, info = ex.join_kind_str_device(B, P, side, kind, flags)
            assert int(res.n_matches) == int(hit.sum()) == n // 2
            assert info["n_hash_pairs"] <= n and info["n_collisions"] == 0, info
            if flags:
                got = ex.str_kind_rows_to_numpy(res)
                assert np.array_equal(np.sort(got[:, rows]), np.flatnonzero(hit).astype(np.uint64))


def test_inner_kind_is_the_inner_string_join(H, ex):
    rng = random.Random(8)
    bk, bv, pk, pv = _dup_relations(rng, 200)
    B, P = rel(H, bk, bv), rel(H, pk, pv)
    for bits in (0, 8):
        for flags in modes(H):
            a, ia = ex.join_str_device(B, P, flags, hash_bits=bits)
            ra = ex.str_rows_to_numpy(a) if flags else None
            b, ib = ex.join_kind_str_device(B, P, PROBE, INNER, flags, hash_bits=bits)
            assert b.checks() == a.checks() and int(b.sum_probe_all) == int(a.sum_probe_all)
            assert (ib["n_hash_pairs"], ib["n_collisions"]) == (ia["n_hash_pairs"], ia["n_collisions"])
            assert [ib[k] for k in ("n_probe_matched", "n_probe_unmatched", "n_build_matched", "n_build_unmatched")] == [0] * 4
            if flags & H.HMJ_ORDERED:
                assert np.array_equal(ex.str_rows_to_numpy(b), ra)
            elif flags:  # (unordered: row order is unspecified, also between two inner string joins)
                assert np.array_equal(unordered(ex.str_rows_to_numpy(b)), unordered(ra))


def test_reference_relations(H, ex):
    from oracle.pyoracle import create_strvec

    with open(os.path.join(ROOT, "tests", "golden", "golden.json")) as f:
        G = json.load(f)["cases"]
    txt = open(os.path.join(ROOT, "tests", "golden", "words.txt")).read().split("\n")
    words = txt[:-1] if txt and txt[-1] == "" else txt
    seen = set()
    for c in G["strgen_join"]:
        n = c["n"]
        if n > 262144:
            continue
        seen.add(n)
        r, s = create_strvec(n, words, c["seed_r"]), create_strvec(n, words, c["seed_s"])
        bk, bv, pk, pv = [k for k, _ in r], [v for _, v in r], [k for k, _ in s], [v for _, v in s]
        B, P = rel(H, bk, bv), rel(H, pk, pv)
        assert c["count"] == n  # (the same key set on both sides)
        res, info = ex.join_kind_str_device(B, P, PROBE, SEMI, 0)
        assert int(res.n_matches) == n and int(res.sum_s) == sum(pv) & M64 and info["n_probe_matched"] == n
        res, info = ex.join_kind_str_device(B, P, PROBE, ANTI, H.HMJ_MATERIALIZE)
        assert int(res.n_matches) == 0 and info["n_probe_unmatched"] == 0
        res, info = ex.join_kind_str_device(B, P, BUILD, BUILD_SEMI, H.HMJ_ORDERED)
        assert int(res.n_matches) == n and info["n_build_matched"] == n
        got = ex.str_kind_rows_to_numpy(res)
        assert np.array_equal(np.sort(got[:, 1]), np.arange(n, dtype=np.uint64))
        assert np.all(np.diff(got[:, 0].astype(np.float64)) >= 0)
        for side, kind in ((PROBE, PROBE_OUTER), (BUILD, BUILD_OUTER), (BUILD, FULL_OUTER)):
            for flags in (0, H.HMJ_ORDERED):
                res, info = ex.join_kind_str_device(B, P, side, kind, flags, probe_fill=PFILL, build_fill=BFILL)
                assert (int(res.n_matches), (int(res.sum_r) + int(res.sum_s)) & M64) == (c["count"], c["sum"]), (n, side, kind)
                assert info["n_probe_unmatched"] == info["n_build_unmatched"] == 0
        # half-disjoint: every second probe key changed (a miss) -> counters and sums against the brute force
        if n <= 65536:
            pk2 = [k if i % 2 else k + "#" for i, k in enumerate(pk)]
            P2 = rel(H, pk2, pv)
            for side, kind in ALL_KINDS[1:]:
                check_kind(H, ex, B, P2, bk, bv, pk2, pv, side, kind, H.HMJ_CHECKSUM)
            check_kind(H, ex, B, P2, bk, bv, pk2, pv, BUILD, FULL_OUTER, H.HMJ_ORDERED | H.HMJ_CHECKSUM)
    assert seen == {2, 1000, 4096, 65536, 262144}


def test_edge_keys(H, ex):
    rng = random.Random(9)
    lengths = [0, 1, 7, 8, 9, 63, 64, 65, 255, 256, 257, 4096]
    hit = [bytes(rng.randrange(256) for _ in range(n)) for n in lengths]
    miss = [k[:-1] + bytes([(k[-1] + 1) & 0xFF]) for k in hit if k]
    small = [b"s%d" % i for i in range(200)] + [b"n\x00ul", b"\x80\xff", b""]
    bk = small + hit + small[:50] + [b"only-build\x00"]
    pk = miss + hit[::-1] + small[::3] + [b"x" * 4096] * 3 + [b""] * 2
    bv = list(range(100, 100 + len(bk)))
    pv = list(range(7, 7 + len(pk)))
    for shift in (0, 1, 7):
        B, P = rel(H, bk, bv, shift, 3), rel(H, pk, pv, 8 - shift, 0)
        for side, kind in ALL_KINDS:
            check_kind(H, ex, B, P, bk, bv, pk, pv, side, kind, H.HMJ_ORDERED | H.HMJ_CHECKSUM)


def test_empty_sides(H, ex):
    import torch

    A = (["a", "b", "c", "b"], [1, 2, 3, 4])
    E = ([], [])
    for (bk, bv), (pk, pv) in ((A, E), (E, A), (E, E)):
        B, P = rel(H, bk, bv), rel(H, pk, pv)
        for side, kind in ALL_KINDS:
            for flags in (0, H.HMJ_ORDERED | H.HMJ_CHECKSUM):
                check_kind(H, ex, B, P, bk, bv, pk, pv, side, kind, flags)
    # every key empty: chars may be NULL
    off_b = torch.zeros(6, dtype=torch.int64, device="cuda")
    off_p = torch.full((4,), 9, dtype=torch.int64, device="cuda")
    vb = torch.arange(5, dtype=torch.int64, device="cuda")
    vp = torch.arange(10, 13, dtype=torch.int64, device="cuda")
    for side, kind in ALL_KINDS:
        want, _ = kind_brute([b""] * 5, list(range(5)), [b""] * 3, [10, 11, 12], side, kind, 0, PFILL, BFILL)
        res, _ = ex.join_kind_str_device((None, off_b, vb), (None, off_p, vp), side, kind, H.HMJ_ORDERED, probe_fill=PFILL,
                                         build_fill=BFILL)
        assert np.array_equal(ex.str_kind_rows_to_numpy(res), want), (side, kind)


def test_errors_leave_the_ctx_usable(H, ex):
    B = rel(H, ["aa", "bb", "cc", "dd"], [1, 2, 3, 4])
    P = rel(H, ["bb", "zz"], [5, 6])
    chars, offs, vals = B

    def good():
        res, info = ex.join_kind_str_device(B, P, PROBE, SEMI, H.HMJ_ORDERED)
        assert ex.str_kind_rows_to_numpy(res).tolist() == [[str_hash(b"bb"), NO_ROW, 0, 0, 5]]
        assert info["n_probe_matched"] == 1

    bad = offs.clone()
    bad[3] = 1  # offsets 0 2 4 1 8: decrease at row 2
    calls = [lambda: ex.join_kind_str_device(B, P, PROBE, SEMI, H.HMJ_FIRST_WINS),
             lambda: ex.join_kind_str_device(B, P, BUILD, BUILD_OUTER, H.HMJ_FIRST_WINS | H.HMJ_ORDERED),
             lambda: ex.join_kind_str_device(B, P, 2, SEMI, 0),
             lambda: ex.join_kind_str_device(B, P, PROBE, 4, 0),
             lambda: ex.join_kind_str_device(B, P, BUILD, 0, 0),
             lambda: ex.join_kind_str_device(B, P, BUILD, 5, 0),
             lambda: ex.join_kind_str_device(B, P, PROBE, SEMI, 0, hash_bits=64),
             lambda: ex.join_kind_str_device((chars, bad, vals), P, BUILD, FULL_OUTER, H.HMJ_ORDERED),
             lambda: ex.join_kind_str_device(P, (chars, bad, vals), PROBE, ANTI, 0)]
    for call in calls:
        with pytest.raises(H.HmjError) as e:
            call()
        assert e.value.code == HMJ_E_ARG
        good()
    # a struct_size that does not reach the fill values
    rb, rp = ex._str_rel(B), ex._str_rel(P)
    res = H.StrResult()
    for size in (0, 8, 16, 31):  # (the fills end at byte 32)
        opts = H.StrKindOpts()
        opts.struct_size = size
        opts.kind = SEMI
        ex._sync_stream()
        assert ex.L.hmj_join_kind_str_device(ex.h, C.byref(rb), C.byref(rp), 0, C.byref(opts), C.byref(res)) == HMJ_E_ARG
        good()
    # NULL opts / out
    opts = H.StrKindOpts()
    opts.struct_size = C.sizeof(H.StrKindOpts)
    assert ex.L.hmj_join_kind_str_device(ex.h, C.byref(rb), C.byref(rp), 0, None, C.byref(res)) == HMJ_E_ARG
    assert ex.L.hmj_join_kind_str_device(ex.h, C.byref(rb), C.byref(rp), 0, C.byref(opts), None) == HMJ_E_ARG
    good()


def test_string_kinds_do_not_change_u64_plans(H):
    """String kind joins with duplicate keys teach their workloads a cool-down; a u64 inner join and a u64 SEMI kind join of
    the same sizes must still plan exactly as on a fresh ctx, and the kinds' workloads carry kind codes 10..14."""
    import torch

    n = 1 << 20
    cb, ob = decimal_keys(0, n // 2)
    chars = torch.from_numpy(np.concatenate([cb, cb])).cuda()
    offs = torch.from_numpy(np.concatenate([ob[:-1], ob + ob[-1]])).cuda()
    S = (chars, offs, torch.arange(n, dtype=torch.int64, device="cuda"))
    fresh = H.Executor(0)
    B, P = fresh.gen_build(n), fresh.gen_probe(n, n, miss_mod=3)
    fresh.join_device(B, P, H.HMJ_MATERIALIZE | H.HMJ_CHECKSUM)
    p_inner = fresh.last_plan()
    r_semi, _ = fresh.join_kind_device(B, P, H.HMJ_JOIN_SEMI, H.HMJ_MATERIALIZE)
    p_semi = fresh.last_plan()
    n_semi = int(r_semi.n_matches)
    fresh.close()
    ex2 = H.Executor(0)
    learnt = 0
    for side, kind in ((PROBE, SEMI), (BUILD, BUILD_ANTI), (PROBE, PROBE_OUTER), (BUILD, FULL_OUTER)):
        for _ in range(3):
            res, info = ex2.join_kind_str_device(S, S, side, kind, H.HMJ_MATERIALIZE)
            assert int(res.n_matches) == (0 if kind == BUILD_ANTI else n if kind == SEMI else 2 * n)
        p = ex2.last_plan()
        assert 10 <= (p["workload"] >> 20) & 15 <= 14, p["workload"]
        learnt |= p["cooling"]
    ex2.join_device(B, P, H.HMJ_MATERIALIZE | H.HMJ_CHECKSUM)
    assert ex2.last_plan() == p_inner
    r2, _ = ex2.join_kind_device(B, P, H.HMJ_JOIN_SEMI, H.HMJ_MATERIALIZE)
    assert ex2.last_plan() == p_semi and int(r2.n_matches) == n_semi
    ex2.close()
    assert learnt, "the string kind joins taught their workloads nothing: the test would not see a shared memo"
