"""GPU checks of NULL keys in the string-key joins (validity bitmaps on hmj_join_kind_str_device, and on
Executor.join_str_device, which routes to its INNER kind) against `expected_null_str_kind_rows` of
test_join_str_nulls_cpu.py: sizes and bit offsets around the wave and workgroup edges, key bytes under NULL slots that
would match (zero-length NULL slots next to a valid b"" included), sliced relations, relations without a chars buffer,
waves on the unstaged path, the calls that must equal a call without bitmaps, forced hash collisions on compacted inputs,
sides that are all NULL or empty, more NULL-key rows than a collision run may hold, several scan blocks against numpy, a
seeded sweep, and the argument errors."""
import ctypes as C
import os
import random

import numpy as np
import pytest

from test_join_str_cpu import M64, str_hash
from test_join_str_gpu import brute, decimal_keys, rel
from test_join_str_kinds_cpu import (ALL_KINDS, ANTI, BUILD, BUILD_ANTI, BUILD_OUTER, BUILD_SEMI, FULL_OUTER, INNER, NO_ROW, PROBE,
                                     PROBE_OUTER, SEMI, tmix_checks)
from test_join_str_nulls_cpu import COUNT_KEYS, COUNTS_PROBE, expected_null_str_kind_rows

pytestmark = pytest.mark.gpu
HMJ_E_ARG = -1
PFILL, BFILL = 0xF1, 2 ** 64 - 2
SEMI_ANTI = [(PROBE, SEMI), (PROBE, ANTI), (BUILD, BUILD_SEMI), (BUILD, BUILD_ANTI)]
SIZES = [1, 63, 64, 65, 255, 256, 257, 1000]
OFFSETS = [0, 1, 7, 13, 63]


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


def modes3(H):
    """ordered, materialising and count modes"""
    return (H.HMJ_ORDERED | H.HMJ_CHECKSUM | H.HMJ_SUM_PROBE, H.HMJ_MATERIALIZE | H.HMJ_CHECKSUM, H.HMJ_CHECKSUM | H.HMJ_SUM_PROBE)


def dev_valid(H, mask, off=0):
    """What build_valid / probe_valid take: None, or (bitmap on the device, bit offset).  mask: True = valid."""
    return None if mask is None else (H.pack_validity(mask, off, "cuda"), off)


def nulls_of(mask, n):
    return np.zeros(n, bool) if mask is None else ~np.asarray(mask, bool)


def rep_pairs(ok, kk, bits):
    """(n_hash_pairs, n_collisions) of a semi / anti kind as the header describes how it runs, over the rows that have a
    key: every row of the side asked about (kk) whose hash exists on the other side (ok) is compared with the FIRST row of
    that hash there, in row order; a row whose key differs from it is then compared with every row of its hash."""
    by = {}
    for k in ok:
        by.setdefault(str_hash(k, bits), []).append(k)
    pairs = diff = 0
    for k in kk:
        same = by.get(str_hash(k, bits))
        if same is None:
            continue
        pairs += 1
        if same[0] != k:
            diff += 1 + sum(1 for o in same if o != k)
            pairs += len(same)
    return pairs, diff


def expect_all(bk, bv, pk, pv, bnull, pnull, bits=0, kinds=ALL_KINDS):
    """The expectation of every kind, computed once: kind -> (rows, counts, checks, pairs of equal hash, of those with
    different keys) -- the pairs the kind compares: the inner join's for INNER and the outer kinds, `rep_pairs` for semi / anti."""
    as_b = lambda k: k.encode() if isinstance(k, str) else bytes(k)
    vb, vp = np.flatnonzero(~bnull), np.flatnonzero(~pnull)
    kb, kp = [as_b(bk[r]) for r in vb], [as_b(pk[s]) for s in vp]
    coll = brute(kb, [bv[r] for r in vb], kp, [pv[s] for s in vp], bits)[1]
    out = {}
    for side, kind in kinds:
        want, counts = expected_null_str_kind_rows(bk, bv, pk, pv, side, kind, bnull, pnull, bits, PFILL, BFILL)
        if (side, kind) in SEMI_ANTI:
            pairs, diff = rep_pairs(kp, kb, bits) if side == BUILD else rep_pairs(kb, kp, bits)
        else:
            pairs, diff = int(((want[:, 1] != NO_ROW) & (want[:, 2] != NO_ROW)).sum()) + coll, coll
        out[(side, kind)] = (want, counts, tmix_checks(want), pairs, diff)
    return out


def call(H, ex, B, P, VB, VP, side, kind, flags, bits=0, entry="kind"):
    """(result, info, rows): through the kind entry, or -- INNER only -- through Executor.join_str_device."""
    if entry == "inner":
        res, info = ex.join_str_device(B, P, flags, hash_bits=bits, build_valid=VB, probe_valid=VP)
        info = dict(info, **dict.fromkeys(COUNT_KEYS, 0))
    else:
        res, info = ex.join_kind_str_device(B, P, side, kind, flags, hash_bits=bits, probe_fill=PFILL, build_fill=BFILL, build_valid=VB,
                                            probe_valid=VP)
    rows = ex.str_kind_rows_to_numpy(res) if flags & (H.HMJ_MATERIALIZE | H.HMJ_ORDERED) else None
    return res, info, rows


def check(H, ex, B, P, VB, VP, expect, pv, bnull, pnull, modes, bits=0, tag=()):
    """Every kind of `expect` in `modes` against its expectation: counts, sums, checksums, the probe sum, the kind's
    counters, the NULL-key rows per side, hash pairs and collisions; rows exactly when ordered, as sorted multisets
    otherwise.  INNER also through the inner entry."""
    sum_p = sum(int(v) for v in pv) & M64
    for (side, kind), (want, counts, ck, pairs, diff) in expect.items():
        for entry in ("kind", "inner") if (side, kind) == (PROBE, INNER) else ("kind",):
            for flags in modes:
                t = tag + (side, kind, entry, flags, bits)
                res, info, got = call(H, ex, B, P, VB, VP, side, kind, flags, bits, entry)
                got_ck = res.checks()
                if flags & H.HMJ_CHECKSUM:
                    assert got_ck == ck, (t, got_ck, ck)
                else:
                    assert [got_ck[k] for k in ("n_matches", "sum_r", "sum_s")] == [ck[k] for k in ("n_matches", "sum_r", "sum_s")], t
                if flags & H.HMJ_SUM_PROBE:
                    assert int(res.sum_probe_all) == sum_p, t  # every probe row, NULL-key rows included
                assert {k: info[k] for k in COUNT_KEYS} == counts, (t, info, counts)
                assert (info["n_build_null"], info["n_probe_null"]) == (int(bnull.sum()), int(pnull.sum())), (t, info)
                assert (info["n_hash_pairs"], info["n_collisions"]) == (pairs, diff), (t, info, pairs, diff)
                if got is None:
                    assert not res.hash, t
                    continue
                assert got.shape == want.shape, (t, got.shape, want.shape)
                if flags & H.HMJ_ORDERED:
                    assert np.array_equal(got, want), (t, np.flatnonzero(np.any(got != want, axis=1))[:5])
                else:
                    assert np.array_equal(unordered(got), unordered(want)), t


def draw_pool(rng, n_pool, max_len=12):
    """Distinct keys, b"" among them."""
    keys = {b""}
    while len(keys) < n_pool:
        keys.add(bytes(rng.randrange(256) for _ in range(rng.randrange(max_len + 1))))
    keys = sorted(keys)
    rng.shuffle(keys)
    return keys


def drawn(rng, nb, np_, n_pool=None, max_len=12):
    """Keys with duplicates and misses on both sides: build rows from the first two thirds of a pool, probe rows from the
    last two thirds; b"" sits in the shared third."""
    n_pool = n_pool or max(6, (nb + np_) // 3)
    pool = draw_pool(rng, n_pool, max_len)
    third = n_pool // 3
    e = pool.index(b"")
    pool[e], pool[third] = pool[third], pool[e]
    bk = [pool[rng.randrange(2 * third)] for _ in range(nb)]
    pk = [pool[third + rng.randrange(n_pool - third)] for _ in range(np_)]
    return bk, pk


def payloads(rng, n):
    return [rng.getrandbits(64) for _ in range(n)]


# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["build", "probe", "both"])
def test_sizes_and_offsets(H, ex, which):
    """Every size on each side (a single row, one short of / exactly / one past a wave and a workgroup, several workgroups)
    crossed with bit offsets inside a byte, across a byte and one short of a 64-bit word; about 30 % NULL-key rows; bitmaps
    on one side only and on both."""
    rng = random.Random(len(which))
    nrng = np.random.default_rng(len(which))
    for i, nb in enumerate(SIZES):
        np_ = SIZES[(i + 3) % len(SIZES)]
        bk, pk = drawn(rng, nb, np_)
        bv, pv = payloads(rng, nb), payloads(rng, np_)
        mb = nrng.random(nb) >= 0.3 if which != "probe" else None
        mp = nrng.random(np_) >= 0.3 if which != "build" else None
        bnull, pnull = nulls_of(mb, nb), nulls_of(mp, np_)
        expect = expect_all(bk, bv, pk, pv, bnull, pnull)
        B, P = rel(H, bk, bv), rel(H, pk, pv)
        for off in OFFSETS:
            check(H, ex, B, P, dev_valid(H, mb, off), dev_valid(H, mp, (off * 5 + 3) % 64 if off else 0), expect, pv, bnull, pnull,
                  modes3(H), tag=(nb, np_, off))
    assert which == "probe" or bnull.sum() > 200  # (the last pair: 1000 x 65)


def test_bytes_under_null_slots(H, ex):
    """Two copies of the same relations that differ only in what lies under the NULL slots.  In one copy the NULL slots of
    each side hold keys that are present and valid on the other side (matches, were they read), every fifth of them with
    length 0 while a valid b"" exists on both sides; in the other they hold random bytes.  Same results, none of those
    matches."""
    rng = random.Random(11)
    nrng = np.random.default_rng(11)
    nb, np_ = 500, 700
    bk, pk = drawn(rng, nb, np_)
    bnull, pnull = nrng.random(nb) < 0.3, nrng.random(np_) < 0.3
    bk[5], pk[7] = b"", b""
    bnull[5] = pnull[7] = False  # a valid empty string on both sides
    live_b = [k for k, z in zip(bk, bnull) if not z]
    live_p = [k for k, z in zip(pk, pnull) if not z]
    bv, pv = payloads(rng, nb), payloads(rng, np_)
    results = []
    for copy in ("matching", "random"):
        def under(i, live_other):
            if copy == "random":
                return bytes(rng.randrange(256) for _ in range(rng.randrange(20)))
            return b"" if i % 5 == 0 else rng.choice(live_other)
        bk2 = [under(i, live_p) if z else k for i, (k, z) in enumerate(zip(bk, bnull))]
        pk2 = [under(i, live_b) if z else k for i, (k, z) in enumerate(zip(pk, pnull))]
        expect = expect_all(bk2, bv, pk2, pv, bnull, pnull)
        if copy == "matching":  # the would-be matches exist in the bytes
            n_plain = len(expected_null_str_kind_rows(bk2, bv, pk2, pv, PROBE, INNER)[0])
            assert n_plain > len(expect[(PROBE, INNER)][0]) + 100
            assert sum(1 for k, z in zip(bk2, bnull) if z and k == b"") > 10 and sum(1 for k, z in zip(pk2, pnull) if z and k == b"") > 10
        B, P = rel(H, bk2, bv), rel(H, pk2, pv)
        check(H, ex, B, P, dev_valid(H, ~bnull, 5), dev_valid(H, ~pnull, 9), expect, pv, bnull, pnull, modes3(H), tag=(copy,))
        results.append({k: v[0] for k, v in expect.items()})
    for k in results[0]:  # the two copies' expectations -- which the device met -- are the same rows
        assert np.array_equal(results[0][k], results[1][k]), k
    inner = results[0][(PROBE, INNER)]
    e = str_hash(b"")
    assert len(inner[inner[:, 0] == e]) == sum(1 for k in live_b if k == b"") * sum(1 for k in live_p if k == b"") > 0


def test_sliced_relations(H, ex):
    """offsets[0] != 0 and chars that start at odd addresses, with bitmaps at their own slice offsets."""
    rng = random.Random(12)
    nrng = np.random.default_rng(12)
    nb, np_ = 300, 421
    bk, pk = drawn(rng, nb, np_, max_len=40)
    bv, pv = payloads(rng, nb), payloads(rng, np_)
    mb, mp = nrng.random(nb) >= 0.3, nrng.random(np_) >= 0.3
    bnull, pnull = ~mb, ~mp
    expect = expect_all(bk, bv, pk, pv, bnull, pnull)
    for shift, base in ((3, 11), (1, 4097), (7, 1)):
        B, P = rel(H, bk, bv, shift, base), rel(H, pk, pv, 8 - shift, base // 2)
        check(H, ex, B, P, dev_valid(H, mb, base % 64), dev_valid(H, mp, shift), expect, pv, bnull, pnull, modes3(H), tag=(shift, base))


def test_no_chars_buffer(H, ex):
    """chars = None: every key, valid or NULL, has length 0.  The valid empty strings match each other; the NULL slots
    match nothing."""
    import torch

    nrng = np.random.default_rng(13)
    nb, np_ = 130, 70
    bv, pv = list(range(100, 100 + nb)), list(range(7, 7 + np_))
    mb, mp = nrng.random(nb) >= 0.4, nrng.random(np_) >= 0.4
    bnull, pnull = ~mb, ~mp
    expect = expect_all([b""] * nb, bv, [b""] * np_, pv, bnull, pnull)
    assert len(expect[(PROBE, INNER)][0]) == int(mb.sum()) * int(mp.sum()) > 0
    B = (None, torch.zeros(nb + 1, dtype=torch.int64, device="cuda"), torch.tensor(bv, dtype=torch.int64, device="cuda"))
    P = (None, torch.full((np_ + 1,), 9, dtype=torch.int64, device="cuda"), torch.tensor(pv, dtype=torch.int64, device="cuda"))
    check(H, ex, B, P, dev_valid(H, mb, 2), dev_valid(H, mp, 0), expect, pv, bnull, pnull, modes3(H))
    check(H, ex, B, P, None, dev_valid(H, mp, 9), expect_all([b""] * nb, bv, [b""] * np_, pv, np.zeros(nb, bool), pnull), pv,
          np.zeros(nb, bool), pnull, modes3(H))


def test_long_keys(H, ex):
    """Keys of about 100 bytes: a wave's 64 of them span more than the 4096 bytes a wave stages in LDS, so those waves read
    their keys from global memory; the waves between them hold short keys and stage.  NULL rows sit in both."""
    rng = random.Random(14)
    nrng = np.random.default_rng(14)

    def keys(n, lo):
        out = []
        for i in range(n):
            long_wave = ((i // 64) % 2) == 1
            k = (lo + rng.randrange(400)) % 600
            out.append((b"L%03d" % k) * 20 + b"x" * (k % 7) if long_wave else b"s%d" % k)
        return out

    nb, np_ = 450, 333
    bk, pk = keys(nb, 0), keys(np_, 200)
    assert sum(len(k) for k in bk[64:128]) > 4096 + 32 and sum(len(k) for k in bk[:64]) < 2048
    bv, pv = payloads(rng, nb), payloads(rng, np_)
    mb, mp = nrng.random(nb) >= 0.3, nrng.random(np_) >= 0.3
    bnull, pnull = ~mb, ~mp
    assert bnull[:64].any() and bnull[64:128].any() and pnull[64:128].any() and pnull[128:192].any()
    expect = expect_all(bk, bv, pk, pv, bnull, pnull)
    assert len(expect[(PROBE, INNER)][0]) > 20
    B, P = rel(H, bk, bv, 1, 5), rel(H, pk, pv)
    check(H, ex, B, P, dev_valid(H, mb, 13), dev_valid(H, mp, 0), expect, pv, bnull, pnull, modes3(H))


def _no_ms(info):
    return {k: v for k, v in info.items() if not k.startswith("ms_")}


def test_calls_that_equal_a_call_without_bitmaps(H, ex):
    """No bitmap passed, bits == NULL on both sides, all-valid bitmaps and a struct_size cut to the size the struct had
    before it grew (garbage behind it): the same fields and the same rows."""
    import torch

    rng = random.Random(21)
    nb, np_ = 700, 1100
    bk, pk = drawn(rng, nb, np_)
    bv, pv = payloads(rng, nb), payloads(rng, np_)
    B, P = rel(H, bk, bv, 3, 2), rel(H, pk, pv)
    nobits = (torch.empty(0, dtype=torch.uint8, device="cuda"), 5)  # (an empty tensor: bits == NULL, the offset ignored)
    VB, VP = dev_valid(H, np.ones(nb, bool), 3), dev_valid(H, np.ones(np_, bool), 0)
    rb, rp = ex._str_rel(B), ex._str_rel(P)
    old = H.StrKindOpts.build_validity.offset
    assert old == 104
    for side, kind in ALL_KINDS:
        for flags in modes3(H):
            a, ia, ra = call(H, ex, B, P, None, None, side, kind, flags)
            ca, sa = a.checks(), int(a.sum_probe_all)
            assert ca["n_matches"] > 0
            for vb, vp in ((nobits, nobits), (VB, VP), (VB, None), (None, VP), (nobits, VP)):
                for entry in ("kind", "inner") if (side, kind) == (PROBE, INNER) else ("kind",):
                    b, ib, rows = call(H, ex, B, P, vb, vp, side, kind, flags, entry=entry)
                    t = (side, kind, entry, flags)
                    assert b.checks() == ca and int(b.sum_probe_all) == sa, t
                    assert _no_ms(ib) == _no_ms(ia) and (ib["n_build_null"], ib["n_probe_null"]) == (0, 0), t
                    if flags & H.HMJ_ORDERED:
                        assert np.array_equal(ra, rows), t
                    elif ra is not None:
                        assert np.array_equal(unordered(ra), unordered(rows)), t
            # raw ctypes: the old struct size, poison where the new fields lie
            o = H.StrKindOpts()
            o.struct_size, o.side, o.kind, o.probe_fill, o.build_fill = old, side, kind, PFILL, BFILL
            o.build_validity.bits, o.build_validity.bit_offset = 0xDEAD0001, 2 ** 64 - 1
            o.probe_validity.bits, o.probe_validity.bit_offset = 0xDEAD0003, 77
            o.n_build_null, o.n_probe_null = 777, 888
            res = H.StrResult()
            ex._sync_stream()
            assert ex.L.hmj_join_kind_str_device(ex.h, C.byref(rb), C.byref(rp), flags, C.byref(o), C.byref(res)) == 0
            assert res.checks() == ca and int(res.sum_probe_all) == sa and o.struct_size == old
            assert (o.build_validity.bits, o.build_validity.bit_offset, o.probe_validity.bits, o.probe_validity.bit_offset,
                    o.n_build_null, o.n_probe_null) == (0xDEAD0001, 2 ** 64 - 1, 0xDEAD0003, 77, 777, 888)
            assert {k: int(getattr(o.counts, k)) for k in COUNT_KEYS} == {k: ia[k] for k in COUNT_KEYS}
            assert (int(o.n_hash_pairs), int(o.n_collisions)) == (ia["n_hash_pairs"], ia["n_collisions"])
            if ra is not None:
                rows = ex.str_kind_rows_to_numpy(res)
                assert np.array_equal(ra, rows) if flags & H.HMJ_ORDERED else np.array_equal(unordered(ra), unordered(rows))
    # a full-size struct: the in fields come back as they were, the out fields are written
    o = H.StrKindOpts()
    o.struct_size, o.side, o.kind = C.sizeof(H.StrKindOpts), PROBE, ANTI
    o.n_build_null, o.n_probe_null = 777, 888
    bits = H.pack_validity(np.arange(np_) % 3 != 0, 2, "cuda")
    o.probe_validity.bits, o.probe_validity.bit_offset = bits.data_ptr(), 2
    res = H.StrResult()
    ex._sync_stream()
    assert ex.L.hmj_join_kind_str_device(ex.h, C.byref(rb), C.byref(rp), 0, C.byref(o), C.byref(res)) == 0
    assert (o.n_build_null, o.n_probe_null) == (0, (np_ + 2) // 3)
    assert (o.probe_validity.bits, o.probe_validity.bit_offset, o.build_validity.bits) == (bits.data_ptr(), 2, None)
    want, _ = expected_null_str_kind_rows(bk, bv, pk, pv, PROBE, ANTI, None, np.arange(np_) % 3 == 0)
    assert int(res.n_matches) == len(want)


@pytest.mark.parametrize("bits", [2, 4])
def test_forced_collisions(H, ex, bits):
    """4 or 16 hash values: semi / anti go through the ambiguous re-join with compacted rows, and every ordered run of equal
    hash mixes keys -- the collision sort must see the rows that have a key only."""
    rng = random.Random(400 + bits)
    nrng = np.random.default_rng(400 + bits)
    nb, np_ = 150 * bits, 200 * bits
    bk, pk = drawn(rng, nb, np_, n_pool=2 * nb)
    bv, pv = payloads(rng, nb), payloads(rng, np_)
    mb, mp = nrng.random(nb) >= 0.25, nrng.random(np_) >= 0.25
    bnull, pnull = ~mb, ~mp
    expect = expect_all(bk, bv, pk, pv, bnull, pnull, bits)
    full = expect[(BUILD, FULL_OUTER)][0]
    head = full[:len(full) - int(bnull.sum()) - int(pnull.sum())]
    run = np.bincount(head[:, 0].astype(np.int64))
    assert expect[(PROBE, INNER)][4] > 1000 and int(head[:, 0].max()) < (1 << bits) and 1 < run.max() <= 1024, run.max()
    assert all(expect[k][4] > 0 for k in SEMI_ANTI) and run[0] > 0 and len(expect[(PROBE, INNER)][0]) > 20  # (rows with a key whose hash folds to 0, the NULL rows' hash)
    B, P = rel(H, bk, bv), rel(H, pk, pv, 5, 3)
    VB, VP = dev_valid(H, mb, 13), dev_valid(H, mp, 7)
    check(H, ex, B, P, VB, VP, expect, pv, bnull, pnull, modes3(H), bits=bits)
    for side, kind in SEMI_ANTI:
        _, info, _ = call(H, ex, B, P, VB, VP, side, kind, 0, bits)
        assert info["n_collisions"] > 0, (side, kind)


def test_all_null_and_empty_sides(H, ex):
    import torch

    rng = random.Random(31)
    nb, np_ = 300, 420
    bk, pk = drawn(rng, nb, np_)
    bv, pv = payloads(rng, nb), payloads(rng, np_)
    B, P = rel(H, bk, bv), rel(H, pk, pv)
    some_b, some_p = np.arange(nb) % 4 != 1, np.arange(np_) % 5 != 2
    none_b, none_p = np.zeros(nb, bool), np.zeros(np_, bool)
    quick = (H.HMJ_ORDERED | H.HMJ_CHECKSUM | H.HMJ_SUM_PROBE, H.HMJ_MATERIALIZE, H.HMJ_CHECKSUM)
    for name, mb, mp in (("build all NULL", none_b, some_p), ("probe all NULL", some_b, none_p), ("both all NULL", none_b, none_p),
                         ("all NULL against no bitmap", none_b, None), ("no bitmap against all NULL", None, none_p)):
        bnull, pnull = nulls_of(mb, nb), nulls_of(mp, np_)
        expect = expect_all(bk, bv, pk, pv, bnull, pnull)
        assert len(expect[(PROBE, INNER)][0]) == 0 and len(expect[(BUILD, FULL_OUTER)][0]) == nb + np_
        check(H, ex, B, P, dev_valid(H, mb, 6), dev_valid(H, mp, 1), expect, pv, bnull, pnull, quick, tag=(name,))
    # n = 0 on a side (with a bitmap pointer for it), the other side all NULL, partly NULL or without a bitmap
    spare = torch.full((8,), 0x5A, dtype=torch.uint8, device="cuda")
    E = rel(H, [], [])
    for eb, ep in ((True, False), (False, True), (True, True)):
        for other in ("all", "some", None):
            kb, kp = ([] if eb else bk), ([] if ep else pk)
            bvv, pvv = ([] if eb else bv), ([] if ep else pv)
            mb = None if eb or other is None else (none_b if other == "all" else some_b)
            mp = None if ep or other is None else (none_p if other == "all" else some_p)
            VB = (spare, 3) if eb else dev_valid(H, mb, 0)
            VP = (spare, 0) if ep else dev_valid(H, mp, 0)
            bnull, pnull = nulls_of(mb, len(kb)), nulls_of(mp, len(kp))
            expect = expect_all(kb, bvv, kp, pvv, bnull, pnull)
            check(H, ex, E if eb else B, E if ep else P, VB, VP, expect, pvv, bnull, pnull, quick, tag=("empty", eb, ep, other))


def test_null_rows_do_not_count_towards_the_run_limit(H, ex):
    """2 hash bits: every run of equal hash mixes keys, and the rows with a key stay below the 1024 rows a collision run may
    hold while each side has more than 1024 NULL-key rows.  Were the NULL-key rows (hash 0) part of the sorted rows, the
    run of hash 0 would exceed the limit; the calls return HMJ_OK and the expectation's rows."""
    rng = random.Random(51)
    nb, np_ = 1500, 1700
    bk, pk = drawn(rng, nb, np_, n_pool=900)
    bv, pv = payloads(rng, nb), payloads(rng, np_)
    mb, mp = np.zeros(nb, bool), np.zeros(np_, bool)
    mb[rng.sample(range(nb), 200)] = True
    mp[rng.sample(range(np_), 260)] = True
    bnull, pnull = ~mb, ~mp
    assert bnull.sum() > 1024 and pnull.sum() > 1024
    expect = expect_all(bk, bv, pk, pv, bnull, pnull, 2)
    full = expect[(BUILD, FULL_OUTER)][0]
    head = full[:len(full) - int(bnull.sum()) - int(pnull.sum())]
    run = np.bincount(head[:, 0].astype(np.int64), minlength=4)
    assert run[0] > 0 and run.max() <= 1024 and run[0] + bnull.sum() > 1024 and expect[(PROBE, INNER)][4] > 0
    B, P = rel(H, bk, bv), rel(H, pk, pv)
    check(H, ex, B, P, dev_valid(H, mb, 1), dev_valid(H, mp, 63), expect, pv, bnull, pnull,
          (H.HMJ_ORDERED | H.HMJ_CHECKSUM | H.HMJ_SUM_PROBE, H.HMJ_CHECKSUM), bits=2)


def test_several_scan_blocks_against_numpy(H, ex):
    """131 075 x 262 145 rows of keys "k<id>", 10 % NULL-key rows: 513 and 1025 workgroups of valid-row counts go through
    launch_scan_u64, whose single workgroup gives each of its 16 waves a chunk of whole 64-entry tiles (here 64 and 128
    entries: several tiles, several waves, a last chunk that is cut short).  Counts and sums from numpy for every kind;
    the ordered FULL_OUTER rows on a strided sample plus the whole NULL tail."""
    import torch

    nb, np_ = (1 << 17) + 3, (1 << 18) + 1
    rng = np.random.default_rng(77)
    ids_b, ids_p = rng.integers(0, 90000, nb), rng.integers(30000, 120000, np_)
    cb, ob = decimal_keys(0, 120000)

    def side_of(ids, vals):
        lo, lens = ob[ids], ob[ids + 1] - ob[ids]
        offs = np.zeros(len(ids) + 1, np.int64)
        np.cumsum(lens, out=offs[1:])
        idx = np.repeat(lo - offs[:-1], lens) + np.arange(offs[-1])
        return torch.from_numpy(cb[idx]).cuda(), torch.from_numpy(offs).cuda(), torch.from_numpy(vals.view(np.int64)).cuda()

    bv = rng.integers(0, 1 << 40, nb, dtype=np.uint64)
    pv = rng.integers(0, 1 << 40, np_, dtype=np.uint64)
    mb, mp = rng.random(nb) >= 0.1, rng.random(np_) >= 0.1
    bnull, pnull = ~mb, ~mp
    # (the ids under the NULL slots are ids of the other side's range: matches, were they read)
    ids_b[bnull] = ids_p[:int(bnull.sum())]
    ids_p[pnull] = ids_b[mb][:int(pnull.sum())]
    B, P = side_of(ids_b, bv), side_of(ids_p, pv)
    vb, vp = np.flatnonzero(mb), np.flatnonzero(mp)
    cnt_b = np.bincount(ids_b[vb], minlength=120000)
    cnt_p = np.bincount(ids_p[vp], minlength=120000)
    sb, sp = np.zeros(120000, np.uint64), np.zeros(120000, np.uint64)
    np.add.at(sb, ids_b[vb], bv[vb])
    np.add.at(sp, ids_p[vp], pv[vp])
    m = lambda x: int(x) & M64
    n_in = int((cnt_b * cnt_p).sum())
    in_r = m(sum(int(x) for x in sb * cnt_p.astype(np.uint64)))
    in_s = m(sum(int(x) for x in sp * cnt_b.astype(np.uint64)))
    p_hit, b_hit = np.zeros(np_, bool), np.zeros(nb, bool)
    p_hit[vp] = cnt_b[ids_p[vp]] > 0
    b_hit[vb] = cnt_p[ids_b[vb]] > 0
    assert n_in > 100000 and p_hit.sum() > 50000 and (~b_hit).sum() > 30000
    sum_at = lambda v, sel: m(v[sel].sum(dtype=np.uint64))
    n_pu, n_bu = int((~p_hit).sum()), int((~b_hit).sum())
    want = {
        (PROBE, INNER): (n_in, in_r, in_s),
        (PROBE, SEMI): (int(p_hit.sum()), 0, sum_at(pv, p_hit)),
        (PROBE, ANTI): (n_pu, 0, sum_at(pv, ~p_hit)),
        (PROBE, PROBE_OUTER): (n_in + n_pu, m(in_r + PFILL * n_pu), m(in_s + sum_at(pv, ~p_hit))),
        (BUILD, BUILD_SEMI): (int(b_hit.sum()), sum_at(bv, b_hit), 0),
        (BUILD, BUILD_ANTI): (n_bu, sum_at(bv, ~b_hit), 0),
        (BUILD, BUILD_OUTER): (n_in + n_bu, m(in_r + sum_at(bv, ~b_hit)), m(in_s + BFILL * n_bu)),
        (BUILD, FULL_OUTER): (n_in + n_pu + n_bu, m(in_r + PFILL * n_pu + sum_at(bv, ~b_hit)), m(in_s + sum_at(pv, ~p_hit) + BFILL * n_bu)),
    }
    VB, VP = dev_valid(H, mb, 5), dev_valid(H, mp, 63)
    for (side, kind), (n, sr, ss) in want.items():
        res, info, _ = call(H, ex, B, P, VB, VP, side, kind, H.HMJ_SUM_PROBE)
        assert (int(res.n_matches), int(res.sum_r), int(res.sum_s)) == (n, sr, ss), (side, kind)
        assert int(res.sum_probe_all) == sum_at(pv, slice(None)) and info["n_collisions"] == 0
        assert (info["n_build_null"], info["n_probe_null"]) == (int(bnull.sum()), int(pnull.sum()))
        if (side, kind) in COUNTS_PROBE:
            assert (info["n_probe_matched"], info["n_probe_unmatched"]) == (int(p_hit.sum()), n_pu)
        if side == BUILD:
            assert (info["n_build_matched"], info["n_build_unmatched"]) == (int(b_hit.sum()), n_bu)
        if (side, kind) not in SEMI_ANTI:
            assert info["n_hash_pairs"] == n_in
    # ordered FULL_OUTER.  The hashes of the 120 000 keys: the device's std::hash (hmj_hash_str_device, pinned against the
    # host's in test_join_str_gpu.py), spot-checked here; distinct, so (hash, r_row, s_row) is the whole order
    hk = ex.hash_str_device(torch.from_numpy(cb).cuda(), torch.from_numpy(ob).cuda()).cpu().numpy().view(np.uint64)
    for i in (0, 9, 10, 99999, 119999):
        assert int(hk[i]) == str_hash(b"k%d" % i)
    assert len(np.unique(hk)) == len(hk)
    order_p = vp[np.argsort(ids_p[vp], kind="stable")]  # probe rows with a key, by id then s_row
    start_p = np.concatenate([[0], np.cumsum(cnt_p)])
    reps = cnt_p[ids_b[vb]]
    pr = np.repeat(vb, reps)  # r_row of every pair
    within = np.arange(len(pr)) - np.repeat(np.cumsum(reps) - reps, reps)
    ps = order_p[start_p[ids_b[pr]] + within]
    NR = np.uint64(NO_ROW)
    ub, up = np.flatnonzero(mb & ~b_hit), np.flatnonzero(mp & ~p_hit)
    rows = np.concatenate([
        np.stack([hk[ids_b[pr]], pr.astype(np.uint64), ps.astype(np.uint64), bv[pr], pv[ps]], 1),
        np.stack([hk[ids_b[ub]], ub.astype(np.uint64), np.full(len(ub), NR), bv[ub], np.full(len(ub), BFILL, np.uint64)], 1),
        np.stack([hk[ids_p[up]], np.full(len(up), NR), up.astype(np.uint64), np.full(len(up), PFILL, np.uint64), pv[up]], 1)])
    rows = rows[np.lexsort((rows[:, 2], rows[:, 1], rows[:, 0]))]
    nbn, npn = np.flatnonzero(bnull), np.flatnonzero(pnull)
    tail = np.concatenate([
        np.stack([np.zeros(len(nbn), np.uint64), nbn.astype(np.uint64), np.full(len(nbn), NR), bv[nbn], np.full(len(nbn), BFILL, np.uint64)], 1),
        np.stack([np.zeros(len(npn), np.uint64), np.full(len(npn), NR), npn.astype(np.uint64), np.full(len(npn), PFILL, np.uint64), pv[npn]], 1)])
    res, info, got = call(H, ex, B, P, VB, VP, BUILD, FULL_OUTER, H.HMJ_ORDERED)
    assert len(got) == len(rows) + len(tail) == want[(BUILD, FULL_OUTER)][0]
    assert np.array_equal(got[:len(rows)][::97], rows[::97]) and np.array_equal(got[len(rows) - 50:len(rows)], rows[-50:])
    assert np.array_equal(got[len(rows):], tail)


def test_seeded_sweep(H, ex):
    """HMJ_STRESS_SEED / HMJ_STRESS_ITERS (default 20) drawn cases: sizes up to 2000, key pools with duplicates, a NULL
    fraction between 0 and 1 per side (0 and 1 included), bit offsets, hash_bits, and three (kind, mode) pairs each.  With few
    hash bits every run of equal hash mixes keys, so those cases stay at 30 rows per side: at most 30 * 30 + 60 result rows
    whatever the duplicates, below the 1024 a collision run may hold -- no drawn case is skipped."""
    seed = int(os.environ.get("HMJ_STRESS_SEED", "2024"))
    iters = int(os.environ.get("HMJ_STRESS_ITERS", "20"))
    rng = random.Random(seed)
    for it in range(iters):
        bits = rng.choice([0, 0, 24, 4, 6])
        cap = 30 if 0 < bits < 24 else 2000
        nb, np_ = rng.randrange(0, cap + 1), rng.randrange(0, cap + 1)
        n_pool = rng.randrange(40, max(41, (nb + np_) // 2 + 2))
        bk, pk = drawn(rng, nb, np_, n_pool=n_pool, max_len=rng.choice([4, 12, 90]))
        bv, pv = payloads(rng, nb), payloads(rng, np_)
        nrng = np.random.default_rng(rng.getrandbits(32))
        masks = []
        for n in (nb, np_):
            frac = rng.choice([0.0, 1.0, rng.random(), rng.random(), None])
            masks.append(None if frac is None else nrng.random(n) >= frac)
        mb, mp = masks
        bnull, pnull = nulls_of(mb, nb), nulls_of(mp, np_)
        kinds = rng.sample(ALL_KINDS, 3)
        expect = expect_all(bk, bv, pk, pv, bnull, pnull, bits, kinds)
        B, P = rel(H, bk, bv, rng.randrange(8), rng.randrange(100)), rel(H, pk, pv, rng.randrange(8), rng.randrange(100))
        VB, VP = dev_valid(H, mb, rng.randrange(64)), dev_valid(H, mp, rng.choice([0, 1, 8, 63, 1000]))
        for k in kinds:
            check(H, ex, B, P, VB, VP, {k: expect[k]}, pv, bnull, pnull, (rng.choice(modes3(H)),), bits=bits, tag=(seed, it, nb, np_))


def test_errors_leave_the_ctx_usable(H, ex):
    """bit_offset + n overflowing 64 bits, and offsets that decrease under a NULL slot, are HMJ_E_ARG; after each a plain
    string join and a nullable one on the same ctx give correct results."""
    import torch

    bk, bv = ["aa", "bb", "cc", "dd"], [1, 2, 3, 4]
    pk, pv = ["bb", "zz", "aa"], [5, 6, 7]
    B, P = rel(H, bk, bv), rel(H, pk, pv)
    chars, offs, vals = B
    bits = torch.full((64,), 0xFF, dtype=torch.uint8, device="cuda")
    mb = np.array([True, False, True, True])
    VB = dev_valid(H, mb, 3)

    def good():
        res, _ = ex.join_str_device(B, P, H.HMJ_ORDERED)
        assert ex.str_rows_to_numpy(res).tolist() == brute(bk, bv, pk, pv)[0].tolist()
        res, info = ex.join_kind_str_device(B, P, BUILD, FULL_OUTER, H.HMJ_ORDERED, probe_fill=PFILL, build_fill=BFILL, build_valid=VB)
        want, counts = expected_null_str_kind_rows(bk, bv, pk, pv, BUILD, FULL_OUTER, ~mb, None, 0, PFILL, BFILL)
        assert np.array_equal(ex.str_kind_rows_to_numpy(res), want) and {k: info[k] for k in COUNT_KEYS} == counts
        assert (info["n_build_null"], info["n_probe_null"]) == (1, 0)

    good()
    for off in (2 ** 64 - 1, 2 ** 64 - 4, 2 ** 64 - 3):
        for kw in (dict(build_valid=(bits, off)), dict(probe_valid=(bits, off))):
            n = 4 if "build_valid" in kw else 3
            if off + n < 2 ** 64:
                continue  # (the largest offsets that do not overflow are not argument errors as such)
            with pytest.raises(H.HmjError) as e:
                ex.join_str_device(B, P, 0, **kw)
            assert e.value.code == HMJ_E_ARG and "bit_offset" in str(e.value), (off, kw)
            good()
            with pytest.raises(H.HmjError) as e:
                ex.join_kind_str_device(B, P, BUILD, FULL_OUTER, H.HMJ_ORDERED, **kw)
            assert e.value.code == HMJ_E_ARG
            good()
    # an entry without bits ignores its offset
    res, info = ex.join_str_device(B, P, 0, probe_valid=(bits[:0], 2 ** 64 - 1), build_valid=(bits, 8))
    assert int(res.n_matches) == 2 and (info["n_build_null"], info["n_probe_null"]) == (0, 0)
    # offsets that decrease under a NULL slot: 0 2 4 1 8 decreases at row 2, which is NULL
    bad = offs.clone()
    bad[3] = 1
    null2 = dev_valid(H, np.array([True, True, False, True]), 1)
    for fn in (lambda: ex.join_kind_str_device((chars, bad, vals), P, BUILD, FULL_OUTER, H.HMJ_ORDERED, build_valid=null2),
               lambda: ex.join_kind_str_device(P, (chars, bad, vals), PROBE, ANTI, 0, probe_valid=null2),
               lambda: ex.join_str_device((chars, bad, vals), P, 0, build_valid=null2, probe_valid=dev_valid(H, np.ones(3, bool)))):
        with pytest.raises(H.HmjError) as e:
            fn()
        assert e.value.code == HMJ_E_ARG and "row 2" in str(e.value), str(e.value)
        good()
    # Python-side checks of the keywords
    with pytest.raises(ValueError):
        ex.join_str_device(B, P, 0, build_valid=(bits.cpu(), 0))
    with pytest.raises(ValueError):
        ex.join_kind_str_device(B, P, PROBE, SEMI, 0, probe_valid=(bits, -1))
    good()


@pytest.mark.parametrize("side,kind", [(PROBE, INNER), (BUILD, FULL_OUTER)])
def test_bad_offsets_under_a_bitmap_then_the_right_ones(H, ex, side, kind):
    """600 rows a side, a bitmap on the probe relation, its offsets decreasing at row 70: the second wave of the first
    workgroup compacts nothing, so the two workgroups behind it compact in front of their places, into an array that has
    room for every row.  Materialising, the call fails with HMJ_E_ARG naming the relation and the row; the same call with
    the offsets put right, on the same context, is the brute force's."""
    rng = random.Random(8070)
    n = 600
    bk, pk = drawn(rng, n, n)
    bv, pv = payloads(rng, n), payloads(rng, n)
    B, P = rel(H, bk, bv), rel(H, pk, pv)
    mp = np.random.default_rng(8070).random(n) >= 0.3
    mp[70] = True
    assert mp[256:].sum() > 64
    VP = dev_valid(H, mp, 3)
    chars, offs, vals = P
    bad = offs.clone()
    bad[70] = bad[71] + 3  # offsets[71] < offsets[70]
    flags = H.HMJ_MATERIALIZE | H.HMJ_CHECKSUM | H.HMJ_SUM_PROBE
    with pytest.raises(H.HmjError) as e:
        ex.join_kind_str_device(B, (chars, bad, vals), side, kind, flags, probe_fill=PFILL, build_fill=BFILL, probe_valid=VP)
    assert e.value.code == HMJ_E_ARG, str(e.value)
    assert "probe relation: offsets decrease at row 70 (offsets[71] < offsets[70])" in str(e.value), str(e.value)
    bnull, pnull = np.zeros(n, bool), ~mp
    expect = expect_all(bk, bv, pk, pv, bnull, pnull, kinds=[(side, kind)])
    check(H, ex, B, P, None, VP, expect, pv, bnull, pnull, (flags,), tag=("offsets put right",))


def test_inner_entry_routes_to_the_inner_kind(H, ex):
    rng = random.Random(8)
    nrng = np.random.default_rng(8)
    nb, np_ = 400, 500
    bk, pk = drawn(rng, nb, np_)
    bv, pv = payloads(rng, nb), payloads(rng, np_)
    B, P = rel(H, bk, bv), rel(H, pk, pv)
    mb, mp = nrng.random(nb) >= 0.3, nrng.random(np_) >= 0.2
    for bits in (0, 6):
        for vb, vp in ((dev_valid(H, mb, 9), dev_valid(H, mp, 2)), (None, dev_valid(H, mp, 2)), (dev_valid(H, mb, 9), None)):
            for flags in modes3(H):
                a, ia, ra = call(H, ex, B, P, vb, vp, PROBE, INNER, flags, bits, "inner")
                b, ib, rb = call(H, ex, B, P, vb, vp, PROBE, INNER, flags, bits, "kind")
                assert a.checks() == b.checks() and int(a.sum_probe_all) == int(b.sum_probe_all)
                assert set(ia) - set(COUNT_KEYS) == {"n_hash_pairs", "n_collisions", "n_build_null", "n_probe_null", "ms_hash", "ms_join",
                                                      "ms_verify", "ms_order"}
                assert all(ia[k] == ib[k] for k in ("n_hash_pairs", "n_collisions", "n_build_null", "n_probe_null"))
                assert ia["n_build_null"] == (0 if vb is None else int((~mb).sum())) and ia["n_probe_null"] == (0 if vp is None else int((~mp).sum()))
                if flags & H.HMJ_ORDERED:
                    assert np.array_equal(ra, rb) and len(ra) > 0
                elif ra is not None:
                    assert np.array_equal(unordered(ra), unordered(rb))
    # without the keywords the inner entry is hmj_join_str_device itself and reports no NULLs
    res, info = ex.join_str_device(B, P, 0)
    assert (info["n_build_null"], info["n_probe_null"]) == (0, 0)
