"""GPU checks of NULL keys in the multi-column joins (validity bitmaps on hmj_join_cols_device / hmj_join_kind_cols_device)
against `expected_null_kind_rows` of test_join_cols_nulls_cpu.py: sizes and bit offsets around the wave and workgroup
edges in both forms, value bytes under NULL slots that would match, the calls that must equal a call without bitmaps, sides
that are all NULL or empty, forced key64 collisions with compacted inputs, several scan blocks against numpy, the argument
error, and what a ctx does after a nullable call."""
import ctypes as C
import os
import random

import numpy as np
import pytest

from test_join_cols_gpu import columns, draw_pool, unordered
from test_join_cols_kinds_cpu import (ALL_KINDS, ANTI, BUILD, BUILD_ANTI, BUILD_OUTER, BUILD_SEMI, COUNT_KEYS, FULL_OUTER, INNER, M64,
                                      NO_ROW, PROBE, PROBE_OUTER, SEMI, key_collisions, kind_checks)
from test_join_cols_kinds_gpu import dev_rel
from test_join_cols_nulls_cpu import COUNTS_PROBE, EMITS_BUILD_NULLS, EMITS_PROBE_NULLS, expected_null_kind_rows

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


def modes3(H):
    """ordered, materialising and count modes"""
    return (H.HMJ_ORDERED | H.HMJ_CHECKSUM | H.HMJ_SUM_PROBE, H.HMJ_MATERIALIZE | H.HMJ_CHECKSUM, H.HMJ_CHECKSUM | H.HMJ_SUM_PROBE)


def draw_masks(rng, n, k, which, frac):
    """Validity per key column (True = valid; None: the column has no bitmap) with about `frac` of the rows NULL-keyed.
    which "one": a bitmap on column 1 only; "all": one per column, drawn independently (different columns NULL in one row),
    row 1 NULL in columns 0 and 1."""
    if which == "one":
        return [None, rng.random(n) >= frac] + [None] * (k - 2)
    per_col = 1.0 - (1.0 - frac) ** (1.0 / k)
    masks = [rng.random(n) >= per_col for _ in range(k)]
    if n > 1:
        masks[0][1] = masks[1][1] = False
    return masks


def null_rows(masks, n):
    out = np.zeros(n, bool)
    for m in masks or ():
        if m is not None:
            out |= ~m
    return out


def dev_valid(H, masks, off=0):
    """What build_valid / probe_valid take: per column None, or (bitmap on the device, bit offset)."""
    return None if masks is None else [None if m is None else (H.pack_validity(m, off, "cuda"), off) for m in masks]


def expect_all(bcols, bv, pcols, pv, widths, bnull, pnull, bits=0, force=False, kinds=ALL_KINDS):
    """The expectation of every kind, computed once: kind -> (rows, counts, checks, inner pairs, collisions)."""
    hashed = force or sum(widths) > 8
    vb, vp = np.flatnonzero(~bnull), np.flatnonzero(~pnull)
    coll = key_collisions([c[vb] for c in bcols], [c[vp] for c in pcols], widths, bits, force) if hashed else 0
    out = {}
    for side, kind in kinds:
        want, counts = expected_null_kind_rows(bcols, bv, pcols, pv, widths, side, kind, bnull, pnull, bits, force, PFILL, BFILL)
        inner = sum(1 for r in want if r[1] != NO_ROW and r[2] != NO_ROW) if (side, kind) not in SEMI_ANTI else None
        out[(side, kind)] = (want, counts, kind_checks(want), inner, coll)
    return out


def call(H, ex, B, P, VB, VP, side, kind, flags, bits=0, force=False, entry="kind"):
    """(result, info, rows): through the kind entry, or -- INNER only -- through hmj_join_cols_device."""
    if entry == "inner":
        res, info = ex.join_cols_device(B[0], B[1], P[0], P[1], flags, hash_bits=bits, force_hashed=force, build_valid=VB, probe_valid=VP)
        info = dict(info, **dict.fromkeys(COUNT_KEYS, 0))
    else:
        res, info = ex.join_kind_cols_device(B[0], B[1], P[0], P[1], side, kind, flags, hash_bits=bits, force_hashed=force,
                                             probe_fill=PFILL, build_fill=BFILL, build_valid=VB, probe_valid=VP)
    rows = ex.cols_kind_rows_to_numpy(res) if flags & (H.HMJ_MATERIALIZE | H.HMJ_ORDERED) else None
    return res, info, rows


def check(H, ex, B, P, VB, VP, expect, widths, pv, n_probe, bnull, pnull, modes, bits=0, force=False, tag=()):
    """Every kind of `expect` in `modes` against its expectation: counts, sums, checksums, the probe sum, the kind's
    counters, the NULL-key rows per side, form, key pairs and collisions; rows exactly when ordered, as sorted multisets
    otherwise.  INNER also through the inner entry."""
    hashed = force or sum(widths) > 8
    sum_p = (sum(int(v) for v in pv) if pv is not None else n_probe * (n_probe - 1) // 2) & M64
    for (side, kind), (want, counts, ck, inner, coll) in expect.items():
        for entry in ("kind", "inner") if (side, kind) == (PROBE, INNER) else ("kind",):
            for flags in modes:
                t = tag + (widths, side, kind, entry, flags)
                res, info, got = call(H, ex, B, P, VB, VP, side, kind, flags, bits, force, entry)
                got_ck = res.checks()
                print(t, got_ck, {k: info[k] for k in ("form", "n_key_pairs", "n_collisions", "n_build_null", "n_probe_null") + COUNT_KEYS})
                if flags & H.HMJ_CHECKSUM:
                    assert got_ck == ck, t
                else:
                    assert [got_ck[k] for k in ("n_matches", "sum_r", "sum_s")] == [ck[k] for k in ("n_matches", "sum_r", "sum_s")], t
                if flags & H.HMJ_SUM_PROBE:
                    assert int(res.sum_probe_all) == sum_p, t  # every probe row, NULL-key rows included
                assert {k: info[k] for k in COUNT_KEYS} == counts, (t, info, counts)
                assert (info["n_build_null"], info["n_probe_null"]) == (int(bnull.sum()), int(pnull.sum())), (t, info)
                if entry == "kind" or (len(bnull) and len(pnull)):
                    assert info["form"] == (H.HMJ_COLS_HASHED if hashed else H.HMJ_COLS_PACKED), t
                if inner is None:
                    assert info["n_collisions"] == 0 or coll > 0, t
                else:
                    assert (info["n_collisions"], info["n_key_pairs"]) == (coll, inner + coll), (t, info, coll, inner)
                if got is None:
                    assert not res.key64, t
                    continue
                assert got.shape == want.shape, (t, got.shape, want.shape)
                if flags & H.HMJ_ORDERED:
                    assert np.array_equal(got, want), (t, np.flatnonzero(np.any(got != want, axis=1))[:5])
                else:
                    assert np.array_equal(unordered(got), unordered(want)), t


def drawn(rng, widths, nb, np_, n_pool=None):
    """Tuples with duplicates and misses on both sides: build rows from the first two thirds of a pool, probe rows from
    the last two thirds."""
    n_pool = n_pool or min(450, max(6, (nb + np_) // 3))  # ([4,4]: draw_pool holds at most 23 * 23 tuples)
    pool = draw_pool(rng, widths, n_pool)
    rng.shuffle(pool)
    third = n_pool // 3
    bt = [pool[rng.randrange(2 * third)] for _ in range(nb)]
    pt = [pool[third + rng.randrange(n_pool - third)] for _ in range(np_)]
    return bt, pt


# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["one", "all"])
@pytest.mark.parametrize("widths", [[4, 4], [8, 4, 2]])
def test_boundaries(H, ex, widths, which):
    """Every size on each side (a single row, one short of / exactly / one past a wave and a workgroup, several workgroups)
    crossed with bit offsets inside a byte, across a byte and one short of a 64-bit word; about 30 % NULL-key rows."""
    rng = random.Random(sum(widths) + len(which))
    nrng = np.random.default_rng(sum(widths) + len(which))
    for i, nb in enumerate(SIZES):
        np_ = SIZES[(i + 3) % len(SIZES)]
        bt, pt = drawn(rng, widths, nb, np_)
        bcols, pcols = columns(bt, widths), columns(pt, widths)
        bv = [rng.getrandbits(64) for _ in range(nb)]
        mb, mp = draw_masks(nrng, nb, len(widths), which, 0.3), draw_masks(nrng, np_, len(widths), which, 0.3)
        bnull, pnull = null_rows(mb, nb), null_rows(mp, np_)
        expect = expect_all(bcols, bv, pcols, None, widths, bnull, pnull)
        B, P = dev_rel(bcols, bv), dev_rel(pcols, None)
        for off in OFFSETS:
            check(H, ex, B, P, dev_valid(H, mb, off), dev_valid(H, mp, (off * 5 + 3) % 64 if off else 0), expect, widths, None, np_,
                  bnull, pnull, modes3(H), tag=(nb, np_, off))
    assert bnull.sum() > 200 and pnull.sum() > 5  # (the last pair: 1000 x 65)


@pytest.mark.parametrize("widths", [[4, 4], [8, 4, 2]])
def test_garbage_under_null_slots(H, ex, widths):
    """Two copies of the same relations that differ only in the value bytes under NULL slots: in one copy those bytes spell
    tuples the other side holds (matches, were they read), in the other they are random.  Same results, none of those
    matches."""
    rng = random.Random(11 + len(widths))
    nrng = np.random.default_rng(11 + len(widths))
    nb, np_ = 500, 700
    bt, pt = drawn(rng, widths, nb, np_)
    mb, mp = draw_masks(nrng, nb, len(widths), "all", 0.3), draw_masks(nrng, np_, len(widths), "one", 0.3)
    bnull, pnull = null_rows(mb, nb), null_rows(mp, np_)
    live_b = [t for t, z in zip(bt, bnull) if not z]
    live_p = [t for t, z in zip(pt, pnull) if not z]
    bv, pv = [rng.getrandbits(64) for _ in bt], [rng.getrandbits(64) for _ in pt]
    results = []
    for copy in ("matching", "random"):
        def under(null, live_other):
            return rng.choice(live_other) if copy == "matching" else tuple(rng.getrandbits(8 * w) for w in widths)
        # a whole NULL-key row is rewritten, so a column that is valid in it changes too: the expectation below takes the
        # rewritten tuples, and never looks at a NULL-key row's
        bt2 = [under(z, live_p) if z else t for t, z in zip(bt, bnull)]
        pt2 = [under(z, live_b) if z else t for t, z in zip(pt, pnull)]
        bcols, pcols = columns(bt2, widths), columns(pt2, widths)
        expect = expect_all(bcols, bv, pcols, pv, widths, bnull, pnull)
        if copy == "matching":  # the would-be matches exist in the bytes
            assert len(expected_null_kind_rows(bcols, bv, pcols, pv, widths, PROBE, INNER)[0]) > len(expect[(PROBE, INNER)][0]) + 100
        B, P = dev_rel(bcols, bv), dev_rel(pcols, pv)
        VB, VP = dev_valid(H, mb, 5), dev_valid(H, mp, 9)
        check(H, ex, B, P, VB, VP, expect, widths, pv, np_, bnull, pnull, modes3(H), tag=(copy,))
        results.append({k: v[0] for k, v in expect.items()})
    for k in results[0]:  # the two copies' expectations -- which the device met -- are the same rows
        assert np.array_equal(results[0][k], results[1][k]), k
        rows = results[0][k]
        if k not in SEMI_ANTI and len(rows):
            pairs = rows[(rows[:, 1] != NO_ROW) & (rows[:, 2] != NO_ROW)]
            assert not bnull[pairs[:, 1].astype(np.int64)].any() and not pnull[pairs[:, 2].astype(np.int64)].any()


@pytest.mark.parametrize("widths", [[4, 4], [8, 4, 2]])
def test_all_valid_bitmaps_change_nothing(H, ex, widths):
    rng = random.Random(21 + len(widths))
    nb, np_ = 700, 1100
    bt, pt = drawn(rng, widths, nb, np_)
    bcols, pcols = columns(bt, widths), columns(pt, widths)
    bv = [rng.getrandbits(64) for _ in bt]
    B, P = dev_rel(bcols, bv), dev_rel(pcols, None)
    ones_b = [np.ones(nb, bool)] * len(widths)
    ones_p = [None, np.ones(np_, bool)] + [None] * (len(widths) - 2)
    VB, VP = dev_valid(H, ones_b, 3), dev_valid(H, ones_p, 0)
    for side, kind in ALL_KINDS:
        for entry in ("kind", "inner") if (side, kind) == (PROBE, INNER) else ("kind",):
            for flags in modes3(H):
                a, ia, ra = call(H, ex, B, P, None, None, side, kind, flags, entry=entry)
                ca, sa = a.checks(), int(a.sum_probe_all)
                for vb, vp in ((VB, VP), (VB, None), (None, VP), ([None] * len(widths), [None] * len(widths))):
                    b, ib, rb = call(H, ex, B, P, vb, vp, side, kind, flags, entry=entry)
                    t = (widths, side, kind, entry, flags, vb is None, vp is None)
                    assert b.checks() == ca and int(b.sum_probe_all) == sa and ca["n_matches"] > 0, t
                    assert {k: v for k, v in ib.items() if not k.startswith("ms_")} == {k: v for k, v in ia.items() if not k.startswith("ms_")}, t
                    assert (ib["n_build_null"], ib["n_probe_null"]) == (0, 0)
                    if flags & H.HMJ_ORDERED:
                        assert np.array_equal(ra, rb), t
                    elif ra is not None:
                        assert np.array_equal(unordered(ra), unordered(rb)), t


def test_old_struct_sizes_ignore_the_new_fields(H, ex):
    """struct_size of a caller built against the header without validity: garbage in the new fields is neither read nor
    overwritten, and the result is the call's without bitmaps."""
    import torch

    n = 300
    a = torch.arange(n, dtype=torch.int32, device="cuda")
    b = torch.arange(n, dtype=torch.int16, device="cuda")
    pa = torch.arange(100, 100 + n, dtype=torch.int32, device="cuda")
    pb = torch.arange(100, 100 + n, dtype=torch.int16, device="cuda")
    rb, kb = ex._cols_rel([a, b], None)
    rp, kp = ex._cols_rel([pa, pb], None)
    junk = C.cast(C.c_void_p(0xDEAD0001), C.POINTER(H.Validity))
    want_sum = sum(range(100, n)) + sum(range(0, n - 100))

    def poison(o):
        o.build_validity, o.probe_validity, o.n_build_null, o.n_probe_null = junk, junk, 777, 888

    def untouched(o):
        return (C.cast(o.build_validity, C.c_void_p).value, C.cast(o.probe_validity, C.c_void_p).value, o.n_build_null,
                o.n_probe_null) == (0xDEAD0001, 0xDEAD0001, 777, 888)

    for size in (12, 48):  # hmj_cols_join_opts has its old layout: its minimum and its whole size
        o = H.ColsJoinOpts()
        o.struct_size = size
        res = H.ColsResult()
        ex._sync_stream()
        assert ex.L.hmj_join_cols_device(ex.h, C.byref(rb), C.byref(rp), 0, C.byref(o), C.byref(res)) == 0, size
        assert int(res.n_matches) == n - 100 and int(res.sum_r) + int(res.sum_s) == want_sum and o.struct_size == size
        assert (o.form, o.n_key_pairs) == ((H.HMJ_COLS_PACKED, n - 100) if size >= 48 else (0, 0))
    for size in (40, 112, 120):  # the old minimum, the old struct, half of the in fields
        for side, kind, rows in ((PROBE, INNER, n - 100), (PROBE, ANTI, 100), (BUILD, FULL_OUTER, n + 100)):
            o = H.ColsKindOpts()
            o.struct_size, o.side, o.kind = size, side, kind
            poison(o)
            res = H.ColsResult()
            ex._sync_stream()
            assert ex.L.hmj_join_kind_cols_device(ex.h, C.byref(rb), C.byref(rp), 0, C.byref(o), C.byref(res)) == 0, size
            assert int(res.n_matches) == rows and untouched(o) and o.struct_size == size and o.form == H.HMJ_COLS_PACKED, (size, kind)
            assert o.n_key_pairs == ((n - 100) if size >= 112 else 0)
    # a full-size struct: the in fields come back as they were, the out fields are written
    o = H.ColsKindOpts()
    o.struct_size, o.side, o.kind = C.sizeof(H.ColsKindOpts), PROBE, ANTI
    o.n_build_null, o.n_probe_null = 777, 888
    bits = H.pack_validity(np.arange(n) % 3 != 0, 2, "cuda")
    arr = (H.Validity * 2)()
    arr[1].bits, arr[1].bit_offset = bits.data_ptr(), 2
    o.probe_validity = arr
    res = H.ColsResult()
    ex._sync_stream()
    assert ex.L.hmj_join_kind_cols_device(ex.h, C.byref(rb), C.byref(rp), 0, C.byref(o), C.byref(res)) == 0
    assert (o.n_build_null, o.n_probe_null) == (0, 100) and C.addressof(o.probe_validity.contents) == C.addressof(arr)
    assert not o.build_validity and int(res.n_matches) == 100 + sum(1 for s in range(n - 100) if s % 3 == 0)
    del kb, kp


@pytest.mark.parametrize("widths", [[4, 4], [8, 4, 2]])
def test_degenerate_sides(H, ex, widths):
    rng = random.Random(31 + len(widths))
    nb, np_ = 300, 420
    bt, pt = drawn(rng, widths, nb, np_)
    bcols, pcols = columns(bt, widths), columns(pt, widths)
    bv, pv = [rng.getrandbits(64) for _ in bt], [rng.getrandbits(64) for _ in pt]
    B, P = dev_rel(bcols, bv), dev_rel(pcols, pv)
    k = len(widths)
    some_b = [None] * (k - 1) + [np.arange(nb) % 4 != 1]
    some_p = [np.arange(np_) % 5 != 2] + [None] * (k - 1)
    none_b = [np.ones(nb, bool), np.zeros(nb, bool)] + [None] * (k - 2)  # every row NULL in column 1
    none_p = [np.zeros(np_, bool)] * k
    quick = (H.HMJ_ORDERED | H.HMJ_CHECKSUM | H.HMJ_SUM_PROBE, H.HMJ_CHECKSUM)
    for name, mb, mp in (("build all NULL", none_b, some_p), ("probe all NULL", some_b, none_p), ("both all NULL", none_b, none_p),
                         ("build side only", some_b, None), ("probe side only", None, some_p), ("all NULL against no bitmap", none_b, None)):
        bnull, pnull = null_rows(mb, nb), null_rows(mp, np_)
        expect = expect_all(bcols, bv, pcols, pv, widths, bnull, pnull)
        if "all NULL" in name:
            assert len(expect[(PROBE, INNER)][0]) == 0 and len(expect[(BUILD, FULL_OUTER)][0]) == nb + np_
        check(H, ex, B, P, dev_valid(H, mb, 6), dev_valid(H, mp, 1), expect, widths, pv, np_, bnull, pnull, quick, tag=(name,))
    # n = 0 on a side, with a bitmap pointer for it
    import torch

    spare = torch.full((8,), 0x5A, dtype=torch.uint8, device="cuda")
    empty = [np.zeros(0, "u%d" % w) for w in widths]
    E = dev_rel(empty, [])
    for eb, ep in ((True, False), (False, True), (True, True)):
        bc, pc = (empty if eb else bcols), (empty if ep else pcols)
        bvv, pvv = ([] if eb else bv), ([] if ep else pv)
        mb, mp = (None if eb else some_b), (None if ep else some_p)
        VB = [(spare, 3)] * k if eb else dev_valid(H, mb, 0)
        VP = [(spare, 0)] * k if ep else dev_valid(H, mp, 0)
        bnull, pnull = null_rows(mb, len(bvv)), null_rows(mp, len(pvv))
        expect = expect_all(bc, bvv, pc, pvv, widths, bnull, pnull)
        check(H, ex, E if eb else B, E if ep else P, VB, VP, expect, widths, pvv, len(pvv), bnull, pnull, quick, tag=("empty", eb, ep))


def test_collisions_with_compacted_inputs(H, ex):
    """force_hashed with 4 hash bits: 16 values of key64.  Semi / anti go through the ambiguous re-join with compacted
    rows, and every ordered run of equal key64 mixes tuples -- the collision sort must see the rows that have a key only."""
    widths = [4, 2, 2]
    rng = random.Random(404)
    nrng = np.random.default_rng(404)
    nb, np_ = 2000, 3000
    bt, pt = drawn(rng, widths, nb, np_, 1500)
    bcols, pcols = columns(bt, widths), columns(pt, widths)
    bv, pv = [rng.getrandbits(64) for _ in bt], [rng.getrandbits(64) for _ in pt]
    mb, mp = draw_masks(nrng, nb, 3, "all", 0.2), draw_masks(nrng, np_, 3, "one", 0.2)
    bnull, pnull = null_rows(mb, nb), null_rows(mp, np_)
    assert 300 < bnull.sum() < 500 and 450 < pnull.sum() < 750
    expect = expect_all(bcols, bv, pcols, pv, widths, bnull, pnull, bits=4, force=True)
    full = expect[(BUILD, FULL_OUTER)][0]
    head = full[:len(full) - int(bnull.sum()) - int(pnull.sum())]
    run = np.bincount(head[:, 0].astype(np.int64))
    assert expect[(PROBE, INNER)][4] > 1000 and int(head[:, 0].max()) < 16 and 1 < run.max() <= 1024, run.max()
    assert len(set(bt) & set(pt)) > 100 and len(expect[(PROBE, INNER)][0]) > 500
    B, P = dev_rel(bcols, bv), dev_rel(pcols, pv)
    check(H, ex, B, P, dev_valid(H, mb, 13), dev_valid(H, mp, 7), expect, widths, pv, np_, bnull, pnull,
          (H.HMJ_ORDERED | H.HMJ_CHECKSUM | H.HMJ_SUM_PROBE,), bits=4, force=True)
    res, info, _ = call(H, ex, B, P, dev_valid(H, mb, 13), dev_valid(H, mp, 7), PROBE, SEMI, 0, 4, True)
    assert info["n_collisions"] > 0


def test_several_scan_blocks_against_numpy(H, ex):
    """100 003 x 150 001 rows ([8,4,2], hashed), 10 % NULL-key rows, count mode: 391 and 586 workgroups of valid-row counts
    through the scan.  Counts and sums from numpy: tuples as structured values through np.unique."""
    nb, np_ = 100003, 150001
    rng = np.random.default_rng(77)
    ids_b, ids_p = rng.integers(0, 60000, nb), rng.integers(20000, 80000, np_)
    tup = lambda ids: [ids.astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15), (ids * 7919).astype(np.uint32), (ids % 65521).astype(np.uint16)]
    bcols, pcols = tup(ids_b), tup(ids_p)
    bv = rng.integers(0, 1 << 40, nb, dtype=np.uint64)
    pv = rng.integers(0, 1 << 40, np_, dtype=np.uint64)
    mb = [None, rng.random(nb) >= 0.05, rng.random(nb) >= 0.05]
    mp = [rng.random(np_) >= 0.1, None, None]
    bnull, pnull = null_rows(mb, nb), null_rows(mp, np_)
    # garbage under the NULL slots: the bytes of tuples that exist on the other side
    for c in range(3):
        bcols[c][bnull] = pcols[c][:int(bnull.sum())]
        pcols[c][pnull] = bcols[c][~bnull][:int(pnull.sum())]
    st = np.dtype([("a", "u8"), ("b", "u4"), ("c", "u2")])
    as_st = lambda cols: np.rec.fromarrays(cols, dtype=st)
    tb, tp = as_st([c[~bnull] for c in bcols]), as_st([c[~pnull] for c in pcols])
    uniq, inv = np.unique(np.concatenate([tb, tp]), return_inverse=True)
    ib, ip = inv[:len(tb)], inv[len(tb):]
    cb, cp = np.bincount(ib, minlength=len(uniq)), np.bincount(ip, minlength=len(uniq))
    sb, sp = np.zeros(len(uniq), np.uint64), np.zeros(len(uniq), np.uint64)
    np.add.at(sb, ib, bv[~bnull])
    np.add.at(sp, ip, pv[~pnull])
    m = lambda x: int(x) & M64
    n_in = int((cb * cp).sum())
    in_r = m(sum(int(x) for x in sb * cp.astype(np.uint64)))
    in_s = m(sum(int(x) for x in sp * cb.astype(np.uint64)))
    p_hit, b_hit = np.zeros(np_, bool), np.zeros(nb, bool)
    p_hit[~pnull] = np.isin(tp, tb)
    b_hit[~bnull] = np.isin(tb, tp)
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
    B, P = dev_rel(bcols, bv), dev_rel(pcols, pv)
    VB, VP = dev_valid(H, mb, 5), dev_valid(H, mp, 63)
    for (side, kind), (n, sr, ss) in want.items():
        res, info, _ = call(H, ex, B, P, VB, VP, side, kind, H.HMJ_SUM_PROBE)
        print(side, kind, res.checks(), info)
        assert (int(res.n_matches), int(res.sum_r), int(res.sum_s)) == (n, sr, ss), (side, kind)
        assert int(res.sum_probe_all) == sum_at(pv, slice(None)) and info["n_collisions"] == 0 and info["form"] == H.HMJ_COLS_HASHED
        assert (info["n_build_null"], info["n_probe_null"]) == (int(bnull.sum()), int(pnull.sum()))
        if (side, kind) in COUNTS_PROBE:
            assert (info["n_probe_matched"], info["n_probe_unmatched"]) == (int(p_hit.sum()), n_pu)
        if side == BUILD:
            assert (info["n_build_matched"], info["n_build_unmatched"]) == (int(b_hit.sum()), n_bu)
        if (side, kind) not in SEMI_ANTI:
            assert info["n_key_pairs"] == n_in


def test_bit_offset_overflow_is_an_argument_error(H, ex):
    import torch

    n = 100
    a = torch.arange(n, dtype=torch.int32, device="cuda")
    b = torch.arange(n, dtype=torch.int16, device="cuda")
    bits = torch.full((64,), 0xFF, dtype=torch.uint8, device="cuda")

    def good():
        res, info = ex.join_cols_device([a, b], None, [a, b], None, H.HMJ_CHECKSUM)
        assert int(res.n_matches) == n and int(res.sum_r) == int(res.sum_s) == n * (n - 1) // 2 and info["n_probe_null"] == 0

    good()
    for off in (2 ** 64 - 1, 2 ** 64 - n):
        for kw in (dict(build_valid=[None, (bits, off)]), dict(probe_valid=[(bits, off), None])):
            with pytest.raises(H.HmjError) as e:
                ex.join_cols_device([a, b], None, [a, b], None, 0, **kw)
            assert e.value.code == HMJ_E_ARG and "bit_offset" in str(e.value), (off, kw)
            good()
            with pytest.raises(H.HmjError) as e:
                ex.join_kind_cols_device([a, b], None, [a, b], None, BUILD, FULL_OUTER, H.HMJ_ORDERED, **kw)
            assert e.value.code == HMJ_E_ARG
            good()
    # the largest offset that does not overflow is not an argument error as such; an entry without bits ignores its offset
    res, info = ex.join_cols_device([a, b], None, [a, b], None, 0, probe_valid=[(bits[:0], 2 ** 64 - 1), (bits, 8)])
    assert int(res.n_matches) == n and info["n_probe_null"] == 0


def test_the_ctx_after_a_nullable_call(H):
    """After a call with bitmaps the same ctx runs a multi-column join without them, a u64 join and a string join with the
    results it gave before; like any other call the nullable one discards a prepared build side."""
    import torch

    os.environ["HMJ_GTABLE"] = "0"  # (a join this small would otherwise take the global table and partition nothing)
    try:
        e = H.Executor(0)
    finally:
        del os.environ["HMJ_GTABLE"]
    try:
        nb, npb = 300000, 200000
        Bu, Pu = e.gen_build(nb), e.gen_probe(npb, nb, miss_mod=4)
        widths = [8, 4, 2]
        rng = random.Random(5)
        bt, pt = drawn(rng, widths, 900, 1300)
        bcols, pcols = columns(bt, widths), columns(pt, widths)
        B, P = dev_rel(bcols, None), dev_rel(pcols, None)
        words = ["k%d" % (i % 700) for i in range(1000)]
        sb = tuple(t.cuda() for t in H.pack_strings(words[:600])) + (torch.arange(600, device="cuda"),)
        sp = tuple(t.cuda() for t in H.pack_strings(words[300:])) + (torch.arange(700, device="cuda"),)
        flags = H.HMJ_ORDERED | H.HMJ_CHECKSUM

        def others():
            u = e.join_device(Bu, Pu, H.HMJ_CHECKSUM).checks()
            c, _ = e.join_cols_device(B[0], None, P[0], None, flags)
            rows_c = e.cols_rows_to_numpy(c)
            s, _ = e.join_str_device(sb, sp, flags)
            return u, c.checks(), rows_c, s.checks(), e.str_rows_to_numpy(s)

        before = others()
        assert before[0]["n_matches"] > 100000 and len(before[2]) > 100 and before[3]["n_matches"] > 100
        mb = draw_masks(np.random.default_rng(5), 900, 3, "all", 0.3)
        mp = draw_masks(np.random.default_rng(6), 1300, 3, "one", 0.3)
        bnull, pnull = null_rows(mb, 900), null_rows(mp, 1300)
        VB, VP = dev_valid(H, mb, 3), dev_valid(H, mp, 11)
        e.set_profiling(True)
        for side, kind in ((PROBE, INNER), (PROBE, ANTI), (BUILD, FULL_OUTER)):
            e.prepare_build(Bu, npb)
            want, counts = expected_null_kind_rows(bcols, None, pcols, None, widths, side, kind, bnull, pnull, probe_fill=PFILL,
                                                   build_fill=BFILL)
            res, info = e.join_kind_cols_device(B[0], None, P[0], None, side, kind, flags, probe_fill=PFILL, build_fill=BFILL,
                                                build_valid=VB, probe_valid=VP)
            assert np.array_equal(e.cols_kind_rows_to_numpy(res), want) and info["n_build_null"] == int(bnull.sum()) > 0
            r = e.join_device(Bu, Pu, 0)
            t = e.last_timing()
            assert int(r.n_matches) == before[0]["n_matches"] and not (t["path"] & H.HMJ_PATH_PREPARED) and t["ms_partition_build"] > 0.0
            after = others()
            assert after[0] == before[0] and after[1] == before[1] and after[3] == before[3]
            assert np.array_equal(after[2], before[2]) and np.array_equal(after[4], before[4])
    finally:
        e.close()
