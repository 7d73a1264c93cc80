"""GPU checks of the multi-column join kinds (hmj_join_kind_cols_device) against the pure-Python expectation of
test_join_cols_kinds_cpu.py: every kind in the count, checksum, materialising and ordered modes in both forms, forced key64
collisions (the ambiguous list of semi / anti, the collision sort over mixed rows), the duplicate bound of semi / anti, the
inner kind against hmj_join_cols_device, one wide column against the u64 kind entries, the forced hashed form against the
packed form, edges and empty sides, errors, the planner's isolation of the kinds' workloads, and 2^20 x 2^20 rows against
numpy."""
import ctypes as C
import os
import random

import numpy as np
import pytest

from test_join_cols_gpu import columns, draw_pool, unordered
from test_join_cols_kinds_cpu import (ALL_KINDS, ANTI, BUILD, BUILD_ANTI, BUILD_OUTER, BUILD_SEMI, COUNT_KEYS, FULL_OUTER, INNER,
                                      M64, NO_ROW, PROBE, PROBE_OUTER, SEMI, expected_kind_rows, key_collisions, kind_checks)

pytestmark = pytest.mark.gpu
HMJ_E_ARG, HMJ_E_UNSUPPORTED = -1, -5
PFILL, BFILL = 0xF1, 2 ** 64 - 2
SEMI_ANTI = [(PROBE, SEMI), (PROBE, ANTI), (BUILD, BUILD_SEMI), (BUILD, BUILD_ANTI)]


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


def dev_col(a, offset=0):
    """A numpy column on the device (as the signed dtype of its width: compared bit for bit anyway); offset: the column
    starts `offset` elements into its allocation -- aligned to its width, not to 16 bytes."""
    import torch

    a = np.ascontiguousarray(a)
    s = a.view("i%d" % a.dtype.itemsize)
    buf = torch.zeros(offset + len(s), dtype=torch.from_numpy(s[:0]).dtype)
    buf[offset:] = torch.from_numpy(s)
    return buf.cuda()[offset:]


def dev_vals(v):
    import torch

    return None if v is None else torch.tensor(np.asarray(v, np.uint64).view(np.int64), device="cuda")


def dev_rel(cols, vals, offset=0):
    return [dev_col(c, offset + k) for k, c in enumerate(cols)] if offset else [dev_col(c) for c in cols], dev_vals(vals)


def kjoin(ex, B, P, side, kind, flags=0, **kw):
    return ex.join_kind_cols_device(B[0], B[1], P[0], P[1], side, kind, flags, **kw)


def sum_of(pv, n):
    return (sum(pv) if pv is not None else n * (n - 1) // 2) & M64


def all_modes(H):
    return (0, H.HMJ_CHECKSUM | H.HMJ_SUM_PROBE, H.HMJ_MATERIALIZE | H.HMJ_CHECKSUM, H.HMJ_ORDERED | H.HMJ_CHECKSUM | H.HMJ_SUM_PROBE)


def check_kind(H, ex, B, P, bcols, bv, pcols, pv, widths, side, kind, bits=0, force=False, modes=None, pfill=PFILL, bfill=BFILL):
    """One kind in the four modes against the expectation: counts and sums; checksums and the probe sum; the multiset of
    rows and the absent columns; the ordered rows one by one; form, counters, key pairs and collisions in every mode."""
    want, counts = expected_kind_rows(bcols, bv, pcols, pv, widths, side, kind, bits, force, pfill, bfill)
    ck = kind_checks(want)
    hashed = force or sum(widths) > 8
    coll = key_collisions(bcols, pcols, widths, bits, force) if hashed else 0
    semi_anti = (side, kind) in SEMI_ANTI
    info = None
    for flags in all_modes(H) if modes is None else modes:
        tag = (widths, side, kind, flags, bits, force)
        res, info = kjoin(ex, B, P, side, kind, flags, hash_bits=bits, force_hashed=force, probe_fill=pfill, build_fill=bfill)
        got_ck = res.checks()
        print(tag, got_ck, {k: info[k] for k in ("form", "n_key_pairs", "n_collisions") + COUNT_KEYS})
        if flags & H.HMJ_CHECKSUM:
            assert got_ck == ck, tag
        else:
            assert (got_ck["n_matches"], got_ck["sum_r"], got_ck["sum_s"]) == (ck["n_matches"], ck["sum_r"], ck["sum_s"]), tag
        if flags & H.HMJ_SUM_PROBE:
            assert int(res.sum_probe_all) == sum_of(pv, len(pcols[0])), tag
        assert {k: info[k] for k in COUNT_KEYS} == counts, (tag, info, counts)
        assert info["form"] == (H.HMJ_COLS_HASHED if hashed else H.HMJ_COLS_PACKED), tag
        if semi_anti:
            assert info["n_collisions"] == 0 or coll > 0, tag
        else:
            inner = sum(1 for r in want if r[1] != NO_ROW and r[2] != NO_ROW)
            assert (info["n_collisions"], info["n_key_pairs"]) == (coll, inner + coll), tag
        if flags & (H.HMJ_MATERIALIZE | H.HMJ_ORDERED):
            got = ex.cols_kind_rows_to_numpy(res)
            assert got.shape == want.shape, (tag, got.shape, want.shape)
            if flags & H.HMJ_ORDERED:
                assert np.array_equal(got, want), (tag, np.flatnonzero(np.any(got != want, axis=1))[:5])
            else:
                assert np.array_equal(unordered(got), unordered(want)), tag
            if len(want):
                assert bool(res.r_row) == bool(res.rval) == (not semi_anti or side == BUILD), tag
                assert bool(res.s_row) == bool(res.sval) == (not semi_anti or side == PROBE), tag
        else:
            assert not res.key64, tag
    return want, info


def kind_relations(rng, widths, nb, np_, n_shared=300, n_only=100):
    """Duplicates and misses on both sides: build rows drawn from n_shared shared and n_only build-only tuples, probe rows
    from the shared and n_only probe-only tuples."""
    pool = draw_pool(rng, widths, n_shared + 2 * n_only)
    rng.shuffle(pool)
    shared, p_only, b_only = pool[:n_shared], pool[n_shared:n_shared + n_only], pool[n_shared + n_only:]
    bt = [(shared + b_only)[rng.randrange(n_shared + n_only)] for _ in range(nb)]
    pt = [(shared + p_only)[rng.randrange(n_shared + n_only)] for _ in range(np_)]
    return columns(bt, widths), columns(pt, widths)


# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("widths,with_vals", [([4, 4], True), ([1, 2, 4], False), ([8, 4, 2], True), ([8] * 8, False)])
def test_every_kind_on_duplicates_and_misses(H, ex, widths, with_vals):
    rng = random.Random(sum(widths) * 10 + len(widths))
    bcols, pcols = kind_relations(rng, widths, 1000, 4097)  # 4097: the last wave of the probe sweep is partial
    bv = [rng.getrandbits(64) for _ in range(1000)] if with_vals else None
    pv = [rng.getrandbits(64) for _ in range(4097)] if with_vals else None
    B, P = dev_rel(bcols, bv), dev_rel(pcols, pv)
    for side, kind in ALL_KINDS:
        want, info = check_kind(H, ex, B, P, bcols, bv, pcols, pv, widths, side, kind)
        assert info["n_collisions"] == 0
        if kind == FULL_OUTER:  # both sweeps emit
            assert info["n_probe_unmatched"] > 500 and info["n_build_unmatched"] > 100 and len(want) > 4000


def collision_relations(widths):
    rng = random.Random(60 + len(widths))
    pool = draw_pool(rng, widths, 800)
    rng.shuffle(pool)
    bt = [t for t in pool[:600] for _ in range(rng.randint(1, 3))] + [t for t in pool[600:700] for _ in range(rng.randint(1, 2))]
    pt = [t for t in pool[:600] for _ in range(rng.randint(0, 3))] + [t for t in pool[700:] for _ in range(rng.randint(1, 2))]
    rng.shuffle(bt)
    rng.shuffle(pt)
    bv = [rng.getrandbits(64) for _ in bt]
    pv = [rng.getrandbits(64) for _ in pt]
    return columns(bt, widths), bv, columns(pt, widths), pv


@pytest.mark.parametrize("widths", [[8, 4, 2], [8] * 8])
def test_forced_collisions(H, ex, widths):
    """hash_bits = 6: 64 values of key64 over 800 distinct tuples.  A probe row's representative is usually a build row of
    another tuple (the ambiguous list), and a run of equal key64 in an ordered result mixes pairs, unmatched probe rows
    and unmatched build rows of several tuples (the collision sort over mixed rows)."""
    bcols, bv, pcols, pv = collision_relations(widths)
    full, _ = expected_kind_rows(bcols, bv, pcols, pv, widths, BUILD, FULL_OUTER, 6, False, PFILL, BFILL)
    run = np.bincount(full[:, 0].astype(np.int64))
    assert key_collisions(bcols, pcols, widths, 6) > 0 and int(full[:, 0].max()) < 64 and 1 < run.max() <= 1024, run.max()
    assert (full[:, 1] == NO_ROW).sum() > 100 and (full[:, 2] == NO_ROW).sum() > 100
    B, P = dev_rel(bcols, bv), dev_rel(pcols, pv)
    for side, kind in ALL_KINDS:
        _, info = check_kind(H, ex, B, P, bcols, bv, pcols, pv, widths, side, kind, bits=6)
        assert info["n_collisions"] > 0, (side, kind)


@pytest.mark.parametrize("force", [False, True])
def test_semi_anti_never_form_the_cross_product(H, ex, force):
    """One tuple 3000 times on each side (9,000,000 pairs in the inner join) and 50 probe-only tuples: without a collision
    semi / anti form at most one pair per row of the side asked about."""
    widths = [4, 4]
    n = 3000
    bt = [(7, 9)] * n
    pt = [(7, 9)] * n + [(8, i) for i in range(50)]
    random.Random(3).shuffle(pt)
    bcols, pcols = columns(bt, widths), columns(pt, widths)
    B, P = dev_rel(bcols, None), dev_rel(pcols, None)
    hit = np.array([t == (7, 9) for t in pt])
    for side, kind, col, rows in ((PROBE, SEMI, 2, np.flatnonzero(hit)), (PROBE, ANTI, 2, np.flatnonzero(~hit)),
                                  (BUILD, BUILD_SEMI, 1, np.arange(n)), (BUILD, BUILD_ANTI, 1, np.arange(0))):
        for flags in (0, H.HMJ_MATERIALIZE):
            res, info = kjoin(ex, B, P, side, kind, flags, force_hashed=force)
            assert int(res.n_matches) == len(rows), (side, kind)
            assert info["n_key_pairs"] <= (len(pt) if side == PROBE else n) and info["n_collisions"] == 0, info
            assert info["form"] == (H.HMJ_COLS_HASHED if force else H.HMJ_COLS_PACKED)
            if flags:
                got = ex.cols_kind_rows_to_numpy(res)
                assert np.array_equal(np.sort(got[:, col]), rows.astype(np.uint64))


def test_inner_kind_is_the_inner_join(H, ex):
    for widths, bits in (([4, 4], 0), ([8, 4, 2], 0), ([8, 4, 2], 6)):
        rng = random.Random(80 + bits + len(widths))
        bcols, pcols = kind_relations(rng, widths, 700, 1500, 200, 60)
        bv = [rng.getrandbits(64) for _ in range(700)]
        B, P = dev_rel(bcols, bv), dev_rel(pcols, None)
        for flags in all_modes(H):
            a, ia = ex.join_cols_device(B[0], B[1], P[0], P[1], flags, hash_bits=bits)
            ra = ex.cols_rows_to_numpy(a)
            ca, sa = a.checks(), int(a.sum_probe_all)
            b, ib = kjoin(ex, B, P, PROBE, INNER, flags, hash_bits=bits, probe_fill=PFILL, build_fill=BFILL)
            assert b.checks() == ca and int(b.sum_probe_all) == sa and int(b.n_matches) > 1000
            assert (ib["form"], ib["n_key_pairs"], ib["n_collisions"]) == (ia["form"], ia["n_key_pairs"], ia["n_collisions"])
            assert (ib["n_collisions"] > 0) == (bits == 6) and [ib[k] for k in COUNT_KEYS] == [0] * 4
            rb = ex.cols_rows_to_numpy(b)
            if flags & H.HMJ_ORDERED:
                assert len(ra) and np.array_equal(rb, ra)
            else:  # (unordered: row order is unspecified, also between two inner joins)
                assert np.array_equal(unordered(rb), unordered(ra))


def test_one_wide_column_equals_the_u64_kinds(H, ex):
    import torch

    rng = np.random.default_rng(12)
    keys = rng.choice(np.arange(1, 1 << 20, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15), 6000, replace=False)
    kb, kp = keys[:4097], keys[1000:6000]  # unique on both sides (so (key) orders the rows), misses on both sides
    bv = rng.integers(0, 1 << 63, len(kb), dtype=np.uint64)
    pv = rng.integers(0, 1 << 63, len(kp), dtype=np.uint64)
    Bu = torch.from_numpy(np.stack([kb, bv], 1).view(np.int64)).cuda()
    Pu = torch.from_numpy(np.stack([kp, pv], 1).view(np.int64)).cuda()
    B, P = dev_rel([kb], bv), dev_rel([kp], pv)
    flags = H.HMJ_ORDERED | H.HMJ_CHECKSUM
    for side, kind in ALL_KINDS[1:]:
        if side == PROBE:
            u, cu = ex.join_kind_device(Bu, Pu, kind, flags, outer_fill=PFILL)
        else:
            u, cu = ex.join_build_kind_device(Bu, Pu, kind, flags, build_fill=BFILL, probe_fill=PFILL)
        want_checks = u.checks()
        if (side, kind) in SEMI_ANTI:
            want_rows, cols = (ex.probe_rows_to_numpy(u), [0, 4]) if side == PROBE else (ex.build_rows_to_numpy(u), [0, 3])
        else:
            want_rows, cols = ex.columns_to_numpy(u, host=False), [0, 3, 4]
        res, info = kjoin(ex, B, P, side, kind, flags, probe_fill=PFILL, build_fill=BFILL)
        assert res.checks() == want_checks, (side, kind)
        assert {k: info[k] for k in cu} == cu and info["form"] == H.HMJ_COLS_PACKED, (side, kind, info, cu)
        got = ex.cols_kind_rows_to_numpy(res)
        assert len(got) > 900 and np.array_equal(got[:, cols], want_rows), (side, kind)
        cnt, ic = kjoin(ex, B, P, side, kind, 0, probe_fill=PFILL, build_fill=BFILL)
        assert (int(cnt.n_matches), int(cnt.sum_r), int(cnt.sum_s)) == tuple(want_checks[k] for k in ("n_matches", "sum_r", "sum_s"))
        assert {k: ic[k] for k in cu} == cu


def test_forced_hashed_form_equals_the_packed_form(H, ex):
    widths = [4, 4]
    rng = random.Random(45)
    bcols, pcols = kind_relations(rng, widths, 1000, 4097)
    bv = [rng.getrandbits(64) for _ in range(1000)]
    B, P = dev_rel(bcols, bv), dev_rel(pcols, None)
    for side, kind in ALL_KINDS:
        rp, ip = kjoin(ex, B, P, side, kind, H.HMJ_MATERIALIZE, probe_fill=PFILL, build_fill=BFILL)
        packed = ex.cols_kind_rows_to_numpy(rp)
        cp = rp.checks()
        rh, ih = kjoin(ex, B, P, side, kind, H.HMJ_MATERIALIZE, force_hashed=True, probe_fill=PFILL, build_fill=BFILL)
        hashed = ex.cols_kind_rows_to_numpy(rh)
        ch = rh.checks()
        assert (ip["form"], ih["form"]) == (H.HMJ_COLS_PACKED, H.HMJ_COLS_HASHED) and ih["n_collisions"] == 0 == ip["n_collisions"]
        assert len(packed) > 100 and np.array_equal(unordered(packed[:, 1:]), unordered(hashed[:, 1:])), (side, kind)
        assert [ch[k] for k in ("n_matches", "sum_r", "sum_s")] == [cp[k] for k in ("n_matches", "sum_r", "sum_s")]
        assert [ih[k] for k in COUNT_KEYS] == [ip[k] for k in COUNT_KEYS]
        cnt, ic = kjoin(ex, B, P, side, kind, 0, force_hashed=True, probe_fill=PFILL, build_fill=BFILL)
        assert (int(cnt.n_matches), int(cnt.sum_r), int(cnt.sum_s)) == (cp["n_matches"], cp["sum_r"], cp["sum_s"])
        assert [ic[k] for k in COUNT_KEYS] == [ip[k] for k in COUNT_KEYS]


def test_edges(H, ex):
    widths = [2, 4, 1]
    some = [(7, 8, 9), (1, 2, 3), (7, 8, 9), (0, 0, 0)]
    quick = lambda H: (0, H.HMJ_ORDERED | H.HMJ_CHECKSUM | H.HMJ_SUM_PROBE)
    # each side empty in turn, both empty: unmatched rows carry their tuple's key64, form is filled
    for force in (False, True):
        for bt, pt in ((some, []), ([], some), ([], [])):
            bcols = columns(bt, widths) if bt else [np.zeros(0, "u%d" % w) for w in widths]
            pcols = columns(pt, widths) if pt else [np.zeros(0, "u%d" % w) for w in widths]
            bv, pv = list(range(50, 50 + len(bt))), list(range(90, 90 + len(pt)))
            B, P = dev_rel(bcols, bv), dev_rel(pcols, pv)
            for side, kind in ALL_KINDS:
                want, info = check_kind(H, ex, B, P, bcols, bv, pcols, pv, widths, side, kind, force=force, modes=quick(H))
                assert info["n_key_pairs"] == 0
                every = (bt and (side, kind) in ((BUILD, BUILD_ANTI), (BUILD, BUILD_OUTER), (BUILD, FULL_OUTER))) or (
                    pt and (side, kind) in ((PROBE, ANTI), (PROBE, PROBE_OUTER), (BUILD, FULL_OUTER)))
                assert len(want) == (4 if every else 0), (side, kind)
        # one row against one row, hit and miss
        one = columns([(7, 8, 9)], widths)
        for other in ([(7, 8, 9)], [(7, 8, 10)]):
            pcols = columns(other, widths)
            B, P = dev_rel(one, [5]), dev_rel(pcols, None)
            for side, kind in ALL_KINDS:
                check_kind(H, ex, B, P, one, [5], pcols, None, widths, side, kind, force=force, modes=quick(H))
    # 2^(8w) - 1 in every column, a top column of all zeros, columns that start inside their allocation; vals None on one
    # side only (the probe side here, the build side below)
    for widths in ([1, 2, 4], [8, 4, 2]):
        top = tuple((1 << (8 * w)) - 1 for w in widths)
        rng = random.Random(widths[0])
        low = draw_pool(rng, widths[1:], 150)
        bt = [top, top] + [(0,) + t for t in low] + [top[:-1] + (top[-1] - 1,)]
        pt = [(0,) + t for t in low[::2]] * 2 + [top] + [(1,) + t for t in low[:20]] + [(0,) * len(widths)]
        bcols, pcols = columns(bt, widths), columns(pt, widths)
        bv = list(range(1000, 1000 + len(bt)))
        for off_b, off_p in ((0, 0), (1, 3), (5, 2)):
            B, P = dev_rel(bcols, bv, off_b), dev_rel(pcols, None, off_p)
            for side, kind in ALL_KINDS:
                want, _ = check_kind(H, ex, B, P, bcols, bv, pcols, None, widths, side, kind, modes=(H.HMJ_ORDERED | H.HMJ_CHECKSUM,))
                assert len(want) >= 1
        pv = list(range(7, 7 + len(pt)))
        B, P = dev_rel(bcols, None), dev_rel(pcols, pv)
        for side, kind in ALL_KINDS:
            check_kind(H, ex, B, P, bcols, None, pcols, pv, widths, side, kind, modes=quick(H))


def test_errors_leave_the_ctx_usable(H, ex):
    import torch

    L, h = ex.L, ex.h
    n = 100
    a = torch.arange(n, dtype=torch.int32, device="cuda")
    b = torch.arange(n, dtype=torch.int16, device="cuda")
    raw = torch.zeros(4 * n + 8, dtype=torch.uint8, device="cuda")
    pa = torch.arange(50, 50 + n, dtype=torch.int32, device="cuda")
    pb = torch.arange(50, 50 + n, dtype=torch.int16, device="cuda")

    def good():
        res, info = ex.join_kind_cols_device([a, b], None, [pa, pb], None, PROBE, SEMI, H.HMJ_ORDERED)
        got = ex.cols_kind_rows_to_numpy(res)
        assert got[:, 2].tolist() == list(range(50)) and got[:, 4].tolist() == list(range(50)) and not got[:, [1, 3]].any()
        assert got[:, 0].tolist() == [(v << 16) | v for v in range(50, 100)]
        assert (info["n_probe_matched"], info["n_probe_unmatched"], info["form"]) == (50, 50, H.HMJ_COLS_PACKED)

    good()
    calls = {
        "unknown side": lambda: ex.join_kind_cols_device([a, b], None, [pa, pb], None, 2, SEMI),
        "BUILD_SIDE kind 0": lambda: ex.join_kind_cols_device([a, b], None, [pa, pb], None, BUILD, 0),
        "BUILD_SIDE kind 5": lambda: ex.join_kind_cols_device([a, b], None, [pa, pb], None, BUILD, 5),
        "PROBE_SIDE kind 4": lambda: ex.join_kind_cols_device([a, b], None, [pa, pb], None, PROBE, 4),
        "FIRST_WINS": lambda: ex.join_kind_cols_device([a, b], None, [pa, pb], None, PROBE, SEMI, H.HMJ_FIRST_WINS),
        "FIRST_WINS ordered": lambda: ex.join_kind_cols_device([a, b], None, [pa, pb], None, BUILD, FULL_OUTER,
                                                               H.HMJ_FIRST_WINS | H.HMJ_ORDERED),
        "hash_bits": lambda: ex.join_kind_cols_device([a, b], None, [pa, pb], None, PROBE, ANTI, hash_bits=64),
        "widths differ": lambda: ex.join_kind_cols_device([a, b], None, [pa, pa], None, BUILD, BUILD_OUTER),
        "n_cols differ": lambda: ex.join_kind_cols_device([a, b], None, [pa], None, PROBE, PROBE_OUTER),
    }
    for name, call in calls.items():
        with pytest.raises(H.HmjError) as e:
            call()
        assert e.value.code == HMJ_E_ARG, name
        good()

    def rel(cols, n_rows=n):
        arr = (H.KeyCol * len(cols))()
        for k, (ptr, width) in enumerate(cols):
            arr[k].data, arr[k].width = ptr, width
        r = H.ColsRel()
        r.cols, r.n_cols, r.vals, r.n = arr, len(cols), None, n_rows
        return r, arr

    def call(rb, rp, size=None, kind=SEMI, opts=True, out=True):
        o = H.ColsKindOpts()
        o.struct_size = C.sizeof(H.ColsKindOpts) if size is None else size
        o.side, o.kind = PROBE, kind
        res = H.ColsResult()
        ex._sync_stream()
        return L.hmj_join_kind_cols_device(h, C.byref(rb[0]) if rb else None, C.byref(rp[0]) if rp else None, 0,
                                           C.byref(o) if opts else None, C.byref(res) if out else None), o, res

    G, GP = rel([(a.data_ptr(), 4), (b.data_ptr(), 2)]), rel([(pa.data_ptr(), 4), (pb.data_ptr(), 2)])
    assert raw.data_ptr() % 4 == 0
    for size in (0, 8, 24, 39):  # (the fills end at byte 40)
        assert call(G, GP, size=size)[0] == HMJ_E_ARG, size
        assert b"struct_size" in L.hmj_last_error(h)
        good()
    rc, _, _ = call(G, rel([(raw.data_ptr() + 1, 4), (pb.data_ptr(), 2)]))
    assert rc == HMJ_E_ARG and b"aligned" in L.hmj_last_error(h) and b"probe" in L.hmj_last_error(h)
    good()
    for kw in (dict(opts=False), dict(out=False)):
        assert call(G, GP, **kw)[0] == HMJ_E_ARG
        good()
    assert call(None, GP)[0] == HMJ_E_ARG and call(G, None)[0] == HMJ_E_ARG
    good()
    # a struct_size that holds the in fields only is enough; the out fields beyond it stay untouched
    rc, o, res = call(G, GP, size=40)
    assert rc == 0 and int(res.n_matches) == 50 and o.form == H.HMJ_COLS_PACKED and o.struct_size == 40
    assert o.counts.n_probe_matched == 0 and o.n_key_pairs == 0


def test_oversized_mixed_run_is_unsupported(H, ex):
    """hash_bits = 1: two values of key64 over 3000 distinct one-to-one tuples: the ordered FULL_OUTER returns
    HMJ_E_UNSUPPORTED as the ordered inner join does; the count-mode call is exact; the ctx stays usable."""
    rng = random.Random(3000)
    widths = [8, 4, 2]
    pool = draw_pool(rng, widths, 3000)
    pt = list(pool)
    rng.shuffle(pt)
    bcols, pcols = columns(pool, widths), columns(pt, widths)
    B, P = dev_rel(bcols, None), dev_rel(pcols, None)
    with pytest.raises(H.HmjError) as e:
        kjoin(ex, B, P, BUILD, FULL_OUTER, H.HMJ_ORDERED, hash_bits=1)
    assert e.value.code == HMJ_E_UNSUPPORTED and "1024 rows" in str(e.value)
    cnt, info = kjoin(ex, B, P, BUILD, FULL_OUTER, 0, hash_bits=1)
    runs = np.bincount(H.cols_key64(bcols, widths, hash_bits=1).astype(np.int64), minlength=2)
    assert int(cnt.n_matches) == 3000 and info["n_collisions"] == int((runs.astype(np.int64) ** 2).sum()) - 3000
    assert [info[k] for k in COUNT_KEYS] == [3000, 0, 3000, 0]
    assert (int(cnt.sum_r), int(cnt.sum_s)) == (3000 * 2999 // 2, 3000 * 2999 // 2)
    res, info = kjoin(ex, B, P, BUILD, FULL_OUTER, H.HMJ_ORDERED)
    got = ex.cols_kind_rows_to_numpy(res)
    assert len(got) == 3000 and info["n_collisions"] == 0 and np.all(got[1:, 0] >= got[:-1, 0])
    assert [pool[int(r)] for r in got[:, 1]] == [pt[int(s)] for s in got[:, 2]]


def test_cols_kinds_do_not_change_u64_plans(H):
    """Multi-column kind joins with duplicate tuples teach their workloads a cool-down; a u64 inner join and a u64 SEMI kind
    join of the same sizes must still plan exactly as on a fresh ctx, and the kinds' workloads carry kind codes 16..19."""
    import torch

    n = 1 << 20
    half = np.arange(n // 2, dtype=np.int64)
    c0 = torch.from_numpy(np.concatenate([half, half])).cuda()  # every tuple twice on each side ([8,4]: the hashed form)
    c1 = torch.from_numpy(np.concatenate([half, half]).astype(np.int32)).cuda()
    fresh = H.Executor(0)
    B, P = fresh.gen_build(n), fresh.gen_probe(n, n, miss_mod=3)
    fresh.join_device(B, P, H.HMJ_MATERIALIZE | H.HMJ_CHECKSUM)
    p_inner = fresh.last_plan()
    r_semi, _ = fresh.join_kind_device(B, P, H.HMJ_JOIN_SEMI, H.HMJ_MATERIALIZE)
    p_semi = fresh.last_plan()
    n_semi = int(r_semi.n_matches)
    fresh.close()
    ex2 = H.Executor(0)
    learnt, seen = 0, set()
    for side, kind in ((PROBE, SEMI), (BUILD, BUILD_ANTI), (PROBE, PROBE_OUTER), (BUILD, FULL_OUTER)):
        for _ in range(3):
            res, info = ex2.join_kind_cols_device([c0, c1], None, [c0, c1], None, side, kind, H.HMJ_MATERIALIZE)
            assert int(res.n_matches) == (0 if kind == BUILD_ANTI else n if kind == SEMI else 2 * n)
            assert info["form"] == H.HMJ_COLS_HASHED and info["n_collisions"] == 0
        p = ex2.last_plan()
        seen.add((p["workload"] >> 20) & 31)
        learnt |= p["cooling"]
    assert seen == {16, 17, 19}, seen  # (18, the ambiguous rows' join, runs only after a collision)
    ex2.join_device(B, P, H.HMJ_MATERIALIZE | H.HMJ_CHECKSUM)
    assert ex2.last_plan() == p_inner
    r2, _ = ex2.join_kind_device(B, P, H.HMJ_JOIN_SEMI, H.HMJ_MATERIALIZE)
    assert ex2.last_plan() == p_semi and int(r2.n_matches) == n_semi
    ex2.close()
    assert learnt, "the multi-column kind joins taught their workloads nothing: the test would not see a shared memo"


def test_a_cols_kind_join_discards_a_prepared_build_side(H):
    os.environ["HMJ_GTABLE"] = "0"  # (a join this small would otherwise take the global table and partition nothing)
    try:
        e = H.Executor(0)
    finally:
        del os.environ["HMJ_GTABLE"]
    try:
        import torch

        nb, npb = 300000, 200000
        B, P = e.gen_build(nb), e.gen_probe(npb, nb, miss_mod=4)
        a = torch.arange(1000, dtype=torch.int32, device="cuda")
        e.set_profiling(True)
        e.prepare_build(B, npb)
        r = e.join_device(B, P, 0)
        want = int(r.n_matches)
        assert e.last_timing()["path"] & H.HMJ_PATH_PREPARED  # (the control: this shape does reuse a prepared build side)
        for side, kind, rows in ((PROBE, SEMI, [a, a]), (BUILD, FULL_OUTER, [a, a]), (PROBE, ANTI, [a[:0], a[:0]])):
            e.prepare_build(B, npb)
            res, _ = e.join_kind_cols_device(rows, None, [a, a], None, side, kind, 0)
            assert int(res.n_matches) == 1000
            r = e.join_device(B, P, 0)
            t = e.last_timing()
            assert int(r.n_matches) == want and not (t["path"] & H.HMJ_PATH_PREPARED) and t["ms_partition_build"] > 0.0
            assert not (e.last_plan()["path"] & H.HMJ_PATH_PREPARED)
    finally:
        e.close()


def make_big():
    """2^20 x 2^20 rows: unique build tuples (a, b, c) -- a alone is unique, and so is its low half --, probe rows drawn from
    them with repeats, every second probe row changed in b to a tuple the build side does not hold.  The expectation
    comes from numpy: a sort-merge on a pairs the rows, comparing b and c confirms them.  Computed once and shared."""
    n = 1 << 20
    rng = np.random.default_rng(2021)
    a = rng.permutation(n).astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15)  # distinct 64-bit values, distinct low halves
    b = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    c = rng.integers(0, 1 << 16, n, dtype=np.uint64).astype(np.uint16)
    pick = rng.integers(0, n, n)
    pa, pb, pc = a[pick].copy(), b[pick].copy(), c[pick].copy()
    pb[::2] ^= np.uint32(0x80000000)
    bv = rng.integers(0, 1 << 63, n, dtype=np.uint64)
    pv = rng.integers(0, 1 << 63, n, dtype=np.uint64)
    assert len(np.unique(a.astype(np.uint32))) == n
    order = np.argsort(a, kind="stable")
    at = np.searchsorted(a[order], pa)
    r_of = order[np.minimum(at, n - 1)]
    hit = (a[r_of] == pa) & (b[r_of] == pb) & (c[r_of] == pc)
    assert np.array_equal(hit, np.arange(n) % 2 == 1) and np.array_equal(r_of, pick)
    b_hit = np.zeros(n, bool)
    b_hit[r_of[hit]] = True
    return {"n": n, "a": a, "b": b, "c": c, "pa": pa, "pb": pb, "pc": pc, "bv": bv, "pv": pv, "hit": hit, "r_of": r_of, "b_hit": b_hit}


@pytest.fixture(scope="module")
def big():
    return make_big()


@pytest.mark.parametrize("form", ["packed", "hashed"])
def test_large_against_numpy(H, ex, big, form):
    n = big["n"]
    if form == "packed":
        widths = [4, 4]
        bcols, pcols = [big["a"].astype(np.uint32), big["b"]], [big["pa"].astype(np.uint32), big["pb"]]
    else:
        widths = [8, 4, 2]
        bcols, pcols = [big["a"], big["b"], big["c"]], [big["pa"], big["pb"], big["pc"]]
    hit, r_of, b_hit, bv, pv = big["hit"], big["r_of"], big["b_hit"], big["bv"], big["pv"]
    kb, kp = H.cols_key64(bcols, widths), H.cols_key64(pcols, widths)
    assert len(np.unique(kb)) == n  # (no 64-bit collision among the build tuples: (key64, r_row, s_row) orders the rows)
    s_hit, s_miss, r_miss = np.flatnonzero(hit), np.flatnonzero(~hit), np.flatnonzero(~b_hit)
    zeros = lambda k: np.zeros(k, np.uint64)
    fill = lambda k, v: np.full(k, v, np.uint64)
    semi = np.stack([kp[s_hit], zeros(len(s_hit)), s_hit.astype(np.uint64), zeros(len(s_hit)), pv[s_hit]], 1)
    full = np.concatenate([
        np.stack([kp[s_hit], r_of[s_hit].astype(np.uint64), s_hit.astype(np.uint64), bv[r_of[s_hit]], pv[s_hit]], 1),
        np.stack([kp[s_miss], fill(len(s_miss), NO_ROW), s_miss.astype(np.uint64), fill(len(s_miss), PFILL), pv[s_miss]], 1),
        np.stack([kb[r_miss], r_miss.astype(np.uint64), fill(len(r_miss), NO_ROW), bv[r_miss], fill(len(r_miss), BFILL)], 1)])
    by = lambda rows: rows[np.lexsort((rows[:, 2], rows[:, 1], rows[:, 0]))]
    semi, full = by(semi), by(full)
    assert len(semi) == n // 2 and len(r_miss) > n // 2 and len(full) == n + len(r_miss)
    want_sp = int(pv.sum(dtype=np.uint64))
    B, P = dev_rel(bcols, bv), dev_rel(pcols, pv)
    want_form = H.HMJ_COLS_PACKED if form == "packed" else H.HMJ_COLS_HASHED
    for side, kind, want, counts in ((PROBE, SEMI, semi, (n // 2, n // 2, 0, 0)),
                                     (BUILD, FULL_OUTER, full, (n // 2, n // 2, n - len(r_miss), len(r_miss)))):
        ck = kind_checks(want)
        res, info = kjoin(ex, B, P, side, kind, H.HMJ_CHECKSUM | H.HMJ_SUM_PROBE, probe_fill=PFILL, build_fill=BFILL)
        print(form, side, kind, res.checks(), info)
        assert res.checks() == ck and int(res.sum_probe_all) == want_sp and not res.key64
        assert info["form"] == want_form and info["n_collisions"] == 0 and tuple(info[k] for k in COUNT_KEYS) == counts
        res, info = kjoin(ex, B, P, side, kind, H.HMJ_ORDERED | H.HMJ_CHECKSUM, probe_fill=PFILL, build_fill=BFILL)
        assert res.checks() == ck and tuple(info[k] for k in COUNT_KEYS) == counts
        got = ex.cols_kind_rows_to_numpy(res)
        assert got.shape == want.shape and np.array_equal(got, want), np.flatnonzero(np.any(got != want, axis=1))[:5]
