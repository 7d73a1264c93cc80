"""GPU checks of hmj_group_cols_device (rows grouped by multi-column keys: GROUP BY / DISTINCT) against `expected_groups`,
the numpy reference test_group_cols_cpu.py checks against a dict of tuples.  Everything is exact integer equality; an
unordered result is compared after its groups are sorted by first_row.  The shapes are the smallest at which each kernel
can go wrong: one lane per sorted position in 256-lane workgroups of four waves, so sizes sit around 64, 256 and 1024, and
group boundaries are placed on and next to wave and workgroup boundaries."""
import ctypes as C
import itertools

import numpy as np
import pytest

from test_group_cols_cpu import RUN_CAP, SWEEP_MAX_SKIPS, draw_case, draw_columns, draw_valid, exceeds_run_cap, sweep_params

pytestmark = pytest.mark.gpu
M64 = (1 << 64) - 1
HMJ_E_ARG, HMJ_E_UNSUPPORTED = -1, -5
COLUMNS = ("key64", "first_row", "count", "sum", "min", "max", "group_of_row")
# (511 .. 513 and 2047 .. 2049: the 512 positions one wave of group_agg_kernel walks, the 2048 of one of its workgroups)
SIZES = [1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1025, 2047, 2048, 2049, 4097]


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


def all_want(H):
    return H.HMJ_GROUP_COUNT | H.HMJ_GROUP_SUM | H.HMJ_GROUP_MIN | H.HMJ_GROUP_MAX | H.HMJ_GROUP_ROW_MAP


def dev_col(a):
    import torch

    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view("i%d" % a.dtype.itemsize).copy()).cuda()


def dev_vals(v):
    import torch

    return None if v is None else torch.from_numpy(np.asarray(v, np.uint64).view(np.int64).copy()).cuda()


def dev_valid(H, valid, offset=0):
    if valid is None:
        return None
    return [None if v is None else (H.pack_validity(v, offset, "cuda"), offset) for v in valid]


def group(H, ex, cols, vals=None, valid=None, flags=None, want=None, offset=0, **kw):
    flags = H.HMJ_MATERIALIZE if flags is None else flags
    want = all_want(H) if want is None else want
    res, info = ex.group_cols_device([dev_col(c) for c in cols], dev_vals(vals), dev_valid(H, valid, offset), flags, want, **kw)
    return res, info, ex.group_rows_to_numpy(res)


def by_first_row(got):
    """The group columns sorted by first_row, and group_of_row renumbered to match."""
    perm = np.argsort(got["first_row"], kind="stable")
    inv = np.empty(len(perm), np.int64)
    inv[perm] = np.arange(len(perm))
    out = {k: (None if got[k] is None else got[k][perm]) for k in COLUMNS[:-1]}
    g = got["group_of_row"]
    out["group_of_row"] = None if g is None else inv[g.astype(np.int64)].astype(np.uint64)
    return out


def check(H, res, info, got, exp, ordered, tag="", want=None):
    want = all_want(H) if want is None else want
    assert (int(res.n_groups), int(res.n_rows), int(res.max_count)) == (exp["n_groups"], exp["n_rows"], exp["max_count"]), tag
    assert (info["form"], info["n_null"], info["n_collisions"]) == (exp["form"], exp["n_null"], exp["n_collisions"]), (tag, info)
    asked = {"key64": True, "first_row": True, "count": want & H.HMJ_GROUP_COUNT, "sum": want & H.HMJ_GROUP_SUM,
             "min": want & H.HMJ_GROUP_MIN, "max": want & H.HMJ_GROUP_MAX, "group_of_row": want & H.HMJ_GROUP_ROW_MAP}
    cmp = got if ordered else by_first_row(got)
    for k in COLUMNS:
        if not asked[k]:
            assert got[k] is None, (tag, k, "a column not asked for must be NULL")
            continue
        assert cmp[k] is not None, (tag, k)
        bad = np.flatnonzero(cmp[k] != exp[k])
        assert len(bad) == 0, (tag, k, bad[:5], cmp[k][bad[:5]], exp[k][bad[:5]])


def run_and_check(H, ex, cols, widths, vals=None, valid=None, ordered=False, tag="", offset=0, **kw):
    flags = H.HMJ_ORDERED if ordered else H.HMJ_MATERIALIZE
    res, info, got = group(H, ex, cols, vals, valid, flags, offset=offset, **kw)
    exp = H.expected_groups(cols, widths, vals, valid, kw.get("hash_bits", 0), kw.get("force_hashed", False), ordered)
    check(H, res, info, got, exp, ordered, tag)
    return res, info, got, exp


# ---- sizes --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_sizes_and_group_boundaries(H, ex, n):
    """Every size with one group, all rows distinct, groups of exactly 64 and 256 rows aligned to the sorted order (packed
    keys i // 64: the stable sort leaves row i at position i), and the same shifted by one row, so that every group
    straddles a wave and every fourth a workgroup boundary; and the same with groups of 512 and 2048 rows, the positions one
    wave and one workgroup of group_agg_kernel walk (kAggChunks * 64, KJ_WAVES waves): a group that ends exactly on a wave's
    range is the only one its carry stores without an atomic, one that crosses it by a single row the smallest atomic finish.
    Payloads near 2^63: the sums wrap."""
    rng = np.random.default_rng(n)
    i = np.arange(n, dtype=np.uint64)
    vals = (np.uint64(1 << 63) - np.uint64(5)) + rng.integers(0, 11, size=n).astype(np.uint64)
    zero = np.zeros(n, np.uint32)
    cases = {"one group": i * np.uint64(0), "distinct": i, "64 aligned": i // np.uint64(64), "256 aligned": i // np.uint64(256),
             "64 shifted": (i + np.uint64(1)) // np.uint64(64), "256 shifted": (i + np.uint64(1)) // np.uint64(256),
             # the aggregate kernel's own ranges: a group that ends exactly on a wave's 512 positions (the only one its
             # carry stores without an atomic) or on a workgroup's 2048, and the same crossing the range by one row
             "512 aligned": i // np.uint64(512), "512 shifted": (i + np.uint64(1)) // np.uint64(512),
             "2048 aligned": i // np.uint64(2048), "2048 shifted": (i + np.uint64(1)) // np.uint64(2048)}
    for name, key in cases.items():
        cols = [zero, key.astype(np.uint32)]
        for ordered in (False, True):
            _, info, _, _ = run_and_check(H, ex, cols, [4, 4], vals, ordered=ordered, tag=(name, n, ordered))
            assert info["form"] == H.HMJ_COLS_PACKED
    for name in ("one group", "distinct", "64 shifted"):  # the hashed heads compare tuples: the same boundaries there
        key = cases[name]
        cols = [key, key.astype(np.uint32), (key & np.uint64(0xFFFF)).astype(np.uint16)]
        _, info, _, _ = run_and_check(H, ex, cols, [8, 4, 2], vals, ordered=True, tag=("hashed", name, n))
        assert info["form"] == H.HMJ_COLS_HASHED


# ---- forms --------------------------------------------------------------------------------------------------------------------
FORMS = [([1], False), ([8], False), ([4, 4], False), ([2, 2, 2, 2], False), ([4, 4], True), ([8, 4, 2], False), ([8] * 8, False)]


@pytest.mark.parametrize("widths,forced", FORMS)
def test_forms(H, ex, widths, forced):
    rng = np.random.default_rng(sum(widths) + len(widths))
    for n, card in ((1000, 37), (1531, 1531)):
        cols = draw_columns(rng, n, widths, card)
        vals = rng.integers(0, 1 << 64, size=n, dtype=np.uint64)
        for ordered in (False, True):
            _, info, _, _ = run_and_check(H, ex, cols, widths, vals, ordered=ordered, force_hashed=forced, tag=(widths, n, ordered))
            assert info["form"] == (H.HMJ_COLS_HASHED if (sum(widths) > 8 or forced) else H.HMJ_COLS_PACKED)


# ---- aggregates -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def agg_case(H):
    rng = np.random.default_rng(777)
    widths = [4, 2, 8]
    cols = draw_columns(rng, 777, widths, 23)
    vals = (np.uint64(1 << 63) - np.uint64(1000)) + rng.integers(0, 2000, size=777).astype(np.uint64)
    return cols, widths, vals, H.expected_groups(cols, widths, vals)


def test_sums_wrap_and_min_max_are_unsigned(H, ex, agg_case):
    cols, widths, vals, exp = agg_case
    res, info, got = group(H, ex, cols, vals)
    check(H, res, info, got, exp, False)
    big = exp["count"] >= 2
    assert big.any() and (exp["sum"][big] < exp["min"][big]).any()  # a wrapped sum lies below its own terms
    assert (exp["max"] >= np.uint64(1 << 63)).any() and (exp["min"] < np.uint64(1 << 63)).any()  # across the sign bit


def test_without_vals_the_payload_is_the_row_index(H, ex, agg_case):
    cols, widths, _, _ = agg_case
    res, info, got, exp = run_and_check(H, ex, cols, widths, None)
    assert np.array_equal(got["min"], got["first_row"])
    rows = np.arange(777, dtype=np.uint64)
    g = got["group_of_row"].astype(np.int64)
    assert np.array_equal(np.bincount(g, weights=rows.astype(np.float64)).astype(np.uint64), got["sum"])  # (small: exact in doubles)


def test_every_want_subset(H, ex, agg_case):
    """All 32 subsets of the five bits on one input: a column not asked for is NULL, and the others do not change."""
    cols, widths, vals, exp = agg_case
    for want in range(32):
        res, info, got = group(H, ex, cols, vals, want=want)
        check(H, res, info, got, exp, False, tag=want, want=want)


def test_row_map(H, ex, agg_case):
    cols, widths, vals, exp = agg_case
    for ordered in (False, True):
        res, info, got = group(H, ex, cols, vals, flags=H.HMJ_ORDERED if ordered else H.HMJ_MATERIALIZE)
        g = got["group_of_row"].astype(np.int64)
        first = got["first_row"].astype(np.int64)
        rows = np.arange(777)
        assert (first[g] <= rows).all()
        for c in cols:
            assert np.array_equal(c[first[g]], c)  # equal tuples
        assert np.array_equal(np.bincount(g, minlength=len(first)).astype(np.uint64), got["count"])


def test_take_through_first_row_is_the_distinct_table(H, ex):
    rng = np.random.default_rng(31)
    widths = [4, 8, 1]
    n = 900
    cols = draw_columns(rng, n, widths, 40)
    valid = draw_valid(rng, n, 3, 0.1, {0, 2})
    dcols, dvalid = [dev_col(c) for c in cols], dev_valid(H, valid, 3)
    res, info = ex.group_cols_device(dcols, None, dvalid, H.HMJ_ORDERED, 0)
    exp = H.expected_groups(cols, widths, None, valid, ordered=True)
    ng = int(res.n_groups)
    assert ng == exp["n_groups"]
    outs, words, tinfo = ex.take_cols_device(dcols, (res.first_row, ng), valid=dvalid)
    got = ex.group_rows_to_numpy(res)  # the group result survives the take
    assert np.array_equal(got["first_row"], exp["first_row"]) and np.array_equal(got["key64"], exp["key64"])
    first = exp["first_row"].astype(np.int64)
    for c in range(3):
        ok = np.ones(ng, bool) if valid[c] is None else valid[c][first]
        assert np.array_equal(H.unpack_validity(words[c], ng), ok), c
        want = np.where(ok, cols[c][first], 0).astype(cols[c].dtype)
        assert np.array_equal(outs[c].cpu().numpy().view(cols[c].dtype), want), c
        assert tinfo["null_count"][c] == int((~ok).sum())


# ---- NULLs ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", [{1}, {0, 2}, {0, 1, 2}])
def test_null_slots_in_one_some_and_all_columns(H, ex, which):
    rng = np.random.default_rng(100 + len(which))
    widths = [2, 4, 1]  # fits 8 bytes: a bitmap alone makes the call hashed
    n = 1300
    cols = draw_columns(rng, n, widths, 25)
    valid = draw_valid(rng, n, 3, 0.1, which)
    dirty = [c.copy() for c in cols]
    for c in which:  # what lies under a NULL slot changes nothing
        dirty[c][~valid[c]] = rng.integers(0, 200, size=int((~valid[c]).sum())).astype(dirty[c].dtype)
    vals = rng.integers(0, 1 << 64, size=n, dtype=np.uint64)
    for offset in (0, 3, 67):
        for ordered in (False, True):
            res, info, got, exp = run_and_check(H, ex, dirty, widths, vals, valid, ordered, tag=(which, offset, ordered), offset=offset)
            clean = H.expected_groups(cols, widths, vals, valid, ordered=ordered)
            assert info["form"] == H.HMJ_COLS_HASHED and info["n_null"] == exp["n_null"] > 0
            assert all(np.array_equal(clean[k], exp[k]) for k in COLUMNS)


def test_an_all_null_relation_is_one_group(H, ex):
    n = 700
    cols = [np.arange(n, dtype=np.uint32), np.arange(n, dtype=np.uint64)]
    valid = [np.zeros(n, bool), np.zeros(n, bool)]
    res, info, got, exp = run_and_check(H, ex, cols, [4, 8], None, valid, ordered=True)
    assert int(res.n_groups) == 1 and int(res.max_count) == n and info["n_null"] == n
    assert got["first_row"].tolist() == [0] and got["sum"].tolist() == [n * (n - 1) // 2]


def test_an_all_valid_bitmap_gives_the_hashed_form_and_the_same_groups(H, ex):
    rng = np.random.default_rng(8)
    cols = draw_columns(rng, 1200, [4, 4], 60)
    plain = run_and_check(H, ex, cols, [4, 4])
    withmap = run_and_check(H, ex, cols, [4, 4], None, [np.ones(1200, bool), None], offset=67)
    assert plain[1]["form"] == H.HMJ_COLS_PACKED and withmap[1]["form"] == H.HMJ_COLS_HASHED and withmap[1]["n_null"] == 0
    a, b = by_first_row(plain[2]), by_first_row(withmap[2])
    for k in ("first_row", "count", "sum", "min", "max", "group_of_row"):
        assert np.array_equal(a[k], b[k]), k


# ---- collisions -----------------------------------------------------------------------------------------------------------------
def test_collisions_in_small_runs(H, ex):
    """hash_bits = 1: two values of key64 over 600 distinct [8, 4] tuples.  Both runs hold several tuples and stay under
    1024 rows (asserted from cols_key64), so each is sorted by (tuple, row) in one workgroup."""
    rng = np.random.default_rng(600)
    widths = [8, 4]
    with np.errstate(over="ignore"):
        base = [rng.permutation(600).astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15), rng.permutation(600).astype(np.uint32)]
    cols = base
    key = H.cols_key64(cols, widths, 1)
    runs = np.bincount(key.astype(np.int64), minlength=2)
    assert len(runs) == 2 and (runs > 1).all() and (runs <= RUN_CAP).all()
    vals = rng.integers(0, 1 << 64, size=600, dtype=np.uint64)
    for ordered in (False, True):
        _, info, _, exp = run_and_check(H, ex, cols, widths, vals, ordered=ordered, hash_bits=1, tag=ordered)
        assert info["n_collisions"] == 598 and exp["n_groups"] == 600
    # duplicates inside the runs: 200 tuples, three rows each, the rows of one tuple far apart
    pick = rng.permutation(np.repeat(np.arange(200), 3))
    cols = [b[pick] for b in base]
    assert len(set(H.cols_key64(cols, widths, 1).tolist())) == 2
    for ordered in (False, True):
        _, info, _, exp = run_and_check(H, ex, cols, widths, vals, ordered=ordered, hash_bits=1, tag=("dup", ordered))
        assert info["n_collisions"] == 198 and exp["max_count"] == 3 and exp["n_groups"] == 200


def test_an_oversized_mixed_run_is_unsupported(H, ex):
    """1100 rows of one key64 that hold two distinct tuples (picked on the host with cols_key64): beyond one workgroup's
    sort, ordered or not.  The same rows with all 64 hash bits are exact on the same ctx afterwards."""
    widths = [8, 4, 2]
    rng = np.random.default_rng(1100)
    cand = draw_columns(rng, 8, widths, 8)
    key = H.cols_key64(cand, widths, 1)
    same = [int(i) for i in np.flatnonzero(key == key[0])]
    same = [i for i in same if i == same[0] or any(cand[c][i] != cand[c][same[0]] for c in range(3))][:2]
    assert len(same) == 2
    pick = np.array(same * 550)
    cols = [c[pick] for c in cand]
    assert len(set(H.cols_key64(cols, widths, 1).tolist())) == 1
    for flags in (0, H.HMJ_MATERIALIZE, H.HMJ_ORDERED):
        with pytest.raises(H.HmjError) as e:
            group(H, ex, cols, flags=flags, hash_bits=1)
        assert e.value.code == HMJ_E_UNSUPPORTED and "1024 rows" in str(e.value)
    res, info, got, exp = run_and_check(H, ex, cols, widths, None, ordered=True)
    assert int(res.n_groups) == 2 and got["count"].tolist() == [550, 550] and info["n_collisions"] == 0


# ---- count-only -----------------------------------------------------------------------------------------------------------------
def test_count_only_fills_no_column(H, ex):
    rng = np.random.default_rng(12)
    for widths in ([4, 4], [8, 4, 2]):
        cols = draw_columns(rng, 5000, widths, 321)
        exp = H.expected_groups(cols, widths)
        res, info, got = group(H, ex, cols, flags=0)
        assert all(got[k] is None for k in COLUMNS)
        assert (int(res.n_groups), int(res.max_count), int(res.n_rows)) == (exp["n_groups"], exp["max_count"], 5000)
        assert (info["form"], info["n_null"], info["n_collisions"]) == (exp["form"], 0, 0)
    res, info, got = group(H, ex, [np.zeros(0, np.uint32)], flags=H.HMJ_ORDERED)  # n == 0
    assert (int(res.n_groups), int(res.max_count), int(res.n_rows), info["form"]) == (0, 0, 0, H.HMJ_COLS_PACKED)
    assert all(got[k] is None for k in COLUMNS)


# ---- the sort's MSD form ----------------------------------------------------------------------------------------------------------
def test_the_msd_sort_path(H, ex):
    """2^22 + 3 rows (the u64 sort changes form from 2^22 rows on), about 2^16 groups of Zipf sizes, [8, 4, 2], every want
    bit.  The tuple is an injective function of a group id, so numpy.unique on the ids is the reference."""
    rng = np.random.default_rng(22)
    n, G = (1 << 22) + 3, 1 << 16
    cdf = np.cumsum(1.0 / np.arange(1, G + 1))
    gid = np.searchsorted(cdf / cdf[-1], rng.random(n)).astype(np.uint64)
    gid = rng.permutation(G).astype(np.uint64)[np.minimum(gid, np.uint64(G - 1)).astype(np.int64)]
    cols = [gid * np.uint64(0x9E3779B97F4A7C15), gid.astype(np.uint32), gid.astype(np.uint16)]
    widths = [8, 4, 2]
    vals = rng.integers(0, 1 << 64, size=n, dtype=np.uint64)
    _, first, inv, count = np.unique(gid, return_index=True, return_inverse=True, return_counts=True)
    order = np.argsort(first, kind="stable")
    rank = np.empty(len(first), np.int64)
    rank[order] = np.arange(len(first))
    g_of_row = rank[inv.reshape(-1)]
    by_group = np.argsort(g_of_row, kind="stable")
    starts = np.concatenate([[0], np.cumsum(count[order])[:-1]]).astype(np.int64)
    sp = vals[by_group]
    res, info, got = group(H, ex, cols, vals)
    assert int(res.n_groups) == len(first) and int(res.max_count) == int(count.max()) and info["n_collisions"] == 0
    cmp = by_first_row(got)
    f = first[order]
    assert np.array_equal(cmp["first_row"], f.astype(np.uint64))
    assert np.array_equal(cmp["key64"], H.cols_key64([c[f] for c in cols], widths))
    assert np.array_equal(cmp["count"], count[order].astype(np.uint64))
    assert np.array_equal(cmp["sum"], np.add.reduceat(sp, starts))
    assert np.array_equal(cmp["min"], np.minimum.reduceat(sp, starts)) and np.array_equal(cmp["max"], np.maximum.reduceat(sp, starts))
    assert np.array_equal(cmp["group_of_row"], g_of_row.astype(np.uint64))


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals(H, ex):
    """Every HMJ_E_ARG case of the header, each followed by a good call on the same ctx."""
    import torch

    n = 100
    a = torch.arange(n, dtype=torch.int32, device="cuda") % 7
    b = torch.arange(n, dtype=torch.int64, device="cuda") % 3
    bitmap = H.pack_validity(np.ones(n, bool), 0, "cuda")
    exp = H.expected_groups([a.cpu().numpy(), b.cpu().numpy()], [4, 8])
    L, h = ex.L, ex.h
    ex._sync_stream()

    def call(flags=H.HMJ_MATERIALIZE, want=1, hash_bits=0, reserved=0, struct_size=None, rel_fix=None, col_fix=None, validity=None,
             null=()):
        kc = (H.KeyCol * 2)()
        kc[0].data, kc[0].width = a.data_ptr(), 4
        kc[1].data, kc[1].width = b.data_ptr(), 8
        if col_fix:
            col_fix(kc)
        rel = H.ColsRel()
        rel.cols, rel.n_cols, rel.n = kc, 2, n
        if rel_fix:
            rel_fix(rel)
        opts = H.GroupOpts()
        opts.struct_size = C.sizeof(H.GroupOpts) if struct_size is None else struct_size
        opts.want, opts.hash_bits, opts.reserved = want, hash_bits, reserved
        if validity is not None:
            opts.validity = validity
        res = H.GroupResult()
        rc = L.hmj_group_cols_device(h, None if "rel" in null else C.byref(rel), flags, None if "opts" in null else C.byref(opts),
                                     None if "out" in null else C.byref(res))
        return rc, res, opts

    def good():
        rc, res, opts = call(want=all_want(H))
        assert rc == 0 and int(res.n_groups) == exp["n_groups"] == 21 and int(res.max_count) == exp["max_count"]
        assert opts.form == H.HMJ_COLS_HASHED and np.array_equal(by_first_row(ex.group_rows_to_numpy(res))["count"], exp["count"])

    def overflow():
        v = (H.Validity * 2)()
        v[0].bits, v[0].bit_offset = bitmap.data_ptr(), M64 - n + 1
        return v

    def setter(field, value, index=None):
        def fix(obj):
            setattr(obj if index is None else obj[index], field, value)
        return fix

    good()
    bad = {
        "NULL rel": dict(null=("rel",)), "NULL opts": dict(null=("opts",)), "NULL out": dict(null=("out",)),
        "HMJ_FIRST_WINS": dict(flags=H.HMJ_MATERIALIZE | H.HMJ_FIRST_WINS), "HMJ_CHECKSUM": dict(flags=H.HMJ_CHECKSUM),
        "HMJ_SUM_PROBE": dict(flags=H.HMJ_SUM_PROBE), "unknown want bits": dict(want=0x20), "more want bits": dict(want=0x8001),
        "reserved": dict(reserved=1), "struct_size": dict(struct_size=H.GroupOpts.validity.offset + 4), "struct_size 0": dict(struct_size=0),
        "hash_bits": dict(hash_bits=64), "n_cols 0": dict(rel_fix=setter("n_cols", 0)), "n_cols 9": dict(rel_fix=setter("n_cols", 9)),
        "NULL cols": dict(rel_fix=setter("cols", None)), "rel reserved": dict(rel_fix=setter("reserved", 2)),
        "too many rows": dict(rel_fix=setter("n", 1 << 32)), "width 3": dict(col_fix=setter("width", 3, 0)),
        "col reserved": dict(col_fix=setter("reserved", 1, 1)), "NULL data": dict(col_fix=setter("data", None, 0)),
        "misaligned": dict(col_fix=setter("data", b.data_ptr() + 4, 1)), "bit_offset + n overflows": dict(validity=overflow()),
    }
    for name, kw in bad.items():
        rc, _, _ = call(**kw)
        assert rc == HMJ_E_ARG, (name, rc)
        assert len(L.hmj_last_error(h)) > 0, name
        good()
    assert L.hmj_group_cols_device(None, None, 0, None, None) == HMJ_E_ARG
    rc, res, opts = call(flags=H.HMJ_MATERIALIZE | H.HMJ_NULL_EQUAL)  # implied: accepted and ignored
    assert rc == 0 and int(res.n_groups) == 21
    rc, res, opts = call(struct_size=H.GroupOpts.n_null.offset)  # a header that ends behind validity: no out field is written
    assert rc == 0 and int(res.n_groups) == 21 and opts.form == H.HMJ_COLS_HASHED and opts.n_null == 0


# ---- neighbours -----------------------------------------------------------------------------------------------------------------
def test_a_group_call_between_two_u64_joins_changes_neither(H, ex):
    rng = np.random.default_rng(3)
    bd, pd = ex.gen_build(50000), ex.gen_probe(70000, 50000, miss_mod=3)
    cols = draw_columns(rng, 3000, [8, 4, 2], 100)
    fl = H.HMJ_ORDERED | H.HMJ_CHECKSUM
    r1 = ex.join_device(bd, pd, fl)
    c1, p1, rows1 = r1.checks(), ex.last_plan()["path"], ex.columns_to_numpy(r1, host=False)
    run_and_check(H, ex, cols, [8, 4, 2])
    assert ex.last_plan()["path"] == p1  # hmj_last_plan keeps describing the join
    r2 = ex.join_device(bd, pd, fl)
    assert r2.checks() == c1 and ex.last_plan()["path"] == p1 and np.array_equal(ex.columns_to_numpy(r2, host=False), rows1)


def test_a_group_call_discards_a_prepared_build_side(H):
    import os

    os.environ["HMJ_GTABLE"] = "0"  # (a join this small would otherwise take the global table and partition nothing)
    try:
        e = H.Executor(0)
    finally:
        del os.environ["HMJ_GTABLE"]
    try:
        rng = np.random.default_rng(4)
        nb, npb = 300000, 200000
        bd, pd = e.gen_build(nb), e.gen_probe(npb, nb, miss_mod=4)
        want = e.join_device(bd, pd, 0).checks()
        e.set_profiling(True)
        e.prepare_build(bd, npb)
        r = e.join_device(bd, pd, 0)
        assert r.checks() == want and e.last_timing()["path"] & H.HMJ_PATH_PREPARED  # (taken when nothing comes between)
        e.prepare_build(bd, npb)
        run_and_check(H, e, draw_columns(rng, 500, [4, 4], 9), [4, 4])
        r = e.join_device(bd, pd, 0)
        t = e.last_timing()
        assert r.checks() == want and not (t["path"] & H.HMJ_PATH_PREPARED) and t["ms_partition_build"] > 0.0
    finally:
        e.close()


def test_the_group_result_survives_a_take(H, ex):
    rng = np.random.default_rng(6)
    cols = draw_columns(rng, 2000, [4, 4], 77)
    vals = rng.integers(0, 1 << 64, size=2000, dtype=np.uint64)
    dcols = [dev_col(c) for c in cols]
    res, info = ex.group_cols_device(dcols, dev_vals(vals), None, H.HMJ_ORDERED, all_want(H))
    before = ex.group_rows_to_numpy(res)
    outs, _, _ = ex.take_cols_device(dcols, (res.group_of_row, 2000))
    outs2, _, _ = ex.take_cols_device(dcols, (res.first_row, int(res.n_groups)))
    after = ex.group_rows_to_numpy(res)
    assert all(np.array_equal(before[k], after[k]) for k in COLUMNS)
    check(H, res, info, after, H.expected_groups(cols, [4, 4], vals, ordered=True), True)
    # ordered and packed: the DISTINCT table ascends by tuple
    k = (outs2[0].cpu().numpy().view(np.uint32).astype(np.uint64) << np.uint64(32)) | outs2[1].cpu().numpy().view(np.uint32)
    assert np.array_equal(k, after["key64"]) and (np.diff(k.astype(np.float64)) > 0).all()


# ---- randomized sweep -------------------------------------------------------------------------------------------------------------
def test_randomized_sweep(H, ex):
    seed, iters = sweep_params()
    rng = np.random.default_rng(seed)
    skipped = 0
    for it in range(iters):
        case = draw_case(rng)
        tag = (seed, it, case["n"], case["widths"], case["hash_bits"])
        kw = dict(hash_bits=case["hash_bits"], force_hashed=case["force_hashed"])
        if exceeds_run_cap(H, case):
            skipped += 1
            with pytest.raises(H.HmjError) as e:
                group(H, ex, case["cols"], case["vals"], case["valid"], offset=case["offset"], **kw)
            assert e.value.code == HMJ_E_UNSUPPORTED, tag
            continue
        run_and_check(H, ex, case["cols"], case["widths"], case["vals"], case["valid"], case["ordered"], tag, case["offset"], **kw)
    assert skipped * 30 <= SWEEP_MAX_SKIPS * iters, (skipped, iters)
