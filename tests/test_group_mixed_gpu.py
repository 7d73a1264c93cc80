"""GPU checks of hmj_group_mixed_device (rows grouped by string and mixed keys: GROUP BY / DISTINCT) against
`expected_mixed_groups`, the host reference test_group_mixed_cpu.py checks against a dict of tuples, and -- on fixed columns
only -- against hmj_group_cols_device itself.  Everything is exact integer equality; an unordered result is compared after
its groups are sorted by first_row.  The shapes are the smallest at which each kernel can go wrong: one lane per sorted
position in 256-lane workgroups of four waves, a key kernel that stages a wave's 64 keys in 4096 bytes of LDS, and a
collision sort of at most 1024 rows in one workgroup."""
import ctypes as C

import numpy as np
import pytest

from test_group_cols_gpu import COLUMNS, all_want, by_first_row, check, dev_vals
from test_group_mixed_cpu import RUN_CAP, SWEEP_MAX_SKIPS, draw_case, draw_columns, draw_fixed, draw_strings, draw_valid, exceeds_run_cap, sweep_params

pytestmark = pytest.mark.gpu
M64 = (1 << 64) - 1
HMJ_E_ARG, HMJ_E_UNSUPPORTED = -1, -5
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


def dev_str(keys, base=0, first=0, null_data=False):
    """A string column on the device: (chars, offsets).  None slots hold no bytes.  base: the chars buffer starts that many
    bytes into its allocation; first: offsets[0]; null_data: no chars buffer at all."""
    import torch

    keys = [b"" if k is None else k for k in keys]
    lens = np.fromiter((len(k) for k in keys), dtype=np.int64, count=len(keys))
    off = np.full(len(keys) + 1, first, np.int64)
    np.cumsum(lens, out=off[1:])
    off[1:] += first
    if null_data:
        assert int(lens.sum()) == 0
        return None, torch.from_numpy(off).cuda()
    raw = np.frombuffer(b"\xa5" * (base + first) + b"".join(keys) + b"\x5a" * 3, np.uint8).copy()
    return torch.from_numpy(raw).cuda()[base:], torch.from_numpy(off).cuda()


def dev_cols(cols, **kw):
    import torch

    return [torch.from_numpy(np.ascontiguousarray(c).view("i%d" % c.dtype.itemsize).copy()).cuda() if isinstance(c, np.ndarray)
            else dev_str(c, **kw) for c in cols]


def dev_valid(H, valid, offset=0):
    if valid is None:
        return None
    return [None if v is None else (H.pack_validity(v, offset, "cuda"), offset) for v in valid]


def group(H, ex, cols, vals=None, valid=None, flags=None, want=None, offset=0, hash_bits=0, **kw):
    flags = H.HMJ_MATERIALIZE if flags is None else flags
    want = all_want(H) if want is None else want
    res, info = ex.group_mixed_device(dev_cols(cols, **kw), dev_vals(vals), dev_valid(H, valid, offset), flags, want, hash_bits)
    return res, info, ex.group_rows_to_numpy(res)


def run_and_check(H, ex, cols, vals=None, valid=None, ordered=False, tag="", offset=0, hash_bits=0, exp=None, **kw):
    flags = H.HMJ_ORDERED if ordered else H.HMJ_MATERIALIZE
    res, info, got = group(H, ex, cols, vals, valid, flags, offset=offset, hash_bits=hash_bits, **kw)
    exp = H.expected_mixed_groups(cols, vals, valid, hash_bits, ordered) if exp is None else exp
    check(H, res, info, got, exp, ordered, tag)
    return res, info, got, exp


def check_count_only(H, ex, cols, exp, valid=None, tag="", hash_bits=0):
    res, info, got = group(H, ex, cols, None, valid, flags=0, hash_bits=hash_bits)
    assert all(got[k] is None for k in COLUMNS), tag
    assert (int(res.n_groups), int(res.max_count), int(res.n_rows)) == (exp["n_groups"], exp["max_count"], exp["n_rows"]), tag
    assert (info["form"], info["n_null"], info["n_collisions"]) == (H.HMJ_COLS_HASHED, exp["n_null"], exp["n_collisions"]), tag


def key_shapes(gid):
    """The three key shapes of the size grid, each an injective function of the group id."""
    g = [int(x) for x in gid]
    return {"s": [[b"key-%d" % x for x in g]],
            "s,u32": [[b"k%d" % (x % 7) for x in g], ((gid * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)).astype(np.uint32)],
            "u16,s,s": [(gid & np.uint64(0xFFFF)).astype(np.uint16), [b"k%05d" % x for x in g], [b"x" * (x % 40) for x in g]]}


# ---- sizes --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_sizes_and_group_boundaries(H, ex, n):
    """Every size with one group, all rows distinct, and groups of exactly 64 and 256 rows, whole and shifted by one row (so
    that the first and last groups are one row off the wave and workgroup sizes), on the three key shapes, count-only,
    materialized and ordered.  Payloads near 2^63: the sums wrap."""
    rng = np.random.default_rng(n)
    i = np.arange(n, dtype=np.uint64)
    vals = (np.uint64(1 << 63) - np.uint64(5)) + rng.integers(0, 11, size=n).astype(np.uint64)
    cases = {"one group": i * np.uint64(0), "distinct": i, "64 aligned": i // np.uint64(64), "256 aligned": i // np.uint64(256),
             "64 shifted": (i + np.uint64(1)) // np.uint64(64), "256 shifted": (i + np.uint64(1)) // np.uint64(256)}
    for name, gid in cases.items():
        for shape, cols in key_shapes(gid).items():
            exp = None
            for ordered in (False, True):
                _, info, _, exp = run_and_check(H, ex, cols, vals, ordered=ordered, tag=(name, shape, n, ordered))
                assert info["form"] == H.HMJ_COLS_HASHED and exp["n_groups"] == len(set(gid.tolist()))
            check_count_only(H, ex, cols, exp, tag=(name, shape, n, "count"))


# ---- aggregates -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def agg_case(H):
    rng = np.random.default_rng(777)
    cols = draw_columns(rng, 777, ["s", 4], 23)
    vals = (np.uint64(1 << 63) - np.uint64(1000)) + rng.integers(0, 2000, size=777).astype(np.uint64)
    return cols, vals, H.expected_mixed_groups(cols, vals)


def test_every_want_subset(H, ex, agg_case):
    """All 32 subsets of the five bits on one input: a column not asked for is NULL, and the others do not change."""
    cols, vals, exp = agg_case
    for want in range(32):
        res, info, got = group(H, ex, cols, vals, want=want)
        check(H, res, info, got, exp, False, tag=want, want=want)
    big = exp["count"] >= 2
    assert big.any() and (exp["sum"][big] < exp["min"][big]).any()  # a wrapped sum lies below its own terms


def test_without_vals_the_payload_is_the_row_index(H, ex, agg_case):
    cols, _, _ = agg_case
    res, info, got, exp = run_and_check(H, ex, cols, None)
    assert np.array_equal(got["min"], got["first_row"])


# ---- fixed columns only: the column entry is the reference ------------------------------------------------------------------------
@pytest.mark.parametrize("widths", [[4], [4, 4], [8, 4, 2], [1, 2, 8, 4]])
def test_fixed_columns_only_equal_the_column_entry(H, ex, widths):
    """With and without bitmaps, ordered: every output column equals hmj_group_cols_device(force_hashed=True) on the same
    data."""
    rng = np.random.default_rng(sum(widths))
    n, k = 1531, len(widths)
    cols = [draw_fixed(rng, n, 60, w) for w in widths]
    vals = rng.integers(0, 1 << 64, size=n, dtype=np.uint64)
    for valid, bits in ((None, 0), (None, 2), (draw_valid(rng, n, k, 0.15, {0}), 0), (draw_valid(rng, n, k, 0.3, set(range(k))), 2)):
        dc, dv, dm = dev_cols(cols), dev_vals(vals), dev_valid(H, valid, 3)
        r1, i1 = ex.group_cols_device(dc, dv, dm, H.HMJ_ORDERED, all_want(H), bits, True)
        a = ex.group_rows_to_numpy(r1)
        head1 = (int(r1.n_groups), int(r1.n_rows), int(r1.max_count), i1["form"], i1["n_null"], i1["n_collisions"])
        r2, i2 = ex.group_mixed_device(dc, dv, dm, H.HMJ_ORDERED, all_want(H), bits)
        b = ex.group_rows_to_numpy(r2)
        assert head1 == (int(r2.n_groups), int(r2.n_rows), int(r2.max_count), i2["form"], i2["n_null"], i2["n_collisions"])
        for f in COLUMNS:
            assert np.array_equal(a[f], b[f]), (widths, bits, f)
        check(H, r2, i2, b, H.expected_mixed_groups(cols, vals, valid, bits, True), True, (widths, bits))


# ---- strings --------------------------------------------------------------------------------------------------------------------
def test_string_layouts(H, ex):
    """Empty strings; no chars buffer at all under all-empty slots; offsets[0] != 0 and an unaligned chars base; keys of
    0..40 bytes that share 8-byte prefixes; a wave whose 64 keys span more than the 4096 staged bytes next to one that fits;
    a 5000-byte key."""
    rng = np.random.default_rng(40)
    empties = [b""] * 300
    for kw in (dict(), dict(null_data=True), dict(first=5), dict(base=3)):
        res, _, got, _ = run_and_check(H, ex, [empties], ordered=True, tag=("empty", kw), **kw)
        assert int(res.n_groups) == 1 and got["count"].tolist() == [300]
    res, _, got, _ = run_and_check(H, ex, [empties, np.arange(300, dtype=np.uint32) % 9], ordered=True, null_data=True)
    assert int(res.n_groups) == 9
    pool = [(b"PREFIX%02d" % (j % 3)) [: min(8, j)] + bytes(rng.integers(0, 256, size=max(0, j - 8), dtype=np.uint8)) for j in range(41)]
    pool += [p + b"\x00" for p in pool[8:20]] + [pool[30][:-1] + b"\xff"]
    keys = [pool[int(j)] for j in rng.integers(0, len(pool), size=1300)]
    for kw in (dict(), dict(first=11), dict(base=1), dict(base=7, first=64), dict(base=15)):
        for ordered in (False, True):
            run_and_check(H, ex, [keys], ordered=ordered, tag=("0..40", kw, ordered), **kw)
            run_and_check(H, ex, [keys], ordered=ordered, hash_bits=1, tag=("0..40, one bit", kw, ordered), **kw)
    # rows 0..63: 64 keys of 70..90 bytes (> 4096 bytes: read from global memory); rows 64..127: short keys (staged); a
    # 5000-byte key twice, in a wave of its own kind
    long_keys = [bytes(rng.integers(0, 256, size=70 + j % 21, dtype=np.uint8)) for j in range(16)]
    huge = bytes(rng.integers(0, 256, size=5000, dtype=np.uint8))
    keys = [long_keys[j % 16] for j in range(64)] + [b"s%d" % (j % 5) for j in range(64)] + [huge, b"tiny", huge[:-1], huge] + [b"z"] * 30
    assert sum(len(k) for k in keys[:64]) > 4096 > sum(len(k) for k in keys[64:128])
    for ordered in (False, True):
        for bits in (0, 1):
            res, _, _, exp = run_and_check(H, ex, [keys], ordered=ordered, hash_bits=bits, base=5, tag=("spans", ordered, bits))
    assert exp["n_groups"] == 16 + 5 + 4


# ---- NULLs ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", [{0}, {0, 2}, {0, 1, 2}])
def test_null_slots_with_garbage_under_them(H, ex, which):
    """Bitmaps at bit offsets 0, 3 and 67; the bytes and values under NULL slots are garbage and change nothing."""
    rng = np.random.default_rng(100 + len(which))
    n = 1300
    cols = draw_columns(rng, n, ["s", 4, "s"], 25)
    valid = draw_valid(rng, n, 3, 0.1, which)
    clean = H.expected_mixed_groups([[b if (valid[c] is None or valid[c][i]) else None for i, b in enumerate(col)] if not isinstance(col, np.ndarray)
                                     else col for c, col in enumerate(cols)], None, valid, ordered=True)
    dirty = [list(c) if not isinstance(c, np.ndarray) else c.copy() for c in cols]
    for c in which:
        for i in np.flatnonzero(~valid[c]):
            dirty[c][int(i)] = b"garbage-%d" % int(i) if c != 1 else 0xDEAD
    vals = rng.integers(0, 1 << 64, size=n, dtype=np.uint64)
    for offset in (0, 3, 67):
        for ordered in (False, True):
            res, info, got, exp = run_and_check(H, ex, dirty, vals, valid, ordered, tag=(which, offset, ordered), offset=offset)
            assert info["n_null"] == exp["n_null"] > 0
            if ordered:
                assert all(np.array_equal(clean[k], exp[k]) for k in ("key64", "first_row", "count", "group_of_row"))
    check_count_only(H, ex, dirty, exp, valid, tag=which)


def test_a_null_string_is_not_the_empty_string(H, ex):
    keys = [b"", b"junk", b"", b"more", b"x"] * 40
    valid = [np.array([1, 0, 1, 0, 1] * 40, bool)]
    res, info, got, exp = run_and_check(H, ex, [keys], None, valid, ordered=False)
    assert int(res.n_groups) == 3 and info["n_null"] == 80 and by_first_row(got)["count"].tolist() == [80, 80, 40]
    # (NULL, x) against (x, NULL)
    x = [b"k"] * 130
    half = np.arange(130) < 65
    res, info, got, exp = run_and_check(H, ex, [x, x], None, [half, ~half], ordered=True, offset=3)
    assert int(res.n_groups) == 2 and got["count"].tolist() == [65, 65]


def test_an_all_null_relation_is_one_group(H, ex):
    n = 700
    cols = [[b"row-%d" % i for i in range(n)], np.arange(n, dtype=np.uint64)]
    valid = [np.zeros(n, bool), np.zeros(n, bool)]
    res, info, got, exp = run_and_check(H, ex, cols, None, valid, ordered=True)
    assert int(res.n_groups) == 1 and int(res.max_count) == n and info["n_null"] == n
    assert got["first_row"].tolist() == [0] and got["sum"].tolist() == [n * (n - 1) // 2]


def test_an_all_valid_bitmap_gives_the_same_groups(H, ex):
    rng = np.random.default_rng(8)
    cols = draw_columns(rng, 1200, ["s", 2], 60)
    plain = run_and_check(H, ex, cols, ordered=True)
    withmap = run_and_check(H, ex, cols, None, [np.ones(1200, bool), None], ordered=True, offset=67)
    assert withmap[1]["n_null"] == 0
    for k in COLUMNS:
        assert np.array_equal(plain[2][k], withmap[2][k]), k


# ---- collisions -----------------------------------------------------------------------------------------------------------------
def test_collisions_in_small_runs(H, ex):
    """hash_bits 1 and 3 over 500 distinct strings, three rows each, the rows of one string far apart: every run of equal
    key64 holds several tuples and stays under 1024 rows (asserted from the reference), so each is sorted by (tuple, row)
    in one workgroup.  The ordered result ties by the strings' byte order."""
    rng = np.random.default_rng(600)
    pool = sorted({bytes(rng.integers(0, 256, size=int(rng.integers(0, 20)), dtype=np.uint8)) for _ in range(600)})[:500]
    keys = [pool[int(j)] for j in rng.permutation(np.repeat(np.arange(500), 3))]
    vals = rng.integers(0, 1 << 64, size=1500, dtype=np.uint64)
    for bits in (1, 3):
        for valid in (None, [rng.random(1500) >= 0.05]):
            for ordered in (False, True):
                _, info, got, exp = run_and_check(H, ex, [keys], vals, valid, ordered, hash_bits=bits, tag=(bits, ordered), offset=3)
                assert 1 < exp["max_mixed_run"] <= RUN_CAP and info["n_collisions"] == exp["n_groups"] - (1 << bits) > 400
    # the same through a (string, u32) tuple whose strings tie: the u32 column decides the order
    cols = [[b"same"] * 1500, rng.permutation(1500).astype(np.uint32) % 500]
    for ordered in (False, True):
        _, info, _, exp = run_and_check(H, ex, cols, vals, ordered=ordered, hash_bits=1, tag=("tie", ordered))
        assert info["n_collisions"] == 498 and exp["max_mixed_run"] <= RUN_CAP


def test_an_oversized_mixed_run_is_unsupported(H, ex):
    """1100 rows of one key64 that hold two distinct strings: beyond one workgroup's sort in every mode.  Each refusal is
    followed by a correct call."""
    cand = [b"cand-%d" % j for j in range(8)]
    key = H.mixed_key64([cand], 1)
    same = [j for j in range(8) if key[j] == key[0]][:2]
    assert len(same) == 2
    keys = [cand[j] for j in same] * 550
    good = [b"g%d" % (j % 11) for j in range(300)]
    for flags in (0, H.HMJ_MATERIALIZE, H.HMJ_ORDERED):
        with pytest.raises(H.HmjError) as e:
            group(H, ex, [keys], flags=flags, hash_bits=1)
        assert e.value.code == HMJ_E_UNSUPPORTED and "1024 rows" in str(e.value) and "mixed-key grouping" in str(e.value)
        run_and_check(H, ex, [good], ordered=True, hash_bits=1)
    res, info, got, exp = run_and_check(H, ex, [keys], ordered=True)
    assert int(res.n_groups) == 2 and got["count"].tolist() == [550, 550] and info["n_collisions"] == 0


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def test_decreasing_offsets_are_refused_before_any_tuple_is_compared(H, ex):
    """A valid relation in which two adjacent offsets are swapped (row 70; row n - 1), so every offset still lies inside the
    allocation: HMJ_E_ARG naming column and row, in the first and in a later string column, without and with bitmaps,
    in every mode and with one hash bit (where every row would be compared); each refusal is followed by a correct call."""
    import torch

    rng = np.random.default_rng(70)
    n = 300
    cols = [[b"a%03d-" % (j % 50) + b"x" * (1 + j % 5) for j in range(n)], draw_fixed(rng, n, 7, 4), [b"b%d" % (j % 9) for j in range(n)]]
    valid = [None, None, np.arange(n) % 4 != 0]
    d = dev_cols(cols)

    def swapped(off, rows):
        h = off.cpu().numpy().copy()
        for r in rows:
            h[r], h[r + 1] = h[r + 1], h[r]
            assert h[r + 1] < h[r]
        return torch.from_numpy(h).cuda()

    for c, rows, row in ((0, (70, n - 1), 70), (2, (70, n - 1), 70), (0, (n - 1,), n - 1), (2, (n - 1,), n - 1)):
        bad = list(d)
        bad[c] = (d[c][0], swapped(d[c][1], rows))
        for dm in (None, dev_valid(H, valid, 3)):
            for flags, bits in ((0, 0), (H.HMJ_MATERIALIZE, 1), (H.HMJ_ORDERED, 1)):
                with pytest.raises(H.HmjError) as e:
                    ex.group_mixed_device(bad, None, dm, flags, all_want(H), bits)
                msg = "grouped relation: column %d: offsets decrease at row %d (offsets[%d] < offsets[%d])" % (c, row, row + 1, row)
                assert e.value.code == HMJ_E_ARG and msg in str(e.value), str(e.value)
            run_and_check(H, ex, cols, None, valid if dm else None, ordered=True, hash_bits=1, offset=3, tag=("after", c, rows))
    # data == NULL with non-empty keys
    with pytest.raises(H.HmjError) as e:
        ex.group_mixed_device([d[1], (None, d[2][1])], None, None, H.HMJ_MATERIALIZE)
    assert e.value.code == HMJ_E_ARG and "grouped relation: column 1: data is NULL but keys have bytes" in str(e.value)
    run_and_check(H, ex, cols, ordered=True)


def test_argument_refusals(H, ex):
    """The HMJ_E_ARG cases found on the host, each followed by a good call on the same ctx."""
    n = 100
    cols = [[b"n%d" % (j % 7) for j in range(n)], np.arange(n, dtype=np.uint64) % 3]
    d = dev_cols(cols)
    exp = H.expected_mixed_groups(cols)
    L, h = ex.L, ex.h
    ex._sync_stream()
    one_validity = (H.Validity * 2)()

    def call(flags=H.HMJ_MATERIALIZE, want=1, hash_bits=0, reserved=0, struct_size=None, validity=None, fix=None, null=(), force=0):
        rel, keep = ex._mixed_rel(d, None, None, "grouped")
        if fix:
            fix(rel)
        opts = H.GroupOpts()
        opts.struct_size = C.sizeof(H.GroupOpts) if struct_size is None else struct_size
        opts.want, opts.hash_bits, opts.reserved, opts.force_hashed = want, hash_bits, reserved, force
        if validity is not None:
            opts.validity = validity
        res = H.GroupResult()
        rc = L.hmj_group_mixed_device(h, None if "rel" in null else C.byref(rel), flags, None if "opts" in null else C.byref(opts),
                                      None if "out" in null else C.byref(res))
        del keep
        return rc, res, opts

    def good(**kw):
        rc, res, opts = call(want=all_want(H), **kw)
        assert rc == 0 and int(res.n_groups) == exp["n_groups"] == 21 and int(res.max_count) == exp["max_count"]
        assert opts.form == H.HMJ_COLS_HASHED and np.array_equal(by_first_row(ex.group_rows_to_numpy(res))["count"], exp["count"])

    def col_set(k, **fields):
        def fix(rel):
            for f, v in fields.items():
                setattr(rel.cols[k], f, v)
        return fix

    def rel_set(**fields):
        def fix(rel):
            for f, v in fields.items():
                setattr(rel, f, v)
        return fix

    good()
    bad = {
        "NULL rel": (dict(null=("rel",)), "grouped relation is NULL"), "NULL opts": (dict(null=("opts",)), "NULL"),
        "NULL out": (dict(null=("out",)), "NULL"),
        "HMJ_FIRST_WINS": (dict(flags=H.HMJ_MATERIALIZE | H.HMJ_FIRST_WINS), "HMJ_FIRST_WINS"),
        "HMJ_CHECKSUM": (dict(flags=H.HMJ_CHECKSUM), "HMJ_CHECKSUM"), "HMJ_SUM_PROBE": (dict(flags=H.HMJ_SUM_PROBE), "HMJ_SUM_PROBE"),
        "unknown want bit": (dict(want=0x20), "want"), "reserved": (dict(reserved=1), "reserved"),
        "struct_size": (dict(struct_size=H.GroupOpts.validity.offset + 4), "struct_size"), "struct_size 0": (dict(struct_size=0), "struct_size"),
        "hash_bits": (dict(hash_bits=64), "hash_bits"), "validity": (dict(validity=one_validity), "validity must be NULL"),
        "n_cols 0": (dict(fix=rel_set(n_cols=0)), "grouped relation: n_cols"), "n_cols 9": (dict(fix=rel_set(n_cols=9)), "n_cols"),
        "NULL cols": (dict(fix=rel_set(cols=None)), "grouped relation: cols is NULL"), "rel reserved": (dict(fix=rel_set(reserved=2)), "reserved"),
        "too many rows": (dict(fix=rel_set(n=1 << 32)), "grouped relation"), "width 3": (dict(fix=col_set(1, width=3)), "column 1 has width 3"),
        "unknown type": (dict(fix=col_set(0, type=7)), "column 0 has unknown type 7"),
        "string width": (dict(fix=col_set(0, width=8)), "string column has width"),
        "fixed offsets": (dict(fix=col_set(1, offsets=d[0][1].data_ptr())), "column 1"),
        "NULL offsets": (dict(fix=col_set(0, offsets=None)), "offsets is NULL"),
        "NULL fixed data": (dict(fix=col_set(1, data=None)), "grouped relation: column 1: data is NULL"),
        "misaligned": (dict(fix=col_set(1, data=d[1].data_ptr() + 4)), "aligned"),
    }
    for name, (kw, word) in bad.items():
        rc, _, _ = call(**kw)
        assert rc == HMJ_E_ARG, (name, rc)
        assert word in L.hmj_last_error(h).decode(), (name, L.hmj_last_error(h))
        good()
    good(flags=H.HMJ_MATERIALIZE | H.HMJ_NULL_EQUAL)  # implied: accepted and ignored
    good(force=1)  # ignored
    rc, res, opts = call(struct_size=H.GroupOpts.n_null.offset)  # a header that ends behind validity: no out field is written
    assert rc == 0 and int(res.n_groups) == 21 and opts.form == H.HMJ_COLS_HASHED and opts.n_null == 0
    res, info, got = group(H, ex, [[], np.zeros(0, np.uint32)], flags=H.HMJ_ORDERED)  # n == 0
    assert (int(res.n_groups), int(res.max_count), int(res.n_rows), info["form"]) == (0, 0, 0, H.HMJ_COLS_HASHED)
    assert all(got[k] is None for k in COLUMNS)


# ---- lifetime and neighbours ------------------------------------------------------------------------------------------------------
def test_take_through_first_row_is_the_distinct_table(H, ex):
    rng = np.random.default_rng(31)
    n = 900
    cols = draw_columns(rng, n, ["s", 4], 40)
    valid = draw_valid(rng, n, 2, 0.1, {0})
    d, dm = dev_cols(cols, base=3, first=2), dev_valid(H, valid, 3)
    res, info = ex.group_mixed_device(d, None, dm, H.HMJ_ORDERED, all_want(H))
    exp = H.expected_mixed_groups(cols, None, valid, ordered=True)
    ng = int(res.n_groups)
    assert ng == exp["n_groups"]
    before = ex.group_rows_to_numpy(res)
    chars, offs, words, tinfo = ex.take_str_device(d[0][0], d[0][1], (res.first_row, ng), valid=dm[0])
    outs, _, _ = ex.take_cols_device([d[1]], (res.first_row, ng))
    after = ex.group_rows_to_numpy(res)  # the group result survives both takes
    assert all(np.array_equal(before[k], after[k]) for k in COLUMNS)
    check(H, res, info, after, exp, True)
    first = exp["first_row"].astype(np.int64)
    want = [cols[0][f] if valid[0][f] else None for f in first]
    assert H.unpack_strings(chars, offs, H.unpack_validity(words, ng)) == want
    assert np.array_equal(outs[0].cpu().numpy().view(np.uint32), cols[1][first])
    assert tinfo["null_count"] == sum(w is None for w in want)


def test_a_group_call_between_two_u64_joins_changes_neither(H, ex):
    rng = np.random.default_rng(3)
    bd, pd = ex.gen_build(50000), ex.gen_probe(70000, 50000, miss_mod=3)
    cols = draw_columns(rng, 3000, ["s", 2, "s"], 100)
    fl = H.HMJ_ORDERED | H.HMJ_CHECKSUM
    r1 = ex.join_device(bd, pd, fl)
    c1, p1, rows1 = r1.checks(), ex.last_plan(), ex.columns_to_numpy(r1, host=False)
    run_and_check(H, ex, cols)
    assert ex.last_plan() == p1  # hmj_last_plan keeps describing the join
    r2 = ex.join_device(bd, pd, fl)
    assert r2.checks() == c1 and ex.last_plan()["path"] == p1["path"] and np.array_equal(ex.columns_to_numpy(r2, host=False), rows1)


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
        run_and_check(H, e, draw_columns(rng, 500, ["s", 4], 9))
        r = e.join_device(bd, pd, 0)
        t = e.last_timing()
        assert r.checks() == want and not (t["path"] & H.HMJ_PATH_PREPARED) and t["ms_partition_build"] > 0.0
    finally:
        e.close()


# ---- the sort's MSD form ----------------------------------------------------------------------------------------------------------
def test_the_msd_sort_path(H, ex):
    """2^22 + 3 rows (the u64 sort changes form from 2^22 rows on) of a (string, u32) key over 2^12 groups, every want bit.
    The tuple is an injective function of a group id, so numpy.unique on the ids is the reference, and key64 comes from
    `mixed_key64` on the 2^12 distinct tuples."""
    import torch

    rng = np.random.default_rng(22)
    n, G, W = (1 << 22) + 3, 1 << 12, 24
    pool = rng.integers(0, 256, size=(G, W), dtype=np.uint8)
    plen = rng.integers(8, W + 1, size=G)
    pool[:, :4] = np.arange(G, dtype="<u4").view(np.uint8).reshape(G, 4)  # distinct whatever the drawn bytes are
    gid = rng.integers(0, G, size=n)
    lens = plen[gid]
    off = np.zeros(n + 1, np.int64)
    np.cumsum(lens, out=off[1:])
    chars = pool[gid][np.arange(W)[None, :] < lens[:, None]]
    num = ((gid.astype(np.uint64) * np.uint64(7919)) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    vals = rng.integers(0, 1 << 64, size=n, dtype=np.uint64)
    d = [(torch.from_numpy(chars).cuda(), torch.from_numpy(off).cuda()), torch.from_numpy(num.view(np.int32)).cuda()]
    res, info = ex.group_mixed_device(d, dev_vals(vals), None, H.HMJ_MATERIALIZE, all_want(H))
    got = ex.group_rows_to_numpy(res)
    _, first, inv, count = np.unique(gid, return_index=True, return_inverse=True, return_counts=True)
    order = np.argsort(first, kind="stable")
    rank = np.empty(len(first), np.int64)
    rank[order] = np.arange(len(first))
    g_of_row = rank[inv.reshape(-1)]
    by_group = np.argsort(g_of_row, kind="stable")
    starts = np.concatenate([[0], np.cumsum(count[order])[:-1]]).astype(np.int64)
    sp = vals[by_group]
    assert int(res.n_groups) == len(first) and int(res.max_count) == int(count.max()) and info["n_collisions"] == 0
    cmp = by_first_row(got)
    f = first[order]
    key_of_gid = H.mixed_key64([[pool[g, :plen[g]].tobytes() for g in range(G)], ((np.arange(G, dtype=np.uint64) * np.uint64(7919))
                                                                                   & np.uint64(0xFFFFFFFF)).astype(np.uint32)])
    assert np.array_equal(cmp["first_row"], f.astype(np.uint64))
    assert np.array_equal(cmp["key64"], key_of_gid[gid[f]])
    assert np.array_equal(cmp["count"], count[order].astype(np.uint64))
    assert np.array_equal(cmp["sum"], np.add.reduceat(sp, starts))
    assert np.array_equal(cmp["min"], np.minimum.reduceat(sp, starts)) and np.array_equal(cmp["max"], np.maximum.reduceat(sp, starts))
    assert np.array_equal(cmp["group_of_row"], g_of_row.astype(np.uint64))


# ---- randomized sweep -------------------------------------------------------------------------------------------------------------
def test_randomized_sweep(H, ex):
    seed, iters = sweep_params()
    rng = np.random.default_rng(seed)
    skipped = 0
    for it in range(iters):
        case = draw_case(rng)
        tag = (seed, it, case["n"], case["shape"], case["hash_bits"])
        if exceeds_run_cap(H, case):
            skipped += 1
            with pytest.raises(H.HmjError) as e:
                group(H, ex, case["cols"], case["vals"], case["valid"], offset=case["offset"], hash_bits=case["hash_bits"])
            assert e.value.code == HMJ_E_UNSUPPORTED, tag
            continue
        run_and_check(H, ex, case["cols"], case["vals"], case["valid"], case["ordered"], tag, case["offset"], case["hash_bits"])
    assert skipped * 30 <= SWEEP_MAX_SKIPS * iters, (skipped, iters)
