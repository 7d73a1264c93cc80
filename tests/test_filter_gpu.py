"""hmj_filter_device on the GPU (include/hmj.h, "filtering rows: typed and string predicates to a row map") against
`expected_filter`: the map is compared entry by entry, n_out and n_unknown exactly, the mask -- where asked for -- bit by bit
with its padding, and every entry of the output buffer at and behind n_out must still hold the sentinel put there."""
import ctypes as C
import functools

import numpy as np
import pytest

from test_filter_cpu import (BETWEEN, ENDS_WITH, EQ, GE, GT, IS_NOT_NULL, IS_NULL, LE, LT, NE, NO_ROW, STARTS_WITH, draw_filter_case,
                             mixed_tables, string_tables, sweep_params, term, truth_table_cases, typed_tables)
from test_join_cols_kinds_cpu import ANTI, BUILD, FULL_OUTER, PROBE
from test_order_by_cpu import DTYPES

pytestmark = pytest.mark.gpu
HMJ_E_ARG = -1
SENTINEL = -0x0123456789ABCDEF
# filter.hip: a workgroup covers 256 positions and has one slot; a workgroup of the slots' scan covers 256 * 8 = 2048 slots.
# From 2048 * 256 + 1 positions on the scan spans two of its own workgroups; this size puts 2 slots and a ragged wave there.
SCAN_TILE_POSITIONS = 2048 * 256
SCAN_SPANS_TWO = SCAN_TILE_POSITIONS + 257
SIZES = [0, 1, 2, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, SCAN_SPANS_TWO]


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


def dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()


def dev_strings(values, pad):
    """A string column on the device: the chars start `pad` bytes into the buffer (offsets[0] == pad); the bytes of a NULL
    slot stay where they are: garbage under it."""
    enc = [b"" if v is None else bytes(v) for v in values]
    lens = np.fromiter((len(b) for b in enc), dtype=np.int64, count=len(enc))
    offsets = np.full(len(enc) + 1, pad, np.int64)
    offsets[1:] += np.cumsum(lens)
    raw = b"\xee" * pad + b"".join(enc)
    return (dev(np.frombuffer(raw, np.uint8)) if raw else None, dev(offsets))


def dev_terms(H, terms):
    """Host terms (test_filter_cpu) as Executor.filter_device takes them.  One host object is one device tensor, so terms that
    share a map share its pointer."""
    cache = {}

    def once(key, make):
        if key not in cache:
            cache[key] = make()
        return cache[key]

    out = []
    for t in terms:
        col, valid, rm = t["column"], t["valid"], t["row_map"]
        if isinstance(col, np.ndarray):
            d = once(("c", id(col)), lambda: dev(col))
        else:
            d = once(("s", id(col), t["pad"]), lambda: dev_strings(col, t["pad"]))
        dv = None if valid is None else once(("v", id(valid), t["bit_offset"]), lambda: H.pack_validity(valid, t["bit_offset"], device="cuda"))
        dm = None if rm is None else once(("m", id(rm)), lambda: dev(np.asarray(rm, np.uint64).view(np.int64)))
        out.append({"column": d, "op": t["op"], "lit": t["lit"], "valid": dv, "bit_offset": t["bit_offset"], "row_map": dm,
                    "clause": t["clause"], "negate": t["negate"]})
    return out


def run(ex, terms, n, want_mask):
    """One call on device terms into a buffer of n + 1 sentinels: (map, mask bits or None, info)."""
    import torch

    out = torch.full((n + 1,), SENTINEL, dtype=torch.int64, device="cuda")
    got, words, info = ex.filter_device(terms, n=n, want_mask=want_mask, out=out)
    assert got.shape[0] == info["n_out"]
    tail = out[info["n_out"]:].cpu().numpy()
    assert np.all(tail == SENTINEL), "an entry at or behind n_out was written (first at +%d)" % int(np.nonzero(tail != SENTINEL)[0][0])
    bits = None
    if want_mask:
        assert words.shape[0] == (n + 63) // 64
        bits = np.unpackbits(words.cpu().numpy().view(np.uint8), bitorder="little")
    return got.cpu().numpy().view(np.uint64), bits, info


def check(ex, H, terms, n, tag="", masks=(True,)):
    want, unknown = H.expected_filter(terms, n)
    d = dev_terms(H, terms)
    for want_mask in masks:
        got, bits, info = run(ex, d, n, want_mask)
        assert info["n_out"] == len(want) and info["n_unknown"] == unknown, (tag, info, len(want), unknown)
        if not np.array_equal(got, want):
            bad = int(np.nonzero(got != want)[0][0])
            raise AssertionError("%s: the map differs from entry %d on: got %d, want %d" % (tag, bad, got[bad], want[bad]))
        if want_mask:
            exp = np.zeros(64 * ((n + 63) // 64), np.uint8)
            exp[want.astype(np.int64)] = 1
            assert np.array_equal(bits, exp), "%s: the mask differs from the map (or its padding is not 0)" % tag
    return want, unknown


# ---- sizes ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_boundary_sizes_in_five_patterns_with_and_without_a_mask(ex, H, n):
    assert SCAN_SPANS_TWO > SCAN_TILE_POSITIONS and (SCAN_SPANS_TWO + 255) // 256 > 2048
    patterns = {"all": np.ones(n, np.int32), "none": np.zeros(n, np.int32), "alternating": (np.arange(n) & 1).astype(np.int32),
                "last": np.zeros(n, np.int32), "first": np.zeros(n, np.int32)}
    if n:
        patterns["last"][-1] = 1
        patterns["first"][0] = 1
    for name, x in patterns.items():
        want, unknown = check(ex, H, [term(x, EQ, 1)], n, "%s n=%d" % (name, n), masks=(True, False))
        assert len(want) == int(x.sum()) and unknown == 0


def test_unknown_positions_are_counted_across_scan_workgroups(ex, H):
    n = SCAN_SPANS_TWO
    rng = np.random.default_rng(3)
    x = rng.integers(0, 3, size=n).astype(np.uint8)
    valid = rng.random(n) >= 0.3
    want, unknown = check(ex, H, [term(x, GE, 1, valid, 7)], n, "unknowns")
    assert unknown == int((~valid).sum()) and 0 < len(want) < n


# ---- every type x every op -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_every_op_on_every_type_around_its_edge_values(ex, H, dtype):
    tables = typed_tables(dtype)
    assert {t[2][0]["op"] for t in tables} == set(range(9))
    hits = 0
    for tag, n, terms in tables:
        want, _ = check(ex, H, terms, n, tag)
        hits += len(want) > 0
    assert hits > len(tables) // 3


def test_between_with_lo_above_hi_selects_nothing_and_signedness_holds(ex, H):
    i8 = np.array([-1, 1, 0, -128, 127], np.int8)
    want, _ = check(ex, H, [term(i8, LT, 1)], 5, "int8 -1 < 1")
    assert [int(p) for p in want] == [0, 2, 3]
    u64 = np.array([1 << 63, (1 << 63) - 1, 0, (1 << 64) - 1], np.uint64)
    want, _ = check(ex, H, [term(u64, GE, 1 << 63)], 4, "uint64 2^63")
    assert [int(p) for p in want] == [0, 3]
    i64 = np.array([-(1 << 63), (1 << 63) - 1, 0], np.int64)
    want, _ = check(ex, H, [term(i64, GT, -(1 << 63))], 3, "int64 min")
    assert [int(p) for p in want] == [1, 2]
    want, _ = check(ex, H, [term(i64, BETWEEN, (5, -5))], 3, "lo > hi")
    assert len(want) == 0
    f = np.array([0.0, -0.0, np.nan, np.inf, -np.inf, 5e-324], np.float64)
    want, _ = check(ex, H, [term(f, EQ, 0.0)], 6, "both zeros")
    assert [int(p) for p in want] == [0, 1]
    want, _ = check(ex, H, [term(f, NE, float("nan"))], 6, "ne nan")
    assert len(want) == 6
    want, _ = check(ex, H, [term(f, LE, float("nan"))], 6, "le nan")
    assert len(want) == 0


@pytest.mark.parametrize("case", truth_table_cases(), ids=[c[0] for c in truth_table_cases()])
def test_the_three_valued_truth_table(ex, H, case):
    tag, n, terms = case
    check(ex, H, terms, n, tag)


# ---- strings -------------------------------------------------------------------------------------------------------------------
def test_every_op_on_strings_around_their_edges(ex, H):
    tables = string_tables()
    assert {t[2][0]["op"] for t in tables} == set(range(11))
    for tag, n, terms in tables:
        check(ex, H, terms, n, tag)


def test_strings_null_against_empty_and_prefixes(ex, H):
    vals = [b"", b"", b"abc", b"abcd", b"abcde", b"\x80", b"a\x00"]
    valid = np.array([True, False, True, True, True, True, True])
    for op, lit, rows in ((EQ, b"", [0]), (STARTS_WITH, b"", [0, 2, 3, 4, 5, 6]), (ENDS_WITH, b"", [0, 2, 3, 4, 5, 6]), (IS_NULL, None, [1]),
                          (STARTS_WITH, b"abcd", [3, 4]), (LT, b"abcd", [0, 2, 6]), (GT, b"abcd", [4, 5]), (ENDS_WITH, b"cd", [3]),
                          (GE, b"\x7f\xff", [5]), (EQ, b"a\x00", [6]), (NE, b"abcd", [0, 2, 4, 5, 6])):
        want, unknown = check(ex, H, [term(vals, op, lit, valid, 1, pad=3)], len(vals), "op %d %r" % (op, lit))
        assert [int(p) for p in want] == rows and unknown == (0 if op == IS_NULL else 1)


def test_garbage_offsets_and_bytes_under_null_slots_are_never_followed(ex, H):
    """Runs of NULL rows whose inner offsets are garbage (huge, decreasing) and whose bytes are not what the reference
    holds: the call neither faults nor reports them, and the result is the reference's."""
    rng = np.random.default_rng(12)
    n = 700
    vals = [bytes(rng.integers(0x61, 0x64, size=int(rng.integers(0, 12))).astype(np.uint8)) for _ in range(n)]
    valid = np.ones(n, bool)
    for start in rng.integers(0, n - 4, size=40):
        valid[start:start + 3] = False
    chars, offsets = dev_strings(vals, 5)
    off = offsets.cpu().numpy().copy()
    inner = np.nonzero(~valid[:-1] & ~valid[1:])[0] + 1  # offsets[r + 1] between two NULL rows: read by neither neighbour's valid row
    assert len(inner) > 40
    off[inner] = np.where(np.arange(len(inner)) & 1, np.int64(1) << 62, np.int64(-5))
    dv = H.pack_validity(valid, 9, device="cuda")
    for op, lit in ((EQ, b"ab"), (LT, b"b"), (STARTS_WITH, b"a"), (ENDS_WITH, b"c"), (IS_NULL, None)):
        want, unknown = H.expected_filter([term(vals, op, lit, valid)], n)
        got, _, info = run(ex, [{"column": (chars, dev(off)), "op": op, "lit": lit, "valid": dv, "bit_offset": 9}], n, True)
        assert np.array_equal(got, want) and info["n_unknown"] == unknown, op


# ---- validity and maps ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bit_offset", [0, 1, 7, 63, 69])
def test_validity_at_bit_offsets(ex, H, bit_offset):
    rng = np.random.default_rng(40 + bit_offset)
    n = 1000
    x = rng.integers(-3, 4, size=n).astype(np.int16)
    valid = rng.random(n) >= 0.4
    strs = [[b"p", b"pq", b""][k] for k in rng.integers(0, 3, size=n)]
    for terms in ([term(x, LE, 0, valid, bit_offset)], [term(x, IS_NULL, None, valid, bit_offset)],
                  [term(strs, STARTS_WITH, b"p", valid, bit_offset, negate=True)],
                  [term(x, GT, 0, valid, bit_offset), term(strs, IS_NOT_NULL, None, ~valid, bit_offset, clause=1)]):
        check(ex, H, terms, n, "bit_offset %d" % bit_offset)


def test_maps_identity_permutation_duplicates_and_no_row(ex, H):
    rng = np.random.default_rng(50)
    ns, n = 500, 1300
    x = rng.integers(0, 10, size=ns).astype(np.uint32)
    valid = rng.random(ns) >= 0.2
    ident = np.arange(ns, dtype=np.uint64)
    perm = rng.permutation(ns).astype(np.uint64)
    dups = rng.integers(0, 7, size=n).astype(np.uint64)
    holes = rng.integers(0, ns, size=n).astype(np.uint64)
    holes[rng.random(n) < 0.3] = NO_ROW
    direct, _ = check(ex, H, [term(x, LT, 5, valid)], ns, "direct")
    through, _ = check(ex, H, [term(x, LT, 5, valid, row_map=ident)], ns, "identity")
    assert np.array_equal(direct, through)
    check(ex, H, [term(x, LT, 5, valid, row_map=perm)], ns, "permutation")
    check(ex, H, [term(x, LT, 5, valid, row_map=dups)], n, "duplicates")
    want, unknown = check(ex, H, [term(x, IS_NULL, None, None, row_map=holes)], n, "no-row is null")
    assert np.array_equal(want, np.nonzero(holes == NO_ROW)[0].astype(np.uint64)) and unknown == 0
    want, unknown = check(ex, H, [term(x, GE, 0, None, row_map=holes)], n, "no-row is unknown")
    assert unknown == int((holes == NO_ROW).sum()) and len(want) == n - unknown
    all_gone = np.full(64, NO_ROW, np.uint64)
    want, unknown = check(ex, H, [term(x[:0], EQ, 1, row_map=all_gone)], 64, "n_src 0")
    assert len(want) == 0 and unknown == 64


def test_hand_made_predicates_over_several_maps(ex, H):
    for tag, n, terms in mixed_tables():
        check(ex, H, terms, n, tag, masks=(True, False))


def test_more_distinct_maps_than_register_slots(ex, H):
    """Seven maps over seven relations in one call: the fifth and later maps are loaded by the terms that name them."""
    rng = np.random.default_rng(60)
    n = 2000
    terms = []
    for k in range(7):
        ns = 100 + 37 * k
        m = rng.integers(0, ns, size=n).astype(np.uint64)
        m[rng.random(n) < 0.1] = NO_ROW
        col = rng.integers(0, 4, size=ns).astype([np.int8, np.uint16, np.int64, np.float32][k % 4])
        terms.append(term(col, NE, k % 4, row_map=m, clause=k // 2))
        if k % 3 == 0:
            terms.append(term(col, IS_NULL, None, row_map=m, clause=k // 2))
    want, unknown = check(ex, H, terms, n, "seven maps")
    assert 0 < len(want) < n


# ---- errors found on the device ------------------------------------------------------------------------------------------------
def test_device_found_errors_leave_the_ctx_usable(ex, H):
    rng = np.random.default_rng(70)
    n, ns = 3000, 400
    x = rng.integers(0, 5, size=ns).astype(np.int32)
    good_map = rng.integers(0, ns, size=n).astype(np.uint64)
    bad_map = good_map.copy()
    bad_map[[5, 777, 2999]] = [ns, 1 << 40, NO_ROW - 1]
    good = [term(x, EQ, 1, row_map=good_map)]
    with pytest.raises(H.HmjError) as e:
        run(ex, dev_terms(H, [term(x, EQ, 1, row_map=bad_map)]), n, True)
    assert e.value.code == HMJ_E_ARG and "3 row_map entries are >= n_src" in str(e.value)
    check(ex, H, good, n, "after a bad map")

    vals = [b"abc"] * ns
    chars, offsets = dev_strings(vals, 0)
    off = offsets.cpu().numpy().copy()
    dec = off.copy()
    dec[[11, 200]] = [0, 3]  # rows 10 and 199 end before they start (row 11 and 200 stay well-formed: they start lower)
    with pytest.raises(H.HmjError) as e:
        run(ex, [{"column": (chars, dev(dec)), "op": EQ, "lit": b"abc", "row_map": dev(good_map.view(np.int64))}], n, False)
    n_dec = int(np.isin(good_map, [10, 199]).sum())
    assert n_dec > 0 and e.value.code == HMJ_E_ARG and "(%d with offsets[r + 1] < offsets[r], 0 that end" % n_dec in str(e.value)
    check(ex, H, good, n, "after decreasing offsets")

    far = off.copy()
    far[ns] = 3 * ns + 1  # the last row ends one byte behind chars_bytes
    with pytest.raises(H.HmjError) as e:
        run(ex, [{"column": (chars, dev(far)), "op": STARTS_WITH, "lit": b"a"}], ns, True)
    assert e.value.code == HMJ_E_ARG and "1 read rows have bad string offsets (0 with" in str(e.value) and "1 that end behind" in str(e.value)
    # the same offsets under a NULL slot are not read: no error
    valid = np.ones(ns, bool)
    valid[ns - 1] = False
    got, _, info = run(ex, [{"column": (chars, dev(far)), "op": STARTS_WITH, "lit": b"a", "valid": H.pack_validity(valid, 0, device="cuda")}],
                       ns, True)
    assert info["n_out"] == ns - 1 and info["n_unknown"] == 1
    check(ex, H, good, n, "after an offset behind chars_bytes")


# ---- the host refusals ---------------------------------------------------------------------------------------------------------
def test_host_refusals(ex, H):
    import torch

    L = ex.L
    n = 128
    data = torch.zeros(n, dtype=torch.int64, device="cuda")
    chars = torch.zeros(4 * n, dtype=torch.uint8, device="cuda")
    offsets = torch.arange(n + 1, dtype=torch.int64, device="cuda") * 4
    bits = torch.full((n // 8 + 16,), 255, dtype=torch.uint8, device="cuda")
    rmap = torch.zeros(n, dtype=torch.int64, device="cuda")
    out = torch.zeros(n, dtype=torch.int64, device="cuda")
    mask = torch.zeros(n // 64, dtype=torch.int64, device="cuda")
    lit_buf = C.create_string_buffer(b"x" * 5000)

    def fixed():
        t = H.FilterTerm()
        t.type, t.op, t.data, t.n_src = H.HMJ_TYPE_I32, H.HMJ_FILTER_EQ, data.data_ptr(), n
        return t

    def string():
        t = H.FilterTerm()
        t.type, t.op, t.data, t.offsets, t.chars_bytes, t.n_src = H.HMJ_FILTER_LARGE_STRING, H.HMJ_FILTER_EQ, chars.data_ptr(), offsets.data_ptr(), 4 * n, n
        t.str_lit[0], t.str_len[0] = C.addressof(lit_buf), 4
        return t

    def call(terms, n_terms=None, nn=n, o=out.data_ptr(), m=mask.data_ptr(), opts="default", terms_null=False):
        arr = (H.FilterTerm * max(len(terms), 1))(*terms)
        if opts == "default":
            opts = H.FilterOpts()
            opts.struct_size = C.sizeof(H.FilterOpts)
        rc = L.hmj_filter_device(ex.h, None if terms_null else arr, len(terms) if n_terms is None else n_terms, nn, o, m,
                                 None if opts is None else C.byref(opts))
        return rc, L.hmj_last_error(ex.h).decode()

    def refused(what, *a, **kw):
        rc, msg = call(*a, **kw)
        assert rc == HMJ_E_ARG and msg, what

    def mutated(make, **fields):
        t = make()
        for k, v in fields.items():
            if k in ("bits", "bit_offset"):
                setattr(t.validity, k, v)
            else:
                setattr(t, k, v)
        return [t]

    assert call([fixed()])[0] == 0 and call([string()])[0] == 0  # the baselines are good calls
    refused("terms NULL", [fixed()], terms_null=True)
    refused("opts NULL", [fixed()], opts=None)
    refused("no terms", [fixed()], n_terms=0)
    refused("17 terms", [fixed()] * 17)
    refused("unknown type 10", mutated(fixed, type=10))
    refused("unknown type 17", mutated(fixed, type=17))
    refused("unknown op", mutated(fixed, op=11))
    refused("unknown flag bits", mutated(fixed, flags=2))
    refused("STARTS_WITH on a fixed column", mutated(fixed, op=H.HMJ_FILTER_STARTS_WITH))
    refused("ENDS_WITH on a fixed column", mutated(fixed, op=H.HMJ_FILTER_ENDS_WITH))
    refused("decreasing clause ids", mutated(fixed, clause=3) + [fixed()])
    refused("a term's reserved", mutated(fixed, reserved=1))
    for field in ("reserved", "reserved2"):
        o = H.FilterOpts()
        o.struct_size = C.sizeof(H.FilterOpts)
        setattr(o, field, 1)
        refused("opts." + field, [fixed()], opts=o)
    o = H.FilterOpts()
    o.struct_size = H.FilterOpts.reserved2.offset
    refused("a short struct_size", [fixed()], opts=o)
    refused("data NULL", mutated(fixed, data=None))
    refused("data misaligned", mutated(fixed, data=data.data_ptr() + 2))
    refused("offsets on a fixed column", mutated(fixed, offsets=offsets.data_ptr()))
    refused("offsets NULL", mutated(string, offsets=None))
    refused("offsets misaligned", mutated(string, offsets=offsets.data_ptr() + 4))
    refused("chars NULL with chars_bytes", mutated(string, data=None))
    refused("row_map misaligned", mutated(fixed, row_map=rmap.data_ptr() + 4))
    refused("row_map_out NULL", [fixed()], o=None)
    refused("row_map_out misaligned", [fixed()], o=out.data_ptr() + 4)
    refused("mask_out misaligned", [fixed()], m=mask.data_ptr() + 4)
    refused("bit_offset + n_src overflows", mutated(fixed, bits=bits.data_ptr(), bit_offset=(1 << 64) - n))
    refused("n above 2^32 - 1", mutated(fixed, row_map=rmap.data_ptr()), nn=1 << 32)
    refused("n_src above 2^32 - 1", mutated(fixed, n_src=1 << 32))
    refused("n_src < n without a map", mutated(fixed, n_src=n - 1))
    t = fixed()
    t.lit[0] = 1 << 32
    refused("a literal that does not fit 4 bytes", [t])
    t = mutated(fixed, type=H.HMJ_TYPE_I8, op=H.HMJ_FILTER_BETWEEN)[0]
    t.lit[0], t.lit[1] = 0xFF, 0x100
    refused("BETWEEN's upper literal does not fit 1 byte", [t])
    t = string()
    t.str_len[0] = 4097
    refused("literal bytes over the cap", [t])
    a, b = string(), string()
    a.str_len[0], b.str_len[0] = 2048, 2049
    refused("literal bytes over the cap in two terms", [a, b])
    t = string()
    t.str_lit[0] = None
    refused("a NULL literal with a length", [t])
    refused("the map overlaps the column", [fixed()], o=data.data_ptr())
    refused("the mask overlaps the column", [fixed()], m=data.data_ptr() + 64)
    refused("the map overlaps the mask", [fixed()], m=out.data_ptr() + 8)
    refused("the map overlaps a term's row_map", mutated(fixed, row_map=out.data_ptr()))
    refused("the mask overlaps the offsets", [string()], m=offsets.data_ptr() + 16)
    refused("the mask overlaps the bitmap", mutated(fixed, bits=mask.data_ptr()))
    refused("the map overlaps the chars", [string()], o=chars.data_ptr())
    # n == 0: HMJ_OK, nothing is looked at that only n > 0 needs, nothing is written
    rc, _ = call(mutated(fixed, data=None, n_src=0), nn=0, o=None, m=None)
    assert rc == 0
    assert call([fixed()])[0] == 0  # and the ctx still works


# ---- the randomized sweep ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def sweep_cases():
    seed, iters = sweep_params()
    rng = np.random.default_rng(seed)
    return [draw_filter_case(rng, it) for it in range(iters)]


@pytest.mark.parametrize("it", range(sweep_params()[1]))
def test_randomized_sweep(ex, H, it):
    case = sweep_cases()[it]
    check(ex, H, case["terms"], case["n"], "seed %d case %d" % (sweep_params()[0], it), masks=(bool(it & 1),))


# ---- pipelines -----------------------------------------------------------------------------------------------------------------
def test_full_outer_join_where_the_partner_is_null(ex, H):
    """`R FULL OUTER JOIN S WHERE s.key IS NULL` through s_row: the rows of R without a partner, as many as the probe-side
    ANTI join of R against S returns; and `r.key IS NULL` through r_row likewise for S against R."""
    rng = np.random.default_rng(80)
    nr, ns = 3000, 4000
    rk = [dev(rng.integers(0, 2500, size=nr).astype(np.int32)), dev(rng.integers(0, 3, size=nr).astype(np.int16))]
    sk = [dev(rng.integers(0, 2500, size=ns).astype(np.int32)), dev(rng.integers(0, 3, size=ns).astype(np.int16))]
    _, anti_r = ex.join_kind_cols_device(sk, None, rk, None, PROBE, ANTI, H.HMJ_MATERIALIZE)  # R probes S
    _, anti_s = ex.join_kind_cols_device(rk, None, sk, None, PROBE, ANTI, H.HMJ_MATERIALIZE)  # S probes R
    res, info = ex.join_kind_cols_device(rk, None, sk, None, BUILD, FULL_OUTER, H.HMJ_MATERIALIZE)
    n = int(res.n_matches)
    rows = ex.cols_kind_rows_to_numpy(res)
    s_null, _, i1 = ex.filter_device([{"column": sk[0], "op": IS_NULL, "row_map": (res.s_row, n)}], n=n)
    r_null, _, i2 = ex.filter_device([{"column": rk[0], "op": IS_NULL, "row_map": (res.r_row, n)}], n=n)
    assert i1["n_out"] == anti_r["n_probe_unmatched"] == info["n_build_unmatched"] > 0
    assert i2["n_out"] == anti_s["n_probe_unmatched"] == info["n_probe_unmatched"] > 0
    assert np.array_equal(s_null.cpu().numpy().view(np.uint64), np.nonzero(rows[:, 2] == NO_ROW)[0].astype(np.uint64))
    assert np.array_equal(r_null.cpu().numpy().view(np.uint64), np.nonzero(rows[:, 1] == NO_ROW)[0].astype(np.uint64))
    # a predicate over both sides in one call: r.k0 < 1000 AND (s.k1 = 2 OR s.key IS NULL)
    both, _, i3 = ex.filter_device([{"column": rk[0], "op": LT, "lit": 1000, "row_map": (res.r_row, n)},
                                    {"column": sk[1], "op": EQ, "lit": 2, "row_map": (res.s_row, n), "clause": 1},
                                    {"column": sk[1], "op": IS_NULL, "row_map": (res.s_row, n), "clause": 1}], n=n)
    want, unknown = H.expected_filter([term(rk[0].cpu().numpy(), LT, 1000, row_map=rows[:, 1].copy()),
                                       term(sk[1].cpu().numpy(), EQ, 2, row_map=rows[:, 2].copy(), clause=1),
                                       term(sk[1].cpu().numpy(), IS_NULL, None, row_map=rows[:, 2].copy(), clause=1)], n)
    assert np.array_equal(both.cpu().numpy().view(np.uint64), want) and i3["n_unknown"] == unknown
    assert np.array_equal(ex.cols_kind_rows_to_numpy(res), rows)  # the result is still there


def test_filter_take_group_equals_grouping_the_filtered_rows(ex, H):
    rng = np.random.default_rng(81)
    n = 5000
    a = rng.integers(0, 30, size=n).astype(np.int32)
    b = rng.integers(0, 4, size=n).astype(np.uint16)
    price = (rng.standard_normal(n) * 50).astype(np.float64)
    pvalid = rng.random(n) >= 0.1
    terms = [term(price, BETWEEN, (-20.0, 60.0), pvalid, 3), term(b, NE, 2, clause=1)]
    keep, _ = H.expected_filter(terms, n)
    rmap, _, info = ex.filter_device(dev_terms(H, terms), n=n)
    assert info["n_out"] == len(keep) > 0
    da, db = dev(a), dev(b)
    outs, _, _ = ex.take_cols_device([da, db], rmap, want_validity=False)
    res, _ = ex.group_cols_device(outs, None, None, H.HMJ_ORDERED, H.HMJ_GROUP_COUNT)
    got = ex.group_rows_to_numpy(res)
    idx = keep.astype(np.int64)
    exp = H.expected_groups([a[idx], b[idx]], [4, 2], ordered=True)
    assert int(res.n_groups) == exp["n_groups"]
    for k in ("key64", "first_row", "count"):
        assert np.array_equal(got[k], exp[k]), k
    # the live grouping survives a filter call
    ex.filter_device(dev_terms(H, terms), n=n)
    again = ex.group_rows_to_numpy(res)
    assert np.array_equal(again["count"], exp["count"])


# ---- context -------------------------------------------------------------------------------------------------------------------
def test_a_filter_between_a_join_and_its_take_keeps_the_result(ex, H):
    rng = np.random.default_rng(82)
    nb, npr = 2000, 6000
    bk, pk = rng.permutation(5000)[:nb].astype(np.int64), rng.integers(0, 5000, size=npr).astype(np.int64)
    bpay = rng.integers(-100, 100, size=nb).astype(np.int32)
    dbk, dpk, dpay = dev(bk), dev(pk), dev(bpay)
    res, _ = ex.join_cols_device([dbk], None, [dpk], None, H.HMJ_MATERIALIZE)
    n = int(res.n_matches)
    before = ex.cols_rows_to_numpy(res)
    rmap, words, info = ex.filter_device([{"column": dpay, "op": GE, "lit": 0, "row_map": (res.r_row, n)}], n=n, want_mask=True)
    want = np.nonzero(bpay[before[:, 1].astype(np.int64)] >= 0)[0].astype(np.uint64)
    assert np.array_equal(rmap.cpu().numpy().view(np.uint64), want) and 0 < len(want) < n
    outs, _, _ = ex.take_cols_device([dpay], (res.r_row, n), want_validity=False)
    assert np.array_equal(outs[0].cpu().numpy(), bpay[before[:, 1].astype(np.int64)])
    assert np.array_equal(ex.cols_rows_to_numpy(res), before)


def test_a_filter_keeps_a_prepared_build_side(H):
    """Between hmj_prepare_build_u64_device and the join: the join still runs on HMJ_PATH_PREPARED."""
    e = H.Executor(0)
    try:
        nb, npb = 300000, 200000
        B, P = e.gen_build(nb), e.gen_probe(npb, nb, miss_mod=4)
        x = np.arange(5000, dtype=np.int32)
        e.set_profiling(True)
        e.prepare_build(B, npb)
        r = e.join_device(B, P, 0)
        want = int(r.n_matches)
        assert e.last_timing()["path"] & H.HMJ_PATH_PREPARED  # (the control: this shape does reuse a prepared build side)
        e.prepare_build(B, npb)
        plan, timing = e.last_plan(), e.last_timing()
        rmap, _, info = e.filter_device([{"column": dev(x), "op": LT, "lit": 100}])
        assert info["n_out"] == 100 and info["ms_eval"] > 0.0 and info["ms_write"] > 0.0  # (profiling is on)
        assert e.last_plan() == plan and e.last_timing() == timing  # hmj_last_plan / hmj_last_timing are as they were
        r = e.join_device(B, P, 0)
        assert int(r.n_matches) == want and e.last_timing()["path"] & H.HMJ_PATH_PREPARED
    finally:
        e.close()
