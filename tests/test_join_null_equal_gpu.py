"""GPU checks of NULL-equals-NULL matching (HMJ_NULL_EQUAL) in hmj_join_kind_cols_device and hmj_join_mixed_device against
`ne_rows` (test_join_null_equal_cpu.py: a brute force over tuples in which NULL is a token of its own) with `cols_key64` /
`mixed_key64` (null_equal=True, pinned there) for key64: all eight kinds in four modes over row counts around the wave and
workgroup edges, bitmaps on one side / some columns / at bit offsets, all-NULL columns and relations, forced key64
collisions through the ambiguous list and the collision sort, the calls the flag must agree with, independence of what
lies under a NULL slot, SQL semantics without the flag, and the argument errors."""
import random

import numpy as np
import pytest

from test_join_cols_gpu import unordered
from test_join_cols_kinds_cpu import (ALL_KINDS, ANTI, BUILD, BUILD_OUTER, COUNT_KEYS, FULL_OUTER, INNER, M64, NO_ROW, PROBE, PROBE_OUTER, SEMI,
                                      kind_checks)
from test_join_null_equal_cpu import ne_rows

pytestmark = pytest.mark.gpu
HMJ_E_ARG = -1
PFILL, BFILL = 0xF1, 2 ** 64 - 2
NULL_FRAC = 0.3
# (build rows, probe rows): one row, one short of / exactly / one past a wave, past a workgroup, several workgroups
SIZE_PAIRS = [(1, 65), (63, 257), (64, 1), (65, 300), (257, 64), (300, 63), (1000, 1000)]
COL_LAYOUTS = {"u32": [4], "u32x2": [4, 4], "u64_u32_u16": [8, 4, 2], "u8x8": [1] * 8}  # u8x8: mask bit 7 is used
MIX_LAYOUTS = {"str": ["s"], "str_u32": ["s", 4], "u32_str_str": [4, "s", "s"]}


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


def all_modes(H):
    """count, materialise, ordered, and the count mode with checksums and the probe sum"""
    return (0, H.HMJ_MATERIALIZE | H.HMJ_CHECKSUM, H.HMJ_ORDERED | H.HMJ_CHECKSUM | H.HMJ_SUM_PROBE, H.HMJ_CHECKSUM | H.HMJ_SUM_PROBE)


def modes2(H):
    return (H.HMJ_ORDERED | H.HMJ_CHECKSUM | H.HMJ_SUM_PROBE, H.HMJ_CHECKSUM | H.HMJ_SUM_PROBE)


# ---- relations on the host ---------------------------------------------------------------------------------------------------
class Rel:
    """layout: per key column a width in bytes or "s" (a string column); rows: the key tuples, None in a NULL slot; bitmap:
    the columns that get a validity bitmap (None: every column that holds a NULL; a column outside it holds none); vals:
    None (the payload of row i is i) or a list of ints."""

    def __init__(self, layout, rows, vals=None, bitmap=None):
        self.layout, self.rows, self.vals, self.n = layout, rows, vals, len(rows)
        has_null = [any(t[c] is None for t in rows) for c in range(len(layout))]
        self.bitmap = [c for c, h in enumerate(has_null) if h] if bitmap is None else list(bitmap)
        assert all(c in self.bitmap for c, h in enumerate(has_null) if h)

    def masks(self):
        """per column None or a bool array, True = valid"""
        return [np.array([t[c] is not None for t in self.rows], bool) if c in self.bitmap else None for c in range(len(self.layout))]

    def columns(self, rng=None):
        """The columns as they go to the device.  Under a NULL slot: zeros / no bytes (rng None), or whatever rng draws."""
        cols = []
        for c, typ in enumerate(self.layout):
            if typ == "s":
                junk = (lambda: bytes(rng.getrandbits(8) for _ in range(rng.randrange(0, 9)))) if rng else (lambda: b"")
                cols.append([junk() if t[c] is None else t[c] for t in self.rows])
            else:
                junk = (lambda: rng.getrandbits(8 * typ)) if rng else (lambda: 0)
                cols.append(np.array([junk() if t[c] is None else t[c] for t in self.rows], "u%d" % typ))
        return cols

    def key64(self, H, bits):
        if not self.n:
            return []
        cols, valid = self.columns(), self.masks()
        if "s" in self.layout:
            k = H.mixed_key64(cols, bits, valid=valid, null_equal=True)
        else:
            k = H.cols_key64(cols, self.layout, hash_bits=bits, valid=valid, null_equal=True)
        return [int(x) for x in k]

    def n_null(self):
        return sum(1 for t in self.rows if any(v is None for v in t))

    def val(self, i):
        return i if self.vals is None else int(self.vals[i]) & M64

    def sum_vals(self):
        return sum(self.val(i) for i in range(self.n)) & M64


def dev_str(keys):
    import torch

    lens = np.fromiter((len(k) for k in keys), dtype=np.int64, count=len(keys))
    off = np.zeros(len(keys) + 1, np.int64)
    np.cumsum(lens, out=off[1:])
    raw = np.frombuffer(b"".join(keys) + b"\x5a" * 3, np.uint8).copy()
    return torch.from_numpy(raw).cuda(), torch.from_numpy(off).cuda()


def dev(H, rel, bit_off=0, junk=None):
    """(cols, vals, valid) as Executor.join_kind_cols_device / join_mixed_device take them.  bit_off: one bit offset for every
    bitmap, or one per column; junk: the rng that fills what lies under NULL slots (None: zeros)."""
    import torch

    cols = [torch.from_numpy(c.view("i%d" % c.dtype.itemsize)).cuda() if isinstance(c, np.ndarray) else dev_str(c) for c in rel.columns(junk)]
    vals = None if rel.vals is None else torch.from_numpy(np.array([v & M64 for v in rel.vals], np.uint64).view(np.int64)).cuda()
    offs = bit_off if isinstance(bit_off, (list, tuple)) else [bit_off] * len(rel.layout)
    valid = [None if m is None else (H.pack_validity(m, offs[c], "cuda"), offs[c]) for c, m in enumerate(rel.masks())]
    return cols, vals, (valid if rel.bitmap else None)


def run(H, ex, B, P, DB, DP, side, kind, flags, bits=0, force=False):
    """One call of the entry the layout belongs to; rows: None in the count modes.  info["form"]: the column entry's only."""
    if "s" in B.layout:
        res, info = ex.join_mixed_device(DB[0], DB[1], DP[0], DP[1], side, kind, flags, hash_bits=bits, probe_fill=PFILL, build_fill=BFILL,
                                         build_valid=DB[2], probe_valid=DP[2])
        rows = ex.mixed_rows_to_numpy(res) if flags & (H.HMJ_MATERIALIZE | H.HMJ_ORDERED) else None
    else:
        res, info = ex.join_kind_cols_device(DB[0], DB[1], DP[0], DP[1], side, kind, flags, hash_bits=bits, force_hashed=force,
                                             probe_fill=PFILL, build_fill=BFILL, build_valid=DB[2], probe_valid=DP[2])
        rows = ex.cols_kind_rows_to_numpy(res) if flags & (H.HMJ_MATERIALIZE | H.HMJ_ORDERED) else None
    return res, info, rows


def expect(H, B, P, side, kind, bits=0):
    return ne_rows(B.rows, P.rows, B.key64(H, bits), P.key64(H, bits), [B.val(i) for i in range(B.n)], [P.val(i) for i in range(P.n)],
                   side, kind, PFILL, BFILL)


def check(H, ex, B, P, DB, DP, bits=0, kinds=ALL_KINDS, modes=None, tag=()):
    """Every kind in `modes` under the flag against the brute force: count and sums, checksums and the probe sum where asked,
    the kind's counters, the rows with a NULL slot per side, key pairs and collisions, the form; key64 and the rows exactly
    when ordered, as sorted multisets otherwise.  Returns what the calls went through (ne_rows' `seen`) and the collisions."""
    seen, n_coll_all = set(), 0
    sum_p = P.sum_vals()
    any_bitmap = bool(B.bitmap or P.bitmap)
    for side, kind in kinds:
        want, counts, n_pairs, n_coll, sn = expect(H, B, P, side, kind, bits)
        ck = kind_checks(want)
        n_coll_all += n_coll
        for flags in modes or all_modes(H):
            t = tag + (side, kind, flags, bits)
            res, info, got = run(H, ex, B, P, DB, DP, side, kind, flags | H.HMJ_NULL_EQUAL, bits)
            got_ck = res.checks()
            print(t, got_ck, {k: info[k] for k in ("n_key_pairs", "n_collisions", "n_build_null", "n_probe_null") + COUNT_KEYS})
            if flags & H.HMJ_CHECKSUM:
                assert got_ck == ck, t
            else:
                assert (got_ck["n_matches"], got_ck["sum_r"], got_ck["sum_s"]) == (ck["n_matches"], ck["sum_r"], ck["sum_s"]), t
            if flags & H.HMJ_SUM_PROBE:
                assert int(res.sum_probe_all) == sum_p, t
            assert {k: info[k] for k in COUNT_KEYS} == counts, (t, info, counts)
            if any_bitmap:  # (informational; a call without any bitmap is the call without the flag, which reports 0)
                assert (info["n_build_null"], info["n_probe_null"]) == (B.n_null(), P.n_null()), (t, info)
                assert (info["n_key_pairs"], info["n_collisions"]) == (n_pairs, n_coll), (t, info, n_pairs, n_coll)
                assert info.get("form", H.HMJ_COLS_HASHED) == H.HMJ_COLS_HASHED, t
            if got is None:
                assert not res.key64, t
                continue
            assert got.shape == want.shape, (t, got.shape, want.shape)
            if flags & H.HMJ_ORDERED:
                assert np.array_equal(got, want), (t, np.flatnonzero(np.any(got != want, axis=1))[:5])
                seen |= sn
            else:
                assert np.array_equal(unordered(got), unordered(want)), t
                seen |= sn & {"ambiguous"}
    return seen, n_coll_all


# ---- drawing relations -------------------------------------------------------------------------------------------------------
def col_values(rng, typ, n_values):
    """The values a column draws from (at most 40): the extremes, 0 / the empty string, and random ones."""
    assert n_values <= 40
    if typ == "s":
        vals = {b"", b"a", b"ab", b"\x00", b"key", b"key\x00"}
        while len(vals) < n_values:
            vals.add(b"k%03d" % rng.randrange(1000) + bytes(rng.getrandbits(8) for _ in range(rng.randrange(0, 12))))
    else:
        top = (1 << (8 * typ)) - 1
        vals = {0, 1, top, top - 1}
        while len(vals) < min(n_values, top + 1):
            vals.add(rng.getrandbits(8 * typ))
    return sorted(vals)


def draw_pool(rng, layout, n, n_values=20, frac=NULL_FRAC):
    """About n distinct tuples with NULL slots (each slot with probability frac).  Always among them: the all-NULL tuple, and
    for a few x the tuples that differ only in NULL against the zero value -- (NULL, x..), (0 or "", x..) -- and in where
    the NULL stands -- (x, NULL, ..) against (NULL, x, ..) where the first two columns have one type."""
    k = len(layout)
    values = [col_values(rng, typ, n_values) for typ in layout]
    zero = [b"" if typ == "s" else 0 for typ in layout]
    pool = {(None,) * k} if frac else set()
    for _ in range(4 if frac else 0):
        rest = tuple(rng.choice(values[c]) for c in range(1, k))
        pool.add((None,) + rest)
        pool.add((zero[0],) + rest)
        if k > 1 and layout[0] == layout[1]:
            x = rng.choice(values[0])
            pool.add((x, None) + rest[1:])
            pool.add((None, x) + rest[1:])
    most = 1  # the tuples the values can spell
    for v in values:
        most *= len(v) + (1 if frac else 0)
    target = max(min(n, most * 3 // 4), len(pool), 2)
    while len(pool) < target:
        pool.add(tuple(None if rng.random() < frac else rng.choice(values[c]) for c in range(k)))
    pool = sorted(pool, key=lambda t: tuple((v is None, v if v is not None else 0) for v in t))
    rng.shuffle(pool)
    return pool


def relations(rng, layout, nb, np_, miss=0.25, frac=NULL_FRAC, extra_b=(), extra_p=(), **kw):
    """Duplicates and misses on both sides: build rows from the front of a pool of distinct tuples, probe rows from its back;
    from a wave of rows on, the all-NULL tuple stands on both sides.  extra_*: rows that take the place of drawn ones."""
    pool = draw_pool(rng, layout, max(4, (nb + np_) // 3), frac=frac, **kw)
    cut = min(len(pool) - 1, max(1, int(len(pool) * miss)))
    bsrc, psrc = pool[:len(pool) - cut], pool[cut:]
    bt = [rng.choice(bsrc) for _ in range(nb)]
    pt = [rng.choice(psrc) for _ in range(np_)]
    for rows, extra in ((bt, list(extra_b)), (pt, list(extra_p))):
        if frac and len(rows) >= 63:
            extra = extra + [(None,) * len(layout)]
        for i, t in zip(rng.sample(range(len(rows)), len(extra)), extra):
            rows[i] = t
    return Rel(layout, bt, [rng.getrandbits(64) for _ in bt]), Rel(layout, pt, None)


def without_nulls(rng, R, keep=()):
    """R with the NULL slots of the columns outside `keep` replaced by values of their column."""
    zero = [b"" if typ == "s" else 0 for typ in R.layout]
    held = [[t[c] for t in R.rows if t[c] is not None] or [zero[c]] for c in range(len(R.layout))]
    return Rel(R.layout, [tuple(rng.choice(held[c]) if v is None and c not in keep else v for c, v in enumerate(t)) for t in R.rows], R.vals)


def colliding(H, layout, bits, a_of, b_of):
    """The first x in 1..20000 for which the tuples a_of(x) and b_of(x) have one key64 under hash_bits `bits`."""
    xs = list(range(1, 20001))
    ka, kb = Rel(layout, [a_of(x) for x in xs]).key64(H, bits), Rel(layout, [b_of(x) for x in xs]).key64(H, bits)
    return next(x for x, p, q in zip(xs, ka, kb) if p == q)


# ---- all kinds, both entries -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(COL_LAYOUTS) + list(MIX_LAYOUTS))
def test_all_kinds(H, ex, name):
    layout = COL_LAYOUTS.get(name) or MIX_LAYOUTS[name]
    rng = random.Random(len(name) * 31 + len(layout))
    for nb, np_ in SIZE_PAIRS:
        B, P = relations(rng, layout, nb, np_)
        if nb == np_ == 1000:  # duplicates and all-NULL tuples on both sides
            full = (None,) * len(layout)
            assert full in B.rows and full in P.rows and len(set(B.rows)) < nb and len(set(P.rows)) < np_
        check(H, ex, B, P, dev(H, B), dev(H, P), tag=(name, nb, np_))


# ---- bitmap variations -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["u64_u32_u16", "u32_str_str"])
def test_bitmap_variations(H, ex, name):
    layout = COL_LAYOUTS.get(name) or MIX_LAYOUTS[name]
    rng = random.Random(77 + len(name))
    B, P = relations(rng, layout, 300, 257)
    strip = lambda R, keep: without_nulls(rng, R, keep)
    # bitmaps on one side only: the other side holds no NULL and passes no bitmap
    for B1, P1 in ((B, strip(P, ())), (strip(B, ()), P)):
        assert bool(B1.bitmap) != bool(P1.bitmap)
        check(H, ex, B1, P1, dev(H, B1), dev(H, P1), modes=modes2(H), tag=(name, "one side"))
    # bitmaps on some columns only (column 1), and a bitmap over a column without NULLs beside them
    B2, P2 = strip(B, (1,)), strip(P, (1,))
    assert B2.bitmap == [1] and P2.bitmap == [1]
    check(H, ex, B2, P2, dev(H, B2), dev(H, P2), modes=modes2(H), tag=(name, "column 1"))
    P3 = Rel(layout, P2.rows, None, bitmap=[0, 1])
    check(H, ex, B2, P3, dev(H, B2), dev(H, P3), kinds=[(PROBE, INNER), (BUILD, FULL_OUTER)], modes=modes2(H), tag=(name, "all-valid bitmap"))
    # bit offsets: inside the first byte, past it, past the first 8-byte word; one per column
    for offs in ([0, 3, 13], [3, 13, 64 + 5], [64 + 5, 0, 3], [13, 64 + 5, 0]):
        check(H, ex, B, P, dev(H, B, offs), dev(H, P, offs[::-1]), kinds=[(PROBE, PROBE_OUTER), (BUILD, FULL_OUTER), (PROBE, SEMI)],
              modes=modes2(H), tag=(name, "bit_offset", tuple(offs)))
    # an all-NULL column
    B4 = Rel(layout, [(t[0], None) + t[2:] for t in B.rows], B.vals)
    P4 = Rel(layout, [(t[0], None) + t[2:] for t in P.rows], None)
    check(H, ex, B4, P4, dev(H, B4), dev(H, P4), modes=modes2(H), tag=(name, "all-NULL column"))
    # an all-NULL relation is not an empty side: its rows match the other side's all-NULL rows
    full = (None,) * len(layout)
    B5 = Rel(layout, [full] * 65, list(range(100, 165)))
    n_full = sum(1 for t in P.rows if t == full)
    assert n_full > 0
    check(H, ex, B5, P, dev(H, B5), dev(H, P), tag=(name, "all-NULL relation"))
    res, info, _ = run(H, ex, B5, P, dev(H, B5), dev(H, P), PROBE, INNER, H.HMJ_NULL_EQUAL)
    assert int(res.n_matches) == 65 * n_full and info["n_build_null"] == 65


# ---- collisions --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,bits,nb,np_", [("u32x2", 3, 65, 63), ("u32x2", 6, 300, 257), ("str_u32", 3, 65, 63), ("str_u32", 6, 300, 257)])
def test_collisions(H, ex, name, bits, nb, np_):
    """Few key64 values: verification and the collision sort, not key64, tell (NULL, x) from (0, x) and (x, NULL), and NULL
    from the empty string.  Both tuples of such a pair, chosen to share their key64, stand on both sides."""
    layout = COL_LAYOUTS.get(name) or MIX_LAYOUTS[name]
    rng = random.Random(bits * 100 + len(name))
    zero = b"" if layout[0] == "s" else 0
    x = colliding(H, layout, bits, lambda x: (None, x), lambda x: (zero, x))
    twins = [((None, x), (zero, x))]
    if layout == [4, 4]:
        y = colliding(H, layout, bits, lambda y: (y, None), lambda y: (None, y))
        twins.append(((y, None), (None, y)))
    extra = [t for pair in twins for t in pair] + [(None, x)]  # (a duplicate of a tuple with a NULL slot)
    B, P = relations(rng, layout, nb, np_, n_values=8, extra_b=extra, extra_p=extra[::-1])
    kb, kp = B.key64(H, bits), P.key64(H, bits)
    for a, b in twins:
        assert a != b and kb[B.rows.index(a)] == kp[P.rows.index(b)] == kb[B.rows.index(b)], (a, b)
    seen, n_coll = check(H, ex, B, P, dev(H, B), dev(H, P), bits=bits, tag=(name, "collisions"))
    print("reached:", sorted(seen), "collisions:", n_coll)
    assert n_coll > 0
    assert seen == {"ambiguous", "sort"}, seen


# ---- identities --------------------------------------------------------------------------------------------------------------
def same_call(H, a, b, t):
    (ra, ia, rowsa), (rb, ib, rowsb) = a, b
    assert ra.checks() == rb.checks(), t
    assert int(ra.sum_probe_all) == int(rb.sum_probe_all), t
    assert {k: ia[k] for k in COUNT_KEYS + ("n_key_pairs", "n_collisions")} == {k: ib[k] for k in COUNT_KEYS + ("n_key_pairs", "n_collisions")}, t
    assert (rowsa is None) == (rowsb is None), t
    if rowsa is not None:
        assert np.array_equal(rowsa, rowsb), t


@pytest.mark.parametrize("name", ["u32x2", "str_u32"])
def test_all_valid_bitmaps_are_the_call_without_the_flag(H, ex, name):
    """Rows, order, sums and key64: a row without NULLs has exactly the plain hashed key64."""
    layout = COL_LAYOUTS.get(name) or MIX_LAYOUTS[name]
    rng = random.Random(5 + len(name))
    B, P = relations(rng, layout, 300, 257, frac=0.0)
    assert B.n_null() == P.n_null() == 0
    Bv, Pv = Rel(layout, B.rows, B.vals, bitmap=range(len(layout))), Rel(layout, P.rows, None, bitmap=[0])
    DB, DP, DBv, DPv = dev(H, B), dev(H, P), dev(H, Bv, 3), dev(H, Pv, 69)
    assert DB[2] is None and DP[2] is None and len(DBv[2]) == len(layout)
    for bits in (0, 5):
        for side, kind in ALL_KINDS:
            for flags in modes2(H):
                t = (name, side, kind, flags, bits)
                plain = run(H, ex, B, P, DB, DP, side, kind, flags, bits, force=True)
                flagged = run(H, ex, Bv, Pv, DBv, DPv, side, kind, flags | H.HMJ_NULL_EQUAL, bits)
                same_call(H, plain, flagged, t)
                assert flagged[1].get("form", H.HMJ_COLS_HASHED) == H.HMJ_COLS_HASHED, t
                assert (flagged[1]["n_build_null"], flagged[1]["n_probe_null"]) == (0, 0), t


def test_the_flag_without_a_bitmap_is_the_call_without_it(H, ex):
    """[4, 4] stays packed: with no bitmap there is no NULL to match."""
    layout = [4, 4]
    rng = random.Random(8)
    B, P = relations(rng, layout, 300, 257, frac=0.0)
    DB, DP = dev(H, B), dev(H, P)
    for side, kind in ALL_KINDS:
        for flags in modes2(H):
            plain = run(H, ex, B, P, DB, DP, side, kind, flags)
            flagged = run(H, ex, B, P, DB, DP, side, kind, flags | H.HMJ_NULL_EQUAL)
            same_call(H, plain, flagged, (side, kind, flags))
            assert plain[1]["form"] == flagged[1]["form"] == H.HMJ_COLS_PACKED
    # ... and the reference agrees (key64 is then the packed tuple, so only counts and sums are compared)
    want = expect(H, B, P, BUILD, FULL_OUTER)[0]
    res, _, _ = run(H, ex, B, P, DB, DP, BUILD, FULL_OUTER, H.HMJ_NULL_EQUAL)
    assert (int(res.n_matches), int(res.sum_r), int(res.sum_s)) == tuple(kind_checks(want)[k] for k in ("n_matches", "sum_r", "sum_s"))


@pytest.mark.parametrize("name", ["u64_u32_u16", "str_u32"])
def test_the_flag_is_the_mask_column_workaround(H, ex, name):
    """k <= 7: the same (r_row, s_row) rows as the call without the flag on the columns with their NULL slots zeroed and the
    rows' NULL masks appended as a 1-byte key column -- what a caller had to build before."""
    layout = COL_LAYOUTS.get(name) or MIX_LAYOUTS[name]
    rng = random.Random(21 + len(name))
    B, P = relations(rng, layout, 300, 257)
    zero = [b"" if typ == "s" else 0 for typ in layout]
    mask = lambda t: sum(1 << c for c, v in enumerate(t) if v is None)
    widen = lambda R: Rel(layout + [1], [tuple(zero[c] if v is None else v for c, v in enumerate(t)) + (mask(t),) for t in R.rows], R.vals)
    B2, P2 = widen(B), widen(P)
    assert B2.n_null() == 0 and any(t[-1] for t in B2.rows) and any(t[-1] for t in P2.rows)
    DB, DP, DB2, DP2 = dev(H, B), dev(H, P), dev(H, B2), dev(H, P2)
    for side, kind in ALL_KINDS:
        flagged = run(H, ex, B, P, DB, DP, side, kind, H.HMJ_MATERIALIZE | H.HMJ_NULL_EQUAL)
        plain = run(H, ex, B2, P2, DB2, DP2, side, kind, H.HMJ_MATERIALIZE, force=True)
        assert np.array_equal(unordered(flagged[2][:, 1:]), unordered(plain[2][:, 1:])), (name, side, kind)
        assert {k: flagged[1][k] for k in COUNT_KEYS} == {k: plain[1][k] for k in COUNT_KEYS}, (name, side, kind)


@pytest.mark.parametrize("name", ["u8x8", "u32_str_str"])
def test_semi_and_anti_partition_and_full_outer_adds_up(H, ex, name):
    layout = COL_LAYOUTS.get(name) or MIX_LAYOUTS[name]
    rng = random.Random(34 + len(name))
    B, P = relations(rng, layout, 257, 300)
    DB, DP = dev(H, B), dev(H, P)
    fl = H.HMJ_ORDERED | H.HMJ_NULL_EQUAL
    semi, anti = run(H, ex, B, P, DB, DP, PROBE, SEMI, fl), run(H, ex, B, P, DB, DP, PROBE, ANTI, fl)
    rows = sorted(semi[2][:, 2].tolist() + anti[2][:, 2].tolist())
    assert rows == list(range(P.n)) and len(semi[2]) and len(anti[2])
    assert any(None in P.rows[s] for s in semi[2][:, 2].tolist())  # rows with NULL slots are matched like any other
    inner, full = run(H, ex, B, P, DB, DP, PROBE, INNER, H.HMJ_NULL_EQUAL), run(H, ex, B, P, DB, DP, BUILD, FULL_OUTER, H.HMJ_NULL_EQUAL)
    bo = run(H, ex, B, P, DB, DP, BUILD, BUILD_OUTER, H.HMJ_NULL_EQUAL)
    assert int(full[0].n_matches) == int(inner[0].n_matches) + full[1]["n_probe_unmatched"] + full[1]["n_build_unmatched"]
    assert full[1]["n_probe_unmatched"] == len(anti[2]) and full[1]["n_build_unmatched"] == bo[1]["n_build_unmatched"]
    assert full[1]["n_probe_matched"] + full[1]["n_probe_unmatched"] == P.n and full[1]["n_build_matched"] + full[1]["n_build_unmatched"] == B.n


# ---- what lies under a NULL slot ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["u64_u32_u16", "u32_str_str"])
def test_nothing_depends_on_what_lies_under_a_null_slot(H, ex, name):
    layout = COL_LAYOUTS.get(name) or MIX_LAYOUTS[name]
    rng = random.Random(55 + len(name))
    B, P = relations(rng, layout, 300, 257)
    DB0, DP0 = dev(H, B), dev(H, P)
    DB1, DP1 = dev(H, B, junk=random.Random(1)), dev(H, P, junk=random.Random(2))
    for bits in (0, 4):
        for side, kind in ALL_KINDS:
            for flags in modes2(H):
                same_call(H, run(H, ex, B, P, DB0, DP0, side, kind, flags | H.HMJ_NULL_EQUAL, bits),
                          run(H, ex, B, P, DB1, DP1, side, kind, flags | H.HMJ_NULL_EQUAL, bits), (name, side, kind, flags, bits))
    check(H, ex, B, P, DB1, DP1, kinds=[(BUILD, FULL_OUTER)], modes=modes2(H), tag=(name, "junk"))


# ---- without the flag --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["u32x2", "str_u32"])
def test_without_the_flag_the_same_inputs_join_under_sql_semantics(H, ex, name):
    layout = COL_LAYOUTS.get(name) or MIX_LAYOUTS[name]
    rng = random.Random(13 + len(name))
    B, P = relations(rng, layout, 300, 257)
    DB, DP = dev(H, B), dev(H, P)
    sql_pairs = sorted((r, s) for r, t in enumerate(B.rows) for s, u in enumerate(P.rows) if t == u and None not in t)
    ne_pairs = sorted((r, s) for r, t in enumerate(B.rows) for s, u in enumerate(P.rows) if t == u)
    assert len(sql_pairs) < len(ne_pairs)
    res, info, rows = run(H, ex, B, P, DB, DP, PROBE, INNER, H.HMJ_MATERIALIZE)
    assert sorted(map(tuple, rows[:, 1:3].tolist())) == sql_pairs
    assert (info["n_build_null"], info["n_probe_null"]) == (B.n_null(), P.n_null())
    res, info, rows = run(H, ex, B, P, DB, DP, PROBE, ANTI, H.HMJ_MATERIALIZE)
    assert sorted(rows[:, 2].tolist()) == sorted(set(range(P.n)) - {s for _, s in sql_pairs})
    assert all(k == 0 for k, s in zip(rows[:, 0].tolist(), rows[:, 2].tolist()) if None in P.rows[s])  # a NULL-key row's key64 is 0
    res, info, rows = run(H, ex, B, P, DB, DP, PROBE, INNER, H.HMJ_MATERIALIZE | H.HMJ_NULL_EQUAL)
    assert sorted(map(tuple, rows[:, 1:3].tolist())) == ne_pairs


# ---- argument errors ---------------------------------------------------------------------------------------------------------
def test_the_string_kinds_entry_refuses_the_flag(H, ex):
    import torch

    keys = [b"a", b"", b"bc"]
    chars, off = dev_str(keys)
    rel = (chars, off, torch.arange(3, dtype=torch.int64, device="cuda"))
    valid = H.pack_validity(np.array([True, False, True]), 0, "cuda")
    for kw in ({}, {"build_valid": valid, "probe_valid": valid}):
        with pytest.raises(H.HmjError) as e:
            ex.join_kind_str_device(rel, rel, PROBE, SEMI, H.HMJ_NULL_EQUAL, **kw)
        assert e.value.code == HMJ_E_ARG and "hmj_join_mixed_device" in str(e.value), str(e.value)
    # the ctx stays usable, and the mixed entry with one string column is the call the message points to
    res, info = ex.join_kind_str_device(rel, rel, PROBE, SEMI, 0, build_valid=valid, probe_valid=valid)
    assert int(res.n_matches) == 2
    res, info = ex.join_mixed_device([(chars, off)], None, [(chars, off)], None, PROBE, SEMI, H.HMJ_NULL_EQUAL, build_valid=[valid],
                                     probe_valid=[valid])
    assert int(res.n_matches) == 3 and info["n_probe_null"] == 1


def test_decreasing_offsets_under_a_null_slot_are_still_refused(H, ex):
    layout = ["s", 4]
    rng = random.Random(3)
    B, P = relations(rng, layout, 257, 300)
    s = next(i for i, t in enumerate(P.rows) if t[0] is None and i > 64)
    DB, DP = dev(H, B), dev(H, P, junk=random.Random(4))
    worse = DP[0][0][1].clone()
    assert int(worse[s]) > 0  # (rows in front of it hold bytes)
    worse[s + 1] = worse[s] - 1  # (row s + 1 then starts one byte early, inside the buffer)
    for side, kind in ((PROBE, INNER), (BUILD, FULL_OUTER)):
        with pytest.raises(H.HmjError) as e:
            ex.join_mixed_device(DB[0], DB[1], [(DP[0][0][0], worse), DP[0][1]], DP[1], side, kind, H.HMJ_NULL_EQUAL, build_valid=DB[2],
                                 probe_valid=DP[2])
        assert e.value.code == HMJ_E_ARG and "probe relation: column 0: offsets decrease at row %d " % s in str(e.value), str(e.value)
        check(H, ex, B, P, DB, DP, kinds=[(side, kind)], modes=modes2(H), tag=("after bad offsets",))
