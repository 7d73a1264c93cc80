"""GPU checks of the mixed-key join (hmj_join_mixed_device: key tuples of Arrow large_string and fixed-width columns) against
a Python dict brute force over tuples, with `mixed_key64` (pinned by test_join_mixed_cpu.py) for key64: row counts around
the wave and workgroup edges for five layouts, string spans that take the staged and the unstaged path of the key kernel,
forced key64 collisions through the ambiguous list and the collision sort, NULL keys, the entries it must agree with,
argument errors, the take entries on its row maps, the planner's isolation, a seeded sweep and one larger case."""
import ctypes as C
import os
import random

import numpy as np
import pytest

from test_join_cols_gpu import unordered
from test_join_cols_kinds_cpu import (ALL_KINDS, ANTI, BUILD, BUILD_ANTI, BUILD_OUTER, BUILD_SEMI, COUNT_KEYS, FULL_OUTER, INNER, M64,
                                      NO_ROW, PROBE, PROBE_OUTER, SEMI, kind_checks)

pytestmark = pytest.mark.gpu
HMJ_E_ARG, HMJ_E_UNSUPPORTED = -1, -5
PFILL, BFILL = 0xF1, 2 ** 64 - 2
SEMI_ANTI = [(PROBE, SEMI), (PROBE, ANTI), (BUILD, BUILD_SEMI), (BUILD, BUILD_ANTI)]
SIZES = [1, 63, 64, 65, 255, 256, 257, 1000]
STAGE = 4096  # bytes of one wave's LDS stage in mix_key_kernel


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


def modes2(H):
    """ordered and count modes"""
    return (H.HMJ_ORDERED | H.HMJ_CHECKSUM | H.HMJ_SUM_PROBE, H.HMJ_CHECKSUM | H.HMJ_SUM_PROBE)


# ---- relations on the host -------------------------------------------------------------------------------------------------
class Rel:
    """cols: per key column a numpy unsigned array (fixed-width) or a list of bytes (string); valid: None, or per column None
    or a bool array (True = valid); vals: None (the payload of row i is i) or a list of ints."""

    def __init__(self, cols, vals=None, valid=None):
        self.cols, self.vals, self.valid = cols, vals, valid
        self.n = len(cols[0])
        assert all(len(c) == self.n for c in cols)

    def tuples(self):
        cs = [[int(x) for x in c] if isinstance(c, np.ndarray) else list(c) for c in self.cols]
        return list(zip(*cs)) if self.n else []

    def null(self):
        out = np.zeros(self.n, bool)
        for m in self.valid or ():
            if m is not None:
                out |= ~m
        return out

    def key64(self, H, bits):
        if not self.n:
            return []
        k = H.mixed_key64(self.cols, bits)
        k[self.null()] = 0
        return [int(x) for x in k]

    def val(self, i):
        return i if self.vals is None else int(self.vals[i]) & M64

    def sum_vals(self):
        return sum(self.val(i) for i in range(self.n)) & M64


def dev_str(keys, base=0, first=0, null_data=False):
    """A string column on the device: (chars, offsets).  base: the chars buffer starts that many bytes into its allocation;
    first: offsets[0] (bytes in front of the first key that belong to no key); null_data: no chars buffer at all."""
    import torch

    lens = np.fromiter((len(k) for k in keys), dtype=np.int64, count=len(keys))
    off = np.full(len(keys) + 1, first, np.int64)
    np.cumsum(lens, out=off[1:])
    off[1:] += first
    if null_data:
        assert int(lens.sum()) == 0
        return None, torch.from_numpy(off).cuda()
    raw = np.frombuffer(b"\xa5" * (base + first) + b"".join(keys) + b"\x5a" * 3, np.uint8).copy()
    return torch.from_numpy(raw).cuda()[base:], torch.from_numpy(off).cuda()


def dev(H, rel, base=0, first=0, bit_off=0, null_data=False):
    """(cols, vals, valid) as Executor.join_mixed_device takes them."""
    import torch

    # (a fixed-width column goes up as the signed dtype of its width: compared bit for bit anyway)
    cols = [torch.from_numpy(np.ascontiguousarray(c).view("i%d" % c.dtype.itemsize)).cuda() if isinstance(c, np.ndarray)
            else dev_str(c, base, first, null_data) for c in rel.cols]
    vals = None if rel.vals is None else torch.from_numpy(np.array([v & M64 for v in rel.vals], np.uint64).view(np.int64)).cuda()
    valid = None if rel.valid is None else [None if m is None else (H.pack_validity(m, bit_off, "cuda"), bit_off) for m in rel.valid]
    return cols, vals, valid


# ---- the expectation ---------------------------------------------------------------------------------------------------------
def expect(H, B, P, side, kind, bits=0):
    """rows [n, 5] (key64, r_row, s_row, rval, sval) in the HMJ_ORDERED order -- (key64, tuple column by column, r_row, s_row),
    NO_ROW last, the NULL-key rows behind them (the build side's by r_row, then the probe side's by s_row); 0 in the columns
    the kind does not produce --, the four counters, n_key_pairs and n_collisions, and what the call went through:
    "ambiguous" (a semi / anti row whose key64 representative holds another tuple), "sort" (a run of equal key64 with
    several tuples among the ordered rows), "tail" (NULL-key rows in the result)."""
    tb, tp = B.tuples(), P.tuples()
    bnull, pnull = B.null(), P.null()
    kb, kp = B.key64(H, bits), P.key64(H, bits)
    b_by, p_by, bk, pk = {}, {}, {}, {}
    for r, t in enumerate(tb):
        if not bnull[r]:
            b_by.setdefault(t, []).append(r)
            bk.setdefault(kb[r], []).append(r)
    for s, t in enumerate(tp):
        if not pnull[s]:
            p_by.setdefault(t, []).append(s)
            pk.setdefault(kp[s], []).append(s)
    pairs = [(kp[s], t, r, s, B.val(r), P.val(s)) for s, t in enumerate(tp) if not pnull[s] for r in b_by.get(t, ())]
    p_match = [(not pnull[s]) and t in b_by for s, t in enumerate(tp)]
    b_match = [(not bnull[r]) and t in p_by for r, t in enumerate(tb)]

    def probe_rows(sel, fill):
        return [(kp[s], t, NO_ROW, s, fill, P.val(s)) for s, t in enumerate(tp) if p_match[s] == sel]

    def build_rows(sel, fill):
        return [(kb[r], t, r, NO_ROW, B.val(r), fill) for r, t in enumerate(tb) if b_match[r] == sel]

    counts = dict.fromkeys(COUNT_KEYS, 0)
    probe_counts = {"n_probe_matched": sum(p_match), "n_probe_unmatched": P.n - sum(p_match)}
    build_counts = {"n_build_matched": sum(b_match), "n_build_unmatched": B.n - sum(b_match)}
    absent = ()
    if (side, kind) == (PROBE, INNER):
        rows = pairs
    elif side == PROBE and kind in (SEMI, ANTI):
        rows, absent = probe_rows(kind == SEMI, 0), (1, 3)
        counts.update(probe_counts)
    elif side == PROBE:
        rows = pairs + probe_rows(False, PFILL)
        counts.update(probe_counts)
    elif kind in (BUILD_SEMI, BUILD_ANTI):
        rows, absent = build_rows(kind == BUILD_SEMI, 0), (2, 4)
        counts.update(build_counts)
    elif kind == BUILD_OUTER:
        rows = pairs + build_rows(False, BFILL)
        counts.update(build_counts)
    else:
        rows = pairs + probe_rows(False, PFILL) + build_rows(False, BFILL)
        counts.update(build_counts)
        counts.update(probe_counts)
    is_null = lambda row: (row[2] != NO_ROW and bnull[row[2]]) or (row[2] == NO_ROW and pnull[row[3]])
    main = sorted((x for x in rows if not is_null(x)), key=lambda x: x[:4])
    tail = sorted((x for x in rows if is_null(x)), key=lambda x: (x[2] == NO_ROW, x[2], x[3]))
    out = np.array([(k, r, s, rv, sv) for k, _, r, s, rv, sv in main + tail], np.uint64).reshape(-1, 5)
    for c in absent:
        out[:, c] = 0
    seen = set()
    # pairs of equal key64 the call compares, and those of them whose tuples differ
    if (side, kind) in SEMI_ANTI:  # the row against the first row of its key64 on the other side, then -- if that one
        n_pairs = n_coll = 0       # holds another tuple -- against every row of its key64 there
        K, ok, tk, to, knull, kk = (tp, bk, tp, tb, pnull, kp) if side == PROBE else (tb, pk, tb, tp, bnull, kb)
        for i, t in enumerate(K):
            o = [] if knull[i] else ok.get(kk[i], [])
            if not o:
                continue
            n_pairs += 1
            if to[o[0]] != t:
                seen.add("ambiguous")
                n_pairs += len(o)
                n_coll += 1 + sum(1 for j in o if to[j] != t)
    else:
        n_pairs = sum(len(bk.get(kp[s], ())) for s in range(P.n) if not pnull[s])
        n_coll = n_pairs - len(pairs)
    if any(a[0] == b[0] and a[1] != b[1] for a, b in zip(main, main[1:])):
        seen.add("sort")
    if tail:
        seen.add("tail")
    return out, counts, n_pairs, n_coll, seen


def run(H, ex, DB, DP, side, kind, flags, bits=0):
    res, info = ex.join_mixed_device(DB[0], DB[1], DP[0], DP[1], side, kind, flags, hash_bits=bits, probe_fill=PFILL, build_fill=BFILL,
                                     build_valid=DB[2], probe_valid=DP[2])
    rows = ex.mixed_rows_to_numpy(res) if flags & (H.HMJ_MATERIALIZE | H.HMJ_ORDERED) else None
    return res, info, rows


def check(H, ex, B, P, DB, DP, bits=0, kinds=ALL_KINDS, modes=None, tag=()):
    """Every kind in `modes` against the brute force: count, the five sums, the probe sum, the kind's counters, the NULL-key
    rows per side, key pairs and collisions; rows exactly when ordered, as sorted multisets otherwise.  Returns what the
    calls went through (expect's `seen`) and the collisions met."""
    seen, n_coll_all = set(), 0
    sum_p = P.sum_vals()
    for side, kind in kinds:
        want, counts, n_pairs, n_coll, sn = expect(H, B, P, side, kind, bits)
        ck = kind_checks(want)
        n_coll_all += n_coll
        for flags in modes or modes2(H):
            t = tag + (side, kind, flags, bits)
            res, info, got = run(H, ex, DB, DP, side, kind, flags, bits)
            got_ck = res.checks()
            print(t, got_ck, {k: info[k] for k in ("n_key_pairs", "n_collisions", "n_build_null", "n_probe_null") + COUNT_KEYS})
            assert got_ck == ck, t
            assert int(res.sum_probe_all) == sum_p, t  # every probe row, NULL-key rows included
            assert {k: info[k] for k in COUNT_KEYS} == counts, (t, info, counts)
            assert (info["n_build_null"], info["n_probe_null"]) == (int(B.null().sum()), int(P.null().sum())), (t, info)
            assert (info["n_key_pairs"], info["n_collisions"]) == (n_pairs, n_coll), (t, info, n_pairs, n_coll)
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
WORDS = [b"", b"a", b"ab", b"abc", b"key", b"key\x00", b"\x00", b"\xff", b"\xff\xfe", "zürich".encode(), b"alphabet", b"alphabets"]


def draw_string(rng, long_share=0.0):
    r = rng.random()
    if r < 0.25:
        return rng.choice(WORDS)
    if r < 0.25 + long_share:
        return bytes(rng.getrandbits(8) for _ in range(rng.randrange(90, 130)))
    return b"k%05d" % rng.randrange(100000) + bytes(rng.getrandbits(8) for _ in range(rng.randrange(0, 20)))


def draw_value(rng, typ, long_share=0.0):
    if typ == "s":
        return draw_string(rng, long_share)
    top = (1 << (8 * typ)) - 1
    return rng.choice((0, 1, top, top - 1, rng.getrandbits(8 * typ), rng.randrange(8)))


def draw_pool(rng, layout, n, long_share=0.0):
    """n distinct tuples (fewer where narrow fixed columns cannot spell that many) over `layout` ("s" or a width per column)
    with ties in the leading columns."""
    if "s" not in layout:  # (no more than half of the tuples the widths can spell)
        n = min(n, max(2, 256 ** sum(layout) // 2))
    pool, seen = [], set()
    heads = [draw_value(rng, layout[0], long_share) for _ in range(max(2, n // 4))]
    while len(pool) < n:
        t = (rng.choice(heads),) + tuple(draw_value(rng, typ, long_share) for typ in layout[1:])
        if len(layout) == 1:
            t = (draw_value(rng, layout[0], long_share),)
        if t not in seen:
            seen.add(t)
            pool.append(t)
    return pool


def columns(tuples, layout):
    return [[t[c] for t in tuples] if typ == "s" else np.array([t[c] for t in tuples], "u%d" % typ) for c, typ in enumerate(layout)]


def drawn(rng, layout, nb, np_, miss=0.33, copies=None, long_share=0.0):
    """Tuples with duplicates and misses on both sides: build rows from the front of a pool of distinct tuples, probe rows
    from its back.  copies: at most that many rows of one tuple per side (None: free)."""
    n_pool = max(3, (nb + np_) // 3) if copies is None else max(3, nb, np_)
    pool = draw_pool(rng, layout, n_pool, long_share)
    n_pool = len(pool)
    cut = min(n_pool - 1, max(1, int(n_pool * miss)))
    bsrc, psrc = pool[:n_pool - cut], pool[cut:]
    if copies is None:
        bt = [rng.choice(bsrc) for _ in range(nb)]
        pt = [rng.choice(psrc) for _ in range(np_)]
    else:
        bt = (bsrc * copies)[:]
        pt = (psrc * copies)[:]
        rng.shuffle(bt)
        rng.shuffle(pt)
        bt, pt = bt[:nb], pt[:np_]
    return bt, pt


def relations(rng, layout, nb, np_, **kw):
    bt, pt = drawn(rng, layout, nb, np_, **kw)
    B = Rel(columns(bt, layout), [rng.getrandbits(64) for _ in bt])
    P = Rel(columns(pt, layout), None)
    return B, P


def draw_masks(nrng, n, k, which, frac=0.3):
    """which: the columns that get a bitmap"""
    masks = [None] * k
    for c in which:
        masks[c] = nrng.random(n) >= frac
    return masks


# ---- row-count edges ---------------------------------------------------------------------------------------------------------
LAYOUTS = {"str_u32": ["s", 4], "u16_str_u64": [2, "s", 8], "str_str": ["s", "s"], "str": ["s"], "u32x3": [4, 4, 4]}


@pytest.mark.parametrize("name", list(LAYOUTS))
def test_row_count_edges(H, ex, name):
    """A single row, one short of / exactly / one past a wave and a workgroup, several workgroups, on each side."""
    layout = LAYOUTS[name]
    rng = random.Random(len(name) * 7 + 1)
    for i, nb in enumerate(SIZES):
        np_ = SIZES[(i + 3) % len(SIZES)]
        B, P = relations(rng, layout, nb, np_)
        check(H, ex, B, P, dev(H, B), dev(H, P), tag=(name, nb, np_))


# ---- string spans ------------------------------------------------------------------------------------------------------------
def test_string_spans(H, ex):
    """Inside one 64-row wave: ~100-byte strings (a span beyond the stage: the unstaged path) beside a wave of short ones, one
    key of 5000 bytes, empty strings, no chars buffer at all, offsets[0] != 0, a chars base 1, 7 and 15 bytes into its
    allocation, embedded NUL and 0xFF bytes, keys equal in their first 8, 16 and 17 bytes that differ in the last byte or
    only in length, and the ("ab","c") / ("a","bc") pair."""
    rng = random.Random(99)
    rb = lambda n: bytes(rng.getrandbits(8) for _ in range(n))
    long_wave = [rb(rng.randrange(90, 120)) for _ in range(64)]    # ~6.7 kB in one wave
    short_wave = [b"s%02d" % i for i in range(64)]
    huge = rb(5000)
    stem = rb(17)
    near = [stem[:8], stem[:8] + b"\x01", stem[:8] + b"\x02", stem[:16], stem[:16] + b"\x01", stem[:16] + b"\x02", stem, stem + b"\x00",
            stem[:16] + b"\xff", stem[:7] + b"\x00", stem[:7] + b"\xff", b"", b"\x00", b"\x00\x00", b"\xff" * 9, b"a\x00b", b"a\x00c"]
    keys = long_wave + short_wave + [huge] + near + [b"", b"", b"x"]
    assert sum(map(len, long_wave)) > STAGE + 64
    days = [rng.randrange(3) for _ in keys]
    bt = list(zip(keys, days))
    pt = [bt[i] for i in rng.sample(range(len(bt)), len(bt))] + [(k + b"!", d) for k, d in bt[::5]] + [(k, d + 1) for k, d in bt[::7]]
    layout = ["s", 4]
    B, P = Rel(columns(bt, layout), [rng.getrandbits(64) for _ in bt]), Rel(columns(pt, layout))
    seen = set()
    for base, first in ((0, 0), (1, 0), (7, 5), (15, 1)):
        seen |= check(H, ex, B, P, dev(H, B, base, first), dev(H, P, 16 - base if base else 0, first), tag=("spans", base, first))[0]
    # no chars buffer: every slot empty -- one valid key, the empty string
    E = Rel([[b""] * 70, np.array([i % 5 for i in range(70)], np.uint32)])
    F = Rel([[b""] * 130, np.array([i % 7 for i in range(130)], np.uint32)])
    check(H, ex, E, F, dev(H, E, null_data=True), dev(H, F, first=9, null_data=True), tag=("no chars",))
    check(H, ex, E, F, dev(H, E, null_data=True), dev(H, F), kinds=[(PROBE, INNER), (BUILD, FULL_OUTER)], tag=("no chars, one side",))
    # the same bytes cut elsewhere are different tuples
    S = Rel([[b"ab", b"a"], [b"c", b"bc"]])
    T = Rel([[b"a", b"ab", b"abc"], [b"bc", b"c", b""]])
    check(H, ex, S, T, dev(H, S), dev(H, T), tag=("cut",))
    res, info, rows = run(H, ex, dev(H, S), dev(H, T), PROBE, INNER, H.HMJ_ORDERED)
    assert sorted((int(r), int(s)) for r, s in rows[:, 1:3]) == [(0, 1), (1, 0)]


# ---- forced collisions -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [1, 3, 8])
def test_forced_collisions(H, ex, bits):
    """Few hash bits on unique tuples: semi and anti go through the ambiguous list, the ordered kinds through the collision
    sort, and ties of key64 must be broken on the string column (the fixed column holds two values only)."""
    rng = random.Random(500 + bits)
    seen, coll = set(), 0
    for layout, n in ((["s", 4], 300), ([4, "s"], 400), (["s", "s"], 500)):
        pool = set()
        while len(pool) < n + n // 3:
            pool.add(tuple(draw_string(rng) if typ == "s" else rng.randrange(2) for typ in layout))
        pool = sorted(pool)
        rng.shuffle(pool)
        bt, pt = pool[:n], pool[n // 3:n + n // 3]  # unique tuples: at most 500 + 167 result rows
        rng.shuffle(pt)
        B, P = Rel(columns(bt, layout), [rng.getrandbits(64) for _ in bt]), Rel(columns(pt, layout))
        s, c = check(H, ex, B, P, dev(H, B), dev(H, P), bits=bits, tag=("collide", tuple(layout)))
        seen |= s
        coll += c
    assert coll > 0 and {"ambiguous", "sort"} <= seen, (coll, seen)


def test_run_cap(H, ex):
    """1100 rows of one key64 with two distinct tuples: the ordered call is HMJ_E_UNSUPPORTED, the unordered one exact, and
    the ctx goes on."""
    cand = [(b"run%d" % i, 7) for i in range(40)]
    k1 = H.mixed_key64([[c[0] for c in cand], np.array([c[1] for c in cand], np.uint32)], 1)
    a, b = [cand[i] for i in np.flatnonzero(k1 == k1[0])[:2]]
    layout = ["s", 4]
    B, P = Rel(columns([a, b], layout)), Rel(columns([a, b] * 550, layout))
    DB, DP = dev(H, B), dev(H, P)
    with pytest.raises(H.HmjError) as e:
        run(H, ex, DB, DP, PROBE, INNER, H.HMJ_ORDERED, bits=1)
    assert e.value.code == HMJ_E_UNSUPPORTED, e.value
    res, info, rows = run(H, ex, DB, DP, PROBE, INNER, H.HMJ_MATERIALIZE | H.HMJ_CHECKSUM, bits=1)
    want = expect(H, B, P, PROBE, INNER, 1)
    assert res.checks() == kind_checks(want[0]) and np.array_equal(unordered(rows), unordered(want[0]))
    assert (info["n_key_pairs"], info["n_collisions"]) == (2200, 1100)
    check(H, ex, B, P, DB, DP, bits=0, tag=("after the cap",))


# ---- NULL keys ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["string", "fixed", "both"])
def test_null_keys(H, ex, which):
    """A bitmap on the string column only, on a fixed column only, on both; bit offsets inside a byte and across bytes; NULL
    slots over garbage bytes with a length; bitmaps on one side only; a side that is all NULL."""
    layout = ["s", 4]
    cols_with = {"string": [0], "fixed": [1], "both": [0, 1]}[which]
    rng = random.Random(len(which))
    nrng = np.random.default_rng(len(which))
    seen = set()
    for nb, np_, off in ((300, 500, 0), (257, 64, 3), (65, 1000, 13)):
        B, P = relations(rng, layout, nb, np_)
        B.valid, P.valid = draw_masks(nrng, nb, 2, cols_with), draw_masks(nrng, np_, 2, cols_with)
        if 0 in cols_with:  # under a NULL slot: bytes that spell a key of the other side, or nothing at all
            for R, O in ((B, P), (P, B)):
                for i in np.flatnonzero(~R.valid[0]):
                    R.cols[0][i] = rng.choice(O.cols[0]) if i % 2 else b""
        if 1 in cols_with:
            B.cols[1][~B.valid[1]] = P.cols[1][0]
        assert B.null().any() and P.null().any()
        seen |= check(H, ex, B, P, dev(H, B, bit_off=off), dev(H, P, bit_off=(off * 5) % 16), tag=("nulls", which, nb, off))[0]
        # bitmaps on one side only
        P1 = Rel(P.cols, P.vals, None)
        check(H, ex, B, P1, dev(H, B, bit_off=off), dev(H, P1), kinds=[(PROBE, ANTI), (BUILD, FULL_OUTER), (PROBE, INNER)],
              tag=("build bitmaps only", which))
    assert "tail" in seen
    # a valid empty string is a key; a NULL slot of length 0 is not
    E = Rel([[b"", b"", b"x"], np.array([1, 1, 1], np.uint32)], None, [np.array([True, False, True]), None])
    F = Rel([[b"", b"x", b""], np.array([1, 1, 1], np.uint32)], None, [np.array([True, True, False]), None])
    check(H, ex, E, F, dev(H, E, bit_off=3), dev(H, F, bit_off=13), tag=("empty vs NULL",))
    rows = run(H, ex, dev(H, E), dev(H, F), PROBE, INNER, H.HMJ_ORDERED)[2]
    assert sorted((int(r), int(s)) for r, s in rows[:, 1:3]) == [(0, 0), (2, 1)]
    # a side that is all NULL
    B, P = relations(rng, layout, 130, 200)
    B.valid = [np.zeros(130, bool) if 0 in cols_with else None, np.zeros(130, bool) if 1 in cols_with else None]
    check(H, ex, B, P, dev(H, B, bit_off=3), dev(H, P), tag=("all NULL", which))
    check(H, ex, P, B, dev(H, P), dev(H, B, bit_off=13), tag=("all NULL probe", which))


def test_all_valid_bitmaps_change_nothing(H, ex):
    rng = random.Random(31)
    layout = [2, "s", 8]
    B, P = relations(rng, layout, 700, 900)
    Bv = Rel(B.cols, B.vals, [np.ones(B.n, bool)] * 3)
    Pv = Rel(P.cols, P.vals, [None, np.ones(P.n, bool), None])
    DB, DP, DBv, DPv = dev(H, B), dev(H, P), dev(H, Bv, bit_off=3), dev(H, Pv)
    for side, kind in ALL_KINDS:
        for flags in modes2(H):
            a, ia, ra = run(H, ex, DB, DP, side, kind, flags)
            for db, dp in ((DBv, DPv), (DBv, DP), (DB, DPv)):
                b, ib, rb = run(H, ex, db, dp, side, kind, flags)
                t = (side, kind, flags)
                assert b.checks() == a.checks() and int(b.sum_probe_all) == int(a.sum_probe_all) and a.checks()["n_matches"] > 0, t
                assert {k: v for k, v in ib.items() if not k.startswith("ms_")} == {k: v for k, v in ia.items() if not k.startswith("ms_")}, t
                if ra is not None:
                    assert np.array_equal(ra, rb), t


# ---- the entries it must agree with ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [0, 5])
def test_fixed_columns_only_equal_the_column_join(H, ex, bits):
    """Fixed columns only: rows, key64, sums, order, n_key_pairs and n_collisions of hmj_join_kind_cols_device(force_hashed)."""
    rng = random.Random(77 + bits)
    n = 400 if bits else 1500
    B, P = relations(rng, [4, 2, 8], n, n + 100, copies=1 if bits else None)
    DB, DP = dev(H, B), dev(H, P)
    for side, kind in ALL_KINDS:
        for flags in modes2(H):
            a, ia, ra = run(H, ex, DB, DP, side, kind, flags, bits)
            b, ib = ex.join_kind_cols_device(DB[0], DB[1], DP[0], DP[1], side, kind, flags, hash_bits=bits, force_hashed=True,
                                             probe_fill=PFILL, build_fill=BFILL)
            t = (side, kind, flags)
            assert a.checks() == b.checks() and int(a.sum_probe_all) == int(b.sum_probe_all), t
            for k in COUNT_KEYS + ("n_key_pairs", "n_collisions"):
                assert ia[k] == ib[k], (t, k)
            if ra is not None:
                assert np.array_equal(ra, ex.cols_kind_rows_to_numpy(b)), t
    assert bits == 0 or ia["n_collisions"] > 0


def test_one_string_column_equals_the_string_join(H, ex):
    """[str] only: the set of (r_row, s_row) and the counters of hmj_join_kind_str_device (key64 differs by definition)."""
    import torch

    rng = random.Random(78)
    B, P = relations(rng, ["s"], 1200, 1500)
    P.vals = list(range(P.n))
    DB, DP = dev(H, B), dev(H, P)
    for side, kind in ALL_KINDS:
        a, ia, ra = run(H, ex, DB, DP, side, kind, H.HMJ_MATERIALIZE | H.HMJ_CHECKSUM)
        b, ib = ex.join_kind_str_device(DB[0][0] + (DB[1],), DP[0][0] + (DP[1],), side, kind, H.HMJ_MATERIALIZE, probe_fill=PFILL,
                                        build_fill=BFILL)
        rb = ex.str_kind_rows_to_numpy(b)
        assert int(a.n_matches) == int(b.n_matches) > 0 and (int(a.sum_r), int(a.sum_s)) == (int(b.sum_r), int(b.sum_s)), (side, kind)
        have = [2, 4] if (side, kind) in SEMI_ANTI[:2] else [1, 3] if (side, kind) in SEMI_ANTI else [1, 2, 3, 4]  # the kind's columns
        assert np.array_equal(unordered(ra[:, have]), unordered(rb[:, have])), (side, kind)
        assert {k: ia[k] for k in COUNT_KEYS} == {k: ib[k] for k in COUNT_KEYS}, (side, kind)
        assert ia["n_collisions"] == ib["n_collisions"] == 0


# ---- argument errors ---------------------------------------------------------------------------------------------------------
def test_argument_errors(H, ex):
    """Every HMJ_E_ARG of the header, each followed by a call that succeeds on the same ctx."""
    import torch

    n = 100
    rng = random.Random(5)
    B, P = relations(rng, ["s", 4], n, n)
    DB, DP = dev(H, B), dev(H, P)
    L = ex.L

    def call(mut=None, flags=0, bits=0, side=PROBE, kind=INNER, size=None, rb_none=False):
        ex._sync_stream()
        rb, kb = ex._mixed_rel(DB[0], DB[1], None, "build")
        rp, kp = ex._mixed_rel(DP[0], DP[1], None, "probe")
        o = H.MixedOpts()
        o.struct_size = C.sizeof(H.MixedOpts) if size is None else size
        o.side, o.kind, o.hash_bits = side, kind, bits
        if mut:
            mut(rb, rp)
        res = H.ColsResult()
        rc = L.hmj_join_mixed_device(ex.h, None if rb_none else C.byref(rb), C.byref(rp), flags, C.byref(o), C.byref(res))
        return rc, L.hmj_last_error(ex.h).decode(), res

    def bad(msg_has, **kw):
        rc, msg, _ = call(**kw)
        assert rc == HMJ_E_ARG, (kw, rc, msg)
        for m in (msg_has,) if isinstance(msg_has, str) else msg_has:
            assert m in msg, (msg, m)
        rc, msg, res = call()  # the ctx stays usable
        assert rc == 0 and int(res.n_matches) == good, (rc, msg)

    rc, _, res = call()
    good = int(res.n_matches)
    assert rc == 0 and good == int(expect(H, B, P, PROBE, INNER)[0].shape[0]) > 0

    def setter(rel, col, **fields):
        def mut(rb, rp):
            r = rb if rel == "build" else rp
            for k, v in fields.items():
                setattr(r.cols[col], k, v)
        return mut

    def rel_setter(**fields):
        def mut(rb, rp):
            for k, v in fields.items():
                setattr(rp, k, v)
        return mut

    # what the column join rejects
    bad("relation is NULL", rb_none=True)
    bad("struct_size", size=24)
    bad("side", side=2)
    bad("kind", side=PROBE, kind=4)
    bad("kind", side=BUILD, kind=0)
    bad("hash_bits", bits=64)
    bad("FIRST_WINS", flags=H.HMJ_FIRST_WINS)
    bad("n_cols", mut=rel_setter(n_cols=0))
    bad("n_cols", mut=rel_setter(n_cols=9))
    bad("cols is NULL", mut=rel_setter(cols=C.cast(None, C.POINTER(H.MixedCol))))
    bad("reserved", mut=rel_setter(reserved=1))
    bad("too many rows", mut=rel_setter(n=1 << 32))
    bad("different n_cols", mut=rel_setter(n_cols=1))
    bad(("column 1", "width 3"), mut=setter("build", 1, width=3))
    bad(("build", "column 1", "data is NULL"), mut=setter("build", 1, data=None))
    bad(("probe", "column 1", "aligned"), mut=setter("probe", 1, data=DP[0][1].data_ptr() + 2))
    # the mixed entry's own
    bad(("column 0", "unknown type 7"), mut=setter("build", 0, type=7))
    bad(("column 0", "string column has width"), mut=setter("probe", 0, width=8))
    bad(("column 1", "offsets"), mut=setter("build", 1, offsets=DB[0][0][1].data_ptr()))
    bad(("column 0", "offsets is NULL"), mut=setter("probe", 0, offsets=None))
    bad(("column 1", "width 4 on the build side", "width 2 on the probe side"), mut=setter("probe", 1, width=2))
    u8 = torch.zeros(n * 8, dtype=torch.uint8, device="cuda")
    bad(("column 0", "type 1", "type 0"), mut=setter("probe", 0, type=H.HMJ_KEY_FIXED, width=8, data=u8.data_ptr(), offsets=None))
    bits_t = H.pack_validity(np.ones(n, bool), 0, "cuda")

    def overflow(rb, rp):
        rp.cols[1].validity.bits = bits_t.data_ptr()
        rp.cols[1].validity.bit_offset = M64 - 5
    bad(("probe", "column 1", "bit_offset"), mut=overflow)
    bad(("build", "column 0", "data is NULL but keys have bytes"), mut=setter("build", 0, data=None))
    # decreasing offsets, found on the device: column 1 of the probe side, column 0 fine -- the first bad row is named
    B2, P2 = relations(rng, ["s", "s"], 300, 300)
    D2B, D2P = dev(H, B2), dev(H, P2)
    off = D2P[0][1][1].clone()
    host = off.cpu().numpy()
    for row in (200, 70):  # offsets[row + 1] < offsets[row]
        host[row] = host[row + 1] + 3
    worse = torch.from_numpy(host).cuda()
    for side, kind, flags in ((PROBE, INNER, 0), (BUILD, FULL_OUTER, H.HMJ_ORDERED), (PROBE, SEMI, H.HMJ_MATERIALIZE)):
        with pytest.raises(H.HmjError) as e:
            ex.join_mixed_device(D2B[0], D2B[1], [D2P[0][0], (D2P[0][1][0], worse)], D2P[1], side, kind, flags)
        assert e.value.code == HMJ_E_ARG and "probe relation: column 1: offsets decrease at row 70 " in str(e.value), str(e.value)
        check(H, ex, B2, P2, D2B, D2P, kinds=[(side, kind)], tag=("after bad offsets",))
    # ... and with bitmaps (the other key kernel); both relations bad: the build relation is named
    P2v = Rel(P2.cols, P2.vals, [np.arange(300) % 3 != 0, None])
    D2Pv = dev(H, P2v, bit_off=3)
    with pytest.raises(H.HmjError) as e:
        ex.join_mixed_device([(D2P[0][0][0], worse), D2B[0][1]], D2B[1], [D2Pv[0][0], (D2Pv[0][1][0], worse)], D2Pv[1], BUILD, FULL_OUTER, 0,
                             probe_valid=D2Pv[2])
    assert e.value.code == HMJ_E_ARG and "build relation: column 0: offsets decrease at row 70 " in str(e.value), str(e.value)
    with pytest.raises(H.HmjError) as e:
        ex.join_mixed_device(D2B[0], D2B[1], [D2Pv[0][0], (D2Pv[0][1][0], worse)], D2Pv[1], PROBE, ANTI, 0, probe_valid=D2Pv[2])
    assert e.value.code == HMJ_E_ARG and "probe relation: column 1: offsets decrease at row 70 " in str(e.value), str(e.value)
    check(H, ex, B2, P2v, D2B, D2Pv, kinds=[(BUILD, FULL_OUTER)], tag=("after bad offsets, bitmaps",))


@pytest.mark.parametrize("side,kind", [(PROBE, INNER), (BUILD, FULL_OUTER)])
def test_bad_offsets_under_a_bitmap_then_the_right_ones(H, ex, side, kind):
    """[str, u32], 600 rows a side, a bitmap on the probe relation's string column, its offsets decreasing at row 70: the
    second wave of the first workgroup compacts nothing, so the two workgroups behind it compact in front of their places,
    into an array that has room for every row.  Materialising, the call fails with HMJ_E_ARG naming relation, column and
    row; the same call with the offsets put right, on the same context, is the brute force's."""
    import torch

    rng = random.Random(8070)
    B, P = relations(rng, ["s", 4], 600, 600)
    P.valid = draw_masks(np.random.default_rng(8070), P.n, 2, [0])
    P.valid[0][70] = True
    assert P.valid[0][256:].sum() > 64
    DB, DP = dev(H, B), dev(H, P, bit_off=3)
    chars, off = DP[0][0]
    host = off.cpu().numpy().copy()
    host[70] = host[71] + 3  # offsets[71] < offsets[70]
    flags = H.HMJ_MATERIALIZE | H.HMJ_CHECKSUM | H.HMJ_SUM_PROBE
    with pytest.raises(H.HmjError) as e:
        ex.join_mixed_device(DB[0], DB[1], [(chars, torch.from_numpy(host).cuda()), DP[0][1]], DP[1], side, kind, flags, probe_fill=PFILL,
                             build_fill=BFILL, probe_valid=DP[2])
    assert e.value.code == HMJ_E_ARG and "probe relation: column 0: offsets decrease at row 70 " in str(e.value), str(e.value)
    check(H, ex, B, P, DB, DP, kinds=[(side, kind)], modes=(flags,), tag=("offsets put right",))


# ---- end to end: the key columns back through the row maps ---------------------------------------------------------------------
def test_take_the_key_columns_back(H, ex):
    """Ordered FULL_OUTER on [str, i32] with NULLs; both key columns taken through r_row and s_row with hmj_take_str_device /
    hmj_take_cols_device; coalesced, they are the expectation's tuples, NULL where NO_ROW stands or the key slot is NULL."""
    rng = random.Random(404)
    nrng = np.random.default_rng(404)
    B, P = relations(rng, ["s", 4], 600, 800)
    B.valid, P.valid = draw_masks(nrng, B.n, 2, [0, 1], 0.15), draw_masks(nrng, P.n, 2, [0], 0.15)
    DB, DP = dev(H, B, bit_off=3), dev(H, P, base=7, first=2)
    want = expect(H, B, P, BUILD, FULL_OUTER)[0]
    res, info, rows = run(H, ex, DB, DP, BUILD, FULL_OUTER, H.HMJ_ORDERED)
    n = int(res.n_matches)
    assert np.array_equal(rows, want) and n > 0
    got = {}
    for name, D, col in (("r", DB, res.r_row), ("s", DP, res.s_row)):
        v = D[2] or [None, None]
        ch, off, words, i1 = ex.take_str_device(D[0][0][0], D[0][0][1], (col, n), valid=v[0])
        days, dwords, i2 = ex.take_cols_device([D[0][1]], (col, n), valid=[v[1]])
        got[name] = (H.unpack_strings(ch, off, H.unpack_validity(words, n)), days[0].cpu().numpy().view(np.uint32),
                     H.unpack_validity(dwords[0], n))
    tb, tp = B.tuples(), P.tuples()
    assert (want[:, 1] == NO_ROW).any() and (want[:, 2] == NO_ROW).any() and B.null().any() and P.null().any()
    for i, (k, r, s, _, _) in enumerate(want.tolist()):
        for name, row, R, tt in (("r", r, B, tb), ("s", s, P, tp)):
            name_s, day, day_ok = got[name][0][i], got[name][1][i], got[name][2][i]
            if row == NO_ROW:
                assert name_s is None and not day_ok
                continue
            m0 = R.valid[0] is None or R.valid[0][row]
            m1 = R.valid[1] is None or R.valid[1][row]
            assert name_s == (tt[row][0] if m0 else None) and bool(day_ok) == bool(m1) and (not m1 or int(day) == tt[row][1]), (i, name)
        if r != NO_ROW and s != NO_ROW:  # a pair: both sides hold the same, non-NULL key
            assert got["r"][0][i] == got["s"][0][i] is not None and got["r"][1][i] == got["s"][1][i]


# ---- planner isolation -------------------------------------------------------------------------------------------------------
def test_mixed_joins_teach_the_other_entries_nothing(H):
    """Mixed joins with duplicate tuples teach their workloads a cool-down; a u64 join and a column join of the same sizes on
    the same ctx must still plan exactly as on a fresh ctx, and the mixed entry's workloads carry kind codes 20..24."""
    import torch

    n = 1 << 20
    half = np.arange(n // 2, dtype=np.int64)
    twice = np.concatenate([half, half])  # every tuple twice on each side
    c0 = torch.from_numpy(twice).cuda()
    c1 = torch.from_numpy(twice.astype(np.int32)).cuda()
    name = (torch.from_numpy(np.frombuffer(twice.astype(">u8").tobytes(), np.uint8).copy()).cuda(),  # 8 bytes a key
            torch.arange(n + 1, dtype=torch.int64, device="cuda") * 8)
    fresh = H.Executor(0)
    B, P = fresh.gen_build(n), fresh.gen_probe(n, n, miss_mod=3)
    fresh.join_device(B, P, H.HMJ_MATERIALIZE | H.HMJ_CHECKSUM)
    p_u64 = fresh.last_plan()
    fresh.join_cols_device([c0, c1], None, [c0, c1], None, H.HMJ_MATERIALIZE)
    p_cols = fresh.last_plan()
    fresh.close()
    ex2 = H.Executor(0)
    learnt, seen = 0, set()
    for side, kind in ((PROBE, INNER), (PROBE, SEMI), (BUILD, BUILD_ANTI), (PROBE, PROBE_OUTER), (BUILD, FULL_OUTER)):
        for _ in range(3):
            res, info = ex2.join_mixed_device([name, c1], None, [name, c1], None, side, kind, H.HMJ_MATERIALIZE)
            assert int(res.n_matches) == (0 if kind == BUILD_ANTI else n if kind == SEMI else 2 * n)
            assert info["n_collisions"] == 0
        p = ex2.last_plan()
        seen.add((p["workload"] >> 20) & 31)
        learnt |= p["cooling"]
    assert seen == {20, 21, 22, 24}, seen  # (23, the ambiguous rows' join, runs only after a collision)
    ex2.join_device(B, P, H.HMJ_MATERIALIZE | H.HMJ_CHECKSUM)
    assert ex2.last_plan() == p_u64
    ex2.join_cols_device([c0, c1], None, [c0, c1], None, H.HMJ_MATERIALIZE)
    assert ex2.last_plan() == p_cols
    ex2.close()
    assert learnt, "the mixed joins taught their workloads nothing: the test would not see a shared memo"


# ---- seeded sweep ------------------------------------------------------------------------------------------------------------
def draw_case(rng, nrng, H):
    """One drawn call: layout, sizes, duplicates, misses, bitmaps, hash bits, kind and flags; and whether some wave of a
    string column is sure to take the unstaged path (a span beyond the stage whatever its alignment)."""
    k = rng.randrange(1, 5)
    layout = [rng.choice(("s", 1, 2, 4, 8)) for _ in range(k)]
    if rng.randrange(4) and "s" not in layout:
        layout[rng.randrange(k)] = "s"
    side, kind = rng.choice(ALL_KINDS)
    flags = rng.choice((H.HMJ_ORDERED, H.HMJ_ORDERED, H.HMJ_MATERIALIZE, 0)) | H.HMJ_CHECKSUM | H.HMJ_SUM_PROBE
    bits = rng.choice((0, 0, 2, 6, 12, 40))
    small = bool(flags & H.HMJ_ORDERED) and 0 < bits < 16  # the whole result within the collision sort's 1024 rows
    nb, np_ = (rng.randrange(1, 200), rng.randrange(1, 200)) if small else (rng.randrange(1, 2001), rng.randrange(1, 2001))
    long_share = rng.choice((0.0, 0.0, 0.6))
    bt, pt = drawn(rng, layout, nb, np_, miss=rng.choice((0.1, 0.33, 0.6)), copies=2 if small else rng.choice((None, 1, 3)),
                   long_share=long_share)
    nb, np_ = len(bt), len(pt)
    B = Rel(columns(bt, layout), rng.choice((None, [rng.getrandbits(64) for _ in bt])))
    P = Rel(columns(pt, layout), rng.choice((None, [rng.getrandbits(64) for _ in pt])))
    for R in (B, P):
        if rng.randrange(2):
            R.valid = draw_masks(nrng, R.n, k, [c for c in range(k) if rng.randrange(2)], rng.choice((0.05, 0.4)))
            if all(m is None for m in R.valid):
                R.valid = None
    unstaged = False
    for R in (B, P):
        for c in R.cols:
            if not isinstance(c, np.ndarray):
                lens = [len(x) for x in c]
                unstaged = unstaged or any(sum(lens[i:i + 64]) > STAGE + 32 for i in range(0, len(lens), 64))
    return B, P, side, kind, flags, bits, unstaged


def test_seeded_sweep(H, ex):
    """HMJ_STRESS_SEED / HMJ_STRESS_ITERS (default 20 iterations): drawn calls against the brute force.  The default seed
    must reach the unstaged span, the ambiguous list, the collision sort and the NULL tail."""
    seed = int(os.environ.get("HMJ_STRESS_SEED", "20261019"))
    iters = int(os.environ.get("HMJ_STRESS_ITERS", "20"))
    rng, nrng = random.Random(seed), np.random.default_rng(seed)
    seen = set()
    for it in range(iters):
        B, P, side, kind, flags, bits, unstaged = draw_case(rng, nrng, H)
        base, first, off = rng.choice((0, 1, 7, 15)), rng.choice((0, 3)), rng.choice((0, 3, 13))
        s, _ = check(H, ex, B, P, dev(H, B, base, first, off), dev(H, P, 0, first, off), bits=bits, kinds=[(side, kind)], modes=(flags,),
                     tag=("sweep", seed, it))
        seen |= s | ({"unstaged"} if unstaged else set())
    print("sweep reached", sorted(seen))
    if "HMJ_STRESS_SEED" not in os.environ and "HMJ_STRESS_ITERS" not in os.environ:
        assert {"unstaged", "ambiguous", "sort", "tail"} <= seen, seen


# ---- one larger case ---------------------------------------------------------------------------------------------------------
def test_larger_case(H, ex):
    """[str, u32] at 2^16 x 2^16 rows with duplicates and a 25 % miss share: inner ordered and full outer count."""
    rng = random.Random(65536)
    n = 1 << 16
    pool = [(b"name-%06d-%s" % (i, b"x" * (i % 13)), i % 7) for i in range(n // 2)]
    miss = [(b"none-%06d" % i, i % 7) for i in range(n // 8)]
    bt = [pool[rng.randrange(len(pool))] for _ in range(n)]
    pt = [miss[rng.randrange(len(miss))] if rng.randrange(4) == 0 else pool[rng.randrange(len(pool))] for _ in range(n)]
    layout = ["s", 4]
    B, P = Rel(columns(bt, layout), [rng.getrandbits(64) for _ in bt]), Rel(columns(pt, layout))
    DB, DP = dev(H, B), dev(H, P)
    check(H, ex, B, P, DB, DP, kinds=[(PROBE, INNER)], modes=(H.HMJ_ORDERED | H.HMJ_CHECKSUM | H.HMJ_SUM_PROBE,), tag=("large",))
    check(H, ex, B, P, DB, DP, kinds=[(BUILD, FULL_OUTER)], modes=(H.HMJ_CHECKSUM | H.HMJ_SUM_PROBE,), tag=("large",))
