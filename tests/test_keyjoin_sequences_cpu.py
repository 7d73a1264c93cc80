"""Generators for the tours of the key-join, take and group entries on ONE long-lived context (test_keyjoin_sequences_gpu.py
runs them) and their CPU-only checks.  The method is test_ctx_sequences_cpu.py's -- `draw_tour`, `transitions`, `Model` and the
flag constants are imported from there --, the entries are the ones merged since: hmj_join_cols_device,
hmj_join_kind_cols_device (bitmaps, HMJ_NULL_EQUAL), hmj_join_mixed_device, hmj_take_cols_device, hmj_take_str_device and
hmj_group_cols_device, with hmj_join_kind_str_device and the u64 entries between them because they share `memo_join`, the
u64 driver's buffers and the sort.

  * `KeyPool`: the cases of one seed, drawn once on the host.  Row counts come from ROWS (the edges of a wave, a 256-lane
    workgroup, the 1024-row run cap, the 512 positions one wave and the 2048 one workgroup of group_agg_kernel walk); one
    packed column case and one group case have 65 537 rows, one of each 300 001 (numpy references: unique build tuples and
    a sort-merge for the join, `expected_groups` for the groups).  Expectations are computed once per (case, kind, form,
    NULL semantics) by the references of the family files: expected_kind_rows, expected_null_kind_rows, ne_rows,
    expected_null_str_kind_rows (kind_brute), expected_take, expected_take_str, H.expected_groups, expect_inner.  The
    SQL-semantics expectation of the mixed entry lives in test_join_mixed_gpu.py (`expect`), which a CPU file does not
    import: the GPU file hands it in (`KeyPool.mixed_sql`), and the checks here show for such an op only that it names a
    case, a kind and a status;
  * eleven op families and `draw_key_sequence`: 122 ops per tour, every ordered pair of families adjacent once, with the
    chains u64 (prepare) -> take_cols -> take_str -> u64 (the join of the prepared tensor, which may take it) and u64 (prepare)
    -> group -> u64 (the same join, which must not);
  * `KeyModel(Model)`: which ops discard a prepared build side, the status of every op, the forced bits and the prefix hint
    in force, and which op's result must survive the next op (only a take keeps it);
  * `largest_mixed_run`: the run cap of the hashed forms from key64 and the tuples alone -- a draw beyond it is kept and its
    ordered op expects HMJ_E_UNSUPPORTED; at most one op in ten of a tour may be such a draw."""
import time
from collections import Counter

import numpy as np

from test_ctx_sequences_cpu import (CHECKSUM, E_ARG, E_UNSUPPORTED, FORCED_BITS, KIND_MODES, MATERIALIZE, ORDERED, SEQ_SEED, SEQ_TOURS,
                                    SUM_PROBE, Model, draw_tour, expect_inner, materialising, transitions)
from test_group_cols_cpu import draw_columns, draw_valid, tuples_of
from test_join_cols_kinds_cpu import (ALL_KINDS, ANTI, BUILD, BUILD_OUTER, COUNT_KEYS, FULL_OUTER, INNER, M64, NO_ROW, PROBE, PROBE_OUTER,
                                      SEMI, expected_kind_rows)
from test_join_cols_nulls_cpu import expected_null_kind_rows
from test_join_null_equal_cpu import ne_rows
from test_join_str_nulls_cpu import expected_null_str_kind_rows
from test_kinds_sweep_cpu import draw_str_case, draw_u64_case
from test_take_cols_cpu import expected_take
from test_take_str_cpu import expected_take_str

NULL_EQUAL = 0x20  # HMJ_NULL_EQUAL (test_the_constants_are_the_bindings below)
GROUP_WANT_ALL = 0x1F
COLS_PACKED, COLS_HASHED = 1, 2
RUN_CAP = 1024  # kRunCap
PFILL, BFILL = 0xF1, 2 ** 64 - 2  # the fills of the family files (test_join_mixed_gpu.expect writes its own into the rows)

FAMILIES = ("cols_inner", "cols_kind", "cols_null_equal", "mixed", "group", "take_cols", "take_str", "str_kind", "u64", "config",
            "refused")
# the takes are the only calls that may stand between a prepare and its join; and a group call directly between a prepare and
# the join of the same tensor (every key join discards a prepared build side rightly, so a group call that left it valid can
# only show when nothing else stands between them)
REQUIRED_CHAINS = (("u64", "take_cols", "take_str", "u64"), ("u64", "group", "u64"))
ROWS = [1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097]
DICT_ROWS = 4097            # rows per side of a case whose expectation is a Python dict of tuples
BIG_ROWS = (65537, 300001)  # one packed column case and one group case of each
COL_LAYOUTS = ([4], [4, 4], [8, 4, 2], [1] * 8)
# the entries of test_join_mixed_gpu.LAYOUTS (the GPU file asserts it)
MIXED_LAYOUTS = (["s", 4], [2, "s", 8], ["s", "s"], ["s"], [4, 4, 4])
BIT_OFFSETS = (0, 3, 67)
HASH_BITS = (0, 0, 0, 6, 7, 8, 9, 10)
COLS_INNER_FLAGS = (0, CHECKSUM, MATERIALIZE | CHECKSUM, ORDERED | CHECKSUM, ORDERED | SUM_PROBE)
GROUP_FLAGS = (0, MATERIALIZE, ORDERED)
PREFIX_HINTS = (1, 16, 48)
N_COLS, N_MIXED, N_GROUPS, N_STR, N_U64 = 8, 6, 6, 4, 2
STR_POOL_KEYS = (60, 1200)
PREPARE_ROWS = 300001  # the u64 case a prepare goes to: large enough for a partitioned plan
LARGEST_U64 = 400001   # one u64 case beyond it
REFUSALS = ("width_3", "unknown_kind", "group_first_wins", "str_kind_null_equal", "take_map_beyond_source", "mixed_decreasing_offsets",
            "cols_run_cap_ordered", "group_run_cap")
RAN = ("cols_run_cap_ordered", "group_run_cap")  # refusals that run (HMJ_E_UNSUPPORTED) and discard a prepared build side
CAP_SHARE = 10  # at most one op in CAP_SHARE of a tour may be a draw beyond the run cap
KIND_FAMILIES = {"cols": ("cols_inner", "cols_kind", "cols_null_equal"), "mixed": ("mixed",), "groups": ("group",), "strs": ("str_kind",),
                 "u64": ("u64",)}
KEY_FAMILIES = ("cols_inner", "cols_kind", "cols_null_equal", "mixed", "str_kind")


# ---- the run cap, from key64 and the tuples alone -------------------------------------------------------------------------------
def largest_mixed_run(tb, tp, kb, kp, side, kind):
    """Rows of the largest run of equal key64 that holds several distinct tuples among the RESULT rows of a kind (the rows
    the ordered call sorts: hmj.h counts the limit over result rows).  tb / tp: the rows' tuples (rows that take part in
    matching only: without the NULL-key rows under SQL semantics, with None in NULL slots under HMJ_NULL_EQUAL); kb / kp:
    their key64."""
    cb, cp = Counter(tb), Counter(tp)
    key_of = {t: int(k) for t, k in zip(tp, kp)}
    key_of.update((t, int(k)) for t, k in zip(tb, kb))
    runs = {}
    for t, k in key_of.items():
        b, p = cb.get(t, 0), cp.get(t, 0)
        if side == PROBE:
            n = {INNER: b * p, SEMI: p if b else 0, ANTI: 0 if b else p, PROBE_OUTER: b * p if b else p}[kind]
        else:  # BUILD_SEMI, BUILD_ANTI, BUILD_OUTER, FULL_OUTER = 1, 2, 3, 4
            n = {1: b if p else 0, 2: 0 if p else b, BUILD_OUTER: b * p if p else b, FULL_OUTER: b * p if b and p else b + p}[kind]
        if n:
            runs.setdefault(k, []).append(n)
    return max((sum(v) for v in runs.values() if len(v) > 1), default=0)


# ---- drawing relations ------------------------------------------------------------------------------------------------------------
def _vals(rng, n):
    return rng.integers(0, 1 << 64, size=n, dtype=np.uint64) if rng.random() < 0.7 else None


def _masks(rng, n, k, which):
    """which: "none", "some" or "all" columns get a bitmap"""
    if which == "none":
        return None
    cols = set(range(k)) if which == "all" else {int(c) for c in rng.choice(k, size=max(1, k // 2), replace=False)}
    # (under HMJ_NULL_EQUAL the NULLs of a column match each other: few of them in a large relation, or a one-column case
    #  is a cross product of its NULL rows)
    return draw_valid(rng, n, k, float(rng.choice([0.05, 0.3])) if n <= 600 else 0.03, cols)


def draw_cols_case(rng, widths, nb, np_, bits, which):
    """Two relations over one pool of tuples (test_group_cols_cpu.draw_columns) with duplicates and misses on both sides:
    build rows from the first three quarters of the pool, probe rows from the last three."""
    card = max(4, (nb + np_) // 3)
    base = draw_columns(rng, card, widths, card)
    ib = rng.integers(0, max(1, card * 3 // 4), size=nb)
    ip = rng.integers(card // 4, card, size=np_)
    side = lambda idx, n: dict(cols=[c[idx] for c in base], vals=_vals(rng, n), masks=_masks(rng, n, len(widths), which),
                               off=int(rng.choice(BIT_OFFSETS)), n=n)
    return dict(widths=list(widths), b=side(ib, nb), p=side(ip, np_), bits=int(bits), rows=(nb, np_), big=None)


def draw_big_cols_case(rng, n):
    """n x n rows, [4, 4] packed, in the manner of test_join_cols_kinds_gpu.make_big: unique build tuples (a, b) whose a fills
    all 32 bits and is unique by itself, probe rows drawn from them with repeats, every second one changed in b to a tuple
    the build side does not hold.  The expectation comes from numpy: a sort-merge on a pairs the rows, b confirms them."""
    with np.errstate(over="ignore"):
        a = (rng.permutation(n).astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15)).astype(np.uint32)  # an odd factor: a bijection mod 2^32
    b = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    pick = rng.integers(0, n, n)
    pa, pb = a[pick].copy(), b[pick].copy()
    pb[::2] ^= np.uint32(0x80000000)
    bv, pv = rng.integers(0, 1 << 63, n, dtype=np.uint64), rng.integers(0, 1 << 63, n, dtype=np.uint64)
    order = np.argsort(a, kind="stable")
    r_of = order[np.minimum(np.searchsorted(a[order], pa), n - 1)]
    hit = (a[r_of] == pa) & (b[r_of] == pb)
    assert len(np.unique(a)) == n and np.array_equal(hit, np.arange(n) % 2 == 1) and np.array_equal(r_of, pick)
    b_hit = np.zeros(n, bool)
    b_hit[r_of[hit]] = True
    big = dict(hit=hit, r_of=r_of, b_hit=b_hit)
    side = lambda cols, vals: dict(cols=cols, vals=vals, masks=None, off=0, n=n)
    return dict(widths=[4, 4], b=side([a, b], bv), p=side([pa, pb], pv), bits=0, rows=(n, n), big=big)


BIG_KINDS = ((PROBE, INNER), (PROBE, SEMI), (BUILD, FULL_OUTER))


def big_cols_expect(c, side, kind, key64_of):
    """(ordered rows, counters, (n_key_pairs, n_collisions)) of a big packed case for one of BIG_KINDS."""
    big, B, P = c["big"], c["b"], c["p"]
    kb, kp = key64_of(B["cols"]), key64_of(P["cols"])
    assert len(np.unique(kb)) == len(kb)  # ((key64, r_row, s_row) orders the rows)
    hit, r_of, b_hit, bv, pv = big["hit"], big["r_of"], big["b_hit"], B["vals"], P["vals"]
    s_hit, s_miss, r_miss = np.flatnonzero(hit), np.flatnonzero(~hit), np.flatnonzero(~b_hit)
    u = lambda x: np.asarray(x).astype(np.uint64)
    fill = lambda k, v: np.full(k, v, np.uint64)
    inner = np.stack([kp[s_hit], u(r_of[s_hit]), u(s_hit), bv[r_of[s_hit]], pv[s_hit]], 1)
    counts = dict.fromkeys(COUNT_KEYS, 0)
    if (side, kind) == (PROBE, INNER):
        rows = inner
    elif (side, kind) == (PROBE, SEMI):
        rows = np.stack([kp[s_hit], fill(len(s_hit), 0), u(s_hit), fill(len(s_hit), 0), pv[s_hit]], 1)
        counts.update(n_probe_matched=len(s_hit), n_probe_unmatched=len(s_miss))
    else:
        rows = np.concatenate([inner, np.stack([kp[s_miss], fill(len(s_miss), NO_ROW), u(s_miss), fill(len(s_miss), PFILL), pv[s_miss]], 1),
                               np.stack([kb[r_miss], u(r_miss), fill(len(r_miss), NO_ROW), bv[r_miss], fill(len(r_miss), BFILL)], 1)])
        counts.update(n_probe_matched=len(s_hit), n_probe_unmatched=len(s_miss), n_build_matched=len(kb) - len(r_miss),
                      n_build_unmatched=len(r_miss))
    rows = rows[np.lexsort((rows[:, 2], rows[:, 1], rows[:, 0]))]
    return np.ascontiguousarray(rows), counts, (len(s_hit), 0)


WORDS = [b"", b"a", b"ab", b"\x00", b"key", b"key\x00", b"\xff\xfe", b"alphabet", b"alphabets"]


def draw_mixed_case(rng, layout, nb, np_, bits, which):
    """Key tuples over `layout` ("s" or a width per column), None in a NULL slot (the representation of
    test_join_null_equal_gpu.Rel): at most 24 values per column -- the extremes, the empty string, strings of about 100
    bytes --, a pool of distinct tuples, build rows from its first three quarters, probe rows from its last three."""
    def values(typ):
        if typ == "s":
            out = set(WORDS[:int(rng.integers(3, len(WORDS) + 1))])
            while len(out) < 24:
                n = int(rng.integers(90, 130)) if rng.random() < 0.15 else int(rng.integers(1, 14))
                out.add(b"k" + rng.integers(0, 256, size=n, dtype=np.uint8).tobytes())
            return sorted(out)
        top = (1 << (8 * typ)) - 1
        return sorted({0, 1, top, top - 1} | {int(x) for x in rng.integers(0, top, size=20, dtype=np.uint64)})

    vals = [values(typ) for typ in layout]
    k = len(layout)
    want = min(max(4, (nb + np_) // 3), 24 ** k // 2)
    pool = set()
    while len(pool) < want:
        pool.add(tuple(v[int(rng.integers(0, len(v)))] for v in vals))
    pool = sorted(pool)
    pool = [pool[i] for i in rng.permutation(len(pool))]
    card = len(pool)

    def side(lo, hi, n):
        rows = [pool[int(i)] for i in rng.integers(lo, hi, size=n)]
        bitmap = [] if which == "none" else sorted(range(k) if which == "all" else {int(c) for c in rng.choice(k, size=max(1, k // 2), replace=False)})
        frac = float(rng.choice([0.05, 0.3]))
        rows = [tuple(None if c in bitmap and rng.random() < frac else v for c, v in enumerate(t)) for t in rows]
        v = _vals(rng, n)
        return dict(rows=rows, vals=None if v is None else [int(x) for x in v], bitmap=bitmap, off=int(rng.choice(BIT_OFFSETS)), n=n)

    return dict(layout=list(layout), b=side(0, max(1, card * 3 // 4), nb), p=side(card // 4, card, np_), bits=int(bits), rows=(nb, np_))


def mixed_columns(layout, side):
    """The columns as they go to the device and into mixed_key64: zeros / no bytes under a NULL slot."""
    return [[b"" if t[c] is None else t[c] for t in side["rows"]] if typ == "s"
            else np.array([0 if t[c] is None else t[c] for t in side["rows"]], "u%d" % typ) for c, typ in enumerate(layout)]


def mixed_masks(layout, side):
    """per column None or a bool array (True = valid)"""
    return [np.array([t[c] is not None for t in side["rows"]], bool) if c in side["bitmap"] else None for c in range(len(layout))]


def draw_group_case(rng, widths, n, card, bits, which, force):
    return dict(widths=list(widths), cols=draw_columns(rng, n, widths, card), vals=_vals(rng, n), valid=_masks(rng, n, len(widths), which),
                off=int(rng.choice(BIT_OFFSETS)), bits=int(bits), force=bool(force), n=n)


def _null_rows(masks, n):
    out = np.zeros(n, bool)
    for m in masks or ():
        if m is not None:
            out |= ~m
    return out


def _val_list(side):
    return list(range(side["n"])) if side["vals"] is None else [int(v) & M64 for v in side["vals"]]


# ---------------------------------------------------------------------------------------------
class KeyPool:
    """The cases of one seed and their expectations, each computed once.  H: the hashmergejoin_amd module (cols_key64,
    mixed_key64, expected_groups: host code)."""

    def __init__(self, seed, H):
        rng = np.random.default_rng([int(seed), 11])
        self.seed, self.H = int(seed), H
        self.mixed_sql = None  # test_join_mixed_gpu's Rel and expect, handed in by the GPU file
        size = lambda: int(rng.choice(ROWS))
        whiches = ["none", "some", "all"]
        self.cols = []
        for i in range(N_COLS):
            widths = COL_LAYOUTS[i % len(COL_LAYOUTS)]
            # the first four cases are large and carry bitmaps: a smaller case without them has something to follow
            nb, np_ = (int(rng.choice(ROWS[-6:])), int(rng.choice(ROWS[-6:]))) if i < 4 else (size(), size())
            self.cols.append(draw_cols_case(rng, widths, nb, np_, rng.choice(HASH_BITS), "all" if i < 2 else "some" if i < 4 else whiches[i % 3]))
        for n in BIG_ROWS:
            self.cols.append(draw_big_cols_case(rng, n))
        self.mixed = []
        for i in range(N_MIXED):
            layout = MIXED_LAYOUTS[i % len(MIXED_LAYOUTS)]
            nb, np_ = (int(rng.choice(ROWS[-6:])), int(rng.choice(ROWS[-6:]))) if i < 2 else (size(), size())
            self.mixed.append(draw_mixed_case(rng, layout, nb, np_, rng.choice(HASH_BITS), "all" if i < 2 else whiches[i % 3]))
        self.groups = []
        for i in range(N_GROUPS):
            n = int(rng.choice(ROWS[-6:])) if i < 2 else size()
            self.groups.append(draw_group_case(rng, COL_LAYOUTS[(i + 1) % len(COL_LAYOUTS)], n, int(rng.choice([3, 40, 700, 5000])),
                                               rng.choice(HASH_BITS), "some" if i < 2 else whiches[i % 3], i % 2 == 1))
        self.groups.append(draw_group_case(rng, [8, 4, 2], BIG_ROWS[0], 9000, 0, "some", False))
        self.groups.append(draw_group_case(rng, [4, 4], BIG_ROWS[1], 70000, 0, "none", False))
        self.strs = []
        while len(self.strs) < N_STR:
            c = draw_str_case(rng, sizes=STR_POOL_KEYS)
            if max(len(c["bk"]), len(c["pk"])) > DICT_ROWS:
                continue
            with_masks = len(self.strs) % 2 == 0
            c["bmask"] = rng.random(len(c["bk"])) >= 0.2 if with_masks else None
            c["pmask"] = rng.random(len(c["pk"])) >= 0.2 if with_masks else None
            c["off_b"], c["off_p"] = int(rng.choice(BIT_OFFSETS)), int(rng.choice(BIT_OFFSETS))
            self.strs.append(c)
        self.u64 = []
        for i in range(N_U64):
            B, P, fills, tag = draw_u64_case(rng, sizes=ROWS)
            self.u64.append(dict(B=B, P=P, fills=fills, tag=tag, rows=(len(B), len(P))))
        B, P, fills, tag = draw_u64_case(rng, sizes=[PREPARE_ROWS])
        self.prepare_case = len(self.u64)
        self.u64.append(dict(B=B, P=P, fills=fills, tag=tag, rows=(len(B), len(P))))
        B, P, fills, tag = draw_u64_case(rng, sizes=[LARGEST_U64])  # larger than the prepare's: the driver's buffers regrow
        self.u64.append(dict(B=B, P=P, fills=fills, tag=tag, rows=(len(B), len(P))))
        for cases in (self.cols, self.mixed, self.groups, self.strs):  # ascending size: "a smaller case" is a smaller index
            cases.sort(key=self.size_of)
        self._cache = {}

    @staticmethod
    def size_of(c):
        if "rows" in c:
            return sum(c["rows"])
        return c["n"] if "n" in c else len(c["bk"]) + len(c["pk"])

    def relations(self, ci):  # (what test_ctx_sequences_gpu.check_inner asks of a pool)
        return self.u64[ci]["B"], self.u64[ci]["P"]

    # ---- key joins ------------------------------------------------------------------------------------
    def expect_cols(self, ci, side, kind, sem, force):
        """dict(rows, counts, pairs, nulls, form, over, sum_probe) of a column join; rows in the HMJ_ORDERED order.  sem, the
        NULL semantics: "plain" (no bitmap is passed), "sql" (bitmaps: a NULL-key row matches nothing) or "ne" (bitmaps
        under HMJ_NULL_EQUAL)."""
        key = ("cols", ci, side, kind, sem, bool(force))
        if key in self._cache:
            return self._cache[key]
        c, H = self.cols[ci], self.H
        B, P, w, bits = c["b"], c["p"], c["widths"], c["bits"]
        hashed = bool(force) or sum(w) > 8 or sem == "ne"
        nulls = (0, 0)
        if c["big"] is not None:
            assert sem == "plain" and not force and (side, kind) in BIG_KINDS
            rows, counts, pairs = big_cols_expect(c, side, kind, lambda cols: H.cols_key64(cols, w))
            over = False
        else:
            if sem == "ne":
                tb, tp = tuples_of(B["cols"], w, B["masks"]), tuples_of(P["cols"], w, P["masks"])
                kb = H.cols_key64(B["cols"], w, hash_bits=bits, valid=B["masks"], null_equal=True)
                kp = H.cols_key64(P["cols"], w, hash_bits=bits, valid=P["masks"], null_equal=True)
                rows, counts, n_pairs, n_coll, _ = ne_rows(tb, tp, [int(x) for x in kb], [int(x) for x in kp], _val_list(B), _val_list(P),
                                                           side, kind, PFILL, BFILL)
                nulls = (sum(None in t for t in tb), sum(None in t for t in tp))
            else:
                bnull = _null_rows(B["masks"] if sem == "sql" else None, B["n"])
                pnull = _null_rows(P["masks"] if sem == "sql" else None, P["n"])
                if sem == "sql":
                    rows, counts = expected_null_kind_rows(B["cols"], B["vals"], P["cols"], P["vals"], w, side, kind, bnull, pnull, bits,
                                                           force, PFILL, BFILL)
                    nulls = (int(bnull.sum()), int(pnull.sum()))
                else:
                    rows, counts = expected_kind_rows(B["cols"], B["vals"], P["cols"], P["vals"], w, side, kind, bits, force, PFILL, BFILL)
                vb, vp = np.flatnonzero(~bnull), np.flatnonzero(~pnull)
                sb, sp = [col[vb] for col in B["cols"]], [col[vp] for col in P["cols"]]
                tb, tp = tuples_of(sb, w, None), tuples_of(sp, w, None)
                kb, kp = H.cols_key64(sb, w, bits, force), H.cols_key64(sp, w, bits, force)
                # the pairs of equal key64 the call compares: ne_rows counts them (no None among these tuples: plain equality)
                _, _, n_pairs, n_coll, _ = ne_rows(tb, tp, [int(x) for x in kb], [int(x) for x in kp], [0] * len(tb), [0] * len(tp), side, kind)
            pairs = (n_pairs, n_coll)
            over = hashed and largest_mixed_run(tb, tp, kb, kp, side, kind) > RUN_CAP
        out = dict(rows=rows, counts=counts, pairs=pairs, nulls=nulls, form=COLS_HASHED if hashed else COLS_PACKED, over=over,
                   sum_probe=sum(_val_list(P)) & M64)
        self._cache[key] = out
        return out

    def expect_mixed(self, mi, side, kind, sem):
        """As expect_cols; the rows of "plain" and "sql" come from test_join_mixed_gpu.expect (self.mixed_sql), "deferred"
        without it.  "plain": no bitmap is passed, so what lies under a NULL slot (zeros, no bytes) is the value."""
        key = ("mixed", mi, side, kind, sem)
        if key in self._cache:
            return self._cache[key]
        c, H = self.mixed[mi], self.H
        B, P, layout, bits = c["b"], c["p"], c["layout"], c["bits"]
        bcols, pcols = mixed_columns(layout, B), mixed_columns(layout, P)
        bm, pm = mixed_masks(layout, B), mixed_masks(layout, P)
        ne = sem == "ne"
        if sem == "plain":
            under = lambda cols, n: [tuple(int(col[i]) if isinstance(col, np.ndarray) else col[i] for col in cols) for i in range(n)]
            B, P = dict(B, rows=under(bcols, B["n"]), bitmap=[]), dict(P, rows=under(pcols, P["n"]), bitmap=[])
        nulls = (sum(None in t for t in B["rows"]), sum(None in t for t in P["rows"]))
        if ne:
            kb = [int(x) for x in H.mixed_key64(bcols, bits, valid=bm, null_equal=True)] if B["n"] else []
            kp = [int(x) for x in H.mixed_key64(pcols, bits, valid=pm, null_equal=True)] if P["n"] else []
            tb, tp = B["rows"], P["rows"]
            rows, counts, n_pairs, n_coll, _ = ne_rows(tb, tp, kb, kp, _val_list(B), _val_list(P), side, kind, PFILL, BFILL)
            if not (B["bitmap"] or P["bitmap"]):
                nulls = (0, 0)
        else:
            vb = [i for i, t in enumerate(B["rows"]) if None not in t]
            vp = [i for i, t in enumerate(P["rows"]) if None not in t]
            kb_all = H.mixed_key64(bcols, bits) if B["n"] else []
            kp_all = H.mixed_key64(pcols, bits) if P["n"] else []
            tb, tp, kb, kp = [B["rows"][i] for i in vb], [P["rows"][i] for i in vp], [int(kb_all[i]) for i in vb], [int(kp_all[i]) for i in vp]
            if self.mixed_sql is None:
                rows = counts = n_pairs = n_coll = "deferred"
            else:
                Rel, expect = self.mixed_sql
                RB = Rel(bcols, B["vals"], bm if B["bitmap"] else None)
                RP = Rel(pcols, P["vals"], pm if P["bitmap"] else None)
                rows, counts, n_pairs, n_coll, _ = expect(H, RB, RP, side, kind, bits)
        out = dict(rows=rows, counts=counts, pairs=(n_pairs, n_coll), nulls=nulls, form=COLS_HASHED,
                   over=largest_mixed_run(tb, tp, kb, kp, side, kind) > RUN_CAP, sum_probe=sum(_val_list(P)) & M64)
        self._cache[key] = out
        return out

    def expect_str(self, si, side, kind, bitmaps):
        key = ("str", si, side, kind, bool(bitmaps))
        if key not in self._cache:
            c = self.strs[si]
            bnull = ~c["bmask"] if bitmaps and c["bmask"] is not None else np.zeros(len(c["bk"]), bool)
            pnull = ~c["pmask"] if bitmaps and c["pmask"] is not None else np.zeros(len(c["pk"]), bool)
            rows, counts = expected_null_str_kind_rows(c["bk"], c["bv"], c["pk"], c["pv"], side, kind, bnull, pnull, c["hash_bits"], PFILL, BFILL)
            self._cache[key] = dict(rows=rows, counts=counts, nulls=(int(bnull.sum()), int(pnull.sum())), sum_probe=sum(c["pv"]) & M64,
                                    bnull=bnull, pnull=pnull, over=False)  # (draw_str_case keeps every run within the cap)
        return self._cache[key]

    def expect_group(self, gi, ordered):
        key = ("group", gi, bool(ordered))
        if key not in self._cache:
            g = self.groups[gi]
            e = self.H.expected_groups(g["cols"], g["widths"], g["vals"], g["valid"], g["bits"], g["force"], bool(ordered))
            e["over"] = e["form"] == COLS_HASHED and e["max_mixed_run"] > RUN_CAP
            self._cache[key] = e
        return self._cache[key]

    def expect_u64(self, ui):
        key = ("u64", ui)
        if key not in self._cache:
            B, P = self.relations(ui)
            self._cache[key] = expect_inner(B, P, False) + (None,)
        return self._cache[key]

    def expect_sorted(self, ui, side):
        key = ("sort", ui, side)
        if key not in self._cache:
            a = self.relations(ui)[side]
            self._cache[key] = a[np.argsort(a[:, 0], kind="stable")]
        return self._cache[key]

    # ---- the takes ------------------------------------------------------------------------------------
    def take_source(self, src):
        """The columns a take reads: src = (family, case, side).  take_cols: (numpy columns, masks, bit offset); the key
        columns of a column or group case, the fixed key columns and the payloads of a mixed case, the payloads of a string
        case.  take_str: (keys, mask, bit offset) of the first string column of a mixed case or of a string case, else None."""
        fam, ci, side = src
        key = ("take", fam, ci, side)
        if key in self._cache:
            return self._cache[key]
        s = "b" if side == 0 else "p"
        if fam == "cols":
            R = self.cols[ci][s]
            fixed, strs = (R["cols"], R["masks"], R["off"]), None
        elif fam == "group":
            g = self.groups[ci]
            fixed, strs = (g["cols"], g["valid"], g["off"]), None
        elif fam == "mixed":
            c = self.mixed[ci]
            R, layout = c[s], c["layout"]
            cols, masks = mixed_columns(layout, R), mixed_masks(layout, R)
            f = [i for i, typ in enumerate(layout) if typ != "s"]
            pay = np.array(_val_list(R), np.uint64)
            fixed = ([cols[i] for i in f] + [pay], [masks[i] for i in f] + [None], R["off"])
            si = [i for i, typ in enumerate(layout) if typ == "s"]
            strs = (cols[si[0]], masks[si[0]], R["off"]) if si else None
        else:
            c = self.strs[ci]
            keys, vals, mask, off = (c["bk"], c["bv"], c["bmask"], c["off_b"]) if side == 0 else (c["pk"], c["pv"], c["pmask"], c["off_p"])
            fixed, strs = ([np.array(vals, np.uint64)], [None], 0), (keys, mask, off)
        self._cache[key] = (fixed, strs)
        return self._cache[key]

    def n_src(self, src):
        fam, ci, side = src
        if fam == "group":
            return self.groups[ci]["n"]
        if fam == "str":
            return len(self.strs[ci]["bk" if side == 0 else "pk"])
        return (self.cols if fam == "cols" else self.mixed)[ci]["rows"][side]


def take_cols_expect(pool, src, row_map):
    (cols, masks, _), _ = pool.take_source(src)
    return expected_take(cols, masks, row_map)


def take_str_expect(pool, src, row_map):
    keys, mask, _ = pool.take_source(src)[1]
    off = np.zeros(len(keys) + 1, np.int64)
    np.cumsum([len(k) for k in keys], out=off[1:])
    return expected_take_str(b"".join(keys), off, mask, row_map)


def drawn_map(seed, n_src, n_out):
    """A row map with HMJ_TAKE_NO_ROW in about a fifth of its entries."""
    rng = np.random.default_rng([int(seed), n_src, n_out])
    m = rng.integers(0, max(1, n_src), size=n_out, dtype=np.uint64)
    m[rng.random(n_out) < 0.2] = np.uint64(NO_ROW)
    if n_src == 0:
        m[:] = np.uint64(NO_ROW)
    return m


# ---------------------------------------------------------------------------------------------
class KeyModel(Model):
    """test_ctx_sequences_cpu.Model over the ops of these tours.  Beyond the forced bits and the prepared build side: the
    prefix hint in force (until the next config op or the next u64 op), and `live`: the index of the op whose result must
    still be readable (a key join, a string kind join or a group call that materialised; only a take keeps it)."""

    def __init__(self):
        super().__init__()
        self.prefix = None
        self.live = None
        self.index = -1

    def step(self, op):
        self.index += 1
        what = op["what"]
        res = {"rc": 0, "may_prepared": False, "forced": self.forced, "prefix": self.prefix, "live": self.live}
        if what in ("take_cols", "take_str"):
            return res  # keeps the last result and a prepared build side
        self.live = None
        if what == "refused":
            res["rc"] = E_UNSUPPORTED if op["which"] in RAN else E_ARG
            if op["which"] in RAN:
                self._discard()
        elif what == "config":
            self.forced = self.prefix = None  # forced bits and a hint hold until the next configuration op
            if op["action"] == "radix_bits":
                self.forced = op["value"]
            elif op["action"] == "prefix_bits":
                self.prefix = op["value"]
            elif op["action"] == "reserve":
                self._discard()
            res["forced"], res["prefix"] = self.forced, self.prefix
        elif what == "u64":
            self.prefix = res["prefix"] = None  # a u64 op restores automatic sampling first: nothing was promised for its keys
            if op["sub"] == "join":
                res["may_prepared"] = self.prepared is not None and self.prepared == op["case"]
                if not res["may_prepared"]:
                    self._discard()
                self.prepared = None
            elif op["sub"] == "prepare":
                self._discard()
                self.prepared = op["case"]
            else:
                self._discard()
        else:  # the key joins and the group call: like any other call
            self._discard()
            if op.get("over") and (what == "group" or op["flags"] & ORDERED):
                res["rc"] = E_UNSUPPORTED
            elif what == "group" and op["flags"] & (MATERIALIZE | ORDERED) or what != "group" and materialising(op["flags"]):
                self.live = self.index
        return res


# ---------------------------------------------------------------------------------------------
def key_expectation(pool, op):
    """What a key join, string kind join or group op is compared against (never None)."""
    what = op["what"]
    if what in ("cols_inner", "cols_kind", "cols_null_equal"):
        return pool.expect_cols(op["case"], op["side"], op["kind"], op["sem"], op["force"])
    if what == "mixed":
        return pool.expect_mixed(op["case"], op["side"], op["kind"], op["sem"])
    if what == "str_kind":
        return pool.expect_str(op["case"], op["side"], op["kind"], op["bitmaps"])
    if what == "group":
        return pool.expect_group(op["case"], bool(op["flags"] & ORDERED))
    raise ValueError(what)


def map_sources(op):
    """The row maps a materialising op leaves, as (column of the result, (family, case, side) the map indexes)."""
    what = op["what"]
    if what == "group":
        if not op["flags"] & (MATERIALIZE | ORDERED):
            return []
        return [("first_row", ("group", op["case"], 0))] + ([("group_of_row", ("group", op["case"], 0))] if op["want"] & 0x10 else [])
    if what not in KEY_FAMILIES or not materialising(op["flags"]):
        return []
    fam = {"mixed": "mixed", "str_kind": "str"}.get(what, "cols")
    semi_anti = op["kind"] in (SEMI, ANTI)
    out = []
    if not (semi_anti and op["side"] == PROBE):
        out.append(("r_row", (fam, op["case"], 0)))
    if not (semi_anti and op["side"] == BUILD):
        out.append(("s_row", (fam, op["case"], 1)))
    return out


def draw_key_sequence(rng, pool, families=FAMILIES, required=REQUIRED_CHAINS):
    """One tour of ops (dicts of plain values).  The few rules beyond chance serve the ledger of the GPU file and are noted
    where they apply."""
    required = tuple(ch for ch in required if set(ch) <= set(families))
    starts = lambda tour, pos: any(tuple(tour[pos:pos + len(ch)]) == ch for ch in required)
    ends = lambda tour, pos: any(pos >= len(ch) - 1 and tuple(tour[pos - len(ch) + 1:pos + 1]) == ch for ch in required)
    # (no u64 op can be the join that ends one chain and the prepare that starts another -- or the prepare in front of a
    #  column kind join or a mixed join, which the ledger asks for in every tour)
    while True:
        tour = draw_tour(rng, families, required)
        if not any(ends(tour, pos) and (starts(tour, pos) or tour[pos + 1:pos + 2] in (["cols_kind"], ["mixed"])) for pos in range(len(tour))):
            break
    unused = {k: list(rng.permutation(len(getattr(pool, k)))) for k in ("cols", "mixed", "groups", "strs", "u64")}
    refusals = [REFUSALS[i] for i in rng.permutation(len(REFUSALS))]
    state = {"forced": None, "prep": None, "refused": 0, "over": 0, "reserve": 1 << 10, "live": None}
    ops = []

    def pick(kind, ok0=lambda i: True):
        cases = getattr(pool, kind)
        n = len(cases)
        # the first case the families of a kind run in a tour is not its largest: that one then regrows buffers smaller calls
        # have used (a take's drawn source does not count: it runs no entry of the family)
        top = max(range(n), key=lambda i: pool.size_of(cases[i]))
        ran = any(o["what"] in KIND_FAMILIES[kind] for o in ops)
        ok = (lambda i: ok0(i) and i != top) if not ran and any(ok0(i) and i != top for i in range(n)) else ok0
        for i in list(unused[kind]):
            if ok(int(i)):  # cases not used yet first: every tour uses the whole pool
                unused[kind].remove(i)
                return int(i)
        cand = [i for i in range(n) if ok(i)] or list(range(n))
        i = int(cand[int(rng.integers(0, len(cand)))])
        if i in unused[kind]:
            unused[kind].remove(i)
        return i

    def neighbour_rule(kind, fam, prev, nxt, has_bitmaps, carried=False):
        """(case, bitmaps): within a pair of the same family the first op takes a case that is not the smallest and has
        bitmaps, the second a smaller one without them (counters, marks and ballots the larger call filled are met again).
        carried: the case itself decides whether bitmaps are passed (a group case), not the op."""
        size = lambda i: pool.size_of(getattr(pool, kind)[i])
        second = lambda j, i: size(j) < size(i) and not (carried and has_bitmaps(j))
        if prev is not None and prev["fam"] == fam:
            return pick(kind, lambda j: second(j, prev["case"])), False
        if nxt == fam:
            return pick(kind, lambda i: has_bitmaps(i) and any(second(j, i) for j in range(len(getattr(pool, kind))))), True
        i = pick(kind)
        return i, bool(has_bitmaps(i) and rng.random() < 0.6)

    def kind_mode():
        return int(KIND_MODES[int(rng.integers(0, 4))] | (SUM_PROBE if rng.integers(0, 3) == 0 else 0))

    def capped(op):
        """A draw beyond the run cap is kept while the tour's share allows it; beyond the share its ordered mode is drawn
        again as a materialising one (the same case and kind: exact, and no cap applies)."""
        exp = key_expectation(pool, op)
        op["over"] = bool(exp["over"])
        hits = op["over"] and (op["what"] == "group" or op["flags"] & ORDERED)
        if hits and (state["over"] + 1) * CAP_SHARE > len(tour):
            assert op["what"] != "group", "a group case beyond the run cap has no mode that is exact"
            op["flags"] = (op["flags"] & ~ORDERED) | MATERIALIZE
            hits = False
        state["over"] += bool(hits)
        return op

    cols_bitmaps = lambda i: pool.cols[i]["b"]["masks"] is not None or pool.cols[i]["p"]["masks"] is not None
    mixed_bitmaps = lambda i: bool(pool.mixed[i]["b"]["bitmap"] or pool.mixed[i]["p"]["bitmap"])
    for pos, fam in enumerate(tour):
        prev = ops[-1] if ops else None
        nxt = tour[pos + 1] if pos + 1 < len(tour) else None
        if fam == "cols_inner":
            ci = pick("cols")
            c = pool.cols[ci]
            force = bool(c["big"] is None and sum(c["widths"]) <= 8 and rng.random() < 0.4)
            op = capped(dict(what=fam, case=ci, side=PROBE, kind=INNER, sem="plain", force=force,
                             flags=int(COLS_INNER_FLAGS[int(rng.integers(0, len(COLS_INNER_FLAGS)))])))
        elif fam == "cols_kind":
            ci, bitmaps = neighbour_rule("cols", fam, prev, nxt, cols_bitmaps)
            c = pool.cols[ci]
            side, kind = BIG_KINDS[int(rng.integers(0, 3))] if c["big"] is not None else ALL_KINDS[int(rng.integers(0, len(ALL_KINDS)))]
            force = bool(c["big"] is None and sum(c["widths"]) <= 8 and rng.random() < 0.3)
            op = capped(dict(what=fam, case=ci, side=int(side), kind=int(kind), sem="sql" if bitmaps else "plain", force=force, flags=kind_mode()))
        elif fam == "cols_null_equal":
            ci = pick("cols", cols_bitmaps)
            side, kind = ALL_KINDS[int(rng.integers(0, len(ALL_KINDS)))]
            op = capped(dict(what=fam, case=ci, side=int(side), kind=int(kind), sem="ne", force=False, flags=kind_mode()))
        elif fam == "mixed":
            mi, bitmaps = neighbour_rule("mixed", fam, prev, nxt, mixed_bitmaps)
            side, kind = ALL_KINDS[int(rng.integers(0, len(ALL_KINDS)))]
            sem = ("ne" if rng.random() < 0.5 else "sql") if bitmaps else "plain"
            op = capped(dict(what=fam, case=mi, side=int(side), kind=int(kind), sem=sem, flags=kind_mode()))
        elif fam == "group":
            gi, _ = neighbour_rule("groups", fam, prev, nxt, lambda i: pool.groups[i]["valid"] is not None, carried=True)
            want = int(rng.integers(0, GROUP_WANT_ALL + 1))
            op = capped(dict(what=fam, case=gi, flags=int(GROUP_FLAGS[int(rng.integers(0, 3))]), want=want))
        elif fam in ("take_cols", "take_str"):
            # through a row map of the most recent op that left one (and whose relation has a column of the take's type);
            # otherwise through a drawn map that holds HMJ_TAKE_NO_ROW
            maps = [m for m in (state["live"] or []) if fam == "take_cols" or pool.take_source(m[1])[1] is not None]
            if maps:
                col, src = maps[int(rng.integers(0, len(maps)))]
                op = dict(what=fam, map=col, src=list(src))
            else:
                first, side = bool(rng.integers(0, 2)), int(rng.integers(0, 2))
                if fam == "take_cols" and first:
                    src = ("cols", pick("cols", lambda i: pool.cols[i]["big"] is None), side)
                elif fam == "take_cols":
                    src = ("group", pick("groups", lambda i: pool.groups[i]["n"] <= DICT_ROWS), 0)
                elif first:
                    src = ("str", pick("strs"), side)
                else:
                    src = ("mixed", pick("mixed", lambda i: "s" in pool.mixed[i]["layout"]), side)
                op = dict(what=fam, map=None, src=list(src), n_out=int(rng.choice(ROWS)))
        elif fam == "str_kind":
            si = pick("strs")
            side, kind = ALL_KINDS[int(rng.integers(0, len(ALL_KINDS)))]
            bitmaps = bool(pool.strs[si]["bmask"] is not None and rng.random() < 0.7)
            op = dict(what=fam, case=si, side=int(side), kind=int(kind), bitmaps=bitmaps, flags=kind_mode(), over=False)
        elif fam == "u64":
            # the prepare of the required chain, then (whatever stood between) the plain count join of the prepared tensor
            # ... and a prepare directly in front of a group call, a column kind join and a mixed join, which must discard it
            chain_end = ends(tour, pos)
            # (a first u64 op that is free goes to a small case: the largest case then regrows the driver's buffers later)
            first = not any(o["fam"] == "u64" for o in ops)
            if starts(tour, pos) or (not chain_end and nxt in ("group", "cols_kind", "mixed")):
                op = dict(what=fam, sub="prepare", case=pool.prepare_case, hint=int(pool.u64[pool.prepare_case]["rows"][1]))
                if pool.prepare_case in unused["u64"]:
                    unused["u64"].remove(pool.prepare_case)
            elif state["prep"] is not None:
                op = dict(what=fam, sub="join", case=state["prep"], flags=0)
            else:
                fresh = any(i != pool.prepare_case for i in unused["u64"])  # (every tour uses the whole pool)
                sub = str(rng.choice(["join", "sort"] if fresh else ["join", "join", "sort", "prepare"]))
                ui = pool.prepare_case if sub == "prepare" else pick("u64", lambda i: not first or max(pool.u64[i]["rows"]) <= DICT_ROWS)
                op = dict(what=fam, sub=sub, case=ui)
                if sub == "join":
                    op["flags"] = int(rng.choice([0, CHECKSUM, MATERIALIZE | CHECKSUM, ORDERED | CHECKSUM]))
                elif sub == "sort":
                    op.update(side=int(rng.integers(0, 2)), inplace=bool(rng.integers(0, 2)))
                else:
                    op["hint"] = int(pool.u64[ui]["rows"][1])
        elif fam == "config":
            action = str(rng.choice(["radix_bits", "radix_bits", "prefix_bits", "prefix_bits", "profiling", "forget", "release", "reserve"]))
            value = None
            if action == "radix_bits":
                value = int(rng.choice(FORCED_BITS))
            elif action == "prefix_bits":
                value = int(rng.choice(PREFIX_HINTS))
            elif action == "profiling":
                value = bool(rng.integers(0, 2))
            elif action == "reserve":
                state["reserve"] = min(state["reserve"] * 4, 1 << 20)  # growing sizes
                value = [state["reserve"], state["reserve"], state["reserve"] // 2, [0, MATERIALIZE, ORDERED][int(rng.integers(0, 3))]]
            op = dict(what=fam, action=action, value=value)
        elif fam == "refused":
            op = dict(what=fam, which=refusals[state["refused"] % len(refusals)])
            state["refused"] += 1
        else:
            raise ValueError(fam)
        op["fam"] = fam
        # the generator's own view: a prepared build side ends for the drawing with the next u64 op only (whatever stood
        # between: the join still goes to the prepared tensor, and KeyModel says whether it may be taken); the maps of the
        # last materialising op stay on offer across takes
        if fam == "u64":
            state["prep"] = op["case"] if op["sub"] == "prepare" else None
        if fam not in ("take_cols", "take_str"):
            refused_by_cap = op.get("over") and (fam == "group" or op.get("flags", 0) & ORDERED)
            state["live"] = None if refused_by_cap else (map_sources(op) or None)
        ops.append(op)
    return ops


def cases_used(ops):
    used = {k: set() for k in ("cols", "mixed", "groups", "strs", "u64")}
    by = {"cols_inner": "cols", "cols_kind": "cols", "cols_null_equal": "cols", "mixed": "mixed", "group": "groups", "str_kind": "strs", "u64": "u64"}
    src_of = {"cols": "cols", "group": "groups", "mixed": "mixed", "str": "strs"}
    for op in ops:
        if op["what"] in by:
            used[by[op["what"]]].add(op["case"])
        elif op["what"] in ("take_cols", "take_str"):
            used[src_of[op["src"][0]]].add(op["src"][1])
    return used


# ---------------------------------------------------------------------------------------------
SEEDS = (SEQ_SEED, 7, 11)
_pools, _tours = {}, {}


def pool_of(seed):
    import hashmergejoin_amd as H

    if seed not in _pools:
        _pools[seed] = KeyPool(seed, H)
    return _pools[seed]


def tours_of(seed):
    """The pool and the default number of tours of a seed, as test_keyjoin_sequences_gpu.py draws them."""
    pool = pool_of(seed)
    if seed not in _tours:
        rng = np.random.default_rng([int(seed), 13])
        _tours[seed] = [draw_key_sequence(rng, pool) for _ in range(SEQ_TOURS)]
    return pool, _tours[seed]


def test_the_constants_are_the_bindings():
    import hashmergejoin_amd as H

    assert NULL_EQUAL == H.HMJ_NULL_EQUAL and (COLS_PACKED, COLS_HASHED) == (H.HMJ_COLS_PACKED, H.HMJ_COLS_HASHED)
    assert GROUP_WANT_ALL == H.HMJ_GROUP_COUNT | H.HMJ_GROUP_SUM | H.HMJ_GROUP_MIN | H.HMJ_GROUP_MAX | H.HMJ_GROUP_ROW_MAP
    assert H.HMJ_GROUP_ROW_MAP == 0x10 and NO_ROW == H.HMJ_TAKE_NO_ROW == H.HMJ_COLS_NO_ROW


def test_every_tour_holds_every_transition_chain_family_and_case():
    for seed in SEEDS:
        pool, tours = tours_of(seed)
        for ops in tours:
            fams = [op["fam"] for op in ops]
            F = len(FAMILIES)
            assert F == 11 and len(ops) == F * F + 1 == 122
            assert transitions(fams) == {(x, y) for x in FAMILIES for y in FAMILIES}, seed
            assert set(fams) == set(FAMILIES)
            for ch in REQUIRED_CHAINS:
                at = [i for i in range(len(fams) - len(ch) + 1) if tuple(fams[i:i + len(ch)]) == ch]
                assert at, (seed, ch)
                a, b = ops[at[0]], ops[at[0] + len(ch) - 1]
                assert a["sub"] == "prepare" and b["sub"] == "join" and b["case"] == a["case"] == pool.prepare_case and b["flags"] == 0, (seed, ch)
            i = next(i for i in range(len(fams) - 3) if tuple(fams[i:i + 4]) == REQUIRED_CHAINS[0])
            assert ops[i + 1]["map"] is None and ops[i + 2]["map"] is None  # (a prepare leaves no row map: drawn ones)
            used = cases_used(ops)
            for k, s in used.items():
                assert s == set(range(len(getattr(pool, k)))), (seed, k, sorted(s))
            assert {op["which"] for op in ops if op["what"] == "refused"} == set(REFUSALS), seed
            # the rules the ledger of the GPU test leans on
            for fam, kind in (("cols_kind", "cols"), ("mixed", "mixed"), ("group", "groups")):
                pairs = [(a, b) for a, b in zip(ops, ops[1:]) if a["fam"] == b["fam"] == fam]
                assert len(pairs) == 1, (seed, fam)
                a, b = pairs[0]
                cases = getattr(pool, kind)
                assert pool.size_of(cases[b["case"]]) < pool.size_of(cases[a["case"]]), (seed, fam)
                if fam == "group":  # (a group case carries its bitmaps or has none: the second case is one without)
                    assert cases[a["case"]]["valid"] is not None and cases[b["case"]]["valid"] is None, (seed, a, b)
                else:
                    assert a["sem"] != "plain" and b["sem"] == "plain", (seed, fam, a, b)
            assert any(op["what"] in ("take_cols", "take_str") and op["map"] is not None for op in ops), seed


def test_every_drawn_op_has_an_expectation_and_a_status():
    for seed in SEEDS:
        pool, tours = tours_of(seed)
        discarded_by = Counter()
        for ops in tours:
            model = KeyModel()
            refused_by_cap = 0
            for i, op in enumerate(ops):
                before = model.discarded
                want = model.step(op)
                discarded_by[op["what"]] += model.discarded - before
                assert want["rc"] in (0, E_ARG, E_UNSUPPORTED), op
                what = op["what"]
                if what in KEY_FAMILIES or what == "group":
                    exp = key_expectation(pool, op)
                    assert exp is not None and exp["over"] == op["over"], op
                    deferred = what == "mixed" and op["sem"] != "ne"  # (test_join_mixed_gpu.expect: the GPU file's)
                    assert deferred == (isinstance(exp.get("rows", None), str)), op
                    assert (want["rc"] == E_UNSUPPORTED) == bool(op["over"] and (what == "group" or op["flags"] & ORDERED)), op
                    refused_by_cap += want["rc"] == E_UNSUPPORTED
                elif what in ("take_cols", "take_str"):
                    src = tuple(op["src"])
                    assert want["rc"] == 0 and (op["map"] is None or want["live"] is not None), op
                    fixed, strs = pool.take_source(src)
                    assert fixed[0] and (what == "take_cols" or strs is not None), op
                    if op["map"] is None:
                        m = drawn_map(seed + i, pool.n_src(src), op["n_out"])
                        assert len((take_cols_expect if what == "take_cols" else take_str_expect)(pool, src, m)[0]) >= 0
                    else:  # the map of the op the model keeps alive
                        live = ops[want["live"]]
                        assert (op["map"], src) in [(c, tuple(s)) for c, s in map_sources(live)], (op, live)
                elif what == "u64":
                    assert want["rc"] == 0 and want["prefix"] is None
                    if op["sub"] == "join":
                        assert pool.expect_u64(op["case"])[1]["n_matches"] >= 0
                    elif op["sub"] == "sort":
                        assert len(pool.expect_sorted(op["case"], op["side"])) == pool.u64[op["case"]]["rows"][op["side"]]
                else:
                    assert (want["rc"] == 0) == (what == "config"), op
            # at most one op in ten is a draw beyond the run cap (the two refusals that are meant to exceed it aside)
            assert refused_by_cap * CAP_SHARE <= len(ops), (seed, refused_by_cap)
            assert model.discarded > 0, seed
        if seed == SEQ_SEED:  # (the ledger of the GPU file)
            assert all(discarded_by[f] for f in ("group", "cols_kind", "mixed")), discarded_by


def test_pool_cases_are_bounded():
    for seed in SEEDS:
        pool = pool_of(seed)
        big = [c for c in pool.cols if c["big"] is not None]
        assert sorted(c["rows"][0] for c in big) == list(BIG_ROWS) and all(c["widths"] == [4, 4] for c in big)
        assert sorted(g["n"] for g in pool.groups if g["n"] > DICT_ROWS) == list(BIG_ROWS)
        for c in pool.cols:
            assert c["big"] is not None or (c["rows"][0] in ROWS and c["rows"][1] in ROWS), c["rows"]
            for s in (c["b"], c["p"]):
                assert s["off"] in BIT_OFFSETS and (s["masks"] is None or len(s["masks"]) == len(c["widths"]))
        assert {tuple(c["widths"]) for c in pool.cols} == {tuple(w) for w in COL_LAYOUTS}
        assert {tuple(c["layout"]) for c in pool.mixed} == {tuple(x) for x in MIXED_LAYOUTS}
        for c in pool.mixed:
            assert c["rows"][0] in ROWS and c["rows"][1] in ROWS and max(c["rows"]) <= DICT_ROWS
        for g in pool.groups:
            assert g["n"] in ROWS or g["n"] in BIG_ROWS
        for c in pool.strs:
            assert max(len(c["bk"]), len(c["pk"])) <= DICT_ROWS
        assert {c["bits"] for c in pool.cols + pool.mixed} <= set(HASH_BITS)
        assert any(c["bits"] for c in pool.cols + pool.mixed + pool.groups), seed  # collisions occur somewhere
        # bitmaps in none, some and all columns
        shapes = set()
        for c in pool.cols:
            for s in (c["b"], c["p"]):
                k = 0 if s["masks"] is None else sum(m is not None for m in s["masks"])
                shapes.add("none" if k == 0 else "all" if k == len(c["widths"]) else "some")
        assert shapes == {"none", "some", "all"}, (seed, shapes)
        assert pool.u64[pool.prepare_case]["rows"][0] == PREPARE_ROWS


def test_the_run_cap_is_read_from_key64_and_tuples():
    t = lambda *xs: [(x,) for x in xs]
    # 600 build and 600 probe rows of two tuples under one key64: 2 * 300 * 300 pairs in one run
    tb, tp = t(*([1, 2] * 300)), t(*([1, 2] * 300))
    one = [7] * 600
    assert largest_mixed_run(tb, tp, one, one, PROBE, INNER) == 2 * 300 * 300
    assert largest_mixed_run(tb, tp, one, one, PROBE, SEMI) == 600 and largest_mixed_run(tb, tp, one, one, PROBE, ANTI) == 0
    assert largest_mixed_run(tb, tp, one, one, BUILD, FULL_OUTER) == 2 * 300 * 300
    # one tuple per key64: never a mixed run, whatever its length
    assert largest_mixed_run(tb, tp, [x[0] for x in tb], [x[0] for x in tp], PROBE, INNER) == 0
    # unmatched rows of another tuple make a run mixed for the kinds that emit them
    tb, tp = t(1, 1), t(1, 2, 2, 2)
    assert largest_mixed_run(tb, tp, [5, 5], [5] * 4, PROBE, INNER) == 0
    assert largest_mixed_run(tb, tp, [5, 5], [5] * 4, PROBE, PROBE_OUTER) == 5 == largest_mixed_run(tb, tp, [5, 5], [5] * 4, BUILD, FULL_OUTER)
    assert largest_mixed_run(tb, tp, [5, 5], [5] * 4, BUILD, BUILD_OUTER) == 0


def test_the_two_plain_references_agree():
    """expected_kind_rows (rows, counters) and ne_rows (which also counts the pairs the call compares) on a case without
    bitmaps: the same rows, so n_key_pairs / n_collisions are taken over the join the rows come from."""
    pool = pool_of(SEQ_SEED)
    ci = next(i for i, c in enumerate(pool.cols) if c["big"] is None and max(c["rows"]) <= 600 and min(c["rows"]) > 2)
    c = pool.cols[ci]
    for side, kind in ALL_KINDS:
        e = pool.expect_cols(ci, side, kind, "plain", True)
        tb, tp = tuples_of(c["b"]["cols"], c["widths"], None), tuples_of(c["p"]["cols"], c["widths"], None)
        kb = [int(x) for x in pool.H.cols_key64(c["b"]["cols"], c["widths"], c["bits"], True)]
        kp = [int(x) for x in pool.H.cols_key64(c["p"]["cols"], c["widths"], c["bits"], True)]
        rows, counts, n_pairs, n_coll, _ = ne_rows(tb, tp, kb, kp, _val_list(c["b"]), _val_list(c["p"]), side, kind, PFILL, BFILL)
        assert np.array_equal(rows, e["rows"]) and counts == e["counts"] and (n_pairs, n_coll) == e["pairs"], (side, kind)


def test_the_expectations_of_the_default_tours_are_quick():
    """Everything the GPU file compares against, for the default seed (the SQL-semantics rows of the mixed entry aside: they
    are test_join_mixed_gpu.expect's).  Measured: see DESIGN.md, "How a long-lived context is tested"."""
    t0 = time.perf_counter()
    pool = KeyPool(SEQ_SEED, pool_of(SEQ_SEED).H)
    rng = np.random.default_rng([SEQ_SEED, 13])
    tours = [draw_key_sequence(rng, pool) for _ in range(SEQ_TOURS)]
    for ops in tours:
        for op in ops:
            if op["what"] in KEY_FAMILIES or op["what"] == "group":
                key_expectation(pool, op)
            elif op["what"] == "u64" and op["sub"] == "join":
                pool.expect_u64(op["case"])
    dt = time.perf_counter() - t0
    print("pool, %d tours and their expectations: %.1f s" % (len(tours), dt))
    assert dt < 45.0, dt  # (15 s is the aim; three times that before the test speaks up on a loaded machine)


def test_the_model_follows_the_written_contract():
    m = KeyModel()
    join = lambda ci: dict(what="u64", sub="join", case=ci, flags=0)
    prep = lambda ci: dict(what="u64", sub="prepare", case=ci)
    take = dict(what="take_cols", map=None, src=["cols", 0, 0], n_out=1)
    group = dict(what="group", case=0, flags=MATERIALIZE, want=1, over=False)
    m.step(prep(3))
    m.step(take)
    m.step(dict(take, what="take_str"))
    assert m.step(join(3))["may_prepared"]  # the takes keep a prepared build side
    for between, may in ((group, False), (dict(what="cols_kind", case=0, flags=0, over=False), False),
                         (dict(what="mixed", case=0, flags=ORDERED, over=True), False), (dict(what="str_kind", case=0, flags=0), False),
                         (dict(what="config", action="prefix_bits", value=16), True), (dict(what="config", action="radix_bits", value=4), True),
                         (dict(what="config", action="forget", value=None), True), (dict(what="config", action="reserve", value=[1, 1, 0, 0]), False),
                         (dict(what="refused", which="width_3"), True), (dict(what="refused", which="take_map_beyond_source"), True),
                         (dict(what="refused", which="group_run_cap"), False), (dict(what="u64", sub="sort", case=0), False)):
        m.step(prep(3))
        m.step(between)
        assert m.step(join(3))["may_prepared"] == may, between
    assert m.discarded == 7
    # forced bits and the hint: until the next config op; the hint also ends with a u64 op
    m.step(dict(what="config", action="radix_bits", value=8))
    assert m.step(group)["forced"] == 8
    m.step(dict(what="config", action="prefix_bits", value=48))
    w = m.step(group)
    assert (w["forced"], w["prefix"]) == (None, 48)
    assert m.step(join(0))["prefix"] is None and m.step(group)["prefix"] is None
    # only a take keeps a result; an op refused by the run cap leaves none
    i = m.index
    assert m.live == i and m.step(take)["live"] == i and m.step(take)["live"] == i
    m.step(dict(what="config", action="profiling", value=True))
    assert m.step(take)["live"] is None
    assert m.step(dict(what="mixed", case=0, flags=ORDERED, over=True))["rc"] == E_UNSUPPORTED and m.live is None
    assert m.step(dict(what="mixed", case=0, flags=MATERIALIZE, over=True))["rc"] == 0 and m.live == m.index
    assert m.step(dict(group, over=True, flags=0))["rc"] == E_UNSUPPORTED
