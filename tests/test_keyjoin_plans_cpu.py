"""CPU-only half of the plan-crossing tests for the key joins' inner u64 join (test_keyjoin_plans_gpu.py imports it): the
key families (packed [4,4], [8] and [2,2,2,2], hashed [8,4,2], a string plus a 4-byte column, one string column,
NULL-equals-NULL over [8,4,2] with bitmaps), the seeded shape classes S1..S11 that steer the u64 join onto its plans, and a
vectorised numpy reference (`Ref`) that pairs rows by TUPLE equality -- dense tuple ids from np.unique over the stacked key
columns, pairs by a sort of the ids and their running counts; key64 only orders the rows and comes from the package mirrors
cols_key64 / mixed_key64 and the string hash.  Checked here, before a GPU is involved: the reference against the pure-Python
brute forces of the family files (ne_rows, expected_kind_rows, kind_brute) for every family and kind at small sizes, and the
properties every shape class promises (unique or duplicated, fan-out, sortedness, hot-key share, no 64-bit collision)."""
import numpy as np
import pytest

from test_join_cols_kinds_cpu import (ANTI, BUILD, BUILD_ANTI, COUNT_KEYS, FULL_OUTER, INNER, M64, NO_ROW, PROBE, PROBE_OUTER, SEMI,
                                      expected_kind_rows)
from test_join_null_equal_cpu import ne_rows
from test_join_str_cpu import str_hash
from test_join_str_kinds_cpu import kind_brute

GOLD = np.uint64(0x9E3779B97F4A7C15)
PFILL, BFILL = 0xF1, 2 ** 64 - 2
# the four entries of a GPU case: between them the three inner calls (MATERIALIZE, | ORDERED, | FIRST_WINS with the
# relations as given and swapped)
ENTRIES = [("inner", PROBE, INNER), ("probe_semi", PROBE, SEMI), ("build_anti", BUILD, BUILD_ANTI), ("full_outer", BUILD, FULL_OUTER)]
REF_KINDS = ENTRIES + [("probe_anti", PROBE, ANTI), ("probe_outer", PROBE, PROBE_OUTER)]
FAMILIES = {  # name: (widths or None, form)
    "packed44": ([4, 4], "packed"), "packed8": ([8], "packed"), "packed2222": ([2, 2, 2, 2], "packed"),
    "hashed842": ([8, 4, 2], "hashed"), "nulleq842": ([8, 4, 2], "hashed"), "mixed": (None, "hashed"), "str": (None, "hashed"),
}
WITH_VALS = ("hashed842", "str")  # families whose relations carry drawn payloads; the others': the payload of row i is i


# ---- families: tuple id -> tuple, tuple -> key64 ---------------------------------------------------------------------------
def spread(ids):
    """ids -> distinct 64-bit values with mixed bits (multiplication by an odd constant is a bijection mod 2^64)."""
    return np.asarray(ids).astype(np.uint64) * GOLD


def strings_of(ids):
    """ids -> distinct byte strings of 5..34 bytes (an 'S' array): with and without whole 8-byte blocks and a tail."""
    u, inv = np.unique(np.asarray(ids), return_inverse=True)
    s = np.char.mod(b"key-%d", u)
    s = np.char.add(s, np.where(u % 3 == 0, b"-with-a-tail-of-22-byte", b"").astype("S23"))
    return s[inv.reshape(-1)]


def tuples_of(fam, ids, rng=None):
    """(cols, valid) of the rows whose tuple ids are `ids`; two rows hold one tuple exactly when their ids are equal.
    nulleq842: column 1 is NULL in tuples with id % 5 == 0, column 2 where id % 7 == 0; what lies under a NULL slot is
    drawn per ROW (rng), so equal tuples differ there."""
    ids = np.asarray(ids, np.int64)
    m = spread(ids)
    if fam == "packed44":
        return [(m >> np.uint64(32)).astype(np.uint32), m.astype(np.uint32)], None
    if fam == "packed8":
        return [m], None
    if fam == "packed2222":
        return [(m >> np.uint64(s)).astype(np.uint16) for s in (48, 32, 16, 0)], None
    if fam in ("hashed842", "nulleq842"):
        cols = [m, (ids ^ 0x5A5A5A5A).astype(np.uint32), (ids * 7).astype(np.uint16)]
        if fam == "hashed842":
            return cols, None
        valid = [None, ids % 5 != 0, ids % 7 != 0]
        for c in (1, 2):
            junk = rng.integers(0, 1 << 16, len(ids)).astype(cols[c].dtype)
            cols[c] = np.where(valid[c], cols[c], junk)
        return cols, valid
    if fam == "mixed":  # 4099 distinct strings; the 4-byte column tells the tuples apart
        return [strings_of(ids % 4099), ids.astype(np.uint32)], None
    if fam == "str":
        return [strings_of(ids)], None
    raise ValueError(fam)


def hash_strings(s, bits=0):
    """The string hash of every slot of an 'S' array: the pure-Python mirror over the distinct strings, gathered."""
    u, inv = np.unique(s, return_inverse=True)
    return np.array([str_hash(bytes(x), bits) for x in u.tolist()], np.uint64)[inv.reshape(-1)]


def key64_of(fam, cols, valid=None, bits=0):
    """key64 of every row from the package mirrors.  A string column enters mixed_key64 as its 64-bit hashes (a fixed
    8-byte column contributes its value to the chain exactly as a string column contributes its hash)."""
    import hashmergejoin_amd as H

    if not len(cols[0]):
        return np.zeros(0, np.uint64)
    if fam == "str":
        return hash_strings(cols[0], bits)
    if fam == "mixed":
        return H.mixed_key64([hash_strings(cols[0]), cols[1]], bits)
    widths = FAMILIES[fam][0]
    if fam == "nulleq842":
        return H.cols_key64(cols, widths, bits, valid=valid, null_equal=True)
    return H.cols_key64(cols, widths, bits)


def canon(bcols, bvalid, pcols, pvalid):
    """Both relations' tuples as uint64 matrices whose rows compare (lexicographically) as the tuples do: a string column
    becomes its rank among both relations' strings, a nullable column the pair (is NULL, value or 0): NULLS LAST."""
    nb = len(bcols[0])
    out = []
    for c in range(len(bcols)):
        both = np.concatenate([bcols[c], pcols[c]])
        if both.dtype.kind == "S":
            both = np.unique(both, return_inverse=True)[1].reshape(-1)
        both = both.astype(np.uint64)
        if bvalid is not None and bvalid[c] is not None:
            null = ~np.concatenate([bvalid[c], pvalid[c]])
            out += [null.astype(np.uint64), np.where(null, np.uint64(0), both)]
        else:
            out.append(both)
    m = np.stack(out, 1)
    return m[:nb], m[nb:]


def tuple_ids(cb, cp):
    """Dense ids of the tuples of both relations, ascending in tuple order: np.unique over the stacked rows.  Where the
    columns' own ranks fit one 64-bit number together, the rows are numbered through that number (np.unique over rows
    compares them as byte strings: minutes at 2^23 rows) -- the same ids, which test_tuple_ids_through_column_ranks pins."""
    m = np.concatenate([cb, cp])
    combined, room = np.zeros(len(m), np.uint64), 1
    for c in range(m.shape[1]):
        values, rank = np.unique(m[:, c], return_inverse=True)
        room *= len(values)
        if room >= 1 << 63:
            combined = None
            break
        combined = combined * np.uint64(len(values)) + rank.reshape(-1).astype(np.uint64)
    if combined is None:
        inv = np.unique(m, axis=0, return_inverse=True)[1].reshape(-1)
    else:
        inv = np.unique(combined, return_inverse=True)[1].reshape(-1)
    return inv[:len(cb)], inv[len(cb):]


# ---- the reference -----------------------------------------------------------------------------------------------------------
class Ref:
    """A join of two relations given as tuple ids (tb, tp), key64 (kb, kp) and payloads (bv, pv; uint64).  rows(side, kind):
    [n, 5] uint64 (key64, r_row, s_row, rval, sval) in the HMJ_ORDERED order -- (key64, tuple order, r_row, s_row), NO_ROW
    last; 0 in the columns the kind does not produce --, the four counters, the pairs of equal key64 the call compares and
    those of them whose tuples differ (semi / anti: the row against the FIRST row of its key64 on the other side, then, if
    that one holds another tuple, against every row of its key64 there).  Each kind is computed once and kept."""

    def __init__(self, tb, tp, kb, kp, bv, pv):
        self.tb, self.tp, self.kb, self.kp, self.bv, self.pv = tb, tp, kb, kp, bv, pv
        nb, np_ = len(tb), len(tp)
        n_t = int(max(tb.max(initial=-1), tp.max(initial=-1))) + 1
        ob = np.argsort(tb, kind="stable")  # build rows by tuple, rows of one tuple ascending
        n_of = np.bincount(tb, minlength=n_t)  # (the ids are dense: a tuple's run in `ob` starts at the counts' running sum)
        lo, cnt = (np.cumsum(n_of) - n_of)[tp], n_of[tp]
        total = int(cnt.sum())
        self.s_pair = np.repeat(np.arange(np_), cnt)
        self.r_pair = ob[np.repeat(lo, cnt) + (np.arange(total) - np.repeat(np.cumsum(cnt) - cnt, cnt))] if total else np.zeros(0, np.int64)
        self.p_match = cnt > 0
        self.b_match = np.bincount(tp, minlength=n_t)[tb] > 0
        key_of = np.zeros(n_t, np.uint64)
        key_of[tb], key_of[tp] = kb, kp
        self.rank = np.empty(n_t, np.int64)  # of a tuple in (key64, tuple order)
        self.rank[np.lexsort((np.arange(n_t), key_of))] = np.arange(n_t)
        self.key_of = key_of
        self.kept = {}

    def _part(self, key, tid, r, s, rv, sv):
        u = lambda a: np.asarray(a).astype(np.uint64)
        return np.stack([u(key), u(tid), u(r), u(s), u(rv), u(sv)], 1).reshape(-1, 6)

    def _pairs(self):
        r, s = self.r_pair, self.s_pair
        return self._part(self.kp[s], self.tp[s], r, s, self.bv[r], self.pv[s])

    def _probe(self, sel, fill):
        s = np.flatnonzero(self.p_match == sel)
        return self._part(self.kp[s], self.tp[s], np.full(len(s), NO_ROW, np.uint64), s, np.full(len(s), fill, np.uint64), self.pv[s])

    def _build(self, sel, fill):
        r = np.flatnonzero(self.b_match == sel)
        return self._part(self.kb[r], self.tb[r], r, np.full(len(r), NO_ROW, np.uint64), self.bv[r], np.full(len(r), fill, np.uint64))

    def _compared(self, side, kind):
        if kind not in (SEMI, ANTI):
            ukey, n_key = np.unique(self.kb, return_counts=True)
            j = np.minimum(np.searchsorted(ukey, self.kp), max(len(ukey) - 1, 0))
            n_pairs = int(n_key[j][ukey[j] == self.kp].sum()) if len(ukey) else 0
            return n_pairs, n_pairs - len(self.r_pair)
        tk, kk, to, ko = (self.tp, self.kp, self.tb, self.kb) if side == PROBE else (self.tb, self.kb, self.tp, self.kp)
        if not len(tk) or not len(to):
            return 0, 0
        order = np.argsort(ko, kind="stable")  # (stable: the first row of a key64 is its smallest row index)
        ukey, first, n_key = np.unique(ko[order], return_index=True, return_counts=True)
        rep_tuple = to[order[first]]
        j = np.minimum(np.searchsorted(ukey, kk), len(ukey) - 1)
        met = ukey[j] == kk
        amb = met & (rep_tuple[j] != tk)
        n_tuple = np.bincount(to, minlength=len(self.rank))
        n_pairs = int(met.sum()) + int(n_key[j][amb].sum())
        return n_pairs, int(amb.sum()) + int((n_key[j][amb] - n_tuple[tk[amb]]).sum())

    def rows(self, side, kind):
        if (side, kind) in self.kept:
            return self.kept[(side, kind)]
        counts = dict.fromkeys(COUNT_KEYS, 0)
        pc = {"n_probe_matched": int(self.p_match.sum()), "n_probe_unmatched": int((~self.p_match).sum())}
        bc = {"n_build_matched": int(self.b_match.sum()), "n_build_unmatched": int((~self.b_match).sum())}
        absent = ()
        if (side, kind) == (PROBE, INNER):
            parts = [self._pairs()]
        elif side == PROBE and kind in (SEMI, ANTI):
            parts, absent = [self._probe(kind == SEMI, 0)], (1, 3)
            counts.update(pc)
        elif (side, kind) == (PROBE, PROBE_OUTER):
            parts = [self._pairs(), self._probe(False, PFILL)]
            counts.update(pc)
        elif (side, kind) == (BUILD, BUILD_ANTI):
            parts, absent = [self._build(False, 0)], (2, 4)
            counts.update(bc)
        elif (side, kind) == (BUILD, FULL_OUTER):
            parts = [self._pairs(), self._probe(False, PFILL), self._build(False, BFILL)]
            counts.update(pc)
            counts.update(bc)
        else:
            raise ValueError((side, kind))
        rows = np.concatenate(parts)
        rows = rows[np.lexsort((row_pair_key(rows[:, 2], rows[:, 3]), self.rank[rows[:, 1].astype(np.int64)]))]
        out = np.ascontiguousarray(rows[:, [0, 2, 3, 4, 5]])
        for c in absent:
            out[:, c] = 0
        self.kept[(side, kind)] = (out, counts) + self._compared(side, kind)
        return self.kept[(side, kind)]

    def max_mixed_run(self):
        """Rows of the largest run of equal key64 that holds several tuples, over the FULL_OUTER rows (which hold every
        other kind's): the collision sort takes at most 1024."""
        rows = self.rows(BUILD, FULL_OUTER)[0]
        tid = np.where(rows[:, 2] != NO_ROW, self.tp[np.minimum(rows[:, 2], len(self.tp) - 1).astype(np.int64)],
                       self.tb[np.minimum(rows[:, 1], len(self.tb) - 1).astype(np.int64)])
        ukey, inv, n_rows = np.unique(rows[:, 0], return_inverse=True, return_counts=True)
        lo = np.full(len(ukey), np.iinfo(np.int64).max)
        hi = np.full(len(ukey), -1)
        np.minimum.at(lo, inv.reshape(-1), tid)
        np.maximum.at(hi, inv.reshape(-1), tid)
        mixed = n_rows[lo != hi]
        return int(mixed.max()) if len(mixed) else 0


def row_pair_key(r, s):
    """(r_row, s_row) as one uint64 that sorts as the pair does, NO_ROW last (row indices stay below 2^32 - 1)."""
    top = np.uint64(0xFFFFFFFF)
    return (np.minimum(r, top) << np.uint64(32)) | np.minimum(s, top)


def by_row_pair(rows):
    """Result rows in the order unordered results are compared in: no two rows of a result share (r_row, s_row)."""
    return rows[np.argsort(row_pair_key(rows[:, 1], rows[:, 2]), kind="stable")] if len(rows) else rows


# ---- cases ---------------------------------------------------------------------------------------------------------------------
class Case:
    """Two relations of a family with everything a test needs: the columns and bitmaps (tuples, not key64), payloads (None:
    the payload of row i is i), key64 from the mirrors, and the reference."""

    def __init__(self, fam, bcols, bvalid, pcols, pvalid, bits=0, seed=1):
        self.fam, self.bits = fam, bits
        self.bcols, self.bvalid, self.pcols, self.pvalid = bcols, bvalid, pcols, pvalid
        self.nb, self.np = len(bcols[0]), len(pcols[0])
        rng = np.random.default_rng(seed)
        self.bvals = rng.integers(0, 1 << 63, self.nb, dtype=np.uint64) if fam in WITH_VALS else None
        self.pvals = rng.integers(0, 1 << 63, self.np, dtype=np.uint64) if fam in WITH_VALS else None
        self.kb, self.kp = key64_of(fam, bcols, bvalid, bits), key64_of(fam, pcols, pvalid, bits)
        self.tb, self.tp = tuple_ids(*canon(bcols, bvalid, pcols, pvalid))
        bv = np.arange(self.nb, dtype=np.uint64) if self.bvals is None else self.bvals
        pv = np.arange(self.np, dtype=np.uint64) if self.pvals is None else self.pvals
        self.ref = Ref(self.tb, self.tp, self.kb, self.kp, bv, pv)
        self.sum_probe = int(pv.sum(dtype=np.uint64))

    def collision_free(self):
        """No two tuples share a key64."""
        keys = np.concatenate([self.kb, self.kp])
        n_tuples = int(max(self.tb.max(initial=-1), self.tp.max(initial=-1))) + 1
        return len(np.unique(keys)) == n_tuples


def case_of_ids(fam, b_ids, p_ids, bits=0, seed=1):
    rng = np.random.default_rng(seed + 77)
    bcols, bvalid = tuples_of(fam, b_ids, rng)
    pcols, pvalid = tuples_of(fam, p_ids, rng)
    return Case(fam, bcols, bvalid, pcols, pvalid, bits, seed)


def probe_ids(rng, nb_ids, n, missing):
    """n probe ids drawn from the build side's ids 0..nb_ids-1, the share `missing` of them replaced by ids it lacks."""
    p = rng.integers(0, nb_ids, n)
    if missing:
        miss = rng.random(n) < missing
        p[miss] = nb_ids + rng.integers(0, nb_ids, int(miss.sum()))
    return p


def ids_s1(nb, seed=1, n_probe=65536 + 1025):
    """S1: a small unique build side; a quarter of the probe rows hold tuples it lacks."""
    rng = np.random.default_rng(seed)
    return rng.permutation(nb), probe_ids(rng, nb, n_probe, 0.25)


def ids_s3(seed=3, n_tuples=750, n_probe=65536 + 1025):
    """S3: S1's small build side with every third tuple twice (1000 rows)."""
    rng = np.random.default_rng(seed)
    t = np.arange(n_tuples)
    return rng.permutation(np.concatenate([t, t[::3]])), probe_ids(rng, n_tuples, n_probe, 0.25)


def ids_s4(seed=4, nb=300000, n_probe=400000):
    """S4: unique on both sides, a third of the probe tuples missing from the build side."""
    rng = np.random.default_rng(seed)
    n_miss = n_probe // 3
    p = np.concatenate([rng.permutation(nb)[:n_probe - n_miss], nb + rng.permutation(nb)[:n_miss]])
    return rng.permutation(nb), rng.permutation(p)


def ids_s5(seed=5, nb=1 << 14, fanout=70, stray=13):
    """S5: foreign keys: every build tuple on `fanout` probe rows, and `stray` probe rows without a build row."""
    rng = np.random.default_rng(seed)
    return rng.permutation(nb), rng.permutation(np.concatenate([np.repeat(np.arange(nb), fanout), nb + np.arange(stray)]))


def ids_s6(nb, n_probe, missing, seed=6):
    """S6: a small unique build side under a long probe side."""
    rng = np.random.default_rng(seed)
    return rng.permutation(nb), probe_ids(rng, nb, n_probe, missing)


def ids_s7(seed=7, hot=0):
    """S7: many-to-many: 200 000 build and 300 000 probe rows over 30 000 build tuples, every tuple 6 or 7 times on the
    build side and 10 times on the probe side, which lacks 3 000 of them and holds 3 000 others.  hot: that many build rows
    are given to tuple 3 000 (which the probe side holds) instead."""
    rng = np.random.default_rng(seed)
    t = np.arange(30000)
    b = rng.permutation(np.concatenate([np.repeat(t[:20000], 7), np.repeat(t[20000:], 6)]))
    if hot:
        b[rng.permutation(len(b))[:hot]] = 3000
    return b, rng.permutation(np.repeat(np.arange(3000, 33000), 10))


def ids_s8(seed=8, share=0.3):
    """S8: S4 with one build tuple on 30 % of the probe rows."""
    rng = np.random.default_rng(seed)
    b, p = ids_s4(seed)
    p[rng.random(len(p)) < share] = b[0]
    return b, p


def case_s9_columns(seed=9, n=(1 << 18) + 9, n_probe=(1 << 20) + 5):
    rng = np.random.default_rng(seed)
    b, p = rng.permutation(n).astype(np.uint32), rng.integers(0, n + n // 4, n_probe).astype(np.uint32)
    return [np.zeros(n, np.uint32), b], [np.zeros(n_probe, np.uint32), p]


def case_s9(seed=9):
    """S9 (packed [4,4]): dense keys (0, id), ids 0..n-1 shuffled, n = 2^18 + 9; 2^20 + 5 probe ids drawn a quarter wider."""
    bcols, pcols = case_s9_columns(seed)
    return Case("packed44", bcols, None, pcols, None, 0, seed)


def case_s10(fam, seed=10):
    """S10 (packed): S4's relations, each arriving sorted by its key tuple: key64 ascends."""
    b, p = ids_s4(seed)
    out = []
    for ids in (b, p):
        cols, _ = tuples_of(fam, ids)
        order = np.argsort(key64_of(fam, cols), kind="stable")
        out.append([c[order] for c in cols])
    return Case(fam, out[0], None, out[1], None, 0, seed)


def case_s11(seed=2020, n=(1 << 22) + 77):
    """S11 (hashed [8,4,2]): n rows per relation, unique build tuples (a, b, c) -- a alone is unique --, probe rows drawn from
    them with repeats, every second probe row changed in b to a tuple the build side lacks (test_join_cols_kinds_gpu.make_big
    at this size)."""
    rng = np.random.default_rng(seed)
    a = rng.permutation(n).astype(np.uint64) * GOLD
    b = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    c = rng.integers(0, 1 << 16, n, dtype=np.uint64).astype(np.uint16)
    pick = rng.integers(0, n, n)
    pa, pb, pc = a[pick].copy(), b[pick].copy(), c[pick].copy()
    pb[::2] ^= np.uint32(0x80000000)
    return Case("hashed842", [a, b, c], None, [pa, pb, pc], None, 0, seed)


def with_marker(case, build_rows, probe_rows):
    """A packed case with the all-ones tuple (key64 == 2^64 - 1, the global table's empty-slot marker) in those rows."""
    bcols, pcols = [c.copy() for c in case.bcols], [c.copy() for c in case.pcols]
    for cols, rows in ((bcols, build_rows), (pcols, probe_rows)):
        for c in cols:
            c[rows] = np.iinfo(c.dtype).max
    return Case(case.fam, bcols, None, pcols, None, 0, 2)


GROUP_SHAPES = ["S7/packed44", "S7/hashed842", "S9", "S10", "hashed/2^20"]


def group_shape(shape):
    """(columns, widths) of the relation hmj_group_cols_device groups: the build side of a join class, or 2^20 rows over 2^17
    hashed [8,4,2] tuples."""
    if shape.startswith("S7/"):
        fam = shape[3:]
        return tuples_of(fam, ids_s7()[0])[0], FAMILIES[fam][0]
    if shape == "S9":
        return case_s9_columns()[0], [4, 4]
    if shape == "S10":
        cols, _ = tuples_of("packed44", ids_s4(10)[0])
        order = np.argsort(key64_of("packed44", cols), kind="stable")
        return [c[order] for c in cols], [4, 4]
    if shape == "hashed/2^20":
        return tuples_of("hashed842", np.random.default_rng(20).integers(0, 1 << 17, 1 << 20))[0], [8, 4, 2]
    raise ValueError(shape)


# ---- the reference against the brute forces ----------------------------------------------------------------------------------
def python_tuples(cols, valid):
    out = []
    for c, col in enumerate(cols):
        vs = [bytes(x) for x in col.tolist()] if col.dtype.kind == "S" else [int(x) for x in col]
        if valid is not None and valid[c] is not None:
            vs = [v if ok else None for v, ok in zip(vs, valid[c])]
        out.append(vs)
    return list(zip(*out))


def small_case(fam, bits, seed):
    """Duplicates and misses on both sides over 300 shared, 80 build-only and 80 probe-only tuples: at most 2000 rows."""
    rng = np.random.default_rng(seed)
    b = np.concatenate([rng.integers(0, 380, 700), np.arange(0, 380, 7)])
    p = np.concatenate([rng.integers(0, 300, 900), rng.integers(380, 460, 150)])
    return case_of_ids(fam, rng.permutation(b), rng.permutation(p), bits, seed)


@pytest.mark.parametrize("fam,bits", [("packed44", 0), ("packed8", 0), ("packed2222", 0), ("hashed842", 0), ("hashed842", 6),
                                      ("nulleq842", 0), ("nulleq842", 6), ("mixed", 0), ("mixed", 6), ("str", 0), ("str", 6)])
def test_reference_equals_the_brute_forces(fam, bits):
    case = small_case(fam, bits, 11 + bits)
    assert case.nb + case.np <= 2000 and (bits > 0) == (not case.collision_free())
    tb, tp = python_tuples(case.bcols, case.bvalid), python_tuples(case.pcols, case.pvalid)
    bv = list(range(case.nb)) if case.bvals is None else [int(x) for x in case.bvals]
    pv = list(range(case.np)) if case.pvals is None else [int(x) for x in case.pvals]
    kb, kp = [int(x) for x in case.kb], [int(x) for x in case.kp]
    ambiguous = 0
    for name, side, kind in REF_KINDS:
        rows, counts, n_pairs, n_coll = case.ref.rows(side, kind)
        want, wcounts, wpairs, wcoll, seen = ne_rows(tb, tp, kb, kp, bv, pv, side, kind, PFILL, BFILL)
        assert np.array_equal(rows, want), (name, np.flatnonzero(np.any(rows != want, axis=1))[:5])
        assert counts == wcounts and (n_pairs, n_coll) == (wpairs, wcoll), (name, counts, wcounts, n_pairs, wpairs, n_coll, wcoll)
        ambiguous += "ambiguous" in seen
        assert (n_coll > 0) == (bits > 0), name
        if fam in ("packed44", "packed8", "packed2222", "hashed842"):  # ... and the column joins' own expectation
            want, wcounts = expected_kind_rows(case.bcols, case.bvals, case.pcols, case.pvals, FAMILIES[fam][0], side, kind, bits,
                                               False, PFILL, BFILL)
            assert np.array_equal(rows, want) and counts == wcounts, name
        if fam == "str":  # ... and the string joins' (which writes NO_ROW into an absent row column)
            want, wcounts = kind_brute([t[0] for t in tb], bv, [t[0] for t in tp], pv, side, kind, bits, PFILL, BFILL)
            for c in (1, 2):
                if kind in (SEMI, ANTI) and c == (1 if side == PROBE else 2):
                    want[:, c] = 0
            assert np.array_equal(rows, want) and counts == wcounts, name
    assert (ambiguous > 0) == (bits > 0)
    run = case.ref.max_mixed_run()
    assert (run > 1) == (bits > 0) and run <= 1024
    # unordered results are compared after a sort by (r_row, s_row): no two rows of a result share the pair
    full = case.ref.rows(BUILD, FULL_OUTER)[0]
    assert len(np.unique(row_pair_key(full[:, 1], full[:, 2]))) == len(full)


def test_tuple_ids_through_column_ranks():
    for fam in ("packed44", "hashed842", "nulleq842", "mixed"):
        case = small_case(fam, 0, 5)
        cb, cp = canon(case.bcols, case.bvalid, case.pcols, case.pvalid)
        inv = np.unique(np.concatenate([cb, cp]), axis=0, return_inverse=True)[1].reshape(-1)
        assert np.array_equal(case.tb, inv[:case.nb]) and np.array_equal(case.tp, inv[case.nb:])
    wide = np.arange(1 << 22, dtype=np.uint64).reshape(-1, 4)[np.random.default_rng(1).integers(0, 1 << 20, 3000)]
    tb, tp = tuple_ids(wide[:1000], wide[1000:])  # four columns of 2^20 values each: the ranks do not fit, rows are compared
    inv = np.unique(wide, axis=0, return_inverse=True)[1].reshape(-1)
    assert np.array_equal(tb, inv[:1000]) and np.array_equal(tp, inv[1000:])


def test_group_shapes():
    for shape in GROUP_SHAPES:
        cols, widths = group_shape(shape)
        assert [c.dtype.itemsize for c in cols] == widths and len({len(c) for c in cols}) == 1
    assert len(group_shape("hashed/2^20")[0][0]) == 1 << 20 and len(group_shape("S9")[0][0]) == (1 << 18) + 9
    k = key64_of("packed44", group_shape("S10")[0])
    assert np.all(k[1:] > k[:-1])


def test_mixed_key64_through_string_hashes_is_mixed_key64():
    import hashmergejoin_amd as H

    cols, _ = tuples_of("mixed", np.arange(0, 9000, 17))
    for bits in (0, 16):
        assert np.array_equal(key64_of("mixed", cols, None, bits), H.mixed_key64([[bytes(x) for x in cols[0].tolist()], cols[1]], bits))
    s = strings_of(np.array([0, 1, 3, 12345677, 3]))
    assert s.tolist() == [b"key-0-with-a-tail-of-22-byte", b"key-1", b"key-3-with-a-tail-of-22-byte", b"key-12345677", s[2]]


# ---- what the shape classes promise --------------------------------------------------------------------------------------------
def dup_stats(t):
    n = np.bincount(t)
    return n[n > 0]


@pytest.mark.parametrize("fam", ["packed44", "hashed842"])
def test_small_build_classes(fam):
    for nb in (1000, 60000):  # S1
        c = case_of_ids(fam, *ids_s1(nb))
        assert (c.nb, c.np) == (nb, 65536 + 1025) and dup_stats(c.tb).max() == 1 and c.collision_free()
        assert 0.22 < 1 - c.ref.p_match.mean() < 0.28
    c = case_of_ids(fam, *ids_s3())  # S3
    assert c.nb == 1000 and sorted(np.bincount(dup_stats(c.tb)).tolist()) == [0, 250, 500] and c.collision_free()
    assert 0.22 < 1 - c.ref.p_match.mean() < 0.28
    for nb, n_probe, missing in ((1000, 300001, 0), (5000, 700000, 1 / 3)):  # S6
        c = case_of_ids(fam, *ids_s6(nb, n_probe, missing))
        assert (c.nb, c.np) == (nb, n_probe) and dup_stats(c.tb).max() == 1 and c.collision_free()
        assert c.ref.p_match.all() if not missing else 0.31 < 1 - c.ref.p_match.mean() < 0.36
        assert c.ref.b_match.all()


@pytest.mark.parametrize("fam", ["packed44", "hashed842"])
def test_mid_size_classes(fam):
    c = case_of_ids(fam, *ids_s4())  # S4
    assert (c.nb, c.np) == (300000, 400000) and dup_stats(c.tb).max() == 1 and dup_stats(c.tp).max() == 1 and c.collision_free()
    assert int((~c.ref.p_match).sum()) == 400000 // 3
    assert not np.all(np.diff(c.kb.astype(np.float64)) >= 0) and not np.all(np.diff(c.kp.astype(np.float64)) >= 0)
    c = case_of_ids(fam, *ids_s5())  # S5
    assert c.nb == 1 << 14 and c.np == 70 * (1 << 14) + 13 and dup_stats(c.tb).max() == 1 and c.collision_free()
    assert int((~c.ref.p_match).sum()) == 13 and c.ref.b_match.all()
    assert sorted(set(dup_stats(c.tp[c.ref.p_match]).tolist())) == [70]
    c = case_of_ids(fam, *ids_s8())  # S8
    hot = dup_stats(c.tp).max()
    assert 0.29 < hot / c.np < 0.31 and c.ref.p_match[c.tp == np.bincount(c.tp).argmax()].all() and dup_stats(c.tb).max() == 1
    assert c.collision_free()


@pytest.mark.parametrize("fam,bits", [("packed44", 0), ("hashed842", 0), ("hashed842", 16), ("mixed", 0), ("mixed", 16), ("str", 0), ("str", 16),
                                      ("nulleq842", 0), ("nulleq842", 16)])
def test_many_to_many_class(fam, bits):
    c = case_of_ids(fam, *ids_s7(), bits=bits)  # S7
    assert (c.nb, c.np) == (200000, 300000) and len(dup_stats(c.tb)) == 30000
    assert set(dup_stats(c.tb).tolist()) == {6, 7} and set(dup_stats(c.tp).tolist()) == {10}
    assert int(c.ref.b_match.sum()) < c.nb and int(c.ref.p_match.sum()) == 270000
    if bits:  # runs of equal key64 hold several tuples, none beyond the collision sort's 1024 rows
        assert not c.collision_free() and 70 < c.ref.max_mixed_run() <= 1024
        assert c.ref.rows(BUILD, FULL_OUTER)[3] > 0 and c.ref.rows(PROBE, SEMI)[3] > 0
    else:
        assert c.collision_free()
    if fam == "packed44":
        h = case_of_ids(fam, *ids_s7(hot=5000))
        assert dup_stats(h.tb).max() >= 5000 and h.ref.p_match[h.tp == np.bincount(h.tb).argmax()].all()


def test_structured_packed_classes():
    c = case_s9()  # S9
    assert (c.nb, c.np) == ((1 << 18) + 9, (1 << 20) + 5) and not c.bcols[0].any()
    assert np.array_equal(np.sort(c.kb), np.arange(c.nb, dtype=np.uint64)) and int(c.kp.max()) >= c.nb
    assert 0.18 < 1 - c.ref.p_match.mean() < 0.22
    for fam in ("packed44", "packed8"):  # S10
        c = case_s10(fam)
        assert np.all(c.kb[1:] > c.kb[:-1]) and np.all(c.kp[1:] > c.kp[:-1])
        assert np.all(np.diff(c.tb) > 0) and int((~c.ref.p_match).sum()) == 400000 // 3
    for fam in ("packed8", "packed44", "packed2222"):  # S2
        base = case_of_ids(fam, *ids_s1(1000))
        c = with_marker(base, [77], slice(5, None, 1000))
        assert int(c.kb[77]) == M64 and (c.kb == M64).sum() == 1 and (c.kp == M64).sum() == 67
        assert c.ref.p_match[5::1000].all() and c.ref.b_match[77]
        c = with_marker(base, [], slice(5, None, 1000))
        assert not (c.kb == M64).any() and not c.ref.p_match[5::1000].any()
