"""The grid caps of the column operators, and the cases that take every capped kernel past its cap (CPU side).

The column operators cap their grids at a few workgroups per compute unit and walk the rest grid-stride; the second and later
trips are where they carry state (LDS counts reused behind a barrier, histograms accumulated over tiles, a prefetched map
entry, ballot words written at base >> 6).  test_grid_caps_gpu.py runs each of them past its cap; this file holds what that
needs and what can be checked without a GPU:
  CAPS        per kernel family the workgroups of the cap and the rows one workgroup takes per trip, with the places in the
              sources that say so -- a test fails when a multiplier or a thread constant is no longer what the table says,
              so that the sizes cannot drift under the caps silently;
  rows_past   the population at which most workgroups make `trips` trips, five make one more, and the last tile is partial
              with whole inactive waves;
  builders    the cases, pure numpy, with the CU count as a parameter: each is checked here at a stand-in CU count against
              the references (and, where cheap, a brute-force sort) and its structural claims are asserted;
  references  a vectorised inner multi-column join (checked against the dict-of-tuples references of the join tests) and a
              vectorised form of test_group_agg_cpu.assert_aggs (same bounds)."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = "hashmergejoin_amd/csrc/"
NO_ROW = 0xFFFFFFFFFFFFFFFF
DESC, NULLS_FIRST = 1, 2
RUN_CAP = 1024  # kRunCap: rows of one mixed run the collision sort holds
U = 2.0 ** -53
STAND_IN_CUS = 1

# ---- the caps ------------------------------------------------------------------------------------------------------------------
# per_cu: workgroups per compute unit (fixed: workgroups whatever the device); rows: what one workgroup takes per trip;
# sources: (file, regular expression, occurrences) -- the launches' multipliers and the thread constants the rows follow from.
CAPS = {
    "topk": dict(per_cu=8, fixed=None, rows=256, sources=[
        (CSRC + "topk.hip", r"num_cus \* 8\b", 1), (CSRC + "hmj_topkplan.h", r"kTopkThreads = 256;", 1), (CSRC + "hmj_order.h", r"OB_THREADS = 256;", 1)]),
    "orderby": dict(per_cu=8, fixed=None, rows=256, sources=[
        (CSRC + "orderby.hip", r"num_cus \* 8\b", 2), (CSRC + "hmj_order.h", r"OB_THREADS = 256;", 1)]),
    "take": dict(per_cu=16, fixed=None, rows=256, sources=[
        (CSRC + "take.hip", r"num_cus \* 16\b", 1), (CSRC + "take.hip", r"TK_THREADS = 256;", 1)]),
    "agg_finish": dict(per_cu=16, fixed=None, rows=256, sources=[
        (CSRC + "groupagg.hip", r"num_cus \* 16\b", 1), (CSRC + "groupagg.hip", r"GA_THREADS = 256;", 1)]),
    "col_keys": dict(per_cu=16, fixed=None, rows=256, sources=[
        (CSRC + "coljoin.hip", r"num_cus \* 16\b", 3), (CSRC + "coljoin.hip", r"CJ_THREADS = KJ_THREADS;", 1),
        (CSRC + "hmj_keyjoin.h", r"KJ_THREADS = 256;", 1)]),
    "run_leader": dict(per_cu=None, fixed=1024, rows=256, sources=[
        (CSRC + "hmj_group.h", r"gl < 1024 \? gl : 1024\b", 1), (CSRC + "hmj_keyjoin.h", r"gl < 1024 \? gl : 1024\b", 1),
        (CSRC + "hmj_keyjoin.h", r"KJ_THREADS = 256;", 1)]),
    "run_sort": dict(per_cu=4, fixed=None, rows=1, sources=[  # one workgroup per list entry
        (CSRC + "hmj_group.h", r"\(u64\)\(4 \* c->num_cus\)", 2), (CSRC + "hmj_keyjoin.h", r"\(u64\)\(4 \* c->num_cus\)", 2)]),
}


def cap_of(family, cus):
    """The workgroups of the family's cap on a device of `cus` compute units."""
    e = CAPS[family]
    return e["fixed"] if e["fixed"] is not None else e["per_cu"] * int(cus)


def rows_past(cap_workgroups, rows_per_workgroup, trips=2):
    """A population past the cap: most workgroups make `trips` trips, five make one more, and the last tile is partial -- 77
    rows, one whole wave, one of 13 lanes and two that are inactive (for tiles of 256 rows)."""
    return trips * cap_workgroups * rows_per_workgroup + 5 * rows_per_workgroup + 77


def size_past(family, cus, trips=2):
    return rows_past(cap_of(family, cus), CAPS[family]["rows"], trips)


def cap_rows(family, cus):
    """The rows one launch of the family takes without a second trip."""
    return cap_of(family, cus) * CAPS[family]["rows"]


def count_in_source(path, pattern):
    with open(os.path.join(ROOT, path)) as f:
        return len(re.findall(pattern, f.read()))


@pytest.mark.parametrize("family", sorted(CAPS))
def test_the_cap_table_is_what_the_sources_say(family):
    for path, pattern, times in CAPS[family]["sources"]:
        found = count_in_source(path, pattern)
        assert found == times, ("CAPS[%r]: %s holds /%s/ %d time(s), the table expects %d: a grid cap or a thread constant changed, and the "
                                "sizes of test_grid_caps_gpu.py may no longer pass it -- bring the table in line with the launch"
                                % (family, path, pattern, found, times))


def test_the_source_check_notices_a_changed_multiplier(tmp_path):
    text = open(os.path.join(ROOT, CSRC + "take.hip")).read()
    assert len(re.findall(r"num_cus \* 16\b", text)) == 1
    for changed in (text.replace("num_cus * 16", "num_cus * 32"), text.replace("num_cus * 16", "num_cus * 160")):
        assert len(re.findall(r"num_cus \* 16\b", changed)) == 0
    assert len(re.findall(r"TK_THREADS = 256;", text.replace("TK_THREADS = 256", "TK_THREADS = 512"))) == 0


def test_rows_past_puts_a_partial_tile_behind_whole_trips():
    assert rows_past(8 * 256, 256) == 1049933 and rows_past(16 * 256, 256) == 2098509 and rows_past(1024, 1) == 2130
    for cap, rows, trips in ((8, 256, 2), (16, 256, 2), (8 * 256, 256, 2), (4, 1, 2), (8, 256, 3)):
        n = rows_past(cap, rows, trips)
        assert n == trips * cap * rows + 5 * rows + 77
        tiles = -(-n // rows)
        per_workgroup = [len(range(w, tiles, cap)) for w in range(cap)]  # tile t goes to workgroup t % cap
        if rows == 256:
            assert tiles == trips * cap + 6 and n % rows == 77  # the last tile: 64 + 13 rows, two waves without a row
            more = min(6, cap)
            assert sorted(per_workgroup)[-more:] == [per_workgroup[0]] * more and per_workgroup[0] > trips
        assert min(per_workgroup) >= trips
    assert size_past("topk", 256) == 1049933 and cap_rows("run_leader", 7) == 262144 and cap_of("run_sort", 256) == 1024


# ---- the digit schedule of a top-k window (hmj_topkplan.h), to count the levels a builder's keys cost ------------------------------
TOPK_DIGIT_BITS = 11


def window_digits(varying):
    """The (shift, width) digits of a window whose rows differ in the bits of `varying`, when no level stops the selection:
    the top 11 bits first, then up to 11 bits ending at the highest varying bit below the decided ones."""
    out, lo = [(64 - TOPK_DIGIT_BITS, TOPK_DIGIT_BITS)], 64 - TOPK_DIGIT_BITS
    while True:
        below = varying & ((1 << lo) - 1)
        if not below:
            return out
        top = below.bit_length()
        width = min(top, TOPK_DIGIT_BITS)
        out.append((top - width, width))
        lo = top - width


def test_window_digits_on_hand_cases():
    assert window_digits(0) == [(53, 11)]
    assert window_digits((1 << 10) - 1) == [(53, 11), (0, 10)]  # keys below 2^10: two levels
    assert window_digits((1 << 64) - 1) == [(53, 11), (42, 11), (31, 11), (20, 11), (9, 11), (0, 9)]
    assert len(window_digits(0x3333333333333333)) == 6


# ---- strings -------------------------------------------------------------------------------------------------------------------
PREFIX = b"twenty-byte-prefix-->"[:20]


def string_pool(rng, distinct=3000):
    """`distinct` different strings behind one 20-byte prefix: tails of 0 to 12 letters, so some strings are prefixes of
    others and the lengths cross the 7-byte blocks of the order stream."""
    pool = {PREFIX, PREFIX + b"a", PREFIX + b"aa", PREFIX + b"b"}
    while len(pool) < distinct:
        ln = int(rng.integers(1, 13))
        pool.add(PREFIX + bytes(rng.integers(0x61, 0x67, size=ln).astype(np.uint8)))
    pool = sorted(pool)
    return [pool[k] for k in rng.permutation(len(pool))]


def string_table(cus, seed=41, trips=2):
    """[pool strings (about 10 % NULL), int32] over size_past("topk") rows.  Returns a dict: n, strs (list of bytes), valid,
    i32 and pool."""
    rng = np.random.default_rng(seed)
    n = size_past("topk", cus, trips)
    pool = string_pool(rng)
    pick = rng.integers(0, len(pool), size=n)
    strs = [pool[k] for k in pick.tolist()]
    return {"n": n, "strs": strs, "valid": rng.random(n) >= 0.1, "i32": rng.integers(-500, 500, size=n).astype(np.int32), "pool": pool, "pick": pick}


def string_specs(table, flags):
    """The arguments of test_order_by_gpu.spec for the table's two columns: the strings under `flags` with their validity at
    bit offset 3 and 3 bytes in front of the chars, the int32 column descending."""
    return [(table["strs"], flags, table["valid"], 3, 3), (table["i32"], DESC, None, 0, 0)]


def bad_offset_rows(cus, trips=2):
    """Two rows of a size_past("topk") table whose offsets a refusal test raises: one in a tile of the trip behind the whole
    ones, one in the partial last tile.  The lower one is what the refusal names."""
    cap, n = cap_of("topk", cus), size_past("topk", cus, trips)
    later = (trips * cap + 2) * 256 + 17
    last = n - 9
    assert trips * cap * 256 <= later < (trips * cap + 5) * 256 and n - 77 <= last < n - 1
    return later, last


# ---- top-k: column mode ----------------------------------------------------------------------------------------------------------
def topk_unique_keys(cus, seed=42):
    rng = np.random.default_rng(seed)
    n = size_past("topk", cus)
    return rng.permutation(n).astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15)  # (odd: a bijection mod 2^64)


def topk_small_keys(cus, seed=43):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 1 << 10, size=size_past("topk", cus)).astype(np.uint64)


def topk_three_values(cus, seed=44):
    """int8 rows of three values; returns (values, rows of the lowest value, rows of the middle one)."""
    rng = np.random.default_rng(seed)
    i8 = np.array([-3, 9, 100], np.int8)[rng.integers(0, 3, size=size_past("topk", cus))]
    return i8, int(np.count_nonzero(i8 == -3)), int(np.count_nonzero(i8 == 9))


# ---- top-k: list mode ------------------------------------------------------------------------------------------------------------
LIST_VALUES = (0x1111111111111111, 0x2222222222222222, 0x3333333333333333)  # they differ in every digit of a window: 6 levels


def topk_list_case(cus, coarse=None, seed=45):
    """Column A: three uint64 values, the middle one in more than cap_rows + 5 * 256 + 77 rows; column B: uint64, random in all
    64 bits (coarse None), in the top 16 only ("top16": about ten rows of the middle value share a B and are equal in every
    column) or in the top 16 and the low 8 ("top16+low8": those rows differ below the digits a selection walks before their
    set fits).  The cut K lies inside the middle value.  Returns a dict: n, a, b, lo, mid, K, shift (the bits of B below it
    are the low ones)."""
    rng = np.random.default_rng(seed)
    n = size_past("topk", cus)
    which = rng.choice(3, size=n, p=[0.15, 0.7, 0.15])
    a = np.array(LIST_VALUES, np.uint64)[which]
    if coarse is None:
        b = rng.integers(0, 1 << 64, size=n, dtype=np.uint64)
    else:
        b = rng.integers(0, 1 << 16, size=n).astype(np.uint64) << np.uint64(48)
        if coarse == "top16+low8":
            b |= rng.integers(0, 1 << 8, size=n).astype(np.uint64)
    lo, mid = int(np.count_nonzero(which == 0)), int(np.count_nonzero(which == 1))
    return {"n": n, "a": a, "b": b, "lo": lo, "mid": mid, "K": lo + mid // 2, "shift": 0 if coarse is None else 48}


def cut_tie_set(case):
    """Of the list case: (rows of the middle value that share B's bits from `shift` up with the K-th row of the order, how
    many of them the cut takes)."""
    order = np.lexsort((case["b"], case["a"]))
    top = case["b"] >> np.uint64(case["shift"])
    at = order[case["K"] - 1]
    same = (case["a"] == case["a"][at]) & (top == top[at])
    first = int(np.searchsorted(top[order[case["lo"]:case["lo"] + case["mid"]]], top[at], "left")) + case["lo"]
    return int(np.count_nonzero(same)), case["K"] - first


# ---- ORDER BY: round 2 over a list as long as the input ------------------------------------------------------------------------------
def order_round2_case(cus, seed=46):
    """Column A: uint64, every value at least twice; column B: uint32, all distinct.  Returns (a, b)."""
    rng = np.random.default_rng(seed)
    n = size_past("orderby", cus)
    d = n // 3
    ids = np.concatenate([np.arange(d), np.arange(d), rng.integers(0, d, size=n - 2 * d)])
    a = (ids[rng.permutation(n)].astype(np.uint64) + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
    return a, rng.permutation(n).astype(np.uint32)


# ---- take_cols -------------------------------------------------------------------------------------------------------------------
TAKE_DTYPES = {1: np.uint8, 2: np.int16, 4: np.float32, 8: np.int64, 16: np.int64}
TAKE_SHAPES = ([1, 2, 4, 8, 16, 8, 4, 2], [2, 16, 4], [16, 1], [8])  # the 8-, 4-, 2- and 1-column bodies
TAKE_PATTERN = 0xA5


def take_positions(cus, trips=2):
    """Map positions in the first tile, in a tile of the trip behind the whole ones, and in the partial last wave."""
    cap, n_out = cap_of("take", cus), size_past("take", cus, trips)
    pos = [3, 200, (trips * cap + 2) * 256 + 17, (trips * cap + 4) * 256 + 255, n_out - 5, n_out - 1]
    assert pos[1] < 256 and trips * cap * 256 <= pos[2] < pos[3] < (trips * cap + 5) * 256 and n_out - 13 <= pos[4]
    return pos


def take_case(cus, widths, n_src=50000, seed=47, trips=2):
    """Source columns of `widths` bytes (a bitmap on every second one, the bytes under its NULL slots spelling TAKE_PATTERN)
    and two maps of size_past("take") entries: `good`, about 20 % NO_ROW and NO_ROW at take_positions, and `bad`, the same
    with entries beyond the source at take_positions.  Returns a dict: cols, masks, good, bad, n_bad, positions."""
    rng = np.random.default_rng(seed + len(widths))
    n_out = size_past("take", cus, trips)
    cols, masks = [], []
    for c, w in enumerate(widths):
        mask = rng.random(n_src) >= 0.3 if c % 2 == 0 else None
        raw = rng.integers(0, 256, size=(n_src, w), dtype=np.uint8)
        if mask is not None:
            raw[~mask] = TAKE_PATTERN
        col = raw.reshape(-1).view(TAKE_DTYPES[w])
        cols.append(col.reshape(n_src, 2) if w == 16 else col)
        masks.append(mask)
    good = rng.integers(0, n_src, size=n_out).astype(np.uint64)
    good[rng.random(n_out) < 0.2] = NO_ROW
    pos = take_positions(cus, trips)
    bad = good.copy()
    good[pos] = NO_ROW
    bad[pos] = np.array([n_src, 2 ** 63, n_src + 1, 2 ** 64 - 2, n_src, 2 ** 40], np.uint64)
    return {"cols": cols, "masks": masks, "good": good, "bad": bad, "n_bad": len(pos), "positions": pos, "n_src": n_src}


# ---- group_agg: the finish kernel ----------------------------------------------------------------------------------------------------
def agg_marked_groups(cus, trips=2):
    """(groups of three rows, groups without a valid row): in the first tile, in the second trip, in the trip behind the whole
    ones and in the partial last wave."""
    cap, ng = cap_of("agg_finish", cus), size_past("agg_finish", cus, trips)
    three = [0, 255, cap * 256, (trips * cap + 1) * 256 + 63, ng - 1]
    none = [1, 64, cap * 256 + 1, (trips * cap + 3) * 256, ng - 2, ng - 77]
    return three, none


def agg_case(cus, seed=48, trips=2):
    """size_past("agg_finish") groups of one row -- the key is the group's number, so that an ordered grouping by it numbers
    the groups as the key does --, a few of three rows, and a few (and about 5 % of the others) without a valid row.
    Returns a dict: ng, key (uint64, shuffled rows), valid, i64, f64, f32, u8, three, none."""
    rng = np.random.default_rng(seed)
    ng = size_past("agg_finish", cus, trips)
    three, none = agg_marked_groups(cus, trips)
    key = np.concatenate([np.arange(ng), np.repeat(three, 2)]).astype(np.uint64)
    key = key[rng.permutation(len(key))]
    n = len(key)
    valid = rng.random(n) >= 0.05
    valid[np.isin(key, np.array(three, np.uint64))] = True
    valid[np.isin(key, np.array(none, np.uint64))] = False
    f32 = (rng.standard_normal(n) * 8).astype(np.float32)
    odd = rng.random(n) < 0.3
    f32[odd] = np.array([np.nan, 0.0, -0.0, np.inf, -np.inf, 1.5], np.float32)[rng.integers(0, 6, size=n)][odd]
    return {"ng": ng, "key": key, "valid": valid, "three": three, "none": none,
            "i64": rng.integers(-2 ** 63, 2 ** 63, size=n, dtype=np.int64), "f32": f32,
            "f64": rng.standard_normal(n) * 2.0 ** rng.integers(-20, 20, size=n), "u8": rng.integers(0, 256, size=n).astype(np.uint8)}


def agg_list(H, case):
    return [(H.HMJ_AGG_SUM, case["i64"], case["valid"]), (H.HMJ_AGG_MEAN, case["f64"], case["valid"]), (H.HMJ_AGG_MIN, case["f32"], case["valid"]),
            (H.HMJ_AGG_COUNT, None, case["valid"]), (H.HMJ_AGG_MAX, case["u8"], case["valid"])]


def gamma(k):
    return k * U / (1.0 - k * U)


def assert_aggs_vectorised(H, got, want, aggs, n_groups, tag=""):
    """test_group_agg_cpu.assert_aggs without its loop over the groups: integers, counts and every MIN / MAX exactly (floats
    bit for bit), the bitmaps and null counts exactly, float SUM and every MEAN under |got - fsum| <= gamma_k sum|x| (MEAN:
    gamma_(k+1), over the count), a reference that is not finite matched as it is, a NULL slot all zero bits."""
    for k, ((v, ok, nulls), w, a) in enumerate(zip(got, want, aggs)):
        op, t = int(a[0]), (k, tag, int(a[0]), None if a[1] is None else str(a[1].dtype))
        assert len(v) == n_groups and v.dtype == w["values"].dtype, t
        assert nulls == w["null_count"], (t, nulls, w["null_count"])
        if ok is not None:
            assert np.array_equal(ok, w["valid"]), (t, np.flatnonzero(ok != w["valid"])[:5])
        bits = "u%d" % v.dtype.itemsize
        if w["abs_sum"] is None:
            bad = np.flatnonzero(v.view(bits) != w["values"].view(bits))
            assert not len(bad), (t, bad[:5], v[bad[:5]], w["values"][bad[:5]])
            continue
        x, y, cnt, s = v.astype(np.float64), w["values"].astype(np.float64), w["count"].astype(np.float64), w["abs_sum"]
        empty = cnt == 0
        assert not v.view(bits)[empty].any(), (t, "a NULL slot holds bits")
        finite = ~empty & np.isfinite(y) & np.isfinite(s)
        rest = ~empty & ~finite
        assert np.all((np.isnan(x[rest]) & np.isnan(y[rest])) | (x[rest] == y[rest])), (t, "non-finite groups differ")
        kk = np.maximum(cnt, 1.0)
        bound = gamma(kk + 1) * s / kk if op == H.HMJ_AGG_MEAN else gamma(kk) * s
        with np.errstate(invalid="ignore"):
            bad = np.flatnonzero(finite & ~(np.abs(x - y) <= bound))
        for g in bad[:5]:
            print("aggregate %d group %d: got %r want %r bound %.3e k %d" % (k, g, x[g], y[g], bound[g], cnt[g]))
        assert not len(bad), (t, bad[:5])


# ---- multi-column keys -----------------------------------------------------------------------------------------------------------
KEY_WIDTHS = [8, 4]


def tuple_of_id(ids):
    """An injective [uint64, uint32] tuple per id (ids below 2^32), and whether the id's second slot is NULL (about 5 %)."""
    ids = np.asarray(ids, np.uint64)
    a = (ids >> np.uint64(3)) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(12345)  # eight ids share column 0
    b = (ids * np.uint64(2654435761) & np.uint64(0xFFFFFFFF)).astype(np.uint32)   # (odd: a bijection mod 2^32)
    return a, b, (ids * np.uint64(0x2545F4914F6CDD1D) >> np.uint64(40)) % np.uint64(20) == 0


def key_group_case(cus, seed=49):
    """size_past("col_keys") rows of [8, 4] tuples drawn from 0.6 n ids, a bitmap on both columns: column 1 NULL where the id
    says so (garbage under the slot), column 0 NULL in about 1 % of the rows.  Returns (cols, valid)."""
    rng = np.random.default_rng(seed)
    n = size_past("col_keys", cus)
    ids = rng.integers(0, int(0.6 * n), size=n)
    a, b, null1 = tuple_of_id(ids)
    null0 = rng.random(n) < 0.01
    b = b.copy()
    b[null1] = rng.integers(0, 1 << 32, size=int(null1.sum())).astype(np.uint32)
    a = a.copy()
    a[null0] = rng.integers(0, 1 << 63, size=int(null0.sum())).astype(np.uint64)
    return [a, b], [~null0, ~null1]


def key_join_case(cus, seed=50):
    """Build: size_past("col_keys") distinct tuples in a drawn order; probe: as many rows drawn from 1.2 times as many ids
    (misses, duplicates).  Column 1 of an id is NULL on both sides or on neither.  Returns (bcols, bvalid, pcols, pvalid):
    bvalid / pvalid one entry per column, None for column 0."""
    rng = np.random.default_rng(seed)
    n = size_past("col_keys", cus)
    bid = rng.permutation(n)
    pid = rng.integers(0, int(1.2 * n), size=n)
    ba, bb, bn = tuple_of_id(bid)
    pa, pb, pn = tuple_of_id(pid)
    pb = pb.copy()
    pb[pn] = 0xEEEEEEEE  # garbage under the NULL slots of one side
    return [ba, bb], [None, ~bn], [pa, pb], [None, ~pn]


def _tuple_keys(cols, widths, valid):
    """The sort keys of one relation's tuples, the first column's first: per column the value (0 under a NULL slot) with the
    NULL flag above it -- NULLS LAST --, the flag a key of its own for an 8-byte column; and the rows with a NULL slot."""
    keys, any_null = [], np.zeros(len(cols[0]), bool)
    for c, (col, w) in enumerate(zip(cols, widths)):
        a = np.ascontiguousarray(col)
        v = a.view("u%d" % w).astype(np.uint64) if a.dtype.itemsize == w else a.astype(np.uint64)
        null = np.zeros(len(v), bool) if valid is None or valid[c] is None else ~np.asarray(valid[c], bool)
        v = np.where(null, np.uint64(0), v)
        any_null |= null
        keys += [null.astype(np.uint64), v] if w == 8 else [v | (null.astype(np.uint64) << np.uint64(8 * w))]
    return keys, any_null


def expected_inner_join(H, bcols, pcols, widths, bvalid=None, pvalid=None, hash_bits=0, null_equal=False, bvals=None, pvals=None):
    """The rows of an inner multi-column join, vectorised: [n, 5] uint64 (key64, r_row, s_row, rval, sval) in the
    HMJ_ORDERED order (key64, tuple column by column as unsigned integers with NULLS LAST, r_row, s_row), and the pairs of
    equal key64 (n_key_pairs).  A row with a NULL slot matches nothing, or -- null_equal -- rows whose NULL slots are the
    same columns' and whose other slots are equal.  vals None: the payload of row i is i."""
    nb, np_ = len(bcols[0]), len(pcols[0])
    (bkeys, b_null), (pkeys, p_null) = _tuple_keys(bcols, widths, bvalid), _tuple_keys(pcols, widths, pvalid)
    keys = [np.concatenate([x, y]) for x, y in zip(bkeys, pkeys)]
    keys = [k for k in keys if k.any()] or keys[:1]  # (a key that is 0 in every row orders nothing)
    order = np.lexsort(keys[::-1])  # the tuples' dense rank in tuple order, both sides at once
    new = np.zeros(nb + np_, bool)
    for k in keys:
        s = k[order]
        new[1:] |= s[1:] != s[:-1]
    tid = np.empty(nb + np_, np.int64)
    tid[order] = np.cumsum(new)
    bt, pt = tid[:nb].copy(), tid[nb:]
    bitmap = (bvalid is not None and any(v is not None for v in bvalid)) or (pvalid is not None and any(v is not None for v in pvalid))
    if null_equal and bitmap:
        kb = H.cols_key64(bcols, widths, hash_bits, valid=bvalid, null_equal=True)
        kp = H.cols_key64(pcols, widths, hash_bits, valid=pvalid, null_equal=True)
        b_rows, p_rows = np.arange(nb), np.arange(np_)
    else:
        kb, kp = H.cols_key64(bcols, widths, hash_bits), H.cols_key64(pcols, widths, hash_bits)
        bt[b_null] = -1  # (no probe row that has a key has this number)
        b_rows, p_rows = np.flatnonzero(~b_null), np.flatnonzero(~p_null)
    # per build row, in row order, the probe rows of its tuple in row order: the pairs arrive ordered by (r_row, s_row)
    by_tuple = p_rows[np.argsort(pt[p_rows], kind="stable")]
    per_tuple = np.bincount(pt[p_rows], minlength=int(tid.max()) + 1)
    first_of = np.cumsum(per_tuple) - per_tuple  # where a tuple's probe rows start in by_tuple
    has = bt >= 0
    lo, cnt = np.where(has, first_of[bt], 0), np.where(has, per_tuple[bt], 0)
    r_row = np.repeat(np.arange(nb), cnt)
    s_row = by_tuple[np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt) + np.repeat(lo, cnt)]
    key = kb[r_row]
    final = np.lexsort((bt[r_row], key))  # (stable)
    r_row, s_row, key = r_row[final], s_row[final], key[final]
    rval = r_row.astype(np.uint64) if bvals is None else np.asarray(bvals, np.uint64)[r_row]
    sval = s_row.astype(np.uint64) if pvals is None else np.asarray(pvals, np.uint64)[s_row]
    rows = np.stack([key, r_row.astype(np.uint64), s_row.astype(np.uint64), rval, sval], axis=1).reshape(-1, 5)
    # pairs of equal key64 among the rows that have a key
    bk, pk = np.sort(kb[b_rows]), np.sort(kp[p_rows])  # (sorted needles: the searches walk bk once)
    n_key_pairs = int((np.searchsorted(bk, pk, "right") - np.searchsorted(bk, pk, "left")).sum())
    return rows, n_key_pairs


# ---- the collision sort -----------------------------------------------------------------------------------------------------------
def collision_case(n_tuples, n_extra, seed=51):
    """n_tuples distinct [8, 4] tuples and n_extra more rows that repeat some of them, in a drawn order.  Returns (cols, ids)."""
    rng = np.random.default_rng(seed)
    ids = np.concatenate([np.arange(n_tuples), rng.integers(0, n_tuples, size=n_extra)])
    ids = ids[rng.permutation(len(ids))]
    a, b, _ = tuple_of_id(ids)
    return [a, b], ids


def run_shape(key64, ids):
    """Of rows with these key64 and tuple numbers: (runs of equal key64 that hold several tuples, rows of the longest such
    run, entries of the collision search's list: positions of the rows sorted by (key64, row) whose key64 equals the
    predecessor's and whose tuple differs)."""
    order = np.argsort(key64, kind="stable")
    k, t = key64[order], ids[order]
    entries = int(np.count_nonzero((k[1:] == k[:-1]) & (t[1:] != t[:-1])))
    uk, inv, rows = np.unique(key64, return_inverse=True, return_counts=True)
    pairs = np.unique(np.stack([inv.reshape(-1), ids]), axis=1)
    tuples = np.bincount(pairs[0], minlength=len(uk))
    mixed = tuples > 1
    return int(mixed.sum()), int(rows[mixed].max()) if mixed.any() else 0, entries


COLLISION_SHAPES = {"runs": dict(n_tuples=40000, n_extra=5000, hash_bits=11), "leader": dict(n_tuples=300000, n_extra=3000, hash_bits=12)}


# ---- the builders at a stand-in CU count --------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def H():
    import hashmergejoin_amd as H

    return H


def test_the_stand_in_sizes_pass_their_caps():
    for family in CAPS:
        assert size_past(family, STAND_IN_CUS) > 2 * cap_rows(family, STAND_IN_CUS)
    assert size_past("topk", STAND_IN_CUS) == 2 * 8 * 256 + 5 * 256 + 77


def test_top_k_column_builders(H):
    from test_order_by_cpu import brute_order

    n = size_past("topk", STAND_IN_CUS)
    u = topk_unique_keys(STAND_IN_CUS)
    assert len(u) == n and len(np.unique(u)) == n
    want = np.argsort(u, kind="stable").astype(np.uint64)
    for offset in (0, n - 10):
        assert np.array_equal(H.expected_top_k([(u, 0, None)], 10, offset), want[offset:offset + 10])
    small = topk_small_keys(STAND_IN_CUS)
    assert int(small.max()) < 1 << 10 and len(window_digits(int(np.bitwise_or.reduce(small) ^ np.bitwise_and.reduce(small)))) == 2
    assert np.array_equal(H.expected_top_k([(small, 0, None)], 37, 5), np.argsort(small, kind="stable")[5:42].astype(np.uint64))
    i8, lo, mid = topk_three_values(STAND_IN_CUS)
    assert sorted(set(i8.tolist())) == [-3, 9, 100] and lo > 20 and mid > 20
    K = lo + mid // 2
    got = H.expected_top_k([(i8, 0, None)], 20, K - 20)
    assert np.array_equal(got, np.flatnonzero(i8 == 9)[mid // 2 - 20:mid // 2].astype(np.uint64))  # the ties in ascending row index
    assert np.array_equal(H.expected_order_by([(i8[:300], 0, None)]), np.array(brute_order([(i8[:300], 0, None)]), np.uint64))


@pytest.mark.parametrize("coarse", [None, "top16", "top16+low8"])
def test_top_k_list_builder(H, coarse):
    case = topk_list_case(STAND_IN_CUS, coarse)
    n, lo, mid, K = case["n"], case["lo"], case["mid"], case["K"]
    assert sorted(set(case["a"].tolist())) == list(LIST_VALUES)
    assert mid > cap_rows("topk", STAND_IN_CUS) + 5 * 256 + 77 and lo < K - 10 and K < lo + mid  # the tie list passes the cap; the cut is inside
    varying = int(np.bitwise_or.reduce(case["a"]) ^ np.bitwise_and.reduce(case["a"]))
    assert len(window_digits(varying)) == 6  # window 0 alone costs six levels: any further one walks the tie list
    want = np.lexsort((case["b"], case["a"])).astype(np.uint64)
    cols = [(case["a"], 0, None), (case["b"], 0, None)]
    assert np.array_equal(H.expected_top_k(cols, 10, K - 10), want[K - 10:K])
    assert int(H.order_stream_bytes(cols).max()) == 16
    digits = window_digits(int(np.bitwise_or.reduce(case["b"]) ^ np.bitwise_and.reduce(case["b"])))
    if coarse is None:
        assert cut_tie_set(case) == (1, 1)
    else:  # two levels walk the 16 top bits; the low 8 are a third digit, which a tie set that fits never reaches
        assert digits == [(53, 11), (42, 11)] + ([(0, 8)] if coarse == "top16+low8" else [])


@pytest.mark.parametrize("coarse", ["top16", "top16+low8"])
def test_the_coarse_list_cases_leave_a_tie_set_that_fits_at_the_device_size(coarse):
    case = topk_list_case(256, coarse)
    ties, taken = cut_tie_set(case)
    assert 1 <= taken < ties <= 64, (ties, taken)
    assert case["mid"] > cap_rows("topk", 256) + 5 * 256 + 77


def test_string_table_builder(H):
    from test_order_by_cpu import brute_order

    t = string_table(STAND_IN_CUS)
    n = t["n"]
    assert n == size_past("topk", STAND_IN_CUS) and len(set(t["pool"])) == len(t["pool"]) >= 3000
    assert all(s.startswith(PREFIX) for s in t["pool"]) and 0.05 < 1 - t["valid"].mean() < 0.15
    assert {len(s) for s in t["pool"]} >= set(range(20, 33))
    later, last = bad_offset_rows(STAND_IN_CUS)
    assert later < last and min(len(t["strs"][r]) for r in (later - 1, later, last - 1, last)) >= 7  # (a raised offset stays inside the chars)
    for flags in (NULLS_FIRST, DESC):
        cols = [(v, f, ok) for v, f, ok, _, _ in string_specs(t, flags)]
        want = H.expected_order_by(cols)
        # numpy alone: the strings' rank in bytes order, NULLs in front or behind, then the int32 descending
        rank = np.argsort(np.array(sorted(range(len(t["pool"])), key=lambda k: t["pool"][k])))[t["pick"]].astype(np.int64)
        rank = -rank if flags & DESC else rank
        rank[~t["valid"]] = -(1 << 40) if flags & NULLS_FIRST else 1 << 40
        assert np.array_equal(want, np.lexsort((-t["i32"].astype(np.int64), rank)).astype(np.uint64))
        assert np.array_equal(H.expected_top_k(cols, 10, 77), want[77:87])
        head = [(c[0][:400], c[1], None if c[2] is None else c[2][:400]) for c in cols]
        assert np.array_equal(H.expected_order_by(head), np.array(brute_order(head), np.uint64))
        S = H.order_stream_bytes(cols)
        assert int(S.max()) >= 1 + 8 * 4 + 4  # four blocks of a 27-byte string behind the marker, the int32: three rounds or more
    # the rows that agree in the first 8 stream bytes outnumber the cap: later rounds run over a list past it
    assert int(t["valid"].sum()) > cap_rows("orderby", STAND_IN_CUS)


def test_order_round2_builder(H):
    a, b = order_round2_case(STAND_IN_CUS)
    n = len(a)
    assert n == size_past("orderby", STAND_IN_CUS) and len(np.unique(b)) == n
    assert int(np.unique(a, return_counts=True)[1].min()) >= 2  # every row is in a segment of several rows after round 1
    want = H.expected_order_by([(a, 0, None), (b, 0, None)])
    assert np.array_equal(want, np.lexsort((b, a)).astype(np.uint64))
    assert int(H.order_stream_bytes([(a, 0, None), (b, 0, None)]).max()) == 12  # 8 bytes in round 1, the rest in round 2


@pytest.mark.parametrize("widths", TAKE_SHAPES, ids=lambda w: "%dcols" % len(w))
def test_take_builder(widths):
    from test_take_cols_cpu import expected_take

    case = take_case(STAND_IN_CUS, widths, n_src=500)
    n_out = size_past("take", STAND_IN_CUS)
    assert len(case["good"]) == len(case["bad"]) == n_out and sorted(set(widths)) == sorted(set(widths) & {1, 2, 4, 8, 16})
    pos = case["positions"]
    assert (case["good"][pos] == NO_ROW).all()
    beyond = (case["bad"] >= case["n_src"]) & (case["bad"] != NO_ROW)
    assert np.flatnonzero(beyond).tolist() == pos and case["n_bad"] == len(pos)
    data, words, nulls, n_no = expected_take(case["cols"], case["masks"], case["good"])
    assert n_no == int((case["good"] == NO_ROW).sum()) > n_out // 10
    for c, (d, w, m) in enumerate(zip(data, words, case["masks"])):
        assert len(w) == (n_out + 63) // 64 and int(w[-1]) >> (n_out % 64) == 0
        assert nulls[c] >= n_no and (m is None) == (nulls[c] == n_no)
        assert not d[pos].any()  # zero bytes under the NO_ROW slots


def test_agg_builder(H):
    from test_group_agg_cpu import assert_aggs

    case = agg_case(STAND_IN_CUS)
    ng, key = case["ng"], case["key"]
    three, none = case["three"], case["none"]
    assert ng == size_past("agg_finish", STAND_IN_CUS) and len(key) == ng + 2 * len(three)
    count = np.bincount(key.astype(np.int64), minlength=ng)
    assert len(count) == ng and set(np.flatnonzero(count == 3).tolist()) == set(three) and int(count.min()) == 1
    assert not set(three) & set(none) and max(three + none) < ng
    aggs = agg_list(H, case)
    want = H.expected_group_aggs(key, ng, aggs)
    for w in want[:3] + want[4:]:
        assert not w["valid"][none].any() and w["valid"][three].all() and 0 < w["null_count"] < ng // 5
    assert want[3]["valid"].all() and want[3]["values"][three].tolist() == [3] * len(three) and want[3]["values"][none].tolist() == [0] * len(none)
    # the three-row sums against Python integers, the mean against a plain sum
    for g in three:
        rows = np.flatnonzero(key == g)
        s = sum(int(x) for x in case["i64"][rows])
        assert int(want[0]["values"][g]) == ((s + (1 << 63)) % (1 << 64)) - (1 << 63)
        assert abs(float(want[1]["values"][g]) - float(case["f64"][rows].sum()) / 3) <= 4 * U * float(np.abs(case["f64"][rows]).sum())
        assert int(want[4]["values"][g]) == int(case["u8"][rows].max())
    # the vectorised comparison accepts what assert_aggs accepts and refuses a wrong bit
    as_got = lambda w: (w["values"].copy(), w["valid"].copy(), w["null_count"])
    got = [as_got(w) for w in want]
    assert_aggs(H, got, want, aggs, ng)
    assert_aggs_vectorised(H, got, want, aggs, ng)
    g = three[1]
    for k, delta in ((0, 1), (1, 1e-3), (2, 1.0), (4, 1)):
        bad = [as_got(w) for w in want]
        bad[k][0][g] += delta
        with pytest.raises(AssertionError):
            assert_aggs_vectorised(H, bad, want, aggs, ng)
    bad = [as_got(w) for w in want]
    bad[1][1][none[0]] = True
    with pytest.raises(AssertionError):
        assert_aggs_vectorised(H, bad, want, aggs, ng)


def test_key_group_builder(H):
    from test_group_cols_cpu import assert_same, brute_groups

    cols, valid = key_group_case(STAND_IN_CUS)
    n = len(cols[0])
    assert n == size_past("col_keys", STAND_IN_CUS) and cols[0].dtype == np.uint64 and cols[1].dtype == np.uint32
    for ordered in (False, True):
        exp = H.expected_groups(cols, KEY_WIDTHS, None, valid, ordered=ordered)
        assert_same(exp, brute_groups(H, cols, KEY_WIDTHS, None, valid, ordered=ordered), ordered)
    assert exp["form"] == H.HMJ_COLS_HASHED and exp["n_collisions"] == 0 and 0.3 * n < exp["n_groups"] < 0.7 * n
    assert exp["n_null"] == int(np.count_nonzero(~valid[0] | ~valid[1])) > n // 50 and exp["max_count"] >= 3


def _tuples(cols, valid):
    out = []
    for i in range(len(cols[0])):
        out.append(tuple(None if (valid is not None and valid[c] is not None and not valid[c][i]) else int(cols[c][i]) for c in range(len(cols))))
    return out


@pytest.mark.parametrize("null_equal", [False, True])
def test_the_vectorised_join_agrees_with_the_dict_of_tuples(H, null_equal):
    from test_join_cols_kinds_cpu import INNER, PROBE
    from test_join_null_equal_cpu import ne_rows

    bcols, bvalid, pcols, pvalid = key_join_case(STAND_IN_CUS)
    nb, np_ = len(bcols[0]), len(pcols[0])
    assert nb == np_ == size_past("col_keys", STAND_IN_CUS)
    tb, tp = _tuples(bcols, bvalid), _tuples(pcols, pvalid)
    assert len(set(tb)) > nb - nb // 50 and sum(None in t for t in tb) > nb // 50 and sum(None in t for t in tp) > np_ // 50
    for bits in (0, 5):
        rows, pairs = expected_inner_join(H, bcols, pcols, KEY_WIDTHS, bvalid, pvalid, bits, null_equal)
        if null_equal:
            kb = H.cols_key64(bcols, KEY_WIDTHS, bits, valid=bvalid, null_equal=True).tolist()
            kp = H.cols_key64(pcols, KEY_WIDTHS, bits, valid=pvalid, null_equal=True).tolist()
            want, _, n_pairs, n_coll, seen = ne_rows(tb, tp, kb, kp, list(range(nb)), list(range(np_)), PROBE, INNER)
        else:  # a row with a NULL slot matches nothing: its tuple is made one of a kind, and it joins no key64 run
            kb, kp = H.cols_key64(bcols, KEY_WIDTHS, bits).tolist(), H.cols_key64(pcols, KEY_WIDTHS, bits).tolist()
            keep_b = [r for r, t in enumerate(tb) if None not in t]
            keep_p = [s for s, t in enumerate(tp) if None not in t]
            want, _, n_pairs, n_coll, seen = ne_rows([tb[r] for r in keep_b], [tp[s] for s in keep_p], [kb[r] for r in keep_b],
                                                      [kp[s] for s in keep_p], keep_b, keep_p, PROBE, INNER)
            want[:, 1], want[:, 2] = want[:, 3], want[:, 4]  # (the payloads are the rows' own numbers)
        assert rows.shape == want.shape and len(rows) > np_ // 2
        assert np.array_equal(rows, want), np.flatnonzero(np.any(rows != want, axis=1))[:5]
        assert pairs == n_pairs and (bits == 0) == (n_coll == 0) and (bits == 0) == ("sort" not in seen)
    matched_nulls = int(np.count_nonzero(~pvalid[1][rows[:, 2].astype(np.int64)]))
    assert (matched_nulls > 0) == null_equal


def test_the_vectorised_join_agrees_with_the_join_tests_brute_force(H):
    from test_join_cols_gpu import brute

    rng = np.random.default_rng(7)
    bcols, ids_b = collision_case(300, 200, seed=8)
    pa, pb, _ = tuple_of_id(rng.integers(0, 400, size=700))
    bv, pv = rng.integers(0, 1 << 64, size=500, dtype=np.uint64), rng.integers(0, 1 << 64, size=700, dtype=np.uint64)
    for bits in (0, 4):
        want, coll = brute(H, bcols, bv.tolist(), [pa, pb], pv.tolist(), KEY_WIDTHS, bits)
        rows, pairs = expected_inner_join(H, bcols, [pa, pb], KEY_WIDTHS, hash_bits=bits, bvals=bv, pvals=pv)
        assert np.array_equal(rows, want) and pairs == len(want) + coll and (coll > 0) == (bits == 4)


@pytest.mark.parametrize("shape", sorted(COLLISION_SHAPES))
def test_collision_builders(H, shape):
    p = COLLISION_SHAPES[shape]
    cols, ids = collision_case(p["n_tuples"], p["n_extra"])
    n = len(ids)
    a, b, _ = tuple_of_id(np.arange(p["n_tuples"]))
    assert len(np.unique(np.stack([a, b.astype(np.uint64)]), axis=1)[0]) == p["n_tuples"]  # the tuples are distinct
    key64 = H.cols_key64(cols, KEY_WIDTHS, p["hash_bits"])
    runs, longest, entries = run_shape(key64, ids)
    assert runs == 1 << p["hash_bits"] and 1 < longest <= RUN_CAP, (runs, longest)  # every run stays under kRunCap
    # at 256 compute units, and at any count up to 304 (the largest this project has met)
    for cus in (256, 304):
        if shape == "runs":
            assert entries > rows_past(cap_of("run_sort", cus), 1) and runs > cap_of("run_sort", cus)  # several led runs per workgroup
        else:
            assert entries > cap_rows("run_leader", cus) + 5 * 256 + 77  # the leader kernel strides
    # the join of the tuples with themselves: every run of its result holds as many tuples, so its list is as long at least
    assert p["n_tuples"] - runs > (cap_rows("run_leader", 256) if shape == "leader" else cap_of("run_sort", 304))
    if shape == "runs":
        exp = H.expected_groups(cols, KEY_WIDTHS, None, None, p["hash_bits"], ordered=True)
        assert exp["n_groups"] == p["n_tuples"] and exp["n_collisions"] == p["n_tuples"] - runs and exp["max_mixed_run"] == longest
        mixed = H.expected_mixed_groups(cols, None, None, p["hash_bits"], ordered=True)
        assert all(np.array_equal(exp[k], mixed[k]) for k in ("key64", "first_row", "count", "group_of_row"))
        # against a plain sort: ordered groups ascend by (key64, tuple), and first_row is the tuple's first row
        first = np.full(p["n_tuples"], n, np.int64)
        np.minimum.at(first, ids, np.arange(n))
        order = np.lexsort((b.astype(np.uint64), a, H.cols_key64([a, b], KEY_WIDTHS, p["hash_bits"])))
        assert np.array_equal(exp["first_row"], first[order].astype(np.uint64))
