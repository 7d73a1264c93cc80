"""Generators for the tours of the column operators on ONE long-lived context -- hmj_filter_device (WHERE), hmj_order_by_device
(ORDER BY), hmj_group_agg_device (aggregates) and hmj_group_mixed_device beside the entries the key tours already visit --
and their CPU-only checks (test_query_sequences_gpu.py runs the tours).  The method is test_ctx_sequences_cpu.py's: `draw_tour`,
`transitions`, `Model` and the flag constants come from there, the cases of the key joins from test_keyjoin_sequences_cpu.py.

  * `QueryPool`: the cases of one seed, drawn once on the host.  Eight tables of two or three key columns (string and
    fixed-width, the layouts of the key tours) and four value columns each over the ten HMJ_TYPE_* types, with bitmaps at bit
    offsets 0, 3 and 67; row counts from ROWS; groupings of 1, 2, 63, 64, 65 and 130 groups; one table whose grouping has a
    group of 70 * 512 + 11 rows (more than 64 walk waves); float columns either drawn over thirty binades (compared under
    gamma_k) or small and integer-valued (every order of summation is exact); two column and two mixed join cases; two small
    u64 cases and the one of PREPARE_ROWS rows a prepare goes to (uniform keys without a hot one: whether a join takes a
    prepared build side depends on its plan, and this shape's is taken);
  * an op names its inputs as plain values: a pool table, a side of a join case, or an output of an earlier op -- ["agg", j]
    and ["take", j] are relations (values with their validity bitmaps), ["filter", j], ["order", j], ["join", j, "r_row"] and
    ["group", j, "first_row"] are row maps, ["mask", j] is a filter's mask_out.  `expect_op` computes what an op must return
    from a store of such outputs: on the CPU the store holds the references' own outputs (`simulate`), on the GPU the host
    copies of what the device returned, so every stage is judged on its own inputs;
  * eleven op families and `draw_query_sequence`: 122 ops per tour, every ordered pair of families adjacent once, with the
    chains u64 (prepare) -> agg / filter / order -> u64 (the join of the prepared tensor), and one prepare with its join
    directly behind it as the chains' control;
  * `QueryModel(Model)`: what include/hmj.h promises between calls -- the prepared build side, the op whose join result and
    the op whose group columns must still be readable, the live grouping, and whether hmj_last_plan / hmj_last_timing must
    be what they were;
  * the comparison functions (numpy in, assertion out), one per entry, and a sensitivity check of each."""
import time

import numpy as np

from test_ctx_sequences_cpu import CHECKSUM, E_ARG, MATERIALIZE, ORDERED, SEQ_SEED, SEQ_TOURS, Model, draw_tour, transitions
from test_filter_cpu import BETWEEN, GE, GT, IS_NOT_NULL, IS_NULL, LE, LT, NE, STARTS_WITH
from test_group_agg_cpu import DTYPES, assert_aggs, gamma
from test_join_cols_kinds_cpu import BUILD, BUILD_OUTER, FULL_OUTER, INNER, NO_ROW, PROBE, PROBE_OUTER
from test_keyjoin_sequences_cpu import (BIT_OFFSETS, MIXED_LAYOUTS, PREPARE_ROWS, WORDS, KeyPool, draw_cols_case, draw_mixed_case, drawn_map,
                                        key_expectation, mixed_columns, mixed_masks)
from test_kinds_sweep_cpu import draw_u64_case
from test_take_cols_cpu import expected_take
from test_take_str_cpu import expected_take_str

AGG_COUNT, AGG_SUM, AGG_MIN, AGG_MAX, AGG_MEAN = range(5)  # HMJ_AGG_* (test_the_constants_are_the_bindings below)
ORDER_DESC, ORDER_NULLS_FIRST = 1, 2
GROUP_COUNT, GROUP_ROW_MAP = 0x1, 0x10
SENTINEL = -0x0123456789ABCDEF  # what the map buffer of a filter holds before the call
AGG_FILL = 0x5A                 # the byte an aggregate's outputs and their guard slots hold before the call

FAMILIES = ("u64", "key_join", "group_cols", "group_mixed", "agg", "order", "filter", "take_cols", "take_str", "config", "refused")
# each of the three new entries directly between a prepare and the join of the prepared tensor: the aggregate and the
# filter must leave the build side, ORDER BY must discard it
REQUIRED_CHAINS = (("u64", "agg", "u64"), ("u64", "filter", "u64"), ("u64", "order", "u64"))
ROWS = [1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513, 2047, 2048, 2049, 4097]
WAVE_GROUPS = (3, 70 * 512 + 11, 5)  # test_group_agg_gpu.test_groups_that_span_waves: one group over more than 64 walk waves
# (layout, fewest rows, groups, key columns with a bitmap) per table; a NULL is one of a column's values, so the groups are
# exactly as many as the distinct tuples drawn
TABLES = ((["s", 4], 2047, 130, (0,)), ([2, "s", 8], 511, 65, (1, 2)), (["s", "s"], 255, 64, ()), (["s"], 255, 63, (0,)),
          ([4, 4, 4], 2047, 1, ()), ([4, 4, 4], 1, 1, (1,)), (["s", 4], 2, 2, ()))
JOIN_KINDS = ((PROBE, INNER), (PROBE, PROBE_OUTER), (BUILD, BUILD_OUTER), (BUILD, FULL_OUTER))  # the kinds that leave both row maps
REFUSALS = ("agg_no_grouping", "agg_wrong_rows", "filter_map_beyond_source", "order_decreasing_offsets", "take_map_beyond_source",
            "group_flags")
HOST_FOUND = ("agg_no_grouping", "agg_wrong_rows")  # refused before any launch: hmj.h says everything is as it was
CONFIG = ("release", "profiling", "forget")
SEAMS = ("agg_bitmap_fed_filter", "agg_bitmap_fed_order", "filter_mask_fed_agg", "take_validity_fed_group", "map_fed_filter_term")
EMPTY_SHARE = CAP_SHARE = 10  # at most one filter op in ten with n_out == 0, one group / key-join op in ten beyond the run cap


class Redraw(Exception):
    """(a drawn tour that cannot be given ops: an aggregate in front of every grouping, for instance)"""


# ---- the pool -----------------------------------------------------------------------------------------------------------------------
def _column_values(rng, typ, v):
    """v distinct values of a key column: the extremes first; strings with the empty one, NUL and high bytes, a few of about
    100 bytes, a third behind one shared prefix of 21 bytes (ORDER BY then needs refinement rounds)."""
    if typ == "s":
        out = list(WORDS[:min(v, len(WORDS))])
        while len(out) < v:
            n = int(rng.integers(90, 130)) if rng.random() < 0.15 else int(rng.integers(1, 14))
            s = (b"a-long-shared-prefix/" if rng.random() < 0.3 else b"k") + rng.integers(0, 256, size=n, dtype=np.uint8).tobytes()
            if s not in out:
                out.append(s)
        return out
    top = (1 << (8 * typ)) - 1
    out = [0, top, 1, top - 1][:v]
    while len(out) < v:
        x = int(rng.integers(0, top, dtype=np.uint64))
        if x not in out:
            out.append(x)
    return out


def draw_value_column(rng, dtype, n, exact):
    """Integers over the whole range of the type; floats small and integer-valued (exact: any order of summation gives the
    same bits) or over thirty binades with mixed signs."""
    dt = np.dtype(dtype)
    if dt.kind == "f":
        a = rng.integers(-50, 51, size=n).astype(dt) if exact else (rng.standard_normal(n) * 2.0 ** rng.integers(-15, 15, size=n)).astype(dt)
    else:
        info = np.iinfo(dt)
        a = rng.integers(info.min, info.max, size=n, dtype=dt, endpoint=True)
    density = float(rng.choice([0.0, 0.1, 0.5]))
    return dict(a=a, valid=(rng.random(n) >= density) if density else None, off=int(rng.choice(BIT_OFFSETS)), exact=bool(exact or dt.kind != "f"))


def draw_table(rng, index, layout, n, card, bitmap):
    k = len(layout)
    v = 1
    while v ** k < card:
        v += 1
    vals = [_column_values(rng, typ, v + 1 if c in bitmap else v) for c, typ in enumerate(layout)]
    for c in bitmap:
        vals[c][int(rng.integers(0, len(vals[c])))] = None  # a NULL is one of the column's values
    tuples, t = [], 0
    while len(tuples) < card:
        row, stride = [], 1
        for col in vals:  # (mixed radix: distinct tuples for every t below the product of the columns' value counts)
            row.append(col[(t // stride) % len(col)])
            stride *= len(col)
        tuples.append(tuple(row))
        t += 1
    assert len(set(tuples)) == card
    idx = np.concatenate([np.arange(card), rng.integers(0, card, size=n - card)])[rng.permutation(n)]
    vcols = [draw_value_column(rng, DTYPES[(4 * index + j) % len(DTYPES)], n, (index + j) % 2 == 0) for j in range(4)]
    return dict(layout=list(layout), n=n, card=card, rows=[tuples[int(i)] for i in idx], bitmap=sorted(bitmap), off=int(rng.choice(BIT_OFFSETS)),
                vals=vcols)


def draw_wave_table(rng, index):
    """One uint64 key column whose grouping has the groups of WAVE_GROUPS: the combine step of the aggregate walks more than
    64 wave partials for the middle one."""
    keys = np.repeat(np.arange(len(WAVE_GROUPS), dtype=np.uint64) * np.uint64(1000003) + np.uint64(5), np.asarray(WAVE_GROUPS, np.int64))
    n = len(keys)
    keys = keys[rng.permutation(n)]
    vcols = [draw_value_column(rng, dt, n, ex) for dt, ex in (("int32", True), ("float64", False), ("float64", True), ("uint16", True))]
    return dict(layout=[8], n=n, card=len(WAVE_GROUPS), rows=[(int(x),) for x in keys], bitmap=[], off=0, vals=vcols)


class QueryPool(KeyPool):
    """The cases of one seed.  KeyPool's expectations of the key joins and its take sources are used as they are (over the
    cases drawn here); H: the hashmergejoin_amd module (host references)."""

    def __init__(self, seed, H):  # (KeyPool's own drawing is not wanted: no super().__init__)
        rng = np.random.default_rng([int(seed), 17])
        self.seed, self.H = int(seed), H
        self.mixed_sql = None
        self.groups, self.strs, self._cache = [], [], {}
        self.tables = []
        for i, (layout, least, card, bitmap) in enumerate(TABLES):
            n = int(rng.choice([r for r in ROWS if r >= max(least, card)])) if least > 2 else least
            self.tables.append(draw_table(rng, i, layout, n, card, bitmap))
        self.wave_table = len(self.tables)
        self.tables.append(draw_wave_table(rng, self.wave_table))
        size = lambda: int(rng.choice(ROWS[5:]))
        self.cols = [draw_cols_case(rng, [4, 4], size(), size(), 0, "some"), draw_cols_case(rng, [8, 4, 2], size(), size(), 0, "all")]
        self.mixed = [draw_mixed_case(rng, MIXED_LAYOUTS[0], size(), size(), 0, "all"), draw_mixed_case(rng, MIXED_LAYOUTS[1], size(), size(), 0, "all")]
        self.u64 = []
        for _ in range(2):
            B, P, fills, tag = draw_u64_case(rng, sizes=ROWS)
            self.u64.append(dict(B=B, P=P, fills=fills, tag=tag, rows=(len(B), len(P))))
        while True:  # uniform keys without a hot one: the shape of the *_keeps_a_prepared_build_side tests, which a join does take
            B, P, fills, tag = draw_u64_case(rng, sizes=[PREPARE_ROWS])
            if tag[2] == "uniform" and tag[5] == "none":
                break
        self.prepare_case = len(self.u64)
        self.u64.append(dict(B=B, P=P, fills=fills, tag=tag, rows=(len(B), len(P))))
        self._rels = {}

    def table_rel(self, ti):
        """A table as a relation: its key columns, then its value columns."""
        key = ("table", ti)
        if key not in self._rels:
            t = self.tables[ti]
            cols = [dict(a=a, valid=m, off=t["off"], exact=True) for a, m in zip(mixed_columns(t["layout"], t), mixed_masks(t["layout"], t))]
            self._rels[key] = dict(n=t["n"], cols=cols + t["vals"], keys=len(t["layout"]))
        return self._rels[key]

    def side_rel(self, fam, ci, side):
        """One side of a join case as a relation: its fixed-width columns (KeyPool.take_source)."""
        key = ("side", fam, ci, side)
        if key not in self._rels:
            (cols, masks, off), _ = self.take_source((fam, ci, side))
            masks = masks or [None] * len(cols)
            self._rels[key] = dict(n=len(cols[0]), cols=[dict(a=np.asarray(a), valid=m, off=off, exact=True) for a, m in zip(cols, masks)], keys=0)
        return self._rels[key]


# ---- inputs: relations, maps and masks by name ----------------------------------------------------------------------------------------
def resolve_rel(pool, store, ref):
    if ref[0] == "table":
        return pool.table_rel(ref[1])
    if ref[0] == "side":
        return pool.side_rel(ref[1], ref[2], ref[3])
    return store[ref[1]]["rel"]  # ["agg", j], ["take", j]


def resolve_map(pool, store, ref):
    if ref[0] == "drawn":
        return drawn_map(ref[1], ref[2], ref[3])
    if ref[0] in ("filter", "order"):
        return store[ref[1]]["map"]
    return store[ref[1]][ref[2]]  # ["join", j, "r_row" / "s_row"], ["group", j, "first_row"]


def is_string(col):
    return not isinstance(col["a"], np.ndarray)


def unpack_words(words, n):
    return np.unpackbits(np.ascontiguousarray(words).view(np.uint8), bitorder="little")[:n].astype(bool)


def literal(x):
    return bytes.fromhex(x) if isinstance(x, str) else x


def filter_terms(rel, op, row_map):
    """The terms of a filter op as H.expected_filter takes them (host values)."""
    out = []
    for c, code, lit, use_valid, clause, negate in op["terms"]:
        col = rel["cols"][c]
        lit = None if lit is None else ([literal(x) for x in lit] if isinstance(lit, list) else literal(lit))
        out.append(dict(column=col["a"], op=code, lit=tuple(lit) if isinstance(lit, list) else lit, valid=col["valid"] if use_valid else None,
                        bit_offset=0, row_map=row_map, clause=clause, negate=negate))
    return out


def order_columns(rel, op):
    return [(rel["cols"][c]["a"], flags, rel["cols"][c]["valid"] if use_valid else None) for c, flags, use_valid in op["cols"]]


def order_stats(H, columns, order):
    """(n_distinct, n_tied_rows) of an ORDER BY from the rule alone: rows are equal when in every column both slots are NULL
    or both are valid and of one value (floats: by bits, every NaN one value)."""
    n = len(order)
    if n == 0:
        return 0, 0
    idx = np.asarray(order).astype(np.int64)
    eq = np.ones(n, bool)
    eq[0] = False
    for vals, _flags, valid in columns:
        ok = np.ones(n, bool) if valid is None else np.asarray(valid, bool)[idx]
        if isinstance(vals, np.ndarray):
            bits = vals.view("u%d" % vals.dtype.itemsize).copy()
            if vals.dtype.kind == "f":
                bits[np.isnan(vals)] = ~bits.dtype.type(0)
            b = bits[idx]
            same = np.concatenate([[False], b[1:] == b[:-1]])
        else:
            v = [vals[i] for i in idx]
            same = np.array([False] + [v[j] == v[j - 1] for j in range(1, n)], bool)
        both_null = np.concatenate([[False], ~ok[1:] & ~ok[:-1]])
        both_ok = np.concatenate([[False], ok[1:] & ok[:-1]])
        eq &= both_null | (both_ok & same)
    tied = eq.copy()
    tied[:-1] |= eq[1:]
    return int(np.count_nonzero(~eq)), int(np.count_nonzero(tied))


def agg_inputs(pool, store, op, rel):
    """(op code, values or None, valid or None) per aggregate: a column's own bitmap, none, or the mask_out of a filter."""
    out = []
    for code, c, validity in op["aggs"]:
        col = None if c is None else rel["cols"][c]
        if validity == "own":
            valid = None if col is None else col["valid"]
        elif validity is None:
            valid = None
        else:
            valid = store[validity[1]]["mask"]
        out.append((code, None if col is None else col["a"], valid))
    return out


def group_keys(rel, op):
    cols = [rel["cols"][c] for c in op["cols"]]
    valid = [c["valid"] for c in cols]
    return [c["a"] for c in cols], (None if all(v is None for v in valid) else valid)


def expect_op(pool, store, op, binding=None):
    """What an op must return, from the outputs `store` holds of the ops it names: a dict in the form the store keeps
    (`simulate` puts it there as it is; the GPU file compares the device's outputs with it and stores those).  binding: the
    store entry of the live grouping's op (an aggregate's)."""
    H, what = pool.H, op["what"]
    if what == "filter":
        rel = resolve_rel(pool, store, op["rel"])
        m = None if op["map"] is None else resolve_map(pool, store, op["map"])
        n = rel["n"] if m is None else len(m)
        want, unknown = H.expected_filter(filter_terms(rel, op, m), n)
        mask = np.zeros(n, bool)
        mask[want.astype(np.int64)] = True
        return dict(map=want, n=n, n_unknown=unknown, mask=mask)
    if what == "order":
        rel = resolve_rel(pool, store, op["rel"])
        columns = order_columns(rel, op)
        want = H.expected_order_by(columns)
        distinct, tied = order_stats(H, columns, want)
        return dict(map=want, n=rel["n"], n_distinct=distinct, n_tied_rows=tied)
    if what == "take_cols":
        rel, m = resolve_rel(pool, store, op["rel"]), resolve_map(pool, store, op["map"])
        src = [rel["cols"][c] for c in op["cols"]]
        data, words, nulls, no_row = expected_take([c["a"] for c in src], [c["valid"] for c in src], m)
        cols = [dict(a=d, valid=unpack_words(w, len(m)), off=0, exact=c["exact"]) for d, w, c in zip(data, words, src)]
        return dict(rel=dict(n=len(m), cols=cols, keys=0), words=words, nulls=nulls, n_no_row=no_row)
    if what == "take_str":
        rel, m = resolve_rel(pool, store, op["rel"]), resolve_map(pool, store, op["map"])
        col = rel["cols"][op["col"]]
        off = np.zeros(rel["n"] + 1, np.int64)
        np.cumsum([len(k) for k in col["a"]], out=off[1:])
        chars, offsets, words, nulls, no_row, total = expected_take_str(b"".join(col["a"]), off, col["valid"], m)
        return dict(chars=chars, offsets=offsets, words=words, nulls=nulls, n_no_row=no_row, total=total)
    if what in ("group_cols", "group_mixed"):
        rel = resolve_rel(pool, store, op["rel"])
        cols, valid = group_keys(rel, op)
        ordered = bool(op["flags"] & ORDERED)
        if what == "group_mixed":
            e = H.expected_mixed_groups(cols, None, valid, 0, ordered)
        else:
            e = H.expected_groups(cols, [c.dtype.itemsize for c in cols], None, valid, 0, False, ordered)
        return dict(exp=e, n_rows=e["n_rows"], n_groups=e["n_groups"], first_row=e["first_row"], group_of_row=e["group_of_row"], count=e["count"],
                    rel=op["rel"])
    if what == "agg":
        rel = resolve_rel(pool, store, binding["rel"])
        aggs = agg_inputs(pool, store, op, rel)
        want = H.expected_group_aggs(binding["group_of_row"], binding["n_groups"], aggs)
        exact = [code in (AGG_COUNT, AGG_MIN, AGG_MAX) or c is None or rel["cols"][c]["exact"] for code, c, _ in op["aggs"]]
        cols = [dict(a=w["values"], valid=w["valid"], off=0, exact=e) for w, e in zip(want, exact)]
        return dict(rel=dict(n=binding["n_groups"], cols=cols, keys=0), want=want, aggs=aggs)
    if what == "key_join":
        e = key_expectation(pool, dict(op, what=op["kw"]))
        return dict(exp=e, n=len(e["rows"]), r_row=e["rows"][:, 1].copy(), s_row=e["rows"][:, 2].copy())
    if what == "u64" and op["sub"] == "join":
        return dict(exp=pool.expect_u64(op["case"]))
    if what == "u64" and op["sub"] == "sort":
        return dict(rows=pool.expect_sorted(op["case"], op["side"]))
    return None  # a prepare, config, refused: a status only


# ---- the contract of hmj.h -----------------------------------------------------------------------------------------------------------
class QueryModel(Model):
    """test_ctx_sequences_cpu.Model over the ops of these tours, from include/hmj.h and nothing else.  Beyond the prepared
    build side: `join_live`, the index of the op whose join result must still be readable; `group_live`, the op whose group
    columns must be; `binding`, the live grouping of hmj_group_agg_device (op, n_rows, n_groups) or None.  step() also says
    whether hmj_last_plan / hmj_last_timing must be what they were before the op ("plan_kept").  Where hmj.h promises
    nothing (a result after a configuration call, everything but the binding after a device-found error) the model stops
    claiming: join_live / group_live become None, and a prepared build side MAY still be taken."""

    def __init__(self):
        super().__init__()
        self.join_live = self.group_live = self.binding = None
        self.index = -1

    def step(self, op):
        self.index += 1
        what = op["what"]
        res = {"rc": 0, "may_prepared": False, "forced": None, "plan_kept": False}
        if what in ("take_cols", "take_str", "agg", "filter"):
            res["plan_kept"] = True  # the takes' rules: everything stays
        elif what == "order":
            res["plan_kept"] = True  # the group result and the live grouping are kept for every n
            if op["n"] >= 1:
                self._discard()
            if op["n"] >= 2:  # the sort ran: the lifetime of the last JOIN result ends
                self.join_live = None
        elif what in ("group_cols", "group_mixed"):
            self._discard()
            self.join_live = self.group_live = self.binding = None  # the binding ends at the entry of every group call
            res["plan_kept"] = True
            if op["flags"] & (MATERIALIZE | ORDERED):
                self.group_live = self.index
                self.binding = {"op": self.index, "n_rows": op["n_rows"], "n_groups": op["n_groups"]}
        elif what == "key_join":
            self._discard()
            self.join_live, self.group_live = self.index, None
        elif what == "u64":
            self.join_live = self.group_live = None
            if op["sub"] == "join":
                res["may_prepared"] = self.prepared is not None and self.prepared == op["case"]
                if not res["may_prepared"]:
                    self._discard()
                self.prepared = None
            else:
                self._discard()
                if op["sub"] == "prepare":
                    self.prepared = op["case"]
        elif what == "config":
            self.join_live = self.group_live = None
            if op["action"] == "release":
                self.binding = None
        elif what == "refused":
            res["rc"] = E_ARG
            if op["which"] in HOST_FOUND:
                res["plan_kept"] = True
            else:
                self.join_live = self.group_live = None
                if op["which"] == "group_flags":  # a group call ends the binding whether it succeeds or not
                    self.binding = None
        else:
            raise ValueError(what)
        res.update(join_live=self.join_live, group_live=self.group_live, binding=self.binding)
        return res


# ---- drawing a tour ------------------------------------------------------------------------------------------------------------------
def _numeric(rel):
    return [c for c, col in enumerate(rel["cols"]) if not is_string(col)]


def _draw_terms(rng, rel, cols, n_terms):
    """n_terms terms over the given columns of a relation, literals taken from the columns' own values."""
    terms = []
    for k in range(n_terms):
        c = int(cols[int(rng.integers(0, len(cols)))])
        col = rel["cols"][c]
        pick = lambda: col["a"][int(rng.integers(0, rel["n"]))] if rel["n"] else (b"" if is_string(col) else 0)
        if is_string(col):
            code = int(rng.choice([GE, LT, NE, STARTS_WITH, IS_NULL, IS_NOT_NULL]))
            lit = None if code in (IS_NULL, IS_NOT_NULL) else bytes(pick())[:3 if code == STARTS_WITH else None].hex()
        else:
            code = int(rng.choice([GE, LT, LE, GT, NE, BETWEEN, IS_NULL, IS_NOT_NULL]))
            plain = lambda x: float(x) if col["a"].dtype.kind == "f" else int(x)
            if code == BETWEEN:
                lit = sorted([plain(pick()), plain(pick())])
            else:
                lit = None if code in (IS_NULL, IS_NOT_NULL) else plain(pick())
        terms.append([c, code, lit, bool(col["valid"] is not None and rng.random() < 0.8), min(k, int(rng.integers(0, 2))), bool(rng.random() < 0.15)])
    terms.sort(key=lambda t: t[4])  # clause ids never decrease
    return terms


def draw_query_sequence(rng, pool, families=FAMILIES, required=REQUIRED_CHAINS):
    """One tour of ops (dicts of plain values) with the sizes the model needs ("n" of an ORDER BY, "n_rows" / "n_groups" of a
    group op), from a run of the references over the drawn ops.  Drawn again until every seam of SEAMS and every refusal
    occurs, an aggregate meets a live grouping wherever the family stands, and the two caps hold."""
    for _ in range(200):
        try:
            ops, store, said = _draw_once(rng, pool, families, required)
        except Redraw:
            continue
        facts = tour_facts(pool, ops, (store, said))
        if (all(facts["seams"][s] for s in SEAMS if set(families) == set(FAMILIES)) and facts["empty_filters"] * EMPTY_SHARE <= facts["filters"]
                and facts["refusals"] >= set(REFUSALS) and facts["wave_after_smaller"] and facts["tables"] == set(range(len(pool.tables)))
                and (facts["control"] or "u64" not in families)):
            return ops
    raise AssertionError("no tour in 200 draws")


def _draw_once(rng, pool, families, required):
    required = tuple(ch for ch in required if set(ch) <= set(families))
    starts = lambda tour, pos: any(tuple(tour[pos:pos + len(ch)]) == ch for ch in required)
    ends = lambda tour, pos: any(pos >= len(ch) - 1 and tuple(tour[pos - len(ch) + 1:pos + 1]) == ch for ch in required)
    group_fams = ("group_cols", "group_mixed")
    while True:  # (no u64 op can be the join that ends one chain and the prepare that starts another)
        tour = draw_tour(rng, families, required)
        # the circuit is closed: turned so that it begins with a group call it holds the same transitions, and no aggregate
        # stands in front of every grouping
        k = next((i for i, f in enumerate(tour) if f in group_fams), 0)
        tour = tour[k:-1] + tour[:k] + [tour[k]]
        joined = "|" + "|".join(tour) + "|"
        pair = next((i for i in range(len(tour) - 1) if tour[i] == tour[i + 1] == "u64"), None)  # the control: a prepare and its join
        if all("|" + "|".join(ch) + "|" in joined for ch in required) and not any(ends(tour, pos) and starts(tour, pos) for pos in range(len(tour))) \
                and (pair is None or not (ends(tour, pair) or starts(tour, pair + 1))):
            break
    # an aggregate stands behind `pos` before any group call does: nothing may end the live grouping there
    agg_ahead = lambda pos: next((f == "agg" for f in tour[pos + 1:] if f == "agg" or f in group_fams), False)
    model, store, ops, said = QueryModel(), {}, [], []
    refusals =[REFUSALS[i] for i in rng.permutation(len(REFUSALS))]
    state = {"prep": None, "agg_tables": set(), "aggs": 0, "joins": [], "u64": 0}
    tables = range(len(pool.tables))
    has_str = lambda ti: "s" in pool.tables[ti]["layout"]
    unused = [int(i) for i in rng.permutation(len(pool.tables))]

    def pick_table(ok=lambda ti: True):
        for ti in unused:
            if ok(ti):
                unused.remove(ti)
                return ti
        cand = [ti for ti in tables if ok(ti)]
        return int(cand[int(rng.integers(0, len(cand)))])

    def binding_entry():
        return None if model.binding is None else store[model.binding["op"]]

    for pos, fam in enumerate(tour):
        prev = ops[-1] if ops else None
        nxt = tour[pos + 1] if pos + 1 < len(tour) else None
        bound = binding_entry()
        if fam == "u64":
            # the prepare of a chain -- and, as the control of the chains, one with its join directly behind it
            if starts(tour, pos) or (nxt == "u64" and state["prep"] is None and not ends(tour, pos + 1) and not starts(tour, pos + 1)):
                op = dict(what=fam, sub="prepare", case=pool.prepare_case, hint=int(pool.u64[pool.prepare_case]["rows"][1]))
            elif state["prep"] is not None:
                op = dict(what=fam, sub="join", case=state["prep"], flags=0)
            else:
                sub = str(rng.choice(["join", "join", "sort"]))
                state["u64"] = (state["u64"] + 1) % pool.prepare_case  # the small cases in turn
                op = dict(what=fam, sub=sub, case=state["u64"])
                if sub == "join":
                    op["flags"] = int(rng.choice([0, CHECKSUM, MATERIALIZE | CHECKSUM, ORDERED | CHECKSUM]))
                else:
                    op.update(side=int(rng.integers(0, 2)), inplace=bool(rng.integers(0, 2)))
            state["prep"] = op["case"] if op["sub"] == "prepare" else None
        elif fam == "key_join":
            if not state["joins"]:  # every join case once before any comes again
                state["joins"] = [("cols_kind", 0), ("cols_kind", 1), ("mixed", 0), ("mixed", 1)]
            kw, ci = state["joins"].pop(int(rng.integers(0, len(state["joins"]))))
            side, kind = JOIN_KINDS[3] if rng.random() < 0.5 else JOIN_KINDS[int(rng.integers(0, 4))]
            sem = "ne" if kw == "mixed" else str(rng.choice(["plain", "sql", "ne"]))
            op = dict(what=fam, kw=kw, case=ci, side=int(side), kind=int(kind), sem=sem, force=False,
                      flags=int(rng.choice([MATERIALIZE | CHECKSUM, ORDERED | CHECKSUM])))
            op["over"] = bool(key_expectation(pool, dict(op, what=kw))["over"])
            if op["over"]:  # (64 hash bits: it takes a genuine collision) -- the unordered mode of the same case is exact
                op["flags"] = MATERIALIZE | CHECKSUM
        elif fam in ("group_cols", "group_mixed"):
            if prev is not None and prev["what"] == "take_cols":  # the take's output validity is the keys' validity
                rel_ref = ["take", pos - 1]
                cols = list(range(min(3, len(store[pos - 1]["rel"]["cols"]))))
            else:
                wave = agg_ahead(pos) and state["aggs"] > 0 and pool.wave_table not in state["agg_tables"]
                ti = pool.wave_table if wave else pick_table(lambda ti: fam == "group_mixed" or not has_str(ti))
                rel_ref, cols = ["table", ti], list(range(len(pool.tables[ti]["layout"])))
            count_only = not agg_ahead(pos) and rng.random() < 0.25
            op = dict(what=fam, rel=rel_ref, cols=cols, flags=0 if count_only else int(rng.choice([MATERIALIZE, ORDERED])),
                      want=int(rng.integers(0, 0x20)) | GROUP_COUNT | GROUP_ROW_MAP)
        elif fam == "agg":
            if bound is None:
                raise Redraw()
            rel = resolve_rel(pool, store, bound["rel"])
            num = _numeric(rel)
            vals = [c for c in num if c >= rel["keys"]] or num
            mask = ["mask", pos - 1] if prev["what"] == "filter" and prev["want_mask"] and store[pos - 1]["n"] == bound["n_rows"] \
                and prev["map"] is None else None
            aggs = []
            for k in range(int(rng.integers(1, 6))):
                code = int(rng.integers(0, 5))
                c = None if code == AGG_COUNT and rng.random() < 0.5 else int(vals[int(rng.integers(0, len(vals)))])
                aggs.append([code, c, mask if (mask is not None and k == 0) else ("own" if rng.random() < 0.8 else None)])
            if nxt in ("filter", "order") and not any(expect_exact(rel, a) for a in aggs):
                exact = [c for c in vals if rel["cols"][c]["exact"]]
                aggs.append([AGG_SUM, int(exact[int(rng.integers(0, len(exact)))]), "own"])
            op = dict(what=fam, aggs=aggs)
            state["aggs"] += 1
            if bound["rel"][0] == "table":
                state["agg_tables"].add(bound["rel"][1])
        elif fam == "order":
            if prev is not None and prev["what"] == "agg":  # the aggregate's bitmap is the column's validity
                rel_ref = ["agg", pos - 1]
                rel = store[pos - 1]["rel"]
                first = next(c for c, col in enumerate(rel["cols"]) if col["exact"])
                cols = [first] + [int(c) for c in rng.permutation(len(rel["cols"]))[:2] if c != first]
            else:
                chain = prev is not None and prev["what"] == "u64" and prev["sub"] == "prepare"
                ti = pick_table(lambda ti: not chain or pool.tables[ti]["n"] >= 2)
                rel_ref, rel = ["table", ti], pool.table_rel(ti)
                cols = [int(c) for c in rng.permutation(len(rel["cols"]))[:int(rng.integers(1, 4))]]
            op = dict(what=fam, rel=rel_ref, n=rel["n"],
                      cols=[[c, int(rng.integers(0, 4)), bool(rel["cols"][c]["valid"] is not None and rng.random() < 0.9)] for c in cols])
        elif fam == "filter":
            m = None
            if nxt == "agg" and bound is not None:  # over the grouped relation: its mask_out is a value column's validity there
                rel_ref = bound["rel"]
                rel = resolve_rel(pool, store, rel_ref)
                terms = _draw_terms(rng, rel, list(range(len(rel["cols"]))), int(rng.integers(1, 4)))
            elif prev is not None and prev["what"] == "agg":  # HAVING: the aggregate's bitmap is the term's validity
                rel_ref, rel = ["agg", pos - 1], store[pos - 1]["rel"]
                c = next(c for c, col in enumerate(rel["cols"]) if col["exact"])
                terms = _draw_terms(rng, rel, [c], 1)
                terms[0][3] = True
                if terms[0][1] in (IS_NULL, IS_NOT_NULL):
                    terms[0][1:3] = [GE, 0]
            elif prev is not None and prev["what"] in ("filter", "order") and prev["rel"][0] != "agg" and prev.get("map") is None:
                # through the earlier op's map (an earlier filter that read through a map itself selected positions of that map)
                rel_ref, rel, m = prev["rel"], resolve_rel(pool, store, prev["rel"]), [prev["what"], pos - 1]
                terms = _draw_terms(rng, rel, list(range(len(rel["cols"]))), int(rng.integers(1, 4)))
            elif prev is not None and prev["what"] == "key_join":  # WHERE s.key IS NULL OR r.v > x, through the result's own maps
                rel_ref, rel, m = ["side", {"cols_kind": "cols", "mixed": "mixed"}[prev["kw"]], prev["case"], 0], None, ["join", pos - 1, "r_row"]
                rel = resolve_rel(pool, store, rel_ref)
                terms = _draw_terms(rng, rel, _numeric(rel), 2)
                terms[0][1:3] = [IS_NULL, None]
                for t in terms:
                    t[4] = 0
            else:
                rel_ref = ["table", pick_table()]
                rel = resolve_rel(pool, store, rel_ref)
                terms = _draw_terms(rng, rel, list(range(len(rel["cols"]))), int(rng.integers(1, 4)))
            op = dict(what=fam, rel=rel_ref, terms=terms, map=m, want_mask=bool(nxt in ("agg", "take_cols") or rng.random() < 0.5))
        elif fam == "take_cols":
            if prev is not None and prev["what"] in ("filter", "order"):
                rel_ref, m = prev["rel"], [prev["what"], pos - 1]
                if prev["what"] == "filter" and prev["map"] is not None:  # positions of that map, not rows of the relation
                    rel_ref, m = prev["rel"], ["drawn", pool.seed + pos, resolve_rel(pool, store, prev["rel"])["n"], int(rng.choice(ROWS))]
            elif prev is not None and prev["what"] == "key_join":
                side = int(rng.integers(0, 2))
                rel_ref = ["side", {"cols_kind": "cols", "mixed": "mixed"}[prev["kw"]], prev["case"], side]
                m = ["join", pos - 1, "r_row" if side == 0 else "s_row"]
            elif prev is not None and prev["what"] in ("group_cols", "group_mixed") and prev["flags"]:
                rel_ref, m = prev["rel"], ["group", pos - 1, "first_row"]  # the DISTINCT table
            else:
                ti = pick_table()
                rel_ref, m = ["table", ti], ["drawn", pool.seed + pos, pool.tables[ti]["n"], int(rng.choice(ROWS))]
            rel = resolve_rel(pool, store, rel_ref)
            num = _numeric(rel)
            op = dict(what=fam, rel=rel_ref, map=m, cols=[int(c) for c in rng.permutation(num)[:4]])
        elif fam == "take_str":
            if prev is not None and prev["what"] in ("filter", "order") and prev["rel"][0] == "table" and has_str(prev["rel"][1]) \
                    and not (prev["what"] == "filter" and prev["map"] is not None):
                rel_ref, m = prev["rel"], [prev["what"], pos - 1]
            else:
                ti = pick_table(has_str)
                rel_ref, m = ["table", ti], ["drawn", pool.seed + pos, pool.tables[ti]["n"], int(rng.choice(ROWS))]
            op = dict(what=fam, rel=rel_ref, map=m, col=pool.tables[rel_ref[1]]["layout"].index("s"))
        elif fam == "config":
            may_release = not agg_ahead(pos)
            action = "release" if nxt == "refused" and may_release else str(rng.choice([a for a in CONFIG if may_release or a != "release"]))
            op = dict(what=fam, action=action, value=bool(rng.integers(0, 2)) if action == "profiling" else None)
        elif fam == "refused":
            ok = lambda w: not ((w == "agg_no_grouping" and bound is not None) or (w == "agg_wrong_rows" and bound is None)
                                or (w == "group_flags" and agg_ahead(pos)))
            which = next((w for w in refusals if ok(w)), None)
            if which is None:
                raise Redraw()
            refusals.remove(which)
            refusals.append(which)
            op = dict(what=fam, which=which)
        else:
            raise ValueError(fam)
        op["fam"] = fam
        out = expect_op(pool, store, op, bound)
        if fam in ("group_cols", "group_mixed"):
            op.update(n_rows=int(out["n_rows"]), n_groups=int(out["n_groups"]))
        if fam == "filter":  # a selection of nothing shows little: other terms, a few times, before one is kept
            for _ in range(6):
                if len(out["map"]) or out["n"] == 0 or op["rel"][0] == "side":
                    break
                rel = resolve_rel(pool, store, op["rel"])
                cols = [op["terms"][0][0]] if op["rel"][0] == "agg" else list(range(len(rel["cols"])))
                op["terms"] = _draw_terms(rng, rel, cols, len(op["terms"]))
                if op["rel"][0] == "agg":
                    op["terms"][0][1:4] = [GE, op["terms"][0][2] if op["terms"][0][1] not in (IS_NULL, IS_NOT_NULL, BETWEEN) else 0, True]
                out = expect_op(pool, store, op, bound)
        said.append(model.step(op))
        if out is not None:
            store[pos] = out
        ops.append(op)
    return ops, store, said


def expect_exact(rel, agg):
    code, c, _ = agg
    return code in (AGG_COUNT, AGG_MIN, AGG_MAX) or c is None or rel["cols"][c]["exact"]


def simulate(pool, ops):
    """The references over a tour: (the store of every op's expected outputs, what the model said per op)."""
    model, store, said = QueryModel(), {}, []
    for i, op in enumerate(ops):
        bound = None if model.binding is None else store[model.binding["op"]]
        out = expect_op(pool, store, op, bound)
        said.append(model.step(op))
        if out is not None:
            store[i] = out
    return store, said


def tour_facts(pool, ops, sim=None):
    """Properties of a drawn tour, from the ops and the references alone: which seams it feeds, how many filters it runs and
    how many of them select nothing, the refusals and tables it uses, and whether the grouping of the wave table is
    aggregated after a smaller one.  sim: simulate()'s pair when the caller has it."""
    store, said = sim or simulate(pool, ops)
    seams = dict.fromkeys(SEAMS, 0)
    filters = empty = 0
    used, agg_rows, wave_after_smaller = set(), [], False
    for i, (op, want) in enumerate(zip(ops, said)):
        what = op["what"]
        if "rel" in op and op["rel"][0] == "table":
            used.add(op["rel"][1])
        if what == "filter":
            filters += 1
            empty += len(store[i]["map"]) == 0
            seams["agg_bitmap_fed_filter"] += op["rel"][0] == "agg" and any(t[3] for t in op["terms"])
            seams["map_fed_filter_term"] += op["map"] is not None and op["map"][0] in ("filter", "order")
        elif what == "order":
            seams["agg_bitmap_fed_order"] += op["rel"][0] == "agg" and any(c[2] for c in op["cols"])
        elif what == "agg":
            seams["filter_mask_fed_agg"] += any(isinstance(a[2], list) for a in op["aggs"])
            n = want["binding"]["n_rows"]
            wave_after_smaller |= n == sum(WAVE_GROUPS) and any(r < n for r in agg_rows)
            agg_rows.append(n)
        elif what in ("group_cols", "group_mixed"):
            seams["take_validity_fed_group"] += op["rel"][0] == "take"
    control = any(a["what"] == b["what"] == "u64" and a["sub"] == "prepare" and b["sub"] == "join" for a, b in zip(ops, ops[1:]))
    return dict(seams=seams, filters=filters, empty_filters=empty, control=control, refusals={op["which"] for op in ops if op["what"] == "refused"},
                tables=used, wave_after_smaller=wave_after_smaller, store=store, said=said)


# ---- the comparison functions: numpy in, assertion out -----------------------------------------------------------------------------------
def compare_filter(buf, words, info, want, tag=""):
    """buf: the whole map buffer as int64, at least n + 1 entries that held SENTINEL before the call; words: mask_out as
    uint64 words or None; info: n_out / n_unknown; want: expect_op's dict."""
    n, wmap = want["n"], want["map"]
    assert info["n_out"] == len(wmap) and info["n_unknown"] == want["n_unknown"], (tag, info, len(wmap), want["n_unknown"])
    got = np.asarray(buf[:len(wmap)]).view(np.uint64)
    if not np.array_equal(got, wmap):
        bad = int(np.nonzero(got != wmap)[0][0])
        raise AssertionError("%s: the map differs from entry %d on: got %d, want %d" % (tag, bad, got[bad], wmap[bad]))
    tail = np.asarray(buf[len(wmap):])
    assert len(tail) >= 1 and np.all(tail == SENTINEL), (tag, "an entry at or behind n_out was written", int(np.nonzero(tail != SENTINEL)[0][0]))
    if words is not None:
        assert len(words) == (n + 63) // 64, tag
        bits = np.unpackbits(np.ascontiguousarray(words).view(np.uint8), bitorder="little")
        exp = np.zeros(64 * len(words), np.uint8)
        exp[:n] = want["mask"]
        assert np.array_equal(bits, exp), (tag, "mask_out differs from the map, or its padding bits are not 0")


def compare_order(got, info, want, tag=""):
    got = np.asarray(got).view(np.uint64)
    assert got.shape == want["map"].shape, (tag, got.shape)
    if not np.array_equal(got, want["map"]):
        bad = int(np.nonzero(got != want["map"])[0][0])
        raise AssertionError("%s: the map differs from position %d on: got row %d, want row %d" % (tag, bad, got[bad], want["map"][bad]))
    assert (info["n_distinct"], info["n_tied_rows"]) == (want["n_distinct"], want["n_tied_rows"]), (tag, info, want["n_distinct"], want["n_tied_rows"])


def compare_agg(H, got, want, tag=""):
    """got: per aggregate (values with one guard slot behind n_groups, bitmap words with one guard word or None,
    null_count), every byte AGG_FILL before the call; want: expect_op's dict."""
    ng = want["rel"]["n"]
    n_words = (ng + 63) // 64
    trimmed = []
    for k, (v, w, nulls) in enumerate(got):
        assert len(v) == ng + 1 and np.all(v[ng:].view(np.uint8) == AGG_FILL), (tag, k, "a slot behind n_groups was written")
        ok = None
        if w is not None:
            w = np.asarray(w).view(np.uint64)
            assert len(w) == n_words + 1 and int(w[n_words]) == int.from_bytes(bytes([AGG_FILL]) * 8, "little"), (tag, k, "a word behind the bitmap")
            if ng % 64:
                assert int(w[n_words - 1]) >> (ng % 64) == 0, (tag, k, "padding bits must be 0")
            ok = unpack_words(w[:n_words], ng)
            assert nulls == ng - int(np.count_nonzero(ok)), (tag, k, "null_count and the bitmap disagree", nulls)
        assert nulls == want["want"][k]["null_count"], (tag, k, nulls, want["want"][k]["null_count"])
        null_slots = ~want["want"][k]["valid"]
        assert not np.any(v[:ng][null_slots].view(np.uint8)), (tag, k, "the value bytes of a NULL slot are not 0")
        trimmed.append((v[:ng], ok, nulls))
    assert_aggs(H, trimmed, want["want"], want["aggs"], ng, tag)


def compare_take_cols(outs, words, info, want, tag=""):
    for c, (o, w) in enumerate(zip(outs, words)):
        d = want["rel"]["cols"][c]["a"]
        assert o.shape == d.shape and np.array_equal(np.ascontiguousarray(o).reshape(-1).view(np.uint8), np.ascontiguousarray(d).reshape(-1).view(np.uint8)), (tag, c)
        assert np.array_equal(np.asarray(w).view(np.uint64), want["words"][c]), (tag, c, "validity words (padding bits included)")
    assert info["null_count"] == want["nulls"] and info["n_no_row"] == want["n_no_row"], (tag, info, want["nulls"], want["n_no_row"])


def compare_take_str(chars, offsets, words, info, want, tag=""):
    assert np.array_equal(np.asarray(offsets).view(np.uint64), want["offsets"]), (tag, "offsets")
    assert np.array_equal(np.asarray(chars), want["chars"]), (tag, "chars")
    assert np.array_equal(np.asarray(words).view(np.uint64), want["words"]), (tag, "validity words (padding bits included)")
    assert (info["null_count"], info["n_no_row"], info["total_bytes"]) == (want["nulls"], want["n_no_row"], want["total"]), (tag, info)


# ---------------------------------------------------------------------------------------------------------------------------------------
SEEDS = (SEQ_SEED, 7, 11)
_pools, _tours = {}, {}


def pool_of(seed):
    import hashmergejoin_amd as H

    if seed not in _pools:
        _pools[seed] = QueryPool(seed, H)
    return _pools[seed]


def tours_of(seed):
    """The pool and the default number of tours of a seed, as test_query_sequences_gpu.py draws them."""
    pool = pool_of(seed)
    if seed not in _tours:
        rng = np.random.default_rng([int(seed), 19])
        _tours[seed] = [draw_query_sequence(rng, pool) for _ in range(SEQ_TOURS)]
    return pool, _tours[seed]


def test_the_constants_are_the_bindings():
    import hashmergejoin_amd as H

    assert (AGG_COUNT, AGG_SUM, AGG_MIN, AGG_MAX, AGG_MEAN) == (H.HMJ_AGG_COUNT, H.HMJ_AGG_SUM, H.HMJ_AGG_MIN, H.HMJ_AGG_MAX, H.HMJ_AGG_MEAN)
    assert (ORDER_DESC, ORDER_NULLS_FIRST) == (H.HMJ_ORDER_DESC, H.HMJ_ORDER_NULLS_FIRST)
    assert (GROUP_COUNT, GROUP_ROW_MAP) == (H.HMJ_GROUP_COUNT, H.HMJ_GROUP_ROW_MAP) and NO_ROW == H.HMJ_TAKE_NO_ROW
    assert [getattr(H, "HMJ_FILTER_" + n) for n in ("GE", "GT", "LE", "LT", "NE", "BETWEEN", "IS_NULL", "IS_NOT_NULL", "STARTS_WITH")] == \
        [GE, GT, LE, LT, NE, BETWEEN, IS_NULL, IS_NOT_NULL, STARTS_WITH]
    assert [getattr(H, "HMJ_TYPE_" + n) for n in ("I8", "I16", "I32", "I64", "U8", "U16", "U32", "U64", "F32", "F64")] == list(range(10))
    assert len(DTYPES) == 10


def test_every_tour_holds_every_transition_chain_family_case_and_seam():
    for seed in SEEDS:
        pool, tours = tours_of(seed)
        for ops in tours:
            fams = [op["fam"] for op in ops]
            F = len(FAMILIES)
            assert F == 11 and len(ops) == F * F + 1 == 122
            assert transitions(fams) == {(x, y) for x in FAMILIES for y in FAMILIES}, seed
            assert set(fams) == set(FAMILIES)
            for ch in REQUIRED_CHAINS:
                at = [i for i in range(len(fams) - 2) if tuple(fams[i:i + 3]) == ch]
                assert at, (seed, ch)
                a, mid, b = ops[at[0]:at[0] + 3]
                assert a["sub"] == "prepare" and b["sub"] == "join" and b["case"] == a["case"] == pool.prepare_case and b["flags"] == 0, (seed, ch)
                assert mid["what"] != "order" or mid["n"] >= 2, (seed, "the ORDER BY of the chain must run its sort")
            facts = tour_facts(pool, ops)
            assert all(facts["seams"][s] for s in SEAMS), (seed, facts["seams"])
            assert facts["refusals"] == set(REFUSALS) and facts["control"], seed
            assert facts["tables"] == set(range(len(pool.tables))) and facts["wave_after_smaller"], seed
            assert {op["case"] for op in ops if op["what"] == "u64"} == set(range(len(pool.u64))), seed
            assert {(op["kw"], op["case"]) for op in ops if op["what"] == "key_join"} == {(k, c) for k in ("cols_kind", "mixed") for c in (0, 1)}, seed
            # the two caps: a tour cannot hide a failure behind empty selections or refused calls
            assert facts["empty_filters"] * EMPTY_SHARE <= facts["filters"], (seed, facts["empty_filters"], facts["filters"])
            capped = sum(bool(op.get("over") and op["flags"] & ORDERED) for op in ops if op["what"] == "key_join")
            capped += sum(store_e["exp"]["max_mixed_run"] > 1024 for i, store_e in facts["store"].items() if ops[i]["what"] in ("group_cols", "group_mixed"))
            n_key = sum(op["what"] in ("key_join", "group_cols", "group_mixed") for op in ops)
            assert capped * CAP_SHARE <= n_key and capped == 0, (seed, capped)
            # a filter term through a join's own maps only while the model says the result is alive
            for i, op in enumerate(ops):
                for ref in (op.get("map"),):
                    if ref is not None and ref[0] == "join":
                        assert facts["said"][i]["join_live"] == ref[1], (seed, i, op)
                    if ref is not None and ref[0] == "group":
                        assert facts["said"][i]["group_live"] == ref[1], (seed, i, op)


def test_every_op_but_config_and_refused_has_an_output_expectation():
    for seed in SEEDS:
        pool, tours = tours_of(seed)
        for ops in tours:
            store, said = simulate(pool, ops)
            for i, (op, want) in enumerate(zip(ops, said)):
                what = op["what"]
                if what in ("config", "refused"):
                    assert i not in store and (want["rc"] == 0) == (what == "config"), op
                    continue
                assert want["rc"] == 0, op
                if what == "u64" and op["sub"] == "prepare":
                    continue  # (its expectation is the join that follows: HMJ_PATH_PREPARED where the model allows it)
                out = store[i]
                if what == "agg":
                    assert want["binding"] is not None and out["rel"]["n"] == want["binding"]["n_groups"] and len(out["want"]) == len(op["aggs"]), op
                    for (code, vals, valid), (_, c, _) in zip(out["aggs"], op["aggs"]):
                        assert (vals is None or len(vals) == want["binding"]["n_rows"]) and (valid is None or len(valid) == want["binding"]["n_rows"]), op
                elif what in ("filter", "order"):
                    assert len(out["map"]) <= out["n"] and (what == "filter" or len(out["map"]) == op["n"]), op
                elif what in ("group_cols", "group_mixed"):
                    assert (out["n_rows"], out["n_groups"]) == (op["n_rows"], op["n_groups"]) and out["exp"]["max_mixed_run"] <= 1024, op
                elif what == "key_join":
                    assert out["n"] == len(out["r_row"]) == len(out["s_row"]) and "counts" in out["exp"], op
                elif what == "take_cols":
                    assert len(out["rel"]["cols"]) == len(op["cols"]) >= 1, op
                elif what == "take_str":
                    assert len(out["offsets"]) == len(resolve_map(pool, store, op["map"])) + 1, op
                else:
                    assert what == "u64" and ("exp" in out or "rows" in out), op


def test_pool_cases_are_bounded():
    for seed in SEEDS:
        pool = pool_of(seed)
        groups, types, offs = set(), set(), set()
        for ti, t in enumerate(pool.tables):
            assert (t["n"] in ROWS and t["n"] <= 4097) or ti == pool.wave_table, (ti, t["n"])
            rel = pool.table_rel(ti)
            cols, valid = group_keys(rel, dict(cols=list(range(rel["keys"]))))
            e = pool.H.expected_mixed_groups(cols, None, valid, 0, True)
            assert e["n_groups"] == t["card"] and e["max_mixed_run"] == 0, (seed, ti, e["n_groups"])
            groups.add(e["n_groups"])
            for v in t["vals"]:
                types.add(str(v["a"].dtype))
                offs.add(v["off"] if v["valid"] is not None else None)
                assert len(v["a"]) == t["n"]
        assert groups >= {1, 2, 3, 63, 64, 65, 130}, (seed, groups)
        assert types == set(DTYPES), (seed, types)
        assert offs - {None} == set(BIT_OFFSETS), (seed, offs)
        wave = pool.tables[pool.wave_table]
        assert wave["n"] == sum(WAVE_GROUPS) and max(WAVE_GROUPS) > 64 * 512
        assert {tuple(t["layout"]) for t in pool.tables} >= {tuple(x) for x in MIXED_LAYOUTS}
        floats = [v["exact"] for t in pool.tables for v in t["vals"] if v["a"].dtype.kind == "f"]
        assert True in floats and False in floats  # integer-valued ones and ones drawn over many binades
        assert pool.u64[pool.prepare_case]["rows"][0] == PREPARE_ROWS and all(max(c["rows"]) <= 4097 for c in pool.u64[:pool.prepare_case])
        assert all(max(c["rows"]) <= 4097 for c in pool.cols + pool.mixed)


def test_the_model_follows_the_written_contract():
    """One hand-written sequence per sentence of include/hmj.h about what stays between calls."""
    prep, join = dict(what="u64", sub="prepare", case=2), dict(what="u64", sub="join", case=2, flags=0)
    group = dict(what="group_cols", flags=MATERIALIZE, n_rows=100, n_groups=7)
    kj = dict(what="key_join")
    agg, flt, tk, ts = dict(what="agg"), dict(what="filter"), dict(what="take_cols"), dict(what="take_str")
    order = lambda n: dict(what="order", n=n)

    def run(*ops):
        m = QueryModel()
        return m, [m.step(op) for op in ops]

    # 1. aggregate, filter and the two takes keep a join result, a prepared build side, the group result, the binding, the plan
    for op in (agg, flt, tk, ts):
        m, said = run(group, prep, op, join)
        assert said[3]["may_prepared"] and said[2]["plan_kept"] and said[2]["binding"]["op"] == 0, op
        m, said = run(kj, op)
        assert said[1]["join_live"] == 0 and said[1]["plan_kept"], op
        m, said = run(group, op)
        assert said[1]["group_live"] == 0 and said[1]["binding"] == {"op": 0, "n_rows": 100, "n_groups": 7}, op
    # 2. ORDER BY with n >= 2 discards a prepared build side and ends the join result; group result, binding, plan stay
    m, said = run(group, prep, order(2), join)
    assert not said[3]["may_prepared"] and m.discarded == 1 and said[2]["plan_kept"] and said[2]["binding"]["op"] == 0
    m, said = run(kj, order(2))
    assert said[1]["join_live"] is None
    m, said = run(group, order(4097))
    assert said[1]["group_live"] == 0 and said[1]["binding"]["n_groups"] == 7
    # 3. n == 1 discards the prepared build side but leaves the join result
    m, said = run(prep, order(1), join)
    assert not said[2]["may_prepared"]
    m, said = run(kj, order(1))
    assert said[1]["join_live"] == 0
    # 4. n == 0 touches nothing
    m, said = run(kj, prep, order(0), join)
    assert said[3]["may_prepared"] and said[2]["plan_kept"] and m.discarded == 0
    m, said = run(kj, order(0))
    assert said[1]["join_live"] == 0
    # 5. the binding begins at a materialising group call that returns HMJ_OK ...
    m, said = run(dict(group, flags=ORDERED, what="group_mixed"))
    assert said[0]["binding"] == {"op": 0, "n_rows": 100, "n_groups": 7}
    # 6. ... ends at the entry of the next group call, count-only calls and refused ones included ...
    m, said = run(group, dict(group, flags=0))
    assert said[1]["binding"] is None and said[1]["group_live"] is None
    m, said = run(group, dict(what="refused", which="group_flags"))
    assert said[1]["binding"] is None and said[1]["rc"] == E_ARG
    m, said = run(group, dict(group, n_rows=5, n_groups=2))
    assert said[1]["binding"] == {"op": 1, "n_rows": 5, "n_groups": 2}
    # 7. ... and at hmj_release_result; set_profiling and forget_workloads leave it
    m, said = run(group, dict(what="config", action="release"))
    assert said[1]["binding"] is None
    m, said = run(group, dict(what="config", action="forget"), dict(what="config", action="profiling"))
    assert said[2]["binding"]["op"] == 0
    # 8. joins, sorts, takes and aggregates in between keep it (not the group COLUMNS: they last until the next call)
    m, said = run(group, kj, dict(what="u64", sub="sort", case=0), join, tk, agg, order(9))
    assert all(s["binding"]["op"] == 0 for s in said) and said[1]["group_live"] is None and said[1]["join_live"] == 1
    # 9. a group call and a key join discard a prepared build side and end the join result
    m, said = run(kj, prep, group, join)
    assert not said[3]["may_prepared"] and said[2]["join_live"] is None and said[2]["plan_kept"]
    m, said = run(prep, kj, join)
    assert not said[2]["may_prepared"]
    # 10. device-found errors leave the ctx usable: the binding stays, nothing else is claimed; a prepared side may be taken
    for which in ("filter_map_beyond_source", "order_decreasing_offsets", "take_map_beyond_source"):
        m, said = run(group, kj, prep, dict(what="refused", which=which), join)
        assert said[3]["rc"] == E_ARG and said[3]["binding"]["op"] == 0 and said[3]["join_live"] is None and not said[3]["plan_kept"], which
        assert said[4]["may_prepared"]
    # 11. an aggregate refused by the host (no live grouping, a wrong n_rows) leaves everything as it was
    for which in HOST_FOUND:
        m, said = run(prep, dict(what="refused", which=which), join)
        assert said[1]["plan_kept"] and said[2]["may_prepared"], which
        m, said = run(kj, dict(what="refused", which=which))
        assert said[1]["join_live"] == 0, which
    # 12. a u64 join of other relations discards the prepared build side like any other call
    m, said = run(prep, dict(join, case=0), join)
    assert not said[1]["may_prepared"] and not said[2]["may_prepared"] and m.discarded == 1


def _perturbed(fn, what):
    try:
        fn()
    except AssertionError:
        return
    raise AssertionError("a wrong output passed: " + what)


def test_every_comparison_refuses_an_output_that_is_wrong_in_one_place():
    import hashmergejoin_amd as H

    rng = np.random.default_rng(5)
    n = 200
    # ---- filter
    x = dict(a=rng.integers(0, 9, size=n).astype(np.int32), valid=rng.random(n) >= 0.2, off=0, exact=True)
    pool = type("P", (), {"H": H, "table_rel": lambda self, ti: dict(n=n, cols=[x], keys=0)})()
    op = dict(what="filter", rel=["table", 0], terms=[[0, GE, 4, True, 0, False]], map=None, want_mask=True)
    want = expect_op(pool, {}, op)
    k = len(want["map"])
    assert 2 <= k < n and want["n_unknown"] > 0
    buf = np.full(n + 1, SENTINEL, np.int64)
    buf[:k] = want["map"].view(np.int64)
    words = np.packbits(np.concatenate([want["mask"], np.zeros(64 * 4 - n, bool)]), bitorder="little").view(np.uint64)
    info = {"n_out": k, "n_unknown": want["n_unknown"]}
    compare_filter(buf, words, info, want)
    compare_filter(buf, None, info, want)
    swapped = buf.copy()
    swapped[[0, 1]] = swapped[[1, 0]]
    _perturbed(lambda: compare_filter(swapped, words, info, want), "two adjacent map entries swapped")
    behind = buf.copy()
    behind[k] = 0
    _perturbed(lambda: compare_filter(behind, words, info, want), "one map entry written behind n_out")
    padded = words.copy()
    padded[-1] |= np.uint64(1 << (n % 64))
    _perturbed(lambda: compare_filter(buf, padded, info, want), "one padding bit set")
    _perturbed(lambda: compare_filter(buf, words, dict(info, n_unknown=info["n_unknown"] + 1), want), "n_unknown off by one")
    # ---- ORDER BY: two adjacent entries swapped among tied rows (a sort that is not stable)
    op = dict(what="order", rel=["table", 0], n=n, cols=[[0, ORDER_DESC, True]])
    want = expect_op(pool, {}, op)
    info = {"n_distinct": want["n_distinct"], "n_tied_rows": want["n_tied_rows"]}
    assert want["n_distinct"] == 10 and want["n_tied_rows"] == n  # nine values and NULL
    compare_order(want["map"].view(np.int64), info, want)
    swapped = want["map"].copy()
    j = next(j for j in range(n - 1) if x["a"][int(swapped[j])] == x["a"][int(swapped[j + 1])] and x["valid"][int(swapped[j])] and x["valid"][int(swapped[j + 1])])
    swapped[[j, j + 1]] = swapped[[j + 1, j]]
    _perturbed(lambda: compare_order(swapped, info, want), "two adjacent map entries swapped among tied rows")
    _perturbed(lambda: compare_order(want["map"], dict(info, n_tied_rows=n - 1), want), "n_tied_rows off by one")
    # ---- aggregates over 70 groups, six of them without a valid value
    ng = 70
    gmap = rng.integers(0, ng - 6, size=n)
    f = dict(a=rng.standard_normal(n) * 2.0 ** rng.integers(-15, 15, size=n), valid=rng.random(n) >= 0.1, off=0, exact=False)
    pool = type("P", (), {"H": H, "table_rel": lambda self, ti: dict(n=n, cols=[x, f], keys=0)})()
    binding = dict(rel=["table", 0], group_of_row=gmap, n_groups=ng, n_rows=n)
    op = dict(what="agg", aggs=[[AGG_SUM, 1, "own"], [AGG_MIN, 0, "own"], [AGG_COUNT, None, None]])
    want = expect_op(pool, {}, op, binding)

    def as_got():
        got = []
        for w in want["want"]:
            v = np.concatenate([w["values"], np.frombuffer(bytes([AGG_FILL]) * w["values"].dtype.itemsize, w["values"].dtype)])
            bits = np.concatenate([w["valid"], np.zeros(128 - ng, bool)])
            words = np.concatenate([np.packbits(bits, bitorder="little").view(np.uint64), np.frombuffer(bytes([AGG_FILL]) * 8, np.uint64)])
            got.append([v, words, w["null_count"]])
        return got

    compare_agg(H, as_got(), want)
    assert want["want"][0]["null_count"] >= 6
    g = as_got()
    g[1][1][1] |= np.uint64(1 << (ng % 64))
    _perturbed(lambda: compare_agg(H, g, want), "one padding bit set")
    g = as_got()
    g[0][2] += 1
    _perturbed(lambda: compare_agg(H, g, want), "null_count off by one")
    g = as_got()
    g[0][0].view(np.uint8)[8 * (ng - 1) + 3] = 1  # (group ng - 1 has no row at all)
    _perturbed(lambda: compare_agg(H, g, want), "one NULL slot's value byte non-zero")
    g = as_got()
    g[2][0][ng] = 0
    _perturbed(lambda: compare_agg(H, g, want), "a slot behind n_groups written")
    slot = int(np.argmax(want["want"][0]["count"]))
    kk, s = int(want["want"][0]["count"][slot]), float(want["want"][0]["values"][slot])
    bound = gamma(kk) * float(want["want"][0]["abs_sum"][slot])
    inside, outside = s + 0.5 * bound, s + bound + 2 * np.spacing(abs(s) + bound)
    g = as_got()
    g[0][0][slot] = inside
    compare_agg(H, g, want)  # another order of summation is accepted ...
    g[0][0][slot] = outside
    _perturbed(lambda: compare_agg(H, g, want), "one group's float sum two ulp beyond its bound")  # ... a wrong sum is not
    # ---- the takes
    m = drawn_map(3, n, 77)
    op = dict(what="take_cols", rel=["table", 0], map=["drawn", 3, n, 77], cols=[0, 1])
    want = expect_op(pool, {}, op)
    outs, words = [c["a"].copy() for c in want["rel"]["cols"]], [w.copy() for w in want["words"]]
    info = {"null_count": list(want["nulls"]), "n_no_row": want["n_no_row"]}
    compare_take_cols(outs, words, info, want)
    assert want["n_no_row"] > 0 and np.count_nonzero(m == np.uint64(NO_ROW)) == want["n_no_row"]
    bad = [w.copy() for w in words]
    bad[0][-1] |= np.uint64(1 << (77 % 64))
    _perturbed(lambda: compare_take_cols(outs, bad, info, want), "one padding bit set")
    _perturbed(lambda: compare_take_cols(outs, words, dict(info, null_count=[want["nulls"][0] + 1, want["nulls"][1]]), want), "null_count off by one")
    bad = [o.copy() for o in outs]
    null_slot = int(np.nonzero(~want["rel"]["cols"][1]["valid"])[0][0])
    bad[1].view(np.uint8)[8 * null_slot] = 1
    _perturbed(lambda: compare_take_cols(bad, words, info, want), "one NULL slot's value byte non-zero")


def test_the_expectations_of_the_default_tours_are_quick():
    """The pool, the default tours (each drawn with a run of the references, drawn again until the caps and seams hold) and
    one more run of the references over them: what the GPU file does on the host before and while it runs the ops.
    Measured: 4.2 s."""
    t0 = time.perf_counter()
    pool = QueryPool(SEQ_SEED, pool_of(SEQ_SEED).H)
    rng = np.random.default_rng([SEQ_SEED, 19])
    tours = [draw_query_sequence(rng, pool) for _ in range(SEQ_TOURS)]
    for ops in tours:
        simulate(pool, ops)
    dt = time.perf_counter() - t0
    print("pool, %d tours and their expectations: %.1f s" % (len(tours), dt))
    assert dt < 12.6, dt  # (4.2 s was measured; three times that before the test speaks up on a loaded machine)
