"""WHERE, ORDER BY, the aggregates and the mixed grouping on ONE long-lived context under drawn sequences of calls, beside the
u64 joins, key joins, group calls and takes the key tours visit (the generators, the model of the contract, the comparison
functions and their CPU checks are test_query_sequences_cpu.py's; the method is test_ctx_sequences_gpu.py's).

  * test_query_calls_on_one_context: one Executor, the default number of tours over eleven op families, each tour run twice in
    a row.  Every op's expectation is computed from the host copies of what its ACTUAL inputs hold -- an earlier aggregate's
    values and bitmap words, an earlier filter's map and mask_out, a take's columns and validity words, the live join's own
    r_row / s_row --, so a stage is judged on its own and not on an upstream float rounding.  Run one checks, after each op,
    the status and everything the op writes (compare_* of the CPU file), hmj_last_plan / hmj_last_timing where the model says
    they stay, and HMJ_PATH_PREPARED only where the model allows it.  Run two adds, after every op, a re-check of everything
    the model says is still alive: the live join's rows are read again and compared with the copy taken right after the
    join, the group columns likewise, and the binding is probed -- a COUNT aggregate without data must equal the group's
    count column, or be HMJ_E_ARG "no live grouping" where the model says there is none.  The probes stay out of run one so
    that they never stand between two adjacent ops;
  * test_the_tours_reached_the_states_they_are_for: the ledger of the default seed;
  * test_whole_queries: two queries that run entirely on the device of the toured context, each compared with one plain
    Python restatement of the whole query (dicts and sorted), on integer-valued data, at the sizes where n_out, the groups
    and the HAVING output are 0, 1, 2, 63, 64, 65 and many.

Every call runs on torch's current stream and every result is read back right after its call.  HMJ_STRESS_SEED /
HMJ_STRESS_ITERS (tours) override the defaults; HMJ_STRESS_DUMP=dir keeps the failing op's index and the ops up to it."""
import ctypes as C
import json
import os
import time

import numpy as np
import pytest

from test_ctx_sequences_cpu import FIRST_WINS, MATERIALIZE, ORDERED, SEQ_TOURS, transitions
from test_ctx_sequences_gpu import check_inner, stress_env
from test_filter_cpu import BETWEEN, GT, IS_NULL, STARTS_WITH
from test_group_cols_gpu import check as check_groups
from test_join_cols_kinds_cpu import BUILD, FULL_OUTER
from test_join_mixed_gpu import LAYOUTS, Rel as MixedRel, dev_str, expect as mixed_expect
from test_keyjoin_sequences_cpu import MIXED_LAYOUTS
from test_keyjoin_sequences_gpu import Ctx as KeyCtx, run_key_join, signed
from test_query_sequences_cpu import (AGG_COUNT, AGG_FILL, AGG_MEAN, AGG_MIN, AGG_SUM, FAMILIES, GROUP_COUNT, GROUP_ROW_MAP, ORDER_DESC,
                                      ORDER_NULLS_FIRST, SEAMS, SENTINEL, WAVE_GROUPS, QueryModel, QueryPool, compare_agg, compare_filter,
                                      compare_order, compare_take_cols, compare_take_str, draw_query_sequence, expect_op, filter_terms, is_string,
                                      resolve_map, resolve_rel, unpack_words)

pytestmark = pytest.mark.gpu
LEDGER = ("took_prepared_directly", "took_prepared_after_agg", "took_prepared_after_filter", "not_prepared_after_order", "agg_after_larger", "filter_after_larger_no_mask",
          "order_after_more_rounds", "agg_bound_to_newer_smaller_grouping", "group_columns_reread_after_order", "join_rows_reread_after_filter",
          "filter_mask_fed_agg", "take_validity_fed_group", "agg_bitmap_fed_filter", "agg_bitmap_fed_order", "map_fed_filter_term",
          "combine_over_64_waves_after_smaller")
assert set(SEAMS) <= set(LEDGER)
REFUSAL_WORDS = {"agg_no_grouping": "no live grouping", "agg_wrong_rows": "n_rows", "filter_map_beyond_source": "1 row_map entries are >= n_src",
                 "order_decreasing_offsets": "offsets decrease at row 2", "take_map_beyond_source": "1 row_map entries",
                 "group_flags": "HMJ_FIRST_WINS is not defined for grouping"}


@pytest.fixture(scope="module")
def H():
    import hashmergejoin_amd as H

    return H


def to_dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()


class Ctx(KeyCtx):
    """The executor under test, the pool's relations on the device, the model, the ledger, and per op of the running tour
    what it returned: `store` holds the host copies (in expect_op's form), `dstore` the device tensors and pointers."""

    def __init__(self, H, seed):  # (KeyCtx.dev serves the join cases and the u64 cases; its own pool is not drawn)
        import torch

        assert torch.cuda.is_available(), "GPU tests need a GPU"
        assert [list(x) for x in MIXED_LAYOUTS] == list(LAYOUTS.values())
        self.H, self.torch = H, torch
        self.ex = H.Executor(0)
        self.pool = QueryPool(seed, H)
        self.pool.mixed_sql = (MixedRel, mixed_expect)
        self.ledger = dict.fromkeys(LEDGER + ("took_prepared",), 0)
        self.executed = self.drawn = 0
        self.done = False
        self._dev = {}
        self.good_str = dev_str([b"aa", b"bb", b"cc", b"dd"])
        bad = self.good_str[1].clone()
        bad[3] = 1
        self.bad_str = (self.good_str[0], bad)
        self.small = torch.arange(100, dtype=torch.int32, device="cuda")
        self.agg_rows, self.no_mask_filters, self.order_rounds = [], [], []  # what the three entries have run so far, over all tours
        self.reset()

    def reset(self):
        self.model = QueryModel()
        self.store, self.dstore = {}, {}
        self.live_join = self.live_group = self.prepared_at = self.last_agg_binding = None

    def rel(self, ref):
        """A relation on the device: a list of {"t": tensor or (chars, offsets), "v": bitmap tensor (uint8) or None, "off"}."""
        if ref[0] in ("agg", "take"):
            return self.dstore[ref[1]]["rel"]
        key = ("rel",) + tuple(ref)
        if key not in self._dev:
            cols = []
            for col in resolve_rel(self.pool, {}, ref)["cols"]:
                t = dev_str(col["a"]) if is_string(col) else to_dev(col["a"])
                v = None if col["valid"] is None else self.H.pack_validity(col["valid"], col["off"], "cuda")
                cols.append({"t": t, "v": v, "off": col["off"]})
            self._dev[key] = cols
        return self._dev[key]

    def row_map(self, ref):
        """A row map as the takes and the filter take it: a tensor, or (device pointer, n) for a result's own column."""
        if ref[0] == "drawn":
            return signed(resolve_map(self.pool, self.store, ref))
        return self.dstore[ref[1]]["map"] if ref[0] in ("filter", "order") else self.dstore[ref[1]][ref[2]]


def validity(col):
    return None if col["v"] is None else (col["v"], col["off"])


# ---- the ops ---------------------------------------------------------------------------------------------------------------------
def run_filter(ctx, op, want, tag, index):
    ex, pool, torch = ctx.ex, ctx.pool, ctx.torch
    exp = expect_op(pool, ctx.store, op)
    rel, drel = resolve_rel(pool, ctx.store, op["rel"]), ctx.rel(op["rel"])
    dm = None if op["map"] is None else ctx.row_map(op["map"])
    terms = []
    for (c, _code, _lit, use_valid, _clause, _negate), t in zip(op["terms"], filter_terms(rel, op, None)):
        terms.append(dict(t, column=drel[c]["t"], valid=drel[c]["v"] if use_valid else None, bit_offset=drel[c]["off"] if use_valid else 0, row_map=dm))
    n = exp["n"]
    buf = torch.full((n + 1,), SENTINEL, dtype=torch.int64, device="cuda")
    got, words, info = ex.filter_device(terms, n=n, want_mask=op["want_mask"], out=buf)
    host_words = None if words is None else words.cpu().numpy().view(np.uint64)
    compare_filter(buf.cpu().numpy(), host_words, info, exp, tag)
    ctx.store[index] = dict(map=got.cpu().numpy().view(np.uint64), n=n, n_unknown=info["n_unknown"],
                            mask=None if host_words is None else unpack_words(host_words, n))
    ctx.dstore[index] = dict(map=got, words=None if words is None else words.view(torch.uint8))
    led = ctx.ledger
    led["agg_bitmap_fed_filter"] += op["rel"][0] == "agg" and any(t[3] for t in op["terms"])
    led["map_fed_filter_term"] += op["map"] is not None and op["map"][0] in ("filter", "order")
    led["filter_after_larger_no_mask"] += any(n < m for m in ctx.no_mask_filters)
    if not op["want_mask"]:
        ctx.no_mask_filters.append(n)


def run_order(ctx, op, want, tag, index):
    ex, pool = ctx.ex, ctx.pool
    exp = expect_op(pool, ctx.store, op)
    drel = ctx.rel(op["rel"])
    assert exp["n"] == op["n"], (tag, "the drawing and the run disagree about the rows", exp["n"])
    cols = [(drel[c]["t"], flags) + ((drel[c]["v"], drel[c]["off"]) if use_valid and drel[c]["v"] is not None else ()) for c, flags, use_valid in op["cols"]]
    out, info = ex.order_by_device(cols, n=op["n"])
    compare_order(out.cpu().numpy(), info, exp, tag)
    ctx.store[index] = dict(map=out.cpu().numpy().view(np.uint64), n=op["n"])
    ctx.dstore[index] = dict(map=out)
    ctx.ledger["agg_bitmap_fed_order"] += op["rel"][0] == "agg" and any(c[2] for c in op["cols"])
    ctx.ledger["order_after_more_rounds"] += any(info["n_rounds"] < r for r in ctx.order_rounds)
    ctx.order_rounds.append(info["n_rounds"])


def raw_agg(ctx, aggs, n_rows, n_groups):
    """hmj_group_agg_device into caller buffers of n_groups + 1 slots and ceil(n_groups / 64) + 1 words, every byte AGG_FILL
    before the call: [(values tensor, words tensor, null_count)].  aggs: (op, tensor or None, bitmap tensor or None, offset)."""
    ex, H, torch = ctx.ex, ctx.H, ctx.torch
    L = H._lib
    ex._sync_stream()
    src, dst = (L.AggSrc * len(aggs))(), (L.AggDst * len(aggs))()
    outs = []
    u64 = getattr(torch, "uint64", torch.int64)
    for k, (code, t, v, off) in enumerate(aggs):
        typ = L.HMJ_TYPE_U64 if t is None else ex._agg_type(t)
        src[k].data = None if t is None or not t.shape[0] else t.data_ptr()
        src[k].type, src[k].op = typ, code
        if v is not None:
            src[k].validity.bits = v.data_ptr() if v.shape[0] else None
            src[k].validity.bit_offset = off
        if code == AGG_COUNT:
            dt = u64
        elif code == AGG_MEAN:
            dt = torch.float64
        elif code == AGG_SUM:
            dt = torch.float64 if typ >= L.HMJ_TYPE_F32 else (torch.int64 if typ <= L.HMJ_TYPE_I64 else u64)
        else:
            dt = t.dtype
        size = torch.empty(0, dtype=dt).element_size()
        o = torch.full(((n_groups + 1) * size,), AGG_FILL, dtype=torch.uint8, device="cuda").view(dt)
        w = torch.full((((n_groups + 63) // 64 + 1) * 8,), AGG_FILL, dtype=torch.uint8, device="cuda").view(torch.int64)
        dst[k].data, dst[k].validity = o.data_ptr(), w.data_ptr()
        outs.append((o, w))
    opts = L.GroupAggOpts()
    opts.struct_size = C.sizeof(L.GroupAggOpts)
    ex._check(ex.L.hmj_group_agg_device(ex.h, src, len(aggs), n_rows, dst, C.byref(opts)))
    assert int(opts.n_groups) == n_groups, (int(opts.n_groups), n_groups)
    return [(o, w, int(dst[k].null_count)) for k, (o, w) in enumerate(outs)]


def run_agg(ctx, op, want, tag, index):
    pool, torch = ctx.pool, ctx.torch
    b = want["binding"]
    assert b is not None, (tag, "the drawing put an aggregate where the model has no live grouping")
    bound = ctx.store[b["op"]]
    assert (bound["n_rows"], bound["n_groups"]) == (b["n_rows"], b["n_groups"]), (tag, "the drawing and the run disagree about the grouping")
    exp = expect_op(pool, ctx.store, op, bound)
    drel = ctx.rel(bound["rel"])
    aggs = []
    for code, c, val in op["aggs"]:
        col = None if c is None else drel[c]
        if val == "own":
            v, off = (None, 0) if col is None or col["v"] is None else (col["v"], col["off"])
        elif val is None:
            v, off = None, 0
        else:
            v, off = ctx.dstore[val[1]]["words"], 0
        aggs.append((code, None if col is None else col["t"], v, off))
    ng = b["n_groups"]
    got = raw_agg(ctx, aggs, b["n_rows"], ng)
    host = [(o.cpu().numpy(), w.cpu().numpy().view(np.uint64), nulls) for o, w, nulls in got]
    compare_agg(ctx.H, host, exp, tag)
    n_words = (ng + 63) // 64
    cols = [dict(a=v[:ng].copy(), valid=unpack_words(w[:n_words], ng), off=0, exact=e["exact"]) for (v, w, _), e in zip(host, exp["rel"]["cols"])]
    ctx.store[index] = dict(rel=dict(n=ng, cols=cols, keys=0))
    ctx.dstore[index] = dict(rel=[{"t": o[:ng], "v": w[:n_words].view(torch.uint8), "off": 0} for o, w, _ in got])
    led, rows = ctx.ledger, b["n_rows"]
    led["filter_mask_fed_agg"] += any(isinstance(a[2], list) for a in op["aggs"])
    led["agg_after_larger"] += any(rows < r for r in ctx.agg_rows)
    led["combine_over_64_waves_after_smaller"] += rows == sum(WAVE_GROUPS) and any(r < rows for r in ctx.agg_rows)
    if ctx.last_agg_binding is not None and ctx.last_agg_binding[0] < b["op"]:
        led["agg_bound_to_newer_smaller_grouping"] += rows < ctx.last_agg_binding[1]
    ctx.last_agg_binding = (b["op"], rows)
    ctx.agg_rows.append(rows)


def run_group(ctx, op, want, tag, index):
    ex, H, pool = ctx.ex, ctx.H, ctx.pool
    exp = expect_op(pool, ctx.store, op)
    assert (exp["n_rows"], exp["n_groups"]) == (op["n_rows"], op["n_groups"]), (tag, "the drawing and the run disagree about the grouping")
    drel = ctx.rel(op["rel"])
    cols = [drel[c] for c in op["cols"]]
    valid = None if all(c["v"] is None for c in cols) else [validity(c) for c in cols]
    keys = [c["t"] for c in cols]
    if op["what"] == "group_mixed":
        res, info = ex.group_mixed_device(keys, None, valid, op["flags"], op["want"])
    else:
        res, info = ex.group_cols_device(keys, None, valid, op["flags"], op["want"])
    e = exp["exp"]
    ctx.ledger["take_validity_fed_group"] += op["rel"][0] == "take"
    if not op["flags"]:
        assert all(v is None for v in ex.group_rows_to_numpy(res).values()), tag
        assert (int(res.n_groups), int(res.n_rows), int(res.max_count)) == (e["n_groups"], e["n_rows"], e["max_count"]), tag
        assert (info["form"], info["n_null"], info["n_collisions"]) == (e["form"], e["n_null"], e["n_collisions"]), (tag, info)
        ctx.store[index] = dict(n_rows=e["n_rows"], n_groups=e["n_groups"], rel=op["rel"])
        return None
    got = ex.group_rows_to_numpy(res)
    check_groups(H, res, info, got, e, bool(op["flags"] & ORDERED), tag, op["want"])
    ctx.store[index] = dict(n_rows=e["n_rows"], n_groups=e["n_groups"], rel=op["rel"], first_row=got["first_row"], group_of_row=got["group_of_row"],
                            count=got["count"])
    ctx.dstore[index] = dict(first_row=(res.first_row, e["n_groups"]))
    return res, got


def run_take_cols(ctx, op, want, tag, index):
    exp = expect_op(ctx.pool, ctx.store, op)
    drel = ctx.rel(op["rel"])
    src = [drel[c] for c in op["cols"]]
    outs, words, info = ctx.ex.take_cols_device([c["t"] for c in src], ctx.row_map(op["map"]), valid=[validity(c) for c in src])
    host_o, host_w = [o.cpu().numpy() for o in outs], [w.cpu().numpy().view(np.uint64) for w in words]
    compare_take_cols(host_o, host_w, info, exp, tag)
    n = exp["rel"]["n"]
    cols = [dict(a=o, valid=unpack_words(w, n), off=0, exact=e["exact"]) for o, w, e in zip(host_o, host_w, exp["rel"]["cols"])]
    ctx.store[index] = dict(rel=dict(n=n, cols=cols, keys=0))
    ctx.dstore[index] = dict(rel=[{"t": o, "v": w.view(ctx.torch.uint8), "off": 0} for o, w in zip(outs, words)])


def run_take_str(ctx, op, want, tag, index):
    exp = expect_op(ctx.pool, ctx.store, op)
    col = ctx.rel(op["rel"])[op["col"]]
    chars, offsets = col["t"]
    co, oo, words, info = ctx.ex.take_str_device(chars, offsets, ctx.row_map(op["map"]), valid=validity(col))
    compare_take_str(co.cpu().numpy(), oo.cpu().numpy(), words.cpu().numpy(), info, exp, tag)


def run_refused(ctx, op, want):
    ex, H, torch, which = ctx.ex, ctx.H, ctx.torch, op["which"]
    a = ctx.small
    try:
        if which == "agg_no_grouping":
            ex.group_agg_device([(AGG_COUNT, None, None)], n_rows=5)
        elif which == "agg_wrong_rows":
            ex.group_agg_device([(AGG_COUNT, None, None)], n_rows=want["binding"]["n_rows"] + 1)
        elif which == "filter_map_beyond_source":
            m = torch.arange(50, dtype=torch.int64, device="cuda")
            m[7] = 100  # == n_src: found on the device, compared before anything is loaded through it
            ex.filter_device([{"column": a, "op": GT, "lit": 3, "row_map": m}], want_mask=True)
        elif which == "order_decreasing_offsets":
            ex.order_by_device([(ctx.bad_str, 0)], n=4)
        elif which == "take_map_beyond_source":
            m = torch.arange(50, dtype=torch.int64, device="cuda")
            m[7] = 100
            ex.take_cols_device([a], m)
        elif which == "group_flags":
            ex.group_cols_device([a], flags=MATERIALIZE | FIRST_WINS)
        else:
            raise ValueError(which)
    except H.HmjError as e:
        return e.code
    return 0


def snapshot(ex):
    return ex.last_plan(), ex.last_timing()["path"]


def probe(ctx, op, want, tag):
    """Run two: everything the model says is still alive, read again."""
    ex, H = ctx.ex, ctx.H
    if want["join_live"] is not None:
        at, read_back, rows = ctx.live_join
        assert at == want["join_live"], (tag, "the run and the model disagree about the live join")
        again = read_back("read again after " + op["what"])
        assert np.array_equal(again, rows), (tag, "the live join's rows changed")
        ctx.ledger["join_rows_reread_after_filter"] += op["what"] == "filter"
    if want["group_live"] is not None:
        at, res, cols = ctx.live_group
        assert at == want["group_live"], (tag, "the run and the model disagree about the live group result")
        again = ex.group_rows_to_numpy(res)
        for name, col in cols.items():
            assert (col is None and again[name] is None) or np.array_equal(col, again[name]), (tag, "the group result's column changed", name)
        ctx.ledger["group_columns_reread_after_order"] += op["what"] == "order"
    before = snapshot(ex)
    if want["binding"] is None:
        with pytest.raises(H.HmjError) as e:
            ex.group_agg_device([(AGG_COUNT, None, None)], n_rows=1)
        assert e.value.code == -1 and "no live grouping" in str(e.value), (tag, str(e.value))
    else:
        b = want["binding"]
        got = raw_agg(ctx, [(AGG_COUNT, None, None, 0)], b["n_rows"], b["n_groups"])
        count = got[0][0].cpu().numpy()[:b["n_groups"]]
        assert np.array_equal(count.view(np.uint64), ctx.store[b["op"]]["count"]), (tag, "COUNT over the live grouping is not its count column")
    assert snapshot(ex) == before, (tag, "an aggregate leaves hmj_last_plan / hmj_last_timing as they were")


def run_op(ctx, op, tag, index, probing):
    ex, H, pool = ctx.ex, ctx.H, ctx.pool
    want = ctx.model.step(op)
    what = op["what"]
    before = snapshot(ex)
    if what == "filter":
        run_filter(ctx, op, want, tag, index)
    elif what == "order":
        run_order(ctx, op, want, tag, index)
    elif what == "agg":
        run_agg(ctx, op, want, tag, index)
    elif what in ("group_cols", "group_mixed"):
        live = run_group(ctx, op, want, tag, index)
        ctx.live_group = None if live is None else (index,) + live
    elif what == "take_cols":
        run_take_cols(ctx, op, want, tag, index)
    elif what == "take_str":
        run_take_str(ctx, op, want, tag, index)
    elif what == "key_join":
        read_back, maps, _ = run_key_join(ctx, dict(op, what=op["kw"]), {"rc": 0}, tag)
        rows = read_back("the copy of the rows")
        ctx.live_join = (index, read_back, rows)
        ctx.store[index] = dict(n=len(rows), r_row=rows[:, 1].copy(), s_row=rows[:, 2].copy())
        ctx.dstore[index] = maps
    elif what == "u64":
        if op["sub"] == "join":
            plan = check_inner(ctx, op, want, pool.expect_u64(op["case"]), tag)
            took = bool(plan["path"] & H.HMJ_PATH_PREPARED)
            if ctx.prepared_at is not None:
                between = [o["what"] for o in ctx.prepared_at]
                ctx.ledger["took_prepared_directly"] += took and not between  # (the control: this shape does reuse a prepared build side)
                ctx.ledger["took_prepared_after_agg"] += took and between == ["agg"]
                ctx.ledger["took_prepared_after_filter"] += took and between == ["filter"]
                ctx.ledger["not_prepared_after_order"] += not took and between == ["order"] and ctx.prepared_at[0]["n"] >= 1
        elif op["sub"] == "sort":
            a = ctx.dev(op["case"])[op["side"]]
            out = ex.sort_device(a.clone() if op["inplace"] else a, inplace=op["inplace"])
            assert np.array_equal(out.cpu().numpy().view(np.uint64), pool.expect_sorted(op["case"], op["side"])), tag
        else:
            ex.prepare_build(ctx.dev(op["case"])[0], op["hint"])
    elif what == "config":
        if op["action"] == "release":
            ex.release_result()
        elif op["action"] == "profiling":
            ex.set_profiling(op["value"])
        else:
            ex.forget_workloads()
    elif what == "refused":
        rc = run_refused(ctx, op, want)
        assert rc == want["rc"], (tag, rc, want["rc"])
        msg = ex.L.hmj_last_error(ex.h).decode()
        assert REFUSAL_WORDS[op["which"]] in msg, (tag, "hmj_last_error after the refused call", msg)
    else:
        raise ValueError(what)
    if want["plan_kept"]:
        assert snapshot(ex) == before, (tag, "the call leaves hmj_last_plan / hmj_last_timing as they were")
    if want["join_live"] is None:
        ctx.live_join = None
    if want["group_live"] is None:
        ctx.live_group = None
    if what == "u64":
        ctx.prepared_at = [] if op["sub"] == "prepare" else None
    elif ctx.prepared_at is not None:
        ctx.prepared_at.append(op)
    if probing:
        probe(ctx, op, want, tag)
    ctx.executed += 1


def dump_failure(ctx, ops, i, run):
    out = os.environ.get("HMJ_STRESS_DUMP")
    if out:
        with open(os.path.join(out, "fail_query_sequence.json"), "w") as f:
            json.dump({"seed": ctx.pool.seed, "run": run, "index": i, "ops": ops[:i + 1]}, f)


def run_tours(ctx, tours, label):
    for t, ops in enumerate(tours):
        ctx.drawn += 2 * len(ops)
        for rep in range(2):  # the second run meets the workspaces and memos of the first, and probes after every op
            ctx.reset()
            t0 = time.perf_counter()
            for i, op in enumerate(ops):
                tag = (label, ctx.pool.seed, t, rep, i, json.dumps(op, sort_keys=True))
                try:
                    run_op(ctx, op, tag, i, probing=rep == 1)
                except Exception:
                    dump_failure(ctx, ops, i, (t, rep))
                    print("failing op:", tag, flush=True)
                    raise
            print("%s: seed %d tour %d run %d: %d ops in %.1f s" % (label, ctx.pool.seed, t, rep, len(ops), time.perf_counter() - t0), flush=True)


@pytest.fixture(scope="module")
def ctx(H):
    _, seed, _ = stress_env()
    c = Ctx(H, seed)
    yield c
    c.close()


def test_query_calls_on_one_context(ctx):
    _, seed, iters = stress_env()
    n_tours = int(iters) if iters else SEQ_TOURS
    rng = np.random.default_rng([seed, 19])
    t0 = time.perf_counter()
    tours = [draw_query_sequence(rng, ctx.pool) for _ in range(n_tours)]
    for ops in tours:
        assert transitions([op["fam"] for op in ops]) == {(x, y) for x in FAMILIES for y in FAMILIES}
    print("%d tours drawn in %.1f s" % (n_tours, time.perf_counter() - t0), flush=True)
    run_tours(ctx, tours, "query calls")
    assert ctx.executed == ctx.drawn == 2 * n_tours * (len(FAMILIES) ** 2 + 1)  # no op was skipped
    print("ledger:", ctx.ledger, flush=True)
    ctx.done = True


def test_the_tours_reached_the_states_they_are_for(ctx):
    """At least one of each: a u64 join that took a build side prepared before an aggregate, and before a filter; one that
    did not after an ORDER BY; an aggregate after one over more rows, a filter after a larger one that kept its mask in the
    workspace, an ORDER BY after one with more rounds; an aggregate bound to a newer and smaller grouping than the one
    before it; group columns read again after an ORDER BY and join rows after a filter (run two); every seam between the
    entries' formats; and the grouping whose middle group spans more than 64 walk waves aggregated after a smaller one."""
    assert ctx.done, "the tours did not finish"
    default, _, _ = stress_env()
    if default:
        missing = [k for k in LEDGER if not ctx.ledger[k]]
        assert not missing, (missing, ctx.ledger)


# ---- whole queries ------------------------------------------------------------------------------------------------------------------
def words_u8(w):
    import torch

    return w.view(torch.uint8)


def names_of(H, chars, offsets, words, n):
    """A taken string column on the host: bytes, or None in a NULL slot."""
    raw, off, ok = chars.cpu().numpy().tobytes(), offsets.cpu().numpy(), unpack_words(words.cpu().numpy(), n)
    return [raw[off[i]:off[i + 1]] if ok[i] else None for i in range(n)]


def taken(out, words, n):
    v, ok = out.cpu().numpy(), unpack_words(words.cpu().numpy(), n)
    return [v[i].item() if ok[i] else None for i in range(n)]


def sales_table(n, seed):
    rng = np.random.default_rng([seed, n])
    names = [b"a%02d" % i for i in range(20)] + [b"b%02d" % i for i in range(10)]
    name = [names[int(i)] for i in rng.integers(0, len(names), size=n)]
    name_ok = rng.random(n) >= 0.1
    day = rng.integers(0, 5, size=n).astype(np.int32)
    price = rng.integers(0, 1000000, size=n).astype(np.float64)
    price_ok = rng.random(n) >= 0.2
    qty = rng.integers(0, 100, size=n).astype(np.int32)
    qty_ok = rng.random(n) >= 0.1
    ts = rng.integers(-2 ** 40, 2 ** 40, size=n).astype(np.int64)
    marks = rng.permutation(n)[:2]  # two rows a BETWEEN can single out
    qty[marks], qty_ok[marks] = [1000000, 1000001][:len(marks)], True
    return dict(n=n, name=name, name_ok=name_ok, day=day, price=price, price_ok=price_ok, qty=qty, qty_ok=qty_ok, ts=ts)


def sales_in_python(t, lo, hi, prefix, c):
    """SELECT name, day, SUM(price), COUNT(qty), MIN(ts) FROM t WHERE (qty BETWEEN lo AND hi OR name STARTS_WITH prefix)
    GROUP BY name, day HAVING SUM(price) > c ORDER BY SUM(price) DESC NULLS FIRST, name, day -- with SQL's NULLs."""
    groups = {}
    for i in range(t["n"]):
        name = t["name"][i] if t["name_ok"][i] else None
        qty = int(t["qty"][i]) if t["qty_ok"][i] else None
        if not ((qty is not None and lo <= qty <= hi) or (name is not None and name.startswith(prefix))):
            continue  # FALSE or UNKNOWN
        g = groups.setdefault((name, int(t["day"][i])), {"sum": None, "count": 0, "min": None})
        if t["price_ok"][i]:
            g["sum"] = (g["sum"] or 0.0) + float(t["price"][i])
        g["count"] += qty is not None
        g["min"] = int(t["ts"][i]) if g["min"] is None else min(g["min"], int(t["ts"][i]))
    rows = [(k[0], k[1], g["sum"], g["count"], g["min"]) for k, g in groups.items()]
    kept = [r for r in rows if r[2] is not None and r[2] > c]
    # DESC over the valid sums; a NULL name sorts last (the default); day makes the order total
    kept = sorted(kept, key=lambda r: (-r[2], r[0] is None, r[0] or b"", r[1]))
    return kept, len(rows), sorted((r[2] for r in rows if r[2] is not None), reverse=True)  # (the rows, the groups, their sums)


SALES = [(1, "many", None), (64, "many", None), (513, "none", None), (513, "one", None), (513, "two", None), (4097, "many", 0), (4097, "many", 1),
         (4097, "many", 63), (4097, "many", 64), (4097, "many", 65), (4097, "many", None)]


def sales_query(ex, H, n, where, having):
    """WHERE -> take -> GROUP BY (string and int key) -> SUM / COUNT / MIN -> ORDER BY over the aggregate (its bitmap is the
    column's validity) -> HAVING as a filter THROUGH the order's map (the same bitmap is the term's validity) -> takes."""
    t = sales_table(n, 41)
    lo, hi, prefix = {"many": (0, 50, b"a1"), "none": (5, 4, b"zz"), "one": (1000000, 1000000, b"zz"), "two": (1000000, 1000001, b"zz")}[where]
    _, _, sums = sales_in_python(t, lo, hi, prefix, -1.0)
    c = -1.0
    if having is not None:  # a literal the host picks so that exactly `having` groups pass (sums are distinct integers here)
        assert len(set(sums)) == len(sums) > having, "the table does not allow this HAVING size"
        c = sums[having] if having < len(sums) else -1.0
    want, n_groups_py, _ = sales_in_python(t, lo, hi, prefix, c)
    if having is not None:
        assert len(want) == having
    name = dev_str([x if ok else b"" for x, ok in zip(t["name"], t["name_ok"])])
    v = lambda k: H.pack_validity(t[k], 3, "cuda")
    name_v, price_v, qty_v = v("name_ok"), v("price_ok"), v("qty_ok")
    day, price, qty, ts = (to_dev(t[k]) for k in ("day", "price", "qty", "ts"))
    W, _, info = ex.filter_device([dict(column=qty, op=BETWEEN, lit=(lo, hi), valid=qty_v, bit_offset=3),
                                   dict(column=name, op=STARTS_WITH, lit=prefix, valid=name_v, bit_offset=3)], n=n)
    n_w = info["n_out"]
    assert n_w == {"none": 0, "one": 1, "two": 2}.get(where, n_w)
    (d_day, d_price, d_qty, d_ts), (w_day, w_price, w_qty, w_ts), _ = ex.take_cols_device([day, price, qty, ts], W, valid=[None, (price_v, 3), (qty_v, 3), None])
    nc, no, nw, _ = ex.take_str_device(name[0], name[1], W, valid=(name_v, 3))
    res, _ = ex.group_mixed_device([(nc, no), d_day], None, [words_u8(nw), None], MATERIALIZE, GROUP_COUNT | GROUP_ROW_MAP)
    ng = int(res.n_groups)
    assert ng == n_groups_py
    (s, s_w, _), (cnt, _, _), (mn, mn_w, _) = ex.group_agg_device([(AGG_SUM, d_price, words_u8(w_price)), (AGG_COUNT, d_qty, words_u8(w_qty)),
                                                                   (AGG_MIN, d_ts, None)], n_rows=n_w)[0]
    gc, go, gw, _ = ex.take_str_device(nc, no, (res.first_row, ng), valid=words_u8(nw))  # the groups' names ...
    (g_day,), _, _ = ex.take_cols_device([d_day], (res.first_row, ng))                  # ... and days
    order, _ = ex.order_by_device([(s, ORDER_DESC | ORDER_NULLS_FIRST, s_w), ((gc, go), 0, words_u8(gw)), (g_day, 0)], n=ng)
    keep, _, hinfo = ex.filter_device([dict(column=s, op=GT, lit=c, valid=s_w, row_map=order)], n=ng)
    assert hinfo["n_out"] == len(want)
    (final,), _, _ = ex.take_cols_device([order], keep)  # positions of the order that pass -> groups, still in order
    k = len(want)
    (f_day, f_s, f_cnt, f_mn), (_, fw_s, _, fw_mn), _ = ex.take_cols_device([g_day, s, cnt, mn], final, valid=[None, words_u8(s_w), None, words_u8(mn_w)])
    fc, fo, fw, _ = ex.take_str_device(gc, go, final, valid=words_u8(gw))
    got = list(zip(names_of(H, fc, fo, fw, k), f_day.cpu().numpy().tolist(), taken(f_s, fw_s, k), [int(x) for x in f_cnt.cpu().numpy()],
                   taken(f_mn, fw_mn, k)))
    assert got == want, (n, where, having, got[:3], want[:3])


def outer_in_python(rk, rg, rv, sk, sw, x):
    """SELECT r.g, COUNT(*), SUM(s.w), COUNT(s.w) FROM r FULL OUTER JOIN s ON r.k = s.k WHERE s.k IS NULL OR r.v > x GROUP BY r.g
    ORDER BY COUNT(*) DESC, r.g NULLS FIRST -- r.g, r.v are NULL in the rows of unmatched s rows, s.w in those of unmatched r rows."""
    by_key = {}
    for j, k in enumerate(sk):
        by_key.setdefault(int(k), []).append(j)
    rows, hit = [], set()
    for i, k in enumerate(rk):
        js = by_key.get(int(k), [])
        hit.update(js)
        rows += [(i, j) for j in js] or [(i, None)]
    rows += [(None, j) for j in range(len(sk)) if j not in hit]
    groups = {}
    for i, j in rows:
        if not (j is None or (i is not None and int(rv[i]) > x)):
            continue
        g = groups.setdefault(None if i is None else int(rg[i]), [0, None, 0])
        g[0] += 1
        if j is not None:
            g[1] = (g[1] or 0) + int(sw[j])
            g[2] += 1
    out = [(k, g[0], g[1], g[2]) for k, g in groups.items()]
    return sorted(out, key=lambda r: (-r[1], r[0] is not None, r[0] or 0)), len(rows)


OUTER = [(1, "many"), (64, "many"), (513, "none"), (513, "one"), (513, "two"), (4097, "many")]


def outer_query(ex, H, n, where, having=None):
    """r FULL OUTER JOIN s -> WHERE through the result's own r_row / s_row -> takes -> GROUP BY -> aggregates -> ORDER BY ->
    take; ORDER BY stands last because it ends the join result.  "none" is the empty chain: 0 rows through the group call,
    the aggregate (n_rows == 0), ORDER BY (n == 0) and the takes."""
    rng = np.random.default_rng([43, n])
    if where == "many":
        rk, sk = rng.integers(0, max(2, n // 2), size=n).astype(np.int32), rng.integers(0, max(2, n // 2), size=n + 3).astype(np.int32)
        rv = rng.integers(0, 100, size=n).astype(np.int64)
        x = 40
    else:  # every r row has exactly one partner and r.v is a permutation: r.v > x selects as many rows as the case names
        rk = rng.permutation(n).astype(np.int32)
        sk = np.concatenate([rk, np.arange(n, n + 5, dtype=np.int32)])[rng.permutation(n + 5)]
        rv = rng.permutation(n).astype(np.int64)
        x = n - 1 - {"none": 0, "one": 1, "two": 2}[where]
    rg = rng.integers(0, 70, size=n).astype(np.int32)
    sw = rng.integers(-1000, 1000, size=len(sk)).astype(np.int64)
    want, n_rows_py = outer_in_python(rk, rg, rv, sk, sw, x)
    d_rk, d_sk, d_rv, d_rg, d_sw = (to_dev(a) for a in (rk, sk, rv, rg, sw))
    res, _ = ex.join_kind_cols_device([d_rk], None, [d_sk], None, BUILD, FULL_OUTER, MATERIALIZE)
    m = int(res.n_matches)
    assert m == n_rows_py
    r_row, s_row = (res.r_row, m), (res.s_row, m)
    W, _, info = ex.filter_device([dict(column=d_sk, op=IS_NULL, row_map=s_row), dict(column=d_rv, op=GT, lit=x, row_map=r_row)], n=m)
    if where != "many":
        assert info["n_out"] == {"none": 0, "one": 1, "two": 2}[where]
    (j_rg,), (jw_rg,), _ = ex.take_cols_device([d_rg], r_row)   # the join's columns, taken before anything ends the result
    (j_sw,), (jw_sw,), _ = ex.take_cols_device([d_sw], s_row)
    (g, w), (g_w, w_w), _ = ex.take_cols_device([j_rg, j_sw], W, valid=[words_u8(jw_rg), words_u8(jw_sw)])
    gres, _ = ex.group_cols_device([g], None, [words_u8(g_w)], MATERIALIZE, GROUP_COUNT | GROUP_ROW_MAP)
    ng = int(gres.n_groups)
    assert ng == len(want)
    (rows, _, _), (s, s_w, _), (cnt, _, _) = ex.group_agg_device([(AGG_COUNT, None, None), (AGG_SUM, w, words_u8(w_w)), (AGG_COUNT, w, words_u8(w_w))],
                                                                 n_rows=info["n_out"])[0]
    (keys,), (keys_w,), _ = ex.take_cols_device([g], (gres.first_row, ng), valid=[words_u8(g_w)])
    order, _ = ex.order_by_device([(rows, ORDER_DESC), (keys, ORDER_NULLS_FIRST, keys_w)], n=ng)
    (f_k, f_rows, f_s, f_cnt), (fw_k, _, fw_s, _), _ = ex.take_cols_device([keys, rows, s, cnt], order, valid=[words_u8(keys_w), None, words_u8(s_w), None])
    got = list(zip(taken(f_k, fw_k, ng), [int(v) for v in f_rows.cpu().numpy()], taken(f_s, fw_s, ng), [int(v) for v in f_cnt.cpu().numpy()]))
    assert got == want, (n, where, got[:3], want[:3])


QUERIES = [("sales",) + q for q in SALES] + [("outer",) + q + (None,) for q in OUTER]


@pytest.mark.parametrize("query,n,where,having", QUERIES)
def test_whole_queries(ctx, H, query, n, where, having):
    """Each query runs entirely on the device of the toured context and is compared with ONE plain-Python restatement of the
    whole query (sales_in_python, outer_in_python: dicts and sorted, none of the H.expected_* references); the data are
    integer-valued, so the comparison is exact.  where: the rows the WHERE clause lets through (none, one, two, many);
    having: the groups the HAVING clause does."""
    assert ctx.done, "the tours did not finish"
    (sales_query if query == "sales" else outer_query)(ctx.ex, H, n, where, having)
