"""The key-join, take and group entries on ONE long-lived context under drawn sequences of calls (the generators, the model of
the contract and their CPU checks are test_keyjoin_sequences_cpu.py's; the method is test_ctx_sequences_gpu.py's).

  * test_key_calls_on_one_context: one Executor, the default number of tours over eleven op families, each tour run twice in
    a row.  After every op: the status; n_matches, sums, checksums, sum_probe_all; the kind counters, n_key_pairs /
    n_hash_pairs, n_collisions, n_*_null, form; which result columns exist; the rows (a sequence under HMJ_ORDERED, a sorted
    multiset otherwise); for a group every column asked for (unordered results by first_row), n_null and max_count; for a
    take values, validity words with their padding bits, null_count, n_no_row, offsets and total_bytes -- and after the take
    the earlier op's result is read back and compared again; for a u64 join HMJ_PATH_PREPARED only where the model allows it
    and the forced radix bits; after a group call and after a take last_plan() and last_timing()["path"] are what they were.
    Key joins, takes and groups run UNDER whatever hmj_set_radix_bits / hmj_set_key_prefix_bits the last config op left;
  * test_the_tours_reached_the_states_they_are_for: the ledger of the default seed;
  * test_a_forgotten_context_joins_and_plans_like_a_new_one: after the tours and hmj_forget_workloads every pool case of the
    key-join and group families runs on the toured context and on a fresh one in lockstep;
  * test_a_planner_hint_does_not_reach_key64: hmj_set_key_prefix_bits describes the caller's u64 keys; the hashed column,
    string and mixed joins and a packed join whose keys fill 64 bits must give the same rows under any hint.

Every call runs on torch's current stream and every result is read back right after its call.  HMJ_STRESS_SEED /
HMJ_STRESS_ITERS (tours) override the defaults; HMJ_STRESS_DUMP=dir keeps the failing op's index and the ops up to it (the
pool is a function of the seed)."""
import ctypes as C
import json
import os
import time

import numpy as np
import pytest

from test_ctx_sequences_cpu import CHECKSUM, FIRST_WINS, MATERIALIZE, ORDERED, SEQ_TOURS, SUM_PROBE, materialising, transitions
from test_ctx_sequences_gpu import PLAN_FIELDS, check_inner, stress_env
from test_group_cols_gpu import check as check_groups
from test_join_cols_kinds_cpu import ANTI, BUILD, COUNT_KEYS, FULL_OUTER, INNER, M64, NO_ROW, PROBE, SEMI, kind_checks
from test_join_mixed_gpu import LAYOUTS, Rel as MixedRel, dev_str, expect as mixed_expect
from test_join_str_gpu import brute as str_brute, rel as str_rel, unordered
from test_join_str_kinds_cpu import kind_brute, tmix_checks
from test_join_str_nulls_gpu import rep_pairs
from test_keyjoin_sequences_cpu import (BFILL, COLS_HASHED, E_UNSUPPORTED, FAMILIES, KEY_FAMILIES, MIXED_LAYOUTS, NULL_EQUAL, PFILL, REFUSALS,
                                        KeyModel, KeyPool, draw_key_sequence, drawn_map, key_expectation, mixed_columns, mixed_masks,
                                        take_cols_expect, take_str_expect)
from test_kinds_sweep_gpu import path_names, to_dev

pytestmark = pytest.mark.gpu
LEDGER = ("took_prepared_after_takes", "discarded_by_group", "discarded_by_cols_kind", "discarded_by_mixed", "cols_kind_after_larger",
          "mixed_after_larger", "group_after_larger", "cols_kind_after_bitmaps", "mixed_after_bitmaps", "group_after_bitmaps",
          "key_join_under_forced_bits", "key_join_under_prefix_hint", "take_read_back") + tuple("regrew_" + f for f in
                                                                                                  ("cols", "mixed", "groups", "strs", "u64"))
SEMI_ANTI = (SEMI, ANTI)


@pytest.fixture(scope="module")
def H():
    import hashmergejoin_amd as H

    return H


def signed(a):
    import torch

    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view("i%d" % a.dtype.itemsize).copy()).cuda()


def dev_vals(v):
    return None if v is None else signed(np.array([int(x) & M64 for x in v], np.uint64) if isinstance(v, list) else np.asarray(v, np.uint64))


def dev_valid(H, masks, off):
    return None if masks is None or all(m is None for m in masks) else [None if m is None else (H.pack_validity(m, off, "cuda"), off) for m in masks]


class Ctx:
    """The executor under test with the pool's relations on the device, the model and the ledger."""

    def __init__(self, H, seed):
        import torch

        assert torch.cuda.is_available(), "GPU tests need a GPU"
        assert [list(x) for x in MIXED_LAYOUTS] == list(LAYOUTS.values())
        self.H, self.torch = H, torch
        self.ex = H.Executor(0)
        self.pool = KeyPool(seed, H)
        self.pool.mixed_sql = (MixedRel, mixed_expect)
        self.model = KeyModel()
        self.ledger = dict.fromkeys(LEDGER + ("took_prepared",), 0)  # (took_prepared: test_ctx_sequences_gpu.check_inner counts it)
        self.executed = self.drawn = 0
        self.largest = dict.fromkeys(("cols", "mixed", "groups", "strs", "u64"), 0)
        self.live = None      # (index of the op, a function that reads its result back and compares it again, its row maps)
        self.prepared_at = None
        self.done = False
        self._dev = {}
        # the relations of the refusals
        rng = np.random.default_rng(3000)
        with np.errstate(over="ignore"):
            t = [rng.permutation(3000).astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15), rng.permutation(3000).astype(np.uint32),
                 rng.integers(0, 1 << 16, 3000).astype(np.uint16)]
        shuffle = rng.permutation(3000)
        self.cap_cols = ([signed(c) for c in t], [signed(c[shuffle]) for c in t])  # 3000 distinct tuples, one-to-one
        k1 = H.cols_key64(t, [8, 4, 2], 1)
        a = int(np.flatnonzero(k1 == k1[0])[1])
        self.cap_group = [signed(c[np.array([0, a] * 550)]) for c in t]  # 1100 rows of one key64 (hash_bits 1), two tuples
        self.good_str = dev_str([b"aa", b"bb", b"cc", b"dd"])
        bad = self.good_str[1].clone()
        bad[3] = 1
        self.bad_str = (self.good_str[0], bad)
        self.small = torch.arange(100, dtype=torch.int32, device="cuda")

    def dev(self, kind, i=None):
        """The case on the device (uploaded once); kind: "cols", "mixed", "groups", "strs", or a u64 case index as
        test_ctx_sequences_gpu.check_inner asks for it."""
        if i is None:
            kind, i = "u64", kind
        key = (kind, i)
        if key in self._dev:
            return self._dev[key]
        H, pool = self.H, self.pool
        if kind == "u64":
            B, P = pool.relations(i)
            d = (to_dev(B), to_dev(P))
        elif kind == "cols":
            c = pool.cols[i]
            d = tuple(([signed(col) for col in s["cols"]], dev_vals(s["vals"]), dev_valid(H, s["masks"], s["off"])) for s in (c["b"], c["p"]))
        elif kind == "mixed":
            c = pool.mixed[i]
            d = []
            for s in (c["b"], c["p"]):
                cols = [signed(col) if isinstance(col, np.ndarray) else dev_str(col) for col in mixed_columns(c["layout"], s)]
                d.append((cols, dev_vals(s["vals"]), dev_valid(H, mixed_masks(c["layout"], s), s["off"])))
            d = tuple(d)
        elif kind == "groups":
            g = pool.groups[i]
            d = ([signed(col) for col in g["cols"]], dev_vals(g["vals"]), dev_valid(H, g["valid"], g["off"]))
        else:
            c = pool.strs[i]
            valid = lambda m, off: None if m is None else (H.pack_validity(m, off, "cuda"), off)
            d = ((str_rel(H, c["bk"], c["bv"], c["shift_b"], c["base_b"]), valid(c["bmask"], c["off_b"])),
                 (str_rel(H, c["pk"], c["pv"], c["shift_p"], c["base_p"]), valid(c["pmask"], c["off_p"])))
        self._dev[key] = d
        return d

    def close(self):
        self.ex.close()


# ---- the key joins ---------------------------------------------------------------------------------------------------------------
def check_key_result(ctx, op, res, info, exp, tag, str_form=False):
    """One key join's result against its expectation; returns the function that reads the rows back and compares them again."""
    ex, flags = ctx.ex, op["flags"]
    rows = exp["rows"]
    if "ck" not in exp:
        exp["ck"] = tmix_checks(rows) if str_form else kind_checks(rows)
    ck, got_ck = exp["ck"], res.checks()
    if flags & CHECKSUM:
        assert got_ck == ck, (tag, got_ck, ck)
    else:
        assert [got_ck[k] for k in ("n_matches", "sum_r", "sum_s")] == [ck[k] for k in ("n_matches", "sum_r", "sum_s")], (tag, got_ck, ck)
    if flags & SUM_PROBE:
        assert int(res.sum_probe_all) == exp["sum_probe"], tag
    assert {k: info.get(k, 0) for k in COUNT_KEYS} == exp["counts"], (tag, info, exp["counts"])
    assert (info["n_build_null"], info["n_probe_null"]) == exp["nulls"], (tag, info, exp["nulls"])
    pairs = (info["n_hash_pairs" if str_form else "n_key_pairs"], info["n_collisions"])
    assert pairs == exp["pairs"], (tag, "pairs of equal key64, and those whose keys differ", pairs, exp["pairs"])
    if not str_form:
        assert info.get("form", COLS_HASHED) == exp["form"], (tag, info)
    key = res.hash if str_form else res.key64
    if not materialising(flags):
        assert not key, tag
        return None
    semi_anti = op["kind"] in SEMI_ANTI
    has_r, has_s = not (semi_anti and op["side"] == PROBE), not (semi_anti and op["side"] == BUILD)
    if len(rows):
        assert key and bool(res.r_row) == bool(res.rval) == has_r and bool(res.s_row) == bool(res.sval) == has_s, (tag, "result columns")
    to_numpy = ex.str_kind_rows_to_numpy if str_form else ex.cols_kind_rows_to_numpy

    def read_back(why):
        got = to_numpy(res)
        assert got.shape == rows.shape, (tag, why, got.shape, rows.shape)
        if flags & ORDERED:
            assert np.array_equal(got, rows), (tag, why, np.flatnonzero(np.any(got != rows, axis=1))[:5])
        else:
            assert np.array_equal(unordered(got), unordered(rows)), (tag, why)
        return got

    read_back("after the call")
    return read_back


def expect_refused_by_cap(ctx, call, tag):
    with pytest.raises(ctx.H.HmjError) as e:
        call()
    assert e.value.code == E_UNSUPPORTED and "1024 rows" in str(e.value), (tag, str(e.value))


def run_key_join(ctx, op, want, tag):
    ex, H, pool = ctx.ex, ctx.H, ctx.pool
    what, flags, side, kind = op["what"], op["flags"], op["side"], op["kind"]
    exp = key_expectation(pool, op)
    str_form = what == "str_kind"
    if what == "str_kind":
        c = pool.strs[op["case"]]
        (B, VB), (P, VP) = ctx.dev("strs", op["case"])
        if "pairs" not in exp:  # the pairs of equal hash the kind compares (test_join_str_nulls_gpu.expect_all)
            kb = [c["bk"][r] for r in np.flatnonzero(~exp["bnull"])]
            kp = [c["pk"][s] for s in np.flatnonzero(~exp["pnull"])]
            if kind in SEMI_ANTI:
                exp["pairs"] = rep_pairs(kp, kb, c["hash_bits"]) if side == BUILD else rep_pairs(kb, kp, c["hash_bits"])
            else:
                coll = str_brute(kb, [0] * len(kb), kp, [0] * len(kp), c["hash_bits"])[1]
                r = exp["rows"]
                exp["pairs"] = (int(((r[:, 1] != NO_ROW) & (r[:, 2] != NO_ROW)).sum()) + coll, coll)
        call = lambda: ex.join_kind_str_device(B, P, side, kind, flags, hash_bits=c["hash_bits"], probe_fill=PFILL, build_fill=BFILL,
                                               build_valid=VB if op["bitmaps"] else None, probe_valid=VP if op["bitmaps"] else None)
    elif what == "mixed":
        c = pool.mixed[op["case"]]
        DB, DP = ctx.dev("mixed", op["case"])
        bitmaps = op["sem"] != "plain"
        call = lambda: ex.join_mixed_device(DB[0], DB[1], DP[0], DP[1], side, kind, flags | (NULL_EQUAL if op["sem"] == "ne" else 0),
                                            hash_bits=c["bits"], probe_fill=PFILL, build_fill=BFILL, build_valid=DB[2] if bitmaps else None,
                                            probe_valid=DP[2] if bitmaps else None)
    else:
        c = pool.cols[op["case"]]
        DB, DP = ctx.dev("cols", op["case"])
        bitmaps = op["sem"] != "plain"
        if what == "cols_inner":
            call = lambda: ex.join_cols_device(DB[0], DB[1], DP[0], DP[1], flags, hash_bits=c["bits"], force_hashed=op["force"])
        else:
            call = lambda: ex.join_kind_cols_device(DB[0], DB[1], DP[0], DP[1], side, kind, flags | (NULL_EQUAL if op["sem"] == "ne" else 0),
                                                    hash_bits=c["bits"], force_hashed=op["force"], probe_fill=PFILL, build_fill=BFILL,
                                                    build_valid=DB[2] if bitmaps else None, probe_valid=DP[2] if bitmaps else None)
    if want["rc"] == E_UNSUPPORTED:
        expect_refused_by_cap(ctx, call, tag)
        return None
    res, info = call()
    plan = ex.last_plan()
    assert not plan["path"] & H.HMJ_PATH_PREPARED, (tag, "a key join took a prepared build side")
    read_back = check_key_result(ctx, op, res, info, exp, tag, str_form)
    if read_back is None:
        return None
    maps = {"r_row": (res.r_row, int(res.n_matches)), "s_row": (res.s_row, int(res.n_matches))}
    return read_back, maps, lambda col: read_back("the map of a take")[:, 1 if col == "r_row" else 2]


def run_group(ctx, op, want, tag):
    ex, H, pool = ctx.ex, ctx.H, ctx.pool
    g = pool.groups[op["case"]]
    cols, vals, valid = ctx.dev("groups", op["case"])
    flags, ordered = op["flags"], bool(op["flags"] & ORDERED)
    exp = key_expectation(pool, op)
    before = (ex.last_plan(), ex.last_timing()["path"])
    call = lambda: ex.group_cols_device(cols, vals, valid, flags, op["want"], hash_bits=g["bits"], force_hashed=g["force"])
    if want["rc"] == E_UNSUPPORTED:
        expect_refused_by_cap(ctx, call, tag)
        return None
    res, info = call()
    assert (ex.last_plan(), ex.last_timing()["path"]) == before, (tag, "a group call leaves hmj_last_plan / hmj_last_timing as they were")
    if not flags:
        got = ex.group_rows_to_numpy(res)
        assert all(v is None for v in got.values()), tag
        assert (int(res.n_groups), int(res.n_rows), int(res.max_count)) == (exp["n_groups"], exp["n_rows"], exp["max_count"]), tag
        assert (info["form"], info["n_null"], info["n_collisions"]) == (exp["form"], exp["n_null"], exp["n_collisions"]), (tag, info)
        return None

    def read_back(why):
        got = ex.group_rows_to_numpy(res)
        check_groups(H, res, info, got, exp, ordered, (tag, why), op["want"])
        return got

    read_back("after the call")
    maps = {"first_row": (res.first_row, int(res.n_groups)), "group_of_row": (res.group_of_row, int(res.n_rows))}
    return read_back, maps, lambda col: read_back("the map of a take")[col]


# ---- the takes -------------------------------------------------------------------------------------------------------------------
def take_sources(ctx, src):
    """The device columns of a take's source relation (uploaded once)."""
    key = ("take",) + src
    if key not in ctx._dev:
        H = ctx.H
        (cols, masks, off), strs = ctx.pool.take_source(src)
        fixed = ([signed(c) for c in cols], dev_valid(H, masks, off))
        s = None
        if strs is not None:
            keys, mask, soff = strs
            s = (dev_str(keys), None if mask is None else (H.pack_validity(mask, soff, "cuda"), soff))
        ctx._dev[key] = (fixed, s)
    return ctx._dev[key]


def run_take(ctx, op, want, tag, index):
    ex, H, pool = ctx.ex, ctx.H, ctx.pool
    src = tuple(op["src"])
    fixed, strs = take_sources(ctx, src)
    before = (ex.last_plan(), ex.last_timing()["path"])
    if op["map"] is not None:  # through a row map of the op whose result is still there
        assert ctx.live is not None and ctx.live[0] == want["live"], (tag, "the drawing and the model disagree about the live result")
        read_back, maps, host_map = ctx.live[1]
        row_map, m = maps[op["map"]], host_map(op["map"])
        assert row_map[0] or not row_map[1], (tag, "the result has no such map")
    else:
        m = drawn_map(pool.seed + index, pool.n_src(src), op["n_out"])
        row_map = signed(m)
    if op["what"] == "take_cols":
        outs, words, info = ex.take_cols_device(fixed[0], row_map, valid=fixed[1])
        want_d, want_w, want_nulls, want_no = take_cols_expect(pool, src, m)
        for c, o in enumerate(outs):
            got = o.cpu().numpy()
            assert got.shape == want_d[c].shape and np.array_equal(got.reshape(-1).view(np.uint8), np.ascontiguousarray(want_d[c]).reshape(-1).view(np.uint8)), (tag, c)
            assert np.array_equal(words[c].cpu().numpy().view(np.uint64), want_w[c]), (tag, c, "validity words (padding bits included)")
        assert info["null_count"] == want_nulls and info["n_no_row"] == want_no, (tag, info, want_nulls, want_no)
    else:
        (chars, offsets), valid = strs
        co, oo, words, info = ex.take_str_device(chars, offsets, row_map, valid=valid)
        want_c, want_o, want_w, want_nulls, want_no, want_total = take_str_expect(pool, src, m)
        assert np.array_equal(oo.cpu().numpy().view(np.uint64), want_o), (tag, "offsets")
        assert np.array_equal(co.cpu().numpy(), want_c), (tag, "chars")
        assert np.array_equal(words.cpu().numpy().view(np.uint64), want_w), (tag, "validity words (padding bits included)")
        assert (info["null_count"], info["n_no_row"], info["total_bytes"]) == (want_nulls, want_no, want_total), (tag, info)
    assert (ex.last_plan(), ex.last_timing()["path"]) == before, (tag, "a take leaves hmj_last_plan / hmj_last_timing as they were")
    if ctx.live is not None:  # the earlier op's result must still equal its expectation
        assert want["live"] == ctx.live[0], tag
        ctx.live[1][0]("after a take")
        ctx.ledger["take_read_back"] += 1


# ---- refusals --------------------------------------------------------------------------------------------------------------------
REFUSAL_WORDS = {"width_3": "has width 3", "unknown_kind": "unknown join kind", "group_first_wins": "HMJ_FIRST_WINS is not defined for grouping",
                 "str_kind_null_equal": "HMJ_NULL_EQUAL is not taken by the string kinds", "take_map_beyond_source": "1 row_map entries",
                 "mixed_decreasing_offsets": "offsets decrease at row 2", "cols_run_cap_ordered": "more than 1024 rows",
                 "group_run_cap": "more than 1024 rows"}
assert set(REFUSAL_WORDS) == set(REFUSALS)


def run_refused(ctx, op):
    """The status of a call the library refuses: the header's documented refusals, none of which reads outside a buffer."""
    ex, H, L, which = ctx.ex, ctx.H, ctx.ex.L, op["which"]
    a = ctx.small
    try:
        if which == "width_3":
            ex._sync_stream()
            kc = (H.KeyCol * 1)()
            kc[0].data, kc[0].width = a.data_ptr(), 3
            rel = H.ColsRel()
            rel.cols, rel.n_cols, rel.n = kc, 1, 100
            opts = H.ColsJoinOpts()
            opts.struct_size = C.sizeof(H.ColsJoinOpts)
            return L.hmj_join_cols_device(ex.h, C.byref(rel), C.byref(rel), 0, C.byref(opts), C.byref(H.ColsResult()))
        if which == "unknown_kind":
            ex.join_kind_cols_device([a], None, [a], None, PROBE, 4, 0)
        elif which == "group_first_wins":
            ex.group_cols_device([a], flags=MATERIALIZE | FIRST_WINS)
        elif which == "str_kind_null_equal":
            B, P = ctx.dev("strs", 0)
            ex.join_kind_str_device(B[0], P[0], PROBE, SEMI, NULL_EQUAL)
        elif which == "take_map_beyond_source":
            m = ctx.torch.arange(50, dtype=ctx.torch.int64, device="cuda")
            m[7] = 100  # == n_src: found on the device, compared before anything is loaded through it
            ex.take_cols_device([a], m)
        elif which == "mixed_decreasing_offsets":
            ex.join_mixed_device([ctx.bad_str, a[:4]], None, [ctx.good_str, a[:4]], None, PROBE, INNER, ORDERED)
        elif which == "cols_run_cap_ordered":
            ex.join_cols_device(ctx.cap_cols[0], None, ctx.cap_cols[1], None, ORDERED, hash_bits=1)
        elif which == "group_run_cap":
            ex.group_cols_device(ctx.cap_group, flags=MATERIALIZE, hash_bits=1)
        else:
            raise ValueError(which)
    except H.HmjError as e:
        return e.code
    return 0


# ---- one op ----------------------------------------------------------------------------------------------------------------------
def note_sizes(ctx, kind, case):
    """(a property of the drawing: buffers only grow, so a case larger than every case its family ran before regrows them)"""
    size = ctx.pool.size_of(getattr(ctx.pool, kind)[case])
    ctx.ledger["regrew_" + kind] += 0 < ctx.largest[kind] < size
    ctx.largest[kind] = max(ctx.largest[kind], size)


def run_op(ctx, op, prev, tag, index):
    ex, H, pool = ctx.ex, ctx.H, ctx.pool
    discarded = ctx.model.discarded
    want = ctx.model.step(op)
    what = op["what"]
    live = None
    if what in KEY_FAMILIES or what == "group":
        kind = {"mixed": "mixed", "str_kind": "strs", "group": "groups"}.get(what, "cols")
        note_sizes(ctx, kind, op["case"])
        live = (run_group if what == "group" else run_key_join)(ctx, op, want, tag)
        if want["rc"] == 0 and what != "group":
            ctx.ledger["key_join_under_forced_bits"] += want["forced"] is not None
            ctx.ledger["key_join_under_prefix_hint"] += want["prefix"] is not None
        if what in ("cols_kind", "mixed", "group"):
            ctx.ledger["discarded_by_" + what] += ctx.model.discarded - discarded
            if prev is not None and prev["what"] == what:
                cases = getattr(pool, kind)
                ctx.ledger[what + "_after_larger"] += pool.size_of(cases[op["case"]]) < pool.size_of(cases[prev["case"]])
                had = cases[prev["case"]]["valid"] is not None if what == "group" else prev["sem"] != "plain"
                has = cases[op["case"]]["valid"] is not None if what == "group" else op["sem"] != "plain"
                ctx.ledger[what + "_after_bitmaps"] += had and not has
    elif what in ("take_cols", "take_str"):
        run_take(ctx, op, want, tag, index)
        live = ctx.live[1] if ctx.live is not None else None
    elif what == "u64":
        note_sizes(ctx, "u64", op["case"])
        ex.set_key_prefix_bits(-1)  # nothing was promised about these keys: automatic sampling
        if op["sub"] == "join":
            plan = check_inner(ctx, op, want, pool.expect_u64(op["case"]), tag)
            nb, npb = pool.u64[op["case"]]["rows"]
            if want["forced"] is not None and nb and npb:
                assert plan["radix_bits"] == want["forced"], (tag, "forced radix bits", want["forced"], plan)
            if plan["path"] & H.HMJ_PATH_PREPARED and ctx.prepared_at is not None:
                between = [o["what"] for o in ctx.prepared_at[1]]
                ctx.ledger["took_prepared_after_takes"] += between == ["take_cols", "take_str"]
        elif op["sub"] == "sort":
            a = ctx.dev(op["case"])[op["side"]]
            out = ex.sort_device(a.clone() if op["inplace"] else a, inplace=op["inplace"])
            assert np.array_equal(out.cpu().numpy().view(np.uint64), pool.expect_sorted(op["case"], op["side"])), tag
        else:
            ex.prepare_build(ctx.dev(op["case"])[0], op["hint"])
            ctx.prepared_at = (index, [])
    elif what == "config":
        action, value = op["action"], op["value"]
        ex.set_radix_bits(None)  # forced bits and a hint hold until the next configuration op
        ex.set_key_prefix_bits(-1)
        if action == "radix_bits":
            ex.set_radix_bits(value)
        elif action == "prefix_bits":
            ex.set_key_prefix_bits(value)
        elif action == "profiling":
            ex.set_profiling(value)
        elif action == "forget":
            ex.forget_workloads()
        elif action == "release":
            ex.release_result()
        else:
            ex.reserve(*value)
    elif what == "refused":
        rc = run_refused(ctx, op)
        assert rc == want["rc"], (tag, rc, want["rc"])
        msg = ex.L.hmj_last_error(ex.h).decode()
        assert REFUSAL_WORDS[op["which"]] in msg, (tag, "hmj_last_error after the refused call", msg)
    else:
        raise ValueError(what)
    if what not in ("take_cols", "take_str"):
        ctx.live = None if live is None else (index, live)
        assert (ctx.live is None) == (ctx.model.live is None) and (ctx.live is None or ctx.live[0] == ctx.model.live), (tag, "the live result")
    if ctx.prepared_at is not None and not (what == "u64" and op["sub"] == "prepare"):
        ctx.prepared_at[1].append(op)
        if what == "u64":
            ctx.prepared_at = None
    ctx.executed += 1


def dump_failure(ctx, ops, i, run):
    out = os.environ.get("HMJ_STRESS_DUMP")
    if out:
        with open(os.path.join(out, "fail_keyjoin_sequence.json"), "w") as f:
            json.dump({"seed": ctx.pool.seed, "run": run, "index": i, "ops": ops[:i + 1]}, f)


def run_tours(ctx, tours, label):
    for t, ops in enumerate(tours):
        ctx.drawn += 2 * len(ops)
        for rep in range(2):  # the second run meets the memos and cool-downs of the first
            ctx.ex.set_radix_bits(None)  # every tour was drawn from automatic planning
            ctx.ex.set_key_prefix_bits(-1)
            ctx.model = KeyModel()
            ctx.live = ctx.prepared_at = None
            t0 = time.perf_counter()
            for i, op in enumerate(ops):
                tag = (label, ctx.pool.seed, t, rep, i, json.dumps(op, sort_keys=True))
                try:
                    run_op(ctx, op, ops[i - 1] if i else None, tag, i)
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


def test_key_calls_on_one_context(ctx):
    _, seed, iters = stress_env()
    n_tours = int(iters) if iters else SEQ_TOURS
    rng = np.random.default_rng([seed, 13])
    t0 = time.perf_counter()
    tours = [draw_key_sequence(rng, ctx.pool) for _ in range(n_tours)]
    for ops in tours:
        assert transitions([op["fam"] for op in ops]) == {(x, y) for x in FAMILIES for y in FAMILIES}
    print("%d tours drawn in %.1f s" % (n_tours, time.perf_counter() - t0), flush=True)
    run_tours(ctx, tours, "key calls")
    assert ctx.executed == ctx.drawn == 2 * n_tours * (len(FAMILIES) ** 2 + 1)  # no op was skipped
    print("ledger:", ctx.ledger, flush=True)
    ctx.done = True


def test_the_tours_reached_the_states_they_are_for(ctx):
    """At least one of each: a u64 join that took a build side prepared before two takes; a prepared build side discarded by
    a group call, by a column kind join and by a mixed join; each of cols_kind, mixed and group directly after a larger
    case of its own family, and after a case with bitmaps when it has none; per family a case larger than every case the
    family had run before; a key join under forced bits and one under a prefix hint; a take that read back an earlier
    result.  The first is read from last_plan(); the others are properties of the drawn ops and the model."""
    assert ctx.done, "the tours did not finish"
    default, _, _ = stress_env()
    if default:
        missing = [k for k in LEDGER if not ctx.ledger[k]]
        assert not missing, (missing, ctx.ledger)


def lockstep_cases(pool):
    """Every pool case of the key-join and group families as one op each (the kind and mode that read the most back)."""
    fl = ORDERED | CHECKSUM
    for ci, c in enumerate(pool.cols):
        big = c["big"] is not None
        yield dict(what="cols_inner", case=ci, side=PROBE, kind=INNER, sem="plain", force=False, flags=fl)
        side, kind = (BUILD, FULL_OUTER)
        has = c["b"]["masks"] is not None or c["p"]["masks"] is not None
        yield dict(what="cols_kind", case=ci, side=side, kind=kind, sem="sql" if has else "plain", force=False, flags=fl)
        if has and not big:
            yield dict(what="cols_null_equal", case=ci, side=side, kind=kind, sem="ne", force=False, flags=fl)
    for mi, c in enumerate(pool.mixed):
        has = bool(c["b"]["bitmap"] or c["p"]["bitmap"])
        for sem in ("sql", "ne") if has else ("plain",):
            yield dict(what="mixed", case=mi, side=BUILD, kind=FULL_OUTER, sem=sem, flags=fl)
    for gi in range(len(pool.groups)):
        yield dict(what="group", case=gi, flags=ORDERED, want=0x1F)
    for si, c in enumerate(pool.strs):
        yield dict(what="str_kind", case=si, side=BUILD, kind=FULL_OUTER, bitmaps=c["bmask"] is not None, flags=fl)


def test_a_forgotten_context_joins_and_plans_like_a_new_one(ctx, H):
    assert ctx.done, "the tours did not finish"
    pool, toured = ctx.pool, ctx.ex
    toured.forget_workloads()
    toured.set_radix_bits(None)
    toured.set_key_prefix_bits(-1)
    fresh = H.Executor(0)
    try:
        for op in lockstep_cases(pool):
            exp = key_expectation(pool, op)
            op["over"] = bool(exp["over"])
            want = {"rc": E_UNSUPPORTED if exp["over"] else 0}
            plans = []
            for name, e in (("toured", toured), ("fresh", fresh)):
                ctx.ex = e
                try:
                    tag = ("lockstep", name, json.dumps(op, sort_keys=True))
                    (run_group if op["what"] == "group" else run_key_join)(ctx, op, want, tag)
                    plans.append({k: e.last_plan()[k] for k in PLAN_FIELDS})
                finally:
                    ctx.ex = toured
            if op["what"] != "group":  # (a group call leaves hmj_last_plan as it was)
                assert plans[0] == plans[1], (op, "plan", path_names(H, plans[0]["path"]), path_names(H, plans[1]["path"]), plans)
    finally:
        fresh.close()


# ---- a planner hint must not reach key64 -------------------------------------------------------------------------------------------
HINT_ROWS = (20000, 30000)


def hint_cases(H):
    """(name, call(ex, flags) -> (res, rows or None), ordered expectation) of the directed test."""
    import torch

    nb, npb = HINT_ROWS
    rng = np.random.default_rng(16)
    # unique build tuples (a, b, c), probe rows drawn from them, every second one changed to a tuple the build side lacks
    with np.errstate(over="ignore"):
        a = rng.permutation(nb).astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15)
    b = rng.integers(0, 1 << 32, nb, dtype=np.uint64).astype(np.uint32)
    c = rng.integers(0, 1 << 16, nb, dtype=np.uint64).astype(np.uint16)
    pick = rng.integers(0, nb, npb)
    pa, pb, pc = a[pick].copy(), b[pick].copy(), c[pick].copy()
    pb[::2] ^= np.uint32(0x80000000)
    bv, pv = rng.integers(0, 1 << 63, nb, dtype=np.uint64), rng.integers(0, 1 << 63, npb, dtype=np.uint64)
    hit = np.arange(npb) % 2 == 1
    b_hit = np.zeros(nb, bool)
    b_hit[pick[hit]] = True
    s_hit, s_miss, r_miss = np.flatnonzero(hit), np.flatnonzero(~hit), np.flatnonzero(~b_hit)
    u = lambda x: np.asarray(x).astype(np.uint64)
    fill = lambda k, v: np.full(k, v, np.uint64)
    by = lambda rows: np.ascontiguousarray(rows[np.lexsort((rows[:, 2], rows[:, 1], rows[:, 0]))])

    def numpy_rows(kb, kp, full):
        assert len(np.unique(kb)) == nb  # (no key64 collision among the build tuples: (key64, r_row, s_row) orders the rows)
        inner = np.stack([kp[s_hit], u(pick[s_hit]), u(s_hit), bv[pick[s_hit]], pv[s_hit]], 1)
        if not full:
            return by(inner)
        return by(np.concatenate([inner, np.stack([kp[s_miss], fill(len(s_miss), NO_ROW), u(s_miss), fill(len(s_miss), PFILL), pv[s_miss]], 1),
                                  np.stack([kb[r_miss], u(r_miss), fill(len(r_miss), NO_ROW), bv[r_miss], fill(len(r_miss), BFILL)], 1)]))

    cases = []
    w3, w2 = [8, 4, 2], [4, 4]
    B3, P3 = ([signed(x) for x in (a, b, c)], signed(bv)), ([signed(x) for x in (pa, pb, pc)], signed(pv))
    kb3, kp3 = H.cols_key64([a, b, c], w3), H.cols_key64([pa, pb, pc], w3)
    rows_of = lambda ex, res, fl: ex.cols_kind_rows_to_numpy(res) if materialising(fl) else None
    cases.append(("hashed [8,4,2] inner", lambda ex, fl: (lambda r: (r[0], rows_of(ex, r[0], fl)))(
        ex.join_cols_device(B3[0], B3[1], P3[0], P3[1], fl)), numpy_rows(kb3, kp3, False)))
    cases.append(("hashed [8,4,2] FULL_OUTER", lambda ex, fl: (lambda r: (r[0], rows_of(ex, r[0], fl)))(
        ex.join_kind_cols_device(B3[0], B3[1], P3[0], P3[1], BUILD, FULL_OUTER, fl, probe_fill=PFILL, build_fill=BFILL)), numpy_rows(kb3, kp3, True)))
    a32, pa32 = a.astype(np.uint32), pa.astype(np.uint32)  # (an odd factor: distinct low halves that fill all 32 bits)
    assert len(np.unique(a32)) == nb and int(a32.max()) >> 31 == 1
    B2, P2 = ([signed(a32), signed(b)], B3[1]), ([signed(pa32), signed(pb)], P3[1])
    kb2, kp2 = H.cols_key64([a32, b], w2), H.cols_key64([pa32, pb], w2)
    cases.append(("packed [4,4] inner", lambda ex, fl: (lambda r: (r[0], rows_of(ex, r[0], fl)))(
        ex.join_cols_device(B2[0], B2[1], P2[0], P2[1], fl)), numpy_rows(kb2, kp2, False)))
    # strings: one key per build tuple, the probe side's misses spelled differently
    bk = [b"name-%016x" % int(x) for x in a]
    pk = [b"name-%016x" % int(x) if h else b"none-%016x" % int(x) for x, h in zip(pa, hit)]
    bvl, pvl = [int(x) for x in bv], [int(x) for x in pv]
    SB, SP = str_rel(H, bk, bvl, 3, 5), str_rel(H, pk, pvl)
    want_s, _ = kind_brute(bk, bvl, pk, pvl, BUILD, FULL_OUTER, 0, PFILL, BFILL)
    cases.append(("string FULL_OUTER", lambda ex, fl: (lambda r: (r[0], ex.str_kind_rows_to_numpy(r[0]) if materialising(fl) else None))(
        ex.join_kind_str_device(SB, SP, BUILD, FULL_OUTER, fl, probe_fill=PFILL, build_fill=BFILL)), want_s))
    MB, MP = MixedRel([bk, b], bvl), MixedRel([pk, pb], pvl)
    want_m = mixed_expect(H, MB, MP, PROBE, INNER)[0]
    DB, DP = ([dev_str(bk), signed(b)], signed(bv)), ([dev_str(pk), signed(pb)], signed(pv))
    cases.append(("mixed [s,4] inner", lambda ex, fl: (lambda r: (r[0], rows_of(ex, r[0], fl)))(
        ex.join_mixed_device(DB[0], DB[1], DP[0], DP[1], PROBE, INNER, fl)), want_m))
    return cases


def test_a_planner_hint_does_not_reach_key64(H):
    """hmj_set_key_prefix_bits promises top bits the CALLER'S u64 keys share.  The hashed column, string and mixed joins run
    their internal ordered u64 join on key64 -- hash values, or a packed tuple that fills all 64 bits --, about which nobody
    promised anything: under a hint the partitions of that join would stop being key ranges and nothing would sort the
    result again.  Each case runs ordered and as a plain count with automatic sampling (and must equal its numpy or tuple
    expectation, with more than one partition: HMJ_GTABLE=0 makes these sizes partition), then again under hints of 1, 16
    and 48 bits and under 1 and 14 forced radix bits: the rows as a sequence and all checks must be those of the first run.
    The entries do not consume the hint: a u64 join whose keys share h top bits still reports key_prefix_bits == h."""
    os.environ["HMJ_GTABLE"] = "0"
    try:
        ex = H.Executor(0)
    finally:
        del os.environ["HMJ_GTABLE"]
    try:
        fl = ORDERED | CHECKSUM
        rng = np.random.default_rng(5)
        u64 = {}
        for h in (1, 16, 48):  # 40 000 distinct keys that truly share their h top bits (all ones) and vary in the bit below them
            low = rng.permutation(1 << 16)[:40000].astype(np.uint64) if h == 48 else rng.integers(0, 1 << (64 - h), size=40000, dtype=np.uint64)
            k = low | np.uint64(((1 << h) - 1) << (64 - h))
            assert len(np.unique(k)) == len(k) and len(np.unique(k >> np.uint64(63 - h))) == 2
            rel = np.stack([k, np.arange(len(k), dtype=np.uint64)], 1)
            u64[h] = (to_dev(rel[:15000]), to_dev(rel[10000:]))  # 5000 rows in common
        for name, call, want in hint_cases(H):
            ex.set_key_prefix_bits(-1)
            ex.set_radix_bits(None)
            res, rows = call(ex, fl)
            plan = ex.last_plan()
            first = (res.checks(), rows)
            ck = (tmix_checks if name.startswith("string") else kind_checks)(want)
            assert first[0] == ck and rows.shape == want.shape, (name, "automatic sampling", first[0], ck)
            assert np.array_equal(rows, want), (name, "automatic sampling", np.flatnonzero(np.any(rows != want, axis=1))[:5])
            assert plan["n_partitions"] > 1, (name, "the internal join did not partition: the test would show nothing", plan)
            count = call(ex, 0)[0].checks()
            assert [count[k] for k in ("n_matches", "sum_r", "sum_s")] == [ck[k] for k in ("n_matches", "sum_r", "sum_s")], name
            for setter, values in (("set_key_prefix_bits", (1, 16, 48)), ("set_radix_bits", (1, 14))):
                for v in values:
                    getattr(ex, setter)(v)
                    try:
                        res, rows = call(ex, fl)
                        assert res.checks() == first[0], (name, setter, v, res.checks(), first[0])
                        bad = np.flatnonzero(np.any(rows != first[1], axis=1)) if rows.shape == first[1].shape else None
                        assert bad is not None and not len(bad), (name, setter, v, "rows differ from the run without it", None if bad is None else bad[:5])
                        assert call(ex, 0)[0].checks() == count, (name, setter, v, "plain count")
                        if setter == "set_key_prefix_bits":  # the hint is still the caller's
                            r = ex.join_device(u64[v][0], u64[v][1], fl)
                            assert int(r.n_matches) == 5000 and ex.last_plan()["key_prefix_bits"] == v, (name, v, ex.last_plan())
                    finally:
                        ex.set_key_prefix_bits(-1)
                        ex.set_radix_bits(None)
    finally:
        ex.close()
