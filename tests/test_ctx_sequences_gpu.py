"""One long-lived context under drawn sequences of mixed calls (the generators, the model of the contract and their CPU
checks are test_ctx_sequences_cpu.py's).

  * test_mixed_calls_on_one_context: one Executor, the default number of tours over the twelve op families, each tour run
    twice in a row, so that the second run meets warm memos and active cool-downs.  After every op the status, count, sums,
    checksums, sum_probe_all, counters, the columns that exist and the rows (a sequence under HMJ_ORDERED, a sorted multiset
    otherwise) are compared exactly; after a refused call hmj_last_error names that refusal and the next op must be right;
    the forced radix bits are those of the model; an inner join reports HMJ_PATH_PREPARED only where the model allows it;
  * test_the_tours_reached_the_states_they_are_for: the ledger of the default seed;
  * test_the_setters_say_why_they_refuse: the directed case of the library fix the tours led to;
  * test_a_forgotten_context_plans_like_a_new_one: after the tours and hmj_forget_workloads, every u64 pool case plans and
    joins as on a fresh Executor;
  * test_mixed_calls_on_a_context_with_a_communicator: one rank over RCCL self send / recv, one tour over eight families:
    what an exchange step leaves behind does not reach the plain calls that follow.

Every call runs on torch's current stream and every result is read back right after its call.  HMJ_STRESS_SEED /
HMJ_STRESS_ITERS (tours) override the defaults; HMJ_STRESS_DUMP=dir keeps the failing op's index, its relations and the ops
up to it."""
import ctypes as C
import json
import os
import time

import numpy as np
import pytest

from test_ctx_sequences_cpu import (CHECKSUM, FAMILIES, MATERIALIZE, ORDERED, OVERSIZED, SEQ_SEED, SEQ_TOURS, SUM_PROBE, Model, Pool,
                                    draw_sequence, draw_tour, expectation, materialising, transitions, u64_case_of)
from test_exchange_kinds_gpu import BUILD_FILL, KINDS, PROBE_FILL, PSIDE, fast_expected, gen_pair
from test_join_str_cpu import M64
from test_join_str_gpu import brute, checks_of, rel, unordered
from test_join_str_kinds_cpu import ANTI as S_ANTI, BUILD as S_BUILD, PROBE as S_PROBE, SEMI as S_SEMI, tmix_checks
from test_kinds_sweep_cpu import VARIANTS, draw_str_case
from test_kinds_sweep_gpu import check_variant, path_names, sort_rows, to_dev

pytestmark = pytest.mark.gpu
PLAN_FIELDS = ("path", "radix_bits", "radix_passes", "pass_bits", "key_prefix_bits", "key_window_low", "n_partitions",
               "probe_items", "attempts", "refused", "cooling")
LEDGER = ("took_prepared", "prepare_discarded", "cooling", "replanned", "slab", "global_table", "str_kind_after_larger", "regrew")


@pytest.fixture(scope="module")
def H():
    import hashmergejoin_amd as H

    return H


def stress_env():
    default = "HMJ_STRESS_ITERS" not in os.environ and "HMJ_STRESS_SEED" not in os.environ
    return default, int(os.environ.get("HMJ_STRESS_SEED", SEQ_SEED)), os.environ.get("HMJ_STRESS_ITERS")


class Ctx:
    """The executor under test with the pool's relations on the device, the model and the ledger."""

    def __init__(self, H, seed):
        import torch

        assert torch.cuda.is_available(), "GPU tests need a GPU"
        self.H, self.torch = H, torch
        self.ex = H.Executor(0)
        self.pool = Pool(seed)
        self.model = Model()
        self.ledger = dict.fromkeys(LEDGER, 0)
        self.executed = self.drawn = 0
        self.largest_rows = 0  # of the u64 relations any call has read so far
        self.done = False
        self._dev, self._sdev = {}, {}
        keys = [b"aa", b"bb", b"cc", b"dd"]  # the relation with decreasing offsets (test_join_str_gpu.test_errors_...)
        self.good_str = rel(H, keys, [1, 2, 3, 4])
        bad = self.good_str[1].clone()
        bad[3] = 1
        self.bad_str = (self.good_str[0], bad, self.good_str[2])
        o = OVERSIZED
        self.oversized = (rel(H, o["bk"], o["bv"]), rel(H, o["pk"], o["pv"]))

    def dev(self, ci):
        if ci not in self._dev:
            B, P = self.pool.relations(ci)
            self._dev[ci] = (to_dev(B), to_dev(P))
        return self._dev[ci]

    def sdev(self, si):
        if si not in self._sdev:
            c = self.pool.strs[si]
            self._sdev[si] = (rel(self.H, c["bk"], c["bv"], c["shift_b"], c["base_b"]), rel(self.H, c["pk"], c["pv"], c["shift_p"], c["base_p"]))
        return self._sdev[si]

    def close(self):
        self.ex.close()


def note_plan(ctx, plan):
    H, led = ctx.H, ctx.ledger
    led["cooling"] += plan["cooling"] != 0
    led["replanned"] += plan["attempts"] > 1
    led["slab"] += bool(plan["path"] & H.HMJ_PATH_SLAB)
    led["global_table"] += bool(plan["path"] & H.HMJ_PATH_GLOBAL_TABLE)


def check_inner(ctx, op, want, exp, tag, host=False):
    """The inner join (device or host entry) against its expectation; returns last_plan()."""
    ex, H, flags = ctx.ex, ctx.H, op["flags"]
    rows, ck, _ = exp
    B, P = ctx.pool.relations(op["case"])
    if host:
        r = ex.join_host(B, P, flags)
    else:
        bd, pd = ctx.dev(op["case"])
        r = ex.join_device(bd, pd, flags)
    plan = ex.last_plan()
    assert (int(r.n_matches), int(r.sum_r), int(r.sum_s)) == (ck["n_matches"], ck["sum_r"], ck["sum_s"]), tag
    if flags & CHECKSUM:
        assert r.checks() == ck, tag
    if flags & SUM_PROBE:
        assert int(r.sum_probe_all) == int(P[:, 1].sum(dtype=np.uint64)), tag
    if materialising(flags):
        got = ex.columns_to_numpy(r, host=host)
        assert got.shape == rows.shape, (tag, got.shape, rows.shape)
        if len(rows):
            assert r.key and r.rval and r.sval, tag
        if flags & ORDERED:
            assert np.array_equal(got, rows), (tag, np.flatnonzero(np.any(got != rows, axis=1))[:5])
        else:
            assert np.array_equal(sort_rows(got), rows), tag
    took = bool(plan["path"] & H.HMJ_PATH_PREPARED)
    assert not took or want["may_prepared"], (tag, "HMJ_PATH_PREPARED without a live prepared build side", path_names(H, plan["path"]))
    ctx.ledger["took_prepared"] += took
    return plan


def check_forced(ctx, op, want, plan, tag):
    nb, npb = ctx.pool.u64[op["case"]]["rows"]
    if want["forced"] is not None and nb and npb:
        assert plan["radix_bits"] == want["forced"], (tag, "forced radix bits", want["forced"], plan)


def run_u64_join(ctx, op, want, tag):
    """A `join` or `kind` op."""
    H, pool = ctx.H, ctx.pool
    exp = expectation(pool, op)
    if op["what"] == "join":
        plan = check_inner(ctx, op, want, exp, tag)
    else:
        B, P = pool.relations(op["case"])
        bd, pd = ctx.dev(op["case"])
        plan = check_variant(ctx.ex, H, B, P, bd, pd, VARIANTS[op["variant"]], op["flags"], pool.u64[op["case"]]["fills"], tag, want=exp)
        assert not plan["path"] & H.HMJ_PATH_PREPARED, (tag, "a kind join took a prepared build side")
    check_forced(ctx, op, want, plan, tag)
    note_plan(ctx, plan)


def check_str_rows(ctx, res, flags, rows, pv, tag, kind_form):
    ex = ctx.ex
    ck = tmix_checks(rows) if kind_form else checks_of(rows)
    got_ck = res.checks()
    if flags & CHECKSUM:
        assert got_ck == ck, tag
    else:
        assert (got_ck["n_matches"], got_ck["sum_r"], got_ck["sum_s"]) == (ck["n_matches"], ck["sum_r"], ck["sum_s"]), tag
    if flags & SUM_PROBE:
        assert int(res.sum_probe_all) == sum(pv) & M64, tag
    if materialising(flags):
        got = ex.str_kind_rows_to_numpy(res) if kind_form else ex.str_rows_to_numpy(res)
        assert got.shape == rows.shape, (tag, got.shape, rows.shape)
        if flags & ORDERED:
            assert np.array_equal(got, rows), tag
        else:
            assert np.array_equal(unordered(got), unordered(rows)), tag
    else:
        assert not res.hash, tag


def run_str(ctx, op, tag):
    ex, pool = ctx.ex, ctx.pool
    c = pool.strs[op["case"]]
    B, P = ctx.sdev(op["case"])
    flags = op["flags"]
    if op["what"] == "str_join":
        rows, cnt = expectation(pool, op)
        res, info = ex.join_str_device(B, P, flags, hash_bits=op["bits"])
        assert {k: info[k] for k in cnt} == cnt, (tag, info, cnt)
        check_str_rows(ctx, res, flags, rows, c["pv"], tag, False)
        if materialising(flags) and len(rows):
            assert res.hash and res.r_row and res.s_row and res.rval and res.sval, tag
    else:
        side, kind = op["side"], op["kind"]
        rows, cnt = expectation(pool, op)
        pf, bf = pool.str_fills(op["case"])
        res, info = ex.join_kind_str_device(B, P, side, kind, flags, hash_bits=c["hash_bits"], probe_fill=pf, build_fill=bf)
        assert {k: info[k] for k in cnt} == cnt, (tag, info, cnt)
        check_str_rows(ctx, res, flags, rows, c["pv"], tag, True)
        if materialising(flags) and len(rows):
            semi_anti = kind in (S_SEMI, S_ANTI)
            assert res.hash and bool(res.r_row) == bool(res.rval) == (not semi_anti or side == S_BUILD), tag
            assert bool(res.s_row) == bool(res.sval) == (not semi_anti or side == S_PROBE), tag
    note_plan(ctx, ex.last_plan())


def raw_kind(ctx, family, bptr, nb, pptr, npb, flags, kind, size=None):
    ex, H = ctx.ex, ctx.H
    ex._sync_stream()
    res = H.JoinResult()
    opts, fn = (H.JoinOpts(), ex.L.hmj_join_kind_u64_device) if family == "probe" else (H.BuildJoinOpts(), ex.L.hmj_join_build_kind_u64_device)
    opts.struct_size = C.sizeof(type(opts)) if size is None else size
    opts.kind = kind
    return fn(ex.h, C.c_void_p(bptr), nb, C.c_void_p(pptr), npb, flags, C.byref(opts), C.byref(res))


def run_refused(ctx, op):
    """The status of a call the library refuses.  Each is taken from an error test of its entry; none reads a row."""
    ex, H, torch = ctx.ex, ctx.H, ctx.torch
    L, which, entry = ex.L, op["which"], op["entry"]
    if which == "radix_bits_40":
        return L.hmj_set_radix_bits(ex.h, 40)
    if which in ("decreasing_offsets", "oversized_mixed_run"):
        try:
            if which == "oversized_mixed_run":
                ex.join_str_device(ctx.oversized[0], ctx.oversized[1], ORDERED, hash_bits=OVERSIZED["hash_bits"])
            elif op["str_entry"] == "str_join":
                ex.join_str_device(ctx.bad_str, ctx.good_str, ORDERED)
            elif op["str_entry"] == "str_kind":
                ex.join_kind_str_device(ctx.good_str, ctx.bad_str, S_PROBE, S_ANTI, 0)
            else:
                ex.hash_str_device(ctx.bad_str[0], ctx.bad_str[1])
        except H.HmjError as e:
            return e.code
        return 0
    bd, pd = ctx.dev(op["case"])
    bptr, nb, pptr, npb = bd.data_ptr(), bd.shape[0], pd.data_ptr(), pd.shape[0]
    family = "build" if entry == "build_kind" else "probe"
    kind = {"probe": H.HMJ_JOIN_SEMI, "build": H.HMJ_BUILD_SEMI}[family]
    if which == "partition_bits_10":
        out = torch.empty_like(bd)
        off = torch.empty(1025, dtype=torch.int64, device="cuda")
        ex._sync_stream()
        return L.hmj_partition_u64_device(ex.h, C.c_void_p(bptr), nb, 0, 10, C.c_void_p(out.data_ptr()), C.c_void_p(off.data_ptr()))
    if which == "unknown_kind":
        return raw_kind(ctx, family, bptr, nb, pptr, npb, 0, 4 if family == "probe" else 5)
    if which == "struct_too_small":
        return raw_kind(ctx, family, bptr, nb, pptr, npb, 0, H.HMJ_JOIN_SEMI if family == "probe" else H.HMJ_FULL_OUTER, size=8)
    if which == "first_wins_outer":
        return raw_kind(ctx, "build", bptr, nb, pptr, npb, H.HMJ_FIRST_WINS, op["kind"])
    if which == "too_many_rows":
        nb = (1 << 32) + 5  # refused by the row count, before any row is read
    elif which == "null_relation":
        if op["null_side"] == 0:
            bptr = None
        else:
            pptr = None
    else:
        raise ValueError(which)
    if entry == "inner":
        ex._sync_stream()
        res = H.JoinResult()
        return L.hmj_join_u64_device(ex.h, C.c_void_p(bptr), nb, C.c_void_p(pptr), npb, 0, C.byref(res))
    return raw_kind(ctx, family, bptr, nb, pptr, npb, CHECKSUM, kind)


def refusal_message(op):
    """What hmj_last_error must say after the refused call: the words of THIS refusal.  (The string is never cleared, so
    "not empty" would hold after the first refusal on the context whatever a later one left; consecutive refusals of a tour
    are of different kinds.)"""
    which, kinds = op["which"], op["entry"] != "inner"
    return {"unknown_kind": "unknown", "struct_too_small": "struct_size too small", "first_wins_outer": "HMJ_FIRST_WINS",
            "too_many_rows": "too many rows" if kinds else "more than 2^32-1 rows",
            "null_relation": ("build_aos" if op["null_side"] == 0 else "probe_aos") + " is NULL",
            "partition_bits_10": "bits must be in 1..9", "radix_bits_40": "at most 27",
            "decreasing_offsets": "offsets decrease at row 2", "oversized_mixed_run": "more than 1024 rows"}[which]


def run_op(ctx, op, prev, tag):
    ex, H, pool, torch = ctx.ex, ctx.H, ctx.pool, ctx.torch
    want = ctx.model.step(op)
    what = op["what"]
    ci = u64_case_of(op)
    if ci is not None and what != "refused":
        rows = max(pool.u64[ci]["rows"])
        # (a property of the drawing, not something the context reports: its buffers only grow, so a call on larger
        #  relations than any before it, after smaller ones, has to regrow them)
        ctx.ledger["regrew"] += 0 < ctx.largest_rows < rows
        ctx.largest_rows = max(ctx.largest_rows, rows)
    if what in ("join", "kind"):
        run_u64_join(ctx, op, want, tag)
    elif what == "prefix":
        ex.set_key_prefix_bits(op["bits"])  # the caller's promise, around exactly one join
        try:
            run_u64_join(ctx, op["inner"], want, tag)
        finally:
            ex.set_key_prefix_bits(-1)
    elif what in ("str_join", "str_kind"):
        run_str(ctx, op, tag)
        if what == "str_kind" and prev is not None and prev["what"] == "str_kind":
            a, b = pool.strs[prev["case"]], pool.strs[op["case"]]
            ctx.ledger["str_kind_after_larger"] += len(b["bk"]) + len(b["pk"]) < len(a["bk"]) + len(a["pk"])
    elif what == "sort":
        a = ctx.dev(op["case"])[op["side"]]
        out = ex.sort_device(a.clone() if op["inplace"] else a, inplace=op["inplace"])
        assert np.array_equal(out.cpu().numpy().view(np.uint64), expectation(pool, op)[0]), tag
    elif what == "partition":
        a = ctx.dev(op["case"])[op["side"]]
        out, off = ex.partition_device(a, op["shift"], op["bits"])
        ref, roff = expectation(pool, op)
        assert np.array_equal(off.cpu().numpy(), roff), tag
        assert np.array_equal(out.cpu().numpy().view(np.uint64), ref), tag
    elif what == "prepare":
        ex.prepare_build(ctx.dev(op["case"])[0], op["hint"])
    elif what == "host":
        note_plan(ctx, check_inner(ctx, op, want, expectation(pool, op), tag, host=True))
    elif what == "hash_str":
        chars, offs, _ = ctx.sdev(op["case"])[op["side"]]
        got = ex.hash_str_device(chars, offs, hash_bits=op["bits"]).cpu().numpy().view(np.uint64)
        assert np.array_equal(got, expectation(pool, op)[0]), tag
    elif what == "config":
        action, value = op["action"], op["value"]
        if action == "radix_bits":
            ex.set_radix_bits(value)
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
        assert refusal_message(op) in msg, (tag, "hmj_last_error after the refused call", msg)
    else:
        raise ValueError(what)
    ctx.ledger["prepare_discarded"] = ctx.model.discarded
    ctx.executed += 1


def dump_failure(ctx, ops, i, run):
    out = os.environ.get("HMJ_STRESS_DUMP")
    if not out:
        return
    op = ops[i]
    with open(os.path.join(out, "fail_ctx_sequence.json"), "w") as f:
        json.dump({"seed": ctx.pool.seed, "run": run, "index": i, "ops": ops[:i + 1]}, f)
    ci = u64_case_of(op)
    if ci is not None:
        B, P = ctx.pool.relations(ci)
        np.save(os.path.join(out, "fail_ctx_B.npy"), B)
        np.save(os.path.join(out, "fail_ctx_P.npy"), P)
    elif op["what"] in ("str_join", "str_kind", "hash_str"):
        c = ctx.pool.strs[op["case"]]
        with open(os.path.join(out, "fail_ctx_str.json"), "w") as f:
            json.dump({k: [x.hex() for x in c[k]] if k in ("bk", "pk") else c[k] for k in ("bk", "bv", "pk", "pv", "hash_bits")}, f)


def run_tours(ctx, tours, label):
    for t, ops in enumerate(tours):
        ctx.drawn += 2 * len(ops)
        for rep in range(2):  # the second run meets the memos and cool-downs of the first
            ctx.ex.set_radix_bits(None)  # every tour was drawn from automatic planning
            ctx.model.forced = None
            t0 = time.perf_counter()
            for i, op in enumerate(ops):
                tag = (label, ctx.pool.seed, t, rep, i, json.dumps(op, sort_keys=True))
                try:
                    run_op(ctx, op, ops[i - 1] if i else None, tag)
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


def test_mixed_calls_on_one_context(ctx):
    _, seed, iters = stress_env()
    n_tours = int(iters) if iters else SEQ_TOURS
    rng = np.random.default_rng([seed, 3])
    t0 = time.perf_counter()
    tours = [draw_sequence(rng, FAMILIES, ctx.pool) for _ in range(n_tours)]
    for ops in tours:
        fams = [op["fam"] for op in ops]
        assert transitions(fams) == {(x, y) for x in FAMILIES for y in FAMILIES}
    print("pool and %d tours drawn in %.1f s" % (n_tours, time.perf_counter() - t0), flush=True)
    run_tours(ctx, tours, "mixed calls")
    assert ctx.executed == ctx.drawn == 2 * n_tours * (len(FAMILIES) ** 2 + 1)  # no op was skipped
    print("ledger:", ctx.ledger, "prepared build sides discarded (model):", ctx.model.discarded, flush=True)
    ctx.done = True


def test_the_tours_reached_the_states_they_are_for(ctx):
    """At least one of each: a join that took the prepared build side, a prepare discarded by an intervening call, a join
    that left a cool-down, a join that planned again, slab partitioning, the global table, a string kind join directly
    after a larger one, a call that regrew buffers smaller calls had used.  The first six are read from last_plan(); the
    last two are properties of the drawn ops (sizes of consecutive string cases; a u64 call on larger relations than every
    call before it, which grow-only buffers must regrow): they say the tours were drawn as intended."""
    assert ctx.done, "the tours did not finish"
    default, _, _ = stress_env()
    if default:
        missing = [k for k in LEDGER if not ctx.ledger[k]]
        assert not missing, (missing, ctx.ledger)


def test_a_forgotten_context_plans_like_a_new_one(ctx, H):
    assert ctx.done, "the tours did not finish"
    ex, pool = ctx.ex, ctx.pool
    ex.forget_workloads()
    ex.set_radix_bits(None)
    ex.set_key_prefix_bits(-1)
    fresh = H.Executor(0)
    try:
        for ci, c in enumerate(pool.u64):
            bd, pd = ctx.dev(ci)
            exp = pool.expect_u64(ci, "inner")
            for flags in ((0, CHECKSUM) if c["big"] else (0, MATERIALIZE | CHECKSUM, ORDERED | CHECKSUM)):
                got = []
                for e in (ex, fresh):
                    r = e.join_device(bd, pd, flags)
                    plan = e.last_plan()
                    rows = e.columns_to_numpy(r, host=False) if materialising(flags) else None
                    got.append(({k: plan[k] for k in PLAN_FIELDS}, r.checks() if flags & CHECKSUM else
                                (int(r.n_matches), int(r.sum_r), int(r.sum_s)), rows))
                tag = (ci, c["tag"], flags)
                assert got[0][0] == got[1][0], (tag, "plan", path_names(H, got[0][0]["path"]), path_names(H, got[1][0]["path"]), got[0][0], got[1][0])
                assert got[0][1] == got[1][1] == (exp[1] if flags & CHECKSUM else tuple(exp[1][k] for k in ("n_matches", "sum_r", "sum_s"))), tag
                if flags & ORDERED:
                    assert np.array_equal(got[0][2], exp[0]) and np.array_equal(got[1][2], exp[0]), tag
                elif flags & MATERIALIZE:
                    assert np.array_equal(sort_rows(got[0][2]), exp[0]) and np.array_equal(sort_rows(got[1][2]), exp[0]), tag
    finally:
        fresh.close()


def test_the_setters_say_why_they_refuse(H):
    """hmj_set_radix_bits and hmj_set_key_prefix_bits returned HMJ_E_ARG for an out-of-range value without a word in
    hmj_last_error (the refused calls of the tours found the first).  On a fresh context, where no earlier refusal can have
    left a message; a refused value changes nothing."""
    ex = H.Executor(0)
    try:
        L = ex.L
        assert L.hmj_last_error(ex.h) == b""
        assert L.hmj_set_radix_bits(ex.h, 40) == -1 and b"at most 27" in L.hmj_last_error(ex.h)
        assert L.hmj_set_key_prefix_bits(ex.h, 60) == -1 and b"-1..48" in L.hmj_last_error(ex.h)
        assert L.hmj_set_radix_bits(ex.h, 28) == -1 and b"at most 27" in L.hmj_last_error(ex.h)
        assert L.hmj_set_key_prefix_bits(ex.h, -2) == -1 and b"-1..48" in L.hmj_last_error(ex.h)
        bd, pd = ex.gen_build(300000), ex.gen_probe(200000, 300000, miss_mod=4)
        ex.set_radix_bits(6)
        assert L.hmj_set_radix_bits(ex.h, 40) == -1  # the forced bits stay
        r = ex.join_device(bd, pd, H.HMJ_MATERIALIZE)
        assert int(r.n_matches) == 150000 and ex.last_plan()["radix_bits"] == 6
        assert L.hmj_set_radix_bits(ex.h, 27) == 0 and L.hmj_set_radix_bits(ex.h, -1) == 0
        assert L.hmj_set_key_prefix_bits(ex.h, 48) == 0 and L.hmj_set_key_prefix_bits(ex.h, -1) == 0
    finally:
        ex.close()


# ---- a context with a communicator ---------------------------------------------------------------------------------------
COMM_FAMILIES = ("exchange_inner", "exchange_kind", "inner", "kind", "str_join", "sort", "prepare_join", "message_bytes")
COMM_LOG2 = (20, 21, 22)
COMM_MESSAGES = ((1 << 22, 1 << 19), (1 << 21, 1 << 18), (1 << 24, 1 << 21), (0, 0))


def test_mixed_calls_on_a_context_with_a_communicator(H):
    """The executor of test_exchange_kinds_gpu's ex1 fixture (one rank, RCCL self exchange) under one tour over eight families.
    The arrival events, min_prefix_bits, sample_build_only and the host wait of an exchange step must not reach the plain
    calls: their results are fast_expected's, and a plain count join plans its partitions as on an executor without a
    communicator."""
    from hashmergejoin_amd import dist as hdist

    _, seed, iters = stress_env()
    rng = np.random.default_rng([seed, 4])
    ex = H.Executor(0)
    plain = H.Executor(0)
    try:
        hdist.init_comm_single(ex, self_exchange=True, timeout_s=120.0)
        rels = {}
        for log2n in COMM_LOG2:
            bd, pd = gen_pair(ex, 1 << log2n)
            B, P = bd.cpu().numpy().view(np.uint64), pd.cpu().numpy().view(np.uint64)
            rels[log2n] = dict(bd=bd, pd=pd, B=B, P=P, cache={}, sorted=None, plans={})
        srng = np.random.default_rng([seed, 5])
        strs = [draw_str_case(srng, sizes=(200, 1500)) for _ in range(2)]
        for c in strs:
            c["dev"] = (rel(H, c["bk"], c["bv"], c["shift_b"], c["base_b"]), rel(H, c["pk"], c["pv"], c["shift_p"], c["base_p"]))
            c["want"] = brute(c["bk"], c["bv"], c["pk"], c["pv"], c["hash_bits"])
        executed = drawn = 0
        for t in range(int(iters) if iters else 1):
            tour = draw_tour(rng, COMM_FAMILIES)
            assert transitions(tour) == {(x, y) for x in COMM_FAMILIES for y in COMM_FAMILIES}
            drawn += len(tour)
            t0 = time.perf_counter()
            for i, fam in enumerate(tour):
                R = rels[int(rng.choice(COMM_LOG2))]
                bd, pd, B, P = R["bd"], R["pd"], R["B"], R["P"]
                flags = int(rng.choice([0, CHECKSUM]))
                kname, side, kind = KINDS[int(rng.integers(0, len(KINDS)))]
                tag = (seed, t, i, fam, len(B), flags, kname)

                def same(res, ck):
                    if flags & CHECKSUM:
                        assert res.checks() == ck, tag
                    else:
                        assert (int(res.n_matches), int(res.sum_r), int(res.sum_s)) == (ck["n_matches"], ck["sum_r"], ck["sum_s"]), tag

                inner_ck = fast_expected(B, P, PSIDE, 0, R["cache"])[0]
                if fam == "exchange_inner":
                    loc, glob = ex.exchange_join(bd, pd, flags)
                    same(glob, inner_ck)
                    same(loc, inner_ck)
                elif fam == "exchange_kind":
                    ck, cnt = fast_expected(B, P, side, kind, R["cache"])
                    loc, glob, got = ex.exchange_join_kind(bd, pd, side, kind, flags, probe_fill=PROBE_FILL, build_fill=BUILD_FILL)
                    same(glob, ck)
                    assert got["global"] == got["local"] == cnt, (tag, got, cnt)
                elif fam == "inner":
                    same(ex.join_device(bd, pd, flags), inner_ck)
                    plan = ex.last_plan()
                    assert not plan["path"] & H.HMJ_PATH_PREPARED, tag
                    key = flags
                    if key not in R["plans"]:  # the same join on an executor that never had a communicator
                        same(plain.join_device(bd, pd, flags), inner_ck)
                        R["plans"][key] = plain.last_plan()
                    for k in ("radix_bits", "key_prefix_bits", "key_window_low", "n_partitions"):
                        assert plan[k] == R["plans"][key][k], (tag, k, plan, R["plans"][key])
                elif fam == "kind":
                    ck, cnt = fast_expected(B, P, side, kind, R["cache"])
                    if side == PSIDE:
                        r, got = ex.join_kind_device(bd, pd, kind, flags, outer_fill=PROBE_FILL)
                        got = dict(got, n_build_matched=0, n_build_unmatched=0)
                    else:
                        r, got = ex.join_build_kind_device(bd, pd, kind, flags, build_fill=BUILD_FILL, probe_fill=PROBE_FILL)
                    same(r, ck)
                    assert got == cnt, (tag, got, cnt)
                elif fam == "str_join":
                    c = strs[int(rng.integers(0, len(strs)))]
                    want, coll = c["want"]
                    res, info = ex.join_str_device(c["dev"][0], c["dev"][1], ORDERED | CHECKSUM, hash_bits=c["hash_bits"])
                    assert res.checks() == checks_of(want) and info["n_collisions"] == coll, tag
                    assert np.array_equal(ex.str_rows_to_numpy(res), want), tag
                elif fam == "sort":
                    if R["sorted"] is None:
                        R["sorted"] = B[np.argsort(B[:, 0], kind="stable")]
                    inplace = bool(rng.integers(0, 2))
                    out = ex.sort_device(bd.clone() if inplace else bd, inplace=inplace)
                    assert np.array_equal(out.cpu().numpy().view(np.uint64), R["sorted"]), tag
                elif fam == "prepare_join":
                    ex.prepare_build(bd, len(P))
                    same(ex.join_device(bd, pd, flags), inner_ck)
                elif fam == "message_bytes":
                    ex.comm_set_message_bytes(*COMM_MESSAGES[int(rng.integers(0, len(COMM_MESSAGES)))])
                else:
                    raise ValueError(fam)
                executed += 1
            print("communicator: seed %d tour %d: %d ops in %.1f s" % (seed, t, len(tour), time.perf_counter() - t0), flush=True)
        assert executed == drawn and drawn % (len(COMM_FAMILIES) ** 2 + 1) == 0
    finally:
        plain.close()
        ex.close()
