"""hmj_top_k_device on the GPU (include/hmj.h, "the first rows of an order") against `expected_top_k`: the order is total
with the row index, so the map must be equal entry by entry, and equal under every plan.  Every call also checks n_out,
plan_taken and K <= n_candidates <= n; under the SELECT plan n_levels against 8 levels per 8-byte window of the longest
stream, and n_rounds against ORDER BY's bound 1 + ceil(max(0, S - 8) / 4)."""
import ctypes as C

import numpy as np
import pytest

from test_order_by_cpu import (DESC, EDGE_STRINGS, NULLS_FIRST, STRING, SWEEP_ITERS, SWEEP_SEED, draw_order_case, edge_tables, special_values,
                               sweep_params)
from test_order_by_gpu import H, dev, dev_cols, ex, spec  # noqa: F401  (H and ex are fixtures)

pytestmark = pytest.mark.gpu
HMJ_E_ARG = -1
U64_MAX = 2 ** 64 - 1
PLANS = ("auto", "select", "full")
# A window is a 64-bit word; its first level takes the top 11 bits and every later one 11 more (fewer where fewer are
# left), so a window has at most 6 levels: a call that ran more has walked a tie list.
WINDOW_LEVELS = 6


def check(ex, H, cols, k, offset=0, tag="", n=None, plans=PLANS, max_tie_rows=0):
    """One cut under every plan of `plans`; returns {plan: info}."""
    n = len(cols[0]["values"]) if n is None else n
    columns = [(c["values"], c["flags"], c["valid"]) for c in cols]
    want = H.expected_top_k(columns, k, offset)
    K = min(n, offset + k)
    assert len(want) == min(k, n - min(n, offset))
    S = int(H.order_stream_bytes(columns).max()) if n else 0
    dcols = dev_cols(H, cols)
    infos, maps = {}, {}
    for plan in plans:
        got, info = ex.top_k_device(dcols, k, offset, n=n, plan=plan, max_tie_rows=max_tie_rows)
        got = got.cpu().numpy().view(np.uint64)
        where = "%s: k=%d offset=%d plan=%s max_tie_rows=%d" % (tag, k, offset, plan, max_tie_rows)
        if not np.array_equal(got, want):
            bad = int(np.nonzero(got != want)[0][0]) if len(got) == len(want) else -1
            raise AssertionError("%s: the map differs from position %d on (%d entries, want %d) %s" % (where, bad, len(got), len(want), info))
        assert info["n_out"] == len(want), (where, info)
        if len(want) == 0 or n == 1:  # no kernel ran
            assert info["plan_taken"] == 0 and info["n_levels"] == 0 and info["n_rounds"] == 0, (where, info)
            assert info["n_candidates"] == (1 if len(want) else 0), (where, info)
        else:
            assert info["plan_taken"] in (H.HMJ_TOPK_SELECT, H.HMJ_TOPK_FULL), (where, info)
            if plan != "auto":
                assert info["plan_taken"] == (H.HMJ_TOPK_SELECT if plan == "select" else H.HMJ_TOPK_FULL), (where, info)
            assert K <= info["n_candidates"] <= n, (where, info, K)
            assert info["n_rounds"] <= 1 + max(0, -(-(S - 8) // 4)), (where, info, S)
            if info["plan_taken"] == H.HMJ_TOPK_SELECT:
                assert 1 <= info["n_levels"] <= 8 * -(-S // 8), (where, info, S)
                assert info["n_tie_rows"] <= n
            else:
                assert info["n_levels"] == 0 and info["n_candidates"] == n and info["n_rounds"] >= 1, (where, info)
        infos[plan], maps[plan] = info, got
    for plan in plans[1:]:
        assert np.array_equal(maps[plan], maps[plans[0]])
    return infos


# ---- sizes -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 2047, 2048, 2049, 4097])
def test_boundary_sizes_cuts_and_offsets(ex, H, n):
    rng = np.random.default_rng(3000 + n)
    i64 = rng.integers(-40, 40, size=n).astype(np.int64) * (1 << 40)  # ties across the cut
    cols = [spec(i64, DESC)]
    ks = sorted({0, 1, 2, 64, max(n - 1, 0), n, n + 5})
    offsets = sorted({0, 1, max(n - 1, 0), n, n + 1, U64_MAX})
    for k in ks:
        for offset in offsets:
            check(ex, H, cols, k, offset, "i64 n=%d" % n, n=n, max_tie_rows=(k + offset) % 3)
    u8 = rng.integers(3, 5, size=n).astype(np.uint8)
    strs = [b"twenty-byte-prefix-->"[:20] + bytes(rng.integers(0x61, 0x64, size=2).astype(np.uint8)) for _ in range(n)]
    for k, offset in ((1, 0), (64, 1), (n, 0), (U64_MAX, max(n - 1, 0)), (U64_MAX, U64_MAX)):
        check(ex, H, [spec(u8), spec(strs)], k, offset, "u8, strings n=%d" % n, n=n, max_tie_rows=1)


# ---- selection selects -----------------------------------------------------------------------------------------------------------
def test_unique_keys_leave_exactly_the_cut_as_candidates(ex, H):
    rng = np.random.default_rng(31)
    n = 70000
    u64 = rng.permutation(n).astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15)  # (odd: a bijection mod 2^64)
    for offset in (0, n - 10):
        info = check(ex, H, [spec(u64)], 10, offset, "unique u64", plans=("select", "full", "auto"), max_tie_rows=1)["select"]
        assert info["n_candidates"] == min(n, offset + 10) and info["n_rounds"] == 1, info
    info = check(ex, H, [spec(u64)], 10, 0, "unique u64, default ties", plans=("select",))["select"]
    assert 10 <= info["n_candidates"] < n // 2, info  # the default tie limit stops early; most rows are still rejected unsorted


def test_skewed_digits_and_tie_sets_whose_stream_is_used_up(ex, H):
    rng = np.random.default_rng(32)
    n = 5000
    small = rng.integers(0, 1 << 10, size=n).astype(np.uint64)  # 54 shared top bits: later digits start at bit 9
    info = check(ex, H, [spec(small)], 37, 5, "u64 below 2^10", max_tie_rows=1)["select"]
    assert info["n_candidates"] == 42 and info["n_levels"] == 2, info  # every row in one bin, then the ten varying bits
    check(ex, H, [spec(small, DESC)], 37, 0, "u64 below 2^10 desc")
    # (the second table's stream is 28 bytes: with the default limit its 5000 ties would fit and be left to the final ordering)
    for ties, cols in ((0, [spec(np.full(n, -7, np.int32))]), (1, [spec([b"same string, 21 bytes"] * n), spec(np.full(n, 2.5, np.float32), DESC)])):
        for k, offset in ((10, 0), (10, 4000), (n, 0)):
            info = check(ex, H, cols, k, offset, "all equal", max_tie_rows=ties)["select"]
            assert info["n_candidates"] == min(n, offset + k), info
            assert info["n_tie_rows"] == (0 if offset + k >= n else n), info
    i8 = np.array([-3, 9, 100], np.int8)[rng.integers(0, 3, size=n)]
    lo, mid = int(np.count_nonzero(i8 == -3)), int(np.count_nonzero(i8 == 9))
    K = lo + mid // 2
    info = check(ex, H, [spec(i8)], 20, K - 20, "three i8 values")["select"]
    assert info["n_candidates"] == K and info["n_tie_rows"] == mid and info["n_levels"] == 1, info
    got, _ = ex.top_k_device([(dev(i8), 0)], mid // 2, lo, plan="select")
    assert got.cpu().numpy().tolist() == np.nonzero(i8 == 9)[0][:mid // 2].tolist()  # the ties in ascending row index


def test_a_bucket_that_lies_wholly_before_the_cut_leaves_no_tie(ex, H):
    rng = np.random.default_rng(33)
    first = (np.uint64(1) << np.uint64(60)) + rng.permutation(1 << 20)[:100].astype(np.uint64)  # one bin of the first digit
    rest = (np.uint64(2) << np.uint64(60)) + rng.integers(0, 1 << 59, size=4900).astype(np.uint64)
    keys = np.concatenate([first, rest])[rng.permutation(5000)]
    info = check(ex, H, [spec(keys)], 100, 0, "whole bucket", max_tie_rows=1)["select"]
    assert info["n_tie_rows"] == 0 and info["n_candidates"] == 100 and info["n_levels"] == 1, info
    info = check(ex, H, [spec(keys)], 60, 39, "inside the bucket", max_tie_rows=1)["select"]
    assert info["n_candidates"] == 99 and info["n_levels"] > 1, info


def test_ties_with_stream_bytes_left_are_narrowed_window_by_window(ex, H):
    rng = np.random.default_rng(34)
    n = 4097
    prefix = b"twenty-byte-prefix-->"[:20]
    tails = rng.permutation(1 << 24)[:n]  # unique strings: the rows differ from stream byte 22 on, in the third window
    strs = [prefix + int(t).to_bytes(3, "big") + b"xy" for t in tails]
    info = check(ex, H, [spec(strs, pad=3)], 10, 5, "shared prefix", max_tie_rows=1)["select"]
    # the first two windows are equal in every row -- one level each, nothing varies --, so a third level ran on a list
    assert info["n_levels"] >= 3 and info["n_candidates"] == 15 and info["n_tie_rows"] == 0, info
    info = check(ex, H, [spec(strs, DESC)], 10, 5, "shared prefix, default ties")["select"]
    assert info["n_levels"] == 1 and info["n_candidates"] == n, info  # 4097 ties fit the default: ORDER BY's rounds do the rest
    info = check(ex, H, [spec(strs), spec(np.arange(n, dtype=np.int32), DESC)], 300, 0, "shared prefix, 300 ties allowed", max_tie_rows=300)["select"]
    assert 300 <= info["n_candidates"] <= 600 and info["n_levels"] > 3, info


# ---- the rules of ORDER BY -------------------------------------------------------------------------------------------------------
def test_every_type_direction_and_null_placement_with_edge_values(ex, H):
    for t, (tag, columns) in enumerate(edge_tables()):
        cols = [spec(v, f, ok, bit_offset=3 if ok is not None else 0) for v, f, ok in columns]
        n = len(columns[0][0])
        check(ex, H, cols, 7 + t % 5, t % 11, tag, plans=("select", "full"), max_tie_rows=t % 2)
        check(ex, H, cols, n, 0, tag, plans=("select",))


def test_nan_zero_and_infinity_through_the_cut(ex, H):
    for dt in ("float32", "float64"):
        vals = np.array([np.nan, 1.0, -0.0, 0.0, -np.nan, np.inf, -np.inf, 0.0, -0.0, np.nan], dt)
        for k in range(0, 11):
            check(ex, H, [spec(vals)], k, 0, dt, max_tie_rows=1)
            check(ex, H, [spec(vals, DESC)], 3, k, dt + " desc", max_tie_rows=1)
        got, _ = ex.top_k_device([(dev(vals), 0)], 4, 1, plan="select")
        assert got.cpu().numpy().tolist() == [2, 8, 3, 7]


@pytest.mark.parametrize("offset", [3, 67])
def test_nulls_at_bit_offsets_mixed_keys_and_garbage_under_null_slots(ex, H, offset):
    rng = np.random.default_rng(60 + offset)
    n = 1500
    valid = rng.random(n) >= 0.3
    f64 = special_values("float64", rng, n, 6)
    i32 = special_values("int32", rng, n, 4)
    strs = [EDGE_STRINGS[k] for k in rng.integers(0, len(EDGE_STRINGS), size=n)]
    for flags in (0, DESC, NULLS_FIRST, DESC | NULLS_FIRST):
        for maker in (lambda: [spec(f64, flags, valid, offset)], lambda: [spec(strs, flags, valid, offset, pad=3), spec(i32, DESC)],
                      lambda: [spec(strs, flags ^ DESC, None, 0, pad=1)]):
            cols = maker()
            k, off = int(rng.integers(1, 600)), int(rng.integers(0, 900))
            check(ex, H, cols, k, off, "flags %d offset %d" % (flags, offset), plans=("select", "full"), max_tie_rows=1)
            for c in cols:  # the same call over other bytes under the NULL slots gives the same map
                if c["valid"] is None:
                    continue
                if c["type"] == STRING:
                    c["values"] = [v if ok else b"\xff garbage under a NULL slot" for v, ok in zip(c["values"], c["valid"])]
                else:
                    junk = c["values"].copy()
                    junk[~c["valid"]] = special_values(c["type"], rng, int(np.count_nonzero(~c["valid"])))
                    c["values"] = junk
            check(ex, H, cols, k, off, "garbage, flags %d offset %d" % (flags, offset), plans=("select",), max_tie_rows=1)


# ---- the drawn sweep -------------------------------------------------------------------------------------------------------------
def test_randomized_sweep_reaches_every_path(ex, H):
    seed, iters = sweep_params()
    rng = np.random.default_rng(seed)
    ledger = {"select": 0, "full": 0, "list level": 0, "trimmed ties": 0, "candidates == K": 0, "candidates > K": 0}
    for it in range(iters):
        case = draw_order_case(rng, it)
        n = min(case["n"], 5000)
        cols = []
        for c in case["cols"]:
            c = dict(c)
            c["values"] = c["values"][:n]
            c["valid"] = None if c["valid"] is None else c["valid"][:n]
            cols.append(c)
        k = int(rng.choice([1, 2, 10, 100, max(n // 3, 1), n, n + 5]))
        offset = int(rng.choice([0, 0, 1, 17, max(n // 2, 1), max(n - 1, 0), n]))
        plan = str(rng.choice(["select", "select", "select", "auto", "full"]))
        ties = int(rng.choice([0, 1, 1, 5, 64]))
        tag = "sweep seed %d case %d (n=%d, %s)" % (seed, it, n, [(c["type"], c["flags"]) for c in cols])
        info = check(ex, H, cols, k, offset, tag, n=n, plans=(plan,), max_tie_rows=ties)[plan]
        K = min(n, offset + k)
        if info["plan_taken"] == H.HMJ_TOPK_FULL:
            ledger["full"] += 1
        elif info["plan_taken"] == H.HMJ_TOPK_SELECT:
            ledger["select"] += 1
            ledger["list level"] += info["n_levels"] > WINDOW_LEVELS
            ledger["trimmed ties"] += info["n_tie_rows"] > 0 and info["n_candidates"] == K  # (ties left, yet nothing beyond the cut written)
            ledger["candidates == K"] += info["n_candidates"] == K
            ledger["candidates > K"] += info["n_candidates"] > K
    print("top-k sweep ledger:", ledger)
    if (seed, iters) == (SWEEP_SEED, SWEEP_ITERS):
        assert all(v > 0 for v in ledger.values()), ledger


# ---- refusals --------------------------------------------------------------------------------------------------------------------
def test_every_refusal_names_its_reason_and_leaves_the_ctx_usable(ex, H):
    import torch

    rng = np.random.default_rng(35)
    n = 1000
    vals = special_values("int32", rng, n, 20)
    strs = [EDGE_STRINGS[k] for k in rng.integers(0, len(EDGE_STRINGS), size=n)]
    good = [spec(vals, DESC, rng.random(n) >= 0.1, 3), spec(strs)]
    L, h = ex.L, ex.h
    col = dev(vals)
    chars, offs = H.pack_strings(strs, "cuda")
    out = torch.zeros(n + 8, dtype=torch.int64, device="cuda")

    def call(n_cols=2, rows=n, k=10, edit=None, opts_edit=None, null=(), map_ptr=None):
        arr, opts = (H.OrderCol * 9)(), H.TopKOpts()
        opts.struct_size = C.sizeof(H.TopKOpts)
        opts.plan = H.HMJ_TOPK_SELECT
        for i in range(9):
            arr[i].type, arr[i].data = H.HMJ_TYPE_I32, col.data_ptr()
        arr[1].type, arr[1].data, arr[1].offsets = H.HMJ_ORDER_LARGE_STRING, chars.data_ptr(), offs.data_ptr()
        if edit:
            edit(arr)
        if opts_edit:
            opts_edit(opts)
        rc = L.hmj_top_k_device(h, None if "cols" in null else arr, n_cols, rows, k, None if "map" in null else C.c_void_p(map_ptr or out.data_ptr()),
                                None if "opts" in null else C.byref(opts))
        return rc, L.hmj_last_error(h).decode(), opts

    def set_(i, **kw):
        return lambda arr: [setattr(arr[i], key, v) for key, v in kw.items()]

    def set_opts(**kw):
        return lambda o: [setattr(o, key, v) for key, v in kw.items()]

    refusals = [
        (dict(null=("cols",)), "cols / opts is NULL"),
        (dict(null=("opts",)), "cols / opts is NULL"),
        (dict(opts_edit=set_opts(plan=3)), "unknown plan"),
        (dict(opts_edit=set_opts(reserved=1)), "reserved must be 0"),
        (dict(opts_edit=set_opts(struct_size=H.TopKOpts.max_tie_rows.offset)), "struct_size too small"),
        (dict(null=("map",)), "row_map_out is NULL"),
        (dict(map_ptr=out.data_ptr() + 4), "row_map_out is not aligned"),
        (dict(map_ptr=col.data_ptr()), "column 0: row_map_out overlaps"),
        (dict(map_ptr=offs.data_ptr() + 8 * (n - 3)), "column 1: row_map_out overlaps"),
        (dict(n_cols=9), "n_cols must be in 1..8"),
        (dict(edit=set_(0, type=17)), "column 0 has unknown type 17"),
        (dict(edit=set_(1, flags=4)), "column 1 has unknown flag bits"),
        (dict(edit=set_(0, data=None)), "column 0: data is NULL"),
        (dict(rows=1 << 32), "more than 2^32 - 1 rows"),
    ]
    for kw, needle in refusals:
        rc, msg, _ = call(**kw)
        assert rc == HMJ_E_ARG and needle in msg, (kw.keys(), rc, msg)
        check(ex, H, good, 25, 3, "after " + needle, plans=("select",), max_tie_rows=1)
    # a prefix of the opts struct is a valid, older caller; ten entries of the map overlap nothing where all n would
    rc, msg, _ = call(opts_edit=set_opts(struct_size=H.TopKOpts.n_out.offset))
    assert rc == 0, msg
    # found on the device by the first level, before anything follows an offset: the lowest-numbered column, its first row
    bad = offs.clone()
    bad[[700, 400]] = bad[[700, 400]] + 1000
    rc, msg, _ = call(edit=set_(1, offsets=bad.data_ptr()))
    assert rc == HMJ_E_ARG and "column 1: offsets decrease at row 400 (offsets[401] < offsets[400])" in msg, msg
    check(ex, H, good, 25, 3, "after decreasing offsets", plans=("select",))
    rc, msg, _ = call(edit=set_(1, data=None))
    assert rc == HMJ_E_ARG and "column 1: data is NULL but keys have bytes" in msg, msg
    check(ex, H, good, 25, 3, "after data == NULL", plans=("select", "full"))
    # an empty result runs the host checks, writes nothing and needs no map
    out.fill_(-1)
    for kw in (dict(k=0), dict(rows=0), dict(opts_edit=set_opts(offset=n)), dict(k=0, null=("map",)), dict(rows=0, map_ptr=out.data_ptr() + 4)):
        rc, msg, opts = call(**kw)
        assert rc == 0 and opts.n_out == 0 and opts.plan_taken == 0 and bool((out == -1).all()), (kw.keys(), msg)
    rc, msg, _ = call(k=0, edit=set_(0, type=17))
    assert rc == HMJ_E_ARG and "unknown type 17" in msg
    # entries from n_out on are not written
    rc, msg, opts = call(k=7, opts_edit=set_opts(offset=n - 3))
    assert rc == 0 and opts.n_out == 3 and bool((out[3:] == -1).all()) and bool((out[:3] >= 0).all()), msg


# ---- the call among the others on one ctx ----------------------------------------------------------------------------------------
def test_the_context_effects_are_those_of_order_by(H):
    import os

    import torch

    os.environ["HMJ_GTABLE"] = "0"  # (the join below would otherwise take the global table and partition nothing)
    try:
        ex = H.Executor(0)
    finally:
        del os.environ["HMJ_GTABLE"]
    try:
        rng = np.random.default_rng(36)
        n = 6000
        names = [b"name-%03d" % k for k in rng.integers(0, 80, size=n)]
        price = np.round(rng.standard_normal(n) * 50, 0) + 0.0  # (no -0.0)
        chars, offs = H.pack_strings(names, "cuda")
        res, _ = ex.group_mixed_device([(chars, offs)], flags=H.HMJ_MATERIALIZE, want=H.HMJ_GROUP_ROW_MAP)
        ng = int(res.n_groups)
        cols = ex.group_rows_to_numpy(res)
        aggs = [(H.HMJ_AGG_SUM, dev(price), None)]
        (sums, _, _), = ex.group_agg_device(aggs)[0]
        key_chars, key_offs, _, _ = ex.take_str_device(chars, offs, (res.first_row, ng))
        # SELECT name, sum(price) GROUP BY name ORDER BY sum(price) DESC, name LIMIT 5 OFFSET 2
        rmap, info = ex.top_k_device([(sums, H.HMJ_ORDER_DESC), ((key_chars, key_offs), 0)], 5, 2, plan="select")
        assert info["n_out"] == 5 and info["plan_taken"] == H.HMJ_TOPK_SELECT
        out_chars, out_offs, _, _ = ex.take_str_device(key_chars, key_offs, rmap)
        (out_sums,), _, _ = ex.take_cols_device([sums], rmap)
        want_sums = H.expected_group_aggs(cols["group_of_row"], ng, [(H.HMJ_AGG_SUM, price, None)])[0]["values"]
        group_names = [names[int(r)] for r in cols["first_row"]]
        table = sorted(zip(group_names, want_sums.tolist()), key=lambda t: (-t[1], t[0]))[2:7]
        assert H.unpack_strings(out_chars, out_offs) == [t[0] for t in table]
        assert out_sums.cpu().numpy().tolist() == [t[1] for t in table]
        # the live grouping is kept: a second aggregate call still succeeds
        (again, _, _), = ex.group_agg_device(aggs)[0]
        assert torch.equal(again, sums)
        # a prepared build side is discarded, and hmj_last_plan keeps describing the last join
        nb, npb = 300000, 200000
        bd, pd = ex.gen_build(nb), ex.gen_probe(npb, nb, miss_mod=4)
        want = ex.join_device(bd, pd, 0).checks()
        ex.set_profiling(True)
        ex.prepare_build(bd, npb)
        r = ex.join_device(bd, pd, 0)
        assert r.checks() == want and ex.last_timing()["path"] & H.HMJ_PATH_PREPARED  # (taken when nothing comes between)
        for plan in ("select", "full"):
            ex.prepare_build(bd, npb)
            plan_before = ex.last_plan()
            _, info = ex.top_k_device([(sums, 0)], 3, plan=plan)
            assert ex.last_plan() == plan_before and info["ms_order"] >= 0.0
            r = ex.join_device(bd, pd, 0)
            t = ex.last_timing()
            assert r.checks() == want and not (t["path"] & H.HMJ_PATH_PREPARED) and t["ms_partition_build"] > 0.0
    finally:
        ex.close()
