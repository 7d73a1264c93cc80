"""Every column-operator entry once under hmj_set_profiling, on one context, and the context's teardown behind them.

The 13 entries of the string, multi-column and mixed-key joins, the groupings, the aggregates, ORDER BY, WHERE and the two
takes run on one Executor at 300 rows (one full 256-row block and a 44-row tail), every validity bitmap at bit_offset 3:
first with profiling on -- every entry then creates its phase events --, then with profiling off.  Results are checked
against the package's host models (expected_*) where it has one and against a dict brute force elsewhere; the ms_* fields
are finite and >= 0 with profiling, 0 without it, and the results are the same.  The executor is closed with all events
alive, and a second one filters and takes.  Last, one refused call per opts struct: HMJ_E_ARG for a struct_size too small
leaves the caller's opts bytes as they were."""
import ctypes as C
import math

import numpy as np
import pytest

from test_join_str_cpu import str_hash

pytestmark = pytest.mark.gpu
N = 300
OFF = 3
M64 = 0xFFFFFFFFFFFFFFFF
FILL = 99


@pytest.fixture(scope="module")
def H():
    import torch

    import hashmergejoin_amd as H

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return H


def make_data():
    rng = np.random.RandomState(20261021)
    d = {}
    d["bs"] = [b"" if i % 37 == 0 else b"key%03d" % (i % 120) for i in range(N)]
    d["ps"] = [b"" if k == 7 else b"key%03d" % k for k in rng.randint(0, 160, N)]
    d["b1"], d["b2"] = rng.randint(0, 20, N).astype(np.int32), rng.randint(0, 5, N).astype(np.int16)
    d["p1"], d["p2"] = rng.randint(0, 24, N).astype(np.int32), rng.randint(0, 5, N).astype(np.int16)
    d["bv"], d["pv"] = np.arange(N, dtype=np.int64) * 3 + 1, np.arange(N, dtype=np.int64) * 5 + 2
    d["bm"], d["pm"] = rng.rand(N) > 0.1, rng.rand(N) > 0.1  # True = valid
    d["f64"] = rng.randint(-50, 50, N).astype(np.float64)     # (integers: every sum is exact)
    d["i64"] = rng.randint(-2 ** 40, 2 ** 40, N).astype(np.int64)
    m = rng.permutation(N).astype(np.int64)
    m[::11] = -1  # HMJ_TAKE_NO_ROW
    d["map"] = m
    return d


def brute_outer(bkeys, bv, pkeys, pv):
    """(r_row, s_row, rval, sval) of the probe-side outer join, sorted; a key None is NULL and has no partner."""
    by = {}
    for r, k in enumerate(bkeys):
        if k is not None:
            by.setdefault(k, []).append(r)
    rows = []
    for s, k in enumerate(pkeys):
        rs = by.get(k, ()) if k is not None else ()
        rows += [(r, s, int(bv[r]), int(pv[s])) for r in rs] or [(M64, s, FILL, int(pv[s]))]
    return sorted(rows)


def brute_inner(bkeys, bv, pkeys, pv):
    return [t for t in brute_outer(bkeys, bv, pkeys, pv) if t[0] != M64]


def pairs(rows):
    return sorted(tuple(int(x) for x in r[1:5]) for r in rows)


def masked(keys, mask):
    return [k if ok else None for k, ok in zip(keys, mask)]


def run_entries(H, ex, d):
    """Every entry once; returns {entry: (what it computed, as plain Python / numpy values, its info dict)}."""
    import torch

    L = H._lib
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    MAT, PROBE, OUTER = L.HMJ_MATERIALIZE, L.HMJ_KIND_PROBE_SIDE, L.HMJ_JOIN_PROBE_OUTER
    bch, bof = H.pack_strings(d["bs"], device="cuda")
    pch, pof = H.pack_strings(d["ps"], device="cuda")
    b1, b2, p1, p2, bv, pv = (dev(d[k]) for k in ("b1", "b2", "p1", "p2", "bv", "pv"))
    f64, i64 = dev(d["f64"]), dev(d["i64"])
    bvt, pvt = (H.pack_validity(d["bm"], OFF, "cuda"), OFF), (H.pack_validity(d["pm"], OFF, "cuda"), OFF)
    bt, pt = list(zip(d["b1"].tolist(), d["b2"].tolist())), list(zip(d["p1"].tolist(), d["p2"].tolist()))
    bmix, pmix = list(zip(d["bs"], d["b1"].tolist())), list(zip(d["ps"], d["p1"].tolist()))
    out = {}

    h = ex.hash_str_device(bch, bof).cpu().numpy().view(np.uint64)
    assert h.tolist() == [str_hash(k, 0) for k in d["bs"]]
    out["hash_str"] = (h, {})

    res, info = ex.join_str_device((bch, bof, bv), (pch, pof, pv), MAT)
    got = pairs(ex.str_rows_to_numpy(res))
    assert got == brute_inner(d["bs"], d["bv"], d["ps"], d["pv"])
    out["join_str"] = (got, info)

    res, info = ex.join_kind_str_device((bch, bof, bv), (pch, pof, pv), PROBE, OUTER, MAT, probe_fill=FILL, build_valid=bvt, probe_valid=pvt)
    got = pairs(ex.str_kind_rows_to_numpy(res))
    assert got == brute_outer(masked(d["bs"], d["bm"]), d["bv"], masked(d["ps"], d["pm"]), d["pv"])
    assert (info["n_build_null"], info["n_probe_null"]) == (int((~d["bm"]).sum()), int((~d["pm"]).sum()))
    assert info["n_probe_unmatched"] == sum(1 for t in got if t[0] == M64)
    out["join_kind_str"] = (got, info)

    res, info = ex.join_cols_device([b1, b2], bv, [p1, p2], pv, MAT)
    got = pairs(ex.cols_rows_to_numpy(res))
    assert got == brute_inner(bt, d["bv"], pt, d["pv"])
    out["join_cols"] = (got, info)

    res, info = ex.join_kind_cols_device([b1, b2], bv, [p1, p2], pv, PROBE, OUTER, MAT, probe_fill=FILL, build_valid=[bvt, None],
                                         probe_valid=[None, pvt])
    got = pairs(ex.cols_kind_rows_to_numpy(res))
    assert got == brute_outer(masked(bt, d["bm"]), d["bv"], masked(pt, d["pm"]), d["pv"])
    assert (info["n_build_null"], info["n_probe_null"]) == (int((~d["bm"]).sum()), int((~d["pm"]).sum()))
    out["join_kind_cols"] = (got, info)

    res, info = ex.join_mixed_device([(bch, bof), b1], bv, [(pch, pof), p1], pv, PROBE, OUTER, MAT, probe_fill=FILL, build_valid=[bvt, None],
                                     probe_valid=[pvt, None])
    got = pairs(ex.mixed_rows_to_numpy(res))
    assert got == brute_outer(masked(bmix, d["bm"]), d["bv"], masked(pmix, d["pm"]), d["pv"])
    out["join_mixed"] = (got, info)

    cols = ("key64", "first_row", "count", "sum", "group_of_row")
    want = L.HMJ_GROUP_COUNT | L.HMJ_GROUP_SUM | L.HMJ_GROUP_ROW_MAP
    res, info = ex.group_cols_device([b1, b2], vals=bv, valid=[bvt, None], flags=L.HMJ_ORDERED, want=want)
    got = ex.group_rows_to_numpy(res)
    exp = H.expected_groups([d["b1"], d["b2"]], [4, 2], vals=d["bv"], valid=[d["bm"], None], ordered=True)
    assert int(res.n_groups) == exp["n_groups"] and info["n_null"] == exp["n_null"]
    for c in cols:
        assert np.array_equal(got[c], exp[c]), c
    out["group_cols"] = ([got[c] for c in cols], info)

    res, info = ex.group_mixed_device([(bch, bof), b1], vals=bv, valid=[bvt, None], flags=L.HMJ_ORDERED, want=want)
    got = ex.group_rows_to_numpy(res)
    exp = H.expected_mixed_groups([masked(d["bs"], d["bm"]), d["b1"]], vals=d["bv"], valid=[d["bm"], None], ordered=True)
    assert int(res.n_groups) == exp["n_groups"] and info["n_null"] == exp["n_null"]
    for c in cols:
        assert np.array_equal(got[c], exp[c]), c
    out["group_mixed"] = ([got[c] for c in cols], info)

    # (op, column, with the probe side's bitmap) over the mixed grouping, which is the live one
    spec = [(L.HMJ_AGG_SUM, "f64", True), (L.HMJ_AGG_MIN, "b1", True), (L.HMJ_AGG_MEAN, "i64", False), (L.HMJ_AGG_COUNT, None, False)]
    on_dev = {"f64": f64, "b1": b1, "i64": i64, None: None}
    aggs = [(op, d[c] if c else None, d["pm"] if nulls else None) for op, c, nulls in spec]
    outs, info = ex.group_agg_device([(op, on_dev[c], pvt[0] if nulls else None, OFF) for op, c, nulls in spec], n_rows=N)
    exp_aggs = H.expected_group_aggs(exp["group_of_row"], exp["n_groups"], aggs)
    got = []
    for (vals, words, nulls), e in zip(outs, exp_aggs):
        v, ok = vals.cpu().numpy(), H.unpack_validity(words, exp["n_groups"])
        assert np.array_equal(ok, e["valid"]) and nulls == e["null_count"]
        assert np.array_equal(v.view(np.uint64), np.asarray(e["values"]).astype(v.dtype).view(np.uint64))
        got += [v, ok]
    assert info["n_groups"] == exp["n_groups"]
    out["group_agg"] = (got, info)

    rmap, info = ex.order_by_device([(b1, L.HMJ_ORDER_DESC, bvt[0], OFF), ((pch, pof), L.HMJ_ORDER_NULLS_FIRST, pvt[0], OFF), (f64, 0)])
    exp_map = H.expected_order_by([(d["b1"], L.HMJ_ORDER_DESC, d["bm"]), (d["ps"], L.HMJ_ORDER_NULLS_FIRST, d["pm"]),
                                   (d["f64"], 0)])
    got = rmap.cpu().numpy().view(np.uint64)
    assert np.array_equal(got, exp_map)
    out["order_by"] = (got, info)

    terms = [{"column": b1, "op": L.HMJ_FILTER_LT, "lit": 12, "valid": bvt[0], "bit_offset": OFF},
             {"column": (pch, pof), "op": L.HMJ_FILTER_STARTS_WITH, "lit": b"key0", "valid": pvt[0], "bit_offset": OFF, "clause": 1},
             {"column": f64, "op": L.HMJ_FILTER_GE, "lit": 0.0, "clause": 1, "row_map": dev(d["map"])}]
    host = [dict(terms[0], column=d["b1"], valid=d["bm"]), dict(terms[1], column=masked(d["ps"], d["pm"]), valid=d["pm"]),
            dict(terms[2], column=d["f64"], row_map=d["map"])]
    sel, words, info = ex.filter_device(terms, want_mask=True)
    exp_sel, exp_unknown = H.expected_filter(host, N)
    got = sel.cpu().numpy().view(np.uint64)
    assert np.array_equal(got, exp_sel) and info["n_unknown"] == exp_unknown and info["n_out"] == len(exp_sel)
    assert np.array_equal(np.flatnonzero(H.unpack_validity(words, N)), exp_sel.astype(np.int64))
    out["filter"] = (got, info)

    m = d["map"]
    have = m >= 0
    (o1, o2), (w1, w2), info = ex.take_cols_device([b1, i64], dev(m), valid=[bvt, None])
    ok1, ok2 = have & d["bm"][np.where(have, m, 0)], have
    assert np.array_equal(H.unpack_validity(w1, N), ok1) and np.array_equal(H.unpack_validity(w2, N), ok2)
    assert np.array_equal(o1.cpu().numpy(), np.where(ok1, d["b1"][np.where(have, m, 0)], 0))
    assert np.array_equal(o2.cpu().numpy(), np.where(ok2, d["i64"][np.where(have, m, 0)], 0))
    assert info["null_count"] == [int((~ok1).sum()), int((~ok2).sum())] and info["n_no_row"] == int((~have).sum())
    out["take_cols"] = ([o1.cpu().numpy(), o2.cpu().numpy()], info)

    ch, of, words, info = ex.take_str_device(pch, pof, dev(m), valid=pvt)
    got = H.unpack_strings(ch.cpu(), of.cpu(), valid=H.unpack_validity(words, N))
    assert got == [d["ps"][r] if r >= 0 and d["pm"][r] else None for r in m]
    assert info["null_count"] == sum(1 for g in got if g is None) and info["n_no_row"] == int((~have).sum())
    out["take_str"] = (got, info)
    return out


def same(a, b):
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray):
        return a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))
    return a == b


def test_every_entry_under_profiling_and_the_teardown_behind_it(H):
    import torch

    d = make_data()
    ex = H.Executor(0)
    try:
        ex.set_profiling(True)
        on = run_entries(H, ex, d)
        assert len(on) == 13
        for name, (_, info) in on.items():
            for k, v in info.items():
                if k.startswith("ms_"):
                    assert math.isfinite(v) and v >= 0.0, (name, k, v)
        ex.set_profiling(False)
        off = run_entries(H, ex, d)
        for name, (result, info) in off.items():
            assert same(result, on[name][0]), name
            for k, v in info.items():
                if k.startswith("ms_"):
                    assert v == 0.0, (name, k, v)
                else:
                    assert v == on[name][1][k], (name, k)
    finally:
        ex.close()  # every workspace holds its events
    ex = H.Executor(0)
    try:
        col = torch.from_numpy(d["b1"]).cuda()
        sel, _, info = ex.filter_device([{"column": col, "op": H._lib.HMJ_FILTER_GE, "lit": 10}])
        exp_sel, _ = H.expected_filter([{"column": d["b1"], "op": H._lib.HMJ_FILTER_GE, "lit": 10}], N)
        assert np.array_equal(sel.cpu().numpy().view(np.uint64), exp_sel)
        (o,), _, info = ex.take_cols_device([col], sel)
        assert np.array_equal(o.cpu().numpy(), d["b1"][exp_sel.astype(np.int64)]) and info["null_count"] == [0]
    finally:
        ex.close()


def test_a_refused_struct_size_leaves_the_opts_as_they_were(H):
    L = H._lib
    ex = H.Executor(0)
    lib = ex.L
    str_rel, cols_rel, mixed_rel = L.StrRel(), L.ColsRel(), L.MixedRel()
    str_res, cols_res, grp_res = L.StrResult(), L.ColsResult(), L.GroupResult()
    calls = [
        (L.StrJoinOpts, lambda o: lib.hmj_join_str_device(ex.h, C.byref(str_rel), C.byref(str_rel), 0, o, C.byref(str_res))),
        (L.StrKindOpts, lambda o: lib.hmj_join_kind_str_device(ex.h, C.byref(str_rel), C.byref(str_rel), 0, o, C.byref(str_res))),
        (L.ColsJoinOpts, lambda o: lib.hmj_join_cols_device(ex.h, C.byref(cols_rel), C.byref(cols_rel), 0, o, C.byref(cols_res))),
        (L.ColsKindOpts, lambda o: lib.hmj_join_kind_cols_device(ex.h, C.byref(cols_rel), C.byref(cols_rel), 0, o, C.byref(cols_res))),
        (L.MixedOpts, lambda o: lib.hmj_join_mixed_device(ex.h, C.byref(mixed_rel), C.byref(mixed_rel), 0, o, C.byref(cols_res))),
        (L.GroupOpts, lambda o: lib.hmj_group_cols_device(ex.h, C.byref(cols_rel), 0, o, C.byref(grp_res))),
        (L.GroupOpts, lambda o: lib.hmj_group_mixed_device(ex.h, C.byref(mixed_rel), 0, o, C.byref(grp_res))),
        (L.GroupAggOpts, lambda o: lib.hmj_group_agg_device(ex.h, (L.AggSrc * 1)(), 1, 0, (L.AggDst * 1)(), o)),
        (L.OrderOpts, lambda o: lib.hmj_order_by_device(ex.h, (L.OrderCol * 1)(), 1, 0, None, o)),
        (L.FilterOpts, lambda o: lib.hmj_filter_device(ex.h, (L.FilterTerm * 1)(), 1, 0, None, None, o)),
        (L.TakeOpts, lambda o: lib.hmj_take_cols_device(ex.h, (L.TakeSrc * 1)(), 1, 0, None, 0, (L.TakeDst * 1)(), o)),
        (L.TakeStrOpts, lambda o: lib.hmj_take_str_device(ex.h, C.byref(L.TakeStrSrc()), 0, None, 0, C.byref(L.TakeStrDst()), o)),
    ]
    try:
        for T, call in calls:
            o = T()
            C.memset(C.byref(o), 0x5A, C.sizeof(T))
            o.struct_size = 4  # holds struct_size alone
            before = bytes(o)
            assert call(C.byref(o)) == -1, T.__name__  # HMJ_E_ARG
            assert "struct_size too small" in lib.hmj_last_error(ex.h).decode(), T.__name__
            assert bytes(o) == before, T.__name__
    finally:
        ex.close()
