"""hmj_window_device on the GPU (include/hmj.h, "window functions over ordered partitions") against `expected_window`:
the order is total with the row index, so the map and every integer output must be equal entry by entry, bitmaps word by
word with padding bits 0, and the null counts and the three counters equal.  Float sums are held to the header's bound
against the exact prefix sums.  The sizes come from the kernels' constants, which tests/test_winplan_cpu.py compares with
hmj_winplan.h's: P positions per wave, G positions per workgroup, T aggregates per carry tile."""
import ctypes as C

import numpy as np
import pytest

from test_order_by_cpu import DESC, NULLS_FIRST, special_values
from test_order_by_gpu import dev, dev_cols, spec
from test_window_cpu import (CUM_COUNT, CUM_MAX, CUM_MIN, CUM_SUM, DENSE_RANK, LAG, LEAD, OPS, RANK, ROW_NUMBER, case_fns,
                             draw_window_case, sweep_params)

pytestmark = pytest.mark.gpu
HMJ_E_ARG = -1
P = 512
G = 2048
T = 2048
U = 2.0 ** -53


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


def fn(op, values=None, valid=None, bit_offset=0, offset=0):
    return {"op": op, "values": values, "valid": valid, "bit_offset": bit_offset, "offset": offset}


def all_nine(x, valid=None, bit_offset=0, lag=1, lead=1):
    return [fn(ROW_NUMBER), fn(RANK), fn(DENSE_RANK), fn(CUM_COUNT, x, valid, bit_offset), fn(CUM_SUM, x, valid, bit_offset),
            fn(CUM_MIN, x, valid, bit_offset), fn(CUM_MAX, x, valid, bit_offset), fn(LAG, x, valid, bit_offset, lag),
            fn(LEAD, x, valid, bit_offset, lead)]


def dev_fns(H, fns):
    out = []
    for f in fns:
        col = None if f["values"] is None else dev(f["values"])
        bits = None if f["valid"] is None else H.pack_validity(f["valid"], f["bit_offset"], device="cuda")
        out.append((f["op"], col, bits, f["bit_offset"], f["offset"]))
    return out


def words_of(valid):
    n = len(valid)
    bits = np.zeros(((n + 63) // 64) * 64, np.uint8)
    bits[:n] = valid
    return np.packbits(bits, bitorder="little").view(np.uint64)


def bits_of(a):
    a = np.ascontiguousarray(a)
    return a.view("u%d" % a.dtype.itemsize)


def compare(H, got_map, got, info, want, fns, tag):
    n = len(want["row_map"])
    got_map = got_map.cpu().numpy().view(np.uint64)
    if not np.array_equal(got_map, want["row_map"]):
        bad = int(np.nonzero(got_map != want["row_map"])[0][0])
        raise AssertionError("%s: the map differs from position %d on: got row %d, want row %d" % (tag, bad, got_map[bad], want["row_map"][bad]))
    for key in ("n_partitions", "n_peer_groups", "max_partition_rows"):
        assert info[key] == want[key], (tag, key, info[key], want[key])
    for k, (f, (vals, words, nulls), w) in enumerate(zip(fns, got, want["outputs"])):
        what = "%s: function %d %s" % (tag, k, OPS[f["op"]])
        assert nulls == w["null_count"], (what, nulls, w["null_count"])
        if words is not None:
            assert np.array_equal(words.cpu().numpy().view(np.uint64), words_of(w["valid"])), what + ": bitmap words"
        v = vals.cpu().numpy()
        assert v.dtype.itemsize == w["values"].dtype.itemsize and len(v) == n, (what, v.dtype, w["values"].dtype)
        v = v.view(w["values"].dtype)
        differ = bits_of(v) != bits_of(w["values"])
        if "abs_sum" in w:  # a float sum: |got - exact| <= gamma_k sum|x| over a finite prefix, the reference within u of exact
            finite = np.isfinite(w["abs_sum"])
            kk = w["count"].astype(np.float64)
            with np.errstate(invalid="ignore"):
                within = np.abs(v - w["values"]) <= (kk * U / (1 - kk * U) + U) * w["abs_sum"]
                either_nan = np.isnan(v) & np.isnan(w["values"])  # behind a NaN or both infinities: which NaN is not specified
            differ = np.where(finite, ~within, differ & ~either_nan) | (~w["valid"] & (bits_of(v) != 0))
        bad = np.nonzero(differ)[0]
        assert len(bad) == 0, (what, "position %d" % bad[0], v[bad[0]], w["values"][bad[0]], "%d differ" % len(bad))


def check(ex, H, cols, npc, fns, n=None, tag="", want_validity=True):
    if n is None:
        n = len(cols[0]["values"]) if cols else len(next(f["values"] for f in fns if f["values"] is not None))
    got_map, got, info = ex.window_device(dev_cols(H, cols), npc, dev_fns(H, fns), n=n, want_validity=want_validity)
    want = H.expected_window([(c["values"], c["flags"], c["valid"]) for c in cols], npc, case_fns({"fns": fns}), n=n)
    compare(H, got_map, got, info, want, fns, tag)
    assert info["n_rounds"] == 0 if (not cols or n <= 1) else info["n_rounds"] >= 1, (tag, info)
    return got_map, got, info


# ---- sizes ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, P - 1, P, P + 1, G - 1, G, G + 1, 5000])
def test_boundary_sizes_with_all_nine_ops_in_one_call(ex, H, n):
    rng = np.random.default_rng(2000 + n)
    k = rng.integers(0, 3, size=n).astype(np.int32)
    t = rng.integers(0, max(2, n // 3), size=n).astype(np.int64) * (1 << 33)
    x = rng.integers(-1000, 1000, size=n).astype(np.int32)
    valid = rng.random(n) >= 0.2
    _, got, info = check(ex, H, [spec(k), spec(t)], 1, all_nine(x, valid, 3), n=n, tag="n=%d" % n)
    assert info["n_partitions"] == len(np.unique(k))
    if n == 0:
        assert all(nulls == 0 for _, _, nulls in got)


def partitions_of(lengths, rng):
    """Rows in shuffled order whose I32 key gives partitions of these lengths, in this order."""
    key = np.repeat(np.arange(len(lengths), dtype=np.int32), lengths)
    return key[rng.permutation(len(key))]


@pytest.mark.parametrize("shape", ["cycle", "all P", "singletons", "one partition"])
def test_partition_lengths_around_the_wave_and_workgroup_ranges(ex, H, shape):
    rng = np.random.default_rng(31)
    lengths = {"cycle": [1, 1, 2, 63, 64, 65, P - 1, P, P + 1, G - 1, G, G + 1, 3 * G + 5] * 2, "all P": [P] * 9,
               "singletons": [1] * (G + 77), "one partition": [G + 1]}[shape]
    key = partitions_of(lengths, rng)
    n = len(key)
    x = rng.integers(-2 ** 40, 2 ** 40, size=n).astype(np.int64)
    f = rng.standard_normal(n)
    valid = rng.random(n) >= 0.3
    fns = all_nine(x, valid, 67, lag=2, lead=P) + [fn(CUM_SUM, f), fn(CUM_MAX, f, valid), fn(CUM_MIN, x)]
    _, _, info = check(ex, H, [spec(key)], 1, fns, tag=shape)  # every key column a partition column: rows keep their order
    assert (info["n_partitions"], info["max_partition_rows"]) == (len(lengths), max(lengths))
    assert info["n_peer_groups"] == len(lengths)  # without order columns a partition is one peer group


def test_one_partition_of_rows_beyond_a_carry_tile_without_keys(ex, H):
    n = (1 << 22) + 77  # more than T wave ranges: the carry's top level (tests/test_winplan_cpu.py)
    assert n > P * T
    rng = np.random.default_rng(32)
    x = rng.integers(-2 ** 50, 2 ** 50, size=n).astype(np.int64)
    f = rng.standard_normal(n)
    f[::100003] = np.nan
    rmap, got, info = ex.window_device([], 0, [(CUM_SUM, dev(x)), (CUM_MAX, dev(f)), (ROW_NUMBER, None)], n=n)
    assert (info["n_partitions"], info["n_peer_groups"], info["max_partition_rows"], info["n_rounds"]) == (1, 1, n, 0)
    assert np.array_equal(rmap.cpu().numpy(), np.arange(n))
    assert np.array_equal(got[0][0].cpu().numpy().view(np.int64), np.cumsum(x))
    want = np.maximum.accumulate(np.where(np.isnan(f), -np.inf, f))  # a NaN loses; the first value is a NaN: until a number comes
    want[0] = np.nan
    assert np.array_equal(bits_of(got[1][0].cpu().numpy()), bits_of(want))
    assert np.array_equal(got[2][0].cpu().numpy().view(np.uint64), np.arange(1, n + 1, dtype=np.uint64))
    assert [g[2] for g in got] == [0, 0, 0]
    full = np.full((n + 63) // 64, ~np.uint64(0))
    full[-1] = np.uint64((1 << (n % 64)) - 1)
    assert all(np.array_equal(g[1].cpu().numpy().view(np.uint64), full) for g in got)


# ---- floats --------------------------------------------------------------------------------------------------------------------
def test_nan_and_infinities_stay_inside_their_partition(ex, H):
    # the first partition ends right in front of a wave range, the second starts on it: the carry must not leak
    n1, n2 = P, P + 70
    k = np.repeat(np.array([0, 1], np.int32), [n1, n2])
    rng = np.random.default_rng(33)
    x = np.concatenate([np.resize(np.array([1.0, np.nan, np.inf, -np.inf]), n1), rng.standard_normal(n2)])
    for dtype in ("float64", "float32"):
        v = x.astype(dtype)
        _, got, _ = check(ex, H, [spec(k)], 1, [fn(CUM_SUM, v), fn(CUM_MIN, v), fn(CUM_MAX, v)], tag=dtype)
        s, lo, hi = (g[0].cpu().numpy() for g in got)
        assert s[0] == 1.0 and np.all(np.isnan(s[1:n1])) and np.all(np.isfinite(s[n1:]))
        assert lo[0] == 1.0 and lo[1] == 1.0 and lo[2] == 1.0 and np.all(lo[3:n1] == -np.inf) and np.all(hi[2:n1] == np.inf)
        assert np.array_equal(lo[n1:], np.minimum.accumulate(v[n1:])) and np.array_equal(hi[n1:], np.maximum.accumulate(v[n1:]))
    allnan = np.full(5, np.nan, np.float32)
    _, got, _ = check(ex, H, [], 0, [fn(CUM_MIN, allnan), fn(CUM_MAX, allnan, np.array([0, 1, 1, 1, 1], bool))], tag="all NaN")
    assert got[0][0].cpu().numpy().view(np.uint32).tolist() == [0x7FC00000] * 5 and got[1][2] == 1


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_sums_of_integer_valued_floats_are_exact(ex, H, dtype):
    n = 1 << 20
    rng = np.random.default_rng(34)
    lim = 2 ** 31 - 256  # (the largest float32 below 2^31; what float32 rounds to is still an integer)
    x = rng.integers(-lim, lim + 1, size=n).astype(dtype)
    assert np.all(np.abs(x) < 2.0 ** 31) and np.all(x == np.round(x))
    _, got, _ = ex.window_device([], 0, [(CUM_SUM, dev(x))], n=n)
    assert np.array_equal(got[0][0].cpu().numpy(), np.cumsum(x.astype(np.float64)))
    key = partitions_of([3 * G + 5, P, 70000, 1, G - 1], rng)
    m = len(key)
    rmap, got, _ = ex.window_device([(dev(key), 0)], 1, [(CUM_SUM, dev(x[:m]))])
    order = rmap.cpu().numpy()
    want = np.concatenate([np.cumsum(x[:m][order][key[order] == p].astype(np.float64)) for p in range(5)])
    assert np.array_equal(got[0][0].cpu().numpy(), want)


def test_random_doubles_stay_within_the_bound_and_the_bits_do_not_depend_on_the_call(ex, H):
    rng = np.random.default_rng(35)
    key = partitions_of([20000, 7, P + 1, 9000], rng)
    n = len(key)
    x = rng.standard_normal(n) * 10.0 ** rng.integers(-8, 9, size=n)
    other = rng.integers(0, 100, size=n).astype(np.int16)
    cols = [spec(key)]
    _, alone, _ = check(ex, H, cols, 1, [fn(CUM_SUM, x)], tag="alone")
    six = [fn(CUM_MIN, other), fn(CUM_SUM, other), fn(CUM_COUNT, other), fn(CUM_MAX, other), fn(CUM_SUM, x), fn(ROW_NUMBER)]
    _, shared, _ = check(ex, H, cols, 1, six, tag="the 5th of 6")  # four scans fill a launch: the sum opens the next
    assert np.array_equal(bits_of(alone[0][0].cpu().numpy()), bits_of(shared[4][0].cpu().numpy()))
    # an unrelated join and sort on the ctx change nothing
    bd, pd = ex.gen_build(50000), ex.gen_probe(80000, 50000, miss_mod=4)
    ex.join_device(bd, pd, 0)
    ex.sort_device(bd)
    _, again, _ = check(ex, H, cols, 1, [fn(CUM_SUM, x)], tag="again")
    assert np.array_equal(bits_of(alone[0][0].cpu().numpy()), bits_of(again[0][0].cpu().numpy()))


# ---- peers and NULLs -------------------------------------------------------------------------------------------------------------
def test_tie_runs_across_wave_and_workgroup_ranges(ex, H):
    rng = np.random.default_rng(36)
    runs = [5, P - 3, 10, 3 * P, 1, G + 9, 64, 2 * G, 7]  # peer groups of one partition: these many rows tie in the order key
    t = np.repeat(np.arange(len(runs), dtype=np.int64), runs)
    k = np.zeros(len(t), np.int32)
    k[-200:] = 1
    perm = rng.permutation(len(t))
    x = rng.integers(0, 50, size=len(t)).astype(np.uint16)
    for flags in (0, DESC):
        _, got, info = check(ex, H, [spec(k[perm]), spec(t[perm], flags)], 1, [fn(RANK), fn(DENSE_RANK), fn(ROW_NUMBER), fn(CUM_SUM, x)],
                             tag="flags %d" % flags)
        assert info["n_partitions"] == 2 and info["n_peer_groups"] == len(runs) + 1


@pytest.mark.parametrize("offset", [0, 3, 67])
def test_nulls_strings_and_flags_in_the_keys_and_bitmaps_at_bit_offsets(ex, H, offset):
    rng = np.random.default_rng(37 + offset)
    n = 3000
    names = [b"a-twenty-byte-prefix" + bytes([0x61 + int(i)]) * int(rng.integers(0, 3)) for i in rng.integers(0, 3, size=n)]
    kvalid = rng.random(n) >= 0.2  # NULL names form one partition
    t = special_values("float32", rng, n, 12)
    tvalid = rng.random(n) >= 0.2
    x = special_values("int8", rng, n)
    valid = rng.random(n) >= 0.4
    for kflags, tflags in ((0, DESC | NULLS_FIRST), (NULLS_FIRST, NULLS_FIRST), (DESC, DESC)):
        cols = [spec(names, kflags, kvalid, offset, pad=5), spec(t, tflags, tvalid, offset)]
        _, _, info = check(ex, H, cols, 1, all_nine(x, valid, offset, lag=1, lead=2), tag="flags %d %d" % (kflags, tflags))
        assert info["n_partitions"] == len({nm for nm, ok in zip(names, kvalid) if ok}) + 1


def test_lag_and_lead_offsets(ex, H):
    rng = np.random.default_rng(38)
    lengths = [P + 40, 3, 2 * P]
    key = partitions_of(lengths, rng)
    n = len(key)
    x = rng.integers(-2 ** 62, 2 ** 62, size=n).astype(np.int64)
    f = special_values("float32", rng, n)
    valid = rng.random(n) >= 0.25
    fns = []
    for off in (0, 1, P, lengths[0] - 1, lengths[0], 2 ** 63, 2 ** 64 - 1):
        fns += [fn(LAG, x, valid, 3, off), fn(LEAD, x, None, 0, off), fn(LEAD, f, valid, 3, off)]
    _, got, _ = check(ex, H, [spec(key)], 1, fns)
    assert got[0][2] == int(n - valid.sum()) and got[1][2] == 0  # offset 0 is the row itself
    assert got[-2][2] == n  # no position 2^64 - 1 rows away


# ---- the randomized sweep ------------------------------------------------------------------------------------------------------
def test_randomized_sweep(ex, H):
    seed, iters = sweep_params()
    rng = np.random.default_rng(seed)
    for it in range(iters):
        case = draw_window_case(rng, it)
        tag = "sweep seed %d case %d (n=%d, npc=%d, keys %s)" % (seed, it, case["n"], case["npc"], [(c["type"], c["flags"]) for c in case["cols"]])
        check(ex, H, case["cols"], case["npc"], case["fns"], n=case["n"], tag=tag, want_validity=[k % 3 != 2 for k in range(len(case["fns"]))])


# ---- the call among the others on one ctx ------------------------------------------------------------------------------------------
def test_the_grouping_survives_a_prepared_build_side_does_not_and_plan_and_timing_stay(H):
    import os

    import torch

    os.environ["HMJ_GTABLE"] = "0"  # (the join below would otherwise take the global table and partition nothing)
    try:
        ex = H.Executor(0)
    finally:
        del os.environ["HMJ_GTABLE"]
    try:
        rng = np.random.default_rng(39)
        n = 6000
        k = rng.integers(0, 50, size=n).astype(np.int32)
        price = np.round(rng.standard_normal(n) * 50, 0) + 0.0
        res, _ = ex.group_cols_device([dev(k)], flags=H.HMJ_MATERIALIZE, want=H.HMJ_GROUP_ROW_MAP | H.HMJ_GROUP_COUNT)
        groups_before = ex.group_rows_to_numpy(res)
        aggs = [(H.HMJ_AGG_SUM, dev(price), None)]
        (sums, _, _), = ex.group_agg_device(aggs)[0]
        nb, npb = 300000, 200000
        bd, pd = ex.gen_build(nb), ex.gen_probe(npb, nb, miss_mod=4)
        want = ex.join_device(bd, pd, 0).checks()
        ex.set_profiling(True)
        ex.prepare_build(bd, npb)
        plan_before, timing_before = ex.last_plan(), ex.last_timing()
        check(ex, H, [spec(k), spec(price)], 1, all_nine(price), tag="between group and aggregate")
        assert ex.last_plan() == plan_before and ex.last_timing() == timing_before
        # the live grouping and the group result are kept: the columns read the same, a second aggregate call still works
        groups_after = ex.group_rows_to_numpy(res)
        assert all(np.array_equal(groups_before[c], groups_after[c]) for c in groups_before)
        (again, _, _), = ex.group_agg_device(aggs)[0]
        assert torch.equal(again, sums)
        # the prepared build side went with the sort
        r = ex.join_device(bd, pd, 0)
        t = ex.last_timing()
        assert r.checks() == want and not (t["path"] & H.HMJ_PATH_PREPARED) and t["ms_partition_build"] > 0.0
        _, _, info = check(ex, H, [spec(k), spec(price)], 1, [fn(ROW_NUMBER)], tag="profiled")
        assert info["ms_order"] > 0.0 and info["ms_heads"] > 0.0 and info["ms_scan"] > 0.0
    finally:
        ex.close()


# ---- refusals ----------------------------------------------------------------------------------------------------------------
def test_every_refusal_names_its_reason_and_leaves_the_ctx_usable(ex, H):
    import torch

    rng = np.random.default_rng(40)
    n = 1000
    kv = rng.integers(0, 4, size=n).astype(np.int32)
    xv = rng.integers(-99, 99, size=n).astype(np.int32)
    strs = [b"s%d" % i for i in rng.integers(0, 9, size=n)]
    good_cols, good_fns = [spec(kv), spec(strs)], all_nine(xv, rng.random(n) >= 0.1, 3)
    L, h = ex.L, ex.h
    key, x = dev(kv), dev(xv)
    chars, offs = H.pack_strings(strs, "cuda")
    bitmap = H.pack_validity(np.ones(n, bool), 0, device="cuda")
    rmap = torch.zeros(n + 8, dtype=torch.int64, device="cuda")
    outs = [torch.zeros(n + 8, dtype=torch.int64, device="cuda") for _ in range(3)]
    words = torch.zeros((n + 63) // 64 + 2, dtype=torch.int64, device="cuda")

    def call(n_keys=2, rows=n, n_fns=3, keys_edit=None, fns_edit=None, dst_edit=None, opts_edit=None, null=(), map_ptr=None):
        keys, fns, dst, opts = (H.OrderCol * 9)(), (H.WindowFn * 33)(), (H.WindowDst * 33)(), H.WindowOpts()
        opts.struct_size, opts.n_partition_cols = C.sizeof(H.WindowOpts), 1
        for k in range(9):
            keys[k].type, keys[k].data = H.HMJ_TYPE_I32, key.data_ptr()
        keys[1].type, keys[1].data, keys[1].offsets = H.HMJ_ORDER_LARGE_STRING, chars.data_ptr(), offs.data_ptr()
        for a in range(33):
            fns[a].type, fns[a].data, fns[a].op = H.HMJ_TYPE_I32, x.data_ptr(), (H.HMJ_WIN_CUM_SUM, H.HMJ_WIN_LAG, H.HMJ_WIN_ROW_NUMBER)[a % 3]
            dst[a].data = outs[a % 3].data_ptr() if a < 3 else None
        dst[0].validity = words.data_ptr()
        for edit, arr in ((keys_edit, keys), (fns_edit, fns), (dst_edit, dst), (opts_edit, opts)):
            if edit:
                edit(arr)
        rc = L.hmj_window_device(h, None if "keys" in null else keys, n_keys, rows, None if "fns" in null else fns, n_fns,
                                 None if "dst" in null else dst, None if "map" in null else C.c_void_p(map_ptr or rmap.data_ptr()),
                                 None if "opts" in null else C.byref(opts))
        return rc, L.hmj_last_error(h).decode()

    def set_(i, **kw):
        def edit(arr):
            for k, v in kw.items():
                setattr(arr[i].validity if k in ("bits", "bit_offset") else arr[i], k, v)
        return edit

    def set_opts(**kw):
        return lambda o: [setattr(o, k, v) for k, v in kw.items()]

    refusals = [
        (dict(null=("fns",)), "fns / dst / opts is NULL"),
        (dict(null=("dst",)), "fns / dst / opts is NULL"),
        (dict(null=("opts",)), "fns / dst / opts is NULL"),
        (dict(null=("keys",)), "keys is NULL with n_keys > 0"),
        (dict(n_keys=9), "n_keys must be in 0..8"),
        (dict(opts_edit=set_opts(n_partition_cols=3)), "n_partition_cols is greater than n_keys"),
        (dict(opts_edit=set_opts(struct_size=H.WindowOpts.reserved.offset)), "struct_size too small"),
        (dict(opts_edit=set_opts(reserved=1)), "reserved must be 0"),
        (dict(n_fns=0), "n_fns must be in 1..32"),
        (dict(n_fns=33), "n_fns must be in 1..32"),
        (dict(fns_edit=set_(1, op=9)), "function 1: unknown op"),
        (dict(fns_edit=set_(2, type=10)), "function 2: unknown type"),
        (dict(rows=1 << 32), "too many rows"),
        (dict(fns_edit=set_(0, data=None)), "function 0: source data is NULL"),
        (dict(fns_edit=set_(1, data=x.data_ptr() + 2)), "function 1: source data is not aligned"),
        (dict(dst_edit=set_(2, data=None)), "function 2: destination data is NULL"),
        (dict(dst_edit=set_(1, data=outs[1].data_ptr() + 2)), "function 1: destination data is not aligned"),
        (dict(dst_edit=set_(0, validity=words.data_ptr() + 4)), "function 0: destination validity is not aligned"),
        (dict(null=("map",)), "row_map_out is NULL"),
        (dict(map_ptr=rmap.data_ptr() + 4), "row_map_out is not aligned"),
        (dict(fns_edit=set_(0, bits=bitmap.data_ptr(), bit_offset=2 ** 64 - 5)), "function 0: validity bit_offset + n overflows"),
        (dict(dst_edit=set_(0, data=x.data_ptr())), "function 0: the destination overlaps a source column, a key column or a bitmap"),
        (dict(dst_edit=set_(1, data=key.data_ptr())), "function 1: the destination overlaps a source column, a key column or a bitmap"),
        (dict(dst_edit=set_(0, validity=offs.data_ptr() + 8 * (n - 3))), "function 0: the destination overlaps a source column"),
        (dict(fns_edit=set_(0, bits=outs[2].data_ptr() + 8, bit_offset=0)), "function 2: the destination overlaps a source column"),
        (dict(dst_edit=set_(1, data=outs[0].data_ptr() + 8)), "function 0: the destination overlaps another destination"),
        (dict(dst_edit=set_(1, validity=words.data_ptr() + 8)), "function 0: the destination overlaps another destination"),
        (dict(map_ptr=outs[1].data_ptr() + 16), "the destination overlaps another destination or row_map_out"),
        (dict(map_ptr=x.data_ptr()), "row_map_out overlaps a source column, a key column or a bitmap"),
        # what hmj_order_by_device rejects in the keys, in its wording
        (dict(keys_edit=set_(0, type=17)), "column 0 has unknown type 17"),
        (dict(keys_edit=set_(1, flags=4)), "column 1 has unknown flag bits"),
        (dict(keys_edit=set_(0, data=None)), "column 0: data is NULL"),
        (dict(keys_edit=set_(1, offsets=None)), "column 1: offsets is NULL"),
        (dict(keys_edit=set_(0, bits=bitmap.data_ptr(), bit_offset=2 ** 64 - 5)), "column 0: validity bit_offset + n overflows"),
    ]
    for kw, needle in refusals:
        rc, msg = call(**kw)
        assert rc == HMJ_E_ARG and needle in msg, (list(kw), rc, msg)
        check(ex, H, good_cols, 1, good_fns, tag="after " + needle)
    # found on the device by the ORDER BY, before anything follows an offset
    bad = offs.clone()
    bad[400] = bad[400] + 1000
    rc, msg = call(keys_edit=set_(1, offsets=bad.data_ptr()))
    assert rc == HMJ_E_ARG and "column 1: offsets decrease at row 400 (offsets[401] < offsets[400])" in msg, msg
    check(ex, H, good_cols, 1, good_fns, tag="after decreasing offsets")
    # a prefix of the opts struct is a valid, older caller: nothing behind `reserved` is written
    rc, msg = call(opts_edit=set_opts(struct_size=H.WindowOpts.ms_order.offset))
    assert rc == 0, msg
    # the ranking functions read no source; CUM_COUNT's data may be NULL
    rc, msg = call(fns_edit=lambda f: [set_(2, data=None, type=0)(f), set_(0, data=None, op=H.HMJ_WIN_CUM_COUNT)(f)])
    assert rc == 0, msg
    # n == 0 writes nothing and looks at no argument that is only checked with n > 0
    for t in outs + [rmap, words]:
        t.fill_(-1)
    rc, msg = call(rows=0, map_ptr=rmap.data_ptr() + 4, fns_edit=set_(0, data=None), dst_edit=set_(1, data=None))
    assert rc == 0 and all(bool((t == -1).all()) for t in outs + [rmap, words]), msg
    rc, msg = call(rows=0, null=("map",))
    assert rc == 0, msg
