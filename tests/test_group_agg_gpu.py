"""hmj_group_agg_device on the GPU (include/hmj.h, "aggregating typed value columns over a grouping"), against
`expected_group_aggs` fed with the device's own group_of_row.  The rows are grouped by one uint64 key column in the packed
form, where key64 is the key and an ordered call puts group g at sorted positions that follow from the group sizes alone:
a test places every group boundary where it wants it -- against the chunk of 64 positions, the 512 positions a wave of the
walk covers and the 2048 of a workgroup."""
import ctypes as C

import numpy as np
import pytest

from test_group_agg_cpu import DTYPES, assert_aggs, draw_agg_case, draw_values, special_values, sweep_params

pytestmark = pytest.mark.gpu
HMJ_E_ARG = -1
OPS = (0, 1, 2, 3, 4)  # HMJ_AGG_COUNT, SUM, MIN, MAX, MEAN


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


def dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()


def group(ex, H, key, ordered=True):
    """Group by one uint64 key column (packed); returns (GroupResult, its columns in numpy)."""
    res, info = ex.group_cols_device([dev(np.asarray(key, np.uint64).view(np.int64))], flags=H.HMJ_ORDERED if ordered else H.HMJ_MATERIALIZE,
                                     want=H.HMJ_GROUP_ROW_MAP | H.HMJ_GROUP_COUNT)
    assert info["form"] == H.HMJ_COLS_PACKED
    return res, ex.group_rows_to_numpy(res)


def dev_aggs(H, aggs):
    """The aggregates on the device.  One numpy array (or mask at one offset) listed in several aggregates becomes ONE device
    tensor, so that neighbours of one source column take the walk's path that reuses the loaded value and validity bit."""
    out, cols, maps = [], {}, {}
    for a in aggs:
        op, vals, valid = a[0], a[1], a[2]
        off = a[3] if len(a) > 3 else 0
        if vals is not None and id(vals) not in cols:
            cols[id(vals)] = dev(vals)
        if valid is not None and (id(valid), off) not in maps:
            maps[(id(valid), off)] = H.pack_validity(valid, off, device="cuda")
        out.append((op, None if vals is None else cols[id(vals)], None if valid is None else maps[(id(valid), off)], off))
    return out


def aggregate(ex, H, aggs, n_groups, want_validity=True, n_rows=None):
    """The aggregate call on the live grouping -> per aggregate (values numpy, validity bools or None, null_count); the
    padding bits of every output bitmap are checked to be 0."""
    got, info = ex.group_agg_device(dev_aggs(H, aggs), want_validity, n_rows=n_rows)
    assert info["n_groups"] == n_groups
    out = []
    for v, w, nulls in got:
        ok = None
        if w is not None:
            words = w.cpu().numpy().view(np.uint64)
            assert len(words) == (n_groups + 63) // 64
            if n_groups % 64:
                assert int(words[-1]) >> (n_groups % 64) == 0, "padding bits must be 0"
            ok = H.unpack_validity(w, n_groups)
            assert nulls == n_groups - int(np.count_nonzero(ok))
        out.append((v.cpu().numpy(), ok, nulls))
    return out


def check(ex, H, key, aggs, ordered=True, want_validity=True, tag=""):
    res, cols = group(ex, H, key, ordered)
    ng = int(res.n_groups)
    got = aggregate(ex, H, aggs, ng, want_validity)
    want = H.expected_group_aggs(cols["group_of_row"], ng, [a[:3] for a in aggs])
    assert_aggs(H, got, want, aggs, ng, tag)
    return res, cols, got, want


def placed_key(rng, sizes):
    """A key column whose ordered grouping puts group g at the sorted positions the sizes give it; the rows are shuffled."""
    key = np.repeat(np.arange(len(sizes), dtype=np.uint64) * np.uint64(1000003) + np.uint64(5), np.asarray(sizes, np.int64))
    return key[rng.permutation(len(key))]


def mixed_aggs(H, rng, n, density=0.1):
    """Six aggregates over three columns -- more than one launch chunk -- that touch every accumulator kind."""
    i32 = special_values("int32", rng, n)
    f64 = draw_values(rng, n, "float64", False)
    f32 = special_values("float32", rng, n)
    valid = rng.random(n) >= density if density else None
    return [(H.HMJ_AGG_SUM, i32, valid), (H.HMJ_AGG_MEAN, f64, None), (H.HMJ_AGG_MIN, f32, valid), (H.HMJ_AGG_MAX, i32, None),
            (H.HMJ_AGG_SUM, f64, valid), (H.HMJ_AGG_COUNT, None, valid)]


# ---- boundary sizes and placed groups ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 511, 512, 513, 2047, 2048, 2049, 4097])
def test_boundary_sizes_in_three_layouts(ex, H, n):
    rng = np.random.default_rng(n)
    layouts = {"one group": np.full(n, 42, np.uint64), "all distinct": rng.permutation(n).astype(np.uint64) * np.uint64(7919),
               "drawn": rng.integers(0, max(1, n // 9), size=n).astype(np.uint64)}
    for name, key in layouts.items():
        res, _, _, _ = check(ex, H, key, mixed_aggs(H, rng, n), tag=(n, name))
        if name != "drawn":
            assert res.n_groups == (1 if name == "one group" else n)


@pytest.mark.parametrize("unit", [64, 512, 2048])
def test_group_boundaries_at_and_beside_every_unit(ex, H, unit):
    """Boundaries at unit * k - 1, unit * k and unit * k + 1 for k = 1, 2, 3: groups that end exactly at a chunk's, a wave's
    and a workgroup's right end, start exactly there, or miss it by one."""
    rng = np.random.default_rng(unit)
    for delta in (-1, 0, 1):
        cuts = [unit + delta, 2 * unit + delta, 3 * unit + delta, 3 * unit + delta + 37]
        sizes = np.diff([0] + cuts)
        key = placed_key(rng, sizes)
        res, cols, _, _ = check(ex, H, key, mixed_aggs(H, rng, len(key)), tag=(unit, delta))
        assert cols["count"].tolist() == sizes.tolist()
    # every boundary of the unit at once, and single rows squeezed against them
    sizes = [unit - 1, 1, 1, unit - 1, unit, 1, unit + 1, unit - 2, 3]
    key = placed_key(rng, sizes)
    res, cols, _, _ = check(ex, H, key, mixed_aggs(H, rng, len(key)), tag=(unit, "mixed"))
    assert cols["count"].tolist() == sizes


def test_groups_that_span_waves(ex, H):
    rng = np.random.default_rng(1600)
    # about 1600 rows from position 500 in n = 5000: a left partial, whole-wave partials and a right partial
    sizes = [500, 1600, 5000 - 2100]
    check(ex, H, placed_key(rng, sizes), mixed_aggs(H, rng, 5000), tag="1600 from 500")
    # starts at a wave's left end and fills several whole waves; then one that ends exactly at a wave's right end
    sizes = [512, 1536, 300, 212, 7]
    res, cols, _, _ = check(ex, H, placed_key(rng, sizes), mixed_aggs(H, rng, sum(sizes)), tag="whole waves")
    assert cols["count"].tolist() == sizes
    # one group over more than 64 waves (the combine step's lanes take several partials each) between two small ones
    sizes = [3, 70 * 512 + 11, 5]
    check(ex, H, placed_key(rng, sizes), mixed_aggs(H, rng, sum(sizes), 0.5), tag="70 waves")


# ---- every type x every op -----------------------------------------------------------------------------------------------------
def test_every_type_and_op_in_one_call(ex, H):
    """50 aggregates in one call: 13 launch chunks over one grouping, every source column under all five ops."""
    rng = np.random.default_rng(50)
    n = 3000
    key = rng.integers(0, 40, size=n).astype(np.uint64)
    aggs = []
    for k, dtype in enumerate(DTYPES):
        order_vals = special_values(dtype, rng, n)
        sum_vals = order_vals if np.dtype(dtype).kind in "iu" else draw_values(rng, n, dtype, False)
        valid = rng.random(n) >= 0.2 if k % 2 else None
        for op in OPS:
            aggs.append((op, order_vals if op in (H.HMJ_AGG_MIN, H.HMJ_AGG_MAX) else sum_vals, valid, (0, 3, 67)[k % 3]))
    _, _, got, want = check(ex, H, key, aggs)
    # the extremes are met: every integer MIN / MAX equals the type's limit in some group
    for (op, vals, _, _), (v, _, _) in zip(aggs, got):
        if vals.dtype.kind in "iu" and op in (H.HMJ_AGG_MIN, H.HMJ_AGG_MAX):
            info = np.iinfo(vals.dtype)
            assert (info.min if op == H.HMJ_AGG_MIN else info.max) in v.tolist()


def test_nine_aggregates_and_one_column_under_several_ops(ex, H):
    rng = np.random.default_rng(9)
    n = 2500
    key = rng.integers(0, 300, size=n).astype(np.uint64)
    x = draw_values(rng, n, "float64", False)
    y = special_values("int16", rng, n)
    valid = rng.random(n) >= 0.3
    aggs = [(op, x, valid) for op in OPS] + [(op, y, None) for op in (1, 2, 3, 4)]
    assert len(aggs) == 9
    check(ex, H, key, aggs)


def test_integer_sums_wrap_and_widen(ex, H):
    g = np.array([0, 0, 0, 1, 1, 2, 2, 2], np.uint64)
    i64 = np.array([2 ** 63 - 1, 1, 0, -2 ** 63, -1, 2 ** 62, 2 ** 62, 2 ** 62], np.int64)
    u64 = np.array([2 ** 64 - 1, 2, 0, 2 ** 63, 2 ** 63, 7, 8, 9], np.uint64)
    i8 = np.array([127, 127, 3, -128, -128, 100, 100, 100], np.int8)
    u8 = np.array([255, 255, 255, 0, 1, 200, 200, 200], np.uint8)
    aggs = [(H.HMJ_AGG_SUM, i64, None), (H.HMJ_AGG_SUM, u64, None), (H.HMJ_AGG_SUM, i8, None), (H.HMJ_AGG_SUM, u8, None),
            (H.HMJ_AGG_MEAN, i64, None), (H.HMJ_AGG_MEAN, u64, None)]
    _, _, got, _ = check(ex, H, g, aggs)
    assert got[0][0].tolist() == [-2 ** 63, 2 ** 63 - 1, -2 ** 62] and got[1][0].tolist() == [1, 0, 24]
    assert got[2][0].tolist() == [257, -256, 300] and got[3][0].tolist() == [765, 1, 600]
    assert got[4][0].tolist()[0] == float(2 ** 63) / 3  # the mean of the values, not of the wrapped sum


def test_float_order_nan_zeros_and_infinities_bit_for_bit(ex, H):
    g = np.array([0, 0, 1, 1, 2, 2, 3, 3, 3, 4, 4, 5], np.uint64)
    nan2 = np.array([0x7FF0000000000001], np.uint64).view(np.float64)[0]  # a signalling NaN with a payload
    f = np.array([-0.0, 0.0, np.nan, nan2, np.nan, 1.5, -np.inf, np.inf, 0.0, 5e-324, -5e-324, -np.nan], np.float64)
    with np.errstate(invalid="ignore"):  # (the signalling NaN's conversion)
        f32 = f.astype(np.float32)
    f32[9], f32[10] = np.float32(1e-45), np.float32(-1e-45)  # float32 denormals
    aggs = [(H.HMJ_AGG_MIN, f, None), (H.HMJ_AGG_MAX, f, None), (H.HMJ_AGG_MIN, f32, None), (H.HMJ_AGG_MAX, f32, None)]
    _, _, got, _ = check(ex, H, g, aggs)
    QN, QN32 = 0x7FF8000000000000, 0x7FC00000
    assert got[0][0].view(np.uint64).tolist() == [1 << 63, QN, 0x3FF8000000000000, 0xFFF0000000000000, (1 << 63) | 1, QN]
    assert got[1][0].view(np.uint64).tolist() == [0, QN, 0x3FF8000000000000, 0x7FF0000000000000, 1, QN]
    assert got[2][0].view(np.uint32).tolist() == [1 << 31, QN32, 0x3FC00000, 0xFF800000, (1 << 31) | 1, QN32]
    assert got[3][0].view(np.uint32).tolist() == [0, QN32, 0x3FC00000, 0x7F800000, 1, QN32]
    assert all(nulls == 0 for _, _, nulls in got)  # a NaN is a valid value


# ---- float SUM and MEAN --------------------------------------------------------------------------------------------------------
def test_small_integer_valued_float_sums_are_exact(ex, H):
    rng = np.random.default_rng(24)
    n = 5000
    key = placed_key(rng, [700, 1800, 1, 2499])
    x = rng.integers(-1000, 1000, size=n)  # |sum| < 5000 * 1000 < 2^24: every order of summation is exact
    aggs = [(H.HMJ_AGG_SUM, x.astype(np.float32), None), (H.HMJ_AGG_SUM, x.astype(np.float64), None), (H.HMJ_AGG_MEAN, x.astype(np.float32), None),
            (H.HMJ_AGG_MEAN, x.astype(np.int32), None)]
    res, cols, got, want = check(ex, H, key, aggs)
    for k in range(4):
        assert got[k][0].tolist() == want[k]["values"].tolist(), k


def test_float_sums_over_thirty_binades_stay_inside_the_summation_bound(ex, H):
    rng = np.random.default_rng(30)
    n = 6000
    key = placed_key(rng, [5, 3000, 600, 2395])
    for dtype in ("float64", "float32"):
        x = draw_values(rng, n, dtype, False)
        valid = rng.random(n) >= 0.1
        check(ex, H, key, [(H.HMJ_AGG_SUM, x, None), (H.HMJ_AGG_MEAN, x, None), (H.HMJ_AGG_SUM, x, valid), (H.HMJ_AGG_MEAN, x, valid)], tag=dtype)


def test_float_sums_have_identical_bits_from_call_to_call(ex, H):
    """The same call twice, and once more behind an unrelated join on the same ctx; one group spans more than 10 waves."""
    rng = np.random.default_rng(10)
    sizes = [100, 12 * 512 + 77, 900, 1, 300]
    n = sum(sizes)
    key = placed_key(rng, sizes)
    x, y = draw_values(rng, n, "float64", False), draw_values(rng, n, "float32", False)
    valid = rng.random(n) >= 0.2
    aggs = [(H.HMJ_AGG_SUM, x, valid), (H.HMJ_AGG_MEAN, y, None), (H.HMJ_AGG_MEAN, x, None), (H.HMJ_AGG_SUM, y, valid), (H.HMJ_AGG_SUM, x, None)]
    res, cols, first, _ = check(ex, H, key, aggs)
    ng = int(res.n_groups)
    again = aggregate(ex, H, aggs, ng)
    r = ex.join_device(ex.gen_build(5000), ex.gen_probe(4000, 5000), H.HMJ_MATERIALIZE)
    assert r.n_matches > 0
    third = aggregate(ex, H, aggs, ng)
    for a, b, c in zip(first, again, third):
        bits = a[0].view(np.uint64).tolist()
        assert bits == b[0].view(np.uint64).tolist() == c[0].view(np.uint64).tolist()


# ---- NULLs -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offset", [0, 3, 67])
def test_bitmaps_at_bit_offsets_all_null_groups_and_garbage_under_null_slots(ex, H, offset):
    rng = np.random.default_rng(offset)
    n = 3000
    key = rng.integers(0, 50, size=n).astype(np.uint64)
    valid = rng.random(n) >= 0.3
    valid[key == 7] = False  # a group with all values NULL
    none = np.zeros(n, bool)  # a column that is entirely NULL
    f = draw_values(rng, n, "float64", False)
    i = special_values("int32", rng, n)
    dirty_f, dirty_i = f.copy(), i.copy()
    dirty_f[~valid] = np.array([0x7FF8DEADBEEF0001, 0xFFF0000000000000], np.uint64).view(np.float64)[rng.integers(0, 2, size=n)][~valid]
    dirty_i[~valid] = rng.integers(-2 ** 31, 2 ** 31, size=n)[~valid]
    clean = [(op, f, valid, offset) for op in (1, 2, 3, 4)] + [(op, i, valid, offset) for op in (1, 2, 3, 4)]
    dirty = [(op, dirty_f, valid, offset) for op in (1, 2, 3, 4)] + [(op, dirty_i, valid, offset) for op in (1, 2, 3, 4)]
    extra = [(H.HMJ_AGG_SUM, dirty_f, none, offset), (H.HMJ_AGG_COUNT, dirty_i, none, offset), (H.HMJ_AGG_COUNT, None, valid, offset),
             (H.HMJ_AGG_COUNT, None, None)]
    res, cols, got_clean, _ = check(ex, H, key, clean)
    ng = int(res.n_groups)
    _, _, got, want = check(ex, H, key, dirty + extra)
    for a, b in zip(got_clean, got):  # what lies under a NULL slot changes no bit
        assert a[0].view("u%d" % a[0].dtype.itemsize).tolist() == b[0].view("u%d" % b[0].dtype.itemsize).tolist() and a[2] == b[2]
    g7 = int(cols["group_of_row"][np.flatnonzero(key == 7)[0]])
    assert not got[0][1][g7] and got[0][0][g7] == 0 and got[0][2] >= 1
    assert got[8][2] == ng and not got[8][1].any() and not got[8][0].any()  # entirely NULL: every slot NULL, bytes 0
    assert got[9][0].tolist() == [0] * ng and got[9][2] == 0  # COUNT of an entirely NULL column: 0, valid
    assert got[11][0].tolist() == cols["count"].tolist()  # COUNT without data and bitmap: the group sizes
    # null_count without an output bitmap
    bare = aggregate(ex, H, dirty + extra, ng, want_validity=False)
    assert [b[2] for b in bare] == [g[2] for g in got] and all(b[1] is None for b in bare)


# ---- binding -----------------------------------------------------------------------------------------------------------------
def expect_arg_error(H, fn, *needles):
    with pytest.raises(H.HmjError) as e:
        fn()
    assert e.value.code == HMJ_E_ARG, str(e.value)
    for s in needles:
        assert s in str(e.value), str(e.value)


def test_binding_begins_and_ends_with_the_group_calls(ex, H):
    import torch

    rng = np.random.default_rng(77)
    n = 1500
    key = rng.integers(0, 30, size=n).astype(np.uint64)
    vals = special_values("int32", rng, n)
    aggs = [(H.HMJ_AGG_SUM, vals, None), (H.HMJ_AGG_MIN, vals, None)]
    fresh = H.Executor(0)
    try:  # before any group call
        expect_arg_error(H, lambda: fresh.group_agg_device(dev_aggs(H, aggs)), "no live grouping")
    finally:
        fresh.close()
    res, cols, got, want = check(ex, H, key, aggs)
    ng = int(res.n_groups)
    # a take and a u64 join in between keep the binding; the group result's own columns stay as they were
    outs, _, _ = ex.take_cols_device([dev(vals)], (res.first_row, ng))
    assert outs[0].cpu().numpy().tolist() == vals[cols["first_row"].astype(np.int64)].tolist()
    r = ex.join_device(ex.gen_build(3000), ex.gen_probe(2000, 3000), H.HMJ_MATERIALIZE | H.HMJ_ORDERED)
    assert r.n_matches > 0
    assert_aggs(H, aggregate(ex, H, aggs, ng), want, aggs, ng)
    after = ex.group_rows_to_numpy(res)
    for name, col in cols.items():
        assert (col is None and after[name] is None) or col.tolist() == after[name].tolist(), name
    # a wrong n_rows
    expect_arg_error(H, lambda: ex.group_agg_device(dev_aggs(H, [(H.HMJ_AGG_COUNT, None, None)]), n_rows=n - 1), "n_rows")
    assert_aggs(H, aggregate(ex, H, aggs, ng), want, aggs, ng)  # the ctx and the binding are as they were
    # a count-only group call ends it
    ex.group_cols_device([dev(key.view(np.int64))], flags=0)
    expect_arg_error(H, lambda: ex.group_agg_device(dev_aggs(H, aggs)), "no live grouping")
    # hmj_release_result ends it
    check(ex, H, key, aggs)
    ex.release_result()
    expect_arg_error(H, lambda: ex.group_agg_device(dev_aggs(H, aggs)), "no live grouping")
    # a later group call that failed ends it
    check(ex, H, key, aggs)
    with pytest.raises(H.HmjError):
        ex.group_cols_device([dev(key.view(np.int64))], flags=H.HMJ_MATERIALIZE | H.HMJ_CHECKSUM)
    expect_arg_error(H, lambda: ex.group_agg_device(dev_aggs(H, aggs)), "no live grouping")
    # n_rows == 0: a live grouping of zero rows
    res0, _ = ex.group_cols_device([torch.empty(0, dtype=torch.int64, device="cuda")], flags=H.HMJ_MATERIALIZE)
    assert res0.n_groups == 0
    got0, info0 = ex.group_agg_device([(H.HMJ_AGG_SUM, torch.empty(0, dtype=torch.float64, device="cuda"), None), (H.HMJ_AGG_COUNT, None, None)])
    assert info0["n_groups"] == 0 and [(len(v), nulls) for v, _, nulls in got0] == [(0, 0), (0, 0)]
    check(ex, H, key, aggs)  # and the ctx goes on


def test_aggregates_over_a_string_key_grouping(ex, H):
    rng = np.random.default_rng(5)
    n = 2000
    names = [b"name-%d" % k for k in rng.integers(0, 60, size=n)]
    day = rng.integers(0, 3, size=n).astype(np.int32)
    chars, offs = H.pack_strings(names, "cuda")
    res, _ = ex.group_mixed_device([(chars, offs), dev(day)], flags=H.HMJ_ORDERED, want=H.HMJ_GROUP_ROW_MAP)
    cols = ex.group_rows_to_numpy(res)
    ng = int(res.n_groups)
    assert ng == len(set(zip(names, day.tolist())))
    aggs = mixed_aggs(H, rng, n)
    got = aggregate(ex, H, aggs, ng)
    assert_aggs(H, got, H.expected_group_aggs(cols["group_of_row"], ng, aggs), aggs, ng)


# ---- refusals ----------------------------------------------------------------------------------------------------------------
def test_every_refusal_names_its_reason_and_leaves_the_ctx_usable(ex, H):
    import torch

    rng = np.random.default_rng(13)
    n = 1000
    key = rng.integers(0, 100, size=n).astype(np.uint64)
    vals = special_values("int32", rng, n)
    good = [(H.HMJ_AGG_SUM, vals, rng.random(n) >= 0.1)]
    res, cols, _, want = check(ex, H, key, good)
    ng = int(res.n_groups)
    L, h = ex.L, ex.h
    col = dev(vals)
    col64 = dev(vals.astype(np.int64))
    bitmap = H.pack_validity(np.ones(n, bool), 0, device="cuda")
    out = torch.zeros(ng + 8, dtype=torch.int64, device="cuda")
    out2 = torch.zeros(ng + 8, dtype=torch.int64, device="cuda")
    words = torch.zeros((ng + 63) // 64 + 1, dtype=torch.int64, device="cuda")

    def call(n_aggs=1, n_rows=n, src_edit=None, dst_edit=None, opts_edit=None, null=()):
        src, dst, opts = (H.AggSrc * 2)(), (H.AggDst * 2)(), H.GroupAggOpts()
        opts.struct_size = C.sizeof(H.GroupAggOpts)
        for k, o in enumerate((out, out2)):
            src[k].data, src[k].type, src[k].op = col.data_ptr(), H.HMJ_TYPE_I32, H.HMJ_AGG_SUM
            dst[k].data = o.data_ptr()
        if src_edit:
            src_edit(src)
        if dst_edit:
            dst_edit(dst)
        if opts_edit:
            opts_edit(opts)
        rc = L.hmj_group_agg_device(h, None if "src" in null else src, n_aggs, n_rows, None if "dst" in null else dst,
                                    None if "opts" in null else C.byref(opts))
        return rc, L.hmj_last_error(h).decode()

    def set_(i, **kw):
        def edit(arr):
            for k, v in kw.items():
                if k in ("bits", "bit_offset"):
                    setattr(arr[i].validity, k, v)
                else:
                    setattr(arr[i], k, v)
        return edit

    def both(*edits):
        return lambda arr: [e(arr) for e in edits]

    cases = {
        "NULL src": (dict(null=("src",)), "NULL"),
        "NULL dst": (dict(null=("dst",)), "NULL"),
        "NULL opts": (dict(null=("opts",)), "NULL"),
        "small struct_size": (dict(opts_edit=lambda o: setattr(o, "struct_size", 4)), "struct_size"),
        "reserved": (dict(opts_edit=lambda o: setattr(o, "reserved", 1)), "reserved"),
        "n_aggs 0": (dict(n_aggs=0), "n_aggs"),
        "n_aggs 65": (dict(n_aggs=H.HMJ_MAX_AGGS + 1), "n_aggs"),
        "unknown type": (dict(src_edit=set_(0, type=10)), "type"),
        "unknown op": (dict(src_edit=set_(0, op=5)), "op"),
        "NULL data": (dict(src_edit=set_(0, data=None)), "source data is NULL"),
        "misaligned data": (dict(src_edit=set_(0, data=col.data_ptr() + 2)), "aligned"),
        "misaligned data (8)": (dict(src_edit=set_(0, data=col64.data_ptr() + 4, type=H.HMJ_TYPE_F64)), "aligned"),
        "NULL dst data": (dict(dst_edit=set_(0, data=None)), "destination data is NULL"),
        "misaligned dst data": (dict(dst_edit=set_(0, data=out.data_ptr() + 4)), "aligned"),
        "misaligned dst validity": (dict(dst_edit=set_(0, validity=words.data_ptr() + 4)), "aligned to 8"),
        "bit_offset overflow": (dict(src_edit=set_(0, bits=bitmap.data_ptr(), bit_offset=(1 << 64) - n + 1)), "overflows"),
        "wrong n_rows": (dict(n_rows=n + 1), "n_rows"),
        "dst over a source column": (dict(dst_edit=set_(0, data=col64.data_ptr()), src_edit=set_(1, data=col64.data_ptr(), type=H.HMJ_TYPE_I64),
                                          n_aggs=2), "overlaps"),
        "dst over a source bitmap": (dict(dst_edit=set_(0, validity=bitmap.data_ptr()), src_edit=set_(0, bits=bitmap.data_ptr())), "overlaps"),
        "dst over another dst": (dict(dst_edit=set_(1, data=out.data_ptr() + 8), n_aggs=2), "overlaps"),
        "dst bitmap over a dst": (dict(dst_edit=set_(1, validity=out.data_ptr()), n_aggs=2), "overlaps"),
    }
    for name, (kw, needle) in cases.items():
        rc, msg = call(**kw)
        assert rc == HMJ_E_ARG and needle in msg, (name, rc, msg)
        rc, msg = call(n_aggs=2)  # the same ctx, a good call of two
        assert rc == 0, (name, msg)
    assert out.cpu().numpy()[:ng].tolist() == out2.cpu().numpy()[:ng].tolist()
    assert out.cpu().numpy()[ng:].tolist() == [0] * 8  # nothing behind the groups is written
    assert_aggs(H, aggregate(ex, H, good, ng), want, good, ng)
    # COUNT may come without data
    rc, msg = call(src_edit=set_(0, data=None, op=H.HMJ_AGG_COUNT))
    assert rc == 0 and out.cpu().numpy()[:ng].tolist() == cols["count"].tolist(), msg


# ---- the randomized sweep ----------------------------------------------------------------------------------------------------
def test_randomized_sweep(ex, H):
    seed, iters = sweep_params()
    rng = np.random.default_rng(seed)
    for it in range(iters):
        case = draw_agg_case(rng, H)
        res, cols, _, _ = check(ex, H, case["key"], case["aggs"], case["ordered"], want_validity=bool(it % 3), tag=("sweep", seed, it))
        assert res.n_groups == len(np.unique(case["key"]))
