"""hmj_order_by_device on the GPU (include/hmj.h, "ordering rows by typed, string and mixed keys") against
`expected_order_by`: the order is total with the row index, so the map must be equal entry by entry.  Every call also checks
n_distinct and n_tied_rows against the reference's own order and n_rounds against the bound 1 + ceil(max(0, S - 8) / 4)."""
import ctypes as C

import numpy as np
import pytest

from test_order_by_cpu import DESC, EDGE_STRINGS, NULLS_FIRST, STRING, draw_order_case, edge_tables, special_values, sweep_params

pytestmark = pytest.mark.gpu
HMJ_E_ARG = -1


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


def spec(values, flags=0, valid=None, bit_offset=0, pad=0):
    kind = str(values.dtype) if isinstance(values, np.ndarray) else STRING
    return {"type": kind, "values": values, "flags": flags, "valid": valid, "bit_offset": bit_offset, "pad": pad}


def dev_cols(H, cols):
    """The columns of a case on the device as Executor.order_by_device takes them.  A string column's chars start `pad`
    bytes into the buffer (offsets[0] == pad); the bytes of a NULL slot stay where they are: garbage under it."""
    out = []
    for c in cols:
        if c["type"] == STRING:
            enc = [b"" if v is None else bytes(v) for v in c["values"]]
            lens = np.fromiter((len(b) for b in enc), dtype=np.int64, count=len(enc))
            offsets = np.full(len(enc) + 1, c["pad"], np.int64)
            offsets[1:] += np.cumsum(lens)
            raw = b"\xee" * c["pad"] + b"".join(enc)
            chars = dev(np.frombuffer(raw, np.uint8)) if raw else None
            col = (chars, dev(offsets))
        else:
            col = dev(c["values"])
        if c["valid"] is None:
            out.append((col, c["flags"]))
        else:
            out.append((col, c["flags"], H.pack_validity(c["valid"], c["bit_offset"], device="cuda"), c["bit_offset"]))
    return out


def equal_to_previous(cols, order):
    """eq[j]: the row at sorted position j has the whole key of the row at position j - 1 (eq[0] False)."""
    n = len(order)
    eq = np.ones(n, bool)
    if n:
        eq[0] = False
    idx = order.astype(np.int64)
    for c in cols:
        ok = np.ones(n, bool) if c["valid"] is None else np.asarray(c["valid"], bool)
        if c["type"] == STRING:
            vals = [c["values"][i] for i in idx]
            same = np.array([False] + [vals[j] == vals[j - 1] for j in range(1, n)], bool)[:n]
        else:
            v = c["values"]
            bits = v.view("u%d" % v.dtype.itemsize).copy()
            if v.dtype.kind == "f":
                bits[np.isnan(v)] = ~bits.dtype.type(0)  # every NaN is one value
            b = bits[idx]
            same = np.concatenate([[False], b[1:] == b[:-1]])[:n]
        o = ok[idx]
        both_null = np.concatenate([[False], ~o[1:] & ~o[:-1]])[:n]
        both_ok = np.concatenate([[False], o[1:] & o[:-1]])[:n]
        eq &= both_null | (both_ok & same)
    return eq


def check(ex, H, cols, tag="", n=None):
    n = len(cols[0]["values"]) if n is None else n
    got, info = ex.order_by_device(dev_cols(H, cols), n=n)
    columns = [(c["values"], c["flags"], c["valid"]) for c in cols]
    want = H.expected_order_by(columns)
    got = got.cpu().numpy().view(np.uint64)
    if not np.array_equal(got, want):
        bad = int(np.nonzero(got != want)[0][0])
        raise AssertionError("%s: the map differs from position %d on: got row %d, want row %d (%s)" % (tag, bad, got[bad], want[bad], info))
    eq = equal_to_previous(cols, want)
    tied = eq.copy()
    tied[:-1] |= eq[1:]
    assert info["n_distinct"] == int(np.count_nonzero(~eq)), (tag, info)
    assert info["n_tied_rows"] == int(np.count_nonzero(tied)), (tag, info)
    S = int(H.order_stream_bytes(columns).max()) if n else 0
    bound = 1 + max(0, -(-(S - 8) // 4))
    assert (info["n_rounds"] == 0) if n <= 1 else (1 <= info["n_rounds"] <= bound), (tag, info, S)
    return got, info


# ---- sizes ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 511, 512, 513, 4095, 4096, 4097, 5000])
def test_boundary_sizes_in_two_layouts(ex, H, n):
    rng = np.random.default_rng(1000 + n)
    i64 = rng.integers(-40, 40, size=n).astype(np.int64) * (1 << 40)
    _, info = check(ex, H, [spec(i64)], "i64 n=%d" % n)
    assert info["n_rounds"] == (0 if n <= 1 else 1)
    u8 = rng.integers(3, 5, size=n).astype(np.uint8)
    strs = [b"twenty-byte-prefix-->" [:20] + bytes(rng.integers(0x61, 0x64, size=2).astype(np.uint8)) for _ in range(n)]
    _, info = check(ex, H, [spec(u8), spec(strs)], "u8, strings n=%d" % n)
    if n >= 63:  # rows that agree in the U8 and in twenty string bytes: the difference sits 24 stream bytes in
        assert info["n_rounds"] >= 3, info


# ---- types, edge values, NULLs ---------------------------------------------------------------------------------------------------
def test_every_type_ascending_and_descending_with_edge_values(ex, H):
    for tag, columns in edge_tables():
        cols = [spec(v, f, ok, bit_offset=3 if ok is not None else 0) for v, f, ok in columns]
        check(ex, H, cols, tag)


@pytest.mark.parametrize("offset", [0, 3, 67])
def test_nulls_first_and_last_at_bit_offsets_with_garbage_under_null_slots(ex, H, offset):
    rng = np.random.default_rng(50 + offset)
    n = 1500
    valid = rng.random(n) >= 0.3
    f64 = special_values("float64", rng, n, 6)
    i16 = special_values("int16", rng, n, 4)
    strs = [EDGE_STRINGS[k] for k in rng.integers(0, len(EDGE_STRINGS), size=n)]
    for flags in (0, DESC, NULLS_FIRST, DESC | NULLS_FIRST):
        for maker in (lambda: [spec(f64, flags, valid, offset)], lambda: [spec(i16, flags, valid, offset), spec(strs, flags ^ DESC, ~valid, offset, pad=5)],
                      lambda: [spec(strs, flags, valid, offset, pad=3), spec(i16, 0)]):
            cols = maker()
            got, _ = check(ex, H, cols, "flags %d offset %d" % (flags, offset))
            # the same call over other bytes under the NULL slots gives the same map
            for c in cols:
                if c["valid"] is None:
                    continue
                if c["type"] == STRING:
                    c["values"] = [v if ok else b"\xff garbage under a NULL slot" for v, ok in zip(c["values"], c["valid"])]
                else:
                    junk = c["values"].copy()
                    junk[~c["valid"]] = special_values(c["type"], rng, int(np.count_nonzero(~c["valid"])))
                    c["values"] = junk
            again, _ = check(ex, H, cols, "garbage, flags %d offset %d" % (flags, offset))
            assert np.array_equal(got, again)


def test_nan_and_zero_handling_through_the_map(ex, H):
    for dt in ("float32", "float64"):
        vals = np.array([np.nan, 1.0, -0.0, 0.0, -np.nan, np.inf, -np.inf, 0.0, -0.0, np.nan], dt)
        got, info = check(ex, H, [spec(vals)], dt)
        assert got.tolist() == [6, 2, 8, 3, 7, 1, 5, 0, 4, 9] and info["n_distinct"] == 6 and info["n_tied_rows"] == 7
        got, _ = check(ex, H, [spec(vals, DESC)], dt + " desc")
        assert got.tolist() == [0, 4, 9, 5, 1, 3, 7, 2, 8, 6]


def test_all_equal_and_all_distinct_keys(ex, H):
    n = 3000
    for cols in ([spec(np.full(n, -7, np.int32))], [spec([b"same string, 21 bytes"] * n), spec(np.full(n, 2.5, np.float32), DESC)]):
        got, info = check(ex, H, cols, "all equal")
        assert got.tolist() == list(range(n)) and info["n_distinct"] == 1 and info["n_tied_rows"] == n
    rng = np.random.default_rng(3)
    u32 = (rng.permutation(n).astype(np.uint32) * np.uint32(1000003))
    _, info = check(ex, H, [spec(u32)], "all distinct")
    assert info["n_rounds"] == 1 and info["n_tied_rows"] == 0 and info["n_distinct"] == n


def test_string_block_boundaries(ex, H):
    rng = np.random.default_rng(8)
    strs = []
    for ln in (0, 1, 6, 7, 8, 13, 14, 15, 21, 22):
        for tail in (b"", b"\x00", b"\xff", b"a"):
            strs.append((b"abcdefghijklmnopqrstuvwxyz"[:ln] + tail))
    strs = strs + strs[::3]
    strs = [strs[k] for k in rng.permutation(len(strs))]
    for flags in (0, DESC):
        check(ex, H, [spec(strs, flags, pad=1)], "blocks flags %d" % flags)
        check(ex, H, [spec(strs, flags), spec(strs, flags ^ DESC)], "two string columns flags %d" % flags)


def test_a_long_shared_prefix_costs_rounds_over_few_rows(ex, H):
    rng = np.random.default_rng(9)
    prefix = bytes(rng.integers(0, 256, size=300).astype(np.uint8))
    strs = [prefix + bytes(rng.integers(0x61, 0x63, size=3).astype(np.uint8)) for _ in range(130)]
    other = [bytes(rng.integers(0, 256, size=9).astype(np.uint8)) for _ in range(2000)]
    rows = strs + other
    rows = [rows[k] for k in rng.permutation(len(rows))]
    _, info = check(ex, H, [spec(rows)], "long prefix")
    assert info["n_rounds"] >= 1 + (8 * (300 // 7) - 8) // 8, info


def test_eight_columns_of_mixed_types(ex, H):
    rng = np.random.default_rng(10)
    n = 4000
    valid = rng.random(n) >= 0.2
    strs = [EDGE_STRINGS[k] for k in rng.integers(0, 6, size=n)]
    cols = [spec(special_values("int8", rng, n, 2), DESC), spec(strs, 0, valid, 3), spec(special_values("float32", rng, n, 3), NULLS_FIRST, valid, 67),
            spec(special_values("uint16", rng, n, 2)), spec(strs, DESC | NULLS_FIRST, ~valid, 0, pad=7), spec(special_values("int64", rng, n, 2), DESC),
            spec(special_values("float64", rng, n, 2)), spec(special_values("uint32", rng, n, 3), DESC)]
    _, info = check(ex, H, cols, "eight columns")
    assert info["n_rounds"] >= 2


def test_a_large_shape_whose_inner_sort_takes_its_msd_form(ex, H):
    rng = np.random.default_rng(12)
    n = (1 << 22) + 1
    a = rng.integers(-2 ** 31, 2 ** 31, size=n).astype(np.int32)
    b = rng.integers(0, 1 << 16, size=n).astype(np.uint16)
    a[rng.integers(0, n, size=n // 8)] = a[0]  # ties in the first column
    got, info = ex.order_by_device([(dev(a), 0), (dev(b), 0)])
    want = np.lexsort((b, a)).astype(np.uint64)
    assert np.array_equal(got.cpu().numpy().view(np.uint64), want)
    assert info["n_rounds"] == 1  # six stream bytes: one word holds the whole key


def test_a_segment_that_spans_workgroups_beside_resolved_rows(ex, H):
    rng = np.random.default_rng(14)
    n = 9000
    u64 = np.concatenate([np.full(6000, 0x0123456789ABCDEF, np.uint64), rng.integers(0, 2 ** 63, size=n - 6000).astype(np.uint64)])
    i16 = rng.integers(-300, 300, size=n).astype(np.int16)
    perm = rng.permutation(n)
    _, info = check(ex, H, [spec(u64[perm]), spec(i16[perm], DESC)], "spanning segment")
    assert info["n_rounds"] == 2


# ---- refusals ----------------------------------------------------------------------------------------------------------------
def test_every_refusal_names_its_reason_and_leaves_the_ctx_usable(ex, H):
    import torch

    rng = np.random.default_rng(13)
    n = 1000
    vals = special_values("int32", rng, n, 20)
    strs = [EDGE_STRINGS[k] for k in rng.integers(0, len(EDGE_STRINGS), size=n)]
    good = [spec(vals, DESC, rng.random(n) >= 0.1, 3), spec(strs)]
    L, h = ex.L, ex.h
    col = dev(vals)
    chars, offs = H.pack_strings(strs, "cuda")
    bitmap = H.pack_validity(np.ones(n, bool), 0, device="cuda")
    out = torch.zeros(n + 8, dtype=torch.int64, device="cuda")

    def call(n_cols=2, rows=n, edit=None, opts_edit=None, null=(), map_ptr=None):
        arr, opts = (H.OrderCol * 9)(), H.OrderOpts()
        opts.struct_size = C.sizeof(H.OrderOpts)
        for k in range(9):
            arr[k].type, arr[k].data = H.HMJ_TYPE_I32, col.data_ptr()
        arr[1].type, arr[1].data, arr[1].offsets = H.HMJ_ORDER_LARGE_STRING, chars.data_ptr(), offs.data_ptr()
        if edit:
            edit(arr)
        if opts_edit:
            opts_edit(opts)
        rc = L.hmj_order_by_device(h, None if "cols" in null else arr, n_cols, rows, None if "map" in null else C.c_void_p(map_ptr or out.data_ptr()),
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
        (dict(null=("cols",)), "cols / opts is NULL"),
        (dict(null=("opts",)), "cols / opts is NULL"),
        (dict(null=("map",)), "row_map_out is NULL"),
        (dict(map_ptr=out.data_ptr() + 4), "row_map_out is not aligned"),
        (dict(n_cols=0), "n_cols must be in 1..8"),
        (dict(n_cols=9), "n_cols must be in 1..8"),
        (dict(edit=set_(0, type=10)), "column 0 has unknown type 10"),
        (dict(edit=set_(0, type=17)), "column 0 has unknown type 17"),
        (dict(edit=set_(1, flags=4)), "column 1 has unknown flag bits"),
        (dict(opts_edit=set_opts(reserved=1)), "reserved must be 0"),
        (dict(opts_edit=set_opts(reserved2=1)), "reserved must be 0"),
        (dict(opts_edit=set_opts(struct_size=H.OrderOpts.reserved2.offset)), "struct_size too small"),
        (dict(edit=set_(0, data=None)), "column 0: data is NULL"),
        (dict(edit=set_(0, data=col.data_ptr() + 2)), "column 0: data is not aligned to its width (4)"),
        (dict(edit=set_(0, offsets=offs.data_ptr())), "column 0: offsets set on a fixed-width column"),
        (dict(edit=set_(1, offsets=None)), "column 1: offsets is NULL"),
        (dict(edit=set_(1, offsets=offs.data_ptr() + 4)), "column 1: offsets is not aligned"),
        (dict(edit=set_(0, bits=bitmap.data_ptr(), bit_offset=2 ** 64 - 5)), "column 0: validity bit_offset + n overflows"),
        (dict(rows=1 << 32), "more than 2^32 - 1 rows"),
        (dict(map_ptr=col.data_ptr()), "column 0: row_map_out overlaps"),
        (dict(n_cols=2, map_ptr=offs.data_ptr() + 8 * (n - 3)), "column 1: row_map_out overlaps"),
        (dict(edit=set_(0, bits=out.data_ptr() + 8, bit_offset=0)), "column 0: row_map_out overlaps"),
    ]
    for kw, needle in refusals:
        rc, msg = call(**kw)
        assert rc == HMJ_E_ARG and needle in msg, (kw.keys(), rc, msg)
        check(ex, H, good, "after " + needle)
    # a prefix of the opts struct is a valid, older caller: nothing behind reserved2 is written
    rc, msg = call(opts_edit=set_opts(struct_size=H.OrderOpts.ms_key.offset))
    assert rc == 0, msg
    # found on the device, before anything follows an offset: the lowest-numbered column, its first row
    bad = offs.clone()
    bad[[700, 400]] = bad[[700, 400]] + 1000  # offsets[401] < offsets[400] first, offsets[701] < offsets[700] later
    bad2 = offs.clone()
    bad2[10] = bad2[10] + 1000
    rc, msg = call(n_cols=3, edit=lambda a: [set_(1, offsets=bad.data_ptr())(a),
                                             set_(2, type=H.HMJ_ORDER_LARGE_STRING, data=chars.data_ptr(), offsets=bad2.data_ptr())(a)])
    assert rc == HMJ_E_ARG and "column 1: offsets decrease at row 400 (offsets[401] < offsets[400])" in msg, msg
    check(ex, H, good, "after decreasing offsets")
    rc, msg = call(edit=set_(1, data=None))
    assert rc == HMJ_E_ARG and "column 1: data is NULL but keys have bytes" in msg, msg
    check(ex, H, good, "after data == NULL")
    # data == NULL is legal when every string is empty; n == 0 writes nothing
    empties = torch.full((n + 1,), 9, dtype=torch.int64, device="cuda")
    got, info = ex.order_by_device([((None, empties), 0)])
    assert got.cpu().numpy().tolist() == list(range(n)) and info["n_distinct"] == 1
    # a NULL slot holds no key bytes, whatever its offsets span: data == NULL stays legal when only NULL slots have a length
    spans = np.zeros(n + 1, np.int64)
    holes = np.zeros(n, bool)
    holes[[5, 700]] = True
    spans[6:] += 4
    spans[701:] += 9
    got, info = ex.order_by_device([((None, dev(spans)), H.HMJ_ORDER_NULLS_FIRST, H.pack_validity(~holes, 3, device="cuda"), 3)])
    assert got.cpu().numpy().tolist() == [5, 700] + [i for i in range(n) if i not in (5, 700)] and info["n_distinct"] == 2
    out.fill_(-1)
    rc, msg = call(rows=0)
    assert rc == 0 and bool((out == -1).all()), msg
    rc, msg = call(rows=0, map_ptr=out.data_ptr() + 4)  # the map's alignment matters with n > 0 only
    assert rc == 0 and bool((out == -1).all()), msg


# ---- the call among the others on one ctx ------------------------------------------------------------------------------------------
def test_group_aggregate_order_and_take_without_leaving_the_device(H):
    import os

    import torch

    os.environ["HMJ_GTABLE"] = "0"  # (the join below would otherwise take the global table and partition nothing)
    try:
        ex = H.Executor(0)
    finally:
        del os.environ["HMJ_GTABLE"]
    try:
        rng = np.random.default_rng(21)
        n = 6000
        names = [b"name-%03d" % k for k in rng.integers(0, 80, size=n)]
        price = np.round(rng.standard_normal(n) * 50, 0) + 0.0  # (no -0.0)
        price[rng.random(n) < 0.3] = 10.0  # sums that tie
        chars, offs = H.pack_strings(names, "cuda")
        res, _ = ex.group_mixed_device([(chars, offs)], flags=H.HMJ_MATERIALIZE, want=H.HMJ_GROUP_ROW_MAP)
        ng = int(res.n_groups)
        cols = ex.group_rows_to_numpy(res)
        aggs = [(H.HMJ_AGG_SUM, dev(price), None)]
        (sums, _, _), = ex.group_agg_device(aggs)[0]
        key_chars, key_offs, _, _ = ex.take_str_device(chars, offs, (res.first_row, ng))
        # SELECT name, sum(price) GROUP BY name ORDER BY sum(price) DESC, name
        rmap, info = ex.order_by_device([(sums, H.HMJ_ORDER_DESC), ((key_chars, key_offs), 0)])
        assert info["n_distinct"] == ng and info["n_tied_rows"] == 0
        out_chars, out_offs, _, _ = ex.take_str_device(key_chars, key_offs, rmap)
        (out_sums,), _, _ = ex.take_cols_device([sums], rmap)
        # the numpy restatement: sums per name in double, the groups' own order of additions left to the group entry's test
        want_sums = H.expected_group_aggs(cols["group_of_row"], ng, [(H.HMJ_AGG_SUM, price, None)])[0]["values"]
        group_names = [names[int(r)] for r in cols["first_row"]]
        table = sorted(zip(group_names, want_sums.tolist()), key=lambda t: (-t[1], t[0]))
        assert H.unpack_strings(out_chars, out_offs) == [t[0] for t in table]
        assert out_sums.cpu().numpy().tolist() == [t[1] for t in table]
        # the live grouping is kept: a second aggregate call still succeeds
        (again, _, _), = ex.group_agg_device(aggs)[0]
        assert torch.equal(again, sums)
        # a prepared build side is discarded, as after hmj_sort_u64_device
        nb, npb = 300000, 200000
        bd, pd = ex.gen_build(nb), ex.gen_probe(npb, nb, miss_mod=4)
        want = ex.join_device(bd, pd, 0).checks()
        ex.set_profiling(True)
        ex.prepare_build(bd, npb)
        r = ex.join_device(bd, pd, 0)
        assert r.checks() == want and ex.last_timing()["path"] & H.HMJ_PATH_PREPARED  # (taken when nothing comes between)
        ex.prepare_build(bd, npb)
        plan_before = ex.last_plan()
        ex.order_by_device([(sums, 0)])
        assert ex.last_plan() == plan_before  # hmj_last_plan keeps describing the last join
        r = ex.join_device(bd, pd, 0)
        t = ex.last_timing()
        assert r.checks() == want and not (t["path"] & H.HMJ_PATH_PREPARED) and t["ms_partition_build"] > 0.0
    finally:
        ex.close()


# ---- the randomized sweep ------------------------------------------------------------------------------------------------------
def test_randomized_sweep(ex, H):
    seed, iters = sweep_params()
    rng = np.random.default_rng(seed)
    for it in range(iters):
        case = draw_order_case(rng, it)
        check(ex, H, case["cols"], "sweep seed %d case %d (n=%d, %s)" % (seed, it, case["n"], [(c["type"], c["flags"]) for c in case["cols"]]),
              n=case["n"])
