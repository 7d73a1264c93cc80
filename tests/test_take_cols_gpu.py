"""GPU checks of hmj_take_cols_device (fixed-width columns taken through a row map, Arrow validity out) against
`expected_take` of test_take_cols_cpu.py, byte for byte: values (zero under NULL slots), bitmap words including the padding,
null counts and the HMJ_TAKE_NO_ROW count.  Sizes around the wave and workgroup edges and one past the grid cap, source
bit offsets, all five widths in one call, column counts across the 8-column launch chunk, the map shapes, out-of-range map
entries (an argument error, never a load), every other argument error, and the takes behind a FULL_OUTER multi-column join,
a string kind join and a prepared build side."""
import ctypes as C
import random

import numpy as np
import pytest

from test_join_cols_gpu import columns
from test_join_cols_kinds_cpu import BUILD, FULL_OUTER
from test_join_cols_kinds_gpu import dev_rel
from test_join_cols_nulls_gpu import dev_valid, draw_masks, drawn, null_rows
from test_take_cols_cpu import NO_ROW, expected_take

pytestmark = pytest.mark.gpu
HMJ_E_ARG = -1
SIZES = [0, 1, 63, 64, 65, 255, 256, 257, 1000]
OFFSETS = [0, 1, 7, 13, 63]
DTYPES = {1: np.uint8, 2: np.int16, 4: np.float32, 8: np.int64, 16: np.int64}  # (compared as bytes: NaN patterns included)
ALL_WIDTHS = [1, 2, 4, 8, 16]
PATTERN = 0xA5  # the bytes under the NULL slots of every source column


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


def draw_col(rng, width, n, mask=None):
    """n random values of `width` bytes ([n,2] int64 for 16); the bytes under the NULL slots of `mask` spell PATTERN."""
    raw = rng.integers(0, 256, size=(n, width), dtype=np.uint8)
    if mask is not None:
        raw[~mask] = PATTERN
    col = raw.reshape(-1).view(DTYPES[width])
    return col.reshape(n, 2) if width == 16 else col


def draw_case(rng, widths, n_src, n_out, frac_no_row=0.3, with_mask=lambda c: c % 2 == 0, frac_null=0.3):
    masks = [(rng.random(n_src) >= frac_null) if with_mask(c) else None for c in range(len(widths))]
    cols = [draw_col(rng, w, n_src, m) for w, m in zip(widths, masks)]
    row_map = rng.integers(0, max(n_src, 1), size=n_out).astype(np.uint64)
    if n_src == 0:
        frac_no_row = 1.0
    row_map[rng.random(n_out) < frac_no_row] = NO_ROW
    return cols, masks, row_map


def dev_map(row_map):
    import torch

    return torch.from_numpy(np.asarray(row_map, np.uint64).view(np.int64).copy()).cuda()


def as_bytes(a):
    return np.ascontiguousarray(a).reshape(-1).view(np.uint8)


def run_take(H, ex, cols, masks, row_map, offs=None, wants=True):
    """Upload and take through the Executor: (outputs, bitmap words, info)."""
    import torch

    dcols = [torch.from_numpy(c).cuda() for c in cols]
    offs = [offs or 0] * len(cols) if not isinstance(offs, (list, tuple)) else list(offs)
    valid = None if masks is None else [None if m is None else (H.pack_validity(m, o, "cuda"), o) for m, o in zip(masks, offs)]
    return ex.take_cols_device(dcols, dev_map(row_map), valid=valid, want_validity=wants)


def check_take(H, ex, cols, masks, row_map, offs=None, wants=True, tag=()):
    """One take through the Executor against expected_take.  offs: the bit offset of every source bitmap (one value, or one
    per column); wants: True, False or one bool per column.  Returns the info dict."""
    want_d, want_w, want_nulls, want_no = expected_take(cols, masks, row_map)
    outs, words, info = run_take(H, ex, cols, masks, row_map, offs, wants)
    wants = [bool(wants)] * len(cols) if isinstance(wants, bool) else list(wants)
    assert (words is None) == (not any(wants)), tag
    for c, col in enumerate(cols):
        got = outs[c].cpu().numpy()
        assert got.dtype == col.dtype and got.shape == want_d[c].shape, (tag, c)
        bad = np.flatnonzero(as_bytes(got) != as_bytes(want_d[c]))
        assert not len(bad), (tag, c, bad[:5])
        if wants[c]:
            gw = words[c].cpu().numpy().view(np.uint64)
            assert np.array_equal(gw, want_w[c]), (tag, c, np.flatnonzero(gw != want_w[c])[:5])
        else:
            assert words is None or words[c] is None, (tag, c)
    assert info["null_count"] == want_nulls and info["n_no_row"] == want_no, (tag, info, want_nulls, want_no)
    return info


# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_out", SIZES)
def test_sizes_and_offsets(H, ex, n_out):
    """Every output size (none, a single row, one short of / exactly / one past a wave and a workgroup, several workgroups)
    crossed with source bit offsets inside a byte, across a byte and one short of a 64-bit word; all five widths in one
    call, bitmaps on columns 0, 2 and 4 only, no output bitmap for columns 1 and 4; about 30 % NO_ROW."""
    rng = np.random.default_rng(n_out)
    n_src = n_out + 37
    cols, masks, row_map = draw_case(rng, ALL_WIDTHS, n_src, n_out)
    for off in OFFSETS:
        info = check_take(H, ex, cols, masks, row_map, offs=[off, 0, (off * 5 + 3) % 64, 0, off], wants=[True, False, True, True, False],
                          tag=(n_out, off))
    if n_out == 1000:
        assert info["n_no_row"] > 200 and min(info["null_count"]) >= info["n_no_row"] and max(info["null_count"]) > info["n_no_row"] + 100


def test_a_second_grid_stride_step(H, ex):
    """The kernel's grid is capped at 16 workgroups of 256 rows per compute unit, so with n_out = 16 * 256 * CUs + 257 the
    first 257 lanes take a second grid-stride step (and the last wave of it is a partial one)."""
    import torch

    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n_out = 16 * 256 * cus + 257
    rng = np.random.default_rng(5)
    cols, masks, row_map = draw_case(rng, [4, 16, 1], 5000, n_out, with_mask=lambda c: c != 1)
    info = check_take(H, ex, cols, masks, row_map, offs=[13, 0, 63], wants=[True, True, False], tag=("grid", n_out))
    assert info["n_no_row"] > n_out // 4


@pytest.mark.parametrize("n_cols", [1, 8, 9, 17, 64])
def test_column_counts(H, ex, n_cols):
    """Column counts up to, across (9, 17) and far beyond the 8 columns of one launch; widths cycle through all five, a
    bitmap on every third column, no output bitmap for the odd columns, a bit offset of its own per column."""
    rng = np.random.default_rng(n_cols)
    widths = [ALL_WIDTHS[c % 5] for c in range(n_cols)]
    cols, masks, row_map = draw_case(rng, widths, 200, 300, with_mask=lambda c: c % 3 == 0)
    info = check_take(H, ex, cols, masks, row_map, offs=[(7 * c) % 64 for c in range(n_cols)], wants=[c % 2 == 0 for c in range(n_cols)],
                      tag=(n_cols,))
    assert len(info["null_count"]) == n_cols and info["n_no_row"] > 50
    check_take(H, ex, cols, masks, row_map, wants=False, tag=(n_cols, "no bitmaps"))


def test_map_shapes(H, ex):
    rng = np.random.default_rng(17)
    n = 777
    widths = [8, 2, 16]
    cols, masks, _ = draw_case(rng, widths, n, n, with_mask=lambda c: c < 2)
    check_take(H, ex, cols, masks, np.arange(n, dtype=np.uint64), offs=5, tag=("identity",))
    check_take(H, ex, cols, masks, rng.permutation(n).astype(np.uint64), offs=5, tag=("permutation",))
    # every entry the same row of a one-row source: valid in column 0, NULL in column 1
    one = [c[:1] for c in cols]
    m1 = [np.array([True]), np.array([False]), None]
    info = check_take(H, ex, one, m1, np.zeros(500, np.uint64), offs=[63, 7, 0], tag=("one row",))
    assert info["null_count"] == [0, 500, 0]
    # a source much larger than the output
    big, bm, bmap = draw_case(rng, [4, 1], 200000, 500, frac_no_row=0.0, with_mask=lambda c: c == 1)
    info = check_take(H, ex, big, bm, bmap, offs=1, tag=("large source",))
    assert info["n_no_row"] == 0 and 100 < info["null_count"][1] < 200
    # nothing but NO_ROW over an empty source: NULL source pointers
    empty, em, emap = draw_case(rng, ALL_WIDTHS, 0, 321)
    assert all(len(c) == 0 for c in empty) and (emap == NO_ROW).all()
    info = check_take(H, ex, empty, em, emap, tag=("empty source",))
    assert info["null_count"] == [321] * 5 and info["n_no_row"] == 321
    check_take(H, ex, empty, None, emap[:0], tag=("empty both",))


def test_all_valid(H, ex):
    """No NO_ROW and no source bitmap: all-ones words, zero padding, null_count 0."""
    import torch

    rng = np.random.default_rng(3)
    n_out = 130
    cols, _, _ = draw_case(rng, ALL_WIDTHS, 90, 0, with_mask=lambda c: False)
    row_map = rng.integers(0, 90, size=n_out).astype(np.uint64)
    info = check_take(H, ex, cols, None, row_map, tag=("all valid",))
    assert info["null_count"] == [0] * 5 and info["n_no_row"] == 0
    _, words, _ = ex.take_cols_device([torch.from_numpy(c).cuda() for c in cols], dev_map(row_map))
    for w in words:
        assert w.cpu().numpy().view(np.uint64).tolist() == [2 ** 64 - 1, 2 ** 64 - 1, 3]


def raw_take(H, ex, src_t, widths, valid, map_t, n_src, n_out, out_t, word_t, reserved=0, struct_size=None, opts_reserved=0):
    """hmj_take_cols_device through ctypes alone, on tensors the caller allocated (None entries: NULL pointers).
    Returns (status, TakeDst array, TakeOpts)."""
    k = len(widths)
    src, dst, opts = (H.TakeSrc * max(k, 1))(), (H.TakeDst * max(k, 1))(), H.TakeOpts()
    for c in range(k):
        src[c].data = src_t[c] if isinstance(src_t[c], int) or src_t[c] is None else src_t[c].data_ptr()
        src[c].width = widths[c]
        src[c].reserved = reserved
        if valid is not None and valid[c] is not None:
            src[c].validity.bits = valid[c][0] if isinstance(valid[c][0], int) else valid[c][0].data_ptr()
            src[c].validity.bit_offset = valid[c][1]
        dst[c].data = out_t[c] if isinstance(out_t[c], int) or out_t[c] is None else out_t[c].data_ptr()
        dst[c].validity = word_t[c] if isinstance(word_t[c], int) or word_t[c] is None else word_t[c].data_ptr()
    opts.struct_size = C.sizeof(H.TakeOpts) if struct_size is None else struct_size
    opts.reserved = opts_reserved
    mp = map_t if isinstance(map_t, int) or map_t is None else map_t.data_ptr()
    ex._sync_stream()
    rc = ex.L.hmj_take_cols_device(ex.h, src, k, n_src, C.c_void_p(mp), n_out, dst, C.byref(opts))
    return rc, dst, opts


@pytest.mark.parametrize("n_out", [1, 63, 65, 257, 1000])
def test_bytes_under_null_slots_and_padding(H, ex, n_out):
    """The source bytes under NULL slots spell a pattern and the output buffers are filled with 0xFF before the call: the
    output bytes under every NULL slot are 0, the padding bits of the last word are 0, and a column without an output
    bitmap still reports its null count."""
    import torch

    rng = np.random.default_rng(1000 + n_out)
    n_src = 300
    cols, masks, row_map = draw_case(rng, ALL_WIDTHS, n_src, n_out, with_mask=lambda c: True, frac_null=0.4)
    for c, m in zip(cols, masks):
        assert (as_bytes(c).reshape(n_src, -1)[~m] == PATTERN).all()
    want_d, want_w, want_nulls, want_no = expected_take(cols, masks, row_map)
    src_t = [torch.from_numpy(c).cuda() for c in cols]
    valid = [(H.pack_validity(m, 13, "cuda"), 13) for m in masks]
    out_t = [torch.full((n_out * w,), 0xFF, dtype=torch.uint8, device="cuda") for w in ALL_WIDTHS]
    word_t = [torch.full(((n_out + 63) // 64,), -1, dtype=torch.int64, device="cuda") if c != 3 else None for c in range(5)]
    rc, dst, opts = raw_take(H, ex, src_t, ALL_WIDTHS, valid, dev_map(row_map), n_src, n_out, out_t, word_t)
    assert rc == 0, ex.L.hmj_last_error(ex.h)
    for c, w in enumerate(ALL_WIDTHS):
        got = out_t[c].cpu().numpy().reshape(n_out, w)
        assert np.array_equal(got.reshape(-1), as_bytes(want_d[c])), c
        null = ~H.unpack_validity(want_w[c], n_out)
        assert null.sum() == want_nulls[c] > 0 or n_out == 1
        assert not got[null].any(), c  # zero bytes, not the pattern and not what the buffer held
        if word_t[c] is not None:
            gw = word_t[c].cpu().numpy().view(np.uint64)
            assert np.array_equal(gw, want_w[c]), c
            assert n_out % 64 == 0 or int(gw[-1]) >> (n_out % 64) == 0  # the padding
    assert [int(dst[c].null_count) for c in range(5)] == want_nulls and int(opts.n_no_row) == want_no


def test_out_of_range_entries_are_an_argument_error(H, ex):
    """A map entry >= n_src that is not NO_ROW: HMJ_E_ARG with the count in the error text.  The kernel compares before it
    loads -- 2^63 times any width is far outside every allocation --, so nothing faults and the same ctx takes correctly
    right after."""
    rng = np.random.default_rng(23)
    n_src, n_out = 500, 700
    cols, masks, row_map = draw_case(rng, ALL_WIDTHS, n_src, n_out)
    for bad, count in (([n_src], 1), ([2 ** 63], 1), ([n_src, 2 ** 63, 2 ** 64 - 2], 3)):
        m = row_map.copy()
        m[rng.choice(n_out, size=len(bad), replace=False)] = np.array(bad, np.uint64)
        with pytest.raises(H.HmjError) as e:
            run_take(H, ex, cols, masks, m, offs=7)
        assert e.value.code == HMJ_E_ARG and ("%d row_map entries" % count) in str(e.value), str(e.value)
        check_take(H, ex, cols, masks, row_map, offs=7, tag=("after", bad))
    # 17 columns: every launch chunk guards the entry, the count is taken once
    cols, masks, row_map = draw_case(rng, [8] * 17, n_src, n_out)
    m = row_map.copy()
    m[5], m[699] = n_src, 2 ** 63
    with pytest.raises(H.HmjError) as e:
        run_take(H, ex, cols, masks, m)
    assert "2 row_map entries" in str(e.value)
    check_take(H, ex, cols, masks, row_map, tag=("after 17",))


def test_argument_errors(H, ex):
    """Each HMJ_E_ARG of the header once; all of them are found on the host before anything is launched."""
    import torch

    n_src, n_out = 100, 64
    a = torch.arange(n_src, dtype=torch.int64, device="cuda")
    b = torch.arange(2 * n_src, dtype=torch.int16, device="cuda")
    bits = torch.full((64,), 255, dtype=torch.uint8, device="cuda")
    mp = dev_map(np.arange(n_out) % n_src)
    o8 = torch.zeros(n_out + 2, dtype=torch.int64, device="cuda")
    o2 = torch.zeros(n_out + 2, dtype=torch.int16, device="cuda")
    w = torch.zeros(4, dtype=torch.int64, device="cuda")

    def err(what, rc_dst_opts):
        rc = rc_dst_opts if isinstance(rc_dst_opts, int) else rc_dst_opts[0]
        assert rc == HMJ_E_ARG, (what, rc)
        assert ex.L.hmj_last_error(ex.h), what

    def take(src_t=(a,), widths=(8,), valid=None, map_t=mp, ns=n_src, no=n_out, out_t=(o8,), word_t=(w,), **kw):
        return raw_take(H, ex, list(src_t), list(widths), valid, map_t, ns, no, list(out_t), list(word_t), **kw)

    assert take()[0] == 0  # the control
    L, h = ex.L, ex.h
    src1, dst1, op = (H.TakeSrc * 1)(), (H.TakeDst * 1)(), H.TakeOpts()
    op.struct_size = C.sizeof(H.TakeOpts)
    err("NULL src", L.hmj_take_cols_device(h, None, 1, 0, None, 0, dst1, C.byref(op)))
    err("NULL dst", L.hmj_take_cols_device(h, src1, 1, 0, None, 0, None, C.byref(op)))
    err("NULL opts", L.hmj_take_cols_device(h, src1, 1, 0, None, 0, dst1, None))
    assert L.hmj_take_cols_device(None, src1, 1, 0, None, 0, dst1, C.byref(op)) == HMJ_E_ARG
    err("NULL map", take(map_t=None))
    err("struct_size", take(struct_size=4))
    err("n_cols 0", take(src_t=(), widths=(), out_t=(), word_t=()))
    err("n_cols 65", take(src_t=(a,) * 65, widths=(8,) * 65, out_t=(o8,) * 65, word_t=(None,) * 65))
    for width in (0, 3, 32):
        err("width", take(widths=(width,)))
    err("NULL source", take(src_t=(None,)))
    err("misaligned source", take(src_t=(b.data_ptr() + 1,), widths=(2,), out_t=(o2,)))
    err("misaligned 16-byte source", take(src_t=(a.data_ptr() + 8,), widths=(16,), ns=10, no=8))
    err("NULL destination", take(out_t=(None,)))
    err("misaligned destination", take(src_t=(b,), widths=(2,), out_t=(o2.data_ptr() + 1,)))
    err("misaligned bitmap words", take(word_t=(w.data_ptr() + 4,)))
    err("reserved (column)", take(reserved=1))
    err("reserved (opts)", take(opts_reserved=1))
    err("bit_offset overflow", take(valid=[(bits, 2 ** 64 - n_src + 1)]))
    err("n_out", take(no=2 ** 32))
    err("n_src", take(ns=2 ** 32))
    # overlaps: a destination that is the map, a source column or a source bitmap; a bitmap on top of a source
    err("data over the map", take(out_t=(mp,)))
    err("in place", take(out_t=(a,)))
    err("data over a later source", take(src_t=(b, a), widths=(2, 8), out_t=(a, o8), word_t=(None, None), no=8))
    err("data over a source bitmap", take(valid=[(bits, 3)], out_t=(bits.data_ptr() + 8,), no=2))
    err("bitmap over a source", take(word_t=(a.data_ptr() + 8 * 50,)))
    err("bitmap over the map", take(word_t=(mp,)))
    # neighbours do not overlap: the output right behind the map's last entry, the bitmap right behind the source
    both = torch.zeros(n_out + n_out, dtype=torch.int64, device="cuda")
    both[:n_out] = mp
    assert take(map_t=both, out_t=(both.data_ptr() + 8 * n_out,))[0] == 0
    assert both[n_out:].cpu().tolist() == [i % n_src for i in range(n_out)]
    # n_out == 0 writes nothing and needs no map or destination; the ctx still takes
    o8.fill_(-7)
    rc, dst, opts = take(map_t=None, no=0, out_t=(None,), word_t=(None,))
    assert rc == 0 and int(dst[0].null_count) == 0 and int(opts.n_no_row) == 0 and (o8 == -7).all()
    rc, dst, opts = take()
    assert rc == 0 and o8[:n_out].cpu().tolist() == [i % n_src for i in range(n_out)] and w.cpu().tolist()[0] == -1
    # a caller whose hmj_take_opts ends behind `reserved` gets the columns and the null counts, and nothing written behind it
    rc, dst, opts = take(struct_size=8)
    assert rc == 0 and int(opts.n_no_row) == 0 and opts.struct_size == 8


# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("widths", [[4, 4], [8, 4, 2]])
def test_full_outer_join_to_columns(H, ex, widths):
    """A FULL_OUTER multi-column join with NULL keys (packed [4,4], hashed [8,4,2]), then its columns: the build key columns
    and a 16-byte non-key column through r_row, the probe key columns through s_row, straight from the result's device
    pointers.  The join's five columns are the same before and after the takes."""
    import torch

    rng = random.Random(31 + len(widths))
    nrng = np.random.default_rng(31 + len(widths))
    nb, np_ = 1000, 1100
    bt, pt = drawn(rng, widths, nb, np_)
    bcols, pcols = columns(bt, widths), columns(pt, widths)
    mb, mp = draw_masks(nrng, nb, len(widths), "all", 0.2), draw_masks(nrng, np_, len(widths), "one", 0.2)
    bnull, pnull = null_rows(mb, nb), null_rows(mp, np_)
    extra = draw_col(nrng, 16, nb)  # a non-key column of the build side, no bitmap
    B, P = dev_rel(bcols, None), dev_rel(pcols, None)
    VB, VP = dev_valid(H, mb, 3), dev_valid(H, mp, 11)
    res, info = ex.join_kind_cols_device(B[0], None, P[0], None, BUILD, FULL_OUTER, H.HMJ_ORDERED, build_valid=VB, probe_valid=VP)
    n = int(res.n_matches)
    before = ex.cols_kind_rows_to_numpy(res)
    plan, timing = ex.last_plan(), ex.last_timing()
    r_row, s_row = before[:, 1], before[:, 2]
    assert n > nb and (r_row == NO_ROW).sum() > 50 and (s_row == NO_ROW).sum() > 50 and info["n_build_null"] == bnull.sum() > 50

    b_out, b_words, b_info = ex.take_cols_device(B[0] + [torch.from_numpy(extra).cuda()], (res.r_row, n), valid=list(VB) + [None])
    p_out, p_words, p_info = ex.take_cols_device(P[0], (res.s_row, n), valid=VP)
    after = ex.cols_kind_rows_to_numpy(res)
    assert np.array_equal(before, after)  # the takes did not disturb the result
    assert ex.last_plan() == plan and ex.last_timing() == timing

    # byte for byte what the maps say
    want = expected_take(bcols + [extra], list(mb) + [None], r_row)
    for c in range(len(widths) + 1):
        assert np.array_equal(as_bytes(b_out[c].cpu().numpy()), as_bytes(want[0][c])), c
        assert np.array_equal(b_words[c].cpu().numpy().view(np.uint64), want[1][c]), c
    assert b_info["null_count"] == want[2] and b_info["n_no_row"] == want[3] == int((r_row == NO_ROW).sum())
    want_p = expected_take(pcols, mp, s_row)
    for c in range(len(widths)):
        assert np.array_equal(as_bytes(p_out[c].cpu().numpy()), as_bytes(want_p[0][c])), c
        assert np.array_equal(p_words[c].cpu().numpy().view(np.uint64), want_p[1][c]), c
    assert p_info["null_count"] == want_p[2] and p_info["n_no_row"] == want_p[3] == int((s_row == NO_ROW).sum())

    # and what that means for the rows of the join
    bval = [H.unpack_validity(w, n) for w in b_words]
    pval = [H.unpack_validity(w, n) for w in p_words]
    pair = (r_row != NO_ROW) & (s_row != NO_ROW)
    assert pair.sum() > 100
    for c in range(len(widths)):
        bc, pc = b_out[c].cpu().numpy(), p_out[c].cpu().numpy()
        assert bval[c][pair].all() and pval[c][pair].all() and np.array_equal(bc[pair], pc[pair])  # matched: equal keys, no NULL
        assert not bval[c][r_row == NO_ROW].any() and not pval[c][s_row == NO_ROW].any()           # no partner: NULL
        assert not bc[~bval[c]].any() and not pc[~pval[c]].any()
    assert not bval[-1][r_row == NO_ROW].any() and bval[-1][r_row != NO_ROW].all()
    # a NULL-key row is emitted unmatched, and is NULL in exactly the columns its bitmaps say
    there = np.flatnonzero(r_row != NO_ROW)
    rows_b = r_row[there].astype(np.int64)
    assert (s_row[there][bnull[rows_b]] == NO_ROW).all()
    for c in range(len(widths)):
        assert np.array_equal(bval[c][there], mb[c][rows_b])
    there = np.flatnonzero(s_row != NO_ROW)
    rows_p = s_row[there].astype(np.int64)
    assert (r_row[there][pnull[rows_p]] == NO_ROW).all()
    for c in range(len(widths)):
        assert np.array_equal(pval[c][there], np.ones(len(there), bool) if mp[c] is None else mp[c][rows_p])


def test_string_kind_join_to_a_payload_column(H, ex):
    """The maps of a string kind join qualify too: a 4-byte column of the build side through a FULL_OUTER string join's
    r_row; the result stays as it was."""
    import torch

    rng = np.random.default_rng(41)
    nb, np_ = 600, 800
    bkeys = [b"k%d" % int(x) for x in rng.integers(0, 400, size=nb)]
    pkeys = [b"k%d" % int(x) for x in rng.integers(200, 700, size=np_)]

    def rel(keys):
        chars, offsets = H.pack_strings(keys, "cuda")
        return chars, offsets, torch.arange(len(keys), dtype=torch.int64, device="cuda")

    mask = rng.random(nb) >= 0.3
    col = draw_col(rng, 4, nb, mask)
    res, _ = ex.join_kind_str_device(rel(bkeys), rel(pkeys), BUILD, FULL_OUTER, H.HMJ_MATERIALIZE)
    n = int(res.n_matches)
    before = ex.str_kind_rows_to_numpy(res)
    r_row = before[:, 1]
    assert 50 < (r_row == H.HMJ_STR_NO_ROW).sum() < n
    outs, words, info = ex.take_cols_device([torch.from_numpy(col).cuda()], (res.r_row, n), valid=[(H.pack_validity(mask, 7, "cuda"), 7)])
    assert np.array_equal(before, ex.str_kind_rows_to_numpy(res))
    want = expected_take([col], [mask], r_row)
    assert np.array_equal(as_bytes(outs[0].cpu().numpy()), as_bytes(want[0][0]))
    assert np.array_equal(words[0].cpu().numpy().view(np.uint64), want[1][0])
    assert info["null_count"] == want[2] and info["n_no_row"] == want[3] == int((r_row == H.HMJ_STR_NO_ROW).sum())
    # rval of a matched row is its build row's payload, here the row index: the taken column lines up with it
    there = r_row != H.HMJ_STR_NO_ROW
    assert np.array_equal(before[there, 3], r_row[there])


def test_a_take_keeps_a_prepared_build_side(H):
    """Between hmj_prepare_build_u64_device and the join: the join still runs on HMJ_PATH_PREPARED."""
    import torch

    e = H.Executor(0)
    try:
        nb, npb = 300000, 200000
        B, P = e.gen_build(nb), e.gen_probe(npb, nb, miss_mod=4)
        rng = np.random.default_rng(7)
        cols, masks, row_map = draw_case(rng, [8, 4], 3000, 5000)
        e.set_profiling(True)
        e.prepare_build(B, npb)
        r = e.join_device(B, P, 0)
        want = int(r.n_matches)
        assert e.last_timing()["path"] & H.HMJ_PATH_PREPARED  # (the control: this shape does reuse a prepared build side)
        e.prepare_build(B, npb)
        info = check_take(H, e, cols, masks, row_map, offs=13, tag=("prepared",))
        assert info["ms_take"] > 0.0  # (profiling is on)
        r = e.join_device(B, P, 0)
        assert int(r.n_matches) == want and e.last_timing()["path"] & H.HMJ_PATH_PREPARED
    finally:
        e.close()
