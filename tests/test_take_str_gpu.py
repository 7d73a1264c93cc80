"""GPU checks of hmj_take_str_device (one Arrow large_string column taken through a row map) against `expected_take_str`
of test_take_str_cpu.py, byte for byte: chars, offsets, bitmap words including the padding, null_count, n_no_row and
total_bytes.  Sizes around the wave and workgroup edges crossed with source bit offsets, the length shapes that can break the
bytes kernel (its tile of 4096 bytes, its 16-byte pieces, the 1024 rows it stages in LDS), byte values and source placements,
pre-filled outputs, the two-call protocol, bad map entries and bad source offsets, every argument error, and the takes behind a
FULL_OUTER string kind join, an ordered inner string join and a prepared build side.
No kernel of the entry caps its grid (one workgroup per 256 rows, per 4096 output bytes), so there is no grid-stride case."""
import ctypes as C

import numpy as np
import pytest

from test_take_str_cpu import NO_ROW, expected_take_str

pytestmark = pytest.mark.gpu
HMJ_E_ARG = -1
SIZES = [0, 1, 63, 64, 65, 255, 256, 257, 1000]
OFFSETS = [0, 1, 7, 13, 63]
TILE = 4096         # kTileBytes of takestr.hip: the output bytes one workgroup of the bytes phase owns
STAGE_ROWS = 1024   # kStageRows of takestr.hip: the rows of a tile whose starts are staged in LDS
PATTERN = 0xA5      # the bytes under the NULL slots of a source column
BUILD, FULL_OUTER = 1, 4  # HMJ_KIND_BUILD_SIDE, HMJ_FULL_OUTER


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


def draw_source(rng, lens, mask=None, off0=0, lo=1, hi=256):
    """A source column of len(lens) rows: (chars uint8 [off0 + sum(lens)], offsets int64 [n + 1]).  The bytes are drawn from
    lo..hi-1 (never PATTERN); those in front of offsets[0] and under the NULL slots of `mask` spell PATTERN."""
    lens = np.asarray(lens, np.int64)
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64) + off0
    chars = rng.integers(lo, hi, size=int(offsets[-1]), dtype=np.uint8)
    chars[chars == PATTERN] = lo
    chars[:off0] = PATTERN
    if mask is not None:
        for r in np.flatnonzero(~np.asarray(mask, bool)):
            chars[offsets[r]:offsets[r + 1]] = PATTERN
    return chars, offsets


def draw_map(rng, n_src, n_out, frac_no_row=0.3):
    row_map = rng.integers(0, max(n_src, 1), size=n_out).astype(np.uint64)
    row_map[rng.random(n_out) < (1.0 if n_src == 0 else frac_no_row)] = NO_ROW
    return row_map


def dev_map(row_map):
    import torch

    return torch.from_numpy(np.asarray(row_map, np.uint64).view(np.int64).copy()).cuda()


def dev_chars(chars, shift=0):
    """The chars on the device, starting `shift` bytes behind an aligned base and ending with the allocation's last byte."""
    import torch

    base = torch.empty(shift + len(chars), dtype=torch.uint8, device="cuda")
    assert base.data_ptr() % 256 == 0
    base[:shift] = PATTERN
    view = base[shift:]
    view.copy_(torch.from_numpy(np.ascontiguousarray(chars)))
    return view


def compare(H, want, got, tag=()):
    """(chars, offsets, words, info) of Executor.take_str_device against the tuple expected_take_str returns."""
    w_chars, w_off, w_words, w_nulls, w_no, w_total = want
    chars, offsets, words, info = got
    assert (info["null_count"], info["n_no_row"], info["total_bytes"]) == (w_nulls, w_no, w_total), (tag, info)
    g_off = offsets.cpu().numpy().view(np.uint64)
    assert np.array_equal(g_off, w_off), (tag, np.flatnonzero(g_off != w_off)[:5])
    if words is not None:
        g_words = words.cpu().numpy().view(np.uint64)
        assert np.array_equal(g_words, w_words), (tag, np.flatnonzero(g_words != w_words)[:5])
    g_chars = chars.cpu().numpy()
    assert g_chars.shape == w_chars.shape, tag
    bad = np.flatnonzero(g_chars != w_chars)
    assert not len(bad), (tag, bad[:5], len(bad))


def check_take(H, ex, chars, offsets, mask, row_map, bit_off=0, shift=0, tag=(), **kw):
    """One take through the Executor against expected_take_str; returns the info dict."""
    import torch

    want = expected_take_str(chars, offsets, mask, row_map)
    valid = None if mask is None else (H.pack_validity(mask, bit_off, "cuda"), bit_off)
    got = ex.take_str_device(dev_chars(chars, shift), torch.from_numpy(np.asarray(offsets, np.int64)).cuda(), dev_map(row_map),
                             valid=valid, **kw)
    compare(H, want, got, tag)
    return got[3]


# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_out", SIZES)
def test_sizes_and_offsets(H, ex, n_out):
    """Every output size (none, a single row, one short of / exactly / one past a wave and a workgroup, several workgroups)
    crossed with source bit offsets inside a byte, across a byte and one short of a 64-bit word; about 30 % NO_ROW, 30 % NULL
    source slots, lengths 0..40."""
    rng = np.random.default_rng(n_out)
    n_src = n_out + 37
    mask = rng.random(n_src) >= 0.3
    chars, offsets = draw_source(rng, rng.integers(0, 41, size=n_src), mask, off0=3)
    row_map = draw_map(rng, n_src, n_out)
    for off in OFFSETS:
        info = check_take(H, ex, chars, offsets, mask, row_map, bit_off=off, shift=off % 16, tag=(n_out, off))
    if n_out == 1000:
        assert info["n_no_row"] > 200 and info["null_count"] > info["n_no_row"] + 100 and info["total_bytes"] > 5000
    check_take(H, ex, chars, offsets, None, row_map, tag=(n_out, "no bitmap"), want_validity=False)


def _shape(rng, name):
    """(lens, mask or None, row_map) of one length shape."""
    if name == "all empty":
        lens = np.zeros(700, np.int64)
    elif name == "one byte":  # 4096 rows per tile: more than are staged
        lens = np.ones(9000, np.int64)
    elif name == "0..40":
        lens = rng.integers(0, 41, size=3000)
    elif name == "piece edges":
        lens = rng.choice([15, 16, 17, 31, 32, 33], size=1500)
    elif name == "a long row":  # 100 000 bytes among short ones: 25 tiles
        lens = rng.integers(0, 20, size=400)
        lens[200] = 100000
    elif name == "a tile, a tile + 1":
        lens = np.array([5, TILE, TILE + 1, 3, TILE, 0, TILE + 1, TILE - 1, 1], np.int64)
    else:
        raise AssertionError(name)
    n = len(lens)
    mask = rng.random(n) >= 0.1
    row_map = np.arange(n, dtype=np.uint64) if name in ("a long row", "a tile, a tile + 1") else draw_map(rng, n, n + 50, 0.1)
    if name == "a long row":
        mask[200] = True
        row_map = np.concatenate([row_map, rng.integers(190, 210, size=30).astype(np.uint64)])  # the long row a few times more
    if name == "a tile, a tile + 1":
        mask[:] = True
    return lens, mask, row_map


@pytest.mark.parametrize("name", ["all empty", "one byte", "0..40", "piece edges", "a long row", "a tile, a tile + 1"])
def test_length_shapes(H, ex, name):
    rng = np.random.default_rng(len(name))
    lens, mask, row_map = _shape(rng, name)
    chars, offsets = draw_source(rng, lens, mask, off0=1)
    info = check_take(H, ex, chars, offsets, mask, row_map, bit_off=5, shift=3, tag=(name,))
    if name == "all empty":
        assert info["total_bytes"] == 0 and 0 < info["null_count"] < len(row_map)
    if name == "a tile, a tile + 1":
        assert info["total_bytes"] == int(lens.sum())
        # the two rows of exactly a tile, each at the start of a tile of the output, and one byte in front of it
        tile = np.array([TILE, TILE, TILE - 1, 7], np.int64)
        c2, o2 = draw_source(rng, tile, None)
        for m in ([0, 1], [3, 0, 1], [2, 0, 2, 3, 1]):
            check_take(H, ex, c2, o2, None, np.array(m, np.uint64), shift=9, tag=(name, m))


def test_many_empty_rows_inside_one_tile(H, ex):
    """20 000 consecutive empty or NULL rows between two non-empty ones: a tile crossed by more rows than the 1024 that are
    staged in LDS, so its lanes search the offsets in global memory -- and a 16-byte piece that starts in the row in front
    of them and ends in the row behind."""
    rng = np.random.default_rng(77)
    n_mid = 20000
    assert n_mid > STAGE_ROWS
    lens = np.concatenate([[21], rng.integers(0, 2, size=n_mid) * 9, [30, 0, 0, 5]]).astype(np.int64)
    mask = np.ones(len(lens), bool)
    mask[1:1 + n_mid] = lens[1:1 + n_mid] == 0  # the rows with bytes are NULL, the empty ones valid ...
    mask[1:1 + n_mid:3] = False                 # ... or NULL too
    chars, offsets = draw_source(rng, lens, mask)
    row_map = np.arange(len(lens), dtype=np.uint64)
    row_map[5:n_mid:7] = NO_ROW
    info = check_take(H, ex, chars, offsets, mask, row_map, bit_off=63, shift=7, tag=("many empty",))
    assert info["total_bytes"] == 21 + 30 + 5 and info["null_count"] > n_mid // 3


@pytest.mark.parametrize("shift", [1, 3, 7, 15])
def test_byte_values_and_source_placement(H, ex, shift):
    """Bytes 0x00 and >= 0x80, source chars starting 1, 3, 7 and 15 bytes behind an aligned base, offsets[0] != 0,
    chars_bytes exactly the end of the last row (which is the end of the allocation), and the first and the last source
    row taken: where loads of whole aligned granules reach in front of and behind the buffer's bytes."""
    rng = np.random.default_rng(shift)
    n_src = 500
    lens = rng.integers(1, 40, size=n_src)
    chars, offsets = draw_source(rng, lens, None, off0=shift + 2, lo=0)
    chars[offsets[0]:] = rng.choice(np.array([0x00, 0x80, 0xFF, 0x7F, 0xC3], np.uint8), size=len(chars) - int(offsets[0]))
    assert int(offsets[-1]) == len(chars) and offsets[0] != 0
    row_map = draw_map(rng, n_src, 800, 0.1)
    row_map[:4] = [n_src - 1, 0, 0, n_src - 1]
    row_map[-2:] = [0, n_src - 1]
    check_take(H, ex, chars, offsets, None, row_map, shift=shift, tag=("placement", shift))
    # the last row alone, and the first alone
    for r in (n_src - 1, 0):
        check_take(H, ex, chars, offsets, None, np.array([r], np.uint64), shift=shift, tag=("single", shift, r))


def raw_take(H, ex, chars, chars_bytes, offsets, valid, map_t, n_src, n_out, out_off, out_chars, capacity, words, struct_size=None,
             reserved=0):
    """hmj_take_str_device through ctypes alone, on tensors the caller allocated (None: a NULL pointer; an int: that address).
    Returns (status, TakeStrDst, TakeStrOpts)."""
    def ptr(t):
        return t if isinstance(t, int) or t is None else t.data_ptr()

    src, dst, opts = H.TakeStrSrc(), H.TakeStrDst(), H.TakeStrOpts()
    src.chars, src.chars_bytes, src.offsets = ptr(chars), chars_bytes, ptr(offsets)
    if valid is not None:
        src.validity.bits, src.validity.bit_offset = ptr(valid[0]), valid[1]
    dst.offsets, dst.chars, dst.chars_capacity, dst.validity = ptr(out_off), ptr(out_chars), capacity, ptr(words)
    opts.struct_size = C.sizeof(H.TakeStrOpts) if struct_size is None else struct_size
    opts.reserved = reserved
    ex._sync_stream()
    rc = ex.L.hmj_take_str_device(ex.h, C.byref(src), n_src, C.c_void_p(ptr(map_t)), n_out, C.byref(dst), C.byref(opts))
    return rc, dst, opts


def _prefilled_case(n_out, seed):
    rng = np.random.default_rng(seed)
    n_src = 300
    mask = rng.random(n_src) >= 0.4
    chars, offsets = draw_source(rng, rng.integers(0, 41, size=n_src), mask, off0=2)
    return chars, offsets, mask, draw_map(rng, n_src, n_out)


@pytest.mark.parametrize("n_out", [1, 63, 65, 257, 1000])
def test_prefilled_outputs_and_the_two_call_protocol(H, ex, n_out):
    """The outputs are filled with 0xFF and the capacity is total_bytes + 64: every byte at and behind total_bytes is still
    0xFF, the padding bits of the last bitmap word are 0, and the pattern under the source's NULL slots never comes out.  The
    sizing call writes the same offsets, words and counts as the full call and no byte; a capacity one byte short is
    HMJ_E_ARG with total_bytes reported and chars untouched, and a correct take on the same ctx follows."""
    import torch

    chars, offsets, mask, row_map = _prefilled_case(n_out, 2000 + n_out)
    want = expected_take_str(chars, offsets, mask, row_map)
    w_chars, w_off, w_words, w_nulls, w_no, total = want
    assert w_nulls > w_no or n_out == 1
    n_src = len(offsets) - 1
    d_chars, d_off, d_map = dev_chars(chars, 5), torch.from_numpy(offsets).cuda(), dev_map(row_map)
    valid = (H.pack_validity(mask, 13, "cuda"), 13)

    def fresh():
        return (torch.full((n_out + 1,), -1, dtype=torch.int64, device="cuda"), torch.full((total + 64,), 0xFF, dtype=torch.uint8, device="cuda"),
                torch.full(((n_out + 63) // 64,), -1, dtype=torch.int64, device="cuda"))

    def same_meta(o, w, dst, opts):
        assert np.array_equal(o.cpu().numpy().view(np.uint64), w_off)
        gw = w.cpu().numpy().view(np.uint64)
        assert np.array_equal(gw, w_words)
        assert n_out % 64 == 0 or int(gw[-1]) >> (n_out % 64) == 0  # the padding
        assert (int(dst.null_count), int(dst.total_bytes), int(opts.n_no_row)) == (w_nulls, total, w_no)

    # the sizing call: no byte copied
    o, c, w = fresh()
    rc, dst, opts = raw_take(H, ex, d_chars, len(chars), d_off, valid, d_map, n_src, n_out, o, None, 0, w)
    assert rc == 0, ex.L.hmj_last_error(ex.h)
    same_meta(o, w, dst, opts)
    # one byte short: HMJ_E_ARG, total_bytes reported, chars untouched
    if total:
        rc, dst, opts = raw_take(H, ex, d_chars, len(chars), d_off, valid, d_map, n_src, n_out, o, c, total - 1, w)
        assert rc == HMJ_E_ARG and int(dst.total_bytes) == total and b"chars_capacity" in ex.L.hmj_last_error(ex.h)
        assert (c == 0xFF).all()
    # the full call with room to spare
    o, c, w = fresh()
    rc, dst, opts = raw_take(H, ex, d_chars, len(chars), d_off, valid, d_map, n_src, n_out, o, c, total + 64, w)
    assert rc == 0, ex.L.hmj_last_error(ex.h)
    same_meta(o, w, dst, opts)
    got = c.cpu().numpy()
    assert np.array_equal(got[:total], w_chars)
    assert (got[total:] == 0xFF).all()      # nothing at or behind total_bytes
    assert not (got[:total] == PATTERN).any()  # nothing from under a NULL slot
    # exactly total_bytes of capacity, through the Executor's one-call form
    compare(H, want, ex.take_str_device(d_chars, d_off, d_map, valid=valid, capacity=total), ("capacity", n_out))
    if total:
        with pytest.raises(H.HmjError) as e:
            ex.take_str_device(d_chars, d_off, d_map, valid=valid, capacity=total - 1)
        assert e.value.code == HMJ_E_ARG


def test_bad_map_entries_and_bad_offsets_are_argument_errors(H, ex):
    """A map entry >= n_src that is not NO_ROW, a taken valid row whose offsets decrease, and one that ends at chars_bytes
    + 1: HMJ_E_ARG with the count in the error text.  All are compared before an address is formed from them -- 2^63 as a
    row or as an offset is far outside every allocation --, so nothing faults and the same ctx takes correctly right after.
    The same bad offsets at a row that is NULL or never taken are fine."""
    import torch

    rng = np.random.default_rng(23)
    n_src, n_out = 500, 700
    mask = rng.random(n_src) >= 0.3
    mask[[10, 11, 12, 499]] = True
    chars, offsets = draw_source(rng, rng.integers(1, 30, size=n_src), mask, off0=4)
    row_map = draw_map(rng, n_src, n_out)
    row_map[:4] = [10, 11, 12, 499]
    d_chars, d_valid = dev_chars(chars, 1), (H.pack_validity(mask, 7, "cuda"), 7)

    def take(offs, m, valid=d_valid):
        return ex.take_str_device(d_chars, torch.from_numpy(np.asarray(offs, np.int64)).cuda(), dev_map(m), valid=valid)

    def good():
        compare(H, expected_take_str(chars, offsets, mask, row_map), take(offsets, row_map), ("after",))

    for bad, count in (([n_src], 1), ([2 ** 63], 1), ([n_src, 2 ** 63, 2 ** 64 - 2], 3)):
        m = row_map.copy()
        m[rng.choice(np.arange(4, n_out), size=len(bad), replace=False)] = np.array(bad, np.uint64)
        with pytest.raises(H.HmjError) as e:
            take(offsets, m)
        assert e.value.code == HMJ_E_ARG and ("%d row_map entries" % count) in str(e.value), str(e.value)
        good()
    # decreasing offsets at the taken valid rows 10 and 11 (offsets[11] far beyond everything: row 10 ends there, row 11 starts there)
    o = offsets.copy().view(np.uint64)
    o[11] = 2 ** 63
    with pytest.raises(H.HmjError) as e:
        take(o.view(np.int64), row_map[:4])  # rows 10, 11, 12, 499 once each
    assert e.value.code == HMJ_E_ARG, str(e.value)
    assert "2 taken rows have bad source offsets (1 with offsets[r + 1] < offsets[r], 1 that end" in str(e.value), str(e.value)
    good()
    o = offsets.copy()
    o[12] = o[11] - 1  # row 11 = [o11, o11 - 1): decreasing; row 12 one byte longer, fine
    with pytest.raises(H.HmjError) as e:
        take(o, row_map[:4])
    assert "1 taken rows have bad source offsets (1 with offsets[r + 1] < offsets[r], 0 that end" in str(e.value), str(e.value)
    good()
    # the last row ends at chars_bytes + 1; it is taken once in the first four entries and maybe more often behind them
    o = offsets.copy()
    o[n_src] += 1
    times = int((row_map == 499).sum())
    with pytest.raises(H.HmjError) as e:
        take(o, row_map)
    assert e.value.code == HMJ_E_ARG and ("%d taken rows have bad source offsets (0 with offsets[r + 1] < offsets[r], %d that end" % (times, times)) in str(e.value)
    good()
    # the same bad offsets at rows that are NULL (13, 14) or never taken (20): fine, and the output is what it was
    quiet = mask.copy()
    quiet[[13, 14]] = False
    m = row_map.copy()
    m[m == 20] = 21
    m[4:6] = [13, 14]
    o = offsets.copy().view(np.uint64)
    o[14] = 2 ** 63          # rows 13 and 14: NULL
    want = expected_take_str(chars, offsets, quiet, m)
    compare(H, want, take(o.view(np.int64), m, (H.pack_validity(quiet, 7, "cuda"), 7)), ("bad offsets under NULL",))
    o = offsets.copy()
    o[21] = o[20] - 3        # row 20 = [o20, o20 - 3): never taken; row 21 is longer by 3 bytes of row 20
    keep = m != 21
    compare(H, expected_take_str(chars, offsets, quiet, m[keep]), take(o, m[keep], (H.pack_validity(quiet, 7, "cuda"), 7)), ("never taken",))


def test_argument_errors(H, ex):
    """Each HMJ_E_ARG of the header once; all of them are found on the host before anything is launched."""
    import torch

    n_src, n_out = 100, 64
    chars = torch.arange(n_src, dtype=torch.int64, device="cuda").view(torch.uint8)  # row r: the 8 bytes of r
    nbytes = 8 * n_src
    offs = torch.arange(n_src + 1, dtype=torch.int64, device="cuda") * 8
    bits = torch.full((64,), 255, dtype=torch.uint8, device="cuda")
    mp = dev_map(np.arange(n_out) % n_src)
    oo = torch.zeros(n_out + 3, dtype=torch.int64, device="cuda")
    oc = torch.zeros(8 * n_out + 64, dtype=torch.uint8, device="cuda")
    w = torch.zeros(4, dtype=torch.int64, device="cuda")
    L, h = ex.L, ex.h

    def err(what, rc_dst_opts):
        rc = rc_dst_opts if isinstance(rc_dst_opts, int) else rc_dst_opts[0]
        assert rc == HMJ_E_ARG, (what, rc)
        assert L.hmj_last_error(h), what

    def take(chars=chars, chars_bytes=nbytes, offsets=offs, valid=None, map_t=mp, ns=n_src, no=n_out, out_off=oo, out_chars=oc,
             capacity=8 * n_out, words=w, **kw):
        return raw_take(H, ex, chars, chars_bytes, offsets, valid, map_t, ns, no, out_off, out_chars, capacity, words, **kw)

    def control():
        rc, dst, opts = take()
        assert rc == 0 and int(dst.total_bytes) == 8 * n_out and int(dst.null_count) == 0
        assert oc[:8 * n_out].view(torch.int64).cpu().tolist() == [i % n_src for i in range(n_out)] and w.cpu().tolist()[0] == -1

    control()
    src1, dst1, op = H.TakeStrSrc(), H.TakeStrDst(), H.TakeStrOpts()
    op.struct_size = C.sizeof(H.TakeStrOpts)
    err("NULL src", L.hmj_take_str_device(h, None, 0, None, 0, C.byref(dst1), C.byref(op)))
    err("NULL dst", L.hmj_take_str_device(h, C.byref(src1), 0, None, 0, None, C.byref(op)))
    err("NULL opts", L.hmj_take_str_device(h, C.byref(src1), 0, None, 0, C.byref(dst1), None))
    assert L.hmj_take_str_device(None, C.byref(src1), 0, None, 0, C.byref(dst1), C.byref(op)) == HMJ_E_ARG
    err("struct_size", take(struct_size=4))
    err("reserved", take(reserved=1))
    err("NULL map", take(map_t=None))
    err("NULL destination offsets", take(out_off=None))
    err("NULL source offsets", take(offsets=None))
    err("NULL source chars", take(chars=None))
    err("misaligned map", take(map_t=mp.data_ptr() + 4))
    err("misaligned source offsets", take(offsets=offs.data_ptr() + 4))
    err("misaligned destination offsets", take(out_off=oo.data_ptr() + 4))
    err("misaligned bitmap words", take(words=w.data_ptr() + 4))
    err("misaligned destination chars", take(out_chars=oc.data_ptr() + 8))
    err("n_out", take(no=2 ** 32))
    err("n_src", take(ns=2 ** 32))
    err("bit_offset overflow", take(valid=(bits, 2 ** 64 - n_src + 1)))
    # overlaps: every destination range over something the call reads, and over another destination
    err("offsets over the map", take(out_off=mp, no=8))
    err("offsets over the source offsets", take(out_off=offs))
    err("offsets over the source chars", take(out_off=chars.data_ptr() + 64))
    err("offsets over the source bitmap", take(valid=(bits, 3), out_off=bits.data_ptr() + 8, no=2))
    err("chars over the map", take(out_chars=mp))
    err("chars over the source offsets", take(out_chars=offs.data_ptr() + 16))
    err("chars in place", take(out_chars=chars))
    err("chars over the source bitmap", take(valid=(bits, 3), out_chars=bits, capacity=16))
    err("words over the map", take(words=mp))
    err("words over the source offsets", take(words=offs))
    err("words over the source chars", take(words=chars.data_ptr() + 8 * 50))
    err("words over the source bitmap", take(valid=(bits, 0), words=bits.data_ptr() + 8))
    err("words over the destination offsets", take(words=oo.data_ptr() + 8 * n_out))
    err("chars over the destination offsets", take(out_chars=oo, capacity=16))
    err("chars over the words", take(out_chars=w, capacity=16))
    control()
    # neighbours do not overlap: the offsets right behind the map's last entry, the words right behind the offsets' last entry, and
    # chars whose capacity ends where the source chars begin
    both = torch.zeros(n_out + n_out + 1 + 1, dtype=torch.int64, device="cuda")
    both[:n_out] = mp
    rc, dst, _ = take(map_t=both, out_off=both.data_ptr() + 8 * n_out, words=both.data_ptr() + 8 * (2 * n_out + 1))
    assert rc == 0 and both[n_out:2 * n_out + 1].cpu().tolist() == [8 * i for i in range(n_out + 1)] and int(both[-1]) == -1
    joined = torch.zeros(8 * n_out + nbytes, dtype=torch.uint8, device="cuda")
    joined[8 * n_out:] = chars
    err("the capacity reaches one byte into the source", take(chars=joined.data_ptr() + 8 * n_out, out_chars=joined, capacity=8 * n_out + 1))
    rc, dst, _ = take(chars=joined.data_ptr() + 8 * n_out, out_chars=joined, capacity=8 * n_out)
    assert rc == 0 and joined[:8 * n_out].view(torch.int64).cpu().tolist() == [i % n_src for i in range(n_out)]
    # n_out == 0 writes nothing and needs no map or destination; the ctx still takes
    oo.fill_(-7)
    oc.fill_(0xEE)
    rc, dst, opts = take(map_t=None, no=0, out_off=None, words=None)
    assert rc == 0 and (int(dst.null_count), int(dst.total_bytes), int(opts.n_no_row)) == (0, 0, 0)
    rc, dst, opts = take(no=0)
    assert rc == 0 and int(dst.total_bytes) == 0 and (oo == -7).all() and (oc == 0xEE).all()
    control()
    # n_src == 0 under a map of NO_ROW alone: NULL source pointers
    none = dev_map(np.full(n_out, NO_ROW, np.uint64))
    rc, dst, opts = take(chars=None, chars_bytes=0, offsets=None, map_t=none, ns=0)
    assert rc == 0 and (int(dst.null_count), int(dst.total_bytes), int(opts.n_no_row)) == (n_out, 0, n_out)
    assert oo[:n_out + 1].cpu().tolist() == [0] * (n_out + 1) and w.cpu().tolist()[0] == 0
    # a caller whose hmj_take_str_opts ends behind `reserved` gets the column and the counts of dst, and nothing written behind it
    rc, dst, opts = take(struct_size=8)
    assert rc == 0 and int(opts.n_no_row) == 0 and opts.struct_size == 8 and int(dst.total_bytes) == 8 * n_out


# ---------------------------------------------------------------------------------------------
def str_rel(H, keys):
    import torch

    chars, offsets = H.pack_strings(keys, "cuda")
    return chars, offsets, torch.arange(len(keys), dtype=torch.int64, device="cuda")


def test_full_outer_string_join_to_key_columns(H, ex):
    """A FULL_OUTER string kind join with NULL keys on both sides and duplicates, then its key columns: the build keys
    through r_row, the probe keys through s_row, straight from the result's device pointers.  The join's result columns,
    last_plan and last_timing are the same before and after the takes."""
    rng = np.random.default_rng(41)
    nb, np_ = 600, 800
    bkeys = [b"key-%d" % int(x) if x % 7 else b"" for x in rng.integers(0, 400, size=nb)]
    pkeys = [b"key-%d" % int(x) if x % 7 else b"" for x in rng.integers(200, 700, size=np_)]
    mb, mp = rng.random(nb) >= 0.2, rng.random(np_) >= 0.2
    B, P = str_rel(H, bkeys), str_rel(H, pkeys)
    VB, VP = (H.pack_validity(mb, 3, "cuda"), 3), (H.pack_validity(mp, 11, "cuda"), 11)
    res, info = ex.join_kind_str_device(B, P, BUILD, FULL_OUTER, H.HMJ_ORDERED, build_valid=VB, probe_valid=VP)
    n = int(res.n_matches)
    before = ex.str_kind_rows_to_numpy(res)
    plan, timing = ex.last_plan(), ex.last_timing()
    r_row, s_row = before[:, 1], before[:, 2]
    assert n > nb and (r_row == NO_ROW).sum() > 50 and (s_row == NO_ROW).sum() > 50
    assert info["n_build_null"] == (~mb).sum() > 50 and info["n_probe_null"] == (~mp).sum() > 50

    b_got = ex.take_str_device(B[0], B[1], (res.r_row, n), valid=VB)
    p_got = ex.take_str_device(P[0], P[1], (res.s_row, n), valid=VP)
    assert np.array_equal(before, ex.str_kind_rows_to_numpy(res))  # the takes did not disturb the result
    assert ex.last_plan() == plan and ex.last_timing() == timing

    # byte for byte what the maps say
    compare(H, expected_take_str(B[0].cpu().numpy(), B[1].cpu().numpy(), mb, r_row), b_got, ("build",))
    compare(H, expected_take_str(P[0].cpu().numpy(), P[1].cpu().numpy(), mp, s_row), p_got, ("probe",))
    assert b_got[3]["n_no_row"] == int((r_row == NO_ROW).sum()) and p_got[3]["n_no_row"] == int((s_row == NO_ROW).sum())

    # and what that means for the rows of the join
    bval, pval = H.unpack_validity(b_got[2], n), H.unpack_validity(p_got[2], n)
    bstr, pstr = H.unpack_strings(b_got[0], b_got[1], bval), H.unpack_strings(p_got[0], p_got[1], pval)
    pair = (r_row != NO_ROW) & (s_row != NO_ROW)
    assert pair.sum() > 100
    for i in range(n):
        if pair[i]:  # matched: equal keys, valid on both sides
            assert bstr[i] is not None and bstr[i] == pstr[i] == bkeys[int(r_row[i])], i
        if r_row[i] == NO_ROW:
            assert bstr[i] is None, i
        elif not mb[int(r_row[i])]:  # a NULL-key row comes out NULL, and unmatched
            assert bstr[i] is None and s_row[i] == NO_ROW, i
        if s_row[i] == NO_ROW:
            assert pstr[i] is None, i
        elif not mp[int(s_row[i])]:
            assert pstr[i] is None and r_row[i] == NO_ROW, i
    assert any(s == b"" for s in bstr) and any(s == b"" for s in pstr)  # the valid empty key is a key like any other


def test_ordered_inner_string_join_lists_its_keys_in_order(H, ex):
    """HMJ_ORDERED on a few thousand distinct words: the key column taken through r_row lists the keys in the documented
    (hash, key bytes) order -- a host sort on hash_str_device's hashes --, and so does the one taken through s_row."""
    rng = np.random.default_rng(43)
    words = [b"word-%d-%s" % (i, b"x" * (i % 23)) for i in range(3000)]
    bkeys = [words[i] for i in rng.permutation(len(words))]
    pkeys = [words[i] for i in rng.permutation(len(words))]
    B, P = str_rel(H, bkeys), str_rel(H, pkeys)
    res, _ = ex.join_str_device(B, P, H.HMJ_ORDERED)
    n = int(res.n_matches)
    assert n == len(words)
    hashes = ex.hash_str_device(B[0], B[1]).cpu().numpy().view(np.uint64)
    want = [k for _, k in sorted(zip((int(x) for x in hashes), bkeys))]
    for rel, row_ptr in ((B, res.r_row), (P, res.s_row)):
        chars, offsets, words_out, info = ex.take_str_device(rel[0], rel[1], (row_ptr, n))
        assert info["null_count"] == 0 and info["n_no_row"] == 0 and info["total_bytes"] == sum(len(k) for k in words)
        assert H.unpack_strings(chars, offsets, H.unpack_validity(words_out, n)) == want


def test_a_take_keeps_a_prepared_build_side(H):
    """Between hmj_prepare_build_u64_device and the join: the join still runs on HMJ_PATH_PREPARED."""
    e = H.Executor(0)
    try:
        nb, npb = 300000, 200000
        B, P = e.gen_build(nb), e.gen_probe(npb, nb, miss_mod=4)
        rng = np.random.default_rng(7)
        mask = rng.random(3000) >= 0.3
        chars, offsets = draw_source(rng, rng.integers(0, 41, size=3000), mask)
        row_map = draw_map(rng, 3000, 5000)
        e.set_profiling(True)
        e.prepare_build(B, npb)
        r = e.join_device(B, P, 0)
        want = int(r.n_matches)
        assert e.last_timing()["path"] & H.HMJ_PATH_PREPARED  # (the control: this shape does reuse a prepared build side)
        e.prepare_build(B, npb)
        info = check_take(H, e, chars, offsets, mask, row_map, bit_off=13, tag=("prepared",))
        assert info["ms_offsets"] > 0.0 and info["ms_chars"] > 0.0  # (profiling is on)
        r = e.join_device(B, P, 0)
        assert int(r.n_matches) == want and e.last_timing()["path"] & H.HMJ_PATH_PREPARED
    finally:
        e.close()
