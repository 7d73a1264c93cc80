"""CPU-only checks of hmj_take_str_device (include/hmj.h, "taking an Arrow string column through a row map"): the library
exports the entry while HMJ_ABI_VERSION stays 5 and refuses a NULL ctx without a GPU, the ctypes mirrors of
hmj_take_str_src / hmj_take_str_dst / hmj_take_str_opts have the header's layout (g++ prints sizeof / offsetof),
`unpack_strings` inverts `pack_strings`, and `expected_take_str` -- the plain numpy / Python expectation
test_take_str_gpu.py imports -- is pinned on a case written out by hand."""
import ctypes as C

import numpy as np
import pytest

from test_join_cols_nulls_cpu import _layout

NO_ROW = 0xFFFFFFFFFFFFFFFF
HMJ_E_ARG = -1


def expected_take_str(chars, offsets, mask, row_map):
    """What hmj_take_str_device writes.  chars: the source bytes (uint8 array or bytes), offsets: n_src + 1 integers into
    them (offsets[0] need not be 0; the entries of a row that is NULL or never taken are not looked at), mask: None or
    n_src bools (True = valid), row_map: integers, NO_ROW = no source row.  Returns (chars_out uint8 [total_bytes],
    offsets_out uint64 [n_out + 1], words uint64 [ceil(n_out / 64)] with row i = bit i & 63 of word i >> 6 and padding 0,
    null_count, n_no_row, total_bytes)."""
    raw = bytes(chars) if isinstance(chars, (bytes, bytearray)) else np.ascontiguousarray(chars).view(np.uint8).tobytes()
    off = [int(x) for x in np.asarray(offsets, np.uint64)]
    n_src = len(off) - 1
    rows = [int(x) for x in np.asarray(row_map, np.uint64)]
    n_out = len(rows)
    pieces, out_off, valid, n_no_row = [], [0], [], 0
    for r in rows:
        ok = r != NO_ROW
        n_no_row += not ok
        if ok:
            assert r < n_src, "a map entry beyond the source"
            ok = mask is None or bool(mask[r])
        piece = b""
        if ok:
            assert off[r] <= off[r + 1] <= len(raw), "bad offsets at a taken valid row"
            piece = raw[off[r]:off[r + 1]]
        pieces.append(piece)
        out_off.append(out_off[-1] + len(piece))
        valid.append(ok)
    bits = np.zeros(64 * ((n_out + 63) // 64), bool)
    bits[:n_out] = valid
    words = np.packbits(bits, bitorder="little").view(np.uint64)
    chars_out = np.frombuffer(b"".join(pieces), np.uint8)
    return chars_out, np.array(out_off, np.uint64), words, int(n_out - sum(valid)), int(n_no_row), int(out_off[-1])


def test_the_library_exports_the_entry():
    import hashmergejoin_amd as H

    L = H.load_library()
    assert hasattr(L, "hmj_take_str_device")
    assert L.hmj_abi_version() == 5
    assert H.HMJ_TAKE_NO_ROW == H.HMJ_STR_NO_ROW == NO_ROW


def test_null_ctx_is_an_argument_error():
    import hashmergejoin_amd as H

    L = H.load_library()
    src, dst, opts = H.TakeStrSrc(), H.TakeStrDst(), H.TakeStrOpts()
    opts.struct_size = C.sizeof(H.TakeStrOpts)
    assert L.hmj_take_str_device(None, C.byref(src), 0, None, 0, C.byref(dst), C.byref(opts)) == HMJ_E_ARG


def test_layouts_match_the_header():
    import hashmergejoin_amd as H

    extra = '  std::printf("HMJ_ABI_VERSION %d\\nno_row %d\\n", HMJ_ABI_VERSION, HMJ_TAKE_NO_ROW == HMJ_STR_NO_ROW);\n'
    for name, T in (("hmj_take_str_src", H.TakeStrSrc), ("hmj_take_str_dst", H.TakeStrDst), ("hmj_take_str_opts", H.TakeStrOpts)):
        fields = [n for n, _ in T._fields_]
        got = _layout(name, fields, extra)
        assert int(got["size"]) == C.sizeof(T), name
        for f in fields:
            assert getattr(T, f).offset == int(got[f]), (name, f)
        assert (int(got["HMJ_ABI_VERSION"]), int(got["no_row"])) == (5, 1)
    assert (C.sizeof(H.TakeStrSrc), C.sizeof(H.TakeStrDst), C.sizeof(H.TakeStrOpts)) == (40, 48, 24)
    assert H.TakeStrOpts.reserved.offset + 4 == 8  # the smallest struct_size the entry takes
    # the structs the other entries take are what they were
    assert (C.sizeof(H.TakeSrc), C.sizeof(H.TakeDst), C.sizeof(H.TakeOpts)) == (32, 24, 24)
    assert (C.sizeof(H.Validity), C.sizeof(H.StrRel), C.sizeof(H.KeyCol), C.sizeof(H.ColsRel), C.sizeof(H.ColsJoinOpts),
            C.sizeof(H.ColsKindOpts)) == (16, 32, 16, 32, 48, 144)


@pytest.mark.parametrize("keys", [[], [b""], [b"", b"", b""], [b"a", b"", b"bc\x00d", b"\x00", b"\xff\x80", b""],
                                  ["grüß", "", "x"]])
def test_unpack_strings_inverts_pack_strings(keys):
    import hashmergejoin_amd as H

    chars, offsets = H.pack_strings(keys)
    want = [k.encode("utf-8") if isinstance(k, str) else k for k in keys]
    assert H.unpack_strings(chars, offsets) == want
    assert H.unpack_strings(chars.numpy(), offsets.numpy()) == want
    valid = [i % 2 == 0 for i in range(len(keys))]
    assert H.unpack_strings(chars, offsets, valid) == [k if v else None for k, v in zip(want, valid)]
    assert H.unpack_strings(chars, offsets, np.array(valid, bool)) == [k if v else None for k, v in zip(want, valid)]
    with pytest.raises(ValueError):
        H.unpack_strings(chars, offsets, valid + [True])
    # and the other way round
    c2, o2 = H.pack_strings(H.unpack_strings(chars, offsets))
    assert np.array_equal(c2.numpy(), chars.numpy()) and np.array_equal(o2.numpy(), offsets.numpy())


# The hand-written case: 5 source rows, 7 output rows.  The chars start with two bytes no row owns (offsets[0] = 2); row 1
# is NULL with the bytes "XXX" under it, which must not come out; row 2 is a valid empty string; row 4 holds a NUL and a byte
# >= 0x80.  The map takes row 3 twice, has two NO_ROW entries and takes the NULL row once.
HAND_CHARS = b"??" + b"ab" + b"XXX" + b"" + b"cde" + b"\x00\xfe"
HAND_OFFSETS = [2, 4, 7, 7, 10, 12]
HAND_MASK = [True, False, True, True, True]
HAND_MAP = [4, NO_ROW, 3, 1, 2, 3, NO_ROW]
HAND_OUT = [b"\x00\xfe", None, b"cde", None, b"", b"cde", None]
HAND_OUT_CHARS = b"\x00\xfecdecde"
HAND_OUT_OFFSETS = [0, 2, 2, 5, 5, 5, 8, 8]
HAND_WORD = 0b0110101  # row 0 is bit 0
HAND_COUNTS = (3, 2, 8)  # null_count, n_no_row, total_bytes


def test_expectation_on_the_hand_written_case():
    import hashmergejoin_amd as H

    chars, offsets, words, nulls, n_no_row, total = expected_take_str(HAND_CHARS, HAND_OFFSETS, HAND_MASK, HAND_MAP)
    assert chars.dtype == np.uint8 and chars.tobytes() == HAND_OUT_CHARS
    assert offsets.dtype == np.uint64 and offsets.tolist() == HAND_OUT_OFFSETS
    assert words.dtype == np.uint64 and words.tolist() == [HAND_WORD]
    assert (nulls, n_no_row, total) == HAND_COUNTS
    assert H.unpack_strings(chars, offsets, H.unpack_validity(words, 7)) == HAND_OUT
    # a uint8 array for the chars gives the same
    again = expected_take_str(np.frombuffer(HAND_CHARS, np.uint8), np.array(HAND_OFFSETS, np.int64), np.array(HAND_MASK), HAND_MAP)
    assert again[0].tobytes() == HAND_OUT_CHARS and again[1].tolist() == HAND_OUT_OFFSETS and again[3:] == HAND_COUNTS
    # no bitmap: the bytes under row 1 are a string like any other
    chars, offsets, words, nulls, n_no_row, total = expected_take_str(HAND_CHARS, HAND_OFFSETS, None, HAND_MAP)
    assert chars.tobytes() == b"\x00\xfecdeXXXcde" and words.tolist() == [0b0111101] and (nulls, n_no_row, total) == (2, 2, 11)
    # the offsets of a row that is NULL or never taken may hold anything: row 1 (NULL) and row 0 (not in the map)
    odd = [999, 9, 7, 7, 10, 12]  # row 0 = [999, 9) and row 1 = [9, 7): both decreasing
    got = expected_take_str(HAND_CHARS, odd, HAND_MASK, HAND_MAP)
    assert got[0].tobytes() == HAND_OUT_CHARS and got[1].tolist() == HAND_OUT_OFFSETS
    # 65 rows, no NO_ROW, no bitmap: all-ones words with zero padding
    got = expected_take_str(HAND_CHARS, HAND_OFFSETS, None, np.arange(65) % 5)
    assert got[2].tolist() == [2 ** 64 - 1, 1] and got[3:5] == (0, 0)
    # an empty map, and an empty source under a map of NO_ROW alone
    got = expected_take_str(b"", [0], None, [])
    assert len(got[0]) == 0 and got[1].tolist() == [0] and len(got[2]) == 0 and got[3:] == (0, 0, 0)
    got = expected_take_str(b"", [5], [], [NO_ROW] * 3)
    assert len(got[0]) == 0 and got[1].tolist() == [0, 0, 0, 0] and got[2].tolist() == [0] and got[3:] == (3, 3, 0)
