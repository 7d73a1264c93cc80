"""CPU-only checks of hmj_take_cols_device (include/hmj.h, "taking fixed-width columns through a row map"): the library
exports the entry and refuses a NULL ctx without a GPU, the ctypes mirrors of hmj_take_src / hmj_take_dst / hmj_take_opts
have the header's layout (g++ prints sizeof / offsetof) while HMJ_ABI_VERSION stays 5, `unpack_validity` inverts
`pack_validity`, and `expected_take` -- the pure-numpy expectation test_take_cols_gpu.py imports -- is pinned on a case
written out by hand."""
import ctypes as C

import numpy as np
import pytest

from test_join_cols_nulls_cpu import _layout

NO_ROW = 0xFFFFFFFFFFFFFFFF
HMJ_E_ARG = -1


def expected_take(cols, masks, row_map):
    """What hmj_take_cols_device writes.  cols: one numpy array per source column, 1-D of 1 / 2 / 4 / 8-byte items or [n,2]
    uint64 (a 16-byte column); masks: None, or per column None / a bool array (True = valid); row_map: integers, NO_ROW =
    no source row.  Returns (data, words, null_count, n_no_row): per column the output values (the sources' dtype and
    shape, zero bytes under a NULL slot), the ceil(n_out / 64) uint64 bitmap words (row i = bit i & 63 of word i >> 6,
    padding 0) and the NULL slots; the map entries equal to NO_ROW."""
    row_map = np.asarray(row_map, np.uint64)
    n_out = len(row_map)
    there = row_map != np.uint64(NO_ROW)
    idx = row_map[there].astype(np.int64)
    data, words, nulls = [], [], []
    for c, col in enumerate(cols):
        col = np.asarray(col)
        assert not len(idx) or int(idx.max()) < len(col), "a map entry beyond the source"
        valid = there.copy()
        m = None if masks is None else masks[c]
        if m is not None:
            valid[there] = np.asarray(m, bool)[idx]
        out = np.zeros((n_out,) + col.shape[1:], col.dtype)
        out[valid] = col[row_map[valid].astype(np.int64)]
        bits = np.zeros(64 * ((n_out + 63) // 64), bool)
        bits[:n_out] = valid
        data.append(out)
        words.append(np.packbits(bits, bitorder="little").view(np.uint64))
        nulls.append(int(n_out - valid.sum()))
    return data, words, nulls, int(n_out - there.sum())


def test_the_library_exports_the_entry():
    import hashmergejoin_amd as H

    L = H.load_library()
    assert hasattr(L, "hmj_take_cols_device")
    assert L.hmj_abi_version() == 5
    assert H.HMJ_TAKE_NO_ROW == H.HMJ_COLS_NO_ROW == H.HMJ_STR_NO_ROW == NO_ROW and H.HMJ_MAX_TAKE_COLS == 64


def test_null_ctx_is_an_argument_error():
    import hashmergejoin_amd as H

    L = H.load_library()
    src, dst, opts = (H.TakeSrc * 1)(), (H.TakeDst * 1)(), H.TakeOpts()
    opts.struct_size = C.sizeof(H.TakeOpts)
    assert L.hmj_take_cols_device(None, src, 1, 0, None, 0, dst, C.byref(opts)) == HMJ_E_ARG


def test_layouts_match_the_header():
    import hashmergejoin_amd as H

    extra = ('  std::printf("HMJ_ABI_VERSION %d\\nmax_cols %d\\nno_row %d\\n", HMJ_ABI_VERSION, HMJ_MAX_TAKE_COLS, '
             "HMJ_TAKE_NO_ROW == HMJ_COLS_NO_ROW && HMJ_TAKE_NO_ROW == HMJ_STR_NO_ROW && HMJ_TAKE_NO_ROW == UINT64_MAX);\n")
    for name, T in (("hmj_take_src", H.TakeSrc), ("hmj_take_dst", H.TakeDst), ("hmj_take_opts", H.TakeOpts)):
        fields = [n for n, _ in T._fields_]
        got = _layout(name, fields, extra)
        assert int(got["size"]) == C.sizeof(T), name
        for f in fields:
            assert getattr(T, f).offset == int(got[f]), (name, f)
        assert (int(got["HMJ_ABI_VERSION"]), int(got["max_cols"]), int(got["no_row"])) == (5, 64, 1)
    assert (C.sizeof(H.TakeSrc), C.sizeof(H.TakeDst), C.sizeof(H.TakeOpts)) == (32, 24, 24)
    assert H.TakeOpts.reserved.offset + 4 == 8  # the smallest struct_size the entry takes
    # the structs the joins take are what they were
    assert (C.sizeof(H.Validity), C.sizeof(H.KeyCol), C.sizeof(H.ColsRel), C.sizeof(H.ColsJoinOpts), C.sizeof(H.ColsKindOpts)) == (16, 16, 32, 48, 144)


# The hand-written case: 5 source rows, 7 output rows.  Column a (2 bytes) has source row 1 NULL, column b (16 bytes) has no
# bitmap, column c (1 byte) has rows 0 and 4 NULL; the values under the NULL slots (0xBEEF, 0xEE) must not come out.
HAND_A = np.array([10, 0xBEEF, 30, 40, 50], np.uint16)
HAND_B = np.array([[1, 2], [3, 4], [5, 6], [7, 8], [9, 2 ** 64 - 1]], np.uint64)
HAND_C = np.array([0xEE, 21, 22, 23, 0xEE], np.uint8)
HAND_MASKS = [np.array([1, 0, 1, 1, 1], bool), None, np.array([0, 1, 1, 1, 0], bool)]
HAND_MAP = [4, NO_ROW, 1, 1, 0, 3, NO_ROW]
HAND_DATA = [[50, 0, 0, 0, 10, 40, 0],
             [[9, 2 ** 64 - 1], [0, 0], [3, 4], [3, 4], [1, 2], [7, 8], [0, 0]],
             [0, 0, 21, 21, 0, 23, 0]]
HAND_WORDS = [0b0110001, 0b0111101, 0b0101100]  # row 0 is bit 0
HAND_NULLS = [4, 2, 4]


def test_expectation_on_the_hand_written_case():
    data, words, nulls, n_no_row = expected_take([HAND_A, HAND_B, HAND_C], HAND_MASKS, HAND_MAP)
    for got, want, src in zip(data, HAND_DATA, (HAND_A, HAND_B, HAND_C)):
        assert got.dtype == src.dtype and got.shape[1:] == src.shape[1:]
        assert got.tolist() == want
    assert [w.tolist() for w in words] == [[w] for w in HAND_WORDS]
    assert (nulls, n_no_row) == (HAND_NULLS, 2)
    # no NO_ROW and no bitmap: all-ones words, zero padding, no NULL
    data, words, nulls, n_no_row = expected_take([HAND_A], None, [0, 1, 2])
    assert data[0].tolist() == [10, 0xBEEF, 30] and words[0].tolist() == [0b111] and (nulls, n_no_row) == ([0], 0)
    data, words, nulls, n_no_row = expected_take([HAND_C], [None], np.arange(65) % 5)
    assert words[0].tolist() == [2 ** 64 - 1, 1] and nulls == [0]
    # an empty map, and an empty source under a map of NO_ROW alone
    data, words, nulls, n_no_row = expected_take([HAND_B], None, [])
    assert data[0].shape == (0, 2) and len(words[0]) == 0 and (nulls, n_no_row) == ([0], 0)
    data, words, nulls, n_no_row = expected_take([HAND_A[:0]], [HAND_MASKS[0][:0]], [NO_ROW] * 3)
    assert data[0].tolist() == [0, 0, 0] and words[0].tolist() == [0] and (nulls, n_no_row) == ([3], 3)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 130])
def test_unpack_validity_inverts_pack_validity(n):
    import hashmergejoin_amd as H

    rng = np.random.default_rng(n)
    mask = rng.random(n) < 0.6
    raw = H.pack_validity(mask).numpy()  # bytes, bit offset 0
    padded = np.zeros(8 * ((n + 63) // 64), np.uint8)
    padded[:len(raw)] = raw
    words = padded.view(np.uint64)
    assert np.array_equal(H.unpack_validity(words, n), mask)
    assert np.array_equal(H.unpack_validity(words.view(np.int64), n), mask)
    import torch

    assert np.array_equal(H.unpack_validity(torch.from_numpy(words.view(np.int64).copy()), n), mask)
    # the words are what expected_take writes for an identity map over a column with this bitmap
    _, w, nulls, _ = expected_take([np.arange(n, dtype=np.uint32)], [mask], np.arange(n))
    assert np.array_equal(w[0], words) and nulls == [int(n - mask.sum())]
    with pytest.raises(ValueError):
        H.unpack_validity(words, 64 * len(words) + 1)
