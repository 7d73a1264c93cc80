"""CPU-only checks of the multi-column key join (hmj_join_cols_device): the symbol is exported, bad arguments fail without a
device, the ctypes mirrors have the header's layout (g++ prints sizeof / offsetof), and `cols_key64` -- the host restatement
of the 64-bit join key, which test_join_cols_gpu.py takes as its expectation -- packs in tuple order and hashes as
include/hmj.h defines."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M64 = (1 << 64) - 1
HMJ_E_ARG = -1


def test_cols_entry_is_exported():
    import hashmergejoin_amd as H

    L = H.load_library()
    assert hasattr(L, "hmj_join_cols_device")
    assert (H.HMJ_COLS_PACKED, H.HMJ_COLS_HASHED, H.HMJ_MAX_KEY_COLS) == (1, 2, 8)


def test_cols_null_ctx_is_an_argument_error():
    import hashmergejoin_amd as H

    L = H.load_library()
    col = (H.KeyCol * 1)()
    col[0].width = 4
    rel = H.ColsRel()
    rel.cols, rel.n_cols = col, 1
    opts = H.ColsJoinOpts()
    opts.struct_size = C.sizeof(H.ColsJoinOpts)
    res = H.ColsResult()
    assert L.hmj_join_cols_device(None, C.byref(rel), C.byref(rel), 0, C.byref(opts), C.byref(res)) == HMJ_E_ARG
    assert L.hmj_join_cols_device(None, None, None, 0, None, None) == HMJ_E_ARG


def test_cols_structs_match_the_header():
    import hashmergejoin_amd as H

    src = r"""
#include <cstddef>
#include <cstdio>
#include "hmj.h"
#define F(T, m) std::printf("%s.%s %zu\n", #T, #m, offsetof(T, m));
int main() {
  std::printf("hmj_key_col %zu\nhmj_cols_rel %zu\nhmj_cols_join_opts %zu\nhmj_cols_result %zu\n", sizeof(hmj_key_col),
              sizeof(hmj_cols_rel), sizeof(hmj_cols_join_opts), sizeof(hmj_cols_result));
  std::printf("HMJ_MAX_KEY_COLS %d\nHMJ_COLS_PACKED %u\nHMJ_COLS_HASHED %u\nHMJ_ABI_VERSION %d\n", HMJ_MAX_KEY_COLS, HMJ_COLS_PACKED,
              HMJ_COLS_HASHED, HMJ_ABI_VERSION);
  F(hmj_key_col, data) F(hmj_key_col, width) F(hmj_key_col, reserved)
  F(hmj_cols_rel, cols) F(hmj_cols_rel, n_cols) F(hmj_cols_rel, reserved) F(hmj_cols_rel, vals) F(hmj_cols_rel, n)
  F(hmj_cols_join_opts, struct_size) F(hmj_cols_join_opts, hash_bits) F(hmj_cols_join_opts, force_hashed)
  F(hmj_cols_join_opts, form) F(hmj_cols_join_opts, n_key_pairs) F(hmj_cols_join_opts, n_collisions)
  F(hmj_cols_join_opts, ms_key) F(hmj_cols_join_opts, ms_join) F(hmj_cols_join_opts, ms_verify) F(hmj_cols_join_opts, ms_order)
  F(hmj_cols_result, n_matches) F(hmj_cols_result, sum_r) F(hmj_cols_result, sum_s) F(hmj_cols_result, xor_fold)
  F(hmj_cols_result, mix_sum) F(hmj_cols_result, sum_probe_all) F(hmj_cols_result, key64) F(hmj_cols_result, r_row)
  F(hmj_cols_result, s_row) F(hmj_cols_result, rval) F(hmj_cols_result, sval)
  return 0;
}
"""
    with tempfile.TemporaryDirectory() as d:
        cc, exe = os.path.join(d, "layout.cc"), os.path.join(d, "layout")
        open(cc, "w").write(src)
        subprocess.check_call(["g++", "-std=c++11", "-I", os.path.join(ROOT, "include"), cc, "-o", exe])
        got = dict(line.split() for line in subprocess.check_output([exe]).decode().splitlines())
    assert (int(got["HMJ_MAX_KEY_COLS"]), int(got["HMJ_COLS_PACKED"]), int(got["HMJ_COLS_HASHED"])) == (
        H.HMJ_MAX_KEY_COLS, H.HMJ_COLS_PACKED, H.HMJ_COLS_HASHED)
    assert int(got["HMJ_ABI_VERSION"]) == 5  # no existing struct changed; the new ones are size-versioned
    mirrors = {"hmj_key_col": H.KeyCol, "hmj_cols_rel": H.ColsRel, "hmj_cols_join_opts": H.ColsJoinOpts,
               "hmj_cols_result": H.ColsResult}
    for cname, cls in mirrors.items():
        assert int(got[cname]) == C.sizeof(cls), cname
        fields = [k for k in got if k.startswith(cname + ".")]
        assert [k.split(".")[1] for k in fields] == [n for n, _ in cls._fields_], cname
        for k in fields:
            assert getattr(cls, k.split(".")[1]).offset == int(got[k]), k


def _draw(rng, widths, n):
    """n tuples over `widths`: few distinct values per column (ties in the leading columns) and the extremes."""
    cols = []
    for w in widths:
        top = (1 << (8 * w)) - 1
        pool = np.array([0, 1, top, top - 1, top >> 1, (top >> 1) + 1] + [int(x) for x in rng.integers(0, top, 6, dtype=np.uint64, endpoint=True)],
                        np.uint64)
        cols.append(pool[rng.integers(0, len(pool), n)].astype("u%d" % w))
    return cols


def test_packed_key64_sorts_as_the_tuples_sort():
    import hashmergejoin_amd as H

    rng = np.random.default_rng(20260117)
    for widths in ([1, 2, 4], [4, 4], [8], [2, 2, 2, 2], [1], [4, 2, 1, 1], [1, 1, 1, 1, 1, 1, 1, 1], [2, 4]):
        cols = _draw(rng, widths, 400)
        key = H.cols_key64(cols, widths)
        assert key.dtype == np.uint64 and key.shape == (400,)
        tuples = [tuple(int(c[i]) for c in cols) for i in range(400)]
        # the definition, in plain integers: column 0 most significant in the low sum(widths) bytes
        for i in (0, 1, 199, 399):
            want = 0
            for v, w in zip(tuples[i], widths):
                want = (want << (8 * w)) | v
            assert int(key[i]) == want and want >> (8 * sum(widths)) == 0
        order = sorted(range(400), key=lambda i: (tuples[i], i))
        assert list(np.argsort(key, kind="stable")) == order, widths
        assert len(set(key.tolist())) == len(set(tuples)), widths  # equal key64 exactly when equal tuples
    # signed integers and floats are their bytes
    a, b = np.array([-1, 0, -2 ** 31], np.int32), np.array([-0.0, 0.0, np.nan], np.float32)
    k = H.cols_key64([a, b], [4, 4])
    assert [int(x) for x in k] == [(0xFFFFFFFF << 32) | 0x80000000, 0, (0x80000000 << 32) | int(b.view(np.uint32)[2])]
    assert int(k[0]) != int(H.cols_key64([a[:1], b[1:2]], [4, 4])[0])  # -0.0 != 0.0


def test_hashed_key64_equals_the_definition():
    import hashmergejoin_amd as H

    # h = k; h = mix64(h + v_c + 0x9E3779B97F4A7C15) per column; computed once from that definition with plain integers
    cases = [
        ([1, 2, 3], [8, 4, 2], 0xE15CA7D62D35B26D),
        ([0xFFFFFFFFFFFFFFFF, 0xFFFFFFFF, 0xFFFF], [8, 4, 2], 0xCF150816CB030AC7),
        ([0x0123456789ABCDEF, 0xDEADBEEF, 0x8001, 0x7F, 5, 6, 7, 8], [8, 4, 2, 1, 8, 8, 8, 8], 0x18C8C537F94641D2),
    ]
    for vals, widths, want in cases:
        cols = [np.array([v], "u%d" % w) for v, w in zip(vals, widths)]
        assert int(H.cols_key64(cols, widths)[0]) == want
        for bits in (1, 6, 12, 63):  # hash_bits keeps the top bits
            assert int(H.cols_key64(cols, widths, hash_bits=bits)[0]) == want >> (64 - bits)
    # one 8-byte column of value 0: splitmix64's first output for seed 1
    assert int(H.cols_key64([np.zeros(1, np.uint64)], [8], force_hashed=True)[0]) == 0x910A2DEC89025CC1
    # a key that fits 8 bytes is hashed only when forced, and hash_bits touches the hashed form only
    c44 = [np.array([7], np.uint32), np.array([9], np.uint32)]
    assert int(H.cols_key64(c44, [4, 4])[0]) == (7 << 32) | 9 == int(H.cols_key64(c44, [4, 4], hash_bits=6)[0])
    forced = int(H.cols_key64(c44, [4, 4], force_hashed=True)[0])
    assert forced != (7 << 32) | 9 and int(H.cols_key64(c44, [4, 4], hash_bits=6, force_hashed=True)[0]) == forced >> 58
    # vectorised == element by element
    rng = np.random.default_rng(5)
    cols = _draw(rng, [8, 4, 2], 50)
    many = H.cols_key64(cols, [8, 4, 2], hash_bits=9)
    for i in (0, 17, 49):
        assert int(many[i]) == int(H.cols_key64([c[i:i + 1] for c in cols], [8, 4, 2], hash_bits=9)[0])
