"""CPU-only checks of the mixed-key join (hmj_join_mixed_device): the symbol is exported, a NULL ctx fails without a device,
the ctypes mirrors have the header's layout (g++ prints sizeof / offsetof), and `mixed_key64` -- the host restatement of the
64-bit join key, which test_join_mixed_gpu.py takes as its expectation -- is the column join's hash chain with a string
column contributing std::hash<std::string> of its bytes (str_hash of test_join_str_cpu.py, pinned by the libstdc++ goldens)."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

from test_join_str_cpu import str_hash

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M64 = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15
HMJ_E_ARG = -1


def mix64(x):
    x ^= x >> 30
    x = (x * 0xBF58476D1CE4E5B9) & M64
    x ^= x >> 27
    x = (x * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def test_mixed_entry_is_exported():
    import hashmergejoin_amd as H

    L = H.load_library()
    assert hasattr(L, "hmj_join_mixed_device")
    assert (H.HMJ_KEY_FIXED, H.HMJ_KEY_LARGE_STRING) == (0, 1)


def test_mixed_null_ctx_is_an_argument_error():
    import hashmergejoin_amd as H

    L = H.load_library()
    col = (H.MixedCol * 1)()
    col[0].type, col[0].width = H.HMJ_KEY_FIXED, 4
    rel = H.MixedRel()
    rel.cols, rel.n_cols = col, 1
    opts = H.MixedOpts()
    opts.struct_size = C.sizeof(H.MixedOpts)
    res = H.ColsResult()
    assert L.hmj_join_mixed_device(None, C.byref(rel), C.byref(rel), 0, C.byref(opts), C.byref(res)) == HMJ_E_ARG
    assert L.hmj_join_mixed_device(None, None, None, 0, None, None) == HMJ_E_ARG


def test_mixed_structs_match_the_header():
    import hashmergejoin_amd as H

    src = r"""
#include <cstddef>
#include <cstdio>
#include "hmj.h"
#define F(T, m) std::printf("%s.%s %zu\n", #T, #m, offsetof(T, m));
int main() {
  std::printf("hmj_mixed_col %zu\nhmj_mixed_rel %zu\nhmj_mixed_opts %zu\n", sizeof(hmj_mixed_col), sizeof(hmj_mixed_rel),
              sizeof(hmj_mixed_opts));
  std::printf("HMJ_KEY_FIXED %u\nHMJ_KEY_LARGE_STRING %u\nHMJ_ABI_VERSION %d\n", HMJ_KEY_FIXED, HMJ_KEY_LARGE_STRING, HMJ_ABI_VERSION);
  F(hmj_mixed_col, type) F(hmj_mixed_col, width) F(hmj_mixed_col, data) F(hmj_mixed_col, offsets) F(hmj_mixed_col, validity)
  F(hmj_mixed_rel, cols) F(hmj_mixed_rel, n_cols) F(hmj_mixed_rel, reserved) F(hmj_mixed_rel, vals) F(hmj_mixed_rel, n)
  F(hmj_mixed_opts, struct_size) F(hmj_mixed_opts, side) F(hmj_mixed_opts, kind) F(hmj_mixed_opts, hash_bits)
  F(hmj_mixed_opts, probe_fill) F(hmj_mixed_opts, build_fill) F(hmj_mixed_opts, counts) F(hmj_mixed_opts, n_key_pairs)
  F(hmj_mixed_opts, n_collisions) F(hmj_mixed_opts, n_build_null) F(hmj_mixed_opts, n_probe_null) F(hmj_mixed_opts, ms_key)
  F(hmj_mixed_opts, ms_join) F(hmj_mixed_opts, ms_verify) F(hmj_mixed_opts, ms_emit) F(hmj_mixed_opts, ms_order)
  return 0;
}
"""
    with tempfile.TemporaryDirectory() as d:
        cc, exe = os.path.join(d, "layout.cc"), os.path.join(d, "layout")
        open(cc, "w").write(src)
        subprocess.check_call(["g++", "-std=c++11", "-I", os.path.join(ROOT, "include"), cc, "-o", exe])
        got = dict(line.split() for line in subprocess.check_output([exe]).decode().splitlines())
    assert (int(got["HMJ_KEY_FIXED"]), int(got["HMJ_KEY_LARGE_STRING"])) == (H.HMJ_KEY_FIXED, H.HMJ_KEY_LARGE_STRING)
    assert int(got["HMJ_ABI_VERSION"]) == 5  # no existing struct changed; the new ones are size-versioned
    mirrors = {"hmj_mixed_col": H.MixedCol, "hmj_mixed_rel": H.MixedRel, "hmj_mixed_opts": H.MixedOpts}
    for cname, cls in mirrors.items():
        assert int(got[cname]) == C.sizeof(cls), cname
        fields = [k for k in got if k.startswith(cname + ".")]
        assert [k.split(".")[1] for k in fields] == [n for n, _ in cls._fields_], cname
        for k in fields:
            assert getattr(cls, k.split(".")[1]).offset == int(got[k]), k


def test_mixed_key64_of_fixed_columns_is_the_column_joins_hashed_key():
    import hashmergejoin_amd as H

    rng = np.random.default_rng(20261019)
    for widths in ([4], [8], [4, 4], [1, 2, 4], [8, 4, 2], [2, 2, 2, 2], [1, 1, 1, 1, 1, 1, 1, 1], [8, 8, 8]):
        cols = [rng.integers(0, 1 << (8 * w), 200, dtype=np.uint64, endpoint=False).astype("u%d" % w) if w < 8
                else rng.integers(0, M64, 200, dtype=np.uint64, endpoint=True) for w in widths]
        for bits in (0, 1, 7, 33, 63):
            assert np.array_equal(H.mixed_key64(cols, bits), H.cols_key64(cols, widths, hash_bits=bits, force_hashed=True)), (widths, bits)
    # signed integers are their bytes, zero-extended from their width
    a = np.array([-1, 0, -2 ** 31], np.int32)
    assert np.array_equal(H.mixed_key64([a]), H.cols_key64([a], [4], force_hashed=True))


def test_mixed_key64_of_a_string_column_is_std_hash_in_the_chain():
    import hashmergejoin_amd as H

    keys = [b"", b"a", b"ab", b"abcdefg", b"abcdefgh", b"abcdefghi", b"\x00", b"\x00\x00", b"\xff" * 17, b"x" * 100, "hé".encode()]
    got = H.mixed_key64([keys])
    for k, g in zip(keys, got):
        assert int(g) == mix64((1 + str_hash(k) + GOLDEN) & M64), k
    # a string column between two fixed ones: the chain in plain integers
    u16, u64 = np.array([7, 65535], np.uint16), np.array([1 << 63, 3], np.uint64)
    got = H.mixed_key64([u16, [b"left", b""], u64])
    for i, s in enumerate((b"left", b"")):
        h = 3
        for v in (int(u16[i]), str_hash(s), int(u64[i])):
            h = mix64((h + v + GOLDEN) & M64)
        assert int(got[i]) == h
    # the length is inside the string's hash: the same bytes cut elsewhere are another key
    two = H.mixed_key64([[b"ab", b"a"], [b"c", b"bc"]])
    assert int(two[0]) != int(two[1])
    # hash_bits keeps the top bits
    cols = [[b"alpha", b"beta", b""], np.array([1, 2, 3], np.int32)]
    full = H.mixed_key64(cols)
    for bits in (1, 63):
        assert [int(x) for x in H.mixed_key64(cols, bits)] == [int(x) >> (64 - bits) for x in full]
