"""CPU-only checks of the string-key join (hmj_hash_str_device / hmj_join_str_device): both symbols are exported, bad
arguments fail without a device, the ctypes mirrors have the header's layout (g++ prints sizeof / offsetof), the
pure-Python restatement of libstdc++'s _Hash_bytes equals every std::hash<std::string> value in tests/golden/str_hash.json,
and pack_strings round-trips.  `str_hash` is imported by test_join_str_gpu.py as its expectation."""
import ctypes as C
import json
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M64 = (1 << 64) - 1
MUL = 0xC6A4A7935BD1E995
SEED = 0xC70F6907


def _shift_mix(v):
    return v ^ (v >> 47)


def str_hash(key, hash_bits=0):
    """std::hash<std::string> of `key` (bytes) as libstdc++ computes it on 64-bit targets (_Hash_bytes, seed 0xc70f6907);
    hash_bits 1..63: the top hash_bits bits (h >> (64 - hash_bits))."""
    n = len(key)
    h = (SEED ^ (n * MUL)) & M64
    full = n & ~7
    for p in range(0, full, 8):
        d = int.from_bytes(key[p:p + 8], "little")
        d = (_shift_mix((d * MUL) & M64) * MUL) & M64
        h = ((h ^ d) * MUL) & M64
    if n & 7:
        h = ((h ^ int.from_bytes(key[full:], "little")) * MUL) & M64
    h = _shift_mix((_shift_mix(h) * MUL) & M64)
    return h >> (64 - hash_bits) if hash_bits else h


def load_str_hash_golden():
    doc = json.load(open(os.path.join(ROOT, "tests", "golden", "str_hash.json")))
    return [(bytes.fromhex(c["key_hex"]), int(c["hash"])) for c in doc["cases"]]


# ---------------------------------------------------------------------------------------------
def test_str_entries_are_exported():
    import hashmergejoin_amd as H

    L = H.load_library()
    assert hasattr(L, "hmj_hash_str_device") and hasattr(L, "hmj_join_str_device")


def test_str_null_ctx_is_an_argument_error():
    import hashmergejoin_amd as H

    L = H.load_library()
    rel = H.StrRel()
    opts = H.StrJoinOpts()
    opts.struct_size = C.sizeof(H.StrJoinOpts)
    res = H.StrResult()
    assert L.hmj_join_str_device(None, C.byref(rel), C.byref(rel), 0, C.byref(opts), C.byref(res)) == -1  # HMJ_E_ARG
    assert L.hmj_join_str_device(None, None, None, 0, None, None) == -1
    assert L.hmj_hash_str_device(None, None, None, 0, 0, None) == -1


def test_str_structs_match_the_header():
    import hashmergejoin_amd as H

    src = r"""
#include <cstddef>
#include <cstdio>
#include "hmj.h"
#define F(T, m) std::printf("%s.%s %zu\n", #T, #m, offsetof(T, m));
int main() {
  std::printf("hmj_str_rel %zu\nhmj_str_join_opts %zu\nhmj_str_result %zu\n", sizeof(hmj_str_rel), sizeof(hmj_str_join_opts),
              sizeof(hmj_str_result));
  F(hmj_str_rel, chars) F(hmj_str_rel, offsets) F(hmj_str_rel, vals) F(hmj_str_rel, n)
  F(hmj_str_join_opts, struct_size) F(hmj_str_join_opts, hash_bits) F(hmj_str_join_opts, n_hash_pairs)
  F(hmj_str_join_opts, n_collisions) F(hmj_str_join_opts, ms_hash) F(hmj_str_join_opts, ms_join)
  F(hmj_str_join_opts, ms_verify) F(hmj_str_join_opts, ms_order)
  F(hmj_str_result, n_matches) F(hmj_str_result, sum_r) F(hmj_str_result, sum_s) F(hmj_str_result, xor_fold)
  F(hmj_str_result, mix_sum) F(hmj_str_result, sum_probe_all) F(hmj_str_result, hash) F(hmj_str_result, r_row)
  F(hmj_str_result, s_row) F(hmj_str_result, rval) F(hmj_str_result, sval)
  return 0;
}
"""
    with tempfile.TemporaryDirectory() as d:
        cc, exe = os.path.join(d, "layout.cc"), os.path.join(d, "layout")
        open(cc, "w").write(src)
        subprocess.check_call(["g++", "-std=c++11", "-I", os.path.join(ROOT, "include"), cc, "-o", exe])
        got = dict(line.split() for line in subprocess.check_output([exe]).decode().splitlines())
    mirrors = {"hmj_str_rel": H.StrRel, "hmj_str_join_opts": H.StrJoinOpts, "hmj_str_result": H.StrResult}
    for cname, cls in mirrors.items():
        assert int(got[cname]) == C.sizeof(cls), cname
        fields = [k for k in got if k.startswith(cname + ".")]
        assert [k.split(".")[1] for k in fields] == [n for n, _ in cls._fields_], cname
        for k in fields:
            assert getattr(cls, k.split(".")[1]).offset == int(got[k]), k


def test_python_hash_bytes_equals_libstdcxx():
    cases = load_str_hash_golden()
    lengths = {len(k) for k, _ in cases}
    assert set(range(81)) <= lengths and len(cases) >= 600
    assert any(b"\x00" in k for k, _ in cases) and any(max(k, default=0) >= 0x80 for k, _ in cases)
    for k, h in cases:
        assert str_hash(k) == h, k
    k, h = cases[30]
    assert str_hash(k, 12) == h >> 52 and str_hash(k, 63) == h >> 1


def test_pack_strings_round_trips():
    import hashmergejoin_amd as H

    keys = ["", "a", "", "nul\x00inside", "héllo wörld", b"\xff\x00\x80", "日本", ""]
    chars, offsets = H.pack_strings(keys)
    assert chars.device.type == "cpu" and offsets.device.type == "cpu"
    assert str(chars.dtype) == "torch.uint8" and str(offsets.dtype) == "torch.int64"
    o = offsets.numpy()
    b = chars.numpy().tobytes()
    assert len(o) == len(keys) + 1 and o[0] == 0 and o[-1] == len(b)
    back = [b[o[i]:o[i + 1]] for i in range(len(keys))]
    assert back == [k.encode("utf-8") if isinstance(k, str) else k for k in keys]
    c0, o0 = H.pack_strings([])
    assert c0.numel() == 0 and o0.tolist() == [0]
    c1, o1 = H.pack_strings(["", ""])
    assert c1.numel() == 0 and o1.tolist() == [0, 0, 0]
    assert np.all(np.diff(o) >= 0)
