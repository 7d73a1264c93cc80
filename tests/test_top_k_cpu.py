"""hmj_top_k_device without a GPU (include/hmj.h, "the first rows of an order"): the library exports the entry, the mirror
of hmj_top_k_opts and the HMJ_TOPK_* constants match the header, the ABI version stays, and `expected_top_k` is the slice of
the comparator's order with saturating arithmetic."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

from test_order_by_cpu import SWEEP_SEED, brute_order, case_columns, draw_order_case, edge_tables

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HMJ_E_ARG = -1
FIELDS = ["struct_size", "plan", "offset", "max_tie_rows", "n_out", "n_candidates", "n_tie_rows", "plan_taken", "n_levels", "n_rounds",
          "reserved", "ms_select", "ms_emit", "ms_order"]


def test_the_library_exports_the_entry_and_refuses_a_null_ctx():
    import hashmergejoin_amd as H

    L = H.load_library()
    assert hasattr(L, "hmj_top_k_device")
    col, opts = H.OrderCol(), H.TopKOpts()
    opts.struct_size = C.sizeof(H.TopKOpts)
    assert L.hmj_top_k_device(None, C.byref(col), 1, 0, 0, None, C.byref(opts)) == HMJ_E_ARG
    for name in ["TopKOpts", "HMJ_TOPK_AUTO", "HMJ_TOPK_SELECT", "HMJ_TOPK_FULL", "expected_top_k"]:
        assert name in H.__all__ and hasattr(H, name), name
    assert hasattr(H.Executor, "top_k_device")
    from hashmergejoin_amd import _lib, _topk, join, reference

    assert H.TopKOpts is _topk.TopKOpts and not hasattr(_lib, "TopKOpts")  # the mirror lives beside _lib, as _window's do
    assert join.expected_top_k is reference.expected_top_k is H.expected_top_k


def test_the_mirror_and_the_constants_match_the_header_and_the_abi_version_stays():
    import hashmergejoin_amd as H

    consts = ["HMJ_TOPK_AUTO", "HMJ_TOPK_SELECT", "HMJ_TOPK_FULL", "HMJ_ABI_VERSION"]
    lines = ['std::printf("sizeof %zu\\n", sizeof(hmj_top_k_opts));']
    lines += ['std::printf("%s %%zu\\n", offsetof(hmj_top_k_opts, %s));' % (f, f) for f in FIELDS]
    lines += ['std::printf("%s %%lld\\n", (long long)%s);' % (k, k) for k in consts]
    src = '#include <cstddef>\n#include <cstdio>\n#include "hmj.h"\nint main() {\n%s\nreturn 0;\n}\n' % "\n".join(lines)
    with tempfile.TemporaryDirectory() as d:
        cc, exe = os.path.join(d, "layout.cc"), os.path.join(d, "layout")
        open(cc, "w").write(src)
        subprocess.check_call(["g++", "-std=c++11", "-I", os.path.join(ROOT, "include"), cc, "-o", exe])
        got = {k: int(v) for k, v in (line.split() for line in subprocess.check_output([exe]).decode().splitlines())}
    assert got["sizeof"] == C.sizeof(H.TopKOpts)
    assert [f for f, _ in H.TopKOpts._fields_] == FIELDS
    for f in FIELDS:
        assert got[f] == getattr(H.TopKOpts, f).offset, f
    assert [got[k] for k in consts[:3]] == [H.HMJ_TOPK_AUTO, H.HMJ_TOPK_SELECT, H.HMJ_TOPK_FULL] == [0, 1, 2]
    assert got["HMJ_ABI_VERSION"] == 5  # a new entry with structs of its own: nothing existing changed
    assert H.load_library().hmj_abi_version() == 5


def cuts(n):
    return [0, 1, 2, max(n - 1, 0), n, n + 5, 2 ** 63, 2 ** 64 - 1]


def check_reference(H, columns, pairs, tag):
    full = brute_order(columns)
    n = len(full)
    for k, offset in pairs:
        got = H.expected_top_k(columns, k, offset)
        assert got.dtype == np.uint64 and np.array_equal(got, full[offset:offset + k]), (tag, k, offset)
        assert len(got) == min(k, n - min(n, offset))


def test_the_reference_is_the_slice_of_the_comparators_order_on_the_edge_tables():
    import hashmergejoin_amd as H

    for tag, columns in edge_tables():
        n = len(columns[0][0])
        check_reference(H, columns, [(k, o) for k in cuts(n) for o in cuts(n)], tag)
    assert len(H.expected_top_k([(np.zeros(0, np.int32), 0)], 3, 0)) == 0
    assert H.expected_top_k([(np.array([3, 1, 2, 1], np.int32), 0)], 2, 1).tolist() == [3, 2]


def test_the_reference_is_the_slice_of_the_comparators_order_on_drawn_cases():
    import hashmergejoin_amd as H

    rng = np.random.default_rng(SWEEP_SEED + 1)
    for it in range(20):
        case = draw_order_case(rng, it)
        n = min(case["n"], 1500)  # (the comparator is Python)
        columns = [(v[:n], f, None if ok is None else ok[:n]) for v, f, ok in case_columns(case)]
        pool = cuts(n)
        pairs = [(int(pool[a]), int(pool[b])) for a, b in rng.integers(0, len(pool), size=(6, 2))]
        check_reference(H, columns, pairs, "case %d" % it)
