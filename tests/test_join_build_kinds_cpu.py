"""CPU-only checks of the build-side join kinds (hmj_join_build_kind_u64_device): the symbol is exported, bad arguments
fail loudly without a device, the binding mirrors hmj.h, and the numpy expectation the GPU tests compare against gives the
hand-checked answers on the SURVEY 3.3 iterator_edge inputs.  `expect_build_kind` is imported by
test_join_build_kinds_gpu.py."""
import ctypes as C
import json
import os
import re

import numpy as np

from test_join_kinds_cpu import M64, _inner_rows, tmix

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BSEMI, BANTI, BOUTER, FULL = 1, 2, 3, 4


def expect_build_kind(B, P, kind, build_fill=0, probe_fill=0):
    """Expected result of a build-side kind: (rows sorted as HMJ_ORDERED sorts them, checks dict, counters dict).
    Rows are [n, 2] (key, rval) for BUILD_SEMI / BUILD_ANTI and [n, 3] (key, rval, sval) for the outer kinds; checks take
    sval = 0 for build semi / anti rows, sval = build_fill for unmatched build rows and rval = probe_fill for unmatched
    probe rows.  The probe counters are those of FULL_OUTER (0 for the other kinds)."""
    B = np.ascontiguousarray(B, np.uint64).reshape(-1, 2)
    P = np.ascontiguousarray(P, np.uint64).reshape(-1, 2)
    bhit = np.isin(B[:, 0], P[:, 0])
    phit = np.isin(P[:, 0], B[:, 0])
    if kind in (BSEMI, BANTI):
        sel = B[bhit] if kind == BSEMI else B[~bhit]
        tri = np.stack([sel[:, 0], sel[:, 1], np.zeros(len(sel), np.uint64)], 1)
    else:
        inner, _ = _inner_rows(B, P, False)
        bmiss = B[~bhit]
        parts = [inner.reshape(-1, 3), np.stack([bmiss[:, 0], bmiss[:, 1], np.full(len(bmiss), build_fill, np.uint64)], 1)]
        if kind == FULL:
            pmiss = P[~phit]
            parts.append(np.stack([pmiss[:, 0], np.full(len(pmiss), probe_fill, np.uint64), pmiss[:, 1]], 1))
        tri = np.concatenate(parts).astype(np.uint64)
    tri = tri.reshape(-1, 3)
    tri = tri[np.lexsort((tri[:, 2], tri[:, 1], tri[:, 0]))] if len(tri) else tri
    m = tmix(tri[:, 0], tri[:, 1], tri[:, 2]) if len(tri) else np.zeros(0, np.uint64)
    with np.errstate(over="ignore"):
        checks = {"n_matches": len(tri), "sum_r": int(tri[:, 1].sum(dtype=np.uint64)) & M64,
                  "sum_s": int(tri[:, 2].sum(dtype=np.uint64)) & M64,
                  "xor_fold": int(np.bitwise_xor.reduce(m)) if len(m) else 0, "mix_sum": int(m.sum(dtype=np.uint64)) & M64}
    nbm, npm = int(bhit.sum()), int(phit.sum())
    counters = {"n_build_matched": nbm, "n_build_unmatched": len(B) - nbm,
                "n_probe_matched": npm if kind == FULL else 0, "n_probe_unmatched": len(P) - npm if kind == FULL else 0}
    rows = tri[:, :2] if kind in (BSEMI, BANTI) else tri
    return np.ascontiguousarray(rows), checks, counters


# ---------------------------------------------------------------------------------------------
def test_build_kind_entry_is_exported():
    import hashmergejoin_amd as H

    assert hasattr(H.load_library(), "hmj_join_build_kind_u64_device")


def test_build_kind_null_arguments_are_argument_errors():
    import hashmergejoin_amd as H

    L = H.load_library()
    opts = H.BuildJoinOpts()
    opts.struct_size = C.sizeof(H.BuildJoinOpts)
    opts.kind = H.HMJ_FULL_OUTER
    res = H.JoinResult()
    f = L.hmj_join_build_kind_u64_device
    assert f(None, None, 0, None, 0, 0, C.byref(opts), C.byref(res)) == -1  # HMJ_E_ARG: NULL ctx
    assert f(None, None, 0, None, 0, 0, None, C.byref(res)) == -1
    assert f(None, None, 0, None, 0, 0, C.byref(opts), None) == -1
    assert f(None, None, 0, None, 0, 0, None, None) == -1


def test_build_kind_constants_are_mirrored_by_the_binding():
    from hashmergejoin_amd import _lib

    import hashmergejoin_amd as H

    src = open(os.path.join(ROOT, "include", "hmj.h")).read()
    found = dict(re.findall(r"#define (HMJ_BUILD_(?:SEMI|ANTI|OUTER)|HMJ_FULL_OUTER) (\d+)u", src))
    assert found == {"HMJ_BUILD_SEMI": "1", "HMJ_BUILD_ANTI": "2", "HMJ_BUILD_OUTER": "3", "HMJ_FULL_OUTER": "4"}
    for name, v in found.items():
        assert getattr(_lib, name) == int(v), name
        assert getattr(H, name) == int(v), name  # re-exported
        assert name in H.__all__
    assert (BSEMI, BANTI, BOUTER, FULL) == (H.HMJ_BUILD_SEMI, H.HMJ_BUILD_ANTI, H.HMJ_BUILD_OUTER, H.HMJ_FULL_OUTER)


def test_build_join_opts_layout_matches_the_header():
    import hashmergejoin_amd as H

    src = open(os.path.join(ROOT, "include", "hmj.h")).read()
    end = src.index("} hmj_build_join_opts;")
    body = src[src.rindex("typedef struct {", 0, end):end]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"(uint32_t|uint64_t)\s+(\w+);", body)
    assert [n for _, n in fields] == [n for n, _ in H.BuildJoinOpts._fields_]
    off = 0
    for (t, n), (_, ct) in zip(fields, H.BuildJoinOpts._fields_):
        size = 4 if t == "uint32_t" else 8
        off = (off + size - 1) // size * size
        assert getattr(H.BuildJoinOpts, n).offset == off, n
        assert C.sizeof(ct) == size, n
        off += size
    assert C.sizeof(H.BuildJoinOpts) == off == 56


# hand-checked answers for the SURVEY 3.3 inputs (golden.json "iterator_edge", in order) with build_fill 8, probe_fill 7:
# build semi / anti rows (key, rval), build outer and full outer rows (key, rval, sval), and
# (n_build_matched, n_build_unmatched, n_probe_matched, n_probe_unmatched) of the full outer join
_PAIRS7 = [[3, r, s] for r in (1, 2, 3) for s in (7, 8, 9)]
EDGE = [
    dict(semi=[[5, 1], [5, 2], [9, 3]], anti=[], bouter=[[5, 1, 10], [5, 2, 10], [5, 1, 20], [5, 2, 20], [9, 3, 30]],
         full=[[5, 1, 10], [5, 2, 10], [5, 1, 20], [5, 2, 20], [9, 3, 30]], cnt=(3, 0, 3, 0)),
    dict(semi=[[5, 1]], anti=[], bouter=[[5, 1, 10], [5, 1, 20]], full=[[5, 1, 10], [5, 1, 20]], cnt=(1, 0, 2, 0)),
    dict(semi=[[5, 1], [7, 2]], anti=[], bouter=[[5, 1, 10], [5, 1, 20], [7, 2, 30]],
         full=[[5, 1, 10], [5, 1, 20], [7, 2, 30]], cnt=(2, 0, 3, 0)),
    dict(semi=[[5, 1], [5, 2], [7, 3]], anti=[], bouter=[[5, 1, 10], [5, 2, 10], [7, 3, 30]],
         full=[[5, 1, 10], [5, 2, 10], [7, 3, 30]], cnt=(3, 0, 2, 0)),
    dict(semi=[], anti=[[1, 1]], bouter=[[1, 1, 8]], full=[[1, 1, 8], [2, 7, 2]], cnt=(0, 1, 0, 1)),
    dict(semi=[], anti=[], bouter=[], full=[[2, 7, 2]], cnt=(0, 0, 0, 1)),
    dict(semi=[[3, 1], [3, 2], [3, 3]], anti=[], bouter=_PAIRS7, full=_PAIRS7 + [[4, 7, 1]], cnt=(3, 0, 3, 1)),
]


def _sorted(rows, width):
    a = np.array(rows, np.uint64).reshape(-1, width)
    return a[np.lexsort(tuple(a[:, k] for k in reversed(range(width))))] if len(a) else a


def test_expectation_helper_on_the_iterator_edge_inputs():
    with open(os.path.join(ROOT, "tests", "golden", "golden.json")) as f:
        cases = json.load(f)["cases"]["iterator_edge"]
    assert len(cases) == len(EDGE)
    for c, want in zip(cases, EDGE):
        R = np.array(c["R"], np.uint64).reshape(-1, 2)
        S = np.array(c["S"], np.uint64).reshape(-1, 2)
        bm, bu, pm, pu = want["cnt"]
        for kind, name, width in ((BSEMI, "semi", 2), (BANTI, "anti", 2), (BOUTER, "bouter", 3), (FULL, "full", 3)):
            rows, ck, cnt = expect_build_kind(R, S, kind, build_fill=8, probe_fill=7)
            w = _sorted(want[name], width)
            assert rows.tolist() == w.tolist(), (c, name)
            assert ck["n_matches"] == len(w)
            assert ck["sum_r"] == sum(int(x[1]) for x in w)
            assert ck["sum_s"] == (sum(int(x[2]) for x in w) if width == 3 else 0)
            # the checksum convention: tmix over (key, rval, sval) with sval = 0 for build semi / anti rows
            w3 = w if width == 3 else np.concatenate([w, np.zeros((len(w), 1), np.uint64)], 1)
            m = tmix(w3[:, 0], w3[:, 1], w3[:, 2]) if len(w3) else np.zeros(0, np.uint64)
            assert ck["xor_fold"] == (int(np.bitwise_xor.reduce(m)) if len(m) else 0)
            assert ck["mix_sum"] == int(m.sum(dtype=np.uint64)) & M64
            assert (cnt["n_build_matched"], cnt["n_build_unmatched"]) == (bm, bu)
            assert (cnt["n_probe_matched"], cnt["n_probe_unmatched"]) == ((pm, pu) if kind == FULL else (0, 0))
        # build semi and build anti rows partition the build rows
        s, _, _ = expect_build_kind(R, S, BSEMI)
        a, _, _ = expect_build_kind(R, S, BANTI)
        assert _sorted(np.concatenate([s, a]).tolist(), 2).tolist() == _sorted(R.tolist(), 2).tolist()
