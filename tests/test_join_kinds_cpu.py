"""CPU-only checks of the join-kind entry (hmj_join_kind_u64_device): the symbol is exported, bad arguments fail loudly
without a device, the binding mirrors hmj.h, and the numpy expectation the GPU tests compare against gives the
hand-checked answers on the SURVEY 3.3 iterator_edge inputs.  `expect_kind` is imported by test_join_kinds_gpu.py."""
import ctypes as C
import json
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M64 = (1 << 64) - 1
SEMI, ANTI, OUTER = 1, 2, 3


def _mix64(x):
    with np.errstate(over="ignore"):
        x = x ^ (x >> np.uint64(30))
        x = x * np.uint64(0xBF58476D1CE4E5B9)
        x = x ^ (x >> np.uint64(27))
        x = x * np.uint64(0x94D049BB133111EB)
        return x ^ (x >> np.uint64(31))


def tmix(key, rval, sval):
    """hmj_dev.h tmix over uint64 arrays."""
    with np.errstate(over="ignore"):
        t = _mix64(key)
        t = _mix64(t ^ rval)
        return _mix64(t + sval)


def _inner_rows(B, P, first_wins):
    """(key, rval, sval) of the relational inner join, every probe row with all build rows of its key (or the first one in
    build input order), in probe order."""
    order = np.argsort(B[:, 0], kind="stable")
    bk, bv = B[order, 0], B[order, 1]
    lo = np.searchsorted(bk, P[:, 0], "left")
    cnt = np.searchsorted(bk, P[:, 0], "right") - lo
    if first_wins:
        cnt = np.minimum(cnt, 1)
    rep = np.repeat(np.arange(len(P)), cnt)
    within = np.arange(len(rep)) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    return np.stack([P[rep, 0], bv[lo[rep] + within], P[rep, 1]], 1).astype(np.uint64), cnt > 0


def expect_kind(B, P, kind, first_wins=False, fill=0):
    """Expected result of a join kind: (rows sorted as HMJ_ORDERED sorts them, checks dict, n_probe_matched).
    Rows are [n, 2] (key, sval) for SEMI / ANTI and [n, 3] (key, rval, sval) for PROBE_OUTER; checks take rval = 0 for
    SEMI / ANTI rows and rval = fill for unmatched outer rows."""
    B = np.ascontiguousarray(B, np.uint64).reshape(-1, 2)
    P = np.ascontiguousarray(P, np.uint64).reshape(-1, 2)
    hit = np.isin(P[:, 0], B[:, 0])
    if kind in (SEMI, ANTI):
        sel = P[hit] if kind == SEMI else P[~hit]
        tri = np.stack([sel[:, 0], np.zeros(len(sel), np.uint64), sel[:, 1]], 1)
    else:
        inner, _ = _inner_rows(B, P, first_wins)
        miss = P[~hit]
        outer = np.stack([miss[:, 0], np.full(len(miss), fill, np.uint64), miss[:, 1]], 1)
        tri = np.concatenate([inner.reshape(-1, 3), outer.reshape(-1, 3)]).astype(np.uint64)
    tri = tri[np.lexsort((tri[:, 2], tri[:, 1], tri[:, 0]))] if len(tri) else tri.reshape(0, 3)
    m = tmix(tri[:, 0], tri[:, 1], tri[:, 2]) if len(tri) else np.zeros(0, np.uint64)
    with np.errstate(over="ignore"):
        checks = {"n_matches": len(tri), "sum_r": int(tri[:, 1].sum(dtype=np.uint64)) & M64,
                  "sum_s": int(tri[:, 2].sum(dtype=np.uint64)) & M64,
                  "xor_fold": int(np.bitwise_xor.reduce(m)) if len(m) else 0, "mix_sum": int(m.sum(dtype=np.uint64)) & M64}
    rows = tri[:, [0, 2]] if kind in (SEMI, ANTI) else tri
    return np.ascontiguousarray(rows), checks, int(hit.sum())


# ---------------------------------------------------------------------------------------------
def test_join_kind_entry_is_exported():
    import hashmergejoin_amd as H

    assert hasattr(H.load_library(), "hmj_join_kind_u64_device")


def test_join_kind_null_ctx_is_an_argument_error():
    import hashmergejoin_amd as H

    L = H.load_library()
    opts = H.JoinOpts()
    opts.struct_size = C.sizeof(H.JoinOpts)
    opts.kind = H.HMJ_JOIN_SEMI
    res = H.JoinResult()
    assert L.hmj_join_kind_u64_device(None, None, 0, None, 0, 0, C.byref(opts), C.byref(res)) == -1  # HMJ_E_ARG
    assert L.hmj_join_kind_u64_device(None, None, 0, None, 0, 0, None, None) == -1


def test_join_kind_constants_are_mirrored_by_the_binding():
    from hashmergejoin_amd import _lib

    import hashmergejoin_amd as H

    src = open(os.path.join(ROOT, "include", "hmj.h")).read()
    found = dict(re.findall(r"#define (HMJ_JOIN_\w+) (\d+)u", src))
    assert set(found) == {"HMJ_JOIN_INNER", "HMJ_JOIN_SEMI", "HMJ_JOIN_ANTI", "HMJ_JOIN_PROBE_OUTER"}
    for name, v in found.items():
        assert getattr(_lib, name) == int(v), name
        assert getattr(H, name) == int(v), name  # re-exported
    assert len(set(found.values())) == 4


def test_join_opts_layout_matches_the_header():
    import hashmergejoin_amd as H

    src = open(os.path.join(ROOT, "include", "hmj.h")).read()
    end = src.index("} hmj_join_opts;")
    body = src[src.rindex("typedef struct {", 0, end):end]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"(uint32_t|uint64_t)\s+(\w+);", body)
    assert [n for _, n in fields] == [n for n, _ in H.JoinOpts._fields_]
    off = 0
    for (t, n), (_, ct) in zip(fields, H.JoinOpts._fields_):
        size = 4 if t == "uint32_t" else 8
        off = (off + size - 1) // size * size
        assert getattr(H.JoinOpts, n).offset == off, n
        assert C.sizeof(ct) == size, n
        off += size
    assert C.sizeof(H.JoinOpts) == off == 32


# hand-checked answers for the SURVEY 3.3 inputs (golden.json "iterator_edge", in order): semi / anti rows (key, sval),
# outer rows (key, rval, sval) with fill 7, and the same under first-wins
EDGE = [
    dict(semi=[[5, 10], [5, 20], [9, 30]], anti=[],
         outer=[[5, 1, 10], [5, 2, 10], [5, 1, 20], [5, 2, 20], [9, 3, 30]], first=[[5, 1, 10], [5, 1, 20], [9, 3, 30]]),
    dict(semi=[[5, 10], [5, 20]], anti=[], outer=[[5, 1, 10], [5, 1, 20]], first=[[5, 1, 10], [5, 1, 20]]),
    dict(semi=[[5, 10], [5, 20], [7, 30]], anti=[], outer=[[5, 1, 10], [5, 1, 20], [7, 2, 30]],
         first=[[5, 1, 10], [5, 1, 20], [7, 2, 30]]),
    dict(semi=[[5, 10], [7, 30]], anti=[], outer=[[5, 1, 10], [5, 2, 10], [7, 3, 30]], first=[[5, 1, 10], [7, 3, 30]]),
    dict(semi=[], anti=[[2, 2]], outer=[[2, 7, 2]], first=[[2, 7, 2]]),
    dict(semi=[], anti=[[2, 2]], outer=[[2, 7, 2]], first=[[2, 7, 2]]),
    dict(semi=[[3, 7], [3, 8], [3, 9]], anti=[[4, 1]],
         outer=[[3, 1, 7], [3, 2, 7], [3, 3, 7], [3, 1, 8], [3, 2, 8], [3, 3, 8], [3, 1, 9], [3, 2, 9], [3, 3, 9], [4, 7, 1]],
         first=[[3, 1, 7], [3, 1, 8], [3, 1, 9], [4, 7, 1]]),
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
        rows, ck, matched = expect_kind(R, S, SEMI)
        assert rows.tolist() == _sorted(want["semi"], 2).tolist() and ck["n_matches"] == len(want["semi"]) == matched
        assert ck["sum_r"] == 0 and ck["sum_s"] == sum(s for _, s in want["semi"])
        rows, ck, matched = expect_kind(R, S, ANTI)
        assert rows.tolist() == _sorted(want["anti"], 2).tolist() and matched == len(S) - len(want["anti"])
        rows, ck, _ = expect_kind(R, S, OUTER, fill=7)
        assert rows.tolist() == _sorted(want["outer"], 3).tolist()
        assert ck["sum_r"] == sum(r for _, r, _ in want["outer"]) and ck["n_matches"] == len(want["outer"])
        rows, ck, _ = expect_kind(R, S, OUTER, first_wins=True, fill=7)
        assert rows.tolist() == _sorted(want["first"], 3).tolist()
        # the checksum convention: tmix over (key, rval, sval) with rval = 0 for semi rows
        _, ck, _ = expect_kind(R, S, SEMI)
        sr = _sorted(want["semi"], 2)
        m = tmix(sr[:, 0], np.zeros(len(sr), np.uint64), sr[:, 1]) if len(sr) else np.zeros(0, np.uint64)
        assert ck["xor_fold"] == (int(np.bitwise_xor.reduce(m)) if len(m) else 0)
