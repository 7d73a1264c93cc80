"""CPU-only checks of NULL keys in the string-key joins (validity bitmaps on hmj_join_kind_str_device; include/hmj.h): the
ctypes mirror of the grown hmj_str_kind_opts has the header's layout (g++ prints sizeof / offsetof) while hmj_validity,
hmj_str_rel, hmj_str_join_opts, hmj_str_result and HMJ_ABI_VERSION are what they were, and `expected_null_str_kind_rows`
-- the pure-Python expectation test_join_str_nulls_gpu.py imports -- is pinned on a case written out by hand (a valid b""
on both sides next to zero-length NULL slots) and keeps SEMI + ANTI = the relation."""
import ctypes as C
import os
import random
import subprocess
import tempfile

import numpy as np

from test_join_str_cpu import M64, str_hash
from test_join_str_kinds_cpu import (ALL_KINDS, ANTI, BUILD, BUILD_ANTI, BUILD_OUTER, BUILD_SEMI, FULL_OUTER, INNER, NO_ROW, PROBE,
                                     PROBE_OUTER, SEMI, kind_brute)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNT_KEYS = ("n_probe_matched", "n_probe_unmatched", "n_build_matched", "n_build_unmatched")
EMITS_PROBE_NULLS = ((PROBE, ANTI), (PROBE, PROBE_OUTER), (BUILD, FULL_OUTER))
EMITS_BUILD_NULLS = ((BUILD, BUILD_ANTI), (BUILD, BUILD_OUTER), (BUILD, FULL_OUTER))
COUNTS_PROBE = ((PROBE, SEMI), (PROBE, ANTI), (PROBE, PROBE_OUTER), (BUILD, FULL_OUTER))


def expected_null_str_kind_rows(bk, bv, pk, pv, side, kind, bnull=None, pnull=None, bits=0, probe_fill=0, build_fill=0):
    """(rows, counts) of a string kind join with NULL keys.  bnull / pnull: bool per row, True = the row's key is NULL
    (None: no NULL on that side); the key bytes of such a row are never looked at.  The rows that have a key are joined by
    `kind_brute` and their row indices mapped back; the NULL-key rows the kind emits follow with hash 0 -- in the
    HMJ_ORDERED order: behind every other row, the build side's by r_row, then the probe side's by s_row.  Absent row
    columns read HMJ_STR_NO_ROW and absent value columns 0, as Executor.str_kind_rows_to_numpy reads them.  counts:
    n_*_unmatched includes the NULL-key rows of the sides the kind counts."""
    nb, np_ = len(bk), len(pk)
    bnull = np.zeros(nb, bool) if bnull is None else np.asarray(bnull, bool)
    pnull = np.zeros(np_, bool) if pnull is None else np.asarray(pnull, bool)
    keep_b, keep_p = np.flatnonzero(~bnull), np.flatnonzero(~pnull)
    rows, counts = kind_brute([bk[r] for r in keep_b], [bv[r] for r in keep_b], [pk[s] for s in keep_p], [pv[s] for s in keep_p],
                              side, kind, bits, probe_fill, build_fill)
    rows = rows.copy()
    for col, keep in ((1, keep_b), (2, keep_p)):
        there = rows[:, col] != NO_ROW
        rows[there, col] = keep[rows[there, col].astype(np.int64)].astype(np.uint64)
    semi_anti = kind in (SEMI, ANTI)  # (BUILD_SEMI == SEMI, BUILD_ANTI == ANTI)
    tail = []
    if (side, kind) in EMITS_BUILD_NULLS:
        for r in np.flatnonzero(bnull):
            tail.append((0, int(r), NO_ROW, int(bv[r]) & M64, 0 if semi_anti else build_fill & M64))
    if (side, kind) in EMITS_PROBE_NULLS:
        for s in np.flatnonzero(pnull):
            tail.append((0, NO_ROW, int(s), 0 if semi_anti else probe_fill & M64, int(pv[s]) & M64))
    if tail:
        rows = np.concatenate([rows, np.array(tail, np.uint64).reshape(-1, 5)])
    counts = dict(counts)
    if (side, kind) in COUNTS_PROBE:
        counts["n_probe_unmatched"] += int(pnull.sum())
    if side == BUILD:
        counts["n_build_unmatched"] += int(bnull.sum())
    return rows, counts


def _layout(struct, fields, extra=""):
    src = "#include <cstddef>\n#include <cstdio>\n#include \"hmj.h\"\nint main() {\n"
    src += '  std::printf("size %%zu\\n", sizeof(%s));\n' % struct
    for f in fields:
        src += '  std::printf("%s %%zu\\n", offsetof(%s, %s));\n' % (f, struct, f)
    src += extra + "  return 0;\n}\n"
    with tempfile.TemporaryDirectory() as d:
        cc, exe = os.path.join(d, "layout.cc"), os.path.join(d, "layout")
        open(cc, "w").write(src)
        subprocess.check_call(["g++", "-std=c++11", "-I", os.path.join(ROOT, "include"), cc, "-o", exe])
        return dict(line.split() for line in subprocess.check_output([exe]).decode().splitlines())


def test_layouts_match_the_header():
    import hashmergejoin_amd as H

    extra = ('  std::printf("HMJ_ABI_VERSION %d\\nstr_rel %zu\\nstr_join_opts %zu\\nstr_result %zu\\nvalidity %zu\\n", HMJ_ABI_VERSION, '
             "sizeof(hmj_str_rel), sizeof(hmj_str_join_opts), sizeof(hmj_str_result), sizeof(hmj_validity));\n")
    for name, T in (("hmj_validity", H.Validity), ("hmj_str_kind_opts", H.StrKindOpts), ("hmj_str_join_opts", H.StrJoinOpts),
                    ("hmj_str_rel", H.StrRel), ("hmj_str_result", H.StrResult)):
        fields = [n for n, _ in T._fields_]
        got = _layout(name, fields, extra)
        assert int(got["size"]) == C.sizeof(T), name
        for f in fields:
            assert getattr(T, f).offset == int(got[f]), (name, f)
    assert int(got["HMJ_ABI_VERSION"]) == 5
    # what the string structs and hmj_validity were before hmj_str_kind_opts grew
    assert (int(got["str_rel"]), int(got["str_join_opts"]), int(got["str_result"]), int(got["validity"])) == (32, 40, 88, 16)
    assert (C.sizeof(H.StrRel), C.sizeof(H.StrJoinOpts), C.sizeof(H.StrResult), C.sizeof(H.Validity)) == (32, 40, 88, 16)
    assert [n for n, _ in H.Validity._fields_] == ["bits", "bit_offset"] and H.Validity.bit_offset.offset == 8
    # the new fields follow the last field of hmj_str_kind_opts as it was (104 bytes), in the order the header gives; the
    # two hmj_validity are embedded by value
    T, old = H.StrKindOpts, 104
    assert [getattr(T, f).offset - old for f in ("build_validity", "probe_validity", "n_build_null", "n_probe_null")] == [0, 16, 32, 40]
    assert C.sizeof(T) == old + 48
    assert [n for n, _ in T._fields_][-4:] == ["build_validity", "probe_validity", "n_build_null", "n_probe_null"]
    assert dict(T._fields_)["build_validity"] is H.Validity and dict(T._fields_)["probe_validity"] is H.Validity
    assert T.ms_order.offset + 4 <= old and T.build_fill.offset + 8 == 32  # the old struct's end; the minimum callers rely on
    assert [n for n, _ in H.StrJoinOpts._fields_][-1] == "ms_order"  # hmj_str_join_opts carries no bitmap


# The hand-written case.  Hashes (std::hash<std::string>, 64 bits): "zz" < "cd" < "ab" < "".
#   build  0 "ab"   1 ""     2 "cd"   3 NULL (length 0)      4 NULL (bytes "ab": probe rows 0 and 5, were they read)
#   probe  0 "ab"   1 ""     2 NULL (length 0)   3 "zz"      4 NULL (bytes "cd": build row 2, were they read)   5 "ab"
# What matches: build 0 with probe 0 and 5, and the two valid empty strings (build 1, probe 1).  Build row 2 and probe row 3
# have no partner; the NULL slots match nothing, the zero-length ones not even the valid b"".
H_AB, H_E, H_CD, H_ZZ = 0x4C4DA6CD289C737B, 0x553E93901E462A6E, 0x3B959DDB2A56F437, 0x0FF4C37181F3852D
HAND_BK, HAND_BV = [b"ab", b"", b"cd", b"", b"ab"], [10, 11, 12, 13, 14]
HAND_PK, HAND_PV = [b"ab", b"", b"", b"zz", b"cd", b"ab"], [20, 21, 22, 23, 24, 25]
HAND_BNULL = [False, False, False, True, True]
HAND_PNULL = [False, False, True, False, True, False]
PF, BF = 0x77, 2 ** 64 - 3
N = NO_ROW
NULL_INNER = [[H_AB, 0, 0, 10, 20], [H_AB, 0, 5, 10, 25], [H_E, 1, 1, 11, 21]]
NULL_ROWS = {
    (PROBE, INNER): NULL_INNER,
    (PROBE, SEMI): [[H_AB, N, 0, 0, 20], [H_AB, N, 5, 0, 25], [H_E, N, 1, 0, 21]],
    (PROBE, ANTI): [[H_ZZ, N, 3, 0, 23], [0, N, 2, 0, 22], [0, N, 4, 0, 24]],
    (PROBE, PROBE_OUTER): [[H_ZZ, N, 3, PF, 23]] + NULL_INNER + [[0, N, 2, PF, 22], [0, N, 4, PF, 24]],
    (BUILD, BUILD_SEMI): [[H_AB, 0, N, 10, 0], [H_E, 1, N, 11, 0]],
    (BUILD, BUILD_ANTI): [[H_CD, 2, N, 12, 0], [0, 3, N, 13, 0], [0, 4, N, 14, 0]],
    (BUILD, BUILD_OUTER): [[H_CD, 2, N, 12, BF]] + NULL_INNER + [[0, 3, N, 13, BF], [0, 4, N, 14, BF]],
    (BUILD, FULL_OUTER): [[H_ZZ, N, 3, PF, 23], [H_CD, 2, N, 12, BF]] + NULL_INNER
                         + [[0, 3, N, 13, BF], [0, 4, N, 14, BF], [0, N, 2, PF, 22], [0, N, 4, PF, 24]],
}
NULL_COUNTS = {  # (n_probe_matched, n_probe_unmatched, n_build_matched, n_build_unmatched)
    (PROBE, INNER): (0, 0, 0, 0), (PROBE, SEMI): (3, 3, 0, 0), (PROBE, ANTI): (3, 3, 0, 0), (PROBE, PROBE_OUTER): (3, 3, 0, 0),
    (BUILD, BUILD_SEMI): (0, 0, 2, 3), (BUILD, BUILD_ANTI): (0, 0, 2, 3), (BUILD, BUILD_OUTER): (0, 0, 2, 3),
    (BUILD, FULL_OUTER): (3, 3, 2, 3),
}


def test_expectation_on_the_hand_written_case():
    assert [str_hash(k) for k in (b"ab", b"", b"cd", b"zz")] == [H_AB, H_E, H_CD, H_ZZ] and H_ZZ < H_CD < H_AB < H_E
    bk, pk = list(HAND_BK), list(HAND_PK)
    for garbage in (False, True):  # the bytes (and lengths) under the NULL slots change: nothing else does
        if garbage:
            bk[3], bk[4], pk[2], pk[4] = b"zz", b"", b"cd", b"\x00" * 9
        for side, kind in ALL_KINDS:
            rows, counts = expected_null_str_kind_rows(bk, HAND_BV, pk, HAND_PV, side, kind, HAND_BNULL, HAND_PNULL, 0, PF, BF)
            assert rows.tolist() == NULL_ROWS[(side, kind)], (side, kind)
            assert tuple(counts[k] for k in COUNT_KEYS) == NULL_COUNTS[(side, kind)], (side, kind)
    # without the bitmaps the zero-length slots are empty strings and the bytes match: other rows
    plain, _ = expected_null_str_kind_rows(HAND_BK, HAND_BV, HAND_PK, HAND_PV, PROBE, INNER)
    assert len(plain) == 2 * 2 + 2 * 2 + 1  # "ab" x "ab", "" x "", "cd" x "cd"
    # without NULLs it is kind_brute
    for side, kind in ALL_KINDS:
        a = expected_null_str_kind_rows(HAND_BK, HAND_BV, HAND_PK, HAND_PV, side, kind, None, None, 4, PF, BF)
        b = kind_brute(HAND_BK, HAND_BV, HAND_PK, HAND_PV, side, kind, 4, PF, BF)
        assert np.array_equal(a[0], b[0]) and a[1] == b[1]
    # hash_bits folds the hashes of the rows that have a key; a NULL-key row keeps hash 0
    rows, _ = expected_null_str_kind_rows(HAND_BK, HAND_BV, HAND_PK, HAND_PV, BUILD, FULL_OUTER, HAND_BNULL, HAND_PNULL, 4, PF, BF)
    assert rows[:, 0].tolist() == [0, 3, 4, 4, 5, 0, 0, 0, 0] and rows[0].tolist() == [0, N, 3, PF, 23]  # ("zz" folds to 0 too)


def test_semi_and_anti_partition_the_relation():
    from test_join_str_gpu import _dup_relations

    for bits in (0, 4):
        rng = random.Random(170 + bits)
        bk, bv, pk, pv = _dup_relations(rng, 60, 6)
        bk, pk = bk + [b""] * 3, pk + [b""] * 2
        bv, pv = bv + [1, 2, 3], pv + [4, 5]
        bnull = np.array([rng.random() < 0.3 for _ in bk])
        pnull = np.array([rng.random() < 0.3 for _ in pk])
        E = lambda side, kind: expected_null_str_kind_rows(bk, bv, pk, pv, side, kind, bnull, pnull, bits, 7, 9)
        semi, c1 = E(PROBE, SEMI)
        anti, c2 = E(PROBE, ANTI)
        assert sorted(semi[:, 2].tolist() + anti[:, 2].tolist()) == list(range(len(pk)))
        assert c1 == c2 and (c1["n_probe_matched"], c1["n_probe_unmatched"]) == (len(semi), len(anti))
        assert not pnull[semi[:, 2].astype(np.int64)].any() and set(np.flatnonzero(pnull)) <= set(anti[:, 2].astype(np.int64))
        bsemi, c3 = E(BUILD, BUILD_SEMI)
        banti, c4 = E(BUILD, BUILD_ANTI)
        assert sorted(bsemi[:, 1].tolist() + banti[:, 1].tolist()) == list(range(len(bk)))
        assert c3 == c4 and (c3["n_build_matched"], c3["n_build_unmatched"]) == (len(bsemi), len(banti))
        assert not bnull[bsemi[:, 1].astype(np.int64)].any()
        inner, c0 = E(PROBE, INNER)
        assert set(c0.values()) == {0} and len(inner) > 0
        assert not bnull[inner[:, 1].astype(np.int64)].any() and not pnull[inner[:, 2].astype(np.int64)].any()
        # every kind: the NULL-key rows are the rows with hash 0 at the end, in (r_row, s_row) order, NO_ROW last
        for side, kind in ALL_KINDS:
            rows, counts = E(side, kind)
            n_tail = (int(bnull.sum()) if (side, kind) in EMITS_BUILD_NULLS else 0) + (int(pnull.sum()) if (side, kind) in EMITS_PROBE_NULLS else 0)
            head, tail = rows[:len(rows) - n_tail], rows[len(rows) - n_tail:]
            assert np.all(head[1:, 0] >= head[:-1, 0]) and not tail[:, 0].any()
            if kind == FULL_OUTER and side == BUILD:
                assert tail[:, 1].tolist() == [int(r) for r in np.flatnonzero(bnull)] + [NO_ROW] * int(pnull.sum())
                assert tail[:, 2].tolist() == [NO_ROW] * int(bnull.sum()) + [int(s) for s in np.flatnonzero(pnull)]
                assert (counts["n_probe_unmatched"], counts["n_build_unmatched"]) == (len(anti), len(banti))
