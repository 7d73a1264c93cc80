"""CPU-only checks of NULL keys in the multi-column joins (validity bitmaps; include/hmj.h): the ctypes mirrors of
hmj_validity and the grown hmj_cols_kind_opts have the header's layout (g++ prints sizeof / offsetof) while hmj_key_col,
hmj_cols_rel, hmj_cols_join_opts (whose layout test_join_cols_cpu.py pins) and HMJ_ABI_VERSION are what they were, `pack_validity` writes Arrow's bit order at any slice offset, and
`expected_null_kind_rows` -- the pure-Python expectation test_join_cols_nulls_gpu.py imports -- is pinned on a case written
out by hand and keeps SEMI + ANTI = the relation."""
import ctypes as C
import os
import random
import subprocess
import tempfile

import numpy as np
import pytest

from test_join_cols_kinds_cpu import (ALL_KINDS, ANTI, BUILD, BUILD_ANTI, BUILD_OUTER, BUILD_SEMI, COUNT_KEYS, FULL_OUTER, HAND_B,
                                      HAND_BV, HAND_P, HAND_PV, HAND_WIDTHS, INNER, M64, NO_ROW, PROBE, PROBE_OUTER, SEMI, BF, PF,
                                      expected_kind_rows, hand_columns)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMITS_PROBE_NULLS = ((PROBE, ANTI), (PROBE, PROBE_OUTER), (BUILD, FULL_OUTER))
EMITS_BUILD_NULLS = ((BUILD, BUILD_ANTI), (BUILD, BUILD_OUTER), (BUILD, FULL_OUTER))
COUNTS_PROBE = ((PROBE, SEMI), (PROBE, ANTI), (PROBE, PROBE_OUTER), (BUILD, FULL_OUTER))


def expected_null_kind_rows(bcols, bv, pcols, pv, widths, side, kind, bnull=None, pnull=None, bits=0, force_hashed=False,
                            probe_fill=0, build_fill=0):
    """(rows, counts) of a multi-column kind join with NULL keys.  bnull / pnull: bool per row, True = the row has a NULL in
    some key column (None: no NULL on that side); the column values of such a row are never looked at.  The rows that have
    a key are joined by `expected_kind_rows` and their row indices mapped back; the NULL-key rows the kind emits follow
    with key64 0 -- in the HMJ_ORDERED order: behind every other row, the build side's by r_row, then the probe side's by
    s_row.  counts: n_*_unmatched includes the NULL-key rows of the sides the kind counts."""
    nb, np_ = len(bcols[0]), len(pcols[0])
    bnull = np.zeros(nb, bool) if bnull is None else np.asarray(bnull, bool)
    pnull = np.zeros(np_, bool) if pnull is None else np.asarray(pnull, bool)
    keep_b, keep_p = np.flatnonzero(~bnull), np.flatnonzero(~pnull)
    bval = (lambda r: int(r)) if bv is None else (lambda r: int(bv[r]) & M64)
    pval = (lambda s: int(s)) if pv is None else (lambda s: int(pv[s]) & M64)
    sub_b = [np.asarray(c)[keep_b] for c in bcols]
    sub_p = [np.asarray(c)[keep_p] for c in pcols]
    rows, counts = expected_kind_rows(sub_b, [bval(r) for r in keep_b], sub_p, [pval(s) for s in keep_p], widths, side, kind, bits,
                                      force_hashed, probe_fill, build_fill)
    rows = rows.copy()
    semi_anti = kind in (SEMI, ANTI)  # (BUILD_SEMI == SEMI, BUILD_ANTI == ANTI)
    has_r = not (semi_anti and side == PROBE)  # (an absent column reads 0: nothing to map)
    has_s = not (semi_anti and side == BUILD)
    if has_r and len(rows):
        there = rows[:, 1] != NO_ROW
        rows[there, 1] = keep_b[rows[there, 1].astype(np.int64)].astype(np.uint64)
    if has_s and len(rows):
        there = rows[:, 2] != NO_ROW
        rows[there, 2] = keep_p[rows[there, 2].astype(np.int64)].astype(np.uint64)
    tail = []
    if (side, kind) in EMITS_BUILD_NULLS:
        for r in np.flatnonzero(bnull):
            tail.append((0, int(r), NO_ROW, bval(r), build_fill & M64) if has_s else (0, int(r), 0, bval(r), 0))
    if (side, kind) in EMITS_PROBE_NULLS:
        for s in np.flatnonzero(pnull):
            tail.append((0, NO_ROW, int(s), probe_fill & M64, pval(s)) if has_r else (0, 0, int(s), 0, pval(s)))
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

    extra = ('  std::printf("HMJ_ABI_VERSION %d\\nkey_col %zu\\ncols_rel %zu\\n", HMJ_ABI_VERSION, sizeof(hmj_key_col), '
             "sizeof(hmj_cols_rel));\n")
    for name, T in (("hmj_validity", H.Validity), ("hmj_cols_join_opts", H.ColsJoinOpts), ("hmj_cols_kind_opts", H.ColsKindOpts)):
        fields = [n for n, _ in T._fields_]
        got = _layout(name, fields, extra)
        assert int(got["size"]) == C.sizeof(T), name
        for f in fields:
            assert getattr(T, f).offset == int(got[f]), (name, f)
        assert int(got["HMJ_ABI_VERSION"]) == 5
        assert (int(got["key_col"]), int(got["cols_rel"])) == (16, 32) == (C.sizeof(H.KeyCol), C.sizeof(H.ColsRel))
    assert C.sizeof(H.Validity) == 16
    # the new fields follow the last field of hmj_cols_kind_opts as it was (112 bytes), in the order the header gives
    T, old = H.ColsKindOpts, 112
    assert [getattr(T, f).offset - old for f in ("build_validity", "probe_validity", "n_build_null", "n_probe_null")] == [0, 8, 16, 24]
    assert C.sizeof(T) == old + 32
    assert [n for n, _ in T._fields_][-4:] == ["build_validity", "probe_validity", "n_build_null", "n_probe_null"]
    # hmj_cols_join_opts keeps its layout: the inner join of nullable columns is the INNER kind
    assert C.sizeof(H.ColsJoinOpts) == 48 and [n for n, _ in H.ColsJoinOpts._fields_][-1] == "ms_order"
    # the minimum sizes existing callers rely on
    assert H.ColsJoinOpts.force_hashed.offset + 4 == 12 and H.ColsKindOpts.build_fill.offset + 8 == 40


@pytest.mark.parametrize("offset", [0, 1, 7, 8, 13])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65])
def test_pack_validity_round_trips(offset, n):
    import hashmergejoin_amd as H

    rng = np.random.default_rng(100 * offset + n)
    mask = rng.random(n) < 0.6
    t = H.pack_validity(mask, offset)
    raw = t.numpy()
    assert raw.dtype == np.uint8 and len(raw) == (offset + n + 7) // 8
    bits = np.unpackbits(raw, bitorder="little").astype(bool)
    assert np.array_equal(bits[offset:offset + n], mask)
    assert bits[:offset].all() and not bits[offset + n:].any()  # ones in front of the slice, zero padding behind it
    for i in range(n):  # the header's formula
        assert bool((int(raw[(offset + i) >> 3]) >> ((offset + i) & 7)) & 1) == bool(mask[i])


# The hand-written case: test_join_cols_kinds_cpu's relations (widths [2, 1], packed) with build row 4 and probe row 2
# NULL-keyed.  Build row 4's bytes (0x100, 0xFF) equal probe row 4's tuple, probe row 2's bytes (3, 1) equal build rows 0
# and 2: neither pair may appear.  What is left to match: build row 1 = (1, 2) against probe rows 0, 3, 5.
HAND_BNULL = [False, False, False, False, True]
HAND_PNULL = [False, False, True, False, False, False]
NULL_INNER = [[258, 1, 0, 11, 20], [258, 1, 3, 11, 23], [258, 1, 5, 11, 25]]
UN_B = [[512, 3, NO_ROW, 13, BF], [769, 0, NO_ROW, 10, BF], [769, 2, NO_ROW, 12, BF]]
UN_P = [[1285, NO_ROW, 1, PF, 21], [65791, NO_ROW, 4, PF, 24]]
NULL_B, NULL_P = [0, 4, NO_ROW, 14, BF], [0, NO_ROW, 2, PF, 22]
NULL_ROWS = {
    (PROBE, INNER): NULL_INNER,
    (PROBE, SEMI): [[258, 0, 0, 0, 20], [258, 0, 3, 0, 23], [258, 0, 5, 0, 25]],
    (PROBE, ANTI): [[1285, 0, 1, 0, 21], [65791, 0, 4, 0, 24], [0, 0, 2, 0, 22]],
    (PROBE, PROBE_OUTER): NULL_INNER + UN_P + [NULL_P],
    (BUILD, BUILD_SEMI): [[258, 1, 0, 11, 0]],
    (BUILD, BUILD_ANTI): [[512, 3, 0, 13, 0], [769, 0, 0, 10, 0], [769, 2, 0, 12, 0], [0, 4, 0, 14, 0]],
    (BUILD, BUILD_OUTER): NULL_INNER + UN_B + [NULL_B],
    (BUILD, FULL_OUTER): NULL_INNER + UN_B + UN_P + [NULL_B, NULL_P],
}
NULL_COUNTS = {
    (PROBE, INNER): (0, 0, 0, 0), (PROBE, SEMI): (3, 3, 0, 0), (PROBE, ANTI): (3, 3, 0, 0), (PROBE, PROBE_OUTER): (3, 3, 0, 0),
    (BUILD, BUILD_SEMI): (0, 0, 1, 4), (BUILD, BUILD_ANTI): (0, 0, 1, 4), (BUILD, BUILD_OUTER): (0, 0, 1, 4),
    (BUILD, FULL_OUTER): (3, 3, 1, 4),
}


def test_expectation_on_the_hand_written_case():
    bcols, pcols = hand_columns(HAND_B), hand_columns(HAND_P)
    for garbage in (False, True):  # the bytes under the NULL slots change: nothing else does
        if garbage:
            bcols = [c.copy() for c in bcols]
            pcols = [c.copy() for c in pcols]
            bcols[0][4], bcols[1][4], pcols[0][2], pcols[1][2] = 5, 5, 2, 0  # probe row 1's tuple, build row 3's tuple
        for side, kind in ALL_KINDS:
            rows, counts = expected_null_kind_rows(bcols, HAND_BV, pcols, HAND_PV, HAND_WIDTHS, side, kind, HAND_BNULL, HAND_PNULL,
                                                   probe_fill=PF, build_fill=BF)
            assert rows.tolist() == NULL_ROWS[(side, kind)], (side, kind)
            assert tuple(counts[k] for k in COUNT_KEYS) == NULL_COUNTS[(side, kind)], (side, kind)
    # without NULLs it is expected_kind_rows; vals None: the payload of row i is i, for NULL-key rows too
    for side, kind in ALL_KINDS:
        a = expected_null_kind_rows(bcols, HAND_BV, pcols, None, HAND_WIDTHS, side, kind, probe_fill=PF, build_fill=BF)
        b = expected_kind_rows(bcols, HAND_BV, pcols, None, HAND_WIDTHS, side, kind, probe_fill=PF, build_fill=BF)
        assert np.array_equal(a[0], b[0]) and a[1] == b[1]
    rows, _ = expected_null_kind_rows(bcols, None, pcols, None, HAND_WIDTHS, BUILD, FULL_OUTER, HAND_BNULL, HAND_PNULL, probe_fill=PF,
                                      build_fill=BF)
    assert rows[-2:].tolist() == [[0, 4, NO_ROW, 4, BF], [0, NO_ROW, 2, PF, 2]]


def test_semi_and_anti_partition_the_relation():
    from test_join_cols_gpu import columns, draw_pool

    for widths, bits in (([4, 4], 0), ([8, 4, 2], 0), ([8, 4, 2], 4)):
        rng = random.Random(170 + bits + len(widths))
        pool = draw_pool(rng, widths, 80)
        bt = [pool[rng.randrange(60)] for _ in range(150)]
        pt = [pool[20 + rng.randrange(60)] for _ in range(210)]
        bcols, pcols = columns(bt, widths), columns(pt, widths)
        bnull = np.array([rng.random() < 0.3 for _ in bt])
        pnull = np.array([rng.random() < 0.3 for _ in pt])
        E = lambda side, kind: expected_null_kind_rows(bcols, None, pcols, None, widths, side, kind, bnull, pnull, bits, False, 7, 9)
        semi, c1 = E(PROBE, SEMI)
        anti, c2 = E(PROBE, ANTI)
        assert sorted(semi[:, 2].tolist() + anti[:, 2].tolist()) == list(range(len(pt)))
        assert c1 == c2 and (c1["n_probe_matched"], c1["n_probe_unmatched"]) == (len(semi), len(anti))
        assert not pnull[semi[:, 2].astype(np.int64)].any() and set(np.flatnonzero(pnull)) <= set(anti[:, 2].astype(np.int64))
        bsemi, c3 = E(BUILD, BUILD_SEMI)
        banti, c4 = E(BUILD, BUILD_ANTI)
        assert sorted(bsemi[:, 1].tolist() + banti[:, 1].tolist()) == list(range(len(bt)))
        assert c3 == c4 and (c3["n_build_matched"], c3["n_build_unmatched"]) == (len(bsemi), len(banti))
        inner, c0 = E(PROBE, INNER)
        assert set(c0.values()) == {0} and len(inner) > 0
        assert not bnull[inner[:, 1].astype(np.int64)].any() and not pnull[inner[:, 2].astype(np.int64)].any()
        # every kind: the NULL-key rows are the rows with key64 0 at the end, in (r_row, s_row) order, NO_ROW last
        for side, kind in ALL_KINDS:
            rows, counts = E(side, kind)
            n_tail = (int(bnull.sum()) if (side, kind) in EMITS_BUILD_NULLS else 0) + (int(pnull.sum()) if (side, kind) in EMITS_PROBE_NULLS else 0)
            head, tail = rows[:len(rows) - n_tail], rows[len(rows) - n_tail:]
            assert np.all(head[1:, 0] >= head[:-1, 0]) and not tail[:, 0].any()
            if kind == FULL_OUTER:
                assert tail[:, 1].tolist() == [int(r) for r in np.flatnonzero(bnull)] + [NO_ROW] * int(pnull.sum())
                assert tail[:, 2].tolist() == [NO_ROW] * int(bnull.sum()) + [int(s) for s in np.flatnonzero(pnull)]
                assert (counts["n_probe_unmatched"], counts["n_build_unmatched"]) == (len(anti), len(banti))
