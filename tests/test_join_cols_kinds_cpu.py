"""CPU-only checks of the multi-column join kinds (hmj_join_kind_cols_device): the symbol is exported, a NULL ctx fails
without a device, the ctypes mirror has the header's layout (g++ prints sizeof / offsetof), and `expected_kind_rows` -- the
pure-Python expectation test_join_cols_kinds_gpu.py imports -- is pinned on a case written out by hand and satisfies the
identities between the kinds."""
import ctypes as C
import os
import random
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M64 = (1 << 64) - 1
NO_ROW = M64
HMJ_E_ARG = -1
PROBE, BUILD = 0, 1
INNER, SEMI, ANTI, PROBE_OUTER = 0, 1, 2, 3
BUILD_SEMI, BUILD_ANTI, BUILD_OUTER, FULL_OUTER = 1, 2, 3, 4
ALL_KINDS = [(PROBE, INNER), (PROBE, SEMI), (PROBE, ANTI), (PROBE, PROBE_OUTER),
             (BUILD, BUILD_SEMI), (BUILD, BUILD_ANTI), (BUILD, BUILD_OUTER), (BUILD, FULL_OUTER)]
COUNT_KEYS = ("n_probe_matched", "n_probe_unmatched", "n_build_matched", "n_build_unmatched")


def expected_kind_rows(bcols, bv, pcols, pv, widths, side, kind, bits=0, force_hashed=False, probe_fill=0, build_fill=0):
    """(rows, counts) of a multi-column kind join.  rows: [n, 5] uint64 (key64, r_row, s_row, rval, sval) in the HMJ_ORDERED
    order -- (key64, tuple as unsigned columns, r_row, s_row), NO_ROW last --, with 0 in the columns the kind does not
    produce, as Executor.cols_kind_rows_to_numpy reads them.  counts: the four hmj_kind_counts fields.  vals None: the
    payload of row i is i."""
    import hashmergejoin_amd as H

    nb, np_ = len(bcols[0]), len(pcols[0])
    kb = [int(x) for x in H.cols_key64(bcols, widths, bits, force_hashed)] if nb else []
    kp = [int(x) for x in H.cols_key64(pcols, widths, bits, force_hashed)] if np_ else []
    tb = list(zip(*[[int(x) for x in c] for c in bcols])) if nb else []
    tp = list(zip(*[[int(x) for x in c] for c in pcols])) if np_ else []
    bval = (lambda r: r) if bv is None else (lambda r: int(bv[r]) & M64)
    pval = (lambda s: s) if pv is None else (lambda s: int(pv[s]) & M64)
    b_by, p_by = {}, {}
    for r, t in enumerate(tb):
        b_by.setdefault(t, []).append(r)
    for s, t in enumerate(tp):
        p_by.setdefault(t, []).append(s)
    # (key64, tuple, r, s, rval, sval); NO_ROW = 2^64 - 1 sorts last among row indices
    pair_rows = [(kp[s], t, r, s, bval(r), pval(s)) for s, t in enumerate(tp) for r in b_by.get(t, ())]
    p_match = [t in b_by for t in tp]
    b_match = [t in p_by for t in tb]
    probe_rows = lambda sel, fill: [(kp[s], t, NO_ROW, s, fill, pval(s)) for s, t in enumerate(tp) if p_match[s] == sel]
    build_rows = lambda sel, fill: [(kb[r], t, r, NO_ROW, bval(r), fill) for r, t in enumerate(tb) if b_match[r] == sel]
    counts = dict.fromkeys(COUNT_KEYS, 0)
    probe_counts = {"n_probe_matched": sum(p_match), "n_probe_unmatched": np_ - sum(p_match)}
    build_counts = {"n_build_matched": sum(b_match), "n_build_unmatched": nb - sum(b_match)}
    absent = ()
    if side == PROBE:
        if kind == INNER:
            rows = pair_rows
        elif kind in (SEMI, ANTI):
            rows, absent = probe_rows(kind == SEMI, 0), (1, 3)
            counts.update(probe_counts)
        elif kind == PROBE_OUTER:
            rows = pair_rows + probe_rows(False, probe_fill & M64)
            counts.update(probe_counts)
        else:
            raise ValueError(kind)
    elif side == BUILD:
        counts.update(build_counts)
        if kind in (BUILD_SEMI, BUILD_ANTI):
            rows, absent = build_rows(kind == BUILD_SEMI, 0), (2, 4)
        elif kind == BUILD_OUTER:
            rows = pair_rows + build_rows(False, build_fill & M64)
        elif kind == FULL_OUTER:
            rows = pair_rows + probe_rows(False, probe_fill & M64) + build_rows(False, build_fill & M64)
            counts.update(probe_counts)
        else:
            raise ValueError(kind)
    else:
        raise ValueError(side)
    rows.sort(key=lambda t: t[:4])
    out = np.array([(k, r, s, rv, sv) for k, _, r, s, rv, sv in rows], np.uint64).reshape(-1, 5)
    for c in absent:
        out[:, c] = 0
    return out, counts


def key_collisions(bcols, pcols, widths, bits=0, force_hashed=False):
    """Pairs (build row, probe row) of equal key64 whose tuples differ: n_collisions of the outer kinds."""
    import hashmergejoin_amd as H

    if not len(bcols[0]) or not len(pcols[0]):
        return 0
    kb = [int(x) for x in H.cols_key64(bcols, widths, bits, force_hashed)]
    kp = [int(x) for x in H.cols_key64(pcols, widths, bits, force_hashed)]
    tb = list(zip(*[[int(x) for x in c] for c in bcols]))
    tp = list(zip(*[[int(x) for x in c] for c in pcols]))
    by_key, by_tuple = {}, {}
    for k, t in zip(kb, tb):
        by_key[k] = by_key.get(k, 0) + 1
        by_tuple[t] = by_tuple.get(t, 0) + 1
    return sum(by_key.get(k, 0) - by_tuple.get(t, 0) for k, t in zip(kp, tp))


def kind_checks(rows):
    """n_matches, sums and HMJ_CHECKSUM's folds over result rows (value columns as expected_kind_rows writes them)."""
    from test_join_kinds_cpu import tmix

    if not len(rows):
        return {"n_matches": 0, "sum_r": 0, "sum_s": 0, "xor_fold": 0, "mix_sum": 0}
    m = tmix(rows[:, 0], rows[:, 3], rows[:, 4])
    with np.errstate(over="ignore"):
        return {"n_matches": len(rows), "sum_r": int(rows[:, 3].sum(dtype=np.uint64)), "sum_s": int(rows[:, 4].sum(dtype=np.uint64)),
                "xor_fold": int(np.bitwise_xor.reduce(m)), "mix_sum": int(m.sum(dtype=np.uint64))}


# ---------------------------------------------------------------------------------------------
def test_cols_kind_entry_is_exported():
    import hashmergejoin_amd as H

    assert hasattr(H.load_library(), "hmj_join_kind_cols_device")
    assert H.HMJ_COLS_NO_ROW == 2 ** 64 - 1 == NO_ROW


def test_cols_kind_null_ctx_is_an_argument_error():
    import hashmergejoin_amd as H

    L = H.load_library()
    col = (H.KeyCol * 1)()
    col[0].width = 4
    rel = H.ColsRel()
    rel.cols, rel.n_cols = col, 1
    opts = H.ColsKindOpts()
    opts.struct_size = C.sizeof(H.ColsKindOpts)
    opts.kind = SEMI
    res = H.ColsResult()
    assert L.hmj_join_kind_cols_device(None, C.byref(rel), C.byref(rel), 0, C.byref(opts), C.byref(res)) == HMJ_E_ARG
    assert L.hmj_join_kind_cols_device(None, C.byref(rel), C.byref(rel), 0, None, C.byref(res)) == HMJ_E_ARG
    assert L.hmj_join_kind_cols_device(None, None, None, 0, None, None) == HMJ_E_ARG


def test_cols_kind_opts_match_the_header():
    import hashmergejoin_amd as H

    fields = [n for n, _ in H.ColsKindOpts._fields_]
    src = "#include <cstddef>\n#include <cstdio>\n#include <cinttypes>\n#include \"hmj.h\"\nint main() {\n"
    src += '  std::printf("size %zu\\n", sizeof(hmj_cols_kind_opts));\n'
    for f in fields:
        src += '  std::printf("%s %%zu\\n", offsetof(hmj_cols_kind_opts, %s));\n' % (f, f)
    src += '  std::printf("counts_size %zu\\nHMJ_ABI_VERSION %d\\n", sizeof(hmj_kind_counts), HMJ_ABI_VERSION);\n'
    src += '  std::printf("HMJ_COLS_NO_ROW %" PRIu64 "\\n", (uint64_t)HMJ_COLS_NO_ROW);\n  return 0;\n}\n'
    with tempfile.TemporaryDirectory() as d:
        cc, exe = os.path.join(d, "layout.cc"), os.path.join(d, "layout")
        open(cc, "w").write(src)
        subprocess.check_call(["g++", "-std=c++11", "-I", os.path.join(ROOT, "include"), cc, "-o", exe])
        got = dict(line.split() for line in subprocess.check_output([exe]).decode().splitlines())
    assert int(got["size"]) == C.sizeof(H.ColsKindOpts)
    assert int(got["counts_size"]) == C.sizeof(H.KindCounts)
    assert int(got["HMJ_ABI_VERSION"]) == 5  # no existing struct changed; the new one is size-versioned
    assert int(got["HMJ_COLS_NO_ROW"]) == H.HMJ_COLS_NO_ROW
    for f in fields:
        assert getattr(H.ColsKindOpts, f).offset == int(got[f]), f
    # the in fields end with build_fill: what struct_size must at least cover
    assert H.ColsKindOpts.build_fill.offset + 8 == 40 == H.ColsKindOpts.counts.offset


# The hand-written case: widths [2, 1] (packed: key64 = (a << 8) | b).  Build rows hold (3,1) twice and the build-only (2,0);
# probe rows hold (1,2) three times and the probe-only (5,5).
HAND_WIDTHS = [2, 1]
HAND_B = [(3, 1), (1, 2), (3, 1), (2, 0), (0x100, 0xFF)]
HAND_P = [(1, 2), (5, 5), (3, 1), (1, 2), (0x100, 0xFF), (1, 2)]
HAND_BV = [10, 11, 12, 13, 14]
HAND_PV = [20, 21, 22, 23, 24, 25]
PF, BF = 0xF1, 0xF2
HAND_INNER = [[258, 1, 0, 11, 20], [258, 1, 3, 11, 23], [258, 1, 5, 11, 25], [769, 0, 2, 10, 22], [769, 2, 2, 12, 22],
              [65791, 4, 4, 14, 24]]
HAND_ROWS = {
    (PROBE, INNER): HAND_INNER,
    (PROBE, SEMI): [[258, 0, 0, 0, 20], [258, 0, 3, 0, 23], [258, 0, 5, 0, 25], [769, 0, 2, 0, 22], [65791, 0, 4, 0, 24]],
    (PROBE, ANTI): [[1285, 0, 1, 0, 21]],
    (PROBE, PROBE_OUTER): HAND_INNER[:5] + [[1285, NO_ROW, 1, PF, 21]] + HAND_INNER[5:],
    (BUILD, BUILD_SEMI): [[258, 1, 0, 11, 0], [769, 0, 0, 10, 0], [769, 2, 0, 12, 0], [65791, 4, 0, 14, 0]],
    (BUILD, BUILD_ANTI): [[512, 3, 0, 13, 0]],
    (BUILD, BUILD_OUTER): HAND_INNER[:3] + [[512, 3, NO_ROW, 13, BF]] + HAND_INNER[3:],
    (BUILD, FULL_OUTER): HAND_INNER[:3] + [[512, 3, NO_ROW, 13, BF]] + HAND_INNER[3:5] + [[1285, NO_ROW, 1, PF, 21]] + HAND_INNER[5:],
}
HAND_COUNTS = {
    (PROBE, INNER): (0, 0, 0, 0), (PROBE, SEMI): (5, 1, 0, 0), (PROBE, ANTI): (5, 1, 0, 0), (PROBE, PROBE_OUTER): (5, 1, 0, 0),
    (BUILD, BUILD_SEMI): (0, 0, 4, 1), (BUILD, BUILD_ANTI): (0, 0, 4, 1), (BUILD, BUILD_OUTER): (0, 0, 4, 1),
    (BUILD, FULL_OUTER): (5, 1, 4, 1),
}


def hand_columns(tuples):
    return [np.array([t[c] for t in tuples], "u%d" % w) for c, w in enumerate(HAND_WIDTHS)]


def test_expectation_on_the_hand_written_case():
    bcols, pcols = hand_columns(HAND_B), hand_columns(HAND_P)
    for side, kind in ALL_KINDS:
        rows, counts = expected_kind_rows(bcols, HAND_BV, pcols, HAND_PV, HAND_WIDTHS, side, kind, probe_fill=PF, build_fill=BF)
        assert rows.tolist() == HAND_ROWS[(side, kind)], (side, kind)
        assert tuple(counts[k] for k in COUNT_KEYS) == HAND_COUNTS[(side, kind)], (side, kind)
    # vals None: the payload of row i is i, for unmatched rows too
    rows, _ = expected_kind_rows(bcols, None, pcols, HAND_PV, HAND_WIDTHS, BUILD, FULL_OUTER, probe_fill=PF, build_fill=BF)
    assert rows.tolist() == [[k, r, s, r if r != NO_ROW else PF, sv] for k, r, s, _, sv in HAND_ROWS[(BUILD, FULL_OUTER)]]
    assert key_collisions(bcols, pcols, HAND_WIDTHS) == 0
    assert kind_checks(np.array(HAND_ROWS[(PROBE, ANTI)], np.uint64))["sum_s"] == 21


def test_expectation_identities():
    from test_join_cols_gpu import brute, columns, draw_pool
    import hashmergejoin_amd as H

    for widths, bits in (([4, 4], 0), ([8, 4, 2], 0), ([8, 4, 2], 6)):
        rng = random.Random(70 + bits + len(widths))
        pool = draw_pool(rng, widths, 160)
        bt = [pool[rng.randrange(120)] for _ in range(200)]          # tuples 0..119; 120..159 are probe-only
        pt = [pool[40 + rng.randrange(120)] for _ in range(260)]     # tuples 40..159; 0..39 are build-only
        bcols, pcols = columns(bt, widths), columns(pt, widths)
        bv = [rng.getrandbits(64) for _ in bt]
        E = lambda side, kind, **kw: expected_kind_rows(bcols, bv, pcols, None, widths, side, kind, bits, **kw)
        inner, c0 = E(PROBE, INNER)
        want, coll = brute(H, bcols, bv, pcols, None, widths, bits)
        assert np.array_equal(inner, want) and set(c0.values()) == {0}
        assert key_collisions(bcols, pcols, widths, bits) == coll and (coll > 0) == (bits == 6)
        semi, c1 = E(PROBE, SEMI)
        anti, c2 = E(PROBE, ANTI)
        assert c1 == c2 and (c1["n_probe_matched"], c1["n_probe_unmatched"]) == (len(semi), len(anti)) and len(anti) > 0
        assert sorted(semi[:, 2].tolist() + anti[:, 2].tolist()) == list(range(len(pt)))  # SEMI u ANTI = probe
        assert not semi[:, [1, 3]].any() and not anti[:, [1, 3]].any()
        bsemi, c3 = E(BUILD, BUILD_SEMI)
        banti, _ = E(BUILD, BUILD_ANTI)
        assert sorted(bsemi[:, 1].tolist() + banti[:, 1].tolist()) == list(range(len(bt)))  # BUILD_SEMI u BUILD_ANTI = build
        assert (c3["n_build_matched"], c3["n_build_unmatched"], c3["n_probe_matched"]) == (len(bsemi), len(banti), 0)
        assert len(banti) > 0 and not bsemi[:, [2, 4]].any()
        po, _ = E(PROBE, PROBE_OUTER, probe_fill=7)
        bo, _ = E(BUILD, BUILD_OUTER, build_fill=9)
        fo, c4 = E(BUILD, FULL_OUTER, probe_fill=7, build_fill=9)
        # FULL_OUTER = inner + the unmatched rows of PROBE_OUTER and BUILD_OUTER
        un_p, un_b = po[po[:, 1] == NO_ROW], bo[bo[:, 2] == NO_ROW]
        assert np.array_equal(po[po[:, 1] != NO_ROW], inner) and np.array_equal(bo[bo[:, 2] != NO_ROW], inner)
        assert np.array_equal(un_p[:, [0, 2, 4]], anti[:, [0, 2, 4]]) and np.all(un_p[:, 3] == 7)
        assert np.array_equal(un_b[:, [0, 1, 3]], banti[:, [0, 1, 3]]) and np.all(un_b[:, 4] == 9)
        both = np.concatenate([inner, un_p, un_b])
        order = lambda rows: rows[np.lexsort(rows.T[::-1])]
        assert np.array_equal(order(fo), order(both))
        assert (c4["n_probe_unmatched"], c4["n_build_unmatched"]) == (len(anti), len(banti))
        # key64 of an unmatched row is its own tuple's
        assert np.array_equal(anti[:, 0], H.cols_key64([c[anti[:, 2].astype(np.int64)] for c in pcols], widths, bits))
        assert np.array_equal(banti[:, 0], H.cols_key64([c[banti[:, 1].astype(np.int64)] for c in bcols], widths, bits))
        for rows in (semi, anti, bsemi, banti, po, bo, fo):  # ordered: key64 ascending everywhere
            assert np.all(rows[1:, 0] >= rows[:-1, 0])
