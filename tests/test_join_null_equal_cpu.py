"""CPU-only checks of NULL-equals-NULL matching (HMJ_NULL_EQUAL; hmj_join_kind_cols_device and hmj_join_mixed_device): the
flag's value in the header is the binding's and a bit of its own, `cols_key64` / `mixed_key64` with null_equal=True restate
the header's key64 definition (hand-computed chains), and the brute-force reference test_join_null_equal_gpu.py compares
the device with -- `ne_rows`, over tuples in which NULL is the token None -- gives the hand-written rows of a 6-row case
for all eight kinds."""
import os
import subprocess
import tempfile

import numpy as np

from test_join_cols_kinds_cpu import (ALL_KINDS, ANTI, BUILD, BUILD_ANTI, BUILD_OUTER, BUILD_SEMI, COUNT_KEYS, FULL_OUTER, INNER, M64,
                                      NO_ROW, PROBE, PROBE_OUTER, SEMI)
from test_join_mixed_cpu import mix64
from test_join_str_cpu import str_hash

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = 0x9E3779B97F4A7C15
SEMI_ANTI = [(PROBE, SEMI), (PROBE, ANTI), (BUILD, BUILD_SEMI), (BUILD, BUILD_ANTI)]


# ---- the reference ------------------------------------------------------------------------------------------------------------
def null_last(t):
    """The sort key of a tuple under HMJ_ORDERED: column by column, a NULL slot (None) behind every valid value."""
    return tuple((1, 0) if v is None else (0, v) for v in t)


def ne_rows(tb, tp, kb, kp, bval, pval, side, kind, pfill=0, bfill=0):
    """A join kind under NULL-equals-NULL matching by brute force.  tb / tp: the build / probe rows' key tuples, None in a
    NULL slot -- plain tuple equality is the match rule: None equals None and nothing else; kb / kp: the rows' key64;
    bval / pval: the rows' payloads.  Returns rows [n, 5] (key64, r_row, s_row, rval, sval) in the HMJ_ORDERED order --
    (key64, tuple column by column with NULLS LAST, r_row, s_row), NO_ROW last; 0 in the columns the kind does not produce
    --, the four counters, n_key_pairs, n_collisions and what the call goes through: "ambiguous" (a semi / anti row whose
    key64 representative holds another tuple), "sort" (a run of equal key64 with several tuples among the ordered rows)."""
    b_by, p_by, bk, pk = {}, {}, {}, {}
    for r, t in enumerate(tb):
        b_by.setdefault(t, []).append(r)
        bk.setdefault(kb[r], []).append(r)
    for s, t in enumerate(tp):
        p_by.setdefault(t, []).append(s)
        pk.setdefault(kp[s], []).append(s)
    pairs = [(kp[s], null_last(t), r, s, bval[r], pval[s]) for s, t in enumerate(tp) for r in b_by.get(t, ())]
    p_match = [t in b_by for t in tp]
    b_match = [t in p_by for t in tb]

    def probe_rows(sel, fill):
        return [(kp[s], null_last(t), NO_ROW, s, fill, pval[s]) for s, t in enumerate(tp) if p_match[s] == sel]

    def build_rows(sel, fill):
        return [(kb[r], null_last(t), r, NO_ROW, bval[r], fill) for r, t in enumerate(tb) if b_match[r] == sel]

    counts = dict.fromkeys(COUNT_KEYS, 0)
    probe_counts = {"n_probe_matched": sum(p_match), "n_probe_unmatched": len(tp) - sum(p_match)}
    build_counts = {"n_build_matched": sum(b_match), "n_build_unmatched": len(tb) - sum(b_match)}
    absent = ()
    if (side, kind) == (PROBE, INNER):
        rows = pairs
    elif side == PROBE and kind in (SEMI, ANTI):
        rows, absent = probe_rows(kind == SEMI, 0), (1, 3)
        counts.update(probe_counts)
    elif side == PROBE:
        rows = pairs + probe_rows(False, pfill)
        counts.update(probe_counts)
    elif kind in (BUILD_SEMI, BUILD_ANTI):
        rows, absent = build_rows(kind == BUILD_SEMI, 0), (2, 4)
        counts.update(build_counts)
    elif kind == BUILD_OUTER:
        rows = pairs + build_rows(False, bfill)
        counts.update(build_counts)
    else:
        rows = pairs + probe_rows(False, pfill) + build_rows(False, bfill)
        counts.update(build_counts)
        counts.update(probe_counts)
    rows.sort(key=lambda x: x[:4])
    out = np.array([(k, r, s, rv, sv) for k, _, r, s, rv, sv in rows], np.uint64).reshape(-1, 5)
    for c in absent:
        out[:, c] = 0
    seen = set()
    if (side, kind) in SEMI_ANTI:  # the row against the first row of its key64 on the other side, then -- if that one holds
        n_pairs = n_coll = 0       # another tuple -- against every row of its key64 there
        K, ok, to, kk = (tp, bk, tb, kp) if side == PROBE else (tb, pk, tp, kb)
        for i, t in enumerate(K):
            o = ok.get(kk[i], [])
            if not o:
                continue
            n_pairs += 1
            if to[o[0]] != t:
                seen.add("ambiguous")
                n_pairs += len(o)
                n_coll += 1 + sum(1 for j in o if to[j] != t)
    else:
        n_pairs = sum(len(bk.get(k, ())) for k in kp)
        n_coll = n_pairs - len(pairs)
    if any(a[0] == b[0] and a[1] != b[1] for a, b in zip(rows, rows[1:])):
        seen.add("sort")
    return out, counts, n_pairs, n_coll, seen


def test_the_reference_on_a_hand_written_case():
    """Three build and three probe rows over (u32, u32); key64 is chosen by hand so that (NULL, 5) and (0, 5) collide."""
    tb = [(None, 5), (0, 5), (5, None)]
    tp = [(None, 5), (7, 7), (0, 5)]
    kb, kp = [10, 10, 20], [10, 30, 10]
    bval, pval = [100, 200, 300], [0, 1, 2]
    PF, BF = 0xF1, 0xB2
    # (0, 5) sorts in front of (NULL, 5): NULLS LAST in the first column
    pair_rows = [(10, 1, 2, 200, 2), (10, 0, 0, 100, 0)]
    want = {
        (PROBE, INNER): (pair_rows, {}, 4, 2, {"sort"}),
        (PROBE, SEMI): ([(10, 0, 2, 0, 2), (10, 0, 0, 0, 0)], {"n_probe_matched": 2, "n_probe_unmatched": 1}, 4, 2, {"ambiguous", "sort"}),
        (PROBE, ANTI): ([(30, 0, 1, 0, 1)], {"n_probe_matched": 2, "n_probe_unmatched": 1}, 4, 2, {"ambiguous"}),
        (PROBE, PROBE_OUTER): (pair_rows + [(30, NO_ROW, 1, PF, 1)], {"n_probe_matched": 2, "n_probe_unmatched": 1}, 4, 2, {"sort"}),
        (BUILD, BUILD_SEMI): ([(10, 1, 0, 200, 0), (10, 0, 0, 100, 0)], {"n_build_matched": 2, "n_build_unmatched": 1}, 4, 2,
                              {"ambiguous", "sort"}),
        (BUILD, BUILD_ANTI): ([(20, 2, 0, 300, 0)], {"n_build_matched": 2, "n_build_unmatched": 1}, 4, 2, {"ambiguous"}),
        (BUILD, BUILD_OUTER): (pair_rows + [(20, 2, NO_ROW, 300, BF)], {"n_build_matched": 2, "n_build_unmatched": 1}, 4, 2, {"sort"}),
        (BUILD, FULL_OUTER): (pair_rows + [(20, 2, NO_ROW, 300, BF), (30, NO_ROW, 1, PF, 1)],
                              {"n_build_matched": 2, "n_build_unmatched": 1, "n_probe_matched": 2, "n_probe_unmatched": 1}, 4, 2, {"sort"}),
    }
    assert set(want) == set(ALL_KINDS)
    for (side, kind), (rows, cnt, n_pairs, n_coll, seen) in want.items():
        got = ne_rows(tb, tp, kb, kp, bval, pval, side, kind, PF, BF)
        counts = dict.fromkeys(COUNT_KEYS, 0)
        counts.update(cnt)
        assert got[0].tolist() == [list(r) for r in rows], (side, kind)
        assert got[1:] == (counts, n_pairs, n_coll, seen), (side, kind, got[1:])
    # a NULL slot equals no value, whichever column it stands in
    out, counts, _, _, _ = ne_rows([(None, 1)], [(1, None), (0, 1), (None, 0)], [1], [1, 1, 1], [0], [0, 1, 2], PROBE, SEMI)
    assert len(out) == 0 and counts["n_probe_unmatched"] == 3
    out, _, _, _, _ = ne_rows([(None,), (b"",)], [(b"",), (None,), (None,)], [1, 2], [2, 1, 1], [7, 8], [0, 1, 2], PROBE, INNER)
    assert out.tolist() == [[1, 0, 1, 7, 1], [1, 0, 2, 7, 2], [2, 1, 0, 8, 0]]


# ---- the flag ----------------------------------------------------------------------------------------------------------------
def test_the_flag_is_the_headers_and_a_bit_of_its_own():
    import hashmergejoin_amd as H

    src = r"""
#include <cstdio>
#include "hmj.h"
int main() {
  std::printf("HMJ_NULL_EQUAL %u\nHMJ_ABI_VERSION %d\n", HMJ_NULL_EQUAL, HMJ_ABI_VERSION);
  std::printf("others %u\n", HMJ_MATERIALIZE | HMJ_ORDERED | HMJ_FIRST_WINS | HMJ_CHECKSUM | HMJ_SUM_PROBE);
  return 0;
}
"""
    with tempfile.TemporaryDirectory() as d:
        cc, exe = os.path.join(d, "flag.cc"), os.path.join(d, "flag")
        open(cc, "w").write(src)
        subprocess.check_call(["g++", "-std=c++11", "-I", os.path.join(ROOT, "include"), cc, "-o", exe])
        got = dict(line.split() for line in subprocess.check_output([exe]).decode().splitlines())
    assert int(got["HMJ_NULL_EQUAL"]) == H.HMJ_NULL_EQUAL == 0x20
    assert int(got["HMJ_ABI_VERSION"]) == 5  # a flag bit: no struct changed
    others = (H.HMJ_MATERIALIZE, H.HMJ_ORDERED, H.HMJ_FIRST_WINS, H.HMJ_CHECKSUM, H.HMJ_SUM_PROBE)
    assert int(got["others"]) == sum(others) == 0x1F
    assert all(H.HMJ_NULL_EQUAL & f == 0 for f in others)
    assert "HMJ_NULL_EQUAL" in H.__all__


# ---- key64 -------------------------------------------------------------------------------------------------------------------
def chain(k, vs, nulls=0, bits=0):
    """The header's four steps in plain integers.  vs: the columns' v_c (0 under a NULL slot); nulls: the mask m."""
    h = k
    for v in vs:
        h = mix64((h + v + GOLDEN) & M64)
    if nulls:
        h = mix64((h + nulls + GOLDEN) & M64)
    return h >> (64 - bits) if bits else h


def test_key64_without_nulls_is_the_plain_hashed_key():
    import hashmergejoin_amd as H

    rng = np.random.default_rng(20261020)
    for widths in ([4], [4, 4], [8, 4, 2], [1] * 8):
        cols = [rng.integers(0, 1 << (8 * w), 100, dtype=np.uint64, endpoint=False).astype("u%d" % w) for w in widths]
        all_valid = [np.ones(100, bool) for _ in widths]
        for bits in (0, 3, 63):
            plain = H.cols_key64(cols, widths, hash_bits=bits, force_hashed=True)
            for valid in (None, all_valid, [None] * len(widths)):
                assert np.array_equal(H.cols_key64(cols, widths, hash_bits=bits, valid=valid, null_equal=True), plain), (widths, bits)
                assert np.array_equal(H.mixed_key64(cols, bits, valid=valid, null_equal=True), plain), (widths, bits)
    # the defaults are today's values: valid alone changes nothing, and a packed key stays packed
    a, b = np.array([1, 2], np.uint32), np.array([3, 4], np.uint32)
    assert H.cols_key64([a, b], [4, 4]).tolist() == [(1 << 32) | 3, (2 << 32) | 4]
    assert H.cols_key64([a, b], [4, 4], valid=[[False, True], None]).tolist() == [(1 << 32) | 3, (2 << 32) | 4]
    strs = [[b"alpha", b""], a]
    assert np.array_equal(H.mixed_key64(strs, valid=[[False, True], None]), H.mixed_key64(strs))
    assert np.array_equal(H.mixed_key64(strs, 7, null_equal=True), H.mixed_key64(strs, 7))


def test_key64_tells_null_slots_from_values_and_from_each_other():
    import hashmergejoin_amd as H

    # rows: (NULL, 5), (0, 5), (5, NULL), (5, 0), (NULL, NULL)
    a, b = np.array([0, 0, 5, 5, 0], np.uint32), np.array([5, 5, 0, 0, 0], np.uint32)
    valid = [np.array([0, 1, 1, 1, 0], bool), np.array([1, 1, 0, 1, 0], bool)]
    got = [int(x) for x in H.cols_key64([a, b], [4, 4], valid=valid, null_equal=True)]
    assert len(set(got)) == 5
    assert got == [chain(2, [0, 5], 1), chain(2, [0, 5]), chain(2, [5, 0], 2), chain(2, [5, 0]), chain(2, [0, 0], 3)]
    assert got == [int(x) for x in H.mixed_key64([a, b], valid=valid, null_equal=True)]
    # hand-computed: k = 1, one u32 column holding NULL, then 7 -- mix64(1 + 0 + G), then mix64(. + 1 + G); mix64(1 + 7 + G)
    one = H.cols_key64([np.array([9, 7], np.uint32)], [4], valid=[[False, True]], null_equal=True)
    assert [int(x) for x in one] == [mix64((mix64((1 + GOLDEN) & M64) + 1 + GOLDEN) & M64), mix64((8 + GOLDEN) & M64)]
    assert mix64((1 + GOLDEN) & M64) == 0x910A2DEC89025CC1  # splitmix64's first output for seed 1: the mix64 in use
    # a NULL string is not the empty string, whose v_c is std::hash of no bytes -- not 0
    s = H.mixed_key64([[None, b"", b"x"]], valid=[[False, True, True]], null_equal=True)
    assert [int(x) for x in s] == [chain(1, [0], 1), chain(1, [str_hash(b"")]), chain(1, [str_hash(b"x")])]
    assert str_hash(b"") != 0 and len({int(x) for x in s}) == 3
    # mask bit 7: the eighth column
    cols = [np.array([c + 1], np.uint8) for c in range(8)]
    valid = [None] * 7 + [np.array([False])]
    assert int(H.cols_key64(cols, [1] * 8, valid=valid, null_equal=True)[0]) == chain(8, [1, 2, 3, 4, 5, 6, 7, 0], 0x80)
    # hash_bits keeps the top bits of the finished chain
    assert int(H.cols_key64(cols, [1] * 8, hash_bits=6, valid=valid, null_equal=True)[0]) == chain(8, [1, 2, 3, 4, 5, 6, 7, 0], 0x80, 6)


def test_key64_does_not_read_what_lies_under_a_null_slot():
    import hashmergejoin_amd as H

    rng = np.random.default_rng(5)
    n = 200
    valid = [rng.random(n) >= 0.3, None, rng.random(n) >= 0.3]
    a, b = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32), rng.integers(0, 1 << 16, n, dtype=np.uint64).astype(np.uint16)
    strs = [bytes(rng.integers(0, 256, int(rng.integers(0, 12)), dtype=np.uint8)) for _ in range(n)]
    a0 = np.where(valid[0], a, 0).astype(np.uint32)
    s0 = [s if ok else b"" for s, ok in zip(strs, valid[2])]
    sn = [s if ok else None for s, ok in zip(strs, valid[2])]
    want = H.mixed_key64([a, b, strs], 0, valid=valid, null_equal=True)
    assert np.array_equal(H.mixed_key64([a0, b, s0], 0, valid=valid, null_equal=True), want)
    assert np.array_equal(H.mixed_key64([a0, b, sn], 0, valid=valid, null_equal=True), want)
    c = rng.integers(0, 256, n, dtype=np.uint64).astype(np.uint8)
    v2 = [valid[0], None, valid[2]]
    assert np.array_equal(H.cols_key64([a0, b, np.where(valid[2], c, 0).astype(np.uint8)], [4, 2, 1], valid=v2, null_equal=True),
                          H.cols_key64([a, b, c], [4, 2, 1], valid=v2, null_equal=True))
