"""CPU-only checks of the string-key join kinds (hmj_join_kind_str_device): the symbol is exported, a NULL ctx fails without a
device, the ctypes mirror has the header's layout (g++ prints sizeof / offsetof), the Python constants equal the header's,
and the pure-Python brute force of every kind agrees with itself and with the inner join's brute force.  `kind_brute` is
imported by test_join_str_kinds_gpu.py as its expectation."""
import ctypes as C
import os
import random
import re
import subprocess
import tempfile

import numpy as np

from test_join_str_cpu import M64, str_hash

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO_ROW = M64
PROBE, BUILD = 0, 1
INNER, SEMI, ANTI, PROBE_OUTER = 0, 1, 2, 3
BUILD_SEMI, BUILD_ANTI, BUILD_OUTER, FULL_OUTER = 1, 2, 3, 4
ALL_KINDS = [(PROBE, INNER), (PROBE, SEMI), (PROBE, ANTI), (PROBE, PROBE_OUTER),
             (BUILD, BUILD_SEMI), (BUILD, BUILD_ANTI), (BUILD, BUILD_OUTER), (BUILD, FULL_OUTER)]


def _b(k):
    return k.encode() if isinstance(k, str) else bytes(k)


def kind_brute(bk, bv, pk, pv, side, kind, bits=0, probe_fill=0, build_fill=0):
    """(rows, counts) of a string kind join.  rows: [n, 5] uint64 (hash, r_row, s_row, rval, sval) in the HMJ_ORDERED order
    -- (hash, key bytes, r_row, s_row), NO_ROW last --, absent row columns NO_ROW and absent value columns 0, as
    Executor.str_kind_rows_to_numpy reads them.  counts: the four hmj_kind_counts fields."""
    bk, pk = [_b(k) for k in bk], [_b(k) for k in pk]
    b_by, p_by = {}, {}
    for r, k in enumerate(bk):
        b_by.setdefault(k, []).append(r)
    for s, k in enumerate(pk):
        p_by.setdefault(k, []).append(s)
    hashes = {k: str_hash(k, bits) for k in set(bk) | set(pk)}
    rows = []  # (hash, key, r, s, rval, sval)
    pair_rows = [(hashes[k], k, r, s, bv[r], pv[s]) for s, k in enumerate(pk) for r in b_by.get(k, ())]
    p_match = [k in b_by for k in pk]
    b_match = [k in p_by for k in bk]
    probe_rows = lambda sel, fill: [(hashes[k], k, NO_ROW, s, fill, pv[s]) for s, k in enumerate(pk) if p_match[s] == sel]
    build_rows = lambda sel, fill: [(hashes[k], k, r, NO_ROW, bv[r], fill) for r, k in enumerate(bk) if b_match[r] == sel]
    counts = {"n_probe_matched": 0, "n_probe_unmatched": 0, "n_build_matched": 0, "n_build_unmatched": 0}
    probe_counts = {"n_probe_matched": sum(p_match), "n_probe_unmatched": len(pk) - sum(p_match)}
    build_counts = {"n_build_matched": sum(b_match), "n_build_unmatched": len(bk) - sum(b_match)}
    if side == PROBE:
        if kind == INNER:
            rows = pair_rows
        elif kind == SEMI:
            rows, counts = probe_rows(True, 0), dict(counts, **probe_counts)
        elif kind == ANTI:
            rows, counts = probe_rows(False, 0), dict(counts, **probe_counts)
        elif kind == PROBE_OUTER:
            rows, counts = pair_rows + probe_rows(False, probe_fill), dict(counts, **probe_counts)
        else:
            raise ValueError(kind)
    else:
        counts = dict(counts, **build_counts)
        if kind == BUILD_SEMI:
            rows = build_rows(True, 0)
        elif kind == BUILD_ANTI:
            rows = build_rows(False, 0)
        elif kind == BUILD_OUTER:
            rows = pair_rows + build_rows(False, build_fill)
        elif kind == FULL_OUTER:
            rows = pair_rows + probe_rows(False, probe_fill) + build_rows(False, build_fill)
            counts.update(probe_counts)
        else:
            raise ValueError(kind)
    rows.sort(key=lambda t: t[:4])
    out = np.array([(h, r, s, rv & M64, sv & M64) for h, _, r, s, rv, sv in rows], np.uint64).reshape(-1, 5)
    return out, counts


def tmix_checks(rows):
    """n_matches, sums and HMJ_CHECKSUM's folds over result rows (value columns as kind_brute writes them)."""
    from test_join_kinds_cpu import tmix

    if not len(rows):
        return {"n_matches": 0, "sum_r": 0, "sum_s": 0, "xor_fold": 0, "mix_sum": 0}
    m = tmix(rows[:, 0], rows[:, 3], rows[:, 4])
    with np.errstate(over="ignore"):
        return {"n_matches": len(rows), "sum_r": int(rows[:, 3].sum(dtype=np.uint64)), "sum_s": int(rows[:, 4].sum(dtype=np.uint64)),
                "xor_fold": int(np.bitwise_xor.reduce(m)), "mix_sum": int(m.sum(dtype=np.uint64))}


# ---------------------------------------------------------------------------------------------
def test_str_kind_entry_is_exported():
    import hashmergejoin_amd as H

    assert hasattr(H.load_library(), "hmj_join_kind_str_device")


def test_str_kind_null_ctx_is_an_argument_error():
    import hashmergejoin_amd as H

    L = H.load_library()
    rel = H.StrRel()
    opts = H.StrKindOpts()
    opts.struct_size = C.sizeof(H.StrKindOpts)
    res = H.StrResult()
    assert L.hmj_join_kind_str_device(None, C.byref(rel), C.byref(rel), 0, C.byref(opts), C.byref(res)) == -1  # HMJ_E_ARG
    assert L.hmj_join_kind_str_device(None, C.byref(rel), C.byref(rel), 0, None, C.byref(res)) == -1
    assert L.hmj_join_kind_str_device(None, C.byref(rel), C.byref(rel), 0, C.byref(opts), None) == -1
    assert L.hmj_join_kind_str_device(None, None, None, 0, None, None) == -1


def test_str_kind_opts_match_the_header():
    import hashmergejoin_amd as H

    fields = [n for n, _ in H.StrKindOpts._fields_]
    src = "#include <cstddef>\n#include <cstdio>\n#include \"hmj.h\"\nint main() {\n"
    src += '  std::printf("size %zu\\n", sizeof(hmj_str_kind_opts));\n'
    for f in fields:
        src += '  std::printf("%s %%zu\\n", offsetof(hmj_str_kind_opts, %s));\n' % (f, f)
    src += '  std::printf("counts_size %zu\\n", sizeof(hmj_kind_counts));\n  return 0;\n}\n'
    with tempfile.TemporaryDirectory() as d:
        cc, exe = os.path.join(d, "layout.cc"), os.path.join(d, "layout")
        open(cc, "w").write(src)
        subprocess.check_call(["g++", "-std=c++11", "-I", os.path.join(ROOT, "include"), cc, "-o", exe])
        got = dict(line.split() for line in subprocess.check_output([exe]).decode().splitlines())
    assert int(got["size"]) == C.sizeof(H.StrKindOpts)
    assert int(got["counts_size"]) == C.sizeof(H.KindCounts)
    for f in fields:
        assert getattr(H.StrKindOpts, f).offset == int(got[f]), f


def test_python_constants_match_the_header():
    import hashmergejoin_amd as H

    hdr = open(os.path.join(ROOT, "include", "hmj.h")).read()
    defs = dict(re.findall(r"^#define (HMJ_\w+) (\S+)", hdr, re.M))
    assert defs["HMJ_STR_NO_ROW"] == "UINT64_MAX" and H.HMJ_STR_NO_ROW == M64 == NO_ROW
    for name in ("HMJ_KIND_PROBE_SIDE", "HMJ_KIND_BUILD_SIDE", "HMJ_JOIN_INNER", "HMJ_JOIN_SEMI", "HMJ_JOIN_ANTI",
                 "HMJ_JOIN_PROBE_OUTER", "HMJ_BUILD_SEMI", "HMJ_BUILD_ANTI", "HMJ_BUILD_OUTER", "HMJ_FULL_OUTER"):
        assert int(defs[name].rstrip("u")) == getattr(H, name), name
    assert (H.HMJ_KIND_PROBE_SIDE, H.HMJ_KIND_BUILD_SIDE) == (PROBE, BUILD)
    assert (H.HMJ_JOIN_SEMI, H.HMJ_JOIN_ANTI, H.HMJ_JOIN_PROBE_OUTER) == (SEMI, ANTI, PROBE_OUTER)
    assert (H.HMJ_BUILD_SEMI, H.HMJ_BUILD_ANTI, H.HMJ_BUILD_OUTER, H.HMJ_FULL_OUTER) == (BUILD_SEMI, BUILD_ANTI, BUILD_OUTER, FULL_OUTER)


def test_brute_force_agrees_with_itself():
    from test_join_str_gpu import _dup_relations, brute

    for bits in (0, 6, 12):
        rng = random.Random(40 + bits)
        bk, bv, pk, pv = _dup_relations(rng, 120, 12)
        inner, _ = kind_brute(bk, bv, pk, pv, PROBE, INNER, bits)
        want, _ = brute(bk, bv, pk, pv, bits)
        assert np.array_equal(inner, want)
        semi, c1 = kind_brute(bk, bv, pk, pv, PROBE, SEMI, bits)
        anti, c2 = kind_brute(bk, bv, pk, pv, PROBE, ANTI, bits)
        assert c1 == c2 and c1["n_probe_matched"] == len(semi) and c1["n_probe_unmatched"] == len(anti)
        assert sorted(semi[:, 2].tolist() + anti[:, 2].tolist()) == list(range(len(pk)))
        assert np.all(semi[:, 1] == NO_ROW) and np.all(semi[:, 3] == 0)
        bsemi, c3 = kind_brute(bk, bv, pk, pv, BUILD, BUILD_SEMI, bits)
        banti, _ = kind_brute(bk, bv, pk, pv, BUILD, BUILD_ANTI, bits)
        assert sorted(bsemi[:, 1].tolist() + banti[:, 1].tolist()) == list(range(len(bk)))
        assert c3["n_build_matched"] == len(bsemi) and c3["n_probe_matched"] == 0
        # outer kinds: the inner rows plus the unmatched rows with their fills
        po, _ = kind_brute(bk, bv, pk, pv, PROBE, PROBE_OUTER, bits, probe_fill=7)
        bo, _ = kind_brute(bk, bv, pk, pv, BUILD, BUILD_OUTER, bits, build_fill=9)
        fo, c4 = kind_brute(bk, bv, pk, pv, BUILD, FULL_OUTER, bits, probe_fill=7, build_fill=9)
        assert len(po) == len(inner) + len(anti) and len(bo) == len(inner) + len(banti)
        assert len(fo) == len(inner) + len(anti) + len(banti)
        assert c4["n_probe_unmatched"] == len(anti) and c4["n_build_unmatched"] == len(banti)
        assert np.all(po[po[:, 1] == NO_ROW][:, 3] == 7) and np.all(bo[bo[:, 2] == NO_ROW][:, 4] == 9)
        # ordered: hash ascending everywhere
        for rows in (semi, anti, bsemi, banti, po, bo, fo):
            assert np.all(np.diff(rows[:, 0].astype(np.float64)) >= 0)
