"""Plan-crossing GPU checks of the key joins' inner u64 join.  Every key join (hmj_join_cols_device, hmj_join_kind_cols_device,
hmj_join_mixed_device, the string entries, the NULL-equals-NULL variants) turns its relations into {key64,row} rows and joins
them with the u64 join, as HMJ_MATERIALIZE, HMJ_MATERIALIZE | HMJ_ORDERED or HMJ_MATERIALIZE | HMJ_FIRST_WINS.  The shape
classes of test_keyjoin_plans_cpu.py steer that join onto its plans -- global table, unique-key write, sorted write and its
foreign-key form, rank sort and rank runs, ordered expansion, split, window / dense build, presorted, slab, key ranges,
chunked build -- with the rows only a key join feeds it: dense ascending row indices as payloads, hashes or packed tuples
(dense, sorted, sharing a prefix, the all-ones marker) as keys.  Per case four entries (inner, PROBE SEMI, BUILD ANTI,
BUILD FULL_OUTER) in two modes (materialising, compared after a sort; HMJ_ORDERED, compared as a sequence), every comparison
exact against the numpy reference that pairs rows by tuple equality: rows, checksums, counters, key pairs, collisions, form.
A ledger of the plans reached per (family, entry, mode) is asserted at the end."""
import os

import numpy as np
import pytest

from test_join_cols_kinds_cpu import COUNT_KEYS, FULL_OUTER, INNER, M64, PROBE, kind_checks
from test_keyjoin_plans_cpu import (BFILL, ENTRIES, FAMILIES, PFILL, by_row_pair, case_of_ids, case_s9, case_s10, case_s11, ids_s1,
                                    ids_s3, ids_s4, ids_s5, ids_s6, ids_s7, ids_s8, with_marker)
from test_keyjoin_plans_cpu import GROUP_SHAPES, group_shape

pytestmark = pytest.mark.gpu
LEDGER = {}   # (family, entry, mode) -> {"path": bits, "refused": bits, "replanned": bool}
CASES_RUN = set()


@pytest.fixture(scope="module")
def H():
    import hashmergejoin_amd as H

    return H


def executor_with(H, hint=True, **env):
    """An Executor created under these HMJ_* switches (read when the context is created).  hint: the context carries a
    planner hint left by a u64 join whose keys do share their top 16 bits -- hmj_set_key_prefix_bits describes the CALLER'S u64
    keys, and every key join on the context must come out, and plan, as if it were not there."""
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    for k, v in env.items():
        os.environ[k] = v
    try:
        e = H.Executor(0)
    finally:
        for k in env:
            del os.environ[k]
    if hint:
        k = np.random.default_rng(16).permutation(1 << 16)[:15000].astype(np.uint64) * np.uint64(0x9E3779B1) + np.uint64(0xABCD << 48)
        rel = torch.from_numpy(np.stack([k, np.arange(15000, dtype=np.uint64)], 1).view(np.int64)).cuda()
        e.set_key_prefix_bits(16)
        r = e.join_device(rel[:10000].contiguous(), rel[5000:].contiguous(), H.HMJ_ORDERED)
        assert int(r.n_matches) == 5000
    return e


@pytest.fixture(scope="module")
def ex_default(H):
    e = executor_with(H)
    yield e
    e.close()


@pytest.fixture(scope="module")
def ex_part(H):  # small build sides are partitioned too
    e = executor_with(H, HMJ_GTABLE="0")
    yield e
    e.close()


@pytest.fixture(scope="module")
def ex_fan(H):  # ordered small-build joins sort (rank, payload) composites from fan-out 1 on
    e = executor_with(H, HMJ_GTABLE_SORT_FANOUT="1")
    yield e
    e.close()


@pytest.fixture(scope="module")
def ex_ranges(H):  # every ordered device-resident join in 2 key ranges
    e = executor_with(H, HMJ_KEY_RANGES_FORCE="1")
    yield e
    e.close()


@pytest.fixture(scope="module")
def ex_slab(H):  # slab partitioning from 2^22 rows on
    e = executor_with(H, HMJ_SLAB_MIN_LOG2="22")
    yield e
    e.close()


# ---- relations on the device, one call ---------------------------------------------------------------------------------------
def dev_col(a):
    import torch

    a = np.ascontiguousarray(a)
    if a.dtype.kind == "S":  # an 'S' array (no NUL inside a string) -> the Arrow large_string layout
        width = a.dtype.itemsize
        raw = np.frombuffer(a.tobytes(), np.uint8).reshape(len(a), width)
        lens = np.char.str_len(a).astype(np.int64)
        chars = raw[np.arange(width)[None, :] < lens[:, None]]
        off = np.zeros(len(a) + 1, np.int64)
        np.cumsum(lens, out=off[1:])
        return torch.from_numpy(chars.copy()).cuda(), torch.from_numpy(off).cuda()
    return torch.from_numpy(a.view("i%d" % a.dtype.itemsize)).cuda()


def dev_vals(v, n, always):
    import torch

    if v is None:
        return torch.arange(n, dtype=torch.int64, device="cuda") if always else None
    return torch.from_numpy(v.view(np.int64)).cuda()


class Dev:
    """A case's relations as the family's entry takes them."""

    def __init__(self, H, case):
        is_str = case.fam == "str"
        self.B, self.P = [dev_col(c) for c in case.bcols], [dev_col(c) for c in case.pcols]
        self.bv, self.pv = dev_vals(case.bvals, case.nb, is_str), dev_vals(case.pvals, case.np, is_str)
        valid = lambda masks: None if masks is None else [None if m is None else H.pack_validity(m, 0, "cuda") for m in masks]
        self.bvalid, self.pvalid = valid(case.bvalid), valid(case.pvalid)


def run(H, ex, case, D, side, kind, flags):
    """One call of the family's entry: (result, rows [n,5] with 0 in the columns the kind does not produce, form or None,
    pairs of equal key64 compared, collisions, counters or None)."""
    fam, bits = case.fam, case.bits
    inner = (side, kind) == (PROBE, INNER)
    if fam == "str":
        B, P = D.B[0] + (D.bv,), D.P[0] + (D.pv,)
        if inner:
            res, info = ex.join_str_device(B, P, flags, bits)
            rows = ex.str_rows_to_numpy(res)
        else:
            res, info = ex.join_kind_str_device(B, P, side, kind, flags, bits, PFILL, BFILL)
            rows = ex.str_kind_rows_to_numpy(res)
            if kind != FULL_OUTER and len(rows):  # semi / anti: the absent row column reads as NO_ROW here
                absent = 1 if side == PROBE else 2
                assert np.all(rows[:, absent] == M64)
                rows[:, absent] = 0
        return res, rows, None, info["n_hash_pairs"], info["n_collisions"], None if inner else info
    if fam == "mixed":
        res, info = ex.join_mixed_device(D.B, D.bv, D.P, D.pv, side, kind, flags, bits, PFILL, BFILL)
        return res, ex.mixed_rows_to_numpy(res), None, info["n_key_pairs"], info["n_collisions"], info
    if fam == "nulleq842":
        res, info = ex.join_kind_cols_device(D.B, D.bv, D.P, D.pv, side, kind, flags | H.HMJ_NULL_EQUAL, bits, False, PFILL, BFILL,
                                             D.bvalid, D.pvalid)
    elif inner:
        res, info = ex.join_cols_device(D.B, D.bv, D.P, D.pv, flags, bits)
    else:
        res, info = ex.join_kind_cols_device(D.B, D.bv, D.P, D.pv, side, kind, flags, bits, False, PFILL, BFILL)
    return res, ex.cols_kind_rows_to_numpy(res), info["form"], info["n_key_pairs"], info["n_collisions"], None if (inner and fam != "nulleq842") else info


CASES = {}  # (class, family, hash_bits, ...) -> the case and its reference, built once per module
LARGE = [None]  # ... a case of more than 2^18 rows only until the next large one is asked for: their result rows fill gigabytes


def case_for(key, build):
    if key in CASES:
        return CASES[key]
    if LARGE[0] is not None and LARGE[0][0] == key:
        return LARGE[0][1]
    case = build()
    if case.nb + case.np <= 1 << 18:
        CASES[key] = case
    else:
        LARGE[0] = (key, case)
    return case


def path_names(H, path):
    names = {getattr(H._lib, n): n[9:] for n in dir(H._lib) if n.startswith("HMJ_PATH_")}
    return "|".join(sorted(names.get(1 << b, hex(1 << b)) for b in range(32) if path >> b & 1))


def refused_names(H, refused):
    names = {getattr(H._lib, n): n[12:] for n in dir(H._lib) if n.startswith("HMJ_REFUSED_")}
    return "|".join(sorted(names.get(1 << b, hex(1 << b)) for b in range(32) if refused >> b & 1))


def check_case(H, ex, case, label, entries=ENTRIES, modes=("materialize", "ordered"), D=None, forget=True):
    """The case's entries in both modes against the reference; returns {(entry, mode): last_plan()} and feeds the ledger."""
    D = D or Dev(H, case)
    if forget:
        ex.forget_workloads()  # (what earlier cases taught the context's workloads is not this case's business)
    want_form = {"packed": H.HMJ_COLS_PACKED, "hashed": H.HMJ_COLS_HASHED}[FAMILIES[case.fam][1]]
    plans = {}
    if not hasattr(case, "checked"):
        case.checked = {}  # per entry: the rows' checksums and their unordered form, once per case
    checked = case.checked
    for name, side, kind in entries:
        want, counts, n_pairs, n_coll = case.ref.rows(side, kind)
        if name not in checked:
            checked[name] = (kind_checks(want), by_row_pair(want))
        ck, want_unordered = checked[name]
        for mode in modes:
            flags = (H.HMJ_ORDERED if mode == "ordered" else H.HMJ_MATERIALIZE) | H.HMJ_CHECKSUM
            tag = (label, case.fam, case.bits, name, mode)
            res, got, form, got_pairs, got_coll, info = run(H, ex, case, D, side, kind, flags)
            p = ex.last_plan()
            plans[(name, mode)] = p
            e = LEDGER.setdefault((case.fam, name, mode), {"path": 0, "refused": 0, "replanned": False})
            e["path"] |= p["path"]
            e["refused"] |= p["refused"]
            e["replanned"] |= p["attempts"] > 1
            print(tag, "rows", len(got), path_names(H, p["path"]), "refused", refused_names(H, p["refused"]), "attempts", p["attempts"],
                  "pairs", got_pairs, "collisions", got_coll, flush=True)
            assert res.checks() == ck, (tag, res.checks(), ck)
            assert (got_pairs, got_coll) == (n_pairs, n_coll), (tag, got_pairs, n_pairs, got_coll, n_coll)
            assert form is None or form == want_form, tag
            if info is not None:
                assert {k: info[k] for k in COUNT_KEYS} == counts, (tag, info, counts)
            assert got.shape == want.shape, (tag, got.shape, want.shape)
            if mode == "ordered":
                assert np.array_equal(got, want), (tag, np.flatnonzero(np.any(got != want, axis=1))[:5])
            else:
                assert np.array_equal(by_row_pair(got), want_unordered), tag
    ex.release_result()
    CASES_RUN.add((label, case.fam, case.bits))
    return plans


def reached(H, plans, names, mode, entries=("inner", "full_outer")):
    """Each of those entries' joins in `mode` took a plan with every one of these HMJ_PATH_* bits ('A|B': one of them)."""
    for entry in entries:
        path = plans[(entry, mode)]["path"]  # (KeyError: the case did not run that entry in that mode)
        for alt in names:
            bits = 0
            for n in alt.split("|"):
                bits |= getattr(H._lib, "HMJ_PATH_" + n)
            assert path & bits, (entry, mode, alt, path_names(H, path))


ALL4 = ("inner", "probe_semi", "build_anti", "full_outer")


# ---- S1, S2, S3: small build sides (the global table) ------------------------------------------------------------------------
@pytest.mark.parametrize("fam,nb", [("packed44", 1000), ("packed44", 60000), ("packed8", 1000), ("hashed842", 1000), ("hashed842", 60000),
                                    ("mixed", 1000), ("str", 1000)])
def test_s1_small_unique_build_side(H, ex_default, fam, nb):
    plans = check_case(H, ex_default, case_for(("S1", fam, 0, nb), lambda: case_of_ids(fam, *ids_s1(nb))), "S1/%d" % nb)
    reached(H, plans, ["GLOBAL_TABLE"], "materialize", ("inner", "probe_semi", "full_outer"))
    # (BUILD ANTI's representative join builds over the PROBE relation: at 1000 tuples its 66 561 rows hold every key some 50
    #  times, more copies than a lookup may walk, and the table gives up; at 60 000 it holds them)
    p = plans[("build_anti", "materialize")]
    assert p["path"] & H.HMJ_PATH_GLOBAL_TABLE or p["refused"] & H._lib.HMJ_REFUSED_GTABLE_GAVE_UP, p
    assert nb == 1000 or p["path"] & H.HMJ_PATH_GLOBAL_TABLE, p


@pytest.mark.parametrize("fam", ["packed8", "packed44", "packed2222"])
def test_s2_all_ones_marker(H, fam):
    """A packed tuple of 8 bytes 0xFF is key64 == 2^64 - 1, the global table's empty-slot marker: the table gives up, the
    partitioned path delivers the rows, the cool-down belongs to the key join's workload."""
    import torch

    L = H._lib
    base = case_for(("S1", fam, 0, 1000), lambda: case_of_ids(fam, *ids_s1(1000)))
    ex = executor_with(H, hint=False)
    try:
        case = with_marker(base, [77], slice(5, None, 1000))
        D = Dev(H, case)
        plans = check_case(H, ex, case, "S2", D=D)
        for entry in ALL4:  # the first join of every entry's workload asked the table and was refused
            p = plans[(entry, "materialize")]
            assert p["refused"] & L.HMJ_REFUSED_GTABLE_GAVE_UP and not p["path"] & H.HMJ_PATH_GLOBAL_TABLE, (entry, p)
        # the same call again: skipped while the workload cools down, the same rows
        plans = check_case(H, ex, case, "S2/again", D=D, modes=("materialize",), forget=False)
        for entry in ALL4:
            p = plans[(entry, "materialize")]
            assert p["refused"] & L.HMJ_REFUSED_GTABLE_COOLING and not p["path"] & H.HMJ_PATH_GLOBAL_TABLE, (entry, p)
        # a u64 join of another shape on the same context still takes the table
        U, V = ex.gen_build(1000), ex.gen_uniform_domain(100000, 1000)
        r = ex.join_device(U, V, 0)
        p = ex.last_plan()
        assert int(r.n_matches) == 100000 and p["path"] & H.HMJ_PATH_GLOBAL_TABLE and p["cooling"] == 0, p
        del U, V
        torch.cuda.synchronize()
        # the marker on the probe side only: the table holds no such key, the rows are unmatched, nothing gives up
        case = with_marker(base, [], slice(5, None, 1000))
        assert not case.ref.p_match[5::1000].any()
        plans = check_case(H, ex, case, "S2/probe-only")
        for entry in ("inner", "probe_semi", "full_outer"):
            p = plans[(entry, "materialize")]
            assert p["path"] & H.HMJ_PATH_GLOBAL_TABLE and not p["refused"] & L.HMJ_REFUSED_GTABLE_GAVE_UP, (entry, p)
        # (BUILD ANTI asks about the build side: its representative join builds the table over the PROBE relation)
        p = plans[("build_anti", "materialize")]
        assert p["refused"] & L.HMJ_REFUSED_GTABLE_GAVE_UP and not p["path"] & H.HMJ_PATH_GLOBAL_TABLE, p
    finally:
        ex.close()


def forced_bits(H, ex, case, label, D):
    """S13: the case again under forced radix bits 0, 4 and 18."""
    chunked = 0
    for bits in (0, 4, 18):
        ex.set_radix_bits(bits)
        try:
            plans = check_case(H, ex, case, "%s/bits%d" % (label, bits), D=D)
        finally:
            ex.set_radix_bits(None)
        chunked |= plans[("inner", "materialize")]["path"] | plans[("inner", "ordered")]["path"]
    return chunked


@pytest.mark.parametrize("fam", ["packed44", "hashed842", "mixed", "str"])
def test_s3_small_build_side_with_duplicates(H, ex_default, ex_part, fam):
    """Every third build tuple twice: the table gives up on the materialising form (a probe row may expand to several
    rows), and the answer is the same before the cool-down, during it and on the call after it ran out."""
    L = H._lib
    ex = ex_default
    case = case_for(("S3", fam, 0), lambda: case_of_ids(fam, *ids_s3()))
    D = Dev(H, case)
    plans = check_case(H, ex, case, "S3", D=D)
    p = plans[("inner", "materialize")]
    assert p["refused"] & L.HMJ_REFUSED_GTABLE_GAVE_UP and not p["path"] & H.HMJ_PATH_GLOBAL_TABLE, p
    reached(H, plans, ["GLOBAL_TABLE"], "materialize", ("probe_semi",))  # (first wins: duplicate build keys are fine)
    want = by_row_pair(case.ref.rows(PROBE, INNER)[0])
    refused = []
    for call in range(2, 11):  # the workload's next 8 materialising joins skip the table; its tenth asks again
        res, got, _, _, _, _ = run(H, ex, case, D, PROBE, INNER, H.HMJ_MATERIALIZE)
        refused.append(ex.last_plan()["refused"] & (L.HMJ_REFUSED_GTABLE_COOLING | L.HMJ_REFUSED_GTABLE_GAVE_UP))
        LEDGER[(fam, "inner", "materialize")]["refused"] |= refused[-1]
        assert np.array_equal(by_row_pair(got), want), call
    assert refused == [L.HMJ_REFUSED_GTABLE_COOLING] * 8 + [L.HMJ_REFUSED_GTABLE_GAVE_UP], refused
    if fam in ("packed44", "hashed842"):
        forced_bits(H, ex_part, case, "S13/S3", D)


# ---- S4, S8, S10, S13: mid-size unique build sides ---------------------------------------------------------------------------
@pytest.mark.parametrize("fam", ["packed44", "packed8", "hashed842", "mixed", "str", "nulleq842"])
def test_s4_mid_size_unique(H, ex_part, fam):
    plans = check_case(H, ex_part, case_for(("S4", fam, 0), lambda: case_of_ids(fam, *ids_s4())), "S4")
    reached(H, plans, ["UNIQ_WRITE"], "materialize")
    reached(H, plans, ["SORTED_WRITE"], "ordered")


@pytest.mark.parametrize("fam", ["packed44", "hashed842", "mixed", "str"])
def test_s8_one_hot_probe_tuple(H, ex_part, fam):
    case = case_for(("S8", fam, 0), lambda: case_of_ids(fam, *ids_s8()))
    D = Dev(H, case)
    plans = check_case(H, ex_part, case, "S8", D=D)
    reached(H, plans, ["SPLIT", "HOT_KEY_HINT"], "materialize")
    if fam in ("packed44", "hashed842"):
        assert forced_bits(H, ex_part, case, "S13/S8", D) & H.HMJ_PATH_CHUNKED_BUILD


@pytest.mark.parametrize("fam", ["packed44", "packed8"])
def test_s10_relations_sorted_by_their_tuple(H, ex_part, fam):
    plans = check_case(H, ex_part, case_for(("S10", fam, 0), lambda: case_s10(fam)), "S10")
    reached(H, plans, ["PRESORTED"], "materialize")
    reached(H, plans, ["PRESORTED"], "ordered")


def test_s9_dense_packed_keys(H, ex_part):
    plans = check_case(H, ex_part, case_for(("S9", "packed44", 0), case_s9), "S9")
    reached(H, plans, ["WINDOW|DENSE_BUILD"], "materialize")
    reached(H, plans, ["WINDOW|DENSE_BUILD"], "ordered")


# ---- S5, S7, S12: fan-out and duplicates ------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam", ["packed44", "hashed842", "mixed"])
def test_s5_foreign_keys(H, ex_part, ex_ranges, fam):
    case = case_for(("S5", fam, 0), lambda: case_of_ids(fam, *ids_s5()))
    D = Dev(H, case)
    plans = check_case(H, ex_part, case, "S5", D=D)
    reached(H, plans, ["SORTED_FK"], "ordered")
    if fam != "mixed":  # S12
        plans = check_case(H, ex_ranges, case, "S12/S5", D=D, modes=("ordered",))
        reached(H, plans, ["KEY_RANGES"], "ordered")


@pytest.mark.parametrize("fam,bits", [("packed44", 0), ("packed8", 0), ("hashed842", 0), ("hashed842", 16), ("mixed", 0), ("mixed", 16),
                                      ("str", 0), ("str", 16), ("nulleq842", 0), ("nulleq842", 16)])
def test_s7_many_to_many(H, ex_part, ex_ranges, fam, bits):
    """hash_bits = 0: equal key64 is equal tuples, the collision sort has nothing to do and the plan's own order is the
    result's.  hash_bits = 16: runs of equal key64 hold several tuples while the plan writes them; the collision sort re-orders
    them inside the order the plan delivered, and n_collisions is exact."""
    case = case_for(("S7", fam, bits), lambda: case_of_ids(fam, *ids_s7(), bits=bits))
    assert case.ref.max_mixed_run() <= 1024 and (bits == 0) == case.collision_free()
    D = Dev(H, case)
    plans = check_case(H, ex_part, case, "S7", D=D)
    reached(H, plans, ["ORDERED_EXPANSION"], "ordered")
    if fam in ("packed44", "hashed842"):  # S12
        plans = check_case(H, ex_ranges, case, "S12/S7", D=D, modes=("ordered",), entries=[ENTRIES[0], ENTRIES[3]])
        reached(H, plans, ["KEY_RANGES"], "ordered")


@pytest.mark.parametrize("fam", ["packed44", "hashed842"])
def test_s7_one_tuple_on_5000_build_rows(H, ex_part, fam):
    case = case_for(("S7/hot", fam, 0), lambda: case_of_ids(fam, *ids_s7(hot=5000)))
    plans = check_case(H, ex_part, case, "S7/hot", entries=[ENTRIES[0], ENTRIES[3]])
    for entry in ("inner", "full_outer"):  # beyond the expansion kernel's capacity: the fallback delivers the rows
        assert plans[(entry, "ordered")]["refused"] & H._lib.HMJ_REFUSED_EXPANSION_GAVE_UP, plans[(entry, "ordered")]


# ---- S6: a small build side under a long probe side, ordered -----------------------------------------------------------------
@pytest.mark.parametrize("fam,nb,n_probe,missing", [
    ("packed44", 1000, 300001, 0), ("packed44", 1000, 300001, 1 / 3), ("packed44", 5000, 700000, 0), ("packed44", 5000, 700000, 1 / 3),
    ("hashed842", 1000, 300001, 0), ("hashed842", 1000, 300001, 1 / 3), ("hashed842", 5000, 700000, 0), ("hashed842", 5000, 700000, 1 / 3),
    ("packed8", 1000, 300001, 0), ("mixed", 1000, 300001, 0), ("str", 1000, 300001, 1 / 3)])
def test_s6_small_build_side_under_a_long_probe_side(H, ex_fan, fam, nb, n_probe, missing):
    """The payloads are the dense ascending row indices: the rank runs' strided pass."""
    case = case_for(("S6", fam, 0, nb, n_probe, bool(missing)), lambda: case_of_ids(fam, *ids_s6(nb, n_probe, missing)))
    plans = check_case(H, ex_fan, case, "S6/%d/%d/%s" % (nb, n_probe, "miss" if missing else "all"))
    reached(H, plans, ["ORDER_BY_RANK_SORT", "RANK_RUNS"], "ordered")
    if not missing:
        reached(H, plans, ["RANK_LOOKUP_IN_PASS"], "ordered")


# ---- S11: 2^22 + 77 rows per relation ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def s11(H):
    case = case_for(("S11", "hashed842", 0), case_s11)
    return case, Dev(H, case)


@pytest.mark.parametrize("entry", [ENTRIES[0], ENTRIES[3]], ids=["inner", "full_outer"])
def test_s11_slab_partitioning(H, ex_slab, s11, entry):
    plans = check_case(H, ex_slab, s11[0], "S11", entries=[entry], D=s11[1])
    reached(H, plans, ["SLAB"], "materialize", (entry[0],))


# ---- grouping: hmj_group_cols_device sorts the same {key64,row} rows ---------------------------------------------------------
GROUP_SORTS = {}  # shape -> the HMJ_PATH_* bits of hmj_sort_u64_device on the shape's {key64,row} rows


@pytest.fixture(scope="module")
def ex_sort(H):  # the sort's MSD form and its chain of slab passes from 2^17 rows on
    e = executor_with(H, hint=False, HMJ_SORT_MSD_MIN_LOG2="17", HMJ_SORT_SLAB_MIN_LOG2="17")
    yield e
    e.close()


@pytest.mark.parametrize("shape", GROUP_SHAPES)
def test_grouping_sorts_the_same_rows(H, ex_sort, shape):
    """hmj_group_cols_device leaves last_plan() untouched, so what its sort took is read from hmj_sort_u64_device on the same
    {key64,row} rows on the same context."""
    import torch

    from test_group_cols_gpu import check, group

    cols, widths = group_shape(shape)
    n = len(cols[0])
    vals = np.random.default_rng(n).integers(0, 1 << 64, size=n, dtype=np.uint64)
    for ordered in (False, True):
        ex_sort.forget_workloads()  # (sorts of one size share a memo: every call meets the shape as the first one did)
        res, info, got = group(H, ex_sort, cols, vals, flags=H.HMJ_ORDERED if ordered else H.HMJ_MATERIALIZE)
        check(H, res, info, got, H.expected_groups(cols, widths, vals, ordered=ordered), ordered, (shape, ordered))
    rows = np.stack([H.cols_key64(cols, widths), np.arange(n, dtype=np.uint64)], 1)
    ex_sort.forget_workloads()
    out = ex_sort.sort_device(torch.from_numpy(rows.view(np.int64)).cuda())
    path = ex_sort.last_timing()["path"]
    assert np.array_equal(out.cpu().numpy().view(np.uint64), rows[np.argsort(rows[:, 0], kind="stable")])
    GROUP_SORTS[shape] = path
    print(("group", shape), n, "rows", int(res.n_groups), "groups", path_names(H, path), flush=True)


# ---- the ledger ----------------------------------------------------------------------------------------------------------------
N_CASES = 77  # check_case runs of distinct (label, family, hash_bits) in a run of the whole file
# What every key form must reach: each of these plan bits on at least one packed and at least one hashed family ...
MINIMUM = ["GLOBAL_TABLE", "UNIQ_WRITE", "EXACT", "SLAB", "SPLIT", "WINDOW|DENSE_BUILD", "PRESORTED", "HOT_KEY_HINT", "CHUNKED_BUILD",
           "SORTED_WRITE", "SORTED_FK", "ORDERED_EXPANSION", "ORDER_BY_RANK_SORT", "RANK_RUNS", "RANK_LOOKUP_IN_PASS", "KEY_RANGES"]
# Excused for the hashed forms, reached by the packed ones.  PRESORTED: launch_check_partitioned (api.hip, where
# HMJ_PATH_PRESORTED is set) must find the rows in key64 order, and a relation sorted by its tuple is in no order by its hash.
# WINDOW / DENSE_BUILD: every bit of a hash varies and its values fill their range, so the dense plan's `fraction < 0.7` and the
# key window's `best_low != 64 - prefix - B` (api.hip, where HMJ_PATH_DENSE_BUILD / HMJ_PATH_WINDOW are set) never hold; with
# hash_bits the unused top bits are a shared prefix, which the sample skips without moving the window.
EXCUSED = {"packed": [], "hashed": ["PRESORTED", "WINDOW|DENSE_BUILD"]}
REFUSALS = ["GTABLE_GAVE_UP", "GTABLE_COOLING", "EXPANSION_GAVE_UP"]
# ... and what no key join can take: the count-only plans (the inner join always materialises), a prepared build side, the
# host entry's pipeline
NEVER = ["LDS_TABLE", "SLAB_PROBE", "SLAB_ONE_PASS", "PREPARED", "HOST_PIPELINE"]
# (family, entry, mode): (HMJ_PATH_* bits, HMJ_REFUSED_* bits, whether a join planned again), observed on an MI355X and compared
# for equality: a plan newly reached is noticed as a plan lost is.  UNSTABLE: the one bit left out of the comparison -- under
# bitmaps the rows that have a key are compacted in no fixed order, so the planner's key sample, and with it HOT_KEY_HINT,
# differs from run to run.
UNSTABLE = {"nulleq842": "HOT_KEY_HINT"}
OBSERVED = {
    ('hashed842', 'build_anti', 'materialize'): ('CHUNKED_BUILD|EXACT|GLOBAL_TABLE|HOT_KEY_HINT|ORDERED_EXPANSION|UNIQ_WRITE', 'GTABLE_GAVE_UP|GTABLE_SHAPE|SLAB_SHAPE', False),
    ('hashed842', 'build_anti', 'ordered'): ('CHUNKED_BUILD|EXACT|GLOBAL_TABLE|HOT_KEY_HINT|ORDERED_EXPANSION|UNIQ_WRITE', 'FAST_WRITE_COOLING|GTABLE_COOLING|GTABLE_SHAPE|SLAB_SHAPE', False),
    ('hashed842', 'full_outer', 'materialize'): ('CHUNKED_BUILD|EXACT|GLOBAL_TABLE|HOT_KEY_HINT|ORDERED_EXPANSION|SLAB|SPLIT|UNIQ_WRITE', 'GTABLE_GAVE_UP|GTABLE_SHAPE|SLAB_SHAPE', False),
    ('hashed842', 'full_outer', 'ordered'): ('CHUNKED_BUILD|EXACT|GLOBAL_TABLE|HOT_KEY_HINT|KEY_RANGES|ORDERED_EXPANSION|ORDER_BY_RANK_SORT|ORDER_DEFERRED|RANK_LOOKUP_IN_PASS|RANK_RUNS|SLAB|SORTED_FK|SORTED_FK_WIDE|SORTED_WRITE|SPLIT|UNIQ_WRITE', 'EXPANSION_GAVE_UP|FAST_WRITE_COOLING|GTABLE_SHAPE|SLAB_SHAPE', True),
    ('hashed842', 'inner', 'materialize'): ('CHUNKED_BUILD|EXACT|GLOBAL_TABLE|HOT_KEY_HINT|ORDERED_EXPANSION|SLAB|SPLIT|UNIQ_WRITE', 'GTABLE_COOLING|GTABLE_GAVE_UP|GTABLE_SHAPE|SLAB_SHAPE', False),
    ('hashed842', 'inner', 'ordered'): ('CHUNKED_BUILD|EXACT|GLOBAL_TABLE|HOT_KEY_HINT|KEY_RANGES|ORDERED_EXPANSION|ORDER_BY_RANK_SORT|ORDER_DEFERRED|RANK_LOOKUP_IN_PASS|RANK_RUNS|SLAB|SORTED_FK|SORTED_FK_WIDE|SORTED_WRITE|SPLIT|UNIQ_WRITE', 'EXPANSION_GAVE_UP|FAST_WRITE_COOLING|GTABLE_SHAPE|SLAB_SHAPE', True),
    ('hashed842', 'probe_semi', 'materialize'): ('CHUNKED_BUILD|EXACT|GLOBAL_TABLE|HOT_KEY_HINT|ORDERED_EXPANSION|SPLIT|UNIQ_WRITE', 'GTABLE_SHAPE|SLAB_SHAPE', False),
    ('hashed842', 'probe_semi', 'ordered'): ('CHUNKED_BUILD|EXACT|GLOBAL_TABLE|HOT_KEY_HINT|ORDERED_EXPANSION|SPLIT|UNIQ_WRITE', 'FAST_WRITE_COOLING|GTABLE_SHAPE|SLAB_SHAPE', False),
    ('mixed', 'build_anti', 'materialize'): ('EXACT|HOT_KEY_HINT|ORDERED_EXPANSION|UNIQ_WRITE', 'GTABLE_GAVE_UP|GTABLE_SHAPE|SLAB_SHAPE', False),
    ('mixed', 'build_anti', 'ordered'): ('EXACT|HOT_KEY_HINT|ORDERED_EXPANSION|UNIQ_WRITE', 'FAST_WRITE_COOLING|GTABLE_COOLING|GTABLE_SHAPE|SLAB_SHAPE', False),
    ('mixed', 'full_outer', 'materialize'): ('EXACT|GLOBAL_TABLE|HOT_KEY_HINT|ORDERED_EXPANSION|SPLIT|UNIQ_WRITE', 'GTABLE_GAVE_UP|GTABLE_SHAPE|SLAB_SHAPE', False),
    ('mixed', 'full_outer', 'ordered'): ('EXACT|GLOBAL_TABLE|HOT_KEY_HINT|ORDERED_EXPANSION|ORDER_BY_RANK_SORT|ORDER_DEFERRED|RANK_LOOKUP_IN_PASS|RANK_RUNS|SLAB|SORTED_FK|SORTED_FK_WIDE|SORTED_WRITE|SPLIT|UNIQ_WRITE', 'EXPANSION_GAVE_UP|FAST_WRITE_COOLING|GTABLE_SHAPE|SLAB_SHAPE', True),
    ('mixed', 'inner', 'materialize'): ('EXACT|GLOBAL_TABLE|HOT_KEY_HINT|ORDERED_EXPANSION|SPLIT|UNIQ_WRITE', 'GTABLE_COOLING|GTABLE_GAVE_UP|GTABLE_SHAPE|SLAB_SHAPE', False),
    ('mixed', 'inner', 'ordered'): ('EXACT|GLOBAL_TABLE|HOT_KEY_HINT|ORDERED_EXPANSION|ORDER_BY_RANK_SORT|ORDER_DEFERRED|RANK_LOOKUP_IN_PASS|RANK_RUNS|SLAB|SORTED_FK|SORTED_FK_WIDE|SORTED_WRITE|SPLIT|UNIQ_WRITE', 'EXPANSION_GAVE_UP|FAST_WRITE_COOLING|GTABLE_SHAPE|SLAB_SHAPE', True),
    ('mixed', 'probe_semi', 'materialize'): ('EXACT|GLOBAL_TABLE|HOT_KEY_HINT|ORDERED_EXPANSION|SPLIT|UNIQ_WRITE', 'GTABLE_SHAPE|SLAB_SHAPE', False),
    ('mixed', 'probe_semi', 'ordered'): ('EXACT|GLOBAL_TABLE|HOT_KEY_HINT|ORDERED_EXPANSION|SPLIT|UNIQ_WRITE', 'FAST_WRITE_COOLING|GTABLE_SHAPE|SLAB_SHAPE', False),
    ('nulleq842', 'build_anti', 'materialize'): ('EXACT|ORDERED_EXPANSION|UNIQ_WRITE', 'GTABLE_SHAPE|SLAB_SHAPE', False),
    ('nulleq842', 'build_anti', 'ordered'): ('EXACT|ORDERED_EXPANSION|UNIQ_WRITE', 'FAST_WRITE_COOLING|GTABLE_SHAPE|SLAB_SHAPE', False),
    ('nulleq842', 'full_outer', 'materialize'): ('EXACT|ORDERED_EXPANSION|UNIQ_WRITE', 'GTABLE_SHAPE|SLAB_SHAPE', False),
    ('nulleq842', 'full_outer', 'ordered'): ('EXACT|ORDERED_EXPANSION|SORTED_WRITE|UNIQ_WRITE', 'GTABLE_SHAPE|SLAB_SHAPE', False),
    ('nulleq842', 'inner', 'materialize'): ('EXACT|ORDERED_EXPANSION|UNIQ_WRITE', 'GTABLE_SHAPE|SLAB_SHAPE', False),
    ('nulleq842', 'inner', 'ordered'): ('EXACT|ORDERED_EXPANSION|SORTED_WRITE|UNIQ_WRITE', 'GTABLE_SHAPE|SLAB_SHAPE', False),
    ('nulleq842', 'probe_semi', 'materialize'): ('EXACT|ORDERED_EXPANSION|UNIQ_WRITE', 'GTABLE_SHAPE|SLAB_SHAPE', False),
    ('nulleq842', 'probe_semi', 'ordered'): ('EXACT|ORDERED_EXPANSION|UNIQ_WRITE', 'FAST_WRITE_COOLING|GTABLE_SHAPE|SLAB_SHAPE', False),
    ('packed2222', 'build_anti', 'materialize'): ('EXACT', 'FAST_WRITE_COOLING|GTABLE_COOLING|GTABLE_GAVE_UP|SLAB_SHAPE', False),
    ('packed2222', 'build_anti', 'ordered'): ('EXACT', 'FAST_WRITE_COOLING|GTABLE_COOLING|SLAB_SHAPE', False),
    ('packed2222', 'full_outer', 'materialize'): ('EXACT|GLOBAL_TABLE|UNIQ_WRITE', 'GTABLE_COOLING|GTABLE_GAVE_UP|SLAB_SHAPE', False),
    ('packed2222', 'full_outer', 'ordered'): ('EXACT|SORTED_FK|SORTED_FK_WIDE|SORTED_WRITE|UNIQ_WRITE', 'GTABLE_SHAPE|SLAB_SHAPE', False),
    ('packed2222', 'inner', 'materialize'): ('EXACT|GLOBAL_TABLE|UNIQ_WRITE', 'GTABLE_COOLING|GTABLE_GAVE_UP|SLAB_SHAPE', False),
    ('packed2222', 'inner', 'ordered'): ('EXACT|SORTED_FK|SORTED_FK_WIDE|SORTED_WRITE|UNIQ_WRITE', 'GTABLE_SHAPE|SLAB_SHAPE', False),
    ('packed2222', 'probe_semi', 'materialize'): ('EXACT|GLOBAL_TABLE|UNIQ_WRITE', 'GTABLE_COOLING|GTABLE_GAVE_UP|SLAB_SHAPE', False),
    ('packed2222', 'probe_semi', 'ordered'): ('EXACT|GLOBAL_TABLE|UNIQ_WRITE', 'GTABLE_COOLING|SLAB_SHAPE', False),
    ('packed44', 'build_anti', 'materialize'): ('CHUNKED_BUILD|DENSE_BUILD|EXACT|GLOBAL_TABLE|HOT_KEY_HINT|PRESORTED|UNIQ_WRITE', 'FAST_WRITE_COOLING|GTABLE_COOLING|GTABLE_GAVE_UP|GTABLE_SHAPE|SLAB_SHAPE|SLAB_SORTED_INPUT', False),
    ('packed44', 'build_anti', 'ordered'): ('CHUNKED_BUILD|DENSE_BUILD|EXACT|GLOBAL_TABLE|HOT_KEY_HINT|PRESORTED|UNIQ_WRITE', 'FAST_WRITE_COOLING|GTABLE_COOLING|GTABLE_SHAPE|SLAB_SHAPE|SLAB_SORTED_INPUT', False),
    ('packed44', 'full_outer', 'materialize'): ('CHUNKED_BUILD|DENSE_BUILD|EXACT|GLOBAL_TABLE|HOT_KEY_HINT|ORDERED_EXPANSION|PRESORTED|SPLIT|UNIQ_WRITE', 'GTABLE_COOLING|GTABLE_GAVE_UP|GTABLE_SHAPE|SLAB_SHAPE|SLAB_SORTED_INPUT', False),
    ('packed44', 'full_outer', 'ordered'): ('CHUNKED_BUILD|DENSE_BUILD|EXACT|GLOBAL_TABLE|HOT_KEY_HINT|KEY_RANGES|ORDERED_EXPANSION|ORDER_BY_RANK_SORT|ORDER_DEFERRED|PRESORTED|RANK_LOOKUP_IN_PASS|RANK_RUNS|SLAB|SORTED_FK|SORTED_FK_WIDE|SORTED_WRITE|SPLIT|UNIQ_WRITE', 'EXPANSION_GAVE_UP|FAST_WRITE_COOLING|GTABLE_SHAPE|SLAB_SHAPE|SLAB_SORTED_INPUT', True),
    ('packed44', 'inner', 'materialize'): ('CHUNKED_BUILD|DENSE_BUILD|EXACT|GLOBAL_TABLE|HOT_KEY_HINT|ORDERED_EXPANSION|PRESORTED|SPLIT|UNIQ_WRITE', 'GTABLE_COOLING|GTABLE_GAVE_UP|GTABLE_SHAPE|SLAB_SHAPE|SLAB_SORTED_INPUT', False),
    ('packed44', 'inner', 'ordered'): ('CHUNKED_BUILD|DENSE_BUILD|EXACT|GLOBAL_TABLE|HOT_KEY_HINT|KEY_RANGES|ORDERED_EXPANSION|ORDER_BY_RANK_SORT|ORDER_DEFERRED|PRESORTED|RANK_LOOKUP_IN_PASS|RANK_RUNS|SLAB|SORTED_FK|SORTED_FK_WIDE|SORTED_WRITE|SPLIT|UNIQ_WRITE', 'EXPANSION_GAVE_UP|FAST_WRITE_COOLING|GTABLE_SHAPE|SLAB_SHAPE|SLAB_SORTED_INPUT', True),
    ('packed44', 'probe_semi', 'materialize'): ('CHUNKED_BUILD|DENSE_BUILD|EXACT|GLOBAL_TABLE|HOT_KEY_HINT|PRESORTED|SPLIT|UNIQ_WRITE', 'GTABLE_COOLING|GTABLE_GAVE_UP|GTABLE_SHAPE|SLAB_SHAPE|SLAB_SORTED_INPUT', False),
    ('packed44', 'probe_semi', 'ordered'): ('CHUNKED_BUILD|DENSE_BUILD|EXACT|GLOBAL_TABLE|HOT_KEY_HINT|PRESORTED|SPLIT|UNIQ_WRITE', 'FAST_WRITE_COOLING|GTABLE_COOLING|GTABLE_SHAPE|SLAB_SHAPE|SLAB_SORTED_INPUT', False),
    ('packed8', 'build_anti', 'materialize'): ('EXACT|HOT_KEY_HINT|PRESORTED|UNIQ_WRITE', 'FAST_WRITE_COOLING|GTABLE_COOLING|GTABLE_GAVE_UP|GTABLE_SHAPE|SLAB_SHAPE|SLAB_SORTED_INPUT', False),
    ('packed8', 'build_anti', 'ordered'): ('EXACT|HOT_KEY_HINT|PRESORTED|UNIQ_WRITE', 'FAST_WRITE_COOLING|GTABLE_COOLING|GTABLE_SHAPE|SLAB_SHAPE|SLAB_SORTED_INPUT', False),
    ('packed8', 'full_outer', 'materialize'): ('EXACT|GLOBAL_TABLE|ORDERED_EXPANSION|PRESORTED|UNIQ_WRITE', 'GTABLE_COOLING|GTABLE_GAVE_UP|GTABLE_SHAPE|SLAB_SHAPE|SLAB_SORTED_INPUT', False),
    ('packed8', 'full_outer', 'ordered'): ('EXACT|GLOBAL_TABLE|ORDERED_EXPANSION|ORDER_BY_RANK_SORT|PRESORTED|RANK_LOOKUP_IN_PASS|RANK_RUNS|SLAB|SORTED_FK|SORTED_FK_WIDE|SORTED_WRITE|UNIQ_WRITE', 'GTABLE_SHAPE|SLAB_SHAPE|SLAB_SORTED_INPUT', False),
    ('packed8', 'inner', 'materialize'): ('EXACT|GLOBAL_TABLE|ORDERED_EXPANSION|PRESORTED|UNIQ_WRITE', 'GTABLE_COOLING|GTABLE_GAVE_UP|GTABLE_SHAPE|SLAB_SHAPE|SLAB_SORTED_INPUT', False),
    ('packed8', 'inner', 'ordered'): ('EXACT|GLOBAL_TABLE|ORDERED_EXPANSION|ORDER_BY_RANK_SORT|PRESORTED|RANK_LOOKUP_IN_PASS|RANK_RUNS|SLAB|SORTED_FK|SORTED_FK_WIDE|SORTED_WRITE|UNIQ_WRITE', 'GTABLE_SHAPE|SLAB_SHAPE|SLAB_SORTED_INPUT', False),
    ('packed8', 'probe_semi', 'materialize'): ('EXACT|GLOBAL_TABLE|PRESORTED|UNIQ_WRITE', 'GTABLE_COOLING|GTABLE_GAVE_UP|GTABLE_SHAPE|SLAB_SHAPE|SLAB_SORTED_INPUT', False),
    ('packed8', 'probe_semi', 'ordered'): ('EXACT|GLOBAL_TABLE|PRESORTED|UNIQ_WRITE', 'FAST_WRITE_COOLING|GTABLE_COOLING|GTABLE_SHAPE|SLAB_SHAPE|SLAB_SORTED_INPUT', False),
    ('str', 'build_anti', 'materialize'): ('EXACT|HOT_KEY_HINT|ORDERED_EXPANSION|UNIQ_WRITE', 'GTABLE_GAVE_UP|GTABLE_SHAPE|SLAB_SHAPE', False),
    ('str', 'build_anti', 'ordered'): ('EXACT|HOT_KEY_HINT|ORDERED_EXPANSION|UNIQ_WRITE', 'FAST_WRITE_COOLING|GTABLE_COOLING|GTABLE_SHAPE|SLAB_SHAPE', False),
    ('str', 'full_outer', 'materialize'): ('EXACT|GLOBAL_TABLE|HOT_KEY_HINT|ORDERED_EXPANSION|SPLIT|UNIQ_WRITE', 'GTABLE_GAVE_UP|GTABLE_SHAPE|SLAB_SHAPE', False),
    ('str', 'full_outer', 'ordered'): ('EXACT|GLOBAL_TABLE|HOT_KEY_HINT|ORDERED_EXPANSION|ORDER_BY_RANK_SORT|ORDER_DEFERRED|RANK_RUNS|SLAB|SORTED_FK|SORTED_FK_WIDE|SORTED_WRITE|SPLIT|UNIQ_WRITE', 'EXPANSION_GAVE_UP|FAST_WRITE_COOLING|GTABLE_SHAPE|SLAB_SHAPE', True),
    ('str', 'inner', 'materialize'): ('EXACT|GLOBAL_TABLE|HOT_KEY_HINT|ORDERED_EXPANSION|SPLIT|UNIQ_WRITE', 'GTABLE_COOLING|GTABLE_GAVE_UP|GTABLE_SHAPE|SLAB_SHAPE', False),
    ('str', 'inner', 'ordered'): ('EXACT|GLOBAL_TABLE|HOT_KEY_HINT|ORDERED_EXPANSION|ORDER_BY_RANK_SORT|ORDER_DEFERRED|RANK_RUNS|SLAB|SORTED_FK|SORTED_FK_WIDE|SORTED_WRITE|SPLIT|UNIQ_WRITE', 'EXPANSION_GAVE_UP|FAST_WRITE_COOLING|GTABLE_SHAPE|SLAB_SHAPE', True),
    ('str', 'probe_semi', 'materialize'): ('EXACT|GLOBAL_TABLE|HOT_KEY_HINT|ORDERED_EXPANSION|SPLIT|UNIQ_WRITE', 'GTABLE_SHAPE|SLAB_SHAPE', False),
    ('str', 'probe_semi', 'ordered'): ('EXACT|GLOBAL_TABLE|HOT_KEY_HINT|ORDERED_EXPANSION|SPLIT|UNIQ_WRITE', 'FAST_WRITE_COOLING|GTABLE_SHAPE|SLAB_SHAPE', False),
}


def bits_of(H, prefix, names):
    out = 0
    for n in filter(None, names.split("|")):
        out |= getattr(H._lib, prefix + n)
    return out


def test_zz_ledger(H):
    seen = {k: (path_names(H, e["path"]), refused_names(H, e["refused"]), bool(e["replanned"])) for k, e in sorted(LEDGER.items())}
    print("key-join plan ledger (%d cases):" % len(CASES_RUN))
    for k, v in seen.items():
        print("    %r: %r," % (k, v), flush=True)
    print("grouping's sorts:", {k: path_names(H, v) for k, v in GROUP_SORTS.items()}, flush=True)
    never = bits_of(H, "HMJ_PATH_", "|".join(NEVER))
    for k, e in LEDGER.items():
        assert not e["path"] & never, (k, seen[k])
    # the rest holds for a run of the whole file: a case that did not run, or did not get to its end, is a failure here too
    assert len(CASES_RUN) == N_CASES and sorted(GROUP_SORTS) == sorted(GROUP_SHAPES), (
        "the ledger is asserted by a run of the whole file: %d of %d cases and %d of %d group shapes ran" % (
            len(CASES_RUN), N_CASES, len(GROUP_SORTS), len(GROUP_SHAPES)), sorted(CASES_RUN))
    for form in ("packed", "hashed"):
        path = refused = 0
        for (fam, _, _), e in LEDGER.items():
            if FAMILIES[fam][1] == form and fam != "packed2222":
                path |= e["path"]
                refused |= e["refused"]
        for alt in MINIMUM:
            assert alt in EXCUSED[form] or path & bits_of(H, "HMJ_PATH_", alt), (form, alt, path_names(H, path))
        for name in REFUSALS:
            assert refused & bits_of(H, "HMJ_REFUSED_", name), (form, name, refused_names(H, refused))
    sorts = 0
    for path in GROUP_SORTS.values():
        sorts |= path
    assert sorts & H.HMJ_PATH_SORT_MSD and sorts & H.HMJ_PATH_SLAB, {k: path_names(H, v) for k, v in GROUP_SORTS.items()}
    assert sorted(LEDGER) == sorted(OBSERVED)
    for k, (paths, refusals, replanned) in OBSERVED.items():
        e = LEDGER[k]
        keep = ~bits_of(H, "HMJ_PATH_", UNSTABLE.get(k[0], ""))
        assert (e["path"] & keep, e["refused"], bool(e["replanned"])) == (
            bits_of(H, "HMJ_PATH_", paths) & keep, bits_of(H, "HMJ_REFUSED_", refusals), replanned), (k, seen[k], OBSERVED[k])
