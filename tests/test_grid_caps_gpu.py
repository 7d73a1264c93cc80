"""Every grid-capped kernel of the column operators past its cap, on the GPU (the table and the cases: test_grid_caps_cpu.py).

The sizes come from the device's compute-unit count through `size_past`, and every test first asserts that its population
exceeds the rows one launch takes without a second trip, so a pass always means that second and third trips ran: LDS count
words reused behind a barrier, histograms accumulated over tiles, ballots on a partial last tile with whole inactive waves,
the take kernel's prefetched map entry, ballot words at base >> 6.  The references are hashmergejoin_amd.reference and numpy's
stable sorts; maps and values are compared entry by entry and bit for bit, through the helpers of the operators' own tests."""
import numpy as np
import pytest

import test_grid_caps_cpu as G
from test_group_agg_gpu import aggregate, group as group_by_key
from test_group_cols_gpu import run_and_check as group_cols_check
from test_group_mixed_gpu import run_and_check as group_mixed_check
from test_join_cols_gpu import dev_col
from test_order_by_gpu import H, check as order_check, dev, dev_cols, ex, spec  # noqa: F401  (H and ex are fixtures)
from test_take_cols_gpu import check_take, run_take
from test_top_k_gpu import WINDOW_LEVELS, check as top_k_check

pytestmark = pytest.mark.gpu
HMJ_E_ARG = -1
BOTH = ("select", "full")


@pytest.fixture(scope="module")
def cus():
    import torch

    return int(torch.cuda.get_device_properties(0).multi_processor_count)


@pytest.fixture(scope="module")
def strings(cus):
    return G.string_table(cus)


def past(family, cus, population):
    """The precondition of every test here: the population makes a workgroup of the family's launch take a second trip."""
    assert population > G.cap_rows(family, cus), (family, cus, population, G.cap_rows(family, cus))
    return population


# ---- top-k: column mode (topk_hist_kernel, topk_mark_kernel over the rows) -----------------------------------------------------------
def test_top_k_unique_keys_past_the_cap(ex, H, cus):
    u = G.topk_unique_keys(cus)
    n = past("topk", cus, len(u))
    assert n == G.size_past("topk", cus)
    for offset in (0, n - 10):
        info = top_k_check(ex, H, [spec(u)], 10, offset, "unique u64", plans=BOTH, max_tie_rows=1)["select"]
        assert info["n_candidates"] == min(n, offset + 10) and info["n_rounds"] == 1, info


def test_top_k_shared_top_bits_past_the_cap(ex, H, cus):
    small = G.topk_small_keys(cus)
    past("topk", cus, len(small))
    info = top_k_check(ex, H, [spec(small)], 10, 5, "u64 below 2^10", plans=BOTH, max_tie_rows=1)["select"]
    assert info["n_levels"] == 2 and info["n_candidates"] == 15, info  # every row in one bin, then the ten varying bits


def test_top_k_three_values_past_the_cap(ex, H, cus):
    i8, lo, mid = G.topk_three_values(cus)
    past("topk", cus, len(i8))
    K = lo + mid // 2
    info = top_k_check(ex, H, [spec(i8)], 20, K - 20, "three i8 values", plans=BOTH)["select"]
    assert info["n_levels"] == 1 and info["n_tie_rows"] == mid and info["n_candidates"] == K, info
    got, _ = ex.top_k_device([(dev(i8), 0)], mid // 2, lo, plan="select")
    assert np.array_equal(got.cpu().numpy().view(np.uint64), np.flatnonzero(i8 == 9)[:mid // 2].astype(np.uint64))  # the ties in ascending row index


# ---- top-k: list mode (topk_gather_kernel, hist<LIST>, mark<LIST> over a tie list past the cap) -------------------------------------------
def test_top_k_tie_list_past_the_cap(ex, H, cus):
    case = G.topk_list_case(cus)
    past("topk", cus, case["n"])
    assert case["mid"] > G.cap_rows("topk", cus) + 5 * 256 + 77  # the tie list of window 1: third trips and a partial last tile
    assert G.cut_tie_set(case) == (1, 1)
    K = case["K"]
    info = top_k_check(ex, H, [spec(case["a"]), spec(case["b"])], 10, K - 10, "tie list", plans=BOTH, max_tie_rows=1)["select"]
    assert info["n_levels"] > WINDOW_LEVELS and info["n_candidates"] == K, info


def test_top_k_tie_list_whose_last_level_fits(ex, H, cus):
    # B varies in its top 16 and low 8 bits: the set tied with the cut on the top 16 fits max_tie_rows before a level reaches
    # the low ones, so it is written whole and the final ordering sorts it
    case = G.topk_list_case(cus, "top16+low8")
    past("topk", cus, case["n"])
    assert case["mid"] > G.cap_rows("topk", cus) + 5 * 256 + 77
    ties, taken = G.cut_tie_set(case)
    assert 1 <= taken < ties <= 64, (ties, taken)  # the set fits and is not taken whole
    K = case["K"]
    info = top_k_check(ex, H, [spec(case["a"]), spec(case["b"])], 10, K - 10, "tie list, fits", plans=BOTH, max_tie_rows=64)["select"]
    assert info["n_levels"] == WINDOW_LEVELS + 2 and info["n_candidates"] == K - taken + ties > K and info["n_tie_rows"] == ties, info
    # B varies in its top 16 bits only and no tie is allowed: the tied rows' stream is used up, they are equal in every column,
    # and the first of them by row index are taken
    case = G.topk_list_case(cus, "top16")
    ties, taken = G.cut_tie_set(case)
    assert 1 <= taken < ties and case["mid"] > G.cap_rows("topk", cus) + 5 * 256 + 77
    K = case["K"]
    info = top_k_check(ex, H, [spec(case["a"]), spec(case["b"])], 10, K - 10, "tie list, used up", plans=("select",), max_tie_rows=1)["select"]
    assert info["n_levels"] == WINDOW_LEVELS + 2 and info["n_candidates"] == K and info["n_tie_rows"] == ties, info


# ---- strings past the cap -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [G.NULLS_FIRST, G.DESC], ids=["nulls_first", "desc"])
def test_top_k_strings_past_the_cap(ex, H, cus, strings, flags):
    n = past("topk", cus, strings["n"])
    cols = [spec(*s) for s in G.string_specs(strings, flags)]
    # the cut among the valid strings: they share 20 bytes, so the windows behind the first walk a list of them
    assert int(strings["valid"].sum()) > G.cap_rows("topk", cus) + 5 * 256 + 77
    info = top_k_check(ex, H, cols, 10, n // 2, "strings flags %d" % flags, plans=BOTH, max_tie_rows=1)["select"]
    assert info["n_levels"] > WINDOW_LEVELS, info
    if flags & G.NULLS_FIRST:  # and the cut among the NULL slots, whose streams end behind the marker and the int32
        top_k_check(ex, H, cols, 10, 77, "strings, cut in the NULLs", plans=("select",), max_tie_rows=1)


def test_top_k_refuses_offsets_that_decrease_in_a_later_trip(ex, H, cus, strings):
    n = past("topk", cus, strings["n"])
    later, last = G.bad_offset_rows(cus)
    assert G.cap_rows("topk", cus) * 2 <= later < last < n
    cols = [spec(*s) for s in G.string_specs(strings, G.NULLS_FIRST)]
    dcols = dev_cols(H, cols)
    (chars, offsets), flags, bitmap, bit_offset = dcols[0]
    bad = offsets.clone()
    bad[[last, later]] = bad[[last, later]] + 1000  # offsets[r + 1] < offsets[r] at both; the rows in front stay inside the chars
    bad_cols = [((chars, bad), flags, bitmap, bit_offset), dcols[1]]
    for plan in BOTH:
        with pytest.raises(H.HmjError) as e:
            ex.top_k_device(bad_cols, 10, 0, plan=plan, max_tie_rows=1)
        assert e.value.code == HMJ_E_ARG, str(e.value)
        assert "column 0: offsets decrease at row %d (offsets[%d] < offsets[%d])" % (later, later + 1, later) in str(e.value), str(e.value)
    # the same executor orders the good table right after
    got, info = ex.top_k_device(dcols, 10, 3, plan="select", max_tie_rows=1)
    want = H.expected_top_k([(c["values"], c["flags"], c["valid"]) for c in cols], 10, 3)
    assert np.array_equal(got.cpu().numpy().view(np.uint64), want) and info["plan_taken"] == H.HMJ_TOPK_SELECT, info


# ---- AUTO takes SELECT ------------------------------------------------------------------------------------------------------------------
def test_top_k_auto_takes_select_from_2_to_the_23_rows(ex, H, cus):
    rng = np.random.default_rng(52)
    n = past("topk", cus, 1 << 23)
    vals = rng.integers(0, 1 << 32, size=n, dtype=np.uint32)
    want = np.argsort(vals, kind="stable").astype(np.uint64)
    d = dev(vals)
    got, info = ex.top_k_device([(d, 0)], 10, plan="auto")
    assert info["plan_taken"] == H.HMJ_TOPK_SELECT and info["n_out"] == 10 and 10 <= info["n_candidates"] < n // 256, info
    assert np.array_equal(got.cpu().numpy().view(np.uint64), want[:10])
    k = n // 256 + 1  # a cut beyond the share of the rows up to which selection pays
    got, info = ex.top_k_device([(d, 0)], k, plan="auto")
    assert info["plan_taken"] == H.HMJ_TOPK_FULL and info["n_out"] == k and info["n_candidates"] == n, info
    assert np.array_equal(got.cpu().numpy().view(np.uint64), want[:k])


# ---- ORDER BY ---------------------------------------------------------------------------------------------------------------------------
def test_order_by_second_round_over_a_list_as_long_as_the_input(ex, H, cus):
    a, b = G.order_round2_case(cus)
    n = past("orderby", cus, len(a))
    assert int(np.unique(a, return_counts=True)[1].min()) >= 2  # every row is active after round 1: the list of round 2 holds n rows
    _, info = order_check(ex, H, [spec(a), spec(b)], "round 2 over every row")
    assert info["n_rounds"] == 2 and info["n_distinct"] == n and info["n_tied_rows"] == 0, info


@pytest.mark.parametrize("flags", [G.NULLS_FIRST, G.DESC], ids=["nulls_first", "desc"])
def test_order_by_strings_past_the_cap(ex, H, cus, strings, flags):
    past("orderby", cus, strings["n"])
    assert int(strings["valid"].sum()) > G.cap_rows("orderby", cus)  # the rows still active behind round 1
    _, info = order_check(ex, H, [spec(*s) for s in G.string_specs(strings, flags)], "strings flags %d" % flags)
    assert info["n_rounds"] >= 3 and info["n_tied_rows"] > 0, info


# ---- take_cols -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("widths", G.TAKE_SHAPES, ids=lambda w: "%dcols" % len(w))
def test_take_cols_past_the_cap(ex, H, cus, widths):
    case = G.take_case(cus, widths)
    n_out = past("take", cus, len(case["good"]))
    assert n_out == G.size_past("take", cus) and max(case["positions"]) == n_out - 1
    # entries beyond the source in the first tile, in a third-trip tile and in the partial last wave: counted, never loaded through
    with pytest.raises(H.HmjError) as e:
        run_take(H, ex, case["cols"], case["masks"], case["bad"], offs=67)
    assert e.value.code == HMJ_E_ARG and ("%d row_map entries" % case["n_bad"]) in str(e.value), str(e.value)
    info = check_take(H, ex, case["cols"], case["masks"], case["good"], offs=67, wants=True, tag=("past the cap", len(widths)))
    assert info["n_no_row"] == int((case["good"] == G.NO_ROW).sum()) > n_out // 10


# ---- group_agg: the finish kernel ----------------------------------------------------------------------------------------------------------
def test_group_agg_finish_past_the_cap(ex, H, cus):
    case = G.agg_case(cus)
    ng = past("agg_finish", cus, case["ng"])
    res, cols = group_by_key(ex, H, case["key"], ordered=True)
    assert int(res.n_groups) == ng and np.array_equal(cols["group_of_row"], case["key"])  # group g is key g
    assert cols["count"][case["three"]].tolist() == [3] * len(case["three"]) and int(cols["count"].sum()) == len(case["key"])
    aggs = G.agg_list(H, case)
    got = aggregate(ex, H, aggs, ng)  # (the words' count and their padding bits are checked there)
    want = H.expected_group_aggs(cols["group_of_row"], ng, aggs)
    G.assert_aggs_vectorised(H, got, want, aggs, ng, "finish past the cap")
    for (v, ok, nulls), w in zip(got, want):
        assert nulls == w["null_count"] and np.array_equal(ok, w["valid"])
    assert not got[0][1][case["none"]].any() and got[3][0][case["none"]].tolist() == [0] * len(case["none"])


# ---- the multi-column key kernels ------------------------------------------------------------------------------------------------------------
def test_group_cols_keys_past_the_cap(ex, H, cus):
    cols, valid = G.key_group_case(cus)
    past("col_keys", cus, len(cols[0]))
    _, info, _, exp = group_cols_check(H, ex, cols, G.KEY_WIDTHS, None, valid, ordered=True, tag="keys past the cap", offset=3)
    assert info["form"] == H.HMJ_COLS_HASHED and exp["n_null"] > 0 and exp["max_count"] >= 3


def join_and_compare(ex, H, bcols, pcols, want, pairs, **kw):
    res, info = ex.join_cols_device([dev_col(c) for c in bcols], None, [dev_col(c) for c in pcols], None, H.HMJ_ORDERED | H.HMJ_CHECKSUM | kw.pop("flags", 0),
                                    **kw)
    got = ex.cols_rows_to_numpy(res)
    assert int(res.n_matches) == len(want) and got.shape == want.shape, (int(res.n_matches), got.shape, want.shape)
    bad = np.flatnonzero(np.any(got != want, axis=1))
    assert not len(bad), (bad[:5], got[bad[:3]], want[bad[:3]])
    assert info["form"] == H.HMJ_COLS_HASHED and info["n_key_pairs"] == pairs and info["n_collisions"] == pairs - len(want), (info, pairs, len(want))
    return info


@pytest.mark.parametrize("null_equal", [False, True], ids=["null_keys", "null_equal"])
def test_join_cols_keys_past_the_cap(ex, H, cus, null_equal):
    bcols, bvalid, pcols, pvalid = G.key_join_case(cus)
    n = past("col_keys", cus, len(bcols[0]))
    assert len(pcols[0]) == n
    if null_equal:  # both sides through the kernel that keys NULL slots
        want, pairs = G.expected_inner_join(H, bcols, pcols, G.KEY_WIDTHS, bvalid, pvalid, 0, True)
        info = join_and_compare(ex, H, bcols, pcols, want, pairs, flags=H.HMJ_NULL_EQUAL,
                                build_valid=[None, (H.pack_validity(bvalid[1], 3, "cuda"), 3)], probe_valid=[None, (H.pack_validity(pvalid[1], 67, "cuda"), 67)])
        assert info["n_build_null"] == int((~bvalid[1]).sum()) and int((~pvalid[1][want[:, 2].astype(np.int64)]).sum()) > 0
    else:  # a bitmap on the probe side only: the build side takes the plain key kernel
        want, pairs = G.expected_inner_join(H, bcols, pcols, G.KEY_WIDTHS, None, pvalid)
        info = join_and_compare(ex, H, bcols, pcols, want, pairs, probe_valid=[None, (H.pack_validity(pvalid[1], 67, "cuda"), 67)])
        assert info["n_build_null"] == 0
    assert info["n_probe_null"] == int((~pvalid[1]).sum()) > n // 50 and len(want) > n // 2


# ---- the collision sort ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=sorted(G.COLLISION_SHAPES))
def collisions(request, H, cus):
    """A collision shape with its run structure: (name, parameters, cols, ids, mixed runs, list entries)."""
    p = G.COLLISION_SHAPES[request.param]
    cols, ids = G.collision_case(p["n_tuples"], p["n_extra"])
    runs, longest, entries = G.run_shape(H.cols_key64(cols, G.KEY_WIDTHS, p["hash_bits"]), ids)
    assert 1 < longest <= G.RUN_CAP
    if request.param == "runs":  # more list entries than workgroups, and more led runs: several sorts per workgroup
        assert entries > G.rows_past(G.cap_of("run_sort", cus), 1) and runs > G.cap_of("run_sort", cus), (entries, runs, cus)
    else:  # the leader kernel strides
        assert entries > G.cap_rows("run_leader", cus) + 5 * 256 + 77, (entries, cus)
    return request.param, p, cols, ids, runs, entries


@pytest.mark.parametrize("ordered", [False, True], ids=["unordered", "ordered"])
def test_group_collision_sort_past_the_cap(ex, H, collisions, ordered):
    name, p, cols, ids, runs, entries = collisions
    _, info, _, exp = group_cols_check(H, ex, cols, G.KEY_WIDTHS, None, None, ordered=ordered, tag=(name, ordered), hash_bits=p["hash_bits"])
    assert exp["n_groups"] == p["n_tuples"] and info["n_collisions"] == p["n_tuples"] - runs
    if name == "runs" or not ordered:  # (the longer shape: the column entry ordered, the mixed entry unordered)
        _, info, _, exp = group_mixed_check(H, ex, cols, None, None, ordered=ordered, tag=(name, "mixed", ordered), hash_bits=p["hash_bits"])
        assert exp["n_groups"] == p["n_tuples"] and info["n_collisions"] == p["n_tuples"] - runs


def test_join_collision_sort_past_the_cap(ex, H, cus, collisions):
    name, p, cols, ids, runs, entries = collisions
    a, b, _ = G.tuple_of_id(np.random.default_rng(53).permutation(p["n_tuples"]))
    # every tuple is in the result and every run of equal key64 holds as many tuples as the relation's: the list is as long at least
    at_least = p["n_tuples"] - runs
    assert at_least > (G.cap_rows("run_leader", cus) if name == "leader" else G.rows_past(G.cap_of("run_sort", cus), 1)), (at_least, cus)
    want, pairs = G.expected_inner_join(H, [a, b], cols, G.KEY_WIDTHS, hash_bits=p["hash_bits"])
    assert len(want) == len(ids) and pairs > len(want)
    join_and_compare(ex, H, [a, b], cols, want, pairs, hash_bits=p["hash_bits"])
