"""CPU-only checks of hmj_group_cols_device (include/hmj.h, "grouping rows by multi-column keys"): the library exports the
entry and refuses a NULL ctx, the two new structs have the layout the ctypes mirrors assume and the ABI version is
unchanged, and `expected_groups` -- the numpy reference test_group_cols_gpu.py compares the device with -- agrees with a
brute-force dict-of-tuples model.  Also here: the draws of the GPU file's randomized sweep (`draw_case`), so that the cap on
skipped draws is checked from `cols_key64` alone."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M64 = (1 << 64) - 1
HMJ_E_ARG = -1
SWEEP_SEED, SWEEP_ITERS, SWEEP_MAX_SKIPS = 20261019, 30, 3  # HMJ_STRESS_SEED / HMJ_STRESS_ITERS override the first two
RUN_CAP = 1024  # rows of a run of equal key64 with several tuples that one workgroup sorts


# ---- the entry and its structs -----------------------------------------------------------------------------------------------
def test_the_library_exports_the_entry_and_refuses_a_null_ctx():
    import hashmergejoin_amd as H

    L = H.load_library()
    assert hasattr(L, "hmj_group_cols_device")
    rel, opts, res = H.ColsRel(), H.GroupOpts(), H.GroupResult()
    opts.struct_size = C.sizeof(H.GroupOpts)
    assert L.hmj_group_cols_device(None, C.byref(rel), 0, C.byref(opts), C.byref(res)) == HMJ_E_ARG
    for name in ("GroupOpts", "GroupResult", "HMJ_GROUP_COUNT", "HMJ_GROUP_SUM", "HMJ_GROUP_MIN", "HMJ_GROUP_MAX", "HMJ_GROUP_ROW_MAP",
                 "expected_groups"):
        assert name in H.__all__ and hasattr(H, name)
    assert hasattr(H.Executor, "group_cols_device") and hasattr(H.Executor, "group_rows_to_numpy")


def test_struct_layouts_match_the_header_and_the_abi_version_stays():
    import hashmergejoin_amd as H

    opts_fields = ["struct_size", "want", "hash_bits", "force_hashed", "form", "reserved", "validity", "n_null", "n_collisions",
                   "ms_key", "ms_sort", "ms_groups", "ms_agg"]
    res_fields = ["n_groups", "n_rows", "max_count", "key64", "first_row", "count", "sum", "min", "max", "group_of_row"]
    lines = ['std::printf("sizeof_opts %zu\\nsizeof_res %zu\\n", sizeof(hmj_group_opts), sizeof(hmj_group_result));']
    lines += ['std::printf("opts.%s %%zu\\n", offsetof(hmj_group_opts, %s));' % (f, f) for f in opts_fields]
    lines += ['std::printf("res.%s %%zu\\n", offsetof(hmj_group_result, %s));' % (f, f) for f in res_fields]
    lines += ['std::printf("want %u %u %u %u %u\\nabi %d\\n", HMJ_GROUP_COUNT, HMJ_GROUP_SUM, HMJ_GROUP_MIN, HMJ_GROUP_MAX, '
              'HMJ_GROUP_ROW_MAP, HMJ_ABI_VERSION);']
    src = '#include <cstddef>\n#include <cstdio>\n#include "hmj.h"\nint main() {\n%s\nreturn 0;\n}\n' % "\n".join(lines)
    with tempfile.TemporaryDirectory() as d:
        cc, exe = os.path.join(d, "layout.cc"), os.path.join(d, "layout")
        open(cc, "w").write(src)
        subprocess.check_call(["g++", "-std=c++11", "-I", os.path.join(ROOT, "include"), cc, "-o", exe])
        got = {}
        for line in subprocess.check_output([exe]).decode().splitlines():
            k, *v = line.split()
            got[k] = [int(x) for x in v]
    assert got["sizeof_opts"] == [C.sizeof(H.GroupOpts)] and got["sizeof_res"] == [C.sizeof(H.GroupResult)]
    assert [f for f, _ in H.GroupOpts._fields_] == opts_fields and [f for f, _ in H.GroupResult._fields_] == res_fields
    for f in opts_fields:
        assert got["opts." + f] == [getattr(H.GroupOpts, f).offset], f
    for f in res_fields:
        assert got["res." + f] == [getattr(H.GroupResult, f).offset], f
    assert got["want"] == [H.HMJ_GROUP_COUNT, H.HMJ_GROUP_SUM, H.HMJ_GROUP_MIN, H.HMJ_GROUP_MAX, H.HMJ_GROUP_ROW_MAP] == [1, 2, 4, 8, 16]
    assert got["abi"] == [5]  # a new entry with structs of its own: nothing existing changed
    assert H.load_library().hmj_abi_version() == 5


# ---- the reference against a brute-force model ---------------------------------------------------------------------------------
def tuples_of(columns, widths, valid):
    """The rows' key tuples in plain integers, None in a NULL slot."""
    n = len(columns[0])
    cols = []
    for c, (col, w) in enumerate(zip(columns, widths)):
        a = np.ascontiguousarray(col)
        if a.dtype.itemsize == w and a.dtype.kind != "u":
            a = a.view("u%d" % w)
        v = [int(x) & ((1 << (8 * w)) - 1) for x in a]
        ok = None if valid is None or valid[c] is None else valid[c]
        cols.append([None if (ok is not None and not ok[i]) else v[i] for i in range(n)])
    return list(zip(*cols))


def null_last(t):
    return tuple((1, 0) if v is None else (0, v) for v in t)


def brute_groups(H, columns, widths, vals, valid, hash_bits=0, force_hashed=False, ordered=False):
    """Groups by a dict of tuples: plain tuple equality is the grouping rule (None equals None and nothing else)."""
    tup = tuples_of(columns, widths, valid)
    bitmap = valid is not None and any(v is not None for v in valid)
    if bitmap:
        key = H.cols_key64(columns, widths, hash_bits, valid=valid, null_equal=True)
    else:
        key = H.cols_key64(columns, widths, hash_bits, force_hashed)
    groups = {}
    for i, t in enumerate(tup):
        groups.setdefault(t, []).append(i)
    order = list(groups)  # by first row
    if ordered:
        order.sort(key=lambda t: (int(key[groups[t][0]]), null_last(t)))
    pay = list(range(len(tup))) if vals is None else [int(v) & M64 for v in vals]
    index = {t: g for g, t in enumerate(order)}
    return {"n_groups": len(order), "max_count": max((len(groups[t]) for t in order), default=0),
            "n_null": sum(1 for t in tup if None in t),
            "n_collisions": len(order) - len({int(key[groups[t][0]]) for t in order}),
            "key64": [int(key[groups[t][0]]) for t in order], "first_row": [groups[t][0] for t in order],
            "count": [len(groups[t]) for t in order], "sum": [sum(pay[i] for i in groups[t]) & M64 for t in order],
            "min": [min(pay[i] for i in groups[t]) for t in order], "max": [max(pay[i] for i in groups[t]) for t in order],
            "group_of_row": [index[t] for t in tup]}


def assert_same(got, want, tag=""):
    for k, v in want.items():
        g = got[k]
        assert (g.tolist() if hasattr(g, "tolist") else g) == v, (tag, k)


def draw_columns(rng, n, widths, card):
    """n rows over `card` distinct tuples (at most; drawn with repeats), as unsigned columns of the given widths."""
    pool = [rng.integers(0, 1 << min(8 * w, 63), size=card, dtype=np.uint64) & np.uint64((1 << (8 * w)) - 1) for w in widths]
    pick = rng.integers(0, card, size=n)
    return [p[pick].astype("u%d" % w) for p, w in zip(pool, widths)]


def draw_valid(rng, n, k, density, which):
    """Validity per column: None (no bitmap) for the columns outside `which`, else n bools with about `density` NULLs."""
    return [(rng.random(n) >= density) if c in which else None for c in range(k)]


def test_expected_groups_agrees_with_a_dict_of_tuples():
    import hashmergejoin_amd as H

    rng = np.random.default_rng(20261019)
    shapes = [([1], 0), ([8], 0), ([4, 4], 0), ([2, 2, 2, 2], 0), ([4, 4], 1), ([8, 4, 2], 0), ([8] * 8, 0)]
    for widths, forced in shapes:
        for n, card, density in ((1, 1, 0.0), (65, 7, 0.0), (300, 40, 0.1), (257, 300, 0.5)):
            cols = draw_columns(rng, n, widths, card)
            vals = rng.integers(0, 1 << 64, size=n, dtype=np.uint64) if n % 2 else None
            which = set(range(len(widths))) if density else set()
            valid = draw_valid(rng, n, len(widths), density, which) if which else None
            for bits in (0, 3):
                for ordered in (False, True):
                    got = H.expected_groups(cols, widths, vals, valid, bits, bool(forced), ordered)
                    want = brute_groups(H, cols, widths, vals, valid, bits, bool(forced), ordered)
                    assert_same(got, want, (widths, n, bits, ordered))
                    hashed = sum(widths) > 8 or forced or valid is not None
                    assert got["form"] == (H.HMJ_COLS_HASHED if hashed else H.HMJ_COLS_PACKED)
    e = H.expected_groups([np.zeros(0, np.uint32)], [4])
    assert e["n_groups"] == 0 and e["max_count"] == 0 and len(e["key64"]) == 0 and len(e["group_of_row"]) == 0


def test_null_slots_are_values_of_their_own():
    import hashmergejoin_amd as H

    a, b = np.array([0, 0, 7, 5], np.uint32), np.array([5, 5, 5, 7], np.uint32)
    # rows: (NULL, 5), (0, 5), (7, 5) and (5, NULL) / (NULL-under-7 ...): the first column's row 0 and the second's row 3 are NULL
    valid = [np.array([0, 1, 1, 1], bool), np.array([1, 1, 1, 0], bool)]
    e = H.expected_groups([a, b], [4, 4], None, valid)
    assert e["n_groups"] == 4 and e["n_null"] == 2 and e["form"] == H.HMJ_COLS_HASHED  # (NULL, 5) is not (0, 5)
    # (NULL, x) and (x, NULL) differ
    x = np.array([9, 9], np.uint32)
    e = H.expected_groups([x, x], [4, 4], None, [np.array([0, 1], bool), np.array([1, 0], bool)])
    assert e["n_groups"] == 2 and e["group_of_row"].tolist() == [0, 1]
    # two NULLs of one column are one group, whatever lies under them
    e = H.expected_groups([np.array([1, 2, 3], np.uint32)], [4], [10, 20, 30], [np.array([0, 1, 0], bool)])
    assert e["n_groups"] == 2 and e["first_row"].tolist() == [0, 1] and e["sum"].tolist() == [40, 20]
    # an all-valid bitmap changes the form, not the groups
    plain = H.expected_groups([a, b], [4, 4])
    withmap = H.expected_groups([a, b], [4, 4], None, [np.ones(4, bool), None])
    assert plain["form"] == H.HMJ_COLS_PACKED and withmap["form"] == H.HMJ_COLS_HASHED
    for k in ("first_row", "count", "group_of_row"):
        assert plain[k].tolist() == withmap[k].tolist()


def test_garbage_under_null_slots_changes_nothing():
    import hashmergejoin_amd as H

    rng = np.random.default_rng(5)
    widths = [8, 4, 2]
    cols = draw_columns(rng, 500, widths, 30)
    valid = draw_valid(rng, 500, 3, 0.2, {0, 2})
    want = H.expected_groups(cols, widths, None, valid, ordered=True)
    dirty = [c.copy() for c in cols]
    for c in (0, 2):
        junk = rng.integers(0, 1 << 16, size=500).astype(dirty[c].dtype)
        dirty[c][~valid[c]] = junk[~valid[c]]
    got = H.expected_groups(dirty, widths, None, valid, ordered=True)
    for k, v in want.items():
        assert (got[k].tolist() if hasattr(v, "tolist") else got[k]) == (v.tolist() if hasattr(v, "tolist") else v), k


def test_a_bitmap_at_a_bit_offset_gives_the_same_groups():
    """pack_validity at offsets 0, 3 and 67 holds the same rows; read back from its offset, the groups are the same."""
    import hashmergejoin_amd as H

    rng = np.random.default_rng(67)
    widths = [4, 2]
    cols = draw_columns(rng, 333, widths, 20)
    mask = rng.random(333) >= 0.15
    base = H.expected_groups(cols, widths, None, [mask, None], ordered=True)
    for off in (0, 3, 67):
        packed = H.pack_validity(mask, off).numpy()
        bits = np.unpackbits(packed, bitorder="little")[off:off + 333].astype(bool)
        got = H.expected_groups(cols, widths, None, [bits, None], ordered=True)
        for k in ("key64", "first_row", "count", "group_of_row"):
            assert got[k].tolist() == base[k].tolist(), (off, k)


def test_ordered_groups_equal_a_lexsort_with_nulls_last():
    import hashmergejoin_amd as H

    rng = np.random.default_rng(11)
    # packed: plainly ascending tuple order
    a, b = rng.integers(0, 5, 200).astype(np.uint16), rng.integers(0, 5, 200).astype(np.uint32)
    e = H.expected_groups([a, b], [2, 4], ordered=True)
    tup = sorted(set(zip(a.tolist(), b.tolist())))
    assert e["key64"].tolist() == [(x << 32) | y for x, y in tup]
    # hashed with NULLs: (key64, then per column (is NULL, value)) through numpy.lexsort
    widths = [8, 4, 2]
    cols = draw_columns(rng, 400, widths, 50)
    valid = draw_valid(rng, 400, 3, 0.3, {0, 1, 2})
    e = H.expected_groups(cols, widths, None, valid, hash_bits=2, ordered=True)
    first = e["first_row"].astype(np.int64)
    keys = []
    for c in range(3):
        null = ~valid[c][first]
        keys += [null, np.where(null, 0, cols[c][first].astype(np.uint64))]
    keys = [e["key64"]] + keys
    assert np.lexsort(tuple(reversed(keys))).tolist() == list(range(len(first)))
    assert e["n_collisions"] > 0  # four values of key64 over 50 tuples: the tuple order inside a key64 is exercised


# ---- the randomized sweep's draws (shared with test_group_cols_gpu.py) ----------------------------------------------------------
def draw_case(rng):
    """One draw of the sweep: n <= 2^16 rows, 1-8 columns of drawn widths, drawn cardinality and NULL density, hash_bits in
    {0, 0, 0, 20, 8}, payloads or none, drawn flags.  Returns a dict of numpy inputs."""
    n = int(rng.choice([1, 2, 63, 64, 65, 255, 256, 257, 1023, 1025, 4097, 20000, 65536]))
    if rng.random() < 0.5:
        n = int(rng.integers(1, (1 << 16) + 1))
    k = int(rng.integers(1, 9))
    widths = [int(w) for w in rng.choice([1, 2, 4, 8], size=k)]
    card = int(rng.choice([1, 3, 17, 300, 5000, 1 << 16]))
    cols = draw_columns(rng, n, widths, card)
    density = float(rng.choice([0.0, 0.0, 0.01, 0.1, 0.9]))
    which = {c for c in range(k) if rng.random() < 0.5} if density else set()
    valid = draw_valid(rng, n, k, density, which) if which else None
    vals = rng.integers(0, 1 << 64, size=n, dtype=np.uint64) if rng.random() < 0.6 else None
    return {"n": n, "widths": widths, "cols": cols, "valid": valid, "vals": vals, "hash_bits": int(rng.choice([0, 0, 0, 20, 8])),
            "force_hashed": bool(rng.random() < 0.3), "ordered": bool(rng.random() < 0.5), "offset": int(rng.choice([0, 3, 67]))}


def sweep_params():
    return int(os.environ.get("HMJ_STRESS_SEED", SWEEP_SEED)), int(os.environ.get("HMJ_STRESS_ITERS", SWEEP_ITERS))


def exceeds_run_cap(H, case):
    """From key64 and the tuples alone: the call holds a run of equal key64 with several tuples and more than 1024 rows."""
    e = H.expected_groups(case["cols"], case["widths"], None, case["valid"], case["hash_bits"], case["force_hashed"])
    return e["form"] == H.HMJ_COLS_HASHED and e["max_mixed_run"] > RUN_CAP


def test_the_default_sweep_skips_at_most_three_draws():
    import hashmergejoin_amd as H

    rng = np.random.default_rng(SWEEP_SEED)
    skipped = sum(exceeds_run_cap(H, draw_case(rng)) for _ in range(SWEEP_ITERS))
    assert skipped <= SWEEP_MAX_SKIPS, skipped
