"""CPU-only checks of hmj_group_mixed_device (include/hmj.h, "grouping rows by string and mixed keys"): the library exports
the entry and refuses a NULL ctx, the ABI version and the two group structs are unchanged, and `expected_mixed_groups` -- the
host reference test_group_mixed_gpu.py compares the device with -- agrees with a brute-force dict of canonical tuples and,
on fixed columns only, with `expected_groups(..., force_hashed=True)`.  Also here: the draws of the GPU file's randomized
sweep (`draw_case`), so that the cap on draws beyond the 1024-row run limit is checked from the reference alone."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M64 = (1 << 64) - 1
HMJ_E_ARG = -1
SWEEP_SEED, SWEEP_ITERS, SWEEP_MAX_SKIPS = 20261020, 30, 3  # HMJ_STRESS_SEED / HMJ_STRESS_ITERS override the first two
RUN_CAP = 1024  # rows of a run of equal key64 with several tuples that one workgroup sorts


# ---- the entry and its structs -----------------------------------------------------------------------------------------------
def test_the_library_exports_the_entry_and_refuses_a_null_ctx():
    import hashmergejoin_amd as H

    L = H.load_library()
    assert hasattr(L, "hmj_group_mixed_device")
    rel, opts, res = H.MixedRel(), H.GroupOpts(), H.GroupResult()
    opts.struct_size = C.sizeof(H.GroupOpts)
    assert L.hmj_group_mixed_device(None, C.byref(rel), 0, C.byref(opts), C.byref(res)) == HMJ_E_ARG
    assert L.hmj_group_mixed_device(None, None, 0, None, None) == HMJ_E_ARG


def test_the_new_names_are_exported():
    import hashmergejoin_amd as H

    assert "expected_mixed_groups" in H.__all__ and callable(H.expected_mixed_groups)
    assert hasattr(H.Executor, "group_mixed_device")
    assert "expected_groups" in H.__all__ and "mixed_key64" in H.__all__  # (what was there stays)


def test_the_abi_version_and_the_group_structs_are_unchanged():
    import hashmergejoin_amd as H

    src = ('#include <cstdio>\n#include "hmj.h"\nint main() {\n'
           'typedef int (*entry)(hmj_ctx*, const hmj_mixed_rel*, uint32_t, hmj_group_opts*, hmj_group_result*);\n'
           'static_assert(sizeof(decltype(entry(&hmj_group_mixed_device))) == sizeof(void*), "the declared signature");\n'
           'std::printf("%d %zu %zu\\n", HMJ_ABI_VERSION, sizeof(hmj_group_opts), sizeof(hmj_group_result));\n'
           'return 0;\n}\n')
    with tempfile.TemporaryDirectory() as d:
        cc, exe = os.path.join(d, "abi.cc"), os.path.join(d, "abi")
        open(cc, "w").write(src)
        subprocess.check_call(["g++", "-std=c++11", "-I", os.path.join(ROOT, "include"), cc, "-o", exe])
        got = [int(x) for x in subprocess.check_output([exe]).decode().split()]
    assert got == [5, 64, 80]  # the sizes the parent's header gives: nothing in either struct moved
    assert got[1:3] == [C.sizeof(H.GroupOpts), C.sizeof(H.GroupResult)]
    assert H.load_library().hmj_abi_version() == 5


# ---- the reference against a brute-force model ---------------------------------------------------------------------------------
def is_str(col):
    return not isinstance(col, np.ndarray)


def tuples_of(columns, valid):
    """The rows' key tuples in plain Python values (int / bytes), None in a NULL slot."""
    n = len(columns[0])
    cols = []
    for c, col in enumerate(columns):
        if is_str(col):
            v = list(col)
        else:
            a = np.ascontiguousarray(col)
            v = [int(x) for x in a.view("u%d" % a.dtype.itemsize)]
        ok = None if valid is None or valid[c] is None else valid[c]
        cols.append([None if (ok is not None and not ok[i]) else v[i] for i in range(n)])
    return list(zip(*cols))


def null_last(t):
    """Per column (is NULL, value): ints order as unsigned integers, bytes as std::string::operator<."""
    return tuple((1, 0) if v is None else (0, v) for v in t)


def brute_groups(H, columns, vals, valid, hash_bits=0, ordered=False):
    """Groups by a dict of tuples: plain tuple equality is the grouping rule (None equals None and nothing else, b"" is
    not None)."""
    tup = tuples_of(columns, valid)
    key = H.mixed_key64(columns, hash_bits, valid, null_equal=True)
    groups = {}
    for i, t in enumerate(tup):
        groups.setdefault(t, []).append(i)
    order = list(groups)  # by first row
    if ordered:
        order.sort(key=lambda t: (int(key[groups[t][0]]), null_last(t)))
    pay = list(range(len(tup))) if vals is None else [int(v) & M64 for v in vals]
    index = {t: g for g, t in enumerate(order)}
    runs = {}
    for t in order:
        runs.setdefault(int(key[groups[t][0]]), []).append(len(groups[t]))
    return {"n_groups": len(order), "n_rows": len(tup), "max_count": max((len(groups[t]) for t in order), default=0),
            "n_null": sum(1 for t in tup if None in t), "form": H.HMJ_COLS_HASHED,
            "n_collisions": len(order) - len(runs),
            "max_mixed_run": max((sum(r) for r in runs.values() if len(r) > 1), default=0),
            "key64": [int(key[groups[t][0]]) for t in order], "first_row": [groups[t][0] for t in order],
            "count": [len(groups[t]) for t in order], "sum": [sum(pay[i] for i in groups[t]) & M64 for t in order],
            "min": [min(pay[i] for i in groups[t]) for t in order], "max": [max(pay[i] for i in groups[t]) for t in order],
            "group_of_row": [index[t] for t in tup]}


def assert_same(got, want, tag=""):
    for k, v in want.items():
        g = got[k]
        assert (g.tolist() if hasattr(g, "tolist") else g) == v, (tag, k)


def draw_strings(rng, n, card, lo=0, hi=24, prefix=b""):
    """n slots over `card` distinct-ish byte strings of lo..hi drawn bytes (NUL and bytes >= 0x80 included) behind `prefix`."""
    pool = [prefix + rng.integers(0, 256, size=int(rng.integers(lo, hi + 1)), dtype=np.uint8).tobytes() for _ in range(card)]
    return [pool[int(i)] for i in rng.integers(0, card, size=n)]


def draw_fixed(rng, n, card, width):
    pool = rng.integers(0, 1 << min(8 * width, 63), size=card, dtype=np.uint64).astype("u%d" % width)
    return pool[rng.integers(0, card, size=n)]


def draw_columns(rng, n, shape, card):
    """shape: one entry per column, "s" (a string column) or a width in bytes."""
    return [draw_strings(rng, n, card) if s == "s" else draw_fixed(rng, n, card, s) for s in shape]


def draw_valid(rng, n, k, density, which):
    """Validity per column: None (no bitmap) for the columns outside `which`, else n bools with about `density` NULLs."""
    return [(rng.random(n) >= density) if c in which else None for c in range(k)]


def with_none_under_nulls(columns, valid):
    """The same relation with None in the NULL slots of its string columns."""
    out = []
    for c, col in enumerate(columns):
        if is_str(col) and valid is not None and valid[c] is not None:
            col = [b if valid[c][i] else None for i, b in enumerate(col)]
        out.append(col)
    return out


def test_expected_mixed_groups_agrees_with_a_dict_of_tuples():
    import hashmergejoin_amd as H

    rng = np.random.default_rng(20261020)
    shapes = [["s"], ["s", 4], [2, "s", "s"], ["s", "s"], [8, "s", 1, "s"]]
    for shape in shapes:
        k = len(shape)
        for n, card, density, which in ((1, 1, 0.0, set()), (65, 7, 0.0, set()), (300, 40, 0.1, {0}), (257, 300, 0.5, set(range(k))),
                                        (200, 9, 0.3, set(range(0, k, 2))), (64, 5, 1.0, set(range(k)))):
            cols = draw_columns(rng, n, shape, card)
            vals = rng.integers(0, 1 << 64, size=n, dtype=np.uint64) if n % 2 else None
            valid = draw_valid(rng, n, k, density, which) if which else None
            for bits in (0, 3):
                for ordered in (False, True):
                    want = brute_groups(H, cols, vals, valid, bits, ordered)
                    assert_same(H.expected_mixed_groups(cols, vals, valid, bits, ordered), want, (shape, n, bits, ordered))
                    holed = with_none_under_nulls(cols, valid)
                    assert_same(H.expected_mixed_groups(holed, vals, valid, bits, ordered), want, (shape, n, bits, ordered, "None"))
    e = H.expected_mixed_groups([[]])
    assert e["n_groups"] == 0 and e["max_count"] == 0 and len(e["key64"]) == 0 and len(e["group_of_row"]) == 0


def test_fixed_columns_only_equal_the_column_reference():
    import hashmergejoin_amd as H

    rng = np.random.default_rng(88)
    for widths in ([4], [4, 4], [8, 4, 2], [1, 2], [8] * 8):
        k = len(widths)
        for n, card, which in ((1, 1, set()), (300, 40, set()), (500, 25, {0}), (257, 300, set(range(k)))):
            cols = [draw_fixed(rng, n, card, w) for w in widths]
            vals = rng.integers(0, 1 << 64, size=n, dtype=np.uint64)
            valid = draw_valid(rng, n, k, 0.2, which) if which else None
            for bits in (0, 2):
                for ordered in (False, True):
                    a = H.expected_mixed_groups(cols, vals, valid, bits, ordered)
                    b = H.expected_groups(cols, widths, vals, valid, bits, force_hashed=True, ordered=ordered)
                    assert set(a) == set(b)
                    for f in b:
                        x, y = a[f], b[f]
                        assert (x.tolist() if hasattr(x, "tolist") else x) == (y.tolist() if hasattr(y, "tolist") else y), (widths, n, f)


def test_hand_cases():
    import hashmergejoin_amd as H

    # a NULL string is not the empty string; two NULLs are one group
    e = H.expected_mixed_groups([[b"", None, b"", None, b"x"]], [1, 2, 4, 8, 16], [np.array([1, 0, 1, 0, 1], bool)])
    assert e["n_groups"] == 3 and e["n_null"] == 2 and e["first_row"].tolist() == [0, 1, 4] and e["sum"].tolist() == [5, 10, 16]
    assert e["key64"][0] != e["key64"][1]
    # (NULL, x) against (x, NULL)
    x = [b"k", b"k"]
    e = H.expected_mixed_groups([x, x], None, [np.array([0, 1], bool), np.array([1, 0], bool)])
    assert e["n_groups"] == 2 and e["group_of_row"].tolist() == [0, 1] and e["key64"][0] != e["key64"][1]
    # keys that share their first 8 / 16 bytes and differ in the last byte; a key that is a prefix of another
    p8, p16 = b"ABCDEFGH", b"ABCDEFGHIJKLMNOP"
    keys = [p8 + b"a", p8 + b"b", p16 + b"a", p16 + b"b", p8, p16, p8 + b"a", b""]
    e = H.expected_mixed_groups([keys], ordered=True, hash_bits=1)
    assert e["n_groups"] == 7 and e["max_count"] == 2
    o = H.expected_mixed_groups([keys])
    assert o["first_row"].tolist() == [0, 1, 2, 3, 4, 5, 7] and o["count"].tolist() == [2, 1, 1, 1, 1, 1, 1]
    # bytes >= 0x80 and embedded NULs: the ordered result is a sort by (key64, tuple, NULLS LAST) with one hash bit
    keys = [b"\x00", b"\x00\x00", b"", b"\x80", b"\x7f\xff", b"a\x00b", b"a\x00", b"a", b"\xff", None, b"\x80\x00", b"a\x00b"]
    valid = [np.array([b is not None for b in keys])]
    nums = np.arange(len(keys), dtype=np.uint8) % 2
    e = H.expected_mixed_groups([keys, nums], None, [valid[0], None], hash_bits=1, ordered=True)
    first = e["first_row"].astype(np.int64).tolist()
    key = H.mixed_key64([keys, nums], 1, [valid[0], None], null_equal=True)
    want = sorted(set(first), key=lambda i: (int(key[i]), (1, b"") if keys[i] is None else (0, keys[i]), int(nums[i])))
    assert first == want and e["n_groups"] == 11 and set(e["key64"].tolist()) <= {0, 1}
    assert e["n_collisions"] == e["n_groups"] - len(set(e["key64"].tolist())) > 0


def test_garbage_under_null_slots_changes_nothing():
    import hashmergejoin_amd as H

    rng = np.random.default_rng(5)
    shape = ["s", 4, "s"]
    cols = draw_columns(rng, 400, shape, 30)
    valid = draw_valid(rng, 400, 3, 0.2, {0, 1})
    want = H.expected_mixed_groups(cols, None, valid, ordered=True)
    dirty = [list(cols[0]), cols[1].copy(), cols[2]]
    for i in np.flatnonzero(~valid[0]):
        dirty[0][int(i)] = b"junk%d" % int(i)
    dirty[1][~valid[1]] = 12345
    got = H.expected_mixed_groups(dirty, None, valid, ordered=True)
    for k, v in want.items():
        assert (got[k].tolist() if hasattr(v, "tolist") else got[k]) == (v.tolist() if hasattr(v, "tolist") else v), k


# ---- the randomized sweep's draws (shared with test_group_mixed_gpu.py) ---------------------------------------------------------
def draw_case(rng):
    """One draw of the sweep: n <= 6000 rows, 1-4 columns of which at least one is a string column, drawn cardinality,
    string lengths and NULL density, hash_bits in {0, 0, 0, 20, 6}, payloads or none.  Returns a dict of host inputs."""
    n = int(rng.choice([1, 2, 63, 64, 65, 255, 256, 257, 1023, 1025, 4097]))
    if rng.random() < 0.5:
        n = int(rng.integers(1, 6001))
    k = int(rng.integers(1, 5))
    shape = [("s" if rng.random() < 0.5 else int(rng.choice([1, 2, 4, 8]))) for _ in range(k)]
    shape[int(rng.integers(0, k))] = "s"
    card = int(rng.choice([1, 3, 17, 300, 5000]))
    hi = int(rng.choice([0, 7, 24, 90]))
    cols = [draw_strings(rng, n, card, 0, hi, prefix=(b"prefix--" if rng.random() < 0.3 else b"")) if s == "s" else draw_fixed(rng, n, card, s)
            for s in shape]
    density = float(rng.choice([0.0, 0.0, 0.01, 0.1, 0.9]))
    which = {c for c in range(k) if rng.random() < 0.5} if density else set()
    valid = draw_valid(rng, n, k, density, which) if which else None
    vals = rng.integers(0, 1 << 64, size=n, dtype=np.uint64) if rng.random() < 0.6 else None
    return {"n": n, "shape": shape, "cols": cols, "valid": valid, "vals": vals, "hash_bits": int(rng.choice([0, 0, 0, 20, 6])),
            "ordered": bool(rng.random() < 0.5), "offset": int(rng.choice([0, 3, 67]))}


def sweep_params():
    return int(os.environ.get("HMJ_STRESS_SEED", SWEEP_SEED)), int(os.environ.get("HMJ_STRESS_ITERS", SWEEP_ITERS))


def exceeds_run_cap(H, case):
    """From the reference alone: the call holds a run of equal key64 with several tuples and more than 1024 rows."""
    return H.expected_mixed_groups(case["cols"], None, case["valid"], case["hash_bits"])["max_mixed_run"] > RUN_CAP


def test_the_default_sweep_exceeds_the_run_cap_in_at_most_three_draws():
    import hashmergejoin_amd as H

    rng = np.random.default_rng(SWEEP_SEED)
    cases = [draw_case(rng) for _ in range(SWEEP_ITERS)]
    skipped = sum(exceeds_run_cap(H, c) for c in cases)
    assert skipped <= SWEEP_MAX_SKIPS, skipped
    assert sum(c["valid"] is not None for c in cases) >= 5 and sum(c["hash_bits"] != 0 for c in cases) >= 5  # both paths are drawn
