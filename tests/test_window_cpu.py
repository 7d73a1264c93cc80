"""CPU-only checks of hmj_window_device (include/hmj.h, "window functions over ordered partitions"): the library exports
the entry and refuses a NULL ctx, the three new structs and every new constant have the values the ctypes mirrors assume
and the ABI version is unchanged, and `expected_window` -- the numpy reference test_window_gpu.py compares the device with
-- agrees with a brute-force restatement written out here in plain Python (`brute_window`, O(n^2): for each row, the rows
of its partition that precede it under a comparator).  Also here, shared with the GPU file: the draws of the randomized
sweep (`draw_window_case`) with their ledger."""
import ctypes as C
import functools
import math
import os
import subprocess
import tempfile
from fractions import Fraction

import numpy as np
import pytest

from test_order_by_cpu import DESC, DTYPES, NULLS_FIRST, STRING, brute_order, cmp_values, draw_strings, special_values

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HMJ_E_ARG = -1
SWEEP_SEED, SWEEP_ITERS = 20261021, 20  # HMJ_STRESS_SEED / HMJ_STRESS_ITERS override them
ROW_NUMBER, RANK, DENSE_RANK, CUM_COUNT, CUM_SUM, CUM_MIN, CUM_MAX, LAG, LEAD = range(9)
OPS = ("ROW_NUMBER", "RANK", "DENSE_RANK", "CUM_COUNT", "CUM_SUM", "CUM_MIN", "CUM_MAX", "LAG", "LEAD")
VALUE_OPS = (CUM_SUM, CUM_MIN, CUM_MAX, LAG, LEAD)


# ---- the entry and its structs -----------------------------------------------------------------------------------------------
def test_the_library_exports_the_entry_and_refuses_a_null_ctx():
    import hashmergejoin_amd as H

    L = H.load_library()
    assert hasattr(L, "hmj_window_device")
    fn, dst, opts = H.WindowFn(), H.WindowDst(), H.WindowOpts()
    opts.struct_size = C.sizeof(H.WindowOpts)
    assert L.hmj_window_device(None, None, 0, 0, C.byref(fn), 1, C.byref(dst), None, C.byref(opts)) == HMJ_E_ARG
    for name in ["WindowFn", "WindowDst", "WindowOpts", "HMJ_MAX_WINDOW_FNS", "expected_window"] + ["HMJ_WIN_" + o for o in OPS]:
        assert name in H.__all__ and hasattr(H, name), name
    assert hasattr(H.Executor, "window_device")
    assert [getattr(H, "HMJ_WIN_" + o) for o in OPS] == list(range(9))
    from hashmergejoin_amd import join, reference

    assert join.expected_window is reference.expected_window is H.expected_window


def test_struct_layouts_and_constants_match_the_header_and_the_abi_version_stays():
    import hashmergejoin_amd as H

    structs = {"hmj_window_fn": (H.WindowFn, ["data", "type", "op", "validity", "offset"]),
               "hmj_window_dst": (H.WindowDst, ["data", "validity", "null_count"]),
               "hmj_window_opts": (H.WindowOpts, ["struct_size", "n_partition_cols", "n_partitions", "n_peer_groups", "max_partition_rows",
                                                  "n_rounds", "reserved", "ms_order", "ms_heads", "ms_scan"])}
    consts = ["HMJ_WIN_" + o for o in OPS] + ["HMJ_MAX_WINDOW_FNS", "HMJ_ABI_VERSION"]
    lines = []
    for cname, (_, fields) in structs.items():
        lines.append('std::printf("sizeof.%s %%zu\\n", sizeof(%s));' % (cname, cname))
        lines += ['std::printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, f, cname, f) for f in fields]
    lines += ['std::printf("%s %%lld\\n", (long long)%s);' % (k, k) for k in consts]
    src = '#include <cstddef>\n#include <cstdio>\n#include "hmj.h"\nint main() {\n%s\nreturn 0;\n}\n' % "\n".join(lines)
    with tempfile.TemporaryDirectory() as d:
        cc, exe = os.path.join(d, "layout.cc"), os.path.join(d, "layout")
        open(cc, "w").write(src)
        subprocess.check_call(["g++", "-std=c++11", "-I", os.path.join(ROOT, "include"), cc, "-o", exe])
        got = {k: int(v) for k, v in (line.split() for line in subprocess.check_output([exe]).decode().splitlines())}
    for cname, (mirror, fields) in structs.items():
        assert got["sizeof." + cname] == C.sizeof(mirror), cname
        assert [f for f, _ in mirror._fields_] == fields
        for f in fields:
            assert got[cname + "." + f] == getattr(mirror, f).offset, (cname, f)
    for k in consts[:-1]:
        assert got[k] == getattr(H, k), k
    assert [got[k] for k in consts[:10]] == list(range(9)) + [32]
    assert got["HMJ_ABI_VERSION"] == 5  # a new entry with structs of its own: nothing existing changed
    assert H.load_library().hmj_abi_version() == 5
    # the struct mirrors live beside _lib, whose own set of mirrors is pinned by test_binding_cpu.py
    from hashmergejoin_amd import _lib, _window

    assert H.WindowFn is _window.WindowFn and not hasattr(_lib, "WindowFn")
    assert len(_lib._SIGNATURES["hmj_window_device"][1]) == 9


# ---- the semantics, written out ------------------------------------------------------------------------------------------------
def py_columns(columns):
    out = []
    for c in columns:
        vals, flags = c[0], c[1]
        valid = c[2] if len(c) > 2 else None
        if isinstance(vals, np.ndarray):
            py = [float(v) if vals.dtype.kind == "f" else int(v) for v in vals]
        else:
            py = [None if v is None else bytes(v) for v in vals]
        ok = [(valid is None or bool(valid[i])) and py[i] is not None for i in range(len(py))]
        out.append((py, flags, ok))
    return out


def cmp_rows(cols, i, j):
    """-1 / 0 / 1 for rows i and j over the given columns, no tie-break: 0 is the ORDER BY's equality."""
    for py, flags, ok in cols:
        if not ok[i] or not ok[j]:
            if ok[i] == ok[j]:
                continue
            return -1 if (not ok[i]) == bool(flags & NULLS_FIRST) else 1
        c = cmp_values(py[i], py[j])
        if c:
            return -c if flags & DESC else c
    return 0


def brute_window(columns, npc, fns, n):
    """`expected_window`'s result by brute force: every row looks at all rows of its partition."""
    cols = py_columns(columns)
    part_cols, order_cols = cols[:npc], cols[npc:]
    full = lambda a, b: cmp_rows(cols, a, b) or ((a > b) - (a < b))  # noqa: E731
    row_map = [int(r) for r in brute_order(columns)] if columns else list(range(n))
    parts = {}
    outs = [{"values": [None] * n, "valid": [True] * n} for _ in fns]
    for i in range(n):
        part = sorted((j for j in range(n) if cmp_rows(part_cols, i, j) == 0), key=functools.cmp_to_key(full))
        parts[part[0]] = len(part)
        at = part.index(i)
        before = part[:at + 1]  # the frame: the partition's first row through this row
        for k, f in enumerate(fns):
            op = int(f[0])
            vals = f[1] if len(f) > 1 else None
            valid = f[2] if len(f) > 2 else None
            off = int(f[4]) if len(f) > 4 else 0
            ok_at = lambda r: valid is None or bool(valid[r])  # noqa: E731
            v, ok = 0, True
            if op == ROW_NUMBER:
                v = at + 1
            elif op == RANK:
                v = 1 + sum(1 for j in part if cmp_rows(order_cols, j, i) < 0)
            elif op == DENSE_RANK:
                v = 1 + sum(1 for a, b in zip(before, before[1:]) if cmp_rows(order_cols, a, b) != 0)
            elif op == CUM_COUNT:
                v = sum(1 for j in before if ok_at(j))
            elif op in (LAG, LEAD):
                p = at - off if op == LAG else at + off
                ok = 0 <= p < len(part) and ok_at(part[p])
                v = vals[part[p]] if ok else 0
            else:
                seen = [vals[j] for j in before if ok_at(j)]
                ok = bool(seen)
                kind = vals.dtype.kind
                if not ok:
                    v = 0
                elif op == CUM_SUM and kind == "f":
                    xs = [float(x) for x in seen]
                    if all(math.isfinite(x) for x in xs):
                        v = float(sum(Fraction(x) for x in xs))
                    else:
                        v = xs[0]
                        for x in xs[1:]:
                            v = v + x
                elif op == CUM_SUM:
                    t = sum(int(x) for x in seen) & 0xFFFFFFFFFFFFFFFF
                    v = t - (1 << 64) if kind == "i" and t >> 63 else t
                else:
                    nums = [x for x in seen if not (kind == "f" and math.isnan(float(x)))]
                    if not nums:
                        v = float("nan")
                    else:
                        conv = float if kind == "f" else int
                        best = nums[0]
                        for x in nums[1:]:
                            c = cmp_values(conv(x), conv(best))
                            if (c < 0) if op == CUM_MIN else (c > 0):
                                best = x
                        v = best
            outs[k]["values"][i], outs[k]["valid"][i] = v, ok
    heads = sum(1 for a, b in zip(row_map, row_map[1:]) if cmp_rows(cols, a, b) != 0) + (1 if n else 0)
    return {"row_map": row_map, "n_partitions": len(parts), "n_peer_groups": heads,
            "max_partition_rows": max(parts.values()) if parts else 0, "outputs": outs}


def bits_of(a):
    a = np.ascontiguousarray(a)
    return a.view("u%d" % a.dtype.itemsize)


def assert_matches_brute(columns, npc, fns, n, tag=""):
    import hashmergejoin_amd as H

    want = brute_window(columns, npc, fns, n)
    got = H.expected_window(columns, npc, fns, n=n)
    assert [int(r) for r in got["row_map"]] == want["row_map"], tag
    for key in ("n_partitions", "n_peer_groups", "max_partition_rows"):
        assert got[key] == want[key], (tag, key, got[key], want[key])
    for k, (g, w) in enumerate(zip(got["outputs"], want["outputs"])):
        ok = np.array([w["valid"][r] for r in want["row_map"]], bool)
        assert np.array_equal(g["valid"], ok), (tag, k, OPS[fns[k][0]])
        assert g["null_count"] == int(n - ok.sum()), (tag, k)
        vals = np.array([w["values"][r] if w["valid"][r] else 0 for r in want["row_map"]], dtype=g["values"].dtype)
        assert np.array_equal(bits_of(g["values"]), bits_of(vals)), (tag, k, OPS[fns[k][0]], g["values"][:20], vals[:20])


def all_ops(x, valid=None, offsets=(1, 1)):
    return [(ROW_NUMBER, None), (RANK, None), (DENSE_RANK, None), (CUM_COUNT, x, valid), (CUM_SUM, x, valid), (CUM_MIN, x, valid),
            (CUM_MAX, x, valid), (LAG, x, valid, 0, offsets[0]), (LEAD, x, valid, 0, offsets[1])]


def hand_made_tables():
    rng = np.random.default_rng(5)
    n = 60
    k = rng.integers(0, 3, size=n).astype(np.int32)
    t = rng.integers(0, 6, size=n).astype(np.int64)
    x = rng.integers(-50, 50, size=n).astype(np.int16)
    f = special_values("float64", rng, n)
    valid = rng.random(n) >= 0.3
    names = [[b"north", b"south", b"a-twenty-byte-prefix-1", b"a-twenty-byte-prefix-2"][i] for i in rng.integers(0, 4, size=n)]
    out = [("i32 partitions, i64 order", [(k, 0), (t, 0)], 1, all_ops(x, valid), n),
           ("no keys", [], 0, all_ops(x, valid, (0, 2)), n),
           ("all partition columns", [(k, DESC), (t, NULLS_FIRST, valid)], 2, all_ops(x, None, (n, n - 1)), n),
           ("no partition columns", [(t, DESC)], 0, all_ops(x, valid, (2 ** 63, 2 ** 63)), n),
           ("string partitions with NULLs, float values", [(names, 0, valid), (t, DESC | NULLS_FIRST, ~valid)], 1, all_ops(f, valid), n),
           ("float partitions: NaNs one partition, the zeros two", [(f, 0), (k, 0)], 1, all_ops(x), n),
           ("one row", [(k[:1], 0)], 1, all_ops(x[:1]), 1)]
    for dtype in DTYPES:
        v = special_values(dtype, rng, n)
        if np.dtype(dtype).kind == "f":  # sums of finite values only: an overflow's place depends on the bracketing
            v = np.where(np.isfinite(v) & (np.abs(v) < 1e30), v, np.dtype(dtype).type(1.5))
        out.append((dtype + " values", [(k, 0), (t, 0)], 1, all_ops(v, valid, (1, 3)), n))
    return out


@pytest.mark.parametrize("tag,columns,npc,fns,n", hand_made_tables(), ids=[t[0] for t in hand_made_tables()])
def test_the_reference_agrees_with_brute_force_on_hand_made_tables(tag, columns, npc, fns, n):
    assert_matches_brute(columns, npc, fns, n, tag)


def test_nan_and_infinity_stay_inside_their_partition():
    import hashmergejoin_amd as H

    k = np.array([0, 0, 0, 0, 1, 1, 1], np.int32)
    x = np.array([1.0, np.nan, np.inf, -np.inf, 2.0, -3.0, 0.5])
    got = H.expected_window([(k, 0)], 1, [(CUM_SUM, x), (CUM_MIN, x), (CUM_MAX, x)])["outputs"]
    assert np.array_equal(got[0]["values"][4:], [2.0, -1.0, -0.5]) and np.all(np.isnan(got[0]["values"][1:4]))
    assert np.array_equal(got[1]["values"], [1.0, 1.0, 1.0, -np.inf, 2.0, -3.0, -3.0])
    assert np.array_equal(got[2]["values"], [1.0, 1.0, np.inf, np.inf, 2.0, 2.0, 2.0])
    assert_matches_brute([(k, 0)], 1, [(CUM_SUM, x), (CUM_MIN, x), (CUM_MAX, x)], 7)


# ---- the randomized sweep's draws ----------------------------------------------------------------------------------------------
def draw_window_case(rng, it, max_n=20000):
    """Case `it` of a sweep: {"n", "npc", "cols": key columns as test_order_by_cpu's draws describe them, "fns": [{"op",
    "values", "valid", "bit_offset", "offset"}]}.  Every fourth case is small enough for `brute_window`; every fifth has no
    keys; n_partition_cols cycles through none, some and all; every value op meets every type within ten cases."""
    n = int(rng.integers(1, 201)) if it % 4 == 0 else int(rng.integers(201, max_n + 1))
    kinds = list(DTYPES) + [STRING]

    def column(kind, distinct):
        flags = int(rng.integers(0, 4))
        values = draw_strings(rng, n, distinct, b"a-twenty-byte-prefix" if rng.random() < 0.5 else b"") if kind == STRING \
            else special_values(kind, rng, n, distinct)
        valid, off = None, 0
        if rng.random() < 0.5:
            valid = rng.random(n) >= (0.1 if rng.random() < 0.7 else 0.9)
            off = int(rng.choice([0, 3, 67, 8]))
        pad = int(rng.integers(0, 9)) if kind == STRING and rng.random() < 0.6 else 0
        return {"type": kind, "values": values, "flags": flags, "valid": valid, "bit_offset": off, "pad": pad}

    n_keys = 0 if it % 5 == 4 else int(rng.integers(1, 4))
    npc = [0, min(1, n_keys), n_keys][it % 3] if n_keys else 0
    cols = []
    for c in range(n_keys):
        kind = kinds[(it * 3 + c * 5 + int(rng.integers(0, 2))) % len(kinds)]
        cols.append(column(kind, int(rng.choice([1, 2, 4, 9])) if c < max(npc, 1) else int(rng.choice([1, 2, 5, 40, 5000]))))
    longest = n  # an offset beyond any partition
    offsets = [0, 1, int(rng.integers(2, 70)), longest + 5, 2 ** 63]
    fns = []

    def fn(op, dtype=None):
        values = valid = None
        off = 0
        if dtype is not None:
            if op == CUM_SUM and np.dtype(dtype).kind == "f":  # finite, far from overflow: the sum's bound is meaningful
                values = (rng.standard_normal(n) * 10.0 ** int(rng.integers(-3, 6))).astype(dtype)
            else:
                values = special_values(dtype, rng, n)
            if rng.random() < 0.6:
                valid = rng.random(n) >= (0.2 if rng.random() < 0.7 else 0.95)
                off = int(rng.choice([0, 3, 67, 8]))
        return {"op": op, "values": values, "valid": valid, "bit_offset": off,
                "offset": offsets[int(rng.integers(0, len(offsets)))] if op in (LAG, LEAD) else 0}

    for op in (ROW_NUMBER, RANK, DENSE_RANK):
        fns.append(fn(op))
    fns.append(fn(CUM_COUNT, DTYPES[it % 10]))
    for k, op in enumerate(VALUE_OPS):
        fns.append(fn(op, DTYPES[(it + 2 * k) % 10]))
    for _ in range(int(rng.integers(0, 4))):  # a few more: the launches are cut differently from case to case
        op = int(rng.integers(0, 9))
        fns.append(fn(op, None if op < CUM_COUNT else DTYPES[int(rng.integers(0, 10))]))
    order = rng.permutation(len(fns))
    return {"n": n, "npc": npc, "cols": cols, "fns": [fns[i] for i in order]}


def case_columns(case):
    return [(c["values"], c["flags"], c["valid"]) for c in case["cols"]]


def case_fns(case):
    """The case's functions as `expected_window` takes them."""
    return [(f["op"], f["values"], f["valid"], f["bit_offset"], f["offset"]) for f in case["fns"]]


def sweep_params():
    return int(os.environ.get("HMJ_STRESS_SEED", SWEEP_SEED)), int(os.environ.get("HMJ_STRESS_ITERS", SWEEP_ITERS))


def test_the_default_sweep_reaches_every_op_type_layout_and_offset_and_its_small_cases_agree_with_brute_force():
    import hashmergejoin_amd as H

    rng = np.random.default_rng(SWEEP_SEED)
    ops, op_types, part_types, order_types = set(), set(), set(), set()
    fn_offsets, key_offsets, npcs, lag_offsets, no_keys, brute = set(), set(), set(), set(), 0, 0
    for it in range(SWEEP_ITERS):
        case = draw_window_case(rng, it)
        n, cols = case["n"], case["cols"]
        assert 1 <= n <= 20000 and len(cols) <= H.HMJ_MAX_ORDER_COLS and 1 <= len(case["fns"]) <= H.HMJ_MAX_WINDOW_FNS
        no_keys += not cols
        if cols:
            npcs.add("none" if case["npc"] == 0 else ("all" if case["npc"] == len(cols) else "some"))
        for k, c in enumerate(cols):
            (part_types if k < case["npc"] else order_types).add("string" if c["type"] == STRING else "typed")
            if c["valid"] is not None:
                key_offsets.add(c["bit_offset"])
        want = H.expected_window(case_columns(case), case["npc"], case_fns(case), n=n)
        for f in case["fns"]:
            ops.add(f["op"])
            if f["op"] in VALUE_OPS:
                op_types.add((f["op"], str(f["values"].dtype)))
            if f["valid"] is not None:
                fn_offsets.add(f["bit_offset"])
            if f["op"] in (LAG, LEAD):
                lag_offsets.add("0" if f["offset"] == 0 else "1" if f["offset"] == 1 else "beyond" if f["offset"] > want["max_partition_rows"] else "in")
        assert sorted(int(r) for r in want["row_map"]) == list(range(n))
        if n <= 200:
            assert_matches_brute(case_columns(case), case["npc"], case_fns(case), n, "case %d" % it)
            brute += 1
    assert ops == set(range(9))
    assert op_types == {(op, t) for op in VALUE_OPS for t in DTYPES}, sorted({(op, t) for op in VALUE_OPS for t in DTYPES} - op_types)
    assert part_types == {"string", "typed"} and order_types == {"string", "typed"}
    assert any(o != 0 for o in fn_offsets) and any(o != 0 for o in key_offsets)
    assert no_keys >= 1 and npcs == {"none", "some", "all"}
    assert {"0", "1", "beyond"} <= lag_offsets
    assert brute >= 4
