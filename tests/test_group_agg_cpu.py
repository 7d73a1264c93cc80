"""CPU-only checks of hmj_group_agg_device (include/hmj.h, "aggregating typed value columns over a grouping"): the library
exports the entry and refuses a NULL ctx, the three new structs and every new constant have the values the ctypes mirrors
assume and the ABI version is unchanged, and `expected_group_aggs` -- the numpy reference test_group_agg_gpu.py compares the
device with -- agrees with a brute-force model in plain Python (int arithmetic with explicit wrap, fractions for the float
sums, a hand-written total order for the floats) over every type x op.  Also here, shared with the GPU file: the draws of its
randomized sweep (`draw_agg_case`) and the comparison of a result with the reference (`assert_aggs`)."""
import ctypes as C
import math
import os
import struct
import subprocess
import tempfile
from fractions import Fraction

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HMJ_E_ARG = -1
SWEEP_SEED, SWEEP_ITERS = 20261020, 30  # HMJ_STRESS_SEED / HMJ_STRESS_ITERS override them
DTYPES = ("int8", "int16", "int32", "int64", "uint8", "uint16", "uint32", "uint64", "float32", "float64")  # HMJ_TYPE_* order
U = 2.0 ** -53


# ---- the entry and its structs -----------------------------------------------------------------------------------------------
def test_the_library_exports_the_entry_and_refuses_a_null_ctx():
    import hashmergejoin_amd as H

    L = H.load_library()
    assert hasattr(L, "hmj_group_agg_device")
    src, dst, opts = H.AggSrc(), H.AggDst(), H.GroupAggOpts()
    opts.struct_size = C.sizeof(H.GroupAggOpts)
    assert L.hmj_group_agg_device(None, C.byref(src), 1, 0, C.byref(dst), C.byref(opts)) == HMJ_E_ARG
    names = ["AggSrc", "AggDst", "GroupAggOpts", "HMJ_AGG_COUNT", "HMJ_AGG_SUM", "HMJ_AGG_MIN", "HMJ_AGG_MAX", "HMJ_AGG_MEAN", "HMJ_MAX_AGGS",
             "expected_group_aggs"] + ["HMJ_TYPE_" + t for t in ("I8", "I16", "I32", "I64", "U8", "U16", "U32", "U64", "F32", "F64")]
    for name in names:
        assert name in H.__all__ and hasattr(H, name), name
    assert hasattr(H.Executor, "group_agg_device")


def test_struct_layouts_and_constants_match_the_header_and_the_abi_version_stays():
    import hashmergejoin_amd as H

    structs = {"hmj_agg_src": (H.AggSrc, ["data", "type", "op", "validity"]),
               "hmj_agg_dst": (H.AggDst, ["data", "validity", "null_count"]),
               "hmj_group_agg_opts": (H.GroupAggOpts, ["struct_size", "reserved", "n_groups", "ms_agg"])}
    consts = ["HMJ_AGG_COUNT", "HMJ_AGG_SUM", "HMJ_AGG_MIN", "HMJ_AGG_MAX", "HMJ_AGG_MEAN", "HMJ_TYPE_I8", "HMJ_TYPE_I16", "HMJ_TYPE_I32",
              "HMJ_TYPE_I64", "HMJ_TYPE_U8", "HMJ_TYPE_U16", "HMJ_TYPE_U32", "HMJ_TYPE_U64", "HMJ_TYPE_F32", "HMJ_TYPE_F64", "HMJ_MAX_AGGS",
              "HMJ_ABI_VERSION"]
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
    assert [got[k] for k in consts[:5]] == [0, 1, 2, 3, 4] and [got[k] for k in consts[5:15]] == list(range(10)) and got["HMJ_MAX_AGGS"] == 64
    assert got["HMJ_ABI_VERSION"] == 5  # a new entry with structs of its own: nothing existing changed
    assert H.load_library().hmj_abi_version() == 5


# ---- the reference against a brute-force model ---------------------------------------------------------------------------------
def bits_of(x, dtype):
    """The bit pattern of a float of the given numpy dtype, as an int."""
    return int(np.array([x], dtype).view("u%d" % np.dtype(dtype).itemsize)[0])


def float_before(a, b):
    """a < b in IEEE order with -0.0 < +0.0 (no NaNs), written out by hand."""
    if a != b:
        return a < b
    return math.copysign(1.0, a) < math.copysign(1.0, b)


def brute_aggs(H, gmap, ng, aggs):
    """Per aggregate: (values as Python numbers or bit patterns for float MIN / MAX, valid list), from loops over the rows."""
    out = []
    for op, vals, valid in aggs:
        members = [[] for _ in range(ng)]
        for i, g in enumerate(gmap):
            if valid is None or valid[i]:
                members[int(g)].append(None if vals is None else vals[i])
        kind = None if vals is None else vals.dtype.kind
        res, ok = [], []
        for m in members:
            ok.append(op == H.HMJ_AGG_COUNT or len(m) > 0)
            if op == H.HMJ_AGG_COUNT:
                res.append(len(m))
            elif not m:
                res.append(0)
            elif op == H.HMJ_AGG_SUM and kind in "iu":
                s = sum(int(x) for x in m)
                res.append(((s + (1 << 63)) % (1 << 64)) - (1 << 63) if kind == "i" else s % (1 << 64))
            elif op in (H.HMJ_AGG_SUM, H.HMJ_AGG_MEAN):
                fl = [float(x) for x in m]  # (a Python int converts to the nearest double, as the device's conversion does)
                if all(math.isfinite(x) for x in fl):
                    s = float(sum(Fraction(x) for x in fl))  # the exact sum, rounded once
                else:
                    s = sum(fl)
                res.append(s / len(m) if op == H.HMJ_AGG_MEAN else s)
            elif kind in "iu":
                res.append(min(int(x) for x in m) if op == H.HMJ_AGG_MIN else max(int(x) for x in m))
            else:
                best = None
                for x in (float(x) for x in m):
                    if math.isnan(x):
                        continue
                    if best is None or (float_before(x, best) if op == H.HMJ_AGG_MIN else float_before(best, x)):
                        best = x
                res.append(bits_of(math.nan if best is None else best, vals.dtype))
        out.append((res, ok))
    return out


def special_values(dtype, rng, n):
    """n values of the dtype that visit its extremes: integer limits, and for floats NaN, +-0.0, +-inf among numbers."""
    dt = np.dtype(dtype)
    if dt.kind in "iu":
        info = np.iinfo(dt)
        pool = np.array([info.min, info.max, info.min + 1, info.max - 1, 0, 1], dt)
        a = rng.integers(info.min, info.max, size=n, dtype=dt, endpoint=True)
        pick = rng.random(n) < 0.5
        a[pick] = pool[rng.integers(0, len(pool), size=n)][pick]
        return a
    pool = np.array([np.nan, -np.nan, 0.0, -0.0, np.inf, -np.inf, 1.5, -2.25], dt)
    a = (rng.standard_normal(n) * 8).astype(dt)
    pick = rng.random(n) < 0.5
    a[pick] = pool[rng.integers(0, len(pool), size=n)][pick]
    return a


def test_expected_group_aggs_agrees_with_a_brute_force_model():
    import hashmergejoin_amd as H

    rng = np.random.default_rng(20261020)
    ops = (H.HMJ_AGG_COUNT, H.HMJ_AGG_SUM, H.HMJ_AGG_MIN, H.HMJ_AGG_MAX, H.HMJ_AGG_MEAN)
    for n, ng in ((1, 1), (40, 5), (200, 23)):
        gmap = rng.integers(0, ng, size=n)
        gmap[rng.integers(0, n)] = ng - 1
        for dtype in DTYPES:
            for density in (None, 0.3):
                vals = special_values(dtype, rng, n)
                valid = None if density is None else rng.random(n) >= density
                if valid is not None and ng > 2:
                    valid[gmap == 1] = False  # a group with all values NULL
                aggs = [(op, None if (op == H.HMJ_AGG_COUNT and density) else vals, valid) for op in ops]
                got = H.expected_group_aggs(gmap, ng, aggs)
                want = brute_aggs(H, gmap, ng, aggs)
                for (op, _, _), g, (wv, wok) in zip(aggs, got, want):
                    tag = (n, dtype, density, op)
                    assert g["valid"].tolist() == wok, tag
                    assert g["null_count"] == wok.count(False), tag
                    assert g["count"].tolist() == [sum(1 for i in range(n) if gmap[i] == k and (valid is None or valid[i])) for k in range(ng)]
                    v = g["values"]
                    if np.dtype(dtype).kind == "f" and op in (H.HMJ_AGG_MIN, H.HMJ_AGG_MAX):
                        assert v.dtype == np.dtype(dtype), tag
                        assert v.view("u%d" % v.dtype.itemsize).tolist() == [w if ok else 0 for w, ok in zip(wv, wok)], tag
                    elif v.dtype.kind == "f":
                        assert v.dtype == np.float64, tag
                        for a, b in zip(v.tolist(), wv):
                            assert (math.isnan(a) and math.isnan(b)) or a == b, (tag, a, b)
                    else:
                        assert v.tolist() == wv, tag
                    want_dtype = {H.HMJ_AGG_COUNT: "uint64", H.HMJ_AGG_MEAN: "float64",
                                  H.HMJ_AGG_SUM: {"i": "int64", "u": "uint64", "f": "float64"}[np.dtype(dtype).kind]}.get(op, dtype)
                    assert v.dtype == np.dtype(want_dtype), tag


def test_directed_cases_of_the_reference():
    import hashmergejoin_amd as H

    g = [0, 0, 0, 1, 1, 2]
    S, MN, MX, ME, CN = H.HMJ_AGG_SUM, H.HMJ_AGG_MIN, H.HMJ_AGG_MAX, H.HMJ_AGG_MEAN, H.HMJ_AGG_COUNT
    i8 = np.array([127, 127, 3, -128, -128, 5], np.int8)
    e = H.expected_group_aggs(g, 3, [(S, i8, None), (ME, i8, None)])
    assert e[0]["values"].tolist() == [257, -256, 5] and e[0]["values"].dtype == np.int64  # past an int8, not wrapped at 8 bits
    assert e[1]["values"].tolist() == [257 / 3, -128.0, 5.0]
    i64 = np.array([2 ** 63 - 1, 1, 0, -2 ** 63, -1, 7], np.int64)
    u64 = np.array([2 ** 64 - 1, 2, 0, 5, 6, 7], np.uint64)
    e = H.expected_group_aggs(g, 3, [(S, i64, None), (S, u64, None), (ME, i64, None)])
    assert e[0]["values"].tolist() == [-2 ** 63, 2 ** 63 - 1, 7] and e[1]["values"].tolist() == [1, 11, 7]
    assert e[2]["values"].tolist()[0] == float(2 ** 63) / 3  # the mean is not the wrapped sum's
    f = np.array([-0.0, 0.0, np.nan, np.nan, np.nan, -np.inf], np.float64)
    e = H.expected_group_aggs(g, 3, [(MN, f, None), (MX, f, None), (CN, None, np.array([1, 0, 0, 0, 0, 1], bool))])
    assert e[0]["values"].view(np.uint64).tolist() == [1 << 63, 0x7FF8000000000000, 0xFFF0000000000000]
    assert e[1]["values"].view(np.uint64).tolist() == [0, 0x7FF8000000000000, 0xFFF0000000000000]
    assert e[2]["values"].tolist() == [1, 0, 1] and e[2]["null_count"] == 0
    # what lies under a NULL slot is not read
    ok = np.array([1, 0, 1, 0, 0, 1], bool)
    a, b = np.array([1.0, 2.0, 3.0, 4.0, 5.0, 6.0]), np.array([1.0, np.nan, 3.0, np.inf, -7.0, 6.0])
    for op in (S, MN, MX, ME):
        x, y = H.expected_group_aggs(g, 3, [(op, a, ok), (op, b, ok)])
        assert x["values"].tolist() == y["values"].tolist() and x["valid"].tolist() == [True, False, True] and x["null_count"] == 1


# ---- comparing a result with the reference (shared with test_group_agg_gpu.py) ---------------------------------------------------
def gamma(k):
    """gamma_k = k u / (1 - k u), u = 2^-53: the relative bound, against sum |x|, of a sum of k doubles in any order."""
    return k * U / (1.0 - k * U)


def assert_aggs(H, got, want, aggs, n_groups, tag=""):
    """got: per aggregate (values numpy, validity bools or None, null_count) as the device gave them; want: what
    `expected_group_aggs` returns for `aggs`.  Integers, counts and every MIN / MAX are compared exactly (floats bit for
    bit); float SUM and every MEAN under the bound any order of summation satisfies, |got - fsum| <= gamma_k sum|x| (MEAN:
    gamma_(k+1), over the count); a reference that is not finite is matched as it is.  Every figure is printed first."""
    for k, ((v, ok, nulls), w, a) in enumerate(zip(got, want, aggs)):
        op, t = int(a[0]), (k, tag, int(a[0]), None if a[1] is None else str(a[1].dtype))
        assert len(v) == n_groups and v.dtype == w["values"].dtype, t
        assert nulls == w["null_count"], (t, nulls, w["null_count"])
        if ok is not None:
            assert ok.tolist() == w["valid"].tolist(), t
        if w["abs_sum"] is None:
            assert v.view("u%d" % v.dtype.itemsize).tolist() == w["values"].view("u%d" % v.dtype.itemsize).tolist(), t
            continue
        cnt = w["count"]
        for g in range(n_groups):
            x, y, kk = float(v[g]), float(w["values"][g]), int(cnt[g])
            if kk == 0:
                assert x == 0.0 and bits_of(v[g], v.dtype) == 0, (t, g)
            elif not (math.isfinite(y) and math.isfinite(float(w["abs_sum"][g]))):
                assert (math.isnan(x) and math.isnan(y)) or x == y, (t, g, x, y)
            else:
                mean = op == H.HMJ_AGG_MEAN
                bound = gamma(kk + 1) * float(w["abs_sum"][g]) / kk if mean else gamma(kk) * float(w["abs_sum"][g])
                if abs(x - y) > bound:
                    print("aggregate %d group %d: got %r want %r |diff| %.3e bound %.3e k %d" % (k, g, x, y, abs(x - y), bound, kk))
                assert abs(x - y) <= bound, (t, g, x, y, bound)


def test_assert_aggs_accepts_the_reference_and_refuses_a_wrong_bit():
    import hashmergejoin_amd as H

    rng = np.random.default_rng(3)
    gmap = rng.integers(0, 7, size=300)
    f = rng.standard_normal(300) * 2.0 ** rng.integers(-15, 15, size=300)
    i = rng.integers(-100, 100, size=300, dtype=np.int32)
    aggs = [(H.HMJ_AGG_SUM, f, None), (H.HMJ_AGG_MEAN, i, None), (H.HMJ_AGG_MIN, f.astype(np.float32), None), (H.HMJ_AGG_SUM, i, None)]
    want = H.expected_group_aggs(gmap, 7, aggs)
    as_got = lambda w: (w["values"].copy(), w["valid"].copy(), w["null_count"])
    assert_aggs(H, [as_got(w) for w in want], want, aggs, 7)
    naive = [as_got(w) for w in want]
    naive[0] = (np.array([np.sum(f[gmap == g]) for g in range(7)]), want[0]["valid"], 0)  # numpy's order of summation: inside the bound
    assert_aggs(H, naive, want, aggs, 7)
    for k, delta in ((0, 1e-9), (3, 1)):
        bad = [as_got(w) for w in want]
        bad[k][0][2] += delta
        try:
            assert_aggs(H, bad, want, aggs, 7)
        except AssertionError:
            continue
        raise AssertionError("a wrong value passed (aggregate %d)" % k)


# ---- the randomized sweep's draws (shared with test_group_agg_gpu.py) -----------------------------------------------------------
def draw_values(rng, n, dtype, op_is_order):
    """A drawn column: integers over the whole range with the extremes mixed in; floats for SUM / MEAN spanning about 30
    binades with mixed signs (finite: the bound needs a finite sum of |x|), floats for MIN / MAX with NaN, +-0.0 and +-inf."""
    dt = np.dtype(dtype)
    if dt.kind in "iu" or op_is_order:
        return special_values(dtype, rng, n)
    return (rng.standard_normal(n) * 2.0 ** rng.integers(-15, 15, size=n)).astype(dt)


def draw_agg_case(rng, H):
    """One draw of the sweep: n <= 6000 rows grouped by one uint64 key column (the packed form: no draw can be
    HMJ_E_UNSUPPORTED) of drawn cardinality 1..n, ordered or not, and 1-6 aggregates of drawn type and op with a drawn NULL
    density of 0, about 10 % or about 90 % and a bitmap at bit offset 0, 3 or 67.  Returns {"n", "key", "ordered", "aggs":
    [(op, values or None, valid or None, bit_offset)]} in numpy."""
    n = int(rng.choice([1, 2, 63, 64, 65, 511, 512, 513, 2047, 2048, 2049, 4097, 6000]))
    if rng.random() < 0.5:
        n = int(rng.integers(1, 6001))
    card = int(rng.choice([1, 2, 7, 100, n])) if rng.random() < 0.6 else int(rng.integers(1, n + 1))
    pool = rng.integers(0, 1 << 64, size=card, dtype=np.uint64)
    key = pool[rng.integers(0, card, size=n)]
    if rng.random() < 0.5:
        key = np.sort(key)  # long runs in row order as well
    aggs = []
    for _ in range(int(rng.integers(1, 7))):
        op = int(rng.choice([H.HMJ_AGG_COUNT, H.HMJ_AGG_SUM, H.HMJ_AGG_MIN, H.HMJ_AGG_MAX, H.HMJ_AGG_MEAN]))
        dtype = DTYPES[int(rng.integers(0, len(DTYPES)))]
        density = float(rng.choice([0.0, 0.1, 0.9]))
        valid = (rng.random(n) >= density) if density else None
        vals = draw_values(rng, n, dtype, op in (H.HMJ_AGG_MIN, H.HMJ_AGG_MAX))
        if op == H.HMJ_AGG_COUNT and rng.random() < 0.5:
            vals = None
        aggs.append((op, vals, valid, int(rng.choice([0, 3, 67]))))
    return {"n": n, "key": key, "ordered": bool(rng.random() < 0.5), "aggs": aggs}


def sweep_params():
    return int(os.environ.get("HMJ_STRESS_SEED", SWEEP_SEED)), int(os.environ.get("HMJ_STRESS_ITERS", SWEEP_ITERS))


def test_the_default_sweep_draws_every_op_type_and_density():
    import hashmergejoin_amd as H

    rng = np.random.default_rng(SWEEP_SEED)
    ops, types, nulls, sizes = set(), set(), set(), []
    for _ in range(SWEEP_ITERS):
        case = draw_agg_case(rng, H)
        assert 1 <= case["n"] <= 6000 and len(case["key"]) == case["n"] and case["key"].dtype == np.uint64 and 1 <= len(case["aggs"]) <= 6
        sizes.append(case["n"])
        for op, vals, valid, off in case["aggs"]:
            ops.add(op)
            types.add(None if vals is None else str(vals.dtype))
            nulls.add(None if valid is None else bool(np.count_nonzero(valid) * 2 > len(valid)))
            assert off in (0, 3, 67) and (vals is not None or op == H.HMJ_AGG_COUNT)
    assert ops == {0, 1, 2, 3, 4} and types >= set(DTYPES) and nulls == {None, True, False} and max(sizes) > 2048
