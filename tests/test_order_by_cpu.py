"""CPU-only checks of hmj_order_by_device (include/hmj.h, "ordering rows by typed, string and mixed keys"): the library
exports the entry and refuses a NULL ctx, both new structs and every new constant have the values the ctypes mirrors assume
and the ABI version is unchanged, and `expected_order_by` -- the numpy reference test_order_by_gpu.py compares the device
with -- agrees with a comparator written out here in plain Python (`brute_order`) and with np.lexsort.  The byte stream the
header describes is restated too (`stream_of`): its memcmp order must be the requested order, its length what
`order_stream_bytes` says.  Also here, shared with the GPU file: the hand-made tables (`edge_tables`) and the draws of the
randomized sweep (`draw_order_case`) with their ledger."""
import ctypes as C
import functools
import math
import os
import subprocess
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HMJ_E_ARG = -1
SWEEP_SEED, SWEEP_ITERS = 20261020, 20  # HMJ_STRESS_SEED / HMJ_STRESS_ITERS override them
DTYPES = ("int8", "int16", "int32", "int64", "uint8", "uint16", "uint32", "uint64", "float32", "float64")  # HMJ_TYPE_* order
STRING = "string"
DESC, NULLS_FIRST = 1, 2
F32_BITS = [0x7FC00000, 0xFFC00001, 0x7F800001, 0xFFFFFFFF, 0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x00000001, 0x80000001,
            0x007FFFFF, 0x3FC00000, 0xC0100000, 0x7F7FFFFF, 0xFF7FFFFF]
F64_BITS = [0x7FF8000000000000, 0xFFF8000000000001, 0x7FF0000000000001, 0xFFFFFFFFFFFFFFFF, 0x0000000000000000, 0x8000000000000000,
            0x7FF0000000000000, 0xFFF0000000000000, 0x0000000000000001, 0x8000000000000001, 0x000FFFFFFFFFFFFF, 0x3FF8000000000000,
            0xC002000000000000, 0x7FEFFFFFFFFFFFFF, 0xFFEFFFFFFFFFFFFF]


# ---- the entry and its structs -----------------------------------------------------------------------------------------------
def test_the_library_exports_the_entry_and_refuses_a_null_ctx():
    import hashmergejoin_amd as H

    L = H.load_library()
    assert hasattr(L, "hmj_order_by_device")
    col, opts = H.OrderCol(), H.OrderOpts()
    opts.struct_size = C.sizeof(H.OrderOpts)
    assert L.hmj_order_by_device(None, C.byref(col), 1, 0, None, C.byref(opts)) == HMJ_E_ARG
    for name in ["OrderCol", "OrderOpts", "HMJ_ORDER_LARGE_STRING", "HMJ_ORDER_DESC", "HMJ_ORDER_NULLS_FIRST", "HMJ_MAX_ORDER_COLS",
                 "expected_order_by", "order_stream_bytes"]:
        assert name in H.__all__ and hasattr(H, name), name
    assert hasattr(H.Executor, "order_by_device")
    assert (H.HMJ_ORDER_DESC, H.HMJ_ORDER_NULLS_FIRST) == (DESC, NULLS_FIRST)


def test_struct_layouts_and_constants_match_the_header_and_the_abi_version_stays():
    import hashmergejoin_amd as H

    structs = {"hmj_order_col": (H.OrderCol, ["type", "flags", "data", "offsets", "validity"]),
               "hmj_order_opts": (H.OrderOpts, ["struct_size", "reserved", "n_distinct", "n_tied_rows", "n_rounds", "reserved2", "ms_key",
                                                "ms_sort", "ms_refine", "ms_map"])}
    consts = ["HMJ_ORDER_LARGE_STRING", "HMJ_ORDER_DESC", "HMJ_ORDER_NULLS_FIRST", "HMJ_MAX_ORDER_COLS", "HMJ_ABI_VERSION"]
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
    assert [got[k] for k in consts[:4]] == [16, 1, 2, 8]
    assert got["HMJ_ABI_VERSION"] == 5  # a new entry with structs of its own: nothing existing changed
    assert H.load_library().hmj_abi_version() == 5


# ---- the order rule, written out ---------------------------------------------------------------------------------------------
def cmp_values(a, b):
    """-1 / 0 / 1 for two valid values of one column, ascending: Python ints, Python floats (numpy scalars converted by the
    caller; every NaN one value above +inf, -0.0 < +0.0) or bytes (unsigned bytes, then length)."""
    if isinstance(a, bytes):
        for x, y in zip(a, b):
            if x != y:
                return -1 if x < y else 1
        return (len(a) > len(b)) - (len(a) < len(b))
    if isinstance(a, float):
        na, nb = math.isnan(a), math.isnan(b)
        if na or nb:
            return int(na) - int(nb)
        if a != b:
            return -1 if a < b else 1
        sa, sb = math.copysign(1.0, a), math.copysign(1.0, b)
        return (sa > sb) - (sa < sb)
    return (a > b) - (a < b)


def brute_order(columns):
    """The map by a comparator over Python values: columns as `expected_order_by` takes them."""
    cols = []
    for c in columns:
        vals, flags = c[0], c[1]
        valid = c[2] if len(c) > 2 else None
        if isinstance(vals, np.ndarray):
            py = [float(v) if vals.dtype.kind == "f" else int(v) for v in vals]
        else:
            py = [None if v is None else bytes(v) for v in vals]
        ok = [(valid is None or bool(valid[i])) and py[i] is not None for i in range(len(py))]
        cols.append((py, flags, ok))
    n = len(cols[0][0]) if cols else 0

    def cmp_rows(i, j):
        for py, flags, ok in cols:
            if not ok[i] or not ok[j]:
                if ok[i] == ok[j]:
                    continue  # two NULL slots are equal
                null_is_i = not ok[i]
                first = bool(flags & NULLS_FIRST)  # absolute: the direction does not move the NULLs
                return -1 if null_is_i == first else 1
            c = cmp_values(py[i], py[j])
            if flags & DESC:
                c = -c
            if c:
                return c
        return (i > j) - (i < j)

    return np.array(sorted(range(n), key=functools.cmp_to_key(cmp_rows)), np.uint64)


def stream_of(columns, i):
    """Row i's order-preserving byte stream as include/hmj.h describes it."""
    out = bytearray()
    for c in columns:
        vals, flags = c[0], c[1]
        valid = c[2] if len(c) > 2 else None
        is_str = not isinstance(vals, np.ndarray)
        holes = is_str and any(v is None for v in vals)
        ok = (valid is None or bool(valid[i])) and not (is_str and vals[i] is None)
        if valid is not None or holes:
            out.append((1 if ok else 0) if flags & NULLS_FIRST else (0 if ok else 1))
        inv = 0xFF if flags & DESC else 0
        if not is_str:
            w = vals.dtype.itemsize
            if not ok:
                out += bytes(w)
                continue
            bits = int(vals[i:i + 1].view("u%d" % w)[0])
            top = 1 << (8 * w - 1)
            if vals.dtype.kind == "i":
                bits ^= top
            elif vals.dtype.kind == "f":
                if (bits & (top - 1)) > ((0x7F800000 if w == 4 else 0x7FF0000000000000)):
                    bits = (1 << (8 * w)) - 1
                elif bits & top:
                    bits ^= (1 << (8 * w)) - 1
                else:
                    bits |= top
            out += bytes(b ^ inv for b in bits.to_bytes(w, "big"))
        elif ok:
            s = bytes(vals[i])
            blocks = max(1, -(-len(s) // 7))
            for k in range(blocks):
                part = s[7 * k:7 * k + 7]
                ctl = 0xFF if k + 1 < blocks else len(part)
                out += bytes(b ^ inv for b in part + bytes(7 - len(part)) + bytes([ctl]))
    return bytes(out)


def special_values(dtype, rng, n, distinct=None):
    """n values of the dtype that visit its extremes -- integer limits, -1, 0; floats: NaNs of both signs and several
    payloads, +-0.0, +-inf, denormals -- drawn from a pool of `distinct` values (default: the whole pool of extremes + 8)."""
    dt = np.dtype(dtype)
    if dt.kind in "iu":
        info = np.iinfo(dt)
        pool = [info.min, info.max, info.min + 1, info.max - 1, 0, 1] + ([-1, -2] if dt.kind == "i" else [2, 3])
        pool = np.concatenate([np.array(pool, dt), rng.integers(info.min, info.max, size=8, dtype=dt, endpoint=True)])
    else:
        bits = np.array(F32_BITS if dt.itemsize == 4 else F64_BITS, "u%d" % dt.itemsize)
        pool = np.concatenate([bits.view(dt), (rng.standard_normal(8) * 8).astype(dt)])
    if distinct is not None:
        pool = pool[rng.permutation(len(pool))[:max(1, distinct)]]
    return pool[rng.integers(0, len(pool), size=n)]


EDGE_STRINGS = [b"", b"\x00", b"\x00\x00", b"\xff", b"abcdef", b"abcdefg", b"abcdefgh", b"abcdefg\x00", b"abcdef\x00", b"abcdef\xff",
                b"abcdefghijklm", b"abcdefghijklmn", b"abcdefghijklmno", b"abcdefghijklmn\x00", b"abcdefghijklm\xff", b"abcdefghijklmn\xff",
                b"abcdefh", b"abcdef\x00\x00", b"\xff\xff\xff\xff\xff\xff\xff", b"\xff\xff\xff\xff\xff\xff\xff\xff", b"b", b"a"]


def edge_tables(rng=None):
    """(tag, columns) hand-made tables: every type with its edge values ascending and descending, the strings of every block
    boundary, NULL against empty, DESC x NULLS FIRST in all four combinations, and a few multi-column ones."""
    rng = np.random.default_rng(7) if rng is None else rng
    out = []
    for dtype in DTYPES:
        vals = special_values(dtype, rng, 96)
        for flags in (0, DESC):
            out.append(("%s flags %d" % (dtype, flags), [(vals, flags, None)]))
        valid = rng.random(96) >= 0.3
        for flags in (0, DESC, NULLS_FIRST, DESC | NULLS_FIRST):
            out.append(("%s nulls flags %d" % (dtype, flags), [(vals, flags, valid)]))
    strs = [EDGE_STRINGS[k] for k in rng.integers(0, len(EDGE_STRINGS), size=90)] + EDGE_STRINGS
    valid = rng.random(len(strs)) >= 0.25
    valid[:4] = [True, False, True, False]
    strs[0], strs[1] = b"", b""  # a NULL string against the empty string
    for flags in (0, DESC, NULLS_FIRST, DESC | NULLS_FIRST):
        out.append(("strings flags %d" % flags, [(list(strs), flags, None)]))
        out.append(("strings nulls flags %d" % flags, [(list(strs), flags, valid)]))
    n = len(strs)
    i8 = special_values("int8", rng, n, 2)
    f32 = special_values("float32", rng, n, 5)
    out.append(("i8, strings desc", [(i8, 0, None), (list(strs), DESC, valid)]))
    out.append(("strings, f32 desc nulls first, i8 desc", [(list(strs), 0, None), (f32, DESC | NULLS_FIRST, valid), (i8, DESC, None)]))
    out.append(("f32 nulls, strings nulls first", [(f32, 0, ~valid), (list(strs), NULLS_FIRST, valid)]))
    return out


@pytest.mark.parametrize("tag,columns", edge_tables(), ids=[t for t, _ in edge_tables()])
def test_the_reference_agrees_with_the_comparator_and_the_stream(tag, columns):
    import hashmergejoin_amd as H

    want = brute_order(columns)
    got = H.expected_order_by(columns)
    assert got.dtype == np.uint64 and np.array_equal(got, want), tag
    n = len(want)
    streams = [stream_of(columns, i) for i in range(n)]
    by_stream = sorted(range(n), key=lambda i: (streams[i], i))
    assert by_stream == [int(x) for x in want], tag + ": the stream's memcmp order is not the requested order"
    assert np.array_equal(H.order_stream_bytes(columns), np.array([len(s) for s in streams], np.int64)), tag
    distinct = sorted(set(streams))
    for a, b in zip(distinct, distinct[1:]):  # prefix-free: no stream begins another
        assert not b.startswith(a), tag


def test_float_order_is_ieee_with_signed_zeros_and_one_nan():
    import hashmergejoin_amd as H

    for dt, bits in (("float32", F32_BITS), ("float64", F64_BITS)):
        vals = np.array(bits, "u%d" % np.dtype(dt).itemsize).view(dt)
        got = [int(i) for i in H.expected_order_by([(vals, 0, None)])]
        # -inf, -max, -1.5.., -denormal, -0.0, +0.0, denormal, ..., +max, +inf, then the four NaNs in row order
        assert got[-4:] == [0, 1, 2, 3] and got[0] == 7 and got[-5] == 6
        assert got.index(5) + 1 == got.index(4)  # -0.0 right in front of +0.0
        desc = [int(i) for i in H.expected_order_by([(vals, DESC, None)])]
        assert desc[:4] == [0, 1, 2, 3] and desc[4] == 6 and desc[-1] == 7


def test_integer_columns_agree_with_lexsort():
    import hashmergejoin_amd as H

    rng = np.random.default_rng(11)
    n = 3000
    a = rng.integers(-5, 5, size=n).astype(np.int32)
    b = rng.integers(0, 40, size=n).astype(np.uint16)
    c = rng.integers(-2 ** 62, 2 ** 62, size=n).astype(np.int64)
    assert np.array_equal(H.expected_order_by([(a, 0), (b, 0), (c, 0)]), np.lexsort((c, b, a)).astype(np.uint64))
    assert np.array_equal(H.expected_order_by([(a, DESC), (b, 0)]), np.lexsort((b, -a.astype(np.int64))).astype(np.uint64))
    assert np.array_equal(H.order_stream_bytes([(a, 0), (b, 0), (c, 0)]), np.full(n, 14, np.int64))
    assert len(H.expected_order_by([(a[:0], 0)])) == 0


# ---- the randomized sweep's draws ----------------------------------------------------------------------------------------------
def draw_strings(rng, n, distinct, prefix=b""):
    alphabet = [0x00, 0xFF, 0x61, 0x62, 0x80]
    lens = [0, 6, 7, 8, 13, 14, 15, int(rng.integers(1, 30))]
    pool = []
    for _ in range(max(1, distinct)):
        ln = lens[int(rng.integers(0, len(lens)))]
        pool.append(prefix + bytes(alphabet[k] for k in rng.integers(0, len(alphabet), size=ln)))
    return [pool[k] for k in rng.integers(0, len(pool), size=n)]


def draw_order_case(rng, it):
    """Case `it` of a sweep: {"n", "cols": [{"type": a DTYPES name or STRING, "values", "flags", "valid": bools or None,
    "bit_offset", "pad": bytes in front of a string column's first key (offsets[0])}]}.  Four shapes in turn: mixed columns of
    few values; a constant U64 in front (the first 8 stream bytes are all equal); two values over at least 8193 rows (a
    duplicate group beyond 4096 rows); strings behind a shared prefix."""
    shape = it % 4
    kinds = list(DTYPES) + [STRING]
    n = int(rng.integers(1, 1 << 15) if shape != 2 else rng.integers(8193, 1 << 15))
    if shape == 0 and it % 8 == 0:
        n = int(rng.integers(1, 300))
    cols = []

    def column(kind, distinct, prefix=b""):
        flags = int(rng.integers(0, 4))
        if kind == STRING:
            values = draw_strings(rng, n, distinct, prefix)
        else:
            values = special_values(kind, rng, n, distinct)
        valid, off = None, 0
        if rng.random() < 0.5:
            valid = rng.random(n) >= (0.1 if rng.random() < 0.7 else 0.9)
            off = int(rng.choice([0, 3, 67, 8]))
        pad = int(rng.integers(0, 9)) if kind == STRING and rng.random() < 0.6 else 0
        return {"type": kind, "values": values, "flags": flags, "valid": valid, "bit_offset": off, "pad": pad}

    if shape == 1:
        const = column("uint64", 1)
        const["valid"], const["bit_offset"] = None, 0
        cols.append(const)
    if shape == 2:
        cols.append(column(["int8", "uint8", "float32"][it // 4 % 3], 2))
        cols[0]["valid"] = None
    elif shape == 3:
        cols.append(column(STRING, int(rng.integers(2, 200)), prefix=b"shared-prefix:" * int(rng.integers(1, 3))))
    k = int(rng.integers(1, 4)) if shape != 2 else 0
    for c in range(k):
        kind = kinds[(it * 3 + c * 5 + int(rng.integers(0, 2))) % len(kinds)]
        cols.append(column(kind, int(rng.choice([1, 2, 5, 40, 5000]))))
    return {"n": n, "cols": cols}


def case_columns(case):
    """The case as `expected_order_by` takes it."""
    return [(c["values"], c["flags"], c["valid"]) for c in case["cols"]]


def sweep_params():
    return int(os.environ.get("HMJ_STRESS_SEED", SWEEP_SEED)), int(os.environ.get("HMJ_STRESS_ITERS", SWEEP_ITERS))


def test_the_default_sweep_draws_every_type_flag_and_layout():
    import hashmergejoin_amd as H

    rng = np.random.default_rng(SWEEP_SEED)
    types, str_flags, fixed_flags = set(), 0, 0
    offsets, pads, equal_heads, big_group = set(), set(), 0, 0
    for it in range(SWEEP_ITERS):
        case = draw_order_case(rng, it)
        n = case["n"]
        assert 1 <= n <= 1 << 15 and 1 <= len(case["cols"]) <= H.HMJ_MAX_ORDER_COLS
        for c in case["cols"]:
            assert len(c["values"]) == n and (c["valid"] is None or len(c["valid"]) == n) and 0 <= c["flags"] <= 3
            types.add(c["type"])
            if c["type"] == STRING:
                str_flags |= c["flags"]
                pads.add(c["pad"] != 0)
            else:
                fixed_flags |= c["flags"]
                assert c["values"].dtype == np.dtype(c["type"])
            if c["valid"] is not None:
                offsets.add(c["bit_offset"])
        cols = case_columns(case)
        first = case["cols"][0]
        if n > 1 and first["type"] == "uint64" and first["valid"] is None and bool(np.all(first["values"] == first["values"][0])):
            assert len({stream_of(cols, i)[:8] for i in range(min(n, 50))}) == 1
            equal_heads += 1
        want = H.expected_order_by(cols)
        assert sorted(int(x) for x in want) == list(range(n))
        streams = [stream_of(cols, int(i)) for i in want[:: max(1, n // 64)]]
        assert streams == sorted(streams)
        if len(case["cols"]) == 1 and first["type"] != STRING and first["valid"] is None:  # one column: its largest group of equal values
            v = first["values"]
            keys = v.view("u%d" % v.dtype.itemsize).copy()
            if v.dtype.kind == "f":
                keys[np.isnan(v)] = ~keys.dtype.type(0)
            big_group = max(big_group, int(np.unique(keys, return_counts=True)[1].max()))
    assert types == set(DTYPES) | {STRING}, sorted(types)
    assert str_flags == 3 and fixed_flags == 3
    assert any(o != 0 for o in offsets) and 0 in offsets
    assert pads == {True, False}  # offsets[0] != 0 and == 0
    assert equal_heads >= 1, "no case whose first 8 stream bytes are all equal"
    assert big_group > 4096, "no duplicate group beyond 4096 rows"
