"""CPU-only checks of hmj_filter_device (include/hmj.h, "filtering rows: typed and string predicates to a row map"): the
library exports the entry and refuses a NULL ctx, both new structs and every new constant have the values the ctypes mirrors
assume and the ABI version is unchanged, and `expected_filter` -- the numpy reference test_filter_gpu.py compares the device
with -- agrees with an evaluator written out here in plain Python (`brute_filter`: a per-row loop over an explicit TRUE /
FALSE / UNKNOWN enum with Kleene's tables spelled out, not min / max).  Also here, shared with the GPU file: the hand-made
tables (`edge_tables`) and the draws of the randomized sweep (`draw_filter_case`) with their ledger.

A host term is a dict as `expected_filter` takes it -- "column" (a numpy array, or a list of bytes), "op", "lit", "valid"
(bools or None), "row_map" (uint64 or None), "clause", "negate" -- plus what only the device layout needs: "bit_offset" and,
for a string column, "pad" (bytes in front of the first string, offsets[0])."""
import ctypes as C
import enum
import os
import subprocess
import tempfile

import numpy as np
import pytest

from test_order_by_cpu import DTYPES, F32_BITS, F64_BITS, special_values

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HMJ_E_ARG = -1
SWEEP_SEED, SWEEP_ITERS = 20261023, 20  # HMJ_STRESS_SEED / HMJ_STRESS_ITERS override them
EQ, NE, LT, LE, GT, GE, BETWEEN, IS_NULL, IS_NOT_NULL, STARTS_WITH, ENDS_WITH = range(11)
FIXED_OPS = [EQ, NE, LT, LE, GT, GE, BETWEEN, IS_NULL, IS_NOT_NULL]
STRING_OPS = FIXED_OPS + [STARTS_WITH, ENDS_WITH]
NO_ROW = 0xFFFFFFFFFFFFFFFF
STRING = "string"
CONSTS = ["HMJ_FILTER_LARGE_STRING", "HMJ_FILTER_EQ", "HMJ_FILTER_NE", "HMJ_FILTER_LT", "HMJ_FILTER_LE", "HMJ_FILTER_GT", "HMJ_FILTER_GE",
          "HMJ_FILTER_BETWEEN", "HMJ_FILTER_IS_NULL", "HMJ_FILTER_IS_NOT_NULL", "HMJ_FILTER_STARTS_WITH", "HMJ_FILTER_ENDS_WITH",
          "HMJ_FILTER_NOT", "HMJ_MAX_FILTER_TERMS", "HMJ_MAX_FILTER_LITERAL_BYTES"]


def term(column, op, lit=None, valid=None, bit_offset=0, row_map=None, clause=0, negate=False, pad=0):
    return {"column": column, "op": op, "lit": lit, "valid": valid, "bit_offset": bit_offset, "row_map": row_map, "clause": clause,
            "negate": negate, "pad": pad}


# ---- the entry and its structs -----------------------------------------------------------------------------------------------
def test_the_library_exports_the_entry_and_refuses_a_null_ctx():
    import hashmergejoin_amd as H

    L = H.load_library()
    assert hasattr(L, "hmj_filter_device")
    t, opts = H.FilterTerm(), H.FilterOpts()
    opts.struct_size = C.sizeof(H.FilterOpts)
    assert L.hmj_filter_device(None, C.byref(t), 1, 0, None, None, C.byref(opts)) == HMJ_E_ARG
    for name in CONSTS + ["FilterTerm", "FilterOpts", "expected_filter"]:
        assert name in H.__all__ and hasattr(H, name), name
    assert hasattr(H.Executor, "filter_device")
    assert [getattr(H, k) for k in CONSTS[1:12]] == list(range(11))


def test_struct_layouts_and_constants_match_the_header_and_the_abi_version_stays():
    import hashmergejoin_amd as H

    structs = {"hmj_filter_term": (H.FilterTerm, ["type", "op", "flags", "clause", "data", "offsets", "chars_bytes", "validity", "n_src",
                                                  "row_map", "lit", "str_lit", "str_len", "reserved"]),
               "hmj_filter_opts": (H.FilterOpts, ["struct_size", "reserved", "n_out", "n_unknown", "ms_eval", "ms_write", "reserved2"])}
    consts = CONSTS + ["HMJ_ORDER_LARGE_STRING", "HMJ_ABI_VERSION"]
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
    for k in CONSTS:
        assert got[k] == getattr(H, k), k
    assert got["HMJ_FILTER_LARGE_STRING"] == got["HMJ_ORDER_LARGE_STRING"] == 16
    assert (got["HMJ_FILTER_NOT"], got["HMJ_MAX_FILTER_TERMS"], got["HMJ_MAX_FILTER_LITERAL_BYTES"]) == (1, 16, 4096)
    assert got["HMJ_ABI_VERSION"] == 5  # a new entry with structs of its own: nothing existing changed
    assert H.load_library().hmj_abi_version() == 5


# ---- the rule, written out ---------------------------------------------------------------------------------------------------
class TV(enum.Enum):
    FALSE = "false"
    UNKNOWN = "unknown"
    TRUE = "true"


def tv_not(a):
    return {TV.TRUE: TV.FALSE, TV.FALSE: TV.TRUE, TV.UNKNOWN: TV.UNKNOWN}[a]


def tv_or(vals):
    if any(v is TV.TRUE for v in vals):
        return TV.TRUE
    return TV.UNKNOWN if any(v is TV.UNKNOWN for v in vals) else TV.FALSE


def tv_and(vals):
    if any(v is TV.FALSE for v in vals):
        return TV.FALSE
    return TV.UNKNOWN if any(v is TV.UNKNOWN for v in vals) else TV.TRUE


def bytes_cmp(a, b):
    """-1 / 0 / 1 as std::string::operator< orders them: unsigned bytes, then length."""
    for x, y in zip(a, b):
        if x != y:
            return -1 if x < y else 1
    return (len(a) > len(b)) - (len(a) < len(b))


def compare(op, x, lits):
    """TRUE / FALSE of one valid Python value against its literal(s): ints, floats (Python's operators are C's: IEEE) or
    bytes."""
    if isinstance(x, bytes):
        if op == STARTS_WITH:
            return len(x) >= len(lits[0]) and x[:len(lits[0])] == lits[0]
        if op == ENDS_WITH:
            return len(x) >= len(lits[0]) and x[len(x) - len(lits[0]):] == lits[0]
        c = [bytes_cmp(x, l) for l in lits]
        lt, eq, gt = [k < 0 for k in c], [k == 0 for k in c], [k > 0 for k in c]
    else:
        lt, eq, gt = [x < l for l in lits], [x == l for l in lits], [x > l for l in lits]
    if op == EQ:
        return eq[0]
    if op == NE:
        return not eq[0]
    if op == LT:
        return lt[0]
    if op == LE:
        return lt[0] or eq[0]
    if op == GT:
        return gt[0]
    if op == GE:
        return gt[0] or eq[0]
    assert op == BETWEEN
    return (gt[0] or eq[0]) and (lt[1] or eq[1])


def as_python(v, dtype=None):
    if isinstance(v, (bytes, bytearray, str)):
        return v.encode("utf-8") if isinstance(v, str) else bytes(v)
    v = np.array([v], dtype=dtype)[0]  # the literal in the column's own type: no casts on the device
    return float(v) if np.dtype(dtype).kind == "f" else int(v)


def brute_term(t, i):
    col = t["column"]
    r = i if t["row_map"] is None else int(t["row_map"][i])
    null = r == NO_ROW
    if not null:
        assert 0 <= r < len(col)
        null = (t["valid"] is not None and not bool(t["valid"][r])) or col[r] is None
    if t["op"] == IS_NULL:
        v = TV.TRUE if null else TV.FALSE
    elif t["op"] == IS_NOT_NULL:
        v = TV.FALSE if null else TV.TRUE
    elif null:
        v = TV.UNKNOWN
    else:
        dtype = col.dtype if isinstance(col, np.ndarray) else None
        lit = t["lit"]
        lits = [as_python(l, dtype) for l in (lit if isinstance(lit, (tuple, list)) else [lit])]
        v = TV.TRUE if compare(t["op"], as_python(col[r], dtype), lits) else TV.FALSE
    return tv_not(v) if t["negate"] else v


def brute_filter(terms, n, positions=None):
    """[TV of the whole predicate] at every position (or at the given ones): clause by clause, Kleene's OR inside, AND across."""
    out = []
    for i in (range(n) if positions is None else positions):
        clauses, ids = [], []
        for t in terms:
            if not ids or ids[-1] != t["clause"]:
                assert not ids or t["clause"] > ids[-1]
                clauses.append([])
                ids.append(t["clause"])
            clauses[-1].append(brute_term(t, i))
        out.append(tv_and([tv_or(c) for c in clauses]))
    return out


def check_reference(tag, terms, n, sample=None):
    import hashmergejoin_amd as H

    pos, unknown = H.expected_filter(terms, n)
    assert pos.dtype == np.uint64 and np.all(pos[1:] > pos[:-1]) and (len(pos) == 0 or int(pos[-1]) < n), tag
    if sample is None or n <= sample:
        want = brute_filter(terms, n)
        assert [int(p) for p in pos] == [i for i, v in enumerate(want) if v is TV.TRUE], tag
        assert unknown == sum(1 for v in want if v is TV.UNKNOWN), tag
    else:  # a long case: the first and last positions and a stride between them
        at = sorted(set(list(range(64)) + list(range(n - 64, n)) + list(range(0, n, max(1, n // sample)))))
        want = brute_filter(terms, n, at)
        passing = set(int(p) for p in pos)
        assert [i in passing for i in at] == [v is TV.TRUE for v in want], tag
    return pos, unknown


# ---- hand-made tables ------------------------------------------------------------------------------------------------------------
def typed_literals(dtype):
    dt = np.dtype(dtype)
    if dt.kind in "iu":
        info = np.iinfo(dt)
        lits = [1, 0, int(info.max), int(info.min), int(info.max) - 1]
        if dt.kind == "i":
            lits.append(-1)
        if dtype == "uint64":
            lits += [1 << 63, (1 << 63) - 1]
        return lits
    tiny = float(np.array([1], "u%d" % dt.itemsize).view(dt)[0])  # the smallest denormal
    return [0.0, -0.0, float("nan"), float("inf"), float("-inf"), tiny, -tiny, 1.5]


def typed_values(dtype, rng, n=96):
    """Values around the literals: the type's extremes (int8 -1 against the literal 1, uint64 2^63, int64 min and max; NaNs of
    both signs, +-0.0, +-inf, denormals) and the literals themselves."""
    vals = special_values(dtype, rng, n)
    lits = np.array(typed_literals(dtype), dtype=dtype)
    vals[:len(lits)] = lits
    return vals


def typed_tables(dtype, rng=None):
    """(tag, n, terms): every op against every literal of `typed_literals` on one column with NULLs; BETWEEN over every
    ordered pair of neighbours and its reverse (lo > hi selects nothing)."""
    rng = np.random.default_rng(5) if rng is None else rng
    vals = typed_values(dtype, rng)
    valid = rng.random(len(vals)) >= 0.25
    valid[:len(typed_literals(dtype))] = True
    lits = typed_literals(dtype)
    out = []
    for k, lit in enumerate(lits):
        for op in FIXED_OPS:
            arg = None if op in (IS_NULL, IS_NOT_NULL) else ((lit, lits[(k + 1) % len(lits)]) if op == BETWEEN else lit)
            for negate in (False, True):
                if negate and k > 1:
                    continue
                out.append(("%s op %d lit %r%s" % (dtype, op, arg, " not" if negate else ""), len(vals),
                            [term(vals, op, arg, valid, bit_offset=(3 * k) % 11, negate=negate)]))
    return out


LONG_ROW = b"abcd" + bytes(range(256)) * 17 + b"abcd"  # 4360 bytes: longer than any literal may be
STRING_VALUES = [b"", b"", b"abcd", b"abc", b"abcde", b"abcdefghijklmnop", b"abcdefgh", b"abcdefg", b"abcdefghi", b"xbcd", b"abcx",
                 b"\x80\xff", b"\x7f", b"\xff", b"a\x00b", b"a\x00", b"a", b"\x00", b"\x00\x00", b"abcdefgh\x80bcdefgh", b"abcdefghabcdefgh",
                 b"zzabcd", b"abcdabcd", LONG_ROW, LONG_ROW[:-1], LONG_ROW + b"\x00", b"abcdefghijklmnopqrstuv"]
STRING_LITERALS = [b"", b"abcd", b"abcdefgh", b"abcdefghi", b"abcdefghabcdefgh", b"\x80\xff", b"a\x00b", b"\x00", b"\xff",
                   LONG_ROW[:4000], LONG_ROW[-4000:], b"abcdefghijklmnopqrstuv"]


def string_tables(rng=None):
    """(tag, n, terms) on one string column: the empty string, NULL against empty (rows 0 and 1), proper prefixes both ways,
    bytes >= 0x80 and NUL, rows beyond 4096 bytes, every op against every literal -- the empty one and two of 4000 bytes
    among them --, offsets[0] != 0."""
    rng = np.random.default_rng(6) if rng is None else rng
    vals = STRING_VALUES + [STRING_VALUES[k] for k in rng.integers(0, len(STRING_VALUES), size=70)]
    valid = rng.random(len(vals)) >= 0.2
    valid[:len(STRING_VALUES)] = True
    valid[1] = False  # NULL against the empty string of row 0
    out = []
    for k, lit in enumerate(STRING_LITERALS):
        for op in STRING_OPS:
            arg = None if op in (IS_NULL, IS_NOT_NULL) else ((lit, STRING_LITERALS[(k + 1) % len(STRING_LITERALS)]) if op == BETWEEN else lit)
            if op == BETWEEN and len(arg[0]) + len(arg[1]) > 4096:
                arg = (lit, b"abcd")
            out.append(("strings op %d lit %d" % (op, k), len(vals), [term(vals, op, arg, valid, bit_offset=k % 9, pad=k % 5, negate=(k == 1))]))
    short = [v for v in vals if len(v) < 20]
    out.append(("a literal longer than every row", len(short), [term(short, op, b"abcdefghijklmnopqrstuvwxyz", None, clause=c)
                                                                for c, op in enumerate([NE, LT, GE])]))
    return out


def mixed_tables(rng=None):
    """(tag, n, terms): multi-term predicates -- an IN-list, the issue's `price < 100 AND (region = 'EU' OR region IS NULL)`,
    maps with HMJ_TAKE_NO_ROW, two maps over relations of different sizes."""
    rng = np.random.default_rng(8) if rng is None else rng
    n = 300
    price = rng.integers(0, 200, size=n).astype(np.int32)
    region = [[b"EU", b"US", b"APAC", b""][k] for k in rng.integers(0, 4, size=n)]
    rvalid = rng.random(n) >= 0.3
    out = [("price < 100 and (region = EU or region is null)", n,
            [term(price, LT, 100), term(region, EQ, b"EU", rvalid, 5, clause=1), term(region, IS_NULL, None, rvalid, 5, clause=1)]),
           ("in-list", n, [term(price, EQ, v) for v in (3, 77, 150, 199, 0)]),
           ("not in-list, nulls", n, [term(price, EQ, v, rvalid, clause=c, negate=True) for c, v in enumerate((3, 77, 150))])]
    ns_r, ns_s = 50, 411
    r_row = rng.integers(0, ns_r, size=n).astype(np.uint64)
    s_row = rng.integers(0, ns_s, size=n).astype(np.uint64)
    r_row[rng.random(n) < 0.2] = NO_ROW
    s_row[rng.random(n) < 0.2] = NO_ROW
    ra = rng.standard_normal(ns_r).astype(np.float64)
    sb = rng.integers(0, 5, size=ns_s).astype(np.uint8)
    sv = rng.random(ns_s) >= 0.5
    out.append(("two maps, two relations", n, [term(ra, GT, 0.0, row_map=r_row), term(sb, BETWEEN, (1, 3), sv, 7, s_row, clause=0),
                                               term(sb, IS_NULL, None, sv, 7, s_row, clause=1), term(ra, IS_NOT_NULL, None, row_map=r_row, clause=1)]))
    out.append(("s.key is null through s_row", n, [term(sb, IS_NULL, None, None, 0, s_row)]))
    return out


def edge_tables():
    out = []
    for dtype in DTYPES:
        out += typed_tables(dtype)
    return out + string_tables() + mixed_tables()


def test_the_reference_agrees_with_the_evaluator_on_the_hand_made_tables():
    tables = edge_tables()
    assert len(tables) > 500
    for tag, n, terms in tables:
        check_reference(tag, terms, n)


def test_float_comparisons_are_ieee_not_the_order_by_total_order():
    import hashmergejoin_amd as H

    for dt, bits in (("float32", F32_BITS), ("float64", F64_BITS)):
        vals = np.array(bits, "u%d" % np.dtype(dt).itemsize).view(dt)
        nan = np.isnan(vals)
        zeros = np.nonzero(vals == 0)[0]
        assert len(zeros) == 2 and nan.sum() == 4
        pos, unk = H.expected_filter([term(vals, EQ, 0.0)], len(vals))
        assert [int(p) for p in pos] == [int(z) for z in zeros] and unk == 0  # x = 0.0 selects both zeros
        pos, _ = H.expected_filter([term(vals, EQ, -0.0)], len(vals))
        assert [int(p) for p in pos] == [int(z) for z in zeros]
        for op in (EQ, LT, LE, GT, GE):  # a NaN literal: nothing passes; a NaN in the column never passes
            assert len(H.expected_filter([term(vals, op, float("nan"))], len(vals))[0]) == 0
            assert not set(int(p) for p in H.expected_filter([term(vals, op, 1.0)], len(vals))[0]) & set(np.nonzero(nan)[0].tolist())
        assert len(H.expected_filter([term(vals, NE, float("nan"))], len(vals))[0]) == len(vals)
        assert set(np.nonzero(nan)[0].tolist()) <= set(int(p) for p in H.expected_filter([term(vals, NE, 1.0)], len(vals))[0])
        assert len(H.expected_filter([term(vals, BETWEEN, (float("-inf"), float("inf")))], len(vals))[0]) == len(vals) - 4
        assert len(H.expected_filter([term(vals, BETWEEN, (1.0, -1.0))], len(vals))[0]) == 0


def test_the_three_valued_truth_table():
    """Two nullable columns x {T, F, U}^2 x NOT on either term x same clause / different clauses, against the table written
    out: OR and AND of Kleene's logic."""
    import hashmergejoin_amd as H

    states = [TV.TRUE, TV.FALSE, TV.UNKNOWN]
    pairs = [(a, b) for a in states for b in states]
    value = {TV.TRUE: 1, TV.FALSE: 0, TV.UNKNOWN: 77}  # the literal is 1; 77 lies under a NULL slot
    a = np.array([value[p[0]] for p in pairs], np.int16)
    b = np.array([value[p[1]] for p in pairs], np.int16)
    va = np.array([p[0] is not TV.UNKNOWN for p in pairs])
    vb = np.array([p[1] is not TV.UNKNOWN for p in pairs])
    OR = {(TV.TRUE, TV.TRUE): TV.TRUE, (TV.TRUE, TV.FALSE): TV.TRUE, (TV.TRUE, TV.UNKNOWN): TV.TRUE, (TV.FALSE, TV.TRUE): TV.TRUE,
          (TV.FALSE, TV.FALSE): TV.FALSE, (TV.FALSE, TV.UNKNOWN): TV.UNKNOWN, (TV.UNKNOWN, TV.TRUE): TV.TRUE,
          (TV.UNKNOWN, TV.FALSE): TV.UNKNOWN, (TV.UNKNOWN, TV.UNKNOWN): TV.UNKNOWN}
    AND = {(TV.TRUE, TV.TRUE): TV.TRUE, (TV.TRUE, TV.FALSE): TV.FALSE, (TV.TRUE, TV.UNKNOWN): TV.UNKNOWN, (TV.FALSE, TV.TRUE): TV.FALSE,
           (TV.FALSE, TV.FALSE): TV.FALSE, (TV.FALSE, TV.UNKNOWN): TV.FALSE, (TV.UNKNOWN, TV.TRUE): TV.UNKNOWN,
           (TV.UNKNOWN, TV.FALSE): TV.FALSE, (TV.UNKNOWN, TV.UNKNOWN): TV.UNKNOWN}
    for not_a in (False, True):
        for not_b in (False, True):
            for table, clause_b in ((OR, 0), (AND, 1)):
                terms = [term(a, EQ, 1, va, negate=not_a), term(b, EQ, 1, vb, clause=clause_b, negate=not_b)]
                want = [table[(tv_not(x) if not_a else x, tv_not(y) if not_b else y)] for x, y in pairs]
                assert brute_filter(terms, len(pairs)) == want
                pos, unk = H.expected_filter(terms, len(pairs))
                assert [int(p) for p in pos] == [i for i, v in enumerate(want) if v is TV.TRUE], (not_a, not_b, clause_b)
                assert unk == sum(1 for v in want if v is TV.UNKNOWN)


def truth_table_cases():
    """The same 8 predicates as (tag, n, terms), for the GPU file."""
    states = [2, 0, 1]
    pairs = [(x, y) for x in states for y in states]
    a = np.array([{2: 1, 0: 0, 1: 77}[p[0]] for p in pairs], np.int16)
    b = np.array([{2: 1, 0: 0, 1: 77}[p[1]] for p in pairs], np.int16)
    va, vb = np.array([p[0] != 1 for p in pairs]), np.array([p[1] != 1 for p in pairs])
    return [("3vl not_a %d not_b %d clause_b %d" % (na, nb, cb), len(pairs),
             [term(a, EQ, 1, va, negate=bool(na)), term(b, EQ, 1, vb, clause=cb, negate=bool(nb))])
            for na in (0, 1) for nb in (0, 1) for cb in (0, 1)]


def test_the_reference_rejects_what_the_library_rejects():
    import hashmergejoin_amd as H

    a = np.arange(10, dtype=np.int32)
    with pytest.raises(ValueError):
        H.expected_filter([term(a, EQ, 1)], 11)  # n_src < n without a map
    with pytest.raises(ValueError):
        H.expected_filter([term(a, EQ, 1, row_map=np.array([10], np.uint64))], 1)  # a map entry >= n_src
    with pytest.raises(ValueError):
        H.expected_filter([term(a, EQ, 1, clause=1), term(a, EQ, 2, clause=0)], 5)
    with pytest.raises(ValueError):
        H.expected_filter([term(a, STARTS_WITH, 1)], 5)
    pos, unk = H.expected_filter([term(a, EQ, 1)], 0)
    assert len(pos) == 0 and unk == 0


# ---- the randomized sweep's draws ----------------------------------------------------------------------------------------------
def draw_strings(rng, n, distinct):
    alphabet = [0x00, 0xFF, 0x61, 0x62, 0x80]
    stems = [b"", b"abcdefgh", b"abcdefghijklmnopqrstuv"]
    pool = []
    for _ in range(max(1, distinct)):
        ln = int(rng.choice([0, 1, 3, 7, 8, 9, 15, 16, 17, int(rng.integers(1, 40))]))
        pool.append(stems[int(rng.integers(0, 3))] + bytes(alphabet[k] for k in rng.integers(0, len(alphabet), size=ln)))
    return [pool[k] for k in rng.integers(0, len(pool), size=n)], pool


def draw_filter_case(rng, it):
    """Case `it` of a sweep: {"n", "terms"} with 1..16 terms in 1..5 clauses over up to six relations, each read directly (its
    rows >= n) or through a map of its own (rows of any count, HMJ_TAKE_NO_ROW entries).  Terms of one relation share the map
    OBJECT, as the device terms must share the pointer.  The term count visits every unrolled body (1, 2, 3..4, 5..8, 9..16)
    in turn; sizes: up to 300, up to 4096, up to 2^16."""
    n = int([rng.integers(1, 300), rng.integers(1, 4097), rng.integers(4097, (1 << 16) + 1), rng.integers(1, (1 << 16) + 1)][it % 4])
    lo, hi = [(1, 1), (2, 2), (3, 4), (5, 8), (9, 16)][it % 5]
    n_terms = int(rng.integers(lo, hi + 1))
    n_rel = int(rng.integers(1, 7))
    rels = []
    for _ in range(n_rel):
        if rng.random() < 0.4:
            rels.append((n + int(rng.integers(0, 50)), None))
        else:
            ns = int(rng.integers(1, 2 * n + 2))
            m = rng.integers(0, ns, size=n).astype(np.uint64)
            if rng.random() < 0.7:
                m[rng.random(n) < (0.1 if rng.random() < 0.7 else 0.8)] = NO_ROW
            rels.append((ns, m))
    n_clauses = int(rng.integers(1, min(5, n_terms) + 1))
    cuts = sorted(rng.permutation(n_terms - 1)[:n_clauses - 1] + 1) if n_terms > 1 else []
    kinds = list(DTYPES) + [STRING] * 5
    terms, clause = [], 0
    for k in range(n_terms):
        if k in cuts:
            clause += int(rng.integers(1, 4))
        ns, m = rels[int(rng.integers(0, n_rel))]
        kind = kinds[int(rng.integers(0, len(kinds)))]
        op = (it * 7 + k * 5 + k // 3) % (11 if kind == STRING else 9)
        if kind == STRING:
            col, pool = draw_strings(rng, ns, int(rng.choice([1, 3, 30])))
            pick = lambda: pool[int(rng.integers(0, len(pool)))][:int(rng.integers(0, 30))] if rng.random() < 0.8 else b"abc"  # noqa: E731
            lit = (pick(), pick()) if op == BETWEEN else pick()
            if op == ENDS_WITH and rng.random() < 0.7:
                src = pool[int(rng.integers(0, len(pool)))]
                lit = src[len(src) - int(rng.integers(0, len(src) + 1)):]
        else:
            col = special_values(kind, rng, ns, int(rng.choice([2, 5, 40])))
            pick = lambda: col[int(rng.integers(0, ns))].item()  # noqa: E731
            lit = (pick(), pick()) if op == BETWEEN else pick()
        if op in (IS_NULL, IS_NOT_NULL):
            lit = None
        valid, off = None, 0
        if rng.random() < 0.6:
            valid = rng.random(ns) >= (0.1 if rng.random() < 0.7 else 0.9)
            off = int(rng.choice([0, 1, 7, 63, 69]))
        pad = int(rng.integers(0, 9)) if kind == STRING and rng.random() < 0.6 else 0
        terms.append(term(col, op, lit, valid, off, m, clause, bool(rng.random() < 0.3), pad))
    return {"n": n, "terms": terms}


def sweep_params():
    return int(os.environ.get("HMJ_STRESS_SEED", SWEEP_SEED)), int(os.environ.get("HMJ_STRESS_ITERS", SWEEP_ITERS))


def test_the_default_sweep_reaches_every_feature_and_the_reference_agrees_on_it():
    """The ledger of what the default seed draws, and `expected_filter` against the evaluator on every draw (long cases at a
    stride of positions)."""
    import hashmergejoin_amd as H

    rng = np.random.default_rng(SWEEP_SEED)
    kinds, ops, bodies, offs, pads, negs = set(), set(), set(), set(), set(), set()
    most_maps, most_clauses, direct, no_row, big, passing, unknown = 0, 0, 0, 0, 0, 0, 0
    for it in range(SWEEP_ITERS):
        case = draw_filter_case(rng, it)
        n, terms = case["n"], case["terms"]
        assert 1 <= n <= 1 << 16 and 1 <= len(terms) <= H.HMJ_MAX_FILTER_TERMS
        ids = [t["clause"] for t in terms]
        assert ids == sorted(ids) and 1 <= len(set(ids)) <= 5
        most_clauses = max(most_clauses, len(set(ids)))
        bodies.add(next(b for b in (1, 2, 4, 8, 16) if len(terms) <= b))
        maps = {id(t["row_map"]) for t in terms if t["row_map"] is not None}
        most_maps = max(most_maps, len(maps))
        lit_bytes = 0
        for t in terms:
            is_str = not isinstance(t["column"], np.ndarray)
            kinds.add(STRING if is_str else str(t["column"].dtype))
            ops.add((is_str, t["op"]))
            negs.add(t["negate"])
            if t["valid"] is not None:
                offs.add(t["bit_offset"])
                assert len(t["valid"]) == len(t["column"])
            if is_str:
                pads.add(t["pad"] != 0)
                lit_bytes += sum(len(l) for l in (t["lit"] if isinstance(t["lit"], tuple) else [t["lit"] or b""]))
            if t["row_map"] is None:
                direct += 1
                assert len(t["column"]) >= n
            else:
                assert len(t["row_map"]) == n
                no_row += int(np.any(t["row_map"] == NO_ROW))
        assert lit_bytes <= H.HMJ_MAX_FILTER_LITERAL_BYTES
        big += n > 4096
        pos, unk = check_reference("sweep %d" % it, terms, n, sample=1500)
        passing += len(pos) > 0
        unknown += unk > 0
    assert kinds == set(DTYPES) | {STRING}, sorted(kinds)
    assert ops == {(False, op) for op in FIXED_OPS} | {(True, op) for op in STRING_OPS}, sorted(ops)
    assert bodies == {1, 2, 4, 8, 16}
    assert most_maps > 4, "no case with more distinct maps than a lane holds in registers"
    assert most_clauses == 5 and negs == {False, True}
    assert offs >= {0, 1, 7, 63, 69} and pads == {True, False}
    assert direct and no_row and big >= 5 and passing >= 5 and unknown >= 5
