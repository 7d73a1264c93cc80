"""CPU-only checks of the Python binding: the marshalling helpers the column entries share (hashmergejoin_amd/_marshal.py)
on stand-in tensors -- every accepted form with the struct fields it fills, every rejected form with its exact text --,
the package's exported names, and the mirror of include/hmj.h in _lib.py: constants, signatures and struct layouts."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import hashmergejoin_amd as H
from hashmergejoin_amd import _lib
from hashmergejoin_amd import _marshal as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64 = 0xFFFFFFFFFFFFFFFF


class T:
    """What the helpers ask of a tensor."""

    def __init__(self, n, dtype="uint8", cuda=True, contiguous=True, dim=1, ptr=0x7000):
        self.is_cuda, self.dtype = cuda, dtype
        self.shape = (n,) if dim == 1 else (n, 2)
        self._contiguous, self._dim, self._ptr = contiguous, dim, ptr

    def is_contiguous(self):
        return self._contiguous

    def dim(self):
        return self._dim

    def element_size(self):
        return np.dtype(self.dtype).itemsize

    def data_ptr(self):
        return self._ptr

    def numel(self):
        return int(np.prod(self.shape))


def bad_columns(dtype="uint8"):
    return [T(4, dtype, cuda=False), T(4, dtype, contiguous=False), T(4, dtype, dim=2)]


def raises(text, fn, *a, **kw):
    with pytest.raises(ValueError) as ei:
        fn(*a, **kw)
    assert str(ei.value) == text, (str(ei.value), text)


# ---- the column check and the dtype table ---------------------------------------------------------------------------
COLUMN_TEXTS = [("key column %d must be a contiguous 1-D device tensor", (3,)),
                ("%s column %d must be a contiguous 1-D device tensor", ("build", 3)),
                ("aggregate %d: the column must be a contiguous 1-D device tensor", (3,)),
                ("column %d must be a contiguous 1-D device tensor", (3,)),
                ("term %d: the column must be a contiguous 1-D device tensor", (3,))]


@pytest.mark.parametrize("fmt,args", COLUMN_TEXTS)
def test_check_column(fmt, args):
    for dtype in ("int8", "float64"):
        M.check_column(T(0, dtype), fmt, *args)
        M.check_column(T(5, dtype), fmt, *args)
        M.check_column(T(5, dtype), "%d %d %d")  # (the text is made only when it is raised)
        for t in bad_columns(dtype):
            raises(fmt % args, M.check_column, t, fmt, *args)


def test_the_entries_raise_the_column_texts():
    # the texts above, where Executor's relation builders form them (neither builder reads self)
    for t in bad_columns("int32"):
        raises("key column 1 must be a contiguous 1-D device tensor", H.Executor._cols_rel, None, [T(4, "int32"), t], None)
        raises("probe column 0 must be a contiguous 1-D device tensor", H.Executor._mixed_rel, None, [t], None, None, "probe")
    rel, arr = H.Executor._cols_rel(None, [T(4, "int32", ptr=0x100), T(4, "uint8", ptr=0x200)], T(4, "int64", ptr=0x300))
    assert (rel.n_cols, rel.n, rel.vals) == (2, 4, 0x300)
    assert [(arr[k].data, arr[k].width) for k in range(2)] == [(0x100, 4), (0x200, 1)]
    rel, keep = H.Executor._mixed_rel(None, [(T(9, ptr=0x400), T(5, "int64", ptr=0x500)), T(4, "int16", ptr=0x600)], None,
                                      [None, (T(1, ptr=0x700), 3)], "build")
    cols = keep[0]
    assert (rel.n_cols, rel.n, rel.vals) == (2, 4, None)
    assert (cols[0].type, cols[0].width, cols[0].data, cols[0].offsets) == (_lib.HMJ_KEY_LARGE_STRING, 0, 0x400, 0x500)
    assert (cols[1].type, cols[1].width, cols[1].data) == (_lib.HMJ_KEY_FIXED, 2, 0x600)
    assert (cols[0].validity.bits, cols[1].validity.bits, cols[1].validity.bit_offset) == (None, 0x700, 3)
    raises("build_valid[1] holds fewer than bit_offset + n bits", H.Executor._mixed_rel, None, [T(4, "int16"), T(4, "int16")], None,
           [None, (T(1), 5)], "build")
    # an empty bitmap is "no NULL" to the mixed entries whatever n is ...
    rel, keep = H.Executor._mixed_rel(None, [T(4, "int16")], None, [T(0)], "build")
    assert keep[0][0].validity.bits is None
    # ... and too short to the column joins
    raises("build_valid[0] holds fewer than bit_offset + n bits", H.Executor._validity, None, [T(0)], rel, "build_valid")
    raises("build_valid: one entry per key column", H.Executor._validity, None, [None, None], rel, "build_valid")
    assert H.Executor._validity(None, None, rel, "build_valid") == (None, None)
    arr, keep = H.Executor._validity(None, [(T(1, ptr=0x800), 4)], rel, "build_valid")
    assert (arr[0].bits, arr[0].bit_offset) == (0x800, 4) and keep[0] is arr


def test_type_code_is_one_table():
    names = ("I8", "I16", "I32", "I64", "U8", "U16", "U32", "U64", "F32", "F64")
    assert len(M.TYPE_NAMES) == len(names)
    for short, name in zip(names, M.TYPE_NAMES):
        code = getattr(_lib, "HMJ_TYPE_" + short)
        assert M.TYPE_NAMES[code] == name
        assert M.type_code(name) == M.type_code(np.dtype(name)) == code
        assert np.dtype(name).kind == {"I": "i", "U": "u", "F": "f"}[short[0]] and np.dtype(name).itemsize * 8 == int(short[1:])
    import torch

    for name in M.TYPE_NAMES:
        if hasattr(torch, name):
            assert M.type_code(getattr(torch, name)) == M.TYPE_NAMES.index(name)
            assert H.Executor._agg_type(None, T(1, getattr(torch, name))) == M.TYPE_NAMES.index(name)
    for bad in ("float16", "bool", "complex64", torch.bfloat16):
        raises("no HMJ_TYPE_* for %s" % (bad,), M.type_code, bad)


# ---- validity ----------------------------------------------------------------------------------------------------------
def fill(valid, n, name="v", **kw):
    dst = _lib.Validity()
    dst.bits, dst.bit_offset = 0xDEAD, 99  # (what is not touched stays visible)
    keep = M.validity(dst, valid, n, "%s", name, **kw)
    return dst.bits, dst.bit_offset, keep


@pytest.mark.parametrize("empty_is_absent", [False, True])
def test_validity_byte_bitmap(empty_is_absent):
    kw = {"empty_is_absent": empty_is_absent}
    assert fill(None, 5, **kw) == (0xDEAD, 99, None)  # no bitmap: nothing written, nothing kept
    b = T(1)
    assert fill(b, 8, **kw) == (0x7000, 0, b)
    assert fill((b, 3), 5, **kw) == (0x7000, 3, b)
    assert fill((b, 8), 0, **kw) == (0x7000, 8, b)  # n = 0 with a bitmap: the pointer is still passed
    assert fill(T(2), 0, **kw)[:2] == (0x7000, 0)
    raises("v holds fewer than bit_offset + n bits", fill, (b, 7), 2, **kw)  # one bit short
    raises("v holds fewer than bit_offset + n bits", fill, b, 9, **kw)
    assert fill((T(2), 7), 9, **kw)[:2] == (0x7000, 7)  # exactly enough
    # an offset that overflows with n is the library's to reject: no length check, the offset passes masked
    assert fill((b, 2 ** 64 - 1), 1, **kw)[:2] == (0x7000, U64)
    assert fill((b, 2 ** 64 + 5), 1, **kw)[:2] == (0x7000, 5)
    raises("v holds fewer than bit_offset + n bits", fill, (b, 2 ** 64 - 1), 0, **kw)  # (no overflow: 2^64 - 1 bits asked of 8)
    raises("v: bit_offset must not be negative", fill, (b, -1), 1, **kw)
    for t in bad_columns() + [T(1, "int64"), T(1, "uint16")]:
        raises("v must be a contiguous 1-D uint8 device tensor", fill, t, 1, **kw)
        raises("v must be a contiguous 1-D uint8 device tensor", fill, (t, -1), 1, **kw)  # the tensor is judged first
    assert fill(T(1, "int8"), 8, **kw)[:2] == (0x7000, 0)  # any 1-byte dtype
    assert fill(T(0), 0, **kw)[:2] == (None, 0)  # an empty tensor passes NULL


def test_validity_empty_tensor_setting():
    # the one difference between the entries, kept as it is: n = 1 over a 0-byte bitmap
    e = T(0)
    assert fill(e, 1, empty_is_absent=True) == (None, 0, e)
    assert fill((e, 5), 1, empty_is_absent=True) == (None, 5, e)
    raises("v holds fewer than bit_offset + n bits", fill, e, 1, empty_is_absent=False)
    raises("v holds fewer than bit_offset + n bits", fill, (e, 1), 0, empty_is_absent=False)
    raises("v holds fewer than bit_offset + n bits", fill, e, 1)  # the default


@pytest.mark.parametrize("owner", ["aggregate 2", "column 2", "term 2"])
def test_validity_any_width(owner):
    kw = {"any_width": True}
    assert fill(None, 5, owner, **kw) == (0xDEAD, 99, None)
    for dtype in ("uint8", "int64"):
        w = T(1, dtype)
        assert fill(w, 10 ** 6, owner, **kw) == (0x7000, 0, w)  # no length check in this flavour
        assert fill((w, 7), 2, owner, **kw) == (0x7000, 7, w)
        assert fill((w, 2 ** 64 - 1), 1, owner, **kw)[:2] == (0x7000, U64)
        assert fill(T(0, dtype), 1, owner, **kw)[:2] == (None, 0)
        assert fill(T(0, dtype), 1, owner, empty_is_absent=True, **kw)[:2] == (None, 0)
        raises("%s: bit_offset must not be negative" % owner, fill, (w, -1), 1, owner, **kw)
        for t in bad_columns(dtype):
            raises("%s: valid must be a contiguous 1-D device tensor" % owner, fill, t, 1, owner, **kw)


# ---- row maps, string columns, want_validity ----------------------------------------------------------------------------
@pytest.mark.parametrize("fmt,args", [("row_map must be a contiguous 1-D int64 device tensor", ()),
                                      ("term %d: row_map must be a contiguous 1-D int64 device tensor", (1,))])
def test_row_map(fmt, args):
    assert M.row_map((0, 0), "int64", fmt, *args) == (None, 0, None)
    assert M.row_map((None, 0), "int64", fmt, *args) == (None, 0, None)
    assert M.row_map((0x9000, 3), "int64", fmt, *args) == (0x9000, 3, None)
    t = T(3, "int64", ptr=0x9100)
    assert M.row_map(t, "int64", fmt, *args) == (0x9100, 3, t)
    e = T(0, "int64", ptr=0x9200)
    assert M.row_map(e, "int64", fmt, *args) == (None, 0, e)
    for t in bad_columns("int64") + [T(3, "uint64"), T(3, "int32"), T(3, "float64")]:
        raises(fmt % args, M.row_map, t, "int64", fmt, *args)
    import torch

    cpu = torch.zeros(3, dtype=torch.int64)
    raises(fmt % args, M.row_map, cpu, torch.int64, fmt, *args)  # a real tensor off the device: the dtype passes, is_cuda does not
    raises(fmt % args, M.row_map, torch.zeros(3, dtype=torch.int32), torch.int64, fmt, *args)


def test_str_column():
    off = T(4, "int64", ptr=0xA000)
    assert M.str_column(None, off, "offsets") == (None, 0, 0xA000)  # chars=None
    assert M.str_column(T(0), off, "offsets") == (None, 0, 0xA000)
    assert M.str_column(T(11, ptr=0xA100), off, "offsets") == (0xA100, 11, 0xA000)
    assert M.str_column(T(11, "int8", ptr=0xA100), off, "offsets") == (0xA100, 11, 0xA000)
    for fmt, args in (("offsets", ()), ("term %d: offsets", (2,))):
        for t in bad_columns("int64") + [T(4, "int32")]:
            raises("%s must be a contiguous 1-D 64-bit device tensor" % (fmt % args), M.str_column, None, t, fmt, *args)
        raises("%s must hold n + 1 entries" % (fmt % args), M.str_column, None, T(0, "int64"), fmt, *args)
    raises("column 2: offsets must be a contiguous 1-D 64-bit device tensor", M.check_col64, T(4, "int32"), "column %d: offsets", 2)
    for t in [T(5, cuda=False), T(5, contiguous=False), T(5, "int16")]:
        raises("chars must be a contiguous 1-byte device tensor", M.str_column, t, off, "offsets")
    raises("offsets must hold n + 1 entries", M.str_column, T(5, cuda=False), T(0, "int64"), "offsets")  # offsets first


@pytest.mark.parametrize("what", ["aggregate", "column"])
def test_want_flags(what):
    assert M.want_flags(True, 3, what) == [True] * 3 and M.want_flags(False, 2, what) == [False] * 2
    assert M.want_flags(1, 2, what) == [True, True] and M.want_flags(True, 0, what) == []
    assert M.want_flags([1, 0, "x"], 3, what) == [True, False, True]
    assert M.want_flags(iter([False]), 1, what) == [False]
    for bad in ([], [True, False], [True] * 4):
        raises("want_validity: one entry per %s" % what, M.want_flags, bad, 3, what)


# ---- opts in, info out ----------------------------------------------------------------------------------------------
def test_new_opts_and_read_info():
    o = M.new_opts(_lib.ColsKindOpts, side=1, kind=3, hash_bits=-1, force_hashed=True, probe_fill=-1, build_fill=2 ** 64 + 7)
    assert o.struct_size == C.sizeof(_lib.ColsKindOpts)
    assert (o.side, o.kind, o.hash_bits, o.force_hashed, o.probe_fill, o.build_fill) == (1, 3, 0xFFFFFFFF, 1, U64, 7)
    assert (o.form, o.n_key_pairs, bool(o.build_validity)) == (0, 0, False)
    for cls in (_lib.TakeOpts, _lib.PlanDesc, _lib.FilterOpts):
        assert M.new_opts(cls).struct_size == C.sizeof(cls)
    o.counts.n_probe_matched, o.counts.n_build_unmatched, o.form, o.n_collisions, o.ms_key = 5, 6, 2, 2 ** 63, 0.5
    info = M.read_info(o, ("form", "n_collisions"), ("ms_key", "ms_emit"))
    assert info == {"n_probe_matched": 5, "n_probe_unmatched": 0, "n_build_matched": 0, "n_build_unmatched": 6, "form": 2,
                    "n_collisions": 2 ** 63, "ms_key": 0.5, "ms_emit": 0.0}
    assert all(type(info[k]) is int for k in info if not k.startswith("ms_")) and type(info["ms_key"]) is float
    t = M.new_opts(_lib.TakeOpts)
    t.n_no_row = 4
    assert M.read_info(t, ("n_no_row",)) == {"n_no_row": 4} and M.read_info(t) == {}  # no hmj_kind_counts in it
    # the order the entries' dicts always had: what the entry read elsewhere, counters, integers, constants, times
    got = M.read_info(o, ("form",), ("ms_key",), first={"null_count": [1]}, between={"total_bytes": 9})
    assert list(got) == ["null_count", "n_probe_matched", "n_probe_unmatched", "n_build_matched", "n_build_unmatched", "form",
                         "total_bytes", "ms_key"]


class FakeTorch:
    """torch as `read_columns` uses it, over host memory: pointers are numpy buffers' addresses."""
    int64 = np.int64

    class cuda:
        synchronize = staticmethod(lambda: None)

    def __init__(self):
        self.allocated = []

    def empty(self, n, dtype, device):
        self.allocated.append((n, device))
        buf = np.empty(n, dtype)
        t = T(n, "int64", ptr=buf.ctypes.data)
        t.cpu = lambda: type("X", (), {"numpy": staticmethod(lambda: buf)})
        return t


def test_read_columns(monkeypatch):
    monkeypatch.setattr(M, "_memcpy_d2d", lambda torch, dst, ptr, nbytes: C.memmove(dst.data_ptr(), ptr, nbytes))
    a, b = np.array([1, 2, 2 ** 64 - 1], np.uint64), np.array([7, 8, 9], np.uint64)
    pa, pb = a.ctypes.data, b.ctypes.data
    ft = FakeTorch()
    got = M.read_columns(ft, 2, [pa, pb, pa], 3)
    assert got.dtype == np.uint64 and np.array_equal(got, np.stack([a, b, a], axis=1))
    assert ft.allocated == [(3, "cuda:2")]  # one staging buffer for all columns
    # a column the kind did not produce: one value, or one per column
    assert np.array_equal(M.read_columns(ft, 0, [pa, None, pb], 3, absent=0), np.stack([a, a * 0, b], axis=1))
    got = M.read_columns(ft, 0, [pa, None, None, pb, None], 3, absent=(0, _lib.HMJ_STR_NO_ROW, _lib.HMJ_STR_NO_ROW, 0, 0))
    assert np.array_equal(got, np.stack([a, a * 0 + np.uint64(U64), a * 0 + np.uint64(U64), b, a * 0], axis=1))
    # the early return: no rows, or no first column -- nothing is allocated
    ft = FakeTorch()
    for ptrs, n in (([pa, pb], 0), ([None, pb], 3), ([0, pb], 3)):
        got = M.read_columns(ft, 0, ptrs, n, absent=0)
        assert got.shape == (0, 2) and got.dtype == np.uint64
    assert ft.allocated == []


# ---- exports ---------------------------------------------------------------------------------------------------------
EXPORTED_BEFORE = """
AggDst AggSrc BuildJoinOpts ColsJoinOpts ColsKindOpts ColsRel ColsResult ExchangeKindOpts Executor FilterOpts FilterTerm
GroupAggOpts GroupOpts GroupResult HMJ_AGG_COUNT HMJ_AGG_MAX HMJ_AGG_MEAN HMJ_AGG_MIN HMJ_AGG_SUM HMJ_BUILD_ANTI HMJ_BUILD_OUTER
HMJ_BUILD_SEMI HMJ_CHECKSUM HMJ_COLS_HASHED HMJ_COLS_NO_ROW HMJ_COLS_PACKED HMJ_FILTER_BETWEEN HMJ_FILTER_ENDS_WITH HMJ_FILTER_EQ
HMJ_FILTER_GE HMJ_FILTER_GT HMJ_FILTER_IS_NOT_NULL HMJ_FILTER_IS_NULL HMJ_FILTER_LARGE_STRING HMJ_FILTER_LE HMJ_FILTER_LT
HMJ_FILTER_NE HMJ_FILTER_NOT HMJ_FILTER_STARTS_WITH HMJ_FIRST_WINS HMJ_FULL_OUTER HMJ_GROUP_COUNT HMJ_GROUP_MAX HMJ_GROUP_MIN
HMJ_GROUP_ROW_MAP HMJ_GROUP_SUM HMJ_JOIN_ANTI HMJ_JOIN_INNER HMJ_JOIN_PROBE_OUTER HMJ_JOIN_SEMI HMJ_KEY_FIXED HMJ_KEY_LARGE_STRING
HMJ_KIND_BUILD_SIDE HMJ_KIND_PROBE_SIDE HMJ_MATERIALIZE HMJ_MAX_AGGS HMJ_MAX_FILTER_LITERAL_BYTES HMJ_MAX_FILTER_TERMS
HMJ_MAX_KEY_COLS HMJ_MAX_ORDER_COLS HMJ_MAX_TAKE_COLS HMJ_NULL_EQUAL HMJ_ORDERED HMJ_ORDER_DESC HMJ_ORDER_LARGE_STRING
HMJ_ORDER_NULLS_FIRST HMJ_STR_NO_ROW HMJ_SUM_PROBE HMJ_TAKE_NO_ROW HMJ_TYPE_F32 HMJ_TYPE_F64 HMJ_TYPE_I16 HMJ_TYPE_I32 HMJ_TYPE_I64
HMJ_TYPE_I8 HMJ_TYPE_U16 HMJ_TYPE_U32 HMJ_TYPE_U64 HMJ_TYPE_U8 HashMergeJoin HmjError JoinOpts JoinResult KeyCol KindCounts
MixedCol MixedOpts MixedRel OrderCol OrderOpts StrJoinOpts StrKindOpts StrRel StrResult TakeDst TakeOpts TakeSrc TakeStrDst
TakeStrOpts TakeStrSrc Timing Validity cols_key64 expected_filter expected_group_aggs expected_groups expected_mixed_groups
expected_order_by lib_path load_library mixed_key64 order_stream_bytes pack_strings pack_validity plan unpack_strings
unpack_validity
""".split()
# names the package carried as attributes without listing them (the tests say H.HMJ_PATH_SLAB)
ATTRIBUTES_BEFORE = """
HMJ_PATH_CHUNKED_BUILD HMJ_PATH_DENSE_BUILD HMJ_PATH_EXACT HMJ_PATH_GLOBAL_TABLE HMJ_PATH_HOST_PIPELINE HMJ_PATH_HOT_KEY_HINT
HMJ_PATH_LOOKBACK_TIMEOUT HMJ_PATH_ORDER_BY_KEY HMJ_PATH_ORDER_BY_RANK_SORT HMJ_PATH_ORDER_DEFERRED HMJ_PATH_ORDERED_EXPANSION
HMJ_PATH_LDS_TABLE HMJ_PATH_KEY_RANGES HMJ_PATH_PREPARED HMJ_PATH_PRESORTED HMJ_PATH_RANK_RUNS HMJ_PATH_SORT_MSD HMJ_PATH_SLAB
HMJ_PATH_SLAB_ONE_PASS HMJ_PATH_SLAB_PROBE HMJ_PATH_SORTED_FK HMJ_PATH_SORTED_FK_HALF HMJ_PATH_SORTED_FK_WIDE HMJ_PATH_SORTED_WRITE
HMJ_PATH_SPLIT HMJ_PATH_UNIQ_WRITE HMJ_PATH_WINDOW dist join
""".split()


def test_every_name_exported_before_still_is():
    assert len(EXPORTED_BEFORE) == len(set(EXPORTED_BEFORE)) == 117
    for name in EXPORTED_BEFORE:
        assert name in H.__all__ and hasattr(H, name), name
    import hashmergejoin_amd.dist  # noqa: F401

    for name in ATTRIBUTES_BEFORE:
        assert hasattr(H, name), name
    assert len(H.__all__) == len(set(H.__all__)) and all(hasattr(H, name) for name in H.__all__)
    # what the binding's mirror now offers without reaching into _lib
    for name in ("HMJ_PATH_RANK_LOOKUP_IN_PASS", "HMJ_COOL_RANK_RUNS", "HMJ_COOL_SORT_MSD", "HMJ_REFUSED_PREFIX_VIOLATED", "HMJ_E_ARG",
                 "PlanDesc", "DigitPlan"):
        assert getattr(H, name) is getattr(_lib, name) and name in H.__all__
    # the host restatements and the plumbing other modules import, from where they were
    from hashmergejoin_amd import join, reference

    for name in ("cols_key64", "mixed_key64", "expected_groups", "expected_mixed_groups", "expected_group_aggs", "expected_order_by",
                 "order_stream_bytes", "expected_filter"):
        assert getattr(join, name) is getattr(reference, name) is getattr(H, name)
    assert callable(join._memcpy_d2d) and callable(join._dev_ptr)


# ---- the mirror of include/hmj.h ------------------------------------------------------------------------------------------
def header():
    src = open(os.path.join(ROOT, "include", "hmj.h")).read()
    return re.sub(r"/\*.*?\*/", " ", src, flags=re.S)


def test_every_integer_define_is_mirrored():
    defs = re.findall(r"^[ \t]*#[ \t]*define[ \t]+(HMJ_\w+)[ \t]+\(?(-?(?:0[xX][0-9a-fA-F]+|\d+))[uU]?[lL]{0,2}\)?[ \t]*$", header(), flags=re.M)
    assert len(defs) >= 136 and len(dict(defs)) == len(defs)
    for name, text in defs:
        assert getattr(_lib, name) == int(text, 0), name
        assert name in _lib.__all__ and getattr(H, name) == int(text, 0), name
    for name in ("HMJ_OK", "HMJ_E_ARG", "HMJ_E_NODEV", "HMJ_E_OOM", "HMJ_E_HIP", "HMJ_E_UNSUPPORTED", "HMJ_COOL_SORT_MSD", "HMJ_ABI_VERSION",
                 "HMJ_PLACE_MAX_CAND", "HMJ_UNIQUE_ID_BYTES", "HMJ_OWNER_DIGIT", "HMJ_OWNER_SPLIT", "HMJ_PATH_SLAB"):
        assert name in dict(defs), name  # (the parser sees negative and hexadecimal values)


def declared_functions():
    out = {}
    for name, params in re.findall(r"\b(hmj_[a-z0-9_]+)\s*\(([^()]*(?:\([^()]*\)[^()]*)*)\)\s*;", header()):
        params = params.strip()
        out[name] = 0 if params in ("", "void") else len(re.sub(r"\([^()]*\)", "", params).split(","))
    return out


def test_every_declared_function_has_its_signature_set():
    fns = declared_functions()
    L = H.load_library()
    assert len(fns) >= 60 and fns["hmj_version"] == 0 and fns["hmj_create"] == 2 and fns["hmj_exchange_digit_layout"] == 9
    for name, n_params in fns.items():
        fn = getattr(L, name)
        assert fn.argtypes is not None, "%s: no argtypes" % name
        assert len(fn.argtypes) == n_params, (name, len(fn.argtypes), n_params)
    assert set(_lib._SIGNATURES) == set(fns)
    assert L.hmj_destroy.restype is None and L.hmj_version.restype is C.c_char_p and L.hmj_host_pool_bytes.restype is C.c_uint64


# mirror class -> (C struct, {mirror field: the header's name for it})
MIRRORS = {
    "JoinResult": ("hmj_result", {}), "Timing": ("hmj_timing", {"ms_scatter_pass0": "ms_scatter_pass[0]", "ms_scatter_pass1": "ms_scatter_pass[1]"}), "PlanDesc": ("hmj_plan_desc", {}), "PlaceInfo": ("hmj_place_info", {}),
    "JoinOpts": ("hmj_join_opts", {}), "BuildJoinOpts": ("hmj_build_join_opts", {}), "KindCounts": ("hmj_kind_counts", {}),
    "ExchangeKindOpts": ("hmj_exchange_kind_opts", {}), "StrRel": ("hmj_str_rel", {}), "StrJoinOpts": ("hmj_str_join_opts", {}),
    "StrResult": ("hmj_str_result", {}), "Validity": ("hmj_validity", {}), "StrKindOpts": ("hmj_str_kind_opts", {}),
    "KeyCol": ("hmj_key_col", {}), "ColsRel": ("hmj_cols_rel", {}), "ColsJoinOpts": ("hmj_cols_join_opts", {}),
    "ColsResult": ("hmj_cols_result", {}), "ColsKindOpts": ("hmj_cols_kind_opts", {}), "MixedCol": ("hmj_mixed_col", {}),
    "MixedRel": ("hmj_mixed_rel", {}), "MixedOpts": ("hmj_mixed_opts", {}), "GroupOpts": ("hmj_group_opts", {}),
    "GroupResult": ("hmj_group_result", {}), "AggSrc": ("hmj_agg_src", {}), "AggDst": ("hmj_agg_dst", {}),
    "GroupAggOpts": ("hmj_group_agg_opts", {}), "OrderCol": ("hmj_order_col", {}), "OrderOpts": ("hmj_order_opts", {}),
    "TakeSrc": ("hmj_take_src", {}), "TakeDst": ("hmj_take_dst", {}), "TakeOpts": ("hmj_take_opts", {}),
    "TakeStrSrc": ("hmj_take_str_src", {}), "TakeStrDst": ("hmj_take_str_dst", {}), "TakeStrOpts": ("hmj_take_str_opts", {}),
    "FilterTerm": ("hmj_filter_term", {}), "FilterOpts": ("hmj_filter_opts", {}), "Transport": ("hmj_transport", {}),
    "ExchangeInfo": ("hmj_exchange_info", {}), "DigitPlan": ("hmj_digit_plan", {}),
}


def test_every_struct_mirror_has_the_headers_layout(tmp_path):
    mirrors = {k: v for k, v in vars(_lib).items() if isinstance(v, type) and issubclass(v, C.Structure)}
    assert set(mirrors) == set(MIRRORS) and len(MIRRORS) == 39
    assert len({c for c, _ in MIRRORS.values()}) == 39 <= len(re.findall(r"\}\s*hmj_\w+\s*;", header()))
    lines = ["#include <cstddef>", "#include <cstdio>", '#include "hmj.h"', "int main() {"]
    for cls, (cname, renamed) in sorted(MIRRORS.items()):
        lines.append('  std::printf("%s  %%zu\\n", sizeof(%s));' % (cls, cname))
        for field, _ in mirrors[cls]._fields_:
            cfield = renamed.get(field, field)
            lines.append('  std::printf("%s %s %%zu %%zu\\n", offsetof(%s, %s), sizeof(((%s*)0)->%s));'
                         % (cls, field, cname, cfield, cname, cfield))
    lines += ["  return 0;", "}"]
    src, exe = tmp_path / "layout.cc", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    subprocess.run(["g++", "-std=c++11", "-O0", "-Wno-invalid-offsetof", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True, timeout=120)
    seen = 0
    for ln in subprocess.run([str(exe)], check=True, capture_output=True, text=True, timeout=30).stdout.splitlines():
        cls, field, *nums = ln.split(" ")
        if not field:
            assert C.sizeof(mirrors[cls]) == int(nums[0]), (cls, C.sizeof(mirrors[cls]), nums)
        else:
            d = getattr(mirrors[cls], field)
            assert (d.offset, d.size) == (int(nums[0]), int(nums[1])), (cls, field, d.offset, d.size, nums)
        seen += 1
    assert seen == 39 + sum(len(m._fields_) for m in mirrors.values())
