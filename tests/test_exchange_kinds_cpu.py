"""CPU-only checks of the distributed join kinds (hmj_exchange_join_kind_u64_device): the symbol is exported, bad arguments
fail loudly without a device, and the binding mirrors hmj.h (constants, struct sizes and field offsets)."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return open(os.path.join(ROOT, "include", "hmj.h")).read()


def _struct_fields(src, name):
    end = src.index("} %s;" % name)
    body = src[src.rindex("typedef struct {", 0, end):end]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for t, names in re.findall(r"(uint32_t|uint64_t|hmj_kind_counts)\s+([\w\s,]+);", body):
        fields += [(t, n.strip()) for n in names.split(",")]
    return fields


def _check_layout(ctype, fields, sizes):
    assert [n for _, n in fields] == [n for n, _ in ctype._fields_]
    off = 0
    for (t, n), (_, ct) in zip(fields, ctype._fields_):
        size, align = sizes[t]
        off = (off + align - 1) // align * align
        assert getattr(ctype, n).offset == off, n
        assert C.sizeof(ct) == size, n
        off += size
    assert C.sizeof(ctype) == off
    return off


def test_exchange_kind_entry_is_exported():
    import hashmergejoin_amd as H

    assert hasattr(H.load_library(), "hmj_exchange_join_kind_u64_device")


def test_exchange_kind_side_constants_are_mirrored_by_the_binding():
    from hashmergejoin_amd import _lib

    import hashmergejoin_amd as H

    found = dict(re.findall(r"#define (HMJ_KIND_(?:PROBE|BUILD)_SIDE) (\d+)u", _header()))
    assert found == {"HMJ_KIND_PROBE_SIDE": "0", "HMJ_KIND_BUILD_SIDE": "1"}
    for name, v in found.items():
        assert getattr(_lib, name) == int(v), name
        assert getattr(H, name) == int(v), name
        assert name in H.__all__


def test_exchange_kind_structs_match_the_header():
    import hashmergejoin_amd as H

    src = _header()
    cnt = _struct_fields(src, "hmj_kind_counts")
    assert _check_layout(H.KindCounts, cnt, {"uint64_t": (8, 8)}) == 32
    opts = _struct_fields(src, "hmj_exchange_kind_opts")
    assert _check_layout(H.ExchangeKindOpts, opts, {"uint32_t": (4, 4), "uint64_t": (8, 8), "hmj_kind_counts": (32, 8)}) == 96
    assert H.ExchangeKindOpts.local.offset == 32 and getattr(H.ExchangeKindOpts, "global").offset == 64


def test_exchange_kind_null_arguments_are_argument_errors():
    import hashmergejoin_amd as H

    L = H.load_library()
    opts = H.ExchangeKindOpts()
    opts.struct_size = C.sizeof(H.ExchangeKindOpts)
    opts.side, opts.kind = H.HMJ_KIND_BUILD_SIDE, H.HMJ_FULL_OUTER
    loc, glob = H.JoinResult(), H.JoinResult()
    f = L.hmj_exchange_join_kind_u64_device
    assert f(None, None, 0, None, 0, 0, C.byref(opts), C.byref(loc), C.byref(glob)) == -1  # HMJ_E_ARG: NULL ctx
    assert f(None, None, 0, None, 0, 0, None, C.byref(loc), None) == -1
    assert f(None, None, 0, None, 0, 0, C.byref(opts), None, None) == -1
