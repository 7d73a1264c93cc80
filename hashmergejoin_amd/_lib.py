"""ctypes binding of include/hmj.h.  Loads hashmergejoin_amd/libhmj_hip.so (built in-tree by
`make`); raises loudly if it is missing -- there is no fallback path."""
import ctypes as C
import os

HMJ_MATERIALIZE = 0x01
HMJ_ORDERED = 0x02
HMJ_FIRST_WINS = 0x04
HMJ_CHECKSUM = 0x08
HMJ_SUM_PROBE = 0x10
HMJ_NULL_EQUAL = 0x20  # NULL key slots match NULL slots of the same column (the column kinds and the mixed entry)
HMJ_OK, HMJ_E_ARG, HMJ_E_NODEV, HMJ_E_OOM, HMJ_E_HIP, HMJ_E_UNSUPPORTED = 0, -1, -2, -3, -4, -5
HMJ_E_RCCL, HMJ_E_PEER, HMJ_E_TIMEOUT = -6, -7, -8
HMJ_ABI_VERSION = 5
# hmj_timing.path bits
HMJ_PATH_SLAB, HMJ_PATH_EXACT, HMJ_PATH_UNIQ_WRITE, HMJ_PATH_SPLIT, HMJ_PATH_WINDOW = 0x1, 0x2, 0x4, 0x8, 0x10
HMJ_PATH_ORDER_DEFERRED, HMJ_PATH_ORDER_BY_KEY, HMJ_PATH_PREPARED, HMJ_PATH_CHUNKED_BUILD = 0x20, 0x40, 0x80, 0x100
HMJ_PATH_HOT_KEY_HINT = 0x200
HMJ_PATH_SLAB_PROBE = 0x400
HMJ_PATH_SORTED_WRITE = 0x800
HMJ_PATH_SORTED_FK = 0x1000
HMJ_PATH_DENSE_BUILD = 0x2000
HMJ_PATH_GLOBAL_TABLE = 0x100000
HMJ_PATH_ORDER_BY_RANK_SORT = 0x200000
HMJ_PATH_ORDERED_EXPANSION = 0x400000
HMJ_PATH_LDS_TABLE = 0x800000
HMJ_PATH_RANK_RUNS = 0x1000000
HMJ_PATH_RANK_LOOKUP_IN_PASS = 0x2000000
HMJ_PATH_SORT_MSD = 0x4000000
HMJ_PATH_KEY_RANGES = 0x8000000
HMJ_PATH_SLAB_ONE_PASS = 0x80000
HMJ_PATH_HOST_PIPELINE = 0x4000
HMJ_PATH_SORTED_FK_HALF = 0x8000
HMJ_PATH_LOOKBACK_TIMEOUT = 0x10000
HMJ_PATH_SORTED_FK_WIDE = 0x20000
HMJ_PATH_PRESORTED = 0x40000
HMJ_PATH_PROBE_KEYS = 0x10000000  # plain count join: the probe side went through the slab passes as 8-byte keys

_HERE = os.path.dirname(os.path.abspath(__file__))
_U64P = C.POINTER(C.c_uint64)


class HmjError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("hmj error %d: %s" % (code, msg))
        self.code = code


class JoinResult(C.Structure):
    _fields_ = [("n_matches", C.c_uint64), ("sum_r", C.c_uint64), ("sum_s", C.c_uint64),
                ("xor_fold", C.c_uint64), ("mix_sum", C.c_uint64), ("sum_probe_all", C.c_uint64),
                ("key", C.c_void_p), ("rval", C.c_void_p), ("sval", C.c_void_p)]

    def checks(self):
        return {k: int(getattr(self, k)) for k in ("n_matches", "sum_r", "sum_s", "xor_fold", "mix_sum")}


# hmj_join_opts.kind (hmj_join_kind_u64_device)
HMJ_JOIN_INNER, HMJ_JOIN_SEMI, HMJ_JOIN_ANTI, HMJ_JOIN_PROBE_OUTER = 0, 1, 2, 3


class JoinOpts(C.Structure):
    """hmj_join_opts: the kind of a join and its fill value (in), matched / unmatched probe rows (out)."""
    _fields_ = [("struct_size", C.c_uint32), ("kind", C.c_uint32), ("outer_fill", C.c_uint64),
                ("n_probe_matched", C.c_uint64), ("n_probe_unmatched", C.c_uint64)]


# hmj_build_join_opts.kind (hmj_join_build_kind_u64_device)
HMJ_BUILD_SEMI, HMJ_BUILD_ANTI, HMJ_BUILD_OUTER, HMJ_FULL_OUTER = 1, 2, 3, 4


class BuildJoinOpts(C.Structure):
    """hmj_build_join_opts: the build-side kind and its fill values (in), matched / unmatched build and probe rows (out)."""
    _fields_ = [("struct_size", C.c_uint32), ("kind", C.c_uint32), ("build_fill", C.c_uint64), ("probe_fill", C.c_uint64),
                ("n_build_matched", C.c_uint64), ("n_build_unmatched", C.c_uint64),
                ("n_probe_matched", C.c_uint64), ("n_probe_unmatched", C.c_uint64)]


# hmj_exchange_kind_opts.side (hmj_exchange_join_kind_u64_device)
HMJ_KIND_PROBE_SIDE, HMJ_KIND_BUILD_SIDE = 0, 1


class KindCounts(C.Structure):
    """hmj_kind_counts: matched / unmatched probe and build rows of a join kind."""
    _fields_ = [("n_probe_matched", C.c_uint64), ("n_probe_unmatched", C.c_uint64),
                ("n_build_matched", C.c_uint64), ("n_build_unmatched", C.c_uint64)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class ExchangeKindOpts(C.Structure):
    """hmj_exchange_kind_opts: side, kind and fill values (in), this rank's and the summed counters (out)."""
    _fields_ = [("struct_size", C.c_uint32), ("side", C.c_uint32), ("kind", C.c_uint32), ("reserved", C.c_uint32),
                ("probe_fill", C.c_uint64), ("build_fill", C.c_uint64), ("local", KindCounts), ("global", KindCounts)]


class StrRel(C.Structure):
    """hmj_str_rel: a string-keyed relation on the device (Arrow large_string layout + payloads)."""
    _fields_ = [("chars", C.c_void_p), ("offsets", C.c_void_p), ("vals", C.c_void_p), ("n", C.c_uint64)]


class StrJoinOpts(C.Structure):
    """hmj_str_join_opts: hash bits (in), pairs of equal hash, dropped collisions and phase times (out)."""
    _fields_ = [("struct_size", C.c_uint32), ("hash_bits", C.c_uint32), ("n_hash_pairs", C.c_uint64),
                ("n_collisions", C.c_uint64), ("ms_hash", C.c_float), ("ms_join", C.c_float), ("ms_verify", C.c_float),
                ("ms_order", C.c_float)]


# hmj_str_kind_opts (hmj_join_kind_str_device): r_row / s_row of an outer join's unmatched row
HMJ_STR_NO_ROW = 0xFFFFFFFFFFFFFFFF


class Validity(C.Structure):
    """hmj_validity: one key column's Arrow validity bitmap on the device (LSB first; NULL bits: no NULL in the column) and
    the slice offset of row 0 in it, in bits."""
    _fields_ = [("bits", C.c_void_p), ("bit_offset", C.c_uint64)]


class StrKindOpts(C.Structure):
    """hmj_str_kind_opts: side, kind, hash bits, fill values and the key column's validity bitmap per side (in); the kind's
    counters, pairs of equal hash, pairs whose keys differ, phase times and the NULL-key rows per side (out)."""
    _fields_ = [("struct_size", C.c_uint32), ("side", C.c_uint32), ("kind", C.c_uint32), ("hash_bits", C.c_uint32),
                ("probe_fill", C.c_uint64), ("build_fill", C.c_uint64), ("counts", KindCounts), ("n_hash_pairs", C.c_uint64),
                ("n_collisions", C.c_uint64), ("ms_hash", C.c_float), ("ms_join", C.c_float), ("ms_verify", C.c_float),
                ("ms_emit", C.c_float), ("ms_order", C.c_float), ("build_validity", Validity), ("probe_validity", Validity),
                ("n_build_null", C.c_uint64), ("n_probe_null", C.c_uint64)]


class StrResult(C.Structure):
    """hmj_str_result: counts and sums as JoinResult (tmix over (hash, rval, sval)); device columns with HMJ_MATERIALIZE."""
    _fields_ = [("n_matches", C.c_uint64), ("sum_r", C.c_uint64), ("sum_s", C.c_uint64),
                ("xor_fold", C.c_uint64), ("mix_sum", C.c_uint64), ("sum_probe_all", C.c_uint64),
                ("hash", C.c_void_p), ("r_row", C.c_void_p), ("s_row", C.c_void_p), ("rval", C.c_void_p), ("sval", C.c_void_p)]

    def checks(self):
        return {k: int(getattr(self, k)) for k in ("n_matches", "sum_r", "sum_s", "xor_fold", "mix_sum")}


# hmj_join_cols_device: multi-column fixed-width keys
HMJ_MAX_KEY_COLS = 8
HMJ_COLS_PACKED, HMJ_COLS_HASHED = 1, 2


class KeyCol(C.Structure):
    """hmj_key_col: one key column on the device -- n values of `width` bytes (1, 2, 4 or 8), aligned to `width`."""
    _fields_ = [("data", C.c_void_p), ("width", C.c_uint32), ("reserved", C.c_uint32)]


class ColsRel(C.Structure):
    """hmj_cols_rel: a relation keyed by a tuple of fixed-width columns (struct of arrays) + optional payloads."""
    _fields_ = [("cols", C.POINTER(KeyCol)), ("n_cols", C.c_uint32), ("reserved", C.c_uint32), ("vals", C.c_void_p),
                ("n", C.c_uint64)]


class ColsJoinOpts(C.Structure):
    """hmj_cols_join_opts: hash bits and the forced hashed form (in); the form taken, pairs of equal key64, dropped
    collisions and phase times (out)."""
    _fields_ = [("struct_size", C.c_uint32), ("hash_bits", C.c_uint32), ("force_hashed", C.c_uint32), ("form", C.c_uint32),
                ("n_key_pairs", C.c_uint64), ("n_collisions", C.c_uint64), ("ms_key", C.c_float), ("ms_join", C.c_float),
                ("ms_verify", C.c_float), ("ms_order", C.c_float)]


# hmj_cols_kind_opts (hmj_join_kind_cols_device): r_row / s_row of an outer join's unmatched row
HMJ_COLS_NO_ROW = 0xFFFFFFFFFFFFFFFF


class ColsKindOpts(C.Structure):
    """hmj_cols_kind_opts: side, kind, hash bits, the forced hashed form, fill values and the validity bitmaps per side
    (in); the form taken, the kind's counters, pairs of equal key64, pairs whose tuples differ, phase times and the
    NULL-key rows per side (out)."""
    _fields_ = [("struct_size", C.c_uint32), ("side", C.c_uint32), ("kind", C.c_uint32), ("hash_bits", C.c_uint32),
                ("force_hashed", C.c_uint32), ("form", C.c_uint32), ("probe_fill", C.c_uint64), ("build_fill", C.c_uint64),
                ("counts", KindCounts), ("n_key_pairs", C.c_uint64), ("n_collisions", C.c_uint64), ("ms_key", C.c_float),
                ("ms_join", C.c_float), ("ms_verify", C.c_float), ("ms_emit", C.c_float), ("ms_order", C.c_float),
                ("build_validity", C.POINTER(Validity)), ("probe_validity", C.POINTER(Validity)), ("n_build_null", C.c_uint64),
                ("n_probe_null", C.c_uint64)]


class ColsResult(C.Structure):
    """hmj_cols_result: counts and sums as JoinResult (tmix over (key64, rval, sval)); device columns with HMJ_MATERIALIZE."""
    _fields_ = [("n_matches", C.c_uint64), ("sum_r", C.c_uint64), ("sum_s", C.c_uint64),
                ("xor_fold", C.c_uint64), ("mix_sum", C.c_uint64), ("sum_probe_all", C.c_uint64),
                ("key64", C.c_void_p), ("r_row", C.c_void_p), ("s_row", C.c_void_p), ("rval", C.c_void_p), ("sval", C.c_void_p)]

    def checks(self):
        return {k: int(getattr(self, k)) for k in ("n_matches", "sum_r", "sum_s", "xor_fold", "mix_sum")}


# hmj_join_mixed_device: key tuples of Arrow large_string and fixed-width columns
HMJ_KEY_FIXED, HMJ_KEY_LARGE_STRING = 0, 1


class MixedCol(C.Structure):
    """hmj_mixed_col: one key column on the device -- FIXED: n values of `width` bytes; LARGE_STRING: a chars buffer (width
    0) and n + 1 64-bit offsets -- and its validity bitmap (bits NULL: no NULL in the column)."""
    _fields_ = [("type", C.c_uint32), ("width", C.c_uint32), ("data", C.c_void_p), ("offsets", C.c_void_p),
                ("validity", Validity)]


class MixedRel(C.Structure):
    """hmj_mixed_rel: a relation keyed by a tuple of string and fixed-width columns + optional payloads."""
    _fields_ = [("cols", C.POINTER(MixedCol)), ("n_cols", C.c_uint32), ("reserved", C.c_uint32), ("vals", C.c_void_p),
                ("n", C.c_uint64)]


class MixedOpts(C.Structure):
    """hmj_mixed_opts: side, kind, hash bits and fill values (in); the kind's counters, pairs of equal key64, pairs whose
    tuples differ, the NULL-key rows per side and phase times (out)."""
    _fields_ = [("struct_size", C.c_uint32), ("side", C.c_uint32), ("kind", C.c_uint32), ("hash_bits", C.c_uint32),
                ("probe_fill", C.c_uint64), ("build_fill", C.c_uint64), ("counts", KindCounts), ("n_key_pairs", C.c_uint64),
                ("n_collisions", C.c_uint64), ("n_build_null", C.c_uint64), ("n_probe_null", C.c_uint64), ("ms_key", C.c_float),
                ("ms_join", C.c_float), ("ms_verify", C.c_float), ("ms_emit", C.c_float), ("ms_order", C.c_float)]


# hmj_group_cols_device / hmj_group_mixed_device: rows grouped by multi-column / string and mixed keys; hmj_group_opts.want
HMJ_GROUP_COUNT, HMJ_GROUP_SUM, HMJ_GROUP_MIN, HMJ_GROUP_MAX, HMJ_GROUP_ROW_MAP = 0x01, 0x02, 0x04, 0x08, 0x10


class GroupOpts(C.Structure):
    """hmj_group_opts: the columns wanted, hash bits, the forced hashed form and the key columns' validity bitmaps (in); the
    form taken, the rows with a NULL key slot, the heads inside runs of equal key64 and phase times (out)."""
    _fields_ = [("struct_size", C.c_uint32), ("want", C.c_uint32), ("hash_bits", C.c_uint32), ("force_hashed", C.c_uint32),
                ("form", C.c_uint32), ("reserved", C.c_uint32), ("validity", C.POINTER(Validity)), ("n_null", C.c_uint64),
                ("n_collisions", C.c_uint64), ("ms_key", C.c_float), ("ms_sort", C.c_float), ("ms_groups", C.c_float),
                ("ms_agg", C.c_float)]


class GroupResult(C.Structure):
    """hmj_group_result: groups, rows and the largest group's rows; device columns with HMJ_MATERIALIZE (NULL when not
    asked for)."""
    _fields_ = [("n_groups", C.c_uint64), ("n_rows", C.c_uint64), ("max_count", C.c_uint64), ("key64", C.c_void_p),
                ("first_row", C.c_void_p), ("count", C.c_void_p), ("sum", C.c_void_p), ("min", C.c_void_p), ("max", C.c_void_p),
                ("group_of_row", C.c_void_p)]


# hmj_group_agg_device: typed value columns aggregated over the ctx's live grouping; hmj_agg_src.op and .type
HMJ_AGG_COUNT, HMJ_AGG_SUM, HMJ_AGG_MIN, HMJ_AGG_MAX, HMJ_AGG_MEAN = 0, 1, 2, 3, 4
HMJ_TYPE_I8, HMJ_TYPE_I16, HMJ_TYPE_I32, HMJ_TYPE_I64 = 0, 1, 2, 3
HMJ_TYPE_U8, HMJ_TYPE_U16, HMJ_TYPE_U32, HMJ_TYPE_U64 = 4, 5, 6, 7
HMJ_TYPE_F32, HMJ_TYPE_F64 = 8, 9
HMJ_MAX_AGGS = 64


class AggSrc(C.Structure):
    """hmj_agg_src: one aggregate's source column on the device -- n_rows values of `type` (HMJ_TYPE_*), aligned to their
    width (NULL allowed for HMJ_AGG_COUNT) --, the operation (HMJ_AGG_*) and the column's validity bitmap (bits NULL: no
    NULL in the column)."""
    _fields_ = [("data", C.c_void_p), ("type", C.c_uint32), ("op", C.c_uint32), ("validity", Validity)]


class AggDst(C.Structure):
    """hmj_agg_dst: one caller-owned output column -- n_groups values of the aggregate's output type, an optional bitmap of
    ceil(n_groups / 64) 64-bit words (in); its NULL slots (out)."""
    _fields_ = [("data", C.c_void_p), ("validity", C.c_void_p), ("null_count", C.c_uint64)]


class GroupAggOpts(C.Structure):
    """hmj_group_agg_opts: the live grouping's groups and the kernel time (out)."""
    _fields_ = [("struct_size", C.c_uint32), ("reserved", C.c_uint32), ("n_groups", C.c_uint64), ("ms_agg", C.c_float)]


# hmj_order_by_device: a stable multi-column ORDER BY to a row map; hmj_order_col.type (beside HMJ_TYPE_*) and .flags
HMJ_ORDER_LARGE_STRING = 16
HMJ_ORDER_DESC, HMJ_ORDER_NULLS_FIRST = 0x1, 0x2
HMJ_MAX_ORDER_COLS = 8


class OrderCol(C.Structure):
    """hmj_order_col: one key column on the device -- n values of a HMJ_TYPE_* aligned to their width, or (type
    HMJ_ORDER_LARGE_STRING) chars and n + 1 64-bit offsets --, its HMJ_ORDER_* flags and its validity bitmap (bits NULL: no
    NULL in the column)."""
    _fields_ = [("type", C.c_uint32), ("flags", C.c_uint32), ("data", C.c_void_p), ("offsets", C.c_void_p), ("validity", Validity)]


class OrderOpts(C.Structure):
    """hmj_order_opts: distinct key tuples, tied rows, sort rounds and the phase times (out)."""
    _fields_ = [("struct_size", C.c_uint32), ("reserved", C.c_uint32), ("n_distinct", C.c_uint64), ("n_tied_rows", C.c_uint64),
                ("n_rounds", C.c_uint32), ("reserved2", C.c_uint32), ("ms_key", C.c_float), ("ms_sort", C.c_float),
                ("ms_refine", C.c_float), ("ms_map", C.c_float)]


# hmj_window_device: window functions over ordered partitions (OVER); hmj_window_fn.op and the cap of a call.  The struct
# mirrors (WindowFn, WindowDst, WindowOpts) live in _window.py.
(HMJ_WIN_ROW_NUMBER, HMJ_WIN_RANK, HMJ_WIN_DENSE_RANK, HMJ_WIN_CUM_COUNT, HMJ_WIN_CUM_SUM, HMJ_WIN_CUM_MIN, HMJ_WIN_CUM_MAX,
 HMJ_WIN_LAG, HMJ_WIN_LEAD) = range(9)
HMJ_MAX_WINDOW_FNS = 32

# hmj_top_k_device: ORDER BY ... LIMIT k [OFFSET o]; hmj_top_k_opts.plan / .plan_taken.  The struct mirror (TopKOpts) lives
# in _topk.py.
HMJ_TOPK_AUTO, HMJ_TOPK_SELECT, HMJ_TOPK_FULL = 0, 1, 2


# hmj_filter_device: a CNF predicate over typed and string columns to a row map (WHERE); hmj_filter_term.type (beside
# HMJ_TYPE_*), .op and .flags, and the two caps of a call
HMJ_FILTER_LARGE_STRING = 16
(HMJ_FILTER_EQ, HMJ_FILTER_NE, HMJ_FILTER_LT, HMJ_FILTER_LE, HMJ_FILTER_GT, HMJ_FILTER_GE, HMJ_FILTER_BETWEEN, HMJ_FILTER_IS_NULL,
 HMJ_FILTER_IS_NOT_NULL, HMJ_FILTER_STARTS_WITH, HMJ_FILTER_ENDS_WITH) = range(11)
HMJ_FILTER_NOT = 0x1
HMJ_MAX_FILTER_TERMS = 16
HMJ_MAX_FILTER_LITERAL_BYTES = 4096


class FilterTerm(C.Structure):
    """hmj_filter_term: one column on the device -- n_src values of a HMJ_TYPE_* aligned to their width, or (type
    HMJ_FILTER_LARGE_STRING) chars_bytes chars and n_src + 1 64-bit offsets --, its validity bitmap (bits NULL: no NULL), the
    row map the term reads it through (NULL: position i reads row i), one HMJ_FILTER_* op with HMJ_FILTER_NOT or not, the
    clause the term belongs to, and the literals: lit for a fixed column (the value's bits in the low bytes), str_lit /
    str_len (HOST pointers) for a string column."""
    _fields_ = [("type", C.c_uint32), ("op", C.c_uint32), ("flags", C.c_uint32), ("clause", C.c_uint32), ("data", C.c_void_p),
                ("offsets", C.c_void_p), ("chars_bytes", C.c_uint64), ("validity", Validity), ("n_src", C.c_uint64),
                ("row_map", C.c_void_p), ("lit", C.c_uint64 * 2), ("str_lit", C.c_void_p * 2), ("str_len", C.c_uint64 * 2),
                ("reserved", C.c_uint64)]


class FilterOpts(C.Structure):
    """hmj_filter_opts: the positions at which the predicate is TRUE and UNKNOWN, and the phase times (out)."""
    _fields_ = [("struct_size", C.c_uint32), ("reserved", C.c_uint32), ("n_out", C.c_uint64), ("n_unknown", C.c_uint64),
                ("ms_eval", C.c_float), ("ms_write", C.c_float), ("reserved2", C.c_uint64)]


# hmj_take_cols_device: fixed-width columns taken through a row map (a join's r_row / s_row)
HMJ_TAKE_NO_ROW = 0xFFFFFFFFFFFFFFFF
HMJ_MAX_TAKE_COLS = 64


class TakeSrc(C.Structure):
    """hmj_take_src: one source column on the device -- n_src values of `width` bytes (1, 2, 4, 8 or 16), aligned to `width`,
    and its validity bitmap (bits NULL: no NULL in the column)."""
    _fields_ = [("data", C.c_void_p), ("width", C.c_uint32), ("reserved", C.c_uint32), ("validity", Validity)]


class TakeDst(C.Structure):
    """hmj_take_dst: one caller-owned output column -- n_out values, an optional bitmap of ceil(n_out / 64) 64-bit words (in);
    its NULL slots (out)."""
    _fields_ = [("data", C.c_void_p), ("validity", C.c_void_p), ("null_count", C.c_uint64)]


class TakeOpts(C.Structure):
    """hmj_take_opts: the map entries equal to HMJ_TAKE_NO_ROW and the kernel time (out)."""
    _fields_ = [("struct_size", C.c_uint32), ("reserved", C.c_uint32), ("n_no_row", C.c_uint64), ("ms_take", C.c_float)]


# hmj_take_str_device: one Arrow large_string / large_binary column taken through a row map
class TakeStrSrc(C.Structure):
    """hmj_take_str_src: the source column on the device -- chars (any alignment; NULL when chars_bytes is 0), the size of
    the chars buffer, n_src + 1 offsets (offsets[0] need not be 0) and its validity bitmap (bits NULL: no NULL)."""
    _fields_ = [("chars", C.c_void_p), ("chars_bytes", C.c_uint64), ("offsets", C.c_void_p), ("validity", Validity)]


class TakeStrDst(C.Structure):
    """hmj_take_str_dst: the caller-owned output column -- n_out + 1 offsets, chars aligned to 16 (NULL: a sizing call) with
    their capacity, an optional bitmap of ceil(n_out / 64) 64-bit words (in); its NULL slots and offsets[n_out] (out)."""
    _fields_ = [("offsets", C.c_void_p), ("chars", C.c_void_p), ("chars_capacity", C.c_uint64), ("validity", C.c_void_p),
                ("null_count", C.c_uint64), ("total_bytes", C.c_uint64)]


class TakeStrOpts(C.Structure):
    """hmj_take_str_opts: the map entries equal to HMJ_TAKE_NO_ROW and the times of the two phases (out)."""
    _fields_ = [("struct_size", C.c_uint32), ("reserved", C.c_uint32), ("n_no_row", C.c_uint64), ("ms_offsets", C.c_float),
                ("ms_chars", C.c_float)]


class Timing(C.Structure):
    _fields_ = [("ms_total", C.c_float), ("ms_h2d", C.c_float), ("ms_d2h", C.c_float),
                ("ms_partition_build", C.c_float), ("ms_partition_probe", C.c_float),
                ("ms_hist", C.c_float), ("ms_scan", C.c_float), ("ms_scatter", C.c_float),
                ("ms_offsets", C.c_float), ("ms_probe_count", C.c_float),
                ("ms_out_scan", C.c_float), ("ms_probe_write", C.c_float), ("ms_order", C.c_float),
                ("radix_bits", C.c_int), ("radix_passes", C.c_int),
                ("n_scatter_launches", C.c_int), ("n_split_retries", C.c_int),
                ("bytes_scatter", C.c_uint64), ("bytes_hist", C.c_uint64),
                ("bytes_probe_count", C.c_uint64), ("bytes_probe_write", C.c_uint64),
                ("path", C.c_uint32), ("key_prefix_bits", C.c_int32), ("key_window_low", C.c_int32),
                ("n_probe_items", C.c_uint32), ("ms_scatter_pass0", C.c_float), ("ms_scatter_pass1", C.c_float)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class PlanDesc(C.Structure):
    """hmj_plan_desc: how the last join was planned and why (include/hmj.h)."""
    _fields_ = [("struct_size", C.c_uint32), ("path", C.c_uint32), ("radix_bits", C.c_int32), ("radix_passes", C.c_int32),
                ("pass_bits", C.c_int32 * 4), ("key_prefix_bits", C.c_int32), ("key_window_low", C.c_int32),
                ("n_partitions", C.c_uint32), ("probe_items", C.c_uint32), ("attempts", C.c_uint32), ("refused", C.c_uint32),
                ("cooling", C.c_uint32), ("workload", C.c_uint64)]

    def as_dict(self):
        d = {n: getattr(self, n) for n, _ in self._fields_}
        d["pass_bits"] = list(self.pass_bits)
        return d


# hmj_plan_desc.refused / .cooling bits
HMJ_REFUSED_GTABLE_SHAPE, HMJ_REFUSED_GTABLE_COOLING, HMJ_REFUSED_GTABLE_GAVE_UP = 0x1, 0x2, 0x4
HMJ_REFUSED_RANK_SORT_MODEL, HMJ_REFUSED_RANK_SORT_COOLING, HMJ_REFUSED_RANK_SORT_GAVE_UP = 0x8, 0x10, 0x20
HMJ_REFUSED_SLAB_SHAPE, HMJ_REFUSED_SLAB_COOLING, HMJ_REFUSED_SLAB_SORTED_INPUT, HMJ_REFUSED_SLAB_OVERFLOW = 0x40, 0x80, 0x100, 0x200
HMJ_REFUSED_FAST_WRITE_COOLING, HMJ_REFUSED_FAST_WRITE_GAVE_UP = 0x400, 0x800
HMJ_REFUSED_SLAB_PROBE_COOLING, HMJ_REFUSED_SLAB_PROBE_OVERFLOW = 0x1000, 0x2000
HMJ_REFUSED_PREFIX_VIOLATED, HMJ_REFUSED_EXPANSION_GAVE_UP = 0x4000, 0x8000
HMJ_REFUSED_PROBE_KEYS_GAVE_UP, HMJ_REFUSED_PROBE_KEYS_COOLING = 0x10000, 0x20000
HMJ_COOL_UNIQ_WRITE, HMJ_COOL_SORTED_WRITE, HMJ_COOL_GTABLE, HMJ_COOL_GTABLE_WRITE = 0x1, 0x2, 0x4, 0x8
HMJ_COOL_RANK_SORT, HMJ_COOL_RANK_SORT_SLAB, HMJ_COOL_EXPANSION, HMJ_COOL_SORT_SLAB = 0x10, 0x20, 0x40, 0x80
HMJ_COOL_SLAB, HMJ_COOL_SLAB_PROBE, HMJ_COOL_ONE_PASS_WRITE, HMJ_COOL_EXACT_PREFIX = 0x100, 0x200, 0x400, 0x800
HMJ_COOL_RANK_RUNS, HMJ_COOL_SORT_MSD = 0x1000, 0x2000
HMJ_COOL_PROBE_KEYS = 0x4000


HMJ_PLACE_MAX_CAND = 4


class PlaceInfo(C.Structure):
    _fields_ = [("name", C.c_char * 16), ("bytes", C.c_uint64), ("fill_TBps", C.c_float), ("candidates", C.c_int),
                ("ms_search", C.c_float), ("searched", C.c_int), ("aborted", C.c_int), ("budget_ms", C.c_float),
                ("cand_ms_alloc", C.c_float * HMJ_PLACE_MAX_CAND), ("cand_ms_fill", C.c_float * HMJ_PLACE_MAX_CAND),
                ("cand_TBps", C.c_float * HMJ_PLACE_MAX_CAND)]


def lib_path():
    # HMJ_LIB: developer override to A/B an alternative build of the same library
    return os.environ.get("HMJ_LIB") or os.path.join(_HERE, "libhmj_hip.so")


class ExchangeInfo(C.Structure):
    _fields_ = [("n_ranks", C.c_int), ("owner_mode", C.c_int), ("rounds_build", C.c_uint32), ("rounds_probe", C.c_uint32),
                ("recv_build", C.c_uint64), ("recv_probe", C.c_uint64), ("ms_split", C.c_float),
                ("ms_exchange_build", C.c_float), ("ms_exchange_probe", C.c_float), ("ms_local", C.c_float),
                ("ms_total", C.c_float), ("digit_bits", C.c_int32), ("digit_low", C.c_int32), ("n_subjoins", C.c_uint32),
                ("fallback", C.c_uint32), ("sample_max_share", C.c_float), ("ms_kernels", C.c_float),
                ("ms_exposed", C.c_float)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


HMJ_MAX_RANKS, HMJ_MAX_ROUNDS = 16, 16
HMJ_UNIQUE_ID_BYTES = 128
HMJ_OWNER_DIGIT, HMJ_OWNER_SPLIT = 0, 1  # hmj_comm_set_owner_path


class DigitPlan(C.Structure):
    _fields_ = [("usable", C.c_int32), ("digit_bits", C.c_int32), ("digit_low", C.c_int32), ("n_rounds", C.c_uint32),
                ("owner_first", C.c_uint32 * (HMJ_MAX_RANKS + 1)),
                ("round_first", (C.c_uint32 * (HMJ_MAX_ROUNDS + 1)) * HMJ_MAX_RANKS), ("max_share", C.c_float)]


# hmj_transport: the two collectives a host may supply instead of RCCL (include/hmj.h)
ALLGATHER_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.c_int)
ALLTOALLV_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64),
                           C.POINTER(C.c_void_p), C.POINTER(C.c_uint64), C.c_void_p)


class Transport(C.Structure):
    _fields_ = [("user", C.c_void_p), ("n_ranks", C.c_int), ("rank", C.c_int), ("allgather_u64", ALLGATHER_FN),
                ("alltoallv", ALLTOALLV_FN)]


# every function of include/hmj.h: name -> (restype, argtypes)
_i, _u, _u32, _vp, _cp, _P = C.c_int, C.c_uint64, C.c_uint32, C.c_void_p, C.c_char_p, C.POINTER
_SIGNATURES = {
    "hmj_create": (_i, [_P(_vp), _i]),
    "hmj_destroy": (None, [_vp]),
    "hmj_set_stream": (_i, [_vp, _vp]),
    "hmj_reserve": (_i, [_vp, _u, _u, _u, _u32]),
    "hmj_set_radix_bits": (_i, [_vp, _i]),
    "hmj_autotune_radix_bits": (_i, [_vp, _u, _u, _i, _P(_i), _P(C.c_double)]),
    "hmj_set_key_prefix_bits": (_i, [_vp, _i]),
    "hmj_plan": (_i, [_u, _P(_i), _P(_i), _P(_i * 4)]),
    "hmj_set_profiling": (_i, [_vp, _i]),
    "hmj_last_timing": (_i, [_vp, _P(Timing)]),
    "hmj_last_plan": (_i, [_vp, _P(PlanDesc)]),
    "hmj_forget_workloads": (_i, [_vp]),
    "hmj_placement_info": (_i, [_vp, _P(PlaceInfo), _i]),
    "hmj_strerror": (_cp, [_i]),
    "hmj_last_error": (_cp, [_vp]),
    "hmj_version": (_cp, []),
    "hmj_abi_version": (_i, []),
    "hmj_join_u64_device": (_i, [_vp, _vp, _u, _vp, _u, _u32, _P(JoinResult)]),
    "hmj_join_kind_u64_device": (_i, [_vp, _vp, _u, _vp, _u, _u32, _P(JoinOpts), _P(JoinResult)]),
    "hmj_join_build_kind_u64_device": (_i, [_vp, _vp, _u, _vp, _u, _u32, _P(BuildJoinOpts), _P(JoinResult)]),
    "hmj_hash_str_device": (_i, [_vp, _vp, _vp, _u, _u32, _vp]),
    "hmj_join_str_device": (_i, [_vp, _P(StrRel), _P(StrRel), _u32, _P(StrJoinOpts), _P(StrResult)]),
    "hmj_join_kind_str_device": (_i, [_vp, _P(StrRel), _P(StrRel), _u32, _P(StrKindOpts), _P(StrResult)]),
    "hmj_join_cols_device": (_i, [_vp, _P(ColsRel), _P(ColsRel), _u32, _P(ColsJoinOpts), _P(ColsResult)]),
    "hmj_join_kind_cols_device": (_i, [_vp, _P(ColsRel), _P(ColsRel), _u32, _P(ColsKindOpts), _P(ColsResult)]),
    "hmj_join_mixed_device": (_i, [_vp, _P(MixedRel), _P(MixedRel), _u32, _P(MixedOpts), _P(ColsResult)]),
    "hmj_group_cols_device": (_i, [_vp, _P(ColsRel), _u32, _P(GroupOpts), _P(GroupResult)]),
    "hmj_group_mixed_device": (_i, [_vp, _P(MixedRel), _u32, _P(GroupOpts), _P(GroupResult)]),
    "hmj_group_agg_device": (_i, [_vp, _P(AggSrc), _u32, _u, _P(AggDst), _P(GroupAggOpts)]),
    "hmj_order_by_device": (_i, [_vp, _P(OrderCol), _u32, _u, _vp, _P(OrderOpts)]),
    "hmj_window_device": (_i, [_vp, _P(OrderCol), _u32, _u, _vp, _u32, _vp, _vp, _vp]),
    "hmj_top_k_device": (_i, [_vp, _P(OrderCol), _u32, _u, _u, _vp, _vp]),
    "hmj_filter_device": (_i, [_vp, _P(FilterTerm), _u32, _u, _vp, _vp, _P(FilterOpts)]),
    "hmj_take_cols_device": (_i, [_vp, _P(TakeSrc), _u32, _u, _vp, _u, _P(TakeDst), _P(TakeOpts)]),
    "hmj_take_str_device": (_i, [_vp, _P(TakeStrSrc), _u, _vp, _u, _P(TakeStrDst), _P(TakeStrOpts)]),
    "hmj_prepare_build_u64_device": (_i, [_vp, _vp, _u, _u]),
    "hmj_join_u64": (_i, [_vp, _vp, _u, _vp, _u, _u32, _P(JoinResult)]),
    "hmj_join_u64_rows": (_i, [_vp, _vp, _u, _vp, _u, _u32, _P(JoinResult), _P(_vp)]),
    "hmj_rows_free": (None, [_vp]),
    "hmj_host_pool_trim": (_u, [_u]),
    "hmj_host_pool_bytes": (_u, []),
    "hmj_set_host_threads": (_i, [_vp, _i]),
    "hmj_release_result": (None, [_vp]),
    "hmj_comm_unique_id": (_i, [_vp]),
    "hmj_comm_init_rank": (_i, [_vp, _i, _i, _vp]),
    "hmj_comm_set_transport": (_i, [_vp, _P(Transport)]),
    "hmj_comm_destroy": (_i, [_vp]),
    "hmj_comm_set_message_bytes": (_i, [_vp, _u, _u]),
    "hmj_exchange_join_u64_device": (_i, [_vp, _vp, _u, _vp, _u, _u32, _P(JoinResult), _P(JoinResult)]),
    "hmj_exchange_join_kind_u64_device": (_i, [_vp, _vp, _u, _vp, _u, _u32, _P(ExchangeKindOpts), _P(JoinResult), _P(JoinResult)]),
    "hmj_owner_split_u64_device": (_i, [_vp, _vp, _u, _i, _U64P, _vp, _vp]),
    "hmj_last_exchange_info": (_i, [_vp, _P(ExchangeInfo)]),
    "hmj_comm_set_timeout_ms": (_i, [_vp, _u]),
    "hmj_comm_get_timeout_ms": (_i, [_vp, _U64P]),
    "hmj_comm_set_owner_path": (_i, [_vp, _i]),
    "hmj_comm_set_self_exchange": (_i, [_vp, _i]),
    "hmj_exchange_digit_plan": (_i, [_i, _U64P, _u, _u32, _P(DigitPlan)]),
    "hmj_exchange_digit_layout": (_i, [_i, _i, _P(DigitPlan), _U64P, _U64P, _U64P, _U64P, _U64P, _U64P]),
    "hmj_exchange_rounds": (_u32, [_i, _U64P, _u]),
    "hmj_exchange_layout": (_i, [_i, _i, _U64P, _u32, _i, _U64P, _U64P, _U64P, _U64P, _U64P]),
    "hmj_partition_u64_device": (_i, [_vp, _vp, _u, _i, _i, _vp, _vp]),
    "hmj_sort_u64_device": (_i, [_vp, _vp, _u, _vp]),
    "hmj_sort_rows_by_u64_host": (_i, [_vp, _vp, _u, _u32, _u32]),
    "hmj_argsort_u64_host": (_i, [_vp, _vp, _u, _u32, _vp]),
    "hmj_gen_build_u64_device": (_i, [_vp, _vp, _u, _u, _u]),
    "hmj_gen_probe_u64_device": (_i, [_vp, _vp, _u, _u, _u, _u, _u]),
    "hmj_gen_from_cdf_u64_device": (_i, [_vp, _vp, _u, _u, _vp, _u, _u, _u]),
    "hmj_gen_uniform_domain_u64_device": (_i, [_vp, _vp, _u, _u, _u, _u, _u]),
}

_LIB = None


def load_library():
    """Load libhmj_hip.so.  torch (if used by the caller) must be imported BEFORE this so that both
    share one HIP runtime (the wheel bundles libamdhip64 under the same SONAME)."""
    global _LIB
    if _LIB is not None:
        return _LIB
    path = lib_path()
    if not os.path.exists(path):
        raise HmjError(-100, "HIP extension not built: %s is missing (run `make` at the repo root)" % path)
    L = C.CDLL(path)
    for name, (restype, argtypes) in _SIGNATURES.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = restype, argtypes
    _LIB = L
    return L


__all__ = sorted(k for k, v in list(globals().items())
                 if k.startswith("HMJ_") or (isinstance(v, type) and issubclass(v, C.Structure)))
__all__ += ["HmjError", "lib_path", "load_library"]
