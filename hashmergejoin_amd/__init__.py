"""hashmergejoin_amd -- MI355X-native radix-partitioned hash join (host-side Python binding).

The product is libhmj_hip.so (hand-written HIP for gfx950 behind the C ABI of include/hmj.h).  This
package is a thin ctypes binding over that ABI plus a mirror of the reference's operator surface
(`HashMergeJoin`, reference hashjoin.h:33-199).  There is no CPU implementation here: if the
library or a GPU is missing, calls raise.
"""
from ._lib import (HMJ_AGG_COUNT, HMJ_AGG_MAX, HMJ_AGG_MEAN, HMJ_AGG_MIN, HMJ_AGG_SUM, HMJ_MAX_AGGS, HMJ_TYPE_F32, HMJ_TYPE_F64, HMJ_TYPE_I8, HMJ_TYPE_I16, HMJ_TYPE_I32, HMJ_TYPE_I64, HMJ_TYPE_U8, HMJ_TYPE_U16, HMJ_TYPE_U32, HMJ_TYPE_U64, AggDst, AggSrc, GroupAggOpts,
                   HMJ_BUILD_ANTI, HMJ_BUILD_OUTER, HMJ_BUILD_SEMI, HMJ_CHECKSUM, HMJ_COLS_HASHED, HMJ_COLS_NO_ROW, HMJ_COLS_PACKED, HMJ_FIRST_WINS, HMJ_FULL_OUTER, HMJ_GROUP_COUNT, HMJ_GROUP_MAX, HMJ_GROUP_MIN, HMJ_GROUP_ROW_MAP, HMJ_GROUP_SUM, HMJ_JOIN_ANTI, HMJ_JOIN_INNER, HMJ_JOIN_PROBE_OUTER, HMJ_JOIN_SEMI, HMJ_KIND_BUILD_SIDE, HMJ_KIND_PROBE_SIDE, HMJ_MATERIALIZE, HMJ_ORDERED, HMJ_PATH_CHUNKED_BUILD, HMJ_PATH_DENSE_BUILD,
                   HMJ_PATH_EXACT, HMJ_PATH_GLOBAL_TABLE, HMJ_PATH_HOST_PIPELINE, HMJ_PATH_HOT_KEY_HINT, HMJ_PATH_LOOKBACK_TIMEOUT, HMJ_PATH_ORDER_BY_KEY, HMJ_PATH_ORDER_BY_RANK_SORT, HMJ_PATH_ORDER_DEFERRED, HMJ_PATH_ORDERED_EXPANSION, HMJ_PATH_LDS_TABLE,
                   HMJ_PATH_KEY_RANGES, HMJ_PATH_PREPARED, HMJ_PATH_PRESORTED, HMJ_PATH_RANK_RUNS, HMJ_PATH_SORT_MSD, HMJ_PATH_SLAB, HMJ_PATH_SLAB_ONE_PASS, HMJ_PATH_SLAB_PROBE, HMJ_PATH_SORTED_FK, HMJ_PATH_SORTED_FK_HALF, HMJ_PATH_SORTED_FK_WIDE, HMJ_PATH_SORTED_WRITE, HMJ_PATH_SPLIT, HMJ_PATH_UNIQ_WRITE, HMJ_PATH_WINDOW,
                   HMJ_KEY_FIXED, HMJ_KEY_LARGE_STRING, HMJ_MAX_KEY_COLS, HMJ_MAX_TAKE_COLS, HMJ_NULL_EQUAL, HMJ_STR_NO_ROW, HMJ_SUM_PROBE, HMJ_TAKE_NO_ROW, BuildJoinOpts, ColsJoinOpts, ColsKindOpts, ColsRel, ColsResult, ExchangeKindOpts, GroupOpts, GroupResult, HmjError, JoinOpts, JoinResult, KeyCol, KindCounts, MixedCol, MixedOpts, MixedRel, StrJoinOpts, StrKindOpts, StrRel, StrResult, TakeDst, TakeOpts, TakeSrc, TakeStrDst, TakeStrOpts, TakeStrSrc, Timing, Validity,
                   HMJ_MAX_ORDER_COLS, HMJ_ORDER_DESC, HMJ_ORDER_LARGE_STRING, HMJ_ORDER_NULLS_FIRST, OrderCol, OrderOpts,
                   HMJ_FILTER_LARGE_STRING, HMJ_FILTER_EQ, HMJ_FILTER_NE, HMJ_FILTER_LT, HMJ_FILTER_LE, HMJ_FILTER_GT, HMJ_FILTER_GE, HMJ_FILTER_BETWEEN, HMJ_FILTER_IS_NULL, HMJ_FILTER_IS_NOT_NULL, HMJ_FILTER_STARTS_WITH, HMJ_FILTER_ENDS_WITH, HMJ_FILTER_NOT, HMJ_MAX_FILTER_TERMS, HMJ_MAX_FILTER_LITERAL_BYTES, FilterTerm, FilterOpts,
                   lib_path, load_library)
from .join import Executor, HashMergeJoin, cols_key64, expected_group_aggs, expected_groups, expected_filter, expected_mixed_groups, expected_order_by, mixed_key64, order_stream_bytes, pack_strings, pack_validity, plan, unpack_strings, unpack_validity

__all__ = ["Executor", "HashMergeJoin", "plan", "HmjError", "JoinResult", "Timing", "load_library",
           "lib_path", "HMJ_MATERIALIZE", "HMJ_ORDERED", "HMJ_FIRST_WINS", "HMJ_CHECKSUM",
           "HMJ_SUM_PROBE", "JoinOpts", "HMJ_JOIN_INNER", "HMJ_JOIN_SEMI", "HMJ_JOIN_ANTI", "HMJ_JOIN_PROBE_OUTER",
           "BuildJoinOpts", "HMJ_BUILD_SEMI", "HMJ_BUILD_ANTI", "HMJ_BUILD_OUTER", "HMJ_FULL_OUTER",
           "ExchangeKindOpts", "KindCounts", "HMJ_KIND_PROBE_SIDE", "HMJ_KIND_BUILD_SIDE",
           "pack_strings", "StrRel", "StrJoinOpts", "StrResult", "StrKindOpts", "HMJ_STR_NO_ROW",
           "KeyCol", "ColsRel", "ColsJoinOpts", "ColsResult", "HMJ_COLS_PACKED", "HMJ_COLS_HASHED", "HMJ_MAX_KEY_COLS",
           "cols_key64", "ColsKindOpts", "HMJ_COLS_NO_ROW", "Validity", "pack_validity",
           "TakeSrc", "TakeDst", "TakeOpts", "HMJ_TAKE_NO_ROW", "HMJ_MAX_TAKE_COLS", "unpack_validity",
           "TakeStrSrc", "TakeStrDst", "TakeStrOpts", "unpack_strings",
           "MixedCol", "MixedRel", "MixedOpts", "HMJ_KEY_FIXED", "HMJ_KEY_LARGE_STRING", "mixed_key64",
           "HMJ_NULL_EQUAL",
           "GroupOpts", "GroupResult", "HMJ_GROUP_COUNT", "HMJ_GROUP_SUM", "HMJ_GROUP_MIN", "HMJ_GROUP_MAX", "HMJ_GROUP_ROW_MAP",
           "expected_groups", "expected_mixed_groups",
           "AggSrc", "AggDst", "GroupAggOpts", "HMJ_AGG_COUNT", "HMJ_AGG_SUM", "HMJ_AGG_MIN", "HMJ_AGG_MAX", "HMJ_AGG_MEAN",
           "HMJ_TYPE_I8", "HMJ_TYPE_I16", "HMJ_TYPE_I32", "HMJ_TYPE_I64", "HMJ_TYPE_U8", "HMJ_TYPE_U16", "HMJ_TYPE_U32",
           "HMJ_TYPE_U64", "HMJ_TYPE_F32", "HMJ_TYPE_F64", "HMJ_MAX_AGGS", "expected_group_aggs",
           "OrderCol", "OrderOpts", "HMJ_ORDER_LARGE_STRING", "HMJ_ORDER_DESC", "HMJ_ORDER_NULLS_FIRST", "HMJ_MAX_ORDER_COLS",
           "expected_order_by", "order_stream_bytes",
           "HMJ_FILTER_LARGE_STRING", "HMJ_FILTER_EQ", "HMJ_FILTER_NE", "HMJ_FILTER_LT", "HMJ_FILTER_LE", "HMJ_FILTER_GT", "HMJ_FILTER_GE", "HMJ_FILTER_BETWEEN",
           "HMJ_FILTER_IS_NULL", "HMJ_FILTER_IS_NOT_NULL", "HMJ_FILTER_STARTS_WITH", "HMJ_FILTER_ENDS_WITH", "HMJ_FILTER_NOT", "HMJ_MAX_FILTER_TERMS", "HMJ_MAX_FILTER_LITERAL_BYTES", "FilterTerm", "FilterOpts", "expected_filter"]
