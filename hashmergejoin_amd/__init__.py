"""hashmergejoin_amd -- MI355X-native radix-partitioned hash join (host-side Python binding).

The product is libhmj_hip.so (hand-written HIP for gfx950 behind the C ABI of include/hmj.h).  This
package is a thin ctypes binding over that ABI plus a mirror of the reference's operator surface
(`HashMergeJoin`, reference hashjoin.h:33-199).  There is no CPU implementation here: if the
library or a GPU is missing, calls raise.
"""
from . import _lib
from ._lib import *  # noqa: F401,F403  (_lib.__all__: the HMJ_* constants, the struct mirrors, HmjError, lib_path, load_library)
from ._topk import TopKOpts
from ._window import WindowDst, WindowFn, WindowOpts
from .join import Executor, HashMergeJoin, pack_strings, pack_validity, plan, unpack_strings, unpack_validity
from .reference import (cols_key64, expected_filter, expected_group_aggs, expected_groups, expected_mixed_groups,
                        expected_order_by, expected_top_k, expected_window, mixed_key64, order_stream_bytes)

__all__ = _lib.__all__ + ["Executor", "HashMergeJoin", "plan", "pack_strings", "unpack_strings", "pack_validity",
                          "unpack_validity", "cols_key64", "mixed_key64", "expected_groups", "expected_mixed_groups",
                          "expected_group_aggs", "expected_order_by", "order_stream_bytes", "expected_filter", "expected_window",
                          "WindowFn", "WindowDst", "WindowOpts", "expected_top_k", "TopKOpts"]
