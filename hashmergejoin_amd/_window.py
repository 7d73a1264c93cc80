"""The struct mirrors of hmj_window_device (include/hmj.h, "window functions over ordered partitions"): hmj_window_fn,
hmj_window_dst and hmj_window_opts.  The HMJ_WIN_* constants and the entry's signature are in _lib like every other
entry's; `Executor.window_device` (join.py) fills these."""
import ctypes as C

from ._lib import Validity


class WindowFn(C.Structure):
    """hmj_window_fn: one function's source column on the device -- n values of `type` (HMJ_TYPE_*), aligned to their
    width (NULL where the op reads no value) --, the operation (HMJ_WIN_*), the column's validity bitmap (bits NULL: no
    NULL in the column) and the row offset of HMJ_WIN_LAG / HMJ_WIN_LEAD."""
    _fields_ = [("data", C.c_void_p), ("type", C.c_uint32), ("op", C.c_uint32), ("validity", Validity), ("offset", C.c_uint64)]


class WindowDst(C.Structure):
    """hmj_window_dst: one caller-owned output column -- n values of the function's output type, an optional bitmap of
    ceil(n / 64) 64-bit words (in); its NULL slots (out)."""
    _fields_ = [("data", C.c_void_p), ("validity", C.c_void_p), ("null_count", C.c_uint64)]


class WindowOpts(C.Structure):
    """hmj_window_opts: the number of PARTITION BY columns among the keys (in); partitions, peer groups, the longest
    partition's rows, the sort rounds of the internal ORDER BY and the phase times (out)."""
    _fields_ = [("struct_size", C.c_uint32), ("n_partition_cols", C.c_uint32), ("n_partitions", C.c_uint64),
                ("n_peer_groups", C.c_uint64), ("max_partition_rows", C.c_uint64), ("n_rounds", C.c_uint32),
                ("reserved", C.c_uint32), ("ms_order", C.c_float), ("ms_heads", C.c_float), ("ms_scan", C.c_float)]


__all__ = ["WindowFn", "WindowDst", "WindowOpts"]
