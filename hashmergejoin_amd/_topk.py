"""The struct mirror of hmj_top_k_device (include/hmj.h, "the first rows of an order"): hmj_top_k_opts.  The HMJ_TOPK_*
constants and the entry's signature are in _lib like every other entry's; `Executor.top_k_device` (join.py) fills it."""
import ctypes as C


class TopKOpts(C.Structure):
    """hmj_top_k_opts: the plan asked for, the rows skipped in front and the tie set a further level narrows (in); the
    entries written, the rows the final ordering sorted, the rows tied with the cut, the plan taken, the histogram levels,
    the sort rounds and the phase times (out)."""
    _fields_ = [("struct_size", C.c_uint32), ("plan", C.c_uint32), ("offset", C.c_uint64), ("max_tie_rows", C.c_uint64),
                ("n_out", C.c_uint64), ("n_candidates", C.c_uint64), ("n_tie_rows", C.c_uint64), ("plan_taken", C.c_uint32),
                ("n_levels", C.c_uint32), ("n_rounds", C.c_uint32), ("reserved", C.c_uint32), ("ms_select", C.c_float),
                ("ms_emit", C.c_float), ("ms_order", C.c_float)]


__all__ = ["TopKOpts"]
