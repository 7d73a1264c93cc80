"""The binding proper: `Executor`, one hmj_ctx (one per GPU / per process) with a method per entry of include/hmj.h, and
`HashMergeJoin`, the mirror of the reference's operator HashMergeJoin<RIter,SIter> (reference hashjoin.h:33-199):
construct from two relations, iterate (key, rval, sval) in ascending-key order, `clear()`.

The u64 entries (join_device, exchange_join, sort_device, the generators) call ctypes directly.  The column entries --
the string, multi-column and mixed-key joins, the groupings and their aggregates, ORDER BY, WHERE and the takes -- marshal
their arguments through `_marshal`.  `pack_strings` / `unpack_strings` / `pack_validity` / `unpack_validity` are the
input and output formats of those entries; the host restatements the tests compare them with live in `reference` and
are re-exported here.  torch is used only to hold device memory and to name the current stream.
"""
import ctypes as C

import numpy as np

from . import _lib
from . import _marshal as M
from ._lib import (HMJ_CHECKSUM, HMJ_FIRST_WINS, HMJ_MATERIALIZE, HMJ_ORDERED, HMJ_SUM_PROBE,  # noqa: F401
                   HmjError, JoinResult, Timing)
from ._marshal import _memcpy_d2d  # noqa: F401  (bench.py, tools/ and tests import it from here)
from ._topk import TopKOpts
from ._window import WindowDst, WindowFn, WindowOpts
from .reference import (cols_key64, expected_filter, expected_group_aggs, expected_groups,  # noqa: F401
                        expected_mixed_groups, expected_order_by, expected_top_k, expected_window, mixed_key64,
                        order_stream_bytes)

SEED_B = 0x243F6A8885A308D3


def plan(n_build):
    """(total_bits, [bits per LSD pass]) the executor will use for a build side of n_build rows."""
    L = _lib.load_library()
    tb, npass, pb = C.c_int(0), C.c_int(0), (C.c_int * 4)()
    rc = L.hmj_plan(n_build, C.byref(tb), C.byref(npass), C.byref(pb))
    if rc:
        raise HmjError(rc, "hmj_plan")
    return tb.value, [pb[i] for i in range(npass.value)]


def _dev_ptr(t):
    """(pointer, rows) of a CUDA/HIP torch tensor holding n x {key,val} as int64/uint64 [n,2]."""
    if t is None:
        return None, 0
    if not t.is_cuda:
        raise ValueError("expected a device tensor")
    if not t.is_contiguous() or t.element_size() != 8 or t.dim() != 2 or t.shape[1] != 2:
        raise ValueError("relation must be a contiguous [n,2] 64-bit tensor {key,val}")
    return t.data_ptr(), t.shape[0]


def _dev_ptrs(build, probe):
    """The (build, n_build, probe, n_probe) arguments of a u64 entry."""
    bp, nb = _dev_ptr(build)
    pp, np_ = _dev_ptr(probe)
    return C.c_void_p(bp), nb, C.c_void_p(pp), np_


def _valid_at(entry, at):
    """The optional (valid[, bit_offset]) tail of an aggregate or an ORDER BY column -> what `_marshal.validity` takes."""
    if len(entry) <= at or entry[at] is None:
        return None
    return entry[at], (entry[at + 1] if len(entry) > at + 1 else 0)


_KIND_COUNTERS = ("n_build_matched", "n_build_unmatched", "n_probe_matched", "n_probe_unmatched")
_JOIN_COLUMNS = ("key64", "r_row", "s_row", "rval", "sval")  # of hmj_cols_result; hmj_str_result: hash first


class Executor:
    """One hmj_ctx.  All methods raise HmjError on a nonzero status."""

    def __init__(self, device=None, use_torch_stream=True):
        import torch  # noqa: F401  (must be loaded before the HIP library, see _lib.load_library)

        self._torch = torch
        self.L = _lib.load_library()
        if device is None:
            device = torch.cuda.current_device()
        self.device = int(device)
        self._dev = torch.device("cuda", self.device)  # (what the column entries allocate on: no "cuda:N" to parse per call)
        h = C.c_void_p()
        rc = self.L.hmj_create(C.byref(h), self.device)
        if rc:
            raise HmjError(rc, self.L.hmj_strerror(rc).decode())
        self.h = h
        self.use_torch_stream = use_torch_stream
        self._keep = None

    def close(self):
        if getattr(self, "h", None):
            self.L.hmj_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc:
            raise HmjError(rc, "%s (%s)" % (self.L.hmj_strerror(rc).decode(), self.L.hmj_last_error(self.h).decode()))

    def _sync_stream(self):
        # run on torch's current stream so the join is ordered after whatever produced its inputs
        # (handle 0 = the HIP default stream, which hmj_set_stream takes as such)
        if self.use_torch_stream:
            s = self._torch.cuda.current_stream(self.device).cuda_stream
            self._check(self.L.hmj_set_stream(self.h, C.c_void_p(s)))

    def _rows(self, res, names, absent=None):
        """The device columns `names` of a join result -> an [n_matches, len(names)] uint64 array."""
        return M.read_columns(self._torch, self.device, [getattr(res, k) for k in names], int(res.n_matches), absent)

    # ---- configuration -----------------------------------------------------------------------
    def reserve(self, n_build, n_probe, max_matches=0, flags=0):
        self._check(self.L.hmj_reserve(self.h, n_build, n_probe, max_matches, flags))

    def set_radix_bits(self, bits):
        self._check(self.L.hmj_set_radix_bits(self.h, -1 if bits is None else bits))

    def set_key_prefix_bits(self, bits):
        """Top `bits` key bits are constant in both relations (consumed by an outer split); -1 = sample."""
        self._check(self.L.hmj_set_key_prefix_bits(self.h, bits))

    def set_profiling(self, on=True):
        self._check(self.L.hmj_set_profiling(self.h, int(bool(on))))

    def last_timing(self):
        t = Timing()
        self._check(self.L.hmj_last_timing(self.h, C.byref(t)))
        return t.as_dict()

    def last_plan(self):
        """hmj_last_plan: path, bits per pass, attempts, why faster formulations were refused, what the workload is
        skipping from now on (dict of hmj_plan_desc's fields)."""
        p = _lib.PlanDesc()
        p.struct_size = C.sizeof(_lib.PlanDesc)
        self._check(self.L.hmj_last_plan(self.h, C.byref(p)))
        return p.as_dict()

    def forget_workloads(self):
        self._check(self.L.hmj_forget_workloads(self.h))

    def placement_info(self):
        """One dict per big partition buffer this executor probed (hmj_placement_info; empty with HMJ_PLACE=0):
        name, bytes, fill rate of the allocation kept, candidates tried, whether a search ran (hmj_reserve or
        HMJ_PLACE=n) and was cut short by its budget, and per candidate the hipMalloc ms, fill ms and fill rate."""
        arr = (_lib.PlaceInfo * 16)()
        n = self.L.hmj_placement_info(self.h, arr, 16)
        out = []
        for i in range(n):
            e, k = arr[i], int(arr[i].candidates)
            out.append({"name": e.name.decode(), "bytes": int(e.bytes), "fill_TBps": round(float(e.fill_TBps), 3),
                        "candidates": k, "ms_search": round(float(e.ms_search), 2), "searched": bool(e.searched),
                        "aborted": bool(e.aborted), "budget_ms": round(float(e.budget_ms), 1),
                        "cand_ms_alloc": [round(float(x), 2) for x in e.cand_ms_alloc[:k]],
                        "cand_ms_fill": [round(float(x), 2) for x in e.cand_ms_fill[:k]],
                        "cand_TBps": [round(float(x), 3) for x in e.cand_TBps[:k]]})
        return out

    # ---- joins -------------------------------------------------------------------------------
    def join_device(self, build, probe, flags=0):
        """build/probe: device tensors [n,2] {key,val}.  Returns JoinResult (columns are device
        pointers owned by the executor; see `columns`)."""
        self._sync_stream()
        res = JoinResult()
        self._check(self.L.hmj_join_u64_device(self.h, *_dev_ptrs(build, probe), flags, C.byref(res)))
        return res

    def join_kind_device(self, build, probe, kind, flags=0, outer_fill=0):
        """Semi / anti / probe-side outer join (hmj_join_kind_u64_device; kind = HMJ_JOIN_*).  Returns (JoinResult,
        {"n_probe_matched": .., "n_probe_unmatched": ..}).  SEMI / ANTI results have no rval column: read them with
        `probe_rows_to_numpy`; PROBE_OUTER rows with `columns_to_numpy`.  HMJ_JOIN_INNER is join_device (counters 0)."""
        self._sync_stream()
        res = JoinResult()
        opts = M.new_opts(_lib.JoinOpts, kind=kind, outer_fill=outer_fill)
        self._check(self.L.hmj_join_kind_u64_device(self.h, *_dev_ptrs(build, probe), flags, C.byref(opts), C.byref(res)))
        return res, M.read_info(opts, _KIND_COUNTERS[2:])

    def probe_rows_to_numpy(self, res):
        """Copy a semi / anti join's device result out as an [n,2] uint64 array of (key, sval)."""
        return self._rows(res, ("key", "sval"))

    def join_build_kind_device(self, build, probe, kind, flags=0, build_fill=0, probe_fill=0):
        """Build-side semi / anti / outer join or the full outer join (hmj_join_build_kind_u64_device; kind = HMJ_BUILD_SEMI,
        HMJ_BUILD_ANTI, HMJ_BUILD_OUTER or HMJ_FULL_OUTER).  Returns (JoinResult, {"n_build_matched", "n_build_unmatched",
        "n_probe_matched", "n_probe_unmatched"}).  BUILD_SEMI / BUILD_ANTI results have no sval column: read them with
        `build_rows_to_numpy`; the outer kinds' rows with `columns_to_numpy`."""
        self._sync_stream()
        res = JoinResult()
        opts = M.new_opts(_lib.BuildJoinOpts, kind=kind, build_fill=build_fill, probe_fill=probe_fill)
        self._check(self.L.hmj_join_build_kind_u64_device(self.h, *_dev_ptrs(build, probe), flags, C.byref(opts),
                                                          C.byref(res)))
        return res, M.read_info(opts, _KIND_COUNTERS)

    def build_rows_to_numpy(self, res):
        """Copy a build semi / anti join's device result out as an [n,2] uint64 array of (key, rval)."""
        return self._rows(res, ("key", "rval"))

    # ---- string keys (hmj_hash_str_device / hmj_join_str_device) ------------------------------------
    def _str_rel(self, rel):
        """(chars uint8, offsets int64 [n + 1], vals int64 [n]) device tensors -> StrRel (chars may be None or empty when
        every key is empty)."""
        chars, offsets, vals = rel
        M.check_col64(offsets, "offsets")
        M.check_col64(vals, "vals")
        n = vals.shape[0]
        if offsets.shape[0] != n + 1:
            raise ValueError("offsets must hold n + 1 entries")
        r = _lib.StrRel()
        r.chars = M.chars_ptr(chars)
        r.offsets = offsets.data_ptr() if n else None
        r.vals = vals.data_ptr() if n else None
        r.n = n
        return r

    def hash_str_device(self, chars, offsets, hash_bits=0):
        """std::hash<std::string> of every key (libstdc++'s _Hash_bytes), computed on the device: int64 tensor [n]
        (read as uint64).  hash_bits 1..63 keeps the top bits only (h >> (64 - hash_bits))."""
        torch = self._torch
        M.check_col64(offsets, "offsets")
        if offsets.shape[0] < 1:
            raise ValueError("offsets must hold n + 1 entries")
        self._sync_stream()
        n = offsets.shape[0] - 1
        out = torch.empty(n, dtype=torch.int64, device=offsets.device)
        self._check(self.L.hmj_hash_str_device(self.h, M.chars_ptr(chars), C.c_void_p(offsets.data_ptr()), max(n, 0),
                                               int(hash_bits), C.c_void_p(out.data_ptr()) if n > 0 else None))
        return out

    def join_str_device(self, build, probe, flags=0, hash_bits=0, build_valid=None, probe_valid=None):
        """Inner join of two string-keyed device relations (hmj_join_str_device).  build / probe: (chars uint8, offsets
        int64 [n + 1], vals int64 [n]) device tensors -- the Arrow large_string layout plus payloads (`pack_strings`).
        *_valid: None, a uint8 device tensor holding the key column's Arrow validity bitmap (`pack_validity`), or (tensor,
        bit_offset); a row whose key is NULL matches nothing, and a valid empty string is not NULL.  hmj_str_join_opts
        carries no bitmap, so a call with *_valid runs the INNER kind of hmj_join_kind_str_device, which is the same join.
        Returns (StrResult, {"n_hash_pairs", "n_collisions", "n_build_null", "n_probe_null", "ms_hash", "ms_join",
        "ms_verify", "ms_order"}); read the rows with `str_rows_to_numpy`."""
        if build_valid is not None or probe_valid is not None:
            res, info = self.join_kind_str_device(build, probe, _lib.HMJ_KIND_PROBE_SIDE, _lib.HMJ_JOIN_INNER, flags, hash_bits,
                                                  build_valid=build_valid, probe_valid=probe_valid)
            keys = ("n_hash_pairs", "n_collisions", "n_build_null", "n_probe_null", "ms_hash", "ms_join", "ms_verify", "ms_order")
            return res, {k: info[k] for k in keys}
        self._sync_stream()
        rb, rp = self._str_rel(build), self._str_rel(probe)
        opts = M.new_opts(_lib.StrJoinOpts, hash_bits=hash_bits)
        res = _lib.StrResult()
        self._check(self.L.hmj_join_str_device(self.h, C.byref(rb), C.byref(rp), flags, C.byref(opts), C.byref(res)))
        return res, M.read_info(opts, ("n_hash_pairs", "n_collisions"), ("ms_hash", "ms_join", "ms_verify", "ms_order"),
                                between={"n_build_null": 0, "n_probe_null": 0})

    def str_rows_to_numpy(self, res):
        """Copy a string join's device result out as an [n,5] uint64 array of (hash, r_row, s_row, rval, sval)."""
        return self._rows(res, ("hash",) + _JOIN_COLUMNS[1:])

    def join_kind_str_device(self, build, probe, side, kind, flags=0, hash_bits=0, probe_fill=0, build_fill=0, build_valid=None,
                             probe_valid=None):
        """Semi / anti / outer joins of two string-keyed device relations (hmj_join_kind_str_device).  side / kind as for
        hmj_exchange_kind_opts: HMJ_KIND_PROBE_SIDE with HMJ_JOIN_*, or HMJ_KIND_BUILD_SIDE with HMJ_BUILD_* / HMJ_FULL_OUTER;
        build / probe and *_valid as for `join_str_device` (a NULL-key row has no partner: ANTI and the outer kinds of its
        side emit it with hash 0).  Returns (StrResult, {"n_probe_matched", "n_probe_unmatched", "n_build_matched",
        "n_build_unmatched", "n_hash_pairs", "n_collisions", "n_build_null", "n_probe_null", "ms_hash", "ms_join",
        "ms_verify", "ms_emit", "ms_order"}); read the rows with `str_kind_rows_to_numpy`."""
        self._sync_stream()
        rb, rp = self._str_rel(build), self._str_rel(probe)
        opts = M.new_opts(_lib.StrKindOpts, side=side, kind=kind, hash_bits=hash_bits, probe_fill=probe_fill, build_fill=build_fill)
        keep = (M.validity(opts.build_validity, build_valid, int(rb.n), "build_valid", empty_is_absent=True),
                M.validity(opts.probe_validity, probe_valid, int(rp.n), "probe_valid", empty_is_absent=True))
        res = _lib.StrResult()
        self._check(self.L.hmj_join_kind_str_device(self.h, C.byref(rb), C.byref(rp), flags, C.byref(opts), C.byref(res)))
        del keep
        return res, M.read_info(opts, ("n_hash_pairs", "n_collisions", "n_build_null", "n_probe_null"),
                                ("ms_hash", "ms_join", "ms_verify", "ms_emit", "ms_order"))

    def str_kind_rows_to_numpy(self, res):
        """Copy a string kind join's device result out as an [n,5] uint64 array of (hash, r_row, s_row, rval, sval); a
        column the kind does not produce reads as HMJ_STR_NO_ROW (row columns) or 0 (value columns)."""
        return self._rows(res, ("hash",) + _JOIN_COLUMNS[1:], absent=(0, _lib.HMJ_STR_NO_ROW, _lib.HMJ_STR_NO_ROW, 0, 0))

    # ---- multi-column fixed-width keys (hmj_join_cols_device) ------------------------------------------
    def _cols_rel(self, cols, vals):
        """Key columns (1-D contiguous device tensors of one length, any dtype) + payloads (int64 [n] or None) -> (ColsRel,
        the KeyCol array it points to: keep it alive for the call).  Widths, alignment and column counts are checked by
        the library."""
        cols = list(cols)
        for k, t in enumerate(cols):
            M.check_column(t, "key column %d must be a contiguous 1-D device tensor", k)
        n = cols[0].shape[0] if cols else (vals.shape[0] if vals is not None else 0)
        if any(t.shape[0] != n for t in cols):
            raise ValueError("key columns must have one length")
        if vals is not None:
            M.check_col64(vals, "vals")
            if vals.shape[0] != n:
                raise ValueError("vals must hold one payload per row")
        arr = (_lib.KeyCol * max(len(cols), 1))()
        for k, t in enumerate(cols):
            arr[k].data = t.data_ptr() if n else None
            arr[k].width = t.element_size()
        r = _lib.ColsRel()
        r.cols = arr
        r.n_cols = len(cols)
        r.vals = vals.data_ptr() if (vals is not None and n) else None
        r.n = n
        return r, arr

    def _validity(self, valid, rel, name):
        """A relation's validity bitmaps -> the Validity array hmj_cols_*_opts point to (None: no bitmap on this side) and
        what keeps it and its tensors alive for the call.  valid: None, or one entry per key column: None, a uint8 device
        tensor (an Arrow bitmap, LSB first), or (tensor, bit_offset)."""
        if valid is None:
            return None, None
        valid = list(valid)
        if len(valid) != rel.n_cols:
            raise ValueError("%s: one entry per key column" % name)
        arr = (_lib.Validity * max(len(valid), 1))()
        return arr, [arr] + [M.validity(arr[k], v, int(rel.n), "%s[%d]", name, k) for k, v in enumerate(valid)]

    def join_cols_device(self, build_cols, build_vals, probe_cols, probe_vals, flags=0, hash_bits=0, force_hashed=False,
                         build_valid=None, probe_valid=None):
        """Inner join of two device relations on a key of several fixed-width columns (hmj_join_cols_device).  *_cols:
        lists of 1-D contiguous device tensors of any dtype whose element_size() is 1, 2, 4 or 8 (compared bit for bit);
        *_vals: an int64 tensor [n], or None (the payload of row i is i).  *_valid: None, or a list with one entry per key
        column -- None, a uint8 device tensor holding the column's Arrow validity bitmap (`pack_validity`), or (tensor,
        bit_offset); a row with a NULL in any key column matches nothing.  hmj_cols_join_opts carries no bitmaps, so a call
        with *_valid runs the INNER kind of hmj_join_kind_cols_device, which is the same join (its "form" is filled for
        empty sides too).  Returns (ColsResult, {"form", "n_key_pairs", "n_collisions", "n_build_null", "n_probe_null",
        "ms_key", "ms_join", "ms_verify", "ms_order"}); read the rows with `cols_rows_to_numpy`, reproduce key64 with
        `cols_key64`."""
        if build_valid is not None or probe_valid is not None:
            res, info = self.join_kind_cols_device(build_cols, build_vals, probe_cols, probe_vals, _lib.HMJ_KIND_PROBE_SIDE,
                                                   _lib.HMJ_JOIN_INNER, flags, hash_bits, force_hashed, build_valid=build_valid,
                                                   probe_valid=probe_valid)
            keys = ("form", "n_key_pairs", "n_collisions", "n_build_null", "n_probe_null", "ms_key", "ms_join", "ms_verify", "ms_order")
            return res, {k: info[k] for k in keys}
        self._sync_stream()
        rb, keep_b = self._cols_rel(build_cols, build_vals)
        rp, keep_p = self._cols_rel(probe_cols, probe_vals)
        opts = M.new_opts(_lib.ColsJoinOpts, hash_bits=hash_bits, force_hashed=bool(force_hashed))
        res = _lib.ColsResult()
        self._check(self.L.hmj_join_cols_device(self.h, C.byref(rb), C.byref(rp), flags, C.byref(opts), C.byref(res)))
        del keep_b, keep_p
        return res, M.read_info(opts, ("form", "n_key_pairs", "n_collisions"), ("ms_key", "ms_join", "ms_verify", "ms_order"),
                                between={"n_build_null": 0, "n_probe_null": 0})

    def cols_rows_to_numpy(self, res):
        """Copy a multi-column join's device result out as an [n,5] uint64 array of (key64, r_row, s_row, rval, sval)."""
        return self._rows(res, _JOIN_COLUMNS)

    def join_kind_cols_device(self, build_cols, build_vals, probe_cols, probe_vals, side, kind, flags=0, hash_bits=0,
                              force_hashed=False, probe_fill=0, build_fill=0, build_valid=None, probe_valid=None):
        """Semi / anti / outer joins of two device relations on a key of several fixed-width columns
        (hmj_join_kind_cols_device).  side / kind as for `join_kind_str_device`: HMJ_KIND_PROBE_SIDE with HMJ_JOIN_*, or
        HMJ_KIND_BUILD_SIDE with HMJ_BUILD_* / HMJ_FULL_OUTER; relations and *_valid as for `join_cols_device` (a NULL-key
        row has no partner: ANTI and the outer kinds of its side emit it with key64 0).  flags | HMJ_NULL_EQUAL with a bitmap
        on either side: NULL slots match NULL slots of the same column, a row with NULL slots is an ordinary row of every
        kind, the key is hashed and `cols_key64(..., valid=, null_equal=True)` reproduces it.  Returns (ColsResult,
        {"n_probe_matched", "n_probe_unmatched", "n_build_matched", "n_build_unmatched", "form", "n_key_pairs",
        "n_collisions", "n_build_null", "n_probe_null", "ms_key", "ms_join", "ms_verify", "ms_emit", "ms_order"}); read
        the rows with `cols_kind_rows_to_numpy`."""
        self._sync_stream()
        rb, keep_b = self._cols_rel(build_cols, build_vals)
        rp, keep_p = self._cols_rel(probe_cols, probe_vals)
        opts = M.new_opts(_lib.ColsKindOpts, side=side, kind=kind, hash_bits=hash_bits, force_hashed=bool(force_hashed),
                          probe_fill=probe_fill, build_fill=build_fill)
        vb, keep_vb = self._validity(build_valid, rb, "build_valid")
        vp, keep_vp = self._validity(probe_valid, rp, "probe_valid")
        if vb is not None:
            opts.build_validity = vb
        if vp is not None:
            opts.probe_validity = vp
        res = _lib.ColsResult()
        self._check(self.L.hmj_join_kind_cols_device(self.h, C.byref(rb), C.byref(rp), flags, C.byref(opts), C.byref(res)))
        del keep_b, keep_p, keep_vb, keep_vp
        return res, M.read_info(opts, ("form", "n_key_pairs", "n_collisions", "n_build_null", "n_probe_null"),
                                ("ms_key", "ms_join", "ms_verify", "ms_emit", "ms_order"))

    def cols_kind_rows_to_numpy(self, res):
        """Copy a multi-column kind join's device result out as an [n,5] uint64 array of (key64, r_row, s_row, rval, sval);
        a column the kind does not produce (r_row / rval of probe SEMI / ANTI, s_row / sval of BUILD_SEMI / BUILD_ANTI)
        reads as 0."""
        return self._rows(res, _JOIN_COLUMNS, absent=0)

    # ---- grouping rows by multi-column keys (hmj_group_cols_device) ----------------------------------------
    def group_cols_device(self, cols, vals=None, valid=None, flags=0, want=_lib.HMJ_GROUP_COUNT, hash_bits=0, force_hashed=False):
        """Group the rows of one device relation by a key of several fixed-width columns (hmj_group_cols_device): GROUP BY /
        DISTINCT with NULLs of a column forming one group.  cols, vals and valid as `join_cols_device` takes one side's.
        flags: 0 (counts only: n_groups, max_count), HMJ_MATERIALIZE (key64 and first_row, + what `want` asks for) or
        HMJ_ORDERED (groups ascending by key64, then tuple, NULLS LAST).  want: HMJ_GROUP_* bits.  Returns (GroupResult,
        {"form", "n_null", "n_collisions", "ms_key", "ms_sort", "ms_groups", "ms_agg"}); read the columns with
        `group_rows_to_numpy`, reproduce them with `expected_groups`."""
        self._sync_stream()
        rel, keep = self._cols_rel(cols, vals)
        opts = M.new_opts(_lib.GroupOpts, want=want, hash_bits=hash_bits, force_hashed=bool(force_hashed))
        v, keep_v = self._validity(valid, rel, "valid")
        if v is not None:
            opts.validity = v
        res = _lib.GroupResult()
        self._group_rows = self._group_groups = 0  # (group_agg_device: the library drops its live grouping here)
        self._check(self.L.hmj_group_cols_device(self.h, C.byref(rel), flags, C.byref(opts), C.byref(res)))
        if flags & (HMJ_MATERIALIZE | HMJ_ORDERED):
            self._group_rows, self._group_groups = int(res.n_rows), int(res.n_groups)
        del keep, keep_v
        return res, M.read_info(opts, ("form", "n_null", "n_collisions"), ("ms_key", "ms_sort", "ms_groups", "ms_agg"))

    def group_rows_to_numpy(self, res):
        """Copy a grouping's device result out: {"key64", "first_row", "count", "sum", "min", "max", "group_of_row"} -> a
        uint64 array (n_groups entries; group_of_row: n_rows), or None for a column the call did not produce."""
        out = {}
        for name in ("key64", "first_row", "count", "sum", "min", "max", "group_of_row"):
            ptr = getattr(res, name)
            n = int(res.n_rows if name == "group_of_row" else res.n_groups)
            out[name] = M.read_columns(self._torch, self.device, (ptr,), n)[:, 0] if ptr else None
        return out

    # ---- mixed keys: string and fixed-width columns in one tuple (hmj_join_mixed_device) ------------------
    def _mixed_rel(self, cols, vals, valid, name):
        """Key columns -- a 1-D contiguous device tensor (fixed-width) or a (chars uint8, offsets int64 [n + 1]) pair (an Arrow
        large_string column; chars may be None or empty when every slot is empty) --, payloads (int64 [n] or None) and the
        per-column validity list -> (MixedRel, what must stay alive for the call).  Types, widths, alignment and column
        counts are checked by the library."""
        cols = list(cols)
        n = None
        for k, col in enumerate(cols):
            if isinstance(col, (tuple, list)):
                M.check_col64(col[1], "%s column %d: offsets", name, k)
                if col[1].shape[0] < 1:
                    raise ValueError("%s column %d: offsets must hold n + 1 entries" % (name, k))
                m = col[1].shape[0] - 1
            else:
                M.check_column(col, "%s column %d must be a contiguous 1-D device tensor", name, k)
                m = col.shape[0]
            if n is None:
                n = m
            if m != n:
                raise ValueError("%s: key columns must have one length" % name)
        if n is None:
            n = vals.shape[0] if vals is not None else 0
        if vals is not None:
            M.check_col64(vals, "vals")
            if vals.shape[0] != n:
                raise ValueError("vals must hold one payload per row")
        valid = [None] * len(cols) if valid is None else list(valid)
        if len(valid) != len(cols):
            raise ValueError("%s_valid: one entry per key column" % name)
        arr = (_lib.MixedCol * max(len(cols), 1))()
        keep = [arr, cols]
        for k, col in enumerate(cols):
            if isinstance(col, (tuple, list)):
                arr[k].type = _lib.HMJ_KEY_LARGE_STRING
                arr[k].width = 0
                arr[k].data = M.chars_ptr(col[0])
                arr[k].offsets = col[1].data_ptr()
            else:
                arr[k].type = _lib.HMJ_KEY_FIXED
                arr[k].width = col.element_size()
                arr[k].data = col.data_ptr() if n else None
            keep.append(M.validity(arr[k].validity, valid[k], n, "%s_valid[%d]", name, k, empty_is_absent=True))
        r = _lib.MixedRel()
        r.cols = arr
        r.n_cols = len(cols)
        r.vals = vals.data_ptr() if (vals is not None and n) else None
        r.n = n
        return r, keep

    def join_mixed_device(self, build_cols, build_vals, probe_cols, probe_vals, side, kind, flags=0, hash_bits=0, probe_fill=0,
                          build_fill=0, build_valid=None, probe_valid=None):
        """Inner / semi / anti / outer joins of two device relations on a key tuple of string and fixed-width columns
        (hmj_join_mixed_device).  *_cols: one entry per key column -- a 1-D contiguous device tensor whose element_size() is
        1, 2, 4 or 8 (compared bit for bit), or a (chars uint8, offsets int64 [n + 1]) pair, the Arrow large_string layout
        (`pack_strings`; compared byte for byte); *_vals: an int64 tensor [n], or None (the payload of row i is i).  side /
        kind as for `join_kind_cols_device`, HMJ_KIND_PROBE_SIDE + HMJ_JOIN_INNER included.  *_valid: None, or a list with
        one entry per key column -- None, a uint8 device tensor holding the column's Arrow validity bitmap
        (`pack_validity`), or (tensor, bit_offset); a row with a NULL in any key column has no partner -- unless flags holds
        HMJ_NULL_EQUAL: then NULL slots match NULL slots of the same column (a NULL string is not the empty string) and
        `mixed_key64(..., valid=, null_equal=True)` reproduces key64.  Returns (ColsResult,
        {"n_probe_matched", "n_probe_unmatched", "n_build_matched", "n_build_unmatched", "n_key_pairs", "n_collisions",
        "n_build_null", "n_probe_null", "ms_key", "ms_join", "ms_verify", "ms_emit", "ms_order"}); read the rows with
        `mixed_rows_to_numpy`, reproduce key64 with `mixed_key64`."""
        self._sync_stream()
        rb, keep_b = self._mixed_rel(build_cols, build_vals, build_valid, "build")
        rp, keep_p = self._mixed_rel(probe_cols, probe_vals, probe_valid, "probe")
        opts = M.new_opts(_lib.MixedOpts, side=side, kind=kind, hash_bits=hash_bits, probe_fill=probe_fill, build_fill=build_fill)
        res = _lib.ColsResult()
        self._check(self.L.hmj_join_mixed_device(self.h, C.byref(rb), C.byref(rp), flags, C.byref(opts), C.byref(res)))
        del keep_b, keep_p
        return res, M.read_info(opts, ("n_key_pairs", "n_collisions", "n_build_null", "n_probe_null"),
                                ("ms_key", "ms_join", "ms_verify", "ms_emit", "ms_order"))

    def mixed_rows_to_numpy(self, res):
        """Copy a mixed-key join's device result out as an [n,5] uint64 array of (key64, r_row, s_row, rval, sval); a column
        the kind does not produce (r_row / rval of probe SEMI / ANTI, s_row / sval of BUILD_SEMI / BUILD_ANTI) reads as 0."""
        return self.cols_kind_rows_to_numpy(res)

    # ---- grouping rows by string and mixed keys (hmj_group_mixed_device) ----------------------------------
    def group_mixed_device(self, cols, vals=None, valid=None, flags=0, want=_lib.HMJ_GROUP_COUNT, hash_bits=0):
        """Group the rows of one device relation by a key tuple of string and fixed-width columns (hmj_group_mixed_device):
        GROUP BY / DISTINCT with NULLs of a column forming one group, a NULL string not being the empty string.  cols, vals
        and valid as `join_mixed_device` takes one side's; flags and want as for `group_cols_device`.  The key is always
        hashed.  Returns (GroupResult, {"form", "n_null", "n_collisions", "ms_key", "ms_sort", "ms_groups", "ms_agg"}); read
        the columns with `group_rows_to_numpy`, reproduce them with `expected_mixed_groups`."""
        self._sync_stream()
        rel, keep = self._mixed_rel(cols, vals, valid, "grouped")
        opts = M.new_opts(_lib.GroupOpts, want=want, hash_bits=hash_bits)
        res = _lib.GroupResult()
        self._group_rows = self._group_groups = 0  # (group_agg_device: the library drops its live grouping here)
        self._check(self.L.hmj_group_mixed_device(self.h, C.byref(rel), flags, C.byref(opts), C.byref(res)))
        if flags & (HMJ_MATERIALIZE | HMJ_ORDERED):
            self._group_rows, self._group_groups = int(res.n_rows), int(res.n_groups)
        del keep
        return res, M.read_info(opts, ("form", "n_null", "n_collisions"), ("ms_key", "ms_sort", "ms_groups", "ms_agg"))

    # ---- typed columns aggregated over the live grouping (hmj_group_agg_device) ----------------------------
    def _agg_type(self, t):
        return M.type_code(t.dtype)

    def group_agg_device(self, aggs, want_validity=True, n_rows=None):
        """Aggregate typed value columns over the executor's live grouping (hmj_group_agg_device): the last successful
        `group_cols_device` / `group_mixed_device` call made with HMJ_MATERIALIZE or HMJ_ORDERED; slot g of every output is
        group g of that call's columns.  aggs: a list of (op, column, valid[, bit_offset]) -- op an HMJ_AGG_* code; column a
        contiguous 1-D device tensor of an integer or float dtype of 1 to 8 bytes (the HMJ_TYPE_* is inferred), or None
        for HMJ_AGG_COUNT; valid None or a contiguous 1-D device tensor holding the column's Arrow bitmap (uint8 bytes as
        `pack_validity` makes them, or 64-bit words), row i at bit bit_offset + i.  want_validity: True, False, or one bool
        per aggregate.  n_rows: the grouped relation's rows (default: the first column's length, or the rows of the last
        group call made through this executor).  The outputs are new tensors: COUNT uint64, SUM int64 / uint64 / float64,
        MIN / MAX the source dtype, MEAN float64.  Returns ([(values, validity words or None, null_count), ...],
        {"n_groups", "ms_agg"}); `unpack_validity` reads the words, `expected_group_aggs` reproduces everything."""
        torch = self._torch
        self._sync_stream()
        aggs = [tuple(a) for a in aggs]
        wants = M.want_flags(want_validity, len(aggs), "aggregate")
        if n_rows is None:
            lens = [a[1].shape[0] for a in aggs if a[1] is not None]
            n_rows = lens[0] if lens else getattr(self, "_group_rows", 0)
        n_rows = int(n_rows)
        # the groups size the outputs: an HMJ_E_ARG call must still reach the library, so any count will do for it
        n_groups = int(getattr(self, "_group_groups", 0))
        dev = self._dev
        src = (_lib.AggSrc * max(len(aggs), 1))()
        dst = (_lib.AggDst * max(len(aggs), 1))()
        outs, words, keep = [], [], []
        f64, i64 = torch.float64, torch.int64
        u64 = getattr(torch, "uint64", i64)
        for k, a in enumerate(aggs):
            op, t = int(a[0]), a[1]
            code = _lib.HMJ_TYPE_U64
            if t is not None:
                M.check_column(t, "aggregate %d: the column must be a contiguous 1-D device tensor", k)
                code = M.type_code(t.dtype)
                src[k].data = t.data_ptr() if t.shape[0] else None
                keep.append(t)
            src[k].type = code
            src[k].op = op & 0xFFFFFFFF
            keep.append(M.validity(src[k].validity, _valid_at(a, 2), n_rows, "aggregate %d", k, any_width=True))
            if op == _lib.HMJ_AGG_COUNT:
                dt = u64
            elif op == _lib.HMJ_AGG_MEAN:
                dt = f64
            elif op == _lib.HMJ_AGG_SUM:
                dt = f64 if code >= _lib.HMJ_TYPE_F32 else (i64 if code <= _lib.HMJ_TYPE_I64 else u64)
            else:
                dt = t.dtype if t is not None else u64
            o = torch.empty(n_groups, dtype=dt, device=dev)
            w = torch.empty((n_groups + 63) // 64, dtype=i64, device=dev) if wants[k] else None
            dst[k].data = o.data_ptr() if n_groups else None
            dst[k].validity = w.data_ptr() if (w is not None and n_groups) else None
            outs.append(o)
            words.append(w)
        opts = M.new_opts(_lib.GroupAggOpts)
        self._check(self.L.hmj_group_agg_device(self.h, src, len(aggs), n_rows, dst, C.byref(opts)))
        del keep
        if int(opts.n_groups) != n_groups:
            raise RuntimeError("the live grouping has %d groups, the executor sized the outputs for %d: group through this "
                               "executor's group_cols_device / group_mixed_device" % (int(opts.n_groups), n_groups))
        return ([(outs[k], words[k], int(dst[k].null_count)) for k in range(len(aggs))],
                M.read_info(opts, ("n_groups",), ("ms_agg",)))

    # ---- ORDER BY: typed, string and mixed keys to a row map (hmj_order_by_device) ---------------------------
    def _order_cols(self, cols, n):
        """The key columns of `order_by_device` and `window_device` -> (the hmj_order_col array, its entries, n, what must stay alive)."""
        cols = [tuple(c) for c in cols]
        if n is None and cols:
            first = cols[0][0]
            n = first[1].shape[0] - 1 if isinstance(first, (tuple, list)) else first.shape[0]
        n = int(n or 0)
        arr = (_lib.OrderCol * max(len(cols), 1))()
        keep = []
        for k, c in enumerate(cols):
            col, flags = c[0], int(c[1]) if len(c) > 1 else 0
            if isinstance(col, (tuple, list)):
                M.check_col64(col[1], "column %d: offsets", k)  # (an offsets tensor without entries is the library's to refuse)
                arr[k].type = _lib.HMJ_ORDER_LARGE_STRING
                arr[k].data = M.chars_ptr(col[0])
                arr[k].offsets = col[1].data_ptr()
                keep += [col[0], col[1]]
            else:
                M.check_column(col, "column %d must be a contiguous 1-D device tensor", k)
                arr[k].type = M.type_code(col.dtype)
                arr[k].data = col.data_ptr() if col.shape[0] else None
                keep.append(col)
            arr[k].flags = flags & 0xFFFFFFFF
            keep.append(M.validity(arr[k].validity, _valid_at(c, 2), n, "column %d", k, any_width=True))
        return arr, len(cols), n, keep

    def order_by_device(self, cols, n=None):
        """A stable multi-column ORDER BY (hmj_order_by_device).  cols: a list of (column, flags[, valid[, bit_offset]]) --
        column a contiguous 1-D device tensor of an integer or float dtype of 1 to 8 bytes (the HMJ_TYPE_* is inferred), or a
        (chars, offsets) pair as `pack_strings` makes it (an Arrow large_string column: chars uint8 or None, offsets int64
        [n + 1]); flags HMJ_ORDER_DESC | HMJ_ORDER_NULLS_FIRST bits; valid None or a contiguous 1-D device tensor holding the
        column's Arrow bitmap (`pack_validity`), row i at bit bit_offset + i.  n: the rows (default: the first column's).
        Returns (row map: a new int64 device tensor of n entries, map[j] = the row at sorted position j, {"n_distinct",
        "n_tied_rows", "n_rounds", "ms_key", "ms_sort", "ms_refine", "ms_map"}); `expected_order_by` reproduces the map, and
        `take_cols_device` / `take_str_device` consume it."""
        torch = self._torch
        self._sync_stream()
        arr, n_cols, n, keep = self._order_cols(cols, n)
        out = torch.empty(n, dtype=torch.int64, device=self._dev)
        opts = M.new_opts(_lib.OrderOpts)
        self._check(self.L.hmj_order_by_device(self.h, arr, n_cols, n, out.data_ptr() if n else None, C.byref(opts)))
        del keep
        return out, M.read_info(opts, ("n_distinct", "n_tied_rows", "n_rounds"), ("ms_key", "ms_sort", "ms_refine", "ms_map"))

    # ---- ORDER BY ... LIMIT k [OFFSET o] (hmj_top_k_device) ----------------------------------------------------
    _TOPK_PLANS = {"auto": _lib.HMJ_TOPK_AUTO, "select": _lib.HMJ_TOPK_SELECT, "full": _lib.HMJ_TOPK_FULL}

    def top_k_device(self, cols, k, offset=0, n=None, plan="auto", max_tie_rows=0):
        """Entries offset .. offset + k of `order_by_device(cols)`'s map without sorting the rows the cut rejects
        (hmj_top_k_device).  cols and n as `order_by_device` takes them; k and offset are any integers in 0 .. 2^64 - 1 (the
        sum saturates); plan "auto", "select" (radix selection, then the candidates are ordered) or "full" (the whole ORDER
        BY, then the slice), or an HMJ_TOPK_* code; max_tie_rows: a set of rows tied with the cut that is larger is narrowed by
        a further level (0: the library's default).  Returns (row map: a new int64 device tensor of n_out = min(k, n - min(n,
        offset)) entries, {"n_out", "n_candidates", "n_tie_rows", "plan_taken", "n_levels", "n_rounds", "ms_select",
        "ms_emit", "ms_order"}); `expected_top_k` reproduces the map."""
        torch = self._torch
        self._sync_stream()
        arr, n_cols, n, keep = self._order_cols(cols, n)
        k, offset = int(k), int(offset)
        if not (0 <= k <= M.U64_MASK and 0 <= offset <= M.U64_MASK):
            raise ValueError("k and offset must be in 0 .. 2^64 - 1")
        lo = min(offset, n)
        n_out = min(k, n - lo)
        out = torch.empty(n_out, dtype=torch.int64, device=self._dev)
        opts = M.new_opts(TopKOpts, plan=self._TOPK_PLANS.get(plan, plan), offset=offset, max_tie_rows=max_tie_rows)
        self._check(self.L.hmj_top_k_device(self.h, arr, n_cols, n, k, out.data_ptr() if n_out else None, C.byref(opts)))
        del keep
        if int(opts.n_out) != n_out:
            raise RuntimeError("hmj_top_k_device wrote %d entries, the executor sized the map for %d" % (int(opts.n_out), n_out))
        return out, M.read_info(opts, ("n_out", "n_candidates", "n_tie_rows", "plan_taken", "n_levels", "n_rounds"),
                                ("ms_select", "ms_emit", "ms_order"))

    # ---- OVER: window functions over ordered partitions (hmj_window_device) -----------------------------------
    def window_device(self, keys, n_partition_cols, fns, n=None, want_validity=True):
        """Window functions over ordered partitions (hmj_window_device).  keys: as `order_by_device` takes its columns (may be
        empty: one partition in row order); the first n_partition_cols of them are PARTITION BY, the rest ORDER BY.  fns: a
        list of (op, column_or_None, valid=None, bit_offset=0, offset=0) -- op an HMJ_WIN_* code; column a contiguous 1-D
        device tensor of an integer or float dtype of 1 to 8 bytes (the HMJ_TYPE_* is inferred), None where the op reads no
        value; valid None or the column's Arrow bitmap on the device (uint8 bytes or 64-bit words), row i at bit bit_offset
        + i; offset the rows HMJ_WIN_LAG / HMJ_WIN_LEAD look away.  n: the rows (default: the first key column's, else the
        first function column's).  want_validity: True, False, or one bool per function.  The outputs are new tensors in
        SORTED order -- slot j belongs to row row_map[j] --: uint64 for the ranking functions and CUM_COUNT, int64 / uint64 /
        float64 for CUM_SUM, the source dtype otherwise.  Returns (row_map, [(values, validity words or None, null_count),
        ...], {"n_partitions", "n_peer_groups", "max_partition_rows", "n_rounds", "ms_order", "ms_heads", "ms_scan"});
        `expected_window` reproduces everything."""
        torch = self._torch
        self._sync_stream()
        fns = [tuple(f) for f in fns]
        wants = M.want_flags(want_validity, len(fns), "function")
        if n is None and not keys:
            lens = [f[1].shape[0] for f in fns if len(f) > 1 and f[1] is not None]
            n = lens[0] if lens else 0
        arr, n_keys, n, keep = self._order_cols(keys, n)
        dev = self._dev
        src = (WindowFn * max(len(fns), 1))()
        dst = (WindowDst * max(len(fns), 1))()
        outs, words = [], []
        f64, i64 = torch.float64, torch.int64
        u64 = getattr(torch, "uint64", i64)
        for k, f in enumerate(fns):
            op, t = int(f[0]), f[1] if len(f) > 1 else None
            code = _lib.HMJ_TYPE_U64
            if t is not None:
                M.check_column(t, "function %d: the column must be a contiguous 1-D device tensor", k)
                code = M.type_code(t.dtype)
                src[k].data = t.data_ptr() if t.shape[0] else None
                keep.append(t)
            src[k].type = code
            src[k].op = op & 0xFFFFFFFF
            src[k].offset = (int(f[4]) if len(f) > 4 else 0) & M.U64_MASK
            keep.append(M.validity(src[k].validity, _valid_at(f, 2), n, "function %d", k, any_width=True))
            if op == _lib.HMJ_WIN_CUM_SUM:
                dt = f64 if code >= _lib.HMJ_TYPE_F32 else (i64 if code <= _lib.HMJ_TYPE_I64 else u64)
            elif op in (_lib.HMJ_WIN_CUM_MIN, _lib.HMJ_WIN_CUM_MAX, _lib.HMJ_WIN_LAG, _lib.HMJ_WIN_LEAD) and t is not None:
                dt = t.dtype
            else:
                dt = u64
            o = torch.empty(n, dtype=dt, device=dev)
            w = torch.empty((n + 63) // 64, dtype=i64, device=dev) if wants[k] else None
            dst[k].data = o.data_ptr() if n else None
            dst[k].validity = w.data_ptr() if (w is not None and n) else None
            outs.append(o)
            words.append(w)
        row_map = torch.empty(n, dtype=i64, device=dev)
        opts = M.new_opts(WindowOpts, n_partition_cols=n_partition_cols)
        self._check(self.L.hmj_window_device(self.h, arr, n_keys, n, src, len(fns), dst,
                                             row_map.data_ptr() if n else None, C.byref(opts)))
        del keep
        return (row_map, [(outs[k], words[k], int(dst[k].null_count)) for k in range(len(fns))],
                M.read_info(opts, ("n_partitions", "n_peer_groups", "max_partition_rows", "n_rounds"),
                            ("ms_order", "ms_heads", "ms_scan")))

    # ---- WHERE: typed and string predicates to a row map (hmj_filter_device) ---------------------------------
    def filter_device(self, terms, n=None, want_mask=False, out=None):
        """Select the positions at which a predicate is TRUE (hmj_filter_device).  terms: a list of dicts {"column", "op",
        "lit", "valid", "bit_offset", "row_map", "clause", "negate"} or of tuples in that order (everything behind op
        optional).  column: a contiguous 1-D device tensor of an integer or float dtype of 1 to 8 bytes (the HMJ_TYPE_* is
        inferred), or a (chars, offsets) pair as `pack_strings` makes it; op: an HMJ_FILTER_* code; lit: a number converted
        to the column's dtype (no cast happens on the device), bytes / str for a string column, a pair of them for
        HMJ_FILTER_BETWEEN, None for IS_NULL / IS_NOT_NULL; valid: None or the column's Arrow bitmap (`pack_validity`), row i
        at bit bit_offset + i; row_map: None (position i reads row i), a contiguous 1-D int64 device tensor or a
        (device_pointer, n) pair -- a result's r_row / s_row --, HMJ_TAKE_NO_ROW entries reading as NULL; clause: terms of
        one clause are ORed, clauses ANDed, ids never decreasing (default 0); negate: HMJ_FILTER_NOT.  n: the positions
        (default: the first term's map length, else its column's rows).  out: None, or an int64 device tensor of at least n
        entries to write the map into.  Returns (the row map trimmed to n_out -- a view of an n-entry tensor, nothing at or
        behind n_out is written --, an int64 tensor of ceil(n / 64) mask words or None, {"n_out", "n_unknown", "ms_eval",
        "ms_write"}); `expected_filter` reproduces the map, `take_cols_device` / `take_str_device` consume it."""
        torch = self._torch
        self._sync_stream()
        keys = ("column", "op", "lit", "valid", "bit_offset", "row_map", "clause", "negate")
        terms = [t if isinstance(t, dict) else dict(zip(keys, t)) for t in terms]
        arr = (_lib.FilterTerm * max(len(terms), 1))()
        keep = []
        first_n = None
        for k, t in enumerate(terms):
            col, op = t["column"], int(t["op"])
            lit = t.get("lit")
            lits = [] if lit is None else (list(lit) if isinstance(lit, (tuple, list)) else [lit])
            if len(lits) > 2:
                raise ValueError("term %d: at most two literals" % k)
            map_n = None
            if t.get("row_map") is not None:
                arr[k].row_map, map_n, rm = M.row_map(t["row_map"], torch.int64,
                                                      "term %d: row_map must be a contiguous 1-D int64 device tensor", k)
                keep.append(rm)
            if isinstance(col, (tuple, list)):
                arr[k].type = _lib.HMJ_FILTER_LARGE_STRING
                arr[k].data, arr[k].chars_bytes, arr[k].offsets = M.str_column(col[0], col[1], "term %d: offsets", k)
                n_src = col[1].shape[0] - 1
                keep += [col[0], col[1]]
                for j, v in enumerate(lits):
                    b = v.encode("utf-8") if isinstance(v, str) else bytes(v)
                    buf = C.create_string_buffer(b, max(len(b), 1))
                    arr[k].str_lit[j] = C.addressof(buf) if b else None
                    arr[k].str_len[j] = len(b)
                    keep.append(buf)
            else:
                M.check_column(col, "term %d: the column must be a contiguous 1-D device tensor", k)
                code = M.type_code(col.dtype)
                arr[k].type = code
                arr[k].data = col.data_ptr() if col.shape[0] else None
                n_src = col.shape[0]
                keep.append(col)
                dt = np.dtype(M.TYPE_NAMES[code])
                for j, v in enumerate(lits):
                    arr[k].lit[j] = int(np.array([v], dtype=dt).view("u%d" % dt.itemsize)[0])
            arr[k].n_src = n_src
            arr[k].op = op & 0xFFFFFFFF
            arr[k].flags = _lib.HMJ_FILTER_NOT if t.get("negate") else 0
            arr[k].clause = int(t.get("clause") or 0)
            if t.get("valid") is not None:
                keep.append(M.validity(arr[k].validity, (t["valid"], t.get("bit_offset") or 0), n_src, "term %d", k, any_width=True))
            if first_n is None:
                first_n = n_src if map_n is None else map_n
        n = int((first_n or 0) if n is None else n)
        dev = self._dev
        if out is None:
            out = torch.empty(n, dtype=torch.int64, device=dev)
        elif not out.is_cuda or not out.is_contiguous() or out.dim() != 1 or out.dtype != torch.int64 or out.shape[0] < n:
            raise ValueError("out must be a contiguous 1-D int64 device tensor of at least n entries")
        words = torch.empty((n + 63) // 64, dtype=torch.int64, device=dev) if want_mask else None
        opts = M.new_opts(_lib.FilterOpts)
        self._check(self.L.hmj_filter_device(self.h, arr, len(terms), n, out.data_ptr() if n else None,
                                             words.data_ptr() if (words is not None and n) else None, C.byref(opts)))
        del keep
        info = M.read_info(opts, ("n_out", "n_unknown"), ("ms_eval", "ms_write"))
        return out[:info["n_out"]], words, info

    # ---- columns through a row map (hmj_take_cols_device) ------------------------------------------------
    def take_cols_device(self, cols, row_map, valid=None, n_out=None, want_validity=True):
        """Take fixed-width columns of one relation through a row map (hmj_take_cols_device): output row i is source row
        row_map[i], or NULL where row_map[i] is HMJ_TAKE_NO_ROW or the source slot is NULL (the bytes of a NULL slot are 0).
        cols: 1-D contiguous device tensors of one length whose element_size() is 1, 2, 4 or 8, or a contiguous [n,2]
        int64 tensor for a 16-byte column.  valid: None, or one entry per column as `join_cols_device` takes them: None, a
        uint8 bitmap tensor, or (tensor, bit_offset).  row_map: a contiguous 1-D int64 device tensor, or (device_pointer, n)
        -- a result's r_row / s_row with its n_matches; the result stays as it is.  n_out: rows to take (default: the whole
        map).  want_validity: True, False, or one bool per column.  The outputs are new tensors on the executor's device.
        Returns (tensors of the sources' dtypes and shapes, int64 tensors of ceil(n_out / 64) bitmap words -- None for a
        column without one, None instead of the list with want_validity=False --, {"null_count": [...], "n_no_row",
        "ms_take"}); `unpack_validity` reads the words."""
        torch = self._torch
        self._sync_stream()
        cols = list(cols)
        map_ptr, map_n, keep_map = M.row_map(row_map, torch.int64, "row_map must be a contiguous 1-D int64 device tensor")
        n_out = map_n if n_out is None else int(n_out)
        if not 0 <= n_out <= map_n:
            raise ValueError("n_out must be in 0..len(row_map)")
        widths = []
        for k, t in enumerate(cols):
            wide = t.dim() == 2 and t.shape[1] == 2 and t.element_size() == 8
            if not t.is_cuda or not t.is_contiguous() or not (t.dim() == 1 or wide):
                raise ValueError("column %d must be a contiguous device tensor, 1-D or [n,2] of 8-byte values" % k)
            widths.append(16 if wide else t.element_size())
        n_src = cols[0].shape[0] if cols else 0
        if any(t.shape[0] != n_src for t in cols):
            raise ValueError("columns must have one length")
        valid = [None] * len(cols) if valid is None else list(valid)
        if len(valid) != len(cols):
            raise ValueError("valid: one entry per column")
        wants = M.want_flags(want_validity, len(cols), "column")
        dev = self._dev
        src = (_lib.TakeSrc * max(len(cols), 1))()
        dst = (_lib.TakeDst * max(len(cols), 1))()
        outs, words, keep = [], [], []
        for k, t in enumerate(cols):
            src[k].data = t.data_ptr() if n_src else None
            src[k].width = widths[k]
            if valid[k] is not None:
                keep.append(M.validity(src[k].validity, valid[k], n_src, "valid[%d]", k))
            o = torch.empty((n_out,) + tuple(t.shape[1:]), dtype=t.dtype, device=dev)
            w = torch.empty((n_out + 63) // 64, dtype=torch.int64, device=dev) if wants[k] else None
            dst[k].data = o.data_ptr() if n_out else None
            dst[k].validity = w.data_ptr() if (w is not None and n_out) else None
            outs.append(o)
            words.append(w)
        opts = M.new_opts(_lib.TakeOpts)
        self._check(self.L.hmj_take_cols_device(self.h, src, len(cols), n_src, C.c_void_p(map_ptr), n_out, dst, C.byref(opts)))
        del keep, keep_map
        info = M.read_info(opts, ("n_no_row",), ("ms_take",), first={"null_count": [int(dst[k].null_count) for k in range(len(cols))]})
        return outs, (words if any(wants) or not cols else None), info

    # ---- a string column through a row map (hmj_take_str_device) -----------------------------------------
    def take_str_device(self, chars, offsets, row_map, valid=None, n_out=None, want_validity=True, capacity=None):
        """Take one Arrow large_string / large_binary column through a row map (hmj_take_str_device): output row i is
        source row row_map[i], or NULL -- with length 0 -- where row_map[i] is HMJ_TAKE_NO_ROW or the source slot is NULL; a
        valid empty string stays valid.  chars: a contiguous 1-byte device tensor of any alignment (None or empty when every
        row is empty), offsets: a contiguous int64 device tensor of n_src + 1 entries (offsets[0] need not be 0); no taken
        row may end behind len(chars).  valid: None, a uint8 bitmap tensor, or (tensor, bit_offset).  row_map and n_out as
        `take_cols_device` takes them, the (device_pointer, n) form of a result's r_row / s_row included; the result stays as
        it is.  capacity=None: a sizing call, an allocation of exactly total_bytes, then the full call; a capacity (an upper
        bound of the output bytes): one call, and HMJ_E_ARG when it is too small.
        Returns (chars_out uint8 [total_bytes], offsets_out int64 [n_out + 1], int64 tensor of ceil(n_out / 64) bitmap words
        or None with want_validity=False, {"null_count", "n_no_row", "total_bytes", "ms_offsets", "ms_chars"}); the times
        are those of the last call made.  `unpack_strings` and `unpack_validity` read the outputs."""
        torch = self._torch
        self._sync_stream()
        map_ptr, map_n, keep_map = M.row_map(row_map, torch.int64, "row_map must be a contiguous 1-D int64 device tensor")
        n_out = map_n if n_out is None else int(n_out)
        if not 0 <= n_out <= map_n:
            raise ValueError("n_out must be in 0..len(row_map)")
        src = _lib.TakeStrSrc()
        src.chars, src.chars_bytes, src.offsets = M.str_column(chars, offsets, "offsets")
        n_src = offsets.shape[0] - 1
        keep = M.validity(src.validity, valid, n_src, "valid", empty_is_absent=True)
        dev = self._dev
        off_out = torch.zeros(n_out + 1, dtype=torch.int64, device=dev)  # (n_out == 0 writes nothing: offsets[0] = 0 is ours)
        words = torch.empty((n_out + 63) // 64, dtype=torch.int64, device=dev) if want_validity else None
        dst = _lib.TakeStrDst()
        dst.offsets = off_out.data_ptr()
        dst.validity = words.data_ptr() if (words is not None and n_out) else None
        opts = M.new_opts(_lib.TakeStrOpts)

        def call():
            self._check(self.L.hmj_take_str_device(self.h, C.byref(src), n_src, C.c_void_p(map_ptr), n_out, C.byref(dst),
                                                   C.byref(opts)))

        if capacity is None:
            call()  # the sizing call
            capacity = int(dst.total_bytes)
        capacity = int(capacity)
        chars_out = torch.empty(max(capacity, 1), dtype=torch.uint8, device=dev)  # (never a NULL pointer: that is the sizing call)
        dst.chars = chars_out.data_ptr()
        dst.chars_capacity = capacity
        call()
        del keep, keep_map
        total = int(dst.total_bytes)
        info = M.read_info(opts, ("n_no_row",), ("ms_offsets", "ms_chars"), first={"null_count": int(dst.null_count)},
                           between={"total_bytes": total})
        return chars_out[:total], off_out, words, info

    def prepare_build(self, build, n_probe_hint):
        """Partition the build side now; the next matching plain-count join_device skips that work."""
        self._sync_stream()
        bp, nb = _dev_ptr(build)
        self._check(self.L.hmj_prepare_build_u64_device(self.h, C.c_void_p(bp), nb, n_probe_hint))

    def join_host(self, build, probe, flags=0):
        """build/probe: numpy uint64 [n,2] in host memory (the reference ctor's situation)."""
        self._sync_stream()
        b = np.ascontiguousarray(build, np.uint64).reshape(-1, 2)
        p = np.ascontiguousarray(probe, np.uint64).reshape(-1, 2)
        res = JoinResult()
        self._check(self.L.hmj_join_u64(self.h, b.ctypes.data_as(C.c_void_p), len(b), p.ctypes.data_as(C.c_void_p),
                                        len(p), flags, C.byref(res)))
        return res

    def columns_to_numpy(self, res, host):
        """Copy the result columns out as an [n,3] uint64 array of (key, rval, sval)."""
        if not host:
            return self._rows(res, ("key", "rval", "sval"))
        n = int(res.n_matches)
        out = np.empty((n, 3), np.uint64)
        if n == 0 or not res.key:
            return out[:0]
        for c, ptr in enumerate((res.key, res.rval, res.sval)):
            out[:, c] = np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_uint64)), shape=(n,))
        return out

    def release_result(self):
        self._group_rows = self._group_groups = 0
        self.L.hmj_release_result(self.h)

    # ---- multi-GPU exchange (hmj_comm_* / hmj_exchange_join_u64_device) -------------------------
    def comm_init_rccl(self, n_ranks, rank, unique_id):
        """unique_id: the 128 bytes rank 0 got from hashmergejoin_amd.dist.new_unique_id()."""
        buf = (C.c_char * 128).from_buffer_copy(bytes(unique_id))
        self._check(self.L.hmj_comm_init_rank(self.h, n_ranks, rank, C.cast(buf, C.c_void_p)))

    def comm_set_transport(self, transport):
        """transport: a _lib.Transport whose callbacks stay alive as long as this executor uses them."""
        self._keep = transport
        self._check(self.L.hmj_comm_set_transport(self.h, C.byref(transport.struct)))

    def comm_set_self_exchange(self, on=True):
        """One-rank communicators: run the whole exchange path (tests / rehearsals) instead of the plain local join."""
        self._check(self.L.hmj_comm_set_self_exchange(self.h, int(bool(on))))

    def comm_set_owner_path(self, split=False):
        """Non-ordered distributed joins: digit-range owners with per-round joins (default) or, split=True, round 2's
        hash owner with its separate owner split and one local join (hmj_comm_set_owner_path)."""
        self._check(self.L.hmj_comm_set_owner_path(self.h, 1 if split else 0))

    def comm_set_timeout_ms(self, timeout_ms):
        """Deadline of one exchange step (hmj_comm_set_timeout_ms; 0 = wait for ever): past it the step returns
        HMJ_E_TIMEOUT and the communicator is unusable."""
        self._check(self.L.hmj_comm_set_timeout_ms(self.h, int(timeout_ms)))

    def comm_get_timeout_ms(self):
        v = C.c_uint64(0)
        self._check(self.L.hmj_comm_get_timeout_ms(self.h, C.byref(v)))
        return int(v.value)

    def comm_set_message_bytes(self, max_message_bytes=0, probe_round_bytes=0):
        self._check(self.L.hmj_comm_set_message_bytes(self.h, max_message_bytes, probe_round_bytes))

    def owner_split(self, rel, n_ranks, splitters=None):
        """hmj_owner_split_u64_device: (rows grouped by owner, [G'+1] offsets) with G' = 2^ceil(log2 n_ranks)."""
        torch = self._torch
        self._sync_stream()
        ptr, n = _dev_ptr(rel)
        out = torch.empty_like(rel)
        nd = 1
        while nd < n_ranks:
            nd *= 2
        off = torch.empty(nd + 1, dtype=torch.int64, device=rel.device)
        sp = None
        if splitters is not None:
            sp = (C.c_uint64 * (n_ranks - 1))(*[int(x) for x in splitters])
        self._check(self.L.hmj_owner_split_u64_device(self.h, C.c_void_p(ptr), n, n_ranks, sp, C.c_void_p(out.data_ptr()),
                                                      C.c_void_p(off.data_ptr())))
        return out, off

    def exchange_join(self, build_shard, probe_shard, flags=0):
        """Distributed join of row shards (collective).  Returns (local JoinResult, global JoinResult)."""
        self._sync_stream()
        loc, glob = JoinResult(), JoinResult()
        self._check(self.L.hmj_exchange_join_u64_device(self.h, *_dev_ptrs(build_shard, probe_shard), flags,
                                                        C.byref(loc), C.byref(glob)))
        return loc, glob

    def exchange_join_kind(self, build_shard, probe_shard, side, kind, flags=0, probe_fill=0, build_fill=0):
        """Distributed join kind of row shards (collective; hmj_exchange_join_kind_u64_device).  side = HMJ_KIND_PROBE_SIDE
        (kind HMJ_JOIN_*) or HMJ_KIND_BUILD_SIDE (kind HMJ_BUILD_* / HMJ_FULL_OUTER).  Returns (local JoinResult, global
        JoinResult, {"local": counters, "global": counters}) with the counters of hmj_kind_counts.  The local columns are
        read as those of the single-GPU kind: `probe_rows_to_numpy`, `build_rows_to_numpy` or `columns_to_numpy`."""
        self._sync_stream()
        loc, glob = JoinResult(), JoinResult()
        opts = M.new_opts(_lib.ExchangeKindOpts, side=side, kind=kind, probe_fill=probe_fill, build_fill=build_fill)
        self._check(self.L.hmj_exchange_join_kind_u64_device(self.h, *_dev_ptrs(build_shard, probe_shard), flags,
                                                             C.byref(opts), C.byref(loc), C.byref(glob)))
        return loc, glob, {"local": opts.local.as_dict(), "global": getattr(opts, "global").as_dict()}

    def last_exchange_info(self):
        info = _lib.ExchangeInfo()
        self._check(self.L.hmj_last_exchange_info(self.h, C.byref(info)))
        return info.as_dict()

    # ---- single radix pass (hmj_partition_u64_device) ------------------------------------------
    def partition_device(self, rel, shift, bits):
        torch = self._torch
        self._sync_stream()
        ptr, n = _dev_ptr(rel)
        out = torch.empty_like(rel)
        off = torch.empty((1 << bits) + 1, dtype=torch.int64, device=rel.device)
        self._check(self.L.hmj_partition_u64_device(self.h, C.c_void_p(ptr), n, shift, bits, C.c_void_p(out.data_ptr()),
                                                    C.c_void_p(off.data_ptr())))
        return out, off

    def autotune(self, n_build, n_probe, apply=True):
        """Time the join of synthetic relations with B-1, B, B+1 radix bits (hmj_autotune_radix_bits).
        Returns (best_bits, {bits: ms}); apply=True keeps the fastest as this executor's plan."""
        self._sync_stream()
        best, ms = C.c_int(0), (C.c_double * 3)()
        self._check(self.L.hmj_autotune_radix_bits(self.h, n_build, n_probe, 1 if apply else 0, C.byref(best), ms))
        b0 = plan(n_build)[0]
        return best.value, {b0 - 1 + k: ms[k] for k in range(3) if ms[k] >= 0}

    def sort_device(self, rel, inplace=False):
        """Full ascending-key sort of a device relation (hmj_sort_u64_device); returns a new tensor, or
        sorts `rel` itself with inplace=True (the radix_int_inplace replacement)."""
        torch = self._torch
        self._sync_stream()
        ptr, n = _dev_ptr(rel)
        out = rel if inplace else torch.empty_like(rel)
        self._check(self.L.hmj_sort_u64_device(self.h, C.c_void_p(ptr), n, C.c_void_p(out.data_ptr())))
        return out

    # ---- generators ----------------------------------------------------------------------------
    def _alloc(self, n):
        torch = self._torch
        return torch.empty((n, 2), dtype=torch.int64, device="cuda:%d" % self.device)

    def gen_build(self, n, start=0, seed=SEED_B):
        self._sync_stream()
        t = self._alloc(n)
        self._check(self.L.hmj_gen_build_u64_device(self.h, C.c_void_p(t.data_ptr()), n, start, seed))
        return t

    def gen_probe(self, n, n_build, start=0, seed=SEED_B, miss_mod=0):
        self._sync_stream()
        t = self._alloc(n)
        self._check(self.L.hmj_gen_probe_u64_device(self.h, C.c_void_p(t.data_ptr()), n, start, n_build, seed, miss_mod))
        return t

    def gen_from_cdf(self, n, thr_dev, start=0, seed=SEED_B, zseed=0x1234567):
        self._sync_stream()
        t = self._alloc(n)
        self._check(self.L.hmj_gen_from_cdf_u64_device(self.h, C.c_void_p(t.data_ptr()), n, start,
                                                       C.c_void_p(thr_dev.data_ptr()), thr_dev.numel(), seed, zseed))
        return t

    def gen_uniform_domain(self, n, domain, start=0, seed=SEED_B, zseed=0x7654321):
        self._sync_stream()
        t = self._alloc(n)
        self._check(self.L.hmj_gen_uniform_domain_u64_device(self.h, C.c_void_p(t.data_ptr()), n, start, domain, seed, zseed))
        return t


def pack_strings(keys, device=None):
    """Keys (str, encoded as UTF-8, or bytes) -> (chars uint8 [total bytes], offsets int64 [n + 1]): the Arrow
    large_string layout hmj_join_str_device reads.  device=None leaves both tensors on the CPU."""
    import torch

    enc = [k.encode("utf-8") if isinstance(k, str) else bytes(k) for k in keys]
    lens = np.fromiter((len(b) for b in enc), dtype=np.int64, count=len(enc))
    offsets = np.zeros(len(enc) + 1, np.int64)
    np.cumsum(lens, out=offsets[1:])
    chars = np.frombuffer(b"".join(enc), dtype=np.uint8).copy()
    c, o = torch.from_numpy(chars), torch.from_numpy(offsets)
    if device is not None:
        c, o = c.to(device), o.to(device)
    return c, o


def unpack_strings(chars, offsets, valid=None):
    """The inverse of `pack_strings`: (chars uint8, offsets int64 [n + 1]; torch tensors or numpy arrays) -> a list of n
    `bytes`.  valid: None, or n bools (True = valid; `unpack_validity` makes them from bitmap words): a NULL slot reads as
    None."""
    if hasattr(chars, "cpu"):
        chars = chars.cpu().numpy()
    if hasattr(offsets, "cpu"):
        offsets = offsets.cpu().numpy()
    raw = np.ascontiguousarray(chars).view(np.uint8).tobytes() if chars is not None else b""
    off = np.asarray(offsets).astype(np.int64).tolist()
    if len(off) < 1:
        raise ValueError("offsets must hold n + 1 entries")
    if valid is not None and len(valid) != len(off) - 1:
        raise ValueError("valid: one entry per row")
    return [None if (valid is not None and not valid[i]) else raw[off[i]:off[i + 1]] for i in range(len(off) - 1)]


def pack_validity(mask, bit_offset=0, device=None):
    """A bool array (True = valid) -> the Arrow validity bitmap of a column slice that starts `bit_offset` bits into it:
    a uint8 tensor of ceil((bit_offset + n) / 8) bytes, least-significant bit first, row i at bit bit_offset + i.  The
    bits in front of bit_offset are set on purpose -- a reader that ignores the offset sees valid rows where it should
    not --; the padding behind the last row is 0.  device=None leaves the tensor on the CPU."""
    import torch

    mask = np.asarray(mask, bool).ravel()
    bit_offset = int(bit_offset)
    if bit_offset < 0:
        raise ValueError("bit_offset must not be negative")
    bits = np.concatenate([np.ones(bit_offset, bool), mask])
    t = torch.from_numpy(np.packbits(bits, bitorder="little"))
    return t if device is None else t.to(device)


def unpack_validity(words, n):
    """The first n rows of an Arrow validity bitmap held as 64-bit words (what `Executor.take_cols_device` returns; a torch
    tensor or a numpy array of int64 / uint64) -> a bool array, True = valid: row i is bit i & 63 of word i >> 6."""
    if hasattr(words, "cpu"):
        words = words.cpu().numpy()
    raw = np.ascontiguousarray(words).view(np.uint8)
    n = int(n)
    if n < 0 or raw.size * 8 < n:
        raise ValueError("the words hold fewer than n bits")
    return np.unpackbits(raw, bitorder="little")[:n].astype(bool)


class HashMergeJoin:
    """Python mirror of the reference operator (hashjoin.h:33-199).

        hmj = HashMergeJoin(r, s, num_threads=1)     # hashjoin.h:56-58
        for key, rval, sval in hmj: ...              # begin()/end(), hashjoin.h:183-191
        hmj.clear()                                  # hashjoin.h:192-195

    r, s: [n,2] uint64 relations {key,val}, numpy (host) or torch (device).  `num_threads` is
    accepted for signature compatibility; the work runs on the GPU.  Iteration order is ascending
    key, as the reference's.  Keys must be unique within each relation for bit-exact parity with
    the reference iterator (its behaviour on duplicates is not relational).
    """

    def __init__(self, r=None, s=None, num_threads=1, executor=None, flags=0):
        self.num_threads = num_threads
        self._rows = None
        self.result = None
        if r is None and s is None:  # HashMergeJoin() = default, hashjoin.h:55
            return
        self._ex = executor or Executor()
        fl = HMJ_MATERIALIZE | HMJ_ORDERED | flags
        host = isinstance(r, np.ndarray)
        res = self._ex.join_host(r, s, fl) if host else self._ex.join_device(r, s, fl)
        self.result = res
        self._rows = self._ex.columns_to_numpy(res, host)

    def __iter__(self):
        if self._rows is None:
            return iter(())
        return (tuple(int(x) for x in row) for row in self._rows)

    def __len__(self):
        return 0 if self._rows is None else len(self._rows)

    def rows(self):
        """All result rows as an [n,3] uint64 array (key, rval, sval)."""
        return np.empty((0, 3), np.uint64) if self._rows is None else self._rows

    def clear(self):
        self._rows = None
        self.result = None
