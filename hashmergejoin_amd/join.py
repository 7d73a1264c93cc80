"""Host-side mirror of the reference's join operator over the C ABI.

`Executor` owns one hmj_ctx (one per GPU / per process).  `HashMergeJoin` mirrors
HashMergeJoin<RIter,SIter> (reference hashjoin.h:33-199): construct from two relations, iterate
(key, rval, sval) in ascending-key order, `clear()`.  torch is used only to hold device memory
and to name the current stream.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import (HMJ_CHECKSUM, HMJ_FIRST_WINS, HMJ_MATERIALIZE, HMJ_ORDERED, HMJ_SUM_PROBE,
                   HmjError, JoinResult, Timing)

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


class Executor:
    """One hmj_ctx.  All methods raise HmjError on a nonzero status."""

    def __init__(self, device=None, use_torch_stream=True):
        import torch  # noqa: F401  (must be loaded before the HIP library, see _lib.load_library)

        self._torch = torch
        self.L = _lib.load_library()
        if device is None:
            device = torch.cuda.current_device()
        self.device = int(device)
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
        bp, nb = _dev_ptr(build)
        pp, np_ = _dev_ptr(probe)
        res = JoinResult()
        self._check(self.L.hmj_join_u64_device(self.h, C.c_void_p(bp), nb, C.c_void_p(pp), np_, flags, C.byref(res)))
        return res

    def join_kind_device(self, build, probe, kind, flags=0, outer_fill=0):
        """Semi / anti / probe-side outer join (hmj_join_kind_u64_device; kind = HMJ_JOIN_*).  Returns (JoinResult,
        {"n_probe_matched": .., "n_probe_unmatched": ..}).  SEMI / ANTI results have no rval column: read them with
        `probe_rows_to_numpy`; PROBE_OUTER rows with `columns_to_numpy`.  HMJ_JOIN_INNER is join_device (counters 0)."""
        self._sync_stream()
        bp, nb = _dev_ptr(build)
        pp, np_ = _dev_ptr(probe)
        res = JoinResult()
        opts = _lib.JoinOpts()
        opts.struct_size = C.sizeof(_lib.JoinOpts)
        opts.kind = int(kind)
        opts.outer_fill = int(outer_fill) & 0xFFFFFFFFFFFFFFFF
        self._check(self.L.hmj_join_kind_u64_device(self.h, C.c_void_p(bp), nb, C.c_void_p(pp), np_, flags, C.byref(opts),
                                                    C.byref(res)))
        return res, {"n_probe_matched": int(opts.n_probe_matched), "n_probe_unmatched": int(opts.n_probe_unmatched)}

    def probe_rows_to_numpy(self, res):
        """Copy a semi / anti join's device result out as an [n,2] uint64 array of (key, sval)."""
        n = int(res.n_matches)
        out = np.empty((n, 2), np.uint64)
        if n == 0 or not res.key:
            return out[:0]
        torch = self._torch
        tmp = torch.empty(n, dtype=torch.int64, device="cuda:%d" % self.device)
        for c, ptr in enumerate((res.key, res.sval)):
            _memcpy_d2d(torch, tmp, ptr, n * 8)
            out[:, c] = tmp.cpu().numpy().view(np.uint64)
        return out

    def join_build_kind_device(self, build, probe, kind, flags=0, build_fill=0, probe_fill=0):
        """Build-side semi / anti / outer join or the full outer join (hmj_join_build_kind_u64_device; kind = HMJ_BUILD_SEMI,
        HMJ_BUILD_ANTI, HMJ_BUILD_OUTER or HMJ_FULL_OUTER).  Returns (JoinResult, {"n_build_matched", "n_build_unmatched",
        "n_probe_matched", "n_probe_unmatched"}).  BUILD_SEMI / BUILD_ANTI results have no sval column: read them with
        `build_rows_to_numpy`; the outer kinds' rows with `columns_to_numpy`."""
        self._sync_stream()
        bp, nb = _dev_ptr(build)
        pp, np_ = _dev_ptr(probe)
        res = JoinResult()
        opts = _lib.BuildJoinOpts()
        opts.struct_size = C.sizeof(_lib.BuildJoinOpts)
        opts.kind = int(kind)
        opts.build_fill = int(build_fill) & 0xFFFFFFFFFFFFFFFF
        opts.probe_fill = int(probe_fill) & 0xFFFFFFFFFFFFFFFF
        self._check(self.L.hmj_join_build_kind_u64_device(self.h, C.c_void_p(bp), nb, C.c_void_p(pp), np_, flags,
                                                          C.byref(opts), C.byref(res)))
        return res, {k: int(getattr(opts, k)) for k in ("n_build_matched", "n_build_unmatched", "n_probe_matched",
                                                         "n_probe_unmatched")}

    def build_rows_to_numpy(self, res):
        """Copy a build semi / anti join's device result out as an [n,2] uint64 array of (key, rval)."""
        n = int(res.n_matches)
        out = np.empty((n, 2), np.uint64)
        if n == 0 or not res.key:
            return out[:0]
        torch = self._torch
        tmp = torch.empty(n, dtype=torch.int64, device="cuda:%d" % self.device)
        for c, ptr in enumerate((res.key, res.rval)):
            _memcpy_d2d(torch, tmp, ptr, n * 8)
            out[:, c] = tmp.cpu().numpy().view(np.uint64)
        return out

    # ---- string keys (hmj_hash_str_device / hmj_join_str_device) ------------------------------------
    def _str_rel(self, rel):
        """(chars uint8, offsets int64 [n + 1], vals int64 [n]) device tensors -> StrRel (chars may be None or empty when
        every key is empty)."""
        chars, offsets, vals = rel
        _check_col(offsets, "offsets")
        _check_col(vals, "vals")
        n = vals.shape[0]
        if offsets.shape[0] != n + 1:
            raise ValueError("offsets must hold n + 1 entries")
        r = _lib.StrRel()
        r.chars = _chars_ptr(chars)
        r.offsets = offsets.data_ptr() if n else None
        r.vals = vals.data_ptr() if n else None
        r.n = n
        return r

    def hash_str_device(self, chars, offsets, hash_bits=0):
        """std::hash<std::string> of every key (libstdc++'s _Hash_bytes), computed on the device: int64 tensor [n]
        (read as uint64).  hash_bits 1..63 keeps the top bits only (h >> (64 - hash_bits))."""
        torch = self._torch
        _check_col(offsets, "offsets")
        if offsets.shape[0] < 1:
            raise ValueError("offsets must hold n + 1 entries")
        self._sync_stream()
        n = offsets.shape[0] - 1
        out = torch.empty(n, dtype=torch.int64, device=offsets.device)
        self._check(self.L.hmj_hash_str_device(self.h, _chars_ptr(chars), C.c_void_p(offsets.data_ptr()), max(n, 0),
                                               int(hash_bits), C.c_void_p(out.data_ptr()) if n > 0 else None))
        return out

    def _str_validity(self, valid, n, name, dst):
        """A string relation's validity bitmap -> the Validity `dst` embedded in hmj_str_kind_opts; returns what must stay
        alive for the call.  valid: None (no bitmap on this side), a uint8 device tensor (an Arrow bitmap, LSB first), or
        (tensor, bit_offset)."""
        if valid is None:
            return None
        t, off = valid if isinstance(valid, tuple) else (valid, 0)
        off = int(off)
        if not t.is_cuda or not t.is_contiguous() or t.dim() != 1 or t.element_size() != 1:
            raise ValueError("%s must be a contiguous 1-D uint8 device tensor" % name)
        if off < 0:
            raise ValueError("%s: bit_offset must not be negative" % name)
        if t.shape[0] and off + n < (1 << 64) and t.shape[0] * 8 < off + n:  # (an overflowing offset is the library's to reject)
            raise ValueError("%s holds fewer than bit_offset + n bits" % name)
        # (an empty tensor: bits == NULL, no NULL on this side; n == 0: the pointer is still passed, nothing reads it)
        dst.bits = t.data_ptr() if t.shape[0] else None
        dst.bit_offset = off & 0xFFFFFFFFFFFFFFFF
        return t

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
        opts = _lib.StrJoinOpts()
        opts.struct_size = C.sizeof(_lib.StrJoinOpts)
        opts.hash_bits = int(hash_bits)
        res = _lib.StrResult()
        self._check(self.L.hmj_join_str_device(self.h, C.byref(rb), C.byref(rp), flags, C.byref(opts), C.byref(res)))
        info = {"n_hash_pairs": int(opts.n_hash_pairs), "n_collisions": int(opts.n_collisions), "n_build_null": 0, "n_probe_null": 0}
        for k in ("ms_hash", "ms_join", "ms_verify", "ms_order"):
            info[k] = float(getattr(opts, k))
        return res, info

    def str_rows_to_numpy(self, res):
        """Copy a string join's device result out as an [n,5] uint64 array of (hash, r_row, s_row, rval, sval)."""
        n = int(res.n_matches)
        out = np.empty((n, 5), np.uint64)
        if n == 0 or not res.hash:
            return out[:0]
        torch = self._torch
        tmp = torch.empty(n, dtype=torch.int64, device="cuda:%d" % self.device)
        for c, ptr in enumerate((res.hash, res.r_row, res.s_row, res.rval, res.sval)):
            _memcpy_d2d(torch, tmp, ptr, n * 8)
            out[:, c] = tmp.cpu().numpy().view(np.uint64)
        return out

    # ---- multi-column fixed-width keys (hmj_join_cols_device) ------------------------------------------
    def _cols_rel(self, cols, vals):
        """Key columns (1-D contiguous device tensors of one length, any dtype) + payloads (int64 [n] or None) -> (ColsRel,
        the KeyCol array it points to: keep it alive for the call).  Widths, alignment and column counts are checked by
        the library."""
        cols = list(cols)
        for k, t in enumerate(cols):
            if not t.is_cuda or not t.is_contiguous() or t.dim() != 1:
                raise ValueError("key column %d must be a contiguous 1-D device tensor" % k)
        n = cols[0].shape[0] if cols else (vals.shape[0] if vals is not None else 0)
        if any(t.shape[0] != n for t in cols):
            raise ValueError("key columns must have one length")
        if vals is not None:
            _check_col(vals, "vals")
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
        n = int(rel.n)
        arr = (_lib.Validity * max(len(valid), 1))()
        keep = [arr]
        for k, v in enumerate(valid):
            if v is None:
                continue
            t, off = v if isinstance(v, tuple) else (v, 0)
            off = int(off)
            if not t.is_cuda or not t.is_contiguous() or t.dim() != 1 or t.element_size() != 1:
                raise ValueError("%s[%d] must be a contiguous 1-D uint8 device tensor" % (name, k))
            if off < 0:
                raise ValueError("%s[%d]: bit_offset must not be negative" % (name, k))
            if off + n < (1 << 64) and t.shape[0] * 8 < off + n:  # (an overflowing offset is the library's to reject)
                raise ValueError("%s[%d] holds fewer than bit_offset + n bits" % (name, k))
            # (n == 0: the pointer is still passed; nothing reads it)
            arr[k].bits = t.data_ptr() if t.shape[0] else None
            arr[k].bit_offset = off & 0xFFFFFFFFFFFFFFFF
            keep.append(t)
        return arr, keep

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
        opts = _lib.ColsJoinOpts()
        opts.struct_size = C.sizeof(_lib.ColsJoinOpts)
        opts.hash_bits = int(hash_bits)
        opts.force_hashed = 1 if force_hashed else 0
        res = _lib.ColsResult()
        self._check(self.L.hmj_join_cols_device(self.h, C.byref(rb), C.byref(rp), flags, C.byref(opts), C.byref(res)))
        del keep_b, keep_p
        info = {"form": int(opts.form), "n_key_pairs": int(opts.n_key_pairs), "n_collisions": int(opts.n_collisions),
                "n_build_null": 0, "n_probe_null": 0}
        for k in ("ms_key", "ms_join", "ms_verify", "ms_order"):
            info[k] = float(getattr(opts, k))
        return res, info

    def cols_rows_to_numpy(self, res):
        """Copy a multi-column join's device result out as an [n,5] uint64 array of (key64, r_row, s_row, rval, sval)."""
        n = int(res.n_matches)
        out = np.empty((n, 5), np.uint64)
        if n == 0 or not res.key64:
            return out[:0]
        torch = self._torch
        tmp = torch.empty(n, dtype=torch.int64, device="cuda:%d" % self.device)
        for c, ptr in enumerate((res.key64, res.r_row, res.s_row, res.rval, res.sval)):
            _memcpy_d2d(torch, tmp, ptr, n * 8)
            out[:, c] = tmp.cpu().numpy().view(np.uint64)
        return out

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
        opts = _lib.ColsKindOpts()
        opts.struct_size = C.sizeof(_lib.ColsKindOpts)
        opts.side = int(side)
        opts.kind = int(kind)
        opts.hash_bits = int(hash_bits)
        opts.force_hashed = 1 if force_hashed else 0
        opts.probe_fill = int(probe_fill) & 0xFFFFFFFFFFFFFFFF
        opts.build_fill = int(build_fill) & 0xFFFFFFFFFFFFFFFF
        vb, keep_vb = self._validity(build_valid, rb, "build_valid")
        vp, keep_vp = self._validity(probe_valid, rp, "probe_valid")
        if vb is not None:
            opts.build_validity = vb
        if vp is not None:
            opts.probe_validity = vp
        res = _lib.ColsResult()
        self._check(self.L.hmj_join_kind_cols_device(self.h, C.byref(rb), C.byref(rp), flags, C.byref(opts), C.byref(res)))
        del keep_b, keep_p, keep_vb, keep_vp
        info = opts.counts.as_dict()
        info.update({"form": int(opts.form), "n_key_pairs": int(opts.n_key_pairs), "n_collisions": int(opts.n_collisions),
                     "n_build_null": int(opts.n_build_null), "n_probe_null": int(opts.n_probe_null)})
        for k in ("ms_key", "ms_join", "ms_verify", "ms_emit", "ms_order"):
            info[k] = float(getattr(opts, k))
        return res, info

    def cols_kind_rows_to_numpy(self, res):
        """Copy a multi-column kind join's device result out as an [n,5] uint64 array of (key64, r_row, s_row, rval, sval);
        a column the kind does not produce (r_row / rval of probe SEMI / ANTI, s_row / sval of BUILD_SEMI / BUILD_ANTI)
        reads as 0."""
        n = int(res.n_matches)
        out = np.empty((n, 5), np.uint64)
        if n == 0 or not res.key64:
            return out[:0]
        torch = self._torch
        tmp = torch.empty(n, dtype=torch.int64, device="cuda:%d" % self.device)
        for c, ptr in enumerate((res.key64, res.r_row, res.s_row, res.rval, res.sval)):
            if not ptr:
                out[:, c] = 0
                continue
            _memcpy_d2d(torch, tmp, ptr, n * 8)
            out[:, c] = tmp.cpu().numpy().view(np.uint64)
        return out

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
        opts = _lib.GroupOpts()
        opts.struct_size = C.sizeof(_lib.GroupOpts)
        opts.want = int(want)
        opts.hash_bits = int(hash_bits)
        opts.force_hashed = 1 if force_hashed else 0
        v, keep_v = self._validity(valid, rel, "valid")
        if v is not None:
            opts.validity = v
        res = _lib.GroupResult()
        self._group_rows = self._group_groups = 0  # (group_agg_device: the library drops its live grouping here)
        self._check(self.L.hmj_group_cols_device(self.h, C.byref(rel), flags, C.byref(opts), C.byref(res)))
        if flags & (HMJ_MATERIALIZE | HMJ_ORDERED):
            self._group_rows, self._group_groups = int(res.n_rows), int(res.n_groups)
        del keep, keep_v
        info = {"form": int(opts.form), "n_null": int(opts.n_null), "n_collisions": int(opts.n_collisions)}
        for k in ("ms_key", "ms_sort", "ms_groups", "ms_agg"):
            info[k] = float(getattr(opts, k))
        return res, info

    def group_rows_to_numpy(self, res):
        """Copy a grouping's device result out: {"key64", "first_row", "count", "sum", "min", "max", "group_of_row"} -> a
        uint64 array (n_groups entries; group_of_row: n_rows), or None for a column the call did not produce."""
        torch = self._torch
        out = {}
        for name in ("key64", "first_row", "count", "sum", "min", "max", "group_of_row"):
            ptr = getattr(res, name)
            n = int(res.n_rows if name == "group_of_row" else res.n_groups)
            if not ptr:
                out[name] = None
                continue
            tmp = torch.empty(n, dtype=torch.int64, device="cuda:%d" % self.device)
            _memcpy_d2d(torch, tmp, ptr, n * 8)
            out[name] = tmp.cpu().numpy().view(np.uint64)
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
                _check_col(col[1], "%s column %d: offsets" % (name, k))
                if col[1].shape[0] < 1:
                    raise ValueError("%s column %d: offsets must hold n + 1 entries" % (name, k))
                m = col[1].shape[0] - 1
            else:
                if not col.is_cuda or not col.is_contiguous() or col.dim() != 1:
                    raise ValueError("%s column %d must be a contiguous 1-D device tensor" % (name, k))
                m = col.shape[0]
            if n is None:
                n = m
            if m != n:
                raise ValueError("%s: key columns must have one length" % name)
        if n is None:
            n = vals.shape[0] if vals is not None else 0
        if vals is not None:
            _check_col(vals, "vals")
            if vals.shape[0] != n:
                raise ValueError("vals must hold one payload per row")
        if valid is not None and len(list(valid)) != len(cols):
            raise ValueError("%s_valid: one entry per key column" % name)
        arr = (_lib.MixedCol * max(len(cols), 1))()
        keep = [arr, cols]
        for k, col in enumerate(cols):
            if isinstance(col, (tuple, list)):
                arr[k].type = _lib.HMJ_KEY_LARGE_STRING
                arr[k].width = 0
                arr[k].data = _chars_ptr(col[0])
                arr[k].offsets = col[1].data_ptr()
            else:
                arr[k].type = _lib.HMJ_KEY_FIXED
                arr[k].width = col.element_size()
                arr[k].data = col.data_ptr() if n else None
            if valid is not None and list(valid)[k] is not None:
                keep.append(self._str_validity(list(valid)[k], n, "%s_valid[%d]" % (name, k), arr[k].validity))
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
        opts = _lib.MixedOpts()
        opts.struct_size = C.sizeof(_lib.MixedOpts)
        opts.side = int(side)
        opts.kind = int(kind)
        opts.hash_bits = int(hash_bits)
        opts.probe_fill = int(probe_fill) & 0xFFFFFFFFFFFFFFFF
        opts.build_fill = int(build_fill) & 0xFFFFFFFFFFFFFFFF
        res = _lib.ColsResult()
        self._check(self.L.hmj_join_mixed_device(self.h, C.byref(rb), C.byref(rp), flags, C.byref(opts), C.byref(res)))
        del keep_b, keep_p
        info = opts.counts.as_dict()
        info.update({"n_key_pairs": int(opts.n_key_pairs), "n_collisions": int(opts.n_collisions),
                     "n_build_null": int(opts.n_build_null), "n_probe_null": int(opts.n_probe_null)})
        for k in ("ms_key", "ms_join", "ms_verify", "ms_emit", "ms_order"):
            info[k] = float(getattr(opts, k))
        return res, info

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
        opts = _lib.GroupOpts()
        opts.struct_size = C.sizeof(_lib.GroupOpts)
        opts.want = int(want)
        opts.hash_bits = int(hash_bits)
        res = _lib.GroupResult()
        self._group_rows = self._group_groups = 0  # (group_agg_device: the library drops its live grouping here)
        self._check(self.L.hmj_group_mixed_device(self.h, C.byref(rel), flags, C.byref(opts), C.byref(res)))
        if flags & (HMJ_MATERIALIZE | HMJ_ORDERED):
            self._group_rows, self._group_groups = int(res.n_rows), int(res.n_groups)
        del keep
        info = {"form": int(opts.form), "n_null": int(opts.n_null), "n_collisions": int(opts.n_collisions)}
        for k in ("ms_key", "ms_sort", "ms_groups", "ms_agg"):
            info[k] = float(getattr(opts, k))
        return res, info

    # ---- typed columns aggregated over the live grouping (hmj_group_agg_device) ----------------------------
    def _agg_type(self, t):
        torch = self._torch
        names = ("int8", "int16", "int32", "int64", "uint8", "uint16", "uint32", "uint64", "float32", "float64")
        for code, name in enumerate(names):
            if getattr(torch, name, None) is t.dtype:
                return code
        raise ValueError("no HMJ_TYPE_* for %s" % (t.dtype,))

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
        wants = [bool(want_validity)] * len(aggs) if isinstance(want_validity, (bool, int)) else [bool(w) for w in want_validity]
        if len(wants) != len(aggs):
            raise ValueError("want_validity: one entry per aggregate")
        if n_rows is None:
            lens = [a[1].shape[0] for a in aggs if a[1] is not None]
            n_rows = lens[0] if lens else getattr(self, "_group_rows", 0)
        n_rows = int(n_rows)
        # the groups size the outputs: an HMJ_E_ARG call must still reach the library, so any count will do for it
        n_groups = int(getattr(self, "_group_groups", 0))
        dev = "cuda:%d" % self.device
        src = (_lib.AggSrc * max(len(aggs), 1))()
        dst = (_lib.AggDst * max(len(aggs), 1))()
        outs, words, keep = [], [], []
        f64, i64 = torch.float64, torch.int64
        u64 = getattr(torch, "uint64", i64)
        for k, a in enumerate(aggs):
            op, t, v = int(a[0]), a[1], a[2] if len(a) > 2 else None
            off = int(a[3]) if len(a) > 3 else 0
            code = _lib.HMJ_TYPE_U64
            if t is not None:
                if not t.is_cuda or not t.is_contiguous() or t.dim() != 1:
                    raise ValueError("aggregate %d: the column must be a contiguous 1-D device tensor" % k)
                code = self._agg_type(t)
                src[k].data = t.data_ptr() if t.shape[0] else None
                keep.append(t)
            src[k].type = code
            src[k].op = op & 0xFFFFFFFF
            if v is not None:
                if not v.is_cuda or not v.is_contiguous() or v.dim() != 1:
                    raise ValueError("aggregate %d: valid must be a contiguous 1-D device tensor" % k)
                if off < 0:
                    raise ValueError("aggregate %d: bit_offset must not be negative" % k)
                src[k].validity.bits = v.data_ptr() if v.shape[0] else None
                src[k].validity.bit_offset = off & 0xFFFFFFFFFFFFFFFF
                keep.append(v)
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
        opts = _lib.GroupAggOpts()
        opts.struct_size = C.sizeof(_lib.GroupAggOpts)
        self._check(self.L.hmj_group_agg_device(self.h, src, len(aggs), n_rows, dst, C.byref(opts)))
        del keep
        if int(opts.n_groups) != n_groups:
            raise RuntimeError("the live grouping has %d groups, the executor sized the outputs for %d: group through this "
                               "executor's group_cols_device / group_mixed_device" % (int(opts.n_groups), n_groups))
        info = {"n_groups": int(opts.n_groups), "ms_agg": float(opts.ms_agg)}
        return [(outs[k], words[k], int(dst[k].null_count)) for k in range(len(aggs))], info

    # ---- ORDER BY: typed, string and mixed keys to a row map (hmj_order_by_device) ---------------------------
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
        cols = [tuple(c) for c in cols]
        if n is None and cols:
            first = cols[0][0]
            n = first[1].shape[0] - 1 if isinstance(first, (tuple, list)) else first.shape[0]
        n = int(n or 0)
        arr = (_lib.OrderCol * max(len(cols), 1))()
        keep = []
        for k, c in enumerate(cols):
            col, flags = c[0], int(c[1]) if len(c) > 1 else 0
            v = c[2] if len(c) > 2 else None
            off = int(c[3]) if len(c) > 3 else 0
            if isinstance(col, (tuple, list)):
                chars, offsets = col
                _check_col(offsets, "column %d: offsets" % k)
                arr[k].type = _lib.HMJ_ORDER_LARGE_STRING
                cp = _chars_ptr(chars)
                arr[k].data = cp.value if cp is not None else None
                arr[k].offsets = offsets.data_ptr()
                keep += [chars, offsets]
            else:
                if not col.is_cuda or not col.is_contiguous() or col.dim() != 1:
                    raise ValueError("column %d must be a contiguous 1-D device tensor" % k)
                arr[k].type = self._agg_type(col)
                arr[k].data = col.data_ptr() if col.shape[0] else None
                keep.append(col)
            arr[k].flags = flags & 0xFFFFFFFF
            if v is not None:
                if not v.is_cuda or not v.is_contiguous() or v.dim() != 1:
                    raise ValueError("column %d: valid must be a contiguous 1-D device tensor" % k)
                if off < 0:
                    raise ValueError("column %d: bit_offset must not be negative" % k)
                arr[k].validity.bits = v.data_ptr() if v.shape[0] else None
                arr[k].validity.bit_offset = off & 0xFFFFFFFFFFFFFFFF
                keep.append(v)
        out = torch.empty(n, dtype=torch.int64, device="cuda:%d" % self.device)
        opts = _lib.OrderOpts()
        opts.struct_size = C.sizeof(_lib.OrderOpts)
        self._check(self.L.hmj_order_by_device(self.h, arr, len(cols), n, out.data_ptr() if n else None, C.byref(opts)))
        del keep
        info = {"n_distinct": int(opts.n_distinct), "n_tied_rows": int(opts.n_tied_rows), "n_rounds": int(opts.n_rounds)}
        for k in ("ms_key", "ms_sort", "ms_refine", "ms_map"):
            info[k] = float(getattr(opts, k))
        return out, info

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
        names = ("int8", "int16", "int32", "int64", "uint8", "uint16", "uint32", "uint64", "float32", "float64")
        first_n = None
        for k, t in enumerate(terms):
            col, op = t["column"], int(t["op"])
            lit = t.get("lit")
            lits = [] if lit is None else (list(lit) if isinstance(lit, (tuple, list)) else [lit])
            if len(lits) > 2:
                raise ValueError("term %d: at most two literals" % k)
            rm = t.get("row_map")
            if rm is None:
                map_n = None
            elif isinstance(rm, tuple):
                arr[k].row_map, map_n = int(rm[0] or 0) or None, int(rm[1])
            else:
                if not rm.is_cuda or not rm.is_contiguous() or rm.dim() != 1 or rm.dtype != torch.int64:
                    raise ValueError("term %d: row_map must be a contiguous 1-D int64 device tensor" % k)
                arr[k].row_map, map_n = (rm.data_ptr() if rm.shape[0] else None), rm.shape[0]
                keep.append(rm)
            if isinstance(col, (tuple, list)):
                chars, offsets = col
                _check_col(offsets, "term %d: offsets" % k)
                if offsets.shape[0] < 1:
                    raise ValueError("term %d: offsets must hold n + 1 entries" % k)
                arr[k].type = _lib.HMJ_FILTER_LARGE_STRING
                cp = _chars_ptr(chars)
                arr[k].data = cp.value if cp is not None else None
                arr[k].chars_bytes = chars.numel() if cp is not None else 0
                arr[k].offsets = offsets.data_ptr()
                n_src = offsets.shape[0] - 1
                keep += [chars, offsets]
                for j, v in enumerate(lits):
                    b = v.encode("utf-8") if isinstance(v, str) else bytes(v)
                    buf = C.create_string_buffer(b, max(len(b), 1))
                    arr[k].str_lit[j] = C.addressof(buf) if b else None
                    arr[k].str_len[j] = len(b)
                    keep.append(buf)
            else:
                if not col.is_cuda or not col.is_contiguous() or col.dim() != 1:
                    raise ValueError("term %d: the column must be a contiguous 1-D device tensor" % k)
                code = self._agg_type(col)
                arr[k].type = code
                arr[k].data = col.data_ptr() if col.shape[0] else None
                n_src = col.shape[0]
                keep.append(col)
                dt = np.dtype(names[code])
                for j, v in enumerate(lits):
                    arr[k].lit[j] = int(np.array([v], dtype=dt).view("u%d" % dt.itemsize)[0])
            arr[k].n_src = n_src
            arr[k].op = op & 0xFFFFFFFF
            arr[k].flags = _lib.HMJ_FILTER_NOT if t.get("negate") else 0
            arr[k].clause = int(t.get("clause") or 0)
            v, off = t.get("valid"), int(t.get("bit_offset") or 0)
            if v is not None:
                if not v.is_cuda or not v.is_contiguous() or v.dim() != 1:
                    raise ValueError("term %d: valid must be a contiguous 1-D device tensor" % k)
                if off < 0:
                    raise ValueError("term %d: bit_offset must not be negative" % k)
                arr[k].validity.bits = v.data_ptr() if v.shape[0] else None
                arr[k].validity.bit_offset = off & 0xFFFFFFFFFFFFFFFF
                keep.append(v)
            if first_n is None:
                first_n = n_src if map_n is None else map_n
        n = int((first_n or 0) if n is None else n)
        dev = "cuda:%d" % self.device
        if out is None:
            out = torch.empty(n, dtype=torch.int64, device=dev)
        elif not out.is_cuda or not out.is_contiguous() or out.dim() != 1 or out.dtype != torch.int64 or out.shape[0] < n:
            raise ValueError("out must be a contiguous 1-D int64 device tensor of at least n entries")
        words = torch.empty((n + 63) // 64, dtype=torch.int64, device=dev) if want_mask else None
        opts = _lib.FilterOpts()
        opts.struct_size = C.sizeof(_lib.FilterOpts)
        self._check(self.L.hmj_filter_device(self.h, arr, len(terms), n, out.data_ptr() if n else None,
                                             words.data_ptr() if (words is not None and n) else None, C.byref(opts)))
        del keep
        info = {"n_out": int(opts.n_out), "n_unknown": int(opts.n_unknown), "ms_eval": float(opts.ms_eval),
                "ms_write": float(opts.ms_write)}
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
        if isinstance(row_map, tuple):
            map_ptr, map_n = int(row_map[0] or 0), int(row_map[1])
        else:
            if not row_map.is_cuda or not row_map.is_contiguous() or row_map.dim() != 1 or row_map.dtype != torch.int64:
                raise ValueError("row_map must be a contiguous 1-D int64 device tensor")
            map_ptr, map_n = (row_map.data_ptr() if row_map.shape[0] else 0), row_map.shape[0]
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
        if valid is not None and len(list(valid)) != len(cols):
            raise ValueError("valid: one entry per column")
        wants = [bool(want_validity)] * len(cols) if isinstance(want_validity, (bool, int)) else [bool(w) for w in want_validity]
        if len(wants) != len(cols):
            raise ValueError("want_validity: one entry per column")
        dev = "cuda:%d" % self.device
        src = (_lib.TakeSrc * max(len(cols), 1))()
        dst = (_lib.TakeDst * max(len(cols), 1))()
        outs, words, keep = [], [], []
        for k, t in enumerate(cols):
            src[k].data = t.data_ptr() if n_src else None
            src[k].width = widths[k]
            v = None if valid is None else list(valid)[k]
            if v is not None:
                b, off = v if isinstance(v, tuple) else (v, 0)
                off = int(off)
                if not b.is_cuda or not b.is_contiguous() or b.dim() != 1 or b.element_size() != 1:
                    raise ValueError("valid[%d] must be a contiguous 1-D uint8 device tensor" % k)
                if off < 0:
                    raise ValueError("valid[%d]: bit_offset must not be negative" % k)
                if off + n_src < (1 << 64) and b.shape[0] * 8 < off + n_src:  # (an overflowing offset is the library's to reject)
                    raise ValueError("valid[%d] holds fewer than bit_offset + n bits" % k)
                src[k].validity.bits = b.data_ptr() if b.shape[0] else None
                src[k].validity.bit_offset = off & 0xFFFFFFFFFFFFFFFF
                keep.append(b)
            o = torch.empty((n_out,) + tuple(t.shape[1:]), dtype=t.dtype, device=dev)
            w = torch.empty((n_out + 63) // 64, dtype=torch.int64, device=dev) if wants[k] else None
            dst[k].data = o.data_ptr() if n_out else None
            dst[k].validity = w.data_ptr() if (w is not None and n_out) else None
            outs.append(o)
            words.append(w)
        opts = _lib.TakeOpts()
        opts.struct_size = C.sizeof(_lib.TakeOpts)
        self._check(self.L.hmj_take_cols_device(self.h, src, len(cols), n_src, C.c_void_p(map_ptr or None), n_out, dst, C.byref(opts)))
        del keep
        info = {"null_count": [int(dst[k].null_count) for k in range(len(cols))], "n_no_row": int(opts.n_no_row),
                "ms_take": float(opts.ms_take)}
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
        if isinstance(row_map, tuple):
            map_ptr, map_n = int(row_map[0] or 0), int(row_map[1])
        else:
            if not row_map.is_cuda or not row_map.is_contiguous() or row_map.dim() != 1 or row_map.dtype != torch.int64:
                raise ValueError("row_map must be a contiguous 1-D int64 device tensor")
            map_ptr, map_n = (row_map.data_ptr() if row_map.shape[0] else 0), row_map.shape[0]
        n_out = map_n if n_out is None else int(n_out)
        if not 0 <= n_out <= map_n:
            raise ValueError("n_out must be in 0..len(row_map)")
        _check_col(offsets, "offsets")
        if offsets.shape[0] < 1:
            raise ValueError("offsets must hold n + 1 entries")
        n_src = offsets.shape[0] - 1
        src = _lib.TakeStrSrc()
        cp = _chars_ptr(chars)
        src.chars = cp.value if cp is not None else None
        src.chars_bytes = chars.numel() if cp is not None else 0
        src.offsets = offsets.data_ptr()
        keep = self._str_validity(valid, n_src, "valid", src.validity)
        dev = "cuda:%d" % self.device
        off_out = torch.zeros(n_out + 1, dtype=torch.int64, device=dev)  # (n_out == 0 writes nothing: offsets[0] = 0 is ours)
        words = torch.empty((n_out + 63) // 64, dtype=torch.int64, device=dev) if want_validity else None
        dst = _lib.TakeStrDst()
        dst.offsets = off_out.data_ptr()
        dst.validity = words.data_ptr() if (words is not None and n_out) else None
        opts = _lib.TakeStrOpts()
        opts.struct_size = C.sizeof(_lib.TakeStrOpts)

        def call():
            self._check(self.L.hmj_take_str_device(self.h, C.byref(src), n_src, C.c_void_p(map_ptr or None), n_out, C.byref(dst),
                                                   C.byref(opts)))

        if capacity is None:
            call()  # the sizing call
            capacity = int(dst.total_bytes)
        capacity = int(capacity)
        chars_out = torch.empty(max(capacity, 1), dtype=torch.uint8, device=dev)  # (never a NULL pointer: that is the sizing call)
        dst.chars = chars_out.data_ptr()
        dst.chars_capacity = capacity
        call()
        del keep
        total = int(dst.total_bytes)
        info = {"null_count": int(dst.null_count), "n_no_row": int(opts.n_no_row), "total_bytes": total,
                "ms_offsets": float(opts.ms_offsets), "ms_chars": float(opts.ms_chars)}
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
        n = int(res.n_matches)
        out = np.empty((n, 3), np.uint64)
        if n == 0 or not res.key:
            return out[:0] if not res.key else out
        if host:
            for c, ptr in enumerate((res.key, res.rval, res.sval)):
                out[:, c] = np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_uint64)), shape=(n,))
        else:
            torch = self._torch
            tmp = torch.empty(n, dtype=torch.int64, device="cuda:%d" % self.device)
            for c, ptr in enumerate((res.key, res.rval, res.sval)):
                _memcpy_d2d(torch, tmp, ptr, n * 8)
                out[:, c] = tmp.cpu().numpy().view(np.uint64)
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
        bp, nb = _dev_ptr(build_shard)
        pp, np_ = _dev_ptr(probe_shard)
        loc, glob = JoinResult(), JoinResult()
        self._check(self.L.hmj_exchange_join_u64_device(self.h, C.c_void_p(bp), nb, C.c_void_p(pp), np_, flags,
                                                        C.byref(loc), C.byref(glob)))
        return loc, glob

    def exchange_join_kind(self, build_shard, probe_shard, side, kind, flags=0, probe_fill=0, build_fill=0):
        """Distributed join kind of row shards (collective; hmj_exchange_join_kind_u64_device).  side = HMJ_KIND_PROBE_SIDE
        (kind HMJ_JOIN_*) or HMJ_KIND_BUILD_SIDE (kind HMJ_BUILD_* / HMJ_FULL_OUTER).  Returns (local JoinResult, global
        JoinResult, {"local": counters, "global": counters}) with the counters of hmj_kind_counts.  The local columns are
        read as those of the single-GPU kind: `probe_rows_to_numpy`, `build_rows_to_numpy` or `columns_to_numpy`."""
        self._sync_stream()
        bp, nb = _dev_ptr(build_shard)
        pp, np_ = _dev_ptr(probe_shard)
        loc, glob = JoinResult(), JoinResult()
        opts = _lib.ExchangeKindOpts()
        opts.struct_size = C.sizeof(_lib.ExchangeKindOpts)
        opts.side = int(side)
        opts.kind = int(kind)
        opts.probe_fill = int(probe_fill) & 0xFFFFFFFFFFFFFFFF
        opts.build_fill = int(build_fill) & 0xFFFFFFFFFFFFFFFF
        self._check(self.L.hmj_exchange_join_kind_u64_device(self.h, C.c_void_p(bp), nb, C.c_void_p(pp), np_, flags,
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
        opts = _lib.StrKindOpts()
        opts.struct_size = C.sizeof(_lib.StrKindOpts)
        opts.side = int(side)
        opts.kind = int(kind)
        opts.hash_bits = int(hash_bits)
        opts.probe_fill = int(probe_fill) & 0xFFFFFFFFFFFFFFFF
        opts.build_fill = int(build_fill) & 0xFFFFFFFFFFFFFFFF
        keep = (self._str_validity(build_valid, int(rb.n), "build_valid", opts.build_validity),
                self._str_validity(probe_valid, int(rp.n), "probe_valid", opts.probe_validity))
        res = _lib.StrResult()
        self._check(self.L.hmj_join_kind_str_device(self.h, C.byref(rb), C.byref(rp), flags, C.byref(opts), C.byref(res)))
        del keep
        info = opts.counts.as_dict()
        info["n_hash_pairs"] = int(opts.n_hash_pairs)
        info["n_collisions"] = int(opts.n_collisions)
        info["n_build_null"] = int(opts.n_build_null)
        info["n_probe_null"] = int(opts.n_probe_null)
        for k in ("ms_hash", "ms_join", "ms_verify", "ms_emit", "ms_order"):
            info[k] = float(getattr(opts, k))
        return res, info

    def str_kind_rows_to_numpy(self, res):
        """Copy a string kind join's device result out as an [n,5] uint64 array of (hash, r_row, s_row, rval, sval); a
        column the kind does not produce reads as HMJ_STR_NO_ROW (row columns) or 0 (value columns)."""
        n = int(res.n_matches)
        out = np.empty((n, 5), np.uint64)
        if n == 0 or not res.hash:
            return out[:0]
        torch = self._torch
        tmp = torch.empty(n, dtype=torch.int64, device="cuda:%d" % self.device)
        for c, ptr in enumerate((res.hash, res.r_row, res.s_row, res.rval, res.sval)):
            if not ptr:
                out[:, c] = _lib.HMJ_STR_NO_ROW if c in (1, 2) else 0
                continue
            _memcpy_d2d(torch, tmp, ptr, n * 8)
            out[:, c] = tmp.cpu().numpy().view(np.uint64)
        return out


def _check_col(t, name):
    """A column the string entries read on the device: contiguous, 1-D, 64-bit, on the GPU."""
    if not t.is_cuda or not t.is_contiguous() or t.element_size() != 8 or t.dim() != 1:
        raise ValueError("%s must be a contiguous 1-D 64-bit device tensor" % name)


def _chars_ptr(chars):
    if chars is None or chars.numel() == 0:
        return None
    if not chars.is_cuda or not chars.is_contiguous() or chars.element_size() != 1:
        raise ValueError("chars must be a contiguous 1-byte device tensor")
    return C.c_void_p(chars.data_ptr())


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


def _mix64(x):
    x = x ^ (x >> np.uint64(30))
    x = x * np.uint64(0xBF58476D1CE4E5B9)
    x = x ^ (x >> np.uint64(27))
    x = x * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def _null_masks(valid, k, n):
    """`valid` of cols_key64 / mixed_key64 -> one bool array [n] per column, True = NULL."""
    if valid is None:
        return [np.zeros(n, bool) for _ in range(k)]
    valid = list(valid)
    if len(valid) != k:
        raise ValueError("valid: one entry per key column")
    out = []
    for v in valid:
        m = np.zeros(n, bool) if v is None else ~np.asarray(v, bool).ravel()
        if len(m) != n:
            raise ValueError("valid: one entry per row")
        out.append(m)
    return out


def _null_equal_chain(vs, nulls, hash_bits):
    """key64 under HMJ_NULL_EQUAL: the hash chain with v_c = 0 under a NULL slot, then -- rows with a NULL slot only -- one
    more step over m = the sum of 2^c over the row's NULL columns."""
    n = len(vs[0])
    h = np.full(n, len(vs), np.uint64)
    m = np.zeros(n, np.uint64)
    with np.errstate(over="ignore"):
        for c, (v, nl) in enumerate(zip(vs, nulls)):
            h = _mix64(h + np.where(nl, np.uint64(0), v) + np.uint64(0x9E3779B97F4A7C15))
            m = m | np.where(nl, np.uint64(1 << c), np.uint64(0))
        h = np.where(m != 0, _mix64(h + m + np.uint64(0x9E3779B97F4A7C15)), h)
    return h >> np.uint64(64 - int(hash_bits)) if hash_bits else h


def cols_key64(columns, widths, hash_bits=0, force_hashed=False, valid=None, null_equal=False):
    """The 64-bit join key hmj_join_cols_device gives every row (include/hmj.h), restated on the host: uint64 array [n].
    columns: one numpy array per key column (any dtype of widths[c] bytes, or integers that fit it); widths: bytes per
    column (1, 2, 4 or 8).  Packed form (widths sum to <= 8, not force_hashed): the columns concatenated, column 0 most
    significant.  Hashed form: h = k; h = mix64(h + v_c + 0x9E3779B97F4A7C15) per column; hash_bits 1..63 keeps the top bits.
    null_equal=True: the key of a HMJ_NULL_EQUAL call that passes a bitmap -- always the hashed form; valid: None, or one
    entry per column, None or n bools (True = valid); a NULL slot has v_c = 0 whatever lies under it, and a row with NULL
    slots takes one more step h = mix64(h + m + 0x9E3779B97F4A7C15), m = the sum of 2^c over its NULL columns.  Without
    null_equal, valid is not read (a NULL-key row of a SQL-semantics call has key64 0 where it is emitted)."""
    widths = [int(w) for w in widths]
    if len(columns) != len(widths) or not 1 <= len(widths) <= _lib.HMJ_MAX_KEY_COLS:
        raise ValueError("1..%d columns, one width each" % _lib.HMJ_MAX_KEY_COLS)
    if any(w not in (1, 2, 4, 8) for w in widths):
        raise ValueError("widths must be 1, 2, 4 or 8")
    if not 0 <= int(hash_bits) <= 63:
        raise ValueError("hash_bits must be in 0..63")
    vs = []
    for col, w in zip(columns, widths):
        a = np.ascontiguousarray(col)
        if a.dtype.itemsize == w and a.dtype.kind != "u":
            a = a.view("u%d" % w)  # signed integers and floats: their bytes
        vs.append(a.astype(np.uint64) & np.uint64((1 << (8 * w)) - 1))
    n = len(vs[0])
    if null_equal:
        return _null_equal_chain(vs, _null_masks(valid, len(vs), n), hash_bits)
    if sum(widths) <= 8 and not force_hashed:
        key = np.zeros(n, np.uint64)
        for v, w in zip(vs, widths):
            key = v if w == 8 else ((key << np.uint64(8 * w)) | v)
        return key
    h = np.full(n, len(widths), np.uint64)
    for v in vs:
        h = _mix64(h + v + np.uint64(0x9E3779B97F4A7C15))
    return h >> np.uint64(64 - int(hash_bits)) if hash_bits else h


def expected_groups(columns, widths, vals=None, valid=None, hash_bits=0, force_hashed=False, ordered=False):
    """What hmj_group_cols_device returns (include/hmj.h), restated on the host in plain numpy.  columns / widths as
    `cols_key64`; vals: n integers (taken mod 2^64) or None (the payload of row i is i); valid: None, or one entry per
    column, None or n bools (True = valid) -- an entry that is not None is a bitmap passed, which makes the form hashed
    even when every bit is set.  Two rows are one group when in every column both slots are NULL or both are valid and
    equal; what lies under a NULL slot is not read.  Returns a dict: "form", "n_groups", "n_rows", "max_count", "n_null",
    "n_collisions" (groups minus distinct key64), "max_mixed_run" (rows of the largest run of equal key64 that holds
    several tuples: the call is HMJ_E_UNSUPPORTED beyond 1024), the uint64 group columns "key64", "first_row", "count",
    "sum", "min", "max", and "group_of_row" [n].  ordered: groups ascending by (key64, the tuple column by column as
    unsigned integers, NULLS LAST per column) as HMJ_ORDERED gives them; else ascending by first_row, the order in which
    an unordered result is compared."""
    widths = [int(w) for w in widths]
    k = len(widths)
    n = len(np.ascontiguousarray(columns[0])) if k else 0
    bitmap = valid is not None and any(v is not None for v in valid)
    nulls = _null_masks(valid, k, n)
    hashed = bitmap or sum(widths) > 8 or bool(force_hashed)
    if bitmap:
        key64 = cols_key64(columns, widths, hash_bits, valid=valid, null_equal=True)
    else:
        key64 = cols_key64(columns, widths, hash_bits, force_hashed)
    # the tuple as the order and the grouping rule see it: per column (is NULL, value or 0 under a NULL slot)
    canon = np.zeros((n, 2 * k), np.uint64)
    for c, (col, w) in enumerate(zip(columns, widths)):
        a = np.ascontiguousarray(col)
        if a.dtype.itemsize == w and a.dtype.kind != "u":
            a = a.view("u%d" % w)
        v = a.astype(np.uint64) & np.uint64((1 << (8 * w)) - 1)
        canon[:, 2 * c] = nulls[c]
        canon[:, 2 * c + 1] = np.where(nulls[c], np.uint64(0), v)
    return _group_table(canon, key64, _group_payloads(vals, n), nulls, hashed, ordered)


def _group_payloads(vals, n):
    """`vals` of expected_groups / expected_mixed_groups -> the n payloads as uint64."""
    if vals is None:
        return np.arange(n, dtype=np.uint64)
    pay = np.asarray(vals)
    if pay.dtype.kind == "i":
        pay = pay.astype(np.int64).view(np.uint64)
    elif pay.dtype.kind == "u":
        pay = pay.astype(np.uint64)
    else:  # Python integers beyond int64
        pay = np.array([int(x) & 0xFFFFFFFFFFFFFFFF for x in pay.ravel()], np.uint64)
    if len(pay) != n:
        raise ValueError("vals: one payload per row")
    return pay


def _group_table(canon, key64, pay, nulls, hashed, ordered):
    """The result dict of expected_groups / expected_mixed_groups from the canonical tuples: canon [n, 2k] uint64, per
    column (is NULL, a number that orders and equals as the column's values do, 0 under a NULL slot)."""
    n, k = canon.shape[0], canon.shape[1] // 2
    out = {"form": _lib.HMJ_COLS_HASHED if hashed else _lib.HMJ_COLS_PACKED, "n_rows": n,
           "n_null": int(np.count_nonzero(np.any(np.stack(nulls), axis=0))) if k and n else 0}
    empty = np.zeros(0, np.uint64)
    if n == 0:
        out.update({"n_groups": 0, "max_count": 0, "n_collisions": 0, "max_mixed_run": 0, "group_of_row": empty})
        out.update({name: empty for name in ("key64", "first_row", "count", "sum", "min", "max")})
        return out
    # groups in tuple order (numpy.unique sorts rows lexicographically; return_index: the first, i.e. smallest, row)
    _, first, inv, count = np.unique(canon, axis=0, return_index=True, return_inverse=True, return_counts=True)
    inv = inv.reshape(-1)
    gkey = key64[first]
    order = np.lexsort((np.arange(len(first)), gkey)) if ordered else np.argsort(first, kind="stable")
    rank = np.empty(len(first), np.int64)
    rank[order] = np.arange(len(first))
    group_of_row = rank[inv]
    by_group = np.argsort(group_of_row, kind="stable")
    starts = np.concatenate([[0], np.cumsum(count[order])[:-1]]).astype(np.int64)
    sorted_pay = pay[by_group]
    with np.errstate(over="ignore"):
        gsum = np.add.reduceat(sorted_pay, starts)
    ukey, kinv = np.unique(key64, return_inverse=True)
    tuples_per_key = np.bincount(kinv.reshape(-1)[first], minlength=len(ukey))
    rows_per_key = np.bincount(kinv.reshape(-1), minlength=len(ukey))
    mixed = rows_per_key[tuples_per_key > 1]
    out.update({"n_groups": len(first), "max_count": int(count.max()), "n_collisions": int(len(first) - len(ukey)),
                "max_mixed_run": int(mixed.max()) if len(mixed) else 0,
                "key64": gkey[order], "first_row": first[order].astype(np.uint64), "count": count[order].astype(np.uint64),
                "sum": gsum.astype(np.uint64), "min": np.minimum.reduceat(sorted_pay, starts),
                "max": np.maximum.reduceat(sorted_pay, starts), "group_of_row": group_of_row.astype(np.uint64)})
    return out


def _float_order_keys(a):
    """Floats (float32 / float64) -> (unsigned keys whose integer order is IEEE order with -0.0 < +0.0, is-NaN mask)."""
    bits = a.view("u%d" % a.dtype.itemsize)
    top = bits.dtype.type(1 << (8 * a.dtype.itemsize - 1))
    keys = np.where(bits & top, ~bits, bits | top)
    return keys, (bits & ~top) > (bits.dtype.type(0x7F800000) if a.dtype.itemsize == 4 else bits.dtype.type(0x7FF0000000000000))


def expected_group_aggs(group_of_row, n_groups, aggs):
    """What hmj_group_agg_device returns (include/hmj.h), restated on the host from group_of_row alone -- no key logic.
    group_of_row: n integers in 0..n_groups-1; aggs: a list of (op, values, valid): op an HMJ_AGG_* code, values a numpy
    array of n integers or floats of the column's dtype (None for HMJ_AGG_COUNT), valid None or n bools (True = valid).
    What lies under a NULL slot is not read.  Returns one dict per aggregate: "values" (n_groups entries of the output
    dtype: COUNT uint64, SUM int64 / uint64 / float64, MIN / MAX the source dtype, MEAN float64; 0 in a NULL slot),
    "valid" (n_groups bools), "null_count", "count" (the valid values per group, int64) and "abs_sum" (float64: the sum of
    |x| over the group's valid values for float SUM and for MEAN, each x converted to double; None otherwise).  Float sums
    are math.fsum per group, i.e. correctly rounded: the device's differ from them by at most gamma_k * abs_sum."""
    import math

    gmap = np.asarray(group_of_row).astype(np.int64).ravel()
    n, ng = len(gmap), int(n_groups)
    if n and (gmap.min() < 0 or gmap.max() >= ng):
        raise ValueError("group_of_row: entries must be in 0..n_groups-1")
    out = []
    for op, vals, valid in [tuple(a)[:3] if len(tuple(a)) > 2 else tuple(a) + (None,) for a in aggs]:
        op = int(op)
        ok = np.ones(n, bool) if valid is None else np.asarray(valid, bool).ravel()
        if len(ok) != n:
            raise ValueError("valid: one entry per row")
        count = np.bincount(gmap[ok], minlength=ng).astype(np.int64)
        res = {"count": count, "abs_sum": None}
        if op == _lib.HMJ_AGG_COUNT:
            res.update({"values": count.astype(np.uint64), "valid": np.ones(ng, bool)})
        else:
            a = np.ascontiguousarray(vals).ravel()
            if len(a) != n or a.dtype.kind not in "iuf" or a.dtype.itemsize > 8 or a.dtype == np.float16:
                raise ValueError("values: n integers or floats of 1 to 8 bytes")
            g, x = gmap[ok], a[ok]
            is_float = a.dtype.kind == "f"
            if op == _lib.HMJ_AGG_MEAN or (op == _lib.HMJ_AGG_SUM and is_float):
                xd = x.astype(np.float64)
                order = np.argsort(g, kind="stable")
                ends = np.cumsum(count)
                sums, abss = np.zeros(ng), np.zeros(ng)
                with np.errstate(all="ignore"):
                    for k in range(ng):
                        seg = xd[order[ends[k] - count[k]:ends[k]]]
                        try:
                            sums[k] = math.fsum(seg)
                        except (OverflowError, ValueError):  # an intermediate overflow, inf - inf: as IEEE addition has it
                            sums[k] = float(np.sum(seg))
                        abss[k] = float(np.sum(np.abs(seg)))
                    v = sums / np.maximum(count, 1) if op == _lib.HMJ_AGG_MEAN else sums
                res["abs_sum"] = abss
            elif op == _lib.HMJ_AGG_SUM:
                wide = x.astype(np.int64).view(np.uint64) if a.dtype.kind == "i" else x.astype(np.uint64)
                acc = np.zeros(ng, np.uint64)
                np.add.at(acc, g, wide)  # (wraps mod 2^64)
                v = acc.view(np.int64) if a.dtype.kind == "i" else acc
            elif op in (_lib.HMJ_AGG_MIN, _lib.HMJ_AGG_MAX):
                low = op == _lib.HMJ_AGG_MIN
                if is_float:
                    keys, nan = _float_order_keys(x)
                    ident = keys.dtype.type(np.iinfo(keys.dtype).max if low else 0)
                    acc = np.full(ng, ident, keys.dtype)
                    (np.minimum if low else np.maximum).at(acc, g[~nan], keys[~nan])
                    numbers = np.bincount(g[~nan], minlength=ng) > 0
                    top = keys.dtype.type(1 << (8 * a.dtype.itemsize - 1))
                    v = np.where(acc & top, acc ^ top, ~acc).view(a.dtype).copy()
                    v[~numbers] = np.nan  # (numpy's default NaN is the canonical quiet one)
                else:
                    info = np.iinfo(a.dtype)
                    acc = np.full(ng, info.max if low else info.min, a.dtype)
                    (np.minimum if low else np.maximum).at(acc, g, x)
                    v = acc
            else:
                raise ValueError("unknown op %d" % op)
            v = np.array(v)
            v[count == 0] = 0
            res.update({"values": v, "valid": count > 0})
        res["null_count"] = int(ng - np.count_nonzero(res["valid"]))
        out.append(res)
    return out


def _order_columns(columns):
    """(values, flags[, valid]) per column -> [(values, flags, valid bools or None, is_string)], n.  values: a numpy array
    of an integer or float dtype, or a list of bytes / str (None where the slot is NULL counts as NULL too)."""
    out, n = [], None
    for c in columns:
        c = tuple(c)
        vals, flags = c[0], int(c[1]) if len(c) > 1 else 0
        valid = None if len(c) < 3 or c[2] is None else np.asarray(c[2], bool).ravel()
        is_str = not isinstance(vals, np.ndarray)
        if is_str:
            vals = [None if v is None else (v.encode("utf-8") if isinstance(v, str) else bytes(v)) for v in vals]
            if any(v is None for v in vals):
                holes = np.array([v is not None for v in vals], bool)
                valid = holes if valid is None else (valid & holes)
        if n is None:
            n = len(vals)
        if len(vals) != n or (valid is not None and len(valid) != n):
            raise ValueError("every column and every valid mask must hold n rows")
        out.append((vals, flags, valid, is_str))
    return out, (n or 0)


def expected_order_by(columns):
    """The row map hmj_order_by_device returns (include/hmj.h), restated on the host from the order rule: columns is a list
    of (values, flags[, valid]) -- values a numpy array of an integer or float dtype, or a list of bytes (a string column);
    flags HMJ_ORDER_* bits; valid None or n bools (True = valid).  Per column every row gets the dense rank of its value
    among the column's valid values -- integers in their signedness, floats in IEEE order with -0.0 < +0.0 and every NaN one
    value above +inf, strings as Python orders bytes (unsigned bytes, then length) --, reversed under HMJ_ORDER_DESC; a NULL
    slot ranks behind all of them, or in front under HMJ_ORDER_NULLS_FIRST.  The map is the stable lexicographic order of
    the rank tuples (ties keep ascending row index).  What lies under a NULL slot is not read.  Returns n uint64."""
    cols, n = _order_columns(columns)
    ranks = []
    for vals, flags, valid, is_str in cols:
        ok = np.ones(n, bool) if valid is None else valid
        idx = np.nonzero(ok)[0]
        rank = np.zeros(n, np.int64)
        if is_str:
            picked = [vals[i] for i in idx]
            order = {v: k for k, v in enumerate(sorted(set(picked)))}
            r = np.fromiter((order[v] for v in picked), dtype=np.int64, count=len(picked))
            distinct = len(order)
        else:
            x = np.ascontiguousarray(vals[idx])
            if x.dtype.kind == "f":
                keys, nan = _float_order_keys(x)
                x = np.where(nan, ~keys.dtype.type(0), keys)  # (no number's key is all ones)
            uniq, r = np.unique(x, return_inverse=True)
            r = r.astype(np.int64).ravel()
            distinct = len(uniq)
        if flags & _lib.HMJ_ORDER_DESC:
            r = distinct - 1 - r
        rank[idx] = r
        rank[~ok] = -1 if flags & _lib.HMJ_ORDER_NULLS_FIRST else distinct
        ranks.append(rank)
    if n == 0:
        return np.zeros(0, np.uint64)
    return np.lexsort(ranks[::-1]).astype(np.uint64)  # (lexsort: the last key is the primary one; stable)


def order_stream_bytes(columns):
    """The length S of every row's order-preserving byte stream in hmj_order_by_device (include/hmj.h): per column one
    marker byte when the column has a validity mask, then the value's width for a fixed column, or 8 * max(1, ceil(len / 7))
    for a valid string and nothing for a NULL one.  hmj_order_opts.n_rounds is at most 1 + ceil(max(0, max S - 8) / 4).
    columns as `expected_order_by` takes them.  Returns n int64."""
    cols, n = _order_columns(columns)
    total = np.zeros(n, np.int64)
    for vals, _flags, valid, is_str in cols:
        if valid is not None:
            total += 1
        if is_str:
            ok = np.ones(n, bool) if valid is None else valid
            total += np.array([8 * max(1, -(-len(vals[i]) // 7)) if ok[i] else 0 for i in range(n)], np.int64).reshape(n)
        else:
            total += vals.dtype.itemsize
    return total


def expected_filter(terms, n):
    """What hmj_filter_device returns (include/hmj.h), restated on the host: terms as `Executor.filter_device` takes them
    (dicts, or tuples (column, op, lit, valid, bit_offset, row_map, clause, negate)) with host values -- column a numpy
    array of an integer or float dtype, or a list of bytes / str (None: a NULL slot); lit as there; valid None or one bool
    per ROW of the column (True = valid; bit_offset is not looked at); row_map None or n entries (uint64 or int64,
    HMJ_TAKE_NO_ROW / -1 a NULL slot).  Every term is numpy's own comparison operator on the column's dtype (C's operators:
    IEEE for floats) or Python's comparison of `bytes` (unsigned bytes, then length), made three-valued -- UNKNOWN on a NULL
    slot except for IS_NULL / IS_NOT_NULL, negation swapping TRUE and FALSE --; a clause is the maximum of its terms and the
    predicate the minimum of its clauses under FALSE < UNKNOWN < TRUE.  What lies under a NULL slot is not read.  Returns
    (the positions at which the predicate is TRUE, ascending, n uint64 at most; the number of UNKNOWN positions)."""
    keys = ("column", "op", "lit", "valid", "bit_offset", "row_map", "clause", "negate")
    F, U, T = 0, 1, 2
    n = int(n)
    pred = np.full(n, T, np.int8)
    cl, cl_id = None, None
    for k, t in enumerate(terms):
        t = t if isinstance(t, dict) else dict(zip(keys, t))
        vals, op = t["column"], int(t["op"])
        lit = t.get("lit")
        lits = [] if lit is None else (list(lit) if isinstance(lit, (tuple, list)) else [lit])
        is_str = not isinstance(vals, np.ndarray)
        n_src = len(vals)
        rm = t.get("row_map")
        if rm is None:
            if n_src < n:
                raise ValueError("term %d: n_src < n without a row_map" % k)
            have, rows = np.ones(n, bool), np.arange(n, dtype=np.int64)
        else:
            rm = np.asarray(rm).astype(np.uint64)[:n]
            if len(rm) != n:
                raise ValueError("term %d: row_map must hold n entries" % k)
            have = rm != np.uint64(_lib.HMJ_TAKE_NO_ROW)
            if np.any(have & (rm >= np.uint64(n_src))):
                raise ValueError("term %d: a row_map entry is >= n_src and not HMJ_TAKE_NO_ROW" % k)
            rows = np.where(have, rm, np.uint64(0)).astype(np.int64)
        ok = have.copy()
        valid = t.get("valid")
        if is_str:
            vals = [None if v is None else (v.encode("utf-8") if isinstance(v, str) else bytes(v)) for v in vals]
            holes = np.array([v is not None for v in vals], bool)
            valid = holes if valid is None else (np.asarray(valid, bool).ravel() & holes)
        if valid is not None:
            valid = np.asarray(valid, bool).ravel()
            if len(valid) != n_src:
                raise ValueError("term %d: valid must hold one entry per row of the column" % k)
            ok[have] = valid[rows[have]]
        if op == _lib.HMJ_FILTER_IS_NULL:
            v = np.where(ok, F, T)
        elif op == _lib.HMJ_FILTER_IS_NOT_NULL:
            v = np.where(ok, T, F)
        else:
            if len(lits) != (2 if op == _lib.HMJ_FILTER_BETWEEN else 1):
                raise ValueError("term %d: the op takes %d literal(s)" % (k, 2 if op == _lib.HMJ_FILTER_BETWEEN else 1))
            idx = np.nonzero(ok)[0]
            res = np.zeros(n, bool)
            if is_str:
                ls = [x.encode("utf-8") if isinstance(x, str) else bytes(x) for x in lits]
                fn = {_lib.HMJ_FILTER_EQ: lambda s: s == ls[0], _lib.HMJ_FILTER_NE: lambda s: s != ls[0],
                      _lib.HMJ_FILTER_LT: lambda s: s < ls[0], _lib.HMJ_FILTER_LE: lambda s: s <= ls[0],
                      _lib.HMJ_FILTER_GT: lambda s: s > ls[0], _lib.HMJ_FILTER_GE: lambda s: s >= ls[0],
                      _lib.HMJ_FILTER_BETWEEN: lambda s: ls[0] <= s and s <= ls[1],
                      _lib.HMJ_FILTER_STARTS_WITH: lambda s: s.startswith(ls[0]),
                      _lib.HMJ_FILTER_ENDS_WITH: lambda s: s.endswith(ls[0])}[op]
                res[idx] = [bool(fn(vals[r])) for r in rows[idx]]
            else:
                x = vals[rows[idx]]
                ls = [np.array([v], dtype=vals.dtype)[0] for v in lits]
                with np.errstate(invalid="ignore"):
                    if op == _lib.HMJ_FILTER_EQ:
                        r = x == ls[0]
                    elif op == _lib.HMJ_FILTER_NE:
                        r = x != ls[0]
                    elif op == _lib.HMJ_FILTER_LT:
                        r = x < ls[0]
                    elif op == _lib.HMJ_FILTER_LE:
                        r = x <= ls[0]
                    elif op == _lib.HMJ_FILTER_GT:
                        r = x > ls[0]
                    elif op == _lib.HMJ_FILTER_GE:
                        r = x >= ls[0]
                    elif op == _lib.HMJ_FILTER_BETWEEN:
                        r = (ls[0] <= x) & (x <= ls[1])
                    else:
                        raise ValueError("term %d: op %d does not apply to a fixed-width column" % (k, op))
                res[idx] = r
            v = np.where(ok, np.where(res, T, F), U)
        v = v.astype(np.int8)
        if t.get("negate"):
            v = (T - v).astype(np.int8)
        cid = int(t.get("clause") or 0)
        if cl is not None and cid != cl_id:
            if cid < cl_id:
                raise ValueError("term %d: clause ids must not decrease" % k)
            pred = np.minimum(pred, cl)
            cl = None
        cl, cl_id = (v if cl is None else np.maximum(cl, v)), cid
    if cl is not None:
        pred = np.minimum(pred, cl)
    return np.nonzero(pred == T)[0].astype(np.uint64), int(np.count_nonzero(pred == U))


def _hash_bytes(b):
    """libstdc++'s _Hash_bytes (64-bit size_t, seed 0xc70f6907): std::hash<std::string> of the bytes b."""
    M, mask = 0xc6a4a7935bd1e995, 0xFFFFFFFFFFFFFFFF
    n = len(b)
    h = (0xc70f6907 ^ (n * M)) & mask
    for k in range(0, n & ~7, 8):
        d = (int.from_bytes(b[k:k + 8], "little") * M) & mask
        d = ((d ^ (d >> 47)) * M) & mask
        h = ((h ^ d) * M) & mask
    if n & 7:
        h = ((h ^ int.from_bytes(b[n & ~7:], "little")) * M) & mask
    h = ((h ^ (h >> 47)) * M) & mask
    return h ^ (h >> 47)


def mixed_key64(columns, hash_bits=0, valid=None, null_equal=False):
    """The 64-bit join key hmj_join_mixed_device gives every row (include/hmj.h), restated on the host: uint64 array [n].
    columns: one entry per key column -- a numpy integer array (a fixed-width column: its values zero-extended from the
    dtype's width) or a list of `bytes` (a string column: libstdc++'s _Hash_bytes of every slot, all 64 bits).
    h = k; h = mix64(h + v_c + 0x9E3779B97F4A7C15) per column; hash_bits 1..63 keeps the top bits.  valid / null_equal as
    for `cols_key64`: under HMJ_NULL_EQUAL a NULL slot has v_c = 0 (a NULL string slot may hold None), and a row with NULL
    slots takes the extra step over its NULL columns' mask."""
    if not 1 <= len(columns) <= _lib.HMJ_MAX_KEY_COLS:
        raise ValueError("1..%d columns" % _lib.HMJ_MAX_KEY_COLS)
    if not 0 <= int(hash_bits) <= 63:
        raise ValueError("hash_bits must be in 0..63")
    vs = []
    for col in columns:
        if isinstance(col, np.ndarray):
            a = np.ascontiguousarray(col)
            if a.dtype.itemsize not in (1, 2, 4, 8):
                raise ValueError("a fixed-width column has 1, 2, 4 or 8 bytes per value")
            vs.append(a.view("u%d" % a.dtype.itemsize).astype(np.uint64))
        else:
            vs.append(np.array([0 if b is None else _hash_bytes(bytes(b)) for b in col], np.uint64))
    if any(len(v) != len(vs[0]) for v in vs):
        raise ValueError("columns must have one length")
    if null_equal:
        return _null_equal_chain(vs, _null_masks(valid, len(vs), len(vs[0])), hash_bits)
    h = np.full(len(vs[0]), len(vs), np.uint64)
    with np.errstate(over="ignore"):
        for v in vs:
            h = _mix64(h + v + np.uint64(0x9E3779B97F4A7C15))
    return h >> np.uint64(64 - int(hash_bits)) if hash_bits else h


def expected_mixed_groups(columns, vals=None, valid=None, hash_bits=0, ordered=False):
    """What hmj_group_mixed_device returns (include/hmj.h), restated on the host.  columns as `mixed_key64` takes them: a
    numpy integer array per fixed-width column, a list of `bytes` per string column (None is fine under a NULL slot);
    vals / valid / ordered as for `expected_groups`.  The form is always hashed and key64 is `mixed_key64(columns,
    hash_bits, valid, null_equal=True)`.  Two rows are one group when in every column both slots are NULL or both are
    valid and equal (strings: length and bytes; a NULL string is not the empty string); what lies under a NULL slot is not
    read.  Returns `expected_groups`' dict, "max_mixed_run" included.  ordered: ascending by (key64, the tuple column by
    column, NULLS LAST per column): fixed columns as unsigned integers, strings as Python orders `bytes`, which is
    std::string::operator<."""
    k = len(columns)
    n = len(columns[0]) if k else 0
    nulls = _null_masks(valid, k, n)
    key64 = mixed_key64(columns, hash_bits, valid, null_equal=True) if k else np.zeros(0, np.uint64)
    canon = np.zeros((n, 2 * k), np.uint64)
    for c, col in enumerate(columns):
        if isinstance(col, np.ndarray):
            a = np.ascontiguousarray(col)
            v = a.view("u%d" % a.dtype.itemsize).astype(np.uint64)
        else:  # a string's number: its rank among the column's distinct valid strings in bytes order
            slots = [b"" if (nulls[c][i] or b is None) else bytes(b) for i, b in enumerate(col)]
            rank = {b: r for r, b in enumerate(sorted(set(slots)))}
            v = np.array([rank[b] for b in slots], np.uint64)
        canon[:, 2 * c] = nulls[c]
        canon[:, 2 * c + 1] = np.where(nulls[c], np.uint64(0), v)
    return _group_table(canon, key64, _group_payloads(vals, n), nulls, True, ordered)


def _memcpy_d2d(torch, dst_tensor, src_ptr, nbytes):
    """Copy nbytes from a raw device pointer into a torch tensor (plumbing only)."""
    hip = C.CDLL(None)  # the HIP runtime torch already loaded
    fn = getattr(hip, "hipMemcpy", None)
    if fn is None:
        import ctypes.util

        hip = C.CDLL("libamdhip64.so")
        fn = hip.hipMemcpy
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    torch.cuda.synchronize()
    rc = fn(C.c_void_p(dst_tensor.data_ptr()), C.c_void_p(src_ptr), nbytes, 3)  # hipMemcpyDeviceToDevice
    if rc:
        raise HmjError(-4, "hipMemcpy d2d failed: %d" % rc)


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
