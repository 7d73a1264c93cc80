"""What the column entries of `Executor` (join.py) share when they turn their arguments into the structs of
include/hmj.h and read the results back: ctypes and duck-typed tensors only -- anything with is_cuda, is_contiguous(),
dim(), shape, element_size(), dtype, data_ptr() and numel() will do; torch is handed in where memory is allocated.
Every function here has at least two callers; what one entry alone needs stays in that entry."""
import ctypes as C

import numpy as np

from ._lib import HmjError

U64_MASK = 0xFFFFFFFFFFFFFFFF

# index = the HMJ_TYPE_* code; also numpy's names of the same types
TYPE_NAMES = ("int8", "int16", "int32", "int64", "uint8", "uint16", "uint32", "uint64", "float32", "float64")
_TYPE_CODES = {name: code for code, name in enumerate(TYPE_NAMES)}


def type_code(dtype):
    """A tensor's dtype (torch.int64, numpy.dtype('int64') or 'int64') -> its HMJ_TYPE_* code."""
    code = _TYPE_CODES.get(str(dtype).rpartition(".")[2])
    if code is None:
        raise ValueError("no HMJ_TYPE_* for %s" % (dtype,))
    return code


# The checks take their message as a format and its arguments: the text is made only when it is raised.
def check_column(t, message, *args):
    """A contiguous 1-D device tensor, or ValueError(message % args)."""
    if not t.is_cuda or not t.is_contiguous() or t.dim() != 1:
        raise ValueError(message % args)


def check_col64(t, name, *args):
    """A column the string entries read on the device: contiguous, 1-D, 64-bit, on the GPU."""
    if not t.is_cuda or not t.is_contiguous() or t.element_size() != 8 or t.dim() != 1:
        raise ValueError("%s must be a contiguous 1-D 64-bit device tensor" % (name % args))


def chars_ptr(chars):
    if chars is None or chars.numel() == 0:
        return None
    if not chars.is_cuda or not chars.is_contiguous() or chars.element_size() != 1:
        raise ValueError("chars must be a contiguous 1-byte device tensor")
    return C.c_void_p(chars.data_ptr())


def str_column(chars, offsets, name, *args):
    """An Arrow large_string column (chars uint8 or None, offsets int64 [n + 1]) -> (chars pointer value or None, the
    bytes in chars, offsets pointer).  name % args is what the messages call the offsets."""
    check_col64(offsets, name, *args)
    if offsets.shape[0] < 1:
        raise ValueError("%s must hold n + 1 entries" % (name % args))
    cp = chars_ptr(chars)
    return (cp.value, chars.numel(), offsets.data_ptr()) if cp is not None else (None, 0, offsets.data_ptr())


def validity(dst, valid, n, name, *args, any_width=False, empty_is_absent=False):
    """Fill the _lib.Validity `dst` from a column's Arrow bitmap (LSB first); returns the tensor that must stay alive for
    the call, None without a bitmap.  valid: None, a device tensor, or (tensor, bit_offset): row i is bit bit_offset + i.
    Two flavours, as the entries grew them:
      any_width=False  a byte bitmap (`pack_validity`): uint8, and long enough for bit_offset + n bits unless that sum
                       overflows 64 bits, which is the library's to reject.  name % args names the bitmap ("valid[2]").
      any_width=True   bytes or 64-bit words, the length left to the caller.  name % args names the owner ("term 2").
    empty_is_absent, byte bitmaps only: an empty tensor is "no NULL in this column" whatever n is -- the string and mixed
    entries and take_str_device (True); the column joins, group_cols_device and take_cols_device (False) raise on it
    when bit_offset + n > 0.  Either way an empty tensor passes bits == NULL."""
    if valid is None:
        return None
    t, off = valid if isinstance(valid, tuple) else (valid, 0)
    off = int(off)
    if not t.is_cuda or not t.is_contiguous() or t.dim() != 1 or not (any_width or t.element_size() == 1):
        raise ValueError(("%s: valid must be a contiguous 1-D device tensor" if any_width else
                          "%s must be a contiguous 1-D uint8 device tensor") % (name % args))
    if off < 0:
        raise ValueError("%s: bit_offset must not be negative" % (name % args))
    if not any_width and not (empty_is_absent and not t.shape[0]) and off + n < (1 << 64) and t.shape[0] * 8 < off + n:
        raise ValueError("%s holds fewer than bit_offset + n bits" % (name % args))
    # (n == 0: the pointer is still passed; nothing reads it)
    dst.bits = t.data_ptr() if t.shape[0] else None
    dst.bit_offset = off & U64_MASK
    return t


def row_map(rm, int64, message, *args):
    """A row map -- a contiguous 1-D device tensor of the dtype `int64` (the caller's torch.int64), or a (device_pointer,
    n) pair such as a result's r_row with its n_matches -- -> (pointer or None, entries, what must stay alive)."""
    if isinstance(rm, tuple):
        return int(rm[0] or 0) or None, int(rm[1]), None
    if not rm.is_cuda or not rm.is_contiguous() or rm.dim() != 1 or rm.dtype != int64:
        raise ValueError(message % args)
    return (rm.data_ptr() if rm.shape[0] else None), rm.shape[0], rm


def want_flags(want_validity, count, what):
    """want_validity (True, False, or one bool per output) -> `count` bools."""
    wants = [bool(want_validity)] * count if isinstance(want_validity, (bool, int)) else [bool(w) for w in want_validity]
    if len(wants) != count:
        raise ValueError("want_validity: one entry per %s" % what)
    return wants


def new_opts(cls, **fields):
    """An options struct with struct_size set and the fields given, each taken mod 2^64 (a fill value may be passed as a
    negative number; narrower fields truncate further, as ctypes has it)."""
    opts = cls()
    opts.struct_size = C.sizeof(cls)
    for k, v in fields.items():
        setattr(opts, k, int(v) & U64_MASK)
    return opts


def read_info(opts, ints=(), floats=(), first=None, between=None):
    """The out fields of an options struct as a dict, in this order: `first` (what the entry read elsewhere, such as its
    outputs' null counts), the struct's hmj_kind_counts (where it has one), the integer fields named, `between`, the
    float fields named.  (ctypes hands an integer field back as an int and a float field as a float.)"""
    info = {} if first is None else first
    if hasattr(opts, "counts"):
        info.update(opts.counts.as_dict())
    for k in ints:
        info[k] = getattr(opts, k)
    if between is not None:
        info.update(between)
    for k in floats:
        info[k] = getattr(opts, k)
    return info


def _memcpy_d2d(torch, dst_tensor, src_ptr, nbytes):
    """Copy nbytes from a raw device pointer into a torch tensor (plumbing only)."""
    hip = C.CDLL(None)  # the HIP runtime torch already loaded
    fn = getattr(hip, "hipMemcpy", None)
    if fn is None:
        hip = C.CDLL("libamdhip64.so")
        fn = hip.hipMemcpy
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    torch.cuda.synchronize()
    rc = fn(C.c_void_p(dst_tensor.data_ptr()), C.c_void_p(src_ptr), nbytes, 3)  # hipMemcpyDeviceToDevice
    if rc:
        raise HmjError(-4, "hipMemcpy d2d failed: %d" % rc)


def read_columns(torch, device, ptrs, n, absent=None):
    """n-entry 64-bit device columns behind raw pointers -> an [n, len(ptrs)] uint64 array; [0, len(ptrs)] when n is 0 or
    the first column is NULL.  absent: the value, or one value per column, that a NULL column behind the first reads as
    (a column the join kind did not produce); None when every column is there."""
    out = np.empty((n, len(ptrs)), np.uint64)
    if n == 0 or not ptrs[0]:
        return out[:0]
    tmp = torch.empty(n, dtype=torch.int64, device="cuda:%d" % device)
    for c, ptr in enumerate(ptrs):
        if not ptr and absent is not None:
            out[:, c] = absent[c] if isinstance(absent, tuple) else absent
            continue
        _memcpy_d2d(torch, tmp, ptr, n * 8)
        out[:, c] = tmp.cpu().numpy().view(np.uint64)
    return out
