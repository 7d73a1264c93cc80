"""Host restatements of what the column entries compute (include/hmj.h), in plain numpy: the 64-bit keys of the
multi-column and mixed-key joins, the groupings and their aggregates, ORDER BY's row map and byte streams, WHERE, and the
window functions.
The tests and tools compare the device's results with them; nothing here touches ctypes or a GPU."""
from fractions import Fraction

import numpy as np

from . import _lib


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
    # groups in tuple order: a stable lexicographic sort of the rows (column 0 first), so the first row of a run of equal
    # tuples is its smallest row -- what numpy.unique(canon, axis=0, return_index, return_inverse, return_counts) gives,
    # several times faster over millions of rows
    by_tuple = np.lexsort(canon.T[::-1])
    s = canon[by_tuple]
    head = np.ones(n, bool)
    head[1:] = np.any(s[1:] != s[:-1], axis=1)
    starts = np.flatnonzero(head)
    first = by_tuple[starts]
    inv = np.empty(n, np.int64)
    inv[by_tuple] = np.cumsum(head) - 1
    count = np.diff(np.append(starts, n))
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
                one = count == 1  # a group of one value: the sum is the value (no loop: a grouping may hold millions of them)
                sums[one] = xd[order[ends[one] - 1]]
                abss[one] = np.abs(sums[one])
                with np.errstate(all="ignore"):
                    for k in np.flatnonzero(count > 1):
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


def _order_ranks(cols, n):
    """`_order_columns`' columns -> per column the int64 rank of every row under the order rule (see `expected_order_by`):
    equal ranks are equal slots, and the stable lexicographic order of the rank tuples is the row map."""
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
    return ranks


def expected_order_by(columns):
    """The row map hmj_order_by_device returns (include/hmj.h), restated on the host from the order rule: columns is a list
    of (values, flags[, valid]) -- values a numpy array of an integer or float dtype, or a list of bytes (a string column);
    flags HMJ_ORDER_* bits; valid None or n bools (True = valid).  Per column every row gets the dense rank of its value
    among the column's valid values -- integers in their signedness, floats in IEEE order with -0.0 < +0.0 and every NaN one
    value above +inf, strings as Python orders bytes (unsigned bytes, then length) --, reversed under HMJ_ORDER_DESC; a NULL
    slot ranks behind all of them, or in front under HMJ_ORDER_NULLS_FIRST.  The map is the stable lexicographic order of
    the rank tuples (ties keep ascending row index).  What lies under a NULL slot is not read.  Returns n uint64."""
    cols, n = _order_columns(columns)
    ranks = _order_ranks(cols, n)
    if n == 0:
        return np.zeros(0, np.uint64)
    return np.lexsort(ranks[::-1]).astype(np.uint64)  # (lexsort: the last key is the primary one; stable)


def expected_top_k(columns, k, offset=0):
    """The row map hmj_top_k_device returns (include/hmj.h): entries offset .. offset + k of `expected_order_by(columns)`,
    the sum saturating as the library's does (k and offset are any values below 2^64).  Returns min(k, n - min(n, offset))
    uint64."""
    full = expected_order_by(columns)
    n = full.shape[0]
    lo = min(int(offset), n)
    return full[lo:min(n, lo + min(int(k), n - lo))]


def expected_window(key_columns, n_partition_cols, fns, n=None):
    """What hmj_window_device returns (include/hmj.h), restated on the host.  key_columns as `expected_order_by` takes them
    (may be empty: one partition in row order; n then comes from the first function column, or from `n`); the first
    n_partition_cols are PARTITION BY, the rest ORDER BY.  fns: a list of (op, values[, valid[, bit_offset[, offset]]]) as
    `Executor.window_device` takes them, with host values -- op an HMJ_WIN_* code; values a numpy array of n integers or
    floats, or None where the op reads no value; valid None or n bools per ROW (True = valid; bit_offset is not looked at);
    offset the rows LAG / LEAD look away.  The order is `expected_order_by`'s; two neighbours of it are in one partition
    (peer group) when their ranks are equal in every partition (every) column; everything else is a walk over the sorted
    positions.  What lies under a NULL slot is not read.  Returns {"row_map" (n uint64), "n_partitions", "n_peer_groups",
    "max_partition_rows", "outputs"}; outputs holds one dict per function, in SORTED order: "values" (n entries of the
    output dtype, 0 in a NULL slot), "valid" (n bools), "null_count"; a float CUM_SUM also has "count" (the prefix's valid
    values, int64) and "abs_sum" (float64: the prefix's sum of |x|) for the error bound, and its values are the correctly
    rounded exact prefix sums where the partition's values are finite, sequential IEEE additions where they are not."""
    cols, nk = _order_columns(key_columns)
    fns = [tuple(f) for f in fns]
    if cols:
        n = nk
    elif n is None:
        lens = [len(f[1]) for f in fns if len(f) > 1 and f[1] is not None]
        n = lens[0] if lens else 0
    n = int(n)
    npc = int(n_partition_cols)
    if not 0 <= npc <= len(cols):
        raise ValueError("n_partition_cols must be in 0..len(key_columns)")
    ranks = _order_ranks(cols, n)
    row_map = np.lexsort(ranks[::-1]).astype(np.int64) if (cols and n) else np.arange(n, dtype=np.int64)
    pos = np.arange(n, dtype=np.int64)
    phead, ghead = np.zeros(n, bool), np.zeros(n, bool)
    if n:
        phead[0] = True
        for k, r in enumerate(ranks):
            s = r[row_map]
            d = s[1:] != s[:-1]
            if k < npc:
                phead[1:] |= d
            ghead[1:] |= d
        ghead |= phead
    pid = np.cumsum(phead) - 1
    starts = np.nonzero(phead)[0]
    ps = starts[pid] if n else pos
    plen = np.bincount(pid, minlength=len(starts)) if n else np.zeros(0, np.int64)
    pe = ps + plen[pid] if n else pos  # one behind the partition's last position
    gs = np.maximum.accumulate(np.where(ghead, pos, 0)) if n else pos
    gcum = np.cumsum(ghead)
    res = {"row_map": row_map.astype(np.uint64), "n_partitions": int(len(starts)), "n_peer_groups": int(np.count_nonzero(ghead)),
           "max_partition_rows": int(plen.max()) if n else 0, "outputs": []}
    for k, f in enumerate(fns):
        op = int(f[0])
        vals = f[1] if len(f) > 1 else None
        valid = None if len(f) < 3 or f[2] is None else np.asarray(f[2], bool).ravel()
        off = int(f[4]) if len(f) > 4 else 0
        out = {}
        if op == _lib.HMJ_WIN_ROW_NUMBER:
            v, ok = pos - ps + 1, np.ones(n, bool)
        elif op == _lib.HMJ_WIN_RANK:
            v, ok = gs - ps + 1, np.ones(n, bool)
        elif op == _lib.HMJ_WIN_DENSE_RANK:
            v, ok = (gcum - gcum[ps] + 1) if n else pos, np.ones(n, bool)
        else:
            if valid is not None and len(valid) != n:
                raise ValueError("function %d: valid must hold n entries" % k)
            have = (np.ones(n, bool) if valid is None else valid)[row_map]
            cnt = np.cumsum(have)
            cnt = (cnt - (cnt[ps] - have[ps])) if n else cnt  # the prefix's valid values
            if op == _lib.HMJ_WIN_CUM_COUNT:
                v, ok = cnt, np.ones(n, bool)
            else:
                if vals is None:
                    raise ValueError("function %d: the op reads values" % k)
                a = np.ascontiguousarray(vals).ravel()
                if len(a) != n or a.dtype.kind not in "iuf" or a.dtype.itemsize > 8 or a.dtype == np.float16:
                    raise ValueError("function %d: values: n integers or floats of 1 to 8 bytes" % k)
                x = a[row_map]
                is_float = a.dtype.kind == "f"
                if op in (_lib.HMJ_WIN_LAG, _lib.HMJ_WIN_LEAD):
                    off = min(off, n)  # (n rows away is outside every partition, like anything beyond it)
                    jj = pos - off if op == _lib.HMJ_WIN_LAG else pos + off
                    ok = (jj >= ps) & (jj < pe)
                    at = np.where(ok, jj, 0).astype(np.int64)
                    ok = ok & have[at] if n else ok
                    v = np.where(ok, x[at] if n else x, a.dtype.type(0))
                elif op == _lib.HMJ_WIN_CUM_SUM and not is_float:
                    wide = x.astype(np.int64).view(np.uint64) if a.dtype.kind == "i" else x.astype(np.uint64)
                    wide = np.where(have, wide, np.uint64(0))
                    cs = np.cumsum(wide, dtype=np.uint64)  # (wraps mod 2^64)
                    v = (cs - (cs[ps] - wide[ps])) if n else cs
                    v = v.view(np.int64) if a.dtype.kind == "i" else v
                    ok = cnt > 0
                elif op == _lib.HMJ_WIN_CUM_SUM:
                    xd = np.where(have, x.astype(np.float64), 0.0)
                    v, abss = np.zeros(n), np.zeros(n)
                    with np.errstate(all="ignore"):
                        for s0, ln in zip(starts, plen):
                            seg, hv = xd[s0:s0 + ln], have[s0:s0 + ln]
                            abss[s0:s0 + ln] = np.cumsum(np.abs(seg))
                            if np.all(np.isfinite(seg)):
                                run, exact = Fraction(0), []
                                for y, h in zip(seg.tolist(), hv.tolist()):
                                    if h:
                                        run += Fraction(y)
                                    exact.append(run)
                                try:
                                    v[s0:s0 + ln] = [float(e) for e in exact]
                                except OverflowError:
                                    v[s0:s0 + ln] = np.cumsum(seg)
                            else:  # as IEEE addition has it, in order
                                run = None
                                for i, (y, h) in enumerate(zip(seg, hv)):
                                    if h:
                                        run = y if run is None else run + y
                                    v[s0 + i] = 0.0 if run is None else run
                    ok = cnt > 0
                    out.update({"count": cnt.astype(np.int64), "abs_sum": abss})
                elif op in (_lib.HMJ_WIN_CUM_MIN, _lib.HMJ_WIN_CUM_MAX):
                    low = op == _lib.HMJ_WIN_CUM_MIN
                    acc_fn = np.minimum.accumulate if low else np.maximum.accumulate
                    if is_float:
                        keys, nan = _float_order_keys(x)
                        ident = keys.dtype.type(np.iinfo(keys.dtype).max if low else 0)
                        keys = np.where(have & ~nan, keys, ident)
                        numbers = np.cumsum(have & ~nan)
                        numbers = (numbers - (numbers[ps] - (have & ~nan)[ps])) if n else numbers
                        acc = keys.copy()
                        for s0, ln in zip(starts, plen):
                            acc[s0:s0 + ln] = acc_fn(keys[s0:s0 + ln])
                        top = keys.dtype.type(1 << (8 * a.dtype.itemsize - 1))
                        v = np.where(acc & top, acc ^ top, ~acc).view(a.dtype).copy()
                        v[numbers == 0] = np.nan  # (numpy's default NaN is the canonical quiet one)
                    else:
                        info = np.iinfo(a.dtype)
                        y = np.where(have, x, a.dtype.type(info.max if low else info.min))
                        v = y.copy()
                        for s0, ln in zip(starts, plen):
                            v[s0:s0 + ln] = acc_fn(y[s0:s0 + ln])
                    ok = cnt > 0
                else:
                    raise ValueError("function %d: unknown op %d" % (k, op))
        if op <= _lib.HMJ_WIN_CUM_COUNT:
            v = np.asarray(v).astype(np.uint64)
        v = np.array(v)
        v[~ok] = 0
        out.update({"values": v, "valid": ok, "null_count": int(n - np.count_nonzero(ok))})
        res["outputs"].append(out)
    return res


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
