#!/usr/bin/env python3
"""Parent against change, call by call: a fixed list of calls -- one or two per plan of the u64 join driver, shapes from the
tests -- against the library HMJ_LIB names, one JSON record per call: return code, hmj_last_error, every field of
hmj_last_timing that is not a time, hmj_last_plan, the six sums, and (materialising calls) which result columns are null
and hashes of the rows -- of the row set, and for ordered calls of the row sequence (an unordered result's sequence is
whatever order the workgroups reached the output cursor in: it differs from run to run of ONE library).  Every call is
issued three times in a row on its context (cool-downs).  Two libraries built from a host-only refactor must write
identical files:

    HMJ_LIB=<parent .so> python tools/ab_calls.py parent.jsonl
    HMJ_LIB=<change .so> python tools/ab_calls.py change.jsonl   # a process each
    cmp parent.jsonl change.jsonl

A second argument chooses the calls: `u64` (the u64 driver's plans), `small` (the ordered join of a small build side and
hmj_sort_u64_device, branch by branch: small_section), `keyed` (the string, column and mixed entries: keyed_section) or
`all` (the default).
"""
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import hashmergejoin_amd as H
from hashmergejoin_amd import _lib
from hashmergejoin_amd.join import _memcpy_d2d

M, O, F, CK, SP = H.HMJ_MATERIALIZE, H.HMJ_ORDERED, H.HMJ_FIRST_WINS, H.HMJ_CHECKSUM, H.HMJ_SUM_PROBE
TIMING = ("path", "radix_bits", "radix_passes", "key_prefix_bits", "key_window_low", "n_probe_items", "n_split_retries",
          "n_scatter_launches", "bytes_scatter", "bytes_hist", "bytes_probe_count", "bytes_probe_write")
SUMS = ("n_matches", "sum_r", "sum_s", "xor_fold", "mix_sum", "sum_probe_all")
out_f = open(sys.argv[1], "w") if len(sys.argv) > 1 else sys.stdout
n_records = 0


def executor(**env):
    """An executor created under HMJ_* settings (read once at hmj_create)."""
    os.environ.update({k: str(v) for k, v in env.items()})
    try:
        return H.Executor(0)
    finally:
        for k in env:
            del os.environ[k]


def to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.uint64).reshape(-1, 2).view(np.int64).copy()).cuda()


def to_np(t):
    return t.cpu().numpy().view(np.uint64)


def zipf_thresholds(domain, theta=0.9):
    w = 1.0 / np.arange(1, domain + 1, dtype=np.float64) ** theta
    cdf = np.cumsum(w) / w.sum()
    thr = np.empty(domain, np.uint64)
    big = cdf >= 1.0 - 2.0 ** -53
    thr[~big] = (cdf[~big] * 2.0 ** 64).astype(np.uint64)
    thr[big] = np.uint64(0xFFFFFFFFFFFFFFFF)
    thr[-1] = np.uint64(0xFFFFFFFFFFFFFFFF)
    return torch.from_numpy(thr.view(np.int64).copy()).cuda()


def column(ex, ptr, n, host):
    if host:
        return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_uint64)), shape=(n,)).copy()
    tmp = torch.empty(n, dtype=torch.int64, device="cuda:0")
    _memcpy_d2d(torch, tmp, ptr, n * 8)
    return tmp.cpu().numpy().view(np.uint64)


def rows_digest(ex, res, host, ordered):
    """Null columns, a hash of the row set and (ordered) one of the row sequence (uint64 arithmetic wraps).  A keyed join's
    result has five columns: key64 (the string join's hash), r_row, s_row, rval, sval."""
    n = int(res.n_matches)
    if hasattr(res, "key"):
        ptrs = (res.key, res.rval, res.sval)
    else:
        ptrs = (res.hash if hasattr(res, "hash") else res.key64, res.rval, res.sval, res.r_row, res.s_row)
    d = {"null_cols": [not p for p in ptrs]}
    if n == 0 or not ptrs[0]:
        return d
    with np.errstate(over="ignore"):
        h = np.zeros(n, np.uint64)
        for p, mul in zip(ptrs, (0x9E3779B97F4A7C15, 0xC2B2AE3D27D4EB4F, 0x165667B19E3779F9, 0x27D4EB2F165667C5, 0x85EBCA77C2B2AE63)):
            if p:
                h = (h ^ column(ex, p, n, host)) * np.uint64(mul)
                h ^= h >> np.uint64(29)
        d["rows_set"] = [int(h.sum(dtype=np.uint64)), int((h * h).sum(dtype=np.uint64))]
        if ordered:
            d["rows_seq"] = int((h * (np.arange(n, dtype=np.uint64) * np.uint64(2) + np.uint64(1))).sum(dtype=np.uint64))
    return d


def record(name, ex, fn, host=False, ordered=False, repeat=3, unstable_path=0):
    """fn() -> JoinResult or (JoinResult, counters); an HmjError is part of the record.  unstable_path: HMJ_PATH_* bits left
    out of the record (they differ between runs of ONE library)."""
    global n_records
    for i in range(repeat):
        rec = {"call": name, "i": i}
        try:
            got = fn()
            res, extra = got if isinstance(got, tuple) else (got, None)
            rec["rc"] = 0
            rec.update({k: int(getattr(res, k)) for k in SUMS})
            if extra is not None:
                rec["counts"] = {k: v for k, v in extra.items() if not k.startswith("ms_")}
            rec.update(rows_digest(ex, res, host, ordered))
        except H.HmjError as e:
            rec["rc"] = e.code
        rec["last_error"] = ex.L.hmj_last_error(ex.h).decode()
        t = ex.last_timing()
        rec["timing"] = {k: int(t[k]) for k in TIMING}
        rec["plan"] = ex.last_plan()
        rec["timing"]["path"] &= ~unstable_path
        rec["plan"]["path"] &= ~unstable_path
        out_f.write(json.dumps(rec, sort_keys=True) + "\n")
        out_f.flush()
        n_records += 1


def joins(name, ex, R, S, flag_list, **kw):
    for fl in flag_list:
        record("%s flags=%#x" % (name, fl), ex, lambda: ex.join_device(R, S, fl), ordered=bool(fl & O), **kw)


def host_join(name, ex, R, S, flags=M):
    Rh, Sh = (R if isinstance(R, np.ndarray) else to_np(R)), (S if isinstance(S, np.ndarray) else to_np(S))
    record("%s host flags=%#x" % (name, flags), ex, lambda: ex.join_host(Rh, Sh, flags), host=True, ordered=bool(flags & O))


def keyed_section():
    """The keyed joins, whose host sequence is hmj_tuplejoin.h's driver: the string entries in every mode for four kinds,
    without bitmaps, with one on the probe side and with one on both; collisions (hash_bits = 4) through the collision sort
    and the ambiguous re-join; the string entries' device-found argument errors and an empty side; the column and the
    mixed entry with bitmaps on both sides.  Shapes from the tests: a few hundred to a few thousand rows, more than one
    workgroup (256 rows) per relation.  HOT_KEY_HINT is left out under bitmaps (tests/test_keyjoin_plans_gpu.py, UNSTABLE)."""
    import random

    PROBE, BUILD = H.HMJ_KIND_PROBE_SIDE, H.HMJ_KIND_BUILD_SIDE
    KINDS = (("inner", PROBE, H.HMJ_JOIN_INNER), ("probe semi", PROBE, H.HMJ_JOIN_SEMI), ("build anti", BUILD, H.HMJ_BUILD_ANTI),
             ("full outer", BUILD, H.HMJ_FULL_OUTER))
    MODES = (("count", CK | SP), ("mat", M | CK | SP), ("ordered", O | CK | SP))
    HOT = H.HMJ_PATH_HOT_KEY_HINT
    prng, nrng = random.Random(11), np.random.default_rng(11)
    kx = H.Executor(0)
    pool = sorted({b"k%06d" % prng.randrange(10 ** 6) + bytes(prng.getrandbits(8) for _ in range(prng.randrange(0, 24))) for _ in range(1500)})
    prng.shuffle(pool)

    def payloads(n):
        return torch.from_numpy(nrng.integers(0, 1 << 62, n, dtype=np.int64)).cuda()

    def str_rel(n, lo, hi):  # duplicates on both sides, misses on both sides
        chars, offs = H.pack_strings([pool[prng.randrange(lo, hi)] for _ in range(n)], "cuda")
        return chars, offs, payloads(n)

    def bitmap(n, off):
        return H.pack_validity(nrng.random(n) >= 0.2, off, "cuda"), off

    def str_calls(tag, B, P, kinds, modes, bits=0):
        nb, npr = B[2].shape[0], P[2].shape[0]
        for vname, vb, vp in (("no bitmap", None, None), ("probe bitmap", None, bitmap(npr, 3)), ("both bitmaps", bitmap(nb, 5), bitmap(npr, 0))):
            for kname, side, kind in kinds:
                for mname, fl in modes:
                    record("str %s %s %s %s" % (tag, kname, mname, vname), kx,
                           lambda: kx.join_kind_str_device(B, P, side, kind, fl, hash_bits=bits, probe_fill=77, build_fill=55, build_valid=vb,
                                                           probe_valid=vp),
                           ordered=bool(fl & O), unstable_path=HOT if vb or vp else 0)

    B, P = str_rel(1500, 0, 1000), str_rel(2100, 500, len(pool))
    str_calls("", B, P, KINDS, MODES)
    for mname, fl in MODES:  # the inner entry proper
        record("str inner entry %s" % mname, kx, lambda: kx.join_str_device(B, P, fl), ordered=bool(fl & O))
    # 16 hash values: runs of equal hash with several keys (the collision sort), representatives that hold another key
    Bs, Ps = str_rel(300, 0, 200), str_rel(330, 100, 300)
    str_calls("hash_bits=4", Bs, Ps, KINDS, MODES[2:], bits=4)
    # what the hash kernels find: decreasing offsets (the first bad row is named), key bytes without a chars buffer; an empty side
    bad = P[1].clone()
    bad[701] = bad[700] - 1
    for kname, side, kind in (KINDS[0], KINDS[3]):
        record("str decreasing offsets %s" % kname, kx, lambda: kx.join_kind_str_device(B, (P[0], bad, P[2]), side, kind, M))
        record("str chars NULL %s" % kname, kx, lambda: kx.join_kind_str_device((None, B[1], B[2]), P, side, kind, M))
        record("str empty build %s" % kname, kx, lambda: kx.join_kind_str_device((B[0], B[1][:1], B[2][:0]), P, side, kind, O | CK | SP,
                                                                                 probe_fill=77), ordered=True)
    record("str bad offsets inner entry", kx, lambda: kx.join_str_device(B, (P[0], bad, P[2]), M))
    # the column and the mixed entry with bitmaps on both sides (their valid rows are compacted into full-size arrays now)
    nb, npr = 1500, 2100
    days = [torch.from_numpy(nrng.integers(0, 40, n, dtype=np.int32)).cuda() for n in (nb, npr)]
    ids = [torch.from_numpy(nrng.integers(0, 50, n, dtype=np.int64)).cuda() for n in (nb, npr)]
    vals = [payloads(nb), payloads(npr)]
    cv = [[bitmap(n, 1), bitmap(n, 6)] for n in (nb, npr)]
    mv = [[bitmap(n, 2), None] for n in (nb, npr)]
    for kname, side, kind in (KINDS[0], KINDS[3]):
        for mname, fl in MODES:
            record("cols %s %s both bitmaps" % (kname, mname), kx,
                   lambda: kx.join_kind_cols_device([ids[0], days[0]], vals[0], [ids[1], days[1]], vals[1], side, kind, fl, force_hashed=True,
                                                    probe_fill=77, build_fill=55, build_valid=cv[0], probe_valid=cv[1]),
                   ordered=bool(fl & O), unstable_path=HOT)
            record("mixed %s %s both bitmaps" % (kname, mname), kx,
                   lambda: kx.join_mixed_device([B[:2], days[0]], vals[0], [P[:2], days[1]], vals[1], side, kind, fl, probe_fill=77,
                                                build_fill=55, build_valid=mv[0], probe_valid=mv[1]),
                   ordered=bool(fl & O), unstable_path=HOT)
    record("mixed decreasing offsets under a bitmap", kx,
           lambda: kx.join_mixed_device([B[:2], days[0]], vals[0], [(P[0], bad), days[1]], vals[1], BUILD, H.HMJ_FULL_OUTER, M,
                                        build_valid=mv[0], probe_valid=mv[1]))
    kx.close()


def record_sort(name, ex, a, inplace=False, repeat=3):
    """record()'s sibling for hmj_sort_u64_device on the rows `a` (numpy, [n, 2]): return code, hmj_last_error, the timing fields
    that are not times, hmj_last_plan and a hash of the output row sequence."""
    global n_records
    for i in range(repeat):
        rec = {"call": name, "i": i}
        try:
            got = to_np(ex.sort_device(to_dev(a), inplace=inplace))
            rec["rc"] = 0
            with np.errstate(over="ignore"):
                h = (got[:, 0] * np.uint64(0x9E3779B97F4A7C15)) ^ (got[:, 1] * np.uint64(0xC2B2AE3D27D4EB4F))
                h ^= h >> np.uint64(29)
                rec["rows_seq"] = int((h * (np.arange(len(h), dtype=np.uint64) * np.uint64(2) + np.uint64(1))).sum(dtype=np.uint64))
        except H.HmjError as e:
            rec["rc"] = e.code
        rec["last_error"] = ex.L.hmj_last_error(ex.h).decode()
        t = ex.last_timing()
        rec["timing"] = {k: int(t[k]) for k in TIMING}
        rec["plan"] = ex.last_plan()
        out_f.write(json.dumps(rec, sort_keys=True) + "\n")
        out_f.flush()
        n_records += 1


def small_section():
    """The ordered join of a small build side under a long probe side (try_small_build_ordered) and hmj_sort_u64_device,
    one call per branch of their fallback ladders; shapes from tests/test_gpu_join.py at the smallest size that reaches the
    branch.  A case whose point is a cool-down (a give-way, a give-up, an overflow) is issued ten times."""
    rng = np.random.default_rng(77)
    M64 = 0xFFFFFFFFFFFFFFFF

    def relations(ex, nb, npb, miss, pay):
        B = to_np(ex.gen_build(nb)).copy()
        P = to_np(ex.gen_uniform_domain(npb, nb) if miss == 0 else ex.gen_probe(npb, nb, miss_mod=miss)).copy()
        if pay == "hot":  # a third of the probe rows carry one key
            P[::3, 0] = B[17, 0]
            P[:, 1] = rng.permutation(npb).astype(np.uint64)
        elif pay == "ties7":
            P[:, 1] = rng.integers(0, 7, size=npb, dtype=np.uint64) * np.uint64(0x0123456789ABCDEF)
        elif pay == "extremes":
            P[:, 1] = rng.integers(0, 1 << 62, size=npb, dtype=np.uint64)
            P[::5, 1] = np.uint64(0)
            P[1::5, 1] = np.uint64(M64)
        elif pay == "clustered":  # all build keys but three below 4000, three near 2^60
            order = np.argsort(B[:, 0], kind="stable")
            sk = B[order, 0].copy()
            newk = np.arange(nb, dtype=np.uint64)
            newk[-3:] = np.uint64(1 << 60) + np.arange(3, dtype=np.uint64) * np.uint64(0x1000000000)
            P[:, 0] = newk[np.searchsorted(sk, P[:, 0])]
            B[order, 0] = newk
        if pay in ("ids", "clustered"):
            P[:, 1] = rng.permutation(npb).astype(np.uint64)
        elif pay == "rowid":
            P[:, 1] = np.uint64(0x0000123400000000) + np.arange(npb, dtype=np.uint64) * np.uint64(3)
        elif pay == "offset":
            P[:, 1] = np.uint64(0xFEDCBA9800000000) + rng.integers(0, 1 << 30, size=npb, dtype=np.uint64)
        elif pay == "wide":
            P[:, 1] = rng.integers(0, 1 << 63, size=npb, dtype=np.uint64) * np.uint64(2)
        elif pay == "stride":  # the first pass's digit is the same for every row
            P[:, 1] = rng.permutation(npb).astype(np.uint64) * np.uint64(1024)
        elif pay == "dupbuild":
            B[1::3, 0] = B[0::3, 0][: len(B[1::3])]
        return B, P

    def ordered(ex, cases, flag_list=(O, O | CK | SP)):
        for nb, npb, miss, pay, repeat in cases:
            B, P = relations(ex, nb, npb, miss, pay)
            joins("small %d x %d miss=%d %s" % (nb, npb, miss, pay), ex, to_dev(B), to_dev(P), flag_list, repeat=repeat)
            ex.release_result()

    exs = executor(HMJ_GTABLE_SORT_FANOUT=1)  # (the cost model switched off, as in the tests)
    exs.set_profiling(True)
    ordered(exs, [(1, 5000, 0, "ids", 3), (300, 5000, 0, "ids", 3),  # no run form
                  (7, 70000, 0, "ids", 3),                            # rank runs
                  (1000, 300001, 3, "offset", 10),                    # the fused attempt gives way to emit + pass A
                  (1000, 200000, 0, "wide", 3),
                  (2000, 700000, 0, "ties7", 3),
                  (1500, 500000, 0, "extremes", 10),                  # runs give up -> composites
                  (3000, 400000, 2, "dupbuild", 10),                  # full give-up
                  (4000, 2200001, 0, "clustered", 3),                 # the build side's MSD sort gives up -> LSD
                  (4000, 1200000, 0, "hot", 10),                      # a run beyond the kernel -> composites
                  (37, 1 << 20, 0, "rowid", 3),                       # cut runs, strided pass
                  (100, 1 << 21, 0, "ties7", 10),                     # cut runs -> composites
                  (300000, 1 << 23, 0, "rowid", 3),                   # grouped ranks
                  (280000, 5000000, 0, "wide", 10)])                  # grouped ranks, no room -> composites
    exs.close()
    exc = executor(HMJ_GTABLE_SORT_FANOUT=1, HMJ_GTABLE_SORT_SLAB_MIN_LOG2=20, HMJ_RANK_RUNS=0)
    exc.set_profiling(True)
    ordered(exc, [(1000, (1 << 22) + 5, 0, "ids", 3),                 # the composites' chain succeeds
                  (4097, 1 << 22, 0, "stride", 10)])                  # ... overflows -> exact passes
    exc.close()
    exd = H.Executor(0)  # the gate: refused by the model, admitted; the host entry on the admitted shape
    exd.set_profiling(True)
    ordered(exd, [(1000, 300000, 0, "uniform", 3), (1000, 1 << 23, 0, "uniform", 3)], (O | CK,))
    B, P = relations(exd, 1000, 1 << 23, 0, "uniform")
    host_join("small gate", exd, B, P, O)
    exd.release_result()
    # ---- hmj_sort_u64_device
    srng = np.random.default_rng(17)

    def rows(keys):
        return np.stack([keys.astype(np.uint64), np.arange(len(keys), dtype=np.uint64)], 1)

    for n in (12345, 1 << 16):  # no survey
        record_sort("sort uniform n=%d" % n, exd, rows(srng.integers(0, 1 << 63, n, dtype=np.uint64)))
    n = (1 << 22) + 4099
    record_sort("sort uniform", exd, rows(srng.integers(0, 1 << 63, n, dtype=np.uint64) * np.uint64(2) + srng.integers(0, 2, n, dtype=np.uint64)))  # MSD
    exd.forget_workloads()
    record_sort("sort few_values", exd, rows(srng.integers(0, 5, n).astype(np.uint64) * np.uint64(0x0101010101010101)), repeat=10)  # MSD gives up
    exd.forget_workloads()
    record_sort("sort sorted", exd, rows(np.sort(srng.integers(0, 1 << 63, n, dtype=np.uint64))), repeat=10)
    exd.forget_workloads()
    n = (1 << 22) + 77
    d16 = (srng.integers(0, 256, n).astype(np.uint64) << np.uint64(8)) | (srng.integers(0, 200, n).astype(np.uint64) << np.uint64(48))
    # (a permutation: three digits vary -- in place an odd number of passes, which end in the scratch buffer)
    for name, keys in (("digits_1_6", d16), ("one_key", np.full(n, 0x1234567890ABCDEF, np.uint64)), ("dense", srng.permutation(n))):
        record_sort("sort " + name, exd, rows(keys))
        record_sort("sort %s in place" % name, exd, rows(keys), inplace=True)
    exd.close()
    exl = executor(HMJ_SORT_SLAB_MIN_LOG2=20, HMJ_SORT_MSD=0)
    exl.set_profiling(True)
    # The chain's success: a permutation of 2^22 + 77 rows, not of 2^20 + 77 -- below 2^22 rows there is no digit survey, the
    # chain sorts on all eight digits and a permutation's constant top digits overflow a slab.  Without a survey the chain
    # succeeds on uniform 64-bit keys (2^20 + 77 rows), and overflows on sixteen copies per key.
    record_sort("sort chain permutation", exl, rows(srng.permutation(n)))  # (surveyed: digits trimmed to the bits that vary)
    n = (1 << 20) + 77  # (no survey: eight digits of eight bits)
    record_sort("sort chain uniform", exl, rows(srng.integers(0, 1 << 63, n, dtype=np.uint64) * np.uint64(2) + srng.integers(0, 2, n, dtype=np.uint64)))
    record_sort("sort chain 16 copies", exl, rows(srng.integers(0, 1 << 63, n >> 4, dtype=np.uint64)[srng.integers(0, n >> 4, n)]), repeat=10)
    exl.close()


SECTION = sys.argv[2] if len(sys.argv) > 2 else "all"  # all | u64 | small | keyed
if SECTION in ("keyed", "small"):
    keyed_section() if SECTION == "keyed" else small_section()
    print("ab_calls: %d records from %s" % (n_records, _lib.lib_path()), file=sys.stderr)
    sys.exit(0)

rng = np.random.default_rng(7)
ex = executor(HMJ_SLAB_MIN_LOG2=22)           # (the slab plans from 2^22 rows on, as in the tests)
exp = executor(HMJ_SLAB_MIN_LOG2=22, HMJ_GTABLE=0)  # ... and small joins on the partitioned plans

# ---- full slab path: count modes, the unique-key write on top (unordered and ordered, with and without unmatched rows)
nb = (1 << 22) + 1000
R, S, Sm = ex.gen_build(nb), ex.gen_probe(nb, nb), ex.gen_probe(nb + 4321, nb, miss_mod=3)
joins("slab", ex, R, S, (0, CK, F | CK | SP, M | CK, O | CK))
joins("slab miss", ex, R, Sm, (CK, M | CK, O | CK))
host_join("slab", ex, R, Sm)
# ... and a build side prepared ahead, reused
record("slab prepared", ex, lambda: (ex.prepare_build(R, nb), ex.join_device(R, S, 0))[1])
# ---- exact path, a hot foreign key: split partitions
Sz = ex.gen_from_cdf(1 << 23, zipf_thresholds(nb, theta=1.1))
joins("split", ex, R, Sz, (0, F | CK | SP, M | CK, O | CK))
host_join("split", ex, R, Sz)
del S, Sm, Sz
# ---- probe-side slabs: a Zipf build side under a uniform probe side; a skewed probe side overflows and retries
nb, npb, dom = 1 << 22, (1 << 24) + 777, 1 << 22
thr = zipf_thresholds(dom)
Rz, Su = ex.gen_from_cdf(nb, thr), ex.gen_uniform_domain(npb, dom)
joins("slab_probe", ex, Rz, Su, (0, F | SP, CK))
del Rz, Su
Rb, Sk = ex.gen_build(nb), ex.gen_from_cdf(npb, thr, zseed=0x5EED)
joins("slab_probe skewed", ex, Rb, Sk, (0, CK))
del R, Rb, Sk, thr
ex.release_result()
# ---- one-pass slab walk: count, materialising, its duplicate-key fallback, a hot key
nb, npb = 300000, (1 << 22) + 777
B = to_np(ex.gen_build(nb)).copy()
P = to_np(ex.gen_uniform_domain(npb, nb)).copy()
Bd, Pd = to_dev(B), to_dev(P)
joins("one_pass", ex, Bd, Pd, (0, CK | SP, F | CK, M | CK, M | F | CK | SP, O | CK))
host_join("one_pass", ex, B, P)
B2 = B.copy()
B2[1::2, 0] = B2[0::2, 0]
P2 = P.copy()
P2[:, 0] = B2[0::2, 0][rng.integers(0, nb // 2, npb)]
joins("one_pass dup keys", ex, to_dev(B2), to_dev(P2), (M | CK, CK))
P3 = P.copy()
P3[::2, 0] = B[12345, 0]
joins("one_pass hot key", ex, Bd, to_dev(P3), (CK,))
del Bd, Pd, B2, P2, P3
ex.release_result()
# ---- global table (L2 and LDS forms), its give-up on duplicate build keys
Rg, Sg = ex.gen_build(1 << 14), ex.gen_uniform_domain(1 << 22, 1 << 14)
joins("gtable", ex, Rg, Sg, (0, CK, M | CK))
host_join("gtable", ex, Rg, Sg)
joins("ltable", ex, ex.gen_build(1000), ex.gen_uniform_domain(1 << 20, 1000), (0, CK))
Bg = to_np(Rg).copy()
Bg[1::2, 0] = Bg[0::2, 0]
joins("gtable dup keys", ex, to_dev(Bg), Sg, (M | CK, CK))
# ---- ordered, small build side: rank runs, rank sort
joins("rank", ex, Rg, Sg, (O | CK,))
host_join("rank", ex, Rg, Sg, O)
joins("rank 2^10", ex, ex.gen_build(1 << 10), ex.gen_uniform_domain(1 << 22, 1 << 10), (O | CK,))
exr = executor(HMJ_RANK_RUNS=0)
joins("rank sort", exr, exr.gen_build(1 << 10), exr.gen_uniform_domain(1 << 22, 1 << 10), (O | CK,))
exr.close()
del Rg, Sg
ex.release_result()
# ---- partitioned plans of small joins: unique-key write, general passes, ordered expansion and its give-up
nb, npb, keys_n = 200000, 300000, 30000
pool = rng.integers(0, 1 << 62, keys_n + keys_n // 4, dtype=np.uint64)
B = np.stack([pool[rng.integers(0, keys_n, nb)], rng.permutation(nb).astype(np.uint64)], 1)
P = np.stack([pool[rng.integers(keys_n // 8, len(pool), npb)], rng.permutation(npb).astype(np.uint64) + np.uint64(1 << 40)], 1)
Bd, Pd = to_dev(B), to_dev(P)
joins("dup keys", exp, Bd, Pd, (0, CK, M | CK, O | CK | SP, O | F | CK))
host_join("dup keys", exp, B, P)
host_join("dup keys", exp, B, P, O)
B[:9000, 0] = pool[5]
P[:3, 0] = pool[5]
joins("dup keys hot", exp, to_dev(B), Pd, (O | CK,))
nk = 1 << 15  # 16 copies of every key on both sides: the expansion asks for one more radix bit
pool = rng.integers(0, 1 << 62, nk, dtype=np.uint64)
B = np.stack([np.repeat(pool, 16)[rng.permutation(nk * 16)], rng.permutation(nk * 16).astype(np.uint64)], 1)
P = np.stack([np.repeat(pool, 16)[rng.permutation(nk * 16)], rng.permutation(nk * 16).astype(np.uint64) + np.uint64(7)], 1)
joins("16 x 16", exp, to_dev(B), to_dev(P), (O | CK,))
R1, S1 = exp.gen_build((1 << 20) + 77), exp.gen_probe((1 << 21) + 5, (1 << 20) + 77, miss_mod=3)
joins("unique keys", exp, R1, S1, (0, CK, M | CK, O | CK, O | F | CK))
host_join("unique keys", exp, R1, S1)
record("exact prepared", exp, lambda: (exp.prepare_build(R1, (1 << 21) + 5), exp.join_device(R1, S1, 0))[1])
# ---- each join kind once
for kind in (H.HMJ_JOIN_SEMI, H.HMJ_JOIN_ANTI, H.HMJ_JOIN_PROBE_OUTER):
    for fl in (CK, M | CK, O | CK):
        record("kind %d flags=%#x" % (kind, fl), exp, lambda: exp.join_kind_device(R1, S1, kind, fl, outer_fill=77),
               ordered=bool(fl & O))
for kind in (H.HMJ_BUILD_SEMI, H.HMJ_BUILD_ANTI, H.HMJ_BUILD_OUTER, H.HMJ_FULL_OUTER):
    for fl in (CK, M | CK, O | CK):
        record("build kind %d flags=%#x" % (kind, fl), exp,
               lambda: exp.join_build_kind_device(R1, S1, kind, fl, build_fill=55, probe_fill=77), ordered=bool(fl & O))
exp.release_result()
# ---- ordered joins cut into key ranges
exk = executor(HMJ_KEY_RANGES_FORCE=2)
joins("key ranges", exk, exk.gen_build(50000), exk.gen_uniform_domain(400001, 50000), (O | CK | SP,))
joins("key ranges miss", exk, exk.gen_build(50000), exk.gen_probe(300000, 50000, miss_mod=3), (O,))
exk.close()
# ---- argument errors (their messages are part of the contract)
def raw_join(build_ptr, n_build):
    res = H.JoinResult()
    ex._check(ex.L.hmj_join_u64_device(ex.h, build_ptr, n_build, C.c_void_p(R1.data_ptr()), 4, 0, C.byref(res)))
    return res


record("misaligned build", ex, lambda: raw_join(C.c_void_p(R1.data_ptr() + 8), 4), repeat=1)
record("null build", ex, lambda: raw_join(None, 4), repeat=1)
record("too many rows", ex, lambda: raw_join(C.c_void_p(R1.data_ptr()), 1 << 33), repeat=1)
ex.close()
exp.close()
if SECTION == "all":
    small_section()
    keyed_section()
print("ab_calls: %d records from %s" % (n_records, _lib.lib_path()), file=sys.stderr)
