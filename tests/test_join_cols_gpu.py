"""GPU checks of the multi-column key join (hmj_join_cols_device): the packed and the hashed form against a Python dict brute
force over tuples (key64 from `cols_key64`, whose definition test_join_cols_cpu.py pins), forced key64 collisions, the
collision sort's cap, cross-checks against the u64 join and between the two forms, edge values and unaligned slices, every
argument error, the planner's isolation of multi-column joins from u64 joins, and 2^20 x 2^20 rows against numpy."""
import ctypes as C
import os
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
M64 = (1 << 64) - 1
HMJ_E_ARG, HMJ_E_UNSUPPORTED = -1, -5


@pytest.fixture(scope="module")
def H():
    import hashmergejoin_amd as H

    return H


@pytest.fixture(scope="module")
def ex(H):
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    e = H.Executor(0)
    yield e
    e.close()


def dev_col(a, offset=0):
    """A numpy column on the device (as the signed dtype of its width: compared bit for bit anyway); offset: the column
    starts `offset` elements into its allocation -- aligned to its width, not to 16 bytes."""
    import torch

    a = np.ascontiguousarray(a)
    s = a.view("i%d" % a.dtype.itemsize)
    buf = torch.zeros(offset + len(s), dtype=torch.from_numpy(s[:0]).dtype)
    buf[offset:] = torch.from_numpy(s)
    return buf.cuda()[offset:]


def dev_vals(v):
    import torch

    return None if v is None else torch.tensor(np.asarray(v, np.uint64).view(np.int64), device="cuda")


def dev_rel(cols, vals, offset=0):
    return [dev_col(c, offset + k) for k, c in enumerate(cols)] if offset else [dev_col(c) for c in cols], dev_vals(vals)


def join(ex, B, P, flags=0, **kw):
    return ex.join_cols_device(B[0], B[1], P[0], P[1], flags, **kw)


def brute(H, bcols, bv, pcols, pv, widths, bits=0, force_hashed=False):
    """Expected rows (key64, r_row, s_row, rval, sval) sorted by (key64, tuple, r_row, s_row), and the pairs of equal key64
    whose tuples differ.  vals None: the payload of row i is i."""
    kb = [int(x) for x in H.cols_key64(bcols, widths, bits, force_hashed)]
    kp = [int(x) for x in H.cols_key64(pcols, widths, bits, force_hashed)]
    tb = list(zip(*[[int(x) for x in c] for c in bcols]))
    tp = list(zip(*[[int(x) for x in c] for c in pcols]))
    by_tuple = {}
    for r, t in enumerate(tb):
        by_tuple.setdefault(t, []).append(r)
    rows = []
    for s, t in enumerate(tp):
        for r in by_tuple.get(t, ()):
            assert kb[r] == kp[s]
            rows.append((kp[s], t, r, s))
    rows.sort()
    out = np.array([(k, r, s, r if bv is None else bv[r], s if pv is None else pv[s]) for k, _, r, s in rows],
                   np.uint64).reshape(-1, 5)
    cb, cp = {}, {}
    for k in kb:
        cb[k] = cb.get(k, 0) + 1
    for k in kp:
        cp[k] = cp.get(k, 0) + 1
    same_key = sum(cb[k] * cp.get(k, 0) for k in cb)
    return out, same_key - len(rows)


def checks_of(rows):
    from test_join_kinds_cpu import tmix

    if not len(rows):
        return {"n_matches": 0, "sum_r": 0, "sum_s": 0, "xor_fold": 0, "mix_sum": 0}
    m = tmix(rows[:, 0], rows[:, 3], rows[:, 4])
    with np.errstate(over="ignore"):
        return {"n_matches": len(rows), "sum_r": int(rows[:, 3].sum(dtype=np.uint64)), "sum_s": int(rows[:, 4].sum(dtype=np.uint64)),
                "xor_fold": int(np.bitwise_xor.reduce(m)), "mix_sum": int(m.sum(dtype=np.uint64))}


def unordered(rows):
    return rows[np.lexsort(rows.T[::-1])] if len(rows) else rows


def sum_of(pv, n):
    return (sum(pv) if pv is not None else n * (n - 1) // 2) & M64


def draw_pool(rng, widths, n):
    """n distinct tuples over `widths`; few values per column, so tuples share leading columns, and the extremes."""
    per_col = []
    for w in widths:
        top = (1 << (8 * w)) - 1
        per_col.append([0, top, top >> 1] + [rng.randrange(top + 1) for _ in range(20)])
    pool = set()
    while len(pool) < n:
        pool.add(tuple(rng.choice(vs) for vs in per_col))
    return sorted(pool)


def columns(tuples, widths):
    return [np.array([t[c] for t in tuples], "u%d" % w) for c, w in enumerate(widths)]


def dup_relations(rng, widths, nb, np_, n_pool=300, n_miss=100):
    """Duplicates on both sides and misses: build rows drawn from n_pool tuples, probe rows from those and n_miss more."""
    pool = draw_pool(rng, widths, n_pool + n_miss)
    rng.shuffle(pool)
    bt = [pool[rng.randrange(n_pool)] for _ in range(nb)]
    pt = [pool[rng.randrange(n_pool + n_miss)] for _ in range(np_)]
    return columns(bt, widths), columns(pt, widths)


def check_all_modes(H, ex, B, P, want, coll, pv, n_probe, form, **kw):
    ck = checks_of(want)
    res, info = join(ex, B, P, 0, **kw)
    assert int(res.n_matches) == len(want) and (int(res.sum_r), int(res.sum_s)) == (ck["sum_r"], ck["sum_s"]) and not res.key64
    assert info["form"] == form and info["n_collisions"] == coll and info["n_key_pairs"] == len(want) + coll
    res, info = join(ex, B, P, H.HMJ_CHECKSUM | H.HMJ_SUM_PROBE, **kw)
    assert res.checks() == ck and int(res.sum_probe_all) == sum_of(pv, n_probe) and not res.key64
    res, info = join(ex, B, P, H.HMJ_MATERIALIZE | H.HMJ_CHECKSUM, **kw)
    assert np.array_equal(unordered(ex.cols_rows_to_numpy(res)), unordered(want))
    assert res.checks() == ck and info["n_collisions"] == coll
    res, info = join(ex, B, P, H.HMJ_ORDERED | H.HMJ_CHECKSUM | H.HMJ_SUM_PROBE, **kw)
    got = ex.cols_rows_to_numpy(res)
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.array_equal(got, want), np.flatnonzero(np.any(got != want, axis=1))[:5]
    assert res.checks() == ck and int(res.sum_probe_all) == sum_of(pv, n_probe)
    assert info["form"] == form and info["n_collisions"] == coll and info["n_key_pairs"] == len(want) + coll


# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("widths,with_vals", [([4, 4], True), ([1, 2, 4], False), ([2, 2, 2, 2], True), ([4, 4], False)])
def test_packed_against_brute_force(H, ex, widths, with_vals):
    rng = random.Random(sum(widths) * 10 + len(widths) + with_vals)
    bcols, pcols = dup_relations(rng, widths, 1000, 4097)
    bv = [rng.getrandbits(64) for _ in range(1000)] if with_vals else None
    pv = [rng.getrandbits(64) for _ in range(4097)] if with_vals else None
    want, coll = brute(H, bcols, bv, pcols, pv, widths)
    assert coll == 0 and len(want) > 4000
    # ascending key64 is ascending tuple order
    tuples = [tuple(int(c[int(r)]) for c in bcols) for r in want[:, 1]]
    assert tuples == sorted(tuples)
    check_all_modes(H, ex, dev_rel(bcols, bv), dev_rel(pcols, pv), want, 0, pv, 4097, H.HMJ_COLS_PACKED)


@pytest.mark.parametrize("widths", [[8, 4, 2], [8] * 8])
def test_hashed_against_brute_force(H, ex, widths):
    rng = random.Random(len(widths))
    bcols, pcols = dup_relations(rng, widths, 1000, 4097)
    bv = [rng.getrandbits(64) for _ in range(1000)]
    want, coll = brute(H, bcols, bv, pcols, None, widths)
    assert coll == 0 and len(want) > 4000
    check_all_modes(H, ex, dev_rel(bcols, bv), dev_rel(pcols, None), want, 0, None, 4097, H.HMJ_COLS_HASHED)


@pytest.mark.parametrize("widths", [[8, 4, 2], [8] * 8])
def test_forced_collisions(H, ex, widths):
    """hash_bits = 6: 64 values of key64 over 600 distinct tuples, 1-3 copies of each on the build side and 0-3 on the probe
    side.  A run of equal key64 holds several tuples but far fewer rows than the collision sort's 1024."""
    rng = random.Random(6 + len(widths))
    pool = draw_pool(rng, widths, 600)
    bt = [t for t in pool for _ in range(rng.randint(1, 3))]
    pt = [t for t in pool for _ in range(rng.randint(0, 3))]
    rng.shuffle(bt)
    rng.shuffle(pt)
    bcols, pcols = columns(bt, widths), columns(pt, widths)
    bv = [rng.getrandbits(64) for _ in bt]
    pv = [rng.getrandbits(64) for _ in pt]
    want, coll = brute(H, bcols, bv, pcols, pv, widths, bits=6)
    assert coll > 0 and int(want[:, 0].max()) < 64
    run = np.bincount(want[:, 0].astype(np.int64))
    assert 1 < run.max() <= 1024, run.max()
    check_all_modes(H, ex, dev_rel(bcols, bv), dev_rel(pcols, pv), want, coll, pv, len(pt), H.HMJ_COLS_HASHED, hash_bits=6)


def test_one_wide_column_equals_the_u64_join(H, ex):
    import torch

    rng = np.random.default_rng(11)
    keys = rng.choice(np.arange(1, 1 << 20, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15), 6000, replace=False)
    kb, kp = keys[:4097], keys[1000:6000]  # unique on both sides, misses on both sides
    bv = rng.integers(0, 1 << 63, len(kb), dtype=np.uint64)
    pv = rng.integers(0, 1 << 63, len(kp), dtype=np.uint64)
    Bu = torch.from_numpy(np.stack([kb, bv], 1).view(np.int64)).cuda()
    Pu = torch.from_numpy(np.stack([kp, pv], 1).view(np.int64)).cuda()
    B, P = dev_rel([kb], bv), dev_rel([kp], pv)
    for flags in (0, H.HMJ_CHECKSUM | H.HMJ_SUM_PROBE, H.HMJ_ORDERED | H.HMJ_CHECKSUM):
        u = ex.join_device(Bu, Pu, flags)
        want_checks, want_sp = u.checks(), int(u.sum_probe_all)
        want_rows = ex.columns_to_numpy(u, host=False) if flags & H.HMJ_ORDERED else None
        res, info = join(ex, B, P, flags)
        assert info["form"] == H.HMJ_COLS_PACKED and int(res.n_matches) == 3097
        ck = res.checks()
        if not flags & H.HMJ_CHECKSUM:
            ck["xor_fold"] = ck["mix_sum"] = want_checks["xor_fold"] = want_checks["mix_sum"] = 0
        assert ck == want_checks
        if flags & H.HMJ_SUM_PROBE:  # (filled when asked, as for the string join; the u64 entry fills it in other modes too)
            assert int(res.sum_probe_all) == want_sp == int(pv.sum(dtype=np.uint64))
        if want_rows is not None:
            assert np.array_equal(ex.cols_rows_to_numpy(res)[:, [0, 3, 4]], want_rows)


def test_forced_hashed_form_equals_the_packed_form(H, ex):
    rng = random.Random(44)
    bcols, pcols = dup_relations(rng, [4, 4], 1000, 4097)
    bv = [rng.getrandbits(64) for _ in range(1000)]
    B, P = dev_rel(bcols, bv), dev_rel(pcols, None)
    rp, ip = join(ex, B, P, H.HMJ_MATERIALIZE | H.HMJ_CHECKSUM)
    packed = ex.cols_rows_to_numpy(rp)
    cp = rp.checks()
    rh, ih = join(ex, B, P, H.HMJ_MATERIALIZE | H.HMJ_CHECKSUM, force_hashed=True)
    hashed = ex.cols_rows_to_numpy(rh)
    ch = rh.checks()
    assert (ip["form"], ih["form"]) == (H.HMJ_COLS_PACKED, H.HMJ_COLS_HASHED) and ih["n_collisions"] == 0
    assert len(packed) > 4000 and np.array_equal(unordered(packed[:, 1:]), unordered(hashed[:, 1:]))
    assert [ch[k] for k in ("n_matches", "sum_r", "sum_s")] == [cp[k] for k in ("n_matches", "sum_r", "sum_s")]
    assert np.array_equal(hashed[:, 0], H.cols_key64([c[hashed[:, 1].astype(np.int64)] for c in bcols], [4, 4], force_hashed=True))
    cnt, _ = join(ex, B, P, 0, force_hashed=True)
    assert (int(cnt.n_matches), int(cnt.sum_r), int(cnt.sum_s)) == (cp["n_matches"], cp["sum_r"], cp["sum_s"])


def test_oversized_mixed_run_is_unsupported(H, ex):
    """hash_bits = 1: two values of key64 over 3000 distinct one-to-one tuples, so each run of matched pairs holds about
    1500 distinct tuples -- beyond one workgroup's collision sort.  The ordered join returns HMJ_E_UNSUPPORTED; the count join
    stays exact; the ctx stays usable."""
    rng = random.Random(3000)
    widths = [8, 4, 2]
    pool = draw_pool(rng, widths, 3000)
    pt = list(pool)
    rng.shuffle(pt)
    bcols, pcols = columns(pool, widths), columns(pt, widths)
    runs = np.bincount(H.cols_key64(bcols, widths, hash_bits=1).astype(np.int64), minlength=2)
    assert runs.min() > 1024, runs
    B, P = dev_rel(bcols, None), dev_rel(pcols, None)
    with pytest.raises(H.HmjError) as e:
        join(ex, B, P, H.HMJ_ORDERED, hash_bits=1)
    assert e.value.code == HMJ_E_UNSUPPORTED and "1024 rows" in str(e.value)
    cnt, info = join(ex, B, P, 0, hash_bits=1)
    assert int(cnt.n_matches) == 3000 and info["n_collisions"] == int((runs.astype(np.int64) ** 2).sum()) - 3000
    res, info = join(ex, B, P, H.HMJ_ORDERED)
    got = ex.cols_rows_to_numpy(res)
    assert len(got) == 3000 and info["n_collisions"] == 0 and np.all(np.diff(got[:, 0].astype(np.float64)) >= 0)
    assert [pool[int(r)] for r in got[:, 1]] == [pt[int(s)] for s in got[:, 2]]


def test_edges(H, ex):
    import torch

    widths = [2, 4, 1]
    one = columns([(7, 8, 9)], widths)
    B1 = dev_rel(one, [5])
    E = ([torch.zeros(0, dtype=torch.int16, device="cuda"), torch.zeros(0, dtype=torch.int32, device="cuda"),
          torch.zeros(0, dtype=torch.int8, device="cuda")], None)
    for flags in (0, H.HMJ_ORDERED):  # n == 0 on each side
        res, info = join(ex, B1, E, flags | H.HMJ_SUM_PROBE)
        assert int(res.n_matches) == 0 and info["n_key_pairs"] == 0 and info["form"] == 0 and int(res.sum_probe_all) == 0
        res, info = join(ex, E, B1, flags | H.HMJ_SUM_PROBE)
        assert int(res.n_matches) == 0 and info["form"] == 0 and int(res.sum_probe_all) == 5
        assert len(ex.cols_rows_to_numpy(res)) == 0
        res, info = join(ex, E, E, flags)
        assert int(res.n_matches) == 0
    # one row against one row, hit and miss
    for force in (False, True):
        res, info = join(ex, B1, dev_rel(one, None), H.HMJ_ORDERED | H.HMJ_CHECKSUM, force_hashed=force)
        want, _ = brute(H, one, [5], one, None, widths, force_hashed=force)
        assert np.array_equal(ex.cols_rows_to_numpy(res), want) and len(want) == 1 and res.checks() == checks_of(want)
        res, info = join(ex, B1, dev_rel(columns([(7, 8, 10)], widths), None), H.HMJ_ORDERED, force_hashed=force)
        assert int(res.n_matches) == 0
    # 2^(8w) - 1 in every column, a top column of all zeros, columns that start inside their allocation
    for widths in ([1, 2, 4], [8, 4, 2]):
        top = tuple((1 << (8 * w)) - 1 for w in widths)
        rng = random.Random(widths[0])
        low = draw_pool(rng, widths[1:], 150)
        bt = [top, top] + [(0,) + t for t in low] + [top[:-1] + (top[-1] - 1,)]
        pt = [(0,) + t for t in low[::2]] * 2 + [top] + [(1,) + t for t in low[:20]] + [(0,) * len(widths)]
        bcols, pcols = columns(bt, widths), columns(pt, widths)
        bv = list(range(1000, 1000 + len(bt)))
        want, coll = brute(H, bcols, bv, pcols, None, widths)
        assert coll == 0 and len(want) >= 2 + 150
        for off_b, off_p in ((0, 0), (1, 3), (5, 2)):
            res, info = join(ex, dev_rel(bcols, bv, off_b), dev_rel(pcols, None, off_p), H.HMJ_ORDERED | H.HMJ_CHECKSUM)
            assert np.array_equal(ex.cols_rows_to_numpy(res), want), (widths, off_b, off_p)
            assert res.checks() == checks_of(want)
    zb, zp = columns([(0, i % 50) for i in range(300)], [4, 4]), columns([(0, i % 70) for i in range(200)], [4, 4])
    want, _ = brute(H, zb, None, zp, None, [4, 4])
    res, info = join(ex, dev_rel(zb, None), dev_rel(zp, None), H.HMJ_ORDERED)
    assert len(want) > 500 and np.array_equal(ex.cols_rows_to_numpy(res), want)


def test_argument_errors_leave_the_ctx_usable(H, ex):
    import torch

    L, h = ex.L, ex.h
    n = 100
    a = torch.arange(n, dtype=torch.int32, device="cuda")
    b = torch.arange(n, dtype=torch.int16, device="cuda")
    raw = torch.zeros(4 * n + 8, dtype=torch.uint8, device="cuda")

    def rel(cols, n_rows=n, reserved=0, n_cols=None, null_cols=False):
        arr = (H.KeyCol * max(len(cols), 1))()
        for k, (ptr, width, res) in enumerate(cols):
            arr[k].data, arr[k].width, arr[k].reserved = ptr, width, res
        r = H.ColsRel()
        r.cols = None if null_cols else arr
        r.n_cols = len(cols) if n_cols is None else n_cols
        r.reserved, r.vals, r.n = reserved, None, n_rows
        return r, arr

    def opts(size=None, bits=0):
        o = H.ColsJoinOpts()
        o.struct_size = C.sizeof(H.ColsJoinOpts) if size is None else size
        o.hash_bits = bits
        return o

    def call(rb, rp, flags=0, o=None, out=True):
        o = opts() if o is None else o
        res = H.ColsResult()
        return L.hmj_join_cols_device(h, C.byref(rb[0]) if rb else None, C.byref(rp[0]) if rp else None, flags,
                                      C.byref(o) if o is not False else None, C.byref(res) if out else None), res

    good = [(a.data_ptr(), 4, 0), (b.data_ptr(), 2, 0)]
    G = rel(good)
    bad_calls = {
        "NULL build": lambda: call(None, G),
        "NULL probe": lambda: call(G, None),
        "NULL opts": lambda: call(G, G, o=False),
        "NULL out": lambda: call(G, G, out=False),
        "struct_size": lambda: call(G, G, o=opts(size=8)),
        "n_cols 0": lambda: call(rel(good, n_cols=0), G),
        "n_cols 9": lambda: call(rel([(a.data_ptr(), 4, 0)] * 9), rel([(a.data_ptr(), 4, 0)] * 9)),
        "NULL cols": lambda: call(rel(good, null_cols=True), G),
        "width 3": lambda: call(rel([(a.data_ptr(), 3, 0), (b.data_ptr(), 2, 0)]), G),
        "width 16": lambda: call(G, rel([(a.data_ptr(), 16, 0), (b.data_ptr(), 2, 0)])),
        "width 0": lambda: call(rel([(a.data_ptr(), 0, 0), (b.data_ptr(), 2, 0)]), G),
        "NULL data": lambda: call(rel([(None, 4, 0), (b.data_ptr(), 2, 0)]), G),
        "misaligned": lambda: call(G, rel([(raw.data_ptr() + 1, 4, 0), (b.data_ptr(), 2, 0)])),
        "col reserved": lambda: call(rel([(a.data_ptr(), 4, 1), (b.data_ptr(), 2, 0)]), G),
        "rel reserved": lambda: call(G, rel(good, reserved=7)),
        "n_cols differ": lambda: call(G, rel(good[:1])),
        "widths differ": lambda: call(G, rel([(a.data_ptr(), 4, 0), (a.data_ptr(), 4, 0)])),
        "rows": lambda: call(rel(good, n_rows=1 << 32), G),
        "hash_bits": lambda: call(G, G, o=opts(bits=64)),
        "FIRST_WINS": lambda: call(G, G, flags=H.HMJ_FIRST_WINS),
        "FIRST_WINS ordered": lambda: call(G, G, flags=H.HMJ_FIRST_WINS | H.HMJ_ORDERED),
    }
    assert raw.data_ptr() % 4 == 0
    for name, fn in bad_calls.items():
        rc, _ = fn()
        assert rc == HMJ_E_ARG, name
        assert L.hmj_last_error(h), name
        rc, res = call(G, G)
        assert rc == 0 and int(res.n_matches) == n, name
    rc, _ = bad_calls["misaligned"]()
    assert rc == HMJ_E_ARG and b"aligned" in L.hmj_last_error(h) and b"probe" in L.hmj_last_error(h)
    # a struct_size that holds the in fields only is enough; the out fields beyond it stay untouched
    o = opts(size=12)
    o.form = 77
    rc, res = call(G, G, o=o)
    assert rc == 0 and int(res.n_matches) == n and o.form == 77 and o.struct_size == 12
    # n == 0 needs no data; the binding refuses tensors the device cannot read as columns before anything runs
    rc, res = call(rel([(None, 4, 0), (None, 2, 0)], n_rows=0), G)
    assert rc == 0 and int(res.n_matches) == 0
    for bad in (a.cpu(), torch.zeros((n, 2), dtype=torch.int32, device="cuda")[:, 0], torch.zeros((n, 1), dtype=torch.int32, device="cuda")):
        with pytest.raises(ValueError):
            ex.join_cols_device([bad, b], None, [a, b], None)
    with pytest.raises(ValueError):
        ex.join_cols_device([a, b[:50]], None, [a, b], None)
    with pytest.raises(ValueError):
        ex.join_cols_device([a, b], torch.zeros(n - 1, dtype=torch.int64, device="cuda"), [a, b], None)
    with pytest.raises(H.HmjError) as e:
        ex.join_cols_device([a, b], None, [a, b], None, hash_bits=64)
    assert e.value.code == HMJ_E_ARG and "hash_bits" in str(e.value)
    res, info = ex.join_cols_device([a, b], None, [a, b], None, H.HMJ_ORDERED)
    assert int(res.n_matches) == n and info["form"] == H.HMJ_COLS_PACKED


def test_cols_joins_do_not_change_u64_plans(H):
    """The inner join of a multi-column join is the u64 join of the same sizes and mode flags; only the kind bits (14) of its
    workload signature tell the two apart.  A multi-column join with duplicate tuples teaches its workload a cool-down; a
    u64 join of the same sizes and flags must still plan exactly as on a fresh ctx."""
    import torch

    n = 1 << 20
    kind_bits = 15 << 20
    half = np.arange(n // 2, dtype=np.int64)
    # every tuple twice on each side: duplicate build keys in the inner {key64,row} join ([8,4]: the hashed form)
    c0 = torch.from_numpy(np.concatenate([half, half])).cuda()
    c1 = torch.from_numpy(np.concatenate([half, half]).astype(np.int32)).cuda()
    learnt = 0
    for flags in (H.HMJ_MATERIALIZE, H.HMJ_ORDERED):
        fresh = H.Executor(0)
        B, P = fresh.gen_build(n), fresh.gen_probe(n, n, miss_mod=3)
        r0 = fresh.columns_to_numpy(fresh.join_device(B, P, flags | H.HMJ_CHECKSUM), host=False)
        p0 = fresh.last_plan()
        fresh.close()
        ex2 = H.Executor(0)
        for _ in range(12):
            res, info = ex2.join_cols_device([c0, c1], None, [c0, c1], None, flags)
            assert int(res.n_matches) == 4 * (n // 2) and info["n_collisions"] == 0 and info["form"] == H.HMJ_COLS_HASHED
            learnt |= ex2.last_plan()["cooling"]
        pcols = ex2.last_plan()
        assert pcols["workload"] != p0["workload"]
        assert pcols["workload"] & ~kind_bits == p0["workload"] & ~kind_bits and pcols["workload"] & kind_bits == 14 << 20
        r1 = ex2.columns_to_numpy(ex2.join_device(B, P, flags | H.HMJ_CHECKSUM), host=False)
        p1 = ex2.last_plan()
        ex2.close()
        assert (p1["path"], p1["cooling"], p1["workload"]) == (p0["path"], p0["cooling"], p0["workload"]), (flags, p1, p0)
        if flags & H.HMJ_ORDERED:
            assert np.array_equal(r1, r0)
        else:
            assert np.array_equal(unordered(r1), unordered(r0))
    assert learnt, "the multi-column joins taught their workloads nothing: the test would not see a shared memo"


def test_a_cols_join_discards_a_prepared_build_side(H):
    os.environ["HMJ_GTABLE"] = "0"  # (a join this small would otherwise take the global table and partition nothing)
    try:
        e = H.Executor(0)
    finally:
        del os.environ["HMJ_GTABLE"]
    try:
        import torch

        nb, npb = 300000, 200000
        B, P = e.gen_build(nb), e.gen_probe(npb, nb, miss_mod=4)
        a = torch.arange(1000, dtype=torch.int32, device="cuda")
        e.set_profiling(True)
        e.prepare_build(B, npb)
        r = e.join_device(B, P, 0)
        want = int(r.n_matches)
        assert e.last_timing()["path"] & H.HMJ_PATH_PREPARED  # (the control: this shape does reuse a prepared build side)
        e.prepare_build(B, npb)
        res, _ = e.join_cols_device([a, a], None, [a, a], None, 0)
        assert int(res.n_matches) == 1000
        r = e.join_device(B, P, 0)
        t = e.last_timing()
        assert int(r.n_matches) == want and not (t["path"] & H.HMJ_PATH_PREPARED) and t["ms_partition_build"] > 0.0
        assert not (e.last_plan()["path"] & H.HMJ_PATH_PREPARED)
        e.prepare_build(B, npb)
        res, _ = e.join_cols_device([a[:0], a[:0]], None, [a, a], None, 0)  # also when given no rows
        r = e.join_device(B, P, 0)
        assert int(r.n_matches) == want and not (e.last_timing()["path"] & H.HMJ_PATH_PREPARED)
    finally:
        e.close()


def make_big():
    """2^20 x 2^20 rows: unique build tuples (a, b), every fourth probe row missing.  The expectation comes from numpy:
    np.unique over the stacked columns numbers the tuples, a sort-merge over those numbers pairs the rows.  Computed once
    (np.unique over rows is the slow part) and shared: the packed case joins on (the low half of a, b), and the low halves of
    a's values are distinct exactly as a's values are, so the same rows match."""
    n = 1 << 20
    rng = np.random.default_rng(2020)
    a = rng.permutation(n).astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15)  # distinct 64-bit values, distinct low halves
    b = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    pick = rng.integers(0, n, n)
    pa, pb = a[pick].copy(), b[pick].copy()
    pb[::4] ^= np.uint32(0x80000000)  # every fourth probe row: a tuple the build side does not hold
    bv = rng.integers(0, 1 << 63, n, dtype=np.uint64)
    pv = rng.integers(0, 1 << 63, n, dtype=np.uint64)
    stacked = np.concatenate([np.stack([a, b.astype(np.uint64)], 1), np.stack([pa, pb.astype(np.uint64)], 1)])
    _, inv = np.unique(stacked, axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    ib, ip = inv[:n], inv[n:]
    order = np.argsort(ib, kind="stable")
    sb = ib[order]
    assert np.all(np.diff(sb) > 0)  # unique build tuples
    lo, hi = np.searchsorted(sb, ip, "left"), np.searchsorted(sb, ip, "right")
    hit = hi > lo
    assert len(np.unique(a.astype(np.uint32))) == n
    return {"n": n, "a": a, "b": b, "pa": pa, "pb": pb, "bv": bv, "pv": pv, "r_row": order[lo[hit]], "s_row": np.flatnonzero(hit)}


@pytest.fixture(scope="module")
def big():
    return make_big()


@pytest.mark.parametrize("form", ["packed", "hashed"])
def test_large_against_numpy(H, ex, big, form):
    from test_join_kinds_cpu import tmix

    n = big["n"]
    if form == "packed":
        widths = [4, 4]
        bcols, pcols = [big["a"].astype(np.uint32), big["b"]], [big["pa"].astype(np.uint32), big["pb"]]
    else:
        widths = [8, 4]
        bcols, pcols = [big["a"], big["b"]], [big["pa"], big["pb"]]
    r_row, s_row = big["r_row"], big["s_row"]  # r_row, s_row of every match, ascending s_row
    assert len(r_row) == n - (n + 3) // 4
    rv, sv = big["bv"][r_row], big["pv"][s_row]
    m = tmix(H.cols_key64([c[s_row] for c in pcols], widths), rv, sv)
    with np.errstate(over="ignore"):
        want = {"n_matches": len(r_row), "sum_r": int(rv.sum(dtype=np.uint64)), "sum_s": int(sv.sum(dtype=np.uint64)),
                "xor_fold": int(np.bitwise_xor.reduce(m)), "mix_sum": int(m.sum(dtype=np.uint64))}
        want_sp = int(big["pv"].sum(dtype=np.uint64))
    B, P = dev_rel(bcols, big["bv"]), dev_rel(pcols, big["pv"])
    res, info = join(ex, B, P, H.HMJ_CHECKSUM | H.HMJ_SUM_PROBE)
    assert res.checks() == want and int(res.sum_probe_all) == want_sp
    assert info["form"] == (H.HMJ_COLS_PACKED if form == "packed" else H.HMJ_COLS_HASHED) and info["n_collisions"] == 0
    res, info = join(ex, B, P, H.HMJ_ORDERED | H.HMJ_CHECKSUM)
    assert res.checks() == want
    got = ex.cols_rows_to_numpy(res)
    assert np.all(got[1:, 0] >= got[:-1, 0])
    assert np.array_equal(np.sort(got[:, 2].astype(np.int64)), s_row)
    o = np.argsort(got[:, 2].astype(np.int64))
    assert np.array_equal(got[o, 1].astype(np.int64), r_row) and np.array_equal(got[o, 3], rv) and np.array_equal(got[o, 4], sv)
