"""GPU checks of the string-key join (hmj_hash_str_device / hmj_join_str_device): hashes against libstdc++'s
std::hash<std::string> (tests/golden/str_hash.json), the reference's own string-key benchmark relations against the compiled
reference's record (golden.json strgen_join / string_join), duplicates, misses, forced hash collisions and edge keys
against a Python dict brute force, errors, and the planner's isolation of string joins from u64 joins."""
import json
import os
import random

import numpy as np
import pytest

from test_join_str_cpu import M64, load_str_hash_golden, str_hash

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HMJ_E_ARG = -1


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


@pytest.fixture(scope="module")
def G():
    with open(os.path.join(ROOT, "tests", "golden", "golden.json")) as f:
        return json.load(f)["cases"]


@pytest.fixture(scope="module")
def words():
    txt = open(os.path.join(ROOT, "tests", "golden", "words.txt")).read()
    w = txt.split("\n")
    return w[:-1] if w and w[-1] == "" else w


def rel(H, keys, vals, shift=0, base=0):
    """(chars, offsets, vals) on the device; shift: chars start `shift` bytes past an aligned allocation; base: offsets[0]."""
    import torch

    chars, offsets = H.pack_strings(keys)
    buf = torch.zeros(shift + base + chars.numel() + 16, dtype=torch.uint8)
    buf[shift + base:shift + base + chars.numel()] = chars
    d = buf.cuda()
    return d[shift:], (offsets + base).cuda(), torch.tensor(np.asarray(vals, np.uint64).view(np.int64), device="cuda")


def rows_of(ex, res):
    return ex.str_rows_to_numpy(res)


def fnv_pairs(rows):
    """FNV-1a over the little-endian bytes of the (rval, sval) rows: the C loop of the oracle over whole triples of
    words, the rest continued here (FNV-1a's state is the running hash alone)."""
    from oracle.pyoracle import Oracle

    a = np.ascontiguousarray(rows, np.uint64).reshape(-1)
    k = len(a) // 3 * 3
    h = Oracle().fnv1a_triples(a[:k].reshape(-1, 3)) if k else 0xCBF29CE484222325
    for b in a[k:].tobytes():
        h = ((h ^ b) * 0x100000001B3) & M64
    return h


def brute(bk, bv, pk, pv, bits=0):
    """Expected rows (hash, r_row, s_row, rval, sval) sorted by (hash, key bytes, r_row, s_row), and the pairs of equal
    hash whose keys differ."""
    bk = [k.encode() if isinstance(k, str) else k for k in bk]
    pk = [k.encode() if isinstance(k, str) else k for k in pk]
    by_key = {}
    for r, k in enumerate(bk):
        by_key.setdefault(k, []).append(r)
    hb = [str_hash(k, bits) for k in bk]
    hp = [str_hash(k, bits) for k in pk]
    rows = []
    for s, k in enumerate(pk):
        for r in by_key.get(k, ()):
            rows.append((hp[s], k, r, s))
    rows.sort()
    out = np.array([(h, r, s, bv[r], pv[s]) for h, _, r, s in rows], np.uint64).reshape(-1, 5)
    cb, cp = {}, {}
    for h in hb:
        cb[h] = cb.get(h, 0) + 1
    for h in hp:
        cp[h] = cp.get(h, 0) + 1
    same_hash = sum(cb[h] * cp.get(h, 0) for h in cb)
    return out, same_hash - len(rows)


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


# ---------------------------------------------------------------------------------------------
def test_hash_str_device_equals_libstdcxx(H, ex):
    cases = load_str_hash_golden()
    keys = [k for k, _ in cases]
    want = np.array([h for _, h in cases], np.uint64)
    for shift, base in ((0, 0), (1, 0), (2, 5), (3, 0), (4, 17), (5, 0), (6, 3), (7, 1000)):
        chars, offsets, _ = rel(H, keys, np.zeros(len(keys), np.uint64), shift, base)
        got = ex.hash_str_device(chars, offsets).cpu().numpy().view(np.uint64)
        assert np.array_equal(got, want), (shift, base, np.flatnonzero(got != want)[:5])
    chars, offsets, _ = rel(H, keys, np.zeros(len(keys), np.uint64), 3, 0)
    got = ex.hash_str_device(chars, offsets, hash_bits=12).cpu().numpy().view(np.uint64)
    assert np.array_equal(got, want >> np.uint64(52))


def _check_against_reference(H, ex, bk, bv, pk, pv, count, sm, fnv):
    B, P = rel(H, bk, bv), rel(H, pk, pv)
    res, info = ex.join_str_device(B, P, H.HMJ_ORDERED)
    rows = rows_of(ex, res)
    assert (int(res.n_matches), (int(res.sum_r) + int(res.sum_s)) & M64) == (count, sm)
    assert fnv_pairs(rows[:, 3:5]) == fnv
    assert info["n_collisions"] == 0 and info["n_hash_pairs"] == count
    assert np.all(np.diff(rows[:, 0].astype(np.float64)) >= 0)
    cnt, _ = ex.join_str_device(B, P, 0)
    assert (int(cnt.n_matches), (int(cnt.sum_r) + int(cnt.sum_s)) & M64) == (count, sm)


def test_reference_parity_strgen(H, ex, G, words):
    from oracle.pyoracle import create_strvec

    seen = set()
    for c in G["strgen_join"]:
        if c["n"] not in (1000, 4096, 65536, 262144, 10 ** 6):
            continue
        seen.add(c["n"])
        r = create_strvec(c["n"], words, c["seed_r"])
        s = create_strvec(c["n"], words, c["seed_s"])
        _check_against_reference(H, ex, [k for k, _ in r], [v for _, v in r], [k for k, _ in s], [v for _, v in s],
                                 c["count"], c["sum"], c["fnv_pairs"])
    assert seen == {1000, 4096, 65536, 262144, 10 ** 6}


def _synth_key(i, seed):
    from oracle.pyoracle import strgen_mix64

    return "w%d-%d" % (strgen_mix64(i + seed) % 1000003, i)


def test_reference_parity_string_join(H, ex, G):
    assert len(G["string_join"]) == 3
    for c in G["string_join"]:
        nr, ns, seed = c["nr"], c["ns"], c["seed"]
        ri = [(2654435761 * k + 1) % nr for k in range(nr)]
        si = [(40503 * k + 5) % ns for k in range(ns)]
        _check_against_reference(H, ex, [_synth_key(i, seed) for i in ri], ri, [_synth_key(nr // 2 + i, seed) for i in si],
                                 [7 * i + 3 for i in si], c["n"], c["sum"], c["fnv_pairs"])


def _dup_relations(rng, n_keys, max_len=40):
    keys = set()
    while len(keys) < n_keys:
        keys.add(bytes(rng.randrange(256) for _ in range(rng.randrange(max_len + 1))))
    keys = sorted(keys)
    rng.shuffle(keys)
    build_keys = keys[: 2 * n_keys // 3]
    bk = [k for k in build_keys for _ in range(rng.randrange(1, 9))]
    pk = [k for k in keys for _ in range(rng.randrange(1, 9))]  # a third of the probe keys have no build row
    rng.shuffle(bk)
    rng.shuffle(pk)
    bv = [rng.getrandbits(64) for _ in bk]
    pv = [rng.getrandbits(64) for _ in pk]
    return bk, bv, pk, pv


def test_duplicates_and_misses(H, ex):
    rng = random.Random(5)
    bk, bv, pk, pv = _dup_relations(rng, 600)
    want, coll = brute(bk, bv, pk, pv)
    assert coll == 0 and len(want) > 1000
    B, P = rel(H, bk, bv, 3, 11), rel(H, pk, pv, 5, 0)
    res, info = ex.join_str_device(B, P, H.HMJ_MATERIALIZE | H.HMJ_CHECKSUM)
    assert np.array_equal(unordered(rows_of(ex, res)), unordered(want))
    assert res.checks() == checks_of(want)
    res, info = ex.join_str_device(B, P, H.HMJ_ORDERED | H.HMJ_CHECKSUM | H.HMJ_SUM_PROBE)
    assert np.array_equal(rows_of(ex, res), want)
    assert res.checks() == checks_of(want) and int(res.sum_probe_all) == sum(pv) & M64
    res, info = ex.join_str_device(B, P, H.HMJ_CHECKSUM | H.HMJ_SUM_PROBE)
    assert res.checks() == checks_of(want) and int(res.sum_probe_all) == sum(pv) & M64 and not res.hash


@pytest.mark.parametrize("bits,n_keys", [(8, 300), (12, 4000), (16, 30000)])
def test_forced_collisions(H, ex, bits, n_keys):
    rng = random.Random(bits)
    bk, bv, pk, pv = _dup_relations(rng, n_keys, 24)
    if bits == 16:  # (fewer duplicates: the brute force stays quick)
        bk, bv, pk, pv = bk[: len(bk) // 3], bv[: len(bv) // 3], pk[: len(pk) // 3], pv[: len(pv) // 3]
    want, coll = brute(bk, bv, pk, pv, bits)
    assert coll > 0
    B, P = rel(H, bk, bv), rel(H, pk, pv)
    res, info = ex.join_str_device(B, P, H.HMJ_MATERIALIZE, hash_bits=bits)
    assert np.array_equal(unordered(rows_of(ex, res)), unordered(want))
    assert info["n_collisions"] == coll and info["n_hash_pairs"] == len(want) + coll
    res, info = ex.join_str_device(B, P, H.HMJ_ORDERED | H.HMJ_CHECKSUM, hash_bits=bits)
    got = rows_of(ex, res)
    assert np.array_equal(got, want), np.flatnonzero(np.any(got != want, axis=1))[:5] if got.shape == want.shape else got.shape
    assert info["n_collisions"] == coll and res.checks() == checks_of(want)
    # rows inside every run of equal hash are in key order
    keys = [bk[int(r)] for r in got[:, 1]]
    for i in range(1, len(got)):
        if got[i, 0] == got[i - 1, 0]:
            assert keys[i - 1] <= keys[i]
    cnt, info = ex.join_str_device(B, P, 0, hash_bits=bits)
    assert int(cnt.n_matches) == len(want) and info["n_collisions"] == coll


def test_edge_keys(H, ex):
    rng = random.Random(9)
    lengths = [0, 1, 7, 8, 9, 63, 64, 65, 255, 256, 257, 4096, 10 ** 5]
    hit = [bytes(rng.randrange(256) for _ in range(n)) for n in lengths]
    miss = [k[:-1] + bytes([(k[-1] + 1) & 0xFF]) for k in hit if k]  # same lengths, last byte differs
    small = [b"s%d" % i for i in range(200)]  # waves whose span stays in LDS next to ones that do not
    bk = small + hit + small[:50]
    pk = miss + hit[::-1] + small[::3] + [b"x" * 4096] * 3
    bv = list(range(100, 100 + len(bk)))
    pv = list(range(7, 7 + len(pk)))
    want, coll = brute(bk, bv, pk, pv)
    assert coll == 0
    for shift in (0, 1, 7):
        B, P = rel(H, bk, bv, shift, 3), rel(H, pk, pv, 8 - shift, 0)
        res, _ = ex.join_str_device(B, P, H.HMJ_ORDERED)
        assert np.array_equal(rows_of(ex, res), want), shift
        got = ex.hash_str_device(B[0], B[1]).cpu().numpy().view(np.uint64)
        assert [int(x) for x in got] == [str_hash(k) for k in bk]


def test_empty_sides_all_miss_and_null_chars(H, ex):
    import torch

    B = rel(H, ["a", "b", "c"], [1, 2, 3])
    E = rel(H, [], [])
    for flags in (0, H.HMJ_ORDERED):
        res, info = ex.join_str_device(B, E, flags)
        assert int(res.n_matches) == 0 and info["n_hash_pairs"] == 0
        res, info = ex.join_str_device(E, B, flags | H.HMJ_SUM_PROBE)
        assert int(res.n_matches) == 0 and int(res.sum_probe_all) == 6
    P = rel(H, ["d", "e", "", "ab"], [4, 5, 6, 7])
    res, info = ex.join_str_device(B, P, H.HMJ_ORDERED)
    assert int(res.n_matches) == 0 and len(rows_of(ex, res)) == 0
    # every key empty: chars may be NULL
    off_b = torch.zeros(6, dtype=torch.int64, device="cuda")
    off_p = torch.full((4,), 9, dtype=torch.int64, device="cuda")
    vb = torch.arange(5, dtype=torch.int64, device="cuda")
    vp = torch.arange(10, 13, dtype=torch.int64, device="cuda")
    res, info = ex.join_str_device((None, off_b, vb), (None, off_p, vp), H.HMJ_ORDERED)
    got = rows_of(ex, res)
    h0 = str_hash(b"")
    want = np.array([(h0, r, s, r, 10 + s) for r in range(5) for s in range(3)], np.uint64)
    assert np.array_equal(got, want)
    assert [int(x) for x in ex.hash_str_device(None, off_b).cpu().numpy().view(np.uint64)] == [h0] * 5


def test_errors_leave_the_ctx_usable(H, ex):
    import torch

    B = rel(H, ["aa", "bb", "cc", "dd"], [1, 2, 3, 4])
    chars, offs, vals = B
    bad = offs.clone()
    bad[3] = 1  # offsets 0 2 4 1 8: decrease at row 2
    with pytest.raises(H.HmjError) as e:
        ex.join_str_device((chars, bad, vals), B, H.HMJ_ORDERED)
    assert e.value.code == HMJ_E_ARG and "row 2" in str(e.value) and "build" in str(e.value)
    with pytest.raises(H.HmjError) as e:
        ex.hash_str_device(chars, bad)
    assert e.value.code == HMJ_E_ARG and "row 2" in str(e.value)
    res, _ = ex.join_str_device(B, B, H.HMJ_ORDERED)
    assert int(res.n_matches) == 4 and [tuple(r[1:3]) for r in rows_of(ex, res)] == sorted(
        [(i, i) for i in range(4)], key=lambda t: str_hash([b"aa", b"bb", b"cc", b"dd"][t[0]]))
    for flags, bits in ((H.HMJ_FIRST_WINS, 0), (H.HMJ_FIRST_WINS | H.HMJ_ORDERED, 0), (0, 64)):
        with pytest.raises(H.HmjError) as e:
            ex.join_str_device(B, B, flags, hash_bits=bits)
        assert e.value.code == HMJ_E_ARG
    with pytest.raises(H.HmjError) as e:
        ex.hash_str_device(chars, offs, hash_bits=64)
    assert e.value.code == HMJ_E_ARG
    with pytest.raises(H.HmjError) as e:  # key bytes without chars
        ex.join_str_device((None, offs, vals), B, 0)
    assert e.value.code == HMJ_E_ARG
    # the binding refuses columns the device cannot read as n + 1 64-bit offsets before anything runs
    for bad_offs in (offs.cpu(), offs.to(torch.int32), torch.zeros(0, dtype=torch.int64, device="cuda"),
                     torch.zeros((5, 1), dtype=torch.int64, device="cuda")):
        with pytest.raises(ValueError):
            ex.hash_str_device(None, bad_offs)
        with pytest.raises(ValueError):
            ex.join_str_device((chars, bad_offs, vals), B, 0)
    with pytest.raises(ValueError):
        ex.join_str_device((chars.cpu(), offs, vals), B, 0)
    res, _ = ex.join_str_device(B, B, 0)
    assert int(res.n_matches) == 4


def decimal_keys(lo, hi):
    """chars / offsets (numpy) of the keys "k%d" for lo <= i < hi, built without a Python loop over the rows."""
    v = np.arange(lo, hi, dtype=np.int64)
    nd = np.ones(len(v), np.int64)
    for p in range(1, 19):
        nd += v >= 10 ** p
    offsets = np.zeros(len(v) + 1, np.int64)
    np.cumsum(nd + 1, out=offsets[1:])
    chars = np.empty(int(offsets[-1]), np.uint8)
    chars[offsets[:-1]] = ord("k")
    for p in range(int(nd.max())):
        sel = nd > p
        chars[offsets[:-1][sel] + nd[sel] - p] = ord("0") + (v[sel] // 10 ** p) % 10
    return chars, offsets


def test_large_count_join(H, ex):
    import torch

    c, o = decimal_keys(98, 102)
    assert [c.tobytes()[o[i]:o[i + 1]] for i in range(4)] == [b"k98", b"k99", b"k100", b"k101"]
    N = 1 << 24
    cb, ob = decimal_keys(0, N)
    cp, op = decimal_keys(N // 2, N // 2 + N)
    B = (torch.from_numpy(cb).cuda(), torch.from_numpy(ob).cuda(), torch.arange(N, dtype=torch.int64, device="cuda"))
    P = (torch.from_numpy(cp).cuda(), torch.from_numpy(op).cuda(), torch.arange(N // 2, N // 2 + N, dtype=torch.int64, device="cuda"))
    res, info = ex.join_str_device(B, P, H.HMJ_SUM_PROBE)
    m = N // 2
    s = (N // 2 + N - 1) * m // 2  # sum of N/2 .. N-1
    assert (int(res.n_matches), int(res.sum_r), int(res.sum_s)) == (m, s, s)
    assert int(res.sum_probe_all) == (N // 2 + N // 2 + N - 1) * N // 2
    assert info["n_collisions"] == 0


def test_string_joins_do_not_change_u64_plans(H):
    """The inner join of a string join is the u64 join of the same sizes and mode flags; only the kind bits of its workload
    signature tell the two apart.  A string join with duplicate keys teaches its workload a cool-down (duplicate build
    hashes); a u64 join of the same sizes and flags must still plan exactly as on a fresh ctx."""
    import torch

    n = 1 << 20
    kind_bits = 15 << 20
    cb, ob = decimal_keys(0, n // 2)
    # every key twice on each side: duplicate build hashes in the inner {hash,row} join
    chars = torch.from_numpy(np.concatenate([cb, cb])).cuda()
    offs = torch.from_numpy(np.concatenate([ob[:-1], ob + ob[-1]])).cuda()
    S = (chars, offs, torch.arange(n, dtype=torch.int64, device="cuda"))
    learnt = 0
    for flags in (H.HMJ_MATERIALIZE, H.HMJ_ORDERED):
        fresh = H.Executor(0)
        B, P = fresh.gen_build(n), fresh.gen_probe(n, n, miss_mod=3)
        r0 = fresh.columns_to_numpy(fresh.join_device(B, P, flags | H.HMJ_CHECKSUM), host=False)
        p0 = fresh.last_plan()
        fresh.close()
        ex2 = H.Executor(0)
        for _ in range(3):
            res, info = ex2.join_str_device(S, S, flags)
            assert int(res.n_matches) == 4 * (n // 2) and info["n_collisions"] == 0
        pstr = ex2.last_plan()
        learnt |= pstr["cooling"]
        # same sizes and mode: the signatures differ in the kind bits only
        assert pstr["workload"] != p0["workload"]
        assert pstr["workload"] & ~kind_bits == p0["workload"] & ~kind_bits
        r1 = ex2.columns_to_numpy(ex2.join_device(B, P, flags | H.HMJ_CHECKSUM), host=False)
        p1 = ex2.last_plan()
        ex2.close()
        assert p1 == p0, (flags, p1, p0)
        if flags & H.HMJ_ORDERED:
            assert np.array_equal(r1, r0)
        else:
            assert np.array_equal(unordered(r1), unordered(r0))
    assert learnt, "the string joins taught their workloads nothing: the test would not see a shared memo"


def test_oversized_mixed_run_is_unsupported(H, ex):
    """hash_bits = 1: two hash values, each run of matched pairs holds ~1000+ distinct keys -- beyond one workgroup's
    collision sort.  Ordered joins return HMJ_E_UNSUPPORTED; unordered and count joins stay exact; the ctx stays usable."""
    keys = [b"u%d" % i for i in range(6000)]
    B = rel(H, keys[:4500], list(range(4500)))
    P = rel(H, keys[1500:], list(range(4500)))
    with pytest.raises(H.HmjError) as e:
        ex.join_str_device(B, P, H.HMJ_ORDERED, hash_bits=1)
    assert e.value.code == -5 and "1024 rows" in str(e.value)  # HMJ_E_UNSUPPORTED
    res, info = ex.join_str_device(B, P, H.HMJ_MATERIALIZE, hash_bits=1)
    got = rows_of(ex, res)
    assert len(got) == 3000 and np.array_equal(np.sort(got[:, 1]), np.arange(1500, 4500, dtype=np.uint64))
    assert np.array_equal(got[:, 2], got[:, 1] - np.uint64(1500))
    assert info["n_collisions"] == info["n_hash_pairs"] - 3000 > 0
    cnt, _ = ex.join_str_device(B, P, 0, hash_bits=1)
    assert int(cnt.n_matches) == 3000
    res, _ = ex.join_str_device(B, P, H.HMJ_ORDERED)
    assert int(res.n_matches) == 3000
