"""The case generators of the join-kind sweeps (test_kinds_sweep_gpu.py imports them) and their CPU-only checks: no drawn
u64 case is skipped and every one stays below 2^23 rows, the numpy expectations of the u64 kinds (expect_kind,
expect_build_kind) agree with each other and with the C oracle's equijoin on every drawn case, and -- on the drawn string
cases with full 64-bit hashes -- with the pure-Python brute force of the string kinds (kind_brute), each key relabelled by its
std::hash value.  The two references were written independently; the GPU sweeps lean on both."""
import math

import numpy as np

from test_join_build_kinds_cpu import BANTI, BOUTER, BSEMI, FULL, expect_build_kind
from test_join_kinds_cpu import ANTI, M64, OUTER, SEMI, _inner_rows, _mix64, expect_kind
from test_join_str_cpu import str_hash
from test_join_str_kinds_cpu import ALL_KINDS, BUILD, INNER, NO_ROW, PROBE, kind_brute, tmix_checks
import test_join_str_kinds_cpu as SK

U64_ITERS, U64_SEED = 30, 20251016  # defaults of the u64 sweep (HMJ_STRESS_ITERS / HMJ_STRESS_SEED override them)
STR_ITERS, STR_SEED = 20, 20251017  # ... and of the string sweep
ROW_CAP = 1 << 23                   # pairs + nb + np of a drawn u64 case, by construction (draw_u64_case)
RUN_CAP = 1024                      # strjoin.hip kRunCap: rows of one run of equal hash with more than one key

SIZES = [1, 2, 31, 32, 33, 63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097, 5119, 5120, 5121, 6143, 6144,
         6145, 8191, 10240, 16383, 16384, 16385, 20000, 65535, 65536, 65537, 100000, 262144, 300001]
DISTS = ["uniform", "dense", "dups", "sorted", "clustered"]

# (name, family, kind code, first-wins): what the u64 sweep runs on every case
VARIANTS = [("SEMI", "probe", SEMI, False), ("ANTI", "probe", ANTI, False), ("PROBE_OUTER", "probe", OUTER, False),
            ("PROBE_OUTER|FIRST_WINS", "probe", OUTER, True), ("SEMI|FIRST_WINS", "probe", SEMI, True),
            ("BUILD_SEMI", "build", BSEMI, False), ("BUILD_ANTI", "build", BANTI, False),
            ("BUILD_OUTER", "build", BOUTER, False), ("FULL_OUTER", "build", FULL, False)]
SEVEN = [v for v in VARIANTS if not v[3]]  # the seven kinds, without the first-wins forms


def _keys(rng, dist, n, dom):
    """The key distributions of test_gpu_join.test_randomized_shapes_and_flags."""
    if dist == "uniform":
        return rng.integers(0, 1 << 63, size=n, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=n, dtype=np.uint64)
    if dist == "dense":
        return rng.integers(0, dom, size=n, dtype=np.uint64)
    if dist == "dups":  # (below 5000 rows the few distinct values are mixed, above it multiplied, as there)
        v = rng.integers(0, max(2, dom // 50), size=n, dtype=np.uint64)
        with np.errstate(over="ignore"):
            return _mix64(v) if n < 5000 else v * np.uint64(0x9E3779B97F4A7C15)
    if dist == "sorted":
        return np.sort(rng.integers(0, 1 << 63, size=n, dtype=np.uint64))
    # clustered: only a few values of the top bits occur
    return (rng.integers(0, 3, size=n, dtype=np.uint64) << np.uint64(61)) | rng.integers(0, 1 << 40, size=n, dtype=np.uint64)


def draw_u64_case(rng, sizes=None):
    """(B, P, fills, tag): two [n, 2] uint64 relations, (probe_fill, build_fill) and tag = (nb, np, dist, dom, share, hot).
    The key domain is raised to at least 50 * ceil(nb * np / 2^22): `dups` then has at least ceil(nb np / 2^22) distinct
    keys and `dense` fifty times as many, so the cross product stays near 2^22 pairs whatever the sizes, and no case needs
    to be skipped.  The hot key is written after the probe keys were drawn from the build keys (a hot build key copied
    into the probe side as well would square).  `sizes`: the row counts to draw from (SIZES unless given; the random stream
    of the default is the one the sweeps have always drawn)."""
    sizes = SIZES if sizes is None else sizes
    nb, npb = int(rng.choice(sizes)), int(rng.choice(sizes))
    dist = str(rng.choice(DISTS))
    dom = max(int(rng.choice([97, 5000, 1 << 20])), 50 * -(-nb * npb // (1 << 22)))
    share = float(rng.choice([0.0, 0.3, 0.6, 1.0]))
    hot = str(rng.choice(["none", "probe", "build"]))
    kb = _keys(rng, dist, nb, dom)
    kp = np.where(rng.random(npb) < share, kb[rng.integers(0, nb, size=npb)], _keys(rng, dist, npb, dom))
    if hot == "probe" and npb > 64:
        kp[rng.random(npb) < 0.3] = kb[0]
    elif hot == "build" and nb > 64:
        kb[rng.random(nb) < 0.1] = kb[0]
    else:
        hot = "none"
    B = np.stack([kb, rng.integers(0, 1 << 62, size=nb, dtype=np.uint64)], 1)
    P = np.stack([kp, rng.integers(0, 1 << 62, size=npb, dtype=np.uint64)], 1)
    fills = tuple(0 if rng.integers(0, 4) == 0 else int(rng.integers(0, 1 << 63, dtype=np.uint64)) * 2 + int(rng.integers(0, 2))
                  for _ in range(2))
    return B, P, fills, (nb, npb, dist, dom, share, hot)


def n_pairs(B, P):
    """Rows of the inner join, from the key counts alone."""
    ub, cb = np.unique(B[:, 0], return_counts=True)
    up, cp = np.unique(P[:, 0], return_counts=True)
    _, ib, ip = np.intersect1d(ub, up, assume_unique=True, return_indices=True)
    return int((cb[ib].astype(np.int64) * cp[ip].astype(np.int64)).sum())


def expect_variant(B, P, variant, fills):
    """(rows, checks, counters) of one of VARIANTS, counters as the entry of its family reports them."""
    _, family, kind, first = variant
    pf, bf = fills
    if family == "probe":
        # (first-wins does not change SEMI)
        rows, ck, matched = expect_kind(B, P, kind, first_wins=first and kind == OUTER, fill=pf)
        return rows, ck, {"n_probe_matched": matched, "n_probe_unmatched": len(P) - matched}
    return expect_build_kind(B, P, kind, build_fill=bf, probe_fill=pf)


# ---------------------------------------------------------------------------------------------
def _rand_bytes(rng, n):
    """n random bytes, a fifth of them 0x00 or 0xFF."""
    a = rng.integers(0, 256, size=n, dtype=np.uint8)
    m = rng.random(n)
    a[m < 0.1] = 0
    a[m > 0.9] = 255
    return a.tobytes()


def key_of_row(bk, pk, r, s):
    return bk[int(r)] if int(r) != NO_ROW else pk[int(s)]


def ambiguous_runs(rows, bk, pk):
    """From result rows (kind_brute's) alone: (rows of the largest run of equal hash that holds more than one distinct key,
    whether such a run takes keys from both relations -- the collision sort's MIXED form)."""
    largest, mixed = 0, False
    i, n = 0, len(rows)
    while i < n:
        j = i + 1
        while j < n and rows[j, 0] == rows[i, 0]:
            j += 1
        if j - i > 1:
            keys = {key_of_row(bk, pk, rows[t, 1], rows[t, 2]) for t in range(i, j)}
            if len(keys) > 1:
                largest = max(largest, j - i)
                from_build = [int(rows[t, 1]) != NO_ROW for t in range(i, j)]
                mixed = mixed or (any(from_build) and not all(from_build))
        i = j
    return largest, mixed


STR_KEYS = (60, 7000)  # distinct keys of a drawn string case: log-uniform between the two


def draw_str_case(rng, sizes=STR_KEYS):
    """A dict: bk / bv / pk / pv (key bytes and 64-bit payloads of the build and the probe side), shift_b / base_b /
    shift_p / base_p for test_join_str_gpu.rel, hash_bits, mixed_run (an ordered outer join of the case sorts a run of equal
    hash with keys of both relations) and redraws.  Distinct keys from length classes: 1..8 bytes, 56..72 bytes (64 such
    keys span about the 4096 bytes a wave stages), the empty key in half the draws (keys are distinct, so `all empty` is one
    key with its copies), up to three keys of 4097..20000 bytes, proper prefixes of other keys and keys that differ from
    another in the last byte only; each key 1..4 times per side, a third of the keys on one side only.  `sizes`: (fewest, most) distinct keys."""
    n_keys = int(math.exp(rng.uniform(math.log(sizes[0]), math.log(sizes[1]))))
    p_short = float(rng.choice([0.1, 0.5, 0.85]))  # the rest from the 56..72 class
    keys = set()
    if rng.random() < 0.5:
        keys.add(b"")
    for _ in range(int(rng.integers(0, 4))):
        keys.add(_rand_bytes(rng, int(rng.integers(4097, 20001))))
    base = []
    while len(keys) < n_keys * 9 // 10:
        n = int(rng.integers(1, 9)) if rng.random() < p_short else int(rng.integers(56, 73))
        k = _rand_bytes(rng, n)
        if k not in keys:
            keys.add(k)
            base.append(k)
    while len(keys) < n_keys:  # a tenth of the keys derived from others
        k = base[int(rng.integers(0, len(base)))]
        if len(k) < 2:
            k = k + _rand_bytes(rng, 3)
        if rng.random() < 0.5:
            keys.add(k[: int(rng.integers(1, len(k)))])  # a proper prefix
        else:
            keys.add(k[:-1] + bytes([(k[-1] + 1 + int(rng.integers(0, 255))) & 0xFF]))  # the last byte differs
    keys = sorted(keys)
    bk, pk = [], []
    for k in keys:
        u = rng.random()
        if u < 5 / 6:
            bk += [k] * int(rng.integers(1, 5))
        if u < 2 / 3 or u >= 5 / 6:
            pk += [k] * int(rng.integers(1, 5))
    bk = [bk[i] for i in rng.permutation(len(bk))]
    pk = [pk[i] for i in rng.permutation(len(pk))]
    assert 50 <= len(bk) <= 20000 and 50 <= len(pk) <= 20000, (len(bk), len(pk))
    bv = [int(x) for x in rng.integers(0, 1 << 63, size=len(bk), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=len(bk), dtype=np.uint64)]
    pv = [int(x) for x in rng.integers(0, 1 << 63, size=len(pk), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=len(pk), dtype=np.uint64)]
    case = dict(bk=bk, bv=bv, pk=pk, pv=pv, n_keys=len(keys), shift_b=int(rng.integers(0, 8)), shift_p=int(rng.integers(0, 8)),
                base_b=int(rng.choice([0, 3, 1000])), base_p=int(rng.choice([0, 3, 1000])), redraws=0)
    bits = 0
    if rng.random() < 0.5:  # few hash bits: about four keys per hash value and fewer, collisions common, runs small
        bits = min(63, max(1, math.ceil(math.log2(len(keys))) - 2 + int(rng.integers(0, 4))))
    # the full outer join's rows hold every other kind's runs (each kind's rows of a hash value are among them)
    rows, _ = kind_brute(bk, bv, pk, pv, BUILD, SK.FULL_OUTER, bits)
    largest, mixed = ambiguous_runs(rows, bk, pk)
    if largest > RUN_CAP:
        bits, case["redraws"] = min(63, bits + 4), 1
        rows, _ = kind_brute(bk, bv, pk, pv, BUILD, SK.FULL_OUTER, bits)
        largest, mixed = ambiguous_runs(rows, bk, pk)
    assert largest <= RUN_CAP, (largest, bits, len(keys))
    case.update(hash_bits=bits, mixed_run=mixed, largest_run=largest)
    return case


def str_tag(case):
    return (len(case["bk"]), len(case["pk"]), case["n_keys"], case["hash_bits"], case["shift_b"], case["base_b"],
            case["shift_p"], case["base_p"])


# ---------------------------------------------------------------------------------------------
def _sorted(a):
    a = np.ascontiguousarray(a, np.uint64)
    return a[np.lexsort(tuple(a[:, k] for k in reversed(range(a.shape[1]))))] if len(a) else a


def test_dups_keys_use_the_oracle_mix(oracle):
    v = np.array([0, 1, 2, 96, 12345, (1 << 64) - 1], np.uint64)
    assert [int(x) for x in _mix64(v)] == [oracle.mix64(int(x)) for x in v]


def test_no_u64_case_is_skipped_and_every_case_is_bounded():
    for seed in (U64_SEED, 1, 2):
        rng = np.random.default_rng(seed)
        largest, seen = 0, set()
        for it in range(U64_ITERS):
            B, P, fills, tag = draw_u64_case(rng)
            assert (len(B), len(P)) == tag[:2] and B.dtype == P.dtype == np.uint64
            rows = n_pairs(B, P) + len(B) + len(P)
            assert rows <= ROW_CAP, (seed, it, tag, rows)  # a condition on the generator: nothing is ever dropped
            largest = max(largest, rows)
            seen.add(tag[2])
        assert seen == set(DISTS), (seed, seen)
        assert largest > 1 << 18, (seed, largest)  # ... and not by drawing small cases only


def test_u64_references_agree_with_each_other_and_the_oracle(oracle):
    rng = np.random.default_rng(U64_SEED)
    for it in range(U64_ITERS):
        B, P, (pf, bf), tag = draw_u64_case(rng)
        tag = (it,) + tag
        ck, inner = oracle.equijoin(B, P)
        _, inner_fw = oracle.equijoin(B, P, first_wins=True)
        bhit, phit = np.isin(B[:, 0], P[:, 0]), np.isin(P[:, 0], B[:, 0])
        semi, _, m1 = expect_kind(B, P, SEMI)
        anti, _, m2 = expect_kind(B, P, ANTI)
        assert m1 == m2 == len(semi) == len(P) - len(anti), tag
        assert np.array_equal(_sorted(np.concatenate([semi, anti])), _sorted(P)), tag
        bsemi, _, c1 = expect_build_kind(B, P, BSEMI)
        banti, _, c2 = expect_build_kind(B, P, BANTI)
        assert c1 == c2 and (c1["n_build_matched"], c1["n_build_unmatched"]) == (len(bsemi), len(banti)), tag
        assert np.array_equal(_sorted(np.concatenate([bsemi, banti])), _sorted(B)), tag
        # the pair rows inside the outer kinds are the oracle's equijoin (a pair row's key occurs on both sides)
        outer, ock, _ = expect_kind(B, P, OUTER, fill=pf)
        assert np.array_equal(outer[np.isin(outer[:, 0], B[:, 0])], inner), tag
        outer_fw, _, _ = expect_kind(B, P, OUTER, first_wins=True, fill=pf)
        assert np.array_equal(outer_fw[np.isin(outer_fw[:, 0], B[:, 0])], inner_fw), tag
        assert len(outer_fw) == len(P), tag
        bouter, _, _ = expect_build_kind(B, P, BOUTER, build_fill=bf)
        assert np.array_equal(bouter[np.isin(bouter[:, 0], P[:, 0])], inner), tag
        full, fck, fc = expect_build_kind(B, P, FULL, build_fill=bf, probe_fill=pf)
        both = np.isin(full[:, 0], B[:, 0]) & np.isin(full[:, 0], P[:, 0])
        assert np.array_equal(full[both], inner), tag
        assert (fc["n_probe_matched"], fc["n_build_matched"]) == (int(phit.sum()), int(bhit.sum())), tag
        # full outer = inner + anti rows with probe_fill + build-anti rows with build_fill, as multisets
        parts = [inner, np.stack([anti[:, 0], np.full(len(anti), pf, np.uint64), anti[:, 1]], 1),
                 np.stack([banti[:, 0], banti[:, 1], np.full(len(banti), bf, np.uint64)], 1)]
        assert np.array_equal(_sorted(np.concatenate(parts)), full), tag
        assert fck["n_matches"] == ck["n_matches"] + len(anti) + len(banti), tag
        assert ock["n_matches"] == ck["n_matches"] + len(anti), tag
        # expect_variant hands the same expectations to the GPU sweep
        for v in VARIANTS:
            rows, vck, cnt = expect_variant(B, P, v, (pf, bf))
            assert vck["n_matches"] == len(rows) and sum(cnt.values()) in (0, len(B), len(P), len(B) + len(P)), (tag, v)
        assert np.array_equal(expect_variant(B, P, VARIANTS[3], (pf, bf))[0], outer_fw), tag
        assert np.array_equal(expect_variant(B, P, VARIANTS[4], (pf, bf))[0], semi), tag


def test_string_cases_meet_their_conditions():
    rng = np.random.default_rng(STR_SEED)
    cases = [draw_str_case(rng) for _ in range(STR_ITERS)]
    for c in cases:
        assert c["redraws"] <= 1 and c["largest_run"] <= RUN_CAP
        assert 50 <= len(c["bk"]) <= 20000 and 50 <= len(c["pk"]) <= 20000
        assert len(c["bk"]) == len(c["bv"]) and len(c["pk"]) == len(c["pv"])
        assert set(c["bk"]) - set(c["pk"]) and set(c["pk"]) - set(c["bk"]) and set(c["bk"]) & set(c["pk"])
    keys = set().union(*[set(c["bk"]) | set(c["pk"]) for c in cases])
    lens = {len(k) for k in keys}
    assert 0 in lens and set(range(1, 9)) <= lens and set(range(56, 73)) <= lens and max(lens) > 4096 >= 72
    assert any(b"\x00" in k for k in keys) and any(b"\xff" in k for k in keys)
    assert any(c["hash_bits"] == 0 for c in cases) and any(c["hash_bits"] > 0 for c in cases)
    # what the GPU sweep's last two assertions need from the default seed
    assert any(c["mixed_run"] for c in cases)
    assert any(c["hash_bits"] and c["largest_run"] > 1 for c in cases)
    # some wave of 64 consecutive keys spans more than the 4096 staged bytes, another one less
    spans = [sum(len(k) for k in c["bk"][i:i + 64]) for c in cases for i in range(0, len(c["bk"]) - 63, 64)]
    assert min(spans) < 4096 < max(spans)


def test_string_brute_force_agrees_with_the_u64_expectations():
    rng = np.random.default_rng(STR_SEED)
    pf, bf = 0x1111222233334444, 0xAAAA0000BBBB0001
    done = 0
    for it in range(STR_ITERS):
        c = draw_str_case(rng)
        if c["hash_bits"]:
            continue
        done += 1
        bk, bv, pk, pv = c["bk"], c["bv"], c["pk"], c["pv"]
        h = {k: str_hash(k) for k in set(bk) | set(pk)}
        assert len(set(h.values())) == len(h), it  # injective: the relabelled join is the same join
        B = np.array([[h[k], v] for k, v in zip(bk, bv)], np.uint64).reshape(-1, 2)
        P = np.array([[h[k], v] for k, v in zip(pk, pv)], np.uint64).reshape(-1, 2)
        for side, kind in ALL_KINDS:
            brows, bcnt = kind_brute(bk, bv, pk, pv, side, kind, 0, pf, bf)
            tag = (it, side, kind)
            if (side, kind) == (PROBE, INNER):
                rows, _ = _inner_rows(B, P, False)
                assert np.array_equal(_sorted(rows), _sorted(brows[:, [0, 3, 4]])), tag
                assert set(bcnt.values()) == {0}
                continue
            if side == PROBE:
                rows, ck, matched = expect_kind(B, P, kind, fill=pf)
                cnt = {"n_probe_matched": matched, "n_probe_unmatched": len(P) - matched, "n_build_matched": 0,
                       "n_build_unmatched": 0}
                cols = [0, 4] if kind in (SEMI, ANTI) else [0, 3, 4]
            else:
                rows, ck, cnt = expect_build_kind(B, P, kind, build_fill=bf, probe_fill=pf)
                cols = [0, 3] if kind in (BSEMI, BANTI) else [0, 3, 4]
            assert cnt == bcnt, tag
            assert ck == tmix_checks(brows), tag
            assert np.array_equal(_sorted(rows), _sorted(brows[:, cols])), tag
            absent = brows[:, [c for c in (3, 4) if c not in cols]]
            assert not absent.any(), tag  # a value column the kind does not produce reads as 0
    assert done >= 3
