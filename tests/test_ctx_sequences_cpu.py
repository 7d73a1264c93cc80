"""Generators for the tests of ONE long-lived context under drawn sequences of mixed calls (test_ctx_sequences_gpu.py runs
them) and their CPU-only checks.

  * a case pool per seed, drawn from the sweeps' generators (draw_u64_case / draw_str_case with `sizes=`): about ten u64
    cases of at most 65 537 rows, two of 300 001, one pair of 2^22 + 5 rows per side (uniform keys, 60 % of the probe keys
    taken from the build side; count and checksum modes only; materialised lazily, never by a CPU test) and six string
    cases.  Expected rows are computed once per (case, kind or first-wins form); every mode of an op reads the same rows;
  * twelve op families and `draw_sequence`: a random Eulerian circuit on the complete directed graph with loops over the
    families -- F^2 + 1 ops in which every ordered pair "family x directly followed by family y" occurs by construction;
  * `Model`: the contract of hmj.h in plain Python -- the forced radix bits in force, the prepared build side (hmj.h names
    the calls that leave it in place), which joins may report HMJ_PATH_PREPARED, the status every op returns.

The checks here: every tour holds all F^2 transitions, every family and pool case is used, every drawn op has an
expectation (nothing is ever skipped), the size bounds hold, and the fast expectation of the big pair equals expect_variant
on a 2^16-row pair drawn the same way.  Expectations are COMPUTED here for the string cases and the u64 cases of up to
CPU_ROWS rows; for the larger u64 cases the same `expectation` code is only shown to apply (the op names a case and a kind
it serves), and for the big pair that its ops are those `fast_expect` serves: computing them, and building the big pair,
is left to the GPU run, which executes every drawn op and asserts that it did."""
import numpy as np

from test_join_kinds_cpu import ANTI, M64, OUTER, SEMI, _inner_rows, tmix
from test_join_build_kinds_cpu import BANTI, BOUTER, BSEMI, FULL
from test_join_str_cpu import str_hash
from test_join_str_kinds_cpu import ALL_KINDS, BUILD, FULL_OUTER, kind_brute
from test_kinds_sweep_cpu import (ROW_CAP, RUN_CAP, VARIANTS, _keys, ambiguous_runs, draw_str_case, draw_u64_case,
                                  expect_variant, n_pairs)

# hmj.h flag values (test_the_flag_values_are_the_bindings below)
MATERIALIZE, ORDERED, FIRST_WINS, CHECKSUM, SUM_PROBE = 1, 2, 4, 8, 16
E_ARG, E_UNSUPPORTED = -1, -5

SEQ_SEED, SEQ_TOURS = 20251102, 2  # defaults of the tours (HMJ_STRESS_SEED / HMJ_STRESS_ITERS override them)
FAMILIES = ("inner", "probe_kind", "build_kind", "str_inner", "str_kind", "sort_partition", "prepare", "host", "config",
            "prefix", "refused", "hash_str")
# the one chain of three the tours must hold: a sort between a prepare and the join that would have taken it (a sort that
# left the prepared state valid shows there and nowhere else: every join discards it rightly)
REQUIRED_CHAINS = (("prepare", "sort_partition", "inner"),)

SMALL_SIZES = [1, 2, 31, 32, 33, 63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097, 5119, 5120, 5121, 6143,
               6144, 6145, 8191, 10240, 16383, 16384, 16385, 20000, 65535, 65536, 65537]
N_SMALL, N_MID, MID_ROWS, BIG_ROWS = 10, 2, 300001, (1 << 22) + 5
POOL_ROWS = 1 << 20  # pairs + nb + np of a pool case (a case beyond it is drawn again: the tours read every result back)
N_STR, STR_POOL_KEYS = 6, (60, 2500)
BIG_SHARE = 0.6

# the nine flag sets of test_gpu_join.test_randomized_shapes_and_flags
INNER_FLAGS = [0, CHECKSUM, MATERIALIZE | CHECKSUM, ORDERED | CHECKSUM, FIRST_WINS | CHECKSUM | SUM_PROBE, FIRST_WINS | ORDERED,
               ORDERED | SUM_PROBE, FIRST_WINS | MATERIALIZE | CHECKSUM, FIRST_WINS | ORDERED | CHECKSUM]
KIND_MODES = [0, CHECKSUM, MATERIALIZE | CHECKSUM, ORDERED | CHECKSUM]
FORCED_BITS = [0, 1, 4, 8, 10, 12, 14]
REFUSALS = ("unknown_kind", "struct_too_small", "first_wins_outer", "too_many_rows", "null_relation", "partition_bits_10",
            "radix_bits_40", "decreasing_offsets", "oversized_mixed_run")
# the relations of the oversized mixed run (test_join_str_gpu.test_oversized_mixed_run_is_unsupported)
OVERSIZED_KEYS = [b"u%d" % i for i in range(6000)]
OVERSIZED = dict(bk=OVERSIZED_KEYS[:4500], bv=list(range(4500)), pk=OVERSIZED_KEYS[1500:], pv=list(range(4500)), hash_bits=1)


def materialising(flags):
    return bool(flags & (MATERIALIZE | ORDERED))


def checks_of_rows(tri):
    """n_matches, sums and HMJ_CHECKSUM's folds of [n, 3] (key, rval, sval) rows."""
    m = tmix(tri[:, 0], tri[:, 1], tri[:, 2]) if len(tri) else np.zeros(0, np.uint64)
    with np.errstate(over="ignore"):
        return {"n_matches": len(tri), "sum_r": int(tri[:, 1].sum(dtype=np.uint64)) & M64,
                "sum_s": int(tri[:, 2].sum(dtype=np.uint64)) & M64,
                "xor_fold": int(np.bitwise_xor.reduce(m)) if len(m) else 0, "mix_sum": int(m.sum(dtype=np.uint64)) & M64}


def expect_inner(B, P, first_wins):
    """(rows in HMJ_ORDERED order, checks) of the inner join (the numpy rows of expect_kind's outer join, without the fills;
    test_the_inner_expectation_is_the_oracles pins them to the C oracle)."""
    tri = _inner_rows(B, P, first_wins)[0].reshape(-1, 3)
    tri = tri[np.lexsort((tri[:, 2], tri[:, 1], tri[:, 0]))] if len(tri) else tri
    return np.ascontiguousarray(tri), checks_of_rows(tri)


def draw_big_pair(rng, n, share=BIG_SHARE):
    """n rows per side: uniform 64-bit build keys, `share` of the probe keys copied from build rows."""
    kb = _keys(rng, "uniform", n, 0)
    kp = np.where(rng.random(n) < share, kb[rng.integers(0, n, size=n)], _keys(rng, "uniform", n, 0))
    B = np.stack([kb, rng.integers(0, 1 << 62, size=n, dtype=np.uint64)], 1)
    P = np.stack([kp, rng.integers(0, 1 << 62, size=n, dtype=np.uint64)], 1)
    return B, P


def fast_expect(B, P, vkey, fills, cache):
    """(None, checks, counters) of "inner" / "inner_fw" / a VARIANTS index over whole relations without sorting rows, as
    test_exchange_kinds_gpu.fast_expected computes them (here with the case's fills and the first-wins forms)."""
    pf, bf = fills
    if "phit" not in cache:
        cache["phit"] = np.isin(P[:, 0], B[:, 0])
        cache["bhit"] = np.isin(B[:, 0], P[:, 0])
    phit, bhit = cache["phit"], cache["bhit"]

    def inner(first):
        key = "inner_fw" if first else "inner"
        if key not in cache:
            cache[key] = _inner_rows(B, P, first)[0].reshape(-1, 3)
        return cache[key]

    z = lambda n, v=0: np.full(n, v, np.uint64)
    if vkey in ("inner", "inner_fw"):
        parts, counters = [inner(vkey == "inner_fw")], None
    else:
        _, family, kind, first = VARIANTS[vkey]
        npm, nbm = int(phit.sum()), int(bhit.sum())
        if family == "probe":
            counters = {"n_probe_matched": npm, "n_probe_unmatched": len(P) - npm}
            if kind in (SEMI, ANTI):
                sel = P[phit] if kind == SEMI else P[~phit]
                parts = [np.stack([sel[:, 0], z(len(sel)), sel[:, 1]], 1)]
            else:
                pm = P[~phit]
                parts = [inner(first), np.stack([pm[:, 0], z(len(pm), pf), pm[:, 1]], 1)]
        else:
            full = kind == FULL
            counters = {"n_build_matched": nbm, "n_build_unmatched": len(B) - nbm, "n_probe_matched": npm if full else 0,
                        "n_probe_unmatched": len(P) - npm if full else 0}
            if kind in (BSEMI, BANTI):
                sel = B[bhit] if kind == BSEMI else B[~bhit]
                parts = [np.stack([sel[:, 0], sel[:, 1], z(len(sel))], 1)]
            else:
                bm = B[~bhit]
                parts = [inner(False), np.stack([bm[:, 0], bm[:, 1], z(len(bm), bf)], 1)]
                if full:
                    pm = P[~phit]
                    parts.append(np.stack([pm[:, 0], z(len(pm), pf), pm[:, 1]], 1))
    ck = {"n_matches": 0, "sum_r": 0, "sum_s": 0, "xor_fold": 0, "mix_sum": 0}
    for part in parts:
        c = checks_of_rows(part.reshape(-1, 3))
        for k in ("n_matches", "sum_r", "sum_s", "mix_sum"):
            ck[k] = (ck[k] + c[k]) & M64
        ck["xor_fold"] ^= c["xor_fold"]
    return None, ck, counters


def shared_prefix_bits(B, P):
    """The top bits in which every key of both relations agrees (what hmj_set_key_prefix_bits' caller may promise)."""
    k = np.concatenate([B[:, 0], P[:, 0]])
    if not len(k):
        return 64
    return 64 - int(np.bitwise_or.reduce(k ^ k[0])).bit_length()


def expect_partition(a, shift, bits):
    """One stable radix pass: (rows grouped by digit in input order, [2^bits + 1] offsets)."""
    d = ((a[:, 0] >> np.uint64(shift)) & np.uint64((1 << bits) - 1)).astype(np.int64)
    off = np.zeros((1 << bits) + 1, np.int64)
    np.cumsum(np.bincount(d, minlength=1 << bits), out=off[1:])
    return a[np.argsort(d, kind="stable")], off


# ---------------------------------------------------------------------------------------------
class Pool:
    """The cases of one seed and their expectations, each computed once."""

    def __init__(self, seed):
        rng = np.random.default_rng([int(seed), 1])
        self.seed = int(seed)
        self.u64 = []  # dicts: B, P, fills, tag, rows (nb, np), big

        def add(sizes, accept=lambda c: True):
            while True:
                B, P, fills, tag = draw_u64_case(rng, sizes=sizes)
                c = dict(B=B, P=P, fills=fills, tag=tag, rows=(len(B), len(P)), big=False)
                if n_pairs(B, P) + len(B) + len(P) <= POOL_ROWS and accept(c):
                    self.u64.append(c)
                    return c

        for _ in range(N_SMALL):
            add(SMALL_SIZES)
        dup = lambda c: len(c["B"]) >= 4096 and len(np.unique(c["B"][:, 0])) < len(c["B"]) and n_pairs(c["B"], c["P"]) > 0
        if not any(dup(c) for c in self.u64):  # duplicate build keys: the unique-key write gives up and cools down
            add(SMALL_SIZES, dup)
        add([MID_ROWS], lambda c: c["tag"][2] == "sorted")  # a sorted relation: slab partitioning is refused for its order
        for _ in range(N_MID - 1):
            add([MID_ROWS])
        self.dup_case = next(i for i, c in enumerate(self.u64) if dup(c))
        self.big = len(self.u64)
        fills = (int(rng.integers(1, 1 << 62)), int(rng.integers(1, 1 << 62)))
        self.u64.append(dict(B=None, P=None, fills=fills, tag=(BIG_ROWS, BIG_ROWS, "uniform", 0, BIG_SHARE, "none"),
                             rows=(BIG_ROWS, BIG_ROWS), big=True))
        self.strs = []
        while len(self.strs) < N_STR:
            c = draw_str_case(rng, sizes=STR_POOL_KEYS)
            # the inner string join also runs with 8..12 forced hash bits: its mixed runs stay within the collision sort
            for bits in rng.permutation(np.arange(8, 13)):
                rows, _ = kind_brute(c["bk"], c["bv"], c["pk"], c["pv"], BUILD, FULL_OUTER, int(bits))
                if ambiguous_runs(rows, c["bk"], c["pk"])[0] <= RUN_CAP:
                    c["forced_bits"] = int(bits)
                    break
            if "forced_bits" in c:
                self.strs.append(c)
        self.strs.sort(key=lambda c: len(c["bk"]) + len(c["pk"]))  # ascending size: "a smaller case" is a smaller index
        self._cache = {}
        self._fast = {}

    def relations(self, ci):
        c = self.u64[ci]
        if c["B"] is None:  # the big pair, on first use
            c["B"], c["P"] = draw_big_pair(np.random.default_rng([self.seed, 2]), BIG_ROWS)
        return c["B"], c["P"]

    def expect_u64(self, ci, vkey):
        """(rows or None for the big pair, checks, counters or None for the inner join); vkey: "inner", "inner_fw" or an
        index into VARIANTS."""
        key = ("u64", ci, vkey)
        if key not in self._cache:
            c = self.u64[ci]
            B, P = self.relations(ci)
            if c["big"]:
                self._cache[key] = fast_expect(B, P, vkey, c["fills"], self._fast)
            elif vkey in ("inner", "inner_fw"):
                self._cache[key] = expect_inner(B, P, vkey == "inner_fw") + (None,)
            else:
                self._cache[key] = expect_variant(B, P, VARIANTS[vkey], c["fills"])
        return self._cache[key]

    def expect_sorted(self, ci, side):
        key = ("sort", ci, side)
        if key not in self._cache:
            a = self.relations(ci)[side]
            self._cache[key] = a[np.argsort(a[:, 0], kind="stable")]
        return self._cache[key]

    def expect_str_inner(self, si, bits):
        """(rows in HMJ_ORDERED order, counters incl. n_hash_pairs / n_collisions) of the inner string join."""
        key = ("str", si, bits)
        if key not in self._cache:
            from test_join_str_gpu import brute  # (plain Python; the module's GPU tests are not collected by importing it)

            c = self.strs[si]
            rows, coll = brute(c["bk"], c["bv"], c["pk"], c["pv"], bits)
            self._cache[key] = (rows, {"n_collisions": coll, "n_hash_pairs": len(rows) + coll})
        return self._cache[key]

    def expect_str_kind(self, si, side, kind, fills):
        key = ("strk", si, side, kind)
        if key not in self._cache:
            c = self.strs[si]
            self._cache[key] = kind_brute(c["bk"], c["bv"], c["pk"], c["pv"], side, kind, c["hash_bits"], fills[0], fills[1])
        return self._cache[key]

    def expect_hashes(self, si, side, bits):
        key = ("hash", si, side, bits)
        if key not in self._cache:
            self._cache[key] = np.array([str_hash(k, bits) for k in self.strs[si]["bk" if side == 0 else "pk"]], np.uint64)
        return self._cache[key]

    def str_fills(self, si):
        return (0x1111222233334444 + si, 0xAAAA0000BBBB0001 + si)


# ---------------------------------------------------------------------------------------------
def draw_tour(rng, families, required=()):
    """A random Eulerian circuit on the complete directed graph with loops over `families`: F^2 + 1 family names, every
    ordered pair (x, y) exactly once as "x directly followed by y".  Hierholzer's algorithm over shuffled edge lists; drawn
    again until every chain of `required` occurs."""
    F = len(families)
    while True:
        out = {v: [int(w) for w in rng.permutation(F)] for v in range(F)}
        stack, circuit = [int(rng.integers(0, F))], []
        while stack:
            v = stack[-1]
            if out[v]:
                stack.append(out[v].pop())
            else:
                circuit.append(stack.pop())
        tour = [families[v] for v in reversed(circuit)]
        assert len(tour) == F * F + 1
        joined = "|" + "|".join(tour) + "|"
        if all("|" + "|".join(ch) + "|" in joined for ch in required):
            return tour


def transitions(tour):
    return {(tour[i], tour[i + 1]) for i in range(len(tour) - 1)}


class Model:
    """The contract of hmj.h in plain Python: what the context carries from call to call as far as a caller may rely on it."""

    def __init__(self):
        self.forced = None      # radix bits in force (hmj_set_radix_bits), None = automatic
        self.prepared = None    # u64 case whose build side is prepared and not yet discarded
        self.discarded = 0      # prepared build sides discarded by a call other than the join they were meant for

    def step(self, op):
        """Advance over one op: {"rc": the status it must return, "may_prepared": an inner join may report
        HMJ_PATH_PREPARED (it need not), "forced": the radix bits in force while it runs}."""
        what = op["what"]
        res = {"rc": 0, "may_prepared": False, "forced": self.forced}
        if what == "refused":
            # refused before it started: the forced bits stay, and hmj.h lets a prepared build side stay as well
            res["rc"] = E_UNSUPPORTED if op["which"] == "oversized_mixed_run" else E_ARG
            if op["which"] == "oversized_mixed_run":  # (this one ran: a string join like any other)
                self._discard()
            return res
        if what == "config":
            if op["action"] == "radix_bits":
                self.forced = op["value"]
            elif op["action"] == "reserve":
                self._discard()
            res["forced"] = self.forced
            return res  # set_profiling, forget_workloads, release_result: no workspace buffer is read or written
        join = op["inner"] if what == "prefix" else op  # (hmj_set_key_prefix_bits leaves the prepared state in place)
        if join["what"] == "join":
            res["may_prepared"] = self.prepared is not None and self.prepared == join["case"]
            if not res["may_prepared"]:
                self._discard()  # (a join of other relations: like any other call)
            self.prepared = None  # one-shot, taken or not
            return res
        if what == "prepare":
            self._discard()
            self.prepared = op["case"]
            return res
        self._discard()  # kind joins, string joins, hashing, sort, partition, the host join
        return res

    def _discard(self):
        if self.prepared is not None:
            self.discarded += 1
        self.prepared = None


def draw_sequence(rng, families, pool, required=REQUIRED_CHAINS):
    """One tour of ops (dicts of plain values): the families from draw_tour, and per op a case, mode, kind and fills.  The
    few rules beyond chance serve the ledger of test_ctx_sequences_gpu.py and are noted where they apply."""
    tour = draw_tour(rng, families, tuple(ch for ch in required if set(ch) <= set(families)))
    n_u64, n_str = len(pool.u64), len(pool.strs)
    unused_u, unused_s = list(rng.permutation(n_u64)), list(rng.permutation(n_str))
    refusals = [REFUSALS[i] for i in rng.permutation(len(REFUSALS))]
    state = {"forced": None, "prep": None, "reserve": 1 << 12, "refused": 0, "todo": [pool.dup_case, pool.big]}
    ops = []

    def pick_u64(ok=lambda c: True):
        # cases not used yet first, so that every tour uses the whole pool; forced 0 / 1 bits keep off the big pair (one
        # or two partitions of 4 M rows are 820 chunked tables each)
        def fits(i):
            c = pool.u64[i]
            return ok(c) and not (c["big"] and state["forced"] in (0, 1))

        for i in unused_u:
            if fits(i) and rng.random() < 0.7:
                unused_u.remove(i)
                return int(i)
        cand = [i for i in range(n_u64) if fits(i)]
        i = int(cand[int(rng.integers(0, len(cand)))])
        if i in unused_u:
            unused_u.remove(i)
        return i

    def pick_str(ok=lambda i: True):
        for i in unused_s:
            if ok(i) and rng.random() < 0.7:
                unused_s.remove(i)
                return int(i)
        cand = [i for i in range(n_str) if ok(i)]
        i = int(cand[int(rng.integers(0, len(cand)))])
        if i in unused_s:
            unused_s.remove(i)
        return i

    def kind_mode(big):
        mode = KIND_MODES[int(rng.integers(0, 2 if big else 4))]
        return mode | (SUM_PROBE if rng.integers(0, 3) == 0 else 0)

    def draw_join(case=None, flags=None):
        ci = pick_u64() if case is None else case
        big = pool.u64[ci]["big"]
        if flags is None:
            sets = [f for f in INNER_FLAGS if not (big and materialising(f))]
            if ci == pool.dup_case:  # duplicate build keys under a materialising mode: the unique-key write gives up
                sets = [f for f in INNER_FLAGS if materialising(f)]
            flags = sets[int(rng.integers(0, len(sets)))]
        return dict(what="join", case=ci, flags=int(flags))

    def draw_kind(family):
        ci = pick_u64()
        vs = [i for i, v in enumerate(VARIANTS) if v[1] == family]
        return dict(what="kind", case=ci, variant=int(vs[int(rng.integers(0, len(vs)))]), flags=int(kind_mode(pool.u64[ci]["big"])))

    for pos, fam in enumerate(tour):
        prev = ops[-1] if ops else None
        nxt = tour[pos + 1] if pos + 1 < len(tour) else None
        if fam == "inner":
            # a prepared build side not yet met by a join: this join goes to it with the plain count flags -- directly
            # after the prepare it may take it; with a sort, hashing, a reserve ... in between it must not
            # ... otherwise the first two inner joins of a tour go to the case with duplicate build keys (a materialising
            # mode: draw_join) and to the big pair (slab partitioning); the rest are drawn
            if state["prep"] is not None:
                op = draw_join(state["prep"], 0)
            elif state["todo"] and not (state["todo"][0] == pool.big and state["forced"] in (0, 1)):
                op = draw_join(state["todo"].pop(0))
                if op["case"] in unused_u:
                    unused_u.remove(op["case"])
            else:
                op = draw_join()
        elif fam in ("probe_kind", "build_kind"):
            op = draw_kind(fam[:-5])
        elif fam == "str_inner":
            si = pick_str()
            bits = 0 if rng.random() < 0.5 else pool.strs[si]["forced_bits"]
            op = dict(what="str_join", case=si, bits=int(bits), flags=int(kind_mode(False)))
        elif fam == "str_kind":
            # a string kind join directly after a larger one: the first of the pair is not the smallest case, the second
            # one is smaller (marks and accumulators sized by the larger join are met again)
            if prev is not None and prev["fam"] == "str_kind":
                si = pick_str(lambda i: i < prev["case"])
            elif nxt == "str_kind":
                si = pick_str(lambda i: i > 0)
            else:
                si = pick_str()
            side, kind = ALL_KINDS[int(rng.integers(1, len(ALL_KINDS)))]
            op = dict(what="str_kind", case=si, side=int(side), kind=int(kind), flags=int(kind_mode(False)))
        elif fam == "sort_partition":
            after_prepare = prev is not None and prev["fam"] == "prepare"
            if after_prepare or rng.random() < 0.5:
                # (after a prepare: the sort whose ping-pong buffer is the prepared partitions' buffer)
                ci = pick_u64()
                op = dict(what="sort", case=ci, side=int(rng.integers(0, 2)), inplace=bool(rng.integers(0, 2)))
            else:
                ci = pick_u64(lambda c: not c["big"])
                bits = int(rng.integers(1, 10))
                op = dict(what="partition", case=ci, side=int(rng.integers(0, 2)), bits=bits, shift=int(rng.integers(0, 65 - bits)))
        elif fam == "prepare":
            # mostly the relations large enough for a partitioned plan (small count joins take the global table)
            u = rng.random()
            if u < 0.5 and state["forced"] not in (0, 1):
                ci = pool.big
                if ci in unused_u:
                    unused_u.remove(ci)
            else:
                ci = pick_u64(lambda c: c["rows"][0] >= MID_ROWS) if u < 0.8 else pick_u64()
            op = dict(what="prepare", case=ci, hint=int(pool.u64[ci]["rows"][1]))
        elif fam == "host":
            ci = pick_u64(lambda c: max(c["rows"]) <= 65537)
            op = dict(what="host", case=ci, flags=ORDERED | CHECKSUM)
        elif fam == "config":
            action = str(rng.choice(["radix_bits", "radix_bits", "profiling", "forget", "release", "reserve"]))
            if state["forced"] is not None and action != "radix_bits":
                action, value = "radix_bits", None  # forced bits hold until the next configuration op
            elif action == "radix_bits":
                few = FORCED_BITS[2:] if state["prep"] == pool.big else FORCED_BITS  # (the join that follows the prepare)
                value = None if state["forced"] is not None and rng.random() < 0.5 else int(rng.choice(few))
            elif action == "profiling":
                value = bool(rng.integers(0, 2))
            elif action == "reserve":
                state["reserve"] = min(state["reserve"] * 4, 1 << 23)  # growing sizes
                value = [state["reserve"], state["reserve"], state["reserve"] // 2, [0, MATERIALIZE, ORDERED][int(rng.integers(0, 3))]]
            else:
                value = None
            op = dict(what="config", action=action, value=value)
        elif fam == "prefix":
            inner = draw_join() if rng.random() < 0.5 else draw_kind("probe" if rng.random() < 0.5 else "build")
            B, P = (None, None) if pool.u64[inner["case"]]["big"] else pool.relations(inner["case"])
            top = 0 if B is None else min(48, shared_prefix_bits(B, P))  # (uniform 64-bit keys share no prefix)
            op = dict(what="prefix", bits=int(rng.integers(0, top + 1)), inner=inner, case=inner["case"])
        elif fam == "refused":
            which = refusals[state["refused"] % len(refusals)]
            state["refused"] += 1
            op = dict(what="refused", which=which, entry=str(rng.choice(["inner", "probe_kind", "build_kind"])),
                      str_entry=str(rng.choice(["str_join", "str_kind", "hash_str"])), null_side=int(rng.integers(0, 2)),
                      kind=int(rng.choice([BOUTER, FULL])), case=pick_u64(lambda c: not c["big"] and min(c["rows"]) > 0))
        elif fam == "hash_str":
            si = pick_str()
            c = pool.strs[si]
            op = dict(what="hash_str", case=si, side=int(rng.integers(0, 2)), bits=int(rng.choice([0, c["hash_bits"], c["forced_bits"]])))
        else:
            raise ValueError(fam)
        op["fam"] = fam
        # the generator's own view of the prepared build side, for the rule of the inner family above: only a join ends it
        # for the drawing.  A sort, a partition, hashing or a reserve does not -- the inner join that follows still goes to
        # the prepared tensor, where the contract (Model) says it must no longer be taken
        if op["what"] == "prepare":
            state["prep"] = op["case"]
        elif op["what"] in ("join", "kind", "str_join", "str_kind", "host", "prefix"):
            state["prep"] = None
        if op["what"] == "config" and op["action"] == "radix_bits":
            state["forced"] = op["value"]
        ops.append(op)
    return ops


def u64_case_of(op):
    """The u64 pool case an op reads, or None."""
    if op["what"] in ("join", "kind", "sort", "partition", "prepare", "host", "prefix"):
        return op["case"]
    if op["what"] == "refused" and op["which"] in ("unknown_kind", "struct_too_small", "first_wins_outer", "too_many_rows",
                                                    "null_relation", "partition_bits_10"):
        return op["case"]
    return None


def expectation(pool, op):
    """What the op is compared against (a tuple whose layout the runner of the op's family knows), computed once per
    (case, kind or first-wins form): the op's mode only selects what of it is read.  Never None: no op is skipped."""
    what = op["what"]
    if what == "join" or what == "host":
        return pool.expect_u64(op["case"], "inner_fw" if op["flags"] & FIRST_WINS else "inner")
    if what == "kind":
        return pool.expect_u64(op["case"], op["variant"])
    if what == "prefix":
        return expectation(pool, op["inner"])
    if what == "str_join":
        return pool.expect_str_inner(op["case"], op["bits"])
    if what == "str_kind":
        return pool.expect_str_kind(op["case"], op["side"], op["kind"], pool.str_fills(op["case"]))
    if what == "sort":
        return (pool.expect_sorted(op["case"], op["side"]),)
    if what == "partition":
        return expect_partition(pool.relations(op["case"])[op["side"]], op["shift"], op["bits"])
    if what == "hash_str":
        return (pool.expect_hashes(op["case"], op["side"], op["bits"]),)
    if what in ("prepare", "config", "refused"):
        return (Model().step(op)["rc"],)  # the status alone
    raise ValueError(what)


# ---------------------------------------------------------------------------------------------
SEEDS = (SEQ_SEED, 7, 11)
CPU_ROWS = 40000  # the CPU checks compute the expectations of u64 cases up to this many rows (both sides)
_pools = {}


def pool_of(seed):
    if seed not in _pools:
        _pools[seed] = Pool(seed)
    return _pools[seed]


_tours = {}


def tours_of(seed):
    """The pool and the default number of tours of a seed, as test_ctx_sequences_gpu.py draws them."""
    pool = pool_of(seed)
    if seed not in _tours:
        rng = np.random.default_rng([int(seed), 3])
        _tours[seed] = [draw_sequence(rng, FAMILIES, pool) for _ in range(SEQ_TOURS)]
    return pool, _tours[seed]


def test_the_flag_values_are_the_bindings():
    import hashmergejoin_amd as H

    assert (MATERIALIZE, ORDERED, FIRST_WINS, CHECKSUM, SUM_PROBE) == \
        (H.HMJ_MATERIALIZE, H.HMJ_ORDERED, H.HMJ_FIRST_WINS, H.HMJ_CHECKSUM, H.HMJ_SUM_PROBE)
    assert (E_ARG, E_UNSUPPORTED) == (-1, -5)  # HMJ_E_ARG, HMJ_E_UNSUPPORTED of hmj.h


def test_every_tour_holds_every_transition_family_and_case():
    for seed in SEEDS:
        pool, tours = tours_of(seed)
        for ops in tours:
            fams = [op["fam"] for op in ops]
            F = len(FAMILIES)
            assert len(ops) == F * F + 1
            assert transitions(fams) == {(x, y) for x in FAMILIES for y in FAMILIES}, seed
            assert set(fams) == set(FAMILIES)
            for ch in REQUIRED_CHAINS:
                assert any(tuple(fams[i:i + len(ch)]) == ch for i in range(len(fams))), (seed, ch)
            used = {u64_case_of(op) for op in ops} - {None}
            assert used == set(range(len(pool.u64))), (seed, sorted(used))
            sused = {op["case"] for op in ops if op["what"] in ("str_join", "str_kind", "hash_str")}
            assert sused == set(range(len(pool.strs))), (seed, sorted(sused))
            assert {op["which"] for op in ops if op["what"] == "refused"} == set(REFUSALS), seed
            # the rules the ledger of the GPU test leans on
            pairs = [(a, b) for a, b in zip(ops, ops[1:]) if a["fam"] == b["fam"] == "str_kind"]
            assert len(pairs) == 1 and pairs[0][1]["case"] < pairs[0][0]["case"], seed
            i = next(i for i in range(len(fams) - 2) if tuple(fams[i:i + 3]) == REQUIRED_CHAINS[0])
            assert ops[i + 1]["what"] == "sort" and ops[i + 2]["case"] == ops[i]["case"] and ops[i + 2]["flags"] == 0, seed
            assert any(a["fam"] == "prepare" and b["fam"] == "inner" and b["case"] == a["case"] and b["flags"] == 0
                       for a, b in zip(ops, ops[1:])), seed
            assert any(op["what"] == "join" and op["case"] == pool.dup_case and materialising(op["flags"]) for op in ops), seed
            assert any(op["what"] == "join" and op["case"] == pool.big for op in ops), seed


def test_no_drawn_op_lacks_an_expectation():
    for seed in SEEDS:
        pool, tours = tours_of(seed)
        for ops in tours:
            model = Model()
            for op in ops:
                want = model.step(op)
                assert want["rc"] in (0, E_ARG, E_UNSUPPORTED) and (want["rc"] == 0) == (op["what"] != "refused"), op
                join = op["inner"] if op["what"] == "prefix" else op
                ci = u64_case_of(op)
                if ci is not None and pool.u64[ci]["big"]:
                    # the big pair is never built here: its ops are those fast_expect serves (the test below checks it)
                    assert op["what"] in ("join", "kind", "prefix", "sort", "prepare"), op
                    assert op["what"] in ("sort", "prepare") or not materialising(join["flags"]), op
                    assert want["forced"] not in (0, 1), op
                    continue
                if ci is not None and sum(pool.u64[ci]["rows"]) > CPU_ROWS:
                    continue  # (the same code as for the smaller cases; the GPU test computes these)
                exp = expectation(pool, op)
                assert exp is not None and all(e is not None for e in exp[:2 if len(exp) > 1 else 1]), op
            assert model.discarded > 0, seed  # some prepared build side meets an intervening call


def test_pool_cases_are_bounded():
    for seed in SEEDS:
        pool = pool_of(seed)
        small = [c for c in pool.u64 if max(c["rows"]) <= 65537]
        mid = [c for c in pool.u64 if c["rows"] == (MID_ROWS, MID_ROWS)]
        assert len(small) in (N_SMALL, N_SMALL + 1) and len(mid) == N_MID and len(pool.u64) == len(small) + len(mid) + 1
        for c in pool.u64:
            if c["big"]:
                # never built here.  Its largest result is the full outer join's: 0.6 n pairs, 0.4 n unmatched probe rows
                # and the build rows no probe row drew, n e^-0.6 = 0.55 n -- 1.55 n rows (the test of the fast
                # expectation measures it at 2^16 rows); no mode of the big pair materialises them
                assert BIG_ROWS * 8 // 5 <= ROW_CAP
                continue
            assert n_pairs(c["B"], c["P"]) + sum(c["rows"]) <= POOL_ROWS <= ROW_CAP, (seed, c["tag"])
        dup = pool.u64[pool.dup_case]
        assert len(np.unique(dup["B"][:, 0])) < len(dup["B"])
        assert any(c["tag"][2] == "sorted" and c["rows"][0] == MID_ROWS for c in pool.u64), seed
        assert len(pool.strs) == N_STR
        for c in pool.strs:
            for bits in (c["hash_bits"], c["forced_bits"], 0):
                rows, _ = kind_brute(c["bk"], c["bv"], c["pk"], c["pv"], BUILD, FULL_OUTER, bits)
                assert ambiguous_runs(rows, c["bk"], c["pk"])[0] <= RUN_CAP, (seed, bits)
    # ... except the one refused op that is meant to exceed it
    o = OVERSIZED
    rows, _ = kind_brute(o["bk"], o["bv"], o["pk"], o["pv"], BUILD, FULL_OUTER, o["hash_bits"])
    largest, mixed = ambiguous_runs(rows, o["bk"], o["pk"])
    assert largest > RUN_CAP and mixed


def test_the_inner_expectation_is_the_oracles(oracle):
    pool = pool_of(SEQ_SEED)
    for ci, c in enumerate(pool.u64):
        if c["big"] or max(c["rows"]) > 65537:
            continue
        for first in (False, True):
            ck, rows = oracle.equijoin(c["B"], c["P"], first_wins=first)
            got_rows, got_ck, _ = pool.expect_u64(ci, "inner_fw" if first else "inner")
            assert got_ck == ck and np.array_equal(got_rows, rows), (ci, first)


def test_the_fast_expectation_of_the_big_pair_is_expect_variants():
    B, P = draw_big_pair(np.random.default_rng([SEQ_SEED, 2]), 1 << 16)
    assert 0.55 < np.isin(P[:, 0], B[:, 0]).mean() < 0.65
    fills, cache = (0x1234, 0x5678), {}
    for vi, v in enumerate(VARIANTS):
        rows, ck, counters = expect_variant(B, P, v, fills)
        assert fast_expect(B, P, vi, fills, cache) == (None, ck, counters), v[0]
        assert ck["n_matches"] <= len(B) * 8 // 5, v[0]  # (test_pool_cases_are_bounded: the big pair's rows)
    for first in (False, True):
        assert fast_expect(B, P, "inner_fw" if first else "inner", fills, cache)[1] == expect_inner(B, P, first)[1]


def test_the_model_follows_the_written_contract():
    m = Model()
    join = lambda ci, fl=0: dict(what="join", case=ci, flags=fl)
    assert not m.step(join(0))["may_prepared"]
    m.step(dict(what="prepare", case=0))
    assert m.step(join(0))["may_prepared"] and not m.step(join(0))["may_prepared"]  # one-shot
    m.step(dict(what="prepare", case=0))
    assert not m.step(join(1))["may_prepared"] and not m.step(join(0))["may_prepared"]  # another build tensor: dropped
    for between, may in ((dict(what="sort", case=1), False), (dict(what="hash_str", case=0), False),
                         (dict(what="partition", case=1), False), (dict(what="config", action="reserve", value=[1, 1, 0, 0]), False),
                         (dict(what="config", action="profiling", value=True), True),
                         (dict(what="config", action="radix_bits", value=4), True),
                         (dict(what="refused", which="radix_bits_40"), True),
                         (dict(what="refused", which="oversized_mixed_run"), False)):
        m.step(dict(what="prepare", case=2))
        m.step(between)
        assert m.step(join(2))["may_prepared"] == may, between
    assert m.forced == 4 and m.step(dict(what="refused", which="radix_bits_40"))["forced"] == 4
    m.step(dict(what="config", action="radix_bits", value=None))
    assert m.forced is None and m.discarded == 6
