"""GPU checks of the distributed join kinds (hmj_exchange_join_kind_u64_device, csrc/exchange.hip).

  * several ranks sharing the one GPU over the gloo callback transport (as in test_dist_gpu.py): all seven kinds in count,
    checksum and HMJ_ORDERED forms on the digit-owner path (one or several rounds, rounds with no build or no probe rows),
    the hash-owner fallback, the owner-split path and key-range owners, against the numpy expectation over the whole
    relations (expect_kind / expect_build_kind);
  * argument errors and ranks that disagree on the kind: every rank returns an error, none hangs;
  * one rank over RCCL self send/recv, the whole exchange path: numpy expectations at 2^22 and 2^24 rows, the single-GPU
    kind entries at 2^26 rows; the inner join keeps its results, path and plan after kind joins on the same ctx."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from test_join_build_kinds_cpu import BANTI, BOUTER, BSEMI, FULL, expect_build_kind
from test_join_kinds_cpu import ANTI, M64, OUTER, SEMI, _inner_rows, expect_kind, tmix

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PSIDE, BSIDE = 0, 1
PROBE_FILL, BUILD_FILL = 0xABCDEF0123, 0x5A5A17
# (name, side, kind): the seven kinds
KINDS = [("semi", PSIDE, SEMI), ("anti", PSIDE, ANTI), ("outer", PSIDE, OUTER), ("bsemi", BSIDE, BSEMI),
         ("banti", BSIDE, BANTI), ("bouter", BSIDE, BOUTER), ("full", BSIDE, FULL)]

# The relations of a case, built the same way by the workers (each slices its shard) and by the checks here.
GEN = r'''
import numpy as np

def relations(case, nb, npr, miss):
    """[nb, 2] build and [npr, 2] probe rows (key, payload) of a case: the union of all ranks' shards."""
    rng = np.random.default_rng(20261015)
    B = np.zeros((nb, 2), np.uint64)
    P = np.zeros((npr, 2), np.uint64)
    B[:, 1] = rng.integers(1, 1 << 48, nb, dtype=np.uint64)
    P[:, 1] = rng.integers(1, 1 << 48, npr, dtype=np.uint64)
    rand64 = lambda n: rng.integers(0, (1 << 64) - 1, n, dtype=np.uint64, endpoint=True)
    if case in ("uniform", "dup", "empty_all", "empty_one"):
        B[:, 0] = rand64(nb)
        if case == "dup":  # build row i and row i + nb/2 share a key, on different ranks: first-wins across shards
            B[nb // 2:, 0] = B[: nb - nb // 2, 0]
        P[:, 0] = B[rng.integers(0, nb, npr), 0] if nb else rand64(npr)
    elif case == "ranges":  # build keys in [0, 3/4), probe keys in [1/4, 1) of the key range: rounds of one relation only
        B[:, 0] = rng.integers(0, 3 << 62, nb, dtype=np.uint64)
        hi = B[B[:, 0] >= np.uint64(1 << 62), 0]
        P[:, 0] = rng.integers(1 << 62, (1 << 64) - 1, npr, dtype=np.uint64, endpoint=True)
        P[::2, 0] = hi[rng.integers(0, len(hi), len(P[::2]))]
    elif case == "clusters":  # two far-apart clusters of dense keys (3/4 and 1/4): the digit ranges cannot balance -> hash owner
        clus = lambda x: x | (((x & np.uint64(3)) == np.uint64(3)).astype(np.uint64) << np.uint64(62))
        B[:, 0] = clus(np.arange(nb, dtype=np.uint64))
        P[:, 0] = clus((np.arange(npr, dtype=np.uint64) * np.uint64(5)) % np.uint64(nb + nb // 4))
    elif case == "dense_top":  # dense integer build keys; every other probe key carries a top bit no build key has
        B[:, 0] = np.arange(nb, dtype=np.uint64)
        P[:, 0] = (np.arange(npr, dtype=np.uint64) * np.uint64(3)) % np.uint64(nb)
        P[1::2, 0] |= np.uint64(1 << 63)
    else:
        raise ValueError(case)
    if miss and npr:
        P[::miss, 0] = rand64(len(P[::miss]))  # (almost surely absent from the build side)
    return B, P

def shard(n, rank, world, skip_first=False):
    """Row range of a rank's shard: contiguous, in rank order (rank 0 holds none with skip_first)."""
    if skip_first:
        return (0, 0) if rank == 0 else ((rank - 1) * n // (world - 1), rank * n // (world - 1))
    return rank * n // world, (rank + 1) * n // world
'''
_ns = {}
exec(GEN, _ns)
relations, shard = _ns["relations"], _ns["shard"]

WORKER = GEN + r'''
import os, sys, json, traceback
import torch
import torch.distributed as dist
sys.path.insert(0, os.environ["HMJ_ROOT"])
import hashmergejoin_amd as H
from hashmergejoin_amd import dist as hdist

rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
torch.cuda.set_device(0)
dist.init_process_group("gloo", rank=rank, world_size=world)
cases, kinds = json.loads(os.environ["CASES"]), json.loads(os.environ["KINDS"])
pf, bf = int(os.environ["PF"]), int(os.environ["BF"])
to_dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int64).copy()).cuda()
ex = H.Executor(0)
hdist.init_comm(ex)
out = {}
for cs in cases:
    name = cs["name"]
    B, P = relations(cs["case"], cs["nb"], cs["np"], cs["miss"])
    b0, b1 = shard(len(B), rank, world, cs["case"] == "empty_one")
    p0, p1 = shard(len(P), rank, world)
    bd, pd = to_dev(B[b0:b1]), to_dev(P[p0:p1])
    if cs.get("maxmsg"):
        ex.comm_set_message_bytes(cs["maxmsg"], cs["maxmsg"] // 4)
    ex.comm_set_owner_path(split=bool(cs.get("split")))
    rec = {"kinds": {}}
    for kname, side, kind in kinds:
        rk = rec["kinds"][kname] = {}
        for form, fl in (("count", 0), ("checksum", H.HMJ_CHECKSUM | H.HMJ_SUM_PROBE), ("ordered", H.HMJ_ORDERED | H.HMJ_CHECKSUM)):
            loc, glob, cnt = hdist.distributed_join_kind(ex, bd, pd, side, kind, fl, probe_fill=pf, build_fill=bf)
            info = ex.last_exchange_info()
            rk[form] = {"glob": glob, "cnt": cnt, "sum_probe_all": int(loc.sum_probe_all),
                        "info": {k: info[k] for k in ("owner_mode", "fallback", "n_subjoins", "rounds_probe", "recv_build", "recv_probe")}}
            if form == "ordered":
                rows = (ex.probe_rows_to_numpy(loc) if kind in (1, 2) and side == 0 else
                        ex.build_rows_to_numpy(loc) if kind in (1, 2) else ex.columns_to_numpy(loc, host=False))
                np.save(os.path.join(os.environ["OUT"], "%s_%s_%d.npy" % (name, kname, rank)), rows)
            ex.release_result()
    _, rec["first"], _ = hdist.distributed_join_kind(ex, bd, pd, H.HMJ_KIND_PROBE_SIDE, H.HMJ_JOIN_PROBE_OUTER,
                                                     H.HMJ_FIRST_WINS | H.HMJ_CHECKSUM, probe_fill=pf)
    _, rec["inner_kind"], cnt = hdist.distributed_join_kind(ex, bd, pd, H.HMJ_KIND_PROBE_SIDE, H.HMJ_JOIN_INNER, H.HMJ_CHECKSUM)
    assert cnt["local"] == cnt["global"] == dict.fromkeys(cnt["local"], 0), cnt
    rec["inner"] = hdist.distributed_join(ex, bd, pd, H.HMJ_CHECKSUM)[1]
    out[name] = rec
json.dump(out, open(os.path.join(os.environ["OUT"], "out%d.json" % rank), "w"))
ex.close()
dist.destroy_process_group()
'''


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def run_ranks(tmp_path, world, script, timeout, **extra):
    port = free_port()
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HMJ_ROOT=ROOT,
                   OUT=str(tmp_path), OMP_NUM_THREADS="1", **extra)
        procs.append(subprocess.Popen([sys.executable, "-c", script], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    outs = []
    try:
        for p in procs:
            outs.append(p.communicate(timeout=timeout)[0].decode())
    finally:
        for p in procs:  # (a rank that hangs is a failure, and must not outlive the test)
            if p.poll() is None:
                p.kill()
                p.communicate()
    assert all(p.returncode == 0 for p in procs), "\n".join(outs)
    return outs


def expected(B, P, side, kind):
    if side == PSIDE:
        rows, ck, hit = expect_kind(B, P, kind, fill=PROBE_FILL)
        cnt = {"n_probe_matched": hit, "n_probe_unmatched": len(P) - hit, "n_build_matched": 0, "n_build_unmatched": 0}
    else:
        rows, ck, cnt = expect_build_kind(B, P, kind, build_fill=BUILD_FILL, probe_fill=PROBE_FILL)
        cnt = dict(cnt)
    return rows, ck, cnt


def check_cases(tmp_path, world, cases):
    res = [json.load(open(tmp_path / ("out%d.json" % r))) for r in range(world)]
    for cs in cases:
        name = cs["name"]
        B, P = relations(cs["case"], cs["nb"], cs["np"], cs["miss"])
        sum_p = int(P[:, 1].sum(dtype=np.uint64)) & M64
        recs = [o[name] for o in res]
        for kname, side, kind in KINDS:
            rows, ck, cnt = expected(B, P, side, kind)
            for form in ("count", "checksum", "ordered"):
                got = [r["kinds"][kname][form] for r in recs]
                where = (name, kname, form)
                for g in got:  # every rank reports the same global reduction
                    if form == "count":
                        assert {k: g["glob"][k] for k in ("n_matches", "sum_r", "sum_s")} == \
                               {k: ck[k] for k in ("n_matches", "sum_r", "sum_s")}, where
                    else:
                        assert g["glob"] == ck, where
                    assert g["cnt"]["global"] == cnt, (where, g["cnt"])
                # local counters are over the rows each rank received, and add up to the global ones
                assert {k: sum(g["cnt"]["local"][k] for g in got) for k in cnt} == cnt, where
                if form == "checksum":
                    assert sum(g["sum_probe_all"] for g in got) & M64 == sum_p, where
            # HMJ_ORDERED: the rank-ordered concatenation of the local rows is the global order
            cat = np.concatenate([np.load(tmp_path / ("%s_%s_%d.npy" % (name, kname, r))).reshape(-1, rows.shape[1])
                                  for r in range(world)])
            assert np.array_equal(cat, rows), (name, kname)
        _, ckf, _ = expect_kind(B, P, OUTER, first_wins=True, fill=PROBE_FILL)
        for r in recs:
            assert r["first"] == ckf, name  # global first-wins: rank r's build shard precedes rank r+1's
            assert r["inner_kind"] == r["inner"], name  # PROBE_SIDE + INNER is the inner exchange join
        infos = [{k: r["kinds"][k]["count"]["info"] for k in r["kinds"]} for r in recs]
        for i in infos:  # owners: the caller's owner split, the hash fallback for clustered keys, else digit ranges
            if cs.get("split") or cs["case"] == "clusters":
                assert i["semi"]["owner_mode"] == 1 and (cs.get("split") or i["semi"]["fallback"] == 1), (name, i)
            elif cs["case"] in ("uniform", "dup", "ranges", "empty_one"):
                assert i["semi"]["owner_mode"] == 3, (name, i)
        assert sum(i["semi"]["recv_build"] for i in infos) == len(B) and sum(i["semi"]["recv_probe"] for i in infos) == len(P)
        if cs["case"] == "ranges":
            # several rounds; some hold no probe rows (build anti / outer join them, the inner join skips them), some no
            # build rows (anti / outer join them)
            assert all(i["semi"]["rounds_probe"] > 4 for i in infos), infos
            assert any(i["banti"]["n_subjoins"] > i["bsemi"]["n_subjoins"] for i in infos), infos
            assert any(i["anti"]["n_subjoins"] > i["semi"]["n_subjoins"] for i in infos), infos
            assert all(i["full"]["n_subjoins"] >= max(i["anti"]["n_subjoins"], i["banti"]["n_subjoins"]) for i in infos), infos


WORLDS = {
    2: [dict(name="u3", case="uniform", nb=300000, np=200000, miss=3),
        dict(name="clusters", case="clusters", nb=300000, np=270000, miss=0),
        dict(name="dense_top_split", case="dense_top", nb=300000, np=300000, miss=0, split=True),
        dict(name="dense_top", case="dense_top", nb=200000, np=260000, miss=5),
        dict(name="empty_all", case="empty_all", nb=0, np=150000, miss=0),
        dict(name="empty_one", case="empty_one", nb=200000, np=200000, miss=3),
        dict(name="ranges", case="ranges", nb=1 << 20, np=1 << 20, miss=0, maxmsg=1 << 20)],
    4: [dict(name="dup0", case="dup", nb=1 << 19, np=(1 << 19) + 777, miss=0),
        dict(name="u3_split", case="uniform", nb=400000, np=300001, miss=3, split=True),
        dict(name="empty_one", case="empty_one", nb=300000, np=250000, miss=0),
        dict(name="dup_rounds", case="dup", nb=1 << 20, np=1 << 20, miss=3, maxmsg=1 << 20)],
}


@pytest.mark.parametrize("world", [2, 4])
def test_kinds_across_ranks_on_one_gpu(tmp_path, world):
    cases = WORLDS[world]
    run_ranks(tmp_path, world, WORKER, 400, CASES=json.dumps(cases), KINDS=json.dumps(KINDS), PF=str(PROBE_FILL), BF=str(BUILD_FILL))
    check_cases(tmp_path, world, cases)


ERR_WORKER = r"""
import os, sys, json
import ctypes as C
import torch
import torch.distributed as dist
sys.path.insert(0, os.environ["HMJ_ROOT"])
import hashmergejoin_amd as H
from hashmergejoin_amd import dist as hdist
from hashmergejoin_amd._lib import HmjError

rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
torch.cuda.set_device(0)
dist.init_process_group("gloo", rank=rank, world_size=world)
ex = H.Executor(0)
hdist.init_comm(ex, timeout_s=60.0)
n = 100000
bd, pd = ex.gen_build(n, start=rank * n), ex.gen_probe(n, world * n, start=rank * n, miss_mod=4)

def raw(side, kind, flags=0, size=None):
    opts = H.ExchangeKindOpts()
    opts.struct_size = C.sizeof(H.ExchangeKindOpts) if size is None else size
    opts.side, opts.kind = side, kind
    loc, glob = H.JoinResult(), H.JoinResult()
    return ex.L.hmj_exchange_join_kind_u64_device(ex.h, C.c_void_p(bd.data_ptr()), n, C.c_void_p(pd.data_ptr()), n, flags,
                                                  C.byref(opts), C.byref(loc), C.byref(glob))

P, B = H.HMJ_KIND_PROBE_SIDE, H.HMJ_KIND_BUILD_SIDE
codes = {
    "unknown_kind": raw(P, 4), "unknown_build_kind": raw(B, 0), "unknown_side": raw(2, 1),
    "struct_too_small": raw(P, H.HMJ_JOIN_SEMI, size=8), "fill_not_covered": raw(B, H.HMJ_FULL_OUTER, size=24),
    "first_wins_build_outer": raw(B, H.HMJ_BUILD_OUTER, H.HMJ_FIRST_WINS),
    "first_wins_full_outer": raw(B, H.HMJ_FULL_OUTER, H.HMJ_FIRST_WINS),
    "ok_before": raw(P, H.HMJ_JOIN_ANTI),
    # the ranks pass different kinds: every rank takes part in every collective and all return HMJ_E_ARG together
    "disagree": raw(P, H.HMJ_JOIN_SEMI if rank == 0 else H.HMJ_JOIN_ANTI, H.HMJ_CHECKSUM),
    "disagree_side": raw(P if rank == 0 else B, H.HMJ_JOIN_SEMI),
    "ok_after": raw(B, H.HMJ_FULL_OUTER, H.HMJ_CHECKSUM),
}
json.dump(codes, open(os.path.join(os.environ["OUT"], "codes%d.json" % rank), "w"))
ex.close()
dist.destroy_process_group()
"""


def test_argument_errors_and_disagreeing_kinds_end_on_every_rank(tmp_path):
    world = 2
    run_ranks(tmp_path, world, ERR_WORKER, 200)
    codes = [json.load(open(tmp_path / ("codes%d.json" % r))) for r in range(world)]
    for c in codes:
        for k in ("unknown_kind", "unknown_build_kind", "unknown_side", "struct_too_small", "fill_not_covered",
                  "first_wins_build_outer", "first_wins_full_outer", "disagree", "disagree_side"):
            assert c[k] == -1, (k, codes)  # HMJ_E_ARG
        assert c["ok_before"] == 0 and c["ok_after"] == 0, codes  # the communicator stays usable


# ---- one rank, RCCL self send/recv: the whole exchange path -------------------------------------------------------------
@pytest.fixture(scope="module")
def ex1():
    import hashmergejoin_amd as H
    from hashmergejoin_amd import dist as hdist

    e = H.Executor(0)
    hdist.init_comm_single(e, self_exchange=True, timeout_s=120.0)
    yield e
    e.close()


def gen_pair(ex, n):
    """n build rows and n probe rows: the build rows are those of the probe side's build relation shifted by n / 4, so that
    rows of either side have no partner (a quarter of the probe rows, and a seventh more through miss_mod)."""
    bd = ex.gen_build(n, start=n // 4)
    pd = ex.gen_probe(n, n, miss_mod=7)
    return bd, pd


def fast_expected(B, P, side, kind, cache):
    """Checks and counters of a kind over whole relations, without building its sorted rows (the big one-rank cases)."""
    if "phit" not in cache:
        cache["phit"] = np.isin(P[:, 0], B[:, 0])
        cache["bhit"] = np.isin(B[:, 0], P[:, 0])
        cache["inner"] = _inner_rows(B, P, False)[0]
    phit, bhit, inner = cache["phit"], cache["bhit"], cache["inner"]
    z = lambda n, v=0: np.full(n, v, np.uint64)
    parts = []
    if side == PSIDE and kind in (SEMI, ANTI):
        sel = P[phit] if kind == SEMI else P[~phit]
        parts.append((sel[:, 0], z(len(sel)), sel[:, 1]))
    elif side == BSIDE and kind in (BSEMI, BANTI):
        sel = B[bhit] if kind == BSEMI else B[~bhit]
        parts.append((sel[:, 0], sel[:, 1], z(len(sel))))
    else:
        parts.append((inner[:, 0], inner[:, 1], inner[:, 2]))
        if kind == FULL or (side == PSIDE and kind == OUTER):
            pm = P[~phit]
            parts.append((pm[:, 0], z(len(pm), PROBE_FILL), pm[:, 1]))
        if side == BSIDE and kind in (BOUTER, FULL):
            bm = B[~bhit]
            parts.append((bm[:, 0], bm[:, 1], z(len(bm), BUILD_FILL)))
    ck = {"n_matches": 0, "sum_r": 0, "sum_s": 0, "xor_fold": 0, "mix_sum": 0}
    for k, r, s in parts:
        m = tmix(k, r, s)
        ck["n_matches"] += len(k)
        ck["sum_r"] = (ck["sum_r"] + int(r.sum(dtype=np.uint64))) & M64
        ck["sum_s"] = (ck["sum_s"] + int(s.sum(dtype=np.uint64))) & M64
        ck["xor_fold"] ^= int(np.bitwise_xor.reduce(m)) if len(m) else 0
        ck["mix_sum"] = (ck["mix_sum"] + int(m.sum(dtype=np.uint64))) & M64
    npm, nbm = int(phit.sum()), int(bhit.sum())
    probe_cnt = side == PSIDE or kind == FULL
    cnt = {"n_probe_matched": npm if probe_cnt else 0, "n_probe_unmatched": len(P) - npm if probe_cnt else 0,
           "n_build_matched": nbm if side == BSIDE else 0, "n_build_unmatched": len(B) - nbm if side == BSIDE else 0}
    return ck, cnt


@pytest.mark.parametrize("log2n,maxmsg", [(22, 1 << 22), (24, 1 << 21)])
def test_one_rank_rccl_kinds_against_numpy(ex1, log2n, maxmsg):
    import hashmergejoin_amd as H

    ex, n = ex1, 1 << log2n
    bd, pd = gen_pair(ex, n)
    B, P = bd.cpu().numpy().view(np.uint64), pd.cpu().numpy().view(np.uint64)
    ex.comm_set_message_bytes(maxmsg, maxmsg // 8)
    cache = {}
    for kname, side, kind in KINDS:
        ck, cnt = fast_expected(B, P, side, kind, cache)
        if log2n == 22:  # (the fast expectation is the sorted one's, on the same relations)
            ck2, cnt2 = expected(B, P, side, kind)[1:]
            assert (ck, cnt) == (ck2, cnt2), kname
        loc, glob, got = ex.exchange_join_kind(bd, pd, side, kind, H.HMJ_CHECKSUM, probe_fill=PROBE_FILL, build_fill=BUILD_FILL)
        info, plan = ex.last_exchange_info(), ex.last_plan()
        assert glob.checks() == ck and loc.checks() == ck, kname
        assert got["global"] == got["local"] == cnt, (kname, got)
        assert info["owner_mode"] == 3 and info["rounds_probe"] > 1 and info["n_subjoins"] > 1, info
        # count rounds keep the digit's bits out of the partition window (c->min_prefix_bits = 64 - digit_low)
        assert plan["key_prefix_bits"] >= 64 - info["digit_low"], (plan, info)
        loc, glob, got = ex.exchange_join_kind(bd, pd, side, kind, 0, probe_fill=PROBE_FILL, build_fill=BUILD_FILL)
        assert (int(glob.n_matches), int(glob.sum_r), int(glob.sum_s)) == (ck["n_matches"], ck["sum_r"], ck["sum_s"]), kname
        assert got["global"] == cnt, kname


def test_one_rank_rccl_kinds_match_the_single_gpu_kinds_at_2_26(ex1):
    import hashmergejoin_amd as H

    ex, n = ex1, 1 << 26
    bd, pd = gen_pair(ex, n)
    ex.comm_set_message_bytes(1 << 28, 1 << 26)
    for kname, side, kind in KINDS:
        for fl in (0, H.HMJ_CHECKSUM):
            loc, glob, got = ex.exchange_join_kind(bd, pd, side, kind, fl, probe_fill=PROBE_FILL, build_fill=BUILD_FILL)
            info = ex.last_exchange_info()
            assert info["n_subjoins"] > 1, info
            if side == PSIDE:
                one, c1 = ex.join_kind_device(bd, pd, kind, fl, outer_fill=PROBE_FILL)
                c1 = dict(c1, n_build_matched=0, n_build_unmatched=0)
            else:
                one, c1 = ex.join_build_kind_device(bd, pd, kind, fl, build_fill=BUILD_FILL, probe_fill=PROBE_FILL)
            assert glob.checks() == one.checks(), (kname, fl)
            assert got["global"] == got["local"] == c1, (kname, fl, got, c1)
    ex.release_result()


def test_inner_exchange_join_unchanged_after_kind_joins(ex1):
    import hashmergejoin_amd as H

    ex, n = ex1, 1 << 24
    bd, pd = gen_pair(ex, n)
    ex.comm_set_message_bytes(1 << 22, 1 << 21)
    keys = ("path", "radix_bits", "radix_passes", "key_prefix_bits", "key_window_low", "n_partitions", "probe_items")

    def inner():
        loc, glob = ex.exchange_join(bd, pd, H.HMJ_CHECKSUM)
        plan, info = ex.last_plan(), ex.last_exchange_info()
        return glob.checks(), {k: plan[k] for k in keys}, {k: info[k] for k in ("owner_mode", "n_subjoins", "rounds_probe")}

    inner()
    before = inner()
    for _, side, kind in KINDS:
        ex.exchange_join_kind(bd, pd, side, kind, H.HMJ_CHECKSUM, probe_fill=PROBE_FILL, build_fill=BUILD_FILL)
    _, glob, cnt = ex.exchange_join_kind(bd, pd, H.HMJ_KIND_PROBE_SIDE, H.HMJ_JOIN_INNER, H.HMJ_CHECKSUM)
    assert glob.checks() == before[0] and cnt["global"] == dict.fromkeys(cnt["global"], 0)
    assert inner() == before
