"""The case table of the sharded lookup (opendht_amd.sharding: range shards, record exchange, K3,
tie exchange, overflow settlement), shared by test_sharding.py (gloo + host stand-ins for the
device steps) and test_gpu_sharded.py / sharded_worker.py (gloo + sharding.LibOps on one device).

A case is one lookup of `q` targets over `n` ids split over `world` ranks; `run` is the call
sequence a pipelined caller issues (bench.py's): exchange into preallocated buffers, merge_*,
read unsettled(tx), synchronise, settle_overflow_*.  What a rank must hold afterwards is the flat
exact top-k of its target slice, and its tie count must lie within the bounds `tie_bounds` derives
from the layout -- none of it taken from the code under test."""
import collections
import functools

import numpy as np
import torch

import oracle as O
from opendht_amd import sharding

NONE = 0xFFFFFFFF
SEED = 31

Case = collections.namedtuple("Case", "name worlds exchange n q k cap producer layout")


def _case(name, exchange, n, q, k=8, cap=256, worlds=(2, 3), producer="batch", layout="base"):
    return Case(name, worlds, exchange, n, q, k, cap, producer, layout)


# Layouts: "base" = a quarter of the ids share their first 64 bits and every second target (the P
# targets) carries them too; "lopsided" = the same ids, P targets in rows [0, 300) only; "hash" =
# hash-distributed ids and targets (no two candidates of a target share 64 bits).
# The order matters: a "hash" case runs right after an overflowing one, through the same
# TieExchange and the same buffers (`Bufs`), and must find none of it.
CASES = (
    _case("A", "allgather", 1500, 60),                                   # ties within the cap
    _case("B", "allgather", 2400, 700),                                  # 350 P rows > 256: every-row settlement
    _case("H_allgather", "allgather", 1500, 700, layout="hash"),         # after B: count 0, flag down
    _case("C", "alltoall", 1500, 60),                                    # slices at 30 / 20, 40: row_base, t0 != 0
    _case("D", "alltoall", 1500, 1100, worlds=(2,)),                     # 275 P rows per owner: both over the cap
    _case("H_alltoall_D", "alltoall", 1500, 700, worlds=(2,), layout="hash"),
    _case("D3", "alltoall", 1500, 60, cap=2, worlds=(3,)),               # D': over a small cap on every rank
    _case("E", "alltoall", 1500, 1200, layout="lopsided"),               # rank 0 over, the others join its settlement
    _case("H_alltoall_E", "alltoall", 1500, 700, worlds=(3,), layout="hash"),
    _case("F_allgather_k1", "allgather", 1500, 61, k=1),                 # odd q: uneven slices
    _case("F_allgather_k14", "allgather", 1500, 61, k=14),               # rows 4-byte aligned: no 16-byte stores
    _case("F_allgather_k32", "allgather", 1500, 61, k=32),
    _case("F_alltoall_k1", "alltoall", 1500, 61, k=1),
    _case("F_alltoall_k14", "alltoall", 1500, 61, k=14),
    _case("F_alltoall_k32", "alltoall", 1500, 61, k=32),
    _case("G_allgather", "allgather", 40, 2, worlds=(3,)),
    _case("G_alltoall", "alltoall", 40, 2, worlds=(3,)),                 # rank 2 owns no target (qr == 0)
    _case("I_allgather", "allgather", 20, 40, worlds=(3,)),              # every shard < k ids: NONE-padded records
    _case("I_alltoall", "alltoall", 20, 40, worlds=(3,)),
    _case("J_scan", "allgather", 1500, 60, producer="scan"),             # A's data, records from K1
    _case("J_index", "allgather", 1500, 60, producer="index"),           # ... and from K4/K5
)
BY_NAME = {c.name: c for c in CASES}


def cases_for(world):
    return [c for c in CASES if world in c.worlds]


def p_rows(case):
    """(q,) bool: the P targets (first 64 bits = the crafted ids')"""
    p = np.zeros(case.q, bool)
    if case.layout == "base":
        p[::2] = True
    elif case.layout == "lopsided":
        p[:300] = True
    return p


@functools.lru_cache(maxsize=None)
def data(case):
    """(ids (n, 20), targets (q, 20)) of the case; computed once, never written to"""
    ids = O.gen_ids(SEED, case.n)
    tg = O.gen_ids(SEED + 1, case.q)
    if case.layout != "hash":
        ids[::4, :8] = ids[1, :8]
        tg[p_rows(case), :8] = ids[1, :8]
    ids.setflags(write=False)
    tg.setflags(write=False)
    return ids, tg


@functools.lru_cache(maxsize=None)
def flat_topk(case):
    """the flat exact top-k of every target over all n ids: (idx (q, k), cnt (q,))"""
    ids, tg = data(case)
    idx, cnt = O.topk(ids, tg, case.k, threads=2)
    idx.setflags(write=False)
    cnt.setflags(write=False)
    return idx, cnt


def target_slice(case, world, rank):
    """[tlo, thi): the targets whose final rows `rank` holds"""
    return (0, case.q) if case.exchange == "allgather" else sharding.shard_range(case.q, world, rank)


def expected(case, world, rank):
    tlo, thi = target_slice(case, world, rank)
    idx, cnt = flat_topk(case)
    return idx[tlo:thi], cnt[tlo:thi]


def tie_bounds(case, world, rank):
    """(lowest, highest) tie count of `rank`, or None where none is stated.  Lowest: the P targets
    of its slice -- every shard holds at least k crafted ids there (n >= 1500: 125 or more per
    shard, k <= 32), so every shard's whole list shares 64 bits with the target and the lists'
    heads tie at place 0.  Highest: the slice's rows.  Hash ids: no row ties."""
    tlo, thi = target_slice(case, world, rank)
    if case.layout == "hash":
        return 0, 0
    if case.n < 1500:
        return None
    return int(p_rows(case)[tlo:thi].sum()), thi - tlo


def shapes(case, world, rank):
    tlo, thi = target_slice(case, world, rank)
    qr = thi - tlo
    return {"rec": (case.q, case.k, 3), "xch": (world * qr, case.k, 3), "idx": (max(qr, 1), case.k),
            "cnt": (max(qr, 1),)}


class Bufs:
    """One flat int32 buffer per role, sized for the largest case of the run: every case takes
    views of the same storage, so a lookup meets the previous lookups' data wherever it does not
    write (the record, exchange and output buffers a pipelined caller reuses)."""

    def __init__(self, cases, world, rank, device):
        need = {}
        for c in cases:
            for name, shape in shapes(c, world, rank).items():
                need[name] = max(need.get(name, 1), int(np.prod(shape)))
        self.flat = {name: torch.full((m,), -7, dtype=torch.int32, device=device) for name, m in need.items()}
        self.tx = {}

    def view(self, name, shape):
        return self.flat[name][:int(np.prod(shape))].view(shape)

    def tie_exchange(self, case, world):
        """the TieExchange of (cap, k), built once with sharding.TIE_CAP = cap and reused"""
        sharding.TIE_CAP = case.cap
        key = (case.cap, case.k)
        if key not in self.tx:
            self.tx[key] = sharding.TieExchange(world, case.k, self.flat["rec"].device)
        return self.tx[key]


def run(case, world, rank, ops, rec, lo, bufs, sync=lambda: None, stream=None):
    """One lookup as a pipelined caller issues it.  rec: this rank's (q, k, 3) records (a view of
    bufs' "rec"); lo: its shard's first global index.  Returns (rows (qr, k) uint32, counts (qr,)
    uint32, tie count, flag read before the settlement)."""
    k = case.k
    tlo, thi = target_slice(case, world, rank)
    qr = thi - tlo
    sh = shapes(case, world, rank)
    oi, oc = bufs.view("idx", sh["idx"]), bufs.view("cnt", sh["cnt"])
    tx = bufs.tie_exchange(case, world)
    if case.exchange == "allgather":
        g = sharding.gather_records(rec, out=bufs.view("xch", sh["xch"]))
        sharding.merge_allgather(ops, rec, g, k, oi, oc, tx, lo, stream)
        flag = sharding.unsettled(tx)
        sync()
        count = sharding.settle_overflow_allgather(ops, rec, g, k, oi, oc, tx, lo, stream)
    else:
        ex = sharding.exchange_records(rec, out=bufs.view("xch", sh["xch"]))
        sharding.merge_alltoall(ops, rec, ex, k, tlo, oi, oc, tx, lo, stream)
        flag = sharding.unsettled(tx)
        sync()
        count = sharding.settle_overflow_alltoall(ops, rec, ex, k, tlo, oi, oc, tx, lo, stream)
    sync()
    return (oi[:qr].cpu().numpy().view(np.uint32).copy(), oc[:qr].cpu().numpy().view(np.uint32).copy(), count,
            bool(flag))


def verdict(case, world, rank, rows, counts, count, flagged):
    """What a rank reports of one case: a dict of plain values (one JSON line of the GPU worker)."""
    want, wcnt = expected(case, world, rank)
    bad = np.nonzero((rows != want).any(axis=1) | (counts != wcnt))[0]
    out = {"case": case.name, "world": world, "rank": rank, "exact": bad.size == 0, "count": int(count),
           "flagged": bool(flagged), "first_bad": None}
    if bad.size:
        i = int(bad[0])
        out["first_bad"] = {"row": i, "got": [int(x) for x in rows[i]], "want": [int(x) for x in want[i]],
                            "got_cnt": int(counts[i]), "want_cnt": int(wcnt[i])}
    return out


def check(results, world):
    """The table's assertions over one world's reports (results: a list of `verdict` dicts, every
    case of the world on every rank).  Returns (ranks that overflowed, ranks that did not)."""
    by = {(r["case"], r["rank"]): r for r in results}
    over = under = 0
    for c in cases_for(world):
        for rank in range(world):
            r = by[(c.name, rank)]
            assert r["exact"], r
            assert r["flagged"] == (r["count"] > c.cap), r
            b = tie_bounds(c, world, rank)
            if b is not None:
                assert b[0] <= r["count"] <= b[1], (r, b)
            over += r["flagged"]
            under += not r["flagged"]
    return over, under
