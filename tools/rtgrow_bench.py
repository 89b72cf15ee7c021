"""Growing the resident routing table (dhtgpu_rtg_*): what a flush of m new nodes costs on the
device, against the route that exists without it, and what the handle pass adds to a query.

Tables: BASELINE cfg 1's (bench.cfg1_table: about 13 buckets / 99 nodes) and the same ids learned
by a client (is_client: about 70 buckets / 555 nodes), every node good, IPv4 tails.  New nodes:
seeded random ids.  One JSON line:
  flush, per table and m in --ms
    rtg_on_new_node     the batch applied to the resident table (in its grown form before the call)
    reupload            the yardstick: dhtgpu_rt_set of the table as it is after the batch, under a
                        new version, + dhtgpu_rt_set_good.  The host's re-pack of its own table into
                        the snapshot arrays comes on top of it and is NOT timed here (the arrays are
                        ready), so the yardstick is a lower bound
    oracle_insert       orc_table_insert of the same batch: the CPU body of the same work
    and the crossover of the two routes from a line through each (fixed cost / per-node difference)
  query, per q in --qs
    rt_find_closest_dev / rt_reply_dev on a grown table and on an uploaded table of the same
    content: HIP events around --calls back-to-back calls / calls
Everything is timed in one process: wall clock around the synchronous call, median of --reps after
--warmup.  The resident table is restored before every timed flush (untimed).  Each timed path's
result is compared with the oracle's table before anything is reported.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
import opendht_amd  # noqa: E402
import oracle as O  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--ms", type=int, nargs="+", default=[1, 8, 64, 512])
ap.add_argument("--qs", type=int, nargs="+", default=[1, 64, 1024])
ap.add_argument("--reps", type=int, default=25)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--calls", type=int, default=200)
ap.add_argument("--seed", type=int, default=2024)
a = ap.parse_args()

dev = torch.device("cuda", 0)
torch.cuda.set_device(0)
ctx = opendht_amd.Context(0)
stream = torch.cuda.ExternalStream(ctx.stream, device=dev)


def stats(xs):
    return {"median_us": statistics.median(xs), "min_us": min(xs), "max_us": max(xs)}


def timed(fn, before=None):
    """wall microseconds of fn(), which must end synchronised; before() runs untimed ahead of each call"""
    xs = []
    for i in range(a.warmup + a.reps):
        if before:
            before()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        if i >= a.warmup:
            xs.append((time.perf_counter() - t0) * 1e6)
    return stats(xs)


def timed_dev(call):
    for _ in range(a.warmup):
        call()
    torch.cuda.synchronize()
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    xs = []
    for _ in range(3):
        ev0.record(stream)
        for _ in range(a.calls):
            call()
        ev1.record(stream)
        ev1.synchronize()
        xs.append(ev0.elapsed_time(ev1) * 1e3 / a.calls)
    return {"device_us_per_call": statistics.median(xs), "device_us_min": min(xs), "device_us_max": max(xs), "calls": a.calls}


def line(ms, ys):
    """least-squares y = fixed + per_node * m"""
    per, fixed = np.polyfit(np.array(ms, float), np.array(ys, float), 1)
    return float(fixed), float(per)


rng = np.random.default_rng(a.seed)
myid = np.frombuffer(rng.bytes(20), dtype=np.uint8).copy()
learned = np.frombuffer(rng.bytes(20 * 10000), dtype=np.uint8).reshape(-1, 20)     # bench.cfg1_table's stream
fresh = np.frombuffer(np.random.default_rng(a.seed + 7).bytes(20 * max(a.ms)), dtype=np.uint8).reshape(-1, 20)
out = {"metric": "resident routing table: flush of m new nodes", "unit": "us", "n_gpus": 1, "higher_is_better": False,
       "config": {"ms": a.ms, "qs": a.qs, "reps": a.reps, "warmup": a.warmup, "calls": a.calls},
       "timing": "one process; wall clock around the synchronous call, median of reps after warmup; queries: HIP events "
                 "around `calls` back-to-back calls / calls",
       "data": "synthetic: tables from seeded random ids, seeded random new nodes", "tables": {}}

for name, client in (("cfg1", False), ("client", True)):
    firsts, off, nodes = O.Table(myid, client).grow(learned).export()
    if not client:
        assert np.array_equal(firsts, bench.cfg1_table(a.seed)[1])
    nn = nodes.shape[0]
    tail = np.random.default_rng(a.seed + 2).integers(0, 256, size=(nn, 6), dtype=np.uint8)
    all_good = np.ones(opendht_amd.RTG_MAX_HANDLE, np.uint8)
    res = {"buckets": int(firsts.shape[0]), "nodes": int(nn), "m": {}}

    def restore():
        ctx.rt_set(myid, firsts, off, nodes, tail, 4)
        ctx.rtg_set_state(all_good[:nn])       # the grown form, content unchanged

    for m in a.ms:
        ids = fresh[:m]
        handles = np.arange(20000, 20000 + m, dtype=np.uint32)
        tails = np.random.default_rng(a.seed + 3).integers(0, 256, size=(m, 6), dtype=np.uint8)
        t = O.Table(myid, client).grow(learned)
        want = np.array([t.insert(x) for x in ids], np.uint8)
        f2, o2, n2 = t.export()
        restore()
        got, _, stat = ctx.rtg_on_new_node(ids, handles, None, tails, client)
        gf, go, gn, gh, gs = ctx.rtg_export()
        assert np.array_equal((got == opendht_amd.RTG_PLACED).astype(np.uint8), want), "rtg_on_new_node differs from the oracle"
        assert np.array_equal(gf, f2) and np.array_equal(go, o2) and np.array_equal(gn, n2), "the grown table differs"
        r = {"placed": int(want.sum()), "splits": int(stat[2])}
        r["rtg_on_new_node"] = timed(lambda: ctx.rtg_on_new_node(ids, handles, None, tails, client), restore)
        tail2 = np.random.default_rng(a.seed + 4).integers(0, 256, size=(n2.shape[0], 6), dtype=np.uint8)
        good2 = np.ones(n2.shape[0], np.uint8)
        ver = [1]

        def reupload():
            ver[0] += 1
            ctx.rt_set(myid, f2, o2, n2, tail2, 4, ver[0])
            ctx.rt_set_good(good2)
            torch.cuda.synchronize()

        r["reupload"] = timed(reupload)
        xs = []
        for _ in range(a.reps):
            t = O.Table(myid, client).grow(learned)
            t0 = time.perf_counter()
            for x in ids:
                t.insert(x)
            xs.append((time.perf_counter() - t0) * 1e6)
        r["oracle_insert"] = stats(xs)
        res["m"][str(m)] = r
    if len(a.ms) >= 2:
        fd, pd = line(a.ms, [res["m"][str(m)]["rtg_on_new_node"]["median_us"] for m in a.ms])
        fy, py = line(a.ms, [res["m"][str(m)]["reupload"]["median_us"] for m in a.ms])
        res["fit"] = {"rtg_fixed_us": fd, "rtg_per_node_us": pd, "reupload_fixed_us": fy, "reupload_per_node_us": py,
                      "crossover_m": (fy - fd) / (pd - py) if pd > py and fy > fd else None}

    # the handle pass: the same content grown and uploaded
    res["q"] = {}
    for q in a.qs:
        tg = np.frombuffer(np.random.default_rng(a.seed + 1).bytes(20 * q), dtype=np.uint8).reshape(-1, 20).copy()
        ts = (q + 63) // 64 * 64
        planes = np.zeros((5, ts), np.uint32)
        planes[:, :q] = opendht_amd.id_words(tg)
        tp = torch.from_numpy(planes.view(np.int32).reshape(-1)).to(dev)
        o_idx = torch.empty((q, 8), dtype=torch.int32, device=dev)
        o_cnt = torch.empty(q, dtype=torch.int32, device=dev)
        o_rep = torch.zeros((q, 8 * 26), dtype=torch.uint8, device=dev)
        o_len = torch.empty(q, dtype=torch.int32, device=dev)
        rq = {}
        for form, prepare in (("uploaded", lambda: ctx.rt_set(myid, firsts, off, nodes, tail, 4)), ("grown", restore)):
            prepare()
            rq[form] = {
                "rt_find_closest_dev": timed_dev(lambda: ctx.rt_find_closest_dev(
                    tp.data_ptr(), ts, q, 8, o_idx.data_ptr(), o_cnt.data_ptr(), ctx.stream)),
                "rt_reply_dev": timed_dev(lambda: ctx.rt_reply_dev(
                    tp.data_ptr(), ts, q, o_rep.data_ptr(), o_len.data_ptr(), None, ctx.stream))}
            want_idx, _ = O.find_closest_batch(firsts, off, nodes, np.ones(nn, np.uint8), tg, 8)
            assert np.array_equal(o_idx.cpu().numpy().view(np.uint32), want_idx), "a query differs from the oracle"
        res["q"][str(q)] = rq
    out["tables"][name] = res

out["value"] = out["tables"]["cfg1"]["m"][str(a.ms[0])]["rtg_on_new_node"]["median_us"]
print(json.dumps(out), flush=True)
ctx.close()
