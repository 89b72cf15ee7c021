"""Resident routing table (dhtgpu_rt_*): what a find_node answer costs from the device mirror,
against the snapshot entry points it sits beside.

Table: BASELINE cfg 1's (bench.cfg1_table: about 12 buckets and 91 nodes, grown from 10,000 random
ids), every node good, IPv4 tails.  Targets: seeded random ids.  Per batch size q in --qs, as one
JSON line:
  yardstick (the parent's code, unchanged)
    find_closest                      dhtgpu_find_closest: the table crosses PCIe on every call
    find_closest_buffer_nodes         ... followed by dhtgpu_buffer_nodes_ids (the reply's bytes)
  resident
    rt_find_closest / rt_reply        the host forms: targets up, results down, one synchronise
    rt_find_closest_dev / rt_reply_dev  the stream-ordered forms on device-resident targets
  plus rt_set (a table upload) and rt_set_good (a good-bit refresh).
Host forms and the yardstick: wall clock around the synchronous call, median of --reps after
warm-up.  _dev forms: HIP events around --calls back-to-back calls on the context's stream after
warm-up, divided by the number of calls (device time per call once the queue is full), and the wall
clock of the same loop ended by one synchronise (what the host pays per call to enqueue).
Every timed path's results are compared with the yardstick's before anything is reported.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
import opendht_amd  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--qs", type=int, nargs="+", default=[1, 64, 1024, 65536])
ap.add_argument("--reps", type=int, default=25)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--calls", type=int, default=200)
ap.add_argument("--seed", type=int, default=2024)
a = ap.parse_args()

dev = torch.device("cuda", 0)
torch.cuda.set_device(0)


def timed(fn, reps=a.reps, warmup=a.warmup):
    """median and (min, max) wall microseconds of fn(), which must end synchronised"""
    for _ in range(warmup):
        fn()
    xs = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        xs.append((time.perf_counter() - t0) * 1e6)
    return {"median_us": statistics.median(xs), "min_us": min(xs), "max_us": max(xs)}


def timed_dev(call, stream):
    """device microseconds per call (events around a.calls calls) and wall microseconds per call"""
    for _ in range(a.warmup):
        call()
    torch.cuda.synchronize()
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    xs, ws = [], []
    for _ in range(3):
        t0 = time.perf_counter()
        ev0.record(stream)
        for _ in range(a.calls):
            call()
        ev1.record(stream)
        ev1.synchronize()
        ws.append((time.perf_counter() - t0) * 1e6 / a.calls)
        xs.append(ev0.elapsed_time(ev1) * 1e3 / a.calls)
    return {"device_us_per_call": statistics.median(xs), "device_us_min": min(xs), "device_us_max": max(xs),
            "wall_us_per_call": statistics.median(ws), "calls": a.calls}


myid, firsts, off, nodes = bench.cfg1_table(a.seed)
nn = nodes.shape[0]
good = np.ones(nn, np.uint8)
tail = np.random.default_rng(a.seed + 2).integers(0, 256, size=(nn, 6), dtype=np.uint8)
ctx = opendht_amd.Context(0)
stream = torch.cuda.ExternalStream(ctx.stream, device=dev)
out = {"metric": "resident routing table: find_node answers per call", "unit": "us", "n_gpus": 1,
       "higher_is_better": False,
       "config": {"table": f"{firsts.shape[0]} buckets, {nn} nodes (cfg 1)", "count": 8, "af": 4, "reps": a.reps,
                  "warmup": a.warmup, "calls": a.calls},
       "timing": {"host forms and yardstick": "wall clock around the synchronous call, median of reps",
                  "_dev forms": "HIP events around `calls` back-to-back calls / calls; wall = the same loop with one synchronise"},
       "data": "synthetic: cfg-1 table from seeded random ids, seeded random targets"}
out["rt_set"] = timed(lambda: ctx.rt_set(myid, firsts, off, nodes, tail, 4))


def refresh():
    ctx.rt_set_good(good)
    torch.cuda.synchronize()


out["rt_set_good"] = timed(refresh)
out["q"] = {}
for q in a.qs:
    tg = np.frombuffer(np.random.default_rng(a.seed + 1).bytes(20 * q), dtype=np.uint8).reshape(-1, 20).copy()
    reps = a.reps if q <= 4096 else max(5, a.reps // 3)
    r = {}
    want, wcnt = ctx.find_closest(firsts, off, nodes, good, tg, 8)
    wbytes, wlen = ctx.buffer_nodes_ids(nodes, tail, 4, tg, want)
    got, cnt = ctx.rt_find_closest(tg, 8)
    rbytes, rlen = ctx.rt_reply(tg)
    assert np.array_equal(got, want) and np.array_equal(cnt, wcnt), "rt_find_closest differs from find_closest"
    assert np.array_equal(rlen, wlen) and np.array_equal(rbytes, wbytes), "rt_reply differs from find_closest + buffer_nodes_ids"
    r["find_closest"] = timed(lambda: ctx.find_closest(firsts, off, nodes, good, tg, 8), reps)

    def two_calls():
        idx, _ = ctx.find_closest(firsts, off, nodes, good, tg, 8)
        ctx.buffer_nodes_ids(nodes, tail, 4, tg, idx)

    r["find_closest_buffer_nodes"] = timed(two_calls, reps)
    r["rt_find_closest"] = timed(lambda: ctx.rt_find_closest(tg, 8), reps)
    r["rt_reply"] = timed(lambda: ctx.rt_reply(tg), reps)
    ts = (q + 63) // 64 * 64
    planes = np.zeros((5, ts), np.uint32)
    planes[:, :q] = opendht_amd.id_words(tg)
    tp = torch.from_numpy(planes.view(np.int32).reshape(-1)).to(dev)
    o_idx = torch.empty((q, 8), dtype=torch.int32, device=dev)
    o_cnt = torch.empty(q, dtype=torch.int32, device=dev)
    o_rep = torch.zeros((q, 8 * 26), dtype=torch.uint8, device=dev)
    o_len = torch.empty(q, dtype=torch.int32, device=dev)
    r["rt_find_closest_dev"] = timed_dev(
        lambda: ctx.rt_find_closest_dev(tp.data_ptr(), ts, q, 8, o_idx.data_ptr(), o_cnt.data_ptr(), ctx.stream), stream)
    r["rt_reply_dev"] = timed_dev(
        lambda: ctx.rt_reply_dev(tp.data_ptr(), ts, q, o_rep.data_ptr(), o_len.data_ptr(), None, ctx.stream), stream)
    assert np.array_equal(o_idx.cpu().numpy().view(np.uint32), want), "rt_find_closest_dev differs"
    assert np.array_equal(o_len.cpu().numpy().view(np.uint32), wlen) and np.array_equal(o_rep.cpu().numpy(), wbytes), \
        "rt_reply_dev differs"
    out["q"][str(q)] = r
out["value"] = out["q"][str(a.qs[-1])]["rt_reply"]["median_us"]
print(json.dumps(out), flush=True)
ctx.close()
