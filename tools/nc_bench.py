"""Resident NodeCache (dhtgpu_nc_*): what a change of the map and a getCachedNodes batch cost from the
resident mirror, against the path a caller has without it (dhtgpu_cache_set / dhtgpu_cache_nodes),
in the same build.

Mirror: --n seeded random keys (default 10^6), handles 0..n-1.  One JSON line:
  mutations, per batch size m in --ms
    nc_insert / nc_erase     m fresh keys into the mirror of n / the same m keys out again (the mirror
                             is back at n keys after each pair)
    cache_set                dhtgpu_cache_set of the resulting n + m keys (version 0: a full upload and sort)
    nc_set                   the same full rebuild through the nc family (what flush() could fall back to)
  lookups, per q in --qs and count in --counts, 30 % of the handles rejected
    nc_nodes                 the host form: targets up, rows down, one synchronise
    nc_nodes_dev             the stream-ordered form on device-resident targets
    cache_nodes              dhtgpu_cache_nodes on the same keys: the accept bytes cross PCIe whole
  plus nc_set_accept (the whole mask) and nc_update_accept (64 handles).
Synchronous calls: wall clock around the call, median of --reps after warm-up.  _dev form: HIP
events around --calls back-to-back calls on the context's stream after warm-up, divided by the
number of calls, and the wall clock of the same loop ended by one synchronise.
Every timed lookup's rows are compared with dhtgpu_cache_nodes' before anything is reported.
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

import opendht_amd  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=1000000)
ap.add_argument("--ms", type=int, nargs="+", default=[1, 1024, 65536])
ap.add_argument("--qs", type=int, nargs="+", default=[1, 64, 1024, 16384])
ap.add_argument("--counts", type=int, nargs="+", default=[8, 14])
ap.add_argument("--reps", type=int, default=15)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--calls", type=int, default=100)
ap.add_argument("--seed", type=int, default=2024)
a = ap.parse_args()

dev = torch.device("cuda", 0)
torch.cuda.set_device(0)


def stats(xs):
    return {"median_us": statistics.median(xs), "min_us": min(xs), "max_us": max(xs)}


def timed(fn, reps=a.reps, warmup=a.warmup):
    """wall microseconds of fn(), which must end synchronised"""
    for _ in range(warmup):
        fn()
    xs = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        xs.append((time.perf_counter() - t0) * 1e6)
    return stats(xs)


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


def rand_ids(seed, n):
    return np.frombuffer(np.random.default_rng(seed).bytes(20 * n), dtype=np.uint8).reshape(-1, 20).copy()


n = a.n
keys = rand_ids(a.seed, n)
ctx = opendht_amd.Context(0)
stream = torch.cuda.ExternalStream(ctx.stream, device=dev)
out = {"metric": "resident NodeCache: mutations and getCachedNodes batches per call", "unit": "us", "n_gpus": 1,
       "higher_is_better": False,
       "config": {"n": n, "ms": a.ms, "qs": a.qs, "counts": a.counts, "rejected": 0.3, "reps": a.reps,
                  "warmup": a.warmup, "calls": a.calls},
       "timing": {"synchronous calls": "wall clock around the call, median of reps",
                  "_dev form": "HIP events around `calls` back-to-back calls / calls; wall = the same loop with one synchronise"},
       "data": "synthetic: seeded random keys and targets"}

ctx.nc_set(keys)
out["nc_set_n"] = timed(lambda: ctx.nc_set(keys), max(3, a.reps // 3), 1)
out["cache_set_n"] = timed(lambda: ctx.cache_set(keys), max(3, a.reps // 3), 1)

# ---- mutations ----------------------------------------------------------------------------------
out["m"] = {}
for m in a.ms:
    fresh = rand_ids(a.seed + 10 + m, m)
    hs = np.arange(n, n + m, dtype=np.uint32)
    both = np.concatenate([keys, fresh])
    ins, era = [], []
    for rep in range(a.warmup + a.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        new = ctx.nc_insert(fresh, hs)
        t1 = time.perf_counter()
        assert new.all() and ctx.nc_size() == n + m
        t2 = time.perf_counter()
        found = ctx.nc_erase(fresh)
        t3 = time.perf_counter()
        assert found.all() and ctx.nc_size() == n
        if rep >= a.warmup:
            ins.append((t1 - t0) * 1e6)
            era.append((t3 - t2) * 1e6)
    full = max(3, a.reps // 3)
    out["m"][str(m)] = {"nc_insert": stats(ins), "nc_erase": stats(era),
                        "cache_set": timed(lambda: ctx.cache_set(both), full, 1),
                        "nc_set": timed(lambda: ctx.nc_set(both), full, 1)}
    ctx.nc_set(keys)

# ---- accept bits --------------------------------------------------------------------------------
accept = (np.random.default_rng(a.seed + 3).random(n) >= 0.3).astype(np.uint8)


def whole_mask():
    ctx.nc_set_accept(accept)
    torch.cuda.synchronize()


def few_bits():
    ctx.nc_update_accept(np.arange(0, 64 * 997, 997, dtype=np.uint32) % n, accept[(np.arange(0, 64 * 997, 997)) % n])
    torch.cuda.synchronize()


out["nc_set_accept"] = timed(whole_mask)
out["nc_update_accept_64"] = timed(few_bits)
ctx.cache_set(keys)

# ---- lookups ------------------------------------------------------------------------------------
out["q"] = {}
for q in a.qs:
    tg = rand_ids(a.seed + 1, q)
    ts = (q + 63) // 64 * 64
    planes = np.zeros((5, ts), np.uint32)
    planes[:, :q] = opendht_amd.id_words(tg)
    tp = torch.from_numpy(planes.view(np.int32).reshape(-1)).to(dev)
    out["q"][str(q)] = {}
    for count in a.counts:
        want, wcnt = ctx.cache_nodes(tg, count, accept)
        got, cnt = ctx.nc_nodes(tg, count)
        assert np.array_equal(got, want) and np.array_equal(cnt, wcnt), "nc_nodes differs from cache_nodes"
        o_h = torch.empty((q, count), dtype=torch.int32, device=dev)
        o_c = torch.empty(q, dtype=torch.int32, device=dev)
        r = {"cache_nodes": timed(lambda: ctx.cache_nodes(tg, count, accept)),
             "nc_nodes": timed(lambda: ctx.nc_nodes(tg, count)),
             "nc_nodes_dev": timed_dev(
                 lambda: ctx.nc_nodes_dev(tp.data_ptr(), ts, q, count, o_h.data_ptr(), o_c.data_ptr(), ctx.stream), stream)}
        assert np.array_equal(o_h.cpu().numpy().view(np.uint32), want), "nc_nodes_dev differs"
        out["q"][str(q)][str(count)] = r
out["value"] = out["q"][str(a.qs[-1])][str(a.counts[0])]["nc_nodes"]["median_us"]
print(json.dumps(out), flush=True)
ctx.close()
