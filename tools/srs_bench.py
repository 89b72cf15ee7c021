"""Resident searches (dhtgpu_srs_*): what one Dht::searchStep over q find_node searches costs on the
device, against the route a caller has without it.

Mirror: --n seeded random keys (default 10^5), handles 0..n-1, all accepted; --qs searches with random
targets; node_expire 600 ticks, refill count 14.  One JSON line, per number of searches q:
  step_dev       device time per dhtgpu_srs_step_dev call: HIP events around --calls back-to-back calls
                 on the context's stream, the clock one tick further each call (lists full, four requests
                 pending: the periodic step that finds nothing to do), and `first`: one call on freshly
                 opened searches (the refill leg inserts 14 nodes, four requests go out), median of --reps
  step           the host form of the same two: slots up, out_send and out4 down, one synchronise (wall)
  parent         the route without srs: dhtgpu_sr_status and dhtgpu_sr_lists with their D2H copies -- what
                 a host searchStep over a shadow SearchNode table needs of every stepped search -- (wall),
                 and `first`: dhtgpu_sr_refill_dev in front of them on freshly opened searches
The parent route uses entry points the parent commit has too: with DHTGPU_LIB naming that commit's
library only `parent` is measured (no dhtgpu_srs_* there).  The CPU body of the step itself is
`tests/cpp/srstep_check --bench`.  Before anything is reported the step's refill is compared with
dhtgpu_sr_refill's rows and its sends with the rows' first four entries.
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
ap.add_argument("--n", type=int, default=100000)
ap.add_argument("--qs", type=int, nargs="+", default=[1, 1024, 16384])
ap.add_argument("--reps", type=int, default=15)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--calls", type=int, default=100)
ap.add_argument("--seed", type=int, default=2026)
a = ap.parse_args()

dev = torch.device("cuda", 0)
torch.cuda.set_device(0)
E, COUNT = 600, 14
HAVE_SRS = hasattr(opendht_amd.lib(), "dhtgpu_srs_step_dev")


def stats(xs):
    return {"median_us": statistics.median(xs), "min_us": min(xs), "max_us": max(xs)}


def timed(fn, before=None):
    """wall microseconds of fn(), which must end synchronised; before() runs outside the clock"""
    xs = []
    for rep in range(a.warmup + a.reps):
        if before:
            before()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        if rep >= a.warmup:
            xs.append((time.perf_counter() - t0) * 1e6)
    return stats(xs)


def rand_ids(seed, n):
    return np.frombuffer(np.random.default_rng(seed).bytes(20 * n), dtype=np.uint8).reshape(-1, 20).copy()


def dev_i32(x):
    return torch.from_numpy(np.ascontiguousarray(x).view(np.int32)).to(dev)


ctx = opendht_amd.Context(0)
stream = torch.cuda.ExternalStream(ctx.stream, device=dev)
ctx.nc_set(rand_ids(a.seed, a.n))
ctx.sr_reset(max(a.qs))
out = {"metric": "resident searches: one Dht::searchStep over q searches per call", "unit": "us", "n_gpus": 1,
       "higher_is_better": False, "library": "DHTGPU_LIB" if os.environ.get("DHTGPU_LIB") else "this build", "srs": HAVE_SRS,
       "config": {"n": a.n, "qs": a.qs, "node_expire": E, "refill_count": COUNT, "reps": a.reps, "warmup": a.warmup,
                  "calls": a.calls},
       "timing": {"wall": "wall clock around the synchronous call(s), median of reps after warm-up",
                  "device": "HIP events around `calls` back-to-back calls on the context's stream / calls"},
       "data": "synthetic: seeded random keys and targets", "q": {}}
ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
clock = 1000

for q in a.qs:
    tg = rand_ids(a.seed + 1 + q, q)
    slots = np.arange(q, dtype=np.uint32)
    d_slots = dev_i32(slots)
    d_ins = torch.zeros(q, dtype=torch.int32, device=dev)
    r = {}

    def reopen():
        ctx.sr_open(slots, tg)

    def parent_route(first):
        if first:
            ctx.sr_refill_dev(d_slots.data_ptr(), q, COUNT, d_ins.data_ptr(), ctx.stream)
        ctx.sr_status(slots)
        ctx.sr_lists(slots)

    reopen()
    ctx.sr_refill(slots, COUNT)
    want_rows = ctx.sr_lists(slots)[0]
    if HAVE_SRS:
        d_send = torch.zeros(q * 64, dtype=torch.int32, device=dev)
        d_out4 = torch.zeros(q * 4, dtype=torch.int32, device=dev)

        def step_dev():
            ctx.srs_step_dev(d_slots.data_ptr(), q, E, COUNT, d_send.data_ptr(), d_out4.data_ptr(), ctx.stream)

        reopen()
        clock += E + 1
        ctx.srs_set_clock(clock)
        send, out4 = ctx.srs_step(slots, E, COUNT)
        rows = ctx.sr_lists(slots)[0]
        assert np.array_equal(rows, want_rows), "the step's refill differs from sr_refill"
        assert (out4 == [4, 4, COUNT, 8]).all() and np.array_equal(send[:, :4], rows[:, :4]), "the step's sends"
        first = []
        for rep in range(a.warmup + a.reps):
            reopen()
            torch.cuda.synchronize()
            ev0.record(stream)
            step_dev()
            ev1.record(stream)
            ev1.synchronize()
            if rep >= a.warmup:
                first.append(ev0.elapsed_time(ev1) * 1e3)
        xs, ws = [], []
        for _ in range(3):
            t0 = time.perf_counter()
            ev0.record(stream)
            for _ in range(a.calls):
                clock += 1
                ctx.srs_set_clock(clock)
                step_dev()
            ev1.record(stream)
            ev1.synchronize()
            ws.append((time.perf_counter() - t0) * 1e6 / a.calls)
            xs.append(ev0.elapsed_time(ev1) * 1e3 / a.calls)
        o4 = d_out4.cpu().numpy().view(np.uint32).reshape(q, 4)
        assert (o4 == [0, 4, 0, 0]).all(), "the periodic step changed something"
        r["step_dev"] = {"device_us_per_call": statistics.median(xs), "device_us_min": min(xs), "device_us_max": max(xs),
                         "wall_us_per_call": statistics.median(ws), "calls": a.calls, "first": stats(first)}
        r["step"] = timed(lambda: ctx.srs_step(slots, E, COUNT))
        r["step_first"] = timed(lambda: ctx.srs_step(slots, E, COUNT), before=reopen)
    r["parent"] = timed(lambda: parent_route(False))
    r["parent_first"] = timed(lambda: parent_route(True), before=reopen)
    out["q"][str(q)] = r

last = out["q"][str(a.qs[-1])]
out["value"] = last["step_dev"]["device_us_per_call"] if HAVE_SRS else last["parent"]["median_us"]
print(json.dumps(out), flush=True)
ctx.close()
