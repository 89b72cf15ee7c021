"""The searches' ordered map (dhtgpu_srm_*): what one dhtgpu_srm_offer call costs -- Dht::trySearchInsert
for a batch of learned nodes over the resident searches -- and, through tests/cpp/srmap_check --bench,
what the same batch costs on the two routes a caller has without it, in the same build.

Cache: --n seeded random keys (default 2^20), handles 0..n-1.  Per number of mapped searches ns and
batch size m, on batches drawn anew from the cache for every call:
  converged   lists pre-filled by dhtgpu_sr_refill(count 14) from the whole cache
  fresh       every search opened again (empty) before each call, small m only
One JSON line:
  srm_offer        the host form: handles and ids up, counts, mask and stats down, one synchronise (wall)
  srm_offer_dev    device time of one call: HIP events on the context's stream, arguments resident
  filtered / hops  out_stats[0] / m and out_stats[1] / m of the timed calls (the filter's share; the
                   insertNode calls of the ordered walk per node)
  adapter          the lines of `srmap_check --bench ns` when --adapter-exe is given: offerBatch on the
                   device, the host walk alone (the CPU body), the host walk plus the flush of the
                   pairs it touched through dhtgpu_sr_insert (the parent commit's route)
Exactness is the business of tests/test_gpu_srmap.py; this tool only times.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import opendht_amd  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=1 << 20)
ap.add_argument("--ns", type=int, nargs="+", default=[1024, 16384])
ap.add_argument("--ms", type=int, nargs="+", default=[1, 64, 1024, 16384])
ap.add_argument("--fresh-ms", type=int, nargs="+", default=[1, 64])
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--seed", type=int, default=2026)
ap.add_argument("--adapter-exe", default=None)
a = ap.parse_args()

dev = torch.device("cuda", 0)
torch.cuda.set_device(0)


def rand_ids(seed, n):
    return np.frombuffer(np.random.default_rng(seed).bytes(20 * n), dtype=np.uint8).reshape(-1, 20).copy()


def dev_i32(x):
    return torch.from_numpy(np.ascontiguousarray(x).view(np.int32)).to(dev)


def stats(xs):
    return {"median_us": statistics.median(xs), "min_us": min(xs), "max_us": max(xs)}


keys = rand_ids(a.seed, a.n)
rng = np.random.default_rng(a.seed + 1)
ctx = opendht_amd.Context(0)
stream = torch.cuda.ExternalStream(ctx.stream, device=dev)
ctx.nc_set(keys)
out = {"metric": "searches' ordered map: one Dht::trySearchInsert batch per call", "unit": "us", "n_gpus": 1,
       "higher_is_better": False,
       "config": {"n": a.n, "ns": a.ns, "ms": a.ms, "fresh_ms": a.fresh_ms, "reps": a.reps, "warmup": a.warmup},
       "timing": {"wall": "wall clock around the synchronous host form, median of reps after warm-up",
                  "device": "HIP events around one _dev call on the context's stream, median of reps after warm-up"},
       "data": "synthetic: seeded random keys and targets", "shapes": {}}

for ns in a.ns:
    targets = rand_ids(a.seed + 2 + ns, ns)
    slots = np.arange(ns, dtype=np.uint32)
    ctx.sr_reset(ns)

    def reopen(fill):
        ctx.sr_open(slots, targets)
        if fill:
            ctx.sr_refill(slots, 14)
        ctx.srm_set(slots)

    for regime, ms in (("converged", a.ms), ("fresh", a.fresh_ms)):
        reopen(regime == "converged")
        for m in ms:
            wall, devt, filt, hops, took = [], [], 0, 0, 0
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            for form in ("host", "dev"):
                for rep in range(a.warmup + a.reps):
                    if regime == "fresh":
                        reopen(False)
                    h = rng.integers(0, a.n, size=m).astype(np.uint32)
                    ids = keys[h]
                    if form == "host":
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        cnt, _, st = ctx.srm_offer(h, ids)
                        dt = (time.perf_counter() - t0) * 1e6
                        if rep >= a.warmup:
                            wall.append(dt)
                            filt, hops, took = filt + int(st[0]), hops + int(st[1]), took + int(np.count_nonzero(cnt))
                    else:
                        stride = (m + 63) // 64 * 64
                        planes = np.zeros((5, stride), np.uint32)
                        planes[:, :m] = opendht_amd.id_words(ids)
                        d_h, d_p = dev_i32(h), dev_i32(planes.reshape(-1))
                        d_cnt = torch.zeros(m, dtype=torch.int32, device=dev)
                        torch.cuda.synchronize()
                        ev0.record(stream)
                        ctx.srm_offer_dev(d_h.data_ptr(), d_p.data_ptr(), stride, m, d_cnt.data_ptr(), None, None, ctx.stream)
                        ev1.record(stream)
                        ev1.synchronize()
                        if rep >= a.warmup:
                            devt.append(ev0.elapsed_time(ev1) * 1e3)
            tot = m * a.reps
            print(f"{regime} ns={ns} m={m}: host {statistics.median(wall):.1f} us, dev {statistics.median(devt):.1f} us",
                  file=sys.stderr, flush=True)
            out["shapes"][f"{regime} ns={ns} m={m}"] = {
                "srm_offer": stats(wall), "srm_offer_dev": stats(devt), "filtered": filt / tot, "hops_per_node": hops / tot,
                "nodes_taken": took / tot}
    if a.adapter_exe:
        ctx.sr_reset(1)
        res = subprocess.run([a.adapter_exe, "--bench", str(ns), str(a.n)], capture_output=True, text=True, timeout=900)
        out.setdefault("adapter", []).extend(res.stdout.strip().splitlines())
        if res.returncode != 0:   # the child failed: nothing more is started on the device
            out["adapter"].append(f"srmap_check --bench {ns}: exit {res.returncode}: {res.stderr[-300:]}")
            break
last = f"converged ns={a.ns[-1]} m={a.ms[-1]}"
out["value"] = out["shapes"][last]["srm_offer_dev"]["median_us"] if last in out["shapes"] else None
print(json.dumps(out), flush=True)
ctx.close()
