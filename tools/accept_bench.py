"""Accept mask (dhtgpu_set_accept ...): what a mask change and a masked lookup cost.

Id set: --n ids generated in HBM (splitmix64 stream), masks seeded at the --fractions accepted.
Every figure is wall clock around a synchronised call, median of --reps runs after warm-up.
Reports, as one JSON line:
  * view rebuild (count + scan + compaction, opendht_amd/csrc/view.hip) per fraction, its
    fraction of 8 TB/s on the algorithmic bytes (20 n + n/8 read, 24 n_acc written), and the
    yardstick: dhtgpu_select_prefix_dev with pbits = 1 on the same planes (about half selected);
  * set_accept -> first answer, end to end (mask upload, rebuild, one K6 call);
  * the K6 step (--q targets, k = 8) unmasked and per fraction, with per-kernel device times;
  * --subs: the per-mask-change cost at a sub-partitioned size (3 * 2^24 ids, every third
    rejected, 2^18 targets): view + sub-partition rebuild + the call, against the steady call.
--parent: the unmasked K6 step only (runs on a library built before the mask existed, loaded
through DHTGPU_LIB, as the yardstick of the masked step).
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
ap.add_argument("--n", type=int, default=1 << 24)
ap.add_argument("--q", type=int, default=65536)
ap.add_argument("--k", type=int, default=8)
ap.add_argument("--reps", type=int, default=25)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--seed", type=int, default=2024)
ap.add_argument("--fractions", type=float, nargs="+", default=[0.5, 0.9])
ap.add_argument("--parent", action="store_true")
ap.add_argument("--subs", action="store_true")
a = ap.parse_args()

dev = torch.device("cuda", 0)
torch.cuda.set_device(0)
L = opendht_amd.lib()
HBM = 8e12


def timed(fn, reps=a.reps, warmup=a.warmup):
    """median and (min, max) wall seconds of fn(), which must end synchronised"""
    for _ in range(warmup):
        fn()
    xs = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        xs.append(time.perf_counter() - t0)
    return statistics.median(xs), min(xs), max(xs)


def us(t):
    return {"median_us": t[0] * 1e6, "min_us": t[1] * 1e6, "max_us": t[2] * 1e6}


ctx = opendht_amd.Context(0)
ctx.gen_ids(a.seed, a.n)
n, q, k = a.n, a.q, a.k
ts = (q + 63) // 64 * 64
tp = torch.empty(5 * ts, dtype=torch.int32, device=dev)
assert L.dhtgpu_gen_dev(a.seed + 7, 0, q, tp.data_ptr(), ts, None) == 0
o_idx = torch.empty((q, k), dtype=torch.int32, device=dev)
o_cnt = torch.empty(q, dtype=torch.int32, device=dev)
torch.cuda.synchronize()


def step():
    ctx.batch_topk_dev(tp.data_ptr(), ts, q, k, o_idx.data_ptr(), o_cnt.data_ptr(), None, 0, ctx.stream)
    torch.cuda.synchronize()


def kernels():
    ms, fb, surv, wave = ctx.batch_topk_timed(tp.data_ptr(), ts, q, k, o_idx.data_ptr(), o_cnt.data_ptr(), ctx.stream)
    return {"f1_us": ms[0] * 1e3, "f2_us": ms[1] * 1e3, "f3_us": ms[2] * 1e3, "f4_us": ms[3] * 1e3,
            "fallback_targets": fb, "survivors": surv}


out = {"metric": "accept mask: view rebuild and masked K6 step", "unit": "us", "n_gpus": 1, "higher_is_better": False,
       "config": {"n_ids": n, "targets": q, "k": k, "reps": a.reps, "warmup": a.warmup,
                  "lib": os.path.basename(opendht_amd.LIB_PATH)},
       "timing": "wall clock around a synchronised call, median of reps after warm-up",
       "data": "synthetic: splitmix64 ids in HBM, seeded masks"}
out["k6_step_unmasked"] = dict(us(timed(step)), kernels=kernels())
out["value"] = out["k6_step_unmasked"]["median_us"]

if not a.parent:
    # the yardstick compaction: the setup-time prefix selection, about half the ids
    planes, stride = ctx.ids_dev()
    sel_out = torch.empty(5 * stride, dtype=torch.int32, device=dev)
    sel_idx = torch.empty(stride, dtype=torch.int32, device=dev)
    sel_n = [0]

    def select():
        sel_n[0] = ctx.select_prefix_dev(planes, stride, n, 1, 0, sel_out.data_ptr(), stride, sel_idx.data_ptr(), ctx.stream)

    t = timed(select)
    out["select_prefix_yardstick"] = dict(us(t), selected=int(sel_n[0]),
                                          note="dhtgpu_select_prefix_dev pbits=1: count + scan + sync + count + scan + compact")
    del sel_out, sel_idx
    rng = np.random.default_rng(a.seed)
    one = np.array([0], np.uint32)
    out["fractions"] = {}
    for f in a.fractions + [1.0]:
        mask = (rng.random(n) < f).astype(np.uint8) if f < 1.0 else np.ones(n, np.uint8)
        r = {}
        # end to end: mask upload (host bytes), rebuild, one K6 call
        def e2e():
            ctx.set_accept(mask)
            step()
        r["set_accept_to_first_answer"] = us(timed(e2e, reps=max(5, a.reps // 5), warmup=2))
        nacc = ctx.num_accepted
        r["accepted"] = nacc
        if f < 1.0:
            def rebuild():
                ctx.update_accept(one, mask[:1])   # (the same value: marks the view stale)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                ctx.num_accepted
                return time.perf_counter() - t0
            for _ in range(a.warmup):
                rebuild()
            xs = [rebuild() for _ in range(a.reps)]
            med = statistics.median(xs)
            byts = 20 * n + n / 8 + 24 * nacc
            r["view_rebuild"] = {"median_us": med * 1e6, "min_us": min(xs) * 1e6, "max_us": max(xs) * 1e6,
                                 "algorithmic_bytes": byts, "fraction_of_8TBps": byts / med / HBM}
        r["k6_step"] = dict(us(timed(step)), kernels=kernels())
        out["fractions"][f"{f:g}"] = r
    ctx.set_accept(None)
    out["k6_step_unmasked_again"] = us(timed(step))

if a.subs and not a.parent:
    ctx.close()
    ctx = opendht_amd.Context(0)
    n2, q2 = 3 << 24, 1 << 18
    ctx.gen_ids(a.seed + 1, n2)
    m2 = np.ones(n2, np.uint8)
    m2[::3] = 0
    ts2 = q2
    tp2 = torch.empty(5 * ts2, dtype=torch.int32, device=dev)
    assert L.dhtgpu_gen_dev(a.seed + 9, 0, q2, tp2.data_ptr(), ts2, None) == 0
    c2 = torch.empty(q2, dtype=torch.int32, device=dev)
    ctx.set_accept(m2)
    flip = np.array([1], np.uint32)
    state = [0]
    out["subpartitioned"] = {"n_ids": n2, "accepted": ctx.num_accepted, "targets": q2}
    for k2 in (8, 32):   # (on 256 CUs one plan serves 2^25 ids at k = 8; k = 32 runs over two sub-partitions)
        o2 = torch.empty((q2, k2), dtype=torch.int32, device=dev)

        def step2():
            ctx.batch_topk_dev(tp2.data_ptr(), ts2, q2, k2, o2.data_ptr(), c2.data_ptr(), None, 0, ctx.stream)
            torch.cuda.synchronize()

        def change():
            ctx.update_accept(flip, np.array([state[0]], np.uint8))
            state[0] ^= 1
            step2()

        def view_only():
            ctx.update_accept(flip, np.array([state[0]], np.uint8))
            state[0] ^= 1
            ctx.num_accepted

        t0 = time.perf_counter()
        step2()
        first = time.perf_counter() - t0
        out["subpartitioned"][f"k{k2}"] = {"first_call_us": first * 1e6, "steady_call": us(timed(step2, reps=10, warmup=2)),
                                           "mask_change_then_call": us(timed(change, reps=5, warmup=1)),
                                           "mask_change_view_only": us(timed(view_only, reps=5, warmup=1)),
                                           "sub_handles_active": ctx.sub_handles_active(q2, k2)}

print(json.dumps(out), flush=True)
ctx.close()
