"""Keys to handles over the resident NodeCache (dhtgpu_ncr_*): what resolving a batch of ids costs on
the device, and -- through tests/cpp/ncresolve_check --bench -- what the same batch costs on the
routes a caller has without it, in the same session.

Mirror: --n seeded random keys (default 2^20), handles 0..n-1.  Per batch size m, on batches drawn
anew for every call (half present keys, half absent ids):
  ncr_find_dev   device time of one call: HIP events on the context's stream, arguments resident
  ncr_find       the host form: ids up, handles down, one synchronise (wall clock)
  variants       with --variants NAME ...: ncr_find_dev of opendht_amd/ab/NAME.so (builds of
                 tools/experiments/build_variant.sh that send every batch through one G), each in a
                 process of its own started between the in-tree measurements -- the G crossover
  adapter        the lines of `ncresolve_check --bench n` when --adapter-exe is given: the host form
                 against m std::map finds (what CacheSlots::slotOf does), ncr_get_nodes against map
                 finds + free-list pops + nc_insert, ncr_extract against map finds + nc_erase
One JSON line.  Exactness is the business of tests/test_gpu_ncresolve.py; this tool only times.
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
ap.add_argument("--ms", type=int, nargs="+", default=[1, 64, 1024, 16384, 131072])
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--seed", type=int, default=2026)
ap.add_argument("--find-only", action="store_true", help="ncr_find_dev alone (what a variant's process runs)")
ap.add_argument("--variants", nargs="*", default=[])
ap.add_argument("--adapter-exe", default=None)
ap.add_argument("--adapter-ms", type=int, nargs="*", default=[], help="batch sizes of the adapter lines (default: its own)")
a = ap.parse_args()

dev = torch.device("cuda", 0)
torch.cuda.set_device(0)


def rand_ids(seed, n):
    return np.frombuffer(np.random.default_rng(seed).bytes(20 * n), dtype=np.uint8).reshape(-1, 20).copy()


def stats(xs):
    return {"median_us": statistics.median(xs), "min_us": min(xs), "max_us": max(xs)}


keys = rand_ids(a.seed, a.n)
rng = np.random.default_rng(a.seed + 1)
ctx = opendht_amd.Context(0)
stream = torch.cuda.ExternalStream(ctx.stream, device=dev)
ctx.nc_set(keys)
out = {"metric": "resident NodeCache: one batch of ids resolved to handles per call", "unit": "us", "n_gpus": 1,
       "higher_is_better": False, "library": os.path.basename(opendht_amd.LIB_PATH),
       "config": {"n": a.n, "ms": a.ms, "reps": a.reps, "warmup": a.warmup},
       "timing": {"wall": "wall clock around the synchronous host form, median of reps after warm-up",
                  "device": "HIP events around one _dev call on the context's stream, median of reps after warm-up"},
       "data": "synthetic: seeded random keys; a batch is half present keys, half absent ids", "shapes": {}}


def batch(m):
    ids = rand_ids(int(rng.integers(1 << 30)), m)
    pick = rng.integers(0, a.n, size=(m + 1) // 2)
    ids[::2] = keys[pick]
    want = np.full(m, 0xFFFFFFFF, np.uint32)
    want[::2] = pick
    return ids, want


for m in a.ms:
    wall, devt, wrong = [], [], 0
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for form in ("dev",) if a.find_only else ("host", "dev"):
        for rep in range(a.warmup + a.reps):
            ids, want = batch(m)
            if form == "host":
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                h = ctx.ncr_find(ids)
                dt = (time.perf_counter() - t0) * 1e6
                if rep >= a.warmup:
                    wall.append(dt)
            else:
                stride = (m + 63) // 64 * 64
                planes = np.zeros((5, stride), np.uint32)
                planes[:, :m] = opendht_amd.id_words(ids)
                d_p = torch.from_numpy(planes.reshape(-1).view(np.int32)).to(dev)
                d_h = torch.zeros(m, dtype=torch.int32, device=dev)
                torch.cuda.synchronize()
                ev0.record(stream)
                ctx.ncr_find_dev(d_p.data_ptr(), stride, m, d_h.data_ptr(), None, ctx.stream)
                ev1.record(stream)
                ev1.synchronize()
                if rep >= a.warmup:
                    devt.append(ev0.elapsed_time(ev1) * 1e3)
                h = d_h.cpu().numpy().view(np.uint32)
            wrong += int(np.count_nonzero(h != want))   # (random 160-bit keys: no duplicates to speak of)
    row = {"ncr_find_dev": stats(devt), "wrong": wrong}
    if wall:
        row["ncr_find"] = stats(wall)
    out["shapes"][f"m={m}"] = row
    print(f"{out['library']} m={m}: dev {statistics.median(devt):.1f} us" +
          (f", host {statistics.median(wall):.1f} us" if wall else ""), file=sys.stderr, flush=True)

failed = False
for name in a.variants:
    lib = os.path.join(ROOT, "opendht_amd", "ab", name + ".so")
    env = dict(os.environ, DHTGPU_LIB=lib)
    res = subprocess.run([sys.executable, os.path.abspath(__file__), "--find-only", "--n", str(a.n), "--reps", str(a.reps),
                          "--warmup", str(a.warmup), "--seed", str(a.seed), "--ms"] + [str(m) for m in a.ms],
                         env=env, capture_output=True, text=True, timeout=600)
    if res.returncode != 0:   # the child failed: nothing more is started on the device
        out.setdefault("variants", {})[name] = f"exit {res.returncode}: {res.stderr[-300:]}"
        failed = True
        break
    out.setdefault("variants", {})[name] = json.loads(res.stdout.strip().splitlines()[-1])["shapes"]
if a.adapter_exe and not failed:
    res = subprocess.run([a.adapter_exe, "--bench", str(a.n)] + [str(m) for m in a.adapter_ms], capture_output=True, text=True, timeout=900)
    out["adapter"] = res.stdout.strip().splitlines()
    if res.returncode != 0:
        out["adapter"].append(f"ncresolve_check --bench: exit {res.returncode}: {res.stderr[-300:]}")
last = f"m={a.ms[-1]}"
out["value"] = out["shapes"][last]["ncr_find_dev"]["median_us"]
print(json.dumps(out), flush=True)
ctx.close()
sys.exit(1 if failed else 0)
