"""Resident searches (dhtgpu_sr_*): what a batch of Dht::refill costs from the resident lists and the
resident NodeCache mirror, against the composition a caller has without them and against the CPU
reference body, in the same build.

Mirror: --n seeded random keys (default 10^6), handles 0..n-1, 30 % rejected; --qs searches with
random targets; count 14.  One JSON line, per number of searches q:
  (a) sr_refill_dev     device time per call: HIP events around --calls back-to-back calls on the
                        context's stream (lists as the first refill left them: the periodic refill),
                        and `first`: one call into freshly opened (empty) lists, median of --reps
  (b) sr_refill         the host form: slots up, counts down, one synchronise (wall clock)
  (c) composed          dhtgpu_nc_nodes, a host gather of the ids of the handles in play into a dense
                        node table, dhtgpu_search_insert with its uploads and downloads (wall clock)
  (d) cpu               the oracle's cached_nodes_batch + search_insert on one thread (wall clock)
and insert: k_sr_insert (host form, and the _dev form by events) against dhtgpu_search_insert on
10,000 searches over 20,000 nodes with up to 60 insertions each, from empty lists.
(a) moves no host data: its arguments are device pointers and scalars.  Every path's rows are compared
before anything is reported.
"""
import argparse
import ctypes
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

import opendht_amd  # noqa: E402
import oracle as O  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=1000000)
ap.add_argument("--qs", type=int, nargs="+", default=[1, 64, 1024, 16384])
ap.add_argument("--count", type=int, default=14)
ap.add_argument("--reps", type=int, default=15)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--calls", type=int, default=100)
ap.add_argument("--seed", type=int, default=2025)
a = ap.parse_args()

dev = torch.device("cuda", 0)
torch.cuda.set_device(0)
NONE = 0xFFFFFFFF


def stats(xs):
    return {"median_us": statistics.median(xs), "min_us": min(xs), "max_us": max(xs)}


def timed(fn, reps=a.reps, warmup=a.warmup, before=None):
    """wall microseconds of fn(), which must end synchronised; before() runs outside the clock"""
    xs = []
    for rep in range(warmup + reps):
        if before:
            before()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        if rep >= warmup:
            xs.append((time.perf_counter() - t0) * 1e6)
    return stats(xs)


def rand_ids(seed, n):
    return np.frombuffer(np.random.default_rng(seed).bytes(20 * n), dtype=np.uint8).reshape(-1, 20).copy()


def dev_i32(x):
    return torch.from_numpy(np.ascontiguousarray(x).view(np.int32)).to(dev)


n, count = a.n, a.count
keys = rand_ids(a.seed, n)
accept = (np.random.default_rng(a.seed + 3).random(n) >= 0.3).astype(np.uint8)
order = np.lexsort(keys.T[::-1])
skeys, sacc = np.ascontiguousarray(keys[order]), np.ascontiguousarray(accept[order])
ctx = opendht_amd.Context(0)
stream = torch.cuda.ExternalStream(ctx.stream, device=dev)
ctx.nc_set(keys)
ctx.nc_set_accept(accept)
qmax = max(a.qs)
ctx.sr_reset(qmax)
out = {"metric": "resident searches: a batch of Dht::refill per call", "unit": "us", "n_gpus": 1, "higher_is_better": False,
       "config": {"n": n, "qs": a.qs, "count": count, "rejected": 0.3, "reps": a.reps, "warmup": a.warmup, "calls": a.calls},
       "timing": {"wall": "wall clock around the synchronous call, median of reps after warm-up",
                  "device": "HIP events around `calls` back-to-back calls on the context's stream / calls"},
       "data": "synthetic: seeded random keys and targets", "q": {}}

for q in a.qs:
    tg = rand_ids(a.seed + 1 + q, q)
    slots = np.arange(q, dtype=np.uint32)
    d_slots = dev_i32(slots)
    d_ins = torch.zeros(q, dtype=torch.int32, device=dev)

    # (d) the reference body on one thread, and the rows every other path must give
    def cpu_body(lists, flags, lens, expired):
        pos, cnt = O.cached_nodes_batch(skeys, sacc, tg, count, threads=1)
        off = np.concatenate([[0], np.cumsum(cnt)]).astype(np.uint64)
        node = np.ascontiguousarray(pos[pos != NONE], dtype=np.uint32)
        tok = np.zeros(max(node.size, 1), np.uint8)
        added = np.zeros(max(node.size, 1), np.uint8)
        u8p, u32p, u64p = (ctypes.POINTER(t) for t in (ctypes.c_uint8, ctypes.c_uint32, ctypes.c_uint64))
        p = lambda x, t: x.ctypes.data_as(t)   # noqa: E731
        O.lib().orc_search_insert(p(skeys, u8p), p(state0, u8p), p(tg, u8p), q, 64, p(lists, u32p), p(flags, u8p),
                                  p(lens, u32p), p(expired, u8p), p(off, u64p), p(node, u32p), p(tok, u8p), p(added, u8p), 1)
        return added

    state0 = np.zeros(n, np.uint8)
    c_lists, c_flags = np.full((q, 64), NONE, np.uint32), np.zeros((q, 64), np.uint8)
    c_lens, c_exp = np.zeros(q, np.uint32), np.zeros(q, np.uint8)
    cpu_body(c_lists, c_flags, c_lens, c_exp)
    want_rows = np.where(c_lists == NONE, NONE, order[np.minimum(c_lists, n - 1)]).astype(np.uint32)   # sorted position -> handle
    r = {"cpu": timed(lambda: cpu_body(c_lists, c_flags, c_lens, c_exp), max(3, a.reps // 3), 1)}

    # (a) / (b): the resident path
    def reopen():
        ctx.sr_open(slots, tg)

    def first_refill():
        ctx.sr_refill_dev(d_slots.data_ptr(), q, count, d_ins.data_ptr(), ctx.stream)
        torch.cuda.synchronize()

    reopen()
    ctx.sr_refill(slots, count)
    rows, _, lens = ctx.sr_lists(slots)
    assert np.array_equal(rows, want_rows) and np.array_equal(lens, c_lens), "sr_refill differs from the CPU body"
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    first = []
    for rep in range(a.warmup + a.reps):
        reopen()
        torch.cuda.synchronize()
        ev0.record(stream)
        ctx.sr_refill_dev(d_slots.data_ptr(), q, count, d_ins.data_ptr(), ctx.stream)
        ev1.record(stream)
        ev1.synchronize()
        if rep >= a.warmup:
            first.append(ev0.elapsed_time(ev1) * 1e3)
    xs, ws = [], []
    for _ in range(3):
        t0 = time.perf_counter()
        ev0.record(stream)
        for _ in range(a.calls):
            ctx.sr_refill_dev(d_slots.data_ptr(), q, count, d_ins.data_ptr(), ctx.stream)
        ev1.record(stream)
        ev1.synchronize()
        ws.append((time.perf_counter() - t0) * 1e6 / a.calls)
        xs.append(ev0.elapsed_time(ev1) * 1e3 / a.calls)
    r["sr_refill_dev"] = {"device_us_per_call": statistics.median(xs), "device_us_min": min(xs), "device_us_max": max(xs),
                          "wall_us_per_call": statistics.median(ws), "calls": a.calls, "first": stats(first)}
    r["sr_refill"] = timed(lambda: ctx.sr_refill(slots, count))
    r["sr_refill_first"] = timed(lambda: ctx.sr_refill(slots, count), before=reopen)
    rows, _, lens = ctx.sr_lists(slots)
    assert np.array_equal(rows, want_rows), "the periodic refill changed the rows"

    # (c) what the parent offers: nc_nodes, a host gather, search_insert (lists kept on the host as handles)
    def composed(lists_h, flags, lens, expired):
        hs, cnt = ctx.nc_nodes(tg, count)
        off = np.concatenate([[0], np.cumsum(cnt)]).astype(np.uint64)
        new = hs[hs != NONE]
        live = lists_h[lists_h != NONE]
        play, inv = np.unique(np.concatenate([live, new]), return_inverse=True)
        table = keys[play]                                  # the host gather of the ids
        dl = np.full(lists_h.shape, NONE, np.uint32)
        dl[lists_h != NONE] = inv[: live.size]
        l2, f2, n2, e2, added = ctx.search_insert(table, np.zeros(play.size, np.uint8), tg, dl, flags, lens, expired, off,
                                                  inv[live.size:].astype(np.uint32), np.zeros(new.size, np.uint8))
        back = np.where(l2 == NONE, NONE, play[np.minimum(l2, play.size - 1)]).astype(np.uint32)
        return back, f2, n2, e2

    empty = (np.full((q, 64), NONE, np.uint32), np.zeros((q, 64), np.uint8), np.zeros(q, np.uint32), np.zeros(q, np.uint8))
    full = composed(*empty)
    assert np.array_equal(full[0], want_rows), "the composition differs from the CPU body"
    r["composed"] = timed(lambda: composed(*full))
    r["composed_first"] = timed(lambda: composed(*empty))
    out["q"][str(q)] = r

# ---- insertNode alone: wave per search against thread per search -------------------------------------
rng = np.random.default_rng(a.seed + 9)
nn, q, maxins = 20000, 10000, 60
ids = rand_ids(a.seed + 20, nn)
ids[: nn // 8, :4] = ids[0, :4]
state = rng.choice([0, 0, 0, 0, 0, 0, 2], size=nn).astype(np.uint8)
state[rng.permutation(nn)[:40]] = 1                       # 40 bad nodes: no list outgrows 64 entries
tg = rand_ids(a.seed + 21, q)
tg[: q // 4, :4] = ids[0, :4]
cnts = rng.integers(0, maxins, size=q)
off = np.concatenate([[0], np.cumsum(cnts)]).astype(np.uint64)
node = rng.integers(0, nn, size=int(off[-1])).astype(np.uint32)
node[::7] = node[::7] % 64
tok = (rng.random(node.size) < 0.3).astype(np.uint8)
slots = np.arange(q, dtype=np.uint32)
empty = (np.full((q, 64), NONE, np.uint32), np.zeros((q, 64), np.uint8), np.zeros(q, np.uint32), np.zeros(q, np.uint8))
ctx.sr_reset(q)
ctx.sr_set_state(state)


def reopen_all():
    ctx.sr_open(slots, tg)


reopen_all()
g_added = ctx.sr_insert(slots, off, node, ids[node], tok)
w = ctx.search_insert(ids, state, tg, *empty, off, node, tok)
rows, flags, lens = ctx.sr_lists(slots)
assert np.array_equal(g_added, w[4]) and np.array_equal(rows, w[0]) and np.array_equal(flags, w[1]), "sr_insert differs"
tot = int(off[-1])
stride = (tot + 63) // 64 * 64
planes = np.zeros((5, stride), np.uint32)
planes[:, :tot] = opendht_amd.id_words(ids[node])
d = [dev_i32(slots), torch.from_numpy(off.view(np.int64)).to(dev), dev_i32(node), dev_i32(planes.reshape(-1)),
     torch.from_numpy(tok).to(dev), torch.zeros(tot, dtype=torch.uint8, device=dev)]
ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
devt = []
for rep in range(a.warmup + a.reps):
    reopen_all()
    torch.cuda.synchronize()
    ev0.record(stream)
    ctx.sr_insert_dev(d[0].data_ptr(), q, d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), stride, d[4].data_ptr(),
                      d[5].data_ptr(), ctx.stream)
    ev1.record(stream)
    ev1.synchronize()
    if rep >= a.warmup:
        devt.append(ev0.elapsed_time(ev1) * 1e3)
assert np.array_equal(d[5].cpu().numpy(), w[4]), "sr_insert_dev differs"
out["insert"] = {"config": {"searches": q, "nodes": nn, "insertions": tot, "max_per_search": maxins},
                 "sr_insert_dev_device": stats(devt),
                 "sr_insert": timed(lambda: ctx.sr_insert(slots, off, node, ids[node], tok), before=reopen_all),
                 "search_insert": timed(lambda: ctx.search_insert(ids, state, tg, *empty, off, node, tok))}
out["value"] = out["q"][str(a.qs[-1])]["sr_refill_dev"]["device_us_per_call"]
print(json.dumps(out), flush=True)
ctx.close()
