"""The sharded lookup as it ships, on one device: one process per rank on cuda:0, a gloo group
between them (device tensors staged through the host by opendht_amd.sharding), and the merge and
tie protocol through sharding.LibOps -- the case table of sharded_cases.py, which test_sharding.py
runs over host stand-ins.  What this cannot reach: RCCL itself and more than one device.

Two checks run in this process without a group: sharding._stream, and the kernels' slice
arguments (row_base, target planes offset by a slice start) over three contexts."""
import json
import os
import socket
import subprocess
import sys
import threading

import numpy as np
import pytest

import sharded_cases as SC

pytestmark = pytest.mark.gpu

WORKER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "sharded_worker.py")


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def run_ranks(world, names):
    """One fresh process per rank; every rank gets communicate(timeout=120) -- a hang guard: the
    table's work is milliseconds, the time is process start-up -- and the first rank to exit
    non-zero or to time out has the others killed at once.  Returns [(status, stdout, stderr)]."""
    port = str(_free_port())
    procs = [subprocess.Popen([sys.executable, WORKER, str(r), str(world), port] + list(names),
                              stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for r in range(world)]
    got = [None] * world

    def reap(i):
        try:
            out, err = procs[i].communicate(timeout=120)
            failed = procs[i].returncode != 0
        except subprocess.TimeoutExpired:
            failed = True
        if failed:
            for p in procs:
                if p.poll() is None:
                    p.kill()
            if procs[i].returncode is None:
                out, err = procs[i].communicate()
        got[i] = (procs[i].returncode, out, err)

    th = [threading.Thread(target=reap, args=(i,)) for i in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    return got


@pytest.mark.parametrize("world", [2, 3])
def test_sharded_table(world):
    """Every case of the table on every rank: rows and counts == the flat exact top-k, the device
    flag unsettled(tx) is up exactly where more rows tied than the cap, the tie counts lie within
    the table's bounds, and some rank overflowed while another did not."""
    names = [c.name for c in SC.cases_for(world)]
    got = run_ranks(world, names)
    report = "\n".join(f"--- rank {r}: status {st}\n{out[-3000:]}\n{err[-3000:]}" for r, (st, out, err) in enumerate(got))
    assert all(st == 0 for st, _, _ in got), report
    results = [json.loads(line) for _, out, _ in got for line in out.splitlines() if line.startswith("{")]
    assert len(results) == world * len(names), report
    for c in SC.cases_for(world):   # the observed tie counts next to the table's bounds
        print(c.name, "world", world, "counts", [r["count"] for r in results if r["case"] == c.name], "bounds",
              [SC.tie_bounds(c, world, r) for r in range(world)], "cap", c.cap)
    over, under = SC.check(results, world)
    assert over > 0 and under > 0, (over, under)


def test_stream_check():
    """The lookup's stream is torch's current one or the call is refused."""
    import torch
    from opendht_amd import sharding
    dev = torch.device("cuda", 0)
    t = torch.empty(1, device=dev)
    other = torch.cuda.Stream(dev)
    cur = torch.cuda.current_stream(dev).cuda_stream
    assert other.cuda_stream != cur
    assert sharding._stream(None, t) == cur
    assert sharding._stream(cur, t) == cur
    with pytest.raises(ValueError):
        sharding._stream(other.cuda_stream, t)
    with torch.cuda.stream(other):
        assert sharding._stream(None, t) == other.cuda_stream
        assert sharding._stream(other.cuda_stream, t) == other.cuda_stream
        with pytest.raises(ValueError):
            sharding._stream(cur, t)
    assert sharding._stream(None, torch.empty(1)) is None


@pytest.mark.parametrize("cap", [256, 2])
def test_alltoall_slices_one_process(cap):
    """The kernels' slice arguments without a process group: three range-shard contexts, case C's
    data, and for every owner slice [tlo, thi) K3 on planes offset by tlo, every context's tie
    words with row_base = tlo, and the settlement on the slice == the flat top-k.  cap 2: more
    rows tie than the list takes, so the every-row form follows."""
    import torch
    import opendht_amd
    from opendht_amd import sharding
    c = SC.BY_NAME["C"]
    world, q, k = 3, c.q, c.k
    ids, tg = SC.data(c)
    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream(dev)
    L = opendht_amd.lib()
    shards = []
    sharding.TIE_CAP = cap
    try:
        with torch.cuda.stream(st):
            s = st.cuda_stream
            ts = (q + 63) // 64 * 64
            tp = torch.zeros(5 * ts, dtype=torch.int32, device=dev)
            tb = torch.from_numpy(tg.reshape(-1).copy()).to(dev)
            assert L.dhtgpu_pack_dev(tb.data_ptr(), q, tp.data_ptr(), ts, s) == 0
            bounds = [sharding.shard_range(c.n, world, j)[0] for j in range(world)] + [c.n]
            rec = torch.full((world, q, k, 3), -7, dtype=torch.int32, device=dev)
            ops = []
            for j in range(world):
                cx = opendht_amd.Context(0)
                shards.append(cx)
                cx.set_ids(ids[bounds[j]:bounds[j + 1]])
                cx.batch_topk_dev(tp.data_ptr(), ts, q, k, None, None, rec[j].data_ptr(), bounds[j], s)
                ops.append(sharding.LibOps(L, cx, tp.data_ptr(), ts))
            wall = torch.full((world, q, k, 3), -7, dtype=torch.int32, device=dev)   # every row's words
            for j in range(world):
                ops[j].tie_words(rec[j], bounds[j], None, 0, wall[j], s)
            for owner in range(world):
                tlo, thi = sharding.shard_range(q, world, owner)
                ex = rec[:, tlo:thi].contiguous()
                oi = torch.full((thi - tlo, k), -7, dtype=torch.int32, device=dev)
                oc = torch.full((thi - tlo,), -7, dtype=torch.int32, device=dev)
                ties = torch.full((1 + cap,), -7, dtype=torch.int32, device=dev)
                words = torch.full((world, cap, k, 3), -7, dtype=torch.int32, device=dev)
                ops[owner].merge(ex, tlo, k, oi, oc, ties, s)
                for j in range(world):
                    ops[j].tie_words(rec[j], bounds[j], ties, tlo, words[j], s)
                ops[owner].merge_ties(ex, words, tlo, k, ties, oi, oc, s)
                st.synchronize()
                count = int(ties[0].item())
                lo_b, hi_b = SC.tie_bounds(c, world, owner)
                assert lo_b <= count <= hi_b, (owner, count)
                if cap == 2:
                    assert count > cap, (owner, count)
                    ops[owner].merge_ties(ex, wall[:, tlo:thi].contiguous(), tlo, k, None, oi, oc, s)
                    st.synchronize()
                want, wcnt = SC.flat_topk(c)
                got, gcnt = oi.cpu().numpy().view(np.uint32), oc.cpu().numpy().view(np.uint32)
                bad = np.nonzero((got != want[tlo:thi]).any(axis=1) | (gcnt != wcnt[tlo:thi]))[0]
                assert bad.size == 0, (f"owner {owner} [{tlo}, {thi}): {bad.size} rows differ, first {bad[:5]}: "
                                       f"{got[bad[0]]} vs {want[tlo + bad[0]]}")
    finally:
        sharding.TIE_CAP = 256
        st.synchronize()
        for cx in shards:
            cx.close()
