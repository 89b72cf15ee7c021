"""One rank of the one-device, multi-rank sharded lookup (started by test_gpu_sharded.py, one fresh
process per rank): python sharded_worker.py RANK WORLD PORT CASE...

Every rank opens cuda:0, joins a gloo group on the loopback rendezvous (device tensors are staged
through the host by opendht_amd.sharding) and runs the named cases of sharded_cases.py in order,
as bench.py runs a step: its shard into one Context, the targets packed on the device, records
from the case's producer, then sharded_cases.run through sharding.LibOps on ONE stream that is
torch's current one.  One JSON line per case on stdout (sharded_cases.verdict); the first HIP
error or exception ends the process with status 1 and runs no further case."""
import datetime
import json
import os
import sys
import traceback

TESTS = os.path.dirname(os.path.abspath(__file__))
for p in (TESTS, os.path.dirname(TESTS)):
    if p not in sys.path:
        sys.path.insert(0, p)


def produce(ctx, case, tp, ts, rec, lo, stream):
    """this rank's (q, k, 3) records by the case's producer, global indices from `lo`"""
    args = (tp.data_ptr(), ts, case.q, case.k, None, None, rec.data_ptr(), lo, stream)
    if case.producer == "batch":
        ctx.batch_topk_dev(*args)
    elif case.producer == "scan":
        ctx.topk_dev(*args)
    elif case.producer == "index":
        ctx.index_build(stream)
        ctx.index_topk_dev(*args)
    else:
        raise ValueError(f"unknown record producer {case.producer!r}")


def main(rank, world, port, names):
    import torch
    import torch.distributed as dist

    import opendht_amd
    import sharded_cases as SC
    from opendht_amd import sharding

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=60))
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream(dev)
    torch.cuda.set_stream(st)
    stream = st.cuda_stream
    L = opendht_amd.lib()
    ctx = opendht_amd.Context(0)
    cases = [SC.BY_NAME[n] for n in names]
    bufs = SC.Bufs(cases, world, rank, dev)
    for c in cases:
        ids, tg = SC.data(c)
        lo, hi = sharding.shard_range(c.n, world, rank)
        ctx.set_ids(ids[lo:hi])
        ts = (c.q + 63) // 64 * 64
        tp = torch.zeros(5 * ts, dtype=torch.int32, device=dev)
        tb = torch.from_numpy(tg.reshape(-1).copy()).to(dev)
        code = L.dhtgpu_pack_dev(tb.data_ptr(), c.q, tp.data_ptr(), ts, stream)
        if code != 0:
            raise RuntimeError(f"pack_dev failed ({code})")
        rec = bufs.view("rec", (c.q, c.k, 3))
        produce(ctx, c, tp, ts, rec, lo, stream)
        ops = sharding.LibOps(L, ctx, tp.data_ptr(), ts)
        got = SC.run(c, world, rank, ops, rec, lo, bufs, sync=torch.cuda.synchronize, stream=stream)
        print(json.dumps(SC.verdict(c, world, rank, *got)), flush=True)
    torch.cuda.synchronize()
    ctx.close()
    dist.destroy_process_group()


if __name__ == "__main__":
    try:
        main(int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), sys.argv[4:])
    except BaseException:   # a HIP error, a collective's timeout: report it and stop at once
        traceback.print_exc()
        sys.stdout.flush()
        sys.stderr.flush()
        os._exit(1)
