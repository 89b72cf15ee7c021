"""bench.py's multi-GPU launch (VERDICT r2 missing #1): `python bench.py --gpus N` started as one
process runs N ranks under torch.distributed.run, decided before anything touches the GPU; and the
bench's cfg-1/cfg-4 workload tables are the ones the reference's onNewNode grows.  CPU only, except
the plain run with --dump-outputs (marked gpu)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _run(args, env_extra=None, timeout=120):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env.update(env_extra or {})
    r = subprocess.run([sys.executable, BENCH] + args, capture_output=True, text=True, timeout=timeout, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    return [json.loads(line) for line in r.stdout.splitlines() if line.startswith("{")]


def test_gpus_n_builds_launcher():
    (plan,) = _run(["--gpus", "4", "--steps", "7", "--dry-run"])
    assert plan["mode"] == "launcher" and plan["gpus"] == 4
    cmd = plan["cmd"]
    assert cmd[1:3] == ["-m", "torch.distributed.run"]
    assert "--nproc-per-node=4" in cmd and "--nnodes=1" in cmd
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1"
    assert cmd[cmd.index(BENCH) + 1:] == ["--gpus", "4", "--steps", "7", "--dry-run"]   # flags passed through
    assert plan["env"]["HSA_ENABLE_IPC_MODE_LEGACY"] == os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY")


def test_gpus_n_launches_n_ranks():
    """The launcher really starts N ranks (each prints its identity and exits before any GPU call)."""
    lines = _run(["--gpus", "2", "--dry-run-ranks"])
    assert sorted(l["rank"] for l in lines) == [0, 1]
    assert all(l["mode"] == "rank" and l["world_size"] == 2 for l in lines)
    assert sorted(l["local_rank"] for l in lines) == [0, 1]


def test_inside_torchrun_no_relaunch():
    (me,) = _run(["--gpus", "2", "--dry-run"], {"WORLD_SIZE": "2", "RANK": "1", "LOCAL_RANK": "1"})
    me.pop("plan")
    assert me == {"mode": "rank", "gpus": 2, "world_size": 2, "rank": 1, "local_rank": 1}
    (one,) = _run(["--dry-run"])
    assert one["mode"] == "single" and one["world_size"] == 1


@pytest.mark.parametrize("world", [2, 4, 8])
def test_multi_gpu_default_is_the_metric_workload(world):
    """N > 1 measures the metric's own workload by default -- the 2^24 cfg-2 ids and
    65,536 targets in TOTAL, strong scaling, on the north-star broadcast route (range shards, K6
    record mode, RCCL all-gather, K3) -- and N = 1 is the first point of the same series."""
    (me,) = _run(["--gpus", str(world), "--dry-run"], {"WORLD_SIZE": str(world), "RANK": "0", "LOCAL_RANK": "0"})
    assert me["plan"] == {"route": "broadcast", "scaling": "strong", "world": world, "n_total": 16777216,
                          "q_total": 65536, "exchange": "allgather"}
    (one,) = _run(["--dry-run"])
    assert one["plan"] == {"route": "broadcast", "scaling": "strong", "world": 1, "n_total": 16777216,
                           "q_total": 65536, "exchange": None}
    # the prefix route stays available, labelled weak
    (pw,) = _run(["--gpus", str(world), "--dry-run", "--route", "prefix"],
                 {"WORLD_SIZE": str(world), "RANK": "0", "LOCAL_RANK": "0"})
    assert pw["plan"]["route"] == "prefix" and pw["plan"]["scaling"] == "weak"
    assert pw["plan"]["n_total"] == world * 16777216


def test_rehearse_plan_two_ranks():
    """the one-GPU rehearsal (--rehearse-one-gpu --gpus 2) runs the same default plan on each rank"""
    lines = _run(["--gpus", "2", "--dry-run-ranks", "--rehearse-one-gpu"])
    assert len(lines) == 2
    for l in lines:
        assert l["plan"]["route"] == "broadcast" and l["plan"]["n_total"] == 16777216
        assert l["plan"]["scaling"] == "strong" and l["plan"]["world"] == 2


def test_bench_tables_are_onnewnode_grown():
    """bench.grow_table (cfg 1 and cfg 4 inputs) == the oracle's restated RoutingTable::onNewNode
    (src/routing_table.cpp:204-262): same buckets, offsets and node order."""
    sys.path.insert(0, ROOT)
    import bench
    for seed, n in ((2024, 10000), (5, 3000), (11, 40000)):
        rng = np.random.default_rng(seed)
        myid = np.frombuffer(rng.bytes(20), dtype=np.uint8).copy()
        ids = np.frombuffer(rng.bytes(20 * n), dtype=np.uint8).reshape(-1, 20)
        got = bench.grow_table(myid, ids)
        want = O.Table(myid).grow(ids).export()
        for g, w in zip(got, want):
            assert np.array_equal(g, w)
    myid, firsts, off, nodes = bench.cfg1_table(2024)
    assert 80 <= nodes.shape[0] <= 110 and off[-1] == nodes.shape[0]


def test_dump_outputs_files(tmp_path):
    """--dump-outputs: float64 .npy files, exact for uint32 values; past 64 MB in all a fixed
    seeded row sample (the same rows on every run) with the row numbers beside it."""
    sys.path.insert(0, ROOT)
    import bench
    a = bench.parse(["--dump-outputs", str(tmp_path), "--steps", "3"])
    assert a.dump_outputs == str(tmp_path) and a.steps == 3 and not a.full
    assert bench.parse(["--full"]).full
    idx = np.arange(40, dtype=np.uint32).reshape(5, 8) + np.uint32(0xFFFFFF00)
    cnt = np.full(5, 8, np.uint32)
    bench.dump_outputs(str(tmp_path / "a"), idx, cnt)
    got = np.load(tmp_path / "a" / "indices.npy")
    assert got.dtype == np.float64 and np.array_equal(got, idx) and not (tmp_path / "a" / "rows.npy").exists()
    assert np.array_equal(np.load(tmp_path / "a" / "counts.npy"), cnt)
    assert bench.DUMP_MAX_BYTES == 64 << 20
    limit = 1 << 16
    rows_max = limit // (8 * 3)
    big = np.arange(rows_max + 7, dtype=np.uint32).reshape(-1, 1)
    for d in ("b", "c"):
        bench.dump_outputs(str(tmp_path / d), big, big[:, 0], rank=1, max_bytes=limit)
    rows = np.load(tmp_path / "b" / "rows_rank1.npy")
    assert rows.shape == (rows_max,) and np.all(np.diff(rows) > 0)
    assert np.array_equal(rows, np.load(tmp_path / "c" / "rows_rank1.npy"))
    assert np.array_equal(np.load(tmp_path / "b" / "indices_rank1.npy")[:, 0], rows)
    total = sum(os.path.getsize(tmp_path / "b" / f) for f in os.listdir(tmp_path / "b"))
    assert total <= limit + 3 * 128   # the arrays fit the limit; each .npy adds its 128-byte header


@pytest.mark.gpu
def test_plain_run_is_the_headline_and_dumps_the_last_step(tmp_path):
    """A plain run prints the headline alone (nothing of --full's legs) and --dump-outputs holds
    what the timed path returned: bit-equal to the oracle over the same seeded inputs."""
    n, q, k, seed = 100003, 301, 8, 77
    (line,) = _run(["--gpus", "1", "--steps", "3", "--warmup", "1", "--n", str(n), "--q", str(q), "--seed", str(seed),
                    "--dump-outputs", str(tmp_path)])
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in line
    assert line["steps"] == 3 and line["ms_per_step"] > 0
    assert abs(line["value"] - q / (line["ms_per_step"] * 1e-3)) <= 1e-6 * line["value"]
    for key in ("roofline", "latency_ms_per_batch", "cpu_baseline", "small_batch", "cfg3_shard", "verified_exact"):
        assert key not in line
    want, wcnt = O.topk(O.gen_ids(seed, n), O.gen_ids(seed + 1, q), k)
    idx, cnt = np.load(tmp_path / "indices.npy"), np.load(tmp_path / "counts.npy")
    assert idx.dtype == np.float64 and idx.shape == (q, k) and cnt.shape == (q,)
    assert np.array_equal(idx, want) and np.array_equal(cnt, wcnt)


def test_classify_threads_match():
    ids = O.gen_ids(3, 50001)
    myid = O.gen_ids(4, 1)[0]
    firsts, _, _ = O.Table(myid).grow(O.gen_ids(5, 20000)).export()
    a, ha = O.classify(firsts, myid, ids)
    b, hb = O.classify(firsts, myid, ids, threads=5)
    assert np.array_equal(a, b) and np.array_equal(ha, hb) and int(ha.sum()) == 50001
