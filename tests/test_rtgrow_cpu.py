"""CPU-side checks of the growing resident routing table (dhtgpu_rtg_*, opendht_amd/csrc/rtgrow.hip):
the Python model of tests/rtgrow_cases.py pinned to the oracle's table in the all-good regime, the
model's state rules on hand-made rows, the kernels' LDS, and the C++ adapter's host paths.  No GPU
needed.  (Header, exports, binding, the pinned constants and a null context: tests/test_abi.py; the
kernels' register and scratch budget: tests/test_kernel_resources.py.)"""
import subprocess

import numpy as np
import pytest

import cpp_check
import kernel_budget as KB
import oracle as O
import rtgrow_cases as C


# ---- the model is pinned by the oracle ------------------------------------------------------------
def model_equals_oracle(myid, ids, client):
    res, (firsts, off, nodes) = C.oracle_run(myid, ids, client)
    m = C.Model(myid, client)
    got, aux = m.batch(ids, np.arange(ids.shape[0]))
    assert set(got.tolist()) <= {C.RTG_PLACED, C.RTG_FULL} and np.all(aux == C.NONE)
    assert np.array_equal((got == C.RTG_PLACED).astype(np.uint8), res)
    f, o, x, h, st = m.export()
    assert np.array_equal(f, firsts) and np.array_equal(o, off) and np.array_equal(x, nodes)
    assert [bytes(ids[j]) for j in h] == [bytes(r) for r in nodes]
    assert np.diff(off).max() <= 8
    assert m.stat() == (firsts.shape[0], nodes.shape[0], firsts.shape[0] - 1)
    return firsts.shape[0], nodes.shape[0]


@pytest.mark.parametrize("client", [0, 1])
@pytest.mark.parametrize("n", C.SIZES)
def test_model_equals_oracle_on_uniform_ids(client, n):
    shapes = [model_equals_oracle(*C.uniform(seed, n), client) for seed in C.SEEDS]
    nbs, nns = C.SHAPES[(client, n)]
    assert tuple(s[0] for s in shapes) == nbs and tuple(s[1] for s in shapes) == nns


def test_the_client_runs_cross_a_round_of_find_bucket():
    assert all(nb > 64 for nb in C.SHAPES[(1, 2000)][0])


@pytest.mark.parametrize("client", [0, 1])
@pytest.mark.parametrize("shuffle", [False, True])
def test_model_equals_oracle_on_the_deep_chain(client, shuffle):
    myid, ids = C.deep_chain(shuffle=shuffle)
    if client:
        ids = np.concatenate([ids, O.gen_ids(1, 2000)])
    nb, nn = model_equals_oracle(myid, ids, client)
    assert nb > 128


# ---- the model's state rules, on rows small enough to check by eye ---------------------------------
def test_model_state_rules():
    myid = bytes([0x80] + [0] * 19)
    far = [bytes([i + 1] + [0] * 19) for i in range(9)]          # the other side of bit 0
    m = C.Model(myid)
    for h in range(8):
        assert m.on_new_node(far[h], h, C.EXPIRED if h in (6, 2) else C.GOOD) == (C.RTG_PLACED, C.NONE)
    assert m.buckets == [[7, 6, 5, 4, 3, 2, 1, 0]]
    assert m.on_new_node(far[8], 8) == (C.RTG_REPLACED, 6) and m.buckets == [[7, 8, 5, 4, 3, 2, 1, 0]]
    assert m.on_new_node(far[6], 9, 0) == (C.RTG_REPLACED, 2) and m.buckets == [[7, 8, 5, 4, 3, 9, 1, 0]]
    assert 6 not in m.ids and 2 not in m.state
    assert m.on_new_node(far[6], 9) == (C.RTG_KNOWN, C.NONE)
    # node 9 is not good, but the table has one bucket: the split goes ahead, and reverses the row
    assert m.on_new_node(bytes([0xC0] + [0] * 19), 10) == (C.RTG_PLACED, C.NONE)
    assert m.firsts == [bytes(20), myid] and m.buckets == [[0, 1, 9, 3, 4, 5, 8, 7], [10]]
    # a full bucket that is not mine: FULL, the ping pick is the first not-good node without a pending message
    assert m.on_new_node(far[2], 11) == (C.RTG_FULL, 9)
    m.update_state([9, 3], [C.PENDING, 0])
    assert m.on_new_node(far[2], 11) == (C.RTG_FULL, 3)
    m.update_state([3], [C.PENDING])
    assert m.on_new_node(far[2], 11) == (C.RTG_FULL, C.NONE)
    m.update_state([4], [C.EXPIRED])
    assert m.expire() == [4] and m.buckets[0] == [0, 1, 9, 3, 5, 8, 7] and m.stat() == (2, 8, 1)
    # dubious blocks the split of my bucket once there are two buckets
    mine = [bytes([0x80 | (0x40 >> k)] + [h] + [0] * 18) for k, h in zip((0, 0, 0, 1, 1, 2, 2), range(20, 27))]
    for h, x in zip(range(20, 27), mine):
        assert m.on_new_node(x, h, C.GOOD if h != 23 else 0) == (C.RTG_PLACED, C.NONE)
    assert len(m.buckets[1]) == 8
    assert m.on_new_node(bytes([0x81] + [0] * 19), 30) == (C.RTG_FULL, 23) and m.stat()[0] == 2
    m.update_good([23], [1])
    assert m.on_new_node(bytes([0x81] + [0] * 19), 30) == (C.RTG_PLACED, C.NONE) and m.stat()[0] > 2


def test_model_stops_at_256_buckets():
    firsts = np.zeros((256, 20), np.uint8)
    firsts[:, 0] = np.arange(256)
    myid = np.array([77] + [1] * 19, np.uint8)
    nodes = np.zeros((8, 20), np.uint8)
    nodes[:, 0] = 77
    nodes[:, 1] = np.arange(8)
    off = np.zeros(257, np.uint32)
    off[78:] = 8
    m = C.Model.from_table(myid, firsts, off, nodes)
    x = np.zeros((3, 20), np.uint8)
    x[:, 0] = (5, 77, 6)
    x[:, 2] = 9
    res, aux = m.batch(x, [100, 101, 102])
    assert res.tolist() == [C.RTG_PLACED, C.RTG_UNAPPLIED, C.RTG_UNAPPLIED] and m.stat() == (256, 9, 0)


# ---- the kernels' budget --------------------------------------------------------------------------
LDS_MAX = 160 * 1024           # one gfx950 workgroup; the table kernels hold 100,416 B


@pytest.mark.skipif(KB.HIPCC is None, reason="hipcc not installed")
def test_rtgrow_kernels_lds():
    """(registers and scratch: tests/test_kernel_resources.py)"""
    usage = KB.usage("rtgrow")
    for k, v in usage.items():
        assert v["LDS"] <= LDS_MAX, f"{k}: {v['LDS']} B of LDS"
    assert max(v["LDS"] for v in usage.values()) > 64 * 1024   # the table kernels' LDS is static: the remark counts it


# ---- the C++ adapter --------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rtgrow_check(tmp_path_factory):
    """tests/cpp/rtgrow_check.cpp built as C++11 with -Wall -Wextra -Werror against the mock table shape"""
    return cpp_check.build("rtgrow", tmp_path_factory.mktemp("rtgrow"))


def test_adapter_compiles_as_cxx11(rtgrow_check):
    assert subprocess.check_output([rtgrow_check], text=True).strip() == "built"


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_adapter_host_table_agrees_with_the_model(rtgrow_check, tmp_path, seed):
    """The mock table that stands for the caller's own in the adapter check (onNewNode, split,
    expireBuckets written after the reference in C++) gives the model's results and the model's
    table on a random walk: what the device is compared with in --run is the model's behaviour."""
    myid, ops = C.random_walk(seed, steps=40)
    client = seed % 2
    m = C.Model(myid, client)
    blob = [np.uint32(client).tobytes(), bytes(myid)]
    want, nops = [], 0
    for op in ops:
        if op[0] == "new":
            res, aux = m.batch(op[1], op[2], op[3])
            for j in range(len(res)):
                blob.append(b"\0" + bytes(op[1][j]) + np.uint32(op[2][j]).tobytes() + bytes([op[3][j]]))
                want.append(f"new {res[j]} {-1 if aux[j] == C.NONE else aux[j]}")
                nops += 1
        elif op[0] == "expire":
            m.expire()
            blob.append(b"\1")
            want.append("expire")
            nops += 1
        elif op[0] == "update":
            m.update_state(op[1], op[2])
            for h, v in zip(op[1], op[2]):
                blob.append(b"\2" + np.uint32(h).tobytes() + bytes([v]))
                nops += 1
    blob.insert(2, np.uint32(nops).tobytes())
    for first, row in zip(m.firsts, m.buckets):
        want.append(" ".join([first.hex()] + [f"{h}:{m.state[h]}" for h in row]))
    path = str(tmp_path / "ops.bin")
    open(path, "wb").write(b"".join(blob))
    out = subprocess.run([rtgrow_check, "--host", path], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert out.stdout.split("\n")[:-1] == want
