"""GPU parity of the resident routing table (dhtgpu_rt_*, opendht_amd/csrc/rtable.hip): the
wave-per-target findClosestNodes, the fused find_node reply and the closeness test against the CPU
oracle (O.find_closest_batch, O.buffer_nodes, O.xor_cmp) and against the snapshot entry points they
sit beside.  Every comparison is exact.  Marked gpu: run on the MI355X box."""
import numpy as np
import pytest

import oracle as O
import rtable_cases as RC

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
EINVAL, ENOIDS = -1, -4


@pytest.fixture(scope="module")
def ctx():
    import opendht_amd
    c = opendht_amd.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def grown():
    return {cluster: RC.grown(cluster) for cluster in (False, True)}


def assert_rows(got, cnt, want, wcnt, what):
    assert np.array_equal(cnt, wcnt), what
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, f"{what}: {bad.size} rows differ, first {bad[:5]}: got {got[bad[0]]} want {want[bad[0]]}"


def load(ctx, c, myid=None, tail=None, af=0, version=0):
    ctx.rt_set(np.zeros(20, np.uint8) if myid is None else myid, c["firsts"], c["off"], c["nodes"], tail, af, version)
    ctx.rt_set_good(c["good"])


def device_targets(tg, stride=None):
    """targets as device word planes of the given stride (torch tensor, stride)"""
    import opendht_amd
    import torch
    q = tg.shape[0]
    stride = stride or q
    planes = np.zeros((5, stride), np.uint32)
    planes[:, :q] = opendht_amd.id_words(tg)
    return torch.from_numpy(planes.view(np.int32).reshape(-1)).to(torch.device("cuda", 0)), stride


# ---- findClosestNodes ------------------------------------------------------------------------
def test_calls_before_rt_set():
    import opendht_amd
    with opendht_amd.Context(0) as c:
        tg = O.gen_ids(1, 2)
        for fn in (lambda: c.rt_find_closest(tg, 8), lambda: c.rt_reply(tg), lambda: c.rt_closer(tg),
                   lambda: c.rt_set_good(np.ones(3, np.uint8)), lambda: c.rt_update_good([0], 1)):
            with pytest.raises(opendht_amd.DhtGpuError) as e:
                fn()
            assert e.value.code == ENOIDS


@pytest.mark.parametrize("cluster", [False, True])
def test_grown_tables_vs_oracle_and_snapshot_form(ctx, grown, cluster):
    myid, firsts, off, nodes, tg = grown[cluster]
    ctx.rt_set(myid, firsts, off, nodes, version=0)
    for fr in RC.FRACTIONS:
        good = RC.good_mask(nodes.shape[0], fr)
        ctx.rt_set_good(good)
        for count in RC.COUNTS:
            want, wcnt = O.find_closest_batch(firsts, off, nodes, good, tg, count, threads=8)
            got, cnt = ctx.rt_find_closest(tg, count)
            assert_rows(got, cnt, want, wcnt, (cluster, fr, count))
            old, ocnt = ctx.find_closest(firsts, off, nodes, good, tg, count)
            assert_rows(got, cnt, old, ocnt, ("find_closest", cluster, fr, count))


@pytest.mark.parametrize("c", RC.synthetic() + RC.ties(), ids=lambda c: c["name"])
def test_synthetic_tables_and_ties(ctx, c):
    load(ctx, c)
    for count in c["counts"]:
        want, wcnt = RC.expected(c, count)
        got, cnt = ctx.rt_find_closest(c["targets"], count)
        assert_rows(got, cnt, want, wcnt, (c["name"], count))


def test_error_arguments(ctx, grown):
    import opendht_amd
    myid, firsts, off, nodes, tg = grown[False]
    ctx.rt_set(myid, firsts, off, nodes)
    L, h = opendht_amd.lib(), ctx._h
    t = np.ascontiguousarray(tg[:4])
    idx, cnt = np.zeros((4, 40), np.uint32), np.zeros(4, np.uint32)
    tp, ip, cp = (opendht_amd._p(t, opendht_amd._u8p), opendht_amd._p(idx, opendht_amd._u32p),
                  opendht_amd._p(cnt, opendht_amd._u32p))
    assert L.dhtgpu_rt_find_closest(h, tp, 4, 0, ip, cp) == EINVAL
    assert L.dhtgpu_rt_find_closest(h, tp, 4, 33, ip, cp) == EINVAL
    assert L.dhtgpu_rt_find_closest(h, None, 4, 8, ip, cp) == EINVAL
    assert L.dhtgpu_rt_find_closest(h, tp, 4, 8, None, cp) == EINVAL
    assert L.dhtgpu_rt_find_closest(h, None, 0, 8, None, None) == 0   # q == 0: no work
    assert L.dhtgpu_rt_closer(h, tp, 4, 33, 1, opendht_amd._p(t, opendht_amd._u8p), None) == EINVAL
    nn = nodes.shape[0]
    with pytest.raises(opendht_amd.DhtGpuError) as e:   # nothing applied
        ctx.rt_update_good([0, nn], [0, 0])
    assert e.value.code == EINVAL
    got, _ = ctx.rt_find_closest(tg, 8)
    want, _ = O.find_closest_batch(firsts, off, nodes, np.ones(nn, np.uint8), tg, 8)
    assert np.array_equal(got, want)
    bad_off = off.copy()
    bad_off[1] = bad_off[2] + 1
    with pytest.raises(opendht_amd.DhtGpuError):
        ctx.rt_set(myid, firsts, bad_off, nodes)


def test_empty_tables(ctx):
    tg = O.gen_ids(5, 5)
    ctx.rt_set(tg[0], np.zeros((0, 20), np.uint8), np.zeros(1, np.uint32), np.zeros((0, 20), np.uint8),
               np.zeros((0, 6), np.uint8), 4)
    idx, cnt = ctx.rt_find_closest(tg, 8)
    assert np.all(cnt == 0) and np.all(idx == NONE)
    out, ln = ctx.rt_reply(tg)
    assert np.all(ln == 0)
    flag, cnt = ctx.rt_closer(tg, 8, 1)
    assert np.all(flag == 0) and np.all(cnt == 0)
    # buckets without nodes
    firsts = np.zeros((2, 20), np.uint8)
    firsts[1, 0] = 0x80
    ctx.rt_set(tg[0], firsts, np.zeros(3, np.uint32), np.zeros((0, 20), np.uint8))
    idx, cnt = ctx.rt_find_closest(tg, 32)
    assert np.all(cnt == 0) and np.all(idx == NONE)


@pytest.mark.parametrize("q,pad", [(1, 0), (3, 0), (4, 0), (5, 0), (257, 0), (257, 6)])
def test_batch_shapes_dev_form(ctx, grown, q, pad):
    """one to 257 targets (four per workgroup), an odd target stride above q"""
    import torch
    myid, firsts, off, nodes, _ = grown[True]
    good = RC.good_mask(nodes.shape[0], 0.7)
    ctx.rt_set(myid, firsts, off, nodes)
    ctx.rt_set_good(good)
    tg = O.gen_ids(900 + q, q)
    tp, ts = device_targets(tg, q + pad)
    assert pad == 0 or ts % 2 == 1
    dev = torch.device("cuda", 0)
    for count in (8, 14):
        o_idx = torch.full((q + 1, count), 0x5A5A5A5A, dtype=torch.int32, device=dev)   # a guard row behind
        o_cnt = torch.full((q + 1,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
        ctx.rt_find_closest_dev(tp.data_ptr(), ts, q, count, o_idx.data_ptr(), o_cnt.data_ptr(), ctx.stream)
        torch.cuda.synchronize()
        want, wcnt = O.find_closest_batch(firsts, off, nodes, good, tg, count)
        got, cnt = o_idx.cpu().numpy().view(np.uint32), o_cnt.cpu().numpy().view(np.uint32)
        assert_rows(got[:q], cnt[:q], want, wcnt, (q, pad, count))
        assert np.all(got[q] == 0x5A5A5A5A) and cnt[q] == 0x5A5A5A5A


# ---- replies -----------------------------------------------------------------------------------
@pytest.mark.parametrize("af", [4, 6])
def test_reply_vs_oracle_and_the_two_call_form(ctx, grown, af):
    myid, firsts, off, nodes, tg = grown[False]
    nn, alen = nodes.shape[0], 4 if af == 4 else 16
    rec = 20 + alen + 2
    tail = O.special_addrs(np.random.default_rng(af), nn, af)
    ctx.rt_set(myid, firsts, off, nodes, tail, af)
    masks = [RC.good_mask(nn, fr) for fr in (1.0, 0.4, 0.0)]
    few = np.zeros(nn, np.uint8)
    few[[3, nn // 2, nn - 1]] = 1   # rows of three nodes
    for good in masks + [few]:
        ctx.rt_set_good(good)
        out, ln, idx = ctx.rt_reply(tg, indices=True)
        want_idx, wcnt = O.find_closest_batch(firsts, off, nodes, good, tg, 8)
        assert np.array_equal(idx, want_idx)
        assert np.array_equal(ln, wcnt * rec)
        old_idx, _ = ctx.find_closest(firsts, off, nodes, good, tg, 8)
        old, oln = ctx.buffer_nodes_ids(nodes, tail, af, tg, old_idx)
        assert np.array_equal(ln, oln)
        for qi in range(tg.shape[0]):
            want = O.buffer_nodes(nodes, tail, alen, tg[qi], want_idx[qi, : wcnt[qi]])
            assert ln[qi] == want.shape[0], qi
            assert np.array_equal(out[qi, : ln[qi]], want), qi
            assert np.array_equal(out[qi, : ln[qi]], old[qi, : ln[qi]]), qi
        out2, ln2 = ctx.rt_reply(tg)   # without the indices
        assert np.array_equal(ln2, ln) and all(np.array_equal(out2[i, : ln[i]], out[i, : ln[i]]) for i in range(len(ln)))


def test_reply_needs_tails(ctx, grown):
    import opendht_amd
    myid, firsts, off, nodes, tg = grown[False]
    ctx.rt_set(myid, firsts, off, nodes)
    with pytest.raises(opendht_amd.DhtGpuError) as e:
        ctx.rt_reply(tg[:3])
    assert e.value.code == EINVAL


# ---- closeness ---------------------------------------------------------------------------------
def closer_expected(myid, firsts, off, nodes, good, tg, count, min_nodes):
    flags = np.zeros(tg.shape[0], np.uint8)
    sizes = np.zeros(tg.shape[0], np.uint32)
    for qi in range(tg.shape[0]):
        r = O.find_closest(firsts, off, nodes, good, tg[qi], count)
        sizes[qi] = len(r)
        flags[qi] = len(r) >= max(min_nodes, 1) and O.xor_cmp(tg[qi], nodes[r[-1]], myid) < 0
    return flags, sizes


@pytest.mark.parametrize("cluster", [False, True])
def test_closer_vs_oracle(ctx, grown, cluster):
    myid, firsts, off, nodes, tg = grown[cluster]
    nn = nodes.shape[0]
    near = np.repeat(myid[None, :], 48, axis=0)   # targets next to myid: one bit flipped, from the last bit up
    for i in range(1, 48):
        near[i, 19 - (i * 3) // 8 % 20] ^= 1 << (i % 8)
    tg = np.concatenate([tg[:120], near, nodes[:8]])
    rng = np.random.default_rng(12)
    masks = {"all": np.ones(nn, np.uint8), "70": RC.good_mask(nn, 0.7), "none": np.zeros(nn, np.uint8)}
    for g in (7, 8, 13, 14):
        m = np.zeros(nn, np.uint8)
        m[rng.choice(nn, g, replace=False)] = 1
        masks[f"{g}_good"] = m
    ctx.rt_set(myid, firsts, off, nodes)
    seen = set()
    for name, good in masks.items():
        ctx.rt_set_good(good)
        for count, min_nodes in ((8, 1), (14, 8)):
            flag, cnt = ctx.rt_closer(tg, count, min_nodes)
            want, sizes = closer_expected(myid, firsts, off, nodes, good, tg, count, min_nodes)
            assert np.array_equal(cnt, sizes), (name, count)
            assert np.array_equal(flag, want), (name, count, np.flatnonzero(flag != want)[:5])
            seen.update(want.tolist())
    assert seen == {0, 1}


def test_closer_last_node_is_myid(ctx):
    """a table whose nodes include myid: for the target myid at count 1 the last (only) result is
    myid itself, xorCmp is 0 and the flag is 0; min_nodes = 0 counts as 1"""
    c = [x for x in RC.synthetic() if x["name"] == "two_buckets"][0]   # 70 % good
    myid = c["nodes"][np.flatnonzero(c["good"])[5]]
    load(ctx, c, myid=myid)
    tg = np.concatenate([myid[None, :], c["targets"]])
    for count, min_nodes in ((1, 1), (1, 0), (8, 1), (14, 8)):
        flag, cnt = ctx.rt_closer(tg, count, min_nodes)
        want, sizes = closer_expected(myid, c["firsts"], c["off"], c["nodes"], c["good"], tg, count, min_nodes)
        assert np.array_equal(flag, want) and np.array_equal(cnt, sizes), (count, min_nodes)
    assert ctx.rt_closer(tg[:1], 1, 1)[0][0] == 0


# ---- state -------------------------------------------------------------------------------------
def test_update_good_then_query(ctx, grown):
    myid, firsts, off, nodes, tg = grown[False]
    nn = nodes.shape[0]
    ctx.rt_set(myid, firsts, off, nodes)
    good = np.ones(nn, np.uint8)
    rng = np.random.default_rng(3)
    for step in range(3):
        idx = rng.choice(nn, 25, replace=False).astype(np.uint32)
        val = rng.integers(0, 2, 25).astype(np.uint8)
        good[idx] = val
        ctx.rt_update_good(idx, val)
        want, wcnt = O.find_closest_batch(firsts, off, nodes, good, tg, 8)
        got, cnt = ctx.rt_find_closest(tg, 8)
        assert_rows(got, cnt, want, wcnt, step)
    ctx.rt_update_good(np.arange(nn, dtype=np.uint32), 0)
    assert np.all(ctx.rt_find_closest(tg, 8)[1] == 0)


@pytest.mark.parametrize("m", [257, 65537])
def test_update_good_many(ctx, m):
    """m distinct nodes with random values in one call, on a table of 66,000 nodes in 256 buckets
    (more than one block of the setter, and 256 blocks and one thread more): every node's byte -- a
    node is the closest good node to its own id exactly when it is good -- against the oracle"""
    ids = RC.sorted_ids(4300, 66000)
    nn = ids.shape[0]
    firsts, off = RC.cut(ids, RC.sizes_for(256, nn, 11))
    rng = np.random.default_rng(m)
    good = RC.good_mask(nn, 0.5, m)
    ctx.rt_set(np.zeros(20, np.uint8), firsts, off, ids)
    ctx.rt_set_good(good)
    idx = rng.choice(nn, m, replace=False).astype(np.uint32)
    val = rng.choice([0, 1, 2, 255], m).astype(np.uint8)   # any nonzero byte is good
    ctx.rt_update_good(idx, val)
    good[idx] = val != 0
    want, wcnt = O.find_closest_batch(firsts, off, ids, good, ids, 1, threads=16)
    got, cnt = ctx.rt_find_closest(ids, 1)
    assert_rows(got, cnt, want, wcnt, m)
    assert np.array_equal(got[:, 0] == np.arange(nn, dtype=np.uint32), good != 0)


def test_version_skips_and_reuploads(ctx, grown):
    myid, firsts, off, nodes, tg = grown[False]
    nn = nodes.shape[0]
    want, wcnt = O.find_closest_batch(firsts, off, nodes, np.ones(nn, np.uint8), tg, 8)
    ctx.rt_set(myid, firsts, off, nodes, version=41)
    other = np.ascontiguousarray(nodes[::-1] ^ 0x5A)   # the caller's arrays, scribbled on
    ctx.rt_set(myid, firsts, off, other, version=41)
    got, cnt = ctx.rt_find_closest(tg, 8)
    assert_rows(got, cnt, want, wcnt, "same version: the first upload answers")
    # a changed version uploads: the same buckets with the nodes of each bucket reversed
    rev = nodes.copy()
    for b in range(firsts.shape[0]):
        rev[off[b]: off[b + 1]] = nodes[off[b]: off[b + 1]][::-1]
    ctx.rt_set(myid, firsts, off, rev, version=42)
    want2, wcnt2 = O.find_closest_batch(firsts, off, rev, np.ones(nn, np.uint8), tg, 8)
    got, cnt = ctx.rt_find_closest(tg, 8)
    assert_rows(got, cnt, want2, wcnt2, "new version")
    assert not np.array_equal(want, want2)


def test_rt_and_id_set_are_independent(ctx, grown):
    myid, firsts, off, nodes, tg = grown[True]
    ids = O.gen_ids(31, 5000)
    ctx.set_ids(ids)
    before = ctx.topk(tg[:50], 8)
    ctx.rt_set(myid, firsts, off, nodes)
    rt_before = ctx.rt_find_closest(tg, 14)
    after = ctx.topk(tg[:50], 8)
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    want, _ = O.topk(ids, tg[:50], 8)
    assert np.array_equal(after[0], want)
    ctx.set_ids(O.gen_ids(32, 3000))
    rt_after = ctx.rt_find_closest(tg, 14)
    assert np.array_equal(rt_before[0], rt_after[0]) and np.array_equal(rt_before[1], rt_after[1])


def test_two_dev_batches_on_a_side_stream(ctx, grown):
    """indices, then the reply and the closeness flags of a second batch, back to back on a
    non-default stream with one synchronise at the end"""
    import torch
    myid, firsts, off, nodes, tg = grown[False]
    nn = nodes.shape[0]
    tail = O.special_addrs(np.random.default_rng(8), nn, 4)
    good = RC.good_mask(nn, 0.7)
    ctx.rt_set(myid, firsts, off, nodes, tail, 4)
    ctx.rt_set_good(good)
    torch.cuda.synchronize()   # (the setters ran on the context's stream)
    dev = torch.device("cuda", 0)
    a, b = tg[:150], tg[150:]
    ta, sa = device_targets(a)
    tb_, sb = device_targets(b, b.shape[0] + 3)
    ia = torch.empty((a.shape[0], 14), dtype=torch.int32, device=dev)
    ca = torch.empty(a.shape[0], dtype=torch.int32, device=dev)
    ob = torch.zeros((b.shape[0], 8 * 26), dtype=torch.uint8, device=dev)
    lb = torch.empty(b.shape[0], dtype=torch.int32, device=dev)
    fb = torch.empty(b.shape[0], dtype=torch.uint8, device=dev)
    side = torch.cuda.Stream(device=dev)
    s = side.cuda_stream
    ctx.rt_find_closest_dev(ta.data_ptr(), sa, a.shape[0], 14, ia.data_ptr(), ca.data_ptr(), s)
    ctx.rt_reply_dev(tb_.data_ptr(), sb, b.shape[0], ob.data_ptr(), lb.data_ptr(), None, s)
    ctx.rt_closer_dev(tb_.data_ptr(), sb, b.shape[0], 8, 1, fb.data_ptr(), None, s)
    side.synchronize()
    want, wcnt = O.find_closest_batch(firsts, off, nodes, good, a, 14)
    assert_rows(ia.cpu().numpy().view(np.uint32), ca.cpu().numpy().view(np.uint32), want, wcnt, "batch a")
    wb, wbc = O.find_closest_batch(firsts, off, nodes, good, b, 8)
    out, ln = ob.cpu().numpy(), lb.cpu().numpy().view(np.uint32)
    assert np.array_equal(ln, wbc * 26)
    for qi in range(b.shape[0]):
        assert np.array_equal(out[qi, : ln[qi]], O.buffer_nodes(nodes, tail, 4, b[qi], wb[qi, : wbc[qi]])), qi
    wf, _ = closer_expected(myid, firsts, off, nodes, good, b, 8, 1)
    assert np.array_equal(fb.cpu().numpy(), wf)


def test_cpp_adapter_resident_table(tmp_path):
    """dhtgpu::ResidentTable's device paths against its host paths and the oracle (tests/cpp/rtable_check.cpp)"""
    import cpp_check
    cpp_check.run(cpp_check.build("rtable", tmp_path), ["--run"], "rtable_check", 120)
