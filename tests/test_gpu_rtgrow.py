"""GPU parity of the growing resident routing table (dhtgpu_rtg_*, opendht_amd/csrc/rtgrow.hip):
batched onNewNode with splits against the oracle's table, the state regimes and expireBuckets
against the Python model of tests/rtgrow_cases.py (pinned to the oracle in
tests/test_rtgrow_cpu.py), and the K1w queries over the grown table against the oracle over its
export.  Every comparison is exact.  Marked gpu: run on the MI355X box."""
import ctypes
import functools

import numpy as np
import pytest

import oracle as O
import rtgrow_cases as C

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
EINVAL, ENOIDS, ERANGE = -1, -4, -6
COUNTS = (1, 8, 14, 32)


@pytest.fixture(scope="module")
def ctx():
    import opendht_amd
    c = opendht_amd.Context(0)
    yield c
    c.close()


def one_bucket(ctx, myid, af=0):
    """the Dht constructor's table: one bucket, first = 0, no node"""
    alen = {0: 0, 4: 4, 6: 16}[af]
    ctx.rt_set(myid, np.zeros((1, 20), np.uint8), [0, 0], np.zeros((0, 20), np.uint8),
               np.zeros((0, alen + 2), np.uint8) if af else None, af)


def same_table(ctx, m, what, alen=0):
    """the device's export and sizes equal the model's"""
    got, want = ctx.rtg_export(), m.export()
    for g, w, name in zip(got, want, ("firsts", "off", "ids", "handles", "state")):
        assert np.array_equal(g, w), (what, name)
    assert ctx.rtg_size() == m.stat()[:2], what
    return want


@functools.lru_cache(maxsize=None)
def oracle_case(kind, client, n, seed):
    if kind == "uniform":
        myid, ids = C.uniform(seed, n)
    else:
        myid, ids = C.deep_chain(shuffle=kind == "deep_shuffled")
        if client:
            ids = np.concatenate([ids, O.gen_ids(1, 2000)])
    res, (firsts, off, nodes) = C.oracle_run(myid, ids, client)
    return myid, ids, res, firsts, off, nodes


def grow_and_compare(ctx, case, client, batch):
    myid, ids, res, firsts, off, nodes = case
    n = ids.shape[0]
    one_bucket(ctx, myid)
    handles = np.arange(n, dtype=np.uint32)
    got, stat = [], None
    for lo in range(0, n, batch):
        r, aux, stat = ctx.rtg_on_new_node(ids[lo: lo + batch], handles[lo: lo + batch], client=client)
        assert np.all(aux == NONE)       # every node is good: nothing to evict, nobody to ping
        got.append(r)
    got = np.concatenate(got)
    assert set(got.tolist()) <= {C.RTG_PLACED, C.RTG_FULL}   # distinct ids and handles: never KNOWN
    assert np.array_equal((got == C.RTG_PLACED).astype(np.uint8), res), np.flatnonzero((got == C.RTG_PLACED) != res)[:5]
    assert stat.tolist() == [firsts.shape[0], nodes.shape[0], firsts.shape[0] - 1]
    f, o, x, h, st = ctx.rtg_export()
    assert np.array_equal(f, firsts) and np.array_equal(o, off) and np.array_equal(x, nodes)
    # the handles in that order: the oracle numbers its nodes by insertion, as the batch does
    placed = handles[res == 1]
    by_id = {bytes(ids[j]): j for j in placed}
    assert np.array_equal(h, np.array([by_id[bytes(r)] for r in nodes], np.uint32))
    assert np.all(st == C.GOOD)


# ---- growth from the one-bucket table against the oracle ----------------------------------------
@pytest.mark.parametrize("client", [0, 1])
@pytest.mark.parametrize("n", C.SIZES)
@pytest.mark.parametrize("seed", C.SEEDS)
def test_growth_vs_oracle(ctx, client, n, seed):
    case = oracle_case("uniform", client, n, seed)
    for batch in (1, 7, 64, n):
        grow_and_compare(ctx, case, client, batch)


@pytest.mark.parametrize("client", [0, 1])
@pytest.mark.parametrize("kind", ["deep", "deep_shuffled"])
def test_deep_chain_vs_oracle(ctx, client, kind):
    """more than 128 buckets: findBucket rounds 3+, a directory shift over more than two wave-widths"""
    case = oracle_case(kind, client, 0, 0)
    assert case[3].shape[0] > 128
    for batch in (64, case[1].shape[0]):
        grow_and_compare(ctx, case, client, batch)


# ---- the state regimes against the model --------------------------------------------------------
def near(myid, d, rng):
    """an id that shares its first d bits with myid and differs at bit d"""
    my = int.from_bytes(bytes(myid), "big")
    r = int.from_bytes(bytes(rng.integers(0, 256, 20, dtype=np.uint8)), "big")
    keep = ((1 << 160) - 1) ^ ((1 << (160 - d)) - 1)
    x = (my & keep) | ((~my) & (1 << (159 - d))) | (r & ((1 << (159 - d)) - 1))
    return np.frombuffer(x.to_bytes(20, "big"), np.uint8)


def new(ctx, m, ids, handles, state=None, tails=None, what=""):
    """one batch on both sides; returns the (agreed) results and aux"""
    ids = np.ascontiguousarray(ids, np.uint8).reshape(-1, 20)
    handles = np.asarray(handles, np.uint32)
    want, waux = m.batch(ids, handles, state, tails)
    res, aux, stat = ctx.rtg_on_new_node(ids, handles, state, tails, client=m.client)
    assert np.array_equal(res, want), (what, res, want)
    assert np.array_equal(aux, waux), (what, aux, waux)
    assert tuple(stat.tolist()) == m.stat(), what
    return res, aux


def test_replace_takes_the_first_expired_in_list_order(ctx):
    rng = np.random.default_rng(3)
    myid = rng.integers(0, 256, 20, dtype=np.uint8)
    one_bucket(ctx, myid)
    m = C.Model(myid)
    ids = rng.integers(0, 256, (8, 20), dtype=np.uint8)
    st = np.full(8, C.GOOD, np.uint8)
    st[7] = C.EXPIRED                                   # inserted last: the list's front
    new(ctx, m, ids, np.arange(8), st)
    res, aux = new(ctx, m, rng.integers(0, 256, (1, 20), dtype=np.uint8), [8])
    assert (res[0], aux[0]) == (C.RTG_REPLACED, 7) and m.buckets[0][0] == 8
    for h, v in ((3, C.EXPIRED), (0, C.EXPIRED | C.PENDING)):   # the middle, then the back
        ctx.rtg_update_state([h], v)
        m.update_state([h], [v])
    res, aux = new(ctx, m, rng.integers(0, 256, (2, 20), dtype=np.uint8), [9, 10])
    assert res.tolist() == [C.RTG_REPLACED] * 2 and aux.tolist() == [3, 0]
    assert m.buckets[0][4] == 9 and m.buckets[0][7] == 10
    same_table(ctx, m, "replaced in place")


def test_replace_after_a_split_reversed_the_row(ctx):
    rng = np.random.default_rng(4)
    myid = rng.integers(0, 256, 20, dtype=np.uint8)
    one_bucket(ctx, myid)
    m = C.Model(myid)
    far = [near(myid, 0, rng) for _ in range(8)]         # all on the other side of bit 0
    new(ctx, m, far, np.arange(8))
    res, _ = new(ctx, m, [near(myid, 1, rng)], [8])       # my bucket is the one bucket: split, placed
    assert res[0] == C.RTG_PLACED and m.stat()[0] == 2
    b = m.find_bucket(bytes(far[0]))
    assert m.buckets[b] == list(range(8))                # the split reversed the row: 0 is now its front
    for h in (0, 7, 4):                                  # front, back, middle of the reversed row
        ctx.rtg_update_state([h], C.EXPIRED)
        m.update_state([h], [C.EXPIRED])
    res, aux = new(ctx, m, [near(myid, 0, rng) for _ in range(3)], [20, 21, 22])
    assert res.tolist() == [C.RTG_REPLACED] * 3 and aux.tolist() == [0, 4, 7]
    same_table(ctx, m, "replaced after a split")


def test_dubious_blocks_the_split_and_the_ping_pick(ctx):
    rng = np.random.default_rng(5)
    myid = rng.integers(0, 256, 20, dtype=np.uint8)
    # one bucket: a not-good node does not block the split (nb == 1 overrides dubious)
    one_bucket(ctx, myid)
    m = C.Model(myid)
    st = np.full(8, C.GOOD, np.uint8)
    st[2] = 0
    new(ctx, m, [near(myid, 0, rng) for _ in range(4)] + [near(myid, 1, rng) for _ in range(4)], np.arange(8), st)
    res, _ = new(ctx, m, [near(myid, 2, rng)], [8])
    assert res[0] == C.RTG_PLACED and m.stat()[0] == 2
    # two buckets: my bucket full with one node not good -> no split, FULL, the ping pick reported
    mine = [near(myid, d, rng) for d in (2, 3, 4)]
    new(ctx, m, mine, [9, 10, 11])
    b = m.find_bucket(bytes(myid))
    assert len(m.buckets[b]) == 8 and m.contains(b, bytes(myid))
    row = list(m.buckets[b])
    ctx.rtg_update_state([row[5], row[2]], [0, 0])
    m.update_state([row[5], row[2]], [0, 0])
    res, aux = new(ctx, m, [near(myid, 5, rng)], [30])
    assert (res[0], aux[0]) == (C.RTG_FULL, row[2]) and m.stat()[0] == 2
    ctx.rtg_update_state([row[2]], C.PENDING)            # the pick skips a pending node
    m.update_state([row[2]], [C.PENDING])
    res, aux = new(ctx, m, [near(myid, 5, rng)], [30])
    assert (res[0], aux[0]) == (C.RTG_FULL, row[5])
    ctx.rtg_update_state([row[5]], C.PENDING)            # all of them pending: nobody to ping
    m.update_state([row[5]], [C.PENDING])
    res, aux = new(ctx, m, [near(myid, 5, rng)], [30])
    assert (res[0], aux[0]) == (C.RTG_FULL, NONE)
    good = np.ones(64, np.uint8)                         # set_state by handle: all good again -> the split goes ahead
    ctx.rtg_set_state(good)
    m.set_state(good)
    res, aux = new(ctx, m, [near(myid, 5, rng)], [30])
    assert res[0] == C.RTG_PLACED and m.stat()[0] > 2
    same_table(ctx, m, "split after set_state")


def test_same_handle_twice_in_a_batch(ctx):
    rng = np.random.default_rng(6)
    myid = rng.integers(0, 256, 20, dtype=np.uint8)
    one_bucket(ctx, myid)
    m = C.Model(myid)
    x = rng.integers(0, 256, (3, 20), dtype=np.uint8)
    res, _ = new(ctx, m, [x[0], x[1], x[0], x[2], x[1]], [0, 1, 0, 2, 1])
    assert res.tolist() == [C.RTG_PLACED, C.RTG_PLACED, C.RTG_KNOWN, C.RTG_PLACED, C.RTG_KNOWN]
    res, _ = new(ctx, m, [x[2]], [2])
    assert res[0] == C.RTG_KNOWN
    same_table(ctx, m, "known")


def test_expire_removes_every_expired_node(ctx):
    rng = np.random.default_rng(7)
    myid, ids = C.uniform(1, 300)
    one_bucket(ctx, myid)
    m = C.Model(myid, True)
    st = np.where(rng.random(300) < 0.3, C.EXPIRED, C.GOOD).astype(np.uint8)
    new(ctx, m, ids, np.arange(300), st)
    assert any(s & C.EXPIRED for s in m.state.values())
    gone = ctx.rtg_expire()
    assert sorted(gone.tolist()) == sorted(m.expire())
    f, off, x, h, s = same_table(ctx, m, "expired")
    assert not np.any(s & C.EXPIRED)
    assert ctx.rtg_expire().size == 0                    # nothing left to remove
    same_table(ctx, m, "expired twice")


def apply(ctx, m, op, what):
    if op[0] == "new":
        new(ctx, m, op[1], op[2], op[3], op[4], what)
    elif op[0] == "expire":
        assert sorted(ctx.rtg_expire().tolist()) == sorted(m.expire()), what
    elif op[0] == "update":
        ctx.rtg_update_state(op[1], op[2])
        m.update_state(op[1], op[2])
    elif op[0] == "set":
        ctx.rtg_set_state(op[1])
        m.set_state(op[1])
    else:                                                # an expired node is never good
        val = np.array([v and not m.state.get(int(h), 0) & C.EXPIRED for h, v in zip(op[1], op[2])], np.uint8)
        ctx.rt_update_good(op[1], val)
        m.update_good(op[1], val)


@pytest.mark.parametrize("seed", range(12))
def test_random_walks_vs_model(ctx, seed):
    myid, ops = C.random_walk(seed)
    one_bucket(ctx, myid)
    m = C.Model(myid, client=seed % 2 == 1)
    for i, op in enumerate(ops):
        apply(ctx, m, op, (seed, i, op[0]))
        same_table(ctx, m, (seed, i, op[0]))


# ---- the K1w queries over a grown table -----------------------------------------------------------
def device_targets(tg):
    import opendht_amd
    import torch
    planes = np.ascontiguousarray(opendht_amd.id_words(tg), np.uint32)
    return torch.from_numpy(planes.view(np.int32).reshape(-1)).to(torch.device("cuda", 0)), tg.shape[0]


def check_queries(ctx, m, tg, alen, what, dev=False):
    firsts, off, ids, handles, state = m.export()
    good = (state & C.GOOD).astype(np.uint8)
    tails = m.tails(alen)
    rec = 20 + alen + 2
    q = tg.shape[0]

    def as_handles(idx):                                 # the oracle's positions -> the handles there
        if not len(handles):
            return idx
        return np.where(idx == NONE, NONE, handles[np.minimum(idx, len(handles) - 1)]).astype(np.uint32)

    want = {c: O.find_closest_batch(firsts, off, ids, good, tg, c) for c in COUNTS}
    for c in COUNTS:
        got, cnt = ctx.rt_find_closest(tg, c)
        assert np.array_equal(cnt, want[c][1]), (what, c)
        assert np.array_equal(got, as_handles(want[c][0])), (what, c)
    out, ln, idx = ctx.rt_reply(tg, indices=True)
    assert np.array_equal(idx, as_handles(want[8][0])) and np.array_equal(ln, want[8][1] * rec), what
    for qi in range(q):
        w = O.buffer_nodes(ids, tails, alen, tg[qi], want[8][0][qi, : want[8][1][qi]]) if len(ids) else np.zeros(0, np.uint8)
        assert np.array_equal(out[qi, : ln[qi]], w), (what, qi)
    for count, min_nodes in ((8, 1), (14, 8)):
        flag, cnt = ctx.rt_closer(tg, count, min_nodes)
        wi, wc = want[count]
        wf = np.array([wc[qi] >= min_nodes and O.xor_cmp(tg[qi], ids[wi[qi, wc[qi] - 1]], np.frombuffer(m.myid, np.uint8)) < 0
                       if wc[qi] else 0 for qi in range(q)], np.uint8)
        assert np.array_equal(cnt, wc) and np.array_equal(flag, wf), (what, count)
    if dev:
        import torch
        d = torch.device("cuda", 0)
        tp, ts = device_targets(tg)
        for c in (8, 32):
            o_idx = torch.full((q, c), 0x5A5A5A5A, dtype=torch.int32, device=d)
            o_cnt = torch.zeros(q, dtype=torch.int32, device=d)
            ctx.rt_find_closest_dev(tp.data_ptr(), ts, q, c, o_idx.data_ptr(), o_cnt.data_ptr(), ctx.stream)
            torch.cuda.synchronize()
            assert np.array_equal(o_idx.cpu().numpy().view(np.uint32), as_handles(want[c][0])), (what, c, "dev")
            assert np.array_equal(o_cnt.cpu().numpy().view(np.uint32), want[c][1]), (what, c, "dev")
        o_b = torch.zeros((q, 8 * rec), dtype=torch.uint8, device=d)
        o_l = torch.zeros(q, dtype=torch.int32, device=d)
        o_i = torch.zeros((q, 8), dtype=torch.int32, device=d)
        ctx.rt_reply_dev(tp.data_ptr(), ts, q, o_b.data_ptr(), o_l.data_ptr(), o_i.data_ptr(), ctx.stream)
        torch.cuda.synchronize()
        assert np.array_equal(o_i.cpu().numpy().view(np.uint32), idx), (what, "reply dev")
        lb, ob = o_l.cpu().numpy().view(np.uint32), o_b.cpu().numpy()
        assert np.array_equal(lb, ln) and all(np.array_equal(ob[i, : ln[i]], out[i, : ln[i]]) for i in range(q)), what


@pytest.mark.parametrize("af", [4, 6])
def test_queries_after_every_mutation_step(ctx, af):
    alen = 4 if af == 4 else 16
    myid, ops = C.random_walk(100 + af, steps=14, alen=alen)
    one_bucket(ctx, myid, af)
    m = C.Model(myid, client=True)
    tg = np.concatenate([O.gen_ids(40 + af, 20), myid[None, :], np.zeros((1, 20), np.uint8)])
    extra = C.uniform(3, 200)[1]
    tails = np.random.default_rng(af).integers(0, 256, (200, alen + 2), dtype=np.uint8)
    ops = [("new", extra, np.arange(5000, 5200, dtype=np.uint32), np.full(200, C.GOOD, np.uint8), tails)] + ops
    for i, op in enumerate(ops):
        apply(ctx, m, op, (af, i, op[0]))
        same_table(ctx, m, (af, i, op[0]))
        near_ids = m.export()[2][::17]
        check_queries(ctx, m, np.concatenate([tg, near_ids]) if len(near_ids) else tg, alen, (af, i, op[0]),
                      dev=i in (0, len(ops) - 1))
    # rt_update_good by handle
    f, off, ids, handles, state = m.export()
    live = handles[(state & C.EXPIRED) == 0]
    pick = live[:: max(1, live.size // 9)]
    val = (np.arange(pick.size) % 2).astype(np.uint8)
    ctx.rt_update_good(pick, val)
    m.update_good(pick, val)
    same_table(ctx, m, "update_good by handle")
    check_queries(ctx, m, tg, alen, "after update_good")


# ---- limits and errors ----------------------------------------------------------------------------
def test_errors_and_limits(ctx):
    import opendht_amd
    L = opendht_amd.lib()
    rng = np.random.default_rng(9)
    myid = rng.integers(0, 256, 20, dtype=np.uint8)
    ids = rng.integers(0, 256, (4, 20), dtype=np.uint8)
    with opendht_amd.Context(0) as c:                    # before rt_set
        for fn in (lambda: c.rtg_on_new_node(ids, [0, 1, 2, 3]), c.rtg_expire, c.rtg_size, c.rtg_export,
                   lambda: c.rtg_set_state(np.ones(4, np.uint8)), lambda: c.rtg_update_state([1], 1)):
            with pytest.raises(opendht_amd.DhtGpuError) as e:
                fn()
            assert e.value.code == ENOIDS
    # an uploaded bucket of 9 nodes
    nine = np.sort(rng.integers(0, 256, (9, 20), dtype=np.uint8), axis=0)
    ctx.rt_set(myid, np.zeros((1, 20), np.uint8), [0, 9], nine)
    for fn in (lambda: ctx.rtg_on_new_node(ids, [10, 11, 12, 13]), ctx.rtg_expire, lambda: ctx.rtg_update_state([1], 1)):
        with pytest.raises(opendht_amd.DhtGpuError) as e:
            fn()
        assert e.value.code == EINVAL
    assert np.array_equal(ctx.rt_find_closest(ids, 8)[0][:, :8], O.find_closest_batch(
        np.zeros((1, 20), np.uint8), np.array([0, 9], np.uint32), nine, np.ones(9, np.uint8), ids, 8)[0])
    # a handle at the bound: nothing applied
    one_bucket(ctx, myid)
    m = C.Model(myid)
    new(ctx, m, ids[:2], [5, 6])
    with pytest.raises(opendht_amd.DhtGpuError) as e:
        ctx.rtg_on_new_node(ids[2:], [7, opendht_amd.RTG_MAX_HANDLE])
    assert e.value.code == EINVAL
    with pytest.raises(opendht_amd.DhtGpuError) as e:
        ctx.rtg_update_state([opendht_amd.RTG_MAX_HANDLE], 1)
    assert e.value.code == EINVAL
    same_table(ctx, m, "bad handle")
    res, aux, stat = ctx.rtg_on_new_node(ids[:0], [])   # m == 0
    assert res.size == 0 and tuple(stat.tolist()) == m.stat()
    # a table set with tails needs the new nodes' tails
    one_bucket(ctx, myid, 4)
    with pytest.raises(opendht_amd.DhtGpuError) as e:
        ctx.rtg_on_new_node(ids, [0, 1, 2, 3])
    assert e.value.code == EINVAL
    # no bucket at all
    ctx.rt_set(myid, np.zeros((0, 20), np.uint8), [0], np.zeros((0, 20), np.uint8))
    res, aux, stat = ctx.rtg_on_new_node(ids, [0, 1, 2, 3])
    assert res.tolist() == [C.RTG_NONE] * 4 and stat.tolist() == [0, 0, 0] and ctx.rtg_export()[2].shape[0] == 0
    # rt_set_good is positional: not on a grown table
    one_bucket(ctx, myid)
    ctx.rtg_on_new_node(ids, [0, 1, 2, 3])
    g = np.ones(4, np.uint8)
    assert L.dhtgpu_rt_set_good(ctx._h, g.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))) == EINVAL


def test_a_257th_bucket_is_unapplied(ctx):
    """256 uploaded buckets (first byte = bucket number), my bucket full: its split would need a
    257th bucket -- that insertion and every later one are UNAPPLIED, the ones before it stay."""
    import opendht_amd
    rng = np.random.default_rng(10)
    firsts = np.zeros((256, 20), np.uint8)
    firsts[:, 0] = np.arange(256)
    myid = rng.integers(0, 256, 20, dtype=np.uint8)
    myid[0] = 77
    nodes = rng.integers(0, 256, (8, 20), dtype=np.uint8)
    nodes[:, 0] = 77
    off = np.zeros(257, np.uint32)
    off[78:] = 8
    ctx.rt_set(myid, firsts, off, nodes)
    m = C.Model.from_table(myid, firsts, off, nodes)
    x = rng.integers(0, 256, (4, 20), dtype=np.uint8)
    x[:, 0] = (5, 77, 200, 5)
    want, waux = m.batch(x, [100, 101, 102, 103])
    assert want.tolist() == [C.RTG_PLACED, C.RTG_UNAPPLIED, C.RTG_UNAPPLIED, C.RTG_UNAPPLIED]
    with pytest.raises(opendht_amd.DhtGpuError) as e:
        ctx.rtg_on_new_node(x, [100, 101, 102, 103])
    assert e.value.code == ERANGE
    assert np.array_equal(e.value.res, want) and np.array_equal(e.value.aux, waux)
    assert e.value.stat.tolist() == [256, 9, 0]
    same_table(ctx, m, "unapplied")
    tg = np.concatenate([x, nodes[:3]])
    got, cnt = ctx.rt_find_closest(tg, 8)                # the table still answers, in handles
    f, o, ids, h, st = m.export()
    wi, wc = O.find_closest_batch(f, o, ids, st & 1, tg, 8)
    assert np.array_equal(cnt, wc) and np.array_equal(got, np.where(wi == NONE, NONE, h[np.minimum(wi, 8)]))


def test_rt_set_drops_the_grown_form(ctx):
    myid, ids = C.uniform(2, 64)
    firsts, off, nodes = O.Table(myid).grow(ids).export()
    tg = O.gen_ids(77, 16)
    ctx.rt_set(myid, firsts, off, nodes, version=5)
    before = ctx.rt_find_closest(tg, 8)
    m = C.Model.from_table(myid, firsts, off, nodes)
    same_table(ctx, m, "an upload exports as it came")
    extra = O.gen_ids(78, 40)
    res, _ = new(ctx, m, extra, np.arange(900, 940))
    placed = np.flatnonzero(res == C.RTG_PLACED)
    assert placed.size and m.stat()[1] > nodes.shape[0]
    same_table(ctx, m, "grown from an upload")
    got, _ = ctx.rt_find_closest(extra[placed], 1)       # a resident id is its own closest node: handles now
    assert np.array_equal(got[:, 0], 900 + placed)
    ctx.rt_set(myid, firsts, off, nodes, version=5)      # the same version: not a short-cut to the grown table
    again = ctx.rt_find_closest(tg, 8)
    assert np.array_equal(again[0], before[0]) and np.array_equal(again[1], before[1])
    assert ctx.rtg_size() == (firsts.shape[0], nodes.shape[0])
    ctx.rt_set_good(np.ones(nodes.shape[0], np.uint8))   # positional again
    ctx.rt_set(myid, firsts, off, nodes, version=5)      # and this one is the short-cut: still the upload
    assert np.array_equal(ctx.rt_find_closest(tg, 8)[0], before[0])


# ---- one long-lived context -----------------------------------------------------------------------
def test_growth_on_a_long_lived_context(ctx):
    """Growth steps between calls of the other families on one context: the table's answers stay
    exact after each step and the others' fixed answers stay byte-identical."""
    myid, ops = C.random_walk(300, steps=10, alen=4)
    set_ids = O.gen_ids(50, 5000)
    tg = O.gen_ids(51, 70)
    ctx.set_ids(set_ids)
    k6 = ctx.batch_topk(tg, 8)
    want_k6 = O.topk(set_ids, tg, 8)
    assert np.array_equal(k6[0], want_k6[0]) and np.array_equal(k6[1], want_k6[1])
    keys = O.gen_ids(52, 400)
    ctx.nc_set(keys[:300])
    ctx.sr_reset(4)
    ctx.sr_open([0, 1, 2, 3], tg[:4])
    one_bucket(ctx, myid, 4)
    m = C.Model(myid)
    nxt = 300

    def others():
        return ctx.nc_nodes(tg, 8) + ctx.sr_lists([0, 1, 2, 3]) + ctx.nc_export()

    for i, op in enumerate(ops):
        before = others()
        apply(ctx, m, op, ("long", i, op[0]))
        assert all(np.array_equal(a, b) for a, b in zip(before, others())), ("long", i, op[0])
        same_table(ctx, m, ("long", i, op[0]))
        check_queries(ctx, m, tg[:12], 4, ("long", i, op[0]))
        # the other families, between the growth steps
        if nxt < 400:
            ctx.nc_insert(keys[nxt: nxt + 20], np.arange(nxt, nxt + 20, dtype=np.uint32))
            nxt += 20
        ctx.sr_refill([i % 4], 14)
        big = O.gen_ids(60 + i, 700 * (1 + i % 3))       # staging and aux2 carved again at another size
        assert np.array_equal(ctx.topk(big[:65], 8)[0], O.topk(set_ids, big[:65], 8)[0])
        ctx.rt_find_closest(big, 32)
        again = ctx.batch_topk(tg, 8)
        assert np.array_equal(again[0], k6[0]) and np.array_equal(again[1], k6[1]), i
        same_table(ctx, m, ("long, after the others", i))
    assert np.all(ctx.sr_lists([0, 1, 2, 3])[2] > 0) and ctx.nc_export()[0].shape[0] == nxt
    check_queries(ctx, m, tg[:12], 4, "long, at the end", dev=True)


def test_cpp_adapter_follows_the_table(tmp_path):
    """dhtgpu::ResidentTable's notes and flushes against a host table, and onNewNodeBatch (tests/cpp/rtgrow_check.cpp)"""
    import cpp_check
    cpp_check.run(cpp_check.build("rtgrow", tmp_path), ["--run"], "rtgrow_check", 120)
