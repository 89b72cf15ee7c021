"""GPU parity of the resident searches (dhtgpu_sr_*, opendht_amd/csrc/rsearch.hip): the wave-per-search
insertNode, the fused Dht::refill and the small kernels against the model of rsearch_cases.py (the CPU
oracle's search_insert and getCachedNodes walk).  Every comparison is exact: rows, flags, lengths,
`expired`, added / inserted and the status words, after every step of every script.  Marked gpu: run
on the MI355X box."""

import numpy as np
import pytest

import ncache_cases as NC
import oracle as O
import rsearch_cases as RS

pytestmark = pytest.mark.gpu

EINVAL, ENOIDS, ERANGE = -1, -4, -6


@pytest.fixture(scope="module")
def ctx():
    import opendht_amd
    c = opendht_amd.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def scripts():
    """every exact case, built once"""
    return dict(RS.all_exact_scripts())


def assert_state(ctx, model, what, skip=()):
    """the whole search set equals the model (but for the slots in `skip`)"""
    slots = np.array([s for s in range(len(model.slots)) if s not in skip], dtype=np.uint32)
    got = ctx.sr_lists(slots) + (ctx.sr_status(slots),)
    want = model.lists(slots) + (model.status(slots),)
    for g, w, nm in zip(got, want, ("rows", "flags", "lens", "status")):
        bad = np.nonzero((g != w).reshape(g.shape[0], -1).any(axis=1))[0]
        assert bad.size == 0, f"{what}: {nm} of {bad.size} slots differ, first slot {slots[bad[0]]}: got {g[bad[0]]} want {w[bad[0]]}"


def run_exact(ctx, script, name):
    """every step on the model and the context, compared after each; returns the context's results"""
    model, results = RS.Model(), []
    for k, step in enumerate(script):
        want, got = RS.run_step(step, model, ctx)
        what = f"{name} step {k} {step[0]}"
        if want is not None:
            assert np.array_equal(got, want), f"{what}: results differ at {np.nonzero(got != want)[0][:5]}"
        if model.slots and step[0] not in ("nc_set", "nc_accept"):
            assert_state(ctx, model, what)
        results.append(got)
    return results


@pytest.mark.parametrize("case", RS.INSERT_SHAPES, ids=lambda c: f"s{c[1]}-i{c[2]}-p{c[3]}-b{c[4]}")
def test_insert_shapes(ctx, scripts, case):
    """Search::insertNode one wave per search: 1 / 4 / 5 / 700 slots per call (the waves of a
    workgroup), 0 / 1 / 64 / 65 / 200 insertions per slot (the 64-insertion chunk), pools of 64 (repeats
    of present nodes) / 500 / 20000 nodes, ids and targets sharing 0 / 32 / 64 / 128 leading bits (the
    compare reaches words 1 to 4), expired and removable nodes, candidates, tokens at 30 %, a fifth
    of the searches expired, lists pre-filled to 13, 14, 15 and >= 50 entries."""
    run_exact(ctx, scripts[f"insert{case[0]}"], f"insert{case[0]}")


@pytest.mark.parametrize("case", RS.REFILL_SHAPES, ids=lambda c: f"n{c[1]}-c{c[2]}-{c[3]}-{c[4]}")
def test_refill_shapes(ctx, scripts, case):
    """Dht::refill fused: mirrors of 0 .. 20000 keys, counts 1 / 14 / 32, every accept kind, refill
    into empty, partly filled and full lists; the same refill again inserts nothing."""
    script = scripts[f"refill{case[0]}"]
    results = run_exact(ctx, script, f"refill{case[0]}")
    assert script[-1][0] == "refill" and script[-2][0] == "refill" and not results[-1].any()


def test_refill_walk_order_and_full_compare(ctx, scripts):
    """non_monotone: the refill offers the walk's nodes, not the closest by distance; clustered: keys
    and targets that differ in word 4 only."""
    run_exact(ctx, scripts["non_monotone"], "non_monotone")
    run_exact(ctx, RS.non_monotone_script(count=3), "non_monotone3")
    run_exact(ctx, scripts["clustered"], "clustered")


def test_life_cycle(ctx, scripts):
    """reset, open, refill, insert with tokens, update_state, insert, set_candidate on and off (an
    absent handle included), nc_erase / nc_insert, refill, sr_expire, refill, re-open: the model after
    every step."""
    run_exact(ctx, scripts["lifecycle"], "lifecycle")


@pytest.mark.parametrize("m", [257, 65537])
def test_update_state_many(ctx, m):
    """m distinct handles with random state bytes in one call (more than one block of the setter,
    and 256 blocks and one thread more), every one of them listed in a search: the status words read
    bit0 of each, and one more insertion per search acts on bit1"""
    nslots, per = (m + 13) // 14 + 3, 14
    rng = np.random.default_rng(m)
    ids = O.gen_ids(880, nslots * (per + 1))
    handles = (rng.permutation(nslots * (per + 1)) + 7).astype(np.uint32)
    slots = np.arange(nslots, dtype=np.uint32)
    first = nslots * per
    upd = rng.choice(handles[:first], m, replace=False)
    val = rng.choice([0, 1, 2, 3], m).astype(np.uint8)
    script = [("reset", nslots), ("open", slots, O.gen_ids(881, nslots)),
              ("insert", slots, RS.csr(np.full(nslots, per)), handles[:first], ids[:first]),
              ("update_state", upd, val),
              ("insert", slots, RS.csr(np.full(nslots, 1)), handles[first:], ids[first:])]
    run_exact(ctx, script, f"update_state m={m}")


def _dev(a, dtype):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(dtype)).to(torch.device("cuda", 0))


def test_stream_ordered_forms(ctx, scripts):
    """The life cycle with insert, refill, status and lists through the _dev entry points on a side
    stream with device buffers.  Consecutive _dev calls are issued without any synchronise between
    them and read after one synchronise; the steps that exist as host forms only (state, candidates,
    nc mutations, open, expire -- ordered on the context's stream) run between two device
    synchronises.  The results equal the model, which the host forms equal."""
    import torch
    dev = torch.device("cuda", 0)
    side = torch.cuda.Stream(device=dev)
    s = side.cuda_stream
    model = RS.Model()
    pending, keep = [], []

    def flush():
        torch.cuda.synchronize()
        for what, bufs, want in pending:
            for b, w, nm in zip(bufs, want, ("result", "rows", "flags", "lens", "status")):
                g = b.cpu().numpy().view(w.dtype).reshape(w.shape)
                assert np.array_equal(g, w), f"{what}: {nm} differ"
        del pending[:], keep[:]

    with torch.cuda.stream(side):   # the buffers' fills and uploads are ordered on the side stream too
        _stream_life_cycle(ctx, scripts["lifecycle"], model, pending, keep, flush, s)
    assert_state(ctx, model, "lifecycle through the _dev forms")


def _stream_life_cycle(ctx, script, model, pending, keep, flush, s):
    import opendht_amd
    import torch
    dev = torch.device("cuda", 0)
    nsl = 0
    for k, step in enumerate(script):
        op = step[0]
        if op not in ("insert", "refill"):
            flush()
            RS.run_step(step, model, ctx)
            torch.cuda.synchronize()
            nsl = len(model.slots)
            continue
        slots = np.ascontiguousarray(step[1], dtype=np.uint32)
        m = slots.shape[0]
        d_slots = _dev(slots, np.int32)
        if op == "insert":
            _, off, handle, ids, tok = step[1:]
            tot = int(off[-1])
            stride = tot + 5
            planes = np.zeros((5, stride), np.uint32)
            planes[:, :tot] = opendht_amd.id_words(ids[:tot])
            d_in = [_dev(np.asarray(off, np.uint64), np.int64), _dev(np.asarray(handle[:tot], np.uint32), np.int32),
                    _dev(planes.reshape(-1), np.int32), _dev(np.asarray(tok[:tot], np.uint8), np.uint8)]
            res = torch.zeros(tot, dtype=torch.uint8, device=dev)
            ctx.sr_insert_dev(d_slots.data_ptr(), m, d_in[0].data_ptr(), d_in[1].data_ptr(), d_in[2].data_ptr(), stride,
                              d_in[3].data_ptr(), res.data_ptr(), s)
            want = model.insert(*step[1:])
            keep.append(d_in)
        else:
            res = torch.zeros(m, dtype=torch.int32, device=dev)
            ctx.sr_refill_dev(d_slots.data_ptr(), m, step[2], res.data_ptr(), s)
            want = model.refill(step[1], step[2])
        every = np.arange(nsl, dtype=np.uint32)
        d_all = _dev(every, np.int32)
        oh = torch.empty((nsl, 64), dtype=torch.int32, device=dev)
        of = torch.empty((nsl, 64), dtype=torch.uint8, device=dev)
        ol = torch.empty(nsl, dtype=torch.int32, device=dev)
        o4 = torch.empty((nsl, 4), dtype=torch.int32, device=dev)
        ctx.sr_lists_dev(d_all.data_ptr(), nsl, oh.data_ptr(), of.data_ptr(), ol.data_ptr(), s)
        ctx.sr_status_dev(d_all.data_ptr(), nsl, o4.data_ptr(), s)
        keep.append((d_slots, d_all))
        pending.append((f"lifecycle step {k} {op}", (res, oh, of, ol, o4), (want,) + model.lists(every) + (model.status(every),)))
    flush()


def test_overflow(ctx):
    """One call in which slots 0, 3 and 6 take 80 distinct expired nodes each: those slots end with 64
    entries -- the first 64 offered, distinct, in ascending distance -- and the overflow bit; the host
    form raises ERANGE after applying everything else, and every other slot of the call equals the
    model.  A refill that drops nodes raises ERANGE too; opening a slot again clears its bit."""
    import opendht_amd
    rng = np.random.default_rng(77)
    nslots, over = 12, (0, 3, 6)
    xids, xh = O.gen_ids(770, 80), np.arange(80, dtype=np.uint32)
    pool, ph = O.gen_ids(771, 300), np.arange(100, 400, dtype=np.uint32)
    state = np.zeros(420, np.uint8)
    state[:80] = 1
    state[400:] = 1
    state[ph[:30]] = rng.choice([1, 2, 3], size=30)
    targets = O.gen_ids(772, nslots)
    slots = np.arange(nslots, dtype=np.uint32)
    model = RS.Model()
    for step in (("reset", nslots), ("set_state", state), ("open", slots, targets)):
        RS.run_step(step, model, ctx)
    hs, ks, cnt = [], [], []
    for sl in slots:
        if sl in over:
            hs.append(xh), ks.append(xids), cnt.append(80)
        else:
            pick = rng.integers(0, 300, size=70)
            hs.append(ph[pick]), ks.append(pool[pick]), cnt.append(70)
    hs, ks, off = np.concatenate(hs), np.concatenate(ks), RS.csr(cnt)
    tok = (rng.random(hs.size) < 0.3).astype(np.uint8)
    want = model.insert(slots, off, hs, ks, tok)
    with pytest.raises(opendht_amd.DhtGpuError) as e:
        ctx.sr_insert(slots, off, hs, ks, tok)
    assert e.value.code == ERANGE
    for sl in slots:
        lo, hi = int(off[sl]), int(off[sl + 1])
        if sl not in over:
            assert np.array_equal(e.value.added[lo:hi], want[lo:hi]), sl
        else:
            assert list(e.value.added[lo:hi]) == [1] * 64 + [0] * 16
    assert_state(ctx, model, "the other slots of the overflowing call", skip=over)
    oslots = np.array(over, dtype=np.uint32)
    rows, _, lens = ctx.sr_lists(oslots)
    st = ctx.sr_status(oslots)
    for i, sl in enumerate(over):
        t = NC.key_int(targets[sl])
        dist = [NC.key_int(xids[h]) ^ t for h in rows[i]]
        assert lens[i] == 64 and sorted(rows[i]) == list(range(64)) and dist == sorted(dist)
        assert list(st[i]) == [64, 64, 64, 2]
    # a refill into a full row of bad nodes: the cache's (expired) nodes are dropped
    RS.run_step(("nc_set", O.gen_ids(773, 20), np.arange(400, 420, dtype=np.uint32)), model, ctx)
    two = np.array([3, 4], dtype=np.uint32)
    winserted = model.refill(two[1:], 14)
    with pytest.raises(opendht_amd.DhtGpuError) as e:
        ctx.sr_refill(two, 14)
    assert e.value.code == ERANGE and e.value.inserted[0] == 0 and e.value.inserted[1] == winserted[0]
    assert_state(ctx, model, "the other slot of the overflowing refill", skip=over)
    assert ctx.sr_status(oslots)[1, 0] == 64
    RS.run_step(("open", oslots[:1], targets[:1]), model, ctx)
    assert list(ctx.sr_status(oslots[:1])[0]) == [0, 0, 0, 0]
    assert ctx.sr_status(oslots)[1, 3] == 2


def test_argument_errors():
    """Before any launch: ENOIDS before sr_reset and for a refill without an nc mirror; EINVAL for a
    slot >= nslots, a handle >= DHTGPU_NC_MAX_HANDLE, duplicate slots in one host call, count 0 / 33;
    ERANGE for more than 2^20 slots."""
    import opendht_amd
    c = opendht_amd.Context(0)
    try:
        def code(f, *a):
            with pytest.raises(opendht_amd.DhtGpuError) as e:
                f(*a)
            return e.value.code

        ids = O.gen_ids(5, 4)
        one, off1 = np.array([0], np.uint32), np.array([0, 1], np.uint64)
        for f, a in ((c.sr_open, (one, ids[:1])), (c.sr_expire, (one,)), (c.sr_set_state, ([0, 1],)),
                     (c.sr_update_state, ([1], 1)), (c.sr_set_candidate, (one, [1], 1)),
                     (c.sr_insert, (one, off1, [1], ids[:1])), (c.sr_refill, (one, 14)), (c.sr_status, (one,)),
                     (c.sr_lists, (one,))):
            assert code(f, *a) == ENOIDS, f.__name__
        assert code(c.sr_reset, (1 << 20) + 1) == ERANGE
        c.sr_reset(4)
        assert code(c.sr_refill, one, 14) == ENOIDS          # no nc mirror
        c.nc_set(ids)
        c.sr_open(np.arange(4, dtype=np.uint32), ids)
        four = np.array([4], np.uint32)
        for f, a in ((c.sr_open, (four, ids[:1])), (c.sr_expire, (four,)), (c.sr_set_candidate, (four, [1], 1)),
                     (c.sr_insert, (four, off1, [1], ids[:1])), (c.sr_refill, (four, 14)), (c.sr_status, (four,)),
                     (c.sr_lists, (four,))):
            assert code(f, *a) == EINVAL, f.__name__
        big = [NC.MAX_HANDLE]
        assert code(c.sr_insert, one, off1, big, ids[:1]) == EINVAL
        assert code(c.sr_update_state, big, 1) == EINVAL
        assert code(c.sr_set_candidate, one, big, 1) == EINVAL
        dup = np.array([1, 2, 1], np.uint32)
        assert code(c.sr_insert, dup, np.array([0, 1, 2, 3], np.uint64), [1, 2, 3], ids[:3]) == EINVAL
        assert code(c.sr_refill, dup, 14) == EINVAL
        assert code(c.sr_refill, one, 0) == EINVAL and code(c.sr_refill, one, 33) == EINVAL
        assert code(c.sr_insert, one, np.array([1, 0], np.uint64), [1], ids[:1]) == EINVAL   # offsets go down
        assert not c.sr_status(np.arange(4, dtype=np.uint32)).any()       # nothing was applied
        assert list(c.sr_refill(np.arange(4, dtype=np.uint32), 14)) == [4, 4, 4, 4]
    finally:
        c.close()


def test_cpp_adapter_on_device(tmp_path):
    """tests/cpp/rsearch_check.cpp --run: dhtgpu::ResidentSearches on mock Search / SearchNode / Node
    types, refillBatch on both sides of its threshold against the oracle."""
    import cpp_check
    cpp_check.run(cpp_check.build("rsearch", tmp_path), ["--run", "--quick"], "rsearch_check (device paths)", 300)
