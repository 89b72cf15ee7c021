"""GPU parity of Dht::trySearchInsert over the resident searches' ordered map (dhtgpu_srm_*,
opendht_amd/csrc/srmap.hip) against the model of srmap_cases.py (the walk of src/dht.cpp:118-150 over
the oracle's insertNode).  Every comparison is exact: out_cnt, out_touched, the stats (the number of
filtered nodes included), rows, flags, lengths and status words after every step of every script, and
the exported map.  Marked gpu: run on the MI355X box."""

import numpy as np
import pytest

import ncache_cases as NC
import oracle as O
import rsearch_cases as RS
import srmap_cases as SM

pytestmark = pytest.mark.gpu

EINVAL, ENOIDS, EUNSORTED, ERANGE = -1, -4, -5, -6


@pytest.fixture(scope="module")
def ctx():
    import opendht_amd
    c = opendht_amd.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def scripts():
    """every case, built once"""
    return dict(SM.all_scripts())


def assert_state(ctx, model, what, skip=()):
    slots = np.array([s for s in range(len(model.slots)) if s not in skip], dtype=np.uint32)
    got = ctx.sr_lists(slots) + (ctx.sr_status(slots),)
    want = model.lists(slots) + (model.status(slots),)
    for g, w, nm in zip(got, want, ("rows", "flags", "lens", "status")):
        bad = np.nonzero((g != w).reshape(g.shape[0], -1).any(axis=1))[0]
        assert bad.size == 0, f"{what}: {nm} of {bad.size} slots differ, first slot {slots[bad[0]]}: got {g[bad[0]]} want {w[bad[0]]}"
    if model.order is not None:
        for g, w, nm in zip(ctx.srm_export(), model.export(), ("map order", "done bits")):
            assert np.array_equal(g, w), f"{what}: {nm} differ"


def assert_offer(got, want, what):
    for g, w, nm in zip(got, want, ("out_cnt", "out_touched", "out_stats")):
        assert np.array_equal(g, w), f"{what}: {nm} differ at {np.nonzero(g != w)[0][:5]}: got {g[g != w][:5]} want {w[g != w][:5]}"


@pytest.mark.parametrize("name", [n for n, _ in SM.all_scripts()])
def test_scripts(ctx, scripts, name):
    """Every script, step by step: maps of 0 / 1 / 2 / 63 / 64 / 65 / 257 searches, offers of 0 / 1 / 63 /
    64 / 65 / 300 nodes, ids below, above and equal to targets, 64 and 128 shared leading bits, fresh
    lists crossed in both directions, converged lists the filter answers, the run of nine refusing
    searches, the cut as the only change, both hazards."""
    model = SM.Model()
    for k, step in enumerate(scripts[name]):
        want, got = SM.run_step(step, model, ctx)
        what = f"{name} step {k} {step[0]}"
        if step[0] == "offer":
            assert_offer(got, want, what)
        elif want is not None:
            assert np.array_equal(got, want), f"{what}: results differ"
        if model.slots and step[0] not in ("nc_set", "nc_accept"):
            assert_state(ctx, model, what)


def _dev(a, dtype):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(dtype)).to(torch.device("cuda", 0))


@pytest.mark.parametrize("name", ["fresh", "shape408", "shape452", "converged"])
def test_dev_form_and_back_to_back_offers(ctx, scripts, name):
    """The offers through dhtgpu_srm_offer_dev on a side stream with device buffers; consecutive offers
    (fresh has two) are issued with no synchronise between them and read after one.  The results equal
    the model, which the host form equals."""
    import opendht_amd
    import torch
    dev = torch.device("cuda", 0)
    side = torch.cuda.Stream(device=dev)
    model, pending, keep = SM.Model(), [], []

    def flush():
        torch.cuda.synchronize()
        for what, bufs, want in pending:
            assert_offer([b.cpu().numpy().view(np.uint32) for b in bufs], want, what)
        del pending[:], keep[:]

    with torch.cuda.stream(side):
        for k, step in enumerate(scripts[name]):
            if step[0] != "offer":
                flush()
                SM.run_step(step, model, ctx)
                torch.cuda.synchronize()
                continue
            h, ids = np.asarray(step[1], np.uint32), RS.as_ids(step[2])
            m = h.shape[0]
            stride = m + 3
            planes = np.zeros((5, stride), np.uint32)
            planes[:, :m] = opendht_amd.id_words(ids)
            d_in = [_dev(h, np.int32), _dev(planes.reshape(-1), np.int32)]
            cnt = torch.full((max(m, 1),), -1, dtype=torch.int32, device=dev)
            touched = torch.full(((len(model.slots) + 31) // 32,), -1, dtype=torch.int32, device=dev)
            stats = torch.full((4,), -1, dtype=torch.int32, device=dev)
            ctx.srm_offer_dev(d_in[0].data_ptr(), d_in[1].data_ptr(), stride, m, cnt.data_ptr(), touched.data_ptr(),
                              stats.data_ptr(), side.cuda_stream)
            keep.append(d_in)
            pending.append((f"{name} step {k} offer_dev", (cnt[:m], touched, stats), model.offer(h, ids)))
        flush()
    assert_state(ctx, model, f"{name} through the _dev form")


def test_map_validity():
    """ENOIDS before srm_set and after an sr_open or sr_reset, srm_set again makes the offer work;
    sr_expire keeps the map; equal targets are EUNSORTED and leave no map; argument errors."""
    import opendht_amd
    c = opendht_amd.Context(0)
    try:
        def code(f, *a):
            with pytest.raises(opendht_amd.DhtGpuError) as e:
                f(*a)
            return e.value.code

        ids = O.gen_ids(9, 6)
        slots = np.arange(4, dtype=np.uint32)
        for f, a in ((c.srm_set, (slots,)), (c.srm_set_done, (slots, 1)), (c.srm_offer, ([1], ids[:1])), (c.srm_export, ())):
            assert code(f, *a) == ENOIDS, f.__name__
        c.sr_reset(5)
        c.sr_open(slots, ids[:4])
        assert code(c.srm_offer, [1], ids[:1]) == ENOIDS and code(c.srm_export) == ENOIDS
        c.srm_set_done(slots[:1], 1)                     # the done bit needs no map
        c.srm_set(slots)
        assert list(c.srm_export()[1]) == [int(s == 0) for s in c.srm_export()[0]]
        assert c.srm_offer([1], ids[4:5])[0][0] >= 1
        c.sr_expire(slots[1:2])
        assert c.srm_offer([2], ids[5:6])[0][0] >= 1     # an expired search stays in the map
        c.sr_open(slots[:1], ids[:1])
        assert code(c.srm_offer, [1], ids[:1]) == ENOIDS and code(c.srm_export) == ENOIDS
        c.srm_set(slots)
        assert not c.srm_export()[1].any()               # the slot opened again is not done
        c.srm_offer([1], ids[4:5])
        assert code(c.srm_set, [0, 1, 0]) == EINVAL and code(c.srm_set, [5]) == EINVAL
        assert code(c.srm_set_done, [5], 1) == EINVAL
        assert code(c.srm_offer, [NC.MAX_HANDLE], ids[:1]) == EINVAL
        c.srm_offer([1], ids[4:5])                       # failed argument checks left the map alone
        c.sr_open(np.array([4], np.uint32), ids[1:2])    # slot 4: the target of slot 1
        assert code(c.srm_set, [0, 1, 4]) == EUNSORTED and code(c.srm_offer, [1], ids[:1]) == ENOIDS
        c.srm_set([0, 4])
        assert sorted(c.srm_export()[0]) == [0, 4]
        c.srm_set([])
        cnt, touched, stats = c.srm_offer([1, 2], ids[:2])
        assert list(cnt) == [0, 0] and not touched.any() and list(stats) == [2, 0, 0, 0]
        c.sr_reset(5)
        assert code(c.srm_offer, [1], ids[:1]) == ENOIDS
    finally:
        c.close()


def test_overflow(ctx):
    """Search A takes 5 good nodes and then 70 distinct expired ones in one offer: it ends with 64
    entries and the overflow bit, the host form raises ERANGE after applying everything, the 11 nodes
    that found the row full were taken by no search (A refuses and is neither expired nor done), and
    searches B and C -- full, reached by every walk that A let pass -- equal the model."""
    import opendht_amd
    rng = np.random.default_rng(88)
    targets = SM.ladder(3)
    slots = np.arange(3, dtype=np.uint32)
    state = np.zeros(300, np.uint8)
    state[100:170] = 1
    model = SM.Model()
    good_h = np.arange(1, 29, dtype=np.uint32)
    good_k = np.concatenate([SM.near(targets[1], rng, 14), SM.near(targets[2], rng, 14)])
    for step in (("reset", 3), ("set_state", state), ("open", slots, targets),
                 ("insert", slots[1:], RS.csr([14, 14]), good_h, good_k, None), ("srm_set", slots)):
        SM.run_step(step, model, ctx)
    bad_k = O.gen_ids(880, 70)
    bad_k[:, 0] = rng.integers(0, 16, size=70)           # below A's target: A is every walk's first search
    h = np.concatenate([np.arange(200, 205), np.arange(100, 170)]).astype(np.uint32)
    k = np.concatenate([SM.near(targets[1], rng, 5, bits=8), bad_k])
    want = model.offer(h, k)
    with pytest.raises(opendht_amd.DhtGpuError) as e:
        ctx.srm_offer(h, k)
    assert e.value.code == ERANGE
    cnt, touched, stats = e.value.result
    assert np.array_equal(cnt[:5], want[0][:5]) and (cnt[:5] == 2).all()
    assert list(cnt[5:]) == [1] * 59 + [0] * 11
    assert touched[0] == 0b011 and list(stats[2:]) == [0, 1]
    assert list(ctx.sr_status(slots[:1])[0]) == [64, 59, 59, 2]   # (the expired nodes lie closer to A's target)
    assert_state(ctx, model, "the other searches of the overflowing offer", skip=(0,))


def test_other_families_untouched(ctx, scripts):
    """One context holding a routing table, a NodeCache mirror and searches: the rt and nc answers are
    byte-identical before and after map builds, done bits and offers."""
    rng = np.random.default_rng(99)
    nodes = O.gen_ids(990, 300)
    nodes = nodes[np.lexsort(nodes.T[::-1])]
    firsts = np.zeros((4, 20), np.uint8)
    firsts[:, 0] = [0, 64, 128, 192]
    off = np.concatenate([[np.count_nonzero(nodes[:, 0] < b) for b in (0, 64, 128, 192)], [300]]).astype(np.uint32)
    keys = O.gen_ids(991, 500)
    tg = O.gen_ids(992, 40)
    ctx.rt_set(O.gen_ids(993, 1)[0], firsts, off, nodes)
    ctx.nc_set(keys, (rng.permutation(500) + 9).astype(np.uint32))

    def answers():
        return ctx.rt_find_closest(tg, 8) + ctx.nc_nodes(tg, 14) + ctx.nc_export()

    before = answers()
    model = SM.Model()
    for step in scripts["shape407"]:
        SM.run_step(step, model, ctx)
    after = answers()
    for b, a in zip(before, after):
        assert b.tobytes() == a.tobytes()
    assert_state(ctx, model, "the searches beside rt and nc state")


def test_cpp_adapter_on_device(tmp_path):
    """tests/cpp/srmap_check.cpp --run: dhtgpu::ResidentSearches::offerBatch on mock Search / SearchNode /
    Node types, on both sides of its threshold in turn, against the oracle's walk."""
    import cpp_check
    cpp_check.run(cpp_check.build("srmap", tmp_path), ["--run"], "srmap_check (device paths)", 120)
