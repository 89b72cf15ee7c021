"""GPU parity of the resident NodeCache (dhtgpu_nc_*, opendht_amd/csrc/ncache.hip): the wave-per-target
getCachedNodes and the one-pass insert / erase against the model of ncache_cases.py (a dict and the
CPU oracle O.cached_nodes_batch) and against dhtgpu_cache_set + dhtgpu_cache_nodes.  Every
comparison is exact.  Marked gpu: run on the MI355X box."""

import numpy as np
import pytest

import ncache_cases as NC
import oracle as O

pytestmark = pytest.mark.gpu

NONE = NC.NONE
EINVAL, ENOIDS, EUNSORTED, ERANGE = -1, -4, -5, -6


@pytest.fixture(scope="module")
def ctx():
    import opendht_amd
    c = opendht_amd.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def keysets():
    """one random key set per size, shared and left unchanged"""
    return {n: O.gen_ids(900 + n, n) if n else np.zeros((0, 20), np.uint8) for n in NC.SIZES}


def assert_rows(got, cnt, want, wcnt, what):
    assert np.array_equal(cnt, wcnt), f"{what}: counts differ"
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, f"{what}: {bad.size} rows differ, first {bad[:5]}: got {got[bad[0]]} want {want[bad[0]]}"


def device_targets(tg, stride):
    import opendht_amd
    import torch
    q = tg.shape[0]
    planes = np.zeros((5, stride), np.uint32)
    planes[:, :q] = opendht_amd.id_words(tg)
    return torch.from_numpy(planes.view(np.int32).reshape(-1)).to(torch.device("cuda", 0))


def nodes_dev(ctx, tg, count, stream=None, sync=True):
    """nc_nodes_dev with an odd target stride; stream None = the context's"""
    import torch
    dev = torch.device("cuda", 0)
    q = tg.shape[0]
    stride = q + 3 if (q + 3) % 2 else q + 4
    tp = device_targets(tg, stride)
    oh = torch.empty((q, count), dtype=torch.int32, device=dev)
    oc = torch.empty(q, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    ctx.nc_nodes_dev(tp.data_ptr(), stride, q, count, oh.data_ptr(), oc.data_ptr(), stream)
    if sync:
        torch.cuda.synchronize()
    return oh, oc, tp


def check_model(ctx, model, what, targets=None, counts=(8,)):
    """the mirror equals the model: size, export, and a lookup batch"""
    keys, handles = model.sorted()
    assert ctx.nc_size() == keys.shape[0], what
    gk, gh = ctx.nc_export()
    assert np.array_equal(gk, keys), f"{what}: exported keys"
    assert np.array_equal(gh, handles), f"{what}: exported handles"
    tg = NC.targets_for(keys, 3) if targets is None else targets
    for count in counts:
        want, wcnt = model.expected(tg, count)
        got, cnt = ctx.nc_nodes(tg, count)
        assert_rows(got, cnt, want, wcnt, (what, count))


# ---- lookups -----------------------------------------------------------------------------------
@pytest.mark.parametrize("n", NC.SIZES)
def test_lookup_sizes_counts_accepts(ctx, keysets, n):
    """every size x count x accept kind: host form = oracle = dhtgpu_cache_set + dhtgpu_cache_nodes
    (handles 0..n-1), and the _dev form on a side stream with an odd stride gives the same rows"""
    import torch
    keys = keysets[n]
    model = NC.Model()
    model.set(keys)
    ctx.nc_set(keys)
    ctx.cache_set(keys)
    skeys, shandles = model.sorted()
    tg = NC.targets_for(keys, n + 1)
    side = torch.cuda.Stream(device=torch.device("cuda", 0))
    for kind in NC.ACCEPTS:
        model.acc = NC.accept_handles(kind, shandles)
        by_handle = np.array([h in model.acc for h in range(n)], dtype=np.uint8)
        ctx.nc_set_accept(by_handle)
        for count in NC.COUNTS:
            want, wcnt = model.expected(tg, count)
            got, cnt = ctx.nc_nodes(tg, count)
            assert_rows(got, cnt, want, wcnt, (n, kind, count))
            old, ocnt = ctx.cache_nodes(tg, count, by_handle if n else None)
            assert_rows(got, cnt, old, ocnt, ("cache_nodes", n, kind, count))
            oh, oc, _ = nodes_dev(ctx, tg, count, side.cuda_stream)
            assert_rows(oh.cpu().numpy().view(np.uint32), oc.cpu().numpy().view(np.uint32), want, wcnt,
                        ("dev", n, kind, count))


def test_custom_handles(ctx, keysets):
    keys = keysets[4097]
    handles = (np.random.default_rng(2).permutation(3 * 4097)[:4097] + 11).astype(np.uint32)
    model = NC.Model()
    model.set(keys, handles)
    ctx.nc_set(keys, handles)
    check_model(ctx, model, "custom handles", counts=(8, 32))
    rej = handles[::3]
    model.update_accept(rej, 0)
    ctx.nc_update_accept(rej, 0)
    check_model(ctx, model, "custom handles, a third rejected", counts=(14,))


def test_non_monotone_walk_order(ctx):
    """the next side is not monotone in XOR distance: the rows follow the head comparison, and a
    distance sort of the same keys is a different row"""
    keys, target = NC.non_monotone()
    model = NC.Model()
    model.set(keys)
    ctx.nc_set(keys)
    for count in (3, 8, 32):
        want, wcnt = model.expected(target, count)
        got, cnt = ctx.nc_nodes(target, count)
        assert_rows(got, cnt, want, wcnt, ("non-monotone", count))
    skeys, sh = model.sorted()
    want, _ = model.expected(target, 3)
    pos = {int(h): i for i, h in enumerate(sh)}
    assert [pos[int(h)] for h in want[0]] == [0, 1, 2]                                  # 0000, 1000, 1001
    assert NC.distance_sorted(skeys, np.ones(len(sh)), target[0], 3) != [0, 1, 2]


def test_clustered_keys(ctx):
    """200 keys that share their first 128 bits: words 0..3 decide nothing"""
    keys, targets = NC.clustered()
    model = NC.Model()
    model.set(keys)
    ctx.nc_set(keys)
    check_model(ctx, model, "clustered", targets, NC.COUNTS)
    _, sh = model.sorted()
    model.acc = NC.accept_handles("reject30", sh)
    ctx.nc_set_accept(np.array([h in model.acc for h in range(len(sh))], np.uint8))
    check_model(ctx, model, "clustered, 30 % rejected", targets, NC.COUNTS)


# ---- mutations ---------------------------------------------------------------------------------
@pytest.mark.parametrize("n", NC.SIZES)
def test_insert_into_every_size(ctx, keysets, n):
    """m in {1, 63, 4097} into a mirror of n keys (handles 7 + 3 i): present keys, one key twice,
    the smallest and the largest key; an accept array leaves a present key's bit alone"""
    keys = keysets[n]
    for m in (1, 63, 4097):
        model = NC.Model()
        h0 = (7 + 3 * np.arange(n)).astype(np.uint32)
        model.set(keys, h0)
        ctx.nc_set(keys, h0)
        ids, handles, accept = NC.mutation_batch(model, m, 31 * n + m, 7 + 3 * n + 100)
        want_new = model.insert(ids, handles, accept)
        got_new = ctx.nc_insert(ids, handles, accept)
        assert np.array_equal(got_new, want_new), (n, m)
        check_model(ctx, model, ("insert", n, m))


@pytest.mark.parametrize("n", [1, 64, 4097, 70000])
def test_erase(ctx, keysets, n):
    """absent keys, the same key twice in one batch, then everything, then insert again"""
    keys = keysets[n]
    model = NC.Model()
    model.set(keys)
    ctx.nc_set(keys)
    batch = np.concatenate([keys[:: max(1, n // 50)], O.gen_ids(5, 9), keys[:1], keys[:1]])
    want = model.erase(batch)
    got = ctx.nc_erase(batch)
    assert np.array_equal(got, want), n
    assert want[-1] == 0 and want[-2] == 0     # repeats of keys[0], which the batch erased first
    check_model(ctx, model, ("erase", n))
    rest, _ = model.sorted()
    every = np.concatenate([rest, keys[:3]]) if rest.shape[0] else keys[:3]
    assert np.array_equal(ctx.nc_erase(every), model.erase(every))
    assert ctx.nc_size() == 0
    check_model(ctx, model, ("erased everything", n))
    again = keys[: min(n, 300)]
    hs = np.arange(5, 5 + again.shape[0], dtype=np.uint32)
    assert np.array_equal(ctx.nc_insert(again, hs), model.insert(again, hs))
    check_model(ctx, model, ("insert after erasing everything", n))


def test_batches_of_many_blocks(ctx, keysets):
    """20,000 keys a batch (79 blocks of 256): the kept keys' offsets carry across blocks, with
    present keys and repeats scattered through the batch"""
    keys = keysets[4097]
    fresh = O.gen_ids(73, 20000)
    model = NC.Model()
    model.set(keys)
    ctx.nc_set(keys)
    ids = fresh.copy()
    ids[5::7] = keys[np.arange(ids[5::7].shape[0]) % 4097]      # present keys
    ids[9000:9100] = ids[100:200]                                # repeats of earlier batch keys
    hs = np.arange(5000, 25000, dtype=np.uint32)
    assert np.array_equal(ctx.nc_insert(ids, hs), model.insert(ids, hs))
    check_model(ctx, model, "insert 20,000")
    gone = np.concatenate([fresh[::2], O.gen_ids(74, 3000), fresh[:500]])
    assert np.array_equal(ctx.nc_erase(gone), model.erase(gone))
    check_model(ctx, model, "erase 13,500")


def test_batch_past_one_scan_round(ctx, keysets):
    """270,000 keys in one batch: more than the 1,024 blocks (262,144 keys) the block-count scan
    takes per round.  Checked with numpy alone (a lexicographic sort of the distinct keys): the
    last 2,000 keys of the batch repeat its first 2,000 and must not be inserted."""
    base = keysets[4096]
    fresh = O.gen_ids(75, 268000)
    ids = np.concatenate([fresh, fresh[:2000]])
    hs = np.arange(10000, 10000 + ids.shape[0], dtype=np.uint32)
    ctx.nc_set(base)
    new = ctx.nc_insert(ids, hs)
    assert new[:268000].all() and not new[268000:].any()
    every = np.concatenate([base, fresh])
    eh = np.concatenate([np.arange(4096, dtype=np.uint32), hs[:268000]])
    w = every.view(">u4").reshape(-1, 5)
    order = np.lexsort((w[:, 4], w[:, 3], w[:, 2], w[:, 1], w[:, 0]))
    gk, gh = ctx.nc_export()
    assert np.array_equal(gk, every[order]) and np.array_equal(gh, eh[order])
    found = ctx.nc_erase(ids)
    assert found[:268000].all() and not found[268000:].any()
    gk, gh = ctx.nc_export()
    w = base.view(">u4").reshape(-1, 5)
    order = np.lexsort((w[:, 4], w[:, 3], w[:, 2], w[:, 1], w[:, 0]))
    assert np.array_equal(gk, base[order]) and np.array_equal(gh, order.astype(np.uint32))


def test_growth_past_the_head_room(ctx):
    """100 keys, then 5,000 more in batches: both buffer sets are reallocated on the way"""
    keys = O.gen_ids(61, 5100)
    model = NC.Model()
    model.set(keys[:100])
    ctx.nc_set(keys[:100])
    at = 100
    for step, m in enumerate((1, 63, 400, 936, 1500, 2100)):
        ids = keys[at: at + m]
        hs = np.arange(at, at + m, dtype=np.uint32)
        assert np.array_equal(ctx.nc_insert(ids, hs), model.insert(ids, hs))
        at += m
        check_model(ctx, model, ("growth", step))
    assert ctx.nc_size() == 5100


def test_random_mutation_sequence(ctx):
    """30 seeded random mutations -- insert, erase, update_accept, set_accept -- checked after each"""
    rng = np.random.default_rng(2024)
    pool = O.gen_ids(88, 6000)
    model = NC.Model()
    model.set(pool[:500], np.arange(500, dtype=np.uint32))
    ctx.nc_set(pool[:500], np.arange(500, dtype=np.uint32))
    next_h = 500
    for step in range(30):
        op = int(rng.integers(0, 4))
        if op == 0:
            m = int(rng.integers(1, 400))
            ids = pool[rng.integers(0, 6000, size=m)]
            hs = np.arange(next_h, next_h + m, dtype=np.uint32)
            acc = (rng.random(m) >= 0.3).astype(np.uint8)
            next_h += m
            assert np.array_equal(ctx.nc_insert(ids, hs, acc), model.insert(ids, hs, acc)), step
        elif op == 1:
            m = int(rng.integers(1, 300))
            ids = pool[rng.integers(0, 6000, size=m)]
            assert np.array_equal(ctx.nc_erase(ids), model.erase(ids)), step
        elif op == 2:
            hs = rng.choice(next_h, size=int(rng.integers(1, 200)), replace=False).astype(np.uint32)
            val = (rng.random(hs.shape[0]) >= 0.5).astype(np.uint8)
            ctx.nc_update_accept(hs, val)
            model.update_accept(hs, val)
        else:
            by = (rng.random(int(rng.integers(1, next_h + 1))) >= 0.3).astype(np.uint8)
            ctx.nc_set_accept(by)
            model.set_accept(by)
        check_model(ctx, model, ("sequence", step, op), counts=(8, 14))


# ---- accept bits -------------------------------------------------------------------------------
def test_update_accept_is_stream_ordered(ctx, keysets):
    """nc_update_accept, then _dev lookups on the context's stream, with no synchronise between"""
    import torch
    keys = keysets[4096]
    model = NC.Model()
    model.set(keys)
    ctx.nc_set(keys)
    tg = NC.targets_for(keys, 9)
    rej = np.arange(0, 4096, 2, dtype=np.uint32)
    oh, oc, tp = nodes_dev(ctx, tg, 8)   # (buffers and targets in place)
    ctx.nc_update_accept(rej, 0)
    q = tg.shape[0]
    ctx.nc_nodes_dev(tp.data_ptr(), tp.numel() // 5, q, 8, oh.data_ptr(), oc.data_ptr(), None)
    torch.cuda.synchronize()
    model.update_accept(rej, 0)
    want, wcnt = model.expected(tg, 8)
    assert_rows(oh.cpu().numpy().view(np.uint32), oc.cpu().numpy().view(np.uint32), want, wcnt, "after update")


@pytest.mark.parametrize("m", [257, 65537])
def test_update_accept_many(ctx, keysets, m):
    """m distinct handles with random values in one call over 70,000 keys (more than one block of
    the setter, and 256 blocks and one thread more): every key as a target at count 1 reads its own
    bit first, against the model"""
    keys = keysets[70000]
    rng = np.random.default_rng(m)
    model = NC.Model()
    model.set(keys)
    ctx.nc_set(keys)
    by_handle = (rng.random(70000) < 0.5).astype(np.uint8)
    model.set_accept(by_handle)
    ctx.nc_set_accept(by_handle)
    hs = rng.choice(70000, m, replace=False).astype(np.uint32)
    val = rng.choice([0, 1, 2, 255], m).astype(np.uint8)   # any nonzero byte accepts
    model.update_accept(hs, val)
    ctx.nc_update_accept(hs, val)
    want, wcnt = model.expected(keys, 1)
    got, cnt = ctx.nc_nodes(keys, 1)
    assert_rows(got, cnt, want, wcnt, m)
    by_handle[hs] = val != 0
    assert np.array_equal(got[:, 0] == np.arange(70000, dtype=np.uint32), by_handle != 0)


def test_handle_bound_and_mask_growth(ctx, keysets):
    import opendht_amd
    keys = keysets[65]
    model = NC.Model()
    model.set(keys)
    ctx.nc_set(keys)
    ctx.nc_update_accept([3, 5], 0)
    model.update_accept([3, 5], 0)
    for fn in (lambda: ctx.nc_update_accept([4, NC.MAX_HANDLE], [0, 0]),
               lambda: ctx.nc_insert(O.gen_ids(3, 2), [70, NC.MAX_HANDLE]),
               lambda: ctx.nc_set(keys[:2], [1, NC.MAX_HANDLE])):
        with pytest.raises(opendht_amd.DhtGpuError) as e:   # nothing applied
            fn()
        assert e.value.code == EINVAL
    check_model(ctx, model, "after refused handles")
    far = np.array([NC.MAX_HANDLE - 1, 1 << 20], dtype=np.uint32)   # past the mask's extent: it grows
    ids = O.gen_ids(4, 2)
    assert np.array_equal(ctx.nc_insert(ids, far, [1, 0]), model.insert(ids, far, [1, 0]))
    check_model(ctx, model, "after far handles")
    ctx.nc_update_accept(far, [0, 1])
    model.update_accept(far, [0, 1])
    check_model(ctx, model, "far handles flipped")


def test_insert_accept_leaves_present_keys_alone(ctx, keysets):
    keys = keysets[64]
    model = NC.Model()
    model.set(keys)
    ctx.nc_set(keys)
    ctx.nc_update_accept([0, 1], [0, 1])
    model.update_accept([0, 1], [0, 1])
    ids = np.concatenate([keys[:2], O.gen_ids(6, 2)])
    hs, acc = np.array([0, 1, 100, 101], np.uint32), np.array([1, 0, 0, 1], np.uint8)
    assert np.array_equal(ctx.nc_insert(ids, hs, acc), [0, 0, 1, 1])
    model.insert(ids, hs, acc)
    assert 0 not in model.acc and 1 in model.acc
    check_model(ctx, model, "present keys keep their bits", counts=(32,))


# ---- errors and isolation ----------------------------------------------------------------------
def test_errors():
    import opendht_amd
    with opendht_amd.Context(0) as c:
        tg = O.gen_ids(1, 3)
        for fn in (lambda: c.nc_nodes(tg, 8), lambda: c.nc_size(), lambda: c.nc_export(),
                   lambda: c.nc_insert(tg, [0, 1, 2]), lambda: c.nc_erase(tg),
                   lambda: c.nc_update_accept([0], 1), lambda: c.nc_set_accept([1])):
            with pytest.raises(opendht_amd.DhtGpuError) as e:
                fn()
            assert e.value.code == ENOIDS
        c.nc_set(O.gen_ids(2, 10))
        with pytest.raises(opendht_amd.DhtGpuError) as e:
            c.nc_set(np.concatenate([tg, tg[:1]]))
        assert e.value.code == EUNSORTED
        with pytest.raises(opendht_amd.DhtGpuError) as e:
            c.nc_nodes(tg, 8)
        assert e.value.code == ENOIDS
        c.nc_set(tg)
        for count in (0, 33):
            with pytest.raises(opendht_amd.DhtGpuError) as e:
                c.nc_nodes(tg, count)
            assert e.value.code == EINVAL
        assert c.nc_nodes(np.zeros((0, 20), np.uint8), 8)[0].shape == (0, 8)
        # n + m >= 2^32 - 1: refused before a key or a handle is read
        L, hs = opendht_amd.lib(), np.zeros(3, np.uint32)
        big = 0xFFFFFFFF - c.nc_size()
        assert L.dhtgpu_nc_insert(c._h, opendht_amd._p(tg, opendht_amd._u8p), opendht_amd._p(hs, opendht_amd._u32p),
                                  None, big, None) == ERANGE
        assert L.dhtgpu_nc_insert(c._h, None, None, None, 0, None) == 0 and c.nc_size() == 3


def test_isolation_from_the_other_families(ctx, keysets):
    """the cache mirror, the k-NN id set and the rt table answer as before after nc_* calls"""
    import rtable_cases as RC
    myid, firsts, off, nodes, tg = RC.grown(False)
    keys = keysets[4095]
    ctx.set_ids(keys)
    ctx.cache_set(keys)
    ctx.rt_set(myid, firsts, off, nodes)
    before = (ctx.cache_nodes(tg, 8), ctx.topk(tg, 8), ctx.rt_find_closest(tg, 8))
    ctx.nc_set(keysets[4097])
    ctx.nc_insert(O.gen_ids(12, 70), np.arange(5000, 5070, dtype=np.uint32))
    ctx.nc_erase(keysets[4097][:100])
    ctx.nc_update_accept([1, 2, 3], 0)
    ctx.nc_nodes(tg, 14)
    after = (ctx.cache_nodes(tg, 8), ctx.topk(tg, 8), ctx.rt_find_closest(tg, 8))
    for b, a in zip(before, after):
        assert np.array_equal(b[0], a[0]) and np.array_equal(b[1], a[1])


# ---- the C++11 adapter -------------------------------------------------------------------------
def test_cpp_adapter_resident_cache(tmp_path):
    """dhtgpu::ResidentCache on both dispatch paths against the oracle through insert / erase /
    expiry rounds (tests/cpp/ncache_check.cpp)"""
    import cpp_check
    cpp_check.run(cpp_check.build("ncache", tmp_path), ["--run"], "ncache_check", 120)
