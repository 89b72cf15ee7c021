"""GPU parity of keys-to-handles over the resident NodeCache (dhtgpu_ncr_*, opendht_amd/csrc/ncresolve.hip):
the lane-group find, get_nodes and extract against the model of ncresolve_cases.py (the sequential
loops of NodeMap::getNode over a dict).  Every comparison is exact.  Marked gpu: run on the MI355X box."""

import numpy as np
import pytest

import ncache_cases as NC
import ncresolve_cases as NR
import oracle as O

pytestmark = pytest.mark.gpu

NONE = NC.NONE
EINVAL, ENOIDS, ERANGE = -1, -4, -6


@pytest.fixture(scope="module")
def ctx():
    import opendht_amd
    c = opendht_amd.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def keysets():
    """one random key set per size, shared and left unchanged"""
    sizes = set(NR.FIND_SIZES) | set(NR.GET_SIZES)
    return {n: O.gen_ids(1700 + n, n) if n else np.zeros((0, 20), np.uint8) for n in sizes}


def fresh_model(ctx, keys, seed=3):
    """the mirror and its model over `keys`, handles a permutation of an offset range, one in five rejected"""
    n = keys.shape[0]
    rng = np.random.default_rng(seed)
    handles = (rng.permutation(n) + 11).astype(np.uint32)
    model = NR.Model()
    model.nc.set(keys, handles)
    ctx.nc_set(keys, handles)
    rej = handles[rng.random(n) < 0.2]
    if rej.size:
        model.nc.update_accept(rej, 0)
        ctx.nc_update_accept(rej, 0)
    return model


def assert_mirror(ctx, model, what, count=8):
    """the mirror equals the model: size, export (keys and handles), and a lookup batch under the accept bits"""
    keys, handles = model.nc.sorted()
    assert ctx.nc_size() == keys.shape[0], what
    gk, gh = ctx.nc_export()
    assert np.array_equal(gk, keys), f"{what}: exported keys"
    assert np.array_equal(gh, handles), f"{what}: exported handles"
    tg = NC.targets_for(keys, 3)
    want, wcnt = model.nc.expected(tg, count)
    got, cnt = ctx.nc_nodes(tg, count)
    assert np.array_equal(cnt, wcnt) and np.array_equal(got, want), f"{what}: nc_nodes"


def assert_find(ctx, model, probes, what):
    want_h, want_a = model.find(probes)
    h, a = ctx.ncr_find(probes, accept=True)
    bad = np.nonzero(h != want_h)[0]
    assert bad.size == 0, f"{what}: {bad.size} handles differ, first at {bad[:5]}: got {h[bad[:5]]} want {want_h[bad[:5]]}"
    assert np.array_equal(a, want_a), f"{what}: accept bytes"
    assert np.array_equal(ctx.ncr_find(probes), want_h), f"{what}: without accept bytes"


def dev_i32(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).to(torch.device("cuda", 0))


# ---- find ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", NR.FIND_SIZES)
def test_find_sizes_and_batches(ctx, keysets, n):
    """every size at which a G-lane descent changes depth, batches on both sides of the G switch:
    present keys, keys +- 1, below the minimum, above the maximum, all-zero, all-ones, repeats"""
    keys = keysets[n]
    model = fresh_model(ctx, keys)
    for m in NR.FIND_BATCHES + (None,):
        assert_find(ctx, model, NR.find_probes(keys, m, 7 + (m or 0)), f"n={n} m={m}")


def test_find_clustered_keys(ctx):
    """keys equal in words 0..3: present and absent probes differ in word 4 only (a word-0 or 64-bit
    compare fails here), through both instantiations"""
    keys, probes = NR.clustered_probes()
    model = fresh_model(ctx, keys)
    want_h, _ = model.find(probes)
    assert (want_h == NONE).any() and (want_h != NONE).any()
    assert_find(ctx, model, probes, "clustered, wide")
    reps = NR.WIDE_MAX_BATCH // probes.shape[0] + 1
    assert_find(ctx, model, np.ascontiguousarray(np.tile(probes, (reps, 1))), "clustered, narrow")


def test_find_accept_follows_update_accept(ctx, keysets):
    """out_accept is the handle's current bit: after nc_update_accept, and for a handle the mask had
    to grow for"""
    keys = keysets[4096]
    model = fresh_model(ctx, keys)
    far = O.gen_ids(5151, 2)
    big = np.array([(1 << 20) + 5, (1 << 21) + 77], dtype=np.uint32)   # past the mask's first extent
    model.nc.insert(far, big, [1, 0])
    ctx.nc_insert(far, big, [1, 0])
    probes = np.concatenate([keys[:300], far, O.gen_ids(5152, 10)])
    assert_find(ctx, model, probes, "after insert")
    hs = np.concatenate([model.find(keys[:300:3])[0], big])
    val = (np.arange(hs.shape[0]) % 2).astype(np.uint8)
    model.nc.update_accept(hs, val)
    ctx.nc_update_accept(hs, val)
    assert_find(ctx, model, probes, "after update_accept")
    past = np.array([(1 << 24) + 3], dtype=np.uint32)   # no key holds it: the mask grows, the answers stay
    ctx.nc_update_accept(past, 1)
    assert_find(ctx, model, probes, "after a mask growth")


def test_find_dev_stride_streams_sentinels(ctx, keysets):
    """the _dev form: a stride > m, two calls back to back on a side stream read after one
    synchronise, the words behind the outputs untouched; with and without accept bytes"""
    import torch
    dev = torch.device("cuda", 0)
    keys = keysets[70000]
    model = fresh_model(ctx, keys)
    side = torch.cuda.Stream(device=dev)
    runs = []
    with torch.cuda.stream(side):
        for m, want_acc in ((257, True), (NR.WIDE_MAX_BATCH + 1, False)):
            probes = NR.find_probes(keys, m, 31 + m)
            stride = m + 5
            d_p = dev_i32(NR.id_planes(probes, stride))
            d_h = torch.full((m + 16,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
            d_a = torch.full((m + 16,), 0x5A, dtype=torch.uint8, device=dev)
            runs.append((m, probes, want_acc, d_p, d_h, d_a, stride))
        torch.cuda.synchronize()   # the uploads, and the mirror's accept bits (ordered on the context's stream)
        for m, probes, want_acc, d_p, d_h, d_a, stride in runs:
            ctx.ncr_find_dev(d_p.data_ptr(), stride, m, d_h.data_ptr(), d_a.data_ptr() if want_acc else None,
                             side.cuda_stream)
        side.synchronize()
    for m, probes, want_acc, d_p, d_h, d_a, stride in runs:
        want_h, want_a = model.find(probes)
        h = d_h.cpu().numpy().view(np.uint32)
        a = d_a.cpu().numpy()
        assert np.array_equal(h[:m], want_h), f"m={m}"
        assert (h[m:] == 0x5A5A5A5A).all(), f"m={m}: words behind out_handle"
        if want_acc:
            assert np.array_equal(a[:m], want_a) and (a[m:] == 0x5A).all(), f"m={m}: accept bytes"
        else:
            assert (a == 0x5A).all(), f"m={m}: out_accept was not asked for"


def test_find_dev_feeds_sr_insert_dev():
    """a learned id reaches the searches with no host lookup: the handles ncr_find_dev writes are the
    ins_handle array dhtgpu_sr_insert_dev reads, on one stream with no synchronise between; the
    lists equal the model's"""
    import opendht_amd
    import rsearch_cases as RS
    import torch
    dev = torch.device("cuda", 0)
    nkeys, nslots, per = 3000, 24, 9
    keys = O.gen_ids(1801, nkeys)
    handles = (np.random.default_rng(4).permutation(nkeys) + 100).astype(np.uint32)
    targets = O.gen_ids(1802, nslots)
    slots = np.arange(nslots, dtype=np.uint32)
    pick = np.random.default_rng(5).choice(nkeys, size=nslots * per, replace=False)
    ids, want_handles = keys[pick], handles[pick]
    off = RS.csr(np.full(nslots, per))
    model = RS.Model()
    model.reset(nslots)
    model.open(slots, targets)
    model.insert(slots, off, want_handles, ids)
    with opendht_amd.Context(0) as c:
        c.nc_set(keys, handles)
        c.sr_reset(nslots)
        c.sr_open(slots, targets)
        tot = nslots * per
        stride = tot + 3
        d_p = dev_i32(NR.id_planes(ids, stride))
        d_slots, d_off = dev_i32(slots), torch.from_numpy(off.view(np.int64)).to(dev)
        d_h = torch.zeros(tot, dtype=torch.int32, device=dev)
        d_res = torch.zeros(tot, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        c.ncr_find_dev(d_p.data_ptr(), stride, tot, d_h.data_ptr(), None, None)
        c.sr_insert_dev(d_slots.data_ptr(), nslots, d_off.data_ptr(), d_h.data_ptr(), d_p.data_ptr(), stride, None,
                        d_res.data_ptr(), None)
        torch.cuda.synchronize()
        assert np.array_equal(d_h.cpu().numpy().view(np.uint32), want_handles)
        got = c.sr_lists(slots)
        for g, w, nm in zip(got, model.lists(slots), ("rows", "flags", "lens")):
            assert np.array_equal(g, w), nm


# ---- get_nodes -----------------------------------------------------------------------------------
def run_get_nodes(ctx, model, ids, free, accept, what):
    want = model.get_nodes(ids, free, accept)
    h, new, used = ctx.ncr_get_nodes(ids, free, accept)
    assert used == want[2], f"{what}: out_used {used} want {want[2]}"
    assert np.array_equal(new, want[1]), f"{what}: out_new"
    assert np.array_equal(h, want[0]), f"{what}: out_handle"
    return h, new, used


@pytest.mark.parametrize("n", NR.GET_SIZES)
def test_get_nodes_batches(ctx, keysets, n):
    """fresh keys, present keys, one key twice, the smallest and the largest key, at every batch
    size, under a shuffled non-contiguous free list and accept bytes that reject some new keys"""
    model = fresh_model(ctx, keysets[n])
    for m in NR.GET_BATCHES:
        ids, _, accept = NC.mutation_batch(model.nc, m, 40 + m, 0)
        free = NR.free_list(model, m + 2, 50 + m)
        run_get_nodes(ctx, model, ids, free, accept, f"n={n} m={m}")
        assert_mirror(ctx, model, f"n={n} after m={m}")
    ids, _, _ = NC.mutation_batch(model.nc, 65, 99, 0)
    run_get_nodes(ctx, model, ids, NR.free_list(model, 70, 98), None, f"n={n}: accept NULL")
    assert_mirror(ctx, model, f"n={n} after accept NULL")


def test_get_nodes_all_present_changes_nothing(ctx, keysets):
    keys = keysets[4096]
    model = fresh_model(ctx, keys)
    before = ctx.nc_export()
    ids = np.ascontiguousarray(keys[np.random.default_rng(8).integers(0, 4096, size=300)])
    h, new, used = run_get_nodes(ctx, model, ids, np.array([900000], np.uint32), np.zeros(300, np.uint8), "all present")
    assert used == 0 and not new.any() and (h != NONE).all()
    after = ctx.nc_export()
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    assert_mirror(ctx, model, "all present")   # (the accept bytes of present keys are ignored)
    h, new, used = ctx.ncr_get_nodes(ids, np.zeros(0, np.uint32))   # no free handle is needed
    assert used == 0 and np.array_equal(h, model.find(ids)[0])


def test_get_nodes_one_key_many_times(ctx, keysets):
    """one absent key 4,097 times and one other key: every repeat gets the run's first handle (found
    by a lower bound in the sorted batch, not by walking back)"""
    model = fresh_model(ctx, keysets[4096])
    k = O.gen_ids(1901, 2)
    ids = np.ascontiguousarray(np.concatenate([np.tile(k[0], (2000, 1)), k[1:2], np.tile(k[0], (2097, 1))]))
    accept = np.ones(4098, np.uint8)
    accept[0] = 0   # the first appearance decides
    h, new, used = run_get_nodes(ctx, model, ids, np.array([777777, 555555, 3], np.uint32), accept, "run head")
    assert used == 2 and h[0] == 777777 and h[2000] == 555555 and (np.delete(h, 2000) == 777777).all()
    assert_mirror(ctx, model, "run head")


def test_get_nodes_exhaustion_applies_nothing(ctx, keysets):
    model = fresh_model(ctx, keysets[4096])
    ids, _, accept = NC.mutation_batch(model.nc, 257, 61, 0)
    with pytest.raises(NR.Exhausted) as e:
        model.get_nodes(ids, [], accept)
    needed = e.value.needed
    free = NR.free_list(model, needed, 62)
    tg = NC.targets_for(model.nc.sorted()[0], 3)
    before = ctx.nc_export() + ctx.nc_nodes(tg, 14)
    import opendht_amd
    with pytest.raises(opendht_amd.DhtGpuError) as ge:
        ctx.ncr_get_nodes(ids, free[: needed - 1], accept)
    assert ge.value.code == ERANGE and ge.value.needed == needed
    after = ctx.nc_export() + ctx.nc_nodes(tg, 14)
    for b, a in zip(before, after):
        assert b.tobytes() == a.tobytes()
    assert_mirror(ctx, model, "after ERANGE")
    run_get_nodes(ctx, model, ids, free, accept, "the retry")
    assert_mirror(ctx, model, "after the retry")


def test_get_nodes_equals_nc_insert_with_its_handles(ctx, keysets):
    """a second context given nc_insert with the handles reported here exports the same mirror"""
    import opendht_amd
    keys = keysets[4096]
    model = fresh_model(ctx, keys, seed=12)
    ids, _, accept = NC.mutation_batch(model.nc, 4097, 71, 0)
    h, new, _ = run_get_nodes(ctx, model, ids, NR.free_list(model, 4097, 72), accept, "first context")
    with opendht_amd.Context(0) as other:
        fresh_model(other, keys, seed=12)
        assert np.array_equal(other.nc_insert(ids, h, accept), new)
        for a, b in zip(ctx.nc_export(), other.nc_export()):
            assert np.array_equal(a, b)
        tg = NC.targets_for(model.nc.sorted()[0], 3)
        for a, b in zip(ctx.nc_nodes(tg, 14), other.nc_nodes(tg, 14)):
            assert np.array_equal(a, b)


# ---- extract -------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 64, 4097, 70000])
def test_extract_and_reuse(ctx, keysets, n):
    """the freed handles match the model (NONE for repeats and absent keys), accept bits stay, and a
    following get_nodes takes the freed handles"""
    keys = keysets[n]
    model = fresh_model(ctx, keys)
    rng = np.random.default_rng(n)
    pick = keys[rng.choice(n, size=min(n, 300), replace=False)]
    ids = np.ascontiguousarray(np.concatenate([pick, O.gen_ids(2001, 20), pick[:7], keys[:1], keys[-1:]]))
    ids = ids[rng.permutation(ids.shape[0])]
    want = model.extract(ids)
    got = ctx.ncr_extract(ids)
    assert np.array_equal(got, want)
    assert_mirror(ctx, model, f"n={n} after extract")
    freed = got[got != NONE]
    ids2 = O.gen_ids(2002, freed.shape[0] + 1)[:-1] if freed.shape[0] else O.gen_ids(2002, 1)[:0]
    if ids2.shape[0]:
        h, new, used = run_get_nodes(ctx, model, ids2, freed[::-1], None, f"n={n} reuse")
        assert used == freed.shape[0] and np.array_equal(h, freed[::-1])
        assert_mirror(ctx, model, f"n={n} after reuse")


# ---- errors and isolation ------------------------------------------------------------------------
def test_errors():
    import ctypes
    import opendht_amd
    L = opendht_amd.lib()
    ids = O.gen_ids(2101, 4)
    free = np.array([5, 6, 7, 8], np.uint32)
    with opendht_amd.Context(0) as c:
        for call in (lambda: c.ncr_find(ids), lambda: c.ncr_get_nodes(ids, free), lambda: c.ncr_extract(ids)):
            with pytest.raises(opendht_amd.DhtGpuError) as e:
                call()
            assert e.value.code == ENOIDS
        c.nc_set(ids[:2])
        u8 = ids.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))
        out = np.zeros(4, np.uint32)
        o32 = out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))
        f32 = free.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))
        assert L.dhtgpu_ncr_find(c._h, None, 4, o32, None) == EINVAL
        assert L.dhtgpu_ncr_find(c._h, u8, 4, None, None) == EINVAL
        assert L.dhtgpu_ncr_find_dev(c._h, None, 4, 4, None, None, None) == EINVAL
        assert L.dhtgpu_ncr_get_nodes(c._h, u8, 4, f32, 4, None, None, None, None) == EINVAL
        assert L.dhtgpu_ncr_get_nodes(c._h, u8, 4, None, 4, None, o32, None, None) == EINVAL
        assert L.dhtgpu_ncr_extract(c._h, u8, 4, None) == EINVAL
        bad = np.array([5, NC.MAX_HANDLE, 7, 8], np.uint32)
        with pytest.raises(opendht_amd.DhtGpuError) as e:
            c.ncr_get_nodes(ids, bad)
        assert e.value.code == EINVAL and c.nc_size() == 2
        # n + m >= 2^32 - 1, as in nc_insert (before any array is read)
        assert L.dhtgpu_ncr_get_nodes(c._h, u8, 0xFFFFFFFD, f32, 4, None, o32, None, None) == ERANGE and c.nc_size() == 2
        # m == 0: a no-op
        assert L.dhtgpu_ncr_find(c._h, None, 0, None, None) == 0
        assert L.dhtgpu_ncr_find_dev(c._h, None, 0, 0, None, None, None) == 0
        assert L.dhtgpu_ncr_get_nodes(c._h, None, 0, None, 0, None, None, None, None) == 0
        assert L.dhtgpu_ncr_extract(c._h, None, 0, None) == 0
        assert c.nc_size() == 2
        h, new, used = c.ncr_get_nodes(ids, free)   # nullable outputs: through the binding all are set; raw:
        assert used == 2 and list(new) == [0, 0, 1, 1] and list(h) == [0, 1, 5, 6]
        assert L.dhtgpu_ncr_get_nodes(c._h, u8, 4, f32, 4, None, o32, None, None) == 0 and list(out) == [0, 1, 5, 6]


def test_isolation_from_the_table_and_the_searches(ctx, keysets):
    """a resident table's reply bytes and a search's rows are the same before and after a get_nodes /
    extract pair on the same context"""
    import rtable_cases as RC
    myid, firsts, off, nodes, tg = RC.grown(False)
    keys = keysets[4096]
    model = fresh_model(ctx, keys)
    tails = np.random.default_rng(6).integers(0, 256, size=(nodes.shape[0], 6), dtype=np.uint8)
    ctx.rt_set(myid, firsts, off, nodes, tails, 4)
    slots = np.arange(6, dtype=np.uint32)
    ctx.sr_reset(6)
    ctx.sr_open(slots, O.gen_ids(2201, 6))
    ctx.sr_refill(slots, 14)
    def state():
        blob, ln = ctx.rt_reply(tg)
        return [bytes(r[:k]) for r, k in zip(blob, ln)], ctx.sr_lists(slots)

    before = state()
    ids = O.gen_ids(2202, 300)
    h, _, _ = run_get_nodes(ctx, model, ids, NR.free_list(model, 300, 5), None, "isolation")
    assert np.array_equal(ctx.ncr_extract(ids), h)
    after = state()
    assert before[0] == after[0] and any(before[0])
    for b, a in zip(before[1], after[1]):
        assert np.array_equal(b, a)
    assert before[1][2].any()   # the searches do hold nodes


# ---- the C++11 adapter -------------------------------------------------------------------------
def test_cpp_adapter_get_node_batch(tmp_path):
    """dhtgpu::ResidentCache::getNodeBatch / slotsOfBatch / noteErase rounds against std::map, the
    mirror exported and compared, the retry on too few handles (tests/cpp/ncresolve_check.cpp)"""
    import cpp_check
    cpp_check.run(cpp_check.build("ncresolve", tmp_path), ["--run"], "ncresolve_check", 120)
