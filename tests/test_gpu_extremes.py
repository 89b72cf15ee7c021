"""GPU parity at the ends of the value ranges (extreme_cases.py; test_extremes_cpu.py shows that each
case reaches its edge): distances equal to DHT_NONE in whole rows of candidates, result indices at
and above 2^31 and up to 0xFFFFFFFE, the keys 00..00 / FF..FF and their neighbours in the
lexicographic families, and resident-search handles up to 2^28 - 1 under both flag bits.  Every
comparison is exact, against the oracle and the families' models.  Marked gpu.

Out of scope: the sub-partitioned K6 route (and dhtgpu_handles_to_indices_dev's mapping), which
needs at least 2^25 ids; test_gpu_subs.py covers it with indices counted from 0.  Of that entry point
only the idx_base range check is tested here."""
import numpy as np
import pytest

import extreme_cases as X
import merge_util as MU
import oracle as O
import srmap_cases as SM
from test_gpu_parity import _ctx_records, check_topk
from test_gpu_srmap import assert_offer, assert_state

pytestmark = pytest.mark.gpu

NONE = X.NONE
EINVAL, ERANGE = -1, -6
FILL = -7


@pytest.fixture(scope="module")
def ctx():
    import opendht_amd
    c = opendht_amd.Context(0)
    yield c
    c.close()


def pack(tg):
    """targets as device word planes: (tensor, stride)"""
    import torch
    import opendht_amd
    dev = torch.device("cuda", 0)
    q = tg.shape[0]
    ts = (q + 63) // 64 * 64
    tp = torch.zeros(5 * ts, dtype=torch.int32, device=dev)
    assert opendht_amd.lib().dhtgpu_pack_dev(torch.from_numpy(tg.reshape(-1)).to(dev).data_ptr(), q, tp.data_ptr(), ts,
                                             None) == 0
    return tp, ts


def dev_rows(fn, c, tg, k, base):
    """the index form of a _dev entry point: (rows, counts)"""
    import torch
    dev = torch.device("cuda", 0)
    q = tg.shape[0]
    tp, ts = pack(tg)
    oi = torch.full((q, k), FILL, dtype=torch.int32, device=dev)
    oc = torch.full((q,), FILL, dtype=torch.int32, device=dev)
    fn(tp.data_ptr(), ts, q, k, oi.data_ptr(), oc.data_ptr(), None, base, c.stream)
    torch.cuda.synchronize()
    return oi.cpu().numpy().view(np.uint32), oc.cpu().numpy().view(np.uint32)


def dev_records(fn, c, tg, k, base):
    """the record form of a _dev entry point: (q, k, 3)"""
    import torch
    dev = torch.device("cuda", 0)
    q = tg.shape[0]
    tp, ts = pack(tg)
    rec = torch.full((q, k, 3), FILL, dtype=torch.int32, device=dev)
    fn(tp.data_ptr(), ts, q, k, None, None, rec.data_ptr(), base, c.stream)
    torch.cuda.synchronize()
    return rec.cpu().numpy().view(np.uint32)


def same_rows(got, want, what):
    bad = np.nonzero((got != want).reshape(got.shape[0], -1).any(axis=1))[0]
    assert bad.size == 0, f"{what}: {bad.size} rows differ, first {bad[:5]}: got {got[bad[0]]} want {want[bad[0]]}"


def every_form(c, ids, tg, k, base, want, wcnt, gidx, what):
    """topk_dev, index_topk_dev and batch_topk_dev at q = 8 (the small-batch kernel) and at every
    target (K6), index form and record form, against oracle rows `want` (context-local) whose
    global index is gidx[local]"""
    wrows = np.where(want == NONE, want, gidx[np.minimum(want, gidx.size - 1)]).astype(np.uint32)
    wrec = X.records_from_rows(ids, want, wcnt, gidx)
    for name, fn in (("topk_dev", c.topk_dev), ("index_topk_dev", c.index_topk_dev), ("batch_topk_dev", c.batch_topk_dev)):
        for q in (8, tg.shape[0]):
            got, cnt = dev_rows(fn, c, tg[:q], k, base)
            assert np.array_equal(cnt, wcnt[:q]), f"{what} {name} q={q}: counts"
            same_rows(got, wrows[:q], f"{what} {name} q={q}")
            same_rows(dev_records(fn, c, tg[:q], k, base), wrec[:q], f"{what} {name} q={q} records")
    same_rows(_ctx_records(c, tg, k, base), wrec, f"{what} batch records")


# ---- A: sentinel distances, flat k-NN ----------------------------------------------------------------------
@pytest.fixture(scope="module")
def far():
    """the far cases and their oracle rows, computed once"""
    out = {}
    for name in X.FAR_SHARED:
        ids, tg, _ = X.far_case(name)
        out[name] = (ids, tg, {k: O.topk(ids, tg, k) for k in X.FAR_KS})
    return out


@pytest.mark.parametrize("k", X.FAR_KS)
@pytest.mark.parametrize("name", list(X.FAR_SHARED))
def test_far_rows_every_path(ctx, far, name, k):
    """2,997 candidates per row at word-0 (far-w0w1: word-0 and word-1) distance 0xFFFFFFFF behind three
    closer ids: K1, K4/K5, KS (8 targets) and K6 (80), index rows and 12-byte records == the oracle."""
    ids, tg, rows = far[name]
    want, wcnt = rows[k]
    check_topk(ctx, ids, tg, k)
    got, cnt = ctx.batch_topk(tg[:8], k)
    assert np.array_equal(cnt, wcnt[:8])
    same_rows(got, want[:8], f"{name} KS")
    every_form(ctx, ids, tg, k, 0, want, wcnt, np.arange(ids.shape[0], dtype=np.uint32), f"{name} k={k}")


@pytest.mark.parametrize("k", X.FAR_KS)
def test_antipode_every_path(ctx, k):
    """n = k: every id is in every row, the last one of rows 2.. at distance 2^160 - 1 (five words of
    0xFFFFFFFF); the batch paths at their own size (KS) and with the targets repeated past 64 (K6)."""
    ids, tg = X.antipode_case(k)
    want, wcnt = O.topk(ids, tg, k)
    check_topk(ctx, ids, tg, k)
    gidx = np.arange(k, dtype=np.uint32)
    every_form(ctx, ids, tg, k, 0, want, wcnt, gidx, f"antipode k={k}")
    rep = -(-80 // tg.shape[0])
    tg80, w80, c80 = np.concatenate([tg] * rep), np.concatenate([want] * rep), np.concatenate([wcnt] * rep)
    got, cnt = ctx.batch_topk(tg80, k)
    assert np.array_equal(cnt, c80)
    same_rows(got, w80, "antipode K6")
    same_rows(_ctx_records(ctx, tg80, k, 0), X.records_from_rows(ids, w80, c80, gidx), "antipode K6 records")


@pytest.mark.parametrize("cap", [256, 4])
@pytest.mark.parametrize("k", X.FAR_KS)
@pytest.mark.parametrize("lists", [2, 3, 8])
def test_far_lists_merge(far, lists, k, cap):
    """K3 alone over far-w0w1 cut into id ranges: every far row's lists end in records {NONE, NONE,
    idx} that tie across lists, so all 40 are listed (cap 4: the every-row settlement runs) and the
    second exchange settles them == the flat top-k."""
    import torch
    import opendht_amd
    ids, tg, rows = far["far-w0w1"]
    want, wcnt = rows[k]
    rec = MU.host_records(ids, X.id_range_bounds(X.FAR_N, lists), tg, k, O)
    tp, ts = pack(tg)
    rd = torch.from_numpy(rec.view(np.int32)).to(torch.device("cuda", 0))
    got, gcnt, nties = MU.merge(opendht_amd.lib(), rd, tp, ts, k, ("host", MU.host_words_fn(ids, rec)), tie_cap=cap)
    assert np.array_equal(gcnt, wcnt)
    same_rows(got, want, f"lists={lists} k={k} cap={cap}")
    assert nties >= X.FAR_ROWS.size


# ---- B: indices at the top of the range -------------------------------------------------------------------
@pytest.fixture(scope="module")
def top():
    ids, tg = X.top_case()
    return ids, tg, {k: O.topk(ids, tg, k) for k in (8, 32)}


@pytest.mark.parametrize("k", [8, 32])
@pytest.mark.parametrize("base", [X.BASE_CROSS, X.BASE_LAST], ids=["cross-2^31", "last-index"])
def test_idx_base_top_of_range(ctx, top, base, k):
    """idx_base 0x7FFFFF00 (indices cross 2^31 inside the set; duplicated ids on both sides: the lower
    unsigned index first) and 0xFFFFFFFF - n (the last id is 0xFFFFFFFE): every _dev entry point, both
    batch routes, index rows and records == the oracle's rows + base, DHT_NONE unchanged."""
    ids, tg, rows = top
    want, wcnt = rows[k]
    ctx.set_ids(ids)
    ctx.index_build()
    every_form(ctx, ids, tg, k, base, want, wcnt, X.add_base(np.arange(X.TOP_N, dtype=np.uint32), base),
               f"base {base:#x} k={k}")


def test_idx_base_under_accept_mask(ctx, top):
    """A mask that rejects a third of the ids: the view's index map + idx_base is kept per base -- base
    0x7FFFFF00, base 0xFFFFFFFF - n, a mask update, both bases again; every entry point and form."""
    ids, tg, _ = top
    k = 8
    gidx = {base: X.add_base(np.arange(X.TOP_N, dtype=np.uint32), base) for base in (X.BASE_CROSS, X.BASE_LAST)}
    ctx.set_ids(ids)
    ctx.set_accept(X.top_mask())
    try:
        for step, mask in enumerate((X.top_mask(), X.top_mask_updated())):
            if step:
                ctx.update_accept(X.TOP_FLIP, np.r_[np.ones(133, np.uint8), np.zeros(X.TOP_FLIP.size - 133, np.uint8)])
            assert ctx.num_accepted == int(mask.sum())
            want, wcnt = X.masked_topk(ids, mask, tg, k)   # rows of the whole set
            for base in (X.BASE_CROSS, X.BASE_LAST):
                every_form(ctx, ids, tg, k, base, want, wcnt, gidx[base], f"mask {step} base {base:#x}")
    finally:
        ctx.set_accept(None)


@pytest.fixture(scope="module")
def shards():
    """the two prefix shards of the stream that ends at global index 0xFFFFFFFE"""
    import opendht_amd
    cs = []
    for p in (0, 1):
        c = opendht_amd.Context(0)
        c.gen_ids_prefix(X.SHARD_SEED, X.SHARD_N, 1, p, start=X.SHARD_START)
        cs.append(c)
    yield cs
    for c in cs:
        c.close()


def tie_words_of(c, rec, k, base):
    """dhtgpu_tie_words_dev over every row of the context's own records: (q, k, 3)"""
    import torch
    dev = torch.device("cuda", 0)
    q = rec.shape[0]
    rd = torch.from_numpy(np.ascontiguousarray(rec).view(np.int32)).to(dev)
    out = torch.full((q, k, 3), FILL, dtype=torch.int32, device=dev)
    c.tie_words_dev(rd.data_ptr(), q, k, base, None, 0, 0, out.data_ptr(), c.stream)
    torch.cuda.synchronize()
    return out.cpu().numpy().view(np.uint32)


def want_tie_words(ids, rec, gidx_to_row):
    w = X.words(ids)
    out = np.full(rec.shape, NONE, np.uint32)
    ok = rec[..., 2] != NONE
    out[ok] = w[gidx_to_row(rec[..., 2][ok].astype(np.int64)), 2:5]
    return out


@pytest.mark.parametrize("k", [8, 32])
def test_prefix_shards_top_of_range(shards, k):
    """Prefix shards of gen_ids_prefix(start = 0xFFFFFFFF - 8192): every global index lies above 2^31, the
    last is 0xFFFFFFFE.  Every kernel of each shard == the oracle over the shard's ids with indices
    start + i; k_tie_words finds every index in the shard's global map (words 2..4 of the named ids);
    the two shards' records merged with the every-row settlement == the flat top-k."""
    import torch
    import opendht_amd
    ids, tg, sel = X.shard_case()
    q = tg.shape[0]
    dev = torch.device("cuda", 0)
    L = opendht_amd.lib()
    rec = torch.empty((2, q, k, 3), dtype=torch.int32, device=dev)
    tp, ts = pack(tg)
    for p, c in enumerate(shards):
        c.set_global_indices(True)
        c.index_build()
        assert c.num_ids == sel[p].size and np.array_equal(c.get_ids(), ids[sel[p]])
        want, wcnt = O.topk(ids[sel[p]], tg, k)
        gidx = X.add_base(sel[p].astype(np.uint32), X.SHARD_START)
        assert gidx.min() > X.TOP
        wrows = np.where(want == NONE, want, gidx[np.minimum(want, gidx.size - 1)]).astype(np.uint32)
        for name, fn in (("scan", c.topk), ("index", c.index_topk), ("batch", c.batch_topk)):
            for n in (8, q):
                got, cnt = fn(tg[:n], k)
                assert np.array_equal(cnt, wcnt[:n]), (p, name, n)
                same_rows(got, wrows[:n], f"shard {p} {name} q={n}")
        every_form(c, ids[sel[p]], tg, k, 0, want, wcnt, gidx, f"shard {p} k={k}")
        r = _ctx_records(c, tg, k, 0)
        same_rows(tie_words_of(c, r, k, 0), want_tie_words(ids, r, lambda g: g - X.SHARD_START), f"shard {p} tie words")
        rec[p] = torch.from_numpy(r.view(np.int32)).to(dev)
    out, cnt, _ = MU.merge(L, rec, tp, ts, k, ("ctx", MU.ctx_words_fn(L, shards, rec, [0, 0], k)), force_all=True)
    want, wcnt = O.topk(ids, tg, k)
    assert np.array_equal(cnt, wcnt)
    same_rows(out, X.add_base(want, X.SHARD_START), "merged shards")


@pytest.mark.parametrize("k", [8, 32])
def test_prefix_shards_local_indices_high_base(shards, k):
    """The same shards with set_global_indices(False) and idx_base: shard 0 at 0xFFFFFFFF - 8192, shard 1
    right behind it (its last id is 0xFFFFFFFE); tie words through idx - base; merged == the flat top-k
    over the two shards' ids in that order."""
    import torch
    import opendht_amd
    ids, tg, sel = X.shard_case()
    q = tg.shape[0]
    dev = torch.device("cuda", 0)
    L = opendht_amd.lib()
    bases = [X.SHARD_START, X.SHARD_START + sel[0].size]
    assert bases[1] + sel[1].size == NONE
    rec = torch.empty((2, q, k, 3), dtype=torch.int32, device=dev)
    tp, ts = pack(tg)
    try:
        for p, c in enumerate(shards):
            c.set_global_indices(False)
            c.index_build()
            mine = ids[sel[p]]
            want, wcnt = O.topk(mine, tg, k)
            got, cnt = c.batch_topk(tg, k)                 # shard-local rows
            assert np.array_equal(cnt, wcnt)
            same_rows(got, want, f"shard {p} local")
            gidx = X.add_base(np.arange(sel[p].size, dtype=np.uint32), bases[p])
            every_form(c, mine, tg, k, bases[p], want, wcnt, gidx, f"shard {p} base {bases[p]:#x}")
            r = _ctx_records(c, tg, k, bases[p])
            same_rows(tie_words_of(c, r, k, bases[p]), want_tie_words(mine, r, lambda g, b=bases[p]: g - b),
                      f"shard {p} tie words")
            rec[p] = torch.from_numpy(r.view(np.int32)).to(dev)
        out, cnt, _ = MU.merge(L, rec, tp, ts, k, ("ctx", MU.ctx_words_fn(L, shards, rec, bases, k)), force_all=True)
    finally:
        for c in shards:
            c.set_global_indices(True)
    want, wcnt = O.topk(np.concatenate([ids[sel[0]], ids[sel[1]]]), tg, k)
    assert np.array_equal(cnt, wcnt)
    same_rows(out, X.add_base(want, X.SHARD_START), "merged shards, local indices + base")


@pytest.mark.parametrize("cap", [256, 4])
@pytest.mark.parametrize("lists,k,seed", X.MERGE_DUP_SHAPES)
def test_merge_raised_indices(lists, k, seed, cap):
    """K3 alone over test_merge_heads_ties_duplicates' lists with every record index raised by 0x7FFFFF00:
    duplicated ids in different lists lie on both sides of 2^31, and the unsigned index decides."""
    import torch
    import opendht_amd
    ids, tg, bounds = X.merge_dup_case(lists, seed)
    rec = MU.host_records(ids, bounds, tg, k, O)
    rec[..., 2] = X.add_base(rec[..., 2], X.BASE_CROSS)
    tp, ts = pack(tg)
    rd = torch.from_numpy(rec.view(np.int32)).to(torch.device("cuda", 0))
    got, gcnt, nties = MU.merge(opendht_amd.lib(), rd, tp, ts, k, ("host", X.raised_words_fn(ids, rec, X.BASE_CROSS)),
                                tie_cap=cap)
    want, wcnt = O.topk(ids, tg, k)
    assert np.array_equal(gcnt, wcnt)
    same_rows(got, X.add_base(want, X.BASE_CROSS), f"lists={lists} cap={cap}")
    assert nties > cap or cap == 256


def _code(f, *a):
    import opendht_amd
    try:
        f(*a)
    except opendht_amd.DhtGpuError as e:
        return e.code
    return 0


@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
def test_idx_base_range_check(masked):
    """idx_base + n <= 0xFFFFFFFF, n = the context's id count (under a mask too: the index space, not the
    view): the last accepted base answers, the first refused one returns DHTGPU_ERANGE from every
    entry point that takes idx_base and leaves the outputs as they were."""
    import torch
    import opendht_amd
    dev = torch.device("cuda", 0)
    ids, tg = X.top_case()
    n, q, k = 1000, 160, 8
    ids = ids[:n]
    tg[0] = ids[n - 1]                                     # (accepted by the mask: 999 % 3 == 0)
    last, first_bad = NONE - n, NONE - n + 1
    tp, ts = pack(tg)
    with opendht_amd.Context(0) as c:
        c.set_ids(ids)
        c.index_build()
        if masked:
            c.set_accept(X.top_mask(n))
        oi = torch.full((q, k), FILL, dtype=torch.int32, device=dev)
        oc = torch.full((q,), FILL, dtype=torch.int32, device=dev)
        rec = torch.full((q, k, 3), FILL, dtype=torch.int32, device=dev)
        words = torch.full((q, k, 3), FILL, dtype=torch.int32, device=dev)
        idx_args = (tp.data_ptr(), ts, q, k, oi.data_ptr(), oc.data_ptr(), None)
        rec_args = (tp.data_ptr(), ts, q, k, None, None, rec.data_ptr())
        for fn in (c.topk_dev, c.index_topk_dev, c.batch_topk_dev):
            for args in (idx_args, rec_args, (tp.data_ptr(), ts, 8) + idx_args[3:]):
                assert _code(fn, *args, first_bad, c.stream) == ERANGE, fn.__name__
                assert _code(fn, *args, NONE, c.stream) == ERANGE, fn.__name__
        held = torch.full((q, k, 3), FILL, dtype=torch.int32, device=dev)
        assert _code(c.tie_words_dev, held.data_ptr(), q, k, first_bad, None, 0, 0, words.data_ptr(), c.stream) == ERANGE
        assert _code(c.handles_to_indices_dev, rec.data_ptr(), q * k, oi.data_ptr(), first_bad, c.stream) == ERANGE
        torch.cuda.synchronize()
        for t in (oi, oc, rec, words):
            assert bool((t == FILL).all()), "a refused call wrote to its outputs"
        # the last accepted base: every call answers (handles_to_indices: no sub-partitioned call has
        # built a handle space on 1,000 ids -- EINVAL, not ERANGE)
        mask = X.top_mask(n) if masked else np.ones(n, np.uint8)
        want, wcnt = X.masked_topk(ids, mask, tg, k)
        every_form(c, ids, tg, k, last, want, wcnt, X.add_base(np.arange(n, dtype=np.uint32), last), "last base")
        r = _ctx_records(c, tg, k, last)
        assert r[0, 0, 2] == 0xFFFFFFFE                    # the last id, at the last index there is
        assert _code(c.tie_words_dev, torch.from_numpy(r.view(np.int32)).to(dev).data_ptr(), q, k, last, None, 0, 0,
                     words.data_ptr(), c.stream) == 0
        torch.cuda.synchronize()
        same_rows(words.cpu().numpy().view(np.uint32), want_tie_words(ids, r, lambda g: g - last), "tie words, last base")
        assert _code(c.handles_to_indices_dev, rec.data_ptr(), q * k, oi.data_ptr(), last, c.stream) == EINVAL


# ---- C: boundary keys, lexicographic families ---------------------------------------------------------------
@pytest.fixture(scope="module")
def boundary():
    keys, tg = X.boundary_keys(), X.boundary_targets()
    masks = {"every": np.ones(keys.shape[0], np.uint8), "ends": X.ends_mask(keys)}
    want = {(m, count): [O.cached_nodes(keys, acc, t, count) for t in tg] for m, acc in masks.items()
            for count in X.WALK_COUNTS}
    return keys, tg, masks, want


@pytest.mark.parametrize("mask", ["every", "ends"])
def test_cached_nodes_boundary_keys(ctx, boundary, mask):
    """k_cached over a sorted upload: targets 00..00 and FF..FF (lower_bound 0 and n - 1), their
    neighbours, every key accepted / only the two end keys (the walk runs off one side at once and
    crosses the whole array on the other) == O.cached_nodes."""
    keys, tg, masks, want = boundary
    ctx.set_ids(keys)
    for count in X.WALK_COUNTS:
        got, cnt = ctx.cached_nodes(tg, count, masks[mask])
        for qi in range(tg.shape[0]):
            w = want[(mask, count)][qi]
            assert cnt[qi] == len(w) and list(got[qi, :cnt[qi]]) == list(w), (count, qi)
            assert np.all(got[qi, cnt[qi]:] == NONE)


@pytest.mark.parametrize("mask", ["every", "ends"])
def test_cache_mirror_boundary_keys(ctx, boundary, mask):
    """the same walks over a shuffled upload (cache_set sorts on the device; indices in caller order)"""
    keys, tg, masks, want = boundary
    sh, order = X.shuffled(keys, 78)
    ctx.cache_set(sh)
    assert np.array_equal(ctx.cache_sorted(), order.astype(np.uint32))
    acc = np.zeros(keys.shape[0], np.uint8)
    acc[order] = masks[mask]                               # caller order
    for count in X.WALK_COUNTS:
        got, cnt = ctx.cache_nodes(tg, count, acc)
        for qi in range(tg.shape[0]):
            w = want[(mask, count)][qi]
            assert cnt[qi] == len(w) and list(got[qi, :cnt[qi]]) == list(order[w]), (count, qi)


@pytest.mark.parametrize("name", X.SORT_CASES)
def test_cache_sorted_boundary_digits(ctx, name):
    """The device radix sort where its 64-bit shortcut fails: one tile and one key past it, digits 0 and
    255 only in the eight high passes with 00..00 and FF..FF among the keys; keys that differ in word 4
    only (one digit in 16 passes) == np.lexsort."""
    keys = X.sort_case(name)
    ctx.cache_set(keys)
    assert np.array_equal(ctx.cache_sorted(), np.lexsort(keys.T[::-1]).astype(np.uint32))


@pytest.mark.parametrize("name", list(X.TABLE_MYIDS))
def test_routing_table_boundary_keys(ctx, name):
    """findClosestNodes and classify over the table grown from the boundary key set by myid = FF..FF and
    00..00: findBucket's first and last bucket, targets at both ends == O.find_closest / O.classify."""
    myid, firsts, off, nodes = X.table_case(name)
    tg = X.boundary_targets()
    good = np.ones(nodes.shape[0], np.uint8)
    good[::5] = 0
    for count in X.CLOSEST_COUNTS:
        got, cnt = ctx.find_closest(firsts, off, nodes, good, tg, count)
        for qi in range(tg.shape[0]):
            w = O.find_closest(firsts, off, nodes, good, tg[qi], count)
            assert cnt[qi] == len(w) and list(got[qi, :cnt[qi]]) == list(w), (count, qi)
            assert np.all(got[qi, cnt[qi]:] == NONE)
    keys = X.boundary_keys()
    ctx.set_ids(keys)
    b, hist = ctx.classify(firsts, myid)
    wb, wh = O.classify(firsts, myid, keys)
    assert np.array_equal(hist, wh) and np.array_equal(b, wb)


# ---- D: top-of-range handles, resident searches ----------------------------------------------------------------
@pytest.mark.parametrize("name", ["insert103", "refill206", "shape404"])
def test_top_handles(ctx, name):
    """An insert script, a refill script and an offer script with every handle h as 2^28 - 1 - h, then
    handle 2^28 - 1 itself stored with both flags (the word 0x3FFFFFFF) and its rows rewritten: sr_lists,
    sr_status and the srm_offer results == the model after every step."""
    script = dict(X.handle_scripts())[name]
    model = SM.Model()
    try:
        for j, step in enumerate(script):
            want, got = X.run_step(step, model, ctx)
            what = f"{name} step {j} {step[0]}"
            if step[0] == "offer":
                assert_offer(got, want, what)
            elif want is not None:
                assert np.array_equal(got, want), f"{what}: results differ"
            if model.slots and step[0] not in ("nc_set", "nc_accept"):
                assert_state(ctx, model, what)
        rows, flags, lens = ctx.sr_lists(np.arange(len(model.slots), dtype=np.uint32))
        assert np.any((rows == X.HANDLE_TOP) & (flags == 3))
    finally:
        ctx.sr_reset(1)   # drops the 256 MB state array
