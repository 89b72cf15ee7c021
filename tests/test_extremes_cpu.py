"""extreme_cases.py reaches the edges it is named for (no GPU): every case is checked against the
oracle's own rows and the families' models, so that test_gpu_extremes.py compares the library at
inputs that really sit at the ends of the ranges.  Each assertion fails when the crafted part of
its case is taken away (the last test does that for the k-NN cases)."""
import numpy as np
import pytest

import extreme_cases as X
import merge_util as MU
import ncache_cases as NC
import oracle as O
import srmap_cases as SM

NONE = X.NONE


def dist_words(ids, tg, rows):
    """(q, k, 5) distance words of oracle rows (NONE rows: garbage, mask with rows != NONE)"""
    return X.words(ids)[np.minimum(rows, ids.shape[0] - 1).astype(np.int64)] ^ X.words(tg)[:, None, :]


# ---- A ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(X.FAR_SHARED))
def test_far_rows_end_at_the_sentinel(name):
    ids, tg, cluster = X.far_case(name)
    nw = len(X.FAR_SHARED[name])
    assert ids.shape[0] == X.FAR_N and tg.shape[0] == X.FAR_Q and cluster.sum() == X.FAR_N - 3
    # the cluster's distance to every complemented target is the sentinel in the shared words
    d = X.words(ids[cluster])[None, :, :nw] ^ X.words(tg[X.FAR_ROWS])[:, None, :nw]
    assert np.all(d == NONE)
    if name == "far-w0w1":   # ... and so are the id words the 12-byte records carry
        assert np.all(X.words(ids[cluster])[:, :2] == NONE)
    for k in X.FAR_KS:
        rows, cnt = O.topk(ids, tg, k)
        assert np.all(cnt == k)
        far = rows[X.FAR_ROWS]
        assert np.array_equal(np.sort(far[:, :3], axis=1), np.tile(np.sort(X.FAR_FREE), (40, 1)))
        assert np.all(cluster[far[:, 3:]])                     # places 4..k: cluster ids
        assert np.all(cluster[far[:, 7]])                      # the 8th place
        dw = dist_words(ids, tg, rows)[X.FAR_ROWS]
        assert np.all(dw[:, 3:, :nw] == NONE)                  # the k-th distance equals the sentinel
        assert np.all(dw[:, :3, 0] != NONE)
        # rows 40..59 tie at distance 0 on the shared words; no other row meets the sentinel
        assert np.all(dist_words(ids, tg, rows)[40:60, :, :nw] == 0)
        assert not np.any(dist_words(ids, tg, rows)[40:, :, 0] == NONE)


@pytest.mark.parametrize("k", X.FAR_KS)
def test_antipode_rows_end_at_full_distance(k):
    ids, tg = X.antipode_case(k)
    assert ids.shape[0] == k and tg.shape[0] == k + 2
    rows, cnt = O.topk(ids, tg, k)
    assert np.all(cnt == k)
    for i in range(k):     # the complement of id i: id i last, every distance word the sentinel
        assert rows[2 + i, k - 1] == i
        assert np.all(X.words(ids[i:i + 1]) ^ X.words(tg[2 + i:3 + i]) == NONE)
    assert rows[0, 0] == 0 and rows[0, k - 1] == 1 and rows[1, 0] == 1 and rows[1, k - 1] == 0
    assert rows[0, 1] == 2                                     # 00..01 next to 00..00
    assert {bytes(x) for x in ids[:4]} == {bytes(20), b"\xff" * 20, bytes(19) + b"\x01", b"\x80" + bytes(19)}


def test_far_batches_take_both_batch_routes():
    """8 targets: the small-batch kernel; 80: K6 (past its bound of 64)"""
    import opendht_amd
    for k in X.FAR_KS:
        assert opendht_amd.batch_plan(X.FAR_N, 8, k)["route"] == opendht_amd.ROUTE_KS
        assert opendht_amd.batch_plan(X.FAR_N, 64, k)["route"] == opendht_amd.ROUTE_KS
        assert opendht_amd.batch_plan(X.FAR_N, X.FAR_Q, k)["route"] == opendht_amd.ROUTE_K6
        assert opendht_amd.batch_plan(X.TOP_N, 160, k)["route"] == opendht_amd.ROUTE_K6
        assert opendht_amd.batch_plan(k, 80, k)["route"] == opendht_amd.ROUTE_K6


@pytest.mark.parametrize("lists", [2, 3, 8])
def test_far_lists_tie_in_every_far_row(lists):
    """cut into id ranges, every list's records of a far row end in cluster ids, equal in both
    record words across lists: K3 cannot order them without the second exchange"""
    ids, tg, cluster = X.far_case("far-w0w1")
    bounds = X.id_range_bounds(X.FAR_N, lists)
    for k in X.FAR_KS:
        rec = MU.host_records(ids, bounds, tg, k, O)
        for r in X.FAR_ROWS:
            holders = [j for j in range(lists) if np.any((rec[j, r, :, 2] != NONE) & (rec[j, r, :, 0] == NONE)
                                                         & (rec[j, r, :, 1] == NONE))]
            assert len(holders) >= 2


# ---- B ----------------------------------------------------------------------------------------------
def test_top_indices_cross_2p31_and_reach_the_last_index():
    ids, tg = X.top_case()
    assert ids.shape[0] == X.TOP_N and tg.shape[0] == 160
    a, b, m = X.TOP_DUP
    assert len({bytes(x) for x in ids}) == X.TOP_N - m
    assert X.BASE_CROSS + X.TOP_N > X.TOP and X.BASE_CROSS < X.TOP
    assert X.BASE_LAST + X.TOP_N - 1 == 0xFFFFFFFE
    for q in (8, 160):
        rows, cnt = O.topk(ids, tg[:q], 8)
        g = X.add_base(rows, X.BASE_CROSS)
        assert np.any((g < X.TOP).any(axis=1) & (g >= X.TOP).any(axis=1))
        assert np.any(X.add_base(rows, X.BASE_LAST) == 0xFFFFFFFE)
        # a duplicated pair on both sides of 2^31 in one row: the copy below 2^31 comes first, which a
        # signed compare of the indices would turn around
        pairs = 0
        for i in range(q):
            if rows[i, 0] + (b - a) == rows[i, 1] and g[i, 0] < X.TOP <= g[i, 1]:
                assert np.array_equal(ids[rows[i, 0]], ids[rows[i, 1]])
                assert np.int32(g[i, 1]) < np.int32(g[i, 0])
                pairs += 1
        assert pairs >= 4
    assert not np.any(X.add_base(rows, X.BASE_LAST) == NONE)


def test_top_mask_rejects_a_third_and_changes():
    ids, tg = X.top_case()
    m0, m1 = X.top_mask(), X.top_mask_updated()
    assert abs(int(m0.sum()) - 2 * X.TOP_N // 3) <= 1
    assert np.any(m0 & ~m1 & 1) and np.any(m1 & ~m0 & 1)
    r0, _ = X.masked_topk(ids, m0, tg, 8)
    r1, _ = X.masked_topk(ids, m1, tg, 8)
    full, _ = O.topk(ids, tg, 8)
    assert np.any(r0 != full) and np.any(r0 != r1)
    assert np.all(m0[r0] == 1) and np.all(m1[r1] == 1)
    g = X.add_base(r0, X.BASE_CROSS)
    assert np.any((g < X.TOP).any(axis=1) & (g >= X.TOP).any(axis=1))


def test_shard_indices_lie_above_2p31():
    ids, tg, sel = X.shard_case()
    assert X.SHARD_START > X.TOP and X.SHARD_START + X.SHARD_N - 1 == 0xFFFFFFFE
    assert sel[0].size + sel[1].size == X.SHARD_N and min(sel[0].size, sel[1].size) > 3000
    rows, _ = O.topk(ids, tg, 8)
    assert np.any(X.add_base(rows, X.SHARD_START) == 0xFFFFFFFE)
    assert np.any(rows == 0)


@pytest.mark.parametrize("lists,k,seed", X.MERGE_DUP_SHAPES)
def test_raised_duplicates_straddle_2p31_across_lists(lists, k, seed):
    ids, tg, bounds = X.merge_dup_case(lists, seed)
    rec = MU.host_records(ids, bounds, tg, k, O)
    low, high = {}, {}
    for j in range(lists):
        g = rec[j, ..., 2]
        for x in np.unique(g[g != NONE]):
            (low if int(x) + X.BASE_CROSS < X.TOP else high).setdefault(bytes(ids[x]), set()).add(j)
    both = [i for i in low if i in high and (high[i] - low[i])]
    assert both, "a duplicated id below 2^31 in one list and above it in another"
    want, _ = O.topk(ids, tg, k)
    g = X.add_base(want, X.BASE_CROSS)
    hit = [(i, r) for i in range(tg.shape[0]) for r in range(k - 1)
           if want[i, r + 1] != NONE and np.array_equal(ids[want[i, r]], ids[want[i, r + 1]]) and g[i, r] < X.TOP <= g[i, r + 1]]
    assert hit, "a final row that holds both copies, ordered by the unsigned index"


# ---- C ----------------------------------------------------------------------------------------------
def test_boundary_walks_reach_both_ends():
    keys, tg = X.boundary_keys(), X.boundary_targets()
    n = keys.shape[0]
    assert n == 506 and len({bytes(k) for k in keys}) == n and tg.shape[0] == 6 + 8 + 20
    assert np.array_equal(keys[0], X.BOUNDARY[0]) and np.array_equal(keys[1], X.BOUNDARY[1])
    assert np.array_equal(keys[-1], X.BOUNDARY[5]) and np.array_equal(keys[-2], X.BOUNDARY[4])
    ints = [NC.key_int(k) for k in keys]
    lb = [int(np.searchsorted(np.array(ints, dtype=object), NC.key_int(t))) for t in tg]
    assert 0 in lb and n - 1 in lb and n - 2 in lb and 1 in lb
    every = np.ones(n, np.uint8)
    ends = X.ends_mask(keys)
    for t in tg:
        assert list(O.cached_nodes(keys, ends, t, 14)) in ([0, n - 1], [n - 1, 0])
        assert len(O.cached_nodes(keys, every, t, 14)) == 14
    # with only the ends accepted, the walk leaves one side at its first step and goes on the other
    first ={tuple(O.cached_nodes(keys, ends, t, 1)) for t in tg}
    assert first == {(0,), (n - 1,)}


@pytest.mark.parametrize("name", X.SORT_CASES)
def test_sort_sets_defeat_the_64_bit_shortcut(name):
    keys = X.sort_case(name)
    n = keys.shape[0]
    assert n == {"tile": 4096, "tile+1": 4097, "word4": 300}[name]
    assert len({bytes(k) for k in keys}) == n
    w = X.words(keys)
    assert len({(int(a), int(b)) for a, b in w[:, :2]}) < n      # equal 64-bit prefixes: the full sort runs
    if name == "word4":
        assert len({tuple(r) for r in w[:, :4]}) == 1 and len(set(w[:, 4])) == n
    else:
        assert X.is_boundary(keys).sum() == 6
        assert set(np.unique(keys[:, :8])) <= {0x00, 0x7F, 0x80, 0xFF}
        rest = keys[~X.is_boundary(keys)]
        assert np.all((rest[:, :8] == 0) .all(axis=1) | (rest[:, :8] == 0xFF).all(axis=1))
    order = np.lexsort(keys.T[::-1])
    assert not np.array_equal(order, np.arange(n))


@pytest.mark.parametrize("name", list(X.TABLE_MYIDS))
def test_tables_grow_from_the_boundary_keys(name):
    myid, firsts, off, nodes = X.table_case(name)
    assert firsts.shape[0] > 4 and not firsts[0].any()
    held = {bytes(x) for x in nodes}
    assert sum(bytes(b) in held for b in X.BOUNDARY) >= 5       # the boundary keys are nodes of the table
    assert bytes(20) in held or b"\xff" * 20 in held
    tg = X.boundary_targets()
    b = [O.find_bucket(firsts, t) for t in tg]
    assert 0 in b and firsts.shape[0] - 1 in b                  # findBucket's first and last bucket
    good = np.ones(nodes.shape[0], np.uint8)
    for t in tg[:14]:
        assert len(O.find_closest(firsts, off, nodes, good, t, 32)) > 8
    buckets, hist = O.classify(firsts, myid, X.boundary_keys())
    assert hist[160] == 1 and hist[0] > 200                     # myid itself, and the far half
    assert buckets.min() == 0 and buckets.max() == firsts.shape[0] - 1


# ---- D ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["insert103", "refill206", "shape404"])
def test_flipped_scripts_hold_the_full_word(name):
    """the flipped script runs on the model like the original, and ends with handle 2^28 - 1 in a
    list with the candidate and the replied flag: the stored word 0x3FFFFFFF"""
    script = dict(X.handle_scripts())[name]
    model = SM.Model()
    seen = set()
    for step in script:
        X.run_step(step, model)
        for sl in model.slots:
            seen.update(sl.row)
    assert max(seen) == X.HANDLE_TOP and min(seen) > X.HANDLE_TOP - (1 << 20)
    full = [(h << 0 | f << 28) for sl in model.slots for h, f in zip(sl.row, sl.flags) if h == X.HANDLE_TOP]
    assert full and all(w == 0x3FFFFFFF for w in full)
    assert not any(sl.over for sl in model.slots)
    assert any(len(sl.row) > 14 for sl in model.slots) or name != "insert103"


def test_flip_is_an_involution_on_handles():
    h = np.array([0, 3, 7, 1 << 20], np.uint32)
    assert list(X.flip(h)) == [X.HANDLE_TOP, X.HANDLE_TOP - 3, X.HANDLE_TOP - 7, X.HANDLE_TOP - (1 << 20)]
    assert np.array_equal(X.flip(X.flip(h)), h)


# ---- the crafted parts are what the assertions see ------------------------------------------------------
def test_uncrafted_sets_miss_the_edges():
    """the same assertions on plain hashed sets of the same sizes fail: no sentinel distance in any
    row, no row on both sides of 2^31 without the base, no equal 64-bit prefixes"""
    ids, tg, _ = X.far_case("far-w0")
    plain = O.gen_ids(7101, X.FAR_N)
    rows, _ = O.topk(plain, tg, 8)
    assert not np.any(dist_words(plain, tg, rows)[..., 0] == NONE)
    ids, tg = X.top_case()
    rows, _ = O.topk(ids, tg, 8)
    assert not np.any(rows >= X.TOP)
    w = X.words(O.gen_ids(7600 + 4096, 4096))
    assert len({(int(a), int(b)) for a, b in w[:, :2]}) == 4096
