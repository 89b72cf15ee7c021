"""The context model and its op generator (tests/ctx_model.py), checked without a GPU: the walks are
deterministic per seed, every op meets the preconditions include/dhtgpu.h states (checked here
against the header's text, not against the generator), the scripted matrix and the seeded walks
cover what tests/test_gpu_sequences.py relies on, and the composed model reproduces the resident
families' own scripts row for row."""
import numpy as np
import pytest

import ctx_model as M
import ncache_cases as NC
import oracle as O
import rsearch_cases as RS

WALK_SEEDS = M.WALK_SEEDS      # the seed list the device runs


@pytest.fixture(scope="module")
def walks():
    return {seed: M.walk(seed) for seed in WALK_SEEDS}


def same_arg(a, b):
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        return isinstance(a, np.ndarray) and isinstance(b, np.ndarray) and a.dtype == b.dtype and np.array_equal(a, b)
    if isinstance(a, tuple):
        return isinstance(b, tuple) and len(a) == len(b) and all(same_arg(x, y) for x, y in zip(a, b))
    return a == b


def test_walk_is_deterministic_per_seed(walks):
    for seed in WALK_SEEDS[:4]:
        again = M.walk(seed)
        assert [o.name for o in again] == [o.name for o in walks[seed]]
        assert all(same_arg(a.args, b.args) for a, b in zip(again, walks[seed]))
    assert [M.describe(o) for o in walks[WALK_SEEDS[0]]] != [M.describe(o) for o in walks[WALK_SEEDS[1]]]
    for seed in WALK_SEEDS:
        assert 40 <= len(walks[seed]) <= 60, (seed, len(walks[seed]))


# ---- the header's preconditions, restated from include/dhtgpu.h -------------------------------------------
MAX_K, MAX_HANDLE, SR_CAP = 32, 1 << 28, 64
OTHER_STREAM = {"set_accept_bits_dev"}      # the ops that issue work on a stream that is not the context's
NC_LOOKUPS_DEV = set()                      # ... none of them is an nc lookup, so nc_insert / nc_erase never meet one


def u32(a):
    return np.asarray(a, dtype=np.int64).reshape(-1)


def distinct(a):
    a = u32(a)
    return np.unique(a).size == a.size


def ids_ok(a):
    a = np.asarray(a)
    return a.dtype == np.uint8 and a.ndim == 2 and a.shape[1] == 20


def unique_rows(a):
    return np.unique(np.asarray(a), axis=0).shape[0] == len(a)


def check_op(o, m):
    """assert the op is one the header allows as the model m stands"""
    a, nm = o.args, o.name
    if nm in ("set_ids",):
        assert ids_ok(a[0]) and len(a[0]) < 0xFFFFFFFF
    elif nm == "gen_ids_prefix":
        assert a[2] <= 16 and a[3] < (1 << a[2]) and a[1] < 0xFFFFFFFF
    elif nm == "write_ids":
        assert m.ids is not None and not m.shard, "write_ids: prefix-shard contexts are EINVAL"
        assert ids_ok(a[1]) and a[0] + len(a[1]) <= m.n
    elif nm in ("set_accept", "set_accept_bits_dev"):
        assert m.ids is not None and (a[0] is None or len(a[0]) == m.n)
        assert not (nm == "set_accept_bits_dev" and a[0] is None)
    elif nm == "update_accept":
        assert m.ids is not None and len(a[0]) == len(a[1]) and distinct(a[0]) and (u32(a[0]) < m.n).all()
    elif nm in ("topk", "index_topk", "batch_topk", "topk_base"):
        assert ids_ok(a[0]) and 1 <= a[1] <= MAX_K
    elif nm == "cached_nodes":
        assert 1 <= a[1] <= MAX_K and (a[2] is None or len(a[2]) == m.n)
        assert m.ids is None or unique_rows(m.ids), "cached_nodes: duplicate ids are EUNSORTED"
    elif nm == "net_prepare":
        assert m.ids is not None and (a[0] is None or len(a[0]) == m.n)
    elif nm == "search_batch":
        assert len(a[0]) == len(a[1])
        if m.net is not None:
            assert (u32(a[1]) < m.n).all()
    elif nm == "classify":
        assert 1 <= len(a[0]) <= 256 and (np.lexsort(np.asarray(a[0]).T[::-1]) == np.arange(len(a[0]))).all()
    elif nm == "peer_merge":
        assert m.ids is not None and not m.shard and 1 <= a[2] <= MAX_K
    elif nm == "shard_merge":       # both halves of a 1-bit split, indices of the global stream, no mask on either
        assert m.shard and m.stream[2] == 1 and m.map_global and m.accept is None and 1 <= a[1] <= MAX_K
    elif nm == "cache_set":
        assert ids_ok(a[0]) and unique_rows(a[0])
    elif nm == "cache_nodes":
        assert 1 <= a[1] <= MAX_K and (m.cache is None or a[2] is None or len(a[2]) == len(m.cache[0]))
    elif nm == "rt_set":
        my, firsts, off, nodes, tail, af, ver = a
        assert len(firsts) <= 256 and len(off) == len(firsts) + 1 and (np.diff(u32(off)) >= 0).all()
        assert int(off[-1]) == len(nodes) and (tail is None and af == 0 or af in (4, 6) and len(tail) == len(nodes))
        assert tail is None or tail.shape[1] == (4 if af == 4 else 16) + 2
    elif nm == "rt_set_good":
        assert m.rt is not None and len(a[0]) == len(m.rt["nodes"])
    elif nm == "rt_update_good":
        assert m.rt is not None and distinct(a[0]) and (u32(a[0]) < len(m.rt["nodes"])).all() and len(a[0]) == len(a[1])
    elif nm in ("rt_find_closest", "nc_nodes"):
        assert 1 <= a[1] <= MAX_K
    elif nm == "nc_set":
        assert unique_rows(a[0]) and (a[1] is None or (distinct(a[1]) and (u32(a[1]) < MAX_HANDLE).all()))
    elif nm == "nc_insert":
        assert m.sr.have_nc and len(a[0]) == len(a[1]) and (u32(a[1]) < MAX_HANDLE).all()
        assert distinct(a[1]) and not (set(u32(a[1]).tolist()) & set(m.nc.map.values())), "one handle per key"
        assert a[2] is None or len(a[2]) == len(a[0])
    elif nm == "nc_erase":
        assert m.sr.have_nc and ids_ok(a[0])
    elif nm == "nc_update_accept":
        assert m.sr.have_nc and distinct(a[0]) and (u32(a[0]) < MAX_HANDLE).all() and len(a[0]) == len(a[1])
    elif nm == "nc_set_accept":
        assert m.sr.have_nc and len(a[0]) <= MAX_HANDLE
    elif nm == "sr_reset":
        assert a[0] <= (1 << 20)
    elif nm in ("sr_open", "sr_expire", "sr_insert", "sr_refill", "sr_status", "sr_lists"):
        if nm in ("sr_status", "sr_lists") and not m.sr_valid:
            return                      # the documented ENOIDS before the first reset
        assert m.sr_valid and distinct(a[0]) and (u32(a[0]) < len(m.sr.slots)).all(), "distinct slots below nslots"
        if nm == "sr_open":
            assert len(a[1]) == len(a[0])
        if nm == "sr_refill":
            assert 1 <= a[1] <= MAX_K
        if nm == "sr_insert":
            off = u32(a[1])
            assert off.size == len(a[0]) + 1 and off[0] == 0 and (np.diff(off) >= 0).all()
            assert len(a[2]) >= off[-1] and len(a[3]) >= off[-1] and (a[4] is None or len(a[4]) >= off[-1])
            assert (u32(a[2]) < MAX_HANDLE).all()
            for h, k in zip(u32(a[2]).tolist(), np.asarray(a[3])):       # one handle per id
                assert m.sr.ids.get(h, bytes(k)) == bytes(k)
    elif nm == "sr_set_state":
        assert m.sr_valid and len(a[0]) <= MAX_HANDLE
    elif nm == "sr_update_state":
        assert m.sr_valid and distinct(a[0]) and (u32(a[0]) < MAX_HANDLE).all()
    elif nm == "sr_set_candidate":
        assert m.sr_valid and (u32(a[0]) < len(m.sr.slots)).all() and (u32(a[1]) < MAX_HANDLE).all()
        assert len(set(zip(u32(a[0]).tolist(), u32(a[1]).tolist()))) == len(a[0]), "distinct (slot, handle) pairs"
    else:
        assert nm in ("gen_ids", "set_global_indices", "set_sub_handles", "num_accepted", "get_ids", "cache_sorted",
                      "rt_reply", "nc_export"), f"no precondition written for {nm}"


def check_sequence(ops):
    m = M.Model()
    for i, o in enumerate(ops):
        try:
            check_op(o, m)
        except AssertionError as e:
            raise AssertionError(f"step {i} {M.describe(o)}: {e}") from None
        assert not (o.name in OTHER_STREAM and o.name in NC_LOOKUPS_DEV)
        M.run(o, m, None, want=False)
        for sl in m.sr.slots:       # an exact case never overflows a row
            assert len(sl.row) <= RS.LIST_BOUND and not sl.over
    return m


def test_every_walk_op_meets_the_headers_preconditions(walks):
    for seed, ops in walks.items():
        check_sequence(ops)


def test_every_matrix_row_meets_the_preconditions_and_probes_its_pair():
    """coverage as a condition: every (mutation, derived structure) pair of the matrix occurs in
    its scripted row -- the structure's query, the mutation, the query again, no rebuild between"""
    assert len(M.MATRIX) == len(M.MUTATIONS) * len(M.STRUCTURES) == len(set(M.MATRIX))
    ns = {st: set() for st in M.STRUCTURES}
    for mu, st in M.MATRIX:
        ops, at = M.matrix_script(mu, st)
        m = check_sequence(ops)
        assert (mu, st) in M.trace(ops), (mu, st)
        assert M.kind_of(ops[at], replayed(ops[:at])) == mu
        ns[st].update(len(o.args[0]) for o in ops if o.name == "set_ids")
    for st in M.STRUCTURES:       # both sizes per structure
        assert set(M.SIZES_N) <= ns[st], (st, ns[st])


def test_scripted_gpu_sequences_meet_the_preconditions():
    """the fixed op lists of tests/test_gpu_sequences.py (isolation set-up and family mutations, the
    setters' set-up), checked like the walks; importing that module needs no GPU"""
    import test_gpu_sequences as T
    ops = T._resident_ops()
    m = check_sequence(ops)
    for steps in T._family_mutations(m).values():
        for _, more in steps:
            ops = ops + more
    check_sequence(ops)
    m = M.Model()
    T._setter_state(None, m)
    for name in T.SETTERS:
        check_op(T._setter_call(name, 257, np.random.default_rng(1), m)[0], m)


def replayed(ops):
    m = M.Model()
    for o in ops:
        M.run(o, m, None, want=False)
    return m


RESIDENT_MUTATIONS = {"cache_set", "rt_set", "rt_set_good", "rt_update_good", "nc_set", "nc_insert", "nc_erase",
                      "nc_update_accept", "nc_set_accept", "sr_reset", "sr_open", "sr_expire", "sr_set_state",
                      "sr_update_state", "sr_set_candidate", "sr_insert", "sr_refill", "net_prepare"}


def test_walk_seeds_cover_every_kind_and_half_the_matrix(walks):
    names, kinds, pairs = set(), set(), set()
    for seed, ops in walks.items():
        m = M.Model()
        for o in ops:
            names.add(o.name)
            k = M.kind_of(o, m)
            if k:
                kinds.add(k)
            M.run(o, m, None, want=False)
        pairs |= M.trace(ops)
    assert kinds == set(M.MUTATIONS), set(M.MUTATIONS) - kinds
    assert RESIDENT_MUTATIONS <= names, RESIDENT_MUTATIONS - names
    assert M.QUERIES <= names, M.QUERIES - names
    assert pairs <= set(M.MATRIX)
    assert 2 * len(pairs) >= len(M.MATRIX), f"{len(pairs)} of {len(M.MATRIX)} pairs probed by the walks"


def test_walks_meet_the_documented_error_paths(walks):
    """ENOIDS before the first nc_set / rt_set / cache_set / sr_reset / set_ids, and from search_batch
    after the ids changed and before net_prepare"""
    stale_net = False
    for seed, ops in walks.items():
        m = M.Model()
        for o in ops:
            if o.name == "search_batch" and m.net is None and m.ids is not None:
                assert M.run(o, m, None)[1] == M.err(M.ENOIDS)
                stale_net = True
            M.run(o, m, None, want=False)
        first = {o.name: M.run(o, M.Model(), None)[1] for o in ops[:5]}
        assert all(M.is_err(w) and w[1] == M.ENOIDS for w in first.values()), first
        assert {"nc_nodes", "rt_find_closest", "cache_sorted", "sr_status", "topk"} <= set(first)
    assert stale_net


# ---- the composition adds nothing of its own ------------------------------------------------------------
_NAME = {v: k for k, v in M._SR_STEPS.items()}


def test_composed_model_reproduces_the_search_lifecycle():
    script = RS.lifecycle_script()
    plain, comp = RS.Model(), M.Model()
    slots = np.arange(40, dtype=np.uint32)
    for step in script:
        want, _ = RS.run_step(step, plain)
        _, mine = M.run(M.Op(_NAME[step[0]], tuple(step[1:])), comp, None)
        if want is not None:
            assert np.array_equal(mine[0], want), step[0]
        assert M.same(comp.sr.lists(slots), plain.lists(slots)), step[0]
        assert np.array_equal(M.run(M.Op("sr_status", (slots,)), comp, None)[1][0], plain.status(slots)), step[0]
    assert RS.max_len(plain) <= RS.LIST_BOUND


def test_composed_model_reproduces_an_nc_mutation_sequence():
    plain, comp = NC.Model(), M.Model()
    keys = O.gen_ids(41, 600)
    plain.set(keys, None)
    M.run(M.Op("nc_set", (keys, None)), comp, None)
    tg = NC.targets_for(keys, 5)
    nxt = 600
    for r in range(4):
        ids, h, acc = NC.mutation_batch(plain, 64, 900 + r, nxt)
        nxt += 64
        assert np.array_equal(M.run(M.Op("nc_insert", (ids, h, acc)), comp, None)[1][0], plain.insert(ids, h, acc))
        gone = ids[::3]
        assert np.array_equal(M.run(M.Op("nc_erase", (gone,)), comp, None)[1][0], plain.erase(gone))
        plain.update_accept(h[:7], 0)
        M.run(M.Op("nc_update_accept", (h[:7], np.zeros(7, np.uint8))), comp, None)
        for count in (8, 14):
            assert M.same(M.run(M.Op("nc_nodes", (tg, count)), comp, None)[1], plain.expected(tg, count)), (r, count)
        assert M.same(M.run(M.Op("nc_export", ()), comp, None)[1], plain.sorted())


def test_version_shortcuts_in_the_model():
    """cache_set / rt_set: the same version with the same shape is skipped, version 0, a new version
    or another n / nb replaces (the rule of include/dhtgpu.h)"""
    m = M.Model()
    a, b = O.gen_ids(1, 100), O.gen_ids(2, 100)
    m.cache_set(a, 5)
    m.cache_set(b, 5)
    assert np.array_equal(m.cache[0], a)
    m.cache_set(b[:50], 5)
    assert len(m.cache[0]) == 50
    m.cache_set(a, 0)
    m.cache_set(b, 0)
    assert np.array_equal(m.cache[0], b)
    t1, t2 = M.rt_table(3, 700, 50), M.rt_table(4, 700, 50)
    m.rt_set(*t1, 9)
    m.rt_set(*t2, 9)
    assert np.array_equal(m.rt["nodes"], t1[3])
    m.rt_set(*t2, 10)
    assert np.array_equal(m.rt["nodes"], t2[3])
