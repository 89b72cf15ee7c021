"""Sequences of calls on one long-lived context, model-checked: after every step each answer is
compared exactly (np.array_equal; everything here is integer work) with tests/ctx_model.py, the
composition of the suite's oracle-backed models.  What is pinned is the context's state ACROSS
calls: the derived structures and their validity flags (DESIGN.md §2 lists them), the buffers the
families share, the version short-cuts, and the setters that do not synchronise.
Marked gpu: run on the MI355X box."""
import ctypes

import numpy as np
import pytest

import ctx_model as M
import oracle as O
import rsearch_cases as RS
from ctx_model import Op

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
WALK_SEEDS = M.WALK_SEEDS


@pytest.fixture(scope="module")
def dev():
    """one context for the whole stale-structure matrix: the rows follow each other on it"""
    import opendht_amd
    with opendht_amd.Context(0) as c, opendht_amd.Context(0) as peer:
        yield M.Device(c, peer)


@pytest.fixture()
def fresh():
    import opendht_amd
    with opendht_amd.Context(0) as c, opendht_amd.Context(0) as peer:
        yield M.Device(c, peer)


# ---- a. the stale-structure matrix ---------------------------------------------------------------------
@pytest.mark.parametrize("mu,st", M.MATRIX, ids=[f"{st}-{mu}" for mu, st in M.MATRIX])
def test_stale_structure(dev, mu, st):
    """Row (mutation, structure) of the matrix: the structure's query builds it and is checked, the
    mutation follows, the same query must answer over the new state (ctx_model.matrix_script; n in
    {4,097, 70,001}, q in {65, 300}, k in {8, 14}; the post-mutation targets include the ids just
    written, which a stale structure answers wrong).  The crawl model's rows demand ENOIDS after
    every id mutation until net_prepare, then O.search_batch over the new ids."""
    ops, _ = M.matrix_script(mu, st)
    M.replay(ops, M.Model(), dev, seed=f"matrix row {mu}/{st}")
    dev.sync()


def _k6_batches(ids):
    """(name, targets, top-32 rows, counts): a full batch, a small one, a clustered one whose
    targets' subtrees are short of k ids (they take the fallback list)"""
    full = O.gen_ids(8102, 1024)
    small = O.gen_ids(8103, 64)
    fb = O.gen_ids(8104, 1024)
    out = []
    for name, tg in (("full", full), ("small", small), ("fallback", fb)):
        want, cnt = O.topk(ids, tg, 32)
        out.append((name, tg, want, cnt))
    return out


def test_k6_slot_state_alternating_routes():
    """The K6 slot state (zeroed, sclean, spar, desc_sig, the fb_hint word) on one context: twelve
    calls that alternate the full-batch route (n = 2^20 + 3, q = 1,024: the sizes test_gpu_fuzz uses
    to reach it), the small-batch path (q = 64), a clustered batch on the fallback list, and k in
    {8, 14, 32}, issued round-robin on four streams so that each of the kBatchDepth = 4 workspaces
    is reused after a call of another kind (three kinds over four streams: every slot meets all
    three).  The reference is one oracle top-32 per batch; a top-k row is its first k entries."""
    import opendht_amd
    import torch
    n = (1 << 20) + 3
    ids = O.gen_ids(8101, n)
    fb = O.gen_ids(8104, 1024)
    # empty the level-12 subtrees of 40 targets down to 2 ids each: their top-k lies outside the
    # mark-level subtree (level >= 13 here), so F3 lists them for the fallback scan
    key = lambda a: ((a[:, 0].astype(np.uint32) << 8) | a[:, 1]) >> 4
    ik, tk = key(ids), key(fb)
    for t in range(0, 400, 10):
        inside = np.nonzero(ik == tk[t])[0][2:]
        ids[inside, 0] ^= 0x80
        ik = key(ids)
    batches = _k6_batches(ids)
    dev = torch.device("cuda", 0)
    streams = [torch.cuda.Stream(dev) for _ in range(4)]
    with opendht_amd.Context(0) as c:
        d = M.Device(c)
        c.set_ids(ids)
        planes = {name: d.planes(tg) for name, tg, _, _ in batches}
        for i in range(12):
            name, tg, want32, _ = batches[i % 3]
            k = (8, 14, 32)[(i // 3 + i) % 3]
            q = tg.shape[0]
            tp, ts = planes[name]
            out = torch.full((q, k), -7, dtype=torch.int32, device=dev)
            cnt = torch.full((q,), -7, dtype=torch.int32, device=dev)
            s = streams[i % 4]
            c.batch_topk_dev(tp.data_ptr(), ts, q, k, out.data_ptr(), cnt.data_ptr(), None, 0, s.cuda_stream)
            s.synchronize()
            got = out.cpu().numpy().view(np.uint32)
            assert np.array_equal(cnt.cpu().numpy().view(np.uint32), np.full(q, k, np.uint32)), (i, name, k)
            bad = np.nonzero((got != want32[:, :k]).any(axis=1))[0]
            assert bad.size == 0, f"call {i} ({name}, k={k}, stream {i % 4}): {bad.size} rows differ, first {bad[:5]}"


def test_version_shortcuts(fresh):
    """cache_set / rt_set: the same version with the same shape is skipped as documented -- the old
    content is still what answers (cache_sorted, rt answers) -- and version 0, a new version or a
    changed n / nb replaces it."""
    m, d = M.Model(), fresh
    a, b = O.gen_ids(61, 4097), O.gen_ids(62, 4097)
    tg = O.gen_ids(63, 65)
    t1, t2, t3 = M.rt_table(64, 3000, 200), M.rt_table(65, 3000, 200), M.rt_table(66, 3000, 150)
    ask_c = [Op("cache_sorted", ()), Op("cache_nodes", (tg, 14, None))]
    ask_r = [Op("rt_find_closest", (tg, 14)), Op("rt_reply", (tg[:17],))]
    ops = [Op("cache_set", (a, 7))] + ask_c + [Op("cache_set", (b, 7))] + ask_c          # skipped: a answers
    ops += [Op("cache_set", (b, 8))] + ask_c + [Op("cache_set", (a[:3001], 8))] + ask_c   # new version; new n
    ops += [Op("cache_set", (b[:3001], 0))] + ask_c + [Op("cache_set", (a[:3001], 0))] + ask_c   # version 0 always uploads
    ops += [Op("rt_set", t1 + (5,))] + ask_r + [Op("rt_set", t2 + (5,))] + ask_r          # skipped: t1 answers
    ops += [Op("rt_set", t2 + (6,))] + ask_r + [Op("rt_set", t3 + (6,))] + ask_r          # new version; new nb
    ops += [Op("rt_set", t1 + (0,))] + ask_r + [Op("rt_set", t2 + (0,))] + ask_r
    M.replay(ops, m, d, seed="version short-cuts")
    assert np.array_equal(m.cache[0], a[:3001]) and np.array_equal(m.rt["nodes"], t2[3])


# ---- b. cross-family isolation --------------------------------------------------------------------------
def _resident_ops():
    rng = np.random.default_rng(9000)
    n = 70001
    mask = (rng.random(n) < 0.6).astype(np.uint8)
    slots = np.arange(40, dtype=np.uint32)
    nck = O.gen_ids(9004, 4097)
    nch = (rng.permutation(4097) + 30000).astype(np.uint32)     # clear of the reply nodes' handles 2000..2199: one handle per id
    return [Op("set_ids", (O.gen_ids(9001, n),)), Op("set_accept", (mask,)),
            Op("cache_set", (O.gen_ids(9002, 4097), 1)),
            Op("rt_set", M.rt_table(9003, 3000, 200) + (1,)), Op("rt_set_good", ((rng.random(3000) < 0.7).astype(np.uint8),)),
            Op("nc_set", (nck, nch)), Op("nc_update_accept", (nch[:900], np.zeros(900, np.uint8))),
            Op("sr_reset", (40,)), Op("sr_open", (slots, O.gen_ids(9005, 40))), Op("sr_refill", (slots[:25], 14))]


def _fixed_queries():
    rng = np.random.default_rng(9100)
    t65, t300, t17 = O.gen_ids(9101, 65), O.gen_ids(9102, 300), O.gen_ids(9103, 17)
    slots = np.arange(40, dtype=np.uint32)
    return {"ids": [Op("topk", (t65, 8)), Op("index_topk", (t300, 14)), Op("batch_topk", (t300, 8)),
                    Op("cached_nodes", (t65, 14, None)), Op("num_accepted", ())],
            "cache": [Op("cache_sorted", ()), Op("cache_nodes", (t65, 14, None))],     # (no accept bytes: the mirror's n changes under the cache family's mutations)
            "rt": [Op("rt_find_closest", (t65, 14)), Op("rt_reply", (t17,))],
            "nc": [Op("nc_nodes", (t65, 14)), Op("nc_export", ())],
            "sr": [Op("sr_status", (slots,)), Op("sr_lists", (slots,))]}


def _ask(d, ops):
    return [M.CTX[o.name](d, *o.args) for o in ops]


def _record(d, m, fixed, fam):
    """the family's fixed answers, each checked against the model"""
    out = []
    for o in fixed[fam]:
        got, want = M.run(o, m, d)
        assert M.same(got, want), f"{fam}: {M.describe(o)} disagrees with the model"
        out.append(got)
    return out


def _others_unchanged(d, fixed, rec, but, after):
    for fam, ops in fixed.items():
        if fam == but:
            continue
        for o, was, now in zip(ops, rec[fam], _ask(d, ops)):
            assert M.same(now, was), f"after {after}: {fam}'s {M.describe(o)} changed"


def _family_mutations(m):
    """per family: (label, ops) small then large; the large ones make the buffers that family
    stages through reallocate (sizes from the ensure / carve calls of the api*.hip units):
      ids    gen_ids_prefix over a 2^20-id stream: staging 5 * 4 B * 2^20 = 20 MB, aux 4 B * its select scratch
      cache  200,000 keys: staging 20 B * n = 4 MB, cache_in, sort_scratch = sort_scratch_bytes(200,000)
      rt     70,001 nodes: rt.buf (the RtView pointers move), staging 1.4 MB; rt_update_good of 65,537: staging 5 B * m
      nc     nc_insert of 65,537 keys: nc.hin 4 B * m, nc.in / sorted / work, sort_scratch, both key sets grow;
             nc_update_accept of 65,537 handles up to 2^22: nc.hin 5 B * m, the mask grows (bits_old)
      sr     sr_update_state of 65,537 handles up to 2^21: sr.io 5 B * m, st grows (st_old); sr_insert of 40 x 30:
             sr.io (slots, offsets, handles, id planes, tokens, results)"""
    rng = np.random.default_rng(9200)
    slots = np.arange(40, dtype=np.uint32)
    held = np.array(sorted(m.nc.map.values()), np.uint32)
    big_h = rng.choice(1 << 22, 65537, replace=False).astype(np.uint32)
    st_h = (5000 + rng.choice(1 << 21, 65537, replace=False)).astype(np.uint32)
    node = rng.integers(0, 200, size=40 * 30)
    pool = O.gen_ids(777, 200)
    return {
        "ids": [("write_ids + update_accept", [Op("write_ids", (77, O.gen_ids(9201, 3))),
                                               Op("update_accept", (rng.choice(70001, 257, replace=False).astype(np.uint32),
                                                                    (rng.random(257) < 0.5).astype(np.uint8)))]),
                ("gen_ids_prefix 2^20, then set_ids + mask", [Op("gen_ids_prefix", (9202, 1 << 20, 3, 5)),
                                                              Op("set_ids", (O.gen_ids(9203, 70001),)),
                                                              Op("set_accept", ((rng.random(70001) < 0.6).astype(np.uint8),))])],
        "cache": [("cache_set 1,000", [Op("cache_set", (O.gen_ids(9204, 1000), 2))]),
                  ("cache_set 200,000, then 4,097", [Op("cache_set", (O.gen_ids(9205, 200000), 3)),
                                                     Op("cache_set", (O.gen_ids(9206, 4097), 4))])],
        "rt": [("rt_update_good 257", [Op("rt_update_good", (rng.choice(3000, 257, replace=False).astype(np.uint32),
                                                             (rng.random(257) < 0.5).astype(np.uint8)))]),
               ("rt_set 70,001 + rt_update_good 65,537", [Op("rt_set", M.rt_table(9207, 70001, 256, 6) + (2,)),
                                                          Op("rt_update_good", (rng.choice(70001, 65537, replace=False).astype(np.uint32),
                                                                                (rng.random(65537) < 0.5).astype(np.uint8)))])],
        "nc": [("nc_insert 64 + nc_update_accept 257", [Op("nc_insert", (O.gen_ids(9208, 64), np.arange(10000, 10064, dtype=np.uint32), None)),
                                                        Op("nc_update_accept", (held[:257], (rng.random(257) < 0.5).astype(np.uint8)))]),
               ("nc_insert 65,537 + nc_update_accept 65,537", [Op("nc_insert", (O.gen_ids(9209, 65537), np.arange(1 << 23, (1 << 23) + 65537, dtype=np.uint32), None)),
                                                               Op("nc_update_accept", (big_h, (rng.random(65537) < 0.5).astype(np.uint8)))])],
        "sr": [("sr_insert 40 x 3", [Op("sr_insert", (slots, RS.csr(np.full(40, 3)), (2000 + node[:120]).astype(np.uint32), pool[node[:120]], None))]),
               ("sr_update_state 65,537 + sr_insert 40 x 30", [Op("sr_update_state", (st_h, np.zeros(65537, np.uint8))),
                                                               Op("sr_insert", (slots, RS.csr(np.full(40, 30)), (2000 + node).astype(np.uint32), pool[node],
                                                                                (rng.random(node.size) < 0.4).astype(np.uint8)))])],
    }


def _stateless(d, m, large):
    """The scratch-heavy stateless calls, each checked against the oracle, small or large enough
    that the shared buffer it stages through must grow (api_dht.hip):
      buffer_nodes_ids  200,000 nodes, 3,000 x 32 candidates, af 6: staging 20 B * nn = 4 MB, wire = wire_bytes(...) ~ 5 MB
      deserialize_nodes 2,000 blobs of 8 records: wire (blob, offsets, senders, outputs) ~ 1.3 MB
      search_insert     100,000 nodes, 2,000 searches at cap 64: staging 2 MB, srch ~ 1.3 MB
      table_stats       256 buckets: srch (firsts planes + 2 x 256 words)
      classify          256 buckets over the resident set: aux2 / staging for n bucket bytes + the histogram
      select_prefix_dev 2^20 ids: aux = 4 B * select_scratch_words(2^20) + 16
      cached_nodes      20,000 targets: staging 400 KB, targets, aux2 = 20,000 * 14 * 4 B, aux3
      merge             peer_merge, 5,000 x 32 records per context: out_idx / out_cnt / rec
    Yields a label after each call."""
    import torch
    import opendht_amd
    rng = np.random.default_rng(9300 + large)
    c = d.ctx
    # buffer_nodes_ids
    nn, q, nc_, af = (200000, 3000, 32, 6) if large else (100, 10, 8, 4)
    alen = 16 if af == 6 else 4
    nodes, tail = O.gen_ids(9301 + large, nn), rng.integers(0, 256, size=(nn, alen + 2), dtype=np.uint8)
    tg = O.gen_ids(9302, q)
    cand = rng.integers(0, nn, size=(q, nc_)).astype(np.uint32)
    cand[::7, ::3] = NONE
    out, ln = c.buffer_nodes_ids(nodes, tail, af, tg, cand)
    for i in range(0, q, max(1, q // 40)):
        want = O.buffer_nodes(nodes, tail, alen, tg[i], cand[i])
        assert ln[i] == want.size and np.array_equal(out[i, : ln[i]], want), ("buffer_nodes_ids", i)
    yield "buffer_nodes_ids"
    # deserialize_nodes
    nmsg, per = (2000, 8) if large else (5, 3)
    recs = np.concatenate([O.gen_ids(9303, nmsg * per), O.special_addrs(rng, nmsg * per, 6)], axis=1)
    myid = recs[3, :20].copy()
    blobs = [recs[i * per:(i + 1) * per].tobytes() for i in range(nmsg)]
    blobs[1] = blobs[1][:-1]       # not a whole number of records
    faf = rng.choice([4, 6, 0], size=nmsg).astype(np.uint8)
    fad = rng.integers(0, 256, size=(nmsg, 16), dtype=np.uint8)
    gi, gt, gs, gm = c.deserialize_nodes(6, myid, blobs, faf, fad)
    assert gm[1] == 1 and gm.sum() == 1 and gi.shape[0] == (nmsg - 1) * per
    msg_of = [i for i in range(nmsg) if i != 1 for _ in range(per)]
    for r in range(0, gi.shape[0], max(1, gi.shape[0] // 60)):
        i = msg_of[r]
        rec = recs[i * per + r % per]
        st, tl = O.deserialize_node(rec, 6, myid, int(faf[i]), fad[i])
        assert gs[r] == st and np.array_equal(gi[r], rec[:20]) and (st == 1 or np.array_equal(gt[r], tl)), ("deserialize", r)
    yield "deserialize_nodes"
    # search_insert
    nn, q, per = (100000, 2000, 10) if large else (64, 4, 5)
    nodes = O.gen_ids(9304 + large, nn)
    state = rng.choice([0, 0, 0, 2], size=nn).astype(np.uint8)
    lists = np.full((q, 64), NONE, np.uint32)
    flags, lens, exp = np.zeros((q, 64), np.uint8), np.zeros(q, np.uint32), np.zeros(q, np.uint8)
    ins = rng.integers(0, nn, size=q * per).astype(np.uint32)
    tok = (rng.random(q * per) < 0.3).astype(np.uint8)
    args = (nodes, state, O.gen_ids(9305, q), lists, flags, lens, exp, RS.csr(np.full(q, per)), ins, tok)
    for g, w, nm in zip(c.search_insert(*args), O.search_insert(*args), ("lists", "flags", "lens", "expired", "added")):
        assert np.array_equal(g, w), ("search_insert", nm)
    yield "search_insert"
    # table_stats
    firsts = M.rt_table(9306, 3000, 256 if large else 5)[1]
    lb, dp = c.table_stats(firsts)
    assert [int(x) for x in lb] == [O.lowbit(f) for f in firsts]
    assert [int(x) for x in dp] == [O.depth(firsts, b) for b in range(len(firsts))]
    yield "table_stats"
    # classify (over the resident id set)
    myid = O.gen_ids(9307, 1)[0]
    got = c.classify(firsts, myid)
    want = O.classify(firsts, myid, m.ids, threads=8)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), "classify"
    yield "classify"
    # select_prefix_dev
    n = (1 << 20) if large else 1000
    sel = O.gen_ids(9308, n)
    pl = torch.from_numpy(opendht_amd.id_words(sel).view(np.int32).copy()).to(d.dev)
    outp = torch.zeros((5, n), dtype=torch.int32, device=d.dev)
    gidx = torch.zeros(n, dtype=torch.int32, device=d.dev)
    torch.cuda.synchronize()
    cnt = c.select_prefix_dev(pl.data_ptr(), n, n, 3, 5, outp.data_ptr(), n, gidx.data_ptr())
    pick = np.flatnonzero((sel[:, 0] >> 5) == 5)
    assert cnt == pick.size and np.array_equal(gidx.cpu().numpy()[:cnt].view(np.uint32), pick.astype(np.uint32)), "select_prefix_dev"
    yield "select_prefix_dev"
    # cached_nodes
    o = Op("cached_nodes", (O.gen_ids(9309, 20000 if large else 65), 14, (rng.random(m.n) < 0.7).astype(np.uint8)))
    got, want = M.run(o, m, d)
    assert M.same(got, want), "cached_nodes"
    yield "cached_nodes"
    # a record merge through merge_util.merge over this context and the peer
    o = Op("peer_merge", (O.gen_ids(9310, 3001), O.gen_ids(9311, 5000 if large else 65), 32 if large else 8))
    got, want = M.run(o, m, d)
    assert M.same(got, want), "merge"
    yield "merge"


@pytest.mark.parametrize("order", ["state_before_growth", "state_after_growth"])
def test_cross_family_isolation(fresh, order):
    """All five resident states on one context -- ids (70,001) + mask, cache_set (4,097 keys), rt_set
    (3,000 nodes with tails), nc_set (4,097 keys), sr_reset + sr_open (40 slots, 25 filled through
    sr_refill) -- and a fixed query set per family.  Then, family by family, that family's mutations,
    small then large (_family_mutations), and the scratch-heavy stateless calls, small then large
    (_stateless): after each, every OTHER family's fixed answers must be the recorded ones byte for
    byte (the mutated family's are checked against the model and recorded again).  Two orders of
    growth: the resident state built on a fresh context, so that the shared buffers grow under it;
    and built after a first pass of the large calls has already grown them."""
    d, m = fresh, M.Model()
    if order == "state_after_growth":
        M.replay([Op("set_ids", (O.gen_ids(9000, 3001),))], m, d)
        for _ in _stateless(d, m, 1):
            pass
        d.ctx.cache_set(O.gen_ids(9205, 200000), 99)
        m.cache_set(O.gen_ids(9205, 200000), 99)
    M.replay(_resident_ops(), m, d, seed="isolation set-up")
    fixed = _fixed_queries()
    rec = {fam: _record(d, m, fixed, fam) for fam in fixed}
    for fam, steps in _family_mutations(m).items():
        for label, ops in steps:
            M.replay(ops, m, d, seed=f"isolation {label}")
            _others_unchanged(d, fixed, rec, fam, label)
            rec[fam] = _record(d, m, fixed, fam)
    for large in (0, 1):
        for label in _stateless(d, m, large):
            _others_unchanged(d, fixed, rec, None, f"{label} ({'large' if large else 'small'})")
    d.sync()


# ---- c. seeded random walks ----------------------------------------------------------------------------
@pytest.mark.parametrize("seed", WALK_SEEDS)
def test_random_walk(fresh, seed):
    """About 40 ops over the whole op set on one fresh context (and a peer for peer_merge), the model
    checked at every query; sizes as in the matrix (n <= 70,001, no full-batch K6 step).  A failure is
    replayable from the seed: ctx_model.walk(seed)."""
    M.replay(M.walk(seed), M.Model(), fresh, seed=seed)
    fresh.sync()


# ---- d. back-to-back non-synchronising setters -------------------------------------------------------------
SIZES = (1, 257, 65537, 257, 65537, 1, 65537, 257)    # test_gpu_prims' sizes: the staging buffer is carved again
                                                     # at every call and grows at the first 65,537


def _p(a, t):
    return a.ctypes.data_as(ctypes.POINTER(t))


def _raw(d, name, *arrays):
    """the C entry point itself, on the caller's arrays (the Python wrapper copies the value bytes)"""
    import opendht_amd
    types = {np.dtype(np.uint32): ctypes.c_uint32, np.dtype(np.uint8): ctypes.c_uint8}
    args = [_p(a, types[a.dtype]) for a in arrays]
    code = getattr(opendht_amd.lib(), "dhtgpu_" + name)(d.ctx._h, *args, arrays[0].shape[0])
    assert code == 0, (name, code)


SETTERS = ("update_accept", "rt_update_good", "nc_update_accept", "sr_update_state", "sr_set_candidate")


def _setter_state(d, m):
    rng = np.random.default_rng(9400)
    slots = np.arange(40, dtype=np.uint32)
    node = rng.integers(0, 200, size=40 * 12)
    M.replay([Op("set_ids", (O.gen_ids(9401, 70001),)),
              Op("rt_set", M.rt_table(9402, 70001, 256) + (1,)),
              Op("nc_set", (O.gen_ids(9403, 4097), rng.choice(1 << 17, 4097, replace=False).astype(np.uint32))),
              Op("sr_reset", (40,)), Op("sr_open", (slots, O.gen_ids(9404, 40))),
              Op("sr_insert", (slots, RS.csr(np.full(40, 12)), (2000 + node).astype(np.uint32), O.gen_ids(777, 200)[node], None))],
             m, d, seed="setter set-up")


def _setter_call(name, size, rng, m):
    """(op, its arrays in the C call's order) for one call of `size` entries"""
    if name == "update_accept":
        a = (rng.choice(m.n, size, replace=False).astype(np.uint32), (rng.random(size) < 0.5).astype(np.uint8))
    elif name == "rt_update_good":
        a = (rng.choice(len(m.rt["nodes"]), size, replace=False).astype(np.uint32), (rng.random(size) < 0.5).astype(np.uint8))
    elif name == "nc_update_accept":
        a = (rng.choice(1 << 17, size, replace=False).astype(np.uint32), (rng.random(size) < 0.5).astype(np.uint8))
    elif name == "sr_update_state":     # removable (2) or nothing: no node turns bad, the lists stay exact
        a = (rng.choice(1 << 17, size, replace=False).astype(np.uint32), (2 * (rng.random(size) < 0.5)).astype(np.uint8))
    else:                               # distinct (slot, handle) pairs; handles 2000..2199 are the listed ones
        pair = rng.choice(40 * 2500, size, replace=False)
        a = ((pair % 40).astype(np.uint32), (pair // 40).astype(np.uint32), (rng.random(size) < 0.5).astype(np.uint8))
    return Op(name, a), a


_AFTER = {"update_accept": lambda: [Op("num_accepted", ()), Op("topk", (O.gen_ids(9410, 65), 8))],
          "rt_update_good": lambda: [Op("rt_find_closest", (O.gen_ids(9411, 65), 14))],
          "nc_update_accept": lambda: [Op("nc_nodes", (O.gen_ids(9412, 65), 14))],
          "sr_update_state": lambda: [Op("sr_status", (np.arange(40, dtype=np.uint32),)),
                                      Op("sr_insert", (np.arange(40, dtype=np.uint32), RS.csr(np.full(40, 2)),
                                                       (2000 + np.arange(80) % 200).astype(np.uint32), O.gen_ids(777, 200)[np.arange(80) % 200], None)),
                                      Op("sr_lists", (np.arange(40, dtype=np.uint32),))],
          "sr_set_candidate": lambda: [Op("sr_status", (np.arange(40, dtype=np.uint32),)), Op("sr_lists", (np.arange(40, dtype=np.uint32),))]}


def _run_setters(d, m, names, clobber, seed):
    """eight calls (the names in rotation) with no query or synchronisation of ours in between, each
    applied to the model with the values PASSED; clobber: the host arrays are overwritten as soon
    as the call has returned"""
    rng = np.random.default_rng(seed)
    log = []
    for i, size in enumerate(SIZES):
        name = names[i % len(names)]
        o, arrays = _setter_call(name, size, rng, m)
        passed = tuple(a.copy() for a in arrays)
        _raw(d, name, *arrays)
        if clobber:
            for a in arrays:
                a[:] = rng.integers(0, 2, size=a.shape).astype(a.dtype)      # in-range whatever is read late
        M.run(Op(name, passed), m, None)
        log.append(f"{name}[{passed[0].shape[0]}]")
    for name in names:
        for o in _AFTER[name]():
            got, want = M.run(o, m, d)
            assert M.same(got, want), f"after {' '.join(log)}{' (arrays overwritten on return)' if clobber else ''}: " \
                                      f"{M.describe(o)} disagrees with the model"


@pytest.mark.parametrize("clobber", [False, True], ids=["arrays_kept", "arrays_overwritten_on_return"])
@pytest.mark.parametrize("name", SETTERS + ("mixed",))
def test_back_to_back_setters(fresh, name, clobber):
    """Eight calls in a row of one non-synchronising setter (or, mixed, nc_update_accept, then
    sr_update_state, then rt_update_good in rotation: they share stage_idx_val) with different
    index and value arrays of 1, 257 and 65,537 entries, then one query against the model after
    all eight.  With clobber, each call's host arrays are overwritten the moment it returns: what
    include/dhtgpu.h promises for arrays in ordinary (pageable) host memory -- stack, heap,
    std::vector, numpy -- is that they are the caller's again when the call returns, so the
    answer must reflect the values passed."""
    m = M.Model()
    _setter_state(fresh, m)
    names = ("nc_update_accept", "sr_update_state", "rt_update_good") if name == "mixed" else (name,)
    _run_setters(fresh, m, names, clobber, 9500 + SETTERS.index(names[0]))
    fresh.sync()
