"""One host model of a whole dhtgpu context, for sequences of calls on one long-lived context
(tests/test_ctx_model_cpu.py checks it on the CPU, tests/test_gpu_sequences.py runs it on the device).

Not a new oracle: a composition of what the suite already has -- tests/oracle.py for the id set, the
accept mask, the cache mirror, the routing table and the crawl model; ncache_cases.Model and
rsearch_cases.Model / run_step for the resident NodeCache and searches; rtable_cases.expected for
the resident table.  The model keeps what a context keeps between calls; an op is a record
(name, args) with one applier onto the model (MODEL) and one onto an opendht_amd.Context (CTX);
run() applies both and returns (got, want) for a query, the expected error code included where
include/dhtgpu.h says the call fails.  walk() draws a seeded sequence whose every op meets the
header's preconditions; trace() says which (mutation, derived structure) pairs a sequence probes.
Test infrastructure only."""
import collections

import numpy as np

import ncache_cases as NC
import oracle as O
import rsearch_cases as RS
import rtable_cases as RT

NONE = 0xFFFFFFFF
EINVAL, ENOIDS, EUNSORTED, ERANGE = -1, -4, -5, -6
MAX_HANDLE = NC.MAX_HANDLE

Op = collections.namedtuple("Op", "name args")


def err(code):
    return ("error", int(code))


def is_err(r):
    return isinstance(r, tuple) and len(r) == 2 and isinstance(r[0], str) and r[0] == "error"


def same(got, want):
    """exact: the same error, or arrays equal one by one"""
    if is_err(got) or is_err(want):
        return is_err(got) and is_err(want) and got[1] == want[1]
    if got is None or want is None:
        return got is None and want is None
    if len(got) != len(want):
        return False
    return all(np.array_equal(np.asarray(g), np.asarray(w)) for g, w in zip(got, want))


def shape_of(x):
    """names and shapes for the op log, never array contents"""
    if isinstance(x, np.ndarray):
        return f"{x.dtype}{list(x.shape)}"
    if isinstance(x, (list, tuple, set)):
        return f"{type(x).__name__}[{len(x)}]"
    return repr(x)


def describe(op):
    return f"{op.name}({', '.join(shape_of(a) for a in op.args)})"


def lex_order(ids):
    return np.lexsort(ids.T[::-1])


def pack_bits(mask):
    """the device bitmask of dhtgpu_set_accept_bits_dev: id i = bit i & 31 of word i >> 5"""
    n = mask.shape[0]
    pad = np.zeros((n + 31) // 32 * 32, np.uint8)
    pad[:n] = mask != 0
    return np.packbits(pad.reshape(-1, 32), axis=1, bitorder="little").view("<u4").reshape(-1).astype(np.uint32)


def prefix_shard(seed, n, pbits, pval, start=0):
    """dhtgpu_gen_ids_prefix restated: (the shard's ids in stream order, their global indices)"""
    ids = O.gen_ids(seed, n, start)
    top = (ids[:, 0].astype(np.uint32) << 8 | ids[:, 1]) >> (16 - pbits) if pbits else np.zeros(n, np.uint32)
    sel = np.flatnonzero(top == pval)
    return np.ascontiguousarray(ids[sel]), (sel + start).astype(np.uint32)


# ---- the model --------------------------------------------------------------------------------------
class Model:
    def __init__(self):
        self.ids = None          # (n, 20) or None: no id set
        self.gidx = None         # prefix shard: the ids' global stream indices
        self.accept = None       # (n,) uint8 or None: no mask
        self.stream = None
        self.map_global = True
        self.sub_handles = False
        self.net = None          # (dead or None, seed): the crawl model stands; None: not prepared
        self.cache = None        # (keys, version)
        self.rt = None           # dict: myid firsts off nodes good tail af version
        self.sr = RS.Model()     # resident searches; its .nc is the resident NodeCache
        self.sr_valid = False

    @property
    def n(self):
        return 0 if self.ids is None else self.ids.shape[0]

    @property
    def shard(self):
        return self.gidx is not None

    def rejects(self):
        """the accept view is in use: a mask is set and rejects at least one id"""
        return self.accept is not None and not self.accept.all()

    # -- the id set
    def new_ids(self, ids, gidx=None, stream=None):
        self.ids = np.ascontiguousarray(ids, dtype=np.uint8).reshape(-1, 20).copy()
        self.gidx = gidx
        self.stream = stream     # prefix shard: (seed, n, pbits, pval) of dhtgpu_gen_ids_prefix
        self.accept = None       # dhtgpu_set_ids / gen_ids / gen_ids_prefix clear the mask
        self.net = None

    def write_ids(self, first, ids):
        self.ids[first: first + len(ids)] = ids      # keeps the mask
        self.net = None          # the crawl model needs dhtgpu_net_prepare again

    def out_index(self, local, base=0):
        """what a lookup returns for context-local indices (NONE stays)"""
        local = np.asarray(local, dtype=np.uint32)
        keep = local == NONE
        safe = np.where(keep, 0, local).astype(np.int64)
        out = self.gidx[safe] if (self.shard and self.map_global) else safe + base
        return np.where(keep, NONE, out).astype(np.uint32)

    def topk(self, targets, k, base=0):
        if self.ids is None:
            return err(ENOIDS)
        q = len(targets)
        sel = np.arange(self.n) if self.accept is None else np.flatnonzero(self.accept)
        if sel.size == 0:
            return np.full((q, k), NONE, np.uint32), np.zeros(q, np.uint32)
        want, cnt = O.topk(self.ids[sel], targets, k)
        local = np.where(want == NONE, NONE, sel[np.minimum(want, sel.size - 1)]).astype(np.uint32)
        return self.out_index(local, base), cnt

    def cached_nodes(self, targets, count, accept):
        if self.ids is None:
            return err(ENOIDS)
        order = lex_order(self.ids)
        acc = np.ones(self.n, np.uint8) if accept is None else np.asarray(accept, np.uint8)
        pos, cnt = O.cached_nodes_batch(self.ids[order], acc[order], targets, count, threads=8)
        local = np.where(pos == NONE, NONE, order[np.minimum(pos, self.n - 1)]).astype(np.uint32)
        return self.out_index(local), cnt

    def net_prepare(self, dead, seed):
        if self.ids is None or self.n == 0:
            return err(ENOIDS)
        if self.shard:
            return err(EINVAL)
        self.net = (None if dead is None else np.asarray(dead, np.uint8).copy(), int(seed))
        return None

    def search_batch(self, targets, searchers):
        if self.net is None:
            return err(ENOIDS)
        return O.search_batch(self.ids, self.net[0], self.net[1], targets, searchers)

    # -- the cache mirror
    def cache_set(self, keys, version):
        if version and self.cache is not None and version == self.cache[1] and len(keys) == len(self.cache[0]):
            return       # same version, same n: the upload is skipped
        self.cache = (np.ascontiguousarray(keys, dtype=np.uint8).copy(), int(version))

    def cache_sorted(self):
        if self.cache is None:
            return err(ENOIDS)
        return (lex_order(self.cache[0]).astype(np.uint32),)

    def cache_nodes(self, targets, count, accept):
        if self.cache is None:
            return err(ENOIDS)
        keys = self.cache[0]
        order = lex_order(keys)
        acc = np.ones(len(keys), np.uint8) if accept is None else np.asarray(accept, np.uint8)
        pos, cnt = O.cached_nodes_batch(keys[order], acc[order], targets, count, threads=8)
        return np.where(pos == NONE, NONE, order[np.minimum(pos, len(keys) - 1)]).astype(np.uint32), cnt

    # -- the resident routing table
    def rt_set(self, myid, firsts, off, nodes, tail, af, version):
        t = self.rt
        if version and t is not None and version == t["version"] and len(firsts) == len(t["firsts"]) and \
                len(nodes) == len(t["nodes"]):
            return       # same version, same bucket and node counts: skipped
        self.rt = {"myid": np.array(myid, np.uint8), "firsts": np.array(firsts, np.uint8), "off": np.array(off, np.uint32),
                   "nodes": np.array(nodes, np.uint8).reshape(-1, 20), "good": np.ones(len(nodes), np.uint8),
                   "tail": None if tail is None else np.array(tail, np.uint8), "af": af, "version": int(version)}

    def rt_case(self, targets):
        t = self.rt
        return {"firsts": t["firsts"], "off": t["off"], "nodes": t["nodes"], "good": t["good"],
                "targets": np.ascontiguousarray(targets, np.uint8)}

    def rt_find_closest(self, targets, count):
        if self.rt is None:
            return err(ENOIDS)
        return RT.expected(self.rt_case(targets), count)

    def rt_reply(self, targets):
        if self.rt is None:
            return err(ENOIDS)
        t = self.rt
        if t["tail"] is None:
            return err(EINVAL)
        idx, cnt = RT.expected(self.rt_case(targets), 8)
        alen = t["tail"].shape[1] - 2
        out = np.zeros((len(targets), 8 * (22 + alen)), np.uint8)
        ln = np.zeros(len(targets), np.uint32)
        for i, tg in enumerate(targets):
            b = O.buffer_nodes(t["nodes"], t["tail"], alen, tg, idx[i, : cnt[i]])
            out[i, : b.size] = b
            ln[i] = b.size
        return out, ln, idx

    # -- the resident NodeCache and searches (their own models)
    @property
    def nc(self):
        return self.sr.nc

    def nc_nodes(self, targets, count):
        if not self.sr.have_nc:
            return err(ENOIDS)
        return self.nc.expected(targets, count)

    def nc_export(self):
        if not self.sr.have_nc:
            return err(ENOIDS)
        return self.nc.sorted()


def clip_reply(r):
    """a reply's bytes past its length are unspecified: zero them"""
    if is_err(r):
        return r
    out, ln = r[0].copy(), r[1]
    for i in range(out.shape[0]):
        out[i, int(ln[i]):] = 0
    return (out, ln) + tuple(r[2:])


# ---- the device side ----------------------------------------------------------------------------------
class Device:
    """What the context-side appliers work with: the context, a peer context for the ops that take
    several, and a second stream."""

    def __init__(self, ctx, peer=None):
        import torch
        self.torch = torch
        self.ctx, self.peer = ctx, peer
        self.dev = torch.device("cuda", 0)
        self.side = torch.cuda.Stream(self.dev)
        self.keep = []      # device arrays a stream-ordered call may still read

    def planes(self, tg):
        """targets as device word planes: (tensor, stride)"""
        import opendht_amd
        torch = self.torch
        q = tg.shape[0]
        ts = (q + 63) // 64 * 64
        tp = torch.from_numpy(np.pad(opendht_amd.id_words(tg), ((0, 0), (0, ts - q))).view(np.int32).copy()).to(self.dev)
        torch.cuda.synchronize()
        return tp, ts

    def sync(self):
        self.torch.cuda.synchronize()
        self.keep.clear()


def guarded(fn):
    """a context call's result, or ("error", code)"""
    import opendht_amd
    try:
        return fn()
    except opendht_amd.DhtGpuError as e:
        return err(e.code)


# name -> (model applier, context applier); a query's appliers return its answer, a mutation's None
MODEL, CTX, QUERIES = {}, {}, set()


def op(name, query=False):
    def deco(pair):
        MODEL[name], CTX[name] = pair()
        if query:
            QUERIES.add(name)
        return pair
    return deco


# ---- id set --------------------------------------------------------------------------------------------
@op("set_ids")
def _():
    return (lambda m, ids: m.new_ids(ids)), (lambda d, ids: d.ctx.set_ids(ids))


@op("gen_ids")
def _():
    return (lambda m, seed, n: m.new_ids(O.gen_ids(seed, n))), (lambda d, seed, n: d.ctx.gen_ids(seed, n))


@op("gen_ids_prefix")
def _():
    return (lambda m, seed, n, pb, pv: m.new_ids(*prefix_shard(seed, n, pb, pv), stream=(seed, n, pb, pv))), \
           (lambda d, seed, n, pb, pv: d.ctx.gen_ids_prefix(seed, n, pb, pv))


@op("write_ids")
def _():
    return (lambda m, first, ids: m.write_ids(first, ids)), (lambda d, first, ids: d.ctx.write_ids(first, ids))


def _m_set_accept(m, mask):
    m.accept = None if mask is None else (np.asarray(mask) != 0).astype(np.uint8)


@op("set_accept")
def _():
    return _m_set_accept, (lambda d, mask: d.ctx.set_accept(mask))


def _m_update_accept(m, idx, val):
    if m.accept is None:
        m.accept = np.ones(m.n, np.uint8)    # with no mask set it starts from every id accepted
    m.accept[np.asarray(idx, np.int64)] = np.asarray(val) != 0


@op("update_accept")
def _():
    return _m_update_accept, (lambda d, idx, val: d.ctx.update_accept(idx, val))


def _c_bits_dev(d, mask):
    torch = d.torch
    with torch.cuda.stream(d.side):     # the copy is ordered on a stream that is not the context's
        bits = torch.from_numpy(pack_bits(np.asarray(mask)).view(np.int32)).to(d.dev)
        d.keep.append(bits)
        d.ctx.set_accept_bits_dev(bits.data_ptr(), d.side.cuda_stream)


@op("set_accept_bits_dev")
def _():
    return _m_set_accept, _c_bits_dev


def _m_flag(name):
    def f(m, on):
        setattr(m, name, bool(on))
    return f


@op("set_global_indices")
def _():
    return _m_flag("map_global"), (lambda d, on: d.ctx.set_global_indices(on))


@op("set_sub_handles")    # only sub-partitioned calls return handles: none at these sizes
def _():
    return _m_flag("sub_handles"), (lambda d, on: d.ctx.set_sub_handles(on))


for _name in ("topk", "index_topk", "batch_topk"):
    def _mk(name):
        return (lambda m, tg, k: m.topk(tg, k)), (lambda d, tg, k: guarded(lambda: getattr(d.ctx, name)(tg, k)))
    MODEL[_name], CTX[_name] = _mk(_name)
    QUERIES.add(_name)


def _c_topk_base(d, tg, k, base):
    torch = d.torch
    tp, ts = d.planes(tg)
    q = tg.shape[0]
    out = torch.full((q, k), -7, dtype=torch.int32, device=d.dev)
    cnt = torch.full((q,), -7, dtype=torch.int32, device=d.dev)
    r = guarded(lambda: d.ctx.topk_dev(tp.data_ptr(), ts, q, k, out.data_ptr(), cnt.data_ptr(), None, base, d.ctx.stream))
    torch.cuda.synchronize()
    return r if is_err(r) else (out.cpu().numpy().view(np.uint32), cnt.cpu().numpy().view(np.uint32))


@op("topk_base", query=True)      # dhtgpu_topk_dev with idx_base != 0: under a mask, through bmap
def _():
    return (lambda m, tg, k, base: m.topk(tg, k, base)), _c_topk_base


@op("num_accepted", query=True)
def _():
    def mod(m):
        if m.ids is None:
            return err(ENOIDS)
        return (np.uint64(m.n if m.accept is None else int(m.accept.sum())),)
    return mod, (lambda d: guarded(lambda: (np.uint64(d.ctx.num_accepted),)))


@op("get_ids", query=True)
def _():
    return (lambda m: err(ENOIDS) if m.ids is None else (m.ids,)), (lambda d: guarded(lambda: (d.ctx.get_ids(),)))


@op("cached_nodes", query=True)
def _():
    return (lambda m, tg, count, acc: m.cached_nodes(tg, count, acc)), \
           (lambda d, tg, count, acc: guarded(lambda: d.ctx.cached_nodes(tg, count, acc)))


@op("net_prepare")
def _():
    def mod(m, dead, seed):
        m.net_prepare(dead, seed)

    def dev(d, dead, seed):
        guarded(lambda: d.ctx.net_prepare(dead, seed))
    return mod, dev


@op("search_batch", query=True)
def _():
    return (lambda m, tg, who: m.search_batch(tg, who)), (lambda d, tg, who: guarded(lambda: d.ctx.search_batch(tg, who)))


@op("classify", query=True)
def _():
    def mod(m, firsts, myid):
        if m.ids is None:
            return err(ENOIDS)
        return O.classify(firsts, myid, m.ids)
    return mod, (lambda d, firsts, myid: guarded(lambda: d.ctx.classify(firsts, myid)))


def _peer_records(d, who, tg, k, base):
    torch = d.torch
    tp, ts = d.planes(tg)
    rec = torch.full((tg.shape[0], k, 3), -7, dtype=torch.int32, device=d.dev)
    who.topk_dev(tp.data_ptr(), ts, tg.shape[0], k, None, None, rec.data_ptr(), base, who.stream)
    torch.cuda.synchronize()
    return rec, tp, ts


def _c_peer_merge(d, ids2, tg, k):
    import merge_util as MU
    import opendht_amd
    torch = d.torch
    n1 = d.ctx.num_ids
    d.peer.set_ids(ids2)
    r1, tp, ts = _peer_records(d, d.ctx, tg, k, 0)
    r2, _, _ = _peer_records(d, d.peer, tg, k, n1)
    rec = torch.stack([r1, r2]).contiguous()
    L = opendht_amd.lib()
    idx, cnt, _ = MU.merge(L, rec, tp, ts, k, ("ctx", MU.ctx_words_fn(L, [d.ctx, d.peer], rec, [0, n1], k)))
    return idx, cnt


def _m_peer_merge(m, ids2, tg, k):
    sel = np.arange(m.n) if m.accept is None else np.flatnonzero(m.accept)
    allids = np.concatenate([m.ids[sel], ids2])
    where = np.concatenate([sel, m.n + np.arange(len(ids2))]).astype(np.uint32)
    want, cnt = O.topk(allids, tg, k)
    return np.where(want == NONE, NONE, where[np.minimum(want, len(where) - 1)]).astype(np.uint32), cnt


@op("peer_merge", query=True)     # two contexts: record-form top-k on each, K3 + the tie exchange over both
def _():
    return _m_peer_merge, _c_peer_merge


def _c_shard_merge(d, tg, k):
    import merge_util as MU
    import opendht_amd
    seed, n, pb, pv = d.shard_stream
    d.peer.gen_ids_prefix(seed, n, pb, 1 - pv)
    r1, tp, ts = _peer_records(d, d.ctx, tg, k, 0)
    r2, _, _ = _peer_records(d, d.peer, tg, k, 0)
    rec = d.torch.stack([r1, r2]).contiguous()
    L = opendht_amd.lib()
    idx, cnt, _ = MU.merge(L, rec, tp, ts, k, ("ctx", MU.ctx_words_fn(L, [d.ctx, d.peer], rec, [0, 0], k)))
    return idx, cnt


def _m_shard_merge(m, tg, k):
    seed, n, pb, pv = m.stream
    return O.topk(O.gen_ids(seed, n), tg, k)


@op("shard_merge", query=True)    # two contexts as the two 1-bit prefix shards of one stream: records by global
def _():                          # index from each, K3 + the tie exchange == the oracle over the whole stream
    def dev(d, tg, k):
        return _c_shard_merge(d, tg, k)
    return _m_shard_merge, dev


# ---- cache mirror --------------------------------------------------------------------------------------
@op("cache_set")
def _():
    return (lambda m, keys, ver: m.cache_set(keys, ver)), (lambda d, keys, ver: d.ctx.cache_set(keys, ver))


@op("cache_sorted", query=True)
def _():
    return (lambda m: m.cache_sorted()), (lambda d: guarded(lambda: (d.ctx.cache_sorted(),)))


@op("cache_nodes", query=True)
def _():
    return (lambda m, tg, count, acc: m.cache_nodes(tg, count, acc)), \
           (lambda d, tg, count, acc: guarded(lambda: d.ctx.cache_nodes(tg, count, acc)))


# ---- resident routing table ----------------------------------------------------------------------------
@op("rt_set")
def _():
    return (lambda m, *a: m.rt_set(*a)), (lambda d, my, f, off, nodes, tail, af, ver: d.ctx.rt_set(my, f, off, nodes, tail, af, ver))


def _m_rt_set_good(m, good):
    m.rt["good"] = (np.asarray(good) != 0).astype(np.uint8)


def _m_rt_update_good(m, idx, val):
    m.rt["good"][np.asarray(idx, np.int64)] = np.asarray(val) != 0


@op("rt_set_good")
def _():
    return _m_rt_set_good, (lambda d, good: d.ctx.rt_set_good(good))


@op("rt_update_good")
def _():
    return _m_rt_update_good, (lambda d, idx, val: d.ctx.rt_update_good(idx, val))


@op("rt_find_closest", query=True)
def _():
    return (lambda m, tg, count: m.rt_find_closest(tg, count)), \
           (lambda d, tg, count: guarded(lambda: d.ctx.rt_find_closest(tg, count)))


@op("rt_reply", query=True)
def _():
    return (lambda m, tg: clip_reply(m.rt_reply(tg))), \
           (lambda d, tg: clip_reply(guarded(lambda: d.ctx.rt_reply(tg, indices=True))))


# ---- resident NodeCache and searches: rsearch_cases.run_step, not restated (run() hands these ops to it:
# its model half and its context half are the two appliers) ---------------------------------------------
_SR_STEPS = {"sr_reset": "reset", "nc_set": "nc_set", "nc_insert": "nc_insert", "nc_erase": "nc_erase",
             "sr_open": "open", "sr_expire": "expire", "sr_set_state": "set_state",
             "sr_update_state": "update_state", "sr_set_candidate": "candidate", "sr_insert": "insert",
             "sr_refill": "refill"}


for _name in ("nc_insert", "nc_erase", "sr_insert", "sr_refill"):
    QUERIES.add(_name)      # they change state and return per-item results: both are compared


@op("nc_update_accept")
def _():
    return (lambda m, h, v: m.nc.update_accept(h, v)), (lambda d, h, v: d.ctx.nc_update_accept(h, v))


@op("nc_set_accept")
def _():
    return (lambda m, a: m.nc.set_accept(a)), (lambda d, a: d.ctx.nc_set_accept(a))


@op("nc_nodes", query=True)
def _():
    return (lambda m, tg, count: m.nc_nodes(tg, count)), (lambda d, tg, count: guarded(lambda: d.ctx.nc_nodes(tg, count)))


@op("nc_export", query=True)
def _():
    return (lambda m: m.nc_export()), (lambda d: guarded(lambda: d.ctx.nc_export()))


@op("sr_status", query=True)
def _():
    return (lambda m, s: (m.sr.status(s),) if m.sr_valid else err(ENOIDS)), \
           (lambda d, s: guarded(lambda: (d.ctx.sr_status(s),)))


@op("sr_lists", query=True)
def _():
    return (lambda m, s: m.sr.lists(s) if m.sr_valid else err(ENOIDS)), (lambda d, s: guarded(lambda: d.ctx.sr_lists(s)))


# ---- running --------------------------------------------------------------------------------------------
def run(o, model, dev=None, want=True):
    """One op on the model and (when given) the device: (got, want); (None, None) for a mutation.
    want=False skips a pure query's expectation (replays that only follow the state).  The nc / sr
    steps go through rsearch_cases.run_step, which applies its two halves itself."""
    if o.name in _SR_STEPS:
        w, g = RS.run_step((_SR_STEPS[o.name],) + tuple(o.args), model.sr, dev.ctx if dev is not None else None)
        if o.name == "sr_reset":
            model.sr_valid = True
        if o.name not in QUERIES:
            return None, None
        return (None if g is None else (g,)), (w,)
    w = MODEL[o.name](model, *o.args) if (want or o.name not in QUERIES) else None
    if dev is not None:
        dev.shard_stream = model.stream
    g = CTX[o.name](dev, *o.args) if dev is not None else None
    if o.name not in QUERIES:
        return None, None
    return g, w


def replay(ops, model, dev=None, seed=None, check=True):
    """Apply ops in order; every query's answer is compared exactly.  A failure names the seed, the
    step and the op log up to it (names and shapes)."""
    for i, o in enumerate(ops):
        got, want = run(o, model, dev)
        if check and dev is not None and o.name in QUERIES and not same(got, want):
            log = "\n".join(f"  {j:3d} {describe(p)}" for j, p in enumerate(ops[: i + 1]))
            raise AssertionError(f"seed {seed}: step {i} {describe(o)} disagrees with the model\n"
                                 f"got  {summary(got)}\nwant {summary(want)}\nops so far:\n{log}")


def summary(r):
    if is_err(r) or r is None:
        return repr(r)
    return ", ".join(shape_of(np.asarray(a)) for a in r)


# ---- the stale-structure matrix -----------------------------------------------------------------------
# derived structure -> the query that builds and reads it (DESIGN.md §2 lists the flags)
STRUCTURES = ("index", "view_index", "bmap", "sview", "net", "k6")
MUTATIONS = ("set_ids_same", "set_ids_smaller", "set_ids_larger", "gen_ids", "gen_ids_prefix1", "gen_ids_prefix3",
             "write_ids_one", "write_ids_run", "write_ids_last", "set_accept", "update_accept", "set_accept_none",
             "set_accept_bits_dev", "set_global_indices", "set_sub_handles")
MATRIX = [(mu, st) for st in STRUCTURES for mu in MUTATIONS]
SIZES_N = (4097, 70001)
SIZES_Q = (65, 300)
SIZES_K = (8, 14)
BASES = (1000, 77)
START_N = (4097, 70001 - 903)    # where a walk starts: set_ids_larger adds 903 ids, up to 70,001


def structure_query(st, rng, model, alt=0, near=None):
    """the ops that read structure st (building it first where a call of its own does that); near:
    ids to aim some targets at (the ids a mutation just wrote: a stale structure answers them wrong)"""
    q, k = int(rng.choice(SIZES_Q)), int(rng.choice(SIZES_K))
    tg = O.gen_ids(int(rng.integers(1, 1 << 30)), q)
    if near is not None and len(near):
        m = min(len(near), 16)
        tg[:m] = near[:m]
        tg[m: 2 * m, :19] = near[:m, :19]      # and next to them
    if st == "index" or st == "view_index":
        return [Op("index_topk", (tg, k))]
    if st == "bmap":
        return [Op("topk_base", (tg, k, BASES[alt % 2]))]
    if st == "sview":
        return [Op("cached_nodes", (tg, 14, None))]
    if st == "net":
        who = rng.integers(0, max(model.n, 1), size=q).astype(np.uint32)
        return [Op("search_batch", (tg, who))]
    if st == "k6":
        return [Op("batch_topk", (tg, k))]
    raise ValueError(st)


def structure_setup(st, rng, model):
    """ops that bring the model to where st's query builds st (a rejecting mask for the view's
    structures, a prepared crawl model)"""
    ops = []
    if model.ids is None:
        n = int(rng.choice(START_N))
        ops.append(Op("set_ids", (O.gen_ids(int(rng.integers(1, 1 << 30)), n),)))
    else:
        n = model.n
    if st in ("view_index", "bmap") and not model.rejects():
        mask = (rng.random(n) < 0.6).astype(np.uint8)
        mask[0], mask[-1] = 0, 1        # rejects at least one id; the last id stays visible
        ops.append(Op("set_accept", (mask,)))
    if st == "net" and model.net is None and not model.shard:
        dead = (rng.random(n) < 0.1).astype(np.uint8) if rng.random() < 0.5 else None
        ops.append(Op("net_prepare", (dead, int(rng.integers(1, 1 << 20)))))
    return ops


def mutation_ops(mu, rng, model):
    """the ops of one mutation kind over the model's current id set, or None where the header
    forbids it there (write_ids on a prefix shard)"""
    n = model.n
    seed = int(rng.integers(1, 1 << 30))
    if mu == "set_ids_same":
        return [Op("set_ids", (O.gen_ids(seed, n),))]
    if mu == "set_ids_smaller":
        return [Op("set_ids", (O.gen_ids(seed, max(n - 1094, 1000)),))]
    if mu == "set_ids_larger":
        return [Op("set_ids", (O.gen_ids(seed, min(n + 903, SIZES_N[1])),))]
    if mu == "gen_ids":
        return [Op("gen_ids", (seed, n))]
    if mu in ("gen_ids_prefix1", "gen_ids_prefix3"):
        pb = 1 if mu.endswith("1") else 3
        # a stream long enough that the shard holds about n ids
        return [Op("gen_ids_prefix", (seed, min(n << pb, SIZES_N[1] << 1), pb, int(rng.integers(0, 1 << pb))))]
    if mu.startswith("write_ids"):
        if model.shard or n == 0:
            return None
        m = {"write_ids_one": 1, "write_ids_run": min(257, n), "write_ids_last": 1}[mu]
        first = n - 1 if mu == "write_ids_last" else int(rng.integers(0, n - m + 1))
        if mu == "write_ids_one" and model.rejects():      # a slot the mask shows
            first = int(rng.choice(np.flatnonzero(model.accept)))
        return [Op("write_ids", (first, O.gen_ids(seed, m)))]
    if mu == "set_accept":
        return [Op("set_accept", ((rng.random(n) < 0.5).astype(np.uint8),))]
    if mu == "set_accept_bits_dev":
        return [Op("set_accept_bits_dev", ((rng.random(n) < 0.5).astype(np.uint8),))]
    if mu == "update_accept":
        m = min(257, n)
        return [Op("update_accept", (rng.choice(n, m, replace=False).astype(np.uint32), (rng.random(m) < 0.5).astype(np.uint8)))]
    if mu == "set_accept_none":
        return [Op("set_accept", (None,))]
    if mu == "set_global_indices":
        return [Op("set_global_indices", (not model.map_global,))]
    if mu == "set_sub_handles":
        return [Op("set_sub_handles", (not model.sub_handles,))]
    raise ValueError(mu)


def matrix_script(mu, st):
    """The scripted row (mu, st) of the matrix: build st by its query, mutate, ask again.  Sizes: n
    alternates over SIZES_N with the row's place in MATRIX (so every structure meets both), q and k
    are drawn from SIZES_Q / SIZES_K.  The set_global_indices rows start on a prefix shard, where the
    setting matters (the crawl model's on a plain set: a shard has none); after a gen_ids_prefix
    mutation the row goes back to set_ids and asks once more.  Returns (ops, index of the mutation)."""
    i = MATRIX.index((mu, st))
    rng = np.random.default_rng([i, 0x5E])
    n = SIZES_N[(i + i // len(MUTATIONS)) % 2]
    model = Model()
    ops = [Op("set_global_indices", (True,)), Op("set_sub_handles", (False,))]   # the context is long-lived
    if mu == "set_global_indices" and st != "net":
        ops.append(Op("gen_ids_prefix", (int(rng.integers(1, 1 << 30)), 2 * n, 1, 1)))
        if st == "bmap":
            ops.append(Op("set_global_indices", (False,)))     # a shard's global map answers instead of bmap
    else:
        ops.append(Op("set_ids", (O.gen_ids(int(rng.integers(1, 1 << 30)), n),)))

    def grow(more):
        for o in more:
            run(o, model, None, want=False)
        ops.extend(more)
    first, ops[:] = list(ops), []
    grow(first)
    grow(structure_setup(st, rng, model))
    grow(structure_query(st, rng, model, 0))
    at = len(ops)
    mut = mutation_ops(mu, rng, model)
    grow(mut)
    grow(structure_query(st, rng, model, 1, written(mut, model)))
    if st == "net":      # the set's K4 index standing again (search_batch reads it too) must not bring the model back
        grow([Op("index_topk", (O.gen_ids(int(rng.integers(1, 1 << 30)), 65), 8))])
        grow(structure_query(st, rng, model, 1, written(mut, model)))
    if st == "net" and not model.shard:      # prepared again, it answers over the new ids
        grow([Op("net_prepare", (None, 77))])
        grow(structure_query(st, rng, model, 0))
    if model.shard and mu.startswith("gen_ids_prefix"):
        grow([Op("set_ids", (O.gen_ids(int(rng.integers(1, 1 << 30)), n),))])
        grow(structure_setup(st, rng, model))
        grow(structure_query(st, rng, model, 0))
    return ops, at


def written(ops, model):
    """ids a mutation's ops put into the set (up to 16), for the targets of the query that follows"""
    for o in ops:
        if o.name == "write_ids":
            return o.args[1][:16]
        if o.name == "set_ids":
            return o.args[0][:16]
    return model.ids[:16] if model.ids is not None else None


def kind_of(o, model):
    """the mutation kind of an id-family op as the model stands before it (None: not one)"""
    a = o.args
    if o.name == "set_ids":
        if model.ids is None:
            return None
        return "set_ids_same" if len(a[0]) == model.n else "set_ids_smaller" if len(a[0]) < model.n else "set_ids_larger"
    if o.name == "gen_ids":
        return "gen_ids"
    if o.name == "gen_ids_prefix":
        return {1: "gen_ids_prefix1", 3: "gen_ids_prefix3"}.get(a[2])
    if o.name == "write_ids":
        if len(a[1]) > 1:
            return "write_ids_run"
        return "write_ids_last" if a[0] == model.n - 1 else "write_ids_one"
    if o.name == "set_accept":
        return "set_accept_none" if a[0] is None else "set_accept"
    if o.name in ("update_accept", "set_accept_bits_dev", "set_global_indices", "set_sub_handles"):
        return o.name
    return None


def reads(o, model):
    """the derived structure an op reads (and builds when it is not standing), as the model stands"""
    if o.name == "index_topk":
        return "view_index" if model.rejects() else "index"
    if o.name == "topk_base" and model.rejects() and not (model.shard and model.map_global) and o.args[2]:
        return "bmap"
    if o.name == "cached_nodes":
        return "sview"
    if o.name == "search_batch" and model.net is not None:
        return "net"
    if o.name == "batch_topk":
        return "k6"
    return None


def trace(ops, model=None):
    """Which (mutation, structure) pairs a sequence probes: a query that reads the structure (and
    so leaves it built), then the mutation, then the same query again with nothing in between that
    rebuilds the structure -- the same query in between starts over, and so does net_prepare for
    the crawl model and the set's K4 index, both of which it rebuilds."""
    model = model or Model()
    open_ = {}       # query name -> (the structure it read, the mutation kinds since)
    pairs = set()
    for o in ops:
        if o.name in open_:
            st, mus = open_.pop(o.name)
            pairs.update((mu, st) for mu in mus)
        st = reads(o, model)
        if st is not None:
            open_[o.name] = (st, [])
        mu = kind_of(o, model)
        if mu is not None:
            for _, mus in open_.values():
                mus.append(mu)
        if o.name == "net_prepare":
            for name in [nm for nm, (st, _) in open_.items() if st in ("net", "index")]:
                open_[name] = (open_[name][0], [])
        run(o, model, None, want=False)
    return pairs


# ---- the seeded walk -----------------------------------------------------------------------------------
def rt_table(seed, nnodes=3000, nb=200, af=4):
    """a table of nnodes nodes in nb buckets (rtable_cases' synthetic cut) with address tails:
    rt_set's arguments but the version"""
    ids = RT.sorted_ids(seed, nnodes)
    firsts, off = RT.cut(ids, RT.sizes_for(nb, nnodes, seed))
    tail = np.random.default_rng(seed).integers(0, 256, size=(nnodes, (4 if af == 4 else 16) + 2), dtype=np.uint8)
    return O.gen_ids(seed + 9, 1)[0], firsts, off, ids, tail, af


class Walker:
    """Draws ops over every family so that each meets include/dhtgpu.h's preconditions as the model
    stands: distinct indices / handles / slots per call, unique nc keys, one handle per key below
    DHTGPU_NC_MAX_HANDLE, in-range indices, write_ids on plain contexts only.  Every call is issued
    on the context's stream or synchronised before the next op, so no nc mutation meets a pending
    _dev lookup."""

    def __init__(self, seed, nops=40):
        self.seed, self.nops = seed, nops
        self.rng = np.random.default_rng([seed, 0xC7])
        self.model = Model()
        self.ops = []
        self.next_handle = 100000 + 1000 * (seed % 50)
        self.rt_version = 0
        self.cache_version = 0
        self.turn = collections.Counter()

    def pick(self, what, ncases):
        """the cases of a family in turn, starting at the seed: a run of seeds meets every one"""
        c = (self.seed + self.turn[what]) % ncases
        self.turn[what] += 1
        return c

    def emit(self, ops):
        for o in ops:
            run(o, self.model, None, want=False)
            self.ops.append(o)

    def tg(self, q):
        return O.gen_ids(int(self.rng.integers(1, 1 << 30)), q)

    # one probe of the matrix: build, mutate, ask again
    def probe(self, pair=None):
        rng, m = self.rng, self.model
        mu, st = pair if pair is not None else MATRIX[int(rng.integers(0, len(MATRIX)))]
        if m.shard and (mu.startswith("write_ids") or st == "net"):
            self.emit([Op("set_ids", (O.gen_ids(int(rng.integers(1, 1 << 30)), int(rng.choice(START_N))),))])
        self.emit(structure_setup(st, rng, m))
        self.emit(structure_query(st, rng, m, 0))
        mut = mutation_ops(mu, rng, m)
        self.emit(mut)
        self.emit(structure_query(st, rng, m, 1, written(mut, m)))

    def cache(self):
        rng, m = self.rng, self.model
        c = self.pick("cache", 3)
        if m.cache is None or c == 0:
            self.cache_version += 1
            n = int(rng.choice((1000, 4097)))
            self.emit([Op("cache_set", (O.gen_ids(int(rng.integers(1, 1 << 30)), n), int(rng.choice((0, self.cache_version)))))])
        elif c == 1:      # the same version and n with other keys: documented to be skipped
            n = len(m.cache[0])
            self.emit([Op("cache_set", (O.gen_ids(int(rng.integers(1, 1 << 30)), n), m.cache[1]))])
        n = len(m.cache[0])
        self.emit([Op("cache_sorted", ()), Op("cache_nodes", (self.tg(65), 14, (rng.random(n) < 0.8).astype(np.uint8)))])

    def rt(self):
        rng, m = self.rng, self.model
        c = self.pick("rt", 4)
        if m.rt is None or c == 0:
            self.rt_version += 1
            self.emit([Op("rt_set", rt_table(int(rng.integers(1, 1 << 20)), int(rng.choice((700, 3000)))) + (self.rt_version,))])
        nn = len(m.rt["nodes"])
        if c == 1:
            self.emit([Op("rt_set_good", ((rng.random(nn) < 0.7).astype(np.uint8),))])
        elif c >= 2:
            k = int(rng.choice((1, 257)))
            self.emit([Op("rt_update_good", (rng.choice(nn, k, replace=False).astype(np.uint32), (rng.random(k) < 0.4).astype(np.uint8)))])
        self.emit([Op("rt_find_closest", (self.tg(65), int(rng.choice(SIZES_K)))), Op("rt_reply", (self.tg(17),))])

    def fresh_handles(self, k):
        h = np.arange(self.next_handle, self.next_handle + k, dtype=np.uint32)
        self.next_handle += k
        return h

    def nc(self):
        rng, m = self.rng, self.model
        c = self.pick("nc", 5)
        if not m.sr.have_nc or c == 0:
            n = int(rng.choice((600, 4097)))
            self.emit([Op("nc_set", (O.gen_ids(int(rng.integers(1, 1 << 30)), n), self.fresh_handles(n)))])
        held = np.array(sorted(m.nc.map.values()), dtype=np.uint32)
        if c == 1:
            k = int(rng.choice((1, 64, 257)))
            ids, _, acc = NC.mutation_batch(m.nc, k, int(rng.integers(1, 1 << 30)), 0)
            self.emit([Op("nc_insert", (ids, self.fresh_handles(k), acc))])
        elif c == 2 and held.size:
            keys = list(m.nc.map.keys())
            pick = rng.choice(len(keys), min(50, len(keys)), replace=False)
            ids = np.frombuffer(b"".join(keys[int(i)] for i in pick), dtype=np.uint8).reshape(-1, 20).copy()
            ids[-1] = 0x5A       # an absent key
            self.emit([Op("nc_erase", (np.ascontiguousarray(ids),))])
        elif c == 3 and held.size:
            k = min(int(rng.choice((1, 257))), held.size)
            self.emit([Op("nc_update_accept", (rng.choice(held, k, replace=False).astype(np.uint32), (rng.random(k) < 0.5).astype(np.uint8)))])
        elif c == 4 and held.size and int(held.max()) < (1 << 22):
            self.emit([Op("nc_set_accept", ((rng.random(int(held.max()) + 1) < 0.7).astype(np.uint8),))])
        self.emit([Op("nc_nodes", (self.tg(65), int(rng.choice(SIZES_K))))])
        if c == 1:
            self.emit([Op("nc_export", ())])

    def sr(self):
        rng, m = self.rng, self.model
        nslots = 40
        slots = np.arange(nslots, dtype=np.uint32)
        c = self.pick("sr", 7)
        if not m.sr_valid or c == 0:
            state = np.zeros(2200, np.uint8)
            state[2000 + rng.choice(200, 20, replace=False)] = 2      # removable only: never "bad"
            self.emit([Op("sr_reset", (nslots,)), Op("sr_set_state", (state,)), Op("sr_open", (slots, self.tg(nslots)))])
        if not any(sl.row for sl in m.sr.slots):
            node = rng.integers(0, 200, size=nslots * 4)
            self.emit([Op("sr_insert", (slots, RS.csr(np.full(nslots, 4)), (2000 + node).astype(np.uint32),
                                        O.gen_ids(777, 200)[node], None))])
        some = rng.permutation(nslots)[: int(rng.integers(1, nslots + 1))].astype(np.uint32)
        listed = sorted({h for sl in m.sr.slots for h in sl.row})
        bad = {h for h, v in m.sr.state.items() if v & 1} | {sl.row[j] for sl in m.sr.slots for j in range(len(sl.row)) if sl.flags[j] & 1}
        room = RS.MAX_BAD - len(bad)      # exact cases never overflow: at most MAX_BAD handles are ever bad
        if c == 1 and m.sr.have_nc:
            self.emit([Op("sr_refill", (some, 14))])
        elif c == 2:
            per = 3
            node = rng.integers(0, 200, size=some.size * per)
            pool = O.gen_ids(777, 200)       # the reply nodes: fixed ids, fixed handles (one handle per id)
            self.emit([Op("sr_insert", (some, RS.csr(np.full(some.size, per)), (2000 + node).astype(np.uint32), pool[node],
                                        (rng.random(node.size) < 0.4).astype(np.uint8)))])
        elif c == 3 and listed and room >= 4:
            pick = rng.choice(len(listed), min(3, len(listed)), replace=False)
            self.emit([Op("sr_update_state", (np.array([listed[int(i)] for i in pick], np.uint32), np.ones(len(pick), np.uint8)))])
        elif c == 4 and listed and room >= 2:
            h = listed[int(rng.integers(0, len(listed)))]
            on = [s for s in range(nslots) if h in m.sr.slots[s].row][:8] or [0]
            self.emit([Op("sr_set_candidate", (np.array(on, np.uint32), np.full(len(on), h, np.uint32), np.ones(len(on), np.uint8)))])
        elif c == 5:
            self.emit([Op("sr_expire", (some[:3],))])
        elif c == 6:
            self.emit([Op("sr_open", (some[:5], self.tg(min(5, some.size))))])
        self.emit([Op("sr_status", (slots,)), Op("sr_lists", (slots,))])

    def misc(self):
        rng, m = self.rng, self.model
        c = self.pick("misc", 5)
        if m.ids is None:
            return
        if c == 4:      # the context and its peer as the two halves of one stream
            self.emit([Op("gen_ids_prefix", (int(rng.integers(1, 1 << 30)), 2 * SIZES_N[0], 1, int(rng.integers(0, 2)))),
                       Op("set_global_indices", (True,)), Op("shard_merge", (self.tg(65), int(rng.choice(SIZES_K))))])
            return
        if c == 0:
            self.emit([Op("num_accepted", ()), Op("topk", (self.tg(int(rng.choice((17,) + SIZES_Q))), int(rng.choice(SIZES_K))))])
        elif c == 1:
            myid = O.gen_ids(int(rng.integers(1, 1 << 20)), 1)[0]
            firsts = O.Table(myid).grow(O.gen_ids(5, 400)).export()[0]
            self.emit([Op("classify", (firsts, myid))])
        elif c == 2 and not m.shard:
            self.emit([Op("peer_merge", (O.gen_ids(int(rng.integers(1, 1 << 30)), 3001), self.tg(65), 8))])
        else:
            self.emit([Op("get_ids", ())])

    def walk(self, pairs=()):
        """about nops ops: the families in a shuffled round, matrix probes in between (pairs: probes
        to take first, else drawn)"""
        pairs = list(pairs)
        fams = [self.cache, self.rt, self.nc, self.sr, self.misc]
        # before anything is set: the documented ENOIDS of every resident family's queries
        self.emit([Op("nc_nodes", (self.tg(5), 8)), Op("rt_find_closest", (self.tg(5), 8)), Op("cache_sorted", ()),
                   Op("sr_status", (np.arange(2, dtype=np.uint32),)), Op("topk", (self.tg(5), 8))])
        while len(self.ops) < self.nops:
            self.probe(pairs.pop(0) if pairs else None)
            fams[self.pick("family", len(fams))]()
        return self.ops


WALK_SEEDS = tuple(range(12))    # tests/test_ctx_model_cpu.py asserts what this list must cover


def walk(seed, nops=40):
    """The seeded sequence (replayable from the seed alone).  The probes a seed takes first are four
    of the matrix's pairs, taken in strides of 23 (coprime to the matrix's 90) from seed * 4, so that
    a run of seeds sweeps every structure; the rest is drawn."""
    first = [MATRIX[(seed * 4 + j) * 23 % len(MATRIX)] for j in range(4)]
    return Walker(seed, nops).walk(first)
