"""Inputs at the ends of the value ranges, shared by test_extremes_cpu.py and test_gpu_extremes.py.

The other case tables vary shapes; this one varies values.  It holds the inputs at which the
kernels' padding and packing conventions meet real data:

  A  distances whose leading words equal DHT_NONE (0xFFFFFFFF), the word that pads every candidate
     list and marks an empty slot -- whole rows of such candidates, and n = k sets at distance
     2^160 - 1;
  B  result indices at and above 2^31 and up to 0xFFFFFFFE (idx_base, prefix shards' global map),
     with duplicated ids whose copies lie on both sides of 2^31;
  C  the keys 00..00, 00..01, 7F..FF, 80..00, FF..FE, FF..FF as keys and as targets of the
     lexicographic families;
  D  resident-search scripts whose handles are counted down from 2^28 - 1, the top of the 28-bit
     handle field that shares a word with the two flag bits.

Everything here is host data; the expected answers come from the oracle and the families' models.
"""
import numpy as np

import ncache_cases as NC
import oracle as O
import rsearch_cases as RS
import srmap_cases as SM

NONE = 0xFFFFFFFF
TOP = 1 << 31


def words(ids):
    """(n, 20) big-endian bytes -> (n, 5) uint32 words"""
    return np.ascontiguousarray(ids, dtype=np.uint8).view(">u4").reshape(-1, 5).astype(np.uint32)


def put_words(ids, rows, first, vals):
    """ids[rows, word first ...] = vals (uint32 words, big-endian)"""
    b = np.array(vals, dtype=">u4").view(np.uint8)
    ids[rows, 4 * first:4 * first + b.size] = b


def key(hexbyte_first, fill, last=None):
    k = np.full(20, fill, np.uint8)
    k[0] = hexbyte_first
    if last is not None:
        k[19] = last
    return k


# ---- A: sentinel distances -------------------------------------------------------------------------
FAR_N, FAR_Q = 3000, 80
FAR_FREE = (17, 1500, 2999)          # the ids outside the cluster
FAR_ROWS = np.arange(40)             # the targets at sentinel distance of the cluster
FAR_KS = (8, 32)
# far-w0: an arbitrary shared word; far-w0w1: the shared words are 0xFFFFFFFF themselves, so the
# 12-byte records carry {DHT_NONE, DHT_NONE, idx} as id words and, for the complemented targets
# (words 0), as distances too
FAR_SHARED = {"far-w0": (0x5A3C9E17,), "far-w0w1": (0xFFFFFFFF, 0xFFFFFFFF)}


def far_case(name):
    """(ids, targets, cluster mask).  Targets 0..39: the cluster's shared words complemented; 40..59:
    the shared words themselves (distance 0 on them); 60..79: hashed.  The first 8 targets (the
    small-batch call) are all of the first kind."""
    shared = FAR_SHARED[name]
    seed = 7100 + len(shared)
    ids = O.gen_ids(seed, FAR_N)
    cluster = np.ones(FAR_N, bool)
    cluster[list(FAR_FREE)] = False
    put_words(ids, cluster, 0, shared)
    tg = O.gen_ids(seed + 50, FAR_Q)
    put_words(tg, np.arange(0, 40), 0, [~w & NONE for w in shared])
    put_words(tg, np.arange(40, 60), 0, shared)
    return ids, tg, cluster


def antipode_case(k):
    """n = k ids (00..00, FF..FF, 00..01, 80..00, hashed) and the targets 00..00, FF..FF and the
    complement of every id: row 2 + i ends with id i at distance 2^160 - 1."""
    ids = O.gen_ids(7200 + k, k)
    ids[0], ids[1] = 0x00, 0xFF
    ids[2] = key(0x00, 0x00, 0x01)
    ids[3] = key(0x80, 0x00)
    tg = np.concatenate([ids[:2], ~ids])
    return ids, np.ascontiguousarray(tg)


def id_range_bounds(n, lists):
    return [int(x) for x in np.linspace(0, n, lists + 1)]


def records_from_rows(ids, rows, cnt, gidx):
    """(q, k, 3) compact records {w0, w1, global index} of oracle rows, NONE padded"""
    w = words(ids)
    q, k = rows.shape
    rec = np.full((q, k, 3), NONE, np.uint32)
    for i in range(q):
        li = rows[i, :int(cnt[i])].astype(np.int64)
        rec[i, :li.size, :2] = w[li, :2]
        rec[i, :li.size, 2] = gidx[li]
    return rec


# ---- B: indices at the top of the range ----------------------------------------------------------------
TOP_N = 4096
BASE_CROSS = 0x7FFFFF00              # local index 256 is global 2^31
BASE_LAST = NONE - TOP_N             # the last id is 0xFFFFFFFE: the last base a set of TOP_N ids accepts
TOP_DUP = (100, 2000, 200)           # ids[2000:2200] = ids[100:300]: pairs 100..255 straddle BASE_CROSS + 256


def top_case():
    """(ids, targets): 4,096 hashed ids, 200 of them twice; 80 members (duplicated ones, the first
    and the last id among them) and 80 hashed targets."""
    ids = O.gen_ids(7300, TOP_N)
    a, b, m = TOP_DUP
    ids[b:b + m] = ids[a:a + m]
    member = np.r_[np.arange(a, a + m, 5), [0, 255, 256, TOP_N - 1], np.arange(300, 300 + 36 * 97, 97)]
    assert member.size == 80
    tg = np.concatenate([ids[member], O.gen_ids(7301, 80)])
    tg[4:8] = ids[[TOP_N - 1, 255, 256, 0]]     # the first 8 (the small-batch call): four straddling pairs + the ends
    return ids, np.ascontiguousarray(tg)


def add_base(rows, base):
    """oracle rows + base as uint32, NONE kept"""
    return np.where(rows == NONE, rows, (rows.astype(np.uint64) + base).astype(np.uint32)).astype(np.uint32)


def top_mask(n=TOP_N):
    """rejects a third of the ids (one copy of some duplicated pairs among them)"""
    return (np.arange(n) % 3 != 1).astype(np.uint8)


TOP_FLIP = np.r_[np.arange(1, 400, 3), np.arange(0, 400, 6)].astype(np.uint32)   # the mask update: on, then off


def top_mask_updated():
    m = top_mask()
    m[TOP_FLIP[:133]] = 1
    m[TOP_FLIP[133:]] = 0
    return m


def masked_topk(ids, mask, tg, k):
    """oracle rows over the accepted ids, as indices of the whole set"""
    sel = np.nonzero(mask)[0].astype(np.uint32)
    rows, cnt = O.topk(ids[sel], tg, k)
    return np.where(rows == NONE, rows, sel[np.minimum(rows, sel.size - 1)]).astype(np.uint32), cnt


SHARD_SEED, SHARD_N = 7400, 8192
SHARD_START = NONE - SHARD_N         # the stream's last id has global index 0xFFFFFFFE


def shard_case():
    """(ids of the stream, targets, [local -> stream position] of prefix shards 0 and 1)"""
    ids = O.gen_ids(SHARD_SEED, SHARD_N, SHARD_START)
    tg = np.concatenate([O.gen_ids(SHARD_SEED + 1, 150), ids[[0, 1, 2, 3, 4095, 4096, SHARD_N - 4, SHARD_N - 3,
                                                               SHARD_N - 2, SHARD_N - 1]]])
    sel = [np.nonzero((ids[:, 0] >> 7) == p)[0] for p in (0, 1)]
    return ids, np.ascontiguousarray(tg), sel


MERGE_DUP_SHAPES = [(3, 14, 2), (8, 8, 4)]     # (lists, k, seed): seeds whose shuffle leaves duplicated ids on both sides


def merge_dup_case(lists, seed):
    """test_gpu_parity.test_merge_heads_ties_duplicates' construction: (ids, targets, bounds)"""
    rng = np.random.default_rng(seed)
    n, q = 4000, 300
    ids = O.gen_ids(600 + seed, n)
    ids[: n // 3, :8] = ids[0, :8]
    ids[n // 2: n // 2 + 40] = ids[10:50]
    ids = ids[rng.permutation(n)]
    tg = O.gen_ids(700 + seed, q)
    tg[: q // 2, :8] = O.gen_ids(600 + seed, 1)[0, :8]
    cuts = np.sort(rng.integers(0, n, size=lists - 1))
    if lists > 2:
        cuts[0] = cuts[1]
    return ids, tg, [0] + [int(c) for c in cuts] + [n]


def raised_words_fn(ids, rec_host, base):
    """merge_util.host_words_fn for records whose indices are global index + base"""
    w = words(ids)

    def fn(j, rows, out):
        g = rec_host[j][rows][..., 2]
        o = np.full(g.shape + (3,), NONE, np.uint32)
        ok = g != NONE
        o[ok] = w[g[ok].astype(np.int64) - base, 2:5]
        return o
    return fn


# ---- C: boundary keys ----------------------------------------------------------------------------------
BOUNDARY = np.stack([key(0x00, 0x00), key(0x00, 0x00, 0x01), key(0x7F, 0xFF), key(0x80, 0x00),
                     key(0xFF, 0xFF, 0xFE), key(0xFF, 0xFF)])
WALK_COUNTS = (1, 8, 14)
CLOSEST_COUNTS = (1, 8, 32)


def boundary_keys():
    """the six boundary keys and 500 hashed ones, in lexicographic order"""
    keys = np.concatenate([BOUNDARY, O.gen_ids(7500, 500)])
    return np.ascontiguousarray(keys[np.lexsort(keys.T[::-1])])


def boundary_targets():
    """the boundary keys, each with its last byte one lower and one higher where the byte allows it,
    and 20 hashed targets"""
    rows = [BOUNDARY]
    for b in BOUNDARY:
        for d in (-1, 1):
            if 0 <= int(b[19]) + d <= 255:
                t = b.copy()
                t[19] = int(b[19]) + d
                rows.append(t[None, :])
    rows.append(O.gen_ids(7501, 20))
    return np.ascontiguousarray(np.concatenate(rows))


def is_boundary(keys):
    return np.array([any(np.array_equal(k, b) for b in BOUNDARY) for k in keys])


def ends_mask(sorted_keys):
    """only 00..00 and FF..FF accepted"""
    m = np.zeros(sorted_keys.shape[0], np.uint8)
    m[[0, -1]] = 1
    return m


def shuffled(keys, seed):
    """(keys in caller order, order): keys[order] is sorted"""
    perm = np.random.default_rng(seed).permutation(keys.shape[0])
    sh = np.ascontiguousarray(keys[perm])
    return sh, np.lexsort(sh.T[::-1])


def sort_case(name):
    """Key sets for the device sort, shuffled.  tile / tile+1: 4,096 and 4,097 keys -- the boundary
    keys, the others equal to 00..00 or FF..FF in words 0 and 1, so the 64-bit shortcut fails and
    all 20 passes run, with digits 0 and 255 only in 8 of them; word4: 300 keys that differ in word
    4 only."""
    if name == "word4":
        keys, _ = NC.clustered(seed=75, n=300)
        return shuffled(keys, 76)[0]
    n = {"tile": 4096, "tile+1": 4097}[name]
    rest = O.gen_ids(7600 + n, n - 6)
    rest[0::2, :8] = 0x00
    rest[1::2, :8] = 0xFF
    return shuffled(np.concatenate([BOUNDARY, rest]), n)[0]


SORT_CASES = ("tile", "tile+1", "word4")
TABLE_MYIDS = {"my=FF..FF": key(0xFF, 0xFF), "my=00..00": key(0x00, 0x00)}


def table_case(name):
    """(myid, firsts, bucket offsets, nodes) of the routing table grown from the boundary key set"""
    myid = TABLE_MYIDS[name]
    keys, _ = shuffled(boundary_keys(), 77)
    keys = np.concatenate([BOUNDARY, keys[~is_boundary(keys)]])   # the boundary keys first: they find room
    firsts, off, nodes = O.Table(myid).grow(keys).export()
    return myid, firsts, off, nodes


# ---- D: top-of-range handles ------------------------------------------------------------------------------
HANDLE_TOP = NC.MAX_HANDLE - 1      # 2^28 - 1: every bit of the handle field
# the argument that holds handles, per step kind (None: the step names none)
HANDLE_ARG = {"candidate": 1, "update_state": 0, "offer": 0, "nc_insert": 1, "insert": 2, "nc_erase": None, "open": None,
              "expire": None, "reset": None, "done": None, "srm_set": None, "refill": None}


def flip(h):
    """handle h -> 2^28 - 1 - h"""
    return (np.uint32(HANDLE_TOP) - np.ascontiguousarray(h, dtype=np.uint32)).astype(np.uint32)


def flip_script(script):
    """The script with every handle h replaced by 2^28 - 1 - h.  The positional state array becomes
    a sparse update (after a reset every state byte is 0, so only the nonzero ones are named) and
    the accept set keeps its form; run_step below applies it by handle."""
    out = []
    for step in script:
        op, a = step[0], list(step[1:])
        if op == "set_state":
            st = np.asarray(a[0], dtype=np.uint8)
            nz = np.nonzero(st)[0]
            out.append(("update_state", flip(nz), st[nz].copy()))
            continue
        if op == "nc_set":
            a[1] = flip(np.arange(len(a[0])) if a[1] is None else a[1])
        elif op == "nc_accept":
            a[0] = {HANDLE_TOP - int(h) for h in a[0]}
        elif HANDLE_ARG[op] is not None:
            a[HANDLE_ARG[op]] = flip(a[HANDLE_ARG[op]])
        out.append((op,) + tuple(a))
    return out


def run_step(step, model, ctx=None, use_filter=True):
    """srmap_cases.run_step; the accept set of a flipped mirror is applied by handle (the positional
    setter would take one byte per handle below 2^28)"""
    if step[0] == "nc_accept":
        model.nc.acc = set(step[1])
        if ctx:
            h = np.array(sorted(model.nc.map.values()), dtype=np.uint32)
            ctx.nc_update_accept(h, np.array([int(x) in model.nc.acc for x in h], dtype=np.uint8))
        return None, None
    return SM.run_step(step, model, ctx, use_filter)


def top_handle_tail(script):
    """Three steps after a flipped script that store handle 2^28 - 1 with both flags.  The scripts'
    generators count their handles from 3, 5 or 7, so the flip reaches 2^28 - 4 at most and the
    top handle is free: it enters up to three open searches next to the first one's target with a
    token (replied), is marked candidate there, and one more insertion per search rewrites the rows
    around it.  (One more bad handle than MAX_BAD: lists stay below 14 + 41 entries.)"""
    model = SM.Model()
    for step in script:
        run_step(step, model)
    slots = np.array([s for s, sl in enumerate(model.slots) if not sl.expired and sl.target != bytes(20)][:3],
                     dtype=np.uint32)
    m = slots.size
    assert m and HANDLE_TOP not in model.ids
    kid = np.frombuffer(model.slots[int(slots[0])].target, dtype=np.uint8).copy()
    kid[19] ^= 1
    assert bytes(kid) not in set(model.ids.values())
    others = [h for h in sorted(model.ids) if not model.state.get(h, 0)][:m]
    top = np.full(m, HANDLE_TOP, np.uint32)
    return [("insert", slots, RS.csr(np.ones(m, np.int64)), top, np.repeat(kid[None, :], m, axis=0), np.ones(m, np.uint8)),
            ("candidate", slots, top, np.ones(m, np.uint8)),
            ("insert", slots, RS.csr(np.ones(m, np.int64)), np.array(others, np.uint32),
             RS.as_ids(np.frombuffer(b"".join(model.ids[h] for h in others), dtype=np.uint8)), np.zeros(m, np.uint8))]


def handle_scripts():
    """(name, script): one insert script and one refill script of rsearch_cases and one offer script
    of srmap_cases, flipped, each followed by top_handle_tail"""
    out = []
    for name, script in (("insert103", RS.insert_script(*RS.INSERT_SHAPES[2])),
                         ("refill206", RS.refill_script(*RS.REFILL_SHAPES[5])),
                         ("shape404", SM.shape_script(*SM.SHAPES[3]))):
        f = flip_script(script)
        out.append((name, f + top_handle_tail(f)))
    return out
