"""The resident searches' model and cases (dhtgpu_sr_*, opendht_amd/csrc/rsearch.hip), shared by
test_rsearch_cpu.py and test_gpu_rsearch.py.

The model keeps per slot the target, the handle row, its flags and `expired`, plus handle -> id and
the state byte by handle.  insert renumbers the handles in play to dense indices, calls the
project's own oracle O.search_insert (Search::insertNode restated, built by build()) at cap 64 and
maps the rows back; refill is ncache_cases.Model.expected (the oracle's getCachedNodes walk) followed
by insert; status is computed here.

A case is a SCRIPT: a list of steps (op, args...) that run() applies to a model and, when given, to a
context, so that the CPU test can run every GPU case on the model alone.  Exact cases never
overflow: a script's `bad` handles -- the only ones that are ever expired or marked candidate --
number at most MAX_BAD = 40, which bounds every list at SEARCH_NODES + MAX_BAD = 54 <= 64 (an
insertion first cuts a full list to 14 non-bad entries)."""
import numpy as np

import ncache_cases as NC
import oracle as O

NONE = 0xFFFFFFFF
CAP = 64             # DHTGPU_SR_CAP
SEARCH_NODES = 14
MAX_BAD = 40
LIST_BOUND = SEARCH_NODES + MAX_BAD


def as_ids(rows):
    return np.ascontiguousarray(rows, dtype=np.uint8).reshape(-1, 20)


class Slot:
    def __init__(self, target):
        self.target = bytes(target)
        self.row, self.flags = [], []
        self.expired = False
        self.over = False


class Model:
    def __init__(self):
        self.nc = NC.Model()
        self.have_nc = False
        self.ids = {}      # handle -> id bytes (what the device keeps as the entry's distance)
        self.state = {}    # handle -> state byte; absent = 0
        self.slots = []

    # ---- the search set -------------------------------------------------------------------------
    def reset(self, nslots):
        self.slots = [Slot(bytes(20)) for _ in range(nslots)]
        self.state = {}

    def open(self, slots, targets):
        for s, t in zip(slots, as_ids(targets)):
            self.slots[int(s)] = Slot(t)

    def expire(self, slots):
        for s in slots:
            sl = self.slots[int(s)]
            sl.expired, sl.row, sl.flags = True, [], []

    def set_state(self, by_handle):
        self.state = {h: int(v) for h, v in enumerate(by_handle)}

    def update_state(self, handles, val):
        for h, v in zip(handles, np.broadcast_to(np.asarray(val), (len(handles),))):
            self.state[int(h)] = int(v)

    def set_candidate(self, slots, handles, val):
        for s, h, v in zip(slots, handles, np.broadcast_to(np.asarray(val), (len(handles),))):
            sl = self.slots[int(s)]
            if int(h) in sl.row:
                j = sl.row.index(int(h))
                sl.flags[j] = (sl.flags[j] & ~1) | (1 if v else 0)

    def insert(self, slots, ins_off, ins_handle, ins_ids, ins_token=None):
        """Search::insertNode through the oracle; returns the (total,) added bytes"""
        slots = [int(s) for s in slots]
        off = np.asarray(ins_off, dtype=np.uint64)
        tot = int(off[-1])
        handle = [int(h) for h in np.asarray(ins_handle).reshape(-1)[:tot]]
        for h, k in zip(handle, as_ids(ins_ids)[:tot]):
            self.ids[h] = bytes(k)
        tok = np.zeros(tot, np.uint8) if ins_token is None else np.asarray(ins_token, dtype=np.uint8)[:tot]
        play = sorted(set(handle).union(*[self.slots[s].row for s in slots]))
        dense = {h: i for i, h in enumerate(play)}
        node_ids = as_ids(np.frombuffer(b"".join(self.ids[h] for h in play), dtype=np.uint8)) if play \
            else np.zeros((1, 20), np.uint8)
        node_state = np.array([self.state.get(h, 0) for h in play] or [0], dtype=np.uint8)
        m = len(slots)
        lists = np.full((m, CAP), NONE, np.uint32)
        flags = np.zeros((m, CAP), np.uint8)
        lens = np.zeros(m, np.uint32)
        expired = np.zeros(m, np.uint8)
        targets = np.zeros((m, 20), np.uint8)
        for j, s in enumerate(slots):
            sl = self.slots[s]
            lens[j] = len(sl.row)
            lists[j, : lens[j]] = [dense[h] for h in sl.row]
            flags[j, : lens[j]] = sl.flags
            expired[j] = sl.expired
            targets[j] = np.frombuffer(sl.target, dtype=np.uint8)
        node = np.array([dense[h] for h in handle], dtype=np.uint32)
        lists, flags, lens, expired, added = O.search_insert(node_ids, node_state, targets, lists, flags, lens, expired,
                                                             off, node, tok)
        for j, s in enumerate(slots):
            sl = self.slots[s]
            if lens[j] > CAP:       # the oracle's list outgrew the row: not an exact case from here on
                sl.over = True
                lens[j] = CAP
            sl.row = [play[i] for i in lists[j, : lens[j]]]
            sl.flags = [int(f) for f in flags[j, : lens[j]]]
            sl.expired = bool(expired[j])
        return added

    def refill(self, slots, count):
        """Dht::refill: the cache's walk, then insertNode for each result in walk order"""
        slots = [int(s) for s in slots]
        targets = as_ids(np.frombuffer(b"".join(self.slots[s].target for s in slots), dtype=np.uint8))
        rows, cnt = self.nc.expected(targets, count)
        key_of = {h: k for k, h in self.nc.map.items()}
        off = np.concatenate([[0], np.cumsum(cnt)]).astype(np.uint64)
        handle = [int(h) for j in range(len(slots)) for h in rows[j, : cnt[j]]]
        ids = as_ids(np.frombuffer(b"".join(key_of[h] for h in handle), dtype=np.uint8)) if handle \
            else np.zeros((0, 20), np.uint8)
        added = self.insert(slots, off, handle, ids)
        return np.array([int(added[int(off[j]):int(off[j + 1])].sum()) for j in range(len(slots))], dtype=np.uint32)

    def is_bad(self, sl, j):
        return bool(self.state.get(sl.row[j], 0) & 1) or bool(sl.flags[j] & 1)

    def status(self, slots):
        out = np.zeros((len(slots), 4), np.uint32)
        for i, s in enumerate(slots):
            sl = self.slots[int(s)]
            bad = [self.is_bad(sl, j) for j in range(len(sl.row))]
            lead = next((j for j, b in enumerate(bad) if not b), len(bad))
            out[i] = [len(sl.row), sum(bad), lead, (1 if sl.expired else 0) | (2 if sl.over else 0)]
        return out

    def lists(self, slots):
        m = len(slots)
        h = np.full((m, CAP), NONE, np.uint32)
        fl = np.zeros((m, CAP), np.uint8)
        ln = np.zeros(m, np.uint32)
        for i, s in enumerate(slots):
            sl = self.slots[int(s)]
            ln[i] = len(sl.row)
            h[i, : ln[i]] = sl.row
            fl[i, : ln[i]] = sl.flags
        return h, fl, ln


# ---- running a script -------------------------------------------------------------------------------
def run_step(step, model, ctx=None):
    """One step on the model and (when given) the context: (the model's result, the context's), None
    for steps without one."""
    op, a = step[0], step[1:]
    want = got = None
    if op == "reset":
        model.reset(a[0])
        if ctx:
            ctx.sr_reset(a[0])
    elif op == "nc_set":
        model.nc.set(a[0], a[1])
        model.have_nc = True
        if ctx:
            ctx.nc_set(a[0], a[1])
    elif op == "nc_accept":     # the accepted handles as a set
        model.nc.acc = set(a[0])
        if ctx:
            nh = max([h for h in model.nc.map.values()] + [0]) + 1
            ctx.nc_set_accept(np.array([h in model.nc.acc for h in range(nh)], dtype=np.uint8))
    elif op == "nc_insert":
        want = model.nc.insert(a[0], a[1], a[2])
        got = ctx.nc_insert(a[0], a[1], a[2]) if ctx else None
    elif op == "nc_erase":
        want = model.nc.erase(a[0])
        got = ctx.nc_erase(a[0]) if ctx else None
    elif op == "open":
        model.open(a[0], a[1])
        if ctx:
            ctx.sr_open(a[0], a[1])
    elif op == "expire":
        model.expire(a[0])
        if ctx:
            ctx.sr_expire(a[0])
    elif op == "set_state":
        model.set_state(a[0])
        if ctx:
            ctx.sr_set_state(a[0])
    elif op == "update_state":
        model.update_state(a[0], a[1])
        if ctx:
            ctx.sr_update_state(a[0], a[1])
    elif op == "candidate":
        model.set_candidate(a[0], a[1], a[2])
        if ctx:
            ctx.sr_set_candidate(a[0], a[1], a[2])
    elif op == "insert":
        want = model.insert(*a)
        got = ctx.sr_insert(*a) if ctx else None
    elif op == "refill":
        want = model.refill(a[0], a[1])
        got = ctx.sr_refill(a[0], a[1]) if ctx else None
    else:
        raise ValueError(op)
    return want, got


def max_len(model):
    return max([len(sl.row) for sl in model.slots] or [0])


# ---- building blocks ----------------------------------------------------------------------------------
def clustered_ids(seed, n, shared_bits):
    """n distinct ids (and their targets drawn the same way) that share their first shared_bits bits"""
    ids = O.gen_ids(seed, n)
    nb = shared_bits // 8
    if nb:
        ids[:, :nb] = ids[0, :nb]
    assert len({bytes(k) for k in ids}) == n
    return ids


def pool_states(rng, pool, nbad_state):
    """state bytes of a pool: the values test_gpu_parity._search_case draws (0, 1, 2, 3) with exactly
    nbad_state nodes expired (bit0) -- all but two of them state 1, so that a long list of bad nodes
    can stand: a removable node leaves with the next insertion -- and of the others one in five
    removable only (2)"""
    st = rng.choice([0, 0, 0, 0, 2], size=pool).astype(np.uint8)
    bad = rng.permutation(pool)[:nbad_state]
    st[bad] = 1
    st[bad[:2]] = 3
    return st


def csr(counts):
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)


def insert_script(seed, nslots, per_slot, pool, shared_bits=0):
    """The insert shapes: nslots searches (every slot of the set, in a shuffled order), per_slot
    insertions each out of `pool` nodes (handles are a permutation of an offset range), ids and
    targets sharing their first shared_bits bits, 20 % of the searches expired before the pre-fill,
    a pre-fill that leaves lists of 13, 14, 15 and >= 50 entries (the slot's index mod 5 picks: good
    nodes only, 13 / 14 of them; 14 good and one bad; 14 good and the 36 state-1 nodes; anything), then the
    main batch with tokens at 30 %.  At most MAX_BAD handles are ever bad."""
    rng = np.random.default_rng(seed)
    ids = clustered_ids(seed, pool, shared_bits)
    handles = (rng.permutation(pool) + 7).astype(np.uint32)
    st_pool = pool_states(rng, pool, MAX_BAD - 2)   # + the two candidates below
    state = np.zeros(int(handles.max()) + 1, np.uint8)
    state[handles] = st_pool
    good = np.nonzero(st_pool == 0)[0]
    bad = np.nonzero(st_pool == 1)[0]
    assert good.size >= 16 and bad.size == MAX_BAD - 4
    targets = clustered_ids(seed + 1, nslots, shared_bits)
    if shared_bits:
        targets[:, : shared_bits // 8] = ids[0, : shared_bits // 8]
    slots = rng.permutation(nslots).astype(np.uint32)
    steps = [("reset", nslots), ("set_state", state), ("open", slots, targets)]
    expired = slots[rng.random(nslots) < 0.2]
    if expired.size:
        steps.append(("expire", np.sort(expired)))
    pre = []
    for j, s in enumerate(slots):
        kind = int(s) % 5
        g = rng.permutation(good)
        b = rng.permutation(bad)
        if kind == 0:
            pick = g[:13]
        elif kind == 1:
            pick = g[:14]
        elif kind == 2:
            pick = np.concatenate([g[:14], b[:1]])
        elif kind == 3:
            pick = np.concatenate([g[:14], b])
        else:
            pick = rng.integers(0, pool, size=int(rng.integers(0, 20)))
        pre.append(pick.astype(np.int64))
    node = np.concatenate(pre) if pre else np.zeros(0, np.int64)
    steps.append(("insert", slots, csr([len(p) for p in pre]), handles[node], ids[node],
                  (rng.random(node.size) < 0.5).astype(np.uint8)))
    counts = np.full(nslots, per_slot)
    node = rng.integers(0, pool, size=int(counts.sum()))
    node[::7] = node[::7] % min(pool, 64)      # repeats of the same nodes
    order = rng.permutation(nslots)            # the main batch names the slots in another order
    steps.append(("insert", slots[order], csr(counts[order]), handles[node], ids[node],
                  (rng.random(node.size) < 0.3).astype(np.uint8)))
    # candidates: two more bad handles, set on whatever lists hold them, then one more batch
    cand = handles[good[:2]] if good.size >= 2 else handles[:0]
    if cand.size:
        cs = np.repeat(slots, cand.size)
        ch = np.tile(cand, nslots)
        steps.append(("candidate", cs, ch, np.ones(cs.size, np.uint8)))
        node = rng.integers(0, pool, size=nslots * 3)
        steps.append(("insert", slots, csr(np.full(nslots, 3)), handles[node], ids[node],
                      (rng.random(node.size) < 0.3).astype(np.uint8)))
    return steps


INSERT_SHAPES = [   # (seed, slots per call, insertions per slot, node pool, shared leading bits)
    (101, 1, 0, 64, 0), (102, 1, 1, 500, 32), (103, 4, 64, 64, 64), (104, 5, 65, 500, 128), (105, 700, 1, 20000, 0),
    (106, 4, 200, 500, 64), (107, 5, 0, 20000, 32), (108, 700, 64, 64, 128), (109, 1, 200, 20000, 128),
    (110, 700, 65, 500, 0), (111, 5, 200, 64, 32), (112, 4, 1, 20000, 64),
]


def refill_script(seed, nkeys, count, accept, fill, keys=None, targets=None, nslots=9):
    """The refill shapes: an nc mirror of nkeys keys (handles a permutation of an offset range) under
    one accept kind, nslots searches whose lists are empty / partly filled / full before the refill
    (`fill`), a refill, and the same refill again (nothing left to insert that was not refused)."""
    rng = np.random.default_rng(seed)
    if keys is None:
        keys = O.gen_ids(seed, nkeys) if nkeys else np.zeros((0, 20), np.uint8)
    nkeys = keys.shape[0]
    handles = (rng.permutation(nkeys) + 3).astype(np.uint32)
    if targets is None:
        targets = NC.targets_for(keys, seed, nrand=4)
    nslots = targets.shape[0]
    slots = np.arange(nslots, dtype=np.uint32)
    model = NC.Model()
    model.set(keys, handles)
    acc = NC.accept_handles(accept, model.sorted()[1])
    # bad handles: expired nodes the cache still offers when its accept bit says so
    state = np.zeros(int(handles.max()) + 1 if nkeys else 1, np.uint8)
    if nkeys:
        pick = rng.permutation(nkeys)[: min(MAX_BAD, nkeys // 3)]
        state[handles[pick]] = 1    # (no removable node here: one would be inserted again by the second refill)
    steps = [("reset", nslots), ("nc_set", keys, handles), ("nc_accept", acc), ("set_state", state),
             ("open", slots, targets)]
    if fill != "empty" and nkeys:
        per = 6 if fill == "part" else 30
        node = rng.integers(0, nkeys, size=nslots * per)
        ok = (state[handles[node]] & 1) == 0     # good nodes only: a full list holds 14 of them
        cnt = [int(ok[j * per:(j + 1) * per].sum()) for j in range(nslots)]
        steps.append(("insert", slots, csr(cnt), handles[node[ok]], keys[node[ok]], None))
    steps.append(("refill", slots, count))
    steps.append(("refill", slots, count))
    return steps


REFILL_SHAPES = [   # (seed, keys, count, accept kind, lists before)
    (201, 0, 14, "all", "empty"), (202, 1, 14, "all", "empty"), (203, 13, 14, "all", "part"), (204, 14, 14, "all", "full"),
    (205, 15, 1, "reject30", "empty"), (206, 300, 14, "reject30", "part"), (207, 300, 32, "all", "full"),
    (208, 300, 14, "ends", "empty"), (209, 300, 1, "none", "part"), (210, 20000, 14, "all", "empty"),
    (211, 20000, 32, "reject30", "full"), (212, 20000, 14, "ends", "part"), (213, 15, 32, "all", "part"),
    (214, 14, 1, "none", "empty"), (215, 13, 32, "ends", "full"),
]


def non_monotone_script(count=8):
    keys, target = NC.non_monotone()
    return refill_script(31, keys.shape[0], count, "all", "empty", keys=keys, targets=target)


def clustered_script(count=14):
    keys, targets = NC.clustered()
    return refill_script(32, keys.shape[0], count, "reject30", "part", keys=keys, targets=targets)


def lifecycle_script(seed=300, nslots=40, nkeys=600):
    """One context's life: reset, open, refill, insert with tokens, update_state (some listed nodes
    expire, some become removable), insert, set_candidate on and off (a handle that is in no list
    included), nc_erase / nc_insert, refill, sr_expire, refill (insertNode's expired branch), a slot
    opened again, refill."""
    rng = np.random.default_rng(seed)
    keys = O.gen_ids(seed, nkeys)
    handles = (rng.permutation(nkeys) + 11).astype(np.uint32)
    extra = O.gen_ids(seed + 1, 200)                    # nodes that only replies bring
    xh = np.arange(2000, 2200, dtype=np.uint32)
    targets = O.gen_ids(seed + 2, nslots)
    targets[: nslots // 4] = keys[: nslots // 4]        # searches for a cached key
    slots = np.arange(nslots, dtype=np.uint32)
    steps = [("reset", nslots), ("nc_set", keys, handles), ("open", slots, targets), ("refill", slots, 14)]
    node = rng.integers(0, 200, size=nslots * 9)
    steps.append(("insert", slots, csr(np.full(nslots, 9)), xh[node], extra[node], (rng.random(node.size) < 0.6).astype(np.uint8)))
    # nodes that expire / become removable: 22 cache handles and 10 reply handles (+ 3 candidates and 3
    # more expired below: 38 bad handles)
    bad = np.concatenate([handles[rng.permutation(nkeys)[:22]], xh[rng.permutation(200)[:10]]])
    steps.append(("update_state", bad, rng.choice([1, 2, 3], size=bad.size).astype(np.uint8)))
    node = rng.integers(0, 200, size=nslots * 5)
    steps.append(("insert", slots, csr(np.full(nslots, 5)), xh[node], extra[node], (rng.random(node.size) < 0.3).astype(np.uint8)))
    cand = np.array([xh[0], xh[1], handles[0], 123456], dtype=np.uint32)    # 123456: in no list
    cs, ch = np.repeat(slots, cand.size), np.tile(cand, nslots)
    steps.append(("candidate", cs, ch, np.ones(cs.size, np.uint8)))
    steps.append(("refill", slots[::2], 14))
    steps.append(("candidate", cs[::2], ch[::2], np.zeros(cs[::2].size, np.uint8)))
    steps.append(("nc_erase", keys[:150]))
    fresh = O.gen_ids(seed + 3, 100)
    steps.append(("nc_insert", fresh, np.arange(3000, 3100, dtype=np.uint32), (rng.random(100) < 0.8).astype(np.uint8)))
    steps.append(("refill", slots, 14))
    steps.append(("expire", slots[1::3]))
    steps.append(("update_state", handles[rng.permutation(nkeys)[:3]], np.ones(3, np.uint8)))
    steps.append(("refill", slots, 14))
    steps.append(("open", slots[:5], O.gen_ids(seed + 4, 5)))
    steps.append(("refill", slots[::-1].copy(), 32))
    return steps


def all_exact_scripts():
    """(name, script) of every exact case the GPU test runs"""
    out = [(f"insert{c[0]}", insert_script(*c)) for c in INSERT_SHAPES]
    out += [(f"refill{c[0]}", refill_script(*c)) for c in REFILL_SHAPES]
    out += [("non_monotone", non_monotone_script()), ("clustered", clustered_script()), ("lifecycle", lifecycle_script())]
    return out
