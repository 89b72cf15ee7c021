"""The model and cases of Dht::trySearchInsert over the resident searches' ordered map (dhtgpu_srm_*,
opendht_amd/csrc/srmap.hip), shared by test_srmap_cpu.py and test_gpu_srmap.py.

The model composes what exists and restates nothing: it is rsearch_cases.Model (whose insert is the
oracle's Search::insertNode) plus the `done` set, the map -- the mapped slots in ascending order of
their targets -- and the walk of src/dht.cpp:118-150, which calls Model.insert one (slot, node) at a
time.  It also computes the filter of srmap.hip (the WALL predicate on the lists as they stand when
the offer begins), so that the number of filtered nodes can be compared, and can run the offer with
the filter or as the plain walk: test_srmap_cpu.py checks that the two agree on every case.

A case is a SCRIPT as in rsearch_cases: its steps plus ("srm_set", slots), ("done", slots, val) and
("offer", handles, ids).  Exact cases keep rsearch_cases' MAX_BAD discipline: at most MAX_BAD handles
are ever expired or candidates, so no list outgrows its row."""
import bisect
import copy

import numpy as np

import oracle as O
import rsearch_cases as RS

EUNSORTED = -5


def dist(a, b):
    return int.from_bytes(bytes(a), "big") ^ int.from_bytes(bytes(b), "big")


class Model(RS.Model):
    def __init__(self):
        super().__init__()
        self.done = set()
        self.order = None      # the map: slots in target order; None = no valid map

    def reset(self, nslots):
        super().reset(nslots)
        self.done, self.order = set(), None

    def open(self, slots, targets):
        super().open(slots, targets)
        self.done -= {int(s) for s in slots}
        self.order = None

    def srm_set(self, slots):
        """the map, or EUNSORTED (and no map) when two targets are equal"""
        slots = [int(s) for s in slots]
        self.order = None
        if len({self.slots[s].target for s in slots}) != len(slots):
            return EUNSORTED
        self.order = sorted(slots, key=lambda s: self.slots[s].target)
        return 0

    def set_done(self, slots, val):
        for s, v in zip(slots, np.broadcast_to(np.asarray(val), (len(slots),))):
            (self.done.add if v else self.done.discard)(int(s))

    def export(self):
        return (np.array(self.order, dtype=np.uint32),
                np.array([s in self.done for s in self.order], dtype=np.uint8))

    # ---- the filter of srmap.hip --------------------------------------------------------------
    def wall_cut(self, s, h, kid):
        """the cut of search s when it is a wall for node (h, kid), else None"""
        sl = self.slots[s]
        if sl.expired or s in self.done:
            return None
        bad = [self.is_bad(sl, j) for j in range(len(sl.row))]
        if len(bad) - sum(bad) < RS.SEARCH_NODES:
            return None
        if any(not b and self.state.get(x, 0) & 2 for b, x in zip(bad, sl.row)) or h in sl.row:
            return None
        good, cut = 0, len(bad)
        for j, b in enumerate(bad):
            good += not b
            if good > RS.SEARCH_NODES:
                cut = j
                break
        return cut if dist(kid, sl.target) > dist(self.ids[sl.row[cut - 1]], sl.target) else None

    def lower_bound(self, kid):
        return bisect.bisect_left([self.slots[s].target for s in self.order], bytes(kid))

    def filtered(self, h, kid):
        """[(slot, cut)] of the two walls when node (h, kid) is answered by the filter, else None"""
        c, cuts = self.lower_bound(kid), []
        for i in (c, c - 1):
            if 0 <= i < len(self.order):
                cut = self.wall_cut(self.order[i], h, kid)
                if cut is None:
                    return None
                cuts.append((self.order[i], cut))
        return cuts

    # ---- Dht::trySearchInsert -----------------------------------------------------------------
    def insert_one(self, s, h, kid):
        return bool(self.insert([s], [0, 1], [h], np.frombuffer(bytes(kid), np.uint8).reshape(1, 20))[0])

    def walk(self, h, kid, touched):
        """src/dht.cpp:118-150 for one node: (searches that took it, insertNode calls)"""
        c, cnt, hops = self.lower_bound(kid), 0, 0
        for rng in (range(c, len(self.order)), range(c - 1, -1, -1)):
            for i in rng:
                s = self.order[i]
                hops += 1
                if self.insert_one(s, h, kid):
                    cnt += 1
                    touched[s >> 5] |= np.uint32(1 << (s & 31))
                elif not self.slots[s].expired and s not in self.done:
                    break
        return cnt, hops

    def offer(self, handles, ids, use_filter=True):
        """(cnt, touched, stats) of one dhtgpu_srm_offer"""
        handles = [int(h) for h in handles]
        ids = RS.as_ids(ids)
        for h, k in zip(handles, ids):
            self.ids[h] = bytes(k)
        m = len(handles)
        cnt = np.zeros(m, np.uint32)
        touched = np.zeros((len(self.slots) + 31) // 32, np.uint32)
        stats = np.zeros(4, np.uint32)
        if not m:
            return cnt, touched, stats
        hazard = any(self.state.get(h, 0) & 3 == 2 for h in handles)
        skip = [None] * m
        if use_filter:
            stats[2] = hazard
            if not hazard:
                skip = [self.filtered(h, k) for h, k in zip(handles, ids)]
                for cuts in skip:
                    for s, cut in cuts or ():
                        sl = self.slots[s]
                        del sl.row[cut:], sl.flags[cut:]
        for j, (h, k) in enumerate(zip(handles, ids)):
            if skip[j] is None:
                cnt[j], hops = self.walk(h, k, touched)
                stats[1] += hops
        stats[0] = sum(x is not None for x in skip)
        stats[3] = any(sl.over for sl in self.slots)
        return cnt, touched, stats


def run_step(step, model, ctx=None, use_filter=True):
    op, a = step[0], step[1:]
    if op == "srm_set":
        want = model.srm_set(a[0])
        got = None
        if ctx:
            import opendht_amd
            try:
                ctx.srm_set(a[0])
                got = 0
            except opendht_amd.DhtGpuError as e:
                got = e.code
        return want, got
    if op == "done":
        model.set_done(a[0], a[1])
        if ctx:
            ctx.srm_set_done(a[0], a[1])
        return None, None
    if op == "offer":
        return model.offer(a[0], a[1], use_filter), (ctx.srm_offer(a[0], a[1]) if ctx else None)
    return RS.run_step(step, model, ctx)


# ---- building blocks --------------------------------------------------------------------------------
def near(target, rng, n, bits=24):
    """n distinct ids that differ from target in their last `bits` bits only"""
    out = np.repeat(np.asarray(target, np.uint8).reshape(1, 20), n, axis=0)
    low = rng.permutation(np.unique(rng.integers(1, 1 << bits, size=4 * n)))[:n]
    assert low.size == n
    for i, v in enumerate(low):
        out[i, 17:] ^= np.frombuffer(int(v).to_bytes(3, "big"), np.uint8)
    return out


def shape_script(seed, ns, m, shared_bits, with2=False):
    """ns mapped searches out of ns + 3 slots, a pool of 400 nodes (38 of them bad); most lists
    pre-filled (full of good nodes / partly / with bad nodes / empty), some searches expired, some
    done; an offer of m nodes -- pool nodes (listed handles among them), ids below and above every
    target, ids equal to a target, one handle twice -- then state changes (listed nodes expire or
    become removable and expired) and candidates, and the same offer again.  with2: one good node in
    eight is removable and not expired (state 2), the hazard of srmap.hip, in lists and offers alike."""
    rng = np.random.default_rng(seed)
    pool = 400
    ids = RS.clustered_ids(seed, pool, shared_bits)
    handles = (rng.permutation(pool) + 5).astype(np.uint32)
    st = np.zeros(pool, np.uint8)
    bad = rng.permutation(pool)[: RS.MAX_BAD - 8]
    st[bad] = 1
    st[bad[:3]] = 3
    if with2:
        st[(st == 0) & (rng.random(pool) < 0.125)] = 2
    state = np.zeros(int(handles.max()) + 40, np.uint8)
    state[handles] = st
    nslots = ns + 3
    slots = rng.permutation(nslots)[:ns].astype(np.uint32)
    targets = RS.clustered_ids(seed + 1, max(ns, 1), shared_bits)[:ns]
    if shared_bits and ns:
        targets[:, : shared_bits // 8] = ids[0, : shared_bits // 8]
    steps = [("reset", nslots), ("set_state", state)]
    if ns:
        steps.append(("open", slots, targets))
        pre = [rng.integers(0, pool, size=(0, 60, 9, 25)[int(s) % 4]) for s in slots]
        node = np.concatenate(pre).astype(np.int64)
        steps.append(("insert", slots, RS.csr([len(p) for p in pre]), handles[node], ids[node], None))
        ex = slots[rng.random(ns) < 0.15]
        if ex.size:
            steps.append(("expire", np.sort(ex)))
        dn = slots[rng.random(ns) < 0.15]
        if dn.size:
            steps.append(("done", dn, np.ones(dn.size, np.uint8)))
    steps.append(("srm_set", slots))
    node = rng.integers(0, pool, size=m)
    oh, oi = handles[node].copy(), ids[node].copy()
    xh = int(handles.max()) + 1          # handles of the constructed ids (state 0)
    special = [np.zeros(20, np.uint8), np.full(20, 255, np.uint8)] + [t for t in targets[:3]]
    for i, k in enumerate(special):
        if m > 2 * i + 1:
            oh[2 * i + 1], oi[2 * i + 1] = xh + i, k
    if m >= 12:
        oh[11], oi[11] = oh[2], oi[2]    # the same handle twice
    steps.append(("offer", oh, oi))
    if ns:
        upd = handles[bad[3:9]]
        steps.append(("update_state", upd, np.array([3, 3, 0, 0, 1, 3], np.uint8)))
        cand = handles[rng.permutation(pool)[:4]]
        cs, ch = np.repeat(slots, cand.size), np.tile(cand, ns)
        steps.append(("candidate", cs, ch, np.ones(cs.size, np.uint8)))
        steps.append(("offer", oh[::-1].copy(), oi[::-1].copy()))
    return steps


SHAPES = [   # (seed, mapped searches, nodes per offer, shared leading bits)
    (401, 0, 1, 0), (402, 0, 300, 0), (403, 1, 0, 0), (404, 1, 65, 64), (405, 2, 63, 128), (406, 63, 64, 0),
    (407, 64, 65, 64), (408, 65, 300, 128), (409, 257, 1, 0), (410, 257, 300, 64), (411, 65, 63, 0), (412, 2, 1, 128),
]


SHAPES2 = [(451, 2, 63, 0), (452, 65, 300, 64), (453, 257, 64, 0)]   # the same with state 2 drawn


def fresh_script():
    """65 searches with empty lists and 20 nodes, 7 of them expired: no list ever holds 14 good nodes,
    so every node enters every search and each walk crosses all 65 in both directions."""
    rng = np.random.default_rng(500)
    ids, targets = O.gen_ids(500, 20), O.gen_ids(501, 65)
    handles = (rng.permutation(20) + 3).astype(np.uint32)
    state = np.zeros(30, np.uint8)
    state[handles[:7]] = 1
    slots = rng.permutation(65).astype(np.uint32)
    return [("reset", 65), ("set_state", state), ("open", slots, targets), ("srm_set", slots), ("offer", handles, ids),
            ("offer", handles[::-1].copy(), ids[::-1].copy())]


def converged_script():
    """8 searches whose lists hold the 14 closest of a pool of 3000 ids; an offer of 300 pool nodes and
    60 new ones: the filter answers most of them."""
    rng = np.random.default_rng(510)
    pool = 3000
    ids, targets = O.gen_ids(510, pool + 60), O.gen_ids(511, 8)
    handles = (rng.permutation(pool + 60) + 1).astype(np.uint32)
    state = np.zeros(pool + 70, np.uint8)
    state[handles[rng.permutation(pool)[:30]]] = 1
    slots = np.arange(8, dtype=np.uint32)
    node = np.tile(np.arange(pool), 8)
    steps = [("reset", 8), ("set_state", state), ("open", slots, targets),
             ("insert", slots, RS.csr(np.full(8, pool)), handles[node], ids[node], None), ("srm_set", slots[::-1].copy())]
    pick = np.concatenate([rng.integers(0, pool, size=300), np.arange(pool, pool + 60)])
    pick = pick[rng.permutation(pick.size)]
    steps.append(("offer", handles[pick], ids[pick]))
    return steps


def ladder(n):
    """n targets in ascending order: byte 0 = 16 * (i + 1)"""
    t = O.gen_ids(520, n)
    t[:, 0] = [16 * (i + 1) for i in range(n)]
    return t


def skip_run_script():
    """12 searches in target order; searches 1..9 refuse every offered node and let the walk pass:
    4 and 7 are expired and list 14 expired nodes of their own, the others list 14 good nodes next to
    their targets and are done.  Searches 0, 10 and 11 are open.  A node whose id lies inside the run
    is refused by all nine and still enters searches 0, 10 and 11."""
    rng = np.random.default_rng(520)
    targets = ladder(12)
    slots = rng.permutation(12).astype(np.uint32)
    state = np.zeros(400, np.uint8)
    state[1:29] = 1
    steps = [("reset", 12), ("set_state", state), ("open", slots, targets), ("expire", np.sort(slots[[4, 7]]))]
    hs, ks, h0 = [], [], 40
    for i in range(1, 10):
        if i in (4, 7):   # 14 expired nodes: the search, expired before, stays expired
            hs.append(np.arange(1, 15, dtype=np.uint32) + (14 if i == 7 else 0))
        else:
            hs.append(np.arange(h0, h0 + 14, dtype=np.uint32))
            h0 += 14
        ks.append(near(targets[i], rng, 14))
    steps.append(("insert", slots[1:10], RS.csr(np.full(9, 14)), np.concatenate(hs), np.concatenate(ks), None))
    steps.append(("done", slots[[1, 2, 3, 5, 6, 8, 9]], np.ones(7, np.uint8)))
    steps.append(("srm_set", slots))
    xi = O.gen_ids(521, 6)
    xi[:, 0] = [16 * 6 - 1, 16 * 6 + 1, 16 * 5 + 3, 16 * 7 + 2, 16 * 3 + 1, 16 * 9 + 9]
    steps.append(("offer", np.arange(300, 306, dtype=np.uint32), xi))
    steps.append(("done", slots[[1, 3]], np.zeros(2, np.uint8)))
    steps.append(("offer", np.arange(306, 312, dtype=np.uint32), O.gen_ids(522, 6)))
    return steps


def trim_only_script():
    """Rows longer than their cut: 4 searches listing 14 good nodes and 10 expired ones among and
    behind them; the expired handles become good again (update_state), so each row holds 24 good
    entries; far nodes are then offered, and the filter's cut is the only change."""
    rng = np.random.default_rng(530)
    targets = ladder(4)
    slots = np.arange(4, dtype=np.uint32)
    state = np.zeros(200, np.uint8)
    bad_h = np.arange(100, 110, dtype=np.uint32)
    state[bad_h] = 1
    bad_ids = near(targets[1], rng, 10, bits=23)
    hs, ks = [], []
    for i in range(4):
        hs += [bad_h, np.arange(14, dtype=np.uint32) + 1000 * (i + 1)]   # (a full list would refuse the far bad nodes)
        ks += [bad_ids, near(targets[i], rng, 14)]
    steps = [("reset", 4), ("set_state", state), ("open", slots, targets),
             ("insert", slots, RS.csr(np.full(4, 24)), np.concatenate(hs), np.concatenate(ks), None),
             ("update_state", bad_h, np.zeros(10, np.uint8)), ("srm_set", slots)]
    far = O.gen_ids(531, 5)
    far[:, 0] = [200, 16 * 2 + 8, 3, 16 * 3 + 9, 250]
    steps.append(("offer", np.arange(50, 55, dtype=np.uint32), far))
    return steps


def hazard_scripts():
    """(listed, batch): a listed good node becomes removable-not-expired (state 2) -- its search is no
    wall: the far node offered next is walked, and a close node then removes it; and a state-2 node in
    the batch -- the whole batch is walked and the hazard flag is set."""
    out = []
    for kind in ("listed", "batch"):
        rng = np.random.default_rng(540)
        targets = ladder(3)
        slots = np.arange(3, dtype=np.uint32)
        hs = np.arange(1, 43, dtype=np.uint32)
        ks = np.concatenate([near(targets[i], rng, 14) for i in range(3)])
        steps = [("reset", 3), ("set_state", np.zeros(100, np.uint8)), ("open", slots, targets),
                 ("insert", slots, RS.csr(np.full(3, 14)), hs, ks, None), ("srm_set", slots)]
        far = O.gen_ids(541, 4)
        far[:, 0] = [16 * 2 + 7, 16 + 9, 200, 2]
        close = near(targets[1], rng, 2, bits=8)
        if kind == "listed":
            steps.append(("update_state", hs[[3, 20, 30]], np.full(3, 2, np.uint8)))
            steps.append(("offer", np.arange(50, 54, dtype=np.uint32), far))
            steps.append(("offer", np.array([60, 61, 52, 50], np.uint32), np.concatenate([close, far[[2, 0]]])))
        else:
            steps.append(("update_state", np.array([61], np.uint32), np.full(1, 2, np.uint8)))
            steps.append(("offer", np.array([50, 60, 61, 51, 52], np.uint32), np.concatenate([far[:1], close, far[1:3]])))
            steps.append(("offer", np.array([53, 50], np.uint32), far[[3, 0]]))
        out.append((f"hazard_{kind}", steps))
    return out


def all_scripts():
    out = [(f"shape{c[0]}", shape_script(*c)) for c in SHAPES]
    out += [(f"shape{c[0]}", shape_script(*c, with2=True)) for c in SHAPES2]
    out += [("fresh", fresh_script()), ("converged", converged_script()), ("skip_run", skip_run_script()),
            ("trim_only", trim_only_script())] + hazard_scripts()
    return out


def clone(model):
    return copy.deepcopy(model)
