"""The model and the cases of the growing resident routing table (dhtgpu_rtg_*,
opendht_amd/csrc/rtgrow.hip).  Model restates RoutingTable::onNewNode / split
(src/routing_table.cpp:204-262, :87-107, :176-202) and Dht::expireBuckets (src/dht.cpp:179-192) with
node states, on plain Python lists: it knows nothing of the library.  tests/test_rtgrow_cpu.py pins
it to the oracle's table in the all-good regime; tests/test_gpu_rtgrow.py compares the device with
it.  Test infrastructure only."""
import numpy as np

import oracle as O

NONE = 0xFFFFFFFF
RTG_NONE, RTG_KNOWN, RTG_PLACED, RTG_REPLACED, RTG_FULL, RTG_UNAPPLIED = range(6)
GOOD, EXPIRED, PENDING = 1, 2, 4
TARGET_NODES = 8
MAX_BUCKETS = 256
MAX_ROUNDS = 161

SIZES = (8, 9, 17, 64, 300, 2000)
SEEDS = (1, 2)
# (client, N) -> ((nb seed 1, nb seed 2), (nn seed 1, nn seed 2)): what the oracle grows from
# uniform() around MYID (checked on the CPU).  The client runs cross one 64-bucket round of findBucket.
SHAPES = {(0, 8): ((1, 1), (8, 8)), (0, 9): ((2, 2), (9, 9)), (0, 17): ((2, 2), (15, 16)), (0, 64): ((4, 5), (31, 32)),
          (0, 300): ((6, 7), (45, 50)), (0, 2000): ((10, 9), (73, 70)),
          (1, 8): ((1, 1), (8, 8)), (1, 9): ((2, 2), (9, 9)), (1, 17): ((3, 3), (17, 17)), (1, 64): ((10, 11), (64, 64)),
          (1, 300): ((47, 54), (293, 295)), (1, 2000): ((67, 66), (529, 526))}


def lowbit(b):
    """InfoHash::lowbit: the position of the last set bit, bit 0 the id's highest; -1 for the zero id"""
    x = int.from_bytes(b, "big")
    return -1 if not x else 159 - ((x & -x).bit_length() - 1)


class Model:
    """One routing table: firsts[b] (bytes), buckets[b] = handles in list order (front first)."""

    def __init__(self, myid, client=False):
        self.myid = bytes(bytearray(myid))
        self.client = bool(client)
        self.firsts = [bytes(20)]        # the Dht constructor's one bucket
        self.buckets = [[]]
        self.ids, self.state, self.tail = {}, {}, {}
        self.splits = 0

    @classmethod
    def from_table(cls, myid, firsts, off, ids, client=False, tails=None):
        """an uploaded table: node i has handle i and is good"""
        m = cls(myid, client)
        m.firsts = [bytes(bytearray(f)) for f in firsts]
        m.buckets = [list(range(int(off[b]), int(off[b + 1]))) for b in range(len(m.firsts))]
        for i, x in enumerate(ids):
            m.ids[i], m.state[i] = bytes(bytearray(x)), GOOD
            m.tail[i] = None if tails is None else bytes(bytearray(tails[i]))
        return m

    # ---- the reference's helpers
    def find_bucket(self, x):
        if not self.firsts:
            return None
        b = 0
        while b + 1 < len(self.firsts) and not x < self.firsts[b + 1]:
            b += 1
        return b

    def contains(self, b, x):
        return self.firsts[b] <= x and (b + 1 == len(self.firsts) or x < self.firsts[b + 1])

    def depth(self, b):
        return max(lowbit(self.firsts[b]), lowbit(self.firsts[b + 1]) if b + 1 < len(self.firsts) else -1) + 1

    def split(self, b):
        bit = self.depth(b)
        first = bytearray(self.firsts[b])
        first[bit // 8] |= 0x80 >> (bit % 8)
        self.firsts.insert(b + 1, bytes(first))
        self.buckets.insert(b + 1, [])
        old, self.buckets[b] = self.buckets[b], []
        for h in old:                                    # taken from the front, pushed to a front
            self.buckets[self.find_bucket(self.ids[h])].insert(0, h)
        self.splits += 1

    # ---- onNewNode
    def on_new_node(self, x, h, st=GOOD, tail=None):
        """(result, aux); UNAPPLIED when a split would need a 257th bucket (nothing done)"""
        x = bytes(bytearray(x))
        for _ in range(MAX_ROUNDS):
            b = self.find_bucket(x)
            if b is None:
                return RTG_NONE, NONE
            row = self.buckets[b]
            if h in row:
                return RTG_KNOWN, NONE
            mybucket = self.contains(b, self.myid)
            if len(row) < TARGET_NODES:
                row.insert(0, h)
                self._put(h, x, st, tail)
                return RTG_PLACED, NONE
            for i, o in enumerate(row):
                if self.state[o] & EXPIRED:
                    self._drop(o)
                    row[i] = h
                    self._put(h, x, st, tail)
                    return RTG_REPLACED, o
            dubious = any(not self.state[o] & GOOD for o in row)
            pick = next((o for o in row if not self.state[o] & GOOD and not self.state[o] & PENDING), NONE)
            d = self.depth(b)
            if not ((mybucket or (self.client and d < 6)) and (not dubious or len(self.firsts) == 1)) or d >= 160:
                return RTG_FULL, pick
            if len(self.firsts) == MAX_BUCKETS:
                return RTG_UNAPPLIED, NONE
            self.split(b)
        return RTG_FULL, NONE

    def batch(self, ids, handles, state=None, tails=None):
        """the batch in order: (results, aux), everything from the first UNAPPLIED on unapplied"""
        res, aux, stopped = [], [], False
        for j, (x, h) in enumerate(zip(ids, handles)):
            r, a = (RTG_UNAPPLIED, NONE) if stopped else self.on_new_node(
                x, int(h), GOOD if state is None else int(state[j]), None if tails is None else bytes(bytearray(tails[j])))
            stopped = stopped or r == RTG_UNAPPLIED
            res.append(r)
            aux.append(a)
        return np.array(res, np.uint8), np.array(aux, np.uint32)

    def _put(self, h, x, st, tail):
        self.ids[h], self.state[h], self.tail[h] = x, st & 7, tail

    def _drop(self, h):
        del self.ids[h], self.state[h], self.tail[h]

    # ---- expireBuckets and the setters
    def expire(self):
        gone = [h for row in self.buckets for h in row if self.state[h] & EXPIRED]
        self.buckets = [[h for h in row if not self.state[h] & EXPIRED] for row in self.buckets]
        for h in gone:
            self._drop(h)
        return gone

    def set_state(self, by_handle):
        for h in self.state:
            if h < len(by_handle):
                self.state[h] = int(by_handle[h]) & 7

    def update_state(self, handles, vals):
        for h, v in zip(handles, vals):
            if int(h) in self.state:
                self.state[int(h)] = int(v) & 7

    def update_good(self, handles, vals):
        for h, v in zip(handles, vals):
            if int(h) in self.state:
                self.state[int(h)] = (self.state[int(h)] & ~GOOD) | (GOOD if v else 0)

    # ---- what the device must hold
    def stat(self):
        return len(self.firsts), sum(len(r) for r in self.buckets), self.splits

    def export(self):
        """firsts (nb, 20), off (nb + 1,), ids (nn, 20), handles (nn,), state (nn,)"""
        order = [h for row in self.buckets for h in row]
        firsts = np.frombuffer(b"".join(self.firsts), np.uint8).reshape(-1, 20).copy()
        off = np.concatenate([[0], np.cumsum([len(r) for r in self.buckets])]).astype(np.uint32)
        ids = np.frombuffer(b"".join(self.ids[h] for h in order), np.uint8).reshape(-1, 20).copy()
        return firsts, off, ids, np.array(order, np.uint32), np.array([self.state[h] for h in order], np.uint8)

    def tails(self, alen):
        order = [h for row in self.buckets for h in row]
        return np.frombuffer(b"".join(self.tail[h] for h in order), np.uint8).reshape(-1, alen + 2).copy()


# ---- cases
MYID = O.gen_ids(99, 1)[0]


def uniform(seed, n):
    """(myid, n splitmix ids)"""
    return MYID, O.gen_ids(seed, n)


def deep_chain(seed=5, depths=151, per=9, shuffle=False):
    """For each d < depths, `per` ids equal to myid in their first d bits and different at bit d,
    the rest random: grown shallow to deep (or shuffled) they split my bucket depths times."""
    rng = np.random.default_rng(seed)
    myid = rng.integers(0, 256, 20, dtype=np.uint8)
    my = int.from_bytes(bytes(myid), "big")
    out = []
    for d in range(depths):
        for _ in range(per):
            r = int.from_bytes(bytes(rng.integers(0, 256, 20, dtype=np.uint8)), "big")
            keep = ((1 << 160) - 1) ^ ((1 << (160 - d)) - 1)          # the first d bits
            x = (my & keep) | ((~my) & (1 << (159 - d))) | (r & ((1 << (159 - d)) - 1))
            out.append(np.frombuffer(x.to_bytes(20, "big"), np.uint8))
    ids = np.array(out)
    assert len({bytes(x) for x in ids}) == ids.shape[0]
    if shuffle:
        ids = ids[rng.permutation(ids.shape[0])]
    return myid, np.ascontiguousarray(ids)


def oracle_run(myid, ids, client):
    """the oracle's table grown with ids: (results 0 / 1, (firsts, off, ids))"""
    t = O.Table(myid, client)
    res = np.array([t.insert(x) for x in ids], np.uint8)
    return res, t.export()


def random_walk(seed, steps=30, alen=0):
    """A seeded list of mixed operations over a small id space with colliding prefixes:
    ("new", ids, handles, state, tails) / ("expire",) / ("update", handles, vals) / ("set", bytes) /
    ("good", handles, vals).  Handles are fresh per new node but for a few deliberate repeats;
    expired nodes are never good."""
    rng = np.random.default_rng(1000 + seed)
    myid = rng.integers(0, 256, 20, dtype=np.uint8)
    ops, nxt = [], 0
    states = (GOOD, GOOD, GOOD, 0, PENDING, EXPIRED, EXPIRED | PENDING, GOOD | PENDING)
    for _ in range(steps):
        k = rng.integers(0, 10)
        if k < 6:
            m = int(rng.choice([1, 3, 9, 20]))
            ids = rng.integers(0, 256, (m, 20), dtype=np.uint8)
            near = rng.random(m) < 0.6                        # most share a prefix with myid
            for j in np.flatnonzero(near):
                nbits = int(rng.integers(0, 12))
                x = int.from_bytes(bytes(ids[j]), "big")
                my = int.from_bytes(bytes(myid), "big")
                keep = ((1 << 160) - 1) ^ ((1 << (160 - nbits)) - 1)
                ids[j] = np.frombuffer(((my & keep) | (x & ~keep & ((1 << 160) - 1))).to_bytes(20, "big"), np.uint8)
            handles = np.arange(nxt, nxt + m, dtype=np.uint32)
            nxt += m
            st = np.array([states[i] for i in rng.integers(0, len(states), m)], np.uint8)
            if m > 1 and rng.random() < 0.3:                  # the same node twice in a batch
                ids[-1], handles[-1], st[-1] = ids[0], handles[0], st[0]
            tails = rng.integers(0, 256, (m, alen + 2), dtype=np.uint8) if alen else None
            ops.append(("new", ids, handles, st, tails))
        elif k == 6:
            ops.append(("expire",))
        elif k == 7 and nxt:
            h = rng.integers(0, nxt + 3, int(rng.integers(1, 12))).astype(np.uint32)
            h = np.unique(h)
            ops.append(("update", h, np.array([states[i] for i in rng.integers(0, len(states), h.size)], np.uint8)))
        elif k == 8 and nxt:
            ops.append(("set", np.array([states[i] for i in rng.integers(0, len(states), int(rng.integers(1, nxt + 5)))],
                                        np.uint8)))
        elif nxt:
            h = np.unique(rng.integers(0, nxt, int(rng.integers(1, 8))).astype(np.uint32))
            ops.append(("good", h, rng.integers(0, 2, h.size).astype(np.uint8)))
    return myid, ops
