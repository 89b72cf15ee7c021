"""The model and scripts of Dht::searchStep on the resident searches (dhtgpu_srs_*,
opendht_amd/csrc/srstep.hip), shared by test_srstep_cpu.py and test_gpu_srstep.py.

The model is srmap_cases.Model -- rsearch_cases.Model (the oracle's Search::insertNode) plus the
`done` set and the map's walk -- with the state searchStep reads: per slot the request state and the
tick of every listed handle and refill_tick, and the clock.  Insertions are applied ONE AT A TIME
through the parent's insert, so that a handle trimmed and inserted again inside one batch comes back
fresh (req 0, tick 0), and step() restates Dht::searchStep for the find_node search from the
reference (src/dht.cpp:562-654, src/search.h:139-161, :560-567, :734-747) as plain loops.

A case is a SCRIPT as in rsearch_cases / srmap_cases, with the steps ("clock", now), ("request",
slots, handles, val) and ("step", slots, node_expire, refill_count).  Scripts keep rsearch_cases'
rule: at most MAX_BAD handles are ever expired or candidates, so no list outgrows 54 entries."""
import numpy as np

import oracle as O
import rsearch_cases as RS
import srmap_cases as SM

NONE, CAP = RS.NONE, RS.CAP
TARGET_NODES, MAX_REQUESTED, SEARCH_MAX_BAD = 8, 4, 25
B_EXPIRED, B_OVER, B_DONE, B_REFILLED, B_SYNCED, B_SKIPPED = 1, 2, 4, 8, 16, 32
E = 600     # the node_expire every script uses


class Model(SM.Model):
    def __init__(self):
        super().__init__()
        self.clock = 0
        self.req, self.tick, self.rtick = [], [], []   # per slot: {handle: req}, {handle: tick}, refill_tick

    # ---- the state that travels with an entry ---------------------------------------------------
    def reset(self, nslots):
        super().reset(nslots)
        self.req = [{} for _ in range(nslots)]
        self.tick = [{} for _ in range(nslots)]
        self.rtick = [0] * nslots

    def open(self, slots, targets):
        super().open(slots, targets)
        for s in slots:
            self.req[int(s)], self.tick[int(s)], self.rtick[int(s)] = {}, {}, 0

    def prune(self, s):
        """an entry that left the list (a trim, a removal, the filter's cut, expire) took its state along"""
        row = set(self.slots[s].row)
        for d in (self.req[s], self.tick[s]):
            for h in [h for h in d if h not in row]:
                del d[h]

    def insert(self, slots, ins_off, ins_handle, ins_ids, ins_token=None):
        off = [int(x) for x in np.asarray(ins_off).reshape(-1)]
        tot = off[-1]
        handle = [int(h) for h in np.asarray(ins_handle).reshape(-1)[:tot]]
        ids = RS.as_ids(ins_ids)[:tot] if tot else np.zeros((0, 20), np.uint8)
        tok = np.zeros(tot, np.uint8) if ins_token is None else np.asarray(ins_token, dtype=np.uint8)[:tot]
        added = np.zeros(tot, np.uint8)
        for j, s in enumerate(int(x) for x in slots):
            for i in range(off[j], off[j + 1]):
                self.prune(s)
                added[i] = super().insert([s], [0, 1], handle[i:i + 1], ids[i:i + 1], tok[i:i + 1])[0]
                self.prune(s)
                if tok[i] and handle[i] in self.slots[s].row:   # src/search.h:712-718: last_get_reply = now
                    self.tick[s][handle[i]] = self.clock
        return added

    def refill(self, slots, count):
        out = super().refill(slots, count)
        for s in slots:
            self.rtick[int(s)] = self.clock    # src/dht.cpp:658
        return out

    def set_clock(self, now):
        self.clock = int(now)

    def set_request(self, slots, handles, val):
        for s, h, v in zip(slots, handles, np.broadcast_to(np.asarray(val), (len(handles),))):
            if int(h) in self.slots[int(s)].row:
                self.req[int(s)][int(h)] = int(v)

    def entries(self, slots):
        req = np.zeros((len(slots), CAP), np.uint8)
        tick = np.zeros((len(slots), CAP), np.uint32)
        for i, s in enumerate(int(x) for x in slots):
            self.prune(s)
            for j, h in enumerate(self.slots[s].row):
                req[i, j], tick[i, j] = self.req[s].get(h, 0), self.tick[s].get(h, 0)
        return req, tick

    # ---- Dht::searchStep ------------------------------------------------------------------------
    def can_get(self, s, j, node_expire):
        """SearchNode::canGet for the one ANY_QUERY request"""
        h = self.slots[s].row[j]
        if self.state.get(h, 0) & 1:
            return False
        req, tick = self.req[s].get(h, 0), self.tick[s].get(h, 0)
        pending = req == 1
        return (not pending and (tick == 0 or self.clock > tick + node_expire)) or req == 0

    def step(self, slots, node_expire, refill_count):
        m = len(slots)
        send = np.full((m, CAP), NONE, np.uint32)
        out4 = np.zeros((m, 4), np.uint32)
        now = self.clock
        for i, s in enumerate(int(x) for x in slots):
            sl = self.slots[s]
            if sl.expired or s in self.done:
                out4[i, 3] = B_SKIPPED | (B_EXPIRED if sl.expired else 0) | (B_OVER if sl.over else 0) | \
                    (B_DONE if s in self.done else 0)
                continue
            self.prune(s)
            bits = inserted = 0
            nbad = sum(self.is_bad(sl, j) for j in range(len(sl.row)))
            if refill_count and self.rtick[s] + node_expire < now and len(sl.row) - nbad < RS.SEARCH_NODES:
                inserted = int(self.refill([s], refill_count)[0])
                bits |= B_REFILLED
            # Search::isSynced
            n = 0
            synced = True
            for j, h in enumerate(sl.row):
                if self.is_bad(sl, j):
                    continue
                t = self.tick[s].get(h, 0)
                if not (sl.flags[j] & 2 and t != 0 and t + node_expire >= now):
                    synced = False
                    break
                n += 1
                if n == TARGET_NODES:
                    break
            synced = synced and n > 0
            sends = []

            def solicited():
                return sum(1 for j, h in enumerate(sl.row) if not self.is_bad(sl, j) and self.req[s].get(h, 0) == 1)

            if synced:
                self.done.add(s)                  # setDone(): getStatus cleared
                self.req[s] = {}
                bits |= B_SYNCED
            else:
                while solicited() < MAX_REQUESTED:   # searchSendGetValues, one request per call
                    j = next((j for j in range(len(sl.row)) if self.can_get(s, j, node_expire)), None)
                    if j is None:
                        break
                    self.req[s][sl.row[j]] = 1
                    sends.append(sl.row[j])
            sol = solicited()
            lead = next((j for j in range(len(sl.row)) if not self.is_bad(sl, j)), len(sl.row))
            if lead >= min(len(sl.row), SEARCH_MAX_BAD):   # Search::expire()
                sl.expired, sl.row, sl.flags = True, [], []
                self.done.add(s)
                self.prune(s)
                sol = 0
            send[i, : len(sends)] = sends
            out4[i] = [len(sends), sol, inserted, bits | (B_EXPIRED if sl.expired else 0) | (B_OVER if sl.over else 0) |
                       (B_DONE if s in self.done else 0)]
        return send, out4


def run_step(step, model, ctx=None):
    op, a = step[0], step[1:]
    if op == "clock":
        model.set_clock(a[0])
        if ctx:
            ctx.srs_set_clock(a[0])
        return None, None
    if op == "request":
        model.set_request(a[0], a[1], a[2])
        if ctx:
            ctx.srs_set_request(a[0], a[1], a[2])
        return None, None
    if op == "step":
        return model.step(a[0], a[1], a[2]), (ctx.srs_step(a[0], a[1], a[2]) if ctx else None)
    return SM.run_step(step, model, ctx)


def model_state(model):
    """everything the device can be asked about the searches: rows, flags, lens, status, req, tick"""
    slots = np.arange(len(model.slots), dtype=np.uint32)
    return model.lists(slots) + (model.status(slots),) + model.entries(slots)


def ctx_state(ctx, nslots):
    slots = np.arange(nslots, dtype=np.uint32)
    return ctx.sr_lists(slots) + (ctx.sr_status(slots),) + ctx.srs_entries(slots)


STATE_NAMES = ("rows", "flags", "lens", "status", "req", "tick")


# ---- building blocks --------------------------------------------------------------------------------
def u32(x):
    return np.asarray(x, dtype=np.uint32).reshape(-1)


def at(target, d):
    """the id at XOR distance d from target"""
    return np.frombuffer((int.from_bytes(bytes(target), "big") ^ int(d)).to_bytes(20, "big"), np.uint8)


def ids_at(target, ds):
    return np.stack([at(target, d) for d in ds]) if len(ds) else np.zeros((0, 20), np.uint8)


class Script:
    """the steps of a script, applied to a model of its own as they are added, so that a later step can
    be chosen from what an earlier one did"""
    def __init__(self):
        self.steps, self.model, self.results, self.notes = [], Model(), [], {}

    def add(self, *step):
        self.steps.append(step)
        want, _ = run_step(step, self.model)
        self.results.append(want)
        return want

    def fill(self, slot, handles, ds, token=None):
        """insertions into one slot: handles at distances ds from its target"""
        t = self.model.slots[slot].target
        tok = None if token is None else np.broadcast_to(np.asarray(token, np.uint8), (len(handles),)).copy()
        return self.add("insert", u32([slot]), RS.csr([len(handles)]), u32(handles), ids_at(t, ds), tok)


def start(nslots, seed, state=None, same_target=False):
    sc = Script()
    sc.add("reset", nslots)
    if state is not None:
        sc.add("set_state", np.asarray(state, np.uint8))
    targets = np.repeat(O.gen_ids(seed, 1), nslots, axis=0) if same_target else O.gen_ids(seed, nslots)
    sc.add("open", np.arange(nslots, dtype=np.uint32), targets)
    return sc


def steps_of(sc):
    return [r for st, r in zip(sc.steps, sc.results) if st[0] == "step"]


# ---- the edge scripts ---------------------------------------------------------------------------------
# The model keeps one id per handle (rsearch_cases.Model.ids), so a handle means the same node in every
# slot: the scripts below that open all their slots on ONE target place handle h at distance h - 9 (or
# FAR + h) in every list; travel_script, whose map needs distinct targets, uses handles 1000 * slot + h.
def tick_edge_script():
    """tick + E == now, both ways.  Slot 0: 8 good entries replied at tick 400; stepped at now = 1000
    (400 + 600 >= 1000: synced) -- slot 1, the same list, at now = 1001 (not synced, and every entry,
    completed, can be asked again: now > tick + E).  Slot 2: 9 entries replied at 400 and completed, one
    more, the closest, never asked; at now = 1000 only that one is sent (now > tick + E fails at
    equality), at 1001 three of the others follow."""
    sc = start(3, 600, same_target=True)
    h = np.arange(10, 20)
    sc.add("clock", 400)
    for s in (0, 1):
        sc.fill(s, h[:8], h[:8] - 9, token=1)
        sc.add("request", u32([s] * 8), u32(h[:8]), 2)
    sc.fill(2, h[1:], h[1:] - 9, token=1)
    sc.add("request", u32([2] * 9), u32(h[1:]), 2)
    sc.fill(2, h[:1], [1])                     # the closest entry never replied: not synced
    sc.add("clock", 1000)
    sc.add("step", u32([0, 2]), E, 0)
    sc.add("clock", 1001)
    sc.add("step", u32([1, 2, 0]), E, 0)
    return sc


def wrap_script():
    """now = 0xFFFFFFFF: ticks within E of it (tick + E passes 2^32: 64-bit sums) are synced and cannot be
    asked again; slot 1 holds an entry replied at now - E - 1, which is asked again."""
    now = 0xFFFFFFFF
    sc = start(2, 610, same_target=True)
    h = np.arange(10, 18)
    sc.add("clock", now - 100)
    sc.fill(0, h, h - 9, token=1)
    sc.fill(1, h[1:], h[1:] - 9, token=1)
    sc.add("clock", now - E - 1)
    sc.fill(1, h[:1], [1], token=1)
    sc.add("request", u32([0] * 8 + [1] * 8), np.tile(u32(h), 2), 2)
    sc.add("clock", now)
    sc.add("step", u32([1, 0]), E, 0)
    return sc


def sol_script():
    """sol going 3 -> 4: three good entries pending, a candidate (its node not expired) and three good
    ones never asked.  The candidate is sent to and not counted, then exactly one good entry."""
    sc = start(1, 620)
    h = np.arange(10, 17)
    sc.add("clock", 1000)
    sc.fill(0, h, h - 9)
    sc.add("request", u32([0] * 3), u32(h[[0, 2, 5]]), 1)
    sc.add("candidate", u32([0]), u32(h[1:2]), 1)
    sc.add("step", u32([0]), E, 0)
    sc.add("step", u32([0]), E, 0)          # sol is 4: nothing more
    return sc


FAR = 1 << 158      # a distance behind most of a random mirror's keys, whatever the target


def refill_script(nkeys=200):
    """len - bad of 13 vs 14 at a due refill, and refill_tick + E == now, which is not due.  Slot 0 lists
    13 good entries and 2 expired ones, slot 1 lists 14 and 2, slot 2 is empty, slot 3 as slot 0 but
    stepped with refill_count 0.  At now = 1000 (refill_tick 0 + 600 < 1000) slots 0 and 2 refill and
    slot 1 does not; slot 2's refill_tick is then 1000: at now = 1600 it is not due (11 of its nodes
    expired meanwhile: 3 good entries), at 1601 it is."""
    rng = np.random.default_rng(630)
    keys = O.gen_ids(630, nkeys)
    handles = (rng.permutation(nkeys) + 100).astype(np.uint32)
    state = np.zeros(400, np.uint8)
    state[[40, 41]] = 1
    sc = Script()
    sc.add("reset", 4)
    sc.add("nc_set", keys, handles)
    sc.add("set_state", state)
    sc.add("open", np.arange(4, dtype=np.uint32), np.repeat(O.gen_ids(631, 1), 4, axis=0))
    sc.add("clock", 1000)
    for s, good in ((0, 13), (1, 14), (3, 13)):
        h = np.array(list(range(10, 10 + good)) + [40, 41])
        sc.fill(s, h, [FAR + int(x) for x in h])
    sc.add("step", u32([0, 1, 2]), E, 14)
    sc.add("step", u32([3]), E, 0)
    row = sc.model.slots[2].row
    sc.add("update_state", u32(row[3:]), 1)    # 11 of slot 2's 14 nodes expire: 3 good entries left
    sc.add("clock", 1000 + E)
    sc.add("step", u32([2]), E, 14)
    sc.add("clock", 1001 + E)
    sc.add("step", u32([2]), E, 14)
    return sc


def expiry_script():
    """Search::expire(): an empty list; 26 entries with 25 leading bad; 24 entries all bad; 30 entries
    with 24 leading bad (not expired); then every slot stepped again (skipped, but for the last)."""
    state = np.zeros(200, np.uint8)
    state[100:125] = 1
    sc = start(4, 640, state, same_target=True)
    sc.add("clock", 1000)
    bad = np.arange(100, 125)
    good = np.arange(130, 136)
    sc.fill(1, list(bad) + [130], list(bad - 99) + [31])
    sc.fill(2, bad[:24], bad[:24] - 99)
    sc.fill(3, list(bad[:24]) + list(good), list(bad[:24] - 99) + list(good - 99))
    sc.add("step", u32([0, 1, 2, 3]), E, 0)
    sc.add("step", u32([3, 2, 1, 0]), E, 0)
    return sc


def travel_script(nkeys=120):
    """State travels.  Five searches (handles 1000 * slot + h) list 14 good entries 10..23 -- every
    other one replied (a token: tick = the clock) -- then two expired nodes and a removable one, whose
    insertion trims entry 23 and which removeExpiredNode then takes out again: 13 good entries, marked
    with req (index + 1) % 3.  Closer nodes then arrive through sr_insert (one slot, two slots in one
    call), sr_refill and srm_offer, and the marked entries move.  Slot 4 last, in ONE batch: 23 comes
    back, 83 trims it, the removable 72 trims 22 -- marked -- and leaves, 22 is inserted again: it reads
    req 0, tick 0."""
    rng = np.random.default_rng(650)
    keys = O.gen_ids(650, nkeys)
    kh = (rng.permutation(nkeys) + 10000).astype(np.uint32)
    state = np.zeros(5000, np.uint8)
    slots = np.arange(5, dtype=np.uint32)
    for s in slots:
        state[[1000 * s + 60, 1000 * s + 61]] = 1
        state[[1000 * s + 70, 1000 * s + 72]] = 2
    sc = Script()
    sc.add("reset", 5)
    sc.add("nc_set", keys, kh)
    sc.add("set_state", state)
    sc.add("open", slots, O.gen_ids(651, 5))
    far = 1 << 159                             # (bit 159 set: farther than about half of the cached keys)
    loc = np.arange(10, 24)
    for s in (int(x) for x in slots):
        h = 1000 * s + loc
        sc.add("clock", 300 + s)
        sc.fill(s, h, [far + 16 * (int(x) - 9) for x in loc], token=(np.arange(14) + 1) % 2)
        sc.fill(s, 1000 * s + np.array([60, 61, 70]), [far + 3, far + 40, far + 100])
        sc.add("request", u32([s] * 14), u32(h), (np.arange(14) + 1) % 3)
    sc.add("clock", 500)
    sc.fill(0, [80, 81], [far + 5, far + 6], token=[1, 0])
    sc.add("insert", slots[1:3], RS.csr([2, 1]), u32([1080, 1081, 2082]),
           np.concatenate([ids_at(sc.model.slots[1].target, [far + 1, far + 50]), ids_at(sc.model.slots[2].target, [far + 2])]),
           np.array([0, 1, 1], np.uint8))
    sc.add("refill", slots[2:4], 5)
    sc.add("srm_set", slots[:4])               # (slot 4 keeps its 13 good entries for the batch below)
    sc.add("offer", u32([90, 91, 92]), O.gen_ids(652, 3))
    sc.notes["before"] = [x[4, list(sc.model.slots[4].row).index(4022)] for x in sc.model.entries(slots)]
    sc.fill(4, [4023, 4083, 4072, 4022], [far + 16 * 14, far + 7, far + 8, far + 16 * 13])
    sc.notes["batch"] = len(sc.steps) - 1
    sc.add("step", slots, E, 14)
    return sc


def traffic_script(seed, nslots, nkeys, rounds, sizes=(1, 4, 5)):
    """Seeded traffic on nslots find_node searches over an nc mirror: every round the clock moves on,
    some searches are stepped (1, 4 or 5 per call, in turn), and every request sent is answered -- a
    reply (req 2, the node inserted again with a token, two closer nodes it told about inserted or
    offered through the map), an expiry (req 0 and the candidate flag, or the node expired) or nothing."""
    rng = np.random.default_rng(seed)
    keys = O.gen_ids(seed, nkeys)
    kh = (rng.permutation(nkeys) + 100).astype(np.uint32)
    sc = Script()
    sc.add("reset", nslots)
    sc.add("nc_set", keys, kh)
    slots = np.arange(nslots, dtype=np.uint32)
    targets = O.gen_ids(seed + 1, nslots)
    sc.add("open", slots, targets)
    sc.add("srm_set", slots)
    now, next_h, nbad, m = 1000, 5000, 0, sc.model
    id_of = {int(h): k for h, k in zip(kh, keys)}
    for r in range(rounds):
        now += int(rng.choice([1, 7, 50, E // 2, E + 1], p=[0.3, 0.3, 0.2, 0.1, 0.1]))
        sc.add("clock", now)
        size = sizes[r % len(sizes)]
        pick = rng.permutation(nslots)[: min(size, nslots)].astype(np.uint32)
        send, out4 = sc.add("step", pick, E, 14 if r % 4 != 3 else 0)
        rq, ins, cand, offer = [], {}, [], []
        for i, s in enumerate(int(x) for x in pick):
            for h in (int(x) for x in send[i, : out4[i, 0]]):
                u = rng.random()
                if s % 3 == 1:            # a search that converges: every node replies and tells nothing new
                    rq.append((s, h, 2))
                    ins.setdefault(s, []).append((h, 1))
                elif u < 0.75:
                    rq.append((s, h, 2))
                    told = []
                    for _ in range(2):
                        d = int(rng.integers(1, 1 << 62)) << int(rng.integers(0, 90))
                        id_of[next_h] = at(targets[s], d)
                        told.append(next_h)
                        next_h += 1
                    ins.setdefault(s, []).extend([(h, 1), (told[0], 0)])
                    offer.append(told[1])
                elif u < 0.9 and nbad < RS.MAX_BAD - SEARCH_MAX_BAD:
                    nbad += 1
                    rq.append((s, h, 0))
                    cand.append((s, h))
        if rq:
            sc.add("request", u32([x[0] for x in rq]), u32([x[1] for x in rq]), np.array([x[2] for x in rq], np.uint8))
        if cand:
            sc.add("candidate", u32([x[0] for x in cand]), u32([x[1] for x in cand]), 1)
        if ins:
            ss = sorted(ins)
            hh = [x[0] for s in ss for x in ins[s]]
            sc.add("insert", u32(ss), RS.csr([len(ins[s]) for s in ss]), u32(hh), np.stack([id_of[h] for h in hh]),
                   np.array([x[1] for s in ss for x in ins[s]], np.uint8))
        if offer:
            sc.add("offer", u32(offer), np.stack([id_of[h] for h in offer]))
        if r == rounds // 2 and m.slots[0].row:   # one search loses its closest nodes: it expires
            sc.add("update_state", u32(m.slots[0].row[:SEARCH_MAX_BAD]), 1)
            sc.add("step", u32([0]), E, 0)        # (a refill would bring closer good nodes in first)
    sc.add("clock", now + 1)
    sc.add("step", slots[:5] if nslots >= 5 else slots, E, 14)
    return sc


def all_scripts():
    """(name, Script) of every case, built once per process"""
    global _ALL
    if _ALL is None:
        _ALL = [("tick_edge", tick_edge_script()), ("wrap", wrap_script()), ("sol", sol_script()),
                ("refill", refill_script()), ("expiry", expiry_script()), ("travel", travel_script()),
                ("traffic7", traffic_script(700, 7, 250, 14)), ("traffic64", traffic_script(710, 64, 256, 9))]
    return _ALL


_ALL = None
