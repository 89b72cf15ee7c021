"""Constructed inputs for K6's routes (tests/test_route_model.py, tests/test_gpu_routes.py).

Every builder asks opendht_amd.batch_plan() for the plan of its shape and builds ids and targets
from the plan's numbers, from bits and not from draws: the id set is a list of level-Lm cell
populations laid out over the F2 workgroups' index ranges, every cell's ids spread evenly over the
cell with hashed low bits (so every deeper level's population is known and all word-0 values are
distinct), and targets are placed in chosen cells.  A builder raises Precondition, naming the plan
field that moved, when its shape no longer reaches the route it is named for.

build(name, k, ctx=None, num_cus=256) -> Case; NAMES lists the cases.
"""
import numpy as np

import opendht_amd
import route_model as M

MAX_IDS, MAX_Q = 1 << 18, 1 << 14


class Precondition(AssertionError):
    """The plan no longer admits the case."""


class Case:
    def __init__(self, name, k, plan, ids, targets, shift=0, shard=None, marks=None):
        self.name, self.k, self.plan, self.ids, self.targets = name, k, plan, ids, targets
        self.shift = shift     # prefix shard: the model works on word 0 shifted by this many bits
        self.shard = shard     # (seed, stream ids, pbits, pval, gidx) of a gen_ids_prefix context
        self.marks = marks or {}   # named target index arrays the case's own checks use
        self.expect = M.expect(plan, ids, targets, k, shift=shift)

    @property
    def n(self):
        return self.ids.shape[0]

    @property
    def q(self):
        return self.targets.shape[0]


def need(cond, msg):
    if not cond:
        raise Precondition(msg)


# ---- bits ------------------------------------------------------------------------------------

def mix(x, salt=0):
    """splitmix64 of uint64 values: the hashed low bits and the words 1..4."""
    with np.errstate(over="ignore"):
        z = np.asarray(x, dtype=np.uint64) + np.uint64(0x9E3779B97F4A7C15) * np.uint64(salt + 1)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def to_ids(w0, salt):
    """(m, 20) big-endian ids: word 0 as given, words 1..4 hashed from the position."""
    m = len(w0)
    w = np.empty((m, 5), dtype=">u4")
    w[:, 0] = np.asarray(w0, dtype=np.uint64).astype(np.uint32)
    pos = np.arange(m, dtype=np.uint64)
    for j in range(1, 5):
        w[:, j] = (mix(pos, salt * 8 + j) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    return w.view(np.uint8).reshape(m, 20).copy()


class IdSet:
    """n ids as populations of the 2^Lm level-Lm cells, laid out over F2's index ranges."""

    def __init__(self, plan, n, pops=None):
        self.plan, self.n, self.Lm = plan, n, plan["Lm"]
        self.ncell = 1 << self.Lm
        self.pops = np.full(self.ncell, n // self.ncell, dtype=np.int64) if pops is None else np.asarray(pops, np.int64)
        if pops is None:
            self.pops[: n - int(self.pops.sum())] += 1
        self.pins = []   # (cell, F2 workgroup, ids of the cell whose index lies in that workgroup's range)

    def cpp(self):
        return 1 << (self.Lm - self.plan["b1"])   # cells per partition

    def cells_of(self, part):
        return np.arange(part * self.cpp(), (part + 1) * self.cpp())

    def resize(self, cell, pop, donors):
        """Give `cell` pop ids; the difference comes from / goes to the donor cells, evenly."""
        d = int(self.pops[cell]) - pop
        self.pops[cell] = pop
        donors = np.asarray(donors)
        self.pops[donors] += d // len(donors)
        self.pops[donors[: d % len(donors)]] += 1
        need((self.pops[donors] >= 0).all(), f"donor cells ran out of ids (n = {self.n}, Lm = {self.Lm})")

    def pin(self, cell, blk, count):
        self.pins.append((int(cell), int(blk), int(count)))

    def realize(self, salt):
        """-> (ids (n, 20), cell of every index, rank inside its cell of every index)."""
        pops, n, per_blk = self.pops, self.n, self.plan["per_blk"]
        assert int(pops.sum()) == n, (int(pops.sum()), n)
        start = np.concatenate(([0], np.cumsum(pops)))
        cell = np.repeat(np.arange(self.ncell), pops)
        rank = np.arange(n) - start[cell]
        blk_of = np.full(n, -1, dtype=np.int64)
        for c, b, cnt in self.pins:
            own = np.arange(start[c], start[c + 1])
            free = own[blk_of[own] < 0][:cnt]
            assert len(free) == cnt, f"cell {c} holds fewer than {cnt} unpinned ids"
            blk_of[free] = b
        nblk = (n + per_blk - 1) // per_blk
        # the unpinned ids interleaved (rank-major), so every cell spreads over the workgroups
        unp = np.nonzero(blk_of < 0)[0]
        unp = unp[np.lexsort((cell[unp], rank[unp]))]
        index_of = np.empty(n, dtype=np.int64)
        pos = 0
        for b in range(nblk):
            size = min(per_blk, n - b * per_blk)
            pinned = np.nonzero(blk_of == b)[0]
            assert len(pinned) <= size, f"workgroup {b}: {len(pinned)} pinned ids for {size} slots"
            mem = np.concatenate((pinned, unp[pos: pos + size - len(pinned)]))
            pos += size - len(pinned)
            mem = mem[np.argsort(mix(mem, salt), kind="stable")]   # pinned and free ids mixed inside the range
            index_of[mem] = b * per_blk + np.arange(size)
        cell_i = np.empty(n, dtype=np.int64)
        rank_i = np.empty(n, dtype=np.int64)
        cell_i[index_of], rank_i[index_of] = cell, rank
        span = 1 << (32 - self.Lm)
        pop_i = pops[cell_i]
        step = span // pop_i
        assert (step >= 1).all()
        w0 = (cell_i * span + (rank_i * span) // pop_i + (mix(np.arange(n), salt + 100) % step.astype(np.uint64)).astype(np.int64))
        self.cell_i, self.rank_i = cell_i, rank_i
        return to_ids(w0, salt), cell_i, rank_i

    def index(self, cell, rank):
        i = np.nonzero((self.cell_i == cell) & (self.rank_i == rank))[0]
        assert len(i) == 1
        return int(i[0])


def targets_in(Lm, cells, salt, zero_low=False, half=None, share_bits=None):
    """Word 0 of one target per entry of `cells` (level-Lm cells), low bits hashed; zero_low: the
    cell's first word (XOR order = rank order); half: inside that level-(Lm + 1) half;
    share_bits: all low bits below level share_bits hashed, the bits above it zero."""
    cells = np.asarray(cells, dtype=np.int64)
    span = 1 << (32 - Lm)
    low = (mix(np.arange(len(cells)), salt) % np.uint64(span)).astype(np.int64)
    if zero_low:
        low[:] = 0
    if half is not None:
        low = (low % (span // 2)) + half * (span // 2)
    if share_bits is not None:
        low = low % (1 << (32 - share_bits))
    return cells * span + low


def spread(count, cells):
    """`count` targets dealt round-robin over `cells`."""
    cells = np.asarray(cells)
    return cells[np.arange(count) % len(cells)]


def find_shape(k, ctx, num_cus, shapes, ok):
    """The first (n, q) of `shapes` whose plan `ok` accepts (ok returns None or the reason)."""
    first = None
    for n, q in shapes:
        p = opendht_amd.batch_plan(n, q, k, ctx=ctx, num_cus=num_cus)
        why = "route is %d, not the one-set K6" % p["route"] if p["route"] != 1 else ok(p, n, q)
        if why is None:
            return n, q, p
        first = first or f"n = {n}, q = {q}, k = {k}: {why}"
    raise Precondition(f"no shape at or below 2^18 ids admits the case; {first}")


def eff_sets(p, n):
    return min(p["nsets"], (n + p["per_blk"] - 1) // p["per_blk"])


def safe_cells(p, n, frac=0.75):
    """Marked cells a partition can hold with every bucket set within frac * scap and the
    partition within frac * the F3 stage (ids spread evenly over the workgroups)."""
    cellpop = max(1, n >> p["Lm"])
    return max(1, int(min(frac * p["scap"] * eff_sets(p, n), frac * p["f3_stage"]) // cellpop))


def grid(ns, qs):
    return [(n, q) for n in ns for q in qs]


QS = [1000, 1500, 2000, 2500, 3000, 4000, 6000, 8192]


# ---- the cases -----------------------------------------------------------------------------------

def _abc_targets(p, n, q, S, salt, usable=None):
    """Case 1's placement: partition 1 gets 40 targets (G = 4), partition 2 gets 100 (G = 2),
    partition 3 gets 129..min(tcap, 256) (G = 1); the rest evenly over the other partitions, every
    partition's targets inside few enough cells that nothing overflows."""
    nparts = 1 << p["b1"]
    hi = min(p["tcap"], 256)
    need(nparts >= 4, f"b1 must be >= 2; b1 is now {p['b1']}")
    need(hi >= 129, f"partition 3 must receive between 129 and min(tcap, 256) targets; tcap is now {p['tcap']}")
    counts = np.zeros(nparts, dtype=np.int64)
    counts[1], counts[2], counts[3] = 40, 100, min(hi, 160)
    rest = q - int(counts.sum())
    others = [x for x in range(nparts) if x not in (1, 2, 3)]
    need(rest >= 0 and rest <= len(others) * p["tcap"], f"q = {q} does not fit the other partitions; tcap is now {p['tcap']}")
    for j, x in enumerate(others):
        counts[x] = rest // len(others) + (1 if j < rest % len(others) else 0)
    mc = safe_cells(p, n)
    cells = []
    for x in range(nparts):
        own = S.cells_of(x) if usable is None else usable(x)
        need(len(own) > 0 or counts[x] == 0, f"partition {x} has no usable cell")
        if counts[x]:
            cells.append(spread(counts[x], own[:mc]))
    return targets_in(p["Lm"], np.concatenate(cells), salt)


def _clean(name, k, ctx, num_cus, packed):
    def ok(p, n, q):
        if packed and p["Lmin"] < 12:
            return f"the packed-key loop needs Lmin >= 12; Lmin is now {p['Lmin']}"
        if not packed and p["Lmin"] >= 12:
            return f"the unpacked-key loop needs Lmin < 12; Lmin is now {p['Lmin']}"
        if min(p["tcap"], 256) < 129:
            return f"partition 3 must receive between 129 and min(tcap, 256) targets; tcap is now {p['tcap']}"
        if (n >> p["Lm"]) < k:
            return f"cells must hold >= k ids; n >> Lm is now {n >> p['Lm']}"
        return None
    shapes = grid([131072, 262144], QS) if packed else grid([65536, 131072, 32768], [600] + QS)
    n, q, p = find_shape(k, ctx, num_cus, shapes, ok)
    S = IdSet(p, n)
    ids, _, _ = S.realize(11)
    tw = _abc_targets(p, n, q, S, 12)
    c = Case(name, k, p, ids, to_ids(tw, 13))
    e = c.expect
    need(e["fallback"] == (0, 0) and e["wave"] == (0, 0), f"{name}: the model routes {e['fallback']} targets to the "
         f"fallback and {e['wave']} to the wave path; scap is now {p['scap']}, the F3 stage {p['f3_stage']}")
    tc = e["tcount"]
    need(tc[1] <= 64 and 64 < tc[2] <= 128 and 128 < tc[3] <= min(p["tcap"], 256), f"G = 4 / 2 / 1 partitions: {tc[1:4]}")
    return c


def clean_packed(k, ctx, num_cus):
    return _clean("clean_packed", k, ctx, num_cus, True)


def clean_unpacked(k, ctx, num_cus):
    return _clean("clean_unpacked", k, ctx, num_cus, False)


def _lm0(name, n, k, ctx, num_cus):
    q = 150
    p = opendht_amd.batch_plan(n, q, k, ctx=ctx, num_cus=num_cus)
    need(p["route"] == 1 and p["Lm"] == 0, f"{name}: n = {n} must plan Lm == 0 on the K6 route; route {p['route']}, Lm {p['Lm']}")
    S = IdSet(p, n)
    ids, _, _ = S.realize(21)
    tw = (mix(np.arange(q), 22) & np.uint64(0xFFFFFFFF)).astype(np.int64)
    c = Case(name, k, p, ids, to_ids(tw, 23))
    need(c.expect["wave"] == (q, q) and c.expect["fallback"] == (0, 0), f"{name}: every target takes the wave path")
    return c


def lm0_n40(k, ctx, num_cus):
    return _lm0("lm0_n40", 40, k, ctx, num_cus)


def lm0_n5(k, ctx, num_cus):
    return _lm0("lm0_n5", 5, k, ctx, num_cus)


def _base_shape(k, ctx, num_cus, extra=None):
    """A narrow-or-not shape with whole cells of >= 2k ids and at least 8 partitions."""
    def ok(p, n, q):
        if (n >> p["Lm"]) < 2 * k:
            return f"cells must hold >= 2k ids; n >> Lm is now {n >> p['Lm']}"
        if p["b1"] < 3:
            return f"b1 must be >= 3; b1 is now {p['b1']}"
        return extra(p, n, q) if extra else None
    return find_shape(k, ctx, num_cus, grid([131072, 262144, 65536], QS), ok)


def _filler(p, n, q_rest, S, avoid_parts, salt):
    """q_rest plain targets over the partitions not in avoid_parts, within every capacity."""
    nparts = 1 << p["b1"]
    parts = [x for x in range(nparts) if x not in avoid_parts]
    need(q_rest <= len(parts) * p["tcap"], f"{q_rest} filler targets do not fit {len(parts)} partitions; tcap is now {p['tcap']}")
    mc = safe_cells(p, n)
    cells = [spread(q_rest // len(parts) + (1 if j < q_rest % len(parts) else 0), S.cells_of(x)[:mc])
             for j, x in enumerate(parts)]
    return targets_in(p["Lm"], np.concatenate(cells), salt)


def short_subtrees(k, ctx, num_cus):
    n, q, p = _base_shape(k, ctx, num_cus)
    S = IdSet(p, n)
    donors = S.cells_of(0)[8:]          # partition 0 takes the removed ids and holds no target
    chosen = {int(S.cells_of(1)[0]): k - 1, int(S.cells_of(1)[1]): 1, int(S.cells_of(2)[0]): 0}
    for cell, pop in chosen.items():
        S.resize(cell, pop, donors)
    ids, _, _ = S.realize(31)
    short = np.repeat(np.array(list(chosen)), 5)
    tw = np.concatenate((targets_in(p["Lm"], short, 32), _filler(p, n, q - len(short), S, {0, 1, 2}, 33)))
    c = Case("short_subtrees", k, p, ids, to_ids(tw, 34), marks={"short": np.arange(len(short))})
    e = c.expect
    need(e["fallback"] == (len(short), len(short)) and (e["cls"][: len(short)] == M.SHORT).all()
         and (e["cls"][len(short):] != M.SHORT).all(), f"short_subtrees: fallback must be exactly the {len(short)} targets "
         f"of the emptied cells; the model says {e['fallback']}")
    return c


def deeper_level(k, ctx, num_cus):
    n, q, p = _base_shape(k, ctx, num_cus, lambda p, n, q: None if p["Lq"] > p["Lmin"] else f"Lq must lie below Lmin; Lq is now {p['Lq']}")
    S = IdSet(p, n)
    donors = S.cells_of(0)[8:]
    thin = S.cells_of(1)[:6]            # k + 2 ids: only level Lmin holds >= want
    for cell in thin:
        S.resize(int(cell), k + 2, donors)
    ids, _, _ = S.realize(41)
    t_thin = np.repeat(thin, 4)
    tw = np.concatenate((targets_in(p["Lm"], t_thin, 42), _filler(p, n, q - len(t_thin), S, {0, 1}, 43)))
    c = Case("deeper_level", k, p, ids, to_ids(tw, 44))
    e = c.expect
    lv = e["level"]
    need((lv[: len(t_thin)] == p["Lmin"]).all() and (lv[len(t_thin):] == p["Lq"]).all() and e["fallback"] == (0, 0),
         f"deeper_level: thin cells must answer at level Lmin = {p['Lmin']} and whole cells at Lq = {p['Lq']}")
    return c


def w0_ties(k, ctx, num_cus):
    n, q, p = _base_shape(k, ctx, num_cus, lambda p, n, q: None if p["Lq"] == p["Lm"] + 1 else f"Lq must be Lm + 1; Lq is now {p['Lq']}")
    S = IdSet(p, n)
    donors = S.cells_of(0)[8:]
    own = S.cells_of(1)
    # four cells of 2 (k + 4) ids: a target on the cell's first word answers from the first half
    # (k + 4 ids, level Lq), its candidates in rank order
    kinds = {"at_want": (k - 1, k), "inside": (2, 3), "beyond": (k + 1, k + 2), "equal_ids": (0, 1)}
    cells = {name: int(own[j]) for j, name in enumerate(kinds)}
    for cell in cells.values():
        S.resize(cell, 2 * (k + 4), donors)
    ids, _, _ = S.realize(51)
    for name, (ra, rb) in kinds.items():
        a, b = S.index(cells[name], ra), S.index(cells[name], rb)
        if name == "equal_ids":
            ids[b] = ids[a]             # the index decides
        else:
            ids[b, :4] = ids[a, :4]     # word 0 only: words 1..4 differ
    special = np.array([cells[x] for x in kinds])
    tw = np.concatenate((targets_in(p["Lm"], special, 52, zero_low=True),
                         targets_in(p["Lm"], np.repeat(special, 3), 53, half=0),
                         _filler(p, n, q - 16, S, {0, 1}, 54)))
    c = Case("w0_ties", k, p, ids, to_ids(tw, 55), marks={"kinds": list(kinds)})
    cls = c.expect["cls"][:4]
    want_cls = [M.WAVE, M.WAVE, M.FAST, M.WAVE]
    need(list(cls) == want_cls and c.expect["fallback"] == (0, 0),
         f"w0_ties: the targets on the cells' first words must route {want_cls} (at_want, inside, beyond, equal_ids); model: {list(cls)}")
    return c


def big_subtree(k, ctx, num_cus):
    n, q, p = _base_shape(k, ctx, num_cus, lambda p, n, q: None if p["Lq"] == p["Lm"] + 1 else f"Lq must be Lm + 1; Lq is now {p['Lq']}")
    S = IdSet(p, n)
    donors = np.concatenate((S.cells_of(0)[8:], S.cells_of(3)))
    a, b = int(S.cells_of(1)[0]), int(S.cells_of(2)[0])
    pop = 2 * 300                        # halves of 300 ids: > kLaneMax, a lane-distributed list (mm > 64)
    need(pop <= p["f3_stage"] and pop // eff_sets(p, n) + 1 <= p["scap"], f"a 600-id cell must fit a set; scap is now {p['scap']}")
    S.resize(a, pop, donors)
    S.resize(b, pop, donors)
    ids, _, _ = S.realize(61)
    ids[S.index(b, 1), :4] = ids[S.index(b, 0), :4]   # a word-0 tie among the first places
    tw = np.concatenate((targets_in(p["Lm"], [b], 62, zero_low=True), targets_in(p["Lm"], [a] * 6 + [b] * 5, 63),
                         _filler(p, n, q - 12, S, {0, 1, 2, 3}, 64)))
    c = Case("big_subtree", k, p, ids, to_ids(tw, 65))
    e = c.expect
    need((e["cls"][:12] == M.WAVE).all() and (e["mm"][:12] > M.LANE_MAX).all() and e["wave"] == (12, 12) and e["fallback"] == (0, 0),
         f"big_subtree: the 12 targets of the two 600-id cells take the wave path; model: wave {e['wave']}, fallback {e['fallback']}")
    return c


def target_spill(k, ctx, num_cus):
    n, q, p = _base_shape(k, ctx, num_cus)
    S = IdSet(p, n)
    ids, _, _ = S.realize(71)
    c1 = p["tcap"] + 50
    cell = int(S.cells_of(1)[3])
    tw = np.concatenate((targets_in(p["Lm"], [cell] * c1, 72, share_bits=19), _filler(p, n, q - c1, S, {1}, 73)))
    need(q - c1 >= 0, f"tcap + 50 targets exceed q = {q}; tcap is now {p['tcap']}")
    c = Case("target_spill", k, p, ids, to_ids(tw, 74))
    e = c.expect
    need(e["tcount"][1] == c1 and e["fallback"][0] >= 50 and len(np.unique(M.word0(c.targets[:c1]) >> np.uint64(13))) == 1,
         f"target_spill: partition 1 must receive tcap + 50 = {c1} targets sharing their top 19 bits; model fallback {e['fallback']}")
    return c


def set_overflow(k, ctx, num_cus):
    n, q, p = _base_shape(k, ctx, num_cus)
    S = IdSet(p, n)
    cellpop = n >> p["Lm"]
    ncells = p["scap"] // cellpop + 2          # whole cells inside workgroup 0's range: > scap ids
    need(ncells <= S.cpp() and ncells * cellpop <= p["f3_stage"] and ncells * cellpop <= p["per_blk"],
         f"{ncells} cells of one partition must fit the F3 stage; scap is now {p['scap']}, the F3 stage {p['f3_stage']}")
    own = S.cells_of(1)[:ncells]
    for cell in own:
        S.pin(cell, 0, cellpop)
    ids, _, _ = S.realize(81)
    t1 = spread(min(p["tcap"], 3 * ncells), own)
    tw = np.concatenate((targets_in(p["Lm"], t1, 82), _filler(p, n, q - len(t1), S, {1}, 83)))
    c = Case("set_overflow", k, p, ids, to_ids(tw, 84))
    e = c.expect
    need(e["part_over"][1] and e["part_over"].sum() == 1 and e["part_m"][1] <= p["f3_stage"] and not e["lossy"].any()
         and e["fallback"] == (len(t1), len(t1)),
         f"set_overflow: set 0 of partition 1 must pass scap = {p['scap']} with the partition within the F3 stage; "
         f"counts {e['set_count'][:, 1]}, fallback {e['fallback']}")
    return c


def partition_overflow(k, ctx, num_cus):
    def ok(p, n, q):
        cellpop = n >> p["Lm"]
        nc = p["f3_stage"] // cellpop + 2
        if nc > (1 << (p["Lm"] - p["b1"])):
            return f"a partition must hold more ids than the F3 stage; it holds {n >> p['b1']}, the F3 stage {p['f3_stage']}"
        if nc > p["tcap"]:
            return f"{nc} cells need as many targets; tcap is now {p['tcap']}"
        nb = (n + p["per_blk"] - 1) // p["per_blk"]
        per_set = -(-nb // p["nsets"]) * (-(-nc * cellpop // nb) + 1)
        if per_set > p["scap"]:
            return f"{nc * cellpop} ids over the sets give {per_set} per set; scap is now {p['scap']}"
        return None
    n, q, p = _base_shape(k, ctx, num_cus, ok)
    S = IdSet(p, n)
    cellpop = n >> p["Lm"]
    nc = p["f3_stage"] // cellpop + 2
    own = S.cells_of(1)[:nc]
    ids, _, _ = S.realize(91)
    t1 = spread(nc, own)
    tw = np.concatenate((targets_in(p["Lm"], t1, 92), _filler(p, n, q - len(t1), S, {1}, 93)))
    c = Case("partition_overflow", k, p, ids, to_ids(tw, 94))
    e = c.expect
    need(not e["part_over"].any() and e["set_count"][:, 1].sum() > p["f3_stage"] and e["fallback"] == (nc, nc),
         f"partition_overflow: partition 1 must pass the F3 stage = {p['f3_stage']} with every set within scap = {p['scap']}; "
         f"counts {e['set_count'][:, 1]}, fallback {e['fallback']}")
    return c


def stage_loss(k, ctx, num_cus):
    def ok(p, n, q):
        if p["f2_mode"] not in (M.F2_SPARSE, M.F2_NARROW):
            return f"F2 must run a sparse or narrow stage; mode is now {p['f2_mode']}"
        if p["f2_stage"] + 2 > min(p["per_blk"], n):
            return f"a workgroup's range ({p['per_blk']} ids) must hold more than the stage ({p['f2_stage']})"
        if ((p["scap"] - 8) << p["b1"]) < p["f2_stage"] + 2:
            return (f"2^b1 partitions of at most scap survivors must pass the F2 stage; b1 is now {p['b1']}, "
                    f"scap {p['scap']}, the stage {p['f2_stage']}")
        if (1 << p["b1"]) * 3 > q:
            return "q too small"
        return None
    n, q, p = find_shape(k, ctx, num_cus, grid([65536, 131072, 262144, 32768], [2000, 2500, 3000, 4000, 6000, 8192, 1000, 1500]), ok)
    S = IdSet(p, n)
    cellpop = n >> p["Lm"]
    nparts = 1 << p["b1"]
    nblk = (n + p["per_blk"] - 1) // p["per_blk"]
    need(nblk >= 2, f"more than one F2 workgroup; per_blk is now {p['per_blk']}")
    total = p["f2_stage"] + 2              # two survivors past the stage: at most two partitions lose
    per_part = [total // nparts + (1 if x < total % nparts else 0) for x in range(nparts)]
    marked = []
    for x in range(nparts):
        nc = -(-per_part[x] // cellpop)
        need(nc <= S.cpp(), f"partition {x} needs {nc} cells; it has {S.cpp()}")
        own = S.cells_of(x)[:nc]
        left = per_part[x]
        for cell in own:
            S.pin(cell, 0, min(cellpop, left))
            for j in range(cellpop - min(cellpop, left)):   # the marked cells' other ids: any other workgroup
                S.pin(cell, 1 + (int(cell) + j) % (nblk - 1), 1)
            left -= min(cellpop, left)
        marked.append(own)
    ids, _, _ = S.realize(101)
    cells = np.concatenate([spread(q // nparts + (1 if x < q % nparts else 0), marked[x]) for x in range(nparts)])
    need(q // nparts + 1 <= p["tcap"], f"q / 2^b1 targets per partition; tcap is now {p['tcap']}")
    c = Case("stage_loss", k, p, ids, to_ids(targets_in(p["Lm"], cells, 102), 103))
    e = c.expect
    need(e["lossy"][0] and e["lossy"].sum() == 1 and e["blk_surv"][0] == total and not e["part_over"].any()
         and not e["part_fallback"].any(),
         f"stage_loss: workgroup 0 must hold {total} survivors (stage {p['f2_stage']}) with no set past scap = {p['scap']}; "
         f"it holds {e['blk_surv'][0]}, sets up to {e['set_count'].max()}")
    return c


def dense(k, ctx, num_cus):
    def ok(p, n, q):
        if p["f2_mode"] != M.F2_DENSE:
            return f"F2 must run dense; mode is now {p['f2_mode']}"
        avg = q >> p["b1"]
        if min(p["tcap"], avg * 3 // 2) <= 256:
            return f"a partition must receive more than 256 targets; tcap is now {p['tcap']}, q / 2^b1 = {avg}"
        if (n >> p["Lm"]) < k:
            return "cells hold fewer than k ids"
        return None
    n, q, p = find_shape(k, ctx, num_cus, grid([32768, 65536], [8192, 16384]), ok)
    S = IdSet(p, n)
    ids, _, _ = S.realize(111)
    nparts = 1 << p["b1"]
    avg = q // nparts
    hi = min(p["tcap"], avg * 3 // 2)
    mc = min(safe_cells(p, n, 0.8), S.cpp())
    cells = []
    for x in range(nparts):
        cnt = hi if x % 2 == 0 else 2 * avg - hi
        own = S.cells_of(x)[:1] if x == 2 else S.cells_of(x)[:mc]   # partition 2: clustered in one cell
        cells.append(spread(cnt, own))
    cells = np.concatenate(cells)
    assert len(cells) == q
    c = Case("dense", k, p, ids, to_ids(targets_in(p["Lm"], cells, 112), 113))
    e = c.expect
    need(e["tcount"].max() > 256 and e["fallback"] == (0, 0) and e["tcount"][2] > 256,
         f"dense: partitions of more than 256 targets answered by F3; the model says fallback {e['fallback']}; scap is now {p['scap']}")
    return c


def _two_pass(name, k, ctx, num_cus, clustered):
    n, q = 32768, 131072
    p = opendht_amd.batch_plan(n, q, k, ctx=ctx, num_cus=num_cus)
    need(p["route"] == 1 and p["f1_two_pass"] == 1, f"{name}: F1 must run as coarse + fine (plan word 13); it is now {p['f1_two_pass']}")
    S = IdSet(p, n)
    ids, _, _ = S.realize(121)
    nparts = 1 << p["b1"]
    if not clustered:
        tw = (mix(np.arange(q), 122) & np.uint64(0xFFFFFFFF)).astype(np.int64)
        tw = (np.arange(q) % (1 << p["Lm"])) * (1 << (32 - p["Lm"])) + tw % (1 << (32 - p["Lm"]))   # every cell alike
    else:
        cb, ccap = M.f1_coarse(p, q)
        big = 3 * q // 4
        hot = int(S.cells_of(nparts - 1)[0])          # 3/4 of the targets in one cell of the last coarse bin
        need(big > ccap, f"{big} targets must overflow a coarse bin of {ccap}")
        mc = min(safe_cells(p, n, 0.8), S.cpp())
        others = [x for x in range(nparts) if (x >> (p["b1"] - cb)) != ((nparts - 1) >> (p["b1"] - cb))]
        rest = q - big
        need(len(others) > 0 and -(-rest // len(others)) <= p["tcap"], f"the other bins hold {rest} targets; tcap is now {p['tcap']}")
        cells = [spread(rest // len(others) + (1 if j < rest % len(others) else 0), S.cells_of(x)[:mc])
                 for j, x in enumerate(others)]
        tw = np.concatenate((targets_in(p["Lm"], [hot] * big, 123), targets_in(p["Lm"], np.concatenate(cells), 124)))
    c = Case(name, k, p, ids, to_ids(tw, 125))
    if clustered:
        e = c.expect
        need(e["fallback"][0] >= big - max(ccap, p["tcap"]) and M.tight(e),
             f"{name}: the hot bin must spill and the model stay tight; fallback {e['fallback']}, survivors {e['survivors']}")
    return c


def two_pass_f1_uniform(k, ctx, num_cus):
    return _two_pass("two_pass_f1_uniform", k, ctx, num_cus, False)


def two_pass_f1_clustered(k, ctx, num_cus):
    return _two_pass("two_pass_f1_clustered", k, ctx, num_cus, True)


SHARD_SEED, SHARD_PBITS, SHARD_PVAL = 4242, 3, 5


def prefix_shard(k, ctx, num_cus):
    """Case 1's placement on a gen_ids_prefix context: the ids are the stream's (oracle.gen_ids),
    the model works on word 0 shifted by the shard's prefix bits."""
    import oracle as O
    last = None
    # (the second stream: a shard just past 2^18 ids, where k = 32 still plans Lm = 12)
    for stream in (1 << 20, (1 << 21) + (1 << 13)):
        allids = O.gen_ids(SHARD_SEED, stream)
        sel = np.nonzero((allids[:, 0] >> (8 - SHARD_PBITS)) == SHARD_PVAL)[0]
        ids = allids[sel]
        n = len(sel)
        try:
            def ok(p, n_, q):
                if p["Lmin"] < 12:
                    return f"the packed-key loop needs Lmin >= 12; Lmin is now {p['Lmin']}"
                if min(p["tcap"], 256) < 129:
                    return f"partition 3 must receive between 129 and min(tcap, 256) targets; tcap is now {p['tcap']}"
                return None
            n, q, p = find_shape(k, ctx, num_cus, [(n, q) for q in QS], ok)
        except Precondition as e:
            last = e
            continue
        need(n <= MAX_IDS + 4096, f"shard of {n} ids")
        iw = M.word0(ids, SHARD_PBITS)
        pops = np.bincount(M.top(iw, p["Lm"]), minlength=1 << p["Lm"])
        sw = np.sort(iw)
        dupcell = np.zeros(1 << p["Lm"], dtype=bool)
        dupcell[M.top(sw[1:][sw[1:] == sw[:-1]], p["Lm"])] = True
        half = np.bincount(M.top(iw, p["Lm"] + 1), minlength=2 << p["Lm"]).reshape(-1, 2).min(axis=1)
        good = (half >= k) & (pops <= 200) & ~dupcell          # both halves answer at level Lq, no ties
        S = IdSet(p, n, pops)
        tws = _abc_targets(p, n, q, S, 132, usable=lambda x: S.cells_of(x)[good[S.cells_of(x)]])
        # the shifted word back to a target id: the shard's prefix, then the 32 bits
        t = to_ids(tws, 133)
        w = t.view(">u4").reshape(-1, 5)
        v = tws.astype(np.uint64)
        w[:, 0] = ((np.uint64(SHARD_PVAL) << np.uint64(32 - SHARD_PBITS)) | (v >> np.uint64(SHARD_PBITS))).astype(np.uint32)
        w[:, 1] = (((v & np.uint64((1 << SHARD_PBITS) - 1)) << np.uint64(32 - SHARD_PBITS)) |
                   (w[:, 1].astype(np.uint64) >> np.uint64(SHARD_PBITS))).astype(np.uint32)
        c = Case("prefix_shard", k, p, ids, t, shift=SHARD_PBITS, shard=(SHARD_SEED, stream, SHARD_PBITS, SHARD_PVAL, sel))
        e = c.expect
        need(e["fallback"] == (0, 0) and e["wave"] == (0, 0) and M.tight(e), f"prefix_shard: clean cells only; model {e['fallback']}, {e['wave']}")
        tc = e["tcount"]
        need(tc[1] <= 64 and 64 < tc[2] <= 128 and 128 < tc[3] <= min(p["tcap"], 256), f"G = 4 / 2 / 1 partitions: {tc[1:4]}")
        return c
    raise last


BUILDERS = {f.__name__: f for f in (clean_packed, clean_unpacked, lm0_n40, lm0_n5, short_subtrees, deeper_level, w0_ties,
                                    big_subtree, target_spill, set_overflow, partition_overflow, stage_loss, dense,
                                    two_pass_f1_uniform, two_pass_f1_clustered, prefix_shard)}
NAMES = list(BUILDERS)
BIG_Q = {"two_pass_f1_uniform", "two_pass_f1_clustered"}   # the cases the issue allows past 2^14 targets


def build(name, k, ctx=None, num_cus=256):
    c = BUILDERS[name](k, ctx, num_cus)
    assert c.n <= MAX_IDS + 4096 and (c.q <= MAX_Q or name in BIG_Q), (name, c.n, c.q)
    return c
