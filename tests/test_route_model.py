"""K6 route accounting on the CPU: the plan query, every constructed case's precondition under the
256-CU plan (tests/route_cases.py), and the numpy routing model (tests/route_model.py) against a
brute-force restatement of the same rules in per-target Python loops."""
import collections

import numpy as np
import pytest

import opendht_amd
import route_cases as RC
import route_model as M

KS = [8, 14, 32]


# ---- the plan query -----------------------------------------------------------------------------

def test_plan_query_routes_and_words():
    p = opendht_amd.batch_plan(50000, 10, 8)
    assert p["route"] == opendht_amd.ROUTE_KS and p["Ls"] == 10 and p["Lm"] == 0   # 50000 >> 11 < 32 <= 50000 >> 10
    assert opendht_amd.batch_plan(1 << 27, 131072, 8)["route"] == opendht_amd.ROUTE_SUBS
    assert opendht_amd.batch_plan(1 << 20, (1 << 22) + 1, 8)["route"] == opendht_amd.ROUTE_REFUSED
    p = opendht_amd.batch_plan(131072, 1000, 8)
    assert p["route"] == opendht_amd.ROUTE_K6 and p["Lmin"] == p["Lm"] and p["b1"] <= p["Lm"] < p["Lq"] + 1
    assert p["per_blk"] * p["nblk2"] >= 131072 > p["per_blk"] * (p["nblk2"] - 1)
    assert p["tcap"] % 64 == 0 and p["scap"] % 64 == 0 and 0 < p["f3_stage"] <= 4096
    assert p["f2_mode"] in (0, 1, 3, 4) and p["f1_two_pass"] == 0
    assert opendht_amd.batch_plan(32768, 131072, 8)["f1_two_pass"] == 1
    # the CU count is part of the plan: fewer CUs, longer F2 ranges
    assert opendht_amd.batch_plan(1 << 22, 4096, 8, num_cus=64)["per_blk"] > opendht_amd.batch_plan(1 << 22, 4096, 8)["per_blk"]
    L = opendht_amd.lib()
    assert L.dhtgpu_batch_plan(None, 256, 1000, 100, 8, None) == opendht_amd.EINVAL
    out = (opendht_amd.ctypes.c_uint32 * 16)()
    assert L.dhtgpu_batch_plan(None, 256, 1000, 100, 0, out) == opendht_amd.EINVAL
    assert L.dhtgpu_batch_plan(None, 256, 1000, 100, 33, out) == opendht_amd.EINVAL


# ---- the brute-force restatement -------------------------------------------------------------------

def brute(plan, ids, targets, k, shift=0, coarse=None):
    """expect()'s account from per-target loops over the survivors sorted by full key."""
    Lm, Lmin, b1, Lq = plan["Lm"], plan["Lmin"], plan["b1"], plan["Lq"]
    tcap, scap, nsets, per_blk = plan["tcap"], plan["scap"], plan["nsets"], plan["per_blk"]
    full = lambda a: [int.from_bytes(bytes(r), "big") for r in np.asarray(a, dtype=np.uint8).reshape(-1, 20)]
    w0 = lambda x: (x >> (128 - shift)) & 0xFFFFFFFF
    pre = lambda w, L: w >> (32 - L) if L else 0
    ikey, tkey = full(ids), full(targets)
    iw, tw = [w0(x) for x in ikey], [w0(x) for x in tkey]
    n, q = len(iw), len(tw)
    want = min(k, n)
    nparts = 1 << b1
    tparts = collections.defaultdict(list)
    for t in range(q):
        tparts[pre(tw[t], b1)].append(t)
    cellcount = collections.Counter(pre(w, Lm) for w in tw)
    drop_lo, drop_hi = {}, {}
    if plan["f1_two_pass"]:
        c, ccap = coarse or M.f1_coarse(plan, q)
        bins = collections.Counter(pre(w, c) for w in tw)
        over = {b: max(0, m - ccap) for b, m in bins.items()}
        for p, ts in tparts.items():
            b = p >> (b1 - c)
            least = max(0, over[b] - (bins[b] - len(ts)))      # the bin's drops cannot all miss p
            most = min(over[b], len(ts))
            drop_lo[p] = len(ts) - min(len(ts) - least, tcap)
            drop_hi[p] = len(ts) - min(len(ts) - most, tcap)
        mark_hi = set(cellcount)
        mark_lo = {cell for cell, m in cellcount.items() if m > over[cell >> (Lm - c)]}
    else:
        for p, ts in tparts.items():
            drop_lo[p] = drop_hi[p] = max(0, len(ts) - tcap)
        mark_lo = mark_hi = set(cellcount)

    def f2(mark):
        cnt = collections.Counter()
        blk_surv = collections.Counter()
        blk_parts = collections.defaultdict(set)
        by_part = collections.defaultdict(list)
        for i, w in enumerate(iw):
            if pre(w, Lm) in mark:
                b, p = i // per_blk, pre(w, b1)
                cnt[b % nsets, p] += 1
                blk_surv[b] += 1
                blk_parts[b].add(p)
                by_part[p].append(i)
        losers = []
        if plan["f2_mode"] in (M.F2_SPARSE, M.F2_NARROW):
            losers = [(b % nsets, sorted(blk_parts[b]), m - plan["f2_stage"]) for b, m in sorted(blk_surv.items())
                      if m > plan["f2_stage"]]
        return cnt, losers, by_part

    cnt_lo, _, _ = f2(mark_lo)
    cnt_hi, losers, by_part = f2(mark_hi)

    def part_state(cnt, p):
        sets = [cnt[s, p] for s in range(nsets)]
        return any(x > scap for x in sets) or sum(min(x, scap) for x in sets) > plan["f3_stage"]
    certain = {p: part_state(cnt_lo, p) for p in range(nparts)}
    may_lose = {(s, p) for s, parts, _ in losers for p in parts}
    possible = {p: part_state(cnt_hi, p) or any((s, p) in may_lose for s in range(nsets)) for p in range(nparts)}

    cls = [None] * q
    for t in range(q):
        p = pre(tw[t], b1)
        mem = []
        for L in range(Lq, Lmin - 1, -1):
            mem = [i for i in by_part[p] if pre(iw[i], L) == pre(tw[t], L)]
            if len(mem) >= want:
                break
        if len(mem) < want:
            cls[t] = M.SHORT
        elif len(mem) > M.LANE_MAX or Lm == 0:
            cls[t] = M.WAVE
        else:
            mem.sort(key=lambda i: (ikey[i] ^ tkey[t], i))
            d = [iw[i] ^ tw[t] for i in mem[: want + 1]]
            cls[t] = M.WAVE if any(d[j] == d[j + 1] for j in range(len(d) - 1)) else M.FAST
    fb_lo_p, fb_hi_p, wv_lo_p, wv_hi_p = {}, {}, {}, {}
    for p in range(nparts):
        ts = tparts.get(p, [])
        c_p, short, wv = len(ts), sum(cls[t] == M.SHORT for t in ts), sum(cls[t] == M.WAVE for t in ts)
        dl, dh = drop_lo.get(p, 0), drop_hi.get(p, 0)
        fb_lo_p[p] = max(dl, c_p if certain[p] else short)
        fb_hi_p[p] = min(dh + (c_p if possible[p] else short), c_p)
        wv_lo_p[p] = max(0, (0 if possible[p] else wv) - dh)
        wv_hi_p[p] = min(0 if certain[p] else wv, c_p - dl)
    fb = [sum(fb_lo_p.values()), sum(fb_hi_p.values())]
    wave = [sum(wv_lo_p.values()), sum(wv_hi_p.values())]
    surv_lo = sum(min(x, scap) for x in cnt_lo.values())
    surv = [surv_lo, sum(scap if key in may_lose else min(x, scap) for key, x in cnt_hi.items())]
    if losers and mark_lo is mark_hi:
        def span(gain_of):
            least = most = 0
            for s, parts, D in losers:
                g = sorted(gain_of(s, p) for p in parts)
                least = max(least, g[0])
                most += sum(g[::-1][:D])
            return least, most
        least, most = span(lambda s, p: fb_hi_p[p] - fb_lo_p[p])
        fb = [fb[0] + least, min(fb[0] + most, fb[1])]
        least, most = span(lambda s, p: wv_hi_p[p] - wv_lo_p[p])
        wave = [max(wave[1] - most, wave[0]), wave[1] - least]
        least, most = span(lambda s, p: scap - min(cnt_hi[s, p], scap))
        surv = [surv[0] + least, min(surv[0] + most, surv[1])]
    final = [M.PART if certain[pre(tw[t], b1)] else cls[t] for t in range(q)]
    return {"fallback": tuple(fb), "wave": tuple(wave), "survivors": tuple(surv), "cls": final}


def agree(plan, ids, targets, k, shift=0, coarse=None, what=""):
    e = M.expect(plan, ids, targets, k, shift=shift, coarse=coarse)
    b = brute(plan, ids, targets, k, shift=shift, coarse=coarse)
    for key in ("fallback", "wave", "survivors"):
        assert tuple(e[key]) == b[key], f"{what}: {key} model {e[key]} brute {b[key]} plan {plan}"
    assert list(e["cls"]) == b["cls"], f"{what}: route classes differ at {np.nonzero(np.array(b['cls']) != e['cls'])[0][:8]}"
    assert e["fallback"][0] <= e["fallback"][1] and e["wave"][0] <= e["wave"][1] and e["survivors"][0] <= e["survivors"][1]
    return e


def cut_down(case, max_ids=2048, max_targets=96):
    """At most max_ids ids and max_targets targets of a case: the targets off the fast path first,
    every id of the chosen targets' level-Lm cells, then ids in index order."""
    e, Lm = case.expect, case.plan["Lm"]
    order = np.concatenate((np.nonzero(e["cls"] != M.FAST)[0][: max_targets // 2], np.nonzero(e["cls"] == M.FAST)[0]))
    icell = M.top(M.word0(case.ids, case.shift), Lm)
    tcell = M.top(M.word0(case.targets, case.shift), Lm)
    keep_t, cells, size = [], set(), 0
    pops = np.bincount(icell, minlength=1 << Lm)
    for t in order:
        c = int(tcell[t])
        if c not in cells:
            if size + pops[c] > max_ids * 3 // 4:
                continue
            cells.add(c)
            size += int(pops[c])
        keep_t.append(int(t))
        if len(keep_t) == max_targets:
            break
    sel = np.nonzero(np.isin(icell, list(cells)))[0]
    rest = np.nonzero(~np.isin(icell, list(cells)))[0][: max_ids - len(sel)]
    return case.ids[np.sort(np.concatenate((sel, rest)))], case.targets[np.sort(keep_t)]


@pytest.fixture(scope="module")
def cases():
    built = {}

    def get(name, k):
        if (name, k) not in built:
            built[name, k] = RC.build(name, k, num_cus=256)
        return built[name, k]
    return get


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("name", RC.NAMES)
def test_case_precondition_and_model(cases, name, k):
    """Every builder's precondition holds under the 256-CU plan (build() raises otherwise), and
    on the case cut down to <= 2,048 ids the model agrees with the brute force: with the plan's own
    capacities, and with capacities shrunk to the cut-down size so that the overflow rules act."""
    c = cases(name, k)
    assert c.plan == opendht_amd.batch_plan(c.n, c.q, k, num_cus=256)
    e = c.expect
    assert e["fallback"][1] <= c.q and e["survivors"][1] <= c.n
    if name not in ("target_spill", "stage_loss"):
        assert M.tight(e), f"{name}: nothing order-dependent happens, yet the model leaves room: {e['fallback']}, {e['wave']}, {e['survivors']}"
    ids, tg = cut_down(c)
    assert len(ids) <= 2048
    roomy = dict(c.plan, per_blk=256)
    agree(roomy, ids, tg, k, shift=c.shift, what=f"{name} k={k} roomy")
    small = dict(c.plan, per_blk=256, tcap=6, scap=40, f3_stage=200, f2_stage=150)
    agree(small, ids, tg, k, shift=c.shift, coarse=(min(c.plan["b1"], 2), 10), what=f"{name} k={k} small")


def test_cases_reach_their_routes(cases):
    """What each case is named for, from the model's account at k = 8 (the builders assert the same
    on every build; this spells the properties out in one place)."""
    e = cases("clean_packed", 8).expect
    assert cases("clean_packed", 8).plan["Lmin"] >= 12 and cases("clean_unpacked", 8).plan["Lmin"] < 12
    assert e["tcount"][1] <= 64 < e["tcount"][2] <= 128 < e["tcount"][3]
    assert cases("lm0_n5", 8).expect["want"] == 5
    e = cases("deeper_level", 8).expect
    assert set(e["level"]) == {cases("deeper_level", 8).plan["Lmin"], cases("deeper_level", 8).plan["Lq"]}
    e = cases("big_subtree", 8).expect
    assert (e["mm"][:12] > 256).all() and (e["mm"][:12] <= 4096).all()
    c = cases("target_spill", 8)
    assert c.expect["tcount"].max() == c.plan["tcap"] + 50 and c.expect["fallback"][0] >= 50
    c = cases("set_overflow", 8)
    assert c.expect["set_count"].max() > c.plan["scap"] and c.expect["part_m"].max() <= c.plan["f3_stage"]
    c = cases("partition_overflow", 8)
    assert c.expect["set_count"].max() <= c.plan["scap"] and c.expect["set_count"].sum(axis=0).max() > c.plan["f3_stage"]
    c = cases("stage_loss", 8)
    assert c.expect["blk_surv"].max() > c.plan["f2_stage"] and c.expect["set_count"].max() <= c.plan["scap"]
    assert 0 < c.expect["fallback"][0] <= c.expect["fallback"][1] < c.q // 4
    c = cases("dense", 8)
    assert c.plan["f2_mode"] == M.F2_DENSE and c.expect["tcount"].max() > 256
    c = cases("two_pass_f1_clustered", 8)
    assert c.plan["f1_two_pass"] == 1 and c.expect["tcount"].max() >= 3 * c.q // 4
    assert cases("prefix_shard", 8).shift == 3


def test_model_against_brute_force_small_shapes():
    """The model against the brute force on small drawn shapes with capacities small enough that
    every rule acts: spills, coarse bins, set and partition overflow, stage loss, short and big
    subtrees, word-0 ties, Lm == 0, n < k."""
    rng = np.random.RandomState(20)
    seen = collections.Counter()
    for it in range(150):
        Lm = int(rng.randint(0, 7))
        b1 = int(rng.randint(0, min(Lm, 3) + 1))
        n, q, k = int(rng.randint(1, 500)), int(rng.randint(1, 160)), int(rng.choice([1, 3, 8, 14]))
        plan = {"route": 1, "Lm": Lm, "Lmin": Lm, "b1": b1, "Lq": Lm + 1, "tcap": int(rng.choice([2, 6, 60])),
                "scap": int(rng.choice([4, 12, 200])), "nsets": int(rng.choice([1, 8])), "f3_stage": int(rng.choice([16, 64, 4096])),
                "f2_mode": int(rng.choice([0, 1, 4])), "f2_stage": int(rng.choice([8, 40, 4096])), "per_blk": int(rng.choice([16, 64])),
                "nblk2": 0, "f1_two_pass": int(rng.randint(0, 2)), "Ls": 0}
        if plan["f1_two_pass"] and Lm < 5:
            plan["f1_two_pass"] = 0
        coarse = (int(rng.randint(0, b1 + 1)), int(rng.choice([3, 20, 1000])))
        # ids clustered in a few cells with few distinct low words (ties), some equal ids
        bits = Lm + 3
        w = (rng.randint(0, 1 << bits, n).astype(np.int64) << (32 - bits)) + rng.randint(0, 3, n)
        if it % 3 == 0:
            w = (rng.randint(0, 1 << 32, n)).astype(np.int64)
        ids = RC.to_ids(w, it)
        ids[:, 4:19] = 0
        ids[:, 19] = rng.randint(0, 2, n)
        tw = (rng.randint(0, 1 << bits, q).astype(np.int64) << (32 - bits)) + rng.randint(0, 3, q)
        e = agree(plan, ids, RC.to_ids(tw, it + 1000), k, coarse=coarse, what=f"draw {it}")
        seen.update(np.array(["fast", "wave", "short", "part"])[e["cls"]].tolist())
        seen["loose"] += not M.tight(e)
    assert all(seen[x] > 0 for x in ("fast", "wave", "short", "part", "loose")), seen
