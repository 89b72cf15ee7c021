"""A numpy model of where one one-set K6 call (kernels: opendht_amd/csrc/batch.hip; plan and launch
decision: batch_plan.cpp) sends its targets.

expect(plan, ids, targets, k) applies the documented rules of F1 / F2 / F3 to 32-bit word 0 and
returns what dhtgpu_batch_topk_timed's stats4 = {fallback targets, survivors, wave-path targets}
must be, as (lo, hi) bounds: lo == hi unless something order-dependent happens (a target bucket
spills, an F2 workgroup loses stage entries, a two-pass F1 bin overflows).  `plan` is the dict of
opendht_amd.batch_plan(); nothing here looks at the device.  Plain and slow on purpose.

Rules (the kernels of batch.hip):
  F1   a target's partition is its top b1 bits; a partition holds tcap targets, the rest spill
       to the whole-set fallback.  Every target F1 buckets or spills marks its level-Lm cell.
       Two-pass F1 (plan word 13) first groups by coarse bins of ccap targets: a target past a
       full bin spills WITHOUT marking (k_f1_coarse), the kept ones go on as above (k_f1_fine).
  F2   workgroup j = index // per_blk keeps the ids of marked cells (survivors) in bucket set
       j % nsets, scap entries per (set, partition).  Sparse / narrow mode: a workgroup with
       more survivors than its stage drops the excess and pushes the partitions that lost
       entries past scap.
  F3   a partition with a set past scap, or more than the F3 stage entries after capping, or lost
       entries sends its targets to the fallback.  Otherwise a target answers from the deepest
       level L in [Lmin, Lq] whose subtree holds >= want = min(k, n) ids: fallback when even
       level Lmin is short; the wave path when the subtree holds > 256 ids, when Lm == 0, or when
       two of the want + 1 smallest word-0 distances (places [0, want]) are equal; else the fast
       path.
"""
import numpy as np

FAST, WAVE, SHORT, PART = 0, 1, 2, 3   # route classes of a target (PART: its partition overflowed)
LANE_MAX = 256                          # kLaneMax
F2_DENSE, F2_SPARSE, F2_SEG, F2_NARROW = 0, 1, 3, 4


def word0(a, shift=0):
    """Word 0 of (m, 20) big-endian ids as uint64; prefix shards: the next 32 bits from bit `shift`."""
    w = np.ascontiguousarray(a, dtype=np.uint8).reshape(-1, 20).view(">u4").reshape(-1, 5)
    w0 = w[:, 0].astype(np.uint64)
    if shift:
        w0 = ((w0 << np.uint64(shift)) | (w[:, 1].astype(np.uint64) >> np.uint64(32 - shift))) & np.uint64(0xFFFFFFFF)
    return w0


def top(w, b):
    """The top b bits of 32-bit words (int64)."""
    if b == 0:
        return np.zeros(len(w), dtype=np.int64)
    return (w >> np.uint64(32 - b)).astype(np.int64)


def f1_coarse(plan, q):
    """(c, ccap) of two-pass F1: coarse bins = top c bits, ccap targets each.  The rule of
    f1_coarse() in batch_plan.cpp: the finest split with >= 512 targets per bin, at most 256 bins,
    c <= b1 and c <= Lm - 5, the fine pass's LDS (2^(Lm-c-5) + 2^(b1-c) words) within 16,384."""
    Lm, b1 = plan["Lm"], plan["b1"]
    lds_ok = lambda c: (1 << (Lm - c - 5)) + (1 << (b1 - c)) <= 16384
    c = 0
    while c < b1 and c + 5 < Lm and (1 << (c + 1)) <= 256 and (1 << (c + 1)) * 512 <= q:
        c += 1
    while c < b1 and c + 5 < Lm and not lds_ok(c):
        c += 1
    M = q / float(1 << c)
    return c, (int(M + 8.0 * np.sqrt(M) + 64.0) + 63) & ~63


def _f2_f3(plan, iw, mark):
    """Per (set, partition) survivor counts under `mark` (bool per level-Lm cell) and what F3
    makes of them."""
    Lm, b1 = plan["Lm"], plan["b1"]
    nsets, scap, per_blk = plan["nsets"], plan["scap"], plan["per_blk"]
    if plan["f2_mode"] == F2_SEG:
        raise NotImplementedError("segmented F2 (sets from about 2^24 ids) is not modelled")
    nparts = 1 << b1
    s = np.nonzero(mark[top(iw, Lm)])[0]
    blk = s // per_blk
    part = top(iw[s], b1)
    nblk = (len(iw) + per_blk - 1) // per_blk
    blk_surv = np.bincount(blk, minlength=nblk)
    cnt = np.bincount((blk % nsets) * nparts + part, minlength=nsets * nparts).reshape(nsets, nparts)
    lossy = np.zeros(nblk, dtype=bool)
    if plan["f2_mode"] in (F2_SPARSE, F2_NARROW):
        lossy = blk_surv > plan["f2_stage"]
    may_lose = np.zeros((nsets, nparts), dtype=bool)   # a workgroup that loses entries holds some of this partition
    losers = []   # per such workgroup: (its set, its partitions, entries it drops)
    for b in np.nonzero(lossy)[0]:
        parts = np.unique(part[blk == b])
        may_lose[b % nsets, parts] = True
        losers.append((int(b % nsets), parts, int(blk_surv[b] - plan["f2_stage"])))
    capped = np.minimum(cnt, scap)
    m_lo = capped.sum(axis=0)
    m_hi = np.where(may_lose, scap, capped).sum(axis=0)
    certain = (cnt > scap).any(axis=0) | (m_lo > plan["f3_stage"])
    return {"cnt": cnt, "blk_surv": blk_surv, "lossy": lossy, "m_lo": m_lo, "m_hi": m_hi, "losers": losers, "capped": capped,
            "certain": certain, "possible": certain | may_lose.any(axis=0)}


def expect(plan, ids, targets, k, shift=0, coarse=None):
    """The model's account of one K6 call over `ids` (n, 20) and `targets` (q, 20) at k.
    coarse: (c, ccap) of two-pass F1 instead of f1_coarse()'s (small shapes in the model's own test)."""
    assert plan["route"] == 1, "one-set K6 plans only"
    Lm, Lmin, b1, Lq, tcap = plan["Lm"], plan["Lmin"], plan["b1"], plan["Lq"], plan["tcap"]
    assert Lmin == Lm, "sibling marking exists on sub-partitioned calls only"
    iw, tw = word0(ids, shift), word0(targets, shift)
    n, q = len(iw), len(tw)
    want = min(k, n)
    nparts = 1 << b1
    tpart = top(tw, b1)
    tcount = np.bincount(tpart, minlength=nparts)
    cellcount = np.bincount(top(tw, Lm), minlength=1 << Lm)

    # F1: targets dropped per partition (to the fallback), cells certainly / possibly marked
    if plan["f1_two_pass"]:
        c, ccap = coarse or f1_coarse(plan, q)
        bcount = np.bincount(top(tw, c), minlength=1 << c)
        over_b = np.maximum(0, bcount - ccap)
        pb = np.arange(nparts) >> (b1 - c)
        cd_lo = np.maximum(0, over_b[pb] - (bcount[pb] - tcount))   # coarse drops that must hit this partition
        cd_hi = np.minimum(over_b[pb], tcount)
        drop_lo = tcount - np.minimum(tcount - cd_lo, tcap)
        drop_hi = tcount - np.minimum(tcount - cd_hi, tcap)
        mark_hi = cellcount > 0
        mark_lo = cellcount > over_b[np.arange(1 << Lm) >> (Lm - c)]   # more targets than the bin can drop
    else:
        drop_lo = drop_hi = np.maximum(0, tcount - tcap)
        mark_lo = mark_hi = cellcount > 0

    f_lo = _f2_f3(plan, iw, mark_lo)
    f_hi = f_lo if mark_hi is mark_lo else _f2_f3(plan, iw, mark_hi)
    certain, possible = f_lo["certain"], f_hi["possible"]

    # F3: the level and route class of every target, as if bucketed in a partition that fits
    sw = np.sort(iw)
    lo = np.zeros(q, dtype=np.int64)
    hi = np.zeros(q, dtype=np.int64)
    level = np.full(q, -1, dtype=np.int64)
    for L in range(Lq, Lmin - 1, -1):
        pre = top(tw, L).astype(np.uint64)
        l = np.searchsorted(sw, pre << np.uint64(32 - L), side="left") if L else np.zeros(q, dtype=np.int64)
        h = np.searchsorted(sw, (pre + np.uint64(1)) << np.uint64(32 - L), side="left") if L else np.full(q, n)
        take = (level < 0) & ((h - l >= want) | (L == Lmin))
        lo[take], hi[take], level[take] = l[take], h[take], L
    mm = hi - lo
    cls = np.full(q, FAST, dtype=np.int64)
    cls[(mm > LANE_MAX) | (Lm == 0)] = WAVE
    cls[mm < want] = SHORT
    # word-0 ties: only subtrees that hold two equal words can have one
    dup = np.concatenate(([0], np.cumsum(sw[1:] == sw[:-1]))) if n > 1 else np.zeros(1, dtype=np.int64)
    for t in np.nonzero((cls == FAST) & (dup[np.maximum(hi - 1, 0)] - dup[np.minimum(lo, n - 1)] > 0))[0]:
        d = np.sort(sw[lo[t]:hi[t]] ^ tw[t])[: want + 1]
        if (d[1:] == d[:-1]).any():
            cls[t] = WAVE
    cls_fit = cls.copy()
    cls[certain[tpart]] = PART

    # totals: per partition, targets dropped by F1 (any of them) and the classes of the rest
    fbc_n = np.bincount(tpart[cls_fit == SHORT], minlength=nparts)
    wc_n = np.bincount(tpart[cls_fit == WAVE], minlength=nparts)
    fbc_lo = np.where(certain, tcount, fbc_n)
    fbc_hi = np.where(possible, tcount, fbc_n)
    wc_lo = np.where(possible, 0, wc_n)
    wc_hi = np.where(certain, 0, wc_n)
    fb_lo_p, fb_hi_p = np.maximum(drop_lo, fbc_lo), np.minimum(drop_hi + fbc_hi, tcount)
    wv_lo_p, wv_hi_p = np.maximum(0, wc_lo - drop_hi), np.minimum(wc_hi, tcount - drop_lo)
    fb = [int(fb_lo_p.sum()), int(fb_hi_p.sum())]
    wave = [int(wv_lo_p.sum()), int(wv_hi_p.sum())]
    surv = [int(f_lo["m_lo"].sum()), int(f_hi["m_hi"].sum())]
    if f_hi["losers"] and mark_hi is mark_lo:
        # a workgroup that drops D entries makes between 1 and D of its partitions lose (each
        # lost partition lost at least one entry): the sums above let every one of them lose or
        # none.  gain[p]: what partition p adds to a sum when it loses.
        def span(lo_p, hi_p, entries=None):
            gain = hi_p - lo_p
            least, most = 0, 0
            for st, parts, D in f_hi["losers"]:
                g = np.sort(gain[st, parts] if entries else gain[parts])
                least = max(least, int(g[0]))
                most += int(g[::-1][:D].sum())
            return least, min(most, int(gain.sum()))
        least, most = span(fb_lo_p, fb_hi_p)
        fb = [fb[0] + least, fb[0] + most]
        least, most = span(wv_lo_p, wv_hi_p)
        wave = [wave[1] - most, wave[1] - least]
        cap = f_hi["capped"]
        least, most = span(cap, np.full_like(cap, plan["scap"]), True)   # a lost (set, partition) counts scap
        surv = [surv[0] + least, surv[0] + most]
    fb, wave, surv = tuple(fb), tuple(wave), tuple(surv)
    return {"fallback": fb, "wave": wave, "survivors": surv, "tcount": tcount, "cls": cls, "cls_fit": cls_fit,
            "level": level, "mm": mm, "tpart": tpart, "spill": drop_hi, "set_count": f_hi["cnt"],
            "blk_surv": f_hi["blk_surv"], "lossy": f_hi["lossy"], "part_m": f_hi["m_lo"],
            "part_over": (f_hi["cnt"] > plan["scap"]).any(axis=0), "part_fallback": certain,
            "part_maybe_fallback": possible, "want": want}


def tight(e):
    """True when the model leaves no room: nothing order-dependent happened."""
    return all(e[key][0] == e[key][1] for key in ("fallback", "wave", "survivors"))
