// batch_plan.cpp -- K6's host planning: the plan of a call (plan_batch), its workspace layout,
// the deal of F2's workgroups over the sub-partitions, and the one decision a launch makes
// (decide_batch).  Pure functions of the call's shape: no device is touched and no HIP header
// is included (tests/cpp/plan_check.cpp compiles this file alone).  batch.hip holds the kernels.
#include "batch_plan.h"

#include <algorithm>
#include <cmath>

namespace dhtgpu {
namespace {

inline size_t al256(size_t b) { return (b + 255) & ~size_t(255); }

uint32_t floor_log2(uint64_t x) {
    uint32_t r = 0;
    while (x > 1) { x >>= 1; ++r; }
    return r;
}

// P(X < k) for X ~ Poisson(m)
double poisson_below(double m, uint32_t k) {
    double term = std::exp(-m), sum = 0.0;
    for (uint32_t j = 0; j < k; ++j) {
        sum += term;
        term *= m / (double)(j + 1);
    }
    return sum;
}

BatchPlan plan_batch_compute(uint64_t n, uint32_t q, uint32_t k, int num_cus, uint32_t pf) {
    BatchPlan P;
    const bool cells = (pf & kPlanCells) != 0, sorted = (pf & kPlanSorted) != 0;
    // mark level: 4k or more ids per level-Lm subtree -- or one level finer (2k..4k) when, on
    // uniform ids, fewer than 0.01 of the q targets are expected to land in a subtree with
    // under k ids (those go to the F4 brute force).  Without the finer step a prefix shard
    // just under a power of two (n = 2^24 - few) would mark at half the resolution and
    // double the survivors.
    const uint64_t per = 4ull * k;
    P.Lm = n >= per ? floor_log2(n / per) : 0;
    P.sib = 0;
    if (n >= per && P.Lm < kMaxLm) {
        if (poisson_below((double)n / (double)(1ull << (P.Lm + 1)), k) * q <= 0.01) {
            ++P.Lm;
        } else if (cells && P.Lm + 1 == kMaxLm && poisson_below((double)n / (double)(1ull << P.Lm), k) * q <= 0.01) {
            // sibling marking (the set's level-kMaxLm cell counts, kept with its sub-partitions):
            // a target whose level-Lm cell holds < k ids marks the sibling cell too, so it answers
            // from its complete level-(Lm - 1) subtree; only a short PAIR falls back.  One level
            // finer than the rule above allows: the survivors drop from 1 - exp(-q / 2^(Lm-1)) to
            // about 1 - exp(-q / 2^Lm) (cfg 3's broadcast rank: 39 % -> 22 %)
            ++P.Lm;
            P.sib = 1;
        }
    }
    if (P.Lm > kMaxLm) P.Lm = kMaxLm;
    // survivors on uniform ids: n (1 - exp(-q (1 + p) / 2^Lm)), p = the fraction of targets that
    // mark a sibling too; partitions of about kF3Cap / 2
    const double psib = P.sib ? poisson_below((double)n / (double)(1ull << P.Lm), k) : 0.0;
    const double f = 1.0 - std::exp(-(double)q * (1.0 + psib) / (double)(1ull << P.Lm));
    const double surv = (double)n * f + 1.0;
    uint32_t b1 = 0;
    while (b1 + P.sib < P.Lm && surv / (double)(1ull << b1) > kF3Cap / 2) ++b1;   // F3 sorts level Lm - sib
    if (P.Lm > kMaxSubBits && b1 < P.Lm - kMaxSubBits) b1 = P.Lm - kMaxSubBits;
    if (b1 > 13) b1 = 13;   // kMaxParts
    // a partition's survivors come in whole level-Lm subtrees (n / 2^Lm ids each, marked
    // with probability f): on uniform ids mean s f mu, variance s f (1 - f) mu^2 + s f mu
    // over its s = 2^(Lm - b1) subtrees.  Split further until mean + 6 sigma fits the F3
    // stage (an overflowing partition sends its targets to the brute force); plans that
    // cannot are refused (batch_supported), e.g. n >> 2^24 with its 256-id subtrees.
    P.fits = false;
    double need = (double)kF3Cap;   // the partition bound the plan was accepted with
    for (;; ++b1) {
        const double sub = (double)(1ull << (P.Lm - b1)), mu = (double)n / (double)(1ull << P.Lm);
        const double mean = sub * f * mu, var = sub * f * (1.0 - f) * mu * mu + sub * f * mu;
        need = mean + 6.0 * std::sqrt(var) + 64.0;
        if (need <= (double)kF3Cap) { P.fits = true; break; }
        if (b1 >= 13 || b1 + P.sib >= P.Lm) break;
    }
    P.b1 = b1;
    // prefix-sorted sub-partitions (the plans with cell counts): an F2 workgroup's range is a
    // narrow prefix range, so a partition's survivors come from one or two workgroups -- one
    // bucket set, sized for the whole partition (with 8 sets planned for an eighth each, every
    // partition overflowed its set)
    P.nsets = sorted ? 1u : kSets;
    P.clump = sorted ? (1.0 - f) * (double)n / (double)(1ull << P.Lm) + 1.0 : 1.0 - f;
    {   // a set holds each id with probability 1 / kSets (ids are spread over the blocks by
        // index, independently of their prefix): mean + 8 sigma + 64 of one set's share
        const double sub = (double)(1ull << (P.Lm - b1)), mu = (double)n / (double)(1ull << P.Lm) / P.nsets;
        const double mean = sub * f * mu, var = sub * f * (1.0 - f) * mu * mu + sub * f * mu;
        const double cap = mean + 8.0 * std::sqrt(var) + 64.0;
        P.scap = cap >= (double)kF3Cap ? kF3Cap : ((uint32_t)cap + 63u) & ~63u;
        // F3 gathers exactly after the counts: the survivors' bytes only (PMC at cfg 2: 18.5 MB
        // against 19.7 MB algorithmic; round 2's fixed speculative slots fetched 40 MB) and no
        // slower (cfg-2 step 37.7-38.1 us against 38.3-38.4 with a planned mean + 5 sigma)
    }
    // F3 sorts by up to 1 bit below the mark level (finer candidate ranges), <= 4096 bins
    P.Lq = P.Lm + 1 < 32 ? P.Lm + 1 : 32;
    while (P.Lq > P.Lm && P.Lq - P.b1 > 12) --P.Lq;
    // F3's LDS: four workgroups per CU (40 KB each) where the plan allows -- sort one bit less
    // finely, and stage the plan's own 6-sigma bound instead of kF3Cap entries (a partition past
    // it sends its targets to the exact fallback, as one past kF3Cap always did).  The cfg-3
    // shard's plan (b1 = 8, 4096 sort bins: 52 KB) ran three per CU, 2.7 rounds of 2,048 blocks.
    P.f3cap = kF3Cap;
    auto lds3 = [&](uint32_t Lq, uint32_t cap) {
        return (size_t)f3_words(1u << (Lq - P.b1)) * 4 + (size_t)(cap + kF3Threads) * 8;
    };
    constexpr size_t kF3Lds4 = kLdsBytes / 4;
    const uint32_t cap6 = std::min<uint32_t>(kF3Cap, ((uint32_t)need + 63u) & ~63u);
    P.cap6 = cap6;
    if (P.fits && lds3(P.Lq, P.f3cap) > kF3Lds4) {
        for (uint32_t lq = P.Lq; lq >= P.Lm && lq > P.b1; --lq) {
            if (lds3(lq, kF3Cap) <= kF3Lds4) { P.Lq = lq; break; }
            if (lds3(lq, cap6) <= kF3Lds4) { P.Lq = lq; P.f3cap = cap6; break; }
            if (lq == P.Lm) break;
        }
    }
    P.nwords = P.Lm >= 5 ? (1u << (P.Lm - 5)) : 1u;
    P.nblk1 = (q + kF1Threads - 1) / kF1Threads;
    // target buckets: mean + 6 sigma + 64 (uniform targets); overflow spills to F4
    const double mu = (double)q / (double)(1u << P.b1);
    P.tcap = ((uint32_t)(mu + 6.0 * std::sqrt(mu) + 64.0) + 63u) & ~63u;
    // F2: one persistent workgroup per CU, ranges in whole chunks
    const uint64_t chunks = (n + kF2Step - 1) / kF2Step;
    const uint64_t g = num_cus > 0 ? (uint64_t)num_cus : 256;
    const uint64_t cpb = (chunks + g - 1) / g;
    P.per_blk = (cpb ? cpb : 1) * kF2Step;
    P.nblk2 = (uint32_t)((n + P.per_blk - 1) / P.per_blk);
    // F2 LDS stage: what is left of the LDS next to the bitmap and histogram
    const size_t fixed = (size_t)f2_fixed_words(P.nwords, 1u << P.b1) * 4;
    const size_t room = fixed < kLdsBytes ? (kLdsBytes - fixed) / 8 : 0;
    P.stage = (uint32_t)(room < kStage ? room : kStage);
    // sparse mode when a block's survivors (mean + 8 sigma on uniform ids) fit the stage,
    // with ranges shrunk (more blocks) while that helps
    P.sparse = 0;
    for (uint64_t pb = P.per_blk; pb >= kF2Step; pb /= 2) {
        const double mean = (double)pb * f, sd = std::sqrt(mean * P.clump);
        if (mean + 8.0 * sd + 256.0 <= (double)P.stage) {
            P.sparse = 1;
            P.per_blk = (pb / kF2Step) * kF2Step;
            P.nblk2 = (uint32_t)((n + P.per_blk - 1) / P.per_blk);
            break;
        }
        if (pb == kF2Step) break;
    }
    // F2's narrow stage (6 B per entry: ranges < 2^16 ids, the cfg-2 shape): sized so that F2
    // plus one F3 workgroup fit a CU's LDS -- the F2 of one batch in flight and the F3 of another
    // then share CUs instead of waiting for each other's workgroups to drain.  F3 stages its
    // plan's own 6-sigma bound where that is what makes the pair fit (a partition past it sends
    // its targets to the exact fallback, as one past kF3Cap does).  1 KB of margin per kernel
    // for the LDS allocation granule.
    P.nstage = 0;
    P.f3cap_wide = P.f3cap;
    if (P.sparse && P.per_blk <= 65536) {
        const double mean = (double)P.per_blk * f, sd = std::sqrt(mean * (1.0 - f));
        const double need2 = mean + 8.0 * sd + 256.0;
        for (int pass = 0; pass < 2 && !P.nstage; ++pass) {
            uint32_t cap3 = P.f3cap_wide;   // pass 1: F3 stages the 6-sigma bound to make room
            if (pass == 1) {
                if (!P.fits || cap6 >= cap3) break;
                cap3 = cap6;
            }
            const size_t f3l = (lds3(P.Lq, cap3) + 1023) & ~(size_t)1023;
            if (fixed + f3l + 1024 >= kLdsBytes) continue;
            const size_t room6 = (kLdsBytes - f3l - fixed - 1024) / 6;
            if ((double)room6 >= need2) {
                P.nstage = (uint32_t)std::min<size_t>(room6, kStage) & ~1u;
                P.f3cap = cap3;   // committed only with the narrow stage it makes room for
            }
        }
    }
    return P;
}

}  // namespace

// plan_batch is a pure function of (n, q, k, CUs, plan flags), asked three times per call
// (workspace size, clean head, the launch): the last few plans are kept per host thread
BatchPlan plan_batch(uint64_t n, uint32_t q, uint32_t k, int num_cus, uint32_t pf) {
    struct Entry { uint64_t n; uint32_t q, k; int cus; uint32_t pf; BatchPlan P; bool used; };
    thread_local Entry cache[6] = {};
    thread_local uint32_t next = 0;
    for (const Entry& e : cache)
        if (e.used && e.n == n && e.q == q && e.k == k && e.cus == num_cus && e.pf == pf)
            return e.P;
    Entry& e = cache[next++ % 6u];
    e = Entry{n, q, k, num_cus, pf, plan_batch_compute(n, q, k, num_cus, pf), true};
    return e.P;
}

size_t f2_lds(const BatchPlan& P, bool narrow) {
    const size_t fixed = (size_t)f2_fixed_words(P.nwords, 1u << P.b1) * 4;
    return fixed + (narrow ? (size_t)P.nstage * 6 : (size_t)P.stage * 8);
}

size_t f3_lds(const BatchPlan& P, uint32_t cap) {
    const uint32_t nsub = 1u << (P.Lq - P.b1);
    return (size_t)f3_words(nsub) * 4 + (size_t)(cap + kF3Threads) * 8;
}

F1Coarse f1_coarse(const BatchPlan& P, uint32_t nsub, uint32_t q) {
    F1Coarse f{~0u, 0, 0};
    if (q < kF1CoarseMinQ || P.Lm < 5) return f;
    auto lds_ok = [&](uint32_t c) { return (1u << (P.Lm - c - 5)) + (1u << (P.b1 - c)) <= kF1bLdsWords; };
    uint32_t c = 0;
    while (c < P.b1 && c + 5 < P.Lm && ((uint64_t)nsub << (c + 1)) <= kF1aTargets / 16 &&
           ((uint64_t)nsub << (c + 1)) * 512 <= q)
        ++c;
    while (c < P.b1 && c + 5 < P.Lm && !lds_ok(c)) ++c;
    if (!lds_ok(c) || ((uint64_t)nsub << c) > kMaxCoarse) return f;
    f.c = c;
    f.nbins = nsub << c;
    const double M = (double)q / (double)f.nbins;
    f.ccap = ((uint32_t)(M + 8.0 * std::sqrt(M) + 64.0) + 63u) & ~63u;
    return f;
}

WsLayout ws_layout(const BatchPlan& P, uint32_t nsub, uint32_t q, uint32_t k) {
    const size_t NP = (size_t)nsub << P.b1;
    WsLayout L{};
    size_t off = 0;
    auto take = [&](size_t bytes) {
        const size_t r = off;
        off += al256(bytes);
        return r;
    };
    // bitmap first and the counter arrays sized for kMaxParts partitions: the compact layout
    // (counters right behind one another) cost F1 0.5 us and the pipelined cfg-2 step 0.3 us
    // (measured); the clean head is memset once per workspace
    L.bitmap = take(std::max<size_t>(65536, (size_t)nsub * P.nwords * 4));
    L.ctr = take(256);
    L.pcount = take((size_t)kSets * NP * 4);
    L.tcount = take((size_t)kMaxParts * kCtrStride * 4);
    L.tie_hdr = take((size_t)kMaxParts * kTieSlots * 16);
    L.fb_done = take((size_t)kFbBlocks * 4);
    L.tie_cnt = take((size_t)kMaxParts * 4);
    L.ccount = take((size_t)kMaxCoarse * 4);
    L.clean = off;
    L.fb_list = take((size_t)q * 4);
    L.fb_sub = take((size_t)q);
    L.tspill = take((size_t)q * 4);
    L.pstat = take(NP * 4);
    L.tbuf = take(NP * P.tcap * 8);
    L.tie_cand = take(NP * kTieSlots * 64 * 8);
    L.pbuf = take(NP * P.nsets * P.scap * 8);
    L.fb_rec = take((size_t)kFbBlocks * kFbGroup * k * 24);
    L.desc = take((size_t)kMaxSubs * sizeof(SubDesc));
    L.blk_sub = take(kMaxF2Blocks);
    const F1Coarse fc = f1_coarse(P, nsub, q);
    L.cbuf = take((size_t)fc.nbins * fc.ccap * 8);
    L.total = off;
    return L;
}

// F2's workgroups over the sub-partitions: whole rounds of num_cus workgroups, each
// sub-partition's share in proportion to its ids.  Sparse mode: the stage is flushed every
// *seg ids, the most it holds on uniform ids (mean + 8 sigma + 256 survivors) in whole ring
// turns -- one round of workgroups however large the set; when not even one ring turn fits, no
// workgroup gets more ids than that bound.
uint32_t deal_f2_blocks(const BatchPlan& P, const SubSpec* subs, uint32_t nsub, uint32_t q_plan, int num_cus,
                        SubDesc* d, uint32_t* seg) {
    const double f = 1.0 - std::exp(-(double)q_plan / (double)(1ull << P.Lm));
    uint64_t pb_cap = 1ull << 40;   // dense mode: no cap
    if (P.sparse) {
        pb_cap = kF2Step;
        for (uint64_t pb = kF2Step; pb <= (1ull << 31); pb += kF2Step) {
            const double mean = (double)pb * f, sd = std::sqrt(mean * P.clump);
            if (mean + 8.0 * sd + 256.0 > (double)P.stage) break;
            pb_cap = pb;
        }
    }
    *seg = 0xFFFFFFFFu;
    constexpr uint64_t turn = (uint64_t)kF2Ring * kF2Sub;
    if (P.sparse && pb_cap >= turn) {
        *seg = (uint32_t)std::min<uint64_t>(pb_cap / turn * turn, 0x80000000ull);
        pb_cap = 1ull << 40;
    }
    const uint64_t g = num_cus > 0 ? (uint64_t)num_cus : 256;
    uint64_t n_tot = 0, need = 0;
    for (uint32_t i = 0; i < nsub; ++i) {
        n_tot += subs[i].n;
        need += (subs[i].n + pb_cap - 1) / pb_cap;
    }
    const uint64_t total = std::max<uint64_t>(1, (need + g - 1) / g) * g;
    uint32_t blk = 0;
    for (uint32_t i = 0; i < nsub; ++i) {
        const uint64_t n = subs[i].n;
        uint64_t want = n_tot ? (uint64_t)std::llround((double)total * (double)n / (double)n_tot) : 0;
        want = std::max<uint64_t>(want, (n + pb_cap - 1) / pb_cap);
        if (n && !want) want = 1;
        // whole groups of kSets workgroups: block b writes bucket set b % kSets, and scap plans
        // every set for 1 / kSets of a partition's survivors (a sub-partition dealt 4 workgroups
        // would fill only 4 sets, each twice over: overflowing partitions, fallback scans)
        want = (want + kSets - 1) / kSets * kSets;
        uint64_t per = want ? (n + want - 1) / want : kF2Step;
        per = (per + kF2Step - 1) / kF2Step * kF2Step;
        if (per > pb_cap) per = pb_cap;
        const uint64_t nb = n ? (n + per - 1) / per : 0;
        const uint64_t lim = (subs[i].w0s ? subs[i].stride : 5 * subs[i].stride) - 4;
        d[i] = SubDesc{subs[i].w0s ? subs[i].w0s : subs[i].planes, subs[i].planes, subs[i].stride, n, subs[i].gidx,
                       subs[i].base, (uint32_t)(lim < 0xFFFFFFF0ull ? lim : 0xFFFFFFF0ull), blk, (uint32_t)nb, per};
        blk += (uint32_t)nb;
    }
    return blk;
}

BatchRoute route_batch(const BatchPlan& P, const SubDesc* hd, uint32_t nsub, uint32_t seg, bool direct, uint32_t q,
                       uint32_t q_plan) {
    BatchRoute R{};
    for (uint32_t i = 0; i < nsub; ++i) R.seg_used = R.seg_used || (hd[i].nblk && hd[i].per_blk > seg);
    // the narrow stage: every workgroup's range under 2^16 ids and its survivors (mean + 8 sigma
    // + 256 on uniform ids) within the narrow stage; no segments
    R.narrow = !direct && P.nstage && P.sparse && !R.seg_used;
    {
        const double f = 1.0 - std::exp(-(double)q_plan / (double)(1ull << P.Lm));
        for (uint32_t i = 0; i < nsub && R.narrow; ++i) {
            const double mean = (double)hd[i].per_blk * f, sd = std::sqrt(mean * P.clump);
            if (hd[i].nblk && (hd[i].per_blk > 65536 || mean + 8.0 * sd + 256.0 > (double)P.nstage)) R.narrow = false;
        }
    }
    R.f2_mode = R.narrow ? kF2Narrow : P.sparse && R.seg_used ? kF2Seg : P.sparse ? kF2Sparse : kF2Dense;
    R.f2_stage = R.narrow ? P.nstage : P.stage;
    R.f3_cap = R.narrow ? P.f3cap : P.f3cap_wide;
    R.f1c = f1_coarse(P, nsub, q);
    R.f1_two_pass = R.f1c.nbins != 0;
    return R;
}

// k_f2_direct's bitmap window over the deal d of prefix-sorted sub-partitions: every workgroup's
// window is bounded by its sub-partition's largest cell span (spans: level-kMaxLm cells that 2^j
// consecutive ids span) over as many consecutive ids as the workgroup holds -- the next power of
// two, at least 64 words (the cfg-3 shard: 1,024 of 16,384)
uint32_t direct_window(const BatchPlan& P, const SubDesc* d, uint32_t nsub, const uint32_t* spans) {
    uint32_t need = 0;
    for (uint32_t i = 0; i < nsub; ++i) {
        if (!d[i].nblk) continue;
        uint32_t j = 0;
        while (j < 31 && (1ull << j) < d[i].per_blk) ++j;
        need = std::max<uint32_t>(need, (spans[i * 32 + j] >> (kMaxLm - P.Lm + 5)) + 3u);
    }
    uint32_t w = 64;
    while (w < need) w <<= 1;
    return w;
}

bool decide_batch(const BatchShape& c, SubDesc* hd, BatchDecision* out) {
    BatchDecision& D = *out;
    const uint32_t nsub = c.nsub, k = c.k;
    // the plan is the largest sub-partition's
    uint64_t n_max = 0, n_all = 0;
    for (uint32_t i = 0; i < nsub; ++i) {
        n_max = std::max<uint64_t>(n_max, c.subs[i].n);
        n_all += c.subs[i].n;
    }
    const BatchPlan P = D.P = plan_batch(n_max, c.q_plan, k, c.num_cus, c.pf);
    const uint32_t NP = nsub << P.b1;
    D.nblk2 = deal_f2_blocks(P, c.subs, nsub, c.q_plan, c.num_cus, hd, &D.seg);
    // F2 direct (prefix-sorted sub-partitions with span tables; one bucket set): one persistent
    // workgroup per CU -- no stage bounds a range, so the dense deal -- taken when its bitmap window
    // is at most 2 words per thread and half the bitmap
    D.direct = false;
    D.wwords = 0;
    if (c.spans && (c.pf & kPlanSorted) && nsub > 1 && P.Lm >= 6 && P.Lm <= kMaxLm && P.nsets == 1) {
        BatchPlan Pd = P;
        Pd.sparse = 0;
        SubDesc hw[kMaxSubs];
        uint32_t segw = 0;
        const uint32_t nbw = deal_f2_blocks(Pd, c.subs, nsub, c.q_plan, c.num_cus, hw, &segw);
        const uint32_t wd = direct_window(P, hw, nsub, c.spans);
        if (wd <= 2 * kF2Threads && 2 * wd <= P.nwords && nbw <= kMaxF2Blocks) {
            D.direct = true;
            D.wwords = wd;
            D.nblk2 = nbw;
            std::copy(hw, hw + nsub, hd);
        }
    }
    if (D.nblk2 > kMaxF2Blocks) return false;
    D.R = route_batch(P, hd, nsub, D.seg, D.direct, c.q, c.q_plan);
    D.nt = 4 * n_all > kNtBytes;   // F2's ring: non-temporal past the Infinity Cache
    D.f2_form = D.direct ? F2Form::Direct
              : D.R.f2_mode == kF2Narrow ? F2Form::Narrow
              : D.R.f2_mode == kF2Seg ? F2Form::Seg
              : D.R.f2_mode == kF2Sparse ? F2Form::Sparse : F2Form::Dense;
    D.f2_src = nsub == 1 ? F2Src::One : D.nt ? F2Src::SubsNT : F2Src::Subs;
    D.f2_lds = D.direct ? (size_t)(8 + D.wwords + kDirParts) * 4 : f2_lds(P, D.R.narrow);
    // F3 stages the plan's 6-sigma bound beside F2's narrow stage (which it makes room for), and on
    // sub-partitioned calls whose partitions run in several rounds of workgroups when that lets 5 or
    // 6 of them share a CU instead of 4 (F3<8> holds 78 VGPRs: 6 waves per SIMD); F3 is a chain of
    // round trips per workgroup, so a round of more workgroups shortens the launch (a partition past
    // the bound sends its targets to the exact fallback, as one past kF3Cap does)
    D.f3_cap = D.R.f3_cap;
    if (!D.R.narrow && nsub > 1 && k <= 8 && P.fits && P.cap6 < D.f3_cap && NP >= 8u * (uint32_t)std::max(c.num_cus, 1)) {
        auto per_cu = [](size_t l) { return std::min<size_t>(6, kLdsBytes / ((l + 1023) & ~(size_t)1023)); };
        if (per_cu(f3_lds(P, P.cap6)) > per_cu(f3_lds(P, D.f3_cap))) D.f3_cap = P.cap6;
    }
    D.f3_lds = f3_lds(P, D.f3_cap);
    // phase stamps hold 8192 workgroups per kernel; no phase-stamp build for sub-partitioned calls
    D.dbg = (NP > 8192 || D.nblk2 > 8192) ? 0u : c.dbg & 256u;
    D.f3_k = k <= 8 ? 8u : k <= 16 ? 16u : 32u;
    D.f3_subs = nsub > 1;
    D.f3_diag = nsub == 1 && D.dbg != 0;
    D.f3_exact = c.n >= k && (k == 8 || k == 16 || k == 32);
    // F4's grid: its workgroups (50 KB of LDS each) hold CUs the other batches' F2 / F3 want,
    // and on one set (ties answered inline by F3) an empty fallback list leaves them nothing to
    // do -- 32 workgroups when the context's last completed call listed no target (a hint F4
    // leaves in mapped host memory; read without a sync, so possibly a call or two old; a list
    // that appears then is scanned by those 32, still exactly), the full grid otherwise (the
    // fallback scan's parallelism).  Round 5: 128 -> 32 with the tie-count reads gone, cfg-2 step
    // 33.6 -> 31.7-31.9 us (profiles/r05/experiments/f4_idle_ab.txt, f4_idle_grid_ab.txt; 16 and
    // 8 equal).  (a sub-partitioned call fills the chip alone and defers ~1 tie per partition over
    // 2,048+ partitions: the full grid keeps them at about one per wave)
    D.f4_grid = (c.fb_idle && nsub == 1) ? kF4IdleGrid : kFbBlocks;
    return true;
}

// ---- the size queries ------------------------------------------------------------------------

bool batch_supported(uint64_t n, uint32_t q, uint32_t k, int num_cus, uint32_t nsub, uint32_t pf) {
    if (k == 0 || k > kMaxK || n >= (1ull << 31) || nsub == 0 || nsub > kMaxSubs) return false;
    const BatchPlan P = plan_batch(n, q, k, num_cus, pf);
    if ((uint64_t)q * nsub > kMaxQ) return false;
    if (((uint64_t)nsub << P.b1) > kMaxParts) return false;
    // dense mode flushes whenever less than one sub-step of room is left
    if (!P.fits || P.Lm - P.b1 > 13 || (!P.sparse && P.stage < kF2Sub + 1024)) return false;
    return f3_lds(P, P.f3cap_wide) <= kLdsBytes && f2_lds(P) <= kLdsBytes;
}

uint32_t split_bits(uint64_t n) {
    uint32_t sb = 1;
    while (sb < 8 && (n >> sb) > (1ull << 24)) ++sb;
    return sb;
}

bool needs_subs(int num_cus, uint64_t n, uint32_t q, uint32_t k) {
    return n > (1ull << 24) && !batch_supported(n, q, k, num_cus) && q <= (1u << 22);
}

bool subs_sort_rule(uint64_t n, uint32_t q, uint32_t k) {
    const uint32_t sbe = split_bits(n);   // (the split build_subs makes)
    const uint64_t nsub_e = n >> sbe;
    const double qsub = (double)q / (double)(1u << sbe);
    uint32_t lm = 0;
    while (lm < 19 && (nsub_e >> (lm + 1)) >= 4ull * k) ++lm;
    lm = lm + 1 < 19 ? lm + 1 : 19;
    return 1.0 - std::exp(-qsub / (double)(1ull << lm)) > 0.02;
}

size_t batch_ctr_offset(uint64_t n, uint32_t q_plan, uint32_t k, int num_cus, uint32_t nsub, uint32_t pf) {
    return ws_layout(plan_batch(n, q_plan, k, num_cus, pf), nsub, 0, k).ctr;
}

size_t batch_clean_bytes(uint64_t n, uint32_t q_plan, uint32_t k, int num_cus, uint32_t nsub, uint32_t pf) {
    return ws_layout(plan_batch(n, q_plan, k, num_cus, pf), nsub, 0, k).clean;
}

size_t batch_bytes(uint64_t n, uint32_t q, uint32_t q_plan, uint32_t k, int num_cus, uint32_t nsub, uint32_t pf) {
    return ws_layout(plan_batch(n, q_plan, k, num_cus, pf), nsub, q, k).total;
}

size_t list_scan_bytes(uint32_t k) { return al256((size_t)kFbBlocks * 4) + al256((size_t)kFbBlocks * kFbGroup * k * 24); }

// KS's level: the deepest with >= 4k ids per subtree on uniform ids (K6's rule), at most 31
uint32_t small_level(uint64_t n, uint32_t k) {
    uint32_t Ls = 0;
    while (Ls < 31 && (n >> (Ls + 1)) >= 4ull * k) ++Ls;
    return Ls;
}

bool small_supported(uint64_t n, uint32_t q, uint32_t k) {
    return q >= 1 && q <= kSmallQ && k >= 1 && k <= kMaxK && n >= 1 && n < (1ull << 31);
}

// cnt[2][kSmallQ] | tab | fb[kSmallFbBlocks][kSmallQ] | F4 scratch (list_scan_bytes(32): done
// counters first) | cand
size_t small_bytes() {
    return al256((size_t)2 * kSmallQ * 4) + al256((size_t)(kSmallQ + 1) * 4) + al256((size_t)kSmallFbBlocks * kSmallQ * 4) +
           list_scan_bytes(kMaxK) + (size_t)kSmallQ * kSmallCap * 16;
}

// The one-set K6 plan of (n, q, k) as a launch on num_cus CUs would use it: words 1..13 of
// dhtgpu_batch_plan (include/dhtgpu.h).  Host only.
void batch_plan_words(uint64_t n, uint32_t q, uint32_t k, int num_cus, uint32_t* out) {
    const SubSpec one{nullptr, nullptr, pad_ids(n), n, nullptr, 0u};
    SubDesc hd[1];
    BatchDecision D;
    if (!decide_batch(BatchShape{&one, 1, q, q, k, num_cus, 0u, nullptr, n, 0u, false}, hd, &D)) return;
    out[1] = D.P.Lm;
    out[2] = D.P.Lm - D.P.sib;
    out[3] = D.P.b1;
    out[4] = D.P.Lq;
    out[5] = D.P.tcap;
    out[6] = D.P.scap;
    out[7] = D.P.nsets;
    out[8] = D.R.f3_cap;
    out[9] = D.R.f2_mode;
    out[10] = D.R.f2_stage;
    out[11] = (uint32_t)hd[0].per_blk;
    out[12] = D.nblk2;
    out[13] = D.R.f1_two_pass ? 1u : 0u;
}

}  // namespace dhtgpu
