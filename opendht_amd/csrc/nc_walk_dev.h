// nc_walk_dev.h -- NodeCache::getCachedNodes (src/node_cache.cpp:42-74) over the resident mirror by
// one wave64, shared by k_nc (ncache.hip: the handles go to a result row) and k_sr_refill
// (rsearch.hip: every accepted key goes straight into a search's node list).  The method -- the
// 64-ary lower bound, the two 64-key windows held as distances, the head-comparison walk -- is
// described at the top of ncache.hip.
#pragma once
#include "dhtgpu_dev.h"
#include "dhtgpu_internal.h"

namespace dhtgpu {

__device__ __forceinline__ uint32_t nc_lane(uint32_t x, uint32_t l) {
    return (uint32_t)__builtin_amdgcn_readlane((int)x, (int)l);
}

// the first key >= t (wave-uniform; every lane of the wave calls this)
__device__ __forceinline__ uint32_t nc_lower_bound(const NcView& v, const uint32_t (&t)[DHT_W], uint32_t lane) {
    uint32_t lo = 0, hi = v.n;   // the bound lies in [lo, hi]
    while (hi - lo > 64) {
        const uint32_t step = (uint32_t)(((uint64_t)(hi - lo) + 63) >> 6);   // >= 2
        const uint64_t p = (uint64_t)lo + (uint64_t)(lane + 1) * step - 1;
        bool lt = false;
        if (p < hi) {
            uint32_t k[DHT_W];
            load_id(v.kp, v.ks, p, k);
            lt = lex_lt(k, t);
        }
        const uint32_t c = (uint32_t)__popcll(__ballot(lt));   // pivots below t: a prefix of the lanes
        const uint64_t nlo = (uint64_t)lo + (uint64_t)c * step;   // pivot c - 1 is below t
        const uint64_t pc = nlo + step - 1;                       // pivot c is not, when it exists
        if (pc < hi) hi = (uint32_t)pc;
        lo = (uint32_t)nlo;   // <= hi: the range shrinks to less than `step` keys
    }
    const uint64_t i = (uint64_t)lo + lane;
    bool lt = false;
    if (i < hi) {
        uint32_t k[DHT_W];
        load_id(v.kp, v.ks, i, k);
        lt = lex_lt(k, t);
    }
    return __builtin_amdgcn_readfirstlane(lo + (uint32_t)__popcll(__ballot(lt)));
}

// The walk from the lower bound: sink(c, xd, h, s) for the c-th accepted key, c < count, in the
// reference's order -- xd[5] its distance to t and h its handle (wave-uniform), and, when STATE,
// s = st[h] (0 for h >= nst; gathered with the windows, one guarded load per key).  Returns the
// number of accepted keys.
template <bool STATE, class Sink>
__device__ __forceinline__ uint32_t nc_walk(const NcView& v, const uint8_t* __restrict__ st, uint32_t nst,
                                            const uint32_t (&t)[DHT_W], uint32_t count, uint32_t lane, Sink&& sink) {
    const uint32_t n = v.n;
    const uint32_t lb = nc_lower_bound(v, t, lane);

    // the two windows: distances (key ^ t), handles, accept ballots
    uint32_t nd[DHT_W], pd[DHT_W], nh = DHT_NONE, ph = DHT_NONE, ns = 0, ps = 0;
    uint64_t nacc = 0, pacc = 0;
#pragma unroll
    for (int w = 0; w < DHT_W; ++w) nd[w] = pd[w] = 0;
    auto load_next = [&](uint32_t base) {   // lane l: key base + l
        const uint64_t i = (uint64_t)base + lane;
        bool a = false;
        if (i < n) {
#pragma unroll
            for (int w = 0; w < DHT_W; ++w) nd[w] = v.kp[(uint64_t)w * v.ks + i] ^ t[w];
            nh = v.hp[i];
            a = (v.bits[nh >> 5] >> (nh & 31u)) & 1u;
            if (STATE) ns = nh < nst ? st[nh] : 0u;
        }
        nacc = __ballot(a);
    };
    auto load_prev = [&](uint32_t base) {   // lane l: key base - 1 - l
        bool a = false;
        if (lane < base) {
            const uint32_t i = base - 1 - lane;
#pragma unroll
            for (int w = 0; w < DHT_W; ++w) pd[w] = v.kp[(uint64_t)w * v.ks + i] ^ t[w];
            ph = v.hp[i];
            a = (v.bits[ph >> 5] >> (ph & 31u)) & 1u;
            if (STATE) ps = ph < nst ? st[ph] : 0u;
        }
        pacc = __ballot(a);
    };
    uint32_t pn = lb, pp = lb;   // the next side's cursor; keys left on the previous side
    uint32_t nb = pn, pb = pp;   // the windows' bases
    load_next(nb);
    load_prev(pb);

    uint32_t c = 0;
    while (c < count) {
        const bool has_n = pn < n, has_p = pp > 0;
        if (!has_n && !has_p) break;
        if (has_n && pn - nb == 64) {
            nb = pn;
            load_next(nb);
        }
        if (has_p && pb - pp == 64) {
            pb = pp;
            load_prev(pb);
        }
        const uint32_t ln = (pn - nb) & 63u, lp = (pb - pp) & 63u;
        uint32_t a[DHT_W], b[DHT_W];   // the two heads (a side that is used up reads a stale lane: unused)
#pragma unroll
        for (int w = 0; w < DHT_W; ++w) {
            a[w] = nc_lane(pd[w], lp);
            b[w] = nc_lane(nd[w], ln);
        }
        bool take_p = !has_n;
        if (has_n && has_p) {   // InfoHash::xorCmp(prev, next) < 0 (keys are unique: no tie)
            bool decided = false;
#pragma unroll
            for (int w = 0; w < DHT_W; ++w) {
                if (!decided && a[w] != b[w]) {
                    take_p = a[w] < b[w];
                    decided = true;
                }
            }
        }
        uint32_t h, s = 0;
        bool acc;
        if (take_p) {
            h = nc_lane(ph, lp);
            if (STATE) s = nc_lane(ps, lp);
            acc = (pacc >> lp) & 1u;
            --pp;
        } else {
            h = nc_lane(nh, ln);
            if (STATE) s = nc_lane(ns, ln);
            acc = (nacc >> ln) & 1u;
            ++pn;
        }
        if (acc) {
            uint32_t xd[DHT_W];
#pragma unroll
            for (int w = 0; w < DHT_W; ++w) xd[w] = take_p ? a[w] : b[w];
            sink(c, xd, h, s);
            ++c;
        }
    }
    return c;
}

}  // namespace dhtgpu
