// sr_row_dev.h -- one resident search's node list held across a wave64 (lane l = entry l), and
// Search::insertNode (src/search.h:636-722) + removeExpiredNode (:541-551) on it in registers.
// Shared by rsearch.hip (k_sr_insert, k_sr_refill, k_sr_status: one wave per search, its insertions
// in order), srmap.hip (Dht::trySearchInsert: one node offered to the searches around its id) and
// srstep.hip (Dht::searchStep).  An entry's req and tick travel with it through every move.
// The method -- the backward walk, the trims and the removal as ballots -- is described at the top
// of rsearch.hip.
#pragma once
#include "dhtgpu_dev.h"
#include "dhtgpu_internal.h"
#include "nc_walk_dev.h"

namespace dhtgpu {

constexpr uint32_t kSearchNodes = 14;    // SEARCH_NODES, src/dht.h:308
constexpr uint32_t kHandleMask = (1u << 28) - 1u;   // DHTGPU_NC_MAX_HANDLE - 1
constexpr uint32_t kFlagShift = 28;

__device__ __forceinline__ uint64_t low_mask(uint32_t n) { return n >= 64 ? ~0ull : (1ull << n) - 1ull; }

// One search's list across the wave: lane l holds entry l.  len, expired, over, done and drop are
// wave-uniform.
struct SrRow {
    uint32_t d[DHT_W];   // distance to the target
    uint32_t h;          // handle
    uint32_t fs;         // bits 0-1: flags (candidate, replied); bits 2-3: req, the request state of
                         // getStatus[ANY_QUERY] (0 none, 1 pending, 2 completed); bits 8-9: the node's state byte
    uint32_t tick;       // SearchNode::last_get_reply in the caller's clock ticks (0: time_point::min())
    uint32_t len;
    bool expired, over;
    bool done;           // Search::done (dhtgpu_srm_set_done): carried through, read by the map's walk only
    bool drop;           // an insertion was dropped in this kernel (over is the slot's sticky bit)
};

constexpr uint32_t kBadBits = 0x101u;    // SearchNode::isBad: candidate || node->isExpired()
constexpr uint32_t kRemovable = 0x200u;
constexpr uint32_t kReqShift = 2, kReqMask = 3u << kReqShift;   // req within SrRow::fs
constexpr uint32_t kSrWaves = 4;         // searches per 256-thread workgroup

// wave j of the call -> its slot (wave-uniform); false: past the list or not a slot
__device__ __forceinline__ bool sr_slot(const SrView& v, const uint32_t* __restrict__ slots, uint32_t m, uint32_t* j,
                                        uint32_t* slot) {
    *j = __builtin_amdgcn_readfirstlane(blockIdx.x * kSrWaves + (threadIdx.x >> 6));
    if (*j >= m) return false;
    *slot = __builtin_amdgcn_readfirstlane(slots[*j]);
    return *slot < v.nslots;
}

__device__ __forceinline__ void sr_load(const SrView& v, uint32_t slot, uint32_t lane, SrRow& r) {
    r.len = __builtin_amdgcn_readfirstlane(v.len[slot]);
    const uint32_t bits = __builtin_amdgcn_readfirstlane((uint32_t)v.bits[slot]);
    r.expired = bits & 1u;
    r.over = bits & 2u;
    r.done = bits & 4u;
    r.drop = false;
#pragma unroll
    for (int w = 0; w < DHT_W; ++w) r.d[w] = 0;
    r.h = 0;
    r.fs = 0;
    r.tick = 0;
    if (lane < r.len) {
        const uint64_t e = (uint64_t)slot * 64 + lane;
#pragma unroll
        for (int w = 0; w < DHT_W; ++w) r.d[w] = v.ep[(uint64_t)w * v.es + e];
        const uint32_t hw = v.ep[(uint64_t)DHT_W * v.es + e];
        r.h = hw & kHandleMask;
        r.fs = hw >> kFlagShift;   // flags and req
        r.tick = v.tk[e];
        if (r.h < v.nst) r.fs |= (uint32_t)v.st[r.h] << 8;
    }
}

__device__ __forceinline__ void sr_store(const SrView& v, uint32_t slot, uint32_t lane, const SrRow& r) {
    if (lane < r.len) {
        const uint64_t e = (uint64_t)slot * 64 + lane;
#pragma unroll
        for (int w = 0; w < DHT_W; ++w) v.ep[(uint64_t)w * v.es + e] = r.d[w];
        v.ep[(uint64_t)DHT_W * v.es + e] = r.h | ((r.fs & 0xFu) << kFlagShift);
        v.tk[e] = r.tick;
    }
    if (lane == 0) {
        v.len[slot] = r.len;
        v.bits[slot] = (uint8_t)((r.expired ? 1u : 0u) | (r.over ? 2u : 0u) | (r.done ? 4u : 0u));
    }
}

// the list cut to its longest prefix with at most SEARCH_NODES non-bad entries: the new length
__device__ __forceinline__ uint32_t sr_trim(const SrRow& r, uint32_t lane) {
    const uint64_t good = ~__ballot((r.fs & kBadBits) != 0) & low_mask(r.len);
    const uint32_t upto = (uint32_t)__popcll(good & low_mask(lane + 1));   // non-bad entries of [0, lane]
    const uint32_t cut = (uint32_t)__popcll(__ballot(upto <= kSearchNodes));
    return cut < r.len ? cut : r.len;
}

// Search::insertNode(x) with x = {distance xd, handle xh, state byte xs, replied with a token xt}
// (all wave-uniform), then removeExpiredNode when x became a search node.  A new entry has req 0 and
// tick 0; a token sets the entry's tick to `now` (the context's clock).  Returns insertNode's result.
__device__ __forceinline__ bool sr_insert(SrRow& r, uint32_t lane, const uint32_t* xd, uint32_t xh, uint32_t xs, bool xt,
                                          uint32_t now) {
    bool far = false, decided = false;   // x farther than this lane's entry (xorCmp > 0)
#pragma unroll
    for (int w = 0; w < DHT_W; ++w) {
        if (!decided && xd[w] != r.d[w]) {
            far = xd[w] > r.d[w];
            decided = true;
        }
    }
    const uint64_t live = low_mask(r.len);
    const uint64_t same = __ballot(r.h == xh) & live;
    const uint64_t stop = (__ballot(far) & live) | same;
    bool found = false;
    uint32_t n = 0;
    if (stop) {
        const uint32_t p = 63u - (uint32_t)__clzll((long long)stop);
        found = (same >> p) & 1ull;
        n = found ? p : p + 1;
    }
    bool added = false, ok = true;
    if (!found) {
        bool full = false;
        uint32_t tcut = r.len;
        if (r.expired) {
            if (r.len >= kSearchNodes) {
                full = true;
                tcut = kSearchNodes;
            }
        } else {
            const uint64_t good = ~__ballot((r.fs & kBadBits) != 0) & live;
            full = (uint32_t)__popcll(good) >= kSearchNodes;
            tcut = sr_trim(r, lane);
        }
        if (full) {
            r.len = tcut;
            if (n >= tcut) ok = false;   // farther than every kept node: not inserted
        }
        if (ok && r.len >= 64) {         // the row cannot hold the list: flagged, the insertion dropped
            r.over = r.drop = true;
            ok = false;
        }
        if (ok) {
            const uint32_t nfs = (xs & 3u) << 8;
#pragma unroll
            for (int w = 0; w < DHT_W; ++w) {
                const uint32_t u = (uint32_t)__shfl_up((int)r.d[w], 1);
                r.d[w] = lane > n ? u : (lane == n ? xd[w] : r.d[w]);
            }
            const uint32_t uh = (uint32_t)__shfl_up((int)r.h, 1), uf = (uint32_t)__shfl_up((int)r.fs, 1);
            const uint32_t ut = (uint32_t)__shfl_up((int)r.tick, 1);
            r.h = lane > n ? uh : (lane == n ? xh : r.h);
            r.fs = lane > n ? uf : (lane == n ? nfs : r.fs);
            r.tick = lane > n ? ut : (lane == n ? 0u : r.tick);
            ++r.len;
            added = true;
            if (xs & 1u) {               // a bad node: an expired search keeps SEARCH_NODES entries
                if (r.expired) r.len = r.len < kSearchNodes ? r.len : kSearchNodes;
                else r.len = sr_trim(r, lane);
            } else if (r.expired) {      // the reference counts every other entry bad here: no trim
                r.expired = false;
            } else {
                r.len = sr_trim(r, lane);
            }
        }
    }
    if (ok && xt && n < r.len && nc_lane(r.h, n & 63u) == xh) {   // a reply with a token
        if (lane == n) {
            r.fs = (r.fs & ~1u) | 2u;
            r.tick = now;
        }
        r.expired = false;
    }
    if (added) {   // Search::removeExpiredNode: the last removable node
        const uint64_t rm = __ballot((r.fs & kRemovable) != 0) & low_mask(r.len);
        if (rm) {
            const uint32_t e = 63u - (uint32_t)__clzll((long long)rm);
#pragma unroll
            for (int w = 0; w < DHT_W; ++w) {
                const uint32_t u = (uint32_t)__shfl_down((int)r.d[w], 1);
                if (lane >= e) r.d[w] = u;
            }
            const uint32_t uh = (uint32_t)__shfl_down((int)r.h, 1), uf = (uint32_t)__shfl_down((int)r.fs, 1);
            const uint32_t ut = (uint32_t)__shfl_down((int)r.tick, 1);
            if (lane >= e) {
                r.h = uh;
                r.fs = uf;
                r.tick = ut;
            }
            --r.len;
        }
    }
    return added;
}

}  // namespace dhtgpu
