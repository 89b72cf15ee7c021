// srstep.hip -- K10s: Dht::searchStep (src/dht.cpp:562-654) for find_node searches over the resident
// rows, for gfx950 (dhtgpu_srs_*).
//   k_srs_step      one wave64 per search, the row of sr_row_dev.h in registers (lane l = entry l)
//   k_srs_request   the request state of one entry (what the engine's callbacks change)
//   k_srs_entries   the rows' req and tick, for a caller that wants to look
//
// A find_node search has no callbacks, announces or listeners, so SearchNode::getStatus holds at
// most the one ANY_QUERY request.  Its state is `req` (0 none -- erased, expired-and-over and
// cancelled alike --, 1 pending, 2 completed) in bits 30-31 of the entry's handle word, and
// last_get_reply is the entry's `tick` in the caller's clock (0: time_point::min()).  Per search, with
// now = the context's clock, E = node_expire, every tick sum in 64 bits, `live` the lanes below len,
// bad_l = candidate_l || state_l & 1 and good = live & ~bad as ballots:
//   on entry        expired || done: nothing changes, `skipped`
//   refill          refill_tick + E < now and popcount(good) < SEARCH_NODES: k_sr_refill's walk, every
//                   accepted key through sr_insert; refill_tick = now
//   isSynced        (src/search.h:734-747) ok_l = replied_l && tick_l != 0 && tick_l + E >= now; lane l
//                   is one of the first TARGET_NODES = 8 good entries when it is good and fewer than 8
//                   good lanes lie below it (a masked population count); synced = good != 0 and no such
//                   lane fails ok.  Then setDone(): done = 1, every req = 0, nothing sent
//   sends           sol = popcount(good & req == 1); canGet_l (src/search.h:139-161, one query) =
//                   !expired_l && (req_l == 0 || (req_l == 2 && (tick_l == 0 || now > tick_l + E))).
//                   searchSendGetValues takes the first canGet entry until sol reaches
//                   MAX_REQUESTED_SEARCH_NODES = 4, counting good entries only: lane l is taken when
//                   canGet_l and fewer than 4 - sol good canGet lanes lie below it.  The taken lanes get
//                   req = 1; lane i of the output row fetches the handle of the i-th taken lane (a
//                   select over the ballot, then one cross-lane read)
//   expiry          leading bad entries (count of trailing ones of the bad ballot) >= min(len, 25):
//                   Search::expire() -- expired = 1, the list cleared, done = 1
// Ballots and cross-lane reads only: no LDS array, and between the row's load and its store no global
// access but the refill's walk of the NodeCache mirror.
#include "dhtgpu_dev.h"
#include "dhtgpu_internal.h"
#include "nc_walk_dev.h"
#include "sr_row_dev.h"

namespace dhtgpu {
namespace {

constexpr uint32_t kTargetNodes = 8;        // TARGET_NODES, src/dht.h
constexpr uint32_t kMaxRequested = 4;       // MAX_REQUESTED_SEARCH_NODES
constexpr uint32_t kSearchMaxBad = 25;      // SEARCH_MAX_BAD_NODES

// the position of the i-th set bit of x (i < popcount(x))
__device__ __forceinline__ uint32_t select_bit(uint64_t x, uint32_t i) {
    uint32_t pos = 0;
#pragma unroll
    for (uint32_t s = 32; s; s >>= 1) {
        const uint32_t c = (uint32_t)__popcll((x >> pos) & low_mask(s));
        if (i >= c) {
            i -= c;
            pos += s;
        }
    }
    return pos;
}

__global__ __launch_bounds__(256) void k_srs_step(SrView v, NcView nc, const uint32_t* __restrict__ slots, uint32_t m,
                                                  uint32_t node_expire, uint32_t refill_count,
                                                  uint32_t* __restrict__ out_send, uint32_t* __restrict__ out4,
                                                  uint32_t* __restrict__ over_any) {
    const uint32_t lane = lane_id();
    uint32_t j, slot;
    if (!sr_slot(v, slots, m, &j, &slot)) return;
    SrRow r;
    sr_load(v, slot, lane, r);
    const uint64_t now = v.clock, E = node_expire;
    uint32_t nsend = 0, sol = 0, inserted = 0, bits = 0, send = DHT_NONE;
    if (r.expired || r.done) {
        bits = 32u;
    } else {
        if (refill_count) {
            const uint64_t rt = __builtin_amdgcn_readfirstlane(v.rtick[slot]);
            const uint32_t ngood = (uint32_t)__popcll(~__ballot((r.fs & kBadBits) != 0) & low_mask(r.len));
            if (rt + E < now && ngood < kSearchNodes) {
                uint32_t t[DHT_W];
#pragma unroll
                for (int w = 0; w < DHT_W; ++w) t[w] = v.tp[(uint64_t)w * v.nslots + slot];
                nc_walk<true>(nc, v.st, v.nst, t, refill_count, lane, [&](uint32_t, const uint32_t* xd, uint32_t h, uint32_t s) {
                    inserted += sr_insert(r, lane, xd, h & kHandleMask, s, false, 0u) ? 1u : 0u;
                });
                if (lane == 0) v.rtick[slot] = v.clock;
                bits |= 8u;
            }
        }
        const uint64_t live = low_mask(r.len);
        const uint64_t bad = __ballot((r.fs & kBadBits) != 0) & live, good = ~bad & live;
        const bool is_good = (good >> lane) & 1ull;
        const uint32_t below = (uint32_t)__popcll(good & low_mask(lane));   // good entries before this one
        const uint64_t tick_end = (uint64_t)r.tick + E;
        const bool ok = (r.fs & 2u) && r.tick != 0 && tick_end >= now;
        const uint64_t first = __ballot(is_good && below < kTargetNodes);
        if (good && !(first & ~__ballot(ok))) {   // Search::isSynced: setDone()
            r.done = true;
            r.fs &= ~kReqMask;
            bits |= 16u;
        } else {
            const uint32_t req = (r.fs & kReqMask) >> kReqShift;
            sol = (uint32_t)__popcll(__ballot(req == 1u) & good);
            const bool can = lane < r.len && !(r.fs & 0x100u) && (req == 0u || (req == 2u && (r.tick == 0 || now > tick_end)));
            if (sol < kMaxRequested) {
                const uint64_t cang = __ballot(can && is_good);
                const bool take = can && (uint32_t)__popcll(cang & low_mask(lane)) < kMaxRequested - sol;
                const uint64_t taken = __ballot(take);
                nsend = (uint32_t)__popcll(taken);
                sol += (uint32_t)__popcll(taken & good);
                if (take) r.fs = (r.fs & ~kReqMask) | (1u << kReqShift);
                const uint32_t h = (uint32_t)__shfl((int)r.h, (int)(lane < nsend ? select_bit(taken, lane) : 0u));
                if (lane < nsend) send = h;
            }
        }
        const uint32_t lead = ~bad ? (uint32_t)__builtin_ctzll(~bad) : 64u;   // bad has no bit at or past len
        if (lead >= (r.len < kSearchMaxBad ? r.len : kSearchMaxBad)) {   // Search::expire()
            r.expired = true;
            r.done = true;
            r.len = 0;
            sol = 0;
        }
        sr_store(v, slot, lane, r);
    }
    out_send[(uint64_t)j * 64 + lane] = send;
    if (lane == 0) {
        uint32_t* o = out4 + (uint64_t)j * 4;
        o[0] = nsend;
        o[1] = sol;
        o[2] = inserted;
        o[3] = bits | (r.expired ? 1u : 0u) | (r.over ? 2u : 0u) | (r.done ? 4u : 0u);
        if (over_any && r.drop) atomicOr(over_any, 1u);
    }
}

__global__ __launch_bounds__(256) void k_srs_request(SrView v, const uint32_t* __restrict__ slots,
                                                     const uint32_t* __restrict__ handles,
                                                     const uint8_t* __restrict__ val, uint32_t m) {
    const uint32_t lane = lane_id();
    uint32_t j, slot;
    if (!sr_slot(v, slots, m, &j, &slot)) return;
    if (lane >= v.len[slot]) return;
    uint32_t* hw = v.ep + (uint64_t)DHT_W * v.es + (uint64_t)slot * 64 + lane;
    const uint32_t x = *hw;
    if ((x & kHandleMask) != handles[j]) return;
    *hw = (x & ~(3u << 30)) | ((uint32_t)(val[j] & 3u) << 30);
}

__global__ __launch_bounds__(256) void k_srs_entries(SrView v, const uint32_t* __restrict__ slots, uint32_t m,
                                                     uint8_t* __restrict__ out_req, uint32_t* __restrict__ out_tick) {
    const uint32_t lane = lane_id();
    uint32_t j, slot;
    if (!sr_slot(v, slots, m, &j, &slot)) return;
    uint32_t req = 0, tick = 0;
    if (lane < v.len[slot]) {
        const uint64_t e = (uint64_t)slot * 64 + lane;
        req = v.ep[(uint64_t)DHT_W * v.es + e] >> 30;
        tick = v.tk[e];
    }
    if (out_req) out_req[(uint64_t)j * 64 + lane] = (uint8_t)req;
    if (out_tick) out_tick[(uint64_t)j * 64 + lane] = tick;
}

inline uint32_t wave_blocks(uint32_t m) { return (m + kSrWaves - 1) / kSrWaves; }

}  // namespace

hipError_t launch_srs_step(const SrView& v, const NcView& nc, const uint32_t* slots, uint32_t m, uint32_t node_expire,
                           uint32_t refill_count, uint32_t* out_send, uint32_t* out4, uint32_t* over_any,
                           hipStream_t s) {
    if (!m) return hipSuccess;
    k_srs_step<<<wave_blocks(m), 64 * kSrWaves, 0, s>>>(v, nc, slots, m, node_expire, refill_count, out_send, out4, over_any);
    return hipGetLastError();
}

hipError_t launch_srs_request(const SrView& v, const uint32_t* slots, const uint32_t* handles, const uint8_t* val,
                              uint32_t m, hipStream_t s) {
    if (!m) return hipSuccess;
    k_srs_request<<<wave_blocks(m), 64 * kSrWaves, 0, s>>>(v, slots, handles, val, m);
    return hipGetLastError();
}

hipError_t launch_srs_entries(const SrView& v, const uint32_t* slots, uint32_t m, uint8_t* out_req, uint32_t* out_tick,
                              hipStream_t s) {
    if (!m) return hipSuccess;
    k_srs_entries<<<wave_blocks(m), 64 * kSrWaves, 0, s>>>(v, slots, m, out_req, out_tick);
    return hipGetLastError();
}

}  // namespace dhtgpu
