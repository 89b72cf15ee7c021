// rsearch.hip -- K10w: the resident searches' kernels for gfx950 (dhtgpu_sr_*).
//   k_sr_insert     Search::insertNode (src/search.h:636-722) + removeExpiredNode (:541-551): one
//                   wave64 per search, its insertions applied in order
//   k_sr_refill     Dht::refill (src/dht.cpp:656-677): getCachedNodes over the resident NodeCache
//                   mirror (the walk of nc_walk_dev.h), every accepted key fed straight into the
//                   insertion -- its distance is already in the window's registers
//   k_sr_open / k_sr_expire / k_sr_candidate / k_sr_status / k_sr_lists
// (update_state's byte setter is the shared one of prims.hip)
//
// A search lives in a slot.  Its node list is a row of 64 entries in six u32 planes -- the five
// words of the node's DISTANCE to the search's target (id ^ target), so that an ordering test is a
// plain five-word compare and needs no target, and the node's handle with the entry's flags in bits
// 28-29 (bit0 candidate, bit1 replied; handles are below 2^28) and srstep.hip's request state in bits
// 30-31, and a seventh plane of ticks (SearchNode::last_get_reply) -- plus the target, the length and a
// bits byte (bit0 Search::expired, bit1 overflowed, bit2 Search::done -- srmap.hip's) per slot.  Node state (bit0 isExpired(), bit1
// isRemovable(now)) is a byte array by handle; a handle at or past its extent reads as 0.
//
// k_sr_insert holds entry l of the list in lane l (dead lanes: l >= len), with the entry's state
// byte gathered once per kernel.  The slot's insertions come in 64 at a time by coalesced loads
// (lane i: insertion i's distance, handle, token, guarded state byte) and are broadcast one by one
// with v_readlane.  Per insertion x, with `live` the lanes below len:
//   backward walk   stop_l = (handle_l == x) || (x farther than entry l); the highest stopping live
//                   lane p gives found (its handle is x) or the position p + 1; no lane stops: 0
//   trims           isBad_l = state_l & 1 || candidate_l as a ballot; the list is cut to the longest
//                   prefix with at most SEARCH_NODES non-bad entries: lane l counts the non-bad
//                   entries of [0, l] (a masked population count), the lanes where that is <= 14
//                   form a prefix, and its length (a population count) is the cut
//   insertion       the entries from the position on move one lane up (ds_bpermute)
//   removeExpired   the highest set bit of the removable ballot; the entries above move one down
// No LDS array and no global access inside the per-insertion loop.  Everything is defined by the
// ballots, so the result equals the reference's sequential walk whether or not a row is sorted.
// Bytes per insertion: 20 (id) + 4 (handle) + 1 (token) + 1 (state gather) read, 1 (added) written;
// per search and call: 20 (target) + 8, and (28 + 1) x len read and 28 x len written for the row.
// Bytes per refill: the same per search, plus k_nc's lookup (20 x 64 per search round, (24 + 4 + 1)
// x 64 per window loaded, two at least) -- no per-insertion traffic at all.
#include "dhtgpu_dev.h"
#include "dhtgpu_internal.h"
#include "nc_walk_dev.h"
#include "sr_row_dev.h"   // SrRow, sr_load / sr_store / sr_trim / sr_insert (shared with srmap.hip)

namespace dhtgpu {
namespace {

__device__ __forceinline__ uint64_t uniform64(uint64_t x) {
    return ((uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)(x >> 32)) << 32) |
           __builtin_amdgcn_readfirstlane((uint32_t)x);
}

__global__ __launch_bounds__(256) void k_sr_insert(SrView v, const uint32_t* __restrict__ slots, uint32_t m,
                                                   const uint64_t* __restrict__ ins_off,
                                                   const uint32_t* __restrict__ ins_h, const uint32_t* __restrict__ ip,
                                                   uint64_t is, const uint8_t* __restrict__ tok,
                                                   uint8_t* __restrict__ added, uint32_t* __restrict__ over_any) {
    const uint32_t lane = lane_id();
    uint32_t j, slot;
    if (!sr_slot(v, slots, m, &j, &slot)) return;
    uint32_t t[DHT_W];
#pragma unroll
    for (int w = 0; w < DHT_W; ++w) t[w] = v.tp[(uint64_t)w * v.nslots + slot];
    SrRow r;
    sr_load(v, slot, lane, r);
    const uint64_t end = uniform64(ins_off[j + 1]);
    for (uint64_t c0 = uniform64(ins_off[j]); c0 < end; c0 += 64) {
        const uint32_t cn = end - c0 < 64 ? (uint32_t)(end - c0) : 64u;
        uint32_t cd[DHT_W], ch = 0, cs = 0;   // cs: the node's state byte | token << 8
#pragma unroll
        for (int w = 0; w < DHT_W; ++w) cd[w] = 0;
        if (lane < cn) {
            const uint64_t i = c0 + lane;
#pragma unroll
            for (int w = 0; w < DHT_W; ++w) cd[w] = ip[(uint64_t)w * is + i] ^ t[w];
            ch = ins_h[i] & kHandleMask;
            if (ch < v.nst) cs = v.st[ch];
            if (tok && tok[i]) cs |= 0x100u;
        }
        bool mine = false;
        for (uint32_t k = 0; k < cn; ++k) {
            uint32_t xd[DHT_W];
#pragma unroll
            for (int w = 0; w < DHT_W; ++w) xd[w] = nc_lane(cd[w], k);
            const uint32_t xs = nc_lane(cs, k);
            const bool a = sr_insert(r, lane, xd, nc_lane(ch, k), xs & 0xFFu, (xs & 0x100u) != 0, v.clock);
            if (lane == k) mine = a;
        }
        if (added && lane < cn) added[c0 + lane] = mine ? 1 : 0;
    }
    sr_store(v, slot, lane, r);
    if (over_any && r.drop && lane == 0) atomicOr(over_any, 1u);
}

__global__ __launch_bounds__(256) void k_sr_refill(SrView v, NcView nc, const uint32_t* __restrict__ slots, uint32_t m,
                                                   uint32_t count, uint32_t* __restrict__ out_inserted,
                                                   uint32_t* __restrict__ over_any) {
    const uint32_t lane = lane_id();
    uint32_t j, slot;
    if (!sr_slot(v, slots, m, &j, &slot)) return;
    uint32_t t[DHT_W];
#pragma unroll
    for (int w = 0; w < DHT_W; ++w) t[w] = v.tp[(uint64_t)w * v.nslots + slot];
    SrRow r;
    sr_load(v, slot, lane, r);
    uint32_t inserted = 0;
    nc_walk<true>(nc, v.st, v.nst, t, count, lane, [&](uint32_t, const uint32_t* xd, uint32_t h, uint32_t s) {
        inserted += sr_insert(r, lane, xd, h & kHandleMask, s, false, 0u) ? 1u : 0u;
    });
    sr_store(v, slot, lane, r);
    if (lane == 0) {
        v.rtick[slot] = v.clock;   // Search::refill_time = now
        out_inserted[j] = inserted;
        if (over_any && r.drop) atomicOr(over_any, 1u);
    }
}

// a new Search in each listed slot: target set, list empty, bits cleared
__global__ __launch_bounds__(256) void k_sr_open(SrView v, const uint32_t* __restrict__ slots,
                                                 const uint32_t* __restrict__ tp, uint64_t ts, uint32_t m) {
    const uint32_t j = blockIdx.x * 256 + threadIdx.x;
    if (j >= m) return;
    const uint32_t slot = slots[j];
    if (slot >= v.nslots) return;
#pragma unroll
    for (int w = 0; w < DHT_W; ++w) v.tp[(uint64_t)w * v.nslots + slot] = tp[(uint64_t)w * ts + j];
    v.len[slot] = 0;
    v.bits[slot] = 0;
    v.rtick[slot] = 0;
}

// Search::expire (src/search.h:560-565): expired = true, the list cleared
__global__ __launch_bounds__(256) void k_sr_expire(SrView v, const uint32_t* __restrict__ slots, uint32_t m) {
    const uint32_t j = blockIdx.x * 256 + threadIdx.x;
    if (j >= m) return;
    const uint32_t slot = slots[j];
    if (slot >= v.nslots) return;
    v.len[slot] = 0;
    v.bits[slot] |= 1u;
}

// srn->candidate = val for the entry of handles[j] in slot slots[j] (one wave per pair; absent: nothing)
__global__ __launch_bounds__(256) void k_sr_candidate(SrView v, const uint32_t* __restrict__ slots,
                                                      const uint32_t* __restrict__ handles,
                                                      const uint8_t* __restrict__ val, uint32_t m) {
    const uint32_t lane = lane_id();
    uint32_t j, slot;
    if (!sr_slot(v, slots, m, &j, &slot)) return;
    if (lane >= v.len[slot]) return;
    uint32_t* hw = v.ep + (uint64_t)DHT_W * v.es + (uint64_t)slot * 64 + lane;
    const uint32_t x = *hw;
    if ((x & kHandleMask) != handles[j]) return;
    *hw = val[j] ? x | (1u << kFlagShift) : x & ~(1u << kFlagShift);
}

// out4[j] = {len, getNumberOfBadNodes, getNumberOfConsecutiveBadNodes (src/search.h:516-530), bits}
__global__ __launch_bounds__(256) void k_sr_status(SrView v, const uint32_t* __restrict__ slots, uint32_t m,
                                                   uint32_t* __restrict__ out4) {
    const uint32_t lane = lane_id();
    uint32_t j, slot;
    if (!sr_slot(v, slots, m, &j, &slot)) return;
    SrRow r;
    sr_load(v, slot, lane, r);
    const uint64_t bad = __ballot((r.fs & kBadBits) != 0) & low_mask(r.len);
    if (lane == 0) {
        uint32_t* o = out4 + (uint64_t)j * 4;
        o[0] = r.len;
        o[1] = (uint32_t)__popcll(bad);
        o[2] = ~bad ? (uint32_t)__builtin_ctzll(~bad) : 64u;
        o[3] = (r.expired ? 1u : 0u) | (r.over ? 2u : 0u);
    }
}

// the rows, closest first (Search::getNodes order), DHT_NONE padded
__global__ __launch_bounds__(256) void k_sr_lists(SrView v, const uint32_t* __restrict__ slots, uint32_t m,
                                                  uint32_t* __restrict__ out_h, uint8_t* __restrict__ out_fl,
                                                  uint32_t* __restrict__ out_len) {
    const uint32_t lane = lane_id();
    uint32_t j, slot;
    if (!sr_slot(v, slots, m, &j, &slot)) return;
    const uint32_t len = v.len[slot];
    uint32_t h = DHT_NONE, fl = 0;
    if (lane < len) {
        const uint32_t hw = v.ep[(uint64_t)DHT_W * v.es + (uint64_t)slot * 64 + lane];
        h = hw & kHandleMask;
        fl = (hw >> kFlagShift) & 3u;
    }
    out_h[(uint64_t)j * 64 + lane] = h;
    if (out_fl) out_fl[(uint64_t)j * 64 + lane] = (uint8_t)fl;
    if (out_len && lane == 0) out_len[j] = len;
}

inline uint32_t wave_blocks(uint32_t m) { return (m + kSrWaves - 1) / kSrWaves; }

}  // namespace

hipError_t launch_sr_insert(const SrView& v, const uint32_t* slots, uint32_t m, const uint64_t* ins_off,
                            const uint32_t* ins_handle, const uint32_t* ip, uint64_t is, const uint8_t* tok,
                            uint8_t* added, uint32_t* over_any, hipStream_t s) {
    if (!m) return hipSuccess;
    k_sr_insert<<<wave_blocks(m), 64 * kSrWaves, 0, s>>>(v, slots, m, ins_off, ins_handle, ip, is, tok, added, over_any);
    return hipGetLastError();
}

hipError_t launch_sr_refill(const SrView& v, const NcView& nc, const uint32_t* slots, uint32_t m, uint32_t count,
                            uint32_t* out_inserted, uint32_t* over_any, hipStream_t s) {
    if (!m) return hipSuccess;
    k_sr_refill<<<wave_blocks(m), 64 * kSrWaves, 0, s>>>(v, nc, slots, m, count, out_inserted, over_any);
    return hipGetLastError();
}

hipError_t launch_sr_open(const SrView& v, const uint32_t* slots, const uint32_t* tp, uint64_t ts, uint32_t m,
                          hipStream_t s) {
    if (!m) return hipSuccess;
    k_sr_open<<<(m + 255) / 256, 256, 0, s>>>(v, slots, tp, ts, m);
    return hipGetLastError();
}

hipError_t launch_sr_expire(const SrView& v, const uint32_t* slots, uint32_t m, hipStream_t s) {
    if (!m) return hipSuccess;
    k_sr_expire<<<(m + 255) / 256, 256, 0, s>>>(v, slots, m);
    return hipGetLastError();
}

hipError_t launch_sr_candidate(const SrView& v, const uint32_t* slots, const uint32_t* handles, const uint8_t* val,
                               uint32_t m, hipStream_t s) {
    if (!m) return hipSuccess;
    k_sr_candidate<<<wave_blocks(m), 64 * kSrWaves, 0, s>>>(v, slots, handles, val, m);
    return hipGetLastError();
}

hipError_t launch_sr_status(const SrView& v, const uint32_t* slots, uint32_t m, uint32_t* out4, hipStream_t s) {
    if (!m) return hipSuccess;
    k_sr_status<<<wave_blocks(m), 64 * kSrWaves, 0, s>>>(v, slots, m, out4);
    return hipGetLastError();
}

hipError_t launch_sr_lists(const SrView& v, const uint32_t* slots, uint32_t m, uint32_t* out_handle, uint8_t* out_flags,
                           uint32_t* out_len, hipStream_t s) {
    if (!m) return hipSuccess;
    k_sr_lists<<<wave_blocks(m), 64 * kSrWaves, 0, s>>>(v, slots, m, out_handle, out_flags, out_len);
    return hipGetLastError();
}

}  // namespace dhtgpu
