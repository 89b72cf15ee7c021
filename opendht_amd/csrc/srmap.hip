// srmap.hip -- K10m: Dht::trySearchInsert (src/dht.cpp:118-150) over the resident searches for gfx950
// (dhtgpu_srm_*).  The searches of a family are a std::map by target; a learned node is offered to
// the searches from lower_bound(id) on, forward and then backward, Search::insertNode on each until
// one refuses that is neither expired nor done.  Here the map is the mapped slots in target order
// with the sorted target planes (SrmView), and a batch of nodes is applied in batch order, exactly.
//   k_srm_gather / k_srm_order / k_srm_done   the map's build and the done bit (bit 2 of a slot's bits)
//   k_srm_filter   one wave64 per node, parallel: the node's lower bound (the 64-ary ballot search of
//                  nc_walk_dev.h over the target planes, five-word compare) and whether its first
//                  search in each direction is a WALL -- a search that is not expired, not done,
//                  holds >= SEARCH_NODES non-bad entries none of which is a non-bad removable one,
//                  does not list the node's handle, and whose threshold (entry cut - 1, cut =
//                  sr_trim's) is closer to its target than the node.  insertNode on a wall refuses
//                  and only cuts the list to `cut`; inside one call a wall stays a wall and its
//                  threshold only moves closer, so a node between two walls is inserted nowhere
//                  whenever its turn comes: its whole effect is out_cnt = 0 and those two cuts.  The
//                  kernel changes nothing: it records the node's flag and its two {slot, cut}, and
//                  raises the chunk's hazard word when a node is removable and not expired (such a
//                  node can take a non-bad entry's place and reopen a search).
//   k_srm_walk     one workgroup of 8 waves, the nodes the filter left, one after the other in batch
//                  order (all of them when the hazard word is set, and then no cut is applied).  Per
//                  node, waves 0-3 take consecutive searches forward and waves 4-7 backward -- 1, 2,
//                  then 4 per direction and round -- each loads its row, runs sr_insert in registers
//                  and posts {valid, added, passes} to LDS; after a barrier every wave reads the
//                  posts of its direction, the waves up to and including the first that does not pass
//                  store their rows (a refusal still trims), the later ones discard, and a direction
//                  goes on while all of its waves passed.  A second barrier ends the round: it orders
//                  the stored rows before any later load of them by another wave of the workgroup
//                  (one CU, one L1: a workgroup barrier with its fence is enough) and frees the posts.
// No scratch, no wait on another workgroup, every loop bounded by ns.
#include "dhtgpu_dev.h"
#include "dhtgpu_internal.h"
#include "nc_walk_dev.h"
#include "prims_dev.h"
#include "sr_row_dev.h"

namespace dhtgpu {
namespace {

constexpr uint32_t kFilterWaves = 4;   // nodes per 256-thread workgroup of the filter
constexpr uint32_t kDirWaves = 4;      // waves per direction of the walk
constexpr int kWalkThreads = 2 * kDirWaves * 64;

__global__ __launch_bounds__(256) void k_srm_gather(SrView v, const uint32_t* __restrict__ slots, uint32_t ns,
                                                    uint32_t* __restrict__ planes, uint64_t stride) {
    const uint32_t j = blockIdx.x * 256 + threadIdx.x;
    if (j >= ns) return;
    const uint32_t slot = slots[j];
#pragma unroll
    for (int w = 0; w < DHT_W; ++w) planes[(uint64_t)w * stride + j] = slot < v.nslots ? v.tp[(uint64_t)w * v.nslots + slot] : 0u;
}

__global__ __launch_bounds__(256) void k_srm_order(const uint32_t* __restrict__ slots, const uint32_t* __restrict__ perm,
                                                   uint32_t ns, uint32_t* __restrict__ order) {
    const uint32_t j = blockIdx.x * 256 + threadIdx.x;
    if (j >= ns) return;
    const uint32_t p = perm[j];
    order[j] = p < ns ? slots[p] : DHT_NONE;
}

__global__ __launch_bounds__(256) void k_srm_done(SrView v, const uint32_t* __restrict__ slots,
                                                  const uint8_t* __restrict__ val, uint32_t m) {
    const uint32_t j = blockIdx.x * 256 + threadIdx.x;
    if (j >= m) return;
    const uint32_t slot = slots[j];
    if (slot >= v.nslots) return;
    const uint8_t b = v.bits[slot];
    v.bits[slot] = val[j] ? (uint8_t)(b | 4u) : (uint8_t)(b & ~4u);
}

// Is the search in `slot` a wall for node x = {id xi, handle xh}?  *cut = its list's cut when it is.
__device__ __forceinline__ bool srm_wall(const SrView& v, uint32_t slot, uint32_t lane, const uint32_t (&xi)[DHT_W],
                                         uint32_t xh, uint32_t* cut) {
    SrRow r;
    sr_load(v, slot, lane, r);
    if (r.expired || r.done) return false;
    const uint64_t live = low_mask(r.len);
    const uint64_t good = ~__ballot((r.fs & kBadBits) != 0) & live;
    if ((uint32_t)__popcll(good) < kSearchNodes) return false;
    if (__ballot((r.fs & kRemovable) != 0) & good) return false;   // its removal could reopen the search
    if (__ballot(r.h == xh) & live) return false;
    bool far = false, decided = false;   // x farther than this lane's entry
#pragma unroll
    for (int w = 0; w < DHT_W; ++w) {
        const uint32_t xd = xi[w] ^ v.tp[(uint64_t)w * v.nslots + slot];
        if (!decided && xd != r.d[w]) {
            far = xd > r.d[w];
            decided = true;
        }
    }
    const uint32_t c = sr_trim(r, lane);   // >= SEARCH_NODES
    *cut = c;
    return (__ballot(far) >> (c - 1)) & 1ull;
}

__global__ __launch_bounds__(256) void k_srm_filter(SrView v, SrmView mp, SrmWork wk, const uint32_t* __restrict__ handles,
                                                    const uint32_t* __restrict__ ip, uint64_t is, uint32_t m) {
    const uint32_t lane = lane_id();
    const uint32_t j = __builtin_amdgcn_readfirstlane(blockIdx.x * kFilterWaves + (threadIdx.x >> 6));
    if (j >= m) return;
    uint32_t xi[DHT_W];
#pragma unroll
    for (int w = 0; w < DHT_W; ++w) xi[w] = __builtin_amdgcn_readfirstlane(ip[(uint64_t)w * is + j]);
    const uint32_t xh = __builtin_amdgcn_readfirstlane(handles[j]) & kHandleMask;
    const uint32_t xs = xh < v.nst ? (uint32_t)v.st[xh] : 0u;
    const NcView keys{mp.ns, mp.tp, mp.ts, nullptr, nullptr};
    const uint32_t c = nc_lower_bound(keys, xi, lane);
    uint32_t tr[4] = {DHT_NONE, 0u, DHT_NONE, 0u};
    bool wall_f = true, wall_b = true;   // a direction with no search is a wall
    if (c < mp.ns) {
        const uint32_t slot = __builtin_amdgcn_readfirstlane(mp.order[c]);
        wall_f = slot < v.nslots && srm_wall(v, slot, lane, xi, xh, &tr[1]);
        tr[0] = slot;
    }
    if (c > 0) {
        const uint32_t slot = __builtin_amdgcn_readfirstlane(mp.order[c - 1]);
        wall_b = slot < v.nslots && srm_wall(v, slot, lane, xi, xh, &tr[3]);
        tr[2] = slot;
    }
    if (lane == 0) {
        wk.pos[j] = c;
        wk.flag[j] = wall_f && wall_b ? 0u : 1u;
#pragma unroll
        for (int i = 0; i < 4; ++i) wk.trim[(uint64_t)j * 4 + i] = tr[i];
        if ((xs & 3u) == 2u) atomicOr(wk.hazard, 1u);
    }
}

__global__ __launch_bounds__(kWalkThreads) void k_srm_walk(SrView v, SrmView mp, SrmWork wk,
                                                           const uint32_t* __restrict__ handles,
                                                           const uint32_t* __restrict__ ip, uint64_t is, uint32_t m,
                                                           uint32_t* out_cnt, uint32_t* out_touched, uint32_t* stats) {
    __shared__ uint32_t post[2][kDirWaves];
    __shared__ uint32_t wsum[kWalkThreads / 64 + 1];
    const uint32_t lane = lane_id(), wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t dir = wave / kDirWaves, k = wave % kDirWaves;   // 0 forward, 1 backward; place in the round
    const bool hazard = *wk.hazard != 0;

    // the nodes to walk, in batch order; the filtered nodes' whole effect
    uint32_t nact = m;
    if (!hazard) {
        nact = block_scan_array<kWalkThreads>(wk.flag, wk.offs, m, wsum);
        for (uint32_t i = threadIdx.x; i < m; i += kWalkThreads) {
            if (wk.flag[i]) {
                wk.list[wk.offs[i]] = i;
                continue;
            }
            out_cnt[i] = 0;
            for (int d = 0; d < 2; ++d) {   // nodes.resize(cut) on the two walls (the same cut from every node)
                const uint32_t slot = wk.trim[(uint64_t)i * 4 + 2 * d], cut = wk.trim[(uint64_t)i * 4 + 2 * d + 1];
                if (slot < v.nslots && v.len[slot] > cut) v.len[slot] = cut;
            }
        }
    }
    __syncthreads();

    uint32_t hops = 0;
    for (uint32_t a = 0; a < nact; ++a) {
        const uint32_t j = hazard ? a : wk.list[a];
        uint32_t xi[DHT_W];
#pragma unroll
        for (int w = 0; w < DHT_W; ++w) xi[w] = __builtin_amdgcn_readfirstlane(ip[(uint64_t)w * is + j]);
        const uint32_t xh = __builtin_amdgcn_readfirstlane(handles[j]) & kHandleMask;
        const uint32_t xs = __builtin_amdgcn_readfirstlane(xh < v.nst ? (uint32_t)v.st[xh] : 0u);
        const uint32_t c = __builtin_amdgcn_readfirstlane(wk.pos[j]);
        uint32_t fpos = c, bpos = c;        // the next forward search; the backward searches left
        bool go_f = fpos < mp.ns, go_b = bpos > 0;
        uint32_t width = 1, cnt = 0;
        while (go_f || go_b) {              // a round moves every live direction on: at most ns rounds
            const uint32_t avail = dir ? bpos : mp.ns - fpos;
            const bool valid = (dir ? go_b : go_f) && k < width && k < avail;
            SrRow r;
            uint32_t slot = DHT_NONE, code = 0;   // code: bit0 valid, bit1 added, bit2 passes
            if (valid) {
                slot = __builtin_amdgcn_readfirstlane(mp.order[dir ? bpos - 1 - k : fpos + k]);
                if (slot < v.nslots) {
                    uint32_t xd[DHT_W];
#pragma unroll
                    for (int w = 0; w < DHT_W; ++w) xd[w] = xi[w] ^ v.tp[(uint64_t)w * v.nslots + slot];
                    sr_load(v, slot, lane, r);
                    const bool added = sr_insert(r, lane, xd, xh, xs, false, 0u);
                    code = 1u | (added ? 2u : 0u) | (added || r.expired || r.done ? 4u : 0u);
                }
            }
            if (lane == 0) post[dir][k] = code;
            __syncthreads();
            uint32_t commit[2] = {0, 0};    // the waves of each direction whose rows stand
#pragma unroll
            for (int d = 0; d < 2; ++d) {
                if (!(d ? go_b : go_f)) continue;
                bool cont = true;
                for (uint32_t kk = 0; kk < width && cont; ++kk) {
                    const uint32_t pc = post[d][kk];
                    if (!(pc & 1u)) {
                        cont = false;
                    } else {
                        ++commit[d];
                        cnt += (pc >> 1) & 1u;
                        cont = (pc & 4u) != 0;
                    }
                }
                if (d) {
                    bpos -= bpos < width ? bpos : width;
                    go_b = cont && bpos > 0;
                } else {
                    fpos += width;
                    go_f = cont && fpos < mp.ns;
                }
            }
            hops += commit[0] + commit[1];
            if (code & 1u && k < commit[dir]) {
                sr_store(v, slot, lane, r);
                if (lane == 0) {
                    if (code & 2u && out_touched) atomicOr(out_touched + (slot >> 5), 1u << (slot & 31u));
                    if (r.drop) atomicOr(stats + 3, 1u);
                }
            }
            width = width < kDirWaves ? width * 2 : kDirWaves;
            __syncthreads();
        }
        if (threadIdx.x == 0) out_cnt[j] = cnt;
    }
    if (threadIdx.x == 0) {
        atomicAdd(stats + 0, m - nact);
        atomicAdd(stats + 1, hops);
        if (hazard) atomicOr(stats + 2, 1u);
    }
}

}  // namespace

hipError_t launch_srm_gather(const SrView& v, const uint32_t* slots, uint32_t ns, uint32_t* planes, uint64_t stride,
                             hipStream_t s) {
    if (!ns) return hipSuccess;
    k_srm_gather<<<(ns + 255) / 256, 256, 0, s>>>(v, slots, ns, planes, stride);
    return hipGetLastError();
}

hipError_t launch_srm_order(const uint32_t* slots, const uint32_t* perm, uint32_t ns, uint32_t* order, hipStream_t s) {
    if (!ns) return hipSuccess;
    k_srm_order<<<(ns + 255) / 256, 256, 0, s>>>(slots, perm, ns, order);
    return hipGetLastError();
}

hipError_t launch_srm_done(const SrView& v, const uint32_t* slots, const uint8_t* val, uint32_t m, hipStream_t s) {
    if (!m) return hipSuccess;
    k_srm_done<<<(m + 255) / 256, 256, 0, s>>>(v, slots, val, m);
    return hipGetLastError();
}

hipError_t launch_srm_offer(const SrView& v, const SrmView& mp, const SrmWork& wk, const uint32_t* handles,
                            const uint32_t* ip, uint64_t is, uint32_t m, uint32_t* out_cnt, uint32_t* out_touched,
                            uint32_t* stats, hipStream_t s) {
    if (!m) return hipSuccess;
    if (m > kSrmChunk) return hipErrorInvalidValue;
    if (hipError_t e = hipMemsetAsync(wk.hazard, 0, 4, s)) return e;
    k_srm_filter<<<(m + kFilterWaves - 1) / kFilterWaves, 64 * kFilterWaves, 0, s>>>(v, mp, wk, handles, ip, is, m);
    k_srm_walk<<<1, kWalkThreads, 0, s>>>(v, mp, wk, handles, ip, is, m, out_cnt, out_touched, stats);
    return hipGetLastError();
}

}  // namespace dhtgpu
