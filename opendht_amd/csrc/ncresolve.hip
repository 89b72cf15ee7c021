// ncresolve.hip -- K8r: keys to handles over the resident NodeCache mirror for gfx950 (dhtgpu_ncr_*).
//   k_ncr_find<G>   NodeMap::find (NodeCache::NodeMap::getNode(id), src/node_cache.cpp:87-97, without
//                   its erase): m keys against the n sorted resident keys, G lanes per key
//   k_ncr_order     a get_nodes batch: the number of new keys before each batch position, in batch
//                   order (first pass: the 256-key blocks' counts; second pass: the positions)
//   k_ncr_assign    a get_nodes batch: the handle of every sorted batch key -- a free handle for a
//                   new key, the resident handle, or the handle of the key's first appearance
//   k_ncr_extract   an extract batch: the handle every erased key held
// The mutations themselves are ncache.hip's (k_nc_rank / k_nc_compact / k_nc_merge), unchanged:
// get_nodes is NodeMap::getNode(id, addr, ...)'s emplace (src/node_cache.cpp:99-111) with the
// handles drawn here, extract is map.erase(key) that reports what it freed.
//
// Find.  The tree has the two ends of a range: k_nc's wave-per-key 64-ary search (ceil(log64 n)
// rounds of 64 loads) and k_nc_rank's thread-per-key bisection (ceil(log2 n) dependent probes).
// k_ncr_find<G> is the lane-group form between them: G lanes share a key, each round they load G
// evenly spaced pivots of the open range and the group's part of the wave's ballot picks one of the
// G + 1 sub-ranges -- ceil(log_{G+1} n) rounds; a range of at most G keys is settled by one round
// over the keys themselves.  A lane compares word 0 first and loads words 1..4 of its pivot only
// when word 0 ties (on random keys: the last rounds; on clustered keys: every round), so a round
// costs 4 B per lane, not 20.  The key index is uniform per group; the group's first lane then
// loads the key at the bound (equality over all 160 bits) with its handle and, if asked, gathers
// the handle's accept word (guarded by the mask's extent) and writes the answers.  No LDS.
// Bytes per key: 20 (key) + rounds x G x 4..20 + 24 (+ 4); rounds at n = 2^20: 7 / 5 / 4 for G =
// 8 / 16 / 64, against 20 probes of the bisection.
#include <algorithm>

#include "dhtgpu_dev.h"
#include "dhtgpu_internal.h"

namespace dhtgpu {
namespace {

// lexicographic key[p] < t, word 0 first: words 1..4 are loaded only on a word-0 tie
__device__ __forceinline__ bool ncr_key_lt(const uint32_t* __restrict__ kp, uint64_t ks, uint64_t p,
                                           const uint32_t (&t)[DHT_W]) {
    const uint32_t k0 = kp[p];
    if (k0 != t[0]) return k0 < t[0];
    uint32_t k[DHT_W - 1];
#pragma unroll
    for (int w = 1; w < DHT_W; ++w) k[w - 1] = kp[(uint64_t)w * ks + p];
#pragma unroll
    for (int w = 1; w < DHT_W; ++w)
        if (k[w - 1] != t[w]) return k[w - 1] < t[w];
    return false;
}

// 256 threads, 256 / G keys per workgroup; group g of the wave owns bits [g * G, g * G + G) of a ballot
template <uint32_t G>
__global__ __launch_bounds__(256) void k_ncr_find(NcView v, uint32_t words, const uint32_t* __restrict__ ip, uint64_t is,
                                                  uint32_t m, uint32_t* __restrict__ out_h,
                                                  uint8_t* __restrict__ out_acc) {
    static_assert(G >= 2 && G <= 64 && (G & (G - 1)) == 0, "G lanes per key: a power of two within a wave");
    const uint32_t lane = lane_id(), l = lane & (G - 1), shift = lane & ~(G - 1);
    const uint64_t gmask = G == 64 ? ~0ull : (1ull << (G & 63)) - 1ull;
    const uint32_t qi = blockIdx.x * (256 / G) + threadIdx.x / G;
    const bool live = qi < m;   // (a group past the batch keeps voting: its range is empty)
    uint32_t t[DHT_W];
#pragma unroll
    for (int w = 0; w < DHT_W; ++w) t[w] = live ? ip[(uint64_t)w * is + qi] : 0u;
    uint32_t lo = 0, hi = live ? v.n : 0u;   // the bound lies in [lo, hi]; uniform per group
    while (__any(hi - lo > G)) {
        bool lt = false;
        uint32_t step = 0;
        if (hi - lo > G) {
            step = (uint32_t)(((uint64_t)(hi - lo) + G) / (G + 1));   // ceil(range / (G + 1)) >= 1
            const uint64_t p = (uint64_t)lo + (uint64_t)(l + 1) * step - 1;
            if (p < hi) lt = ncr_key_lt(v.kp, v.ks, p, t);
        }
        const uint32_t c = (uint32_t)__popcll((__ballot(lt) >> shift) & gmask);   // pivots below t: a prefix of the group
        if (step) {
            const uint64_t nlo = (uint64_t)lo + (uint64_t)c * step;   // pivot c - 1 is below t
            const uint64_t pc = nlo + step - 1;                       // pivot c is not, when it exists:
            if (c < G && pc < hi) hi = (uint32_t)pc;                  // there are G pivots, and G + 1 sub-ranges
            lo = (uint32_t)nlo;   // <= hi: at most `step` keys are left
        }
    }
    bool lt = false;
    {
        const uint64_t i = (uint64_t)lo + l;
        if (i < hi) lt = ncr_key_lt(v.kp, v.ks, i, t);
    }
    const uint32_t lb = lo + (uint32_t)__popcll((__ballot(lt) >> shift) & gmask);
    if (!live || l != 0) return;
    uint32_t h = DHT_NONE, acc = 0;
    if (lb < v.n) {
        uint32_t k[DHT_W];
        load_id(v.kp, v.ks, lb, k);
        const uint32_t hh = v.hp[lb];
        bool eq = true;
#pragma unroll
        for (int w = 0; w < DHT_W; ++w) eq = eq && k[w] == t[w];
        if (eq) {
            h = hh;
            if (out_acc && (h >> 5) < words) acc = (v.bits[h >> 5] >> (h & 31u)) & 1u;
        }
    }
    out_h[qi] = h;
    if (out_acc) out_acc[qi] = (uint8_t)acc;
}

// the new bytes of a get_nodes batch in batch order (k_nc_rank's result bytes): COUNT -- bsum[block]
// = the block's number of new keys; else ord[i] = boff[block] + the new keys before i in its block
// (ballots, the waves' counts through LDS: the k_nc_rank / k_nc_compact pattern)
template <bool COUNT>
__global__ __launch_bounds__(256) void k_ncr_order(const uint8_t* __restrict__ res, uint32_t m,
                                                   uint32_t* __restrict__ bsum, const uint32_t* __restrict__ boff,
                                                   uint32_t* __restrict__ ord) {
    __shared__ uint32_t wc[4];
    const uint32_t i = blockIdx.x * 256 + threadIdx.x, lane = lane_id(), w = threadIdx.x >> 6;
    const bool is_new = i < m && res[i];
    const uint64_t mask = __ballot(is_new);
    if (lane == 0) wc[w] = (uint32_t)__popcll(mask);
    __syncthreads();
    if (COUNT) {
        if (threadIdx.x == 0) bsum[blockIdx.x] = wc[0] + wc[1] + wc[2] + wc[3];
        return;
    }
    if (i >= m) return;
    uint32_t e = boff[blockIdx.x] + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
    for (uint32_t x = 0; x < w; ++x) e += wc[x];
    ord[i] = e;
}

struct NcrAssign {
    NcView v;
    const uint32_t* bp; uint64_t bs;        // the sorted batch
    const uint32_t* perm; uint32_t m;       // perm[j] = batch position of sorted key j
    const uint32_t* rank; const uint32_t* flag;   // k_nc_rank<false>'s
    const uint32_t* ord;                    // k_ncr_order's, by batch position
    const uint32_t* free; uint32_t nfree;   // the caller's free handles (the first min(nfree, m))
    uint32_t* hout;                         // [m] by batch position
};

// the r-th new key's handle; past the free list (the call then fails, nothing is applied): none
__device__ __forceinline__ uint32_t ncr_draw(const NcrAssign& a, uint32_t j) {
    const uint32_t r = a.ord[a.perm[j]];
    return r < a.nfree ? a.free[r] : DHT_NONE;
}

// One thread per sorted batch key.  A kept key draws free[ord]; a resident key has hp[rank]; any
// other key repeats an absent key, and the first key of its run of equal keys is the kept one (the
// sort is stable): found by a lower bound of the thread's own key in the sorted batch -- log2 m
// probes whatever the run's length.
__global__ __launch_bounds__(256) void k_ncr_assign(NcrAssign a) {
    const uint32_t j = blockIdx.x * 256 + threadIdx.x;
    if (j >= a.m) return;
    uint32_t h;
    if (a.flag[j]) {
        h = ncr_draw(a, j);
    } else {
        uint32_t b[DHT_W], k[DHT_W];
        load_id(a.bp, a.bs, j, b);
        const uint32_t r = a.rank[j];
        bool present = false;
        if (r < a.v.n) {
            load_id(a.v.kp, a.v.ks, r, k);
            present = lex_le(k, b);   // k >= b already
        }
        if (present) {
            h = a.v.hp[r];
        } else {
            uint32_t lo = 0, hi = j;   // the run's first key lies in [0, j]
            while (lo < hi) {
                const uint32_t mid = lo + (hi - lo) / 2;
                load_id(a.bp, a.bs, mid, k);
                if (lex_lt(k, b)) lo = mid + 1;
                else hi = mid;
            }
            h = ncr_draw(a, lo);
        }
    }
    a.hout[a.perm[j]] = h;
}

// out[perm[j]] = the handle sorted key j's erase frees (k_nc_rank<true>'s rank and flag), else none
__global__ __launch_bounds__(256) void k_ncr_extract(const uint32_t* __restrict__ hp, const uint32_t* __restrict__ perm,
                                                     const uint32_t* __restrict__ rank,
                                                     const uint32_t* __restrict__ flag, uint32_t m,
                                                     uint32_t* __restrict__ out) {
    const uint32_t j = blockIdx.x * 256 + threadIdx.x;
    if (j >= m) return;
    out[perm[j]] = flag[j] ? hp[rank[j]] : DHT_NONE;
}

inline uint32_t blocks256(uint64_t n) { return (uint32_t)((n + 255) / 256); }

template <uint32_t G>
hipError_t find_with(const NcView& v, uint32_t words, const uint32_t* ip, uint64_t is, uint32_t m, uint32_t* out_h,
                     uint8_t* out_acc, hipStream_t s) {
    constexpr uint32_t per = 256 / G;
    k_ncr_find<G><<<(m + per - 1) / per, 256, 0, s>>>(v, words, ip, is, m, out_h, out_acc);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_ncr_find(const NcView& v, uint64_t mask_words, const uint32_t* ip, uint64_t is, uint32_t m,
                           uint32_t* out_handle, uint8_t* out_accept, hipStream_t s) {
    if (!m) return hipSuccess;
    const uint32_t words = (uint32_t)std::min<uint64_t>(mask_words, 0xFFFFFFFFull);
    if (m <= kNcrWideMaxBatch) return find_with<kNcrWideLanes>(v, words, ip, is, m, out_handle, out_accept, s);
    return find_with<kNcrNarrowLanes>(v, words, ip, is, m, out_handle, out_accept, s);
}

hipError_t launch_ncr_assign(const NcView& v, const uint32_t* bp, uint64_t bs, const uint32_t* perm, uint32_t m,
                             const uint32_t* rank, const uint32_t* flag, const uint8_t* res, uint32_t* bsum,
                             uint32_t* boff, uint32_t* d_total, uint32_t* ord, const uint32_t* free_handles, uint32_t nfree,
                             uint32_t* hout, hipStream_t s) {
    if (!m) return hipSuccess;
    const uint32_t nb = blocks256(m);
    k_ncr_order<true><<<nb, 256, 0, s>>>(res, m, bsum, nullptr, nullptr);
    if (hipError_t e = launch_excl_scan(bsum, boff, 1, nb, d_total, s)) return e;
    k_ncr_order<false><<<nb, 256, 0, s>>>(res, m, nullptr, boff, ord);
    k_ncr_assign<<<nb, 256, 0, s>>>(NcrAssign{v, bp, bs, perm, m, rank, flag, ord, free_handles, nfree, hout});
    return hipGetLastError();
}

hipError_t launch_ncr_extract(const NcView& v, const uint32_t* perm, const uint32_t* rank, const uint32_t* flag,
                              uint32_t m, uint32_t* out, hipStream_t s) {
    if (!m) return hipSuccess;
    k_ncr_extract<<<blocks256(m), 256, 0, s>>>(v.hp, perm, rank, flag, m, out);
    return hipGetLastError();
}

}  // namespace dhtgpu
