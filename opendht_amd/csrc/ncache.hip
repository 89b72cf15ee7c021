// ncache.hip -- K8w: the resident NodeCache mirror's kernels for gfx950 (dhtgpu_nc_*).
//   k_nc            NodeCache::getCachedNodes (src/node_cache.cpp:42-74) over the mirror: one wave64
//                   per target, the accepted keys' handles in the reference's walk order
//   k_nc_rank       a sorted mutation batch against the resident keys: rank, keep flag, result byte,
//                   kept keys per 256-key block
//   k_nc_compact    the kept batch keys' ranks and sources, compacted
//   k_nc_merge      the resident keys and the kept batch keys into the other buffer set
//   k_nc_handles    the handle plane of dhtgpu_nc_set (+ the handles' accept bits)
//   k_nc_bits_pack  accept bits by handle from bytes (set_accept)
// The scan of k_nc_rank's block counts and update_accept's bit setter are the shared ones of prims.hip.
//
// The mirror is NodeCache::NodeMap (include/opendht/node_cache.h:43) as six u32 planes -- the five
// key words, lexicographically sorted, and the caller's handle of each key (the map's value) --
// plus an accept bitmask indexed by handle (bit = lock() && !isExpired() && !isClient(),
// src/node_cache.cpp:68-69).
//
// Lookup.  K8 (table.hip, k_cached) gives one thread ceil(log2 n) dependent probes of five strided
// loads and a serial walk of two dependent five-word loads per step.  Here the target index is
// wave-uniform and:
//   lower bound  64-ary: each round the lanes compare 64 evenly spaced pivots of the open range
//                with the five-word lexicographic compare; the ballot's population count picks the
//                sub-range, which is under 1/64 of the range.  A range of at most 64 keys is
//                settled by one round over the keys themselves: ceil(log64(n + 1)) rounds.
//   windows      64 consecutive keys on each side of the lower bound (lane l: key lb + l of the
//                next side, key lb - 1 - l of the previous side) come in by coalesced plane loads,
//                already XORed with the target, with their handles; the accept bits of a window
//                are one ballot.
//   walk         the reference's head comparison, not a distance sort (neither side is monotone
//                in XOR distance): the two heads are read out of the windows' registers
//                (v_readlane), compared over all 160 bits, the closer one is consumed, and its
//                handle goes to lane c of the result when its accept bit is set.  A side whose
//                window is used up loads its next 64 keys.  Every step advances exactly one of
//                the two cursors, so a walk takes at most n steps; no loop waits on data.
// Bytes per target: 20 (target) + 20 x 64 per search round + (24 + 4) x 64 per window loaded (two
// at least; the accept words are a gather).
//
// Mutation (insert = std::map::emplace, erase = map.erase(key), m keys): the batch is sorted by
// sort.hip (stable: of equal keys the first in batch order comes first), ranked in the resident
// keys by a lower bound per batch key (m x ceil(log2 n) probes), the keep flags are counted per
// 256-key block and the counts scanned, and one pass writes the other buffer set: resident key i lands at i + #{kept batch keys ranked <= i}
// on insert and at i - #{erased positions < i} on erase, kept batch key j at rank_j + kept-index_j.
// The count per resident key is a search of the compacted rank list, narrowed per 256-key block
// to the few entries that fall into the block.  Algorithmic bytes of the pass: 24 B read and 24 B
// written per resident key (each key once), 24 B + 12 B per kept batch key; the rank list (4 B per
// kept key) stays in L2.  No radix pass touches the resident keys.
#include "dhtgpu_dev.h"
#include "dhtgpu_internal.h"
#include "nc_walk_dev.h"

namespace dhtgpu {
namespace {

constexpr uint32_t kNcWaves = 4;   // targets per 256-thread workgroup

// (the lower bound, the windows and the walk: nc_walk_dev.h, shared with k_sr_refill)
__global__ __launch_bounds__(256) void k_nc(NcView v, const uint32_t* __restrict__ tp, uint64_t ts, uint32_t q,
                                            uint32_t count, uint32_t* __restrict__ out_h,
                                            uint32_t* __restrict__ out_cnt) {
    const uint32_t lane = lane_id();
    const uint32_t qi = __builtin_amdgcn_readfirstlane(blockIdx.x * kNcWaves + (threadIdx.x >> 6));
    if (qi >= q) return;
    uint32_t t[DHT_W];
#pragma unroll
    for (int w = 0; w < DHT_W; ++w) t[w] = tp[(uint64_t)w * ts + qi];
    uint32_t outv = DHT_NONE;   // lane c: the c-th accepted key's handle
    const uint32_t c = nc_walk<false>(v, nullptr, 0, t, count, lane, [&](uint32_t ci, const uint32_t*, uint32_t h, uint32_t) {
        if (lane == ci) outv = h;
    });
    if (lane < count) out_h[(uint64_t)qi * count + lane] = outv;
    if (lane == 0) out_cnt[qi] = c;
}

// Batch key j (sorted) against the resident keys: rank[j] = its lower bound, flag[j] = 1 when the
// mutation applies to it -- insert: not resident and not equal to the batch key before it; erase:
// resident and not equal to the batch key before it -- res[perm[j]] = flag[j], and bsum[block] =
// the block's number of set flags.
template <bool ERASE>
__global__ __launch_bounds__(256) void k_nc_rank(const uint32_t* __restrict__ kp, uint64_t ks, uint32_t n,
                                                 const uint32_t* __restrict__ bp, uint64_t bs,
                                                 const uint32_t* __restrict__ perm, uint32_t m,
                                                 uint32_t* __restrict__ rank, uint32_t* __restrict__ flag,
                                                 uint32_t* __restrict__ bsum, uint8_t* __restrict__ res) {
    __shared__ uint32_t wc[4];
    const uint32_t j = blockIdx.x * 256 + threadIdx.x;
    bool keep = false;
    if (j < m) {
        uint32_t b[DHT_W], k[DHT_W];
        load_id(bp, bs, j, b);
        uint32_t lo = 0, hi = n;
        while (lo < hi) {
            const uint32_t mid = lo + (hi - lo) / 2;
            load_id(kp, ks, mid, k);
            if (lex_lt(k, b)) lo = mid + 1;
            else hi = mid;
        }
        bool present = false;
        if (lo < n) {
            load_id(kp, ks, lo, k);
            present = lex_le(k, b);   // k >= b already
        }
        bool dup = false;
        if (j > 0) {
            load_id(bp, bs, j - 1, k);
            dup = lex_le(b, k);       // sorted: k <= b
        }
        keep = (ERASE ? present : !present) && !dup;
        rank[j] = lo;
        flag[j] = keep;
        res[perm[j]] = keep;
    }
    const uint64_t mask = __ballot(keep);
    if (lane_id() == 0) wc[threadIdx.x >> 6] = (uint32_t)__popcll(mask);
    __syncthreads();
    if (threadIdx.x == 0) bsum[blockIdx.x] = wc[0] + wc[1] + wc[2] + wc[3];
}

// the kept batch keys' ranks and sources as dense lists: kept key j goes to boff[block] + the kept
// keys before it in its block (ballots, the waves' counts through LDS)
__global__ __launch_bounds__(256) void k_nc_compact(const uint32_t* __restrict__ rank, const uint32_t* __restrict__ flag,
                                                    const uint32_t* __restrict__ boff, uint32_t m,
                                                    uint32_t* __restrict__ kpos, uint32_t* __restrict__ ksrc) {
    __shared__ uint32_t wc[4];
    const uint32_t j = blockIdx.x * 256 + threadIdx.x, lane = lane_id(), w = threadIdx.x >> 6;
    const bool keep = j < m && flag[j];
    const uint64_t mask = __ballot(keep);
    if (lane == 0) wc[w] = (uint32_t)__popcll(mask);
    __syncthreads();
    if (!keep) return;
    uint32_t e = boff[blockIdx.x] + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
    for (uint32_t i = 0; i < w; ++i) e += wc[i];
    kpos[e] = rank[j];
    ksrc[e] = j;
}

// #{e < cnt: kpos[e] < x} (STRICT) or #{kpos[e] <= x}, known to lie in [lo, hi]
template <bool STRICT>
__device__ __forceinline__ uint32_t nc_count(const uint32_t* __restrict__ kpos, uint32_t lo, uint32_t hi, uint32_t x) {
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        const uint32_t p = kpos[mid];
        if (STRICT ? p < x : p <= x) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

struct NcMerge {
    const uint32_t* src; uint64_t ss; uint32_t n;   // the resident planes (five key words + handles)
    uint32_t* dst; uint64_t ds;                     // the other buffer set
    const uint32_t* kpos; uint32_t cnt;             // insert: the kept batch keys' ranks; erase: the erased positions
    // insert only: the sorted batch, its kept keys' sources, the batch's handles and accept bytes
    // in the caller's order (accept nullable: accepted), the accept mask
    const uint32_t* bp; uint64_t bs;
    const uint32_t* ksrc; const uint32_t* perm;
    const uint32_t* hin; const uint8_t* ain;
    uint32_t* bits;
};

// threads [0, n): the resident keys; insert: threads [n, n + cnt) the kept batch keys
template <bool ERASE>
__global__ __launch_bounds__(256) void k_nc_merge(NcMerge a) {
    __shared__ uint32_t range[2];
    const uint64_t i0 = (uint64_t)blockIdx.x * 256;
    if (threadIdx.x == 0 && i0 < a.n) {   // the block's keys see counts in [range[0], range[1]]
        const uint64_t last = i0 + 255 < a.n ? i0 + 255 : (uint64_t)a.n - 1;
        range[0] = nc_count<ERASE>(a.kpos, 0, a.cnt, (uint32_t)i0);
        range[1] = nc_count<ERASE>(a.kpos, range[0], a.cnt, (uint32_t)last);
    }
    __syncthreads();
    const uint64_t i = i0 + threadIdx.x;
    if (i < a.n) {
        const uint32_t c = nc_count<ERASE>(a.kpos, range[0], range[1], (uint32_t)i);
        uint64_t pos;
        if (ERASE) {
            if (c < a.cnt && a.kpos[c] == (uint32_t)i) return;   // erased
            pos = i - c;
        } else {
            pos = i + c;
        }
#pragma unroll
        for (int w = 0; w < DHT_W + 1; ++w) a.dst[(uint64_t)w * a.ds + pos] = a.src[(uint64_t)w * a.ss + i];
        return;
    }
    if (ERASE) return;
    const uint64_t e = i - a.n;
    if (e >= a.cnt) return;
    const uint32_t j = a.ksrc[e], o = a.perm[j], h = a.hin[o];
    const uint64_t pos = (uint64_t)a.kpos[e] + e;
#pragma unroll
    for (int w = 0; w < DHT_W; ++w) a.dst[(uint64_t)w * a.ds + pos] = a.bp[(uint64_t)w * a.bs + j];
    a.dst[(uint64_t)DHT_W * a.ds + pos] = h;
    if (!a.ain || a.ain[o]) atomicOr(a.bits + (h >> 5), 1u << (h & 31u));
    else atomicAnd(a.bits + (h >> 5), ~(1u << (h & 31u)));
}

// hp[j] = the handle of sorted key j: hin[perm[j]] (its accept bit set), or perm[j] when hin is null
__global__ __launch_bounds__(256) void k_nc_handles(const uint32_t* __restrict__ perm, const uint32_t* __restrict__ hin,
                                                    uint32_t n, uint32_t* __restrict__ hp, uint32_t* __restrict__ bits) {
    const uint32_t j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    if (!hin) {
        hp[j] = perm[j];
        return;
    }
    const uint32_t h = hin[perm[j]];
    hp[j] = h;
    atomicOr(bits + (h >> 5), 1u << (h & 31u));
}

// bits of handles [0, nh) from bytes[nh]; the last word keeps its bits past nh
__global__ __launch_bounds__(256) void k_nc_bits_pack(const uint8_t* __restrict__ bytes, uint32_t nh,
                                                      uint32_t* __restrict__ bits) {
    const uint32_t w = blockIdx.x * 256 + threadIdx.x;
    if ((uint64_t)w * 32 >= nh) return;
    const uint32_t left = nh - w * 32;
    const uint32_t cnt = left < 32 ? left : 32u;
    uint32_t x = 0;
    for (uint32_t b = 0; b < cnt; ++b) x |= (bytes[(uint64_t)w * 32 + b] ? 1u : 0u) << b;
    if (cnt < 32) x |= bits[w] & ~((1u << cnt) - 1u);
    bits[w] = x;
}

inline uint32_t blocks256(uint64_t n) { return (uint32_t)((n + 255) / 256); }

}  // namespace

hipError_t launch_nc_nodes(const NcView& v, const uint32_t* tp, uint64_t ts, uint32_t q, uint32_t count,
                           uint32_t* out_handle, uint32_t* out_cnt, hipStream_t s) {
    if (!q) return hipSuccess;
    k_nc<<<(q + kNcWaves - 1) / kNcWaves, 64 * kNcWaves, 0, s>>>(v, tp, ts, q, count, out_handle, out_cnt);
    return hipGetLastError();
}

hipError_t launch_nc_rank(bool erase, const NcView& v, const uint32_t* bp, uint64_t bs, const uint32_t* perm, uint32_t m,
                          uint32_t* rank, uint32_t* flag, uint32_t* bsum, uint32_t* boff, uint32_t* kpos, uint32_t* ksrc,
                          uint32_t* d_total, uint8_t* res, hipStream_t s) {
    if (!m) return hipSuccess;
    const uint32_t nb = blocks256(m);
    if (erase) k_nc_rank<true><<<nb, 256, 0, s>>>(v.kp, v.ks, v.n, bp, bs, perm, m, rank, flag, bsum, res);
    else k_nc_rank<false><<<nb, 256, 0, s>>>(v.kp, v.ks, v.n, bp, bs, perm, m, rank, flag, bsum, res);
    // the blocks' counts scanned + their total, the one host read-back (4 KB per million batch keys)
    if (hipError_t e = launch_excl_scan(bsum, boff, 1, nb, d_total, s)) return e;
    k_nc_compact<<<nb, 256, 0, s>>>(rank, flag, boff, m, kpos, ksrc);
    return hipGetLastError();
}

hipError_t launch_nc_insert(const NcView& v, uint32_t* dst, uint64_t ds, const uint32_t* kpos, const uint32_t* ksrc,
                            uint32_t cnt, const uint32_t* bp, uint64_t bs, const uint32_t* perm, const uint32_t* hin,
                            const uint8_t* ain, uint32_t* bits, hipStream_t s) {
    const uint64_t threads = (uint64_t)v.n + cnt;
    if (!threads) return hipSuccess;
    k_nc_merge<false><<<blocks256(threads), 256, 0, s>>>(NcMerge{v.kp, v.ks, v.n, dst, ds, kpos, cnt, bp, bs, ksrc, perm,
                                                                 hin, ain, bits});
    return hipGetLastError();
}

hipError_t launch_nc_erase(const NcView& v, uint32_t* dst, uint64_t ds, const uint32_t* kpos, uint32_t cnt,
                           hipStream_t s) {
    if (!v.n) return hipSuccess;
    k_nc_merge<true><<<blocks256(v.n), 256, 0, s>>>(NcMerge{v.kp, v.ks, v.n, dst, ds, kpos, cnt, nullptr, 0, nullptr,
                                                            nullptr, nullptr, nullptr, nullptr});
    return hipGetLastError();
}

hipError_t launch_nc_handles(const uint32_t* perm, const uint32_t* hin, uint32_t n, uint32_t* hp, uint32_t* bits,
                             hipStream_t s) {
    if (!n) return hipSuccess;
    k_nc_handles<<<blocks256(n), 256, 0, s>>>(perm, hin, n, hp, bits);
    return hipGetLastError();
}

hipError_t launch_nc_bits_pack(const uint8_t* bytes, uint32_t nh, uint32_t* bits, hipStream_t s) {
    if (!nh) return hipSuccess;
    k_nc_bits_pack<<<blocks256(((uint64_t)nh + 31) / 32), 256, 0, s>>>(bytes, nh, bits);
    return hipGetLastError();
}

}  // namespace dhtgpu
