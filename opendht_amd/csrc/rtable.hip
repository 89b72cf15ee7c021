// rtable.hip -- K1w: the resident routing table's wave-per-target kernels for gfx950.
//   k_rt<form, K>  RoutingTable::findClosestNodes (src/routing_table.cpp:110-150) over the
//                  table mirror of dhtgpu_rt_set, in three output forms:
//                    indices   the result of dhtgpu_find_closest
//                    reply     + NetworkEngine::bufferNodes (src/network_engine.cpp:1003-1032):
//                              onFindNode / onGetValues' findClosestNodes(target, now, 8) packed
//                    closer    + key.xorCmp(nodes.back()->id, myid) < 0, the closeness test of
//                              maintainStorage (src/dht.cpp:1862-1879) and onAnnounce (:2293-2294)
//   k_rt_gpre      prefix sums of the per-bucket good counts (after a change of the good bytes)
//
// K1r (table.hip) gives one thread a serial, dependent-load walk; that suits 65,536 targets and
// leaves the machine idle at a responder's batch sizes.  Here one wave64 answers one target, the
// target index is wave-uniform (header reads are scalar loads) and every phase is a few ballots:
//   findBucket  lanes compare 64 bucket firsts per round (five-word lexicographic compare); the
//               highest set lane of the ballot is the last bucket b >= 1 with first_b <= t
//               (table.hip:52-62), bucket 0 when none.  At most four rounds (nb <= 256).
//   walk        after R rounds the reference has visited buckets [max(0, j-R), min(nb, j+R)), so
//               the walk ends at the smallest R >= 1 with gpre[min(nb, j+R)] - gpre[max(0, j-R)]
//               >= count, or at R = max(j, nb - j) when both sides have run out (table.hip:63-70).
//               Lane l evaluates R = base + l + 1; the ballot's first lane is the answer.
//   selection   the slice [lo, hi) is read 64 nodes per step (word 0, word 1, the good byte: three
//               coalesced loads).  The best `count` so far live one per lane, closest in lane 0.
//               The first step meets an empty list: each of its good nodes is broadcast in turn,
//               the ballot of the step's good nodes closer than it is its place, and the lane of
//               that number takes it -- the whole selection when the slice holds at most 64 nodes
//               (every grown table).  Later steps insert into the list: of a step's good nodes
//               only those not behind the list's last entry are broadcast, every lane compares its
//               entry, the ballot's population count is the place, the lanes behind shift up by
//               one.  (d0, d1) decide; words 2..4 are loaded on a 64-bit tie only; equal ids order
//               by lower index -- the order of ent_less.
// Bytes per target: 20 (target) + 20 nb (firsts) + 4 (nb + 1) (prefix sums, L2-resident) + 9 per
// node of the slice; the reply form adds 8 x (20 + alen + 2) gathered and as many written.
#include "dhtgpu_dev.h"
#include "dhtgpu_internal.h"

namespace dhtgpu {
namespace {

constexpr uint32_t kRtWaves = 4;     // targets per 256-thread workgroup
constexpr uint32_t kRtReplyNodes = 8;   // TARGET_NODES / SEND_NODES (src/network_engine.cpp:62)

enum RtForm : int { kRtIdx = 0, kRtReply = 1, kRtCloser = 2 };

// outputs of the three forms (the unused ones are null)
struct RtOut {
    uint32_t* idx;    // q x count indices (reply: q x 8, nullable)
    uint32_t* cnt;    // q counts (closer: nullable)
    uint8_t* bytes;   // reply: q x 8 records
    uint32_t* len;    // reply: q byte lengths
    uint8_t* flag;    // closer: q flags
    uint32_t min_nodes;
};

// (a ^ t) < (b ^ t) over words 2..4, then the lower index: the tail of ent_less
__device__ __forceinline__ bool rt_tie_less(const uint32_t* __restrict__ np, uint64_t ns, uint32_t ia, uint32_t ib,
                                            const uint32_t* t) {
#pragma unroll
    for (int w = 2; w < DHT_W; ++w) {
        const uint32_t da = np[(uint64_t)w * ns + ia] ^ t[w], db = np[(uint64_t)w * ns + ib] ^ t[w];
        if (da != db) return da < db;
    }
    return ia < ib;
}

// the value of the lane below (lanes 1 .. K - 1): a list of K <= 16 entries lies in one 16-lane
// row, where a DPP row shift does it inside the VALU; 32 entries cross rows (ds_bpermute)
template <uint32_t K>
__device__ __forceinline__ uint32_t rt_up1(uint32_t x) {
    if constexpr (K <= 16) return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x111, 0xF, 0xF, false);   // row_shr:1
    else return __shfl_up(x, 1);
}

// FORM: the output (RtForm); K: the list's capacity, count <= K
template <int FORM, uint32_t K>
__global__ __launch_bounds__(256) void k_rt(RtView v, const uint32_t* __restrict__ tp, uint64_t ts, uint32_t q,
                                            uint32_t count, RtOut o) {
    static_assert(K <= DHTGPU_MAX_K_DEV, "one list entry per lane");
    const uint32_t lane = lane_id();
    const uint32_t qi = __builtin_amdgcn_readfirstlane(blockIdx.x * kRtWaves + (threadIdx.x >> 6));
    if (qi >= q) return;
    uint32_t t[DHT_W];
#pragma unroll
    for (int w = 0; w < DHT_W; ++w) t[w] = tp[(uint64_t)w * ts + qi];

    uint32_t lo = 0, hi = 0;
    if (v.nb) {
        // findBucket
        uint32_t j = 0;
        for (uint32_t base = 0; base < v.nb; base += 64) {
            const uint32_t b = base + lane;
            bool le = false;
            if (b >= 1 && b < v.nb) {
                uint32_t f[DHT_W];
#pragma unroll
                for (int w = 0; w < DHT_W; ++w) f[w] = v.fp[(uint64_t)w * v.nb + b];
                le = lex_le(f, t);
            }
            const uint64_t m = __ballot(le);
            if (m) j = base + 63u - (uint32_t)__clzll((long long)m);
        }
        // outward walk: the first round count R at which it stops
        const uint32_t rmax = j > v.nb - j ? j : v.nb - j;
        uint32_t rs = rmax;
        for (uint32_t base = 0; base < rmax; base += 64) {
            const uint32_t r = base + lane + 1;
            const uint32_t a = j > r ? j - r : 0u, e = j + r < v.nb ? j + r : v.nb;
            const bool ok = r >= rmax || v.gpre[e] - v.gpre[a] >= count;
            const uint64_t m = __ballot(ok);
            if (m) {
                rs = base + (uint32_t)__ffsll((long long)m);
                break;
            }
        }
        lo = v.off[j > rs ? j - rs : 0u];
        hi = v.off[j + rs < v.nb ? j + rs : v.nb];
    }
    lo = __builtin_amdgcn_readfirstlane(lo);
    hi = __builtin_amdgcn_readfirstlane(hi);

    // selection: lane r < have holds the r-th closest good node so far
    uint32_t ed0 = DHT_NONE, ed1 = DHT_NONE, eidx = DHT_NONE;
    uint32_t have = 0;
    for (uint32_t base = lo; base < hi; base += 64) {
        const uint32_t i = base + lane;
        bool act = false;
        uint32_t cd0 = 0, cd1 = 0;
        if (i < hi) {
            act = v.good[i] != 0;
            cd0 = v.np[i] ^ t[0];
            cd1 = v.np[v.ns + i] ^ t[1];
        }
        uint64_t m = __ballot(act);
        if (base == lo) {
            // the first step meets an empty list: a good node's place is the number of the step's
            // good nodes closer than it, and the lane of that number takes it
            for (uint64_t it = m; it; it &= it - 1) {
                const uint32_t src = (uint32_t)__ffsll((long long)it) - 1;
                const uint32_t x0 = (uint32_t)__builtin_amdgcn_readlane((int)cd0, (int)src);
                const uint32_t x1 = (uint32_t)__builtin_amdgcn_readlane((int)cd1, (int)src);
                const uint32_t xi = base + src;
                bool lt = false;
                if (act && lane != src) {
                    if (cd0 != x0) lt = cd0 < x0;
                    else if (cd1 != x1) lt = cd1 < x1;
                    else lt = rt_tie_less(v.np, v.ns, i, xi, t);
                }
                const uint32_t pos = (uint32_t)__popcll(__ballot(lt));
                if (lane == pos && pos < count) {
                    ed0 = x0;
                    ed1 = x1;
                    eidx = xi;
                }
            }
            const uint32_t n = (uint32_t)__popcll(m);
            have = n < count ? n : count;
            continue;
        }
        if (have == count) {   // a full list: only what is not behind its last entry
            const uint32_t w0 = (uint32_t)__builtin_amdgcn_readlane((int)ed0, (int)(count - 1));
            const uint32_t w1 = (uint32_t)__builtin_amdgcn_readlane((int)ed1, (int)(count - 1));
            m &= __ballot(cd0 < w0 || (cd0 == w0 && cd1 <= w1));
        }
        while (m) {
            const uint32_t src = (uint32_t)__ffsll((long long)m) - 1;
            m &= m - 1;
            const uint32_t x0 = (uint32_t)__builtin_amdgcn_readlane((int)cd0, (int)src);
            const uint32_t x1 = (uint32_t)__builtin_amdgcn_readlane((int)cd1, (int)src);
            const uint32_t xi = base + src;
            // the entries closer than the candidate are a prefix of the list
            bool lt = false;
            if (lane < have) {
                if (ed0 != x0) lt = ed0 < x0;
                else if (ed1 != x1) lt = ed1 < x1;
                else lt = rt_tie_less(v.np, v.ns, eidx, xi, t);
            }
            const uint32_t pos = (uint32_t)__popcll(__ballot(lt));
            if (pos >= count) continue;
            const uint32_t u0 = rt_up1<K>(ed0), u1 = rt_up1<K>(ed1), ui = rt_up1<K>(eidx);
            if (lane == pos) {
                ed0 = x0;
                ed1 = x1;
                eidx = xi;
            } else if (lane > pos && lane < count) {
                ed0 = u0;
                ed1 = u1;
                eidx = ui;
            }
            if (have < count) ++have;
            if (have == count) {
                const uint32_t w0 = (uint32_t)__builtin_amdgcn_readlane((int)ed0, (int)(count - 1));
                const uint32_t w1 = (uint32_t)__builtin_amdgcn_readlane((int)ed1, (int)(count - 1));
                m &= __ballot(cd0 < w0 || (cd0 == w0 && cd1 <= w1));
            }
        }
    }

    if constexpr (FORM == kRtIdx) {
        if (lane < count) o.idx[(uint64_t)qi * count + lane] = eidx;
        if (lane == 0) o.cnt[qi] = have;
    } else if constexpr (FORM == kRtReply) {
        const uint32_t rec = 20 + v.alen + 2;
        if (lane < have) {   // one record per lane, as k_wire_encode writes it
            uint8_t* dst = o.bytes + ((uint64_t)qi * kRtReplyNodes + lane) * rec;
#pragma unroll
            for (int w = 0; w < DHT_W; ++w) {
                const uint32_t x = v.np[(uint64_t)w * v.ns + eidx];
                dst[4 * w] = (uint8_t)(x >> 24);
                dst[4 * w + 1] = (uint8_t)(x >> 16);
                dst[4 * w + 2] = (uint8_t)(x >> 8);
                dst[4 * w + 3] = (uint8_t)x;
            }
            const uint8_t* src = v.tail + (uint64_t)eidx * (v.alen + 2);
            for (uint32_t b = 0; b < v.alen + 2; ++b) dst[20 + b] = src[b];
        }
        if (lane == 0) o.len[qi] = have * rec;
        if (o.idx && lane < kRtReplyNodes) o.idx[(uint64_t)qi * kRtReplyNodes + lane] = eidx;
    } else {
        // target.xorCmp(last result's id, myid) < 0, evaluated by the lane that holds the last result
        bool closer = false;
        if (have && lane == have - 1) {
            bool decided = false;
#pragma unroll
            for (int w = 0; w < DHT_W; ++w) {
                const uint32_t dn = v.np[(uint64_t)w * v.ns + eidx] ^ t[w], dm = v.myid[w] ^ t[w];
                if (!decided && dn != dm) {
                    closer = dn < dm;
                    decided = true;
                }
            }
        }
        const bool any = __ballot(closer) != 0;
        const uint32_t need = o.min_nodes ? o.min_nodes : 1u;
        if (lane == 0) {
            o.flag[qi] = have >= need && any ? 1 : 0;
            if (o.cnt) o.cnt[qi] = have;
        }
    }
}

// gpre[b] = good nodes of buckets [0, b), b <= nb: one wave per bucket counts (ballots over the
// bucket's good bytes), then thread b sums the counts before it
__global__ __launch_bounds__(256) void k_rt_gpre(uint32_t nb, const uint32_t* __restrict__ off,
                                                 const uint8_t* __restrict__ good, uint32_t* __restrict__ gpre) {
    __shared__ uint32_t s[256];
    const uint32_t lane = lane_id();
    for (uint32_t b = threadIdx.x >> 6; b < nb; b += 4) {
        const uint32_t lo = off[b], hi = off[b + 1];
        uint32_t c = 0;
        for (uint32_t base = lo; base < hi; base += 64) {
            const uint32_t i = base + lane;
            c += (uint32_t)__popcll(__ballot(i < hi && good[i] != 0));
        }
        if (lane == 0) s[b] = c;
    }
    __syncthreads();
    const uint32_t b = threadIdx.x;
    if (b < nb) {
        uint32_t sum = 0;
        for (uint32_t i = 0; i <= b; ++i) sum += s[i];
        gpre[b + 1] = sum;
    }
    if (b == 0) gpre[0] = 0;
}

template <int FORM>
hipError_t launch_rt(const RtView& v, const uint32_t* tp, uint64_t ts, uint32_t q, uint32_t count, const RtOut& o,
                     hipStream_t s) {
    if (!q) return hipSuccess;
    const dim3 grid((q + kRtWaves - 1) / kRtWaves), block(64 * kRtWaves);
    if constexpr (FORM == kRtReply) {   // count = kRtReplyNodes
        k_rt<FORM, 8><<<grid, block, 0, s>>>(v, tp, ts, q, count, o);
    } else {
        if (count <= 8) k_rt<FORM, 8><<<grid, block, 0, s>>>(v, tp, ts, q, count, o);
        else if (count <= 16) k_rt<FORM, 16><<<grid, block, 0, s>>>(v, tp, ts, q, count, o);
        else k_rt<FORM, 32><<<grid, block, 0, s>>>(v, tp, ts, q, count, o);
    }
    return hipGetLastError();
}

}  // namespace

hipError_t launch_rt_gpre(const RtView& v, uint32_t* gpre, hipStream_t s) {
    k_rt_gpre<<<1, 256, 0, s>>>(v.nb, v.off, v.good, gpre);
    return hipGetLastError();
}

hipError_t launch_rt_find(const RtView& v, const uint32_t* tp, uint64_t ts, uint32_t q, uint32_t count,
                          uint32_t* out_idx, uint32_t* out_cnt, hipStream_t s) {
    return launch_rt<kRtIdx>(v, tp, ts, q, count, RtOut{out_idx, out_cnt, nullptr, nullptr, nullptr, 0}, s);
}

hipError_t launch_rt_reply(const RtView& v, const uint32_t* tp, uint64_t ts, uint32_t q, uint8_t* out,
                           uint32_t* out_len, uint32_t* out_idx, hipStream_t s) {
    return launch_rt<kRtReply>(v, tp, ts, q, kRtReplyNodes, RtOut{out_idx, nullptr, out, out_len, nullptr, 0}, s);
}

hipError_t launch_rt_closer(const RtView& v, const uint32_t* tp, uint64_t ts, uint32_t q, uint32_t count,
                            uint32_t min_nodes, uint8_t* out_flag, uint32_t* out_cnt, hipStream_t s) {
    return launch_rt<kRtCloser>(v, tp, ts, q, count, RtOut{nullptr, out_cnt, nullptr, nullptr, out_flag, min_nodes}, s);
}

}  // namespace dhtgpu
