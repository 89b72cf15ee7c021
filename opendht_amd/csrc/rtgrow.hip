// rtgrow.hip -- K1g: the resident routing table grows and is maintained on the device (gfx950).
//   k_rtg<false>   a batch of RoutingTable::onNewNode (src/routing_table.cpp:204-262, split :87-107 /
//                  :176-202) applied in order: KNOWN / PLACED / REPLACED / split and retry / FULL
//   k_rtg<true>    Dht::expireBuckets (src/dht.cpp:179-192): every expired node leaves its bucket
//   k_rtg_set_state / k_rtg_handles   the state bytes by handle; K1w's positions -> handles
//
// The work is sequential across insertions (a split changes the next insertion's bucket) and
// parallel inside one, so a call is one launch of one workgroup that holds the table in LDS:
//   load        the dense K1w blob becomes a bucket directory (five first words, row id, count; a
//               split shifts only this) and rows of 8 slots that never move.  A row is stored in
//               REVERSED list order -- slot 0 is the list's back, slot count - 1 its front -- so
//               emplace_front is a store behind the row's last slot, and "the first node in list
//               order" of a ballot over the row is its highest lane.
//   insertion   by wave 0, the node's values wave-uniform: findBucket is k_rt's ballot over the
//               directory (64 firsts per round); lanes 0..7 hold the row and the known / expired /
//               not-good / ping-pick tests are four ballots; contains(myid) and depth are uniform
//               arithmetic; a split hands the new bucket a fresh row, sends each node to its side by
//               one ballot and places it by the population count of its side's lanes above it (the
//               reference takes the old list from its front and pushes each node to the front of
//               its bucket), then shifts the directory tail by one entry, top chunk first.
//   write-back  by the workgroup: the counts' exclusive scan (block_scan_excl) gives off; rows go
//               to the dense planes of the other blob of the pair, the handle -> position map is
//               scattered, and {nb, nn, splits, stopped} go back with the results.
// LDS: 5 * 256 + 3 * 256 directory words, 2,048 slots x (5 id words + handle + 5 tail words + 1 state
// byte) = 100,416 B, inside the 160 KB of a gfx950 workgroup.
#include "dhtgpu_dev.h"
#include "dhtgpu_internal.h"
#include "prims_dev.h"

namespace dhtgpu {
namespace {

constexpr uint32_t kNB = kRtgBuckets, kNN = kRtgNodes, kRow = 8, kTailW = 5, kThreads = 256;
constexpr uint32_t kMaxRounds = 161;   // a split per bit of the id, and the placement

enum : uint8_t { kResNone = 0, kResKnown = 1, kResPlaced = 2, kResReplaced = 3, kResFull = 4, kResUnapplied = 5 };
enum : uint8_t { kStGood = 1, kStExpired = 2, kStPending = 4 };

// the table in LDS
struct Lds {
    uint32_t* first;   // [5][kNB] bucket firsts, first[w * kNB + b]
    uint32_t* row;     // [kNB] the bucket's row
    uint32_t* cnt;     // [kNB] its nodes
    uint32_t* off;     // [kNB + 1] write-back: exclusive scan of cnt
    uint32_t* wsum;    // block_scan_excl's scratch
    uint32_t* misc;    // {nb, splits, stopped, removed}
    uint32_t* w;       // [5][kNN] slot id words, w[k * kNN + slot]
    uint32_t* h;       // [kNN] slot handles
    uint32_t* t;       // [kTailW][kNN] slot tails (address || port, little-endian packed)
    uint8_t* st;       // [kNN] slot state bytes (bit 0 good, 1 expired, 2 pending)
};
constexpr uint32_t kLdsWords = 5 * kNB + 3 * kNB + 4 + 8 + 4 + (5 + 1 + kTailW) * kNN;
constexpr uint32_t kLdsBytes = kLdsWords * 4 + kNN;
static_assert(kLdsBytes <= 160 * 1024, "the table fits the LDS of one gfx950 workgroup");

__device__ __forceinline__ Lds lds_carve(uint32_t* p) {
    Lds s;
    s.first = p;
    s.row = s.first + 5 * kNB;
    s.cnt = s.row + kNB;
    s.off = s.cnt + kNB;
    s.wsum = s.off + kNB + 4;
    s.misc = s.wsum + 8;
    s.w = s.misc + 4;
    s.h = s.w + 5 * kNN;
    s.t = s.h + kNN;
    s.st = reinterpret_cast<uint8_t*>(s.t + kTailW * kNN);
    return s;
}

// what one lane's LDS stores must mean to the other lanes of its wave before they go on
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// one slot in registers
struct Slot {
    uint32_t w[DHT_W], h, t[kTailW];
    uint8_t st;
};
__device__ __forceinline__ Slot slot_load(const Lds& s, uint32_t i) {
    Slot x;
#pragma unroll
    for (int k = 0; k < DHT_W; ++k) x.w[k] = s.w[k * kNN + i];
#pragma unroll
    for (uint32_t k = 0; k < kTailW; ++k) x.t[k] = s.t[k * kNN + i];
    x.h = s.h[i];
    x.st = s.st[i];
    return x;
}
__device__ __forceinline__ void slot_store(const Lds& s, uint32_t i, const Slot& x) {
#pragma unroll
    for (int k = 0; k < DHT_W; ++k) s.w[k * kNN + i] = x.w[k];
#pragma unroll
    for (uint32_t k = 0; k < kTailW; ++k) s.t[k * kNN + i] = x.t[k];
    s.h[i] = x.h;
    s.st[i] = x.st;
}

// rec <= 18 bytes at p packed into kTailW words, byte j in bits 8 (j & 3) of word j >> 2
__device__ __forceinline__ void tail_pack(const uint8_t* p, uint32_t rec, uint32_t* t) {
#pragma unroll
    for (uint32_t k = 0; k < kTailW; ++k) {
        uint32_t x = 0;
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j)
            if (4 * k + j < rec) x |= (uint32_t)p[4 * k + j] << (8 * j);
        t[k] = x;
    }
}

// InfoHash::lowbit (infohash.h:116-130): the position of the last set bit, bit 0 the id's highest; -1 for zero
__device__ __forceinline__ int lowbit5(const uint32_t* f) {
    int r = -1;
#pragma unroll
    for (int k = 0; k < DHT_W; ++k)
        if (f[k]) r = 32 * k + 31 - (int)__builtin_ctz(f[k]);
    return r;
}

// the dense blob -> directory and rows.  Every bucket holds at most kRow nodes (checked by the host).
__device__ void rtg_load(const Lds& s, const RtView& v, const uint32_t* __restrict__ hsrc, const uint8_t* __restrict__ ssrc,
                         uint32_t* __restrict__ hmap) {
    const uint32_t rec = v.alen ? v.alen + 2 : 0;
    for (uint32_t b = threadIdx.x; b < kNB; b += kThreads) {
        const bool in = b < v.nb;
        s.row[b] = b;
        const uint32_t c = in ? v.off[b + 1] - v.off[b] : 0u;
        s.cnt[b] = c <= kRow ? c : 0u;
#pragma unroll
        for (int k = 0; k < DHT_W; ++k) s.first[k * kNB + b] = in ? v.fp[(uint64_t)k * v.nb + b] : 0u;
    }
    if (threadIdx.x == 0) {
        s.misc[0] = v.nb;
        s.misc[1] = s.misc[2] = s.misc[3] = 0;
    }
    for (uint32_t item = threadIdx.x; item < v.nb * kRow; item += kThreads) {
        const uint32_t b = item / kRow, p = item % kRow;
        const uint32_t lo = v.off[b], c = v.off[b + 1] - lo;
        if (p >= c || c > kRow) continue;
        const uint32_t i = lo + p, slot = b * kRow + (c - 1 - p);
        Slot x;
#pragma unroll
        for (int k = 0; k < DHT_W; ++k) x.w[k] = v.np[(uint64_t)k * v.ns + i];
        x.h = hsrc ? hsrc[i] : i;
        x.st = (uint8_t)((v.good[i] ? kStGood : 0) | (ssrc ? ssrc[i] & (kStExpired | kStPending) : 0));
        tail_pack(v.tail + (uint64_t)i * rec, rec, x.t);
        slot_store(s, slot, x);
        if (hsrc && x.h < kRtgMaxHandle) hmap[x.h] = DHT_NONE;   // (an ungrown table's map was cleared by the host)
    }
}

// directory and rows -> the dense planes of d, the handle -> position map, the four status words
__device__ void rtg_store(const Lds& s, const RtgBlob& d, uint32_t alen, const uint32_t* __restrict__ myid,
                          uint32_t* __restrict__ hmap, uint32_t* __restrict__ out_stat) {
    const uint32_t nb = s.misc[0];
    const uint32_t c = threadIdx.x < nb ? s.cnt[threadIdx.x] : 0u;
    uint32_t nn;
    const uint32_t o = block_scan_excl<kThreads>(c, s.wsum, nn);
    if (threadIdx.x < nb) {
        s.off[threadIdx.x] = o;
        d.off[threadIdx.x] = o;
#pragma unroll
        for (int k = 0; k < DHT_W; ++k) d.fp[(uint64_t)k * nb + threadIdx.x] = s.first[k * kNB + threadIdx.x];
    }
    if (threadIdx.x == 0) {
        d.off[nb] = nn;
        out_stat[0] = nb;
        out_stat[1] = nn;
        out_stat[2] = s.misc[1];
        out_stat[3] = s.misc[2];
    }
    if (threadIdx.x < DHT_W) d.myid[threadIdx.x] = myid[threadIdx.x];
    // gpre[b] = good nodes of buckets [0, b): what k_rt_gpre would recount from the planes
    uint32_t g = 0;
    for (uint32_t p = 0; p < c; ++p) g += s.st[s.row[threadIdx.x] * kRow + p] & kStGood;
    uint32_t gtot;
    const uint32_t go = block_scan_excl<kThreads>(g, s.wsum, gtot);   // (its barriers also publish s.off)
    if (threadIdx.x < nb) d.gpre[threadIdx.x] = go;
    if (threadIdx.x == 0) d.gpre[nb] = gtot;
    const uint32_t rec = alen ? alen + 2 : 0;
    for (uint32_t item = threadIdx.x; item < nb * kRow; item += kThreads) {
        const uint32_t b = item / kRow, p = item % kRow, cb = s.cnt[b];
        if (p >= cb) continue;
        const Slot x = slot_load(s, s.row[b] * kRow + (cb - 1 - p));
        const uint32_t i = s.off[b] + p;   // < kNN: nb <= kNB buckets of at most kRow nodes
#pragma unroll
        for (int k = 0; k < DHT_W; ++k) d.np[(uint64_t)k * kNN + i] = x.w[k];
        d.good[i] = x.st & kStGood;
        d.state[i] = x.st;
        d.handle[i] = x.h;
        if (x.h < kRtgMaxHandle) hmap[x.h] = i;
        uint8_t* tp = d.tail + (uint64_t)i * rec;
#pragma unroll
        for (uint32_t k = 0; k < kTailW; ++k)
#pragma unroll
            for (uint32_t j = 0; j < 4; ++j)
                if (4 * k + j < rec) tp[4 * k + j] = (uint8_t)(x.t[k] >> (8 * j));
    }
}

// The batch, by one wave.  Every value but the row's (lanes 0..7) is wave-uniform.
__device__ void rtg_insert_batch(const Lds& s, const uint32_t* my, const RtgBatch& a) {
    const uint32_t lane = lane_id();
    uint32_t nb = s.misc[0], splits = 0;
    bool stopped = false;
    const uint32_t rec = a.alen ? a.alen + 2 : 0;
    Slot mine = {};
    for (uint32_t j = 0; j < a.m; ++j) {
        // 64 nodes of the batch at a time, one per lane (one round trip to memory per 64), each then
        // broadcast to the wave when its turn comes
        if (j % 64 == 0 && j + lane < a.m) {
            const uint32_t i = j + lane;
#pragma unroll
            for (int k = 0; k < DHT_W; ++k) {
                const uint8_t* p = a.ids20 + (uint64_t)i * 20 + 4 * k;
                mine.w[k] = ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3];
            }
            mine.h = a.handles[i];
            mine.st = a.state ? a.state[i] & (kStGood | kStExpired | kStPending) : kStGood;
            tail_pack(a.tail + (uint64_t)i * rec, rec, mine.t);
        }
        const int src = (int)(j % 64);
        Slot n;
#pragma unroll
        for (int k = 0; k < DHT_W; ++k) n.w[k] = (uint32_t)__builtin_amdgcn_readlane((int)mine.w[k], src);
#pragma unroll
        for (uint32_t k = 0; k < kTailW; ++k) n.t[k] = (uint32_t)__builtin_amdgcn_readlane((int)mine.t[k], src);
        n.h = (uint32_t)__builtin_amdgcn_readlane((int)mine.h, src);
        n.st = (uint8_t)__builtin_amdgcn_readlane((int)mine.st, src);
        uint32_t res = kResFull, aux = DHT_NONE;
        if (stopped) res = kResUnapplied;
        else if (!nb) res = kResNone;
        else for (uint32_t round = 0; round < kMaxRounds; ++round) {
            wave_sync();
            aux = DHT_NONE;
            // findBucket: the last bucket b >= 1 with first_b <= id, else bucket 0
            uint32_t jb = 0;
            for (uint32_t base = 0; base < nb; base += 64) {
                const uint32_t b = base + lane;
                bool le = false;
                if (b >= 1 && b < nb) {
                    uint32_t f[DHT_W];
#pragma unroll
                    for (int k = 0; k < DHT_W; ++k) f[k] = s.first[k * kNB + b];
                    le = lex_le(f, n.w);
                }
                const uint64_t mk = __ballot(le);
                if (mk) jb = base + 63u - (uint32_t)__clzll((long long)mk);
            }
            jb = __builtin_amdgcn_readfirstlane(jb);
            const uint32_t r = __builtin_amdgcn_readfirstlane(s.row[jb]), c = __builtin_amdgcn_readfirstlane(s.cnt[jb]);
            const bool in = lane < c;
            const uint32_t sh = in ? s.h[r * kRow + lane] : DHT_NONE;
            const uint32_t ss = in ? s.st[r * kRow + lane] : (uint32_t)kStGood;
            if (__ballot(in && sh == n.h)) {
                res = kResKnown;
                break;
            }
            if (c < kRow) {   // emplace_front: behind the row's last slot
                if (lane == 0) {
                    slot_store(s, r * kRow + c, n);
                    s.cnt[jb] = c + 1;
                }
                res = kResPlaced;
                break;
            }
            const uint64_t ex = __ballot(in && (ss & kStExpired));
            if (ex) {   // the first expired node in list order is overwritten in place
                const uint32_t vl = __builtin_amdgcn_readfirstlane(63u - (uint32_t)__clzll((long long)ex));
                aux = (uint32_t)__builtin_amdgcn_readlane((int)sh, (int)vl);
                if (lane == 0) slot_store(s, r * kRow + vl, n);
                res = kResReplaced;
                break;
            }
            const bool dubious = __ballot(in && !(ss & kStGood)) != 0;
            const uint64_t pk = __ballot(in && !(ss & kStGood) && !(ss & kStPending));
            if (pk) {
                const uint32_t pl = __builtin_amdgcn_readfirstlane(63u - (uint32_t)__clzll((long long)pk));
                aux = (uint32_t)__builtin_amdgcn_readlane((int)sh, (int)pl);
            }
            // contains(b, myid) and depth(b)
            const bool has_next = jb + 1 < nb;
            uint32_t f0[DHT_W], f1[DHT_W];
#pragma unroll
            for (int k = 0; k < DHT_W; ++k) {
                f0[k] = s.first[k * kNB + jb];
                f1[k] = has_next ? s.first[k * kNB + jb + 1] : 0u;
            }
            const bool mybucket = lex_le(f0, my) && (!has_next || lex_lt(my, f1));
            const int lb0 = lowbit5(f0), lb1 = has_next ? lowbit5(f1) : -1;
            const uint32_t depth = (uint32_t)((lb0 > lb1 ? lb0 : lb1) + 1);
            const bool can = (mybucket || ((a.flags & 1u) && depth < 6)) && (!dubious || nb == 1);
            if (!can || depth >= 160) break;   // FULL
            if (nb == kNB) {   // a 257th bucket: this insertion and every later one stay unapplied
                res = kResUnapplied;
                aux = DHT_NONE;
                stopped = true;
                break;
            }
            // split(b): the new bucket's first = first_b with bit depth set
            uint32_t nf[DHT_W];
#pragma unroll
            for (int k = 0; k < DHT_W; ++k) nf[k] = f0[k] | ((uint32_t)k == depth >> 5 ? 0x80000000u >> (depth & 31) : 0u);
            // the directory entries behind b move up by one, top chunk first
            for (uint32_t hi = nb; hi > jb + 1;) {
                const uint32_t lo = hi - (jb + 1) > 64 ? hi - 64 : jb + 1;
                const uint32_t e = lo + lane;
                uint32_t f[DHT_W], er = 0, ec = 0;
                if (e < hi) {
#pragma unroll
                    for (int k = 0; k < DHT_W; ++k) f[k] = s.first[k * kNB + e];
                    er = s.row[e];
                    ec = s.cnt[e];
                }
                wave_sync();
                if (e < hi) {   // e + 1 <= nb < kNB
#pragma unroll
                    for (int k = 0; k < DHT_W; ++k) s.first[k * kNB + e + 1] = f[k];
                    s.row[e + 1] = er;
                    s.cnt[e + 1] = ec;
                }
                wave_sync();
                hi = lo;
            }
            // the nodes: taken from the list's front (the highest slot), each to the front of its side
            Slot x = {};
            bool side = false;
            if (lane < kRow) {
                x = slot_load(s, r * kRow + lane);
                side = lex_le(nf, x.w);
            }
            const uint32_t m1 = (uint32_t)__ballot(lane < kRow && side) & 0xFFu, m0 = ~m1 & 0xFFu;
            wave_sync();
            if (lane < kRow) {
                const uint32_t above = (side ? m1 : m0) >> (lane + 1);
                slot_store(s, (side ? nb : r) * kRow + (uint32_t)__popc(above), x);   // row nb: fresh, nb < kNB
            }
            if (lane == 0) {
                s.cnt[jb] = (uint32_t)__popc(m0);
#pragma unroll
                for (int k = 0; k < DHT_W; ++k) s.first[k * kNB + jb + 1] = nf[k];
                s.row[jb + 1] = nb;
                s.cnt[jb + 1] = (uint32_t)__popc(m1);
            }
            ++nb;
            ++splits;
        }
        if (lane == 0) {
            a.out_res[j] = (uint8_t)res;
            a.out_aux[j] = aux;
        }
    }
    if (lane == 0) {
        s.misc[0] = nb;
        s.misc[1] = splits;
        s.misc[2] = stopped ? 1u : 0u;
    }
}

// Dht::expireBuckets: a wave takes 8 rows at a time, lane = 8 * row + slot; the survivors keep their order
__device__ void rtg_expire_rows(const Lds& s, uint32_t* __restrict__ out_handles) {
    const uint32_t lane = lane_id(), nb = s.misc[0], sl = lane % kRow;
    for (uint32_t base = (threadIdx.x >> 6) * 8; base < nb; base += kThreads / 64 * 8) {
        const uint32_t b = base + lane / kRow;
        const bool in = b < nb && sl < s.cnt[b];
        const uint32_t r = b < nb ? s.row[b] : 0u;
        Slot x = {};
        if (in) x = slot_load(s, r * kRow + sl);
        const bool gone = in && (x.st & kStExpired);
        const uint32_t km = (uint32_t)(__ballot(in && !gone) >> (lane & ~7u)) & 0xFFu;
        if (gone) {
            const uint32_t pos = atomicAdd(&s.misc[3], 1u);
            if (out_handles) out_handles[pos] = x.h;   // pos < nn before the call
        }
        wave_sync();
        if (in && !gone) slot_store(s, r * kRow + (uint32_t)__popc(km & ((1u << sl) - 1u)), x);
        if (b < nb && sl == 0) s.cnt[b] = (uint32_t)__popc(km);
    }
}

template <bool EXPIRE>
__global__ __launch_bounds__(kThreads) void k_rtg(RtView v, const uint32_t* __restrict__ hsrc, const uint8_t* __restrict__ ssrc,
                                                  RtgBlob d, uint32_t* __restrict__ hmap, RtgBatch a,
                                                  uint32_t* __restrict__ out_handles, uint32_t* __restrict__ out_stat) {
    __shared__ uint32_t lds_raw[kLdsBytes / 4];
    const Lds s = lds_carve(lds_raw);
    rtg_load(s, v, hsrc, ssrc, hmap);
    __syncthreads();
    if constexpr (EXPIRE) {
        rtg_expire_rows(s, out_handles);
        __syncthreads();
        if (threadIdx.x == 0) s.misc[2] = s.misc[3];   // the fourth status word: nodes removed
    } else {
        if (threadIdx.x < 64) {
            uint32_t my[DHT_W];
#pragma unroll
            for (int k = 0; k < DHT_W; ++k) my[k] = v.myid[k];
            rtg_insert_batch(s, my, a);
        }
    }
    __syncthreads();
    rtg_store(s, d, v.alen, v.myid, hmap, out_stat);
}

// good / state of every resident node from the bytes of its handle (handles at or past nh: unchanged)
__global__ __launch_bounds__(kThreads) void k_rtg_set_state(const uint32_t* __restrict__ handle, uint32_t nn,
                                                            const uint8_t* __restrict__ by_handle, uint32_t nh,
                                                            uint8_t* __restrict__ good, uint8_t* __restrict__ state) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= nn) return;
    const uint32_t h = handle[i];
    if (h >= nh) return;
    const uint8_t x = by_handle[h] & (kStGood | kStExpired | kStPending);
    good[i] = x & kStGood;
    state[i] = x;
}

// the indexed setter through the handle -> position map
__global__ __launch_bounds__(kThreads) void k_rtg_update(uint8_t* __restrict__ good, uint8_t* __restrict__ state,
                                                         const uint32_t* __restrict__ hmap, const uint32_t* __restrict__ h,
                                                         const uint8_t* __restrict__ val, uint64_t m, bool whole) {
    const uint64_t j = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (j >= m) return;
    const uint32_t i = h[j] < kRtgMaxHandle ? hmap[h[j]] : DHT_NONE;
    if (i >= kNN) return;
    const uint8_t x = whole ? val[j] & (kStGood | kStExpired | kStPending)
                            : (uint8_t)((state[i] & ~kStGood) | (val[j] ? kStGood : 0));
    good[i] = x & kStGood;
    state[i] = x;
}

// K1w's result positions -> handles, in place; DHT_NONE stays
__global__ __launch_bounds__(kThreads) void k_rtg_handles(const uint32_t* __restrict__ handle, uint32_t nn,
                                                          uint32_t* __restrict__ idx, uint64_t m) {
    const uint64_t j = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    if (j >= m) return;
    const uint32_t i = idx[j];
    if (i < nn) idx[j] = handle[i];
}

template <bool EXPIRE>
hipError_t launch_rtg(const RtView& v, const uint32_t* hsrc, const uint8_t* ssrc, const RtgBlob& d, uint32_t* hmap,
                      const RtgBatch& a, uint32_t* out_handles, uint32_t* out_stat, hipStream_t s) {
    if (v.nb > kNB || v.nn > kNN) return hipErrorInvalidValue;
    k_rtg<EXPIRE><<<1, kThreads, 0, s>>>(v, hsrc, ssrc, d, hmap, a, out_handles, out_stat);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_rtg_insert(const RtView& v, const uint32_t* hsrc, const uint8_t* ssrc, const RtgBlob& d, uint32_t* hmap,
                             const RtgBatch& a, uint32_t* out_stat, hipStream_t s) {
    return launch_rtg<false>(v, hsrc, ssrc, d, hmap, a, nullptr, out_stat, s);
}

hipError_t launch_rtg_expire(const RtView& v, const uint32_t* hsrc, const uint8_t* ssrc, const RtgBlob& d, uint32_t* hmap,
                             uint32_t* out_handles, uint32_t* out_stat, hipStream_t s) {
    return launch_rtg<true>(v, hsrc, ssrc, d, hmap, RtgBatch{}, out_handles, out_stat, s);
}

hipError_t launch_rtg_set_state(const RtgBlob& d, uint32_t nn, const uint8_t* by_handle, uint32_t nh, hipStream_t s) {
    if (!nn || !nh) return hipSuccess;
    k_rtg_set_state<<<(nn + kThreads - 1) / kThreads, kThreads, 0, s>>>(d.handle, nn, by_handle, nh, d.good, d.state);
    return hipGetLastError();
}

hipError_t launch_rtg_update(const RtgBlob& d, const uint32_t* hmap, const uint32_t* h, const uint8_t* val, uint64_t m,
                             bool whole, hipStream_t s) {
    if (!m) return hipSuccess;
    k_rtg_update<<<(uint32_t)((m + kThreads - 1) / kThreads), kThreads, 0, s>>>(d.good, d.state, hmap, h, val, m, whole);
    return hipGetLastError();
}

hipError_t launch_rtg_handles(const uint32_t* handle, uint32_t nn, uint32_t* idx, uint64_t m, hipStream_t s) {
    if (!m) return hipSuccess;
    k_rtg_handles<<<(uint32_t)((m + kThreads - 1) / kThreads), kThreads, 0, s>>>(handle, nn, idx, m);
    return hipGetLastError();
}

}  // namespace dhtgpu
