// view.hip -- the accept mask's live view: stable stream compaction of the id planes by a
// bitmask (id i = bit (i & 31) of word i >> 5), into planes of their own plus the view -> set
// index map (and, on prefix shards, the view's shifted word-0 plane and the map composed with
// the shard's global index map).  It runs on every mask change, so it is written as an
// HBM-streaming kernel:
//   V1 k_view_count    one wave per 4,096-id tile: popcounts of the tile's 128 mask words (n / 8
//                      bytes read; no id word is read to count)
//   V2 launch_excl_scan (prims.hip)  exclusive scan of the tile counts (one workgroup) + the total
//   V3 k_view_compact  one workgroup per tile.  An accepted id's rank is the tile's offset + the
//                      popcounts of the mask words below it (an LDS prefix over the 128 words, one
//                      barrier per tile) + the popcount of its own word's lower bits: no ballot,
//                      no barrier per 256 ids.  Planes are read with 16-B loads, only where the
//                      four ids' mask nibble is nonzero (a tile whose words are all zero returns
//                      before any load), scattered by rank into an LDS stage of the tile and
//                      written out from there to consecutive addresses, one plane at a time over
//                      two alternating stages (one barrier per plane).
// Algorithmic bytes: 20 n + n / 8 read (less for empty tiles), 24 n_acc written (28 on shards).
#include "dhtgpu_dev.h"
#include "dhtgpu_internal.h"
#include "prims_dev.h"

namespace dhtgpu {
namespace {

constexpr uint32_t kViewThreads = 256;
constexpr uint32_t kViewWords = kTile / 32;   // mask words per tile

// bytes (nonzero = accepted) -> mask words: a lane packs 16 bytes, lane pairs make a word.
// bytes: 32 * nwords of them (the caller zero-pads past n)
__global__ __launch_bounds__(kViewThreads) void k_view_pack(const uint4* __restrict__ bytes, uint64_t nwords,
                                                            uint32_t* __restrict__ bits) {
    const uint64_t g = (uint64_t)blockIdx.x * kViewThreads + threadIdx.x;   // 16-byte group
    uint32_t b = 0;
    if (g < 2 * nwords) {
        const uint4 v = bytes[g];
        const uint32_t x[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) b |= ((x[j] >> (8 * e)) & 0xFFu) ? 1u << (4 * j + e) : 0u;
    }
    const uint32_t hi = __shfl_xor(b, 1);
    if (!(g & 1) && g < 2 * nwords) bits[g >> 1] = b | (hi << 16);
}

// bits past n cleared in the word that holds bit n (the words after it are the caller's, zero)
__global__ void k_view_trim(uint32_t* __restrict__ bits, uint64_t n) {
    if (threadIdx.x == 0 && blockIdx.x == 0 && (n & 31)) bits[n >> 5] &= (1u << (n & 31)) - 1u;
}

__global__ __launch_bounds__(kViewThreads) void k_view_count(const uint2* __restrict__ bits, uint32_t ntiles,
                                                             uint32_t* __restrict__ tcount) {
    const uint32_t tile = blockIdx.x * (kViewThreads / 64) + (threadIdx.x >> 6);
    if (tile >= ntiles) return;   // (wave-uniform)
    const uint2 w = bits[(uint64_t)tile * (kViewWords / 2) + lane_id()];
    const uint32_t c = wave_sum(__popc(w.x) + __popc(w.y));
    if (lane_id() == 0) tcount[tile] = c;
}

struct ViewArgs {
    const uint32_t* planes; uint64_t stride;   // the set (16-B aligned planes: stride % kTile == 0)
    const uint32_t* bits;                      // kViewWords mask words per tile, zero past n
    const uint32_t* toff;                      // exclusive tile offsets (V2)
    uint32_t* out; uint64_t out_stride;        // view planes
    uint32_t* map;                             // view -> set index
    uint32_t* w0s; uint32_t shift;             // nullable: view word 0 << shift | word 1 >> (32 - shift)
    const uint32_t* gidx; uint32_t* gmap;      // nullable: gmap[j] = gidx[map[j]]
};

__global__ __launch_bounds__(kViewThreads) void k_view_compact(const ViewArgs a) {
    __shared__ uint32_t wbits[kViewWords];
    __shared__ uint32_t wpre[kViewWords + 1];
    __shared__ uint32_t wtot0;
    __shared__ uint32_t stage[2][kTile];
    const uint32_t t = threadIdx.x;
    const uint64_t base = (uint64_t)blockIdx.x * kTile;
    if (t < kViewWords) {   // waves 0 and 1: the tile's mask words and their exclusive popcount prefix
        const uint32_t w = a.bits[(uint64_t)blockIdx.x * kViewWords + t];
        const uint32_t pc = __popc(w);
        const uint32_t inc = wave_scan_incl(pc);   // (waves 0 and 1 are whole: kViewWords = 128)
        wbits[t] = w;
        wpre[t] = inc - pc;   // (wave 1: + wave 0's total, below)
        if (t == 63) wtot0 = inc;
        if (t == kViewWords - 1) wpre[kViewWords] = inc;
    }
    __syncthreads();
    const uint32_t add = wtot0;
    const uint32_t cnt = wpre[kViewWords] + add;
    if (cnt == 0) return;   // an empty tile loads nothing (block-uniform)
    const uint64_t o0 = a.toff[blockIdx.x];

    // the thread's four 16-B groups: ids 4 * (t + 256 j) .. + 3 of the tile
    uint32_t nib[4], rank[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint32_t i4 = 4u * (t + kViewThreads * j), wi = i4 >> 5, sh = i4 & 31u;
        const uint32_t w = wbits[wi];
        nib[j] = (w >> sh) & 0xFu;
        rank[j] = wpre[wi] + (wi >= 64 ? add : 0u) + __popc(w & ((1u << sh) - 1u));
    }
    auto load = [&](uint32_t plane, uint4* v) {
        const uint32_t* p = a.planes + (uint64_t)plane * a.stride + base;
#pragma unroll
        for (int j = 0; j < 4; ++j)
            v[j] = nib[j] ? *reinterpret_cast<const uint4*>(p + 4u * (t + kViewThreads * j)) : make_uint4(0, 0, 0, 0);
    };
    auto scatter = [&](uint32_t* st, const uint4* v) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t x[4] = {v[j].x, v[j].y, v[j].z, v[j].w};
            uint32_t r = rank[j];
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (nib[j] >> e & 1u) st[r++] = x[e];
        }
    };

    uint4 cur[4], nxt[4], w0[4];
    load(0, cur);
#pragma unroll
    for (uint32_t w = 0; w < DHT_W; ++w) {
        if (w + 1 < DHT_W) load(w + 1, nxt);   // the next plane's loads in flight over this plane's stage
        if (w == 0 && a.w0s)
            for (int j = 0; j < 4; ++j) w0[j] = cur[j];
        uint32_t* st = stage[w & 1];
        scatter(st, cur);
        __syncthreads();
        uint32_t* dst = a.out + (uint64_t)w * a.out_stride + o0;
        for (uint32_t p = t; p < cnt; p += kViewThreads) dst[p] = st[p];
        if (w == 1 && a.w0s) {   // word 0 is still in registers beside word 1
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                w0[j].x = (w0[j].x << a.shift) | (cur[j].x >> (32u - a.shift));
                w0[j].y = (w0[j].y << a.shift) | (cur[j].y >> (32u - a.shift));
                w0[j].z = (w0[j].z << a.shift) | (cur[j].z >> (32u - a.shift));
                w0[j].w = (w0[j].w << a.shift) | (cur[j].w >> (32u - a.shift));
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) cur[j] = nxt[j];
    }
    // stage 5: the set indices; stage 6: the shifted word 0 (a stage is free again once the
    // barrier after the next stage's scatter has passed)
    {
        uint32_t* st = stage[1];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            uint32_t r = rank[j];
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (nib[j] >> e & 1u) st[r++] = (uint32_t)(base + 4u * (t + kViewThreads * j) + e);
        }
        __syncthreads();
        for (uint32_t p = t; p < cnt; p += kViewThreads) {
            const uint32_t i = st[p];
            a.map[o0 + p] = i;
            if (a.gmap) a.gmap[o0 + p] = a.gidx[i];
        }
    }
    if (a.w0s) {
        uint32_t* st = stage[0];
        scatter(st, w0);
        __syncthreads();
        for (uint32_t p = t; p < cnt; p += kViewThreads) a.w0s[o0 + p] = st[p];
    }
}

__global__ __launch_bounds__(kViewThreads) void k_view_add(const uint32_t* __restrict__ map, uint64_t m, uint32_t base,
                                                           uint32_t* __restrict__ out) {
    for (uint64_t i = (uint64_t)blockIdx.x * kViewThreads + threadIdx.x; i < m; i += (uint64_t)gridDim.x * kViewThreads)
        out[i] = map[i] + base;
}

inline uint32_t grid_for(uint64_t n) {
    const uint64_t g = (n + kViewThreads - 1) / kViewThreads;
    return (uint32_t)(g > 65535ull * 32 ? 65535ull * 32 : g ? g : 1);
}

}  // namespace

uint64_t view_mask_words(uint64_t stride) { return stride / 32; }

hipError_t launch_view_pack(const uint8_t* bytes, uint64_t nwords, uint32_t* bits, hipStream_t s) {
    if (!nwords) return hipSuccess;
    k_view_pack<<<grid_for(2 * nwords), kViewThreads, 0, s>>>(reinterpret_cast<const uint4*>(bytes), nwords, bits);
    return hipGetLastError();
}

hipError_t launch_view_trim(uint32_t* bits, uint64_t n, hipStream_t s) {
    if (!(n & 31)) return hipSuccess;
    k_view_trim<<<1, 64, 0, s>>>(bits, n);
    return hipGetLastError();
}

hipError_t launch_view_count(const uint32_t* bits, uint64_t stride, uint32_t* toff, unsigned long long* d_total,
                             hipStream_t s) {
    const uint32_t ntiles = (uint32_t)(stride / kTile);
    if (!ntiles) return hipMemsetAsync(d_total, 0, 8, s);
    k_view_count<<<(ntiles + kViewThreads / 64 - 1) / (kViewThreads / 64), kViewThreads, 0, s>>>(
        reinterpret_cast<const uint2*>(bits), ntiles, toff);
    return launch_excl_scan(toff, toff, 1, ntiles, d_total, s);
}

hipError_t launch_view_compact(const uint32_t* planes, uint64_t stride, const uint32_t* bits, const uint32_t* toff,
                               uint32_t* out, uint64_t out_stride, uint32_t* map, uint32_t* w0s, uint32_t shift,
                               const uint32_t* gidx, uint32_t* gmap, hipStream_t s) {
    const uint32_t ntiles = (uint32_t)(stride / kTile);
    if (!ntiles) return hipSuccess;
    if (shift == 0 || shift >= 32) w0s = nullptr;
    const ViewArgs a{planes, stride, bits, toff, out, out_stride, map, w0s, shift, gidx, gidx ? gmap : nullptr};
    k_view_compact<<<ntiles, kViewThreads, 0, s>>>(a);
    return hipGetLastError();
}

hipError_t launch_view_add(const uint32_t* map, uint64_t m, uint32_t base, uint32_t* out, hipStream_t s) {
    if (!m) return hipSuccess;
    k_view_add<<<grid_for(m), kViewThreads, 0, s>>>(map, m, base, out);
    return hipGetLastError();
}

}  // namespace dhtgpu
