// prims_dev.h -- the small device building blocks every kernel family shares (gfx950, wave64):
// the wave scan and sum, and the one exclusive scan by a workgroup (a value per thread, or an
// array strip-mined over it).  Their launchers for whole arrays are prims.hip.
#pragma once
#include "dhtgpu_dev.h"

namespace dhtgpu {

// Inclusive scan over the 64 lanes of a wave with DPP (no LDS): row_shr 1/2/4/8 inside each
// 16-lane row, then row_bcast 15 / 31 across rows.  Lanes whose DPP source is out of range
// take `old` = 0.  Needs the whole wave active.
__device__ __forceinline__ uint32_t wave_scan_incl(uint32_t x) {
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x111, 0xF, 0xF, false);   // row_shr:1
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x112, 0xF, 0xF, false);   // row_shr:2
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x114, 0xF, 0xF, false);   // row_shr:4
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x118, 0xF, 0xF, false);   // row_shr:8
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x142, 0xA, 0xF, false);   // row_bcast:15
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x143, 0xC, 0xF, false);   // row_bcast:31
    return x;
}

// the sum over the 64 lanes of a wave, in every lane
__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// Exclusive scan over the NT threads of a block, in registers: returns the sum of v over the
// threads below this one, total = the sum over the block.  Every thread must call it (whole waves,
// two barriers).  wsum: NT / 64 + 1 words of LDS scratch, free again on return.  Each wave scans
// its lanes, the waves' sums cross through wsum, and every wave scans those sums for itself.
template <int NT>
__device__ __forceinline__ uint32_t block_scan_excl(uint32_t v, uint32_t* wsum, uint32_t& total) {
    constexpr uint32_t NW = NT / 64;
    static_assert(NT % 64 == 0 && NW >= 1 && NW <= 64, "whole waves, at most 64 of them");
    const uint32_t lane = lane_id(), w = threadIdx.x >> 6;
    const uint32_t x = wave_scan_incl(v);
    if (lane == 63) wsum[w] = x;
    __syncthreads();
    const uint32_t s = lane < NW ? wsum[lane] : 0u;
    const uint32_t xs = wave_scan_incl(s);
    if (threadIdx.x == NW - 1) wsum[NW] = xs;
    const uint32_t before = (uint32_t)__builtin_amdgcn_readlane((int)(xs - s), __builtin_amdgcn_readfirstlane((int)w));
    __syncthreads();
    total = wsum[NW];
    return before + x - v;
}

// Exclusive scan of in[0, len) into out[0, len) by a block of NT threads (out == in: in place),
// NT entries at a time with a carry; returns the total.  The arrays are global memory or LDS;
// thread t takes entries t, t + NT, ...  Every thread must call it.  It ends without a barrier: on
// return a thread may read the entries it wrote, and the others' after the block's next barrier.
// wsum: as for block_scan_excl.
template <int NT>
__device__ __forceinline__ uint32_t block_scan_array(const uint32_t* in, uint32_t* out, uint32_t len, uint32_t* wsum) {
    uint32_t carry = 0;
    for (uint32_t b = 0; b < len; b += NT) {
        const uint32_t i = b + threadIdx.x;
        const uint32_t v = i < len ? in[i] : 0u;
        uint32_t tot;
        const uint32_t e = block_scan_excl<NT>(v, wsum, tot);
        if (i < len) out[i] = carry + e;
        carry += tot;
    }
    return carry;
}

}  // namespace dhtgpu
