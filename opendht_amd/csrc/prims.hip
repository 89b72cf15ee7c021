// prims.hip -- the shared primitives' launchers (prims_dev.h holds the device forms): the exclusive
// scan of short arrays by one workgroup per row, and the indexed bit / byte setters behind the
// families' update entry points.  None is on the k-NN hot path.
#include "dhtgpu_internal.h"
#include "prims_dev.h"

namespace dhtgpu {
namespace {

constexpr uint32_t kScanThreads = 1024;
constexpr uint32_t kSetThreads = 256;

template <class T>
__global__ __launch_bounds__(kScanThreads) void k_scan_rows(const uint32_t* in, uint32_t* out, uint32_t len,
                                                            T* __restrict__ tot) {
    __shared__ uint32_t wsum[kScanThreads / 64 + 1];
    const uint64_t row = (uint64_t)blockIdx.x * len;
    const uint32_t total = block_scan_array<kScanThreads>(in + row, out + row, len, wsum);
    if (threadIdx.x == 0) tot[blockIdx.x] = total;
}

__global__ __launch_bounds__(kSetThreads) void k_bits_update(uint32_t* __restrict__ bits, const uint32_t* __restrict__ idx,
                                                             const uint8_t* __restrict__ val, uint64_t m) {
    for (uint64_t j = (uint64_t)blockIdx.x * kSetThreads + threadIdx.x; j < m; j += (uint64_t)gridDim.x * kSetThreads) {
        const uint32_t i = idx[j], bit = 1u << (i & 31);
        if (val[j]) atomicOr(bits + (i >> 5), bit);
        else atomicAnd(bits + (i >> 5), ~bit);
    }
}

__global__ __launch_bounds__(kSetThreads) void k_bytes_update(uint8_t* __restrict__ bytes, const uint32_t* __restrict__ idx,
                                                              const uint8_t* __restrict__ val, uint64_t m, bool normalise) {
    for (uint64_t j = (uint64_t)blockIdx.x * kSetThreads + threadIdx.x; j < m; j += (uint64_t)gridDim.x * kSetThreads)
        bytes[idx[j]] = normalise ? val[j] != 0 : val[j];
}

inline uint32_t set_grid(uint64_t m) {
    const uint64_t g = (m + kSetThreads - 1) / kSetThreads;
    return (uint32_t)(g > 65535ull * 32 ? 65535ull * 32 : g);
}

template <class T>
hipError_t scan_rows(const uint32_t* in, uint32_t* out, uint32_t rows, uint32_t len, T* tot, hipStream_t s) {
    if (!rows) return hipSuccess;
    k_scan_rows<T><<<rows, kScanThreads, 0, s>>>(in, out, len, tot);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_excl_scan(const uint32_t* in, uint32_t* out, uint32_t rows, uint32_t len, uint32_t* tot, hipStream_t s) {
    return scan_rows(in, out, rows, len, tot, s);
}

hipError_t launch_excl_scan(const uint32_t* in, uint32_t* out, uint32_t rows, uint32_t len, unsigned long long* tot,
                            hipStream_t s) {
    return scan_rows(in, out, rows, len, tot, s);
}

hipError_t launch_bits_update(uint32_t* bits, const uint32_t* idx, const uint8_t* val, uint64_t m, hipStream_t s) {
    if (!m) return hipSuccess;
    k_bits_update<<<set_grid(m), kSetThreads, 0, s>>>(bits, idx, val, m);
    return hipGetLastError();
}

hipError_t launch_bytes_update(uint8_t* bytes, const uint32_t* idx, const uint8_t* val, uint64_t m, bool normalise,
                               hipStream_t s) {
    if (!m) return hipSuccess;
    k_bytes_update<<<set_grid(m), kSetThreads, 0, s>>>(bytes, idx, val, m, normalise);
    return hipGetLastError();
}

}  // namespace dhtgpu
