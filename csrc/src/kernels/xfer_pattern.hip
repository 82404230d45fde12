// Verification patterns: benchmarks and tests fill and check data on the device,
// without a host round trip.
#include <hip/hip_runtime.h>

#include "ocm/xfer.h"

namespace ocm {

__device__ __host__ __forceinline__ uint32_t pattern_word(uint64_t i, uint32_t seed) {
    uint64_t x = (i + 1) * 0x9E3779B97F4A7C15ull ^ ((uint64_t)seed << 32 | seed);
    x ^= x >> 31;
    x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 29;
    return (uint32_t)x;
}

namespace {

constexpr int kThreads = 256;

__global__ __launch_bounds__(kThreads) void fill_kernel(uint32_t *p, uint64_t words, uint64_t first, uint32_t seed) {
    for (uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x; i < words; i += (uint64_t)gridDim.x * kThreads)
        p[i] = pattern_word(first + i, seed);
}

__global__ __launch_bounds__(kThreads) void check_kernel(const uint32_t *p, uint64_t words, uint64_t first, uint32_t seed,
                                                         unsigned long long *bad) {
    unsigned long long local = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x; i < words; i += (uint64_t)gridDim.x * kThreads)
        local += p[i] != pattern_word(first + i, seed);
    if (local) atomicAdd(bad, local);
}

}  // namespace

hipError_t pattern_fill(void *p, uint64_t words, uint64_t first_word, uint32_t seed, hipStream_t stream) {
    if (!words) return hipSuccess;
    const uint64_t want = (words + kThreads - 1) / kThreads;
    const unsigned grid = (unsigned)(want < 4096 ? want : 4096);
    hipLaunchKernelGGL(fill_kernel, dim3(grid), dim3(kThreads), 0, stream, static_cast<uint32_t *>(p), words, first_word, seed);
    return hipGetLastError();
}

hipError_t pattern_check(const void *p, uint64_t words, uint64_t first_word, uint32_t seed, unsigned long long *bad_dev,
                         hipStream_t stream) {
    if (!words) return hipSuccess;
    const uint64_t want = (words + kThreads - 1) / kThreads;
    const unsigned grid = (unsigned)(want < 4096 ? want : 4096);
    hipLaunchKernelGGL(check_kernel, dim3(grid), dim3(kThreads), 0, stream, static_cast<const uint32_t *>(p), words,
                       first_word, seed, bad_dev);
    return hipGetLastError();
}

uint32_t pattern_word_host(uint64_t i, uint32_t seed) { return pattern_word(i, seed); }

}  // namespace ocm
