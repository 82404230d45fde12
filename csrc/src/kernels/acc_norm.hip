// gfx950 sum of squares and non-finite count over fp32 accumulators in a remote state space
// (see ocm/acc_norm.h): acc_norm_kernel reads, acc_norm_finish_kernel adds up.
//
// Geometry and addressing are the fused Adam's (optim.hip): grid (gx, count), blockIdx.y picks
// the tensor, each lane owns 4 consecutive words per 16-byte nontemporal load and keeps 4 loads
// in flight before the first use; the tail (n % 4) is done by lane 0 of the tensor's last
// workgroup. kHost: the accumulators are one pinned host-tier extent whose offsets fit 32
// bits, read through a buffer resource on the host grid. Nothing is stored into the
// accumulator space.
//
// Every lane keeps an fp64 sum (the square of an fp32 value is exact in fp64) and an integer
// count. The order of every addition is fixed by the launch shape: a lane's vectors in loop
// order, the 64 lanes of a wave by halving cross-lane moves, the four waves in wave order
// through LDS, then one (double, uint64) partial per (tensor, workgroup) with a plain store.
// The finishing kernel, one workgroup on the same stream, adds a tensor's partials in
// workgroup order, as eight consecutive runs whose sums are then added in run order, and, when
// asked, the per-tensor results of the whole list in index order. No atomics, no fences.
#include <hip/hip_runtime.h>

#include "ocm/acc_norm.h"
#include "state_space.h"

namespace ocm {

namespace {

constexpr int kThreads = kAdamThreads;
constexpr int kV = 4;        // vectors in flight per lane
constexpr int kWave = 64;
constexpr int kWaves = kThreads / kWave;
constexpr int kRuns = 8;     // lanes of the finishing kernel per tensor
static_assert(kRuns * kAdamMaxTensors == kThreads, "one workgroup finishes one launch");

__device__ __forceinline__ void take(float x, double &s, uint64_t &bad) {
    const double d = (double)x;
    s = __builtin_fma(d, d, s);  // d * d is exact: one rounding, the addition's
    bad += acc_norm_nonfinite(__float_as_uint(x)) ? 1u : 0u;
}

template <bool kHost>
__global__ __launch_bounds__(kThreads) void acc_norm_kernel(AccNormArgs a) {
    const uint64_t n = a.n[blockIdx.y], g_off = a.g_off[blockIdx.y];  // uniform: scalar loads from the kernarg segment
    const uint64_t nvec = n >> 2;
    const uint64_t lanes = (uint64_t)gridDim.x * kThreads;
    const uint64_t tid = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    __amdgpu_buffer_rsrc_t rs;
    if constexpr (kHost) rs = host_rsrc(a.space);
    double s = 0.0;
    uint64_t bad = 0;
    for (uint64_t base = tid; base < nvec; base += lanes * kV) {
        f32x4 g[kV];
#pragma unroll
        for (int k = 0; k < kV; k++) {
            const uint64_t i = base + (uint64_t)k * lanes;
            if (i < nvec) {
                if constexpr (kHost)
                    g[k] = host_ld(rs, g_off + (i << 4));
                else
                    g[k] = __builtin_nontemporal_load(reinterpret_cast<const f32x4 *>(state_ptr(a.space, g_off + (i << 4))));
            }
        }
#pragma unroll
        for (int k = 0; k < kV; k++) {
            const uint64_t i = base + (uint64_t)k * lanes;
            if (i < nvec) {
#pragma unroll
                for (int j = 0; j < 4; j++) take(g[k][j], s, bad);
            }
        }
    }
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0)
        for (uint64_t i = nvec << 2; i < n; i++) take(*reinterpret_cast<const float *>(state_ptr(a.space, g_off + 4 * i)), s, bad);
    // the wave: lane l takes lane l + off, off = 32 .. 1; lane 0 ends with the wave's sum
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) {
        s += __shfl_down(s, off, kWave);
        bad += __shfl_down((unsigned long long)bad, off, kWave);
    }
    __shared__ double wave_s[kWaves];
    __shared__ uint64_t wave_bad[kWaves];
    if ((threadIdx.x & (kWave - 1)) == 0) {
        wave_s[threadIdx.x / kWave] = s;
        wave_bad[threadIdx.x / kWave] = bad;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        AccNormPartial p{wave_s[0], wave_bad[0]};
        for (int w = 1; w < kWaves; w++) {
            p.sumsq += wave_s[w];
            p.nonfinite += wave_bad[w];
        }
        a.work[(uint64_t)blockIdx.y * gridDim.x + blockIdx.x] = p;
    }
}

// One workgroup. Lanes 8 t .. 8 t + 7 (one wave holds them all) add tensor t's partials: lane r
// the r-th run of ceil(gx / 8) consecutive workgroups in order, then the runs in order.
__global__ __launch_bounds__(kThreads) void acc_norm_finish_kernel(AccNormFinishArgs f) {
    const uint32_t t = threadIdx.x / kRuns, r = threadIdx.x % kRuns;
    const uint32_t run = (f.gx + kRuns - 1) / kRuns;
    double s = 0.0;
    uint64_t bad = 0;
    if (t < f.count) {
        const AccNormPartial *w = f.work + (uint64_t)t * f.gx;
        const uint32_t x1 = min(f.gx, (r + 1) * run);
        for (uint32_t x = r * run; x < x1; x++) {
            s += w[x].sumsq;
            bad += w[x].nonfinite;
        }
    }
    const int first = (int)(threadIdx.x - r);
    double ts = __shfl(s, first, kWave);
    uint64_t tb = __shfl((unsigned long long)bad, first, kWave);
#pragma unroll
    for (int k = 1; k < kRuns; k++) {
        ts += __shfl(s, first + k, kWave);
        tb += __shfl((unsigned long long)bad, first + k, kWave);
    }
    if (t < f.count && r == 0) {
        f.sumsq[t] = ts;
        f.nonfinite[t] = tb;
    }
    if (!f.totals) return;  // uniform
    // The totals over the whole list in index order: this launch's results (stored above by this
    // workgroup) and those of the launches before it on the stream, a chunk at a time through LDS.
    __shared__ double chunk_s[kThreads];
    __shared__ uint64_t chunk_bad[kThreads];
    __syncthreads();
    s = 0.0;
    bad = 0;
    for (uint32_t c0 = 0; c0 < f.total_count; c0 += kThreads) {
        const uint32_t i = c0 + threadIdx.x;
        if (i < f.total_count) {
            chunk_s[threadIdx.x] = f.all_sumsq[i];
            chunk_bad[threadIdx.x] = f.all_nonfinite[i];
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            const uint32_t m = min((uint32_t)kThreads, f.total_count - c0);
            for (uint32_t j = 0; j < m; j++) {
                s += chunk_s[j];
                bad += chunk_bad[j];
            }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        f.all_sumsq[f.total_count] = s;
        f.all_nonfinite[f.total_count] = bad;
    }
}

}  // namespace

hipError_t acc_norm_launch(const AccNormArgs &a, AccNormFinishArgs f, uint64_t work_bytes, const AdamKnobs &knobs,
                           hipStream_t stream) {
    if (a.count > (uint32_t)kAdamMaxTensors) return hipErrorInvalidValue;
    if (!f.sumsq || !f.nonfinite || (f.totals && (!f.all_sumsq || !f.all_nonfinite))) return hipErrorInvalidValue;
    AccNormShape s{0, false, 0};
    if (a.count) {
        if (!state_space_ok(a.space)) return hipErrorInvalidValue;
        for (uint32_t k = 0; k < a.count; k++)
            if (a.g_off[k] & 15u) return hipErrorInvalidValue;
        s = acc_norm_launch_shape(a.n, a.g_off, a.count, a.space.host != 0, a.space.n_ext, optim_cus(), knobs);
        // every workgroup stores one partial: the workspace must hold them all
        if (s.gx && (!a.work || (uint64_t)s.gx * a.count * sizeof(AccNormPartial) > work_bytes))
            return hipErrorInvalidValue;
    }
    if (s.gx) {
        const auto kernel = s.host ? acc_norm_kernel<true> : acc_norm_kernel<false>;
        const hipError_t e = state_launch(kernel, dim3(s.gx, a.count), stream, a, s.host,
                                          [&](AccNormArgs &x) { x.space.host_span = (uint32_t)s.span; });
        if (e != hipSuccess) return e;
    }
    if (a.count == 0 && !f.totals) return hipSuccess;
    f.work = a.work;
    f.count = a.count;
    f.gx = s.gx;
    hipLaunchKernelGGL(acc_norm_finish_kernel, dim3(1), dim3(kThreads), 0, stream, f);
    return hipGetLastError();
}

}  // namespace ocm
