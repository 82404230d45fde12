// One-sided accumulate: remote fp32 += scale * local (fp32, bf16 or fp16), one launch
// per list; see ocm/acc.h for the plan and the element rule (two roundings, never an fma).
//
// A wave-tile is 1024 elements in op-relative coordinates: 256 accumulator vectors of
// 16 bytes, of which lane l owns l, l + 64, l + 128 and l + 192, so every load and store
// of the wave is contiguous. A tile's addresses are formed first (with several extents
// stripe_ptr reads an extent base per lane from the kernel arguments; the four reads share
// one wait), then the four remote loads and the four local loads (16 bytes for fp32
// elements, 8 for 16-bit ones) are issued with nothing between them, in a full tile and
// in a partial one: a tile pays one read round trip to the pool. Every remote vector is
// mapped through the extents on its own: offsets are multiples of 16 and a stripe unit is
// at least 16 bytes, so no vector straddles a unit, wherever a tile crosses one. Lanes past
// a partial tile's end neither load nor store; a partial tile finishes its vectors one
// after the other, and the compiler's wait in front of each also covers the store before
// it. No LDS, no atomics: a lane reads and writes only its own vectors.
#include <hip/hip_runtime.h>

#include "ocm/acc.h"
#include "xfer_copy.h"
#include "xfer_host.h"

namespace ocm {

namespace {

typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
// Both halves are global memory; saying so keeps every access a global_ one (a generic pointer that
// reaches a load through two paths becomes a flat_ access, which waits on two counters).
typedef __attribute__((address_space(1))) u32x4 *GlobalVec;

constexpr uint32_t kAccTileVecs = kAccTileElems / 4;  // accumulator vectors of a tile
constexpr int kAccVecs = kAccTileVecs / 64;           // ... of which a lane owns this many

// The local elements that go with one accumulator vector.
template <uint32_t DT>
struct LocalVec {
    using T = u32x2;  // four 16-bit elements
    static constexpr uint32_t kBytes = 8;
    static __device__ __forceinline__ float elem(const T &v, int j) {
        const uint32_t w = v[j >> 1];
        return acc_widen16((j & 1) ? (w >> 16) : (w & 0xffffu), DT == kAccBf16);
    }
};
template <>
struct LocalVec<kAccF32> {
    using T = u32x4;
    static constexpr uint32_t kBytes = 16;
    static __device__ __forceinline__ float elem(const T &v, int j) { return acc_bits_float(v[j]); }
};

template <uint32_t DT>
__device__ __forceinline__ typename LocalVec<DT>::T load_local(const char *lin, uint32_t v) {
    using T = typename LocalVec<DT>::T;
    return __builtin_nontemporal_load((const __attribute__((address_space(1))) T *)(lin + (uint64_t)LocalVec<DT>::kBytes * v));
}

// One accumulator vector: the rule on its four elements, then the store.
template <uint32_t DT, bool NT>
__device__ __forceinline__ void acc_vec(GlobalVec rp, const u32x4 &r, const typename LocalVec<DT>::T &x, float scale) {
    u32x4 o;
#pragma unroll
    for (int j = 0; j < 4; j++) o[j] = acc_float_bits(acc_rule(acc_bits_float(r[j]), LocalVec<DT>::elem(x, j), scale));
    if constexpr (NT)
        __builtin_nontemporal_store(o, rp);
    else
        *rp = o;
}

// Vectors K.. of a partial tile. A lane that owns vector K + 1 owns vector K, so the conditions
// nest: the loads are issued on the way in, nothing between them, and each vector is finished
// on the way out. (Four branches side by side made the compiler merge loaded and unloaded
// registers after each one, with a wait in front of every next pair of loads.)
template <uint32_t DT, bool NT, int K>
__device__ __forceinline__ void acc_partial(const GlobalVec (&rp)[kAccVecs], const char *lin, uint32_t nv, float scale,
                                            uint32_t lane) {
    const uint32_t v = lane + 64u * K;
    if (v < nv) {
        const u32x4 r = __builtin_nontemporal_load(rp[K]);
        const typename LocalVec<DT>::T x = load_local<DT>(lin, v);
        if constexpr (K + 1 < kAccVecs) acc_partial<DT, NT, K + 1>(rp, lin, nv, scale, lane);
        acc_vec<DT, NT>(rp[K], r, x, scale);
    }
}

// One tile: `nv` accumulator vectors (1..256) at striped offset `rem`, their elements at
// `lin`. FULL: nv == 256, no lane is masked.
template <uint32_t DT, bool NT, bool FULL>
__device__ __forceinline__ void acc_tile(const XferBatchArgs &a, const char *lin, uint64_t rem, uint32_t nv, float scale,
                                         uint32_t lane) {
    GlobalVec rp[kAccVecs];
    // Addresses first: with several extents stripe_ptr reads an extent base per lane, and the
    // four reads share one wait here instead of one in front of each data load. (Lanes past
    // the end of a partial tile map vector 0 and touch nothing.)
    const uint32_t n_ext = a.n_ext;  // kernel argument: uniform
    if (n_ext == 1) {
#pragma unroll
        for (int k = 0; k < kAccVecs; k++) rp[k] = (GlobalVec)stripe_ptr(a, 1u, 0u, rem + 16ull * (lane + 64u * k));
    } else {
        __builtin_assume(n_ext > 1);
#pragma unroll
        for (int k = 0; k < kAccVecs; k++) {
            const uint32_t v = lane + 64u * k;
            rp[k] = (GlobalVec)stripe_ptr(a, n_ext, a.unit_shift, rem + 16ull * ((FULL || v < nv) ? v : 0u));
        }
    }
    if constexpr (FULL) {
        // the eight data loads, nothing between them
        u32x4 r[kAccVecs];
        typename LocalVec<DT>::T x[kAccVecs];
#pragma unroll
        for (int k = 0; k < kAccVecs; k++) {
            r[k] = __builtin_nontemporal_load(rp[k]);
            x[k] = load_local<DT>(lin, lane + 64u * k);
        }
#pragma unroll
        for (int k = 0; k < kAccVecs; k++) acc_vec<DT, NT>(rp[k], r[k], x[k], scale);
    } else {
        acc_partial<DT, NT, 0>(rp, lin, nv, scale, lane);
    }
}

template <uint32_t DT, bool NT>
__device__ __forceinline__ void acc_tile_any(const XferBatchArgs &a, const char *lin, uint64_t rem, uint32_t nv, float scale,
                                             uint32_t lane) {
    if (nv == kAccTileVecs)  // wave-uniform
        acc_tile<DT, NT, true>(a, lin, rem, nv, scale, lane);
    else
        acc_tile<DT, NT, false>(a, lin, rem, nv, scale, lane);
}

template <bool NT>
__global__ __launch_bounds__(kThreads) void xfer_acc_kernel(XferBatchArgs a) {
    // wave index, made scalar: everything below but the lane's own vectors is wave-uniform
    const uint32_t wl = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t w = __builtin_amdgcn_readfirstlane(blockIdx.x * kWaves + wl);
    const uint32_t lane = threadIdx.x & 63u;
    uint64_t t, t1;
    list_wave_range(w, a.grid, a.total_tiles, &t, &t1);
    if (t >= t1) return;
    const XferBatchOp *ops;
    uint32_t i = list_wave_start(a, w, &ops);
    for (; t < t1; t++) {
        while (i + 1 < a.n_ops && uniform64(ops[i + 1].first_tile) <= t) i++;
        const XferBatchOp &op = ops[i];
        // the descriptor's fields, made scalar (ops[] may be read with vector loads)
        const uint32_t elems = uniform32((uint32_t)op.len), dtype = uniform32(op.pad);
        const uint64_t lin_off = uniform64(op.lin_off), rem_off = uniform64(op.rem_off);
        const uint32_t e0 = uniform32((uint32_t)(t - op.first_tile)) << kAccTileShift;  // elems < 2^31
        const uint32_t left = elems - e0;
        const uint32_t nv = (left < kAccTileElems ? left : kAccTileElems) >> 2;
        const float scale = acc_bits_float(uniform32(op.put));
        const uint64_t rem = rem_off + 4ull * e0;
        const char *lin = a.lin + lin_off;
        if (dtype == kAccF32)
            acc_tile_any<kAccF32, NT>(a, lin + 4ull * e0, rem, nv, scale, lane);
        else if (dtype == kAccBf16)
            acc_tile_any<kAccBf16, NT>(a, lin + 2ull * e0, rem, nv, scale, lane);
        else
            acc_tile_any<kAccFp16, NT>(a, lin + 2ull * e0, rem, nv, scale, lane);
    }
}

}  // namespace

hipError_t xfer_acc_launch(const XferBatchArgs &a, const XferTuning &t, hipStream_t stream) {
    if (a.total_tiles == 0 || a.n_ops == 0) return hipSuccess;
    if (!kernels::list_args_valid<true>(a) || a.abs_lin) return hipErrorInvalidValue;  // lin_off is an offset here
    const bool nt = t.nontemporal && !a.host_tier;
    hipLaunchKernelGGL(nt ? xfer_acc_kernel<true> : xfer_acc_kernel<false>, dim3(a.grid), dim3(kThreads), 0, stream, a);
    return hipGetLastError();
}

}  // namespace ocm
