// A state space (ocm/state_space.h) from a kernel: addressing, the buffer accesses of a space in
// the pinned host tier, and what the launchers of optim.hip, optim_rows.hip and acc_norm.hip share.
#pragma once
#include <hip/hip_runtime.h>

#include "ocm/optim.h"
#include "ocm/state_space.h"

namespace ocm {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// Where byte x of a state space lies: state_place's dispatch, written out so that each branch
// loads its own extent base. One load of ext[index] after the branches join (state_place itself)
// changes the kernels' vector register counts. `s` is read in place, in the kernarg segment: a
// copy of ext[] would put the dynamically indexed array in scratch (xfer_copy.h).
__device__ __forceinline__ char *state_ptr(const StateSpace &s, uint64_t x) {
    if (s.n_ext == 1) return s.ext[0] + x;
    if (state_units_fit32(s.unit_shift, x)) {
        const StatePlace p = state_place32(s.n_ext, s.unit_shift, x);
        return s.ext[p.index] + p.off;
    }
    const StatePlace p = state_place64(s.n_ext, s.unit_shift, x);
    return s.ext[p.index] + p.off;
}

// ---- a space in the pinned host tier, one extent whose offsets fit 32 bits ----
// PCIe, not HBM, bounds this: the state streams in and out over one x16 Gen5
// link at once. Buffer loads/stores on the extent (uniform base, 32-bit lane
// offsets) so the stores can carry sc1 (write-through), which streams into host
// memory faster than nontemporal or plain stores (profiles/pcie_stream_r03.json:
// 57.0 vs 55.5 GB/s).
constexpr int kAuxNT = 2, kAuxSC1 = 16;  // cache-policy bits of buffer accesses on gfx950

__device__ __forceinline__ __amdgpu_buffer_rsrc_t host_rsrc(const StateSpace &s) {
    return __builtin_amdgcn_make_buffer_rsrc(s.ext[0], 0, (int)s.host_span, 0x00020000);
}

__device__ __forceinline__ f32x4 host_ld(__amdgpu_buffer_rsrc_t r, uint64_t off) {
    return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r, (int)(uint32_t)off, 0, kAuxNT));
}

__device__ __forceinline__ void host_st(__amdgpu_buffer_rsrc_t r, uint64_t off, f32x4 x) {
    typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, x), r, (int)(uint32_t)off, 0, kAuxSC1);
}

// Launches workgroups of kAdamThreads on `grid`; the host variants (`host`) get their arguments
// with each space's host_span filled by set_spans (below 2^32, or the launch shape is not `host`).
template <class Args, class SetSpans>
hipError_t state_launch(void (*kernel)(Args), dim3 grid, hipStream_t stream, Args a, bool host, SetSpans set_spans) {
    if (host) set_spans(a);
    hipLaunchKernelGGL(kernel, grid, dim3(kAdamThreads), 0, stream, a);
    return hipGetLastError();
}

}  // namespace ocm
