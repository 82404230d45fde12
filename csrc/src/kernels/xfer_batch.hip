// Batched one-sided ops (scatter/gather lists) as one launch of wave-granular
// copies; see ocm/xfer.h for the plan the host makes and the kernel walks.
#include <hip/hip_runtime.h>

#include <cstring>

#include "ocm/xfer.h"
#include "xfer_copy.h"
#include "xfer_host.h"

namespace ocm {

namespace {

constexpr uint32_t kBatchTileShift = 12;  // 4 KiB per wave-tile: one round of WaveCopy (xfer_copy.h)

// HOST: the host-tier shape. Its puts were meant to store write-through (sc1) into
// the pinned host extents, as the PCIe streaming kernel does (57.0 vs 55.5 GB/s),
// but pointer stores carry no sc1 bit: they are plain stores, whatever NT says.
// (Making them write-through is an open measurement: docs/DESIGN.md.)
template <bool NT, bool HOST = false>
__global__ __launch_bounds__(kThreads) void xfer_batch_kernel(XferBatchArgs a) {
    // wave index, made scalar: everything below is wave-uniform
    const uint32_t w = __builtin_amdgcn_readfirstlane(blockIdx.x * kWaves + (threadIdx.x >> 6));
    uint64_t t, t1;
    list_wave_range(w, a.grid, a.total_tiles, &t, &t1);
    if (t >= t1) return;
    const XferBatchOp *ops;
    uint32_t i = list_wave_start(a, w, &ops);
    for (; t < t1; t++) {
        while (i + 1 < a.n_ops && ops[i + 1].first_tile <= t) i++;
        const XferBatchOp &op = ops[i];
        char *lin = a.abs_lin ? reinterpret_cast<char *>(static_cast<uintptr_t>(op.lin_off)) : a.lin + op.lin_off;
        TileSpan sp = tile_span_of(a, a.n_ext, a.unit_shift, a.tile_shift, lin, op.rem_off, op.len, op.put,
                                   t - op.first_tile, xfer_first_tile(op.rem_off, a.tile_shift));
        if (HOST && op.put)
            copy_span<WaveCopy<false>>(sp.dst, sp.src, sp.n);
        else
            copy_span<WaveCopy<NT>>(sp.dst, sp.src, sp.n);
    }
}

// The host-tier kernel for host-tier batches (OCM_BATCH_HOST_SC1=0: the generic kernel).
bool host_sc1() {
    static const bool on = kernels::env_int("OCM_BATCH_HOST_SC1", 1) != 0;
    return on;
}

using BatchKernel = void (*)(XferBatchArgs);

BatchKernel batch_kernel_for(const XferBatchArgs &a, const XferTuning &t) {
    if (a.host_tier && host_sc1()) return xfer_batch_kernel<true, true>;
    return t.nontemporal ? xfer_batch_kernel<true> : xfer_batch_kernel<false>;
}

}  // namespace

uint32_t xfer_batch_tile_shift(uint32_t n_ext, uint32_t unit_shift) {
    return (n_ext > 1 && unit_shift < kBatchTileShift) ? unit_shift : kBatchTileShift;
}

uint32_t xfer_batch_grid(uint64_t total_tiles, bool host_tier) {
    // One wave per tile until the chip holds 8 workgroups (32 waves) per CU.
    const uint64_t want = (total_tiles + kWaves - 1) / kWaves;
    // Host tier: 128 workgroups; 4096-block KV swaps 48.0-48.1 /
    // 48.8-49.9 GiB/s out/in against 46.8-46.9 / 47.5-48.1 with the HBM shape
    // (profiles/kv_swap_host_r03.json; the PCIe ceiling is ~53).
    static const int host_grid = kernels::env_int("OCM_BATCH_HOST_GRID", 128);
    const uint64_t cap = host_tier && host_grid > 0 ? (uint64_t)host_grid : (uint64_t)kernels::num_cus() * 8;
    return (uint32_t)(want < cap ? (want ? want : 1) : cap);
}

hipError_t xfer_batch_launch(const XferBatchArgs &a, const XferTuning &t, hipStream_t stream) {
    if (a.total_tiles == 0 || a.n_ops == 0) return hipSuccess;
    if (!kernels::list_args_valid<false>(a)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(batch_kernel_for(a, t), dim3(a.grid), dim3(kThreads), 0, stream, a);
    return hipGetLastError();
}

hipError_t xfer_batch_graph_node(hipGraph_t graph, hipGraphNode_t dep, const XferBatchArgs &a, const XferTuning &t,
                                 hipGraphNode_t *node) {
    const size_t ndep = dep ? 1 : 0;
    if (a.total_tiles == 0 || a.n_ops == 0) return hipGraphAddEmptyNode(node, graph, dep ? &dep : nullptr, ndep);
    if (!kernels::list_args_valid<false>(a)) return hipErrorInvalidValue;
    // Parameters by address: `a` must outlive the graph (the plan's stage
    // storage), whether or not the runtime copies them into the node.
    void *params[] = {const_cast<XferBatchArgs *>(&a)};
    hipKernelNodeParams kp;
    std::memset(&kp, 0, sizeof(kp));
    kp.func = reinterpret_cast<void *>(batch_kernel_for(a, t));
    kp.gridDim = dim3(a.grid);
    kp.blockDim = dim3(kThreads);
    kp.sharedMemBytes = 0;
    kp.kernelParams = params;
    kp.extra = nullptr;
    return hipGraphAddKernelNode(node, graph, dep ? &dep : nullptr, ndep, &kp);
}

}  // namespace ocm
