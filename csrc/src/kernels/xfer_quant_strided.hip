// Strided converting one-sided ops: rows of 16-bit elements <-> one MXFP8 or MXFP4 record per
// row, one launch per list; see ocm/quant_strided.h for the descriptor, the
// row-relative tile rule and the plan the host makes.
//
// A wave walks a contiguous tile range, as in xfer_quant_kernel. Entering an op it
// finds the row and piece of its first tile there (list_locate of ocm/list.h: the only
// divide, skipped for rows of one tile) and counts from then on. Each tile is located
// by the shared rule (quant_strided_tile) and then encoded or decoded by the tile
// bodies the converting kernel uses (quant_tile.h). Everything but the lane's own
// vectors is wave-uniform: the descriptor is read through scalar loads, from the
// kernel arguments for short lists.
#include <hip/hip_runtime.h>

#include "ocm/mx4.h"
#include "ocm/quant.h"
#include "ocm/quant_strided.h"
#include "quant_tile.h"
#include "xfer_copy.h"
#include "xfer_host.h"

namespace ocm {

namespace {

// The descriptor of an op, in scalar registers (uniform32 / uniform64, xfer_copy.h).
__device__ __forceinline__ XferQuantStridedOp load_op(const XferQuantStridedOp *p) {
    XferQuantStridedOp o;
    o.lin_off = uniform64(p->lin_off);
    o.rem_off = uniform64(p->rem_off);
    o.lin_stride = uniform64(p->lin_stride);
    o.rem_stride = uniform64(p->rem_stride);
    o.first_tile = uniform64(p->first_tile);
    o.row_elems = uniform32(p->row_elems);
    o.rows = uniform32(p->rows);
    o.tiles_per_row = uniform32(p->tiles_per_row);
    o.put = uniform32(p->put);
    o.dtype = uniform32(p->dtype);
    o.pad = 0;
    return o;
}

template <bool PUT_NT>
__global__ __launch_bounds__(kThreads) void xfer_quant_strided_kernel(XferQuantStridedArgs a) {
    __shared__ __attribute__((aligned(16))) uint8_t scale_lds[kWaves][64];
    // wave index, made scalar: everything below but the lane's own vectors is wave-uniform
    const uint32_t wl = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t w = __builtin_amdgcn_readfirstlane(blockIdx.x * kWaves + wl);
    const uint32_t lane = threadIdx.x & 63u;
    uint64_t t, t1;
    list_wave_range(w, a.grid, a.total_tiles, &t, &t1);
    if (t >= t1) return;
    const XferQuantStridedOp *ops;
    uint32_t i = list_wave_start(a, w, &ops);
    XferQuantStridedOp op;  // the op of tile t, in scalar registers
    uint64_t next = 0;      // first tile of the op after it (none: past every tile)
    uint64_t row = 0;       // tile t is piece k of row `row`
    uint32_t k = 0;
    for (; t < t1; t++) {
        if (t >= next) {  // the wave's first tile, or the op's tiles are done: enter the op of tile t
            next = list_enter_op(ops, a.n_ops, t, &i, ListLoadUniform());
            op = load_op(ops + i);
            list_locate(op.tiles_per_row, t - op.first_tile, &row, &k);
            row = uniform64(row);
            k = uniform32(k);
        }
        const QuantTileLoc q = quant_strided_tile(op, row, k, quant_code_shift(op.dtype));  // log2(elements per code byte)
        quant_tile<PUT_NT>(a, a.lin + q.lin_off, q.codes, q.scales, q.ne, op.dtype, op.put, lane, scale_lds[wl]);
        list_next_piece(op.tiles_per_row, &row, &k);
    }
}

}  // namespace

hipError_t xfer_quant_strided_launch(const XferQuantStridedArgs &a, const XferTuning &t, hipStream_t stream) {
    if (a.total_tiles == 0 || a.n_ops == 0) return hipSuccess;
    if (!kernels::list_args_valid<true>(a) || !a.lin) return hipErrorInvalidValue;
    const bool nt = t.nontemporal && !a.host_tier;
    hipLaunchKernelGGL(nt ? xfer_quant_strided_kernel<true> : xfer_quant_strided_kernel<false>, dim3(a.grid), dim3(kThreads), 0,
                       stream, a);
    return hipGetLastError();
}

}  // namespace ocm
