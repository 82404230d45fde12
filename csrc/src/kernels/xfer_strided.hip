// Strided one-sided ops (rows of row_bytes, one stride per side) as one launch of
// wave-granular copies; see ocm/strided.h for the descriptors, the row-relative tile
// geometry and the plan the host makes.
//
// A wave walks a contiguous tile range, as in xfer_batch_kernel. Entering an op it
// finds the row and piece of its first tile there (list_locate of ocm/list.h: the
// only divide, skipped for rows of one tile) and counts from then on. Each tile is
// one or two spans (strided_row_pieces), each inside one stripe unit, copied by the
// shared copy loop (copy_piece of xfer_copy.h). Everything but the lane's own vectors
// is wave-uniform: the descriptor is read through scalar loads, from the kernel
// arguments for short lists.
#include <hip/hip_runtime.h>

#include "ocm/strided.h"
#include "ocm/xfer.h"
#include "xfer_copy.h"
#include "xfer_host.h"

namespace ocm {

namespace {

// The descriptor of an op, in scalar registers (uniform32 / uniform64, xfer_copy.h).
__device__ __forceinline__ XferStridedOp load_op(const XferStridedOp *p) {
    XferStridedOp o;
    o.lin_off = uniform64(p->lin_off);
    o.rem_off = uniform64(p->rem_off);
    o.row_bytes = uniform64(p->row_bytes);
    o.lin_stride = uniform64(p->lin_stride);
    o.rem_stride = uniform64(p->rem_stride);
    o.tiles_per_row = uniform64(p->tiles_per_row);
    o.first_tile = uniform64(p->first_tile);
    o.rows = uniform32(p->rows);
    o.put = uniform32(p->put);
    return o;
}

template <bool NT, bool HOST>
__global__ __launch_bounds__(kThreads) void xfer_strided_kernel(XferStridedArgs a) {
    // wave index, made scalar: everything below but the lane's own vectors is wave-uniform
    const uint32_t w = __builtin_amdgcn_readfirstlane(blockIdx.x * kWaves + (threadIdx.x >> 6));
    uint64_t t, t1;
    list_wave_range(w, a.grid, a.total_tiles, &t, &t1);
    if (t >= t1) return;
    const XferStridedOp *ops;
    uint32_t i = list_wave_start(a, w, &ops);
    XferStridedOp op;       // the op of tile t, in scalar registers
    uint64_t next = 0;       // first tile of the op after it (none: past every tile)
    uint64_t row = 0, k = 0; // tile t is piece k of row `row`
    for (; t < t1; t++) {
        if (t >= next) {  // the wave's first tile, or the op's tiles are done: enter the op of tile t
            next = list_enter_op(ops, a.n_ops, t, &i, ListLoadUniform());
            op = load_op(ops + i);
            list_locate(op.tiles_per_row, t - op.first_tile, &row, &k);
            row = uniform64(row);
            k = uniform64(k);
        }
        StridedPiece p[2];
        const int np = strided_row_pieces(op, row, k, a.n_ext, a.unit_shift, a.tile_shift, p);
        copy_piece<NT, HOST>(a, p[0], op.put);
        if (np == 2) copy_piece<NT, HOST>(a, p[1], op.put);
        list_next_piece(op.tiles_per_row, &row, &k);
    }
}

}  // namespace

hipError_t xfer_strided_launch(const XferStridedArgs &a, const XferTuning &t, hipStream_t stream) {
    if (a.total_tiles == 0 || a.n_ops == 0) return hipSuccess;
    if (!kernels::list_args_valid<false>(a) || !kernels::list_tile_fits_unit(a) || !a.lin) return hipErrorInvalidValue;
    auto kernel = a.host_tier    ? xfer_strided_kernel<true, true>
                  : t.nontemporal ? xfer_strided_kernel<true, false>
                                  : xfer_strided_kernel<false, false>;
    hipLaunchKernelGGL(kernel, dim3(a.grid), dim3(kThreads), 0, stream, a);
    return hipGetLastError();
}

}  // namespace ocm
