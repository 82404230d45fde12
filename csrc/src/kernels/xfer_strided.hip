// Strided one-sided ops (rows of row_bytes, one stride per side) as one launch of
// wave-granular copies; see ocm/strided.h for the descriptors, the row-relative tile
// geometry and the plan the host makes.
//
// A wave walks a contiguous tile range, as in xfer_batch_kernel. Entering an op it
// finds the row and piece of its first tile there (strided_locate: the only divide,
// skipped for rows of one tile) and counts from then on. Each tile is one or two
// spans (strided_row_pieces), each inside one stripe unit, copied by the shared
// copy loop. Everything but the lane's own vectors is wave-uniform: the descriptor
// is read through scalar loads, from the kernel arguments for short lists.
#include <hip/hip_runtime.h>

#include "ocm/strided.h"
#include "ocm/xfer.h"
#include "xfer_copy.h"
#include "xfer_host.h"

namespace ocm {

static_assert(sizeof(XferStridedArgs::ext) == sizeof(XferBatchArgs::ext), "extent table of a pair");

namespace {

constexpr int kStridedUnroll = 4;  // 64 lanes x 16 B x 4 in flight: one 4 KiB wave-tile a round

template <bool NT>
using WaveCopy = CopyCfg<64, kStridedUnroll, PointerAccess<NT>>;

// One span, inside one stripe unit. HOST: every extent is pinned host memory; puts
// store plain there, as the batch kernel's do.
template <bool NT, bool HOST>
__device__ __forceinline__ void copy_piece(const XferStridedArgs &a, const StridedPiece &p, uint32_t put) {
    char *lp = a.lin + p.lin_off;
    char *rp = stripe_ptr(a, a.n_ext, a.unit_shift, p.rem_off);
    if (put) {
        if (HOST)
            copy_span<WaveCopy<false>>(rp, lp, p.n);
        else
            copy_span<WaveCopy<NT>>(rp, lp, p.n);
    } else {
        copy_span<WaveCopy<NT>>(lp, rp, p.n);
    }
}

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
            for (;;) {
                next = i + 1 < a.n_ops ? uniform64(ops[i + 1].first_tile) : ~0ull;
                if (next > t) break;
                i++;
            }
            op = load_op(ops + i);
            strided_locate(op, t - op.first_tile, &row, &k);
            row = uniform64(row);
            k = uniform64(k);
        }
        StridedPiece p[2];
        const int np = strided_row_pieces(op, row, k, a.n_ext, a.unit_shift, a.tile_shift, p);
        copy_piece<NT, HOST>(a, p[0], op.put);
        if (np == 2) copy_piece<NT, HOST>(a, p[1], op.put);
        if (++k == op.tiles_per_row) {
            k = 0;
            row++;
        }
    }
}

}  // namespace

hipError_t xfer_strided_launch(const XferStridedArgs &a, const XferTuning &t, hipStream_t stream) {
    if (a.total_tiles == 0 || a.n_ops == 0) return hipSuccess;
    if (!kernels::list_args_valid<false, false>(a, kStridedInlineOps) || !a.lin) return hipErrorInvalidValue;
    // a tile is at most one stripe unit (two spans a tile at the most)
    if (a.tile_shift > 63 || (a.n_ext > 1 && a.tile_shift > a.unit_shift)) return hipErrorInvalidValue;
    auto kernel = a.host_tier    ? xfer_strided_kernel<true, true>
                  : t.nontemporal ? xfer_strided_kernel<true, false>
                                  : xfer_strided_kernel<false, false>;
    hipLaunchKernelGGL(kernel, dim3(a.grid), dim3(kThreads), 0, stream, a);
    return hipGetLastError();
}

}  // namespace ocm
