// Indexed one-sided ops (rows picked on either side by index arrays in the local half)
// as one launch of wave-granular copies; see ocm/indexed.h for the descriptors, the
// bounds rule and the plan the host makes, ocm/strided.h for the row-relative tile
// geometry both kernels share.
//
// A wave walks a contiguous tile range, as in xfer_strided_kernel. Entering an op it
// finds the row and piece of its first tile (list_locate of ocm/list.h: the only divide,
// skipped for rows of one tile) and counts from then on. A wave owns whole tiles, so the two
// indices of a tile's row are one value per wave: they are loaded into scalar registers
// (uniform32 / uniform64) when the wave enters a row, kept while the pieces of that row
// go by, and loaded again when the row number increments. A row with an index outside
// its table is skipped whole (indexed_in_range): its tiles cost the wave their loop
// iterations and nothing else, and the wave that owns piece 0 of the row counts it, one
// device-scope atomic add from one lane. Whether the arrays hold int32 or int64 is a
// wave-uniform branch on a descriptor field, not another instantiation.
//
// The index arrays are read as they are when the kernel runs. A torch kernel may have
// written them just before: ocm_stream_wait orders this launch after it, as for any
// data of the local half.
#include <hip/hip_runtime.h>

#include "indexed_row.h"
#include "ocm/indexed.h"
#include "ocm/xfer.h"
#include "xfer_copy.h"
#include "xfer_host.h"

namespace ocm {

namespace {

// What a wave keeps of its op across the copy loops, in scalar registers (uniform32 /
// uniform64, xfer_copy.h). The fields that only entering a row needs (enter_row,
// indexed_row.h) are read from the descriptor there, in the kernel arguments or in L2,
// beside the index loads they would wait for anyway: kept live as well, they cost
// register spills.
struct OpInLoop {
    uint64_t row_bytes, tiles_per_row;
    uint32_t put;
};

template <bool NT, bool HOST>
__global__ __launch_bounds__(kThreads) void xfer_indexed_kernel(XferIndexedArgs a) {
    // wave index, made scalar: everything below but the lane's own vectors is wave-uniform
    const uint32_t w = __builtin_amdgcn_readfirstlane(blockIdx.x * kWaves + (threadIdx.x >> 6));
    uint64_t t, t1;
    list_wave_range(w, a.grid, a.total_tiles, &t, &t1);
    if (t >= t1) return;
    const XferIndexedOp *ops;
    uint32_t i = list_wave_start(a, w, &ops);
    OpInLoop op;                  // of the op of tile t
    uint64_t next = 0;            // first tile of the op after it (none: past every tile)
    uint64_t j = 0, k = 0;        // tile t is piece k of the op's row j
    uint64_t lrow = 0, rrow = 0;  // first byte of the table row that row j is, per side
    bool enter = true;            // row j is new to the wave: its indices are to be loaded
    bool ok = false;              // both indices of row j are inside their tables
    for (; t < t1; t++) {
        if (t >= next) {  // the wave's first tile, or the op's tiles are done: enter the op of tile t
            next = list_enter_op(ops, a.n_ops, t, &i, ListLoadUniform());
            op.row_bytes = uniform64(ops[i].row_bytes);
            op.tiles_per_row = uniform64(ops[i].tiles_per_row);
            op.put = uniform32(ops[i].put);
            list_locate(op.tiles_per_row, t - uniform64(ops[i].first_tile), &j, &k);
            j = uniform64(j);
            k = uniform64(k);
            enter = true;
        }
        if (enter) {
            enter = false;
            ok = enter_row(a.lin, ops + i, j, &lrow, &rrow);
            // counted once per row: by the wave that owns its piece 0
            if (!ok && k == 0 && (threadIdx.x & 63) == 0) atomicAdd(a.skipped, 1ull);
        }
        if (ok) {
            StridedPiece p[2];
            const int np = strided_pieces_at(lrow, rrow, op.row_bytes, k, a.n_ext, a.unit_shift, a.tile_shift, p);
            copy_piece<NT, HOST>(a, p[0], op.put);
            if (np == 2) copy_piece<NT, HOST>(a, p[1], op.put);
        }
        if (list_next_piece(op.tiles_per_row, &j, &k)) enter = true;
    }
}

}  // namespace

hipError_t xfer_indexed_launch(const XferIndexedArgs &a, const XferTuning &t, hipStream_t stream) {
    if (a.total_tiles == 0 || a.n_ops == 0) return hipSuccess;
    if (!kernels::list_args_valid<false>(a) || !kernels::list_tile_fits_unit(a) || !a.lin || !a.skipped)
        return hipErrorInvalidValue;
    auto kernel = a.host_tier    ? xfer_indexed_kernel<true, true>
                  : t.nontemporal ? xfer_indexed_kernel<true, false>
                                  : xfer_indexed_kernel<false, false>;
    hipLaunchKernelGGL(kernel, dim3(a.grid), dim3(kThreads), 0, stream, a);
    hipError_t err = hipGetLastError();
    // the count so far, where the host reads it once the stream has got here (no atomics to host memory)
    if (err == hipSuccess && a.skipped_host)
        err = hipMemcpyAsync(a.skipped_host, a.skipped, sizeof(*a.skipped), hipMemcpyDeviceToHost, stream);
    return err;
}

}  // namespace ocm
