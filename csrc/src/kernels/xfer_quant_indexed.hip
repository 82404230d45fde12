// Indexed converting one-sided ops: rows of 16-bit elements <-> one MXFP8 or MXFP4 record
// per row, the row on either side picked by index arrays in the local half, one launch
// per list; see ocm/quant_indexed.h for the descriptor and the plan, ocm/indexed.h for
// the bounds rule, ocm/quant_strided.h for the tile rule of a row.
//
// A wave walks a contiguous tile range, as in xfer_indexed_kernel. Entering an op it
// finds the row and piece of its first tile (list_locate of ocm/list.h: the only divide,
// skipped for rows of one tile) and counts from then on. A wave owns whole tiles, so the
// two indices of a tile's row are one value per wave: they are loaded into scalar
// registers when the wave enters a row (enter_row, indexed_row.h: the code
// xfer_indexed_kernel runs), kept while the pieces of that row go by, and loaded again
// when the row number increments. A row with an index outside its table is skipped whole:
// its tiles cost the wave their loop iterations and nothing else, and the wave that owns
// piece 0 of the row counts it, one device-scope atomic add from one lane. A tile of a
// row that moves is located by the shared rule (quant_row_tile) from where the row starts
// on either side, and encoded or decoded by the tile bodies every converting kernel uses
// (quant_tile.h). Index width, record format, element type and direction are wave-uniform
// branches on descriptor fields, not instantiations.
#include <hip/hip_runtime.h>

#include "indexed_row.h"
#include "ocm/mx4.h"
#include "ocm/quant.h"
#include "ocm/quant_indexed.h"
#include "quant_tile.h"
#include "xfer_copy.h"
#include "xfer_host.h"

namespace ocm {

namespace {

// What a wave keeps of its op across the tile bodies, in scalar registers; what only
// entering a row needs is read from the descriptor there (indexed_row.h).
struct OpInLoop {
    uint32_t row_elems, tiles_per_row, put, dtype;
};

template <bool PUT_NT>
__global__ __launch_bounds__(kThreads) void xfer_quant_indexed_kernel(XferQuantIndexedArgs a) {
    __shared__ __attribute__((aligned(16))) uint8_t scale_lds[kWaves][64];
    // wave index, made scalar: everything below but the lane's own vectors is wave-uniform
    const uint32_t wl = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t w = __builtin_amdgcn_readfirstlane(blockIdx.x * kWaves + wl);
    const uint32_t lane = threadIdx.x & 63u;
    uint64_t t, t1;
    list_wave_range(w, a.grid, a.total_tiles, &t, &t1);
    if (t >= t1) return;
    const XferQuantIndexedOp *ops;
    uint32_t i = list_wave_start(a, w, &ops);
    OpInLoop op;                  // of the op of tile t
    uint64_t next = 0;            // first tile of the op after it (none: past every tile)
    uint64_t j = 0;               // tile t is piece k of the op's row j
    uint32_t k = 0;
    uint64_t lrow = 0, rrow = 0;  // where the table row that row j is starts, per side
    bool enter = true;            // row j is new to the wave: its indices are to be loaded
    bool ok = false;              // both indices of row j are inside their tables
    for (; t < t1; t++) {
        if (t >= next) {  // the wave's first tile, or the op's tiles are done: enter the op of tile t
            next = list_enter_op(ops, a.n_ops, t, &i, ListLoadUniform());
            op.row_elems = uniform32(ops[i].row_elems);
            op.tiles_per_row = uniform32(ops[i].tiles_per_row);
            op.put = uniform32(ops[i].put);
            op.dtype = uniform32(ops[i].dtype);
            list_locate(op.tiles_per_row, t - uniform64(ops[i].first_tile), &j, &k);
            j = uniform64(j);
            k = uniform32(k);
            enter = true;
        }
        if (enter) {
            enter = false;
            ok = enter_row(a.lin, ops + i, j, &lrow, &rrow);
            // counted once per row: by the wave that owns its piece 0
            if (!ok && k == 0 && lane == 0) atomicAdd(a.skipped, 1ull);
        }
        if (ok) {
            const QuantTileLoc q = quant_row_tile(lrow, rrow, op.row_elems, k, quant_code_shift(op.dtype));
            quant_tile<PUT_NT>(a, a.lin + q.lin_off, q.codes, q.scales, q.ne, op.dtype, op.put, lane, scale_lds[wl]);
        }
        if (list_next_piece(op.tiles_per_row, &j, &k)) enter = true;
    }
}

}  // namespace

hipError_t xfer_quant_indexed_launch(const XferQuantIndexedArgs &a, const XferTuning &t, hipStream_t stream) {
    if (a.total_tiles == 0 || a.n_ops == 0) return hipSuccess;
    if (!kernels::list_args_valid<true>(a) || !a.lin || !a.skipped) return hipErrorInvalidValue;
    const bool nt = t.nontemporal && !a.host_tier;  // puts store plain into pinned host memory
    hipLaunchKernelGGL(nt ? xfer_quant_indexed_kernel<true> : xfer_quant_indexed_kernel<false>, dim3(a.grid), dim3(kThreads), 0,
                       stream, a);
    hipError_t err = hipGetLastError();
    // the count so far, where the host reads it once the stream has got here (no atomics to host memory)
    if (err == hipSuccess && a.skipped_host)
        err = hipMemcpyAsync(a.skipped_host, a.skipped, sizeof(*a.skipped), hipMemcpyDeviceToHost, stream);
    return err;
}

}  // namespace ocm
