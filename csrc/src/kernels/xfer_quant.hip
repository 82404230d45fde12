// Converting one-sided ops: bf16 / fp16 <-> MXFP8 or MXFP4 records (ocm/mx8.h, ocm/mx4.h)
// as the bytes cross to the remote half, one launch per list; see ocm/quant.h for the
// plan. The tile bodies (put_tile, get_tile and their _mx4 forms) are in quant_tile.h,
// shared with xfer_quant_strided.hip; an op's format, like its element type, is a
// wave-uniform branch. What follows describes the MXFP8 tile; quant_tile.h has both.
//
// A wave-tile is 2048 elements, done in two rounds of 1024. In a round lane l owns
// elements [16 l, 16 l + 16): two 16-byte vectors of source, one 16-byte vector of
// codes, so code stores (puts) and code loads (gets) are whole vectors, contiguous
// across the wave. A group of 32 elements is a lane pair; its amax is one
// __shfl_xor away. Every 16-byte vector of the record is mapped through the
// extents on its own (stripe_ptr): the record starts on a 32-byte boundary and
// stripe units are at least 16 bytes, so no vector straddles a unit, wherever the
// codes or the scale bytes cross one. A tile's 64 scale bytes are gathered in LDS
// (wave-private, 64 bytes) and leave as four vectors; a partial tile's last
// vector goes byte by byte.
#include <hip/hip_runtime.h>

#include "ocm/mx4.h"
#include "ocm/quant.h"
#include "quant_tile.h"
#include "xfer_copy.h"
#include "xfer_host.h"

namespace ocm {

namespace {

template <bool PUT_NT>
__global__ __launch_bounds__(kThreads) void xfer_quant_kernel(XferBatchArgs a) {
    __shared__ __attribute__((aligned(16))) uint8_t scale_lds[kWaves][64];
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
        while (i + 1 < a.n_ops && ops[i + 1].first_tile <= t) i++;
        const XferBatchOp &op = ops[i];
        const uint32_t e0 = (uint32_t)(t - op.first_tile) << kQuantTileShift;  // elems < 2^31
        const uint32_t left = (uint32_t)op.len - e0;
        const uint32_t ne = left < kQuantTileElems ? left : kQuantTileElems;
        char *lin = a.lin + op.lin_off + 2ull * e0;
        const uint32_t cs = quant_code_shift(op.pad);  // elements per code byte, log2
        const uint64_t codes = op.rem_off + (e0 >> cs), scales = op.rem_off + (op.len >> cs) + (e0 >> 5);
        quant_tile<PUT_NT>(a, lin, codes, scales, ne, op.pad, op.put, lane, scale_lds[wl]);
    }
}

}  // namespace

hipError_t xfer_quant_launch(const XferBatchArgs &a, const XferTuning &t, hipStream_t stream) {
    if (a.total_tiles == 0 || a.n_ops == 0) return hipSuccess;
    if (!kernels::list_args_valid<true>(a) || a.abs_lin) return hipErrorInvalidValue;  // lin_off is an offset here
    const bool nt = t.nontemporal && !a.host_tier;
    hipLaunchKernelGGL(nt ? xfer_quant_kernel<true> : xfer_quant_kernel<false>, dim3(a.grid), dim3(kThreads), 0, stream, a);
    return hipGetLastError();
}

}  // namespace ocm
