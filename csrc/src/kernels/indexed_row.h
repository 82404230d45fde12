// How a wave of the indexed kernels (xfer_indexed.hip, xfer_quant_indexed.hip) enters a
// row: both indices into scalar registers, the bounds rule (indexed_in_range of
// ocm/indexed.h), and where the row starts on either side. `Op` is the kind's descriptor
// (XferIndexedOp, XferQuantIndexedOp): the fields read here have one name in both. They
// are read from the descriptor when a row is entered, in the kernel arguments or in L2,
// beside the index loads they would wait for anyway: kept live across the tile loop as
// well, they cost register spills. Device only: include from a HIP translation unit,
// inside no namespace.
#pragma once
#include <hip/hip_runtime.h>

#include "ocm/indexed.h"
#include "xfer_copy.h"

namespace ocm {

namespace {

// The table row that entry j of the index array at `idx_off` of the local half picks
// (no array: row j itself), widened for indexed_in_range. One value per wave.
__device__ __forceinline__ uint64_t row_of(const char *lin, uint64_t idx_off, uint32_t index_type, uint64_t j) {
    if (idx_off == OCM_INDEX_NONE) return j;
    if (index_type == OCM_INDEX_I64) return uniform64(*reinterpret_cast<const uint64_t *>(lin + idx_off + (j << 3)));
    return indexed_widen32(uniform32(*reinterpret_cast<const uint32_t *>(lin + idx_off + (j << 2))));
}

// The wave enters row j of op *d: both indices, the bounds rule, and where the row starts
// on either side. False: the row is skipped (*lrow / *rrow are then not to be used).
template <class Op>
__device__ __forceinline__ bool enter_row(const char *lin, const Op *d, uint64_t j, uint64_t *lrow, uint64_t *rrow) {
    const uint32_t type = uniform32(d->index_type);
    const uint64_t lr = row_of(lin, uniform64(d->lin_idx_off), type, j);
    const uint64_t rr = row_of(lin, uniform64(d->rem_idx_off), type, j);
    // in range, and the table fits its half (the kind's validator): neither product can overflow
    *lrow = uniform64(d->lin_off) + lr * uniform64(d->lin_stride);
    *rrow = uniform64(d->rem_off) + rr * uniform64(d->rem_stride);
    return indexed_in_range(lr, uniform32(d->lin_rows)) && indexed_in_range(rr, uniform32(d->rem_rows));
}

}  // namespace

}  // namespace ocm
