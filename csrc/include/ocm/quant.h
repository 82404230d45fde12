// Converting one-sided ops (ocm_copy_onesided_quant): a put reads 16-bit elements
// from the linear side and writes an MXFP8 record (ocm/mx8.h) into the striped
// side, a get reads the record and widens it. One launch serves a whole list,
// planned like a batch (ocm/xfer.h): the list is cut into wave-tiles of
// kQuantTileElems elements, the host prefix-sums each op's tile count into
// `first_tile`, and every wave walks a contiguous tile range.
//
// The descriptors are XferBatchOp records read differently: len counts elements,
// rem_off is the record's first byte (codes, then the scale bytes), pad holds the
// element type (enum ocm_quant_dtype). XferBatchArgs carries them unchanged
// (tile_shift is unused), so large lists take the batch path's staged upload.
#pragma once
#include "ocm/mx8.h"
#include "ocm/xfer.h"

namespace ocm {

// Fills first_tile (quant_tile_count of ocm/mx8.h per op), returns total tiles.
inline uint64_t xfer_quant_plan(XferBatchOp *ops, uint32_t n) {
    return list_plan(ops, n, [](const XferBatchOp &op) { return quant_tile_count(op.len); });
}
// a.grid from xfer_batch_grid, a.wave_op from list_wave_ops (large lists).
// Stores: nontemporal (t.nontemporal), except that puts into a pool wholly in the
// pinned host tier (a.host_tier) store plain, as the batch kernel's host shape does.
hipError_t xfer_quant_launch(const XferBatchArgs &a, const XferTuning &t, hipStream_t stream);

// Strided converting lists (ocm/quant_strided.h: the descriptor, the row-relative tile
// rule and the host plan): one launch, one record per row; stores as above.
struct XferQuantStridedArgs;
hipError_t xfer_quant_strided_launch(const XferQuantStridedArgs &a, const XferTuning &t, hipStream_t stream);

// Indexed converting lists (ocm/quant_indexed.h: the descriptor and the host plan;
// ocm/indexed.h: the bounds rule): one launch, one record per picked row; stores as above.
// a.skipped: a device word the kernel counts skipped rows into, copied to a.skipped_host
// after the kernel.
struct XferQuantIndexedArgs;
hipError_t xfer_quant_indexed_launch(const XferQuantIndexedArgs &a, const XferTuning &t, hipStream_t stream);

}  // namespace ocm
