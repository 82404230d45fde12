// Indexed converting one-sided ops (ocm_copy_onesided_quant_indexed): `rows` rows of
// `row_elems` 16-bit elements out of a table in the local half, one MXFP8 or MXFP4 record
// (ocm/mx8.h, ocm/mx4.h) per row out of a table of records in the remote half, the row on
// either side picked by an index array that lives in the local half. By definition the
// call is the ocm_copy_onesided_quant list with one op per in-range row, so a plain or
// strided converting get can read what an indexed put wrote.
//
// Nothing here is a rule of its own. Which rows move, and what happens to the others,
// is ocm/indexed.h's: indexed_in_range on either index, the row skipped whole and counted
// once, the validator's table and index-array checks (indexed_check_table,
// indexed_check_index_array) with the bytes a row has on each side (2 * row_elems local,
// quant_record_bytes remote). Where a tile of a picked row lies is ocm/quant_strided.h's
// quant_row_tile, from the row's two start offsets. The list is planned as every
// descriptor list is (ocm/list.h): tile t of an op is piece t % tiles_per_row of its row
// t / tiles_per_row, whatever rows the indices pick.
//
// Out of scope: transfer plans and hipGraph capture, the copy service,
// index-times-stride (layer-major) ops, a defined result for duplicate destination rows,
// and scatter-add.
//
// This header is what the kernel (xfer_quant_indexed.hip), the host side
// (quant_indexed.cpp) and the stand-alone test program (ocm_quant_indexed_tests.cpp)
// share; it needs no HIP.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdio>

#include "ocm/indexed.h"
#include "ocm/list.h"
#include "ocm/quant_strided.h"
#include "oncillamem.h"

namespace ocm {

// What XferQuantStridedOp and XferIndexedOp carry, once.
struct XferQuantIndexedOp {
    uint64_t lin_off;        // first element of row 0 of the local table (bytes)
    uint64_t rem_off;        // first byte of the record of row 0 of the remote table, striped coordinates
    uint64_t lin_stride;     // bytes between rows of the local table
    uint64_t rem_stride;     // bytes between records of the remote table
    uint64_t first_tile;     // exclusive prefix sum of the ops' tile counts (rows * tiles_per_row)
    uint64_t lin_idx_off;    // byte offset in the local half of the local-side indices, or OCM_INDEX_NONE
    uint64_t rem_idx_off;    // same, remote-side indices
    uint32_t row_elems;      // a multiple of 32 below 2^31
    uint32_t rows;           // rows moved: entries of each index array
    uint32_t tiles_per_row;  // ceil(row_elems / kQuantTileElems)
    uint32_t put;            // 1: encode local -> remote, 0: decode remote -> local
    uint32_t dtype;          // enum ocm_quant_dtype | enum ocm_quant_format
    uint32_t lin_rows;       // rows the local table has
    uint32_t rem_rows;       // rows the remote table has
    uint32_t index_type;     // enum ocm_index_type
};
static_assert(sizeof(XferQuantIndexedOp) == 88, "indexed converting op layout");
static_assert(sizeof(struct ocm_quant_indexed_params) == 96, "ocm_quant_indexed_params layout");

// Tiles of an op (0 for an empty one): rows < 2^32 times tiles_per_row < 2^20.
OCM_QS_HD inline uint64_t quant_indexed_tile_count(const XferQuantIndexedOp &op) { return (uint64_t)op.rows * op.tiles_per_row; }

// Piece k of the op's row that table rows lr / rr are (both in range): exactly tile k of
// the plain converting op (lin_off + lr * lin_stride, rem_off + rr * rem_stride, row_elems).
OCM_QS_HD inline QuantTileLoc quant_indexed_tile(const XferQuantIndexedOp &op, uint64_t lr, uint64_t rr, uint32_t k,
                                                 uint32_t code_shift) {
    return quant_row_tile(op.lin_off + lr * op.lin_stride, op.rem_off + rr * op.rem_stride, op.row_elems, k, code_shift);
}

#if !defined(__HIP_DEVICE_COMPILE__)
// One op against halves of local_bytes / remote_bytes. 0: fine (*src = the 16-bit bytes
// its rows name, *wire = their record bytes, both nominal: every row counts, in range or
// not; 0 for an empty op); -1: `why` says what is wrong, naming the side. No sum or
// product here can overflow: the table and index-array checks are indexed.h's division
// forms, and a table that passed them holds rows that do not overlap inside a half, so
// rows * row bytes fits.
inline int quant_indexed_check_op(const struct ocm_quant_indexed_params &p, uint64_t local_bytes, uint64_t remote_bytes,
                                  uint64_t *src, uint64_t *wire, char *why, size_t why_len) {
    *src = *wire = 0;
    if (quant_check_dtype(p.dtype, why, why_len) != 0) return -1;
    if (p.reserved != 0) {
        std::snprintf(why, why_len, "reserved is %u (0 is needed)", p.reserved);
        return -1;
    }
    if (p.row_elems % kMx8Group != 0 || p.row_elems >= (1ull << 31)) {
        std::snprintf(why, why_len, "rows of %llu elements (a multiple of 32 below 2^31 is needed)",
                      (unsigned long long)p.row_elems);
        return -1;
    }
    if (p.rows == 0 || p.row_elems == 0) return 0;  // does nothing, whatever else it says
    if (indexed_check_kind(p.index_type, p.local_index_offset, p.remote_index_offset, why, why_len) != 0) return -1;
    const IndexedSide sides[2] = {
        {"local", p.local_offset, p.local_stride, local_bytes, p.local_rows, p.local_index_offset, 2 * p.row_elems},
        {"remote", p.remote_offset, p.remote_stride, remote_bytes, p.remote_rows, p.remote_index_offset,
         quant_record_bytes(p.row_elems, p.dtype)}};
    if (indexed_check_counts(p.rows, sides, why, why_len) != 0) return -1;
    const uint64_t align[2] = {16, 32};
    for (int i = 0; i < 2; i++) {
        const IndexedSide &s = sides[i];
        if (s.off % align[i] != 0) {
            std::snprintf(why, why_len, "%s offset %llu is not a multiple of %llu", s.side, (unsigned long long)s.off,
                          (unsigned long long)align[i]);
            return -1;
        }
        if (s.stride % align[i] != 0) {
            std::snprintf(why, why_len, "%s stride %llu is not a multiple of %llu", s.side, (unsigned long long)s.stride,
                          (unsigned long long)align[i]);
            return -1;
        }
    }
    for (const auto &s : sides)
        if (indexed_check_table(s, p.rows, why, why_len) != 0) return -1;
    for (const auto &s : sides)
        if (s.idx_off != OCM_INDEX_NONE &&
            indexed_check_index_array(s, p.index_type, p.rows, local_bytes, p.op_flag == 0, sides[0], why, why_len) != 0)
            return -1;
    // rows < 2^32, row bytes < 2^32
    *src = p.rows * sides[0].row_bytes;
    *wire = p.rows * sides[1].row_bytes;
    return 0;
}

// The device descriptor of a checked op (an empty op keeps no rows and no elements, so
// it has no tiles whatever its other fields say).
inline XferQuantIndexedOp quant_indexed_op(const struct ocm_quant_indexed_params &p) {
    const bool empty = p.rows == 0 || p.row_elems == 0;
    XferQuantIndexedOp o{};
    o.lin_off = p.local_offset;
    o.rem_off = p.remote_offset;
    o.lin_stride = p.local_stride;
    o.rem_stride = p.remote_stride;
    o.lin_idx_off = p.local_index_offset;
    o.rem_idx_off = p.remote_index_offset;
    o.row_elems = empty ? 0 : (uint32_t)p.row_elems;
    o.rows = empty ? 0 : (uint32_t)p.rows;
    o.put = p.op_flag != 0;
    o.dtype = p.dtype;
    o.lin_rows = empty ? 0 : (uint32_t)p.local_rows;
    o.rem_rows = empty ? 0 : (uint32_t)p.remote_rows;
    o.index_type = p.index_type;
    return o;
}

// Row j of a checked op as the host path moves it, the indices read from the local half
// at `base` (host memory): true, and *q is the plain converting op the row is; false:
// an index is outside its table and the row is skipped.
inline bool quant_indexed_host_row(const struct ocm_quant_indexed_params &p, const char *base, uint64_t j,
                                   struct ocm_quant_params *q) {
    const uint64_t lr = p.local_index_offset != OCM_INDEX_NONE ? indexed_load_host(base, p.local_index_offset, p.index_type, j) : j;
    const uint64_t rr = p.remote_index_offset != OCM_INDEX_NONE ? indexed_load_host(base, p.remote_index_offset, p.index_type, j) : j;
    if (!indexed_in_range(lr, p.local_rows) || !indexed_in_range(rr, p.remote_rows)) return false;
    // in range, and the table fits its half (quant_indexed_check_op): neither product can overflow
    *q = {p.local_offset + lr * p.local_stride, p.remote_offset + rr * p.remote_stride, p.row_elems, p.op_flag, p.dtype};
    return true;
}
#endif

// ---- launch (xfer_quant_indexed.hip) ----
// ops carried in the kernarg segment: the most that fit it beside the head and the two skip pointers
constexpr int kQuantIndexedInlineOps = 45;

// tile_shift is kQuantTileShift (tiles are cut in elements)
struct XferQuantIndexedArgs : ListArgs<XferQuantIndexedOp, kQuantIndexedInlineOps> {
    unsigned long long *skipped;       // device word: rows skipped, counted up (the allocation's, shared with the indexed op)
    unsigned long long *skipped_host;  // pinned host word the launcher copies it to after the kernel (the kernel reads neither)
};
static_assert(list_args_fit<XferQuantIndexedArgs>, "kernarg segment limit");
static_assert(sizeof(XferQuantIndexedArgs) + sizeof(XferQuantIndexedOp) > kKernargLimit, "one more inline op would fit");

// Host-side plan: fills tiles_per_row and first_tile, returns total tiles.
inline uint64_t xfer_quant_indexed_plan(XferQuantIndexedOp *ops, uint32_t n, uint32_t /*tile_shift*/) {
    return list_plan(ops, n, [](XferQuantIndexedOp &op) {
        op.tiles_per_row = quant_strided_tiles_per_row(op.row_elems);
        return quant_indexed_tile_count(op);
    });
}

}  // namespace ocm
