// Strided converting one-sided ops (ocm_copy_onesided_quant_strided): `rows` rows of
// `row_elems` 16-bit elements on the local side, one MXFP8 or MXFP4 record (ocm/mx8.h,
// ocm/mx4.h: the row's codes, then its scale bytes) per row on the remote side, one stride per side. By
// definition the call is the ocm_copy_onesided_quant list with one op per row, so a
// plain converting get can read one row of what a strided put wrote. One launch serves
// a whole list, planned as every descriptor list is (ocm/list.h); one descriptor per op
// is all the kernel reads, whatever the number of rows.
//
// Tiles are cut in row-relative coordinates, as the strided copy cuts them
// (ocm/strided.h): every row has ceil(row_elems / kQuantTileElems) tiles, tile t of an
// op is row t / tiles_per_row, piece t % tiles_per_row, and piece k holds the row's
// elements [k << kQuantTileShift, min((k + 1) << kQuantTileShift, row_elems)). A tile
// never spans two rows: each row's scale bytes lie behind its own codes.
//
// This header is the arithmetic the kernel (xfer_quant_strided.hip), the host side
// (quant_strided.cpp) and the stand-alone test program (ocm_quant_strided_tests.cpp)
// share; it needs no HIP.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdio>

#include "ocm/list.h"
#include "ocm/mx4.h"
#include "oncillamem.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define OCM_QS_HD __host__ __device__
#else
#define OCM_QS_HD
#endif

namespace ocm {

struct XferQuantStridedOp {
    uint64_t lin_off;        // first element of row 0 in the linear buffer (bytes)
    uint64_t rem_off;        // first byte of row 0's record in striped coordinates
    uint64_t lin_stride;     // bytes from one row's start to the next, linear side
    uint64_t rem_stride;     // bytes from one row's record to the next, striped side
    uint64_t first_tile;     // exclusive prefix sum of the ops' tile counts (rows * tiles_per_row)
    uint32_t row_elems;      // a multiple of 32 below 2^31
    uint32_t rows;
    uint32_t tiles_per_row;  // ceil(row_elems / kQuantTileElems)
    uint32_t put;            // 1: encode lin -> striped, 0: decode striped -> lin
    uint32_t dtype;          // enum ocm_quant_dtype | enum ocm_quant_format
    uint32_t pad;
};
static_assert(sizeof(XferQuantStridedOp) == 64, "strided converting op layout");

// Where one tile lies: its elements in the linear buffer, its codes and its scale bytes
// in striped coordinates, and how many elements it holds (a multiple of 32, at most
// kQuantTileElems).
struct QuantTileLoc {
    uint64_t lin_off, codes, scales;
    uint32_t ne;
};

OCM_QS_HD inline uint32_t quant_strided_tiles_per_row(uint64_t row_elems) { return (uint32_t)quant_tile_count(row_elems); }

// Tiles of an op (0 for an empty one): rows < 2^32 times tiles_per_row < 2^20.
OCM_QS_HD inline uint64_t quant_strided_tile_count(const XferQuantStridedOp &op) {
    return (uint64_t)op.rows * op.tiles_per_row;
}

// THE tile rule of a row: piece k of the row of `row_elems` elements that starts at byte
// `lrow` of the linear buffer and whose record starts at `rec` in striped coordinates,
// exactly the tile (k) of the plain converting op (lrow, rec, row_elems). code_shift: log2
// of the elements a code byte of the op's format holds (quant_code_shift). Which row that
// is comes from the caller: strides (quant_strided_tile) or index arrays
// (ocm/quant_indexed.h).
OCM_QS_HD inline QuantTileLoc quant_row_tile(uint64_t lrow, uint64_t rec, uint32_t row_elems, uint32_t k, uint32_t code_shift) {
    const uint32_t e0 = k << kQuantTileShift;  // row_elems < 2^31
    const uint32_t left = row_elems - e0;
    QuantTileLoc q;
    q.ne = left < kQuantTileElems ? left : kQuantTileElems;
    q.lin_off = lrow + 2ull * e0;
    q.codes = rec + (e0 >> code_shift);
    q.scales = rec + (row_elems >> code_shift) + (e0 >> 5);
    return q;
}

// Piece k of row `row`: exactly the tile (k) of the plain converting op
// (lin_off + row * lin_stride, rem_off + row * rem_stride, row_elems).
OCM_QS_HD inline QuantTileLoc quant_strided_tile(const XferQuantStridedOp &op, uint64_t row, uint32_t k, uint32_t code_shift) {
    const uint64_t rec = op.rem_off + row * op.rem_stride;
    return quant_row_tile(op.lin_off + row * op.lin_stride, rec, op.row_elems, k, code_shift);
}

#if !defined(__HIP_DEVICE_COMPILE__)
// One op against halves of local_bytes / remote_bytes. 0: fine (*src = the 16-bit bytes
// it converts, *wire = its record bytes; both 0 for an empty op); -1: `why` says what is
// wrong, naming the side. No sum or product here can overflow: the last row's end is
// tested as stride <= (room left) / (rows - 1), as strided_check_op does.
inline int quant_strided_check_op(const struct ocm_quant_strided_params &p, uint64_t local_bytes, uint64_t remote_bytes,
                                  uint64_t *src, uint64_t *wire, char *why, size_t why_len) {
    *src = *wire = 0;
    if (quant_check_dtype(p.dtype, why, why_len) != 0) return -1;
    if (p.row_elems % kMx8Group != 0 || p.row_elems >= (1ull << 31)) {
        std::snprintf(why, why_len, "rows of %llu elements (a multiple of 32 below 2^31 is needed)",
                      (unsigned long long)p.row_elems);
        return -1;
    }
    if (p.rows >= (1ull << 32)) {
        std::snprintf(why, why_len, "%llu rows (fewer than 2^32 are needed)", (unsigned long long)p.rows);
        return -1;
    }
    if (p.rows == 0 || p.row_elems == 0) return 0;
    const struct {
        const char *side;
        uint64_t off, stride, size, row_bytes, align;
    } sides[2] = {{"local", p.local_offset, p.local_stride, local_bytes, 2 * p.row_elems, 16},
                  {"remote", p.remote_offset, p.remote_stride, remote_bytes, quant_record_bytes(p.row_elems, p.dtype), 32}};
    for (const auto &s : sides) {
        if (s.off % s.align != 0) {
            std::snprintf(why, why_len, "%s offset %llu is not a multiple of %llu", s.side, (unsigned long long)s.off,
                          (unsigned long long)s.align);
            return -1;
        }
        if (s.stride % s.align != 0) {
            std::snprintf(why, why_len, "%s stride %llu is not a multiple of %llu", s.side, (unsigned long long)s.stride,
                          (unsigned long long)s.align);
            return -1;
        }
        if (p.rows > 1 && s.stride < s.row_bytes) {
            std::snprintf(why, why_len, "%s stride %llu is below the row's %llu bytes (rows would overlap)", s.side,
                          (unsigned long long)s.stride, (unsigned long long)s.row_bytes);
            return -1;
        }
        bool fits = s.off <= s.size && s.row_bytes <= s.size - s.off;
        if (fits && p.rows > 1) fits = s.stride <= (s.size - s.off - s.row_bytes) / (p.rows - 1);
        if (!fits) {
            std::snprintf(why, why_len, "%s range [%llu, +%llu rows x %llu bytes, stride %llu) exceeds %llu bytes", s.side,
                          (unsigned long long)s.off, (unsigned long long)p.rows, (unsigned long long)s.row_bytes,
                          (unsigned long long)s.stride, (unsigned long long)s.size);
            return -1;
        }
    }
    // rows never overlap and lie inside their halves: neither product can overflow
    *src = p.rows * sides[0].row_bytes;
    *wire = p.rows * sides[1].row_bytes;
    return 0;
}

// The device descriptor of a checked op (an empty op keeps no rows and no elements, so
// it has no tiles whatever its other fields say).
inline XferQuantStridedOp quant_strided_op(const struct ocm_quant_strided_params &p) {
    const bool empty = p.rows == 0 || p.row_elems == 0;
    XferQuantStridedOp op{};
    op.lin_off = p.local_offset;
    op.rem_off = p.remote_offset;
    op.lin_stride = p.local_stride;
    op.rem_stride = p.remote_stride;
    op.row_elems = empty ? 0 : (uint32_t)p.row_elems;
    op.rows = empty ? 0 : (uint32_t)p.rows;
    op.put = p.op_flag != 0;
    op.dtype = p.dtype;
    return op;
}
#endif

// ---- launch (xfer_quant_strided.hip) ----
constexpr int kQuantStridedInlineOps = 24;  // ops carried in the kernarg segment

// tile_shift is kQuantTileShift (tiles are cut in elements)
struct XferQuantStridedArgs : ListArgs<XferQuantStridedOp, kQuantStridedInlineOps> {};
static_assert(list_args_fit<XferQuantStridedArgs>, "kernarg segment limit");
// the head and nothing else, where it has always been
static_assert(offsetof(XferQuantStridedArgs, ops) == 104 && offsetof(XferQuantStridedArgs, wave_op) == 112 &&
                  offsetof(XferQuantStridedArgs, inline_ops) == 120 &&
                  sizeof(XferQuantStridedArgs) == 120 + kQuantStridedInlineOps * sizeof(XferQuantStridedOp),
              "strided converting launch argument layout");

// Host-side plan: fills tiles_per_row and first_tile, returns total tiles.
inline uint64_t xfer_quant_strided_plan(XferQuantStridedOp *ops, uint32_t n, uint32_t /*tile_shift*/) {
    return list_plan(ops, n, [](XferQuantStridedOp &op) {
        op.tiles_per_row = quant_strided_tiles_per_row(op.row_elems);
        return quant_strided_tile_count(op);
    });
}

}  // namespace ocm
