// Strided one-sided ops (ocm_copy_onesided_strided): `rows` pieces of `row_bytes`,
// one stride per side, between the linear side and the striped side. One launch
// serves a whole list, planned as every descriptor list is (ocm/list.h): the list is
// cut into wave-tiles, the host prefix-sums each op's tile count into `first_tile`, and
// every wave walks a contiguous tile range. One descriptor per op is all the kernel reads:
// nothing grows with the number of rows.
//
// Tiles are cut in row-relative coordinates: piece k of a row is its bytes
// [k << tile_shift, min((k + 1) << tile_shift, row_bytes)), whatever the row's
// alignment on either side, so every row of an op has the same tiles_per_row and tile
// t is row t / tiles_per_row, piece t % tiles_per_row. (Tiles aligned in striped
// coordinates, as a batch cuts them, would give rows that start at different offsets
// mod the tile different counts: a per-row table, or a search.) A tile is at most one
// stripe unit long, so it crosses at most one unit boundary of the striped side and
// becomes at most two spans.
//
// This header is the arithmetic the kernel (xfer_strided.hip), the host plan
// (strided.cpp) and the stand-alone test program (ocm_strided_tests.cpp) share; it
// needs no HIP.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdio>

#include "ocm/list.h"
#include "oncillamem.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define OCM_STRIDED_HD __host__ __device__
#else
#define OCM_STRIDED_HD
#endif

namespace ocm {

struct XferStridedOp {
    uint64_t lin_off;        // first byte of row 0 in the linear buffer
    uint64_t rem_off;        // first byte of row 0 in striped coordinates
    uint64_t row_bytes;
    uint64_t lin_stride;     // bytes from one row's start to the next, linear side
    uint64_t rem_stride;     // same, striped side
    uint64_t tiles_per_row;  // ceil(row_bytes / tile)
    uint64_t first_tile;     // exclusive prefix sum of the ops' tile counts (rows * tiles_per_row)
    uint32_t rows;
    uint32_t put;            // 1: lin -> striped, 0: striped -> lin
};
static_assert(sizeof(XferStridedOp) == 64, "strided op layout");

// One contiguous span of a tile: n bytes at lin_off of the linear buffer and rem_off
// of the striped address space, inside one stripe unit.
struct StridedPiece {
    uint64_t lin_off, rem_off, n;
};

OCM_STRIDED_HD inline uint64_t strided_tiles_per_row(uint64_t row_bytes, uint32_t tile_shift) {
    return (row_bytes >> tile_shift) + ((row_bytes & ((1ull << tile_shift) - 1)) ? 1 : 0);
}

// Tiles of an op (0 for an empty one). rows < 2^32 and rows * row_bytes fits the
// remote half, so the product cannot overflow.
OCM_STRIDED_HD inline uint64_t strided_tile_count(const XferStridedOp &op) { return (uint64_t)op.rows * op.tiles_per_row; }

// The spans of piece k of a row of row_bytes whose first byte is lin_row_off of the linear
// buffer and rem_row_off of the striped address space: 1, or 2 when the piece crosses a
// stripe-unit boundary of the striped side (n_ext > 1; tile <= unit, so at most one
// boundary). The span arithmetic every row-relative kernel shares.
OCM_STRIDED_HD inline int strided_pieces_at(uint64_t lin_row_off, uint64_t rem_row_off, uint64_t row_bytes, uint64_t k,
                                            uint32_t n_ext, uint32_t unit_shift, uint32_t tile_shift, StridedPiece out[2]) {
    const uint64_t in_row = k << tile_shift;
    const uint64_t left = row_bytes - in_row;
    const uint64_t n = left < (1ull << tile_shift) ? left : (1ull << tile_shift);
    const uint64_t lo = lin_row_off + in_row;
    const uint64_t ro = rem_row_off + in_row;
    out[0].lin_off = lo;
    out[0].rem_off = ro;
    out[0].n = n;
    if (n_ext > 1) {
        const uint64_t unit = 1ull << unit_shift;
        const uint64_t room = unit - (ro & (unit - 1));  // bytes up to the next unit boundary
        if (room < n) {
            out[0].n = room;
            out[1].lin_off = lo + room;
            out[1].rem_off = ro + room;
            out[1].n = n - room;
            return 2;
        }
    }
    return 1;
}

// The spans of piece k of the row that is row `lin_row` of the linear side's table and row
// `rem_row` of the striped side's. `Op`: a descriptor with lin_off, rem_off, row_bytes and
// one stride per side (XferStridedOp; XferIndexedOp of ocm/indexed.h, whose rows are picked
// by index arrays).
template <class Op>
OCM_STRIDED_HD inline int strided_row_pieces(const Op &op, uint64_t lin_row, uint64_t rem_row, uint64_t k, uint32_t n_ext,
                                             uint32_t unit_shift, uint32_t tile_shift, StridedPiece out[2]) {
    return strided_pieces_at(op.lin_off + lin_row * op.lin_stride, op.rem_off + rem_row * op.rem_stride, op.row_bytes, k, n_ext,
                             unit_shift, tile_shift, out);
}

// A strided op's row is the same row on both sides.
OCM_STRIDED_HD inline int strided_row_pieces(const XferStridedOp &op, uint64_t row, uint64_t k, uint32_t n_ext,
                                             uint32_t unit_shift, uint32_t tile_shift, StridedPiece out[2]) {
    return strided_row_pieces(op, row, row, k, n_ext, unit_shift, tile_shift, out);
}

// The spans of tile t of an op (t < strided_tile_count(op)).
OCM_STRIDED_HD inline int strided_tile_pieces(const XferStridedOp &op, uint64_t t, uint32_t n_ext, uint32_t unit_shift,
                                              uint32_t tile_shift, StridedPiece out[2]) {
    uint64_t row, k;
    list_locate(op.tiles_per_row, t, &row, &k);
    return strided_row_pieces(op, row, k, n_ext, unit_shift, tile_shift, out);
}

#if !defined(__HIP_DEVICE_COMPILE__)
// One op against halves of local_bytes / remote_bytes. 0: fine (*moved = the bytes it
// moves, 0 for an empty op); -1: `why` says what is wrong. No sum or product here can
// overflow: the last row's end is tested as stride <= (room left) / (rows - 1).
inline int strided_check_op(const struct ocm_strided_params &p, uint64_t local_bytes, uint64_t remote_bytes,
                            uint64_t *moved, char *why, size_t why_len) {
    *moved = 0;
    if (p.reserved != 0) {
        std::snprintf(why, why_len, "reserved field is %u (must be 0)", p.reserved);
        return -1;
    }
    if (p.rows >= (1ull << 32)) {
        std::snprintf(why, why_len, "%llu rows (fewer than 2^32 are needed)", (unsigned long long)p.rows);
        return -1;
    }
    if (p.rows == 0 || p.row_bytes == 0) return 0;
    const struct {
        const char *side;
        uint64_t off, stride, size;
    } sides[2] = {{"local", p.local_offset, p.local_stride, local_bytes}, {"remote", p.remote_offset, p.remote_stride, remote_bytes}};
    for (const auto &s : sides) {
        if (p.rows > 1 && s.stride < p.row_bytes) {
            std::snprintf(why, why_len, "%s stride %llu is below the row's %llu bytes (rows would overlap)", s.side,
                          (unsigned long long)s.stride, (unsigned long long)p.row_bytes);
            return -1;
        }
        bool fits = s.off <= s.size && p.row_bytes <= s.size - s.off;
        if (fits && p.rows > 1) fits = s.stride <= (s.size - s.off - p.row_bytes) / (p.rows - 1);
        if (!fits) {
            std::snprintf(why, why_len, "%s range [%llu, +%llu rows x %llu bytes, stride %llu) exceeds %llu bytes", s.side,
                          (unsigned long long)s.off, (unsigned long long)p.rows, (unsigned long long)p.row_bytes,
                          (unsigned long long)s.stride, (unsigned long long)s.size);
            return -1;
        }
    }
    *moved = p.rows * p.row_bytes;
    return 0;
}
#endif

// ---- launch (xfer_strided.hip) ----
constexpr int kStridedInlineOps = 24;  // ops carried in the kernarg segment

struct XferStridedArgs : ListArgs<XferStridedOp, kStridedInlineOps> {};
static_assert(list_args_fit<XferStridedArgs>, "kernarg segment limit");
// the head and nothing else, where it has always been
static_assert(offsetof(XferStridedArgs, ops) == 104 && offsetof(XferStridedArgs, wave_op) == 112 &&
                  offsetof(XferStridedArgs, inline_ops) == 120 && sizeof(XferStridedArgs) == 120 + kStridedInlineOps * sizeof(XferStridedOp),
              "strided launch argument layout");

// Host-side plan: fills tiles_per_row and first_tile, returns total tiles.
inline uint64_t xfer_strided_plan(XferStridedOp *ops, uint32_t n, uint32_t tile_shift) {
    return list_plan(ops, n, [tile_shift](XferStridedOp &op) {
        op.tiles_per_row = strided_tiles_per_row(op.row_bytes, tile_shift);
        return strided_tile_count(op);
    });
}

}  // namespace ocm
