// Indexed one-sided ops (ocm_copy_onesided_indexed): `rows` pieces of `row_bytes` between
// a table of rows in the local half and one in the remote half, the row on either side
// picked by an index array that lives in the local half: gather, scatter, or both. One
// launch serves a whole list, planned as every descriptor list is (ocm/list.h), and the
// tiles are cut row-relative exactly as strided tiles are (ocm/strided.h): tile t of an
// op is piece t % tiles_per_row of its row j = t / tiles_per_row, whatever rows the
// indices pick, so one descriptor per op is all the host sends and nothing grows with
// the number of rows.
//
// The indices are read when the transfer runs, on the device: the host cannot check
// them at the call. Row j is skipped, whole and on both sides, when either of its
// indices is outside [0, table rows) of its side (indexed_in_range, compared unsigned,
// so negative values are out of range); the table fits its half (indexed_check_op), so
// index * stride cannot overflow or leave the half for an index that passed. Skipped
// rows are counted, once per row.
//
// The index arrays are data of the local half like any other: a torch kernel may have
// written them just before, and what orders the transfer after that kernel is
// ocm_stream_wait, as for the rows themselves.
//
// Out of scope: transfer plans and hipGraph capture, the copy service, put-side accumulate
// variants, index-times-stride (layer-major) ops, a defined result for duplicate
// destination rows, and scatter-add. The converting (MX) variant is a call of its own,
// ocm_copy_onesided_quant_indexed (ocm/quant_indexed.h), and so is the gather-side
// accumulate, the pooled lookup ocm_copy_onesided_bag (ocm/bag.h); both share the bounds
// rule, the validator's helpers and the skip count of this one.
//
// This header is what the kernel (xfer_indexed.hip), the host side (indexed.cpp) and the
// stand-alone test program (ocm_indexed_tests.cpp) share; it needs no HIP.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdio>

#include "ocm/list.h"
#include "ocm/strided.h"
#include "oncillamem.h"

namespace ocm {

struct XferIndexedOp {
    uint64_t lin_off;        // first byte of row 0 of the local table
    uint64_t rem_off;        // first byte of row 0 of the remote table, striped coordinates
    uint64_t row_bytes;
    uint64_t lin_stride;     // bytes between rows of the local table
    uint64_t rem_stride;     // same, remote table
    uint64_t tiles_per_row;  // ceil(row_bytes / tile)
    uint64_t first_tile;     // exclusive prefix sum of the ops' tile counts (rows * tiles_per_row)
    uint64_t lin_idx_off;    // byte offset in the local half of the local-side indices, or OCM_INDEX_NONE
    uint64_t rem_idx_off;    // same, remote-side indices
    uint32_t rows;           // rows moved: entries of each index array
    uint32_t put;            // 1: local -> remote, 0: remote -> local
    uint32_t lin_rows;       // rows the local table has
    uint32_t rem_rows;       // rows the remote table has
    uint32_t index_type;     // enum ocm_index_type
    uint32_t pad;
};
static_assert(sizeof(XferIndexedOp) == 96, "indexed op layout");
static_assert(sizeof(struct ocm_indexed_params) == 88, "ocm_indexed_params layout");

OCM_STRIDED_HD inline uint32_t indexed_index_bytes(uint32_t index_type) { return index_type == OCM_INDEX_I64 ? 8u : 4u; }

// An index as read from its array, widened for the comparison: int32 values sign-extend,
// so that -1 is 2^64 - 1 and never a row.
OCM_STRIDED_HD inline uint64_t indexed_widen32(uint32_t raw) { return (uint64_t)(int64_t)(int32_t)raw; }

// THE bounds rule: a row moves only if this holds for the index of either side.
OCM_STRIDED_HD inline bool indexed_in_range(uint64_t index, uint64_t table_rows) { return index < table_rows; }

OCM_STRIDED_HD inline uint64_t indexed_tile_count(const XferIndexedOp &op) { return (uint64_t)op.rows * op.tiles_per_row; }

#if !defined(__HIP_DEVICE_COMPILE__)
// Index j of the array at byte `off` of the local half `base` (host memory), widened.
inline uint64_t indexed_load_host(const char *base, uint64_t off, uint32_t index_type, uint64_t j) {
    if (index_type == OCM_INDEX_I64) {
        uint64_t v;
        __builtin_memcpy(&v, base + off + j * 8, 8);
        return v;
    }
    uint32_t v;
    __builtin_memcpy(&v, base + off + j * 4, 4);
    return indexed_widen32(v);
}

// One side of an op as the checks below see it. row_bytes is per side: the indexed op
// moves the same bytes on both, the converting one (ocm/quant_indexed.h) 16-bit elements
// on the local side and a record on the remote one.
struct IndexedSide {
    const char *side;
    uint64_t off, stride, size, table_rows, idx_off, row_bytes;
};

// index_type is known, and at least one side has an index. 0, or -1 with `why`.
inline int indexed_check_kind(uint32_t index_type, uint64_t local_index_offset, uint64_t remote_index_offset, char *why,
                              size_t why_len) {
    if (index_type != OCM_INDEX_I32 && index_type != OCM_INDEX_I64) {
        std::snprintf(why, why_len, "index_type %u is unknown (OCM_INDEX_I32 = 1, OCM_INDEX_I64 = 2)", index_type);
        return -1;
    }
    if (local_index_offset == OCM_INDEX_NONE && remote_index_offset == OCM_INDEX_NONE) {
        std::snprintf(why, why_len, "no index on either side (a strided op moves rows in order)");
        return -1;
    }
    return 0;
}

// rows and both tables' rows are below 2^32.
inline int indexed_check_counts(uint64_t rows, const IndexedSide (&sides)[2], char *why, size_t why_len) {
    if (rows >= (1ull << 32)) {
        std::snprintf(why, why_len, "%llu rows (fewer than 2^32 are needed)", (unsigned long long)rows);
        return -1;
    }
    for (const auto &s : sides)
        if (s.table_rows >= (1ull << 32)) {
            std::snprintf(why, why_len, "%s table of %llu rows (fewer than 2^32 are needed)", s.side,
                          (unsigned long long)s.table_rows);
            return -1;
        }
    return 0;
}

// The table of one side: rows do not overlap, its last row ends inside its half, and a
// side without an index has a row for every row of the op. No sum or product here can
// overflow: the last row is tested as stride <= (room left) / (rows - 1).
inline int indexed_check_table(const IndexedSide &s, uint64_t rows, char *why, size_t why_len) {
    if (s.table_rows > 1 && s.stride < s.row_bytes) {
        std::snprintf(why, why_len, "%s stride %llu is below the row's %llu bytes (rows would overlap)", s.side,
                      (unsigned long long)s.stride, (unsigned long long)s.row_bytes);
        return -1;
    }
    // a table of no rows holds no byte: every index of that side is out of range
    bool fits = s.table_rows == 0 || (s.off <= s.size && s.row_bytes <= s.size - s.off);
    if (fits && s.table_rows > 1) fits = s.stride <= (s.size - s.off - s.row_bytes) / (s.table_rows - 1);
    if (!fits) {
        std::snprintf(why, why_len, "%s table [%llu, +%llu rows x %llu bytes, stride %llu) exceeds %llu bytes", s.side,
                      (unsigned long long)s.off, (unsigned long long)s.table_rows, (unsigned long long)s.row_bytes,
                      (unsigned long long)s.stride, (unsigned long long)s.size);
        return -1;
    }
    if (s.idx_off == OCM_INDEX_NONE && s.table_rows < rows) {
        std::snprintf(why, why_len, "%s side has no index and a table of %llu rows, fewer than the op's %llu", s.side,
                      (unsigned long long)s.table_rows, (unsigned long long)rows);
        return -1;
    }
    return 0;
}

// The index array of side `s` (it has one): aligned to its element size, `rows` entries
// inside the local half, tested as rows <= (room left) / element size; and for a get,
// which writes the local table `local` (checked by indexed_check_table already), outside
// that table.
inline int indexed_check_index_array(const IndexedSide &s, uint32_t index_type, uint64_t rows, uint64_t local_bytes, bool get,
                                     const IndexedSide &local, char *why, size_t why_len) {
    const uint64_t isz = indexed_index_bytes(index_type);
    if (s.idx_off % isz) {
        std::snprintf(why, why_len, "%s index offset %llu is not a multiple of the index size %llu", s.side,
                      (unsigned long long)s.idx_off, (unsigned long long)isz);
        return -1;
    }
    if (s.idx_off > local_bytes || rows > (local_bytes - s.idx_off) / isz) {
        std::snprintf(why, why_len, "%s index array [%llu, +%llu x %llu bytes) exceeds the local half's %llu bytes", s.side,
                      (unsigned long long)s.idx_off, (unsigned long long)rows, (unsigned long long)isz,
                      (unsigned long long)local_bytes);
        return -1;
    }
    // a get writes the local table: it must not write the indices the same op reads
    if (get && local.table_rows > 0) {
        const uint64_t t0 = local.off, t1 = local.off + (local.table_rows - 1) * local.stride + local.row_bytes;
        const uint64_t i0 = s.idx_off, i1 = s.idx_off + rows * isz;
        if (i0 < t1 && t0 < i1) {
            std::snprintf(why, why_len, "%s index array [%llu, %llu) overlaps the local table [%llu, %llu) that the get writes",
                          s.side, (unsigned long long)i0, (unsigned long long)i1, (unsigned long long)t0,
                          (unsigned long long)t1);
            return -1;
        }
    }
    return 0;
}

// One op against halves of local_bytes / remote_bytes. 0: fine (*moved = rows * row_bytes,
// the nominal bytes; 0 for an empty op); -1: `why` says what is wrong. The rules are the
// helpers above, which the converting indexed op's validator (ocm/quant_indexed.h) calls
// as well.
inline int indexed_check_op(const struct ocm_indexed_params &p, uint64_t local_bytes, uint64_t remote_bytes,
                            uint64_t *moved, char *why, size_t why_len) {
    *moved = 0;
    if (p.rows == 0 || p.row_bytes == 0) return 0;  // does nothing, whatever else it says
    if (indexed_check_kind(p.index_type, p.local_index_offset, p.remote_index_offset, why, why_len) != 0) return -1;
    const IndexedSide sides[2] = {
        {"local", p.local_offset, p.local_stride, local_bytes, p.local_rows, p.local_index_offset, p.row_bytes},
        {"remote", p.remote_offset, p.remote_stride, remote_bytes, p.remote_rows, p.remote_index_offset, p.row_bytes}};
    if (indexed_check_counts(p.rows, sides, why, why_len) != 0) return -1;
    for (const auto &s : sides)
        if (indexed_check_table(s, p.rows, why, why_len) != 0) return -1;
    for (const auto &s : sides)
        if (s.idx_off != OCM_INDEX_NONE &&
            indexed_check_index_array(s, p.index_type, p.rows, local_bytes, p.op_flag == 0, sides[0], why, why_len) != 0)
            return -1;
    *moved = p.rows * p.row_bytes;
    return 0;
}

// The descriptor of a checked op, before the plan (an empty op takes no tiles).
inline XferIndexedOp indexed_op(const struct ocm_indexed_params &p) {
    XferIndexedOp o{};
    const bool empty = p.rows == 0 || p.row_bytes == 0;
    o.lin_off = p.local_offset;
    o.rem_off = p.remote_offset;
    o.row_bytes = empty ? 0 : p.row_bytes;
    o.rows = empty ? 0 : (uint32_t)p.rows;
    o.lin_stride = p.local_stride;
    o.rem_stride = p.remote_stride;
    o.lin_idx_off = p.local_index_offset;
    o.rem_idx_off = p.remote_index_offset;
    o.lin_rows = empty ? 0 : (uint32_t)p.local_rows;
    o.rem_rows = empty ? 0 : (uint32_t)p.remote_rows;
    o.index_type = p.index_type;
    o.put = p.op_flag != 0;
    return o;
}
#endif

// ---- launch (xfer_indexed.hip) ----
constexpr int kIndexedInlineOps = 16;  // ops carried in the kernarg segment

struct XferIndexedArgs : ListArgs<XferIndexedOp, kIndexedInlineOps> {
    unsigned long long *skipped;          // device word: rows skipped, counted up (never reset by a launch)
    unsigned long long *skipped_host;     // pinned host word the launcher copies it to after the kernel (the kernel reads neither)
};
static_assert(list_args_fit<XferIndexedArgs>, "kernarg segment limit");

// Host-side plan: fills tiles_per_row and first_tile, returns total tiles.
inline uint64_t xfer_indexed_plan(XferIndexedOp *ops, uint32_t n, uint32_t tile_shift) {
    return list_plan(ops, n, [tile_shift](XferIndexedOp &op) {
        op.tiles_per_row = strided_tiles_per_row(op.row_bytes, tile_shift);
        return indexed_tile_count(op);
    });
}

}  // namespace ocm
