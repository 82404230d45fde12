// Pooled embedding lookup (ocm_copy_onesided_bag): a fused gather-reduce. The remote half
// holds a table of rows, the local half an id array cut into bags by an offsets array
// (include-last-offset form: bags + 1 entries) and optionally one fp32 weight per id;
// bag b's output row is the sum, weighted sum or mean of the table rows its ids pick,
// written in bag order to a table in the local half. The remote half is only read, so
// there are no remote atomics and duplicate ids simply add twice. One launch serves a
// whole list, planned as every descriptor list is (ocm/list.h).
//
// The result is defined bit for bit, so that the kernel (xfer_bag.hip), the host path
// (bag.cpp) and the numpy model of the tests agree whatever the pair. For bag b:
//   lo = min(widen(off[b]), ids), hi = min(widen(off[b + 1]), ids), hi = max(hi, lo)
//        (bag_bounds; widening and the unsigned compare are indexed_widen32's);
//   acc[e] = +0; for j = lo .. hi - 1 in that order, when indexed_in_range(id[j],
//        remote_rows): acc[e] = fl32(acc[e] + fl32(w[j] * widen(x[id[j]][e]))), two
//        roundings and never an fma (acc_rule of ocm/acc.h; without weights w is 1, so the
//        product is x itself); otherwise entry j adds nothing and is counted once;
//   mean: acc[e] = fl32(acc[e] / (float)(hi - lo)) when hi > lo (bag_mean): skipped
//        entries count in the divisor; their number is reported and the call fails anyway;
//   out[b][e] = acc[e] narrowed to the table's type, round to nearest even (bag_narrow16).
// An empty bag writes zeros.
//
// Tiles: tile t of an op is piece t % tiles_per_row of BAG t / tiles_per_row, 64 lanes x
// one 16-byte vector of the row (kBagTileBytes), so an op has bags * tiles_per_row tiles.
// The host plan cannot see the bags' lengths (the offsets are read on the device when the
// transfer runs) and does not try to: a wave's work per tile is proportional to its bag's
// length, and a list whose bags differ widely in length is balanced only as far as equal
// numbers of bags per wave balance it.
//
// Out-of-range ids go to the allocation's skip words, the ones the indexed ops count into
// (ocm/indexed.h). Out of scope: a max mode, MX-compressed tables, transfer plans, and
// scatter-add into remote memory.
//
// This header is what the kernel, the host side and the stand-alone test program
// (ocm_bag_tests.cpp) share; it needs no HIP.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdio>

#include "ocm/acc.h"
#include "ocm/indexed.h"
#include "ocm/list.h"
#include "oncillamem.h"

namespace ocm {

constexpr uint32_t kBagTileShift = 10;  // 1 KiB of a table row: 64 lanes x one 16-byte vector
constexpr uint32_t kBagTileBytes = 1u << kBagTileShift;
constexpr int kBagInFlight = 4;  // rows of a bag whose loads a wave issues before it uses the first

struct XferBagOp {
    uint64_t lin_off;        // first byte of bag 0's output row in the local half
    uint64_t rem_off;        // first byte of row 0 of the remote table, striped coordinates
    uint64_t lin_stride;     // bytes between output rows
    uint64_t rem_stride;     // bytes between table rows
    uint64_t tiles_per_row;  // ceil(row_bytes / kBagTileBytes)
    uint64_t first_tile;     // exclusive prefix sum of the ops' tile counts (bags * tiles_per_row)
    uint64_t idx_off;        // byte offsets in the local half: the ids,
    uint64_t offs_off;       // the bags + 1 offsets,
    uint64_t w_off;          // the fp32 weights, or OCM_INDEX_NONE
    uint32_t bags;
    uint32_t ids;            // entries of the id array
    uint32_t rem_rows;       // rows the remote table has
    uint32_t row_bytes;      // a positive multiple of 16
    uint32_t index_type;     // enum ocm_index_type: ids and offsets alike
    uint32_t dtype;          // enum ocm_acc_dtype: table and output alike
    uint32_t mode;           // enum ocm_bag_mode
    uint32_t pad;
};
static_assert(sizeof(XferBagOp) == 104, "bag op layout");
static_assert(sizeof(struct ocm_bag_params) == 104, "ocm_bag_params layout");

// ---- the rule ----
// Where bag b's entries lie in the id array: [*lo, *hi), from its two offsets as read
// (widened already) and the array's length. Offsets past the array are clamped to it, a
// decreasing pair is an empty bag.
OCM_ACC_HD inline void bag_bounds(uint64_t off_b, uint64_t off_b1, uint32_t ids, uint32_t *lo, uint32_t *hi) {
    *lo = off_b < ids ? (uint32_t)off_b : ids;
    *hi = off_b1 < ids ? (uint32_t)off_b1 : ids;
    if (*hi < *lo) *hi = *lo;
}

// The mean of a bag of n > 0 entries: one correctly rounded division.
OCM_ACC_HD inline float bag_mean(float acc, uint32_t n) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __fdiv_rn(acc, (float)n);
#else
    return acc / (float)n;
#endif
}

// fp32 to a 16-bit element, round to nearest even. bf16 as f32_to_bf16 of the Adam
// kernels (kernels/adam_rule.h) narrows; fp16 by the hardware's _rn convert on the device
// and the same rounding in integer arithmetic on the host. A NaN gives some NaN.
OCM_ACC_HD inline uint32_t bag_narrow16(float f, bool bf16) {
    uint32_t u = acc_float_bits(f);
    if (bf16) {
        if ((u & 0x7fffffffu) > 0x7f800000u) return (u >> 16) | 0x40u;
        u += 0x7fffu + ((u >> 16) & 1u);
        return u >> 16;
    }
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_bit_cast(uint16_t, (_Float16)f);
#else
    const uint32_t sign = (u >> 16) & 0x8000u;
    u &= 0x7fffffffu;
    if (u > 0x7f800000u) return sign | 0x7e00u;
    if (u >= 0x477ff000u) return sign | 0x7c00u;  // 65520 and above round to infinity
    if (u < 0x38800000u) {                         // below 2^-14: an fp16 subnormal, |f| * 2^24 rounded to an integer
        const float scaled = acc_bits_float(u) * 16777216.0f;  // exact, below 1024
        const float r = (scaled + 8388608.0f) - 8388608.0f;    // to nearest even
        return sign | (uint32_t)r;                              // 1024 is the smallest normal's encoding
    }
    u += 0xc8000fffu + ((u >> 13) & 1u);  // exponent bias 127 -> 15, then round the 13 dropped bits
    return sign | (u >> 13);
#endif
}

OCM_ACC_HD inline uint64_t bag_tiles_per_row(uint64_t row_bytes) { return (row_bytes + kBagTileBytes - 1) >> kBagTileShift; }
OCM_ACC_HD inline uint64_t bag_tile_count(const XferBagOp &op) { return (uint64_t)op.bags * op.tiles_per_row; }

#if !defined(__HIP_DEVICE_COMPILE__)
// acc[e] = rule(acc[e], widen(row[e]), w) over the n elements of one table row.
inline void bag_add_row_host(float *acc, const void *row, uint64_t n, uint32_t dtype, float w) {
    acc_apply_host(acc, row, n, dtype, w);
}

// The output row of a bag of `count` entries (hi - lo) whose sum is acc[0 .. n).
inline void bag_finish_host(const float *acc, void *out, uint64_t n, uint32_t dtype, uint32_t mode, uint32_t count) {
    const bool mean = mode == OCM_BAG_MEAN && count > 0;
    for (uint64_t e = 0; e < n; e++) {
        const float r = mean ? bag_mean(acc[e], count) : acc[e];
        if (dtype == kAccF32) {
            static_cast<float *>(out)[e] = r;
        } else {
            static_cast<uint16_t *>(out)[e] = (uint16_t)bag_narrow16(r, dtype == kAccBf16);
        }
    }
}

// One op against halves of local_bytes / remote_bytes. 0: fine (*moved = ids * row bytes, the
// nominal bytes read; 0 for an op without bags); -1: `why` says what is wrong. The table and
// array rules are indexed_check_table's and indexed_check_index_array's (ocm/indexed.h), whose
// forms cannot overflow.
inline int bag_check_op(const struct ocm_bag_params &p, uint64_t local_bytes, uint64_t remote_bytes, uint64_t *moved, char *why,
                        size_t why_len) {
    *moved = 0;
    if (p.bags == 0) return 0;  // does nothing, whatever else it says
    if (p.index_type != OCM_INDEX_I32 && p.index_type != OCM_INDEX_I64) {
        std::snprintf(why, why_len, "index_type %u is unknown (OCM_INDEX_I32 = 1, OCM_INDEX_I64 = 2)", p.index_type);
        return -1;
    }
    const uint64_t esize = acc_elem_size(p.dtype);
    if (esize == 0) {
        std::snprintf(why, why_len, "unknown element type %u", p.dtype);
        return -1;
    }
    if (p.mode != OCM_BAG_SUM && p.mode != OCM_BAG_MEAN) {
        std::snprintf(why, why_len, "mode %u is unknown (OCM_BAG_SUM = 0, OCM_BAG_MEAN = 1; there is no max)", p.mode);
        return -1;
    }
    if (p.reserved != 0) {
        std::snprintf(why, why_len, "reserved is %u, not 0", p.reserved);
        return -1;
    }
    if (p.mode == OCM_BAG_MEAN && p.weights_offset != OCM_INDEX_NONE) {
        std::snprintf(why, why_len, "per-sample weights go with OCM_BAG_SUM only, not with the mean");
        return -1;
    }
    if (p.row_elems == 0 || p.row_elems >= (1ull << 32) / esize || (p.row_elems * esize) % 16 != 0) {
        std::snprintf(why, why_len, "rows of %llu elements of %llu bytes (a positive multiple of 16 bytes below 2^32 is needed)",
                      (unsigned long long)p.row_elems, (unsigned long long)esize);
        return -1;
    }
    const uint64_t row_bytes = p.row_elems * esize;
    if (p.ids >= (1ull << 32)) {
        std::snprintf(why, why_len, "%llu ids (fewer than 2^32 are needed)", (unsigned long long)p.ids);
        return -1;
    }
    // The output has a row for every bag; the remote table is always picked from by id (its side
    // "has an index", whatever index_offset says: an op without ids never reads it), so the rule
    // for sides without one, a table row for every row of the op, does not apply to it.
    const IndexedSide sides[2] = {{"local", p.local_offset, p.local_stride, local_bytes, p.bags, OCM_INDEX_NONE, row_bytes},
                                  {"remote", p.remote_offset, p.remote_stride, remote_bytes, p.remote_rows, 0, row_bytes}};
    if (indexed_check_counts(p.bags, sides, why, why_len) != 0) return -1;
    for (const auto &s : sides) {
        // with a stripe unit of at least 16 bytes no 16-byte vector straddles a unit
        if (s.off % 16 != 0 || s.stride % 16 != 0) {
            std::snprintf(why, why_len, "%s offset %llu or stride %llu is not a multiple of 16", s.side, (unsigned long long)s.off,
                          (unsigned long long)s.stride);
            return -1;
        }
        if (indexed_check_table(s, p.bags, why, why_len) != 0) return -1;
    }
    // the arrays, in the local half: aligned, inside it, and outside the output table
    IndexedSide arr = {"offsets", 0, 0, 0, 0, p.offsets_offset, 0};
    if (indexed_check_index_array(arr, p.index_type, p.bags + 1, local_bytes, true, sides[0], why, why_len) != 0) return -1;
    if (p.ids != 0) {  // without ids neither array is read
        arr = {"ids", 0, 0, 0, 0, p.index_offset, 0};
        if (indexed_check_index_array(arr, p.index_type, p.ids, local_bytes, true, sides[0], why, why_len) != 0) return -1;
        arr = {"weights", 0, 0, 0, 0, p.weights_offset, 0};  // fp32: the size of an int32 index
        if (p.weights_offset != OCM_INDEX_NONE &&
            indexed_check_index_array(arr, OCM_INDEX_I32, p.ids, local_bytes, true, sides[0], why, why_len) != 0)
            return -1;
    }
    *moved = p.ids * row_bytes;
    return 0;
}

// The descriptor of a checked op, before the plan (an op without bags takes no tiles).
inline XferBagOp bag_op(const struct ocm_bag_params &p) {
    XferBagOp o{};
    if (p.bags == 0) return o;
    o.lin_off = p.local_offset;
    o.rem_off = p.remote_offset;
    o.lin_stride = p.local_stride;
    o.rem_stride = p.remote_stride;
    o.idx_off = p.index_offset;
    o.offs_off = p.offsets_offset;
    o.w_off = p.ids ? p.weights_offset : OCM_INDEX_NONE;
    o.bags = (uint32_t)p.bags;
    o.ids = (uint32_t)p.ids;
    o.rem_rows = (uint32_t)p.remote_rows;
    o.row_bytes = (uint32_t)(p.row_elems * acc_elem_size(p.dtype));
    o.index_type = p.index_type;
    o.dtype = p.dtype;
    o.mode = p.mode;
    return o;
}
#endif

// ---- launch (xfer_bag.hip) ----
constexpr int kBagInlineOps = 16;  // ops carried in the kernarg segment

struct XferBagArgs : ListArgs<XferBagOp, kBagInlineOps> {
    unsigned long long *skipped;       // device word: entries skipped, counted up (never reset by a launch)
    unsigned long long *skipped_host;  // pinned host word the launcher copies it to after the kernel
};
static_assert(list_args_fit<XferBagArgs>, "kernarg segment limit");

// Host-side plan: fills tiles_per_row and first_tile, returns total tiles. The tile is
// kBagTileBytes whatever the pair (tile_shift is the list head's, always kBagTileShift).
inline uint64_t xfer_bag_plan(XferBagOp *ops, uint32_t n, uint32_t) {
    return list_plan(ops, n, [](XferBagOp &op) {
        op.tiles_per_row = bag_tiles_per_row(op.row_bytes);
        return bag_tile_count(op);
    });
}

}  // namespace ocm
