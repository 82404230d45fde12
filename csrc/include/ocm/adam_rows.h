// Row-sparse fused Adam (ocm_x_adam_rows): `rows` ids pick rows of an embedding table in the
// remote half of one pair; the rows' exp_avg / exp_avg_sq (and, for a bf16 table, their fp32
// master weights) sit in tables of the same shape in the remote half of a state pair, which
// may be the same one. One launch updates the picked rows where they live, with the dense
// kernel's element rule (adam1, csrc/src/kernels/adam_rule.h) and the caller's global step
// in the bias corrections: a row's moments do not move while it is not picked ("lazy" Adam).
//
// The ids are read on the device when the kernel runs. A row whose id is outside
// [0, table_rows) is skipped whole and counted: the bounds rule is the indexed ops'
// (indexed_widen32 / indexed_in_range, ocm/indexed.h), and every table fits its half
// (adam_rows_check), so id * stride cannot overflow or leave the half for an id that passed.
// Duplicate ids have no defined result.
//
// This header is what the kernel (optim_rows.hip), the host side (optim.cpp) and the
// stand-alone test program (ocm_adam_rows_tests.cpp) share; it calls nothing of HIP.
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "ocm/indexed.h"
#include "ocm/optim.h"

// The descriptor of one step, as the hook takes it. Offsets and strides of the four tables
// are bytes in their pair's remote half, striped coordinates.
struct ocm_adam_rows {
    uint64_t rows;                   // k: entries of the id array, rows of the gradient
    uint64_t dim;                    // elements per row
    uint64_t table_rows;             // rows every table has
    uint32_t index_type;             // OCM_INDEX_I32 / OCM_INDEX_I64
    uint32_t bf16;                   // 0: fp32 table and gradient; 1: bf16 table and gradient, fp32 master in the state
    uint64_t table_off, table_stride;  // the embedding table (dtype elements), in the table's pair
    uint64_t m_off, m_stride;        // exp_avg, fp32, in the state's pair
    uint64_t v_off, v_stride;        // exp_avg_sq, fp32, in the state's pair
    uint64_t w_off, w_stride;        // fp32 master rows, in the state's pair (bf16 only)
    uint64_t g_stride;               // elements between rows of the gradient
};

namespace ocm {

static_assert(sizeof(ocm_adam_rows) == 104, "ocm_adam_rows layout");

// ---- tile geometry ----
// One tile is one wave-wide pass of a row: 64 lanes x one 16-byte fp32 vector.
constexpr uint32_t kAdamRowsTileShift = 8;
constexpr uint32_t kAdamRowsTileElems = 1u << kAdamRowsTileShift;  // 256
constexpr int kAdamRowsInFlight = 4;  // tiles whose loads a wave issues before the first use
constexpr int kAdamRowsWgPerCu = 4;   // workgroups (of kListWaves waves) per CU at the most

OCM_STRIDED_HD inline uint64_t adam_rows_tiles_per_row(uint64_t dim) {
    return (dim + kAdamRowsTileElems - 1) >> kAdamRowsTileShift;
}

// First element of the vector that `lane` owns in piece k of a row (live when below dim).
OCM_STRIDED_HD inline uint64_t adam_rows_elem(uint64_t k, uint32_t lane) {
    return (k << kAdamRowsTileShift) + ((uint64_t)lane << 2);
}

// The bounds rule, which is the indexed ops': the id as read (int32 widened by
// indexed_widen32, int64 as it is) picks a row only if indexed_in_range holds.
OCM_STRIDED_HD inline bool adam_rows_picks(uint64_t id, uint64_t table_rows) { return indexed_in_range(id, table_rows); }

// The launch: `grid` workgroups of kListWaves waves; wave w walks the tiles
// list_wave_range(w, grid, total_tiles) gives it, tile t being piece k of row j by
// list_locate(tiles_per_row, t). A pure function of k, dim, the CU count and the knobs:
// enough waves that each has kAdamRowsInFlight tiles to keep in flight, at most
// kAdamRowsWgPerCu workgroups a CU (k.grid > 0: that many workgroups, whatever the rule says).
struct AdamRowsShape {
    uint32_t grid;                   // workgroups; 0: no work
    uint64_t tiles_per_row, total_tiles;
};

inline AdamRowsShape adam_rows_launch_shape(uint64_t rows, uint64_t dim, int cus, const AdamKnobs &k) {
    AdamRowsShape s{0, adam_rows_tiles_per_row(dim), 0};
    s.total_tiles = rows * s.tiles_per_row;  // rows < 2^32 and dim < 2^32 (adam_rows_check)
    if (s.total_tiles == 0) return s;
    const uint64_t per_wg = (uint64_t)kListWaves * kAdamRowsInFlight;
    const uint64_t want = (s.total_tiles + per_wg - 1) / per_wg;
    const uint64_t cap = (uint64_t)(cus > 0 ? cus : 1) * kAdamRowsWgPerCu;
    s.grid = (uint32_t)(want < cap ? want : cap);
    if (k.grid > 0) s.grid = (uint32_t)k.grid;
    return s;
}

#if !defined(__HIP_DEVICE_COMPILE__)
// ---- the validator ----
// One step against remote halves of table_bytes / state_bytes. same_pair: the table and the
// state are one allocation, so the table must keep clear of the state tables (which must
// keep clear of each other in any case). 0: fine; -1: `why` says what is wrong. Counts are
// bounded first and every range is tested as bytes <= size - offset, a table's last row as
// stride <= (room left) / (rows - 1), as indexed_check_op does: nothing here can overflow.
inline int adam_rows_check(const ocm_adam_rows &d, uint64_t table_bytes, uint64_t state_bytes, bool same_pair,
                           char *why, size_t why_len) {
    if (d.index_type != OCM_INDEX_I32 && d.index_type != OCM_INDEX_I64) {
        std::snprintf(why, why_len, "index_type %u is unknown (OCM_INDEX_I32 = 1, OCM_INDEX_I64 = 2)", d.index_type);
        return -1;
    }
    if (d.bf16 > 1) {
        std::snprintf(why, why_len, "table dtype %u is unknown (0: fp32, 1: bf16)", d.bf16);
        return -1;
    }
    if (d.rows >= (1ull << 32)) {
        std::snprintf(why, why_len, "%llu rows (fewer than 2^32 are needed)", (unsigned long long)d.rows);
        return -1;
    }
    if (d.table_rows >= (1ull << 32)) {
        std::snprintf(why, why_len, "tables of %llu rows (fewer than 2^32 are needed)", (unsigned long long)d.table_rows);
        return -1;
    }
    if (d.dim == 0 || d.dim % 4 != 0 || d.dim >= (1ull << 32)) {
        std::snprintf(why, why_len, "dim %llu is not a positive multiple of 4 below 2^32", (unsigned long long)d.dim);
        return -1;
    }
    if (d.g_stride % 4 != 0 || d.g_stride >= (1ull << 30) || (d.rows > 1 && d.g_stride < d.dim)) {
        std::snprintf(why, why_len, "gradient stride %llu is not a multiple of 4 in [dim, 2^30) elements",
                      (unsigned long long)d.g_stride);
        return -1;
    }
    const uint64_t elem = d.bf16 ? 2 : 4;
    struct Tab {
        const char *name;
        uint64_t off, stride, row_bytes, align, size;
        bool in_state;
    };
    const Tab tabs[4] = {{"table", d.table_off, d.table_stride, d.dim * elem, 4 * elem, table_bytes, false},
                         {"exp_avg", d.m_off, d.m_stride, d.dim * 4, 16, state_bytes, true},
                         {"exp_avg_sq", d.v_off, d.v_stride, d.dim * 4, 16, state_bytes, true},
                         {"master", d.w_off, d.w_stride, d.dim * 4, 16, state_bytes, true}};
    const int n_tabs = d.bf16 ? 4 : 3;
    for (int i = 0; i < n_tabs; i++) {
        const Tab &t = tabs[i];
        if (t.off % t.align || t.stride % t.align) {
            std::snprintf(why, why_len, "%s offset %llu or stride %llu is not a multiple of %llu", t.name,
                          (unsigned long long)t.off, (unsigned long long)t.stride, (unsigned long long)t.align);
            return -1;
        }
        if (d.table_rows > 1 && t.stride < t.row_bytes) {
            std::snprintf(why, why_len, "%s stride %llu is below the row's %llu bytes (rows would overlap)", t.name,
                          (unsigned long long)t.stride, (unsigned long long)t.row_bytes);
            return -1;
        }
        // a table of no rows holds no byte: every id is out of range
        bool fits = d.table_rows == 0 || (t.off <= t.size && t.row_bytes <= t.size - t.off);
        if (fits && d.table_rows > 1) fits = t.stride <= (t.size - t.off - t.row_bytes) / (d.table_rows - 1);
        if (!fits) {
            std::snprintf(why, why_len, "%s [%llu, +%llu rows x %llu bytes, stride %llu) exceeds the remote half's %llu bytes",
                          t.name, (unsigned long long)t.off, (unsigned long long)d.table_rows,
                          (unsigned long long)t.row_bytes, (unsigned long long)t.stride, (unsigned long long)t.size);
            return -1;
        }
    }
    if (d.table_rows == 0) return 0;
    // whole byte ranges, pairwise: each fits its half, so no end can overflow
    auto end = [&](const Tab &t) { return t.off + (d.table_rows - 1) * t.stride + t.row_bytes; };
    for (int i = 0; i < n_tabs; i++)
        for (int j = i + 1; j < n_tabs; j++) {
            if (tabs[i].in_state != tabs[j].in_state && !same_pair) continue;  // other memory
            if (tabs[i].off < end(tabs[j]) && tabs[j].off < end(tabs[i])) {
                std::snprintf(why, why_len, "%s [%llu, %llu) overlaps %s [%llu, %llu)", tabs[i].name,
                              (unsigned long long)tabs[i].off, (unsigned long long)end(tabs[i]), tabs[j].name,
                              (unsigned long long)tabs[j].off, (unsigned long long)end(tabs[j]));
                return -1;
            }
        }
    return 0;
}

// The hyper-parameters of a row-sparse step: no weight decay of either kind (what it would
// mean for rows that are not picked is a policy nobody has chosen), a finite gradient scale.
inline int adam_rows_check_hp(const float hp[9], float gscale, char *why, size_t why_len) {
    uint32_t bits;
    std::memcpy(&bits, &gscale, 4);
    if ((bits & 0x7f800000u) == 0x7f800000u) {
        std::snprintf(why, why_len, "gscale is not finite");
        return -1;
    }
    if (hp[3] != 0.f || hp[6] == hp[6]) {  // hp[6]: AdamW's weight multiplier, NaN when there is none
        std::snprintf(why, why_len, "weight decay (L2 or decoupled) is not defined for rows that are not picked: "
                                    "hp[3] must be 0 and hp[6] NaN");
        return -1;
    }
    return 0;
}
#endif

// ---- launch (optim_rows.hip) ----
struct AdamRowsArgs {
    AdamArgs c;                      // the state's pair and the hyper-parameters (wd 0, not decoupled)
    StateSpace table;                // the table's pair
    ocm_adam_rows d;
    const void *ids;                 // device: d.rows ids of d.index_type
    const void *g;                   // device: d.rows x d.dim gradient, fp32 (16-byte aligned) or bf16 (8-byte)
    unsigned long long *skipped;     // device word counted up per skipped row, or null
    float gscale;
    uint32_t grid;                   // (set by the launcher) AdamRowsShape
    uint64_t tiles_per_row, total_tiles;
};
static_assert(sizeof(AdamRowsArgs) < 4096, "kernarg segment limit");

hipError_t adam_rows_launch(const AdamRowsArgs &a, const AdamKnobs &knobs, hipStream_t stream);

}  // namespace ocm
