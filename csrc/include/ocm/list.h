// The plan every descriptor list shares (batch, converting, strided, indexed and accumulate
// ops: ocm/xfer.h, ocm/quant.h, ocm/strided.h, ocm/indexed.h, ocm/acc.h). A list is cut into
// wave-tiles; the host prefix-sums each op's tile count into `first_tile`, sizes a
// grid of workgroups of kListWaves waves, and every wave takes one contiguous tile
// range plus the op its first tile belongs to (the wave table), so waves never
// search: they walk forward through the ops they cover. How many tiles an op has is
// the kind's own rule, defined beside its geometry and passed in here. The launch
// arguments every list kernel takes (ListArgs) and the walk of the kinds whose ops have
// rows (list_enter_op, list_locate, list_next_piece) are here as well.
//
// A wrong tile count or a range cut two ways would size a grid for tiles that no
// wave copies, so each of these expressions exists once: the kernels, the host plans
// and the stand-alone test programs (ocm_list_tests.cpp) share this header; it needs
// no HIP.
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define OCM_LIST_HD __host__ __device__
#else
#define OCM_LIST_HD
#endif

namespace ocm {

constexpr int kListWaves = 4;  // waves of a workgroup (kWaves of the kernels)
constexpr int kXferMaxExtents = 8;
constexpr size_t kKernargLimit = 4096;  // bytes of kernel arguments a launch takes

// The launch arguments of every list kernel: the pair's side, the plan's side, and the
// descriptors, which travel here (inline_ops) for lists of at most INLINE ops and in device
// memory (ops, wave_op) for longer ones. A kind's arguments are this head, behind which a
// kind puts fields of its own (a derived struct: XferBatchArgs, XferIndexedArgs).
template <class OP, int INLINE>
struct ListArgs {
    using Op = OP;
    static constexpr int kInline = INLINE;  // ops carried in the kernarg segment
    char *lin;                     // linear side
    char *ext[kXferMaxExtents];    // extent bases of the striped side
    uint32_t unit_shift;           // log2(stripe unit); ignored when n_ext == 1
    uint32_t n_ext;                // 1..8
    uint32_t tile_shift;
    uint32_t n_ops;
    uint64_t total_tiles;
    uint32_t grid;                 // workgroups (kListWaves waves each)
    uint32_t host_tier;            // 1: every extent is pinned host memory (PCIe launch shape, plain stores for puts)
    const Op *ops;                 // device copy when n_ops > INLINE
    const uint32_t *wave_op;       // device: first op of each wave (n_ops > INLINE)
    Op inline_ops[INLINE];
};
// Whether arguments `Args` (a ListArgs or a kind's struct derived from one) fit a launch:
// asserted beside every kind's struct, and where every list kernel enters its list
// (list_wave_start, kernels/xfer_copy.h) for whatever it is instantiated with.
template <class Args>
constexpr bool list_args_fit = sizeof(Args) <= kKernargLimit;

// Tiles [*t0, *t1) of wave `w` of `grid` workgroups: equal shares, rounded up, so the
// last waves may get fewer tiles or none (*t0 >= *t1).
OCM_LIST_HD inline void list_wave_range(uint64_t w, uint32_t grid, uint64_t total_tiles, uint64_t *t0, uint64_t *t1) {
    const uint64_t waves = (uint64_t)grid * kListWaves;
    const uint64_t per = (total_tiles + waves - 1) / waves;
    const uint64_t t = w * per;
    *t0 = t;
    *t1 = t + per < total_tiles ? t + per : total_tiles;
}

// Host-side plan: first_tile of every op is the exclusive prefix sum of the ops' tile
// counts. tiles_of(op) is the kind's rule (it may fill fields of the op that the rule
// needs). Returns the total.
template <class Op, class TilesOf>
inline uint64_t list_plan(Op *ops, uint32_t n, TilesOf tiles_of) {
    uint64_t total = 0;
    for (uint32_t i = 0; i < n; i++) {
        ops[i].first_tile = total;
        total += tiles_of(ops[i]);
    }
    return total;
}

// The wave table: out[w] is the op that holds the first tile of wave w, for every wave
// of `grid` workgroups (kListWaves * grid entries; the last op for waves without tiles).
template <class Op>
inline void list_wave_ops(const Op *ops, uint32_t n, uint64_t total_tiles, uint32_t grid, uint32_t *out) {
    const uint64_t waves = (uint64_t)grid * kListWaves;
    uint32_t i = 0;
    for (uint64_t w = 0; w < waves; w++) {
        uint64_t t0, t1;
        list_wave_range(w, grid, total_tiles, &t0, &t1);
        while (i + 1 < n && ops[i + 1].first_tile <= t0) i++;
        out[w] = i;
    }
}

// ---- ops with rows (strided, strided converting, indexed, indexed converting) ----
// Every row of an op has tiles_per_row tiles: tile t of the op is piece t % tiles_per_row
// of row t / tiles_per_row. A wave locates the first tile it has in an op (the only
// divide) and counts from then on. The kernels and the stand-alone test programs run
// these three functions; `K` is the width a kind keeps the piece number in.

// Row and piece of tile t (relative to the op's first tile). The divide is by a
// wave-uniform value.
template <class K>
OCM_LIST_HD inline void list_locate(uint64_t tiles_per_row, uint64_t t, uint64_t *row, K *k) {
    if (tiles_per_row == 1) {  // rows of at most one tile (KV blocks, embedding rows): no divide
        *row = t;
        *k = 0;
        return;
    }
    *row = t / tiles_per_row;
    *k = (K)(t - *row * tiles_per_row);
}

// A loader that takes a descriptor field as it is (the kernels pass one that moves it
// to scalar registers).
struct ListLoadPlain {
    OCM_LIST_HD uint64_t operator()(uint64_t v) const { return v; }
};

// Enters the op of tile t: advances *i from an op at or before it, past empty ops, until
// the op after *i starts beyond t. Returns that op's first tile, where the wave has to
// enter again (past every tile when *i is the last op).
template <class Op, class Load = ListLoadPlain>
OCM_LIST_HD inline uint64_t list_enter_op(const Op *ops, uint32_t n_ops, uint64_t t, uint32_t *i, Load load = Load()) {
    for (;;) {
        const uint64_t next = *i + 1 < n_ops ? load(ops[*i + 1].first_tile) : ~0ull;
        if (next > t) return next;
        ++*i;
    }
}

// The tile after piece *k of row *row. True: it is piece 0 of the next row.
template <class K>
OCM_LIST_HD inline bool list_next_piece(K tiles_per_row, uint64_t *row, K *k) {
    if (++*k != tiles_per_row) return false;
    *k = 0;
    ++*row;
    return true;
}

}  // namespace ocm
