// The plan every descriptor list shares (batch, converting, strided and accumulate
// ops: ocm/xfer.h, ocm/quant.h, ocm/strided.h, ocm/acc.h). A list is cut into
// wave-tiles; the host prefix-sums each op's tile count into `first_tile`, sizes a
// grid of workgroups of kListWaves waves, and every wave takes one contiguous tile
// range plus the op its first tile belongs to (the wave table), so waves never
// search: they walk forward through the ops they cover. How many tiles an op has is
// the kind's own rule, defined beside its geometry and passed in here.
//
// A wrong tile count or a range cut two ways would size a grid for tiles that no
// wave copies, so each of these expressions exists once: the kernels, the host plans
// and the stand-alone test programs (ocm_list_tests.cpp) share this header; it needs
// no HIP.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define OCM_LIST_HD __host__ __device__
#else
#define OCM_LIST_HD
#endif

namespace ocm {

constexpr int kListWaves = 4;  // waves of a workgroup (kWaves of the kernels)

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

}  // namespace ocm
