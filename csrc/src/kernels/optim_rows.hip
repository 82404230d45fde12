// gfx950 row-sparse fused Adam over an embedding table and its optimizer state in remote
// memory (ocm/adam_rows.h): one launch updates the rows that an id array picks, where they
// live, with the dense kernel's element rule (adam_rule.h).
//
// A wave walks a contiguous tile range (list_wave_range), as xfer_indexed_kernel does; tile
// t is piece k of row j (list_locate: one divide per wave, none for rows of one tile),
// 64 lanes x one 16-byte fp32 vector. For a tile of row j the wave loads ids[j] into a scalar
// register (uniform32 / uniform64) and applies the bounds rule; a row whose id is outside
// the table is skipped whole, and the wave that owns its piece 0 counts it, one device-scope
// atomic add from one lane. The ids of a round's tiles are loaded together, ahead of the
// round's vectors: pieces of one row load the same word again, from the same cache line.
//
// Each lane of an in-range row loads one vector of exp_avg, exp_avg_sq and the weight
// through state_ptr() (two spaces: the table's pair and the state's, each with its own
// extent table and stripe shift) and one of the gradient from local HBM, runs adam1 on four
// elements and stores the three back. A 16-byte vector at a 16-byte aligned offset, or an
// 8-byte bf16 vector at an 8-byte aligned one, never crosses a stripe unit, so the extent
// arithmetic runs once per vector. Embedding rows are short (a 64-wide fp32 row is a
// quarter of a wave), so a wave issues the loads of kAdamRowsInFlight tiles, of as many
// rows, before the first use: the remote round trip is paid once per round, not per row.
//
// kBf16: the table is bf16 and is only written; the update runs on fp32 master rows in the
// state, and the table row gets their round-to-nearest-even (f32_to_bf16). The gradient is
// bf16 as well.
#include <hip/hip_runtime.h>

#include "adam_rule.h"
#include "ocm/adam_rows.h"
#include "state_space.h"
#include "xfer_copy.h"

namespace ocm {

namespace {

constexpr int kRowsThreads = kListWaves * 64;

// Entry j of the id array as the lane loads it (every lane the same word), and widened for the
// bounds rule, in scalar registers. The two are apart so that a round's id loads are all issued
// before the first is waited for: the wait for an id also waits for every vector load before it.
__device__ __forceinline__ uint64_t load_id(const void *ids, uint32_t index_type, uint64_t j) {
    if (index_type == OCM_INDEX_I64) return static_cast<const uint64_t *>(ids)[j];
    return static_cast<const uint32_t *>(ids)[j];
}

__device__ __forceinline__ uint64_t row_id(uint64_t raw, uint32_t index_type) {
    if (index_type == OCM_INDEX_I64) return uniform64(raw);
    return indexed_widen32(uniform32((uint32_t)raw));
}

template <bool kBf16, int kV>
__global__ __launch_bounds__(kRowsThreads) void adam_rows_kernel(AdamRowsArgs a) {
    // wave index, made scalar: everything below but the lane's own vectors is wave-uniform
    const uint32_t w = __builtin_amdgcn_readfirstlane(blockIdx.x * kListWaves + (threadIdx.x >> 6));
    uint64_t t, t1;
    list_wave_range(w, a.grid, a.total_tiles, &t, &t1);
    if (t >= t1) return;
    const uint32_t lane = threadIdx.x & 63;
    const ocm_adam_rows &d = a.d;
    const StateSpace &c = a.c.state;
    uint64_t j, k;  // tile t is piece k of row j
    list_locate(a.tiles_per_row, t, &j, &k);
    j = uniform64(j);
    k = uniform64(k);
    for (; t < t1; t += kV) {
        f32x4 wv[kV], m[kV], v[kV], g[kV];
        f32x4 *wp[kV], *mp[kV], *vp[kV];
        u16x4 *tp[kV];
        bool live[kV];
        uint64_t raw[kV];
        {  // the ids of the round's rows: one load per slot, all issued before the first use
            uint64_t jj = j, kk = k;
#pragma unroll
            for (int u = 0; u < kV; u++) {
                raw[u] = 0;
                if (t + u >= t1) continue;
                raw[u] = load_id(a.ids, d.index_type, jj);
                if (++kk == a.tiles_per_row) {
                    kk = 0;
                    jj++;
                }
            }
        }
#pragma unroll
        for (int u = 0; u < kV; u++) {
            live[u] = false;
            if (t + u >= t1) continue;
            const uint64_t id = row_id(raw[u], d.index_type);
            const bool ok = adam_rows_picks(id, d.table_rows);
            // counted once per row: by the wave that owns its piece 0
            if (!ok && k == 0 && lane == 0 && a.skipped) atomicAdd(a.skipped, 1ull);
            const uint64_t e = adam_rows_elem(k, lane);
            live[u] = ok && e < d.dim;
            if (live[u]) {
                // in range, and every table fits its half (adam_rows_check): no product overflows
                mp[u] = reinterpret_cast<f32x4 *>(state_ptr(c, d.m_off + id * d.m_stride + (e << 2)));
                vp[u] = reinterpret_cast<f32x4 *>(state_ptr(c, d.v_off + id * d.v_stride + (e << 2)));
                m[u] = __builtin_nontemporal_load(mp[u]);
                v[u] = __builtin_nontemporal_load(vp[u]);
                const uint64_t ge = j * d.g_stride + e;
                if constexpr (kBf16) {
                    wp[u] = reinterpret_cast<f32x4 *>(state_ptr(c, d.w_off + id * d.w_stride + (e << 2)));
                    tp[u] = reinterpret_cast<u16x4 *>(state_ptr(a.table, d.table_off + id * d.table_stride + (e << 1)));
                    const u16x4 gh = __builtin_nontemporal_load(reinterpret_cast<const u16x4 *>(
                        static_cast<const unsigned short *>(a.g) + ge));
#pragma unroll
                    for (int i = 0; i < 4; i++) g[u][i] = bf16_to_f32(gh[i]);
                } else {
                    wp[u] = reinterpret_cast<f32x4 *>(state_ptr(a.table, d.table_off + id * d.table_stride + (e << 2)));
                    g[u] = __builtin_nontemporal_load(reinterpret_cast<const f32x4 *>(static_cast<const float *>(a.g) + ge));
                }
                wv[u] = __builtin_nontemporal_load(wp[u]);
            }
            if (++k == a.tiles_per_row) {
                k = 0;
                j++;
            }
        }
#pragma unroll
        for (int u = 0; u < kV; u++) {
            if (!live[u]) continue;
#pragma unroll
            for (int i = 0; i < 4; i++) {
                float wi = wv[u][i], mi = m[u][i], vi = v[u][i];
                adam1(wi, acc_grad(a.gscale, g[u][i]), mi, vi, a.c.h);
                wv[u][i] = wi;
                m[u][i] = mi;
                v[u][i] = vi;
            }
            if constexpr (kBf16) {
                u16x4 out;
#pragma unroll
                for (int i = 0; i < 4; i++) out[i] = f32_to_bf16(wv[u][i]);
                __builtin_nontemporal_store(out, tp[u]);
            }
            __builtin_nontemporal_store(wv[u], wp[u]);
            __builtin_nontemporal_store(m[u], mp[u]);
            __builtin_nontemporal_store(v[u], vp[u]);
        }
    }
}

}  // namespace

hipError_t adam_rows_launch(const AdamRowsArgs &a, const AdamKnobs &knobs, hipStream_t stream) {
    const ocm_adam_rows &d = a.d;
    if (d.rows == 0) return hipSuccess;
    if (!state_space_ok(a.c.state) || !state_space_ok(a.table)) return hipErrorInvalidValue;
    if (!a.ids || !a.g || d.dim == 0 || d.dim % 4 || d.rows >= (1ull << 32) || d.table_rows >= (1ull << 32) ||
        (d.index_type != OCM_INDEX_I32 && d.index_type != OCM_INDEX_I64))
        return hipErrorInvalidValue;
    const uintptr_t tal = d.bf16 ? 7u : 15u;
    if (((uintptr_t)a.g & tal) || ((uintptr_t)a.ids & (indexed_index_bytes(d.index_type) - 1)) || (d.g_stride & 3u) ||
        ((d.table_off | d.table_stride) & tal) || ((d.m_off | d.m_stride | d.v_off | d.v_stride) & 15u) ||
        (d.bf16 && ((d.w_off | d.w_stride) & 15u)))
        return hipErrorInvalidValue;
    const AdamRowsShape s = adam_rows_launch_shape(d.rows, d.dim, optim_cus(), knobs);
    if (s.grid == 0) return hipSuccess;
    AdamRowsArgs x = a;
    x.grid = s.grid;
    x.tiles_per_row = s.tiles_per_row;
    x.total_tiles = s.total_tiles;
    auto kernel = d.bf16 ? adam_rows_kernel<true, kAdamRowsInFlight> : adam_rows_kernel<false, kAdamRowsInFlight>;
    hipLaunchKernelGGL(kernel, dim3(x.grid), dim3(kRowsThreads), 0, stream, x);
    return hipGetLastError();
}

}  // namespace ocm
