// Pooled embedding lookup (ocm_copy_onesided_bag) as one launch: every bag's table rows
// are read out of the remote half and summed in registers, and only the sum is written;
// see ocm/bag.h for the descriptors, the rule (defined bit for bit) and the plan.
//
// A wave walks a contiguous tile range, as in xfer_indexed_kernel; tile t is piece k of
// BAG b (list_locate of ocm/list.h: the only divide, skipped for rows of one tile): lane l
// owns the 16-byte vector at byte 1024 k + 16 l of the row, four fp32 or eight 16-bit
// elements, whose fp32 accumulators stay in its registers from the bag's first id to its
// last. No LDS and no cross-lane traffic: a lane reads and writes only its own vector.
// The host plan cannot see bag lengths, so a wave's work per tile is proportional to its
// bag's length (ocm/bag.h).
//
// Entering a bag the wave loads off[b] and off[b + 1] into scalar registers and walks the
// ids as wave-uniform scalars, a window of kBagInFlight at a time: the window's ids (and
// weights) are loaded together, then the row vectors of its leading in-range ids with
// nothing between them, so a bag pays about len / kBagInFlight round trips to the pool,
// not len. The loads of a window nest (slot u + 1 is loaded only if slot u was): side by
// side, each under a condition of its own, the compiler waits for every load before it
// issues the next. A window ends early at the bag's end or in front of an out-of-range id,
// which is counted and stepped over: no load is ever issued for it. Every remote vector is
// mapped through the extents on its own (stripe_ptr): offsets and strides are multiples of
// 16 and a stripe unit is at least 16 bytes, so no vector straddles a unit and rows that
// cross units need no splitting, as in xfer_acc.hip.
//
// The only atomic is the skip count: one add of the bag's bad entries, from one lane of
// the wave that owns piece 0 of the bag. Element type and weights-or-not are template
// parameters of the piece (the accumulators of 16-bit rows are eight registers, of fp32
// rows four), chosen by wave-uniform branches on descriptor fields, as is int32 / int64.
// The op is a get: the stores go to the local half, nontemporal or plain (NT).
#include <hip/hip_runtime.h>

#include "ocm/bag.h"
#include "ocm/xfer.h"
#include "xfer_copy.h"
#include "xfer_host.h"

namespace ocm {

namespace {

// Both halves are global memory; saying so keeps every access a global_ one.
typedef __attribute__((address_space(1))) u32x4 *GlobalVec;

// Entry j of an id or offsets array as the lane loads it (every lane the same word), and
// widened for the rule, in scalar registers. The two are apart so that a window's loads are
// all issued before the first is waited for.
__device__ __forceinline__ uint64_t bag_load_index(const char *arr, uint32_t index_type, uint32_t j) {
    if (index_type == OCM_INDEX_I64) return reinterpret_cast<const uint64_t *>(arr)[j];
    return reinterpret_cast<const uint32_t *>(arr)[j];
}
__device__ __forceinline__ uint64_t bag_index(uint64_t raw, uint32_t index_type) {
    if (index_type == OCM_INDEX_I64) return uniform64(raw);
    return indexed_widen32(uniform32((uint32_t)raw));
}

// The vector of a lane as elements.
template <uint32_t DT>
struct BagVec {
    static constexpr int kElems = 8;  // 16-bit elements
    static __device__ __forceinline__ float elem(const u32x4 &v, int e) {
        const uint32_t w = v[e >> 1];
        return acc_widen16((e & 1) ? (w >> 16) : (w & 0xffffu), DT == kAccBf16);
    }
    static __device__ __forceinline__ u32x4 pack(const float (&r)[kElems]) {
        u32x4 o;
#pragma unroll
        for (int i = 0; i < 4; i++)
            o[i] = bag_narrow16(r[2 * i], DT == kAccBf16) | (bag_narrow16(r[2 * i + 1], DT == kAccBf16) << 16);
        return o;
    }
};
template <>
struct BagVec<kAccF32> {
    static constexpr int kElems = 4;
    static __device__ __forceinline__ float elem(const u32x4 &v, int e) { return acc_bits_float(v[e]); }
    static __device__ __forceinline__ u32x4 pack(const float (&r)[kElems]) {
        u32x4 o;
#pragma unroll
        for (int i = 0; i < 4; i++) o[i] = acc_float_bits(r[i]);
        return o;
    }
};

// Slots U.. of a window of n: a slot is loaded only if the one before it was, so the
// conditions nest and the loads follow each other with nothing between them.
template <int U>
__device__ __forceinline__ void bag_loads(const GlobalVec (&p)[kBagInFlight], uint32_t n, u32x4 (&v)[kBagInFlight]) {
    if ((uint32_t)U < n) {
        v[U] = __builtin_nontemporal_load(p[U]);
        if constexpr (U + 1 < kBagInFlight) bag_loads<U + 1>(p, n, v);
    }
}

// Piece k of bag b of op *d: the lane's vector of the bag's output row. Returns the
// bag's entries with an id outside the table (the same for every piece of the bag).
template <uint32_t DT, bool WEIGHTS, bool NT>
__device__ __forceinline__ uint32_t bag_piece(const XferBagArgs &a, const XferBagOp *d, uint64_t b, uint32_t k, uint32_t lane) {
    using V = BagVec<DT>;
    const uint32_t type = uniform32(d->index_type);
    const uint32_t ids = uniform32(d->ids), rem_rows = uniform32(d->rem_rows);
    const char *idx = a.lin + uniform64(d->idx_off);
    const float *wts = reinterpret_cast<const float *>(a.lin + uniform64(d->w_off));  // read only with WEIGHTS
    uint32_t lo, hi;
    {
        const char *offs = a.lin + uniform64(d->offs_off);
        const uint64_t r0 = bag_load_index(offs, type, (uint32_t)b), r1 = bag_load_index(offs, type, (uint32_t)b + 1);
        bag_bounds(bag_index(r0, type), bag_index(r1, type), ids, &lo, &hi);
    }
    const uint32_t vb = (k << kBagTileShift) + (lane << 4);  // the lane's vector, bytes into the row
    const bool live = vb < uniform32(d->row_bytes);           // row_bytes % 16 == 0: a vector is inside or outside
    const uint64_t rem0 = uniform64(d->rem_off) + vb, rem_stride = uniform64(d->rem_stride);
    float acc[V::kElems];
#pragma unroll
    for (int e = 0; e < V::kElems; e++) acc[e] = 0.0f;
    uint32_t bad = 0;
    for (uint32_t j = lo; j < hi;) {
        // the window's ids and weights: slots past the bag's end read its last entry again
        uint64_t raw[kBagInFlight];
        float w[kBagInFlight];
#pragma unroll
        for (int u = 0; u < kBagInFlight; u++) {
            const uint32_t ju = (uint64_t)j + u < hi ? j + u : hi - 1;
            raw[u] = bag_load_index(idx, type, ju);
            if constexpr (WEIGHTS) w[u] = wts[ju];
        }
        // n: the leading slots that are entries of the bag with an id inside the table
        uint32_t n = 0;
        uint64_t rem[kBagInFlight];  // the lane's vector of each slot's row, striped coordinates
#pragma unroll
        for (int u = 0; u < kBagInFlight; u++) {
            const uint64_t id = bag_index(raw[u], type);
            if (n == (uint32_t)u && (uint64_t)j + u < hi && indexed_in_range(id, rem_rows)) n = u + 1;
            if constexpr (WEIGHTS)
                w[u] = acc_bits_float(uniform32(acc_float_bits(w[u])));
            else
                w[u] = 1.0f;
            // in range, and the table fits its half (bag_check_op): the product cannot overflow.
            // A slot that is not loaded maps row 0 and touches nothing.
            rem[u] = rem0 + (n == (uint32_t)u + 1 ? id : 0) * rem_stride;
        }
        // Addresses first: with several extents stripe_ptr reads an extent base per lane, and the
        // window's reads share one wait here instead of one in front of each data load.
        GlobalVec p[kBagInFlight];
        const uint32_t n_ext = a.n_ext;  // kernel argument: uniform
        if (n_ext == 1) {
#pragma unroll
            for (int u = 0; u < kBagInFlight; u++) p[u] = (GlobalVec)stripe_ptr(a, 1u, 0u, rem[u]);
        } else {
            __builtin_assume(n_ext > 1);
#pragma unroll
            for (int u = 0; u < kBagInFlight; u++) p[u] = (GlobalVec)stripe_ptr(a, n_ext, a.unit_shift, rem[u]);
        }
        u32x4 v[kBagInFlight];
#pragma unroll
        for (int u = 0; u < kBagInFlight; u++) v[u] = u32x4{0, 0, 0, 0};
        if (live) bag_loads<0>(p, n, v);
#pragma unroll
        for (int u = 0; u < kBagInFlight; u++) {
            if ((uint32_t)u < n) {  // in the bag's order, slot by slot
#pragma unroll
                for (int e = 0; e < V::kElems; e++) acc[e] = acc_rule(acc[e], V::elem(v[u], e), w[u]);
            }
        }
        j += n;
        if (n < (uint32_t)kBagInFlight && j < hi) {  // the window ended in front of an id outside the table
            bad++;
            j++;
        }
    }
    if (uniform32(d->mode) == OCM_BAG_MEAN && hi > lo) {
#pragma unroll
        for (int e = 0; e < V::kElems; e++) acc[e] = bag_mean(acc[e], hi - lo);
    }
    if (live) {
        u32x4 *out = reinterpret_cast<u32x4 *>(a.lin + uniform64(d->lin_off) + b * uniform64(d->lin_stride) + vb);
        store16<NT>(out, V::pack(acc));
    }
    return bad;
}

template <bool NT>
__global__ __launch_bounds__(kThreads) void xfer_bag_kernel(XferBagArgs a) {
    // wave index, made scalar: everything below but the lane's own vectors is wave-uniform
    const uint32_t w = __builtin_amdgcn_readfirstlane(blockIdx.x * kWaves + (threadIdx.x >> 6));
    const uint32_t lane = threadIdx.x & 63u;
    uint64_t t, t1;
    list_wave_range(w, a.grid, a.total_tiles, &t, &t1);
    if (t >= t1) return;
    const XferBagOp *ops;
    uint32_t i = list_wave_start(a, w, &ops);
    uint64_t next = 0;            // first tile of the op after the one of tile t (none: past every tile)
    uint64_t tiles_per_row = 1;
    uint64_t b = 0, k = 0;        // tile t is piece k of the op's bag b
    uint32_t dtype = 0, weights = 0;
    for (; t < t1; t++) {
        if (t >= next) {  // the wave's first tile, or the op's tiles are done: enter the op of tile t
            next = list_enter_op(ops, a.n_ops, t, &i, ListLoadUniform());
            tiles_per_row = uniform64(ops[i].tiles_per_row);
            list_locate(tiles_per_row, t - uniform64(ops[i].first_tile), &b, &k);
            b = uniform64(b);
            k = uniform64(k);
            dtype = uniform32(ops[i].dtype);
            weights = uniform64(ops[i].w_off) != OCM_INDEX_NONE;
        }
        const XferBagOp *d = ops + i;
        uint32_t bad;
        if (dtype == kAccF32)
            bad = weights ? bag_piece<kAccF32, true, NT>(a, d, b, (uint32_t)k, lane) : bag_piece<kAccF32, false, NT>(a, d, b, (uint32_t)k, lane);
        else if (dtype == kAccBf16)
            bad = weights ? bag_piece<kAccBf16, true, NT>(a, d, b, (uint32_t)k, lane) : bag_piece<kAccBf16, false, NT>(a, d, b, (uint32_t)k, lane);
        else
            bad = weights ? bag_piece<kAccFp16, true, NT>(a, d, b, (uint32_t)k, lane) : bag_piece<kAccFp16, false, NT>(a, d, b, (uint32_t)k, lane);
        // counted once per entry: by the wave that owns piece 0 of the bag, in one add
        if (bad != 0 && k == 0 && lane == 0) atomicAdd(a.skipped, (unsigned long long)bad);
        list_next_piece(tiles_per_row, &b, &k);
    }
}

}  // namespace

hipError_t xfer_bag_launch(const XferBagArgs &a, const XferTuning &t, hipStream_t stream) {
    if (a.total_tiles == 0 || a.n_ops == 0) return hipSuccess;
    if (!kernels::list_args_valid<true>(a) || a.tile_shift != kBagTileShift || !a.lin || !a.skipped) return hipErrorInvalidValue;
    auto kernel = (a.host_tier || t.nontemporal) ? xfer_bag_kernel<true> : xfer_bag_kernel<false>;
    hipLaunchKernelGGL(kernel, dim3(a.grid), dim3(kThreads), 0, stream, a);
    hipError_t err = hipGetLastError();
    // the count so far, where the host reads it once the stream has got here (no atomics to host memory)
    if (err == hipSuccess && a.skipped_host)
        err = hipMemcpyAsync(a.skipped_host, a.skipped, sizeof(*a.skipped), hipMemcpyDeviceToHost, stream);
    return err;
}

}  // namespace ocm
