// gfx950 one-sided transfer kernels (put/get over xGMI, HBM and pinned host).
//
// See ocm/xfer.h for the contract. Two variants:
//   XFER_REG  register-staged: each lane keeps UNROLL 16-byte loads in flight,
//             then issues UNROLL 16-byte stores (nontemporal on the destination).
//   XFER_LDS  LDS-DMA staged: each wave streams its 8 KiB slice of a tile into a
//             wave-private LDS double buffer with global_load_lds_dwordx4 while
//             it drains the previous tile from LDS (ds_read_b128 + global store).
//             Wave-private buffers need no workgroup barrier; ordering is the
//             issuing wave's own counted vmcnt (guide: "Pipelining across barriers").
// Work decomposition: the striped address space is cut into tiles aligned to
// the tile size (a power of two <= stripe unit), so a tile never crosses a
// stripe unit and maps to one contiguous range on both sides. Workgroups
// grid-stride over tiles; per-tile extent/offset math runs once per workgroup.
// The copy loop and the tile geometry are in xfer_copy.h.
// Reference parity: the one-sided data movers they replace are ib_read /
// ib_write (one signaled RDMA READ/WRITE work request, post_send src/rdma.c:47-92)
// and extoll_read / extoll_write (8 MiB chunks, 2 outstanding, extoll_rma2_transfer
// src/extoll.c:40-167).
#include <hip/hip_runtime.h>

#include <cstring>

#include "ocm/xfer.h"
#include "xfer_copy.h"
#include "xfer_host.h"

namespace ocm {

namespace {

constexpr int kWaveSlice = (1 << kTileShift) / kWaves;        // 8 KiB per wave per tile
constexpr int kChunksPerWave = kWaveSlice / 1024;             // 8 glds (1 KiB each) per wave per tile

// This workgroup's tiles blockIdx.x, blockIdx.x + grid, ... of `a`, each copied
// with Cfg. MASKED (the push kernel): only tiles of the extents in `ext_mask`.
template <class Cfg, bool MASKED = false>
__device__ __forceinline__ void copy_tiles(const XferArgs &a, uint32_t ext_mask = 0) {
    const uint64_t first = xfer_first_tile(a.rem_off, a.tile_shift);
    const uint64_t ntiles = xfer_tile_count(a.rem_off, a.len, a.tile_shift);
    const uint64_t r0 = a.rem_off;
    for (uint64_t ti = blockIdx.x; ti < ntiles; ti += gridDim.x) {
        if (MASKED && a.n_ext > 1) {
            const uint64_t lo = first + (ti << a.tile_shift);
            const uint64_t ts = lo > r0 ? lo : r0;
            const uint32_t e = (uint32_t)(ts >> a.unit_shift) % a.n_ext;
            if (!((ext_mask >> e) & 1u)) continue;  // workgroup-uniform
        }
        TileSpan s = tile_span(a, ti, first);
        copy_span<Cfg>(s.dst, s.src, s.n);
    }
}

template <int ST>
__global__ __launch_bounds__(kThreads) void xfer_reg_kernel(XferArgs a, XferDone d) {
    copy_tiles<BlockCopy<ST>>(a);
    xfer_publish(d);
}

// ---- LDS-DMA variant ----
typedef __attribute__((address_space(3))) void lds_void;
typedef const __attribute__((address_space(1))) void glob_void;

__device__ __forceinline__ bool full_aligned(const TileSpan &s) {
    return s.n == (1ull << kTileShift) && (((uintptr_t)s.dst | (uintptr_t)s.src) & 15u) == 0;
}

// Issue this wave's 8 x 1 KiB LDS-DMA loads of a full tile into `buf`.
__device__ __forceinline__ void stage_tile(const char *src, char *buf, int wave, int lane) {
    const char *g = src + (size_t)wave * kWaveSlice + (size_t)lane * 16;
    char *l = buf + (size_t)wave * kWaveSlice;  // wave-uniform LDS base; lane offset is implicit
#pragma unroll
    for (int c = 0; c < kChunksPerWave; c++)
        __builtin_amdgcn_global_load_lds((glob_void *)(g + c * 1024), (lds_void *)(l + c * 1024), 16, 0, 0);
}

template <bool NT>
__device__ __forceinline__ void drain_tile(char *dst, const char *buf, int wave, int lane) {
    const char *l = buf + (size_t)wave * kWaveSlice + (size_t)lane * 16;
    char *g = dst + (size_t)wave * kWaveSlice + (size_t)lane * 16;
    u32x4 v[kChunksPerWave];
#pragma unroll
    for (int c = 0; c < kChunksPerWave; c++) v[c] = *reinterpret_cast<const u32x4 *>(l + c * 1024);
#pragma unroll
    for (int c = 0; c < kChunksPerWave; c++)
        store16<NT>(reinterpret_cast<u32x4 *>(g + c * 1024), v[c]);
}

// Body of the LDS-DMA kernel: this workgroup's tiles ti, ti + grid, ...
template <bool NT>
__device__ __forceinline__ void lds_stream(const XferArgs &a, char *lds, int wave, int lane, uint64_t ti,
                                           uint64_t first, uint64_t ntiles) {
    TileSpan cur = tile_span(a, ti, first);
    bool cur_staged = full_aligned(cur);
    if (cur_staged) stage_tile(cur.src, lds, wave, lane);
    int slot = 0;
    for (;;) {
        const uint64_t nt = ti + gridDim.x;
        TileSpan nxt;
        bool nxt_staged = false;
        if (nt < ntiles) {
            nxt = tile_span(a, nt, first);
            nxt_staged = full_aligned(nxt);
            if (nxt_staged) stage_tile(nxt.src, lds + (slot ^ 1) * (1 << kTileShift), wave, lane);
        }
        if (cur_staged) {
            // Retire this wave's loads of `cur`, leaving the next tile's 8 in flight.
            if (nxt_staged)
                asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
            else
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            drain_tile<NT>(cur.dst, lds + slot * (1 << kTileShift), wave, lane);
        } else {
            copy_span<BlockCopy<NT ? ST_NT : ST_PLAIN>>(cur.dst, cur.src, cur.n);
        }
        if (nt >= ntiles) break;
        ti = nt;
        cur = nxt;
        cur_staged = nxt_staged;
        slot ^= 1;
    }
}

template <bool NT>
__global__ __launch_bounds__(kThreads) void xfer_lds_kernel(XferArgs a, XferDone d) {
    // One LDS array (guide: a second __shared__ object can de-pipeline glds).
    __shared__ __attribute__((aligned(16))) char lds[2 * (1 << kTileShift)];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const uint64_t first = xfer_first_tile(a.rem_off, a.tile_shift);
    const uint64_t ntiles = xfer_tile_count(a.rem_off, a.len, a.tile_shift);
    uint64_t ti = blockIdx.x;
    if (ti < ntiles) lds_stream<NT>(a, lds, wave, lane, ti, first, ntiles);  // grid <= ntiles: always true
    xfer_publish(d);
}

// ---- PCIe streaming variant (host-tier extents) ----
// Large ops between this GPU's HBM and the pinned host tier are bound by PCIe,
// not by the CUs, and the 32 KiB-tile register kernel on a full-chip grid
// stays at 54-55 GB/s. Measured over shapes (tools/pcie_stream_probe.hip,
// profiles/pcie_stream_r03.json, 256 MiB, against hipMemcpyAsync at 56.8-57.1):
//   get (host -> HBM): 2 loads in flight per lane and 128 workgroups reach
//       57.4 GB/s; cache bits of either side change nothing; full-chip grids
//       lose up to 2 GB/s (too many streams scatter the read window);
//   put (HBM -> host): write-through (sc1) stores are the whole difference,
//       57.0 against 55.5 GB/s with plain or nontemporal stores, flat from 48
//       to 256 workgroups.
// So: 8 KiB tiles (256 lanes x 16 B x 2), grid-strided over a small grid, and
// sc1 stores when the destination is the host tier.
constexpr int kPcieUnroll = 2;
constexpr uint32_t kPcieTileShift = 13;  // 256 x 16 B x kPcieUnroll
constexpr unsigned kPcieBlocksDefault = 128;

// SA: store bits (kAuxSC1 when the destination is the host tier).
template <int SA>
using PcieCopy = CopyCfg<kThreads, kPcieUnroll, BufferAccess<kAuxNT, SA>>;

template <int SA>
__global__ __launch_bounds__(kThreads) void xfer_pcie_kernel(XferArgs a, XferDone d) {
    copy_tiles<PcieCopy<SA>>(a);
    xfer_publish(d);
}

// ---- push-based get ----
// Launched on an owner's GPU: tiles of the extents in `mask` only (the other
// owners' launches take the rest); loads from this GPU's HBM, nontemporal
// stores into the app's buffer on another GPU over xGMI.
__global__ __launch_bounds__(kThreads) void xfer_push_kernel(XferArgs a, uint32_t mask) {
    copy_tiles<BlockCopy<ST_NT>, true>(a, mask);
}

}  // namespace

XferTuning xfer_tuning_from_env() {
    XferTuning t;
    const char *v = std::getenv("OCM_XFER_VARIANT");
    if (v && (!std::strcmp(v, "lds") || !std::strcmp(v, "2"))) t.variant = XFER_LDS;
    if (v && (!std::strcmp(v, "reg") || !std::strcmp(v, "1"))) t.variant = XFER_REG;
    if (v && (!std::strcmp(v, "pcie") || !std::strcmp(v, "4"))) t.variant = XFER_PCIE;
    if (v && (!std::strcmp(v, "push") || !std::strcmp(v, "5"))) t.variant = XFER_PUSH;
    t.max_blocks = kernels::env_int("OCM_XFER_BLOCKS", 0);
    t.nontemporal = kernels::env_int("OCM_XFER_NT", 1) != 0;
    t.write_through = kernels::env_int("OCM_XFER_NT", 1) == 2;  // 2: sc1 loads and stores (register kernel)
    return t;
}

hipError_t xfer_normalize(XferArgs &a) {
    if (a.n_ext < 1 || a.n_ext > (uint32_t)kXferMaxExtents) return hipErrorInvalidValue;
    a.tile_shift = kTileShift;
    if (a.n_ext > 1) {
        if (a.unit_shift < 4) return hipErrorInvalidValue;
        if (a.unit_shift < kTileShift) a.tile_shift = a.unit_shift;  // tile must not cross a stripe unit
    }
    return hipSuccess;
}

hipError_t xfer_launch(const XferArgs &in, const XferTuning &t, hipStream_t stream, const XferDone *done) {
    if (in.len == 0) return hipSuccess;
    XferArgs a = in;
    if (xfer_normalize(a) != hipSuccess) return hipErrorInvalidValue;
    const uint64_t ntiles = xfer_tile_count(a.rem_off, a.len, a.tile_shift);
    int variant = t.variant;
    if (variant == XFER_AUTO) variant = XFER_REG;
    const XferDone d0 = done ? *done : XferDone{};
    if (variant == XFER_PCIE) {
        if (a.tile_shift > kPcieTileShift) a.tile_shift = kPcieTileShift;
        const uint64_t tiles = xfer_tile_count(a.rem_off, a.len, a.tile_shift);
        const uint64_t cap = t.max_blocks > 0 ? (uint64_t)t.max_blocks : (uint64_t)kPcieBlocksDefault;
        const unsigned g = (unsigned)(tiles < cap ? tiles : cap);
        // sc1 (write-through) stores into the host tier, plain ones into HBM
        if (a.put && t.nontemporal)
            hipLaunchKernelGGL(xfer_pcie_kernel<kAuxSC1>, dim3(g), dim3(kThreads), 0, stream, a, d0);
        else
            hipLaunchKernelGGL(xfer_pcie_kernel<0>, dim3(g), dim3(kThreads), 0, stream, a, d0);
        return hipGetLastError();
    }
    if (a.tile_shift != kTileShift) variant = XFER_REG;  // LDS path is built for 32 KiB tiles
    // Grid caps from the round-1 sweep (profiles/ksweep_r01.json): LDS-DMA
    // peaks at 4 blocks per CU (2 resident, 64 KiB LDS each), the register
    // path at 2 per CU; never more blocks than tiles.
    int cap = t.max_blocks > 0 ? t.max_blocks : kernels::num_cus() * (variant == XFER_LDS ? 4 : 2);
    const unsigned grid = (unsigned)(ntiles < (uint64_t)cap ? ntiles : (uint64_t)cap);
    if (variant == XFER_LDS) {
        if (t.nontemporal)
            hipLaunchKernelGGL(xfer_lds_kernel<true>, dim3(grid), dim3(kThreads), 0, stream, a, d0);
        else
            hipLaunchKernelGGL(xfer_lds_kernel<false>, dim3(grid), dim3(kThreads), 0, stream, a, d0);
    } else {
        if (t.write_through)
            hipLaunchKernelGGL(xfer_reg_kernel<ST_WT>, dim3(grid), dim3(kThreads), 0, stream, a, d0);
        else if (t.nontemporal)
            hipLaunchKernelGGL(xfer_reg_kernel<ST_NT>, dim3(grid), dim3(kThreads), 0, stream, a, d0);
        else
            hipLaunchKernelGGL(xfer_reg_kernel<ST_PLAIN>, dim3(grid), dim3(kThreads), 0, stream, a, d0);
    }
    return hipGetLastError();
}

hipError_t xfer_push_launch(const XferArgs &in, uint32_t ext_mask, int max_blocks, hipStream_t stream) {
    if (in.len == 0 || ext_mask == 0) return hipSuccess;
    XferArgs a = in;
    if (a.put || xfer_normalize(a) != hipSuccess) return hipErrorInvalidValue;
    const uint64_t tiles = xfer_tile_count(a.rem_off, a.len, a.tile_shift);
    const uint32_t mine = (uint32_t)__builtin_popcount(ext_mask & ((1u << a.n_ext) - 1));
    const uint64_t own = a.n_ext > 1 ? (tiles * mine + a.n_ext - 1) / a.n_ext : tiles;
    const uint64_t cap = max_blocks > 0 ? (uint64_t)max_blocks : (uint64_t)kernels::num_cus() * 2;
    const unsigned g = (unsigned)(own < cap ? (own ? own : 1) : cap);
    hipLaunchKernelGGL(xfer_push_kernel, dim3(g), dim3(kThreads), 0, stream, a, ext_mask);
    return hipGetLastError();
}

hipError_t xfer_copy(void *dst, const void *src, uint64_t bytes, const XferTuning &t, hipStream_t stream) {
    XferArgs a;
    std::memset(&a, 0, sizeof(a));
    a.lin = const_cast<char *>(static_cast<const char *>(src));
    a.ext[0] = static_cast<char *>(dst);
    a.rem_off = 0;
    a.len = bytes;
    a.n_ext = 1;
    a.put = 1;
    return xfer_launch(a, t, stream);
}

}  // namespace ocm
