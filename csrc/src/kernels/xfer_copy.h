// Device-side primitives shared by the transfer kernels (xfer.hip, xfer_service.hip and
// the list kernels xfer_batch / _quant / _strided / _acc.hip): the one copy loop, tile
// geometry, how a wave enters a descriptor list, and the release / publish hand-off. Device only: include from a HIP translation unit, inside no namespace.
#pragma once
#include <hip/hip_runtime.h>

#include "ocm/list.h"
#include "ocm/xfer.h"

namespace ocm {

namespace {

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

constexpr int kThreads = 256;
constexpr int kUnroll = 8;                                    // 8 x 16 B in flight per lane
constexpr uint32_t kTileShift = 15;                           // 32 KiB tiles = 256 lanes x 16 B x 8
constexpr int kWaves = kThreads / 64;
static_assert(kWaves == kListWaves, "the host plans lists for workgroups of kListWaves waves");

// Store flavours of the copy loops:
//   ST_PLAIN  plain stores (cached in the XCD's L2);
//   ST_NT     nontemporal stores (streaming; still released by a fence);
//   ST_WT     write-through (sc1) stores: the bytes leave L2 for memory as they
//             are stored, so a drain (s_waitcnt vmcnt(0)) of every storing wave
//             is all a hand-off needs - no buffer_wbl2 release fence
//             (guide: Guideline 16 R1; MI355X_MICROARCH.md visibility table);
//             the loads of such a span are sc1 as well.
enum StoreKind : int { ST_PLAIN = 0, ST_NT = 1, ST_WT = 2 };

// Buffer descriptor over [base, base + bytes), built from wave-uniform values
// (every caller passes a workgroup-uniform span). Buffer accesses are range
// checked in hardware: a load past the end returns 0 without touching memory
// and a store past the end is dropped, so a partial tile needs no per-lane
// branches. (Branches around loads made the compiler put an s_waitcnt vmcnt(0)
// in front of each one inside the service loop: a partial host-tier tile then
// paid one PCIe round trip per 4 KiB.)
__device__ __forceinline__ __amdgpu_buffer_rsrc_t span_rsrc(const void *base, uint32_t bytes) {
    const uint64_t b = reinterpret_cast<uint64_t>(base);
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)b);
    const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(b >> 32));
    const uint32_t n = __builtin_amdgcn_readfirstlane(bytes);
    return __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<void *>(((uint64_t)hi << 32) | lo), 0, (int)n, 0x00020000);
}

// cache-policy bits of buffer accesses on gfx950: nt = 2, sc1 = 16
constexpr int kAuxNT = 2, kAuxSC1 = 16;

template <int ST>
constexpr int store_aux() {
    return ST == ST_WT ? kAuxSC1 : ST == ST_NT ? kAuxNT : 0;
}
// ST_WT spans are loaded sc1 too: such loads bypass the CU's L1 and read host /
// peer memory from memory rather than from stale L2 copies (measured:
// profiles/svc_copy_probe_r02.json), so the persistent service needs no acquire.
template <int ST>
constexpr int load_aux() {
    return ST == ST_WT ? kAuxSC1 : kAuxNT;
}

// One byte (head, tail, unaligned spans); ATOMIC: relaxed agent-scope atomics
// (sc1, like the vectors of a write-through span).
template <bool ATOMIC>
__device__ __forceinline__ void copy_byte(char *d, const char *s) {
    if constexpr (ATOMIC)
        __hip_atomic_store(d, __hip_atomic_load(s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
    else
        *d = *s;
}

// Bytes in front of the destination's first 16-byte boundary, at most n.
__device__ __forceinline__ uint64_t span_head(const char *dst, uint64_t n) {
    const uint64_t head = (16u - ((uintptr_t)dst & 15u)) & 15u;
    return head < n ? head : n;
}

// Plain / nt store of one vector through a pointer (LDS drain, batch waves).
// There is no write-through flavour: a pointer store carries no sc1 bit.
template <bool NT>
__device__ __forceinline__ void store16(u32x4 *p, u32x4 v) {
    if constexpr (NT)
        __builtin_nontemporal_store(v, p);
    else
        *p = v;
}

// ---- how a copy reaches its 16-byte vectors ----
// Through buffer descriptors over the aligned middle of the span, with cache bits
// LA / SA. Range checked: a round may run past the end (see span_rsrc).
template <int LA, int SA>
struct BufferAccess {
    static constexpr bool kRangeChecked = true;
    using Index = uint32_t;  // descriptor offsets are 32-bit: spans under 2 GiB
    __amdgpu_buffer_rsrc_t rs, rd;
    __device__ __forceinline__ BufferAccess(char *dst, const char *src, uint32_t bytes)
        : rs(span_rsrc(src, bytes)), rd(span_rsrc(dst, bytes)) {}
    __device__ __forceinline__ u32x4 load(Index i) const {
        return __builtin_amdgcn_raw_buffer_load_b128(rs, (int)(i << 4), 0, LA);
    }
    __device__ __forceinline__ void store(Index i, u32x4 v) const {
        __builtin_amdgcn_raw_buffer_store_b128(v, rd, (int)(i << 4), 0, SA);
    }
};

// Through pointers: nontemporal loads, plain or nontemporal (NT) stores. Nothing
// checks the range, so only full rounds are unrolled and the rest goes a vector
// at a time.
template <bool NT>
struct PointerAccess {
    static constexpr bool kRangeChecked = false;
    using Index = uint64_t;
    const u32x4 *s;
    u32x4 *d;
    __device__ __forceinline__ PointerAccess(char *dst, const char *src, uint64_t)
        : s(reinterpret_cast<const u32x4 *>(src)), d(reinterpret_cast<u32x4 *>(dst)) {}
    __device__ __forceinline__ u32x4 load(Index i) const { return __builtin_nontemporal_load(s + i); }
    __device__ __forceinline__ void store(Index i, u32x4 v) const { store16<NT>(d + i, v); }
};

// What a copy loop fixes at compile time: the lanes that cooperate (a workgroup
// of kThreads or one wave), the 16-byte loads each keeps in flight, the access
// policy, and whether the byte head / tail go as atomics.
template <int LANES, int UNROLL, class ACCESS, bool ATOMIC_BYTES = false>
struct CopyCfg {
    static_assert(LANES == kThreads || LANES == 64, "a workgroup or one wave");
    static constexpr int kLanes = LANES, kRound = LANES * UNROLL;  // vectors per round
    static constexpr int kVecs = UNROLL;
    static constexpr bool kAtomicBytes = ATOMIC_BYTES;
    using Access = ACCESS;
    __device__ static __forceinline__ int lane() { return LANES == 64 ? (int)(threadIdx.x & 63) : (int)threadIdx.x; }
};

// The workgroup-cooperative copy of the register, push and service kernels.
template <int ST>
using BlockCopy = CopyCfg<kThreads, kUnroll, BufferAccess<load_aux<ST>(), store_aux<ST>()>, ST == ST_WT>;

// One round: every load in flight before the first store.
template <class Cfg>
__device__ __forceinline__ void load_round(const typename Cfg::Access &acc, typename Cfg::Access::Index i,
                                           u32x4 (&v)[Cfg::kVecs]) {
#pragma unroll
    for (int k = 0; k < Cfg::kVecs; k++) v[k] = acc.load(i + k * Cfg::kLanes);
}

template <class Cfg>
__device__ __forceinline__ void store_round(const typename Cfg::Access &acc, typename Cfg::Access::Index i,
                                            const u32x4 (&v)[Cfg::kVecs]) {
#pragma unroll
    for (int k = 0; k < Cfg::kVecs; k++) acc.store(i + k * Cfg::kLanes, v[k]);
}

// Cooperative copy of n bytes by the lanes of Cfg: a byte head up to the
// destination's 16-byte alignment, rounds of vectors, a byte tail. Any n works
// (n <= one tile is the common case; range-checked spans of 2 GiB or more,
// which no caller makes, take the byte loop).
template <class Cfg>
__device__ __forceinline__ void copy_span(char *__restrict__ dst, const char *__restrict__ src, uint64_t n) {
    using Access = typename Cfg::Access;
    using Index = typename Access::Index;
    constexpr bool AB = Cfg::kAtomicBytes;
    const int lane = Cfg::lane();
    const uint64_t head = span_head(dst, n);
    if ((uint64_t)lane < head) copy_byte<AB>(dst + lane, src + lane);
    dst += head;
    src += head;
    n -= head;
    if (((uintptr_t)src & 15u) == 0 && (!Access::kRangeChecked || n < (1ull << 31))) {
        const Index nv = (Index)(n >> 4);
        const Access acc(dst, src, nv << 4);
        if constexpr (Access::kRangeChecked) {
            // past-the-end lanes of the last round are dropped by the range check
            for (Index base = 0; base < nv; base += Cfg::kRound) {
                u32x4 v[Cfg::kVecs];
                load_round<Cfg>(acc, base + lane, v);
                store_round<Cfg>(acc, base + lane, v);
            }
        } else {
            Index i = lane;
            for (; i + (Cfg::kRound - Cfg::kLanes) < nv; i += Cfg::kRound) {
                u32x4 v[Cfg::kVecs];
                load_round<Cfg>(acc, i, v);
                store_round<Cfg>(acc, i, v);
            }
            for (; i < nv; i += Cfg::kLanes) acc.store(i, acc.load(i));
        }
        const uint64_t done = (uint64_t)nv << 4, tail = n & 15u;
        if ((uint64_t)lane < tail) copy_byte<AB>(dst + done + lane, src + done + lane);
    } else {
        // Source and destination disagree mod 16: byte loop (rare; unaligned user offsets).
        for (uint64_t i = lane; i < n; i += Cfg::kLanes) copy_byte<AB>(dst + i, src + i);
    }
}

struct TileSpan {
    char *dst;
    const char *src;
    uint64_t n;
};

// Two tile spans with all their loads in flight before the first store: a
// workgroup that copies two tiles from a far source (host tier over PCIe, peer
// HBM over xGMI) pays one read round trip instead of two. Each span is at most
// one round. Spans whose source and destination disagree mod 16 (unaligned user
// offsets), or longer ones, go one after the other.
template <class Cfg>
__device__ __forceinline__ void copy_span2(const TileSpan &a, const TileSpan &b) {
    using Access = typename Cfg::Access;
    static_assert(Access::kRangeChecked, "a partial round relies on the range check");
    constexpr bool AB = Cfg::kAtomicBytes;
    const bool vec = (((uintptr_t)a.src ^ (uintptr_t)a.dst) & 15u) == 0 &&
                     (((uintptr_t)b.src ^ (uintptr_t)b.dst) & 15u) == 0 &&
                     a.n <= (uint64_t)Cfg::kRound * 16 && b.n <= (uint64_t)Cfg::kRound * 16;
    if (!vec) {
        copy_span<Cfg>(a.dst, a.src, a.n);
        copy_span<Cfg>(b.dst, b.src, b.n);
        return;
    }
    const int lane = Cfg::lane();
    // byte heads up to 16-byte alignment (same offset mod 16 on both sides)
    const uint64_t ha = span_head(a.dst, a.n), hb = span_head(b.dst, b.n);
    if ((uint64_t)lane < ha) copy_byte<AB>(a.dst + lane, a.src + lane);
    if ((uint64_t)lane < hb) copy_byte<AB>(b.dst + lane, b.src + lane);
    const uint32_t nva = (uint32_t)((a.n - ha) >> 4), nvb = (uint32_t)((b.n - hb) >> 4);
    const Access acca(a.dst + ha, a.src + ha, nva << 4), accb(b.dst + hb, b.src + hb, nvb << 4);
    u32x4 va[Cfg::kVecs], vb[Cfg::kVecs];
    load_round<Cfg>(acca, lane, va);
    load_round<Cfg>(accb, lane, vb);
    store_round<Cfg>(acca, lane, va);
    store_round<Cfg>(accb, lane, vb);
    const uint64_t ta = (a.n - ha) & 15u, tb = (b.n - hb) & 15u;
    const uint64_t oa = ha + ((uint64_t)nva << 4), ob = hb + ((uint64_t)nvb << 4);
    if ((uint64_t)lane < ta) copy_byte<AB>(a.dst + oa + lane, a.src + oa + lane);
    if ((uint64_t)lane < tb) copy_byte<AB>(b.dst + ob + lane, b.src + ob + lane);
}

// Address of byte `off` of the striped address space. `E` holds the extent bases
// (`E::ext[]`); it is read in place (kernarg segment or LDS): copying it to a
// local array would put the dynamically indexed array in scratch.
template <class E>
__device__ __forceinline__ char *stripe_ptr(const E &x, uint32_t n_ext, uint32_t unit_shift, uint64_t off) {
    if (n_ext == 1) return x.ext[0] + off;
    // Stripe unit u of the address space lives on extent u % n at (u / n) * unit.
    const uint64_t unit_mask = (1ull << unit_shift) - 1;
    const uint32_t u = (uint32_t)(off >> unit_shift);
    const uint32_t e = u % n_ext;
    const uint64_t eoff = ((uint64_t)(u / n_ext) << unit_shift) | (off & unit_mask);
    return x.ext[e] + eoff;
}

// Span of tile `ti` of a transfer of [rem_off, rem_off + len) in striped
// coordinates (extent bases in `x`, see stripe_ptr).
template <class E>
__device__ __forceinline__ TileSpan tile_span_of(const E &x, uint32_t n_ext, uint32_t unit_shift, uint32_t tile_shift,
                                                 char *lin, uint64_t rem_off, uint64_t len, uint32_t put, uint64_t ti,
                                                 uint64_t first_tile) {
    const uint64_t tile = 1ull << tile_shift;
    const uint64_t r0 = rem_off, r1 = rem_off + len;
    const uint64_t lo = first_tile + (ti << tile_shift);
    const uint64_t ts = lo > r0 ? lo : r0;
    const uint64_t te = (lo + tile) < r1 ? (lo + tile) : r1;
    char *rp = stripe_ptr(x, n_ext, unit_shift, ts);
    char *lp = lin + (ts - r0);
    TileSpan s;
    s.dst = put ? rp : lp;
    s.src = put ? lp : rp;
    s.n = te - ts;
    return s;
}

__device__ __forceinline__ TileSpan tile_span(const XferArgs &a, uint64_t ti, uint64_t first_tile) {
    return tile_span_of(a, a.n_ext, a.unit_shift, a.tile_shift, a.lin, a.rem_off, a.len, a.put, ti, first_tile);
}

// ---- descriptor lists (ocm/list.h) ----
// A value every lane holds alike, moved to scalar registers. A list's descriptors are
// read through a pointer that is the kernel arguments or device memory (a generic
// pointer, whose loads the compiler takes for per-lane values): this states what they are.
__device__ __forceinline__ uint32_t uniform32(uint32_t v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ uint64_t uniform64(uint64_t v) {
    return ((uint64_t)uniform32((uint32_t)(v >> 32)) << 32) | uniform32((uint32_t)v);
}

// How a wave with tiles enters the list of launch arguments `a`. Every list kernel opens with
//     uint64_t t, t1;
//     list_wave_range(w, a.grid, a.total_tiles, &t, &t1);   (ocm/list.h; w wave-uniform)
//     if (t >= t1) return;
//     const Op *ops;
//     uint32_t i = list_wave_start(a, w, &ops);
// *ops: the descriptors, in the kernel arguments for a list of at most the inline
// capacity, else in device memory. Returns the op to start the walk from. (The early
// return stays in the kernel: folded in here, the merge after it kept one instantiation
// from reading the arguments in place, and it copied all 2 KiB of them to scratch.)
template <class Args>
__device__ __forceinline__ uint32_t list_wave_start(const Args &a, uint32_t w, const typename Args::Op **ops) {
    static_assert(list_args_fit<Args>, "kernarg segment limit");
    const bool inl = a.n_ops <= (uint32_t)Args::kInline;
    *ops = inl ? a.inline_ops : a.ops;
    return inl ? 0u : a.wave_op[w];
}

// What a wave of the row kernels hands list_enter_op (ocm/list.h) to read a descriptor's
// first_tile with: into scalar registers.
struct ListLoadUniform {
    __device__ __forceinline__ uint64_t operator()(uint64_t v) const { return uniform64(v); }
};

// ---- the wave-granular copy of the batch, strided and indexed kernels ----
constexpr int kWaveUnroll = 4;  // 64 lanes x 16 B x 4 in flight: one 4 KiB wave-tile a round

template <bool NT>
using WaveCopy = CopyCfg<64, kWaveUnroll, PointerAccess<NT>>;

// One span (StridedPiece of ocm/strided.h), inside one stripe unit, of a list with launch
// arguments `a`. HOST: every extent is pinned host memory; puts store plain there, as the
// batch kernel's do.
template <bool NT, bool HOST, class Args, class Piece>
__device__ __forceinline__ void copy_piece(const Args &a, const Piece &p, uint32_t put) {
    char *lp = a.lin + p.lin_off;
    char *rp = stripe_ptr(a, a.n_ext, a.unit_shift, p.rem_off);
    if (put) {
        if (HOST)
            copy_span<WaveCopy<false>>(rp, lp, p.n);
        else
            copy_span<WaveCopy<NT>>(rp, lp, p.n);
    } else {
        copy_span<WaveCopy<NT>>(lp, rp, p.n);
    }
}

// Drain every wave's stores into L2, join the workgroup, then ONE system-scope
// fence per workgroup writes them back and makes them visible to the host,
// DMA engines and other kernels (guide: scoped release after a barrier).
__device__ __forceinline__ void block_release_system() {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) __threadfence_system();
}

// Kernel-published completion (see XferDone): the last workgroup to count in
// re-arms the counter and releases the host flag.
__device__ __forceinline__ void xfer_publish(const XferDone &d) {
    if (!d.flag) return;  // kernel argument: uniform
    block_release_system();
    if (threadIdx.x == 0) {
        const unsigned old = __hip_atomic_fetch_add(d.cnt, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        if (old == gridDim.x - 1) {
            __hip_atomic_store(d.cnt, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(d.flag, d.val, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
}

}  // namespace

}  // namespace ocm
