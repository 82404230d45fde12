// The persistent copy service: a resident gang of workgroups that polls request
// records in host memory and copies their tiles (protocol: ocm/xfer.h). This unit
// alone is also compiled device-only into the code object embedded in libocm
// (AQL dispatch, ocm/aql.h), so it holds the service's two kernels and nothing else
// that runs on the device.
#include <hip/hip_runtime.h>

#include <cstring>

#include "ocm/xfer.h"
#include "xfer_copy.h"

namespace ocm {

namespace {

__host__ __device__ __forceinline__ unsigned long long service_mix(unsigned long long h, unsigned long long w) {
    h ^= w + 0x9E3779B97F4A7C15ull + (h << 6) + (h >> 2);
    h *= 0xBF58476D1CE4E5B9ull;
    return h ^ (h >> 31);
}

// Hash of a request record's seq and words 0..kServiceReqGang (args, gang word).
__host__ __device__ __forceinline__ unsigned long long service_sum(unsigned long long seq, const unsigned long long *w) {
    unsigned long long h = service_mix(0, seq);
    for (int i = 0; i <= kServiceReqGang; i++) h = service_mix(h, w[i]);
    return h;
}

__device__ __forceinline__ unsigned long long readlane64(unsigned long long w, int lane) {
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)w, lane);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(w >> 32), lane);
    return ((unsigned long long)hi << 32) | lo;
}

// Tiles first, first + stride, ... of the request in `sh` (args at sh + 2).
template <int ST>
__device__ __forceinline__ void service_copy(const unsigned long long *sh, uint64_t first, uint64_t stride) {
    const XferArgs &a = *reinterpret_cast<const XferArgs *>(sh + 2);  // read in place (no scratch copy)
    const uint64_t ntiles = xfer_tile_count(a.rem_off, a.len, a.tile_shift);
    const uint64_t base = xfer_first_tile(a.rem_off, a.tile_shift);
    // tiles two at a time: both tiles' loads in flight at once (copy_span2)
    uint64_t ti = first;
    for (; ti + stride < ntiles; ti += 2 * stride)
        copy_span2<BlockCopy<ST>>(tile_span(a, ti, base), tile_span(a, ti + stride, base));
    if (ti < ntiles) {
        TileSpan sp = tile_span(a, ti, base);
        copy_span<BlockCopy<ST>>(sp.dst, sp.src, sp.n);
    }
}

__device__ __forceinline__ void service_stamp(ServiceBox *box, unsigned proto, unsigned id, int k) {
    if ((proto & kServiceProtoTrace) && threadIdx.x == 0 && id < (unsigned)kServiceTraceWgs)
        __hip_atomic_store(&box->trace[id][k], __builtin_amdgcn_s_memrealtime(), __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
}

// Copy member `id`'s share of the request in `sh` and make it visible
// system-wide; the member that completes the request publishes `done`.
__device__ __forceinline__ void service_serve(const unsigned long long *sh, unsigned long long s, ServiceSlot *slot,
                                              ServiceBox *box, unsigned proto, unsigned id) {
    const unsigned long long gang = sh[1];
    const unsigned long long active = gang & 0xFFFFull, target = (gang >> 16) & kServiceGangTargetMask;
    if (id >= active) return;  // block-uniform: members past `active` sit this one out
    // STRICT requests (extents in another GPU's HBM) take the fenced hand-off even
    // under the WT protocol: sc1 accesses keep this GPU's caches coherent with host
    // memory and its own HBM, but a resident instance may hold L2 lines of peer
    // memory from an earlier request, and nothing else invalidates them.
    const bool strict = (gang & kServiceGangStrict) != 0;
    const bool wt = (proto & kServiceProtoWT) && (!strict || (proto & kServiceProtoStrictWT));
    service_stamp(box, proto, id, 1);
    if (wt) {
        if (strict) {  // STRICTWT: drop stale L2 lines of peer memory before the sc1 (L2-served) loads
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        service_copy<ST_WT>(sh, id, active);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // EVERY storing wave drains its sc1 stores
        __syncthreads();
    } else {
        if (proto & kServiceProtoWT) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");  // the poll skipped it
        service_copy<ST_PLAIN>(sh, id, active);
        block_release_system();
    }
    service_stamp(box, proto, id, 2);
    if (threadIdx.x == 0 && service_wg_done(proto, active)) {
        // WGDONE: this member's own completion word; the host waits for all of them.
        if (wt)
            __hip_atomic_store(&slot->wg_done[id], s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        else
            __hip_atomic_store(&slot->wg_done[id], s, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    } else if (threadIdx.x == 0) {
        bool last = active == 1;
        if (!last) {
            const unsigned long long old =
                wt ? __hip_atomic_fetch_add(&box->cnt, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                   : __hip_atomic_fetch_add(&box->cnt, 1ull, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
            last = old == target - 1;
        }
        if (last) {
            if (wt)
                __hip_atomic_store(&slot->done, s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);  // after the drain
            else
                __hip_atomic_store(&slot->done, s, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
    service_stamp(box, proto, id, 3);
}

// Whether every member named by the last request workgroup 0 served (seq
// `last`, gang word `gang`) has finished it. Wave 0 of workgroup 0, all lanes.
__device__ __forceinline__ bool service_last_complete(ServiceSlot *slot, ServiceBox *box, unsigned proto,
                                                      unsigned long long last, unsigned long long gang) {
    const unsigned long long active = gang & 0xFFFFull, target = (gang >> 16) & kServiceGangTargetMask;
    if (active <= 1) return true;  // workgroup 0 served it alone
    const unsigned lane = threadIdx.x & 63u;
    bool ok = true;
    if (service_wg_done(proto, active)) {
        for (unsigned long long i = lane; i < active; i += 64)
            ok &= __hip_atomic_load(&slot->wg_done[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) == last;
    } else {
        ok = __hip_atomic_load(&box->cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= target;
    }
    return __builtin_amdgcn_ballot_w64(!ok) == 0;
}

// The poll state of one service workgroup (wave 0 polls; every field is
// wave-uniform). A struct with force-inlined members, not lambdas: lambdas that
// capture the kernel's locals by reference left them in scratch memory (336
// bytes a lane), and every scratch load is a drain of the loads in flight.
struct ServicePoll {
    // fixed for the instance
    const unsigned long long *req, *greq;
    ServiceSlot *slot;
    ServiceBox *box;
    unsigned long long first_seq, idle_ticks, checkin_base, degraded_idle_ticks, lone_ticks, started;
    unsigned proto, epoch, grid;
    int tid;
    bool lead, direct;
    // state
    unsigned long long last = 0;       // requests carry strictly increasing seqs
    unsigned long long last_gang = 0;  // gang word of request `last` (workgroup 0's idle-exit test)
    unsigned long long roster = 0;     // members published so far (workgroup 0)
    unsigned long long idle_start = 0;
    unsigned long long s = 0;          // the poll's outcome: a seq to serve or kServiceStop
    int base = 0;                      // first lane of the record being served
    bool served = false;
    bool lone = false;        // the lead alone: the members have left (lone_ticks)
    bool superseded = false;  // the lead saw a newer instance: it leaves without touching the slot
    // The last gang request was already seen complete by an earlier idle check. The idle
    // window runs from the lead's own share, and a PCIe-bound gang op of 8-16 MiB ends up
    // to ~50 us later on its slowest member: leaving at the first check that finds it
    // complete raced the host's next post (12-15 % of those ops relaunched,
    // profiles/bench_n1_r04_final_b.json). A gang op gets one more window from then.
    bool gang_drained = false;

    // One load instruction per poll: lanes 0..15 read the whole record (args, gang
    // word, sum, seq); a seq whose hash checks out is whole.
    __device__ __forceinline__ unsigned long long load() const {
        const bool count = lead && !lone && roster < grid;  // wave-uniform
        unsigned long long v = 0;
        if (tid < 16)
            v = (lead || direct) ? __hip_atomic_load(req + tid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM)
                                 : __hip_atomic_load(req + tid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        else if (direct && lead && !lone && tid < 32)
            v = __hip_atomic_load(greq + (tid - 16), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        else if (!lead && tid == 16)
            v = __hip_atomic_load(&box->stop, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // the lead left
        else if (count && tid == 32)
            v = __hip_atomic_load(&box->checkin, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        else if (lone && tid == 48)
            v = __hip_atomic_load(&slot->epoch_now, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        return v;
    }

    // The lead's pipelined poll (PIPE) reads 16 bytes a lane into an LDS slot (LDS
    // DMA, lane L at slot + 16 L): lanes 0..7 the small-op record, 8..15 the gang
    // record (direct lead), 16 the check-in counter, 17 the epoch word; the others
    // re-read the small-op record (the same lines: no extra request).
    __device__ __forceinline__ const void *pipe_addr() const {
        const int l = tid & 63;
        const char *a = reinterpret_cast<const char *>(req) + 16 * (l & 7);
        if (l >= 8 && l < 16 && direct && !lone) a = reinterpret_cast<const char *>(greq) + 16 * (l - 8);
        if (l == 16) a = reinterpret_cast<const char *>(&box->checkin);
        if (l == 17) a = reinterpret_cast<const char *>(&slot->epoch_now);
        return a;
    }

    // One poll result `v`: 0 poll again, 1 leave the poll loop (s, base set), 2 the
    // seq landed before the rest of the record (read again at once), 3 the lead just
    // went lone (it polls one at a time from now on).
    __device__ __forceinline__ int check(unsigned long long v) {
        if (lead && !lone && roster < grid) {
            const unsigned long long r = readlane64(v, 32) - checkin_base;  // check-ins, the lead's included
            if (r > roster) {  // members counted here are running: requests may name them
                if (tid == 0)
                    __hip_atomic_store(&slot->roster, service_tag(epoch, r), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                roster = r;
            }
        }
        base = 0;
        s = readlane64(v, 15);
        if (!lead && readlane64(v, 16) == first_seq) {  // the lead of THIS instance left
            s = kServiceStop;
            return 1;
        }
        if (lone && (readlane64(v, 48) & kServiceGangEpochMask) != epoch) {  // replaced by a full instance
            s = kServiceStop;
            superseded = true;
            return 1;
        }
        if (direct && lead && !lone) {
            const unsigned long long s2 = readlane64(v, 31);  // the gang record's seq
            if (s2 == kServiceStop) {  // the host parked it
                s = kServiceStop;
                return 1;
            }
            if (s2 > last && s2 != 0) {
                s = s2;  // the host posts one request at a time: at most one record is new
                base = 16;
            }
        }
        if (s == kServiceStop) return 1;
        if (s > last) {
            unsigned long long h = service_mix(0, s);
#pragma unroll
            for (int i = 0; i <= kServiceReqGang; i++) h = service_mix(h, readlane64(v, base + i));
            if (h != readlane64(v, base + 14)) return 2;  // seq landed before the rest: read it again
            // Whole. A member of an earlier instance (started late) leaves a newer one's
            // request alone; a lead that sees one has been replaced and leaves. A lone
            // lead takes no gang request (its members are gone: the host starts a full
            // instance for it).
            const unsigned long long g = readlane64(v, base + kServiceReqGang);
            const bool mine = ((g >> kServiceGangEpochShift) & kServiceGangEpochMask) == epoch;
            if (lead && !mine) {
                s = kServiceStop;
                superseded = true;
                return 1;
            }
            if (mine && !(lone && (g & 0xFFFFull) > 1)) return 1;
        }
        // While part of the grid has not started (the roster is short) it waits
        // longer (degraded_idle_ticks): the kernel cannot complete before those
        // workgroups get CUs and leave anyway, so leaving early would release a
        // device-wide sync no sooner, and every relaunch would need another
        // stream while they wait (the pool is small).
        // (the window by assignments: a select between fields would take their addresses
        // and keep the whole struct in scratch)
        unsigned long long window = degraded_idle_ticks;
        if (roster >= grid) window = idle_ticks;
        if (lone) window = lone_ticks;
        if (lead && __builtin_amdgcn_s_memrealtime() - idle_start > window &&
            (served || __builtin_amdgcn_s_memrealtime() - started > 2000000ull)) {
            // Leave only once every member the last request named is done
            // with it: a member that saw the STOP first would never serve it.
            const bool complete = service_last_complete(slot, box, proto, last, last_gang);
            idle_start = __builtin_amdgcn_s_memrealtime();
            if (complete && (gang_drained || (last_gang & 0xFFFFull) <= 1 || !served)) {
                // Only an instance whose whole grid has started goes lone: one with
                // workgroups still waiting for a CU leaves whole, as its lane drains
                // only once they have started (and left at once), and the full
                // instance that would replace a lone lead needs a drained lane.
                if (lone || lone_ticks == 0 || roster < grid) {
                    s = kServiceStop;
                    return 1;
                }
                // The members leave; the lead stays alone and says so (the host
                // then sizes no gang on this instance).
                lone = true;
                if (tid == 0) {
                    __hip_atomic_store(&box->stop, first_seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    __hip_atomic_store(&slot->lone, service_tag(epoch, last + 1), __ATOMIC_RELEASE,
                                       __HIP_MEMORY_SCOPE_SYSTEM);
                }
                return 3;
            } else if (complete) {
                gang_drained = true;  // complete only now: the host gets a whole window to post
            }
        }
        return 0;
    }

    // Whether poll result `v` needs check(): a seq past `last` (or STOP) in either
    // record, a member checked in, or the idle window over. Cheap and branch-free, so
    // the pipelined loop below stays small; check() does the rest, outside it.
    __device__ __forceinline__ bool attention(unsigned long long seq, unsigned long long gseq, unsigned long long ck,
                                              unsigned long long window) const {
        bool a = seq > last;                         // a new small-op request, or STOP (~0)
        if (direct) a |= gseq > last;                // the gang record (direct lead)
        if (roster < grid) a |= ck - checkin_base > roster;
        const unsigned long long now = __builtin_amdgcn_s_memrealtime();
        a |= now - idle_start > window && (served || now - started > 2000000ull);
        return a;
    }

    // Poll until a request to serve or a reason to leave (s). Returns the record as
    // read by this lane (lane i: word i of the two records, lane 32 the check-in
    // counter, lane 48 the epoch word). PIPE (lead only, not while lone):
    // kServicePollDepth polls of the host record in flight at once, issued ~0.2 us
    // apart, instead of one poll that waits out its PCIe round trip (~1.2 us) before
    // the next. The host's post is then seen within ~0.2 us of landing plus the
    // return trip, whatever its phase against the poll loop; with one poll at a time
    // a post that just missed a read waited for the whole next round trip, and a
    // back-to-back ping-pong locked into that phase for hundreds of ops (the small-op
    // "slow mode": +1.3 us of crossings).
    //
    // The polls are LDS DMA (global_load_lds_dwordx4) into slots of `lds`, issued and
    // read in inline asm: no poll in flight ever targets a register, so the compiler's
    // register allocation and its own wait counting cannot meet one (compiled C++ polls
    // into registers were drained at every loop back edge, and copied between
    // registers before they had landed). Slot k is waited for with vmcnt(7) (the 7
    // polls issued after it stay in flight), read, and re-issued unless it found
    // something, so the found request's copy is held behind no extra poll (loads
    // return in order).
    __device__ __forceinline__ void pipe_issue(const void *addr, unsigned lds_slot) const {
        unsigned m0_saved;
        asm volatile(
            "s_mov_b32 %0, m0\n\t"
            "s_mov_b32 m0, %2\n\t"
            "global_load_lds_dwordx4 %1, off sc0 sc1\n\t"
            "s_mov_b32 m0, %0"
            : "=&s"(m0_saved)
            : "v"(addr), "s"(lds_slot)
            : "memory");
    }
    // The spacing between poll issues: kServicePollSleep, or the count in proto bits
    // 8..15 (OCM_SERVICE_POLL_SLEEP) in units of s_sleep(1). Wave-uniform (proto is).
    __device__ __forceinline__ void pipe_sleep() const {
        const unsigned n = (proto >> kServicePollSleepShift) & 0xFFu;
        if (n == 0) {
            __builtin_amdgcn_s_sleep(kServicePollSleep);
        } else {
            for (unsigned i = 1; i < n; i++) __builtin_amdgcn_s_sleep(1);
        }
    }
    __device__ __forceinline__ unsigned long long lds_word(unsigned lds_addr) const {
        unsigned long long v;
        asm volatile("ds_read_b64 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(v) : "v"(lds_addr) : "memory");
        return v;
    }
    __device__ __forceinline__ unsigned long long poll(unsigned lds) {
        unsigned long long w = 0;
        int rc = 0;
        while (lead && (proto & kServiceProtoPipe) && !lone) {
            const unsigned long long window = roster >= grid ? idle_ticks : degraded_idle_ticks;
            const void *addr = pipe_addr();
            static_assert(kServicePollDepth == 8, "eight poll slots: vmcnt(7)");
            // JITTER (proto bits 24..27, a mask; OCM_SERVICE_POLL_JITTER): start the polls a
            // pseudo-random 0..mask units of s_sleep(1) late, so their schedule does not keep
            // one phase against the host's posts from op to op
            const unsigned jitter = (proto >> kServicePollJitterShift) & 0xFu;
            if (jitter) {
                const unsigned n = (unsigned)(__builtin_amdgcn_s_memrealtime() * 0x9E3779B1ull >> 40) & jitter;
                for (unsigned i = 0; i < n; i++) __builtin_amdgcn_s_sleep(1);
            }
#pragma unroll
            for (int k = 0; k < kServicePollDepth; k++) {
                pipe_issue(addr, lds + k * kServicePollSlotBytes);
                pipe_sleep();
            }
            // One exit, after the unrolled body (a break from inside it makes the
            // structurized loop do the exit's work on every pass). found: 1 + the slot.
            int found = 0;
            do {
#pragma unroll
                for (int k = 0; k < kServicePollDepth; k++) {
                    if (!found) {
                        const unsigned sl = lds + k * kServicePollSlotBytes;
                        asm volatile("s_waitcnt vmcnt(7)" ::: "memory");
                        const unsigned long long seq = lds_word(sl + 120);      // small-op record word 15
                        const unsigned long long gseq = lds_word(sl + 128 + 120);  // gang record word 15
                        const unsigned long long ck = lds_word(sl + 256);      // lane 16: the check-in counter
                        if (attention(seq, gseq, ck, window)) {
                            found = k + 1;
                        } else {
                            pipe_issue(addr, sl);
                            pipe_sleep();
                        }
                    }
                }
            } while (!found);
            // The slot as the one-load poll's lanes hold it: word i of the two records
            // in lane i, the check-in counter in lane 32, the epoch word in lane 48.
            const int l = tid & 63;
            const unsigned off = l < 32 ? 8u * l : l == 32 ? 256u : l == 48 ? 272u : 0u;
            w = lds_word(lds + (found - 1) * kServicePollSlotBytes + off);
            rc = check(w);
            if (rc == 1) return w;
        }
        for (;;) {
            w = load();
            rc = check(w);
            if (rc == 1) return w;
            if (rc == 2) continue;
            if (lone)
                __builtin_amdgcn_s_sleep(24);  // ~0.6 us: one PCIe read of the record per poll
            else if (lead || direct)
                __builtin_amdgcn_s_sleep(8);  // ~0.2 us between PCIe polls
            else
                __builtin_amdgcn_s_sleep(1);
        }
    }
};

// Workgroup 0 polls the host request record across PCIe; for a gang request it
// relays the record, as read (the host's hash included), to the gang through
// device memory with one 16-lane write-through store, before anything else.
// The gang polls that device copy: 32 workgroups polling the host record
// directly cost every op 3-4 us (profiles/svc_v3_direct_r02.json), and a relay
// that re-hashed and fenced first cost the gang ~2 us (profiles/svc_trace_r02.json).
// GANGREC (grq != nullptr): gang requests sit in their own host record, which
// members 0..direct_wgs-1 poll themselves; workgroup 0 reads both records in
// one load (lanes 0..15 the small-op record, 16..31 the gang record) and
// relays only gangs wider than direct_wgs to the others. 16 direct pollers
// cost small ops nothing measurable; 32 cost them ~1 us
// (profiles/svc_direct_gang_ab_r02.json).
// Members are numbered in check-in order; member 0 (the first workgroup to
// start) is "workgroup 0" of the protocol above and publishes how many have
// checked in (the roster, see ocm/xfer.h): lane 32 of its poll reads the
// check-in counter until the whole grid is in.
}  // namespace

// The copy service. extern "C": libocm also dispatches it by name from the device
// code object embedded in the library, on an AQL queue of its own (ocm/aql.h).
extern "C" __global__ __launch_bounds__(kThreads) void ocm_service_kernel(ServiceKernelArgs ka) {
    if (ka.first_seq == 0) return;  // a cancelled pre-armed dispatch (ocm/aql.h aql_disarm)
    const ServiceReq *rq = ka.req, *grq = ka.gang_req;
    ServiceSlot *slot = ka.slot;
    ServiceBox *box = ka.box;
    const unsigned long long first_seq = ka.first_seq;
    const unsigned proto = ka.proto, direct_wgs = ka.direct_wgs, epoch = ka.epoch;
    __shared__ __attribute__((aligned(16))) unsigned long long sh[16];
    __shared__ unsigned sh_id;
    const int tid = threadIdx.x;
    // Member ids in check-in order. The first workgroup to start is workgroup 0 of
    // the protocol (the lead), whichever block it is: the dispatcher spreads blocks
    // over the XCDs, and block 0's XCD may have no room while others do (measured
    // under tests/test_gpu_service.py's CU hog: block 0 waited for the hog to end).
    // The counter only grows across instances (the box is not cleared between
    // launches): tickets of this instance start at checkin_base.
    if (tid == 0)
        sh_id = (unsigned)(__hip_atomic_fetch_add(&box->checkin, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) -
                           ka.checkin_base);
    __syncthreads();
    const unsigned id = __builtin_amdgcn_readfirstlane(sh_id);  // this workgroup's member id
    const bool lead = id == 0;
    const bool direct = grq != nullptr && id < direct_wgs;  // polls the host gang record itself
    const unsigned long long relay_above = grq != nullptr ? direct_wgs : 1;  // gangs wider than this are relayed
    // COPIES: direct member i polls copy i of the gang record (the lead, member 0, copy 0)
    const ServiceReq *gmine = grq + ((proto & kServiceProtoCopies) && direct ? id : 0u);
    ServicePoll P;
    P.req = reinterpret_cast<const unsigned long long *>(
        lead ? static_cast<const void *>(rq) : direct ? static_cast<const void *>(gmine) : static_cast<const void *>(box->rec));
    P.greq = reinterpret_cast<const unsigned long long *>(grq);
    P.slot = slot;
    P.box = box;
    P.first_seq = first_seq;
    P.idle_ticks = ka.idle_ticks;
    P.checkin_base = ka.checkin_base;
    P.degraded_idle_ticks = ka.degraded_idle_ticks;
    P.lone_ticks = ka.lone_ticks;
    P.proto = proto;
    P.epoch = epoch;
    P.grid = ka.blocks;
    P.tid = tid;
    P.lead = lead;
    P.direct = direct;
    P.last = first_seq - 1;
    P.idle_start = __builtin_amdgcn_s_memrealtime();
    // The host launches an instance only for a request it is about to post, and it
    // may first wait for the roster: no idle exit before the first request (with a
    // 1 us idle window the lead left before every post, and host and kernel
    // relaunched each other until the op timed out), unless none comes in 20 ms.
    P.started = P.idle_start;
    // This instance's own sum (the host folds each instance's into its total when it
    // starts the next): no read across PCIe before the first poll.
    unsigned long long ticks_sum = 0;
    if (lead && tid == 0) {
        // where the lead runs (diagnostic; a posted write, nothing waits for it): 1 + its XCD
        // (HW_REG_XCC_ID[3:0]) in bits 0..7, its HW_REG_HW_ID (CU, shader array, engine) above
        const unsigned long long xcc = __builtin_amdgcn_s_getreg((3 << 11) | (0 << 6) | 20) & 0xFu;
        const unsigned long long hwid = (unsigned)__builtin_amdgcn_s_getreg((31 << 11) | (0 << 6) | 4);
        __hip_atomic_store(&slot->lead_xcd, service_tag(epoch, (1ull + xcc) | (hwid << 8)), __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(&slot->start_ticks, service_tag(epoch, P.started), __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_SYSTEM);
    }
    // wave 0 (a wave-uniform test: `tid < 64` reads as divergent to the compiler, and
    // the poll state it updates would then live in vector registers under exec masks)
    const bool wave0 = __builtin_amdgcn_readfirstlane(tid) < 64;
    // PIPE poll slots (ServicePoll::poll), LDS addresses; one __shared__ array with sh
    __shared__ __attribute__((aligned(16))) char poll_lds[kServicePollDepth * kServicePollSlotBytes];
    const unsigned poll_slots = (unsigned)(uintptr_t)(__attribute__((address_space(3))) char *)poll_lds;
    // The first request inline (ServiceKernelArgs::first_rec): the lead serves it without
    // polling. Wave-uniform (scalar kernel arguments, the lead flag from readfirstlane).
    bool inline_first = lead && ka.first_rec[15] == first_seq;
    for (;;) {
        if (wave0) {
            unsigned long long w = 0;
            if (inline_first) {
                // lane i: word i of the record, as a poll would have read it (an unrolled select:
                // a lane-indexed read of the argument array would copy it to scratch)
#pragma unroll
                for (int i = 0; i < 16; i++)
                    if (tid == i) w = ka.first_rec[i];
                P.s = first_seq;
                P.base = 0;
                inline_first = false;
            } else {
                w = P.poll(poll_slots);
            }
            const int base = P.base;  // first lane of the record being served (wave-uniform)
            const unsigned long long s = P.s;
            if (lead && s != kServiceStop && (readlane64(w, base + kServiceReqGang) & 0xFFFFull) > relay_above &&
                tid >= base && tid < base + 16)
                __hip_atomic_store(&box->rec[tid - base], w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // relay, sc1
            // Data loads are sc1 (ST_WT protocol): they bypass this CU's L1 and are
            // not served from stale L2 copies of host or peer memory, so no acquire
            // fence is needed; the plain protocol keeps the system-scope acquire.
            if (!(proto & kServiceProtoWT)) {
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            }
            const int r = tid - base;  // this lane's word of the served record
            if (r >= 0 && r <= kServiceReqGang) sh[r == kServiceReqGang ? 1 : 2 + r] = w;  // args -> sh[2..], gang -> sh[1]
            if (tid == 0) sh[0] = s;
        }
        __syncthreads();
        const unsigned long long s = sh[0];
        if (s == kServiceStop) break;
        const unsigned long long t_seen = __builtin_amdgcn_s_memrealtime();
        service_stamp(box, proto, id, 0);
        service_serve(sh, s, slot, box, proto, id);
        if (lead && !P.served && tid == 0)  // diagnostic, after `done`: when the instance's first request was seen
            __hip_atomic_store(&slot->first_seen_ticks, service_tag(epoch, t_seen), __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_SYSTEM);
        P.last = s;
        P.last_gang = sh[1];
        P.served = true;
        P.gang_drained = false;
        P.idle_start = __builtin_amdgcn_s_memrealtime();  // every lane: the idle test must stay wave-uniform
        if (lead) {
            // Diagnostic, after `done` so it never delays it: a running sum in a
            // register, published with a plain store (no PCIe atomic round trip).
            ticks_sum += P.idle_start - t_seen;
            if (tid == 0) __hip_atomic_store(&slot->gpu_ticks, ticks_sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            if ((proto & kServiceProtoTrace) && tid == 0) {  // per-op stamps (device memory, after `done`)
                unsigned long long *o = box->optrace[s & (kServiceOpTrace - 1)];
                __hip_atomic_store(&o[1], t_seen, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(&o[2], P.idle_start, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(&o[0], s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
        __syncthreads();  // sh is rewritten by the next poll
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // no poll still landing in LDS when the wave ends
    if (lead && tid == 0) {
        // Every member leaves when it sees this instance's first seq here (an
        // earlier instance's value never matches, so the box needs no clearing).
        __hip_atomic_store(&box->stop, first_seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (!P.superseded)
            __hip_atomic_store(&slot->exited, service_tag(epoch, P.last + 1), __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// Zero a lane's gang box on the lane's own AQL queue (one workgroup), ahead of an
// instance dispatched with the barrier bit: no host memset and stream sync.
extern "C" __global__ __launch_bounds__(kThreads) void ocm_service_box_clear(ServiceBox *box) {
    unsigned long long *w = reinterpret_cast<unsigned long long *>(box);
    for (unsigned i = threadIdx.x; i < sizeof(ServiceBox) / 8; i += kThreads) w[i] = 0ull;
}

uint32_t service_gang_size(const XferArgs &a, unsigned blocks, unsigned solo_tiles) {
    const uint64_t ntiles = xfer_tile_count(a.rem_off, a.len, a.tile_shift);
    if (blocks <= 1 || ntiles <= solo_tiles) return 1;
    return (uint32_t)(ntiles < blocks ? ntiles : blocks);
}

void service_record(unsigned long long out[16], const XferArgs &a, unsigned long long gang, unsigned long long seq) {
    unsigned long long w[kServiceReqGang + 1] = {};
    std::memcpy(w, &a, sizeof(a));
    w[kServiceReqGang] = gang;
    for (int i = 0; i <= kServiceReqGang; i++) out[i] = w[i];
    out[14] = service_sum(seq, w);
    out[15] = seq;
}

void service_post(ServiceReq *req, const XferArgs &a, unsigned long long gang, unsigned long long seq,
                  unsigned copies) {
    unsigned long long w[kServiceReqGang + 1] = {};
    std::memcpy(w, &a, sizeof(a));
    w[kServiceReqGang] = gang;
    const unsigned long long h = service_sum(seq, w);
    // Line 0 (words 0..7) of every copy first and fenced, then line 1 (words 8..13,
    // sum, seq): a poll that saw seq ahead of the rest fails the hash and reads again.
    // The last copy first: copy 0 is the lead's.
    for (unsigned c = copies; c-- > 0;)
        for (int i = 0; i < 8; i++) __atomic_store_n(&req[c].args[i], w[i], __ATOMIC_RELAXED);
    __builtin_ia32_sfence();
    for (unsigned c = copies; c-- > 0;) {
        for (int i = 8; i <= kServiceReqGang; i++) __atomic_store_n(&req[c].args[i], w[i], __ATOMIC_RELAXED);
        __atomic_store_n(&req[c].sum, h, __ATOMIC_RELAXED);
        __atomic_store_n(&req[c].seq, seq, __ATOMIC_RELEASE);
    }
    __builtin_ia32_sfence();
}

void service_store_seq(ServiceReq *req, unsigned long long seq, unsigned copies) {
    for (unsigned c = 0; c < copies; c++) __atomic_store_n(&req[c].seq, seq, __ATOMIC_RELEASE);
    __builtin_ia32_sfence();
}

hipError_t service_launch(const ServiceKernelArgs &args, unsigned blocks, bool reset_box, hipStream_t stream) {
    if (!args.req || !args.slot || !args.box || blocks == 0 || blocks != args.blocks || args.first_seq == 0 ||
        (args.gang_req && args.direct_wgs == 0) || args.epoch > kServiceGangEpochMask)
        return hipErrorInvalidValue;
    if (reset_box) {
        hipError_t e = hipMemsetAsync(args.box, 0, sizeof(ServiceBox), stream);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(ocm_service_kernel, dim3(blocks), dim3(kThreads), 0, stream, args);
    return hipGetLastError();
}

}  // namespace ocm
