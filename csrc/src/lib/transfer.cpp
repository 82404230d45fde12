// libocm copy engine: striped segments, per-allocation lanes and events,
// one-sided transfers (one function per engine: network tier, CPU, the resident
// copy service, push gets, gfx950 kernel launches, DMA) and process-local copies.
// Reference parity: ocm_copy src/lib.c:501-665 and ocm_copy_onesided
// src/lib.c:669-723, whose RDMA/RMA legs (ib_read/ib_write over post_send,
// src/rdma.c:47-92,241-302; extoll_read/extoll_write over extoll_rma2_transfer,
// src/extoll.c:40-167,286-310, 8 MiB x 2 outstanding) become
// gfx950 kernel launches or the resident copy service (service.cpp) here.
#include "internal.h"

namespace ocmlib {

// ---------------------------------------------------------------- copy engine


// Split [rem_off, rem_off+len) of a striped buffer into contiguous pieces.
void segments(const lib_alloc *a, uint64_t rem_off, uint64_t len, std::vector<Seg> &out) {
    out.clear();
    const int n = (int)a->ext.size();
    if (n == 1 || a->stripe_unit == 0) {
        out.push_back({0, rem_off, 0, len});
        return;
    }
    const uint64_t unit = a->stripe_unit;
    uint64_t pos = rem_off, done = 0;
    while (done < len) {
        const uint64_t u = pos / unit, within = pos % unit;
        const uint64_t take = std::min(unit - within, len - done);
        out.push_back({(int)(u % n), (u / n) * unit + within, done, take});
        pos += take;
        done += take;
    }
}


int wait_event(hipEvent_t ev) {
    State &s = S();
    hipError_t e = hipSuccess;
    if (s.cfg.sync_mode == 1) {
        while ((e = hipEventQuery(ev)) == hipErrorNotReady) {
        }
    } else {
        e = hipEventSynchronize(ev);
    }
    if (e != hipSuccess) OCM_FAIL(-1, "event wait: %s", hipGetErrorString(e));
    return 0;
}

// ocm_stream_wait dependency: order it before work on `st` (nullptr: the
// copy service, which has no stream, so wait on the host).
int honor_dep(lib_alloc *a, hipStream_t st, bool host_wait) {
    if (!a->dep_pending) return 0;
    a->dep_pending = false;
    hipError_t e = host_wait ? hipEventSynchronize(a->dep_ev) : hipStreamWaitEvent(st, a->dep_ev, 0);
    if (e != hipSuccess) OCM_FAIL(-1, "stream dependency: %s", hipGetErrorString(e));
    return 0;
}

// Completion of `a`'s queued async ops (its lane up to the recorded event).
int wait_alloc(lib_alloc *a) {
    State &s = S();
    if (!a || !a->async_pending) return 0;
    a->async_pending = false;
    if (!a->ev) return 0;
    DeviceGuard g(s.device);
    return wait_event(a->ev);
}

// The lane of `a`'s async ops, with a->ev created; the library stream, with
// a->ev == nullptr, when no lane or no event could be created.
hipStream_t lane_stream(lib_alloc *a) {
    State &s = S();
    if (a->lane < 0) {
        if (s.lanes.empty()) {
            DeviceGuard g(s.device);
            for (int i = 0; i < std::max(1, s.cfg.n_lanes); i++) {
                hipStream_t st = nullptr;
                if (hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess) {
                    (void)hipGetLastError();
                    break;
                }
                s.lanes.push_back(st);
            }
        }
        if (s.lanes.empty()) return s.stream;
        if (!s.lane_flags && s.cfg.launch_flags) {
            DeviceGuard g(s.device);
            const size_t nl = s.lanes.size();
            if (hipHostMalloc(reinterpret_cast<void **>(&s.lane_flags), nl * 128,
                              hipHostMallocCoherent | hipHostMallocMapped) != hipSuccess ||
                hipMalloc(reinterpret_cast<void **>(&s.lane_cnt), nl * 128) != hipSuccess ||
                hipMemset(s.lane_cnt, 0, nl * 128) != hipSuccess) {
                (void)hipGetLastError();
                s.cfg.launch_flags = false;  // events only
            } else {
                std::memset(s.lane_flags, 0, nl * 128);
                s.lane_flag_seq.assign(nl, 0);
            }
        }
        a->lane = s.next_lane++ % (int)s.lanes.size();
    }
    if (!a->ev) {
        DeviceGuard g(s.device);
        if (hipEventCreateWithFlags(&a->ev, hipEventDisableTiming) != hipSuccess) {
            (void)hipGetLastError();
            a->ev = nullptr;
            return s.stream;
        }
    }
    return s.lanes[a->lane];
}

int sync_stream() {
    State &s = S();
    if (!s.stream) return 0;
    DeviceGuard g(s.device);
    hipError_t e = hipSuccess;
    if (s.cfg.sync_mode == 0 || !s.done) {
        e = hipStreamSynchronize(s.stream);
    } else {
        e = hipEventRecord(s.done, s.stream);
        if (e == hipSuccess && s.cfg.sync_mode == 1) {
            // Spin: lowest completion latency for small one-sided ops.
            while ((e = hipEventQuery(s.done)) == hipErrorNotReady) {
            }
        } else if (e == hipSuccess) {
            e = hipEventSynchronize(s.done);
        }
    }
    if (e != hipSuccess) OCM_FAIL(-1, "stream sync: %s", hipGetErrorString(e));
    return 0;
}

int async_done(lib_alloc *a, hipStream_t st) {
    State &s = S();
    if (st != s.stream && a->ev) {
        const hipError_t err = hipEventRecord(a->ev, st);
        if (err != hipSuccess) OCM_FAIL(-1, "event record failed: %s", hipGetErrorString(err));
    } else if (a->ev == nullptr && sync_stream() != 0) {
        return -1;  // no lane available: complete it now
    }
    a->async_pending = a->ev != nullptr;
    return 0;
}

int wait_done(const XferDone &d, hipEvent_t ev) {
    for (unsigned spins = 1;; spins++) {
        if ((long long)(__atomic_load_n(d.flag, __ATOMIC_ACQUIRE) - d.val) >= 0) return 0;
        if ((spins & 4095) == 0) {
            // Backstop: the runtime saw the kernel end (the flag is then set, or
            // the kernel had nothing to publish); errors surface here too.
            const hipError_t e = hipEventQuery(ev);
            if (e == hipSuccess) return 0;
            if (e != hipErrorNotReady) OCM_FAIL(-1, "event wait: %s", hipGetErrorString(e));
        }
    }
}

// ---- one-sided transfers: the pieces the engines share ----

// The tuning of one direction's kernel ops: the per-direction tuning if set, else the process tuning.
static const XferTuning &dir_tuning(bool put) {
    State &s = S();
    const XferTuning &dt = s.dir_tuning[put ? 1 : 0];
    return dt.variant != XFER_AUTO ? dt : s.tuning;
}

// Launch arguments of one transfer on `a`: the op, and the pair's side.
static int pair_args(const lib_alloc *a, bool put, char *lin, uint64_t rem_off, uint64_t len, XferArgs *x) {
    std::memset(x, 0, sizeof(*x));
    x->lin = lin;
    x->rem_off = rem_off;
    x->len = len;
    x->put = put ? 1 : 0;
    if (pair_side(a, 0, x) < 0)
        OCM_FAIL(-1, "stripe unit %llu is not a power of two", (unsigned long long)a->stripe_unit);
    return 0;
}

// A piece between a host-resident local half and the host tier, or any piece of a
// process without a GPU: this thread copies it (the CPU is the fastest engine).
static bool cpu_copies(Loc lloc, const Extent &e) {
    return S().device < 0 || (lloc != LOC_DEVICE && e.r.tier != TIER_GPU);
}

// Copy `n` pieces of pair `a` between `lin` and their extents: memcpy where
// cpu_copies(), hipMemcpyAsync on `st` otherwise. Stops at the first error.
static hipError_t copy_segs(const lib_alloc *a, const Seg *segs, size_t n, bool put, char *lin, Loc lloc,
                            hipStream_t st) {
    for (const Seg *g = segs; g != segs + n; g++) {
        const Extent &e = a->ext[g->ext];
        const bool cpu = cpu_copies(lloc, e);
        char *r = (cpu ? e.hptr : e.dptr) + g->ext_off, *l = lin + g->lin_off;
        if (cpu) {
            std::memcpy(put ? r : l, put ? l : r, g->len);
            continue;
        }
        const hipError_t err = hipMemcpyAsync(put ? r : l, put ? l : r, g->len, hipMemcpyDefault, st);
        if (err != hipSuccess) return err;
    }
    return hipSuccess;
}

// ---- one-sided transfers: the engines ----
// Each moves [rem_off, rem_off + len) of `a`'s remote half to or from the linear
// buffer `lin` (location `lloc`). xfer() below picks one.

// Another node: stream every piece through its owner's data server (blocking).
static int xfer_net(lib_alloc *a, bool put, char *lin, Loc lloc, uint64_t rem_off, uint64_t len) {
    State &s = S();
    std::vector<Seg> segs;
    segments(a, rem_off, len, segs);
    if (wait_alloc(a) != 0) return -1;
    if (honor_dep(a, nullptr, true) != 0) return -1;
    DeviceGuard dg(s.device);
    for (auto &g : segs) {
        const Extent &e = a->ext[g.ext];
        if (e.net) {
            if (net_piece(e, put, lin + g.lin_off, lloc, g.ext_off, g.len) != 0) return -1;
            continue;
        }
        // mixed placement: this piece is on this node
        if (copy_segs(a, &g, 1, put, lin, lloc, s.stream) != hipSuccess) OCM_FAIL(-1, "transfer launch failed");
        if (!cpu_copies(lloc, e) && sync_stream() != 0) return -1;
    }
    return 0;
}

// A process without a GPU: every extent is host tier, and this thread copies.
static int xfer_cpu(lib_alloc *a, bool put, char *lin, Loc lloc, uint64_t rem_off, uint64_t len) {
    std::vector<Seg> segs;
    segments(a, rem_off, len, segs);
    (void)copy_segs(a, segs.data(), segs.size(), put, lin, lloc, nullptr);
    return 0;
}

// The resident copy service (no launch, no stream sync). 0: done; -1: the service
// failed and nothing holds the request any more (never launched, or drained after
// STOP), so a launch may redo the op; -2: failed for good (an instance may still
// hold the request, and a launch now would race it).
static int xfer_service(lib_alloc *a, bool put, char *lin, uint64_t rem_off, uint64_t len) {
    State &s = S();
    XferArgs x;
    if (pair_args(a, put, lin, rem_off, len, &x) != 0) return -2;
    if (wait_alloc(a) != 0) return -2;  // keep program order with queued async ops
    if (honor_dep(a, nullptr, true) != 0) return -2;
    // Gets from the host tier are bound by PCIe read round trips: two tiles
    // already go faster on two workgroups (64 KiB: 7.7 vs 8.4 us); puts and
    // HBM owners keep small requests on workgroup 0 (profiles/svc_v4_r02.json).
    const unsigned solo = (!put && !a->any_gpu) ? std::min(s.cfg.svc_solo_tiles, s.cfg.svc_solo_tiles_host_get)
                                                : s.cfg.svc_solo_tiles;
    return service_xfer(x, solo, a->any_gpu, a->any_peer || s.cfg.svc_force_strict);
}

// Push-based get (XFER_PUSH): kernels on the owners' GPUs store into the local half.
static int xfer_push(lib_alloc *a, char *lin, uint64_t rem_off, uint64_t len, hipStream_t st, bool async) {
    before_launch();
    if (push_get(a, lin, rem_off, len, st, async) != 0) return -1;
    return async ? async_done(a, st) : 0;
}

// One launch of the repo's own kernels on `st`.
static int xfer_kernel(lib_alloc *a, bool put, char *lin, uint64_t rem_off, uint64_t len, hipStream_t st, bool async,
                       XferDone *done) {
    State &s = S();
    // No resident poller during a large copy over PCIe (its doorbell reads share
    // the link) or when asked (A/B); without a queue of its own the service
    // would also hold this launch until its idle exit.
    if ((s.cfg.svc_park_kernel || !a->any_gpu) && len > s.cfg.svc_limit(a)) service_park();
    before_launch();
    XferArgs x;
    if (pair_args(a, put, lin, rem_off, len, &x) != 0) return -1;
    XferTuning t = dir_tuning(put);
    if (t.variant == XFER_AUTO) {
        // Measured (profiles/ksweep_r01.json): LDS-DMA staging wins HBM->HBM
        // copies up to ~256 MiB on the same GPU; everything else (peer HBM
        // over xGMI, host-mapped memory, huge copies) uses the register path.
        bool same_gpu = true;  // the local half is on this GPU: only such ops are launched
        for (auto &e : a->ext) same_gpu &= e.r.tier == TIER_GPU && e.r.owner_gpu == s.device;
        t.variant = !a->any_gpu ? XFER_PCIE : (same_gpu && len <= (256ull << 20)) ? XFER_LDS : XFER_REG;
    }
    XferDone dn;
    if (done && async && len <= s.cfg.launch_flag_max && s.cfg.launch_flags && s.lane_flags && st != s.stream &&
        a->lane >= 0 && a->ev) {
        dn.flag = s.lane_flags + (size_t)a->lane * 16;
        dn.cnt = s.lane_cnt + (size_t)a->lane * 32;
        dn.val = ++s.lane_flag_seq[(size_t)a->lane];
    }
    const hipError_t err = xfer_launch(x, t, st, dn.flag ? &dn : nullptr);
    if (err != hipSuccess) OCM_FAIL(-1, "transfer launch failed: %s", hipGetErrorString(err));
    if (done) *done = dn;
    return async ? async_done(a, st) : sync_stream();
}

// The runtime's copy engines, piece by piece on `st` (and this thread for host <-> host tier).
static int xfer_dma(lib_alloc *a, bool put, char *lin, Loc lloc, uint64_t rem_off, uint64_t len, hipStream_t st,
                    bool async) {
    service_park();  // no resident poller beside the DMA engines: its doorbell reads share PCIe with them
    std::vector<Seg> segs;
    segments(a, rem_off, len, segs);
    // Pieces between a host-resident local half and the host tier are copied
    // by this thread right away: first let the work they must follow finish
    // (an ocm_stream_wait dependency and earlier async ops, both queued on st).
    bool cpu_piece = false;
    for (auto &g : segs) cpu_piece |= cpu_copies(lloc, a->ext[g.ext]);
    hipError_t err = hipSuccess;
    if (cpu_piece && (err = hipStreamSynchronize(st)) != hipSuccess)
        OCM_FAIL(-1, "ordering a host copy after queued work: %s", hipGetErrorString(err));
    err = copy_segs(a, segs.data(), segs.size(), put, lin, lloc, st);
    if (err != hipSuccess) OCM_FAIL(-1, "transfer launch failed: %s", hipGetErrorString(err));
    return async ? async_done(a, st) : sync_stream();
}

// One-sided transfer between the linear buffer `lin` (location `lloc`) and the
// remote half of `a` at striped offset `rem_off`.
int xfer(lib_alloc *a, bool put, char *lin, Loc lloc, uint64_t rem_off, uint64_t len, bool async, XferDone *done) {
    State &s = S();
    if (done) *done = XferDone{};
    if (len == 0) return 0;
    if (a->any_net) return xfer_net(a, put, lin, lloc, rem_off, len);
    if (s.device < 0) return xfer_cpu(a, put, lin, lloc, rem_off, len);
    DeviceGuard guard(s.device);
    const bool lin_dev = lloc == LOC_DEVICE;
    const bool dma_pick = dir_tuning(put).variant == XFER_DMA;
    // Small blocking ops go to the resident copy service.
    if (lin_dev && a->all_dev_ok && !async && len <= s.cfg.svc_limit(a) && !dma_pick) {
        const int rc = xfer_service(a, put, lin, rem_off, len);
        if (rc == 0) return 0;
        if (rc == -2) return -1;
        OCM_WARN("copy service failed (%s); falling back to launches", last_error());
        s.cfg.svc_max = 0;
    }
    // Async ops queue on the allocation's lane; blocking ops on the library stream
    // after the allocation's queued async work.
    if (!async && wait_alloc(a) != 0) return -1;
    hipStream_t st = async ? lane_stream(a) : s.stream;
    if (honor_dep(a, st, false) != 0) return -1;
    // Every extent kind goes through the repo's own kernels: HBM extents the
    // register / LDS-DMA kernels, host-tier extents the PCIe streaming kernel
    // (57.0-57.4 GB/s, at or above the runtime's copy at 56.8-57.1:
    // profiles/pcie_stream_r03.json). OCM_HOST_ENGINE=sdma keeps the runtime's
    // copy engines for host-tier pairs as a measured baseline.
    const bool use_kernel =
        lin_dev && !dma_pick && (a->any_gpu || s.cfg.host_engine_kernel || len <= s.cfg.host_kernel_max);
    if (!use_kernel) return xfer_dma(a, put, lin, lloc, rem_off, len, st, async);
    if (!put && a->all_gpu && dir_tuning(false).variant == XFER_PUSH) return xfer_push(a, lin, rem_off, len, st, async);
    return xfer_kernel(a, put, lin, rem_off, len, st, async, done);
}

// ---- push-based get (XFER_PUSH) ----
// RDMA READ vs WRITE (reference src/rdma.c:240-263): over xGMI a remote write is
// usually cheaper than a remote read, so a get can be turned into pushes. For
// every owner GPU d of the pair's extents, this process launches a kernel on d
// (a stream of its own there) that reads d's extents from d's HBM and stores
// them into the local half over xGMI. The owner's CPU and daemon take no part.
// Needs: the slab mapped on d (extent_view: a second IPC open by d's context),
// peer access d -> this GPU and, for a pool-allocated local half, pool access
// for d (local_pool() grants it to every peer at creation).

void push_release() {
    State &s = S();
    for (auto &kv : s.push) {
        DeviceGuard g(kv.first);
        if (kv.second.stream) (void)hipStreamSynchronize(kv.second.stream);
    }
}

static PushDev *push_dev(int d) {
    State &s = S();
    PushDev &p = s.push[d];
    if (p.ready) return &p;
    DeviceGuard g(d);
    if (d != s.device) {
        int can = 0;
        if (hipDeviceCanAccessPeer(&can, d, s.device) != hipSuccess || !can)
            OCM_FAIL(nullptr, "push get: GPU %d cannot reach GPU %d", d, s.device);
        const hipError_t pe = hipDeviceEnablePeerAccess(s.device, 0);
        if (pe != hipSuccess && pe != hipErrorPeerAccessAlreadyEnabled)
            OCM_FAIL(nullptr, "push get: peer access %d -> %d: %s", d, s.device, hipGetErrorString(pe));
        (void)hipGetLastError();
    }
    if (!p.stream && hipStreamCreateWithFlags(&p.stream, hipStreamNonBlocking) != hipSuccess)
        OCM_FAIL(nullptr, "push get: no stream on GPU %d", d);
    if (!p.done && hipEventCreateWithFlags(&p.done, hipEventDisableTiming) != hipSuccess)
        OCM_FAIL(nullptr, "push get: no event on GPU %d", d);
    p.ready = true;
    return &p;
}

int push_get(lib_alloc *a, char *lin, uint64_t rem_off, uint64_t len, hipStream_t st, bool async) {
    State &s = S();
    if (!a->all_gpu || a->any_net) OCM_FAIL(-1, "push get needs every extent in a GPU's HBM");
    std::map<int, uint32_t> owners;  // device -> extent mask
    for (size_t i = 0; i < a->ext.size(); i++) {
        const int d = a->ext[i].r.owner_gpu;
        if (d < 0) OCM_FAIL(-1, "push get: extent %zu has no owner GPU", i);
        owners[d] |= 1u << i;
    }
    DeviceGuard g(s.device);
    if (!s.push_order && hipEventCreateWithFlags(&s.push_order, hipEventDisableTiming) != hipSuccess)
        OCM_FAIL(-1, "push get: no event");
    if (hipEventRecord(s.push_order, st) != hipSuccess) OCM_FAIL(-1, "push get: ordering event");
    std::vector<PushDev *> used;
    for (auto &kv : owners) {
        const int d = kv.first;
        PushDev *p = push_dev(d);
        if (!p) return -1;
        XferArgs x;  // lin, the local half: peer-accessible from d (peer access + pool access)
        if (pair_args(a, false, lin, rem_off, len, &x) != 0) return -1;
        for (size_t i = 0; i < a->ext.size(); i++) {  // d's own extents only, at their addresses on d
            x.ext[i] = nullptr;
            if (!((kv.second >> i) & 1u)) continue;
            x.ext[i] = extent_view(a->ext[i], d);
            if (!x.ext[i]) return -1;
        }
        DeviceGuard gd(d);
        hipError_t e = hipStreamWaitEvent(p->stream, s.push_order, 0);  // after the work queued before this op
        if (e == hipSuccess) e = xfer_push_launch(x, kv.second, s.dir_tuning[0].max_blocks, p->stream);
        if (e == hipSuccess) e = hipEventRecord(p->done, p->stream);
        if (e != hipSuccess) OCM_FAIL(-1, "push get on GPU %d: %s", d, hipGetErrorString(e));
        used.push_back(p);
        s.push_launches++;
    }
    for (PushDev *p : used) {
        const hipError_t e = async ? hipStreamWaitEvent(st, p->done, 0) : hipEventSynchronize(p->done);
        if (e != hipSuccess) OCM_FAIL(-1, "push get completion: %s", hipGetErrorString(e));
    }
    return 0;
}

// Copy between two process-local buffers.
int copy_local(void *dst, Loc dl, const void *src, Loc sl, size_t n) {
    State &s = S();
    if (n == 0) return 0;
    if (dl != LOC_DEVICE && sl != LOC_DEVICE) {
        std::memcpy(dst, src, n);
        return 0;
    }
    DeviceGuard g(s.device);
    hipError_t e;
    before_launch();
    if (dl == LOC_DEVICE && sl == LOC_DEVICE) {
        XferTuning t = s.tuning;
        if (t.variant == XFER_AUTO) t.variant = n <= (256ull << 20) ? XFER_LDS : XFER_REG;
        e = xfer_copy(dst, src, n, t, s.stream);
    } else
    {
        e = hipMemcpyAsync(dst, src, n, hipMemcpyDefault, s.stream);
    }
    if (e != hipSuccess) OCM_FAIL(-1, "local copy failed: %s", hipGetErrorString(e));
    return sync_stream();
}


}  // namespace ocmlib
