// libocm: the application library behind oncillamem.h. This unit holds the C ABI and
// nothing else; the ocm_x_* hooks live in introspect.cpp, optim.cpp and probe.cpp, the
// torch allocator in torch_alloc.cpp.
//
// Parity with reference src/lib.c (struct lib_alloc, ocm_init/tini/alloc/free,
// accessors, ocm_copy, ocm_copy_onesided). MI355X design:
//   * control: one mailbox RPC to the local ocmd (seq-matched; a bounded poll
//     for the reply, then a blocking wait), multi-record replies for striped pairs;
//   * registration: remote HBM extents are imported once per slab with
//     hipIpcOpenMemHandle (lazy peer access) and cached; host-tier extents are
//     mmap'ed from the owner's memfd and hipHostRegister'ed (device-mapped);
//   * data: one-sided put/get run the gfx950 transfer kernel (ocm/xfer.h) on a
//     per-process non-blocking stream; host-tier legs use the DMA engines
//     (hipMemcpyAsync); completion = stream sync, or ocm_wait() for the async form.
// Reference defects deliberately not reproduced: inverted ocm_is_remote
// (src/lib.c:461), NULL deref before check in ocm_free (:357-359), stub
// copy_in/out (:491-499), swapped GPU->RMA offsets (:654).
#include "lists.h"
#include "ocm/affinity.h"
#include "ocm/stackdump.h"

using namespace ocm;
using namespace ocmlib;

// Connect to the daemon's mailbox, retrying while it starts (reference: 10 x 10 ms), and
// offer it the shared-memory link; s.daemon is its answer.
static int attach_daemon() {
    State &s = S();
    const int connect_ms = s.cfg.connect_timeout_ms;
    s.pid = getpid();
    s.ns = pmsg_namespace();
    s.daemon_rank = env_int("OCM_DAEMON_RANK", env_int("LOCAL_RANK", 0));
    s.daemon_mbox = daemon_mailbox_name(s.daemon_rank, s.ns);
    long deadline = now_ms() + connect_ms;
    if (s.chan.connect(s.daemon_mbox, connect_ms) != 0)
        OCM_FAIL(-1, "no ocmd mailbox @%s (is the daemon running?)", s.daemon_mbox.c_str());
    // Shared-memory fast path of the mailbox (ocm/shmlink.h), offered with CONNECT.
    // Every CONNECT offers a fresh link: the daemon attaches each offer anew, with
    // its ring counts at zero, so a retried CONNECT must not reuse a link whose
    // counts have moved on.
    Msg reply;
    for (;;) {
        if (s.cfg.shm_link && s.link.create() != 0) OCM_WARN("no shared-memory link (%s); mailbox only", strerror(errno));
        Msg c = new_msg(MSG_CONNECT);
        if (rpc(c, &reply, std::max(1000, connect_ms)) != 0) {
            s.chan.close();
            s.link.close();
            return -1;
        }
        if (s.link.ok() && !s.last_via_link) {
            // The daemon answered on the socket: it did not take the link (it found it
            // unusable, or does not take links at all). Requests stay on the socket.
            OCM_INFO("ocmd declined the shared-memory link; using the mailbox socket");
            s.link.close();
        }
        if (reply.err != EAGAIN) break;
        if (now_ms() > deadline) {
            s.chan.close();
            s.link.close();
            OCM_FAIL(-1, "daemon mesh not ready after %d ms", connect_ms);
        }
        usleep(20000);  // mesh still joining
    }
    s.daemon = reply.u.node;
    return 0;
}

// Pick the GPU this process copies on (OCM_GPU, else the daemon's GPU) and set it up:
// the library stream and event, peer access, and this thread next to the GPU.
static int open_device() {
    State &s = S();
    int ndev = 0;
    if (!s.cfg.no_gpu && hipGetDeviceCount(&ndev) != hipSuccess) {
        (void)hipGetLastError();
        ndev = 0;
    }
    int dev = env_int("OCM_GPU", s.daemon.gpu);
    if (dev < 0 && ndev > 0 && s.daemon.gpu >= 0) dev = 0;
    s.device = (ndev > 0 && dev >= 0 && dev < ndev) ? dev : -1;
    s.peers_enabled = 0;
    if (s.device < 0) return 0;
    DeviceGuard guard(s.device);
    if (hipStreamCreateWithFlags(&s.stream, hipStreamNonBlocking) != hipSuccess) {
        (void)hipGetLastError();
        OCM_FAIL(-1, "cannot create HIP stream on device %d", s.device);
    }
    if (hipEventCreateWithFlags(&s.done, hipEventDisableTiming) != hipSuccess) {
        (void)hipGetLastError();
        s.done = nullptr;
    }
    // Map every peer MI355X now: remote extents are read/written by kernels
    // on this device over xGMI (imports also request lazy peer access).
    for (int p = 0; p < ndev; p++) {
        int can = 0;
        if (p == s.device || hipDeviceCanAccessPeer(&can, s.device, p) != hipSuccess || !can) continue;
        hipError_t pe = hipDeviceEnablePeerAccess(p, 0);
        if (pe != hipSuccess && pe != hipErrorPeerAccessAlreadyEnabled)
            OCM_WARN("peer access %d -> %d: %s", s.device, p, hipGetErrorString(pe));
        else
            s.peers_enabled++;
        (void)hipGetLastError();
    }
    // This thread next to the GPU, on the L3 complex its daemon uses (ocm/affinity.h).
    char bus[64] = {0};
    if (hipDeviceGetPCIBusId(bus, sizeof(bus), s.device) == hipSuccess)
        (void)pin_near_gpu(bus, s.device, PinRole::App, s.daemon_rank);
    else
        (void)hipGetLastError();
    return 0;
}

// ================================================================ C API

extern "C" {

int ocm_init(void) {
    hang_watch_set_extra(print_hang_state);
    if (env_int("OCM_CRASH_STACK", 0) == 1) install_crash_stacks();
    HangWatch hw("ocm_init");
    State &s = S();
    std::lock_guard<std::recursive_mutex> lk(s.mu);
    if (s.inited) return 0;
    // State outlives ocm_tini: every knob comes from the environment alone, on every init.
    s.cfg = config_from_env();
    s.svc_arm_window_ns.store(s.cfg.svc_arm_window_ns);
    s.tuning = xfer_tuning_from_env();
    if (attach_daemon() != 0 || open_device() != 0) return -1;
    s.inited = true;
    if (s.device >= 0 && s.cfg.svc_max > 0 && s.cfg.svc_eager && service_prepare() != 0)
        OCM_LOG("copy service setup deferred to the first op: %s", last_error());
    OCM_LOG("attached to ocmd rank %d (gpu %d, %u nodes), copying on device %d", s.daemon_rank, s.daemon.gpu,
            s.daemon.num_nodes, s.device);
    return 0;
}

// An application that exits without ocm_tini may leave the copy service's lone
// lead resident on the library's AQL queue: tell it to leave (a store to the
// host record; nothing waits, the process is going away).
__attribute__((destructor)) static void ocm_lib_exit() {
    State &s = S();
    // the pre-arm helper thread makes no HSA call from here on (the runtime is being torn
    // down; the thread itself ends with the process)
    s.svc_armer_stop.store(true);
    s.svc_arm_cv.notify_all();
    if (s.svc && s.svc_req) {
        service_store_seq(s.svc_req, kServiceStop);
        if (s.svc_greq) service_store_seq(s.svc_greq, kServiceStop, s.svc_greq_copies);
    }
}

int ocm_tini(void) {
    HangWatch hw("ocm_tini");
    State &s = S();
    std::lock_guard<std::recursive_mutex> lk(s.mu);
    if (!s.inited) return -1;
    service_stop();  // no copy-service instance may outlive the mappings below
    std::vector<lib_alloc *> left(s.allocs.begin(), s.allocs.end());
    for (auto *a : left) ocm_free(a);
    Msg d = new_msg(MSG_DISCONNECT);
    s.chan.send(&d, kMsgBytes, 1000);
    push_release();
    DeviceGuard g(s.device);
    for (auto &kv : s.imports) {
        Mapping &m = kv.second;
        if (kv.first.tier == TIER_GPU) close_gpu_mapping(m);
        if (m.registered) (void)hipHostUnregister(m.hbase);
        if (m.hbase) munmap(m.hbase, m.bytes);
    }
    s.imports.clear();
    net_close_all();
    close_fd_chans();
    for (auto st : s.lanes) {
        (void)hipStreamSynchronize(st);
        (void)hipStreamDestroy(st);
    }
    s.lanes.clear();
    s.next_lane = 0;
    if (s.lane_flags) {
        (void)hipHostFree(s.lane_flags);
        (void)hipFree(s.lane_cnt);
        s.lane_flags = nullptr;
        s.lane_cnt = nullptr;
        s.lane_flag_seq.clear();
    }
    release_dev_cache();
    if (s.pattern_bad) (void)hipFree(s.pattern_bad);
    s.pattern_bad = nullptr;
    if (s.stream) {
        (void)hipStreamSynchronize(s.stream);
        (void)hipStreamDestroy(s.stream);
        s.stream = nullptr;
    }
    if (s.pool) (void)hipMemPoolDestroy(s.pool);
    s.pool = nullptr;
    s.pool_tried = false;
    if (s.pinned) s.pinned->release_all();
    s.chan.close();
    s.link.close();
    s.inited = false;
    trace_flush("app");
    return 0;
}

ocm_alloc_t ocm_alloc(ocm_alloc_param_t p) { return ocm_alloc_ex(p, nullptr); }

static ocm_alloc_t alloc_impl(ocm_alloc_param_t p, const struct ocm_alloc_ex_params *ex);

ocm_alloc_t ocm_alloc_ex(ocm_alloc_param_t p, const struct ocm_alloc_ex_params *ex) {
    const uint64_t traced = p ? (p->rem_alloc_bytes ? p->rem_alloc_bytes : p->local_alloc_bytes) : 0;
    return abi_call("ocm_alloc", true, "alloc", traced, [&] { return alloc_impl(p, ex); },
                    [](OpCounters &c, uint64_t ns, bool ok) {
                        c.n_alloc += ok;
                        c.ns_alloc += ok ? ns : 0;
                    });
}

// What the extents of a pair say about it (lib_alloc's flags). A network extent clears
// all_gpu and any_gpu; same_gpu needs a device; any_peer counts only HBM extents of
// this node on another GPU.
static void classify_extents(lib_alloc *a) {
    const int dev = S().device;
    bool all_hbm = true, any_hbm = false, all_here = true;
    a->all_dev_ok = true;
    a->any_net = a->any_peer = false;
    for (const Extent &e : a->ext) {
        const bool hbm = e.r.tier == TIER_GPU;
        all_hbm &= hbm;
        any_hbm |= hbm;
        all_here &= e.r.owner_gpu == dev;
        a->all_dev_ok &= e.dev_ok;
        a->any_net |= e.net;
        a->any_peer |= !e.net && hbm && e.r.owner_gpu != dev;
    }
    a->all_gpu = all_hbm && !a->any_net;
    a->any_gpu = any_hbm && !a->any_net;
    a->same_gpu = a->all_gpu && dev >= 0 && all_here;
}

// Take back an allocation the owner granted and this side could not finish: unmap what
// was imported, free it at the owner, release the local half, and keep the error.
static ocm_alloc_t undo_alloc(lib_alloc *a) {
    const std::string why = last_error();
    for (auto &e : a->ext)
        if (e.dptr || e.hptr) release_extent(e, false);
    Msg f = new_msg(MSG_REQ_FREE);
    f.u.req.alloc_id = a->alloc_id;
    Msg fr;
    rpc(f, &fr, S().cfg.rpc_timeout_ms);
    free_local_half(a);
    delete a;
    set_last_error("%s", why.c_str());
    return nullptr;
}

// The remote half of a granted pair: its extent records (they follow the reply `r`),
// their imports, and what they say about the pair.
static bool attach_extents(lib_alloc *a, const Msg &r) {
    a->remote = true;
    a->remote_bytes = r.u.region.bytes;
    a->stripe_unit = r.u.region.stripe_unit;
    const int n = r.u.region.n_extents;
    a->ext.resize(n);
    if (n < 1 || n > kMaxExtents) return false;
    for (int i = 0; i < n; i++) {
        Msg e;
        if (recv_seq(&e, r.seq, MSG_EXTENT, S().cfg.rpc_timeout_ms) != 0) return false;
        const int idx = e.u.region.extent_idx;
        if (idx >= n) return false;
        a->ext[idx].r = e.u.region;
    }
    for (int i = 0; i < n; i++)
        if (import_extent(a->ext[i]) != 0) return false;
    classify_extents(a);
    return true;
}

static ocm_alloc_t alloc_impl(ocm_alloc_param_t p, const struct ocm_alloc_ex_params *ex) {
    State &s = S();
    std::lock_guard<std::recursive_mutex> lk(s.mu);
    if (!s.inited) OCM_FAIL(nullptr, "ocm_alloc before ocm_init");
    if (!p) OCM_FAIL(nullptr, "ocm_alloc: NULL parameters");
    enum ocm_kind kind = p->kind;
    if (kind == OCM_LOCAL_RMA || kind == OCM_LOCAL_RDMA) kind = OCM_LOCAL_HOST;
    if (kind < OCM_LOCAL_HOST || kind > OCM_REMOTE_GPU) OCM_FAIL(nullptr, "ocm_alloc: invalid kind %d", (int)p->kind);
    const bool pair = is_pair(kind);
    if (kind == OCM_LOCAL_GPU && s.device < 0) OCM_FAIL(nullptr, "OCM_LOCAL_GPU requested but no GPU is available");
    const uint64_t req_bytes = pair ? p->rem_alloc_bytes : p->local_alloc_bytes;
    if (req_bytes == 0) OCM_FAIL(nullptr, "ocm_alloc: zero-byte request");

    Msg m = new_msg(MSG_REQ_ALLOC);
    m.u.req.orig_rank = s.daemon_rank;
    m.u.req.remote_rank = ex ? ex->remote_rank : -1;
    m.u.req.bytes = req_bytes;
    m.u.req.kind = (uint32_t)kind;
    m.u.req.flags = ex ? ex->flags : 0;
    if (s.device < 0) m.u.req.flags |= OCM_ALLOC_HOST_TIER;  // a CPU-only app cannot map HBM
    m.u.req.stripe_width = ex ? ex->stripe_width : 0;
    m.u.req.stripe_unit = ex ? ex->stripe_unit : 0;
    m.u.req.tier = (m.u.req.flags & OCM_ALLOC_HOST_TIER) ? TIER_HOST : TIER_GPU;
    m.u.req.app_pid = s.pid;
    if (m.u.req.stripe_unit && log2_exact(m.u.req.stripe_unit) < 12)
        OCM_FAIL(nullptr, "stripe unit must be a power of two >= 4 KiB");
    Msg r;
    if (rpc(m, &r, s.cfg.rpc_timeout_ms) != 0) return nullptr;
    if (r.type != MSG_RELEASE_APP) OCM_FAIL(nullptr, "unexpected reply %s", msg_type_str(r.type));
    if (r.err) OCM_FAIL(nullptr, "ocm_alloc of %llu bytes failed: %s", (unsigned long long)req_bytes, strerror(r.err));

    auto *a = new lib_alloc();
    a->kind = kind;
    a->alloc_id = r.u.region.alloc_id;
    if (pair && !attach_extents(a, r)) return undo_alloc(a);
    const Loc want = kind == OCM_REMOTE_GPU || kind == OCM_LOCAL_GPU ? LOC_DEVICE : pair ? LOC_PINNED : LOC_HOST;
    if (alloc_local_half(a, p->local_alloc_bytes, want) != 0) return undo_alloc(a);
    if ((m.u.req.flags & OCM_ALLOC_ZERO) && a->local) {
        if (a->loc == LOC_DEVICE) {
            DeviceGuard g(s.device);
            (void)hipMemsetAsync(a->local, 0, a->local_bytes, s.stream);
            sync_stream();
        } else {
            std::memset(a->local, 0, a->local_bytes);
        }
    }
    s.allocs.insert(a);
    return a;
}

static int free_impl(ocm_alloc_t a);

int ocm_free(ocm_alloc_t a) {
    return abi_call("ocm_free", true, "free", 0, [&] { return free_impl(a); },
                    [](OpCounters &c, uint64_t ns, bool ok) {
                        c.n_free += ok;
                        c.ns_free += ns;  // failed frees too
                    });
}

static int free_impl(ocm_alloc_t a) {
    State &s = S();
    std::lock_guard<std::recursive_mutex> lk(s.mu);
    if (!a || !s.allocs.count(a)) OCM_FAIL(-1, "ocm_free: unknown allocation");
    if (a->plans) OCM_FAIL(-1, "ocm_free: allocation is used by %d plan stage(s); destroy the plans first", a->plans);
    wait_alloc(a);
    if (a->batch_dev || a->batch_host) {
        DeviceGuard g(s.device);
        if (a->batch_up) (void)hipEventSynchronize(a->batch_up);
        if (a->batch_dev) (void)hipFreeAsync(a->batch_dev, s.stream);
        if (a->batch_host) (void)hipHostFree(a->batch_host);
        if (a->batch_up) (void)hipEventDestroy(a->batch_up);
        a->batch_dev = a->batch_host = nullptr;
        a->batch_up = nullptr;
    }
    indexed_release(a);
    if (a->ev) {
        DeviceGuard g(s.device);
        (void)hipEventDestroy(a->ev);
        a->ev = nullptr;
    }
    if (a->dep_ev) {
        DeviceGuard g(s.device);
        (void)hipEventDestroy(a->dep_ev);
        a->dep_ev = nullptr;
    }
    // Unmap dedicated remote slabs before the owner frees them.
    for (auto &e : a->ext) release_extent(e, false);
    free_local_half(a);
    Msg f = new_msg(MSG_REQ_FREE);
    f.u.req.alloc_id = a->alloc_id;
    f.u.req.n_extents = (int32_t)a->ext.size();
    Msg r;
    int rc = rpc(f, &r, s.cfg.rpc_timeout_ms);
    s.allocs.erase(a);
    delete a;
    if (rc != 0) return -1;
    if (r.err) OCM_FAIL(-1, "ocm_free: %s", strerror(r.err));
    return 0;
}

int ocm_localbuf(ocm_alloc_t a, void **buf, size_t *len) {
    if (!a || !buf || !len) return -1;
    *buf = a->local;
    *len = a->local_bytes;
    return 0;
}

bool ocm_is_remote(ocm_alloc_t a) { return a && a->remote; }

enum ocm_kind ocm_alloc_kind(ocm_alloc_t a) { return a ? a->kind : (enum ocm_kind)0; }

int ocm_remote_sz(ocm_alloc_t a, size_t *len) {
    if (!a || !len || !a->remote) return -1;  // no remote buffer for local kinds
    *len = a->remote_bytes;
    return 0;
}

void *ocm_remotebuf(ocm_alloc_t a) {
    if (!a || a->ext.size() != 1 || a->ext[0].net) return nullptr;
    return S().device >= 0 ? a->ext[0].dptr : a->ext[0].hptr;
}

static int onesided_impl(ocm_alloc_t a, ocm_param_t p, bool async);

static int ocm_copy_onesided_impl(ocm_alloc_t a, ocm_param_t p, bool async) {
    const bool put = p && p->op_flag != 0;
    return abi_call(put ? "ocm_put" : "ocm_get", true, put ? "put" : "get", p ? p->bytes : 0,
                    [&] { return onesided_impl(a, p, async); },
                    [&](OpCounters &c, uint64_t ns, bool ok) {
                        if (!ok || !p) return;
                        (put ? c.n_put : c.n_get)++;
                        (put ? c.bytes_put : c.bytes_get) += p->bytes;
                        (put ? c.ns_put : c.ns_get) += ns;
                    });
}

static int onesided_impl(ocm_alloc_t a, ocm_param_t p, bool async) {
    State &s = S();
    hipEvent_t wait_ev = nullptr;
    XferDone wait_done_flag;
    {
        std::lock_guard<std::recursive_mutex> lk(s.mu);
        if (!a || !p) OCM_FAIL(-1, "ocm_copy_onesided: NULL argument");
        if (!s.allocs.count(a)) OCM_FAIL(-1, "ocm_copy_onesided: unknown allocation");
        if (!a->remote) OCM_FAIL(-1, "one-sided copy needs a remote pair (kind %d)", (int)a->kind);
        // Bounds (reference src/rdma.c:55-59, src/lib.c:679): the local side is
        // src_offset, the remote side dest_offset, for both directions (overflow-safe).
        if (p->src_offset > a->local_bytes || p->bytes > a->local_bytes - p->src_offset)
            OCM_FAIL(-1, "one-sided copy: local range [%llu,+%llu) exceeds %zu bytes",
                     (unsigned long long)p->src_offset, (unsigned long long)p->bytes, a->local_bytes);
        if (p->dest_offset > a->remote_bytes || p->bytes > a->remote_bytes - p->dest_offset)
            OCM_FAIL(-1, "one-sided copy: remote range [%llu,+%llu) exceeds %zu bytes",
                     (unsigned long long)p->dest_offset, (unsigned long long)p->bytes, a->remote_bytes);
        char *lin = static_cast<char *>(a->local) + p->src_offset;
        const bool put = p->op_flag != 0;
        // Large blocking ops: launch on the allocation's lane under the lock, wait
        // outside it, so other threads' ops proceed meanwhile. Small ones keep the
        // copy service (no launch) and the network tier its own blocking path.
        const bool service = a->loc == LOC_DEVICE && a->all_dev_ok && p->bytes <= s.cfg.svc_limit(a);
        if (async || s.device < 0 || service || a->any_net)
            return xfer(a, put, lin, a->loc, p->dest_offset, p->bytes, async);
        if (xfer(a, put, lin, a->loc, p->dest_offset, p->bytes, true, &wait_done_flag) != 0) return -1;
        if (!a->async_pending || !a->ev) return 0;  // it completed inside xfer
        wait_ev = a->ev;
    }
    DeviceGuard g(s.device);
    // The kernel publishes its own completion (~6 us before the runtime's event).
    if (wait_done_flag.flag) return wait_done(wait_done_flag, wait_ev);
    return wait_event(wait_ev);
}

int ocm_copy_onesided(ocm_alloc_t a, ocm_param_t p) { return ocm_copy_onesided_impl(a, p, false); }
int ocm_copy_onesided_async(ocm_alloc_t a, ocm_param_t p) { return ocm_copy_onesided_impl(a, p, true); }

int ocm_wait(ocm_alloc_t a) {
    State &s = S();
    std::lock_guard<std::recursive_mutex> lk(s.mu);
    if (a) {
        if (!s.allocs.count(a)) OCM_FAIL(-1, "ocm_wait: unknown allocation");
        const int rc = wait_alloc(a);
        return rc != 0 ? rc : indexed_take_skips(a);
    }
    int rc = 0;  // NULL: every allocation
    for (auto *x : s.allocs) rc |= wait_alloc(x);
    rc |= sync_stream();
    for (auto *x : s.allocs) rc |= indexed_take_skips(x);
    return rc;
}

static bool range_ok(uint64_t off, uint64_t n, uint64_t cap) { return off <= cap && n <= cap - off; }

static int copy_impl(ocm_alloc_t dst, ocm_alloc_t src, ocm_param_t p);

int ocm_copy(ocm_alloc_t dst, ocm_alloc_t src, ocm_param_t p) {
    return abi_call("ocm_copy", true, "copy", p ? p->bytes : 0, [&] { return copy_impl(dst, src, p); },
                    [&](OpCounters &c, uint64_t, bool ok) {
                        if (!ok || !p) return;
                        c.n_copy++;
                        c.bytes_copy += p->bytes;
                    });
}

static int copy_impl(ocm_alloc_t dst, ocm_alloc_t src, ocm_param_t p) {
    State &s = S();
    std::lock_guard<std::recursive_mutex> lk(s.mu);
    if (!dst || !src || !p) OCM_FAIL(-1, "ocm_copy: NULL argument");
    if (wait_alloc(dst) != 0 || wait_alloc(src) != 0) return -1;  // their queued async ops come first
    // A read (op_flag == 0) is the write with the roles swapped (reference src/lib.c:511-515).
    struct ocm_params q = *p;
    if (!q.op_flag) {
        std::swap(dst, src);
        q.op_flag = 1;
    }
    const uint64_t n = q.bytes;
    if (!src->remote && !dst->remote) {
        if (!range_ok(q.src_offset, n, src->local_bytes) || !range_ok(q.dest_offset, n, dst->local_bytes))
            OCM_FAIL(-1, "ocm_copy: range out of bounds");
        return copy_local(static_cast<char *>(dst->local) + q.dest_offset, dst->loc,
                          static_cast<char *>(src->local) + q.src_offset, src->loc, n);
    }
    if (!src->remote && dst->remote) {
        // Stage into dst's local half, then one-sided write local[src_offset_2] -> remote[dest_offset_2].
        if (!range_ok(q.src_offset, n, src->local_bytes) || !range_ok(q.dest_offset, n, dst->local_bytes) ||
            !range_ok(q.src_offset_2, n, dst->local_bytes) || !range_ok(q.dest_offset_2, n, dst->remote_bytes))
            OCM_FAIL(-1, "ocm_copy: range out of bounds");
        if (copy_local(static_cast<char *>(dst->local) + q.dest_offset, dst->loc,
                       static_cast<char *>(src->local) + q.src_offset, src->loc, n) != 0)
            return -1;
        return xfer(dst, true, static_cast<char *>(dst->local) + q.src_offset_2, dst->loc, q.dest_offset_2, n, false);
    }
    if (src->remote && !dst->remote) {
        // One-sided read remote[dest_offset_2] -> src local[src_offset_2], then unstage.
        if (!range_ok(q.src_offset_2, n, src->local_bytes) || !range_ok(q.dest_offset_2, n, src->remote_bytes) ||
            !range_ok(q.src_offset, n, src->local_bytes) || !range_ok(q.dest_offset, n, dst->local_bytes))
            OCM_FAIL(-1, "ocm_copy: range out of bounds");
        if (xfer(src, false, static_cast<char *>(src->local) + q.src_offset_2, src->loc, q.dest_offset_2, n, false) != 0)
            return -1;
        return copy_local(static_cast<char *>(dst->local) + q.dest_offset, dst->loc,
                          static_cast<char *>(src->local) + q.src_offset, src->loc, n);
    }
    // remote -> remote (not supported by the reference): direct, no staging.
    if (!range_ok(q.src_offset, n, src->remote_bytes) || !range_ok(q.dest_offset, n, dst->remote_bytes))
        OCM_FAIL(-1, "ocm_copy: range out of bounds");
    if (src->any_net || dst->any_net) {
        // A side on another node: bounce through host memory, 64 MiB at a time.
        const uint64_t chunk = std::min<uint64_t>(n, 64ull << 20);
        std::vector<char> tmp(chunk);
        for (uint64_t done = 0; done < n;) {
            const uint64_t k = std::min(chunk, n - done);
            if (xfer(src, false, tmp.data(), LOC_HOST, q.src_offset + done, k, false) != 0) return -1;
            if (xfer(dst, true, tmp.data(), LOC_HOST, q.dest_offset + done, k, false) != 0) return -1;
            done += k;
        }
        return 0;
    }
    std::vector<Seg> ss;
    segments(src, q.src_offset, n, ss);
    const bool one_launch = s.device >= 0 && src->all_dev_ok && dst->all_dev_ok &&
                            (dst->ext.size() == 1 || log2_exact(dst->stripe_unit) >= 4);
    if (one_launch) {
        // Every source segment is a device address: one batched launch writes them all.
        std::vector<XferBatchOp> v(ss.size());
        for (size_t i = 0; i < ss.size(); i++) {
            const Seg &g = ss[i];
            v[i].lin_off = reinterpret_cast<uintptr_t>(src->ext[g.ext].dptr + g.ext_off);
            v[i].rem_off = q.dest_offset + g.lin_off;
            v[i].len = g.len;
            v[i].put = 1;
        }
        return batch_put_abs(dst, v);
    }
    for (auto &g : ss) {
        const Extent &e = src->ext[g.ext];
        char *sp = (s.device >= 0 ? e.dptr : e.hptr) + g.ext_off;
        const Loc sl = (s.device >= 0 && (e.r.tier == TIER_GPU || e.dptr != e.hptr)) ? LOC_DEVICE : LOC_HOST;
        if (xfer(dst, true, sp, sl, q.dest_offset + g.lin_off, g.len, false) != 0) return -1;
    }
    return 0;
}

int ocm_copy_in(ocm_alloc_t dst, void *src) {
    State &s = S();
    std::lock_guard<std::recursive_mutex> lk(s.mu);
    if (!dst || !src) OCM_FAIL(-1, "ocm_copy_in: NULL argument");
    if (wait_alloc(dst) != 0) return -1;
    const Loc sl = pointer_loc(src);
    if (dst->remote) return xfer(dst, true, static_cast<char *>(src), sl, 0, dst->remote_bytes, false);
    return copy_local(dst->local, dst->loc, src, sl, dst->local_bytes);
}

int ocm_copy_out(void *dst, ocm_alloc_t src) {
    State &s = S();
    std::lock_guard<std::recursive_mutex> lk(s.mu);
    if (!dst || !src) OCM_FAIL(-1, "ocm_copy_out: NULL argument");
    if (wait_alloc(src) != 0) return -1;
    const Loc dl = pointer_loc(dst);
    if (src->remote) return xfer(src, false, static_cast<char *>(dst), dl, 0, src->remote_bytes, false);
    return copy_local(dst, dl, src->local, src->loc, src->local_bytes);
}

int ocm_remote_info(ocm_alloc_t a, struct ocm_remote_info *info) {
    if (!a || !info) return -1;
    std::memset(info, 0, sizeof(*info));
    info->alloc_id = a->alloc_id;
    info->remote_bytes = a->remote_bytes;
    info->stripe_unit = a->stripe_unit;
    info->n_extents = (uint32_t)a->ext.size();
    for (size_t i = 0; i < a->ext.size() && i < OCM_MAX_EXTENTS; i++) {
        info->tier[i] = a->ext[i].r.tier;
        info->owner_rank[i] = a->ext[i].r.owner_rank;
        info->owner_gpu[i] = a->ext[i].r.owner_gpu;
        info->extent_bytes[i] = a->ext[i].r.bytes;
        if (a->ext[i].net) info->net_mask |= 1u << i;
    }
    return a->remote ? 0 : -1;
}

int ocm_stats(int rank, struct ocm_daemon_stats *out) {
    State &s = S();
    std::lock_guard<std::recursive_mutex> lk(s.mu);
    if (!s.inited || !out) return -1;
    Msg m = new_msg(MSG_STATS);
    m.u.req.remote_rank = rank;
    Msg r;
    if (rpc(m, &r, s.cfg.rpc_timeout_ms) != 0) return -1;
    if (r.err) OCM_FAIL(-1, "stats from rank %d: %s", rank, strerror(r.err));
    const NodeConfig &c = r.u.node;
    std::memset(out, 0, sizeof(*out));
    out->rank = c.rank;
    out->gpu = c.gpu;
    out->num_nodes = (int32_t)c.num_nodes;
    out->num_apps = (int32_t)c.num_apps;
    out->gpu_capacity = c.gpu_capacity;
    out->gpu_used = c.gpu_used;
    out->host_capacity = c.host_capacity;
    out->host_used = c.host_used;
    out->n_alloc = c.n_alloc;
    out->n_free = c.n_free;
    out->n_reclaimed = c.n_reclaimed;
    out->n_spilled = c.n_spilled;
    out->n_slabs = c.n_slabs;
    out->ctrl_ticks = c.ticks;
    out->n_leases = c.n_leases;
    out->lease_allocs = c.lease_allocs;
    out->xgmi_peers = c.xgmi_peers;
    out->min_hops = c.min_hops;
    out->max_hops = c.max_hops;
    out->ctrl_transport = c.ctrl;
    return 0;
}

int ocm_rank(void) { return S().inited ? S().daemon_rank : -1; }
int ocm_num_nodes(void) { return S().inited ? (int)S().daemon.num_nodes : -1; }
int ocm_device(void) { return S().inited ? S().device : -1; }
const char *ocm_last_error(void) { return last_error(); }

}  // extern "C"
