// libocm internals shared by the library's translation units (not installed).
//
// runtime.cpp  process state, mailbox RPC, IPC/memfd import cache, local halves
// transfer.cpp copy engine: segments, lanes/events, xfer and its engines, local copies
// service.cpp  the resident copy service's host side: lanes, start/park/stop, armer, service_xfer
// net.cpp      network-tier client (owners on other nodes)
// batch.cpp    batched one-sided ops, stream interop, transfer plans (hipGraph)
// quant.cpp    converting one-sided ops (ocm_copy_onesided_quant: MXFP8 records)
// quant_strided.cpp  strided converting ops (ocm_copy_onesided_quant_strided: one MXFP8 record per row)
// strided.cpp  strided one-sided ops (ocm_copy_onesided_strided: rows, one stride per side)
// indexed.cpp  indexed one-sided ops (ocm_copy_onesided_indexed: rows picked by index arrays in the local half)
// quant_indexed.cpp  indexed converting ops (ocm_copy_onesided_quant_indexed: one MX record per row picked by index arrays)
// bag.cpp      pooled embedding lookup (ocm_copy_onesided_bag: the rows of every bag summed on the way in)
// acc.cpp      one-sided accumulate (ocm_copy_onesided_accumulate: remote fp32 += scale * local)
// libocm.cpp   the C ABI (oncillamem.h)
// config.cpp   the environment's knobs, parsed once per ocm_init into State::cfg
// introspect.cpp  ocm_x_* hooks that read counters, layouts and the service's state, and the run-time setters
// optim.cpp    fused Adam over optimizer state in a remote half (ocm_x_adam*)
// probe.cpp    raw-pointer probe and benchmark hooks (ocm_x_xfer, ocm_x_batch, ocm_x_time_*, ocm_x_pattern*)
// torch_alloc.cpp  the PyTorch pluggable allocator
#pragma once
#include <fcntl.h>
#include <hip/hip_runtime_api.h>
#include <sys/mman.h>
#include <sys/syscall.h>
#include <time.h>
#include <unistd.h>

#include <algorithm>
#include <array>
#include <atomic>
#include <cerrno>
#include <condition_variable>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <optional>
#include <set>
#include <string>
#include <thread>
#include <vector>

#include "config.h"
#include "oncillamem.h"
#include "ocm/log.h"
#include "ocm/msg.h"
#include "ocm/netdata.h"
#include "ocm/pmsg.h"
#include "ocm/range_alloc.h"
#include "ocm/shmlink.h"
#include "ocm/sock.h"
#include "ocm/stackdump.h"
#include "ocm/trace.h"
#include "ocm/aql.h"
#include "ocm/quant.h"
#include "ocm/xfer.h"


namespace ocmlib {
using namespace ocm;
#pragma GCC visibility push(hidden)


enum Loc { LOC_HOST = 0, LOC_PINNED = 1, LOC_DEVICE = 2 };

// One data-server connection of the network tier, with its own pinned staging
// buffer for device-side local halves (allocated on first device use).
struct NetConn {
    int fd = -1;
    void *stage = nullptr;
};

struct Extent {
    Region r;
    char *dptr = nullptr;  // device-usable address of the extent start (nullptr: none)
    char *hptr = nullptr;  // host address (host tier only)
    bool dev_ok = false;   // a kernel on this process's GPU can access dptr
    bool net = false;      // owner on another node: streamed through its data server
    std::string ep;        // "ip:port" of that data server
    uint64_t net_token = 0;  // presented first on each connection to it
    uint64_t net_grant = 0;  // this extent's capability, named by every request
};


}  // namespace ocmlib

// lib_alloc is the public opaque handle (oncillamem.h), so it keeps default visibility
// while the ocmlib types it holds are hidden; g++ warns about that (-Wattributes), clang
// does not. Hiding lib_alloc instead would hide every C entry point taking it.
#pragma GCC diagnostic push
#pragma GCC diagnostic ignored "-Wattributes"
struct lib_alloc {
    enum ocm_kind kind;
    uint64_t alloc_id = 0;
    void *local = nullptr;
    size_t local_bytes = 0;
    ocmlib::Loc loc = ocmlib::LOC_HOST;
    bool remote = false;
    size_t remote_bytes = 0;
    uint64_t stripe_unit = 0;
    std::vector<ocmlib::Extent> ext;
    bool all_gpu = false;
    bool any_gpu = false;
    bool all_dev_ok = false;  // every extent reachable by a kernel on this GPU
    bool any_net = false;     // some extent lives on another node
    bool same_gpu = false;    // every extent in this process's own GPU's HBM (another daemon on it, via IPC)
    bool any_peer = false;    // some extent in ANOTHER GPU's HBM (xGMI): the copy service's fenced hand-off
    bool async_pending = false;
    bool pooled = false;      // local half from the stream-ordered pool
    int lane = -1;            // async ops: index into State::lanes (per-allocation ordering)
    hipEvent_t ev = nullptr;  // completion of the last async op (ocm_wait)
    void *batch_dev = nullptr;  // device copy of large batch descriptor lists
    void *batch_host = nullptr; // pinned staging for their upload
    size_t batch_cap = 0;
    hipEvent_t batch_up = nullptr;  // the last upload out of batch_host finished
    hipEvent_t dep_ev = nullptr;    // ocm_stream_wait: external work the next op depends on
    bool dep_pending = false;
    int plans = 0;                  // ocm_plan stages that reference this allocation
    // Indexed ops (indexed.cpp): rows skipped for an index outside its table. The kernel
    // counts them up in a device word that is never reset; after every launch the word is
    // copied to a pinned host word on the same stream, and `skip_seen` is how much of it
    // has been reported. `skip_host_path`: rows the host path skipped in async calls.
    unsigned long long *skip_dev = nullptr;
    unsigned long long *skip_host = nullptr;
    uint64_t skip_seen = 0;
    uint64_t skip_host_path = 0;
};
#pragma GCC diagnostic pop

struct ocm_plan {
    struct Stage {
        lib_alloc *a = nullptr;
        ocm::XferBatchArgs args;
        void *dev = nullptr;  // descriptors + wave table (large lists)
    };
    std::vector<Stage> stages;
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    uint64_t bytes = 0, n_ops = 0;
};


namespace ocmlib {

struct SlabKey {
    int owner;
    uint32_t tier;
    uint32_t slab;
    bool operator<(const SlabKey &o) const {
        return owner != o.owner ? owner < o.owner : tier != o.tier ? tier < o.tier : slab < o.slab;
    }
};

struct Mapping {
    char *dbase = nullptr;
    char *hbase = nullptr;
    uint64_t bytes = 0;
    uint8_t handle[kHandleBytes] = {};
    int refs = 0;
    bool dedicated = false;
    bool registered = false;
    // HBM slab of a daemon embedded in this process (ocm_x_set_slab_resolver): dbase is
    // that daemon's own pointer, not an IPC import, and is never closed here
    bool local = false;
    // HBM slabs: the same slab opened on OTHER devices of this process (push-based
    // gets launch on the owner's GPU and need an address valid there).
    std::map<int, char *> dev_views;
    // round 6: HBM slabs imported from the owner's DMA-BUF (hipImportExternalMemory)
    // instead of hipIpcOpenMemHandle; the views then have imports of their own
    hipExternalMemory_t ext = nullptr;
    std::map<int, hipExternalMemory_t> view_ext;
};

// Push-based gets: one stream per owner device this process launches on.
struct PushDev {
    hipStream_t stream = nullptr;
    hipEvent_t done = nullptr;
    bool ready = false;
};

// Largest blocking op the copy service takes for this pair.
inline uint64_t Config::svc_limit(const lib_alloc *a) const {
    if (svc_max == 0) return 0;
    if (!a->any_gpu) return svc_max_host;
    return a->same_gpu ? std::max(svc_max, svc_max_local) : svc_max;
}

struct State {
    std::recursive_mutex mu;
    bool inited = false;
    Config cfg;  // the environment's knobs, assigned whole by every ocm_init (config.h)
    pid_t pid = 0;
    std::string ns, daemon_mbox;
    Channel chan;
    ShmLink link;
    bool last_via_link = false;  // the last record recv_record returned came over the link  // shared-memory fast path to the daemon (OCM_SHM_LINK=0: the mailbox alone)
    NodeConfig daemon{};
    int daemon_rank = 0;
    int device = -1;
    // xGMI self-diagnosis (ocm_x_xgmi_diag): peers this device got access to at
    // init, and slabs of OTHER GPUs' HBM imported / refused by hipIpcOpenMemHandle.
    int peers_enabled = 0;
    uint64_t ipc_peer_imports = 0, ipc_peer_failures = 0;
    hipStream_t stream = nullptr;
    uint64_t seq = 0;
    std::map<SlabKey, Mapping> imports;
    std::set<lib_alloc *> allocs;
    XferTuning tuning;
    // Per-direction override ([0] get, [1] put) for one-sided kernel ops,
    // set by an autotune (variant XFER_AUTO: use `tuning`).
    XferTuning dir_tuning[2];
    OpCounters ctr;
    // persistent copy service (small blocking one-sided ops)
    ServiceSlot *svc = nullptr;
    ServiceReq *svc_req = nullptr;   // request record (&svc->req)
    ServiceReq *svc_greq = nullptr;  // GANGREC: gang requests' record, a page of its own
    unsigned svc_greq_copies = 1;    // COPIES: one gang record per direct poller on that page
    char *svc_rec_pages = nullptr;   // separately allocated record pages (GANGREC / WCREQ), freed at stop
    ServiceBox *svc_box = nullptr;   // device-memory mailbox of the gang (the current lane's)
    unsigned long long *pattern_bad = nullptr;  // device counter of ocm_x_pattern checks
    hipStream_t svc_stream = nullptr;  // the current lane's stream
    // Lanes of the service: a stream and a gang box each. An instance whose lead has
    // left may still have workgroups that never got a CU (another process holds
    // them); the next instance starts on a lane whose stream has drained, a new lane
    // (up to OCM_SERVICE_STREAMS, default 4), or waits for one. Requests carry the
    // instance's epoch (ocm/xfer.h), so such a late workgroup never takes one.
    struct SvcLane {
        bool aql = false;                   // an AQL queue of the library's own (else `stream`)
        AqlLane q;
        hipStream_t stream = nullptr;
        ServiceBox *box = nullptr;
        bool dirty = true;                  // clear the box before its next launch
        unsigned long long checkins = 0;    // the box's check-in counter once its instances drained
        unsigned long long gang_total = 0;  // the box's gang completion counter (mirror)
    };
    std::vector<SvcLane> svc_lanes;
    bool svc_aql = false;  // the lanes are AQL queues of the library's own (cfg.svc_queue_aql, and the code object loaded)
    AqlKernel svc_kernel;
    AqlKernel svc_clear_kernel;     // ocm_service_box_clear (object 0: clear with a host memset)
    uint64_t svc_promotions = 0;  // gang ops that replaced a lone lead with a full instance
    uint64_t svc_overlaps = 0;    // instances dispatched on a lane whose previous lead had not left yet
    uint64_t svc_drain_max_ns = 0;   // the longest wait for a lane to drain (health)
    unsigned svc_drain_max_site = 0; // where: 1 start, 2 park, 3 stop, 4 abort, 5 re-post
    int svc_lane = -1;
    unsigned svc_epoch = 0;
    int svc_stream_prio = 0;
    bool svc_prio_ok = false;
    bool svc_running = false;
    bool svc_shared_queue = false;  // no priority stream for the service: it may share a launch stream's hardware queue
    unsigned long long svc_seq = 0;
    uint64_t svc_ops = 0, svc_ns_post = 0, svc_ns_wait = 0;  // service diagnostics (ocm_x_service_stats)
    uint64_t svc_gpu_ticks_done = 0;  // GPU ticks of the instances before the current one
    uint64_t svc_relaunches = 0;    // instances started after an idle exit (ocm_x_service_stats)
    uint64_t svc_ns_relaunch = 0;   // host time of those restarts (reap + launch), ocm_x_service_health
    // round 5: ops that started an instance, split (ocm_x_service_health): host ns from the
    // dispatch to seeing the lead's start stamp, GPU ticks (100 MHz) from the lead's start to
    // its first request seen, and host ns from entering the op to its completion
    uint64_t svc_cold_ops = 0, svc_cold_ns_to_start = 0, svc_cold_ticks_to_seen = 0, svc_cold_ns_total = 0;
    // round 6: the last kColdRing cold ops one by one, so a few
    // pathological starts show as a p99 / max with the op's seq instead of vanishing
    // into a mean (ocm_x_service_cold); `fired`: the start fired a pre-armed instance
    struct ColdSample {
        uint64_t seq = 0, to_start_ns = 0, total_ns = 0, seen_ticks = 0;
        bool fired = false;
    };
    static constexpr size_t kColdRing = 4096;
    std::vector<ColdSample> svc_cold_ring;
    uint64_t svc_cold_next = 0;      // samples ever written (ring index = next % kColdRing)
    bool svc_start_fired = false;    // the last service_start fired a pre-armed instance
    // every lane drain: count, total ns, and how many took over 1 ms (the max is above)
    uint64_t svc_drains = 0, svc_drain_ns_total = 0, svc_drains_over_1ms = 0;
    // OCM_SERVICE_PROTO TRACE: the host's side of each op at [seq % kServiceOpTrace]:
    // seq, entry, posted, done seen (now_ns), lane, flags (1: started an instance), width
    std::vector<std::array<uint64_t, 7>> svc_optrace;
    // Embedded daemon in this process (libocmd.so): maps its own slabs' IPC handles to
    // their device pointers (HIP does not open a process's own handles)
    void *(*slab_resolver)(const unsigned char *handle) = nullptr;
    uint64_t svc_fires = 0, svc_arms = 0, svc_disarms = 0, svc_inline_starts = 0;  // disarms: cancelled at the window's end
    std::atomic<uint64_t> svc_arm_window_ns{0};  // cfg.svc_arm_window_ns at init (ocm_x_set_prearm_window); read by the armer without the library lock
    uint64_t svc_arm_after_ns = 0;                // idle time after which the armer arms
    std::atomic<uint64_t> svc_last_op_ns{0};      // completion of the last service op
    std::atomic<bool> svc_armer_waiting{false};   // the armer sleeps until the next op
    std::atomic<bool> svc_armer_stop{false};
    std::mutex svc_arm_mu;
    std::condition_variable svc_arm_cv;
    std::thread *svc_armer = nullptr;             // started with the first instance (never copied into a fork)
    pid_t svc_armer_pid = 0;
    uint64_t svc_ns_pick = 0, svc_ns_launch = 0, svc_epoch_starts = 0;  // every start: choosing a lane, the launch call
    uint64_t svc_launch_ns = 0;  // when the running instance was launched (the roster wait, cfg.svc_roster_wait_ns)
    // Health counters (ocm_x_service_health): gang ops sized below the width they
    // wanted because fewer members were resident, instances that left with the
    // posted op unfinished (re-posted), ops abandoned after OCM_SERVICE_TIMEOUT_MS
    // (drained, then redone by a launch), and whether an instance could not even
    // be drained (the service is then off for good and the op fails).
    uint64_t svc_degraded = 0, svc_incomplete_exits = 0, svc_aborts = 0;
    unsigned long long svc_roster_min = ~0ull;  // smallest roster a gang op was sized to
    bool svc_wedged = false;
    // network tier
    std::map<std::string, NetConn> net_conns;  // "ip:port#stream" -> connection
    std::map<int, int> fd_chans;               // owner rank -> mailbox connection for slab fds (MSG_SLAB_FD)
    // Local GPU halves: stream-ordered pool (no device-wide sync in free, freed
    // blocks reused without a new VA mapping). Reference K8: cudaMalloc/cudaFree.
    hipMemPool_t pool = nullptr;
    // Async one-sided ops run on lane streams, one lane per allocation (round
    // robin), so ops on different allocations (different peers / links) overlap.
    std::vector<hipStream_t> lanes;
    int next_lane = 0;
    // Kernel-published completion of blocking launch-path ops (XferDone), one
    // slot per lane: a host-coherent flag line and a device counter line.
    unsigned long long *lane_flags = nullptr;  // 16 words per lane
    unsigned int *lane_cnt = nullptr;          // 32 words per lane
    std::vector<unsigned long long> lane_flag_seq;
    bool pool_tried = false;
    uint64_t pool_keep = 8ull << 30;       // bytes kept reserved across frees
    // Freed pool blocks kept for an exact-size reuse (OCM_LOCAL_CACHE bytes, 0 = off):
    // a reuse needs no HIP call at all, where a pool allocation right after a
    // stream-ordered free must wait for that free on the stream.
    std::multimap<size_t, void *> dev_cache;
    uint64_t dev_cache_bytes = 0;
    hipEvent_t done = nullptr;
    class PinnedArena *pinned = nullptr;   // created on first use
    std::map<int, PushDev> push;           // XFER_PUSH: owner device -> its stream
    hipEvent_t push_order = nullptr;       // the app stream's position the push launches wait for
    uint64_t push_launches = 0;
};

State &S();
long now_ms();
Msg new_msg(uint32_t type);
// Send a request and wait for the reply carrying the same seq.
int rpc(Msg &req, Msg *reply, int timeout_ms);
int recv_seq(Msg *m, uint64_t seq, uint32_t type, int timeout_ms);
bool is_pair(enum ocm_kind k);

// The ABI side of a timed call: trace range, hang watch (watched calls, under the range's
// name), timing, count(counters, ns, ok) and the op log, which records `traced` bytes.
// impl returns an int (0: success) or a pointer (non-null: success).
template <class Impl, class Count>
auto abi_call(const char *range, bool watched, const char *op, const uint64_t &traced, Impl impl, Count count) {
    TraceRange tr(range);
    std::optional<HangWatch> hw;
    if (watched) hw.emplace(range);
    const uint64_t t0 = now_ns();
    const auto r = impl();
    const uint64_t t1 = now_ns();
    int rc;
    if constexpr (std::is_pointer_v<decltype(impl())>)
        rc = r ? 0 : -1;
    else
        rc = r;
    count(S().ctr, t1 - t0, rc == 0);
    trace_op(op, traced, t0, t1, rc);
    return r;
}

// Run-time tuning as the hooks give it: nt 0 plain stores, 1 nontemporal, 2 sc1 loads and stores (register kernel).
inline XferTuning tuning_of(int variant, int blocks, int nt) {
    XferTuning t;
    t.variant = variant;
    t.max_blocks = blocks;
    t.nontemporal = nt != 0;
    t.write_through = nt == 2;
    return t;
}

struct DeviceGuard {
    int prev = -1;
    bool active = false;
    explicit DeviceGuard(int dev) {
        if (dev < 0) return;
        if (hipGetDevice(&prev) == hipSuccess && prev != dev) {
            (void)hipSetDevice(dev);
            active = true;
        }
    }
    ~DeviceGuard() {
        if (active) (void)hipSetDevice(prev);
    }
};

inline int log2_exact(uint64_t v) {
    if (v == 0 || (v & (v - 1))) return -1;
    return __builtin_ctzll(v);
}

// The pair's side of a kernel's launch arguments (any of the argument structs with
// ext, n_ext and unit_shift): the extent table, its length and, for a striped pair,
// log2 of the stripe unit. Returns that shift (0: not striped), or -1 when the pair is
// striped and its unit is not a power of two or is below 2^min_shift (4 for the
// kernels that need 16-byte units); unit_shift is then left alone.
template <class Args>
int pair_side_shift(uint64_t unit, int min_shift, Args *args) {
    const int sh = args->n_ext > 1 ? log2_exact(unit) : 0;
    if (sh < 0 || (args->n_ext > 1 && sh < min_shift)) return -1;
    args->unit_shift = (uint32_t)sh;
    return sh;
}
template <class Args>
int pair_side(const lib_alloc *a, int min_shift, Args *args) {
    for (size_t i = 0; i < a->ext.size(); i++) args->ext[i] = a->ext[i].dptr;
    args->n_ext = (uint32_t)a->ext.size();
    return pair_side_shift(a->stripe_unit, min_shift, args);
}
// The same over raw extent pointers (ocm_x_xfer, ocm_x_batch).
template <class Args>
int pair_side(void *const *ext, int n_ext, uint64_t unit, int min_shift, Args *args) {
    for (int i = 0; i < n_ext; i++) args->ext[i] = static_cast<char *>(ext[i]);
    args->n_ext = (uint32_t)n_ext;
    return pair_side_shift(unit, min_shift, args);
}

// ---- import cache (runtime.cpp)
int import_extent(Extent &e);
int slab_fd_from_owner(int owner, uint32_t slab_id, uint32_t tier);
void close_fd_chans();
void release_extent(const Extent &e, bool force);

// ---- pinned host arena for local halves (runtime.cpp)
// hipHostMalloc pins pages (64 MiB ~ 10 ms) and hipHostFree synchronizes the
// device (~230 us even for 4 KiB), so pinned local halves come from chunks
// pinned once: small requests are best-fit ranges of shared 64 MiB chunks,
// large ones get a dedicated chunk that is cached for reuse after free. Idle
// chunks beyond OCM_PINNED_KEEP bytes (default 2 GiB) are unpinned.
class PinnedArena {
public:
    void *alloc(size_t bytes);
    bool free(void *p);  // false: not from this arena
    void release_all();
    uint64_t pinned() const { return pinned_; }

private:
    struct Chunk {
        char *base = nullptr;
        uint64_t bytes = 0;
        bool dedicated = false;
        RangeAllocator ra;
    };
    void trim();
    std::map<uintptr_t, Chunk> chunks_;  // base -> chunk
    uint64_t pinned_ = 0;
};

// ---- local halves (runtime.cpp)
Loc pointer_loc(const void *p);
void release_dev_cache();
hipMemPool_t local_pool();
int free_local_half(lib_alloc *a);
int alloc_local_half(lib_alloc *a, size_t bytes, Loc want);

// ---- copy engine (transfer.cpp)
struct Seg {
    int ext;
    uint64_t ext_off;
    uint64_t lin_off;
    uint64_t len;
};
void segments(const lib_alloc *a, uint64_t rem_off, uint64_t len, std::vector<Seg> &out);
int wait_event(hipEvent_t ev);
int honor_dep(lib_alloc *a, hipStream_t st, bool host_wait);
int wait_alloc(lib_alloc *a);
hipStream_t lane_stream(lib_alloc *a);
int sync_stream();
// The end of an async op queued on `st` (lane_stream): records the allocation's event
// on its lane, or, with no lane available, completes the op now.
int async_done(lib_alloc *a, hipStream_t st);
// The hang watch's dump of library state (OCM_HANG_DUMP_S; runtime.cpp).
void print_hang_state(int fd);
// Close an HBM mapping of another process's slab: its per-device views, then the import
// itself (a DMA-BUF import or an IPC open). runtime.cpp.
void close_gpu_mapping(Mapping &m);
// `done` (optional, async launches on a lane): receives the kernel-published
// completion flag of the launch, or flag == nullptr when the op has none.
int xfer(lib_alloc *a, bool put, char *lin, Loc lloc, uint64_t rem_off, uint64_t len, bool async,
         XferDone *done = nullptr);
// Wait for a kernel-published flag (>= val), with the runtime event as the backstop.
int wait_done(const XferDone &d, hipEvent_t ev);
int copy_local(void *dst, Loc dl, const void *src, Loc sl, size_t n);
// Push-based get (XFER_PUSH): launches on every owner's GPU, ordered after the work
// queued on `st`; blocking ops wait on the host, async ones make `st` wait.
int push_get(lib_alloc *a, char *lin, uint64_t rem_off, uint64_t len, hipStream_t st, bool async);
void push_release();
// An address of extent e valid on device `dev` (its owner's GPU), opening its slab there once.
char *extent_view(const Extent &e, int dev);

// ---- copy service (service.cpp)
// OCM_SERVICE_EAGER: the copy service's setup at ocm_init
int service_prepare();
int service_start(unsigned long long first_seq, const XferArgs *inline_x = nullptr, bool strict = false);
void service_park();
void service_stop();
// OCM_SERVICE_PREARM: the idle-time armer thread
void service_armer_start();
void service_armer_note_op(uint64_t t_done);
// strict: an extent is in another GPU's HBM (kServiceGangStrict).
// 0: done; -1: failed, and no instance holds the request any more (a launch may
// redo the op); -2: failed and the instance could not be drained (no fallback).
int service_xfer(XferArgs x, unsigned solo_tiles, bool hbm, bool strict);
// Before a library launch: park the service when it may share the launch's hardware queue.
void before_launch();

// ---- descriptor lists (batches and their kin): lists.h

// ---- indexed ops (indexed.cpp), and the indexed converting ops that share their skip count (quant_indexed.cpp)
// The allocation's skip words (skip_dev, skip_host), made on first use: the device word
// zeroed on `st`, which every later op of the allocation is ordered after.
int skip_words(lib_alloc *a, hipStream_t st);
// Rows that `a`'s completed async indexed ops, of either call, skipped and no call has
// reported yet: 0 when there are none, else -1 with the error set, once (ocm_wait).
int indexed_take_skips(lib_alloc *a);
// Reports k rows as skipped: 0 when k is 0, else counts them (n_indexed_skipped) and
// returns -1 with the error "indexed ops skipped k row(s)" set.
int indexed_fail_skips(uint64_t k);
// Frees the allocation's skip words (ocm_free).
void indexed_release(lib_alloc *a);

// ---- network tier (net.cpp)
void net_drop(const std::string &ep);
void net_close_all();
int net_piece(const Extent &e, bool put, char *lin, Loc lloc, uint64_t ext_off, uint64_t len);

#pragma GCC visibility pop
}  // namespace ocmlib
