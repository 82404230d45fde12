// libocm copy service, host side: the lanes its instances run on, setup, start, park
// and stop, the pre-arm helper thread, and one blocking op through the resident
// kernel (service_xfer). The device side is kernels/xfer_service.hip; the records,
// status words and protocol bits both sides share are in ocm/xfer.h.
#include "internal.h"

namespace ocmlib {

// ---- persistent copy service ----
// Instances run on lanes: an AQL queue of the library's own (ocm/aql.h; HIP does
// not know it, so a device-wide synchronize never waits for the service and the
// lead may stay resident alone between bursts, OCM_SERVICE_LONE_US) or, when that
// is unavailable or OCM_SERVICE_QUEUE=hip, a HIP stream of the service's priority
// (then the whole instance leaves after OCM_SERVICE_IDLE_US).

static bool lane_idle(State::SvcLane &l) {
    if (l.aql) return aql_lane_idle(&l.q);
    const hipError_t e = hipStreamQuery(l.stream);
    (void)hipGetLastError();
    return e == hipSuccess;
}

// Wait until every workgroup of the lane's last instance has left. 0: drained;
// -1: not within timeout_ns. `site` names the caller in the health counters
// (the longest drain and where it happened).
enum DrainSite : unsigned { kDrainStart = 1, kDrainPark, kDrainStop, kDrainAbort, kDrainRepost };
static int lane_drain_timed(State::SvcLane &l, uint64_t timeout_ns) {
    if (l.aql) return aql_lane_wait(&l.q, timeout_ns);
    const uint64_t t0 = now_ns();
    hipError_t e;
    while ((e = hipStreamQuery(l.stream)) == hipErrorNotReady) {
        if (now_ns() - t0 > timeout_ns) return -1;
        usleep(20);
    }
    (void)hipGetLastError();
    return 0;
}
static int lane_drain(State::SvcLane &l, uint64_t timeout_ns, DrainSite site) {
    State &s = S();
    const uint64_t t0 = now_ns();
    const int rc = lane_drain_timed(l, timeout_ns);
    const uint64_t dt = now_ns() - t0;
    s.svc_drains++;
    s.svc_drain_ns_total += dt;
    s.svc_drains_over_1ms += dt > 1000000ull;
    if (dt > s.svc_drain_max_ns) {
        s.svc_drain_max_ns = dt;
        s.svc_drain_max_site = site;
    }
    return rc;
}

// The current instance's tagged status words (ocm/xfer.h): 0 unless it wrote them.
static unsigned long long svc_word(const unsigned long long *w) {
    return service_untag(S().svc_epoch, __atomic_load_n(w, __ATOMIC_ACQUIRE));
}

// STOP on both records: the small-op record and, if present, the gang record with its copies.
static void service_post_stop() {
    State &s = S();
    service_store_seq(s.svc_req, kServiceStop);
    if (s.svc_greq) service_store_seq(s.svc_greq, kServiceStop, s.svc_greq_copies);
}

// A new lane: an AQL queue or a stream of the service's priority, and a gang box. -1 on failure.
static int service_new_lane() {
    State &s = S();
    State::SvcLane l;
    if (s.svc_aql) {
        if (aql_lane_create(&l.q, true) != 0) return -1;
        l.aql = true;
    } else {
        hipError_t e = s.svc_prio_ok ? hipStreamCreateWithPriority(&l.stream, hipStreamNonBlocking, s.svc_stream_prio)
                                     : hipStreamCreateWithFlags(&l.stream, hipStreamNonBlocking);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            return -1;
        }
    }
    if (hipMalloc(reinterpret_cast<void **>(&l.box), sizeof(ServiceBox)) != hipSuccess) {
        (void)hipGetLastError();
        if (l.aql)
            aql_lane_destroy(&l.q);
        else
            (void)hipStreamDestroy(l.stream);
        return -1;
    }
    l.dirty = true;  // fresh device memory: its first launch clears it
    s.svc_lanes.push_back(l);
    return (int)s.svc_lanes.size() - 1;
}

// The copy service's one-time setup: its coherent slot, the AQL code object and
// kernels, the first lane and the record pages. Idempotent; 0 when ready.
static int service_setup() {
    State &s = S();
    if (!s.svc) {
        if (hipHostMalloc(reinterpret_cast<void **>(&s.svc), sizeof(ServiceSlot),
                          hipHostMallocCoherent | hipHostMallocMapped) != hipSuccess) {
            (void)hipGetLastError();
            s.svc = nullptr;
            s.cfg.svc_max = 0;
            OCM_FAIL(-1, "copy service: no coherent host memory");
        }
        std::memset(s.svc, 0, sizeof(ServiceSlot));
        s.svc_req = &s.svc->req;
        // The library's own AQL queue when the embedded code object loads for this
        // device; otherwise HIP streams (and no lone lead: a device-wide synchronize
        // would wait for it).
        s.svc_aql = false;
        if (s.cfg.svc_queue_aql) {
            const char *why = nullptr;
            if (aql_open(s.device, &why) != 0)
                OCM_INFO("copy service on HIP streams: AQL queue unavailable (%s)", why ? why : "?");
            else if (aql_kernel(kServiceKernelSymbol, &s.svc_kernel) != 0 ||
                     s.svc_kernel.kernarg_bytes < sizeof(ServiceKernelArgs))
                OCM_INFO("copy service on HIP streams: no usable %s in the embedded code object", kServiceKernelSymbol);
            else
                s.svc_aql = true;
            // OCM_SERVICE_CLEAR_KERNEL=0: clear gang boxes with a host memset (A/B)
            if (s.svc_aql && (env_int("OCM_SERVICE_CLEAR_KERNEL", 1) == 0 ||
                              aql_kernel(kServiceBoxClearSymbol, &s.svc_clear_kernel) != 0))
                s.svc_clear_kernel = AqlKernel{};
        }
        if (!s.svc_aql) s.cfg.svc_lone_ticks = 0;
        // Streams of their own priority: HIP shares its few hardware queues
        // (GPU_MAX_HW_QUEUES) among a process's streams, and a launch on a stream
        // that shares the service's queue waits behind the persistent kernel until
        // its idle exit (2 ms per large op in bench.py with torch's streams around, when
        // the idle exit was 2 ms).
        // Queues are pooled per priority, so the service's is not shared with the
        // normal-priority streams of the library and the application.
        int lo = 0, hi = 0;
        s.svc_prio_ok = hipDeviceGetStreamPriorityRange(&lo, &hi) == hipSuccess && lo != hi;
        (void)hipGetLastError();
        s.svc_stream_prio = env_int("OCM_SERVICE_STREAM_PRIO", hi);
        if (service_new_lane() < 0 && s.svc_aql) {
            OCM_INFO("copy service on HIP streams: no AQL queue could be created");
            s.svc_aql = false;
            s.cfg.svc_lone_ticks = 0;
            service_new_lane();
        }
        if (s.svc_lanes.empty() && s.svc_prio_ok) {
            s.svc_prio_ok = false;
            s.svc_shared_queue = true;  // launches park the service first (see before_launch)
            service_new_lane();
        }
        if (s.svc_lanes.empty()) {
            s.cfg.svc_max = 0;
            OCM_FAIL(-1, "copy service: no stream or device mailbox");
        }
        s.svc_lane = 0;
        const bool gangrec = (s.cfg.svc_proto & kServiceProtoGangRec) && s.cfg.svc_blocks > 1;
        const bool wc = (s.cfg.svc_proto & kServiceProtoWCReq) != 0;
        if (gangrec || wc) {
            // page 0: the small-op record when write-combined; page 1: the gang record
            const unsigned flags = (wc ? hipHostMallocWriteCombined : hipHostMallocCoherent) | hipHostMallocMapped;
            if (hipHostMalloc(reinterpret_cast<void **>(&s.svc_rec_pages), 8192, flags) != hipSuccess) {
                (void)hipGetLastError();
                s.svc_rec_pages = nullptr;  // one coherent record, relay protocol
                OCM_WARN("copy service: no %s record pages; using one coherent record and the relay protocol",
                         wc ? "write-combined" : "gang");
            } else {
                for (int i = 0; i < 8192 / 8; i++) __atomic_store_n(reinterpret_cast<unsigned long long *>(s.svc_rec_pages) + i, 0ull, __ATOMIC_RELAXED);
                __builtin_ia32_sfence();
                if (wc) s.svc_req = reinterpret_cast<ServiceReq *>(s.svc_rec_pages);
                if (gangrec) {
                    s.svc_greq = reinterpret_cast<ServiceReq *>(s.svc_rec_pages + 4096);
                    s.svc_greq_copies = (s.cfg.svc_proto & kServiceProtoCopies)
                                            ? std::max(1u, std::min(std::min(s.cfg.svc_direct, s.cfg.svc_blocks),
                                                                    (unsigned)kServiceGangCopiesMax))
                                            : 1u;
                }
            }
        }
    }
    return 0;
}

// OCM_SERVICE_EAGER (default on; ocm_init): the setup above at attach time instead of
// inside the first op, which paid ~6 ms for it (the multi-ms cold
// starts of profiles/pytest_gpu_r06b.log were all first ops of a process). The first
// lane's gang box is cleared here, so the armer can queue the first instance too.
int service_prepare() {
    State &s = S();
    DeviceGuard g(s.device);
    if (service_setup() != 0) return -1;
    State::SvcLane &l = s.svc_lanes[(size_t)s.svc_lane];
    if (l.dirty && hipMemsetAsync(l.box, 0, sizeof(ServiceBox), s.stream) == hipSuccess &&
        hipStreamSynchronize(s.stream) == hipSuccess) {
        l.dirty = false;
        l.gang_total = 0;
        l.checkins = 0;
    }
    (void)hipGetLastError();
    if (l.aql && s.cfg.svc_prearm) {
        service_armer_start();
        service_armer_note_op(now_ns());  // arms once the idle period has passed
    }
    return 0;
}

int service_start(unsigned long long first_seq, const XferArgs *inline_x, bool strict) {
    State &s = S();
    DeviceGuard g(s.device);
    if (service_setup() != 0) return -1;
    if (s.svc_wedged) OCM_FAIL(-1, "copy service: a previous instance could not be drained");
    // A lane whose last instance has drained: the current one normally (its last
    // instance's workgroups leave microseconds after its lead), another drained one,
    // a new one, or - every lane still holding workgroups that found no CU, or a
    // lone lead that has not yet seen it was replaced - wait for the current.
    // HIP lanes: when the last instance had its whole grid resident (its roster is
    // still in the slot), its workgroups leave right behind its lead: stay on its
    // lane without a runtime query (stream order starts the new instance after them;
    // they ignore the new epoch meanwhile). A stream query costs ~10 us of host
    // time; an AQL lane's is one load of its completion signal.
    // AQL lanes: when the last instance had its whole grid resident (a lone lead
    // included: only such an instance goes lone), the new one goes on the same
    // queue right away, beside a lead that has not left yet (it leaves on the new
    // epoch; the packet starts once the old one's workgroups have all been
    // dispatched, which they have): no new queue, no wait.
    const uint64_t tq = now_ns();
    int pick = -1;
    bool overlap = false;
    const int n = (int)s.svc_lanes.size();
    const bool whole = s.svc_lane >= 0 && svc_word(&s.svc->roster) >= s.cfg.svc_blocks;
    if (whole && !s.svc_aql && !s.cfg.svc_relaunch_query) pick = s.svc_lane;
    if (whole && s.svc_aql && !s.svc_lanes[(size_t)s.svc_lane].dirty && !s.cfg.svc_box_reset_always &&
        s.svc_lanes[(size_t)s.svc_lane].gang_total <= (1ull << 30)) {  // a box clear would make a third dispatch
        const long run = aql_lane_inflight(&s.svc_lanes[(size_t)s.svc_lane].q);
        if (run <= 1) {
            pick = s.svc_lane;
            overlap = run == 1;
        }
    }
    for (int k = 0; k < n && pick < 0; k++) {
        const int i = (s.svc_lane + k) % n;
        if (lane_idle(s.svc_lanes[(size_t)i])) pick = i;
    }
    if (pick < 0 && (unsigned)n < s.cfg.svc_lanes_max) pick = service_new_lane();
    if (pick < 0) {
        pick = s.svc_lane;
        if (s.svc_lanes[(size_t)pick].aql) {
            // a lone lead on it leaves once it sees the new epoch
            __atomic_store_n(&s.svc->epoch_now, (unsigned long long)((s.svc_epoch + 1) & (unsigned)kServiceGangEpochMask),
                             __ATOMIC_RELEASE);
            __builtin_ia32_sfence();
        }
        if (lane_drain(s.svc_lanes[(size_t)pick], s.cfg.svc_drain_ns, kDrainStart) != 0) {
            s.svc_wedged = true;
            s.cfg.svc_max = 0;
            OCM_FAIL(-1, "copy service: no lane drained within OCM_SERVICE_DRAIN_MS");
        }
    }
    s.svc_lane = pick;
    State::SvcLane &l = s.svc_lanes[(size_t)pick];
    s.svc_stream = l.stream;
    s.svc_box = l.box;
    s.svc_epoch = (s.svc_epoch + 1) & (unsigned)kServiceGangEpochMask;
    // the last instance's GPU time (diagnostic) joins the total; a lead that is still
    // leaving serves nothing more, so it writes no more ticks
    s.svc_gpu_ticks_done += __atomic_exchange_n(&s.svc->gpu_ticks, 0ull, __ATOMIC_ACQ_REL);
    __atomic_store_n(&s.svc->exited, 0ull, __ATOMIC_RELEASE);
    __atomic_store_n(&s.svc->roster, 0ull, __ATOMIC_RELEASE);  // the new lead publishes its own
    __atomic_store_n(&s.svc->lone, 0ull, __ATOMIC_RELEASE);
    // A lone lead of an earlier instance (another lane) leaves when it sees this.
    __atomic_store_n(&s.svc->epoch_now, (unsigned long long)s.svc_epoch, __ATOMIC_RELEASE);
    service_store_seq(s.svc_req, 0ull);  // clear a STOP left by a parked instance
    if (s.svc_greq) service_store_seq(s.svc_greq, 0ull, s.svc_greq_copies);
    // the gang counter mirror stays below the 31-bit target field (ocm/xfer.h)
    const bool reset = l.dirty || s.cfg.svc_box_reset_always || l.gang_total > (1ull << 30);
    if (reset) {
        l.gang_total = 0;  // the launch zeroes the device counters
        l.checkins = 0;
    }
    ServiceKernelArgs ka;
    std::memset(&ka, 0, sizeof(ka));
    ka.req = s.svc_req;
    ka.gang_req = s.svc_greq;
    ka.slot = s.svc;
    ka.box = l.box;
    ka.first_seq = first_seq;
    ka.idle_ticks = s.cfg.svc_idle_ticks;
    ka.proto = s.cfg.svc_proto;
    ka.direct_wgs = std::min(s.cfg.svc_direct, s.cfg.svc_blocks);
    ka.checkin_base = l.checkins;
    ka.epoch = s.svc_epoch;
    ka.blocks = s.cfg.svc_blocks;
    ka.degraded_idle_ticks = s.cfg.svc_degraded_idle_ticks;
    ka.lone_ticks = l.aql ? s.cfg.svc_lone_ticks : 0;
    if (inline_x && s.cfg.svc_inline) {
        // the solo request the caller posts next, as it will post it (active 1, no target)
        const unsigned long long gang = 1ull | ((unsigned long long)s.svc_epoch << kServiceGangEpochShift) |
                                        (strict ? kServiceGangStrict : 0ull);
        service_record(ka.first_rec, *inline_x, gang, first_seq);
        s.svc_inline_starts++;
    }
    const uint64_t tl = now_ns();
    s.svc_ns_pick += tl - tq;
    if (l.aql && s.cfg.svc_prearm && !s.svc_armer) service_armer_start();
    s.svc_start_fired = false;
    if (l.aql && s.cfg.svc_prearm && l.q.armed && !reset && aql_fire(&l.q, &ka, sizeof(ka)) == 0) {
        // the instance the armer queued while the service was idle: write its arguments,
        // open its gate (the armer queues the next one once the service is idle again)
        s.svc_fires++;
        s.svc_start_fired = true;
        if (overlap) s.svc_overlaps++;
    } else if (l.aql) {
        // The box is cleared first: on the lane itself, the instance behind it with the
        // barrier bit (the queue is not a HIP stream); a host memset if that kernel is missing.
        bool barrier = false;
        if (reset && s.svc_clear_kernel.object && !overlap) {
            ServiceBox *bx = l.box;
            if (aql_dispatch(&l.q, s.svc_clear_kernel, &bx, sizeof(bx), 1, 256) != 0) {
                s.cfg.svc_max = 0;
                OCM_FAIL(-1, "copy service: gang box clear dispatch failed");
            }
            barrier = overlap = true;
        } else if (reset && (hipMemsetAsync(l.box, 0, sizeof(ServiceBox), s.stream) != hipSuccess ||
                             hipStreamSynchronize(s.stream) != hipSuccess)) {
            (void)hipGetLastError();
            s.cfg.svc_max = 0;
            OCM_FAIL(-1, "copy service: clearing the gang box failed");
        }
        if (aql_dispatch(&l.q, s.svc_kernel, &ka, sizeof(ka), s.cfg.svc_blocks, 256, overlap, barrier) != 0) {
            s.cfg.svc_max = 0;
            OCM_FAIL(-1, "copy service dispatch failed");
        }
        if (overlap && !barrier) s.svc_overlaps++;
    } else if (service_launch(ka, s.cfg.svc_blocks, reset, l.stream) != hipSuccess) {
        (void)hipGetLastError();
        s.cfg.svc_max = 0;
        OCM_FAIL(-1, "copy service launch failed");
    }
    s.svc_ns_launch += now_ns() - tl;
    s.svc_epoch_starts++;
    l.dirty = false;
    l.checkins += s.cfg.svc_blocks;  // every workgroup takes one ticket before the instance drains
    s.svc_running = true;
    s.svc_launch_ns = now_ns();
    return 0;
}

// Without a stream priority of its own (svc_shared_queue) the service may share
// a hardware queue with the library's launch streams, and a launch queued behind
// the persistent kernel would wait for its idle exit: park it first. Application
// kernels on such a queue still wait up to OCM_SERVICE_IDLE_US.
void before_launch() {
    State &s = S();
    if (s.svc_shared_queue) service_park();
}

// Park the resident kernel: its doorbell polls cross PCIe and slow down
// large DMA-engine transfers (measured: 53 -> 34 GiB/s on host-tier sweeps).
void service_park() {
    State &s = S();
    if (!s.svc || !s.svc_running) return;
    DeviceGuard g(s.device);
    service_post_stop();
    State::SvcLane &l = s.svc_lanes[(size_t)s.svc_lane];
    if (l.aql) {
        if (lane_drain(l, s.cfg.svc_drain_ns, kDrainPark) != 0) {
            s.svc_wedged = true;
            s.cfg.svc_max = 0;
            OCM_WARN("copy service did not leave on STOP within OCM_SERVICE_DRAIN_MS; the service is off");
        }
    } else {
        (void)hipStreamSynchronize(l.stream);
    }
    s.svc_running = false;
}

// The armer (OCM_SERVICE_PREARM): sleeps until the service has been idle for
// svc_arm_after_ns past its last op, then, if the instance has left and its lane is
// drained, queues the next instance behind a closed gate (aql_arm). One arm per idle
// period; an op wakes it for the next one. It never blocks on the library lock (the
// op path and service_stop hold it): it tries, and retries a little later.
static void service_armer_try_arm() {
    State &s = S();
    std::unique_lock<std::recursive_mutex> lk(s.mu, std::try_to_lock);
    if (!lk.owns_lock() || s.svc_armer_stop.load()) return;
    if (!s.svc || !s.cfg.svc_prearm || s.svc_lane < 0) return;
    State::SvcLane &l = s.svc_lanes[(size_t)s.svc_lane];
    if (!l.aql || l.q.armed || l.dirty) return;
    if (s.svc_running && svc_word(&s.svc->exited) == 0) return;  // an instance (a lone lead) still runs
    if (aql_lane_inflight(&l.q) != 0) return;
    DeviceGuard g(s.device);
    if (aql_arm(&l.q, s.svc_kernel, sizeof(ServiceKernelArgs), s.cfg.svc_blocks, 256) == 0) s.svc_arms++;
}

// The window's end (OCM_SERVICE_PREARM_MS): cancel the instance still armed, so the
// packet processor stops polling its gate (the cancelled kernel returns at once). Returns
// false when the library lock was busy (try again a little later).
static bool service_armer_try_disarm() {
    State &s = S();
    std::unique_lock<std::recursive_mutex> lk(s.mu, std::try_to_lock);
    if (!lk.owns_lock()) return false;
    if (s.svc_armer_stop.load() || !s.svc || s.svc_lane < 0 || s.svc_lane >= (int)s.svc_lanes.size()) return true;
    State::SvcLane &l = s.svc_lanes[(size_t)s.svc_lane];
    if (!l.aql || !l.q.armed) return true;
    DeviceGuard g(s.device);
    aql_disarm(&l.q);
    s.svc_disarms++;
    return true;
}

static void service_armer_loop() {
    name_thread("ocm-armer");
    State &s = S();
    uint64_t armed_for = 0;     // the last op whose idle period has been armed
    uint64_t disarmed_for = 0;  // ... and whose armed instance has been cancelled at the window's end
    uint64_t armed_at = 0;
    std::unique_lock<std::mutex> lk(s.svc_arm_mu);
    while (!s.svc_armer_stop.load()) {
        const uint64_t last = s.svc_last_op_ns.load();
        const uint64_t now = now_ns();
        const uint64_t window = s.svc_arm_window_ns.load(std::memory_order_relaxed);
        if (last != 0 && armed_for == last && disarmed_for != last && window) {
            // armed for this idle period: wait for an op (it notifies) or the window's end
            if (now < armed_at + window) {
                s.svc_armer_waiting.store(true);
                s.svc_arm_cv.wait_for(lk, std::chrono::nanoseconds(armed_at + window - now));
                s.svc_armer_waiting.store(false);
                continue;
            }
            if (s.svc_last_op_ns.load() != last) continue;
            lk.unlock();
            const bool done = service_armer_try_disarm();
            lk.lock();
            if (done)
                disarmed_for = last;
            else
                s.svc_arm_cv.wait_for(lk, std::chrono::microseconds(500));
            continue;
        }
        if (last == 0 || armed_for == last) {
            // nothing to arm for: sleep until an op (it notifies while we wait)
            s.svc_armer_waiting.store(true);
            s.svc_arm_cv.wait_for(lk, std::chrono::milliseconds(200));
            s.svc_armer_waiting.store(false);
            continue;
        }
        if (now < last + s.svc_arm_after_ns) {
            s.svc_arm_cv.wait_for(lk, std::chrono::nanoseconds(last + s.svc_arm_after_ns - now));
            continue;
        }
        lk.unlock();
        service_armer_try_arm();
        lk.lock();
        bool armed = false;
        {
            std::unique_lock<std::recursive_mutex> l2(s.mu, std::try_to_lock);
            armed = l2.owns_lock() && s.svc_lane >= 0 && s.svc_lane < (int)s.svc_lanes.size() &&
                    s.svc_lanes[(size_t)s.svc_lane].q.armed;
        }
        if (armed || s.svc_last_op_ns.load() != last) {
            armed_for = last;
            armed_at = now_ns();
            if (!armed) disarmed_for = last;  // an op came first: nothing armed to cancel
        } else {
            s.svc_arm_cv.wait_for(lk, std::chrono::microseconds(500));  // the lead may still be leaving
            if (now_ns() - last > 100 * s.svc_arm_after_ns) armed_for = disarmed_for = last;  // give up on this period
        }
    }
}

void service_armer_start() {
    State &s = S();
    if (s.svc_armer) return;
    s.svc_arm_after_ns = s.cfg.svc_idle_ticks * 10ull + (s.cfg.svc_lone_ticks * 10ull) + 500000ull;  // ticks: 100 MHz
    s.svc_armer_stop.store(false);
    s.svc_armer_pid = getpid();
    s.svc_armer = new std::thread(service_armer_loop);
}

// Called by every completed service op: the armer's idle clock starts over.
void service_armer_note_op(uint64_t t_done) {
    State &s = S();
    s.svc_last_op_ns.store(t_done, std::memory_order_relaxed);
    if (s.svc_armer_waiting.load(std::memory_order_relaxed)) {
        // only the first op after an idle period gets here; under the mutex, so the
        // wake-up cannot fall between the armer's flag and its wait
        std::lock_guard<std::mutex> lk(s.svc_arm_mu);
        s.svc_armer_waiting.store(false, std::memory_order_relaxed);
        s.svc_arm_cv.notify_one();
    }
}

static void service_armer_stop() {
    State &s = S();
    if (!s.svc_armer) return;
    if (s.svc_armer_pid != getpid()) {  // a forked child: the thread is the parent's
        s.svc_armer = nullptr;
        return;
    }
    {
        std::lock_guard<std::mutex> lk(s.svc_arm_mu);
        s.svc_armer_stop.store(true);
    }
    s.svc_arm_cv.notify_all();
    s.svc_armer->join();
    delete s.svc_armer;
    s.svc_armer = nullptr;
}

void service_stop() {
    State &s = S();
    service_armer_stop();  // before the lanes go (it takes the lock only by try_lock)
    if (!s.svc) return;
    DeviceGuard g(s.device);
    service_post_stop();
    s.svc_running = false;
    for (State::SvcLane &l : s.svc_lanes) {  // every lane drained before its box goes
        if (l.aql) {
            if (lane_drain(l, s.cfg.svc_drain_ns, kDrainStop) != 0) {
                // never free what a kernel that did not leave may still touch
                OCM_WARN("copy service: a lane did not drain at shutdown; its queue and box are leaked");
                continue;
            }
            aql_lane_destroy(&l.q);
        } else {
            (void)hipStreamSynchronize(l.stream);
            (void)hipStreamDestroy(l.stream);
        }
        if (l.box) (void)hipFree(l.box);
    }
    s.svc_lanes.clear();
    s.svc_lane = -1;
    s.svc_req = nullptr;
    if (s.svc_rec_pages) (void)hipHostFree(s.svc_rec_pages);
    s.svc_rec_pages = nullptr;
    s.svc_greq = nullptr;
    (void)hipHostFree(s.svc);
    s.svc = nullptr;
    s.svc_box = nullptr;
    s.svc_stream = nullptr;
}

// Members of the running instance a gang may name (ocm/xfer.h roster): right
// after a launch wait up to svc_roster_wait_ns for `want` of them to check in,
// then settle for the ones that did (at least workgroup 0).
static unsigned service_roster(unsigned want) {
    State &s = S();
    unsigned long long r = svc_word(&s.svc->roster);
    while (r < want && now_ns() - s.svc_launch_ns < s.cfg.svc_roster_wait_ns) {
        __builtin_ia32_pause();
        r = svc_word(&s.svc->roster);
    }
    if (r < 1) r = 1;
    if (r < want) s.svc_degraded++;
    if (r < s.svc_roster_min) s.svc_roster_min = r;
    return (unsigned)std::min<unsigned long long>(r, want);
}

// Give up on the instance holding request `seq`: STOP on both records, then wait
// (bounded) until the kernel has left, so no member can still run the request
// when the op is redone by a launch. -1: drained; -2: it would not drain.
static int service_abort(unsigned long long seq, unsigned long long active, const char *why) {
    State &s = S();
    DeviceGuard g(s.device);
    unsigned long long wg_in = 0;
    for (unsigned long long i = 0; i < active && i < (unsigned long long)kServiceWgDoneMax; i++)
        wg_in += __atomic_load_n(&s.svc->wg_done[i], __ATOMIC_ACQUIRE) == seq;
    const unsigned long long ex = svc_word(&s.svc->exited);
    const unsigned long long roster = svc_word(&s.svc->roster);
    service_post_stop();
    s.svc_aborts++;
    if (lane_drain(s.svc_lanes[(size_t)s.svc_lane], s.cfg.svc_drain_ns, kDrainAbort) != 0) {
        s.svc_wedged = true;
        s.cfg.svc_max = 0;
        OCM_FAIL(-2, "copy service %s (seq %llu, %llu members, %llu done words, roster %llu, exited %llu) "
                     "and did not leave on STOP: not redoing the op",
                 why, seq, active, wg_in, roster, ex);
    }
    s.svc_running = false;
    if (s.svc_lane >= 0) s.svc_lanes[(size_t)s.svc_lane].dirty = true;
    OCM_FAIL(-1, "copy service %s (seq %llu, %llu members, %llu done words, roster %llu, exited %llu); drained",
             why, seq, active, wg_in, roster, ex);
}

// One op in flight on the service: what the caller asked for, and what
// size_and_post decided about its gang and finished() polls for.
struct SvcOp {
    XferArgs x;  // normalized
    unsigned solo_tiles;
    bool hbm, strict;
    bool direct;  // small enough for the direct pollers (no relay)
    unsigned long long seq;
    unsigned long long active;  // members of the gang (1: a solo op)
    bool wgdone;                // completes through every member's own word
    ServiceReq *rq;             // the record posted to
    unsigned long long gang;    // the gang word posted with it
};

// The host's clock readings of one op (now_ns), for the accounting at its end.
struct SvcTimes {
    uint64_t enter;       // service_xfer entered
    uint64_t dispatched;  // this op started an instance: when (its latency is split at completion); else 0
    uint64_t t0, posted;  // before and after sizing and posting the request
    uint64_t start_seen;  // cold op: when the host saw the new lead's start stamp
};

// The host sizes the gang and the completion count every workgroup agrees on:
// up to the direct pollers (no relay) for ops they copy fast enough, and never
// wider than the members already running (the roster). Then it posts the request.
static int size_and_post(SvcOp &o) {
    State &s = S();
    const XferArgs &x = o.x;
    unsigned width = o.direct ? std::min(s.cfg.svc_direct, s.cfg.svc_blocks)
                              : (o.hbm ? s.cfg.svc_blocks : std::min(s.cfg.svc_gang_host, s.cfg.svc_blocks));
    if (!o.hbm && !x.put && x.len >= s.cfg.svc_host_get_narrow_min) width = std::min(width, s.cfg.svc_host_get_width);
    if (service_gang_size(x, width, o.solo_tiles) > 1) {
        // A lone lead takes no gang: a full instance replaces it (the lead leaves
        // on the new epoch by itself; it holds no request of ours).
        if (svc_word(&s.svc->lone) != 0) {
            s.svc_promotions++;
            if (service_start(o.seq) != 0) return -1;
        }
        width = service_roster(width);
    }
    o.active = service_gang_size(x, width, o.solo_tiles);
    o.wgdone = service_wg_done(s.cfg.svc_proto, o.active);
    unsigned long long target = 0;
    if (o.active > 1 && !o.wgdone) {  // WGDONE gangs leave the counter alone
        if (s.svc_lanes[(size_t)s.svc_lane].gang_total + o.active > kServiceGangTargetMask) {
            // A resident instance serving counter-completed gangs for long enough
            // would carry its target past the gang word's 31-bit field into the epoch
            // bits: park it; the fresh instance starts from a cleared box.
            service_park();
            s.svc_lanes[(size_t)s.svc_lane].dirty = true;
            if (service_start(o.seq) != 0) return -1;
            width = std::min(width, service_roster(width));
            o.active = service_gang_size(x, width, o.solo_tiles);
            o.wgdone = service_wg_done(s.cfg.svc_proto, o.active);
        }
        State::SvcLane &l = s.svc_lanes[(size_t)s.svc_lane];
        if (o.active > 1 && !o.wgdone) {
            l.gang_total += o.active;
            target = l.gang_total;
        }
    }
    o.gang = o.active | (target << 16) | ((unsigned long long)s.svc_epoch << kServiceGangEpochShift) |
             (o.strict ? kServiceGangStrict : 0ull);
    // GANGREC: gang requests go to the record the whole gang polls.
    o.rq = (o.active > 1 && s.svc_greq) ? s.svc_greq : s.svc_req;
    service_post(o.rq, x, o.gang, o.seq, o.rq == s.svc_greq ? s.svc_greq_copies : 1u);
    return 0;
}

// Completed: `done` (a solo op or the gang's last member), or under WGDONE
// every member's own word.
static inline bool finished(const State &s, const SvcOp &o) {
    if (!o.wgdone) return __atomic_load_n(&s.svc->done, __ATOMIC_ACQUIRE) == o.seq;
    for (unsigned long long i = o.active; i-- > 0;)
        if (__atomic_load_n(&s.svc->wg_done[i], __ATOMIC_ACQUIRE) != o.seq) return false;
    return true;
}

// The books of a completed op, seen done at t_done: the op count and the post and wait
// sums (ocm_x_service_stats), the armer's idle clock, the op trace slot (PROTO TRACE)
// and, for an op that started an instance, the cold-start split and its ring
// (ocm_x_service_health, ocm_x_service_cold). Out of line: the spin loop stays small.
__attribute__((noinline)) static void account_done(const SvcOp &o, SvcTimes &t, uint64_t t_done) {
    State &s = S();
    s.svc_ops++;
    s.svc_ns_post += t.posted - t.t0;
    s.svc_ns_wait += t_done - t.posted;
    if (s.cfg.svc_prearm) service_armer_note_op(t_done);
    if (s.cfg.svc_proto & kServiceProtoTrace) {
        if (s.svc_optrace.empty()) s.svc_optrace.resize(kServiceOpTrace);
        s.svc_optrace[o.seq & (kServiceOpTrace - 1)] = {o.seq, t.enter, t.posted, t_done, (uint64_t)s.svc_lane,
                                                        t.dispatched ? 1ull : 0ull, o.active};
    }
    if (!t.dispatched) return;
    const unsigned long long st = svc_word(&s.svc->start_ticks), fs = svc_word(&s.svc->first_seen_ticks);
    if (!t.start_seen) t.start_seen = t_done;  // the start stamp landed with done
    if (st && fs >= st) {
        s.svc_cold_ops++;
        s.svc_cold_ns_to_start += t.start_seen - t.dispatched;
        s.svc_cold_ticks_to_seen += fs - st;
        s.svc_cold_ns_total += t_done - t.enter;
        if (s.svc_cold_ring.empty()) s.svc_cold_ring.resize(State::kColdRing);
        State::ColdSample &cs = s.svc_cold_ring[s.svc_cold_next++ % State::kColdRing];
        cs.seq = o.seq;
        cs.to_start_ns = t.start_seen - t.dispatched;
        cs.total_ns = t_done - t.enter;
        cs.seen_ticks = fs - st;
        cs.fired = s.svc_start_fired;
    }
}

// The instance left with the op unfinished (`ex`: its exit word; 0: only its members
// left, and the lone lead is told to leave too): drain its lane and, unless the op
// turns out complete, give it to a new instance. kOpDone, kOpReposted, or < 0:
// failed, the value service_xfer returns.
enum : int { kOpDone = 0, kOpReposted = 1 };
static int service_repost(SvcOp &o, unsigned long long ex) {
    State &s = S();
    DeviceGuard g(s.device);
    if (!ex) service_post_stop();
    if (lane_drain(s.svc_lanes[(size_t)s.svc_lane], s.cfg.svc_drain_ns, kDrainRepost) != 0)
        return service_abort(o.seq, o.active, "left part of a request behind and did not drain");
    s.svc_running = false;
    s.svc_relaunches++;
    if (finished(s, o)) {
        s.svc_ops++;
        return kOpDone;
    }
    if (ex > o.seq) s.svc_incomplete_exits++;
    // Members may have counted part of the request in: start from a clean box.
    s.svc_lanes[(size_t)s.svc_lane].dirty = true;
    // Re-post under a fresh seq. Direct gang members of the instance that
    // left may have served part of this request and stored its seq in their
    // WGDONE words; under the old seq those stale words would count as the
    // new instance's members finishing, and the op would return while some
    // of them were still copying (a later write to the local half then raced
    // the copy: tests/test_gpu_service.py::test_service_direct_and_relayed_gangs_interleave).
    o.seq = ++s.svc_seq;
    if (service_start(o.seq) != 0) return -1;
    if (size_and_post(o) != 0) return -1;  // sized to the new instance's roster; start cleared the doorbell
    return kOpReposted;
}

// Run one normalized transfer through the resident kernel and wait for it.
int service_xfer(XferArgs x, unsigned solo_tiles, bool hbm, bool strict) {
    State &s = S();
    if (xfer_normalize(x) != hipSuccess) OCM_FAIL(-1, "invalid transfer");
    if (!hbm && x.len >= s.cfg.svc_host_tile_min && x.len <= s.cfg.svc_host_tile_max) {
        const unsigned sh = x.put ? s.cfg.svc_host_tile_shift_put : s.cfg.svc_host_tile_shift_get;
        if (sh >= 12 && sh < x.tile_shift) x.tile_shift = sh;
    }
    SvcOp o{x, solo_tiles, hbm, strict, false, ++s.svc_seq, 1, false, s.svc_req, 0};
    SvcTimes t{now_ns(), 0, 0, 0, 0};
    bool relaunched = false;
    if (s.svc_running && svc_word(&s.svc->exited) != 0) {
        // The instance left on its idle timeout (OCM_SERVICE_IDLE_US), its last request
        // complete: start the next one right away instead of posting to nobody. No wait
        // for its stream: the next instance takes a drained lane, and a workgroup of the
        // old one still polling (or starting late) leaves requests of a newer epoch alone.
        s.svc_running = false;
        s.svc_relaunches++;
        relaunched = true;
    }
    if (!s.svc_running) {
        // a solo op (its tiles within one workgroup's share) rides in the new instance's
        // arguments: ServiceKernelArgs::first_rec
        const bool solo = service_gang_size(o.x, 0xFFFFu, solo_tiles) == 1;
        if (service_start(o.seq, solo ? &o.x : nullptr, strict) != 0) return -1;
        t.dispatched = now_ns();
        if (relaunched) s.svc_ns_relaunch += t.dispatched - t.enter;
    }
    o.direct = s.svc_greq && o.x.len <= (hbm ? s.cfg.svc_direct_max_hbm : s.cfg.svc_direct_max_host);
    t.t0 = now_ns();
    if (size_and_post(o) != 0) return -1;
    t.posted = now_ns();
    for (unsigned spins = 1;; spins++) {
        if (finished(s, o)) {
            account_done(o, t, now_ns());
            return 0;
        }
        if (t.dispatched && !t.start_seen && svc_word(&s.svc->start_ticks)) t.start_seen = now_ns();
        if ((spins & 1023) == 0) {
            // The kernel leaves after idle_ticks without work, and only once the
            // last request it took is complete. If it left before taking this one
            // (exited <= seq), start a new instance for it. exited > seq with the
            // op unfinished is not expected (workgroup 0 waits for its members):
            // counted, and handled the same way, since after the drain no member
            // of the old instance is left to finish it. The same when the members
            // of the instance left (a lone lead) before this gang request: the lead
            // is told to leave too, and the op goes to a new instance.
            const unsigned long long ex = svc_word(&s.svc->exited);
            const unsigned long long ln = o.active > 1 ? svc_word(&s.svc->lone) : 0;
            if (ex || (ln && ln <= o.seq)) {
                const int rc = service_repost(o, ex);
                if (rc != kOpReposted) return rc;
            }
            if (now_ns() - t.t0 > s.cfg.svc_timeout_ns) return service_abort(o.seq, o.active, "did not complete a transfer in time");
        }
    }
}

}  // namespace ocmlib
