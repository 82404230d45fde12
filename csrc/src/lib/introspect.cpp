// Hooks for tests and benchmarks that look inside the library (not part of the ABI):
// counters, layouts, the copy service's statistics, health, cold starts and traces, the
// daemon's tick and placement statistics, and the run-time setters.
#include <cmath>

#include "internal.h"

using namespace ocm;
using namespace ocmlib;

extern "C" {


// Per-process operation counters (see ocm/trace.h): 28 x uint64.
void ocm_x_counters(uint64_t out[28]) {
    const OpCounters &c = S().ctr;
    const uint64_t v[28] = {c.n_put,  c.n_get,    c.bytes_put, c.bytes_get,   c.n_alloc,     c.n_free,
                            c.n_copy, c.bytes_copy, c.ns_put,  c.ns_get,      c.ns_alloc,    c.ns_free,
                            c.n_batch, c.n_batch_ops, c.bytes_batch, c.ns_batch, c.n_batch_launches,
                            c.n_slab_fd, c.n_slab_path, c.n_link_rpc, c.n_link_wake,
                            c.n_quant, c.n_quant_ops, c.bytes_quant_src, c.bytes_quant_wire,
                            c.n_strided, c.n_strided_ops, c.bytes_strided};
    std::memcpy(out, v, sizeof(v));
}

// The accumulate counters (ocm_x_counters keeps its 28 entries): calls, ops, accumulator bytes.
void ocm_x_acc_counters(uint64_t out[3]) {
    const OpCounters &c = S().ctr;
    out[0] = c.n_acc;
    out[1] = c.n_acc_ops;
    out[2] = c.bytes_acc;
}

// The strided converting counters, likewise: calls, ops, 16-bit source bytes, record bytes.
void ocm_x_quant_strided_counters(uint64_t out[4]) {
    const OpCounters &c = S().ctr;
    out[0] = c.n_quant_strided;
    out[1] = c.n_quant_strided_ops;
    out[2] = c.bytes_quant_strided_src;
    out[3] = c.bytes_quant_strided_wire;
}

// The indexed counters, likewise: calls, ops, rows named, nominal bytes, rows skipped.
void ocm_x_indexed_counters(uint64_t out[5]) {
    const OpCounters &c = S().ctr;
    out[0] = c.n_indexed;
    out[1] = c.n_indexed_ops;
    out[2] = c.n_indexed_rows;
    out[3] = c.bytes_indexed;
    out[4] = c.n_indexed_skipped;
}

// The indexed converting counters, likewise: calls, ops, rows named, 16-bit source bytes, record
// bytes (rows skipped are in ocm_x_indexed_counters' n_indexed_skipped, with the indexed ops').
void ocm_x_quant_indexed_counters(uint64_t out[5]) {
    const OpCounters &c = S().ctr;
    out[0] = c.n_quant_indexed;
    out[1] = c.n_quant_indexed_ops;
    out[2] = c.n_quant_indexed_rows;
    out[3] = c.bytes_quant_indexed_src;
    out[4] = c.bytes_quant_indexed_wire;
}

// The pooled-lookup counters, likewise: calls, ops, bags named, ids named, nominal bytes read
// (entries skipped are in ocm_x_indexed_counters' n_indexed_skipped, with the indexed ops').
void ocm_x_bag_counters(uint64_t out[5]) {
    const OpCounters &c = S().ctr;
    out[0] = c.n_bag;
    out[1] = c.n_bag_ops;
    out[2] = c.n_bag_bags;
    out[3] = c.n_bag_ids;
    out[4] = c.bytes_bag;
}

// Raw 64-byte handle of extent i (tests: the network tier's capability checks).
int ocm_x_extent_handle(ocm_alloc_t a, int i, uint8_t *out) {
    if (!a || !out || i < 0 || (size_t)i >= a->ext.size()) return -1;
    std::memcpy(out, a->ext[(size_t)i].r.handle, kHandleBytes);
    return 0;
}

// Layout of the app's shared-memory link (ocm/shmlink.h), for tests that drive a
// link by hand: {mapped bytes, req_taken, rsp_taken, daemon_polling, app_waiting,
// req[0], rsp[0], slot bytes, seq offset in a slot, slots, magic}.
void ocm_x_link_layout(uint64_t out[11]) {
    out[0] = ((uint64_t)sizeof(ShmLinkLayout) + 4095) & ~4095ull;
    out[1] = offsetof(ShmLinkLayout, req_taken);
    out[2] = offsetof(ShmLinkLayout, rsp_taken);
    out[3] = offsetof(ShmLinkLayout, daemon_polling);
    out[4] = offsetof(ShmLinkLayout, app_waiting);
    out[5] = offsetof(ShmLinkLayout, req);
    out[6] = offsetof(ShmLinkLayout, rsp);
    out[7] = sizeof(ShmLinkSlot);
    out[8] = offsetof(ShmLinkSlot, seq);
    out[9] = kShmLinkSlots;
    out[10] = kShmLinkMagic;
}

// xGMI self-diagnosis of this process: {device, peers with access enabled,
// other GPUs' HBM slabs imported, such imports refused, push-get launches}.
void ocm_x_xgmi_diag(uint64_t out[5]) {
    State &s = S();
    std::lock_guard<std::recursive_mutex> lk(s.mu);
    out[0] = (uint64_t)(int64_t)s.device;
    out[1] = (uint64_t)s.peers_enabled;
    out[2] = s.ipc_peer_imports;
    out[3] = s.ipc_peer_failures;
    out[4] = s.push_launches;
}

// Where extent i lives inside its owner's slab: {offset in the slab, extent
// bytes, slab bytes, owner GPU (-1: host tier)}. With ocm_x_extent_handle, a
// process on the OWNER's GPU can map the same bytes (tests: owner-side kernels).
int ocm_x_extent_region(ocm_alloc_t a, int i, uint64_t out[4]) {
    if (!a || !out || i < 0 || (size_t)i >= a->ext.size()) return -1;
    const Region &r = a->ext[(size_t)i].r;
    out[0] = r.offset;
    out[1] = r.bytes;
    out[2] = r.slab_bytes;
    out[3] = (uint64_t)(int64_t)r.owner_gpu;
    return 0;
}
// Park the resident copy service now. A device-wide synchronize
// (hipDeviceSynchronize, torch.cuda.synchronize) waits for every stream,
// including the service's persistent kernel, which otherwise leaves by itself
// after OCM_SERVICE_IDLE_US (50 us) without work; the next small op relaunches it.
// Optional: only callers that cannot afford those microseconds need it.
void ocm_x_quiesce(void) {
    State &s = S();
    std::lock_guard<std::recursive_mutex> lk(s.mu);
    service_park();
}

// The local daemon's tick control transport statistics (TickStatsWire as 16
// words: ticks, own records, latency sum / max ns, periods, period sum ns,
// start() calls, their sum / max ns, transport | ticks_per_start << 32, then the
// hop breakdown: wait sum ns, exec sum ns, deliver sum ns, deliveries, idle ticks,
// TCP wake-ups sent).
int ocm_x_tick_stats(uint64_t out[16]) {
    State &s = S();
    std::lock_guard<std::recursive_mutex> lk(s.mu);
    if (!s.inited || !out) return -1;
    Msg m = new_msg(MSG_TICK_STATS);
    Msg r;
    if (rpc(m, &r, s.cfg.rpc_timeout_ms) != 0) return -1;
    TickStatsWire st;
    std::memcpy(&st, r.u.raw, sizeof(st));
    const uint64_t v[16] = {st.ticks, st.own_records, st.lat_sum_ns, st.lat_max_ns, st.periods, st.period_sum_ns,
                            st.starts, st.start_sum_ns, st.start_max_ns,
                            (uint64_t)st.transport | ((uint64_t)st.ticks_per_start << 32),
                            st.wait_sum_ns, st.exec_sum_ns, st.deliver_sum_ns, st.deliver_n, st.lazy_ticks,
                            st.tcp_wakes};
    std::memcpy(out, v, sizeof(v));
    return 0;
}

// The local daemon's stream-placement counters (PlaceStatsWire, 16 words as laid
// out there: state | disabled << 32, sync, syncs, allocs over two hops, over rank0,
// extents allocated straight from the stream, rank0's DO_ALLOC sends, divergences,
// aborts, duplicate replies freed, extents adopted, the placing directory's digest,
// inputs applied).
int ocm_x_place_stats(uint64_t out[16]) {
    State &s = S();
    std::lock_guard<std::recursive_mutex> lk(s.mu);
    if (!s.inited || !out) return -1;
    Msg m = new_msg(MSG_PLACE_STATS);
    Msg r;
    if (rpc(m, &r, s.cfg.rpc_timeout_ms) != 0) return -1;
    static_assert(sizeof(PlaceStatsWire) == 16 * sizeof(uint64_t), "place stats are 16 words");
    std::memcpy(out, r.u.raw, sizeof(PlaceStatsWire));
    return 0;
}

// Copy-service diagnostics: {ops, ns posting requests, ns waiting for done,
// GPU ticks (100 MHz) from doorbell seen to done published, relaunches after an
// idle exit}. The doorbell record stays in host memory (a BAR-mapped HBM record
// measured slower: profiles/svc_doorbell_hbm_ab_r02.json).
void ocm_x_service_stats(uint64_t out[5]) {
    State &s = S();
    std::lock_guard<std::recursive_mutex> lk(s.mu);
    out[0] = s.svc_ops;
    out[1] = s.svc_ns_post;
    out[2] = s.svc_ns_wait;
    out[3] = s.svc_gpu_ticks_done + (s.svc ? __atomic_load_n(&s.svc->gpu_ticks, __ATOMIC_ACQUIRE) : 0);
    out[4] = s.svc_relaunches;  // instances started because the previous one left idle
}

// Copy-service health: {gang ops sized below their wanted width because fewer
// members were resident, instances that left with the posted op unfinished,
// ops abandoned after OCM_SERVICE_TIMEOUT_MS (drained, then redone by a launch),
// 1 if an instance could not be drained (service off, op failed), the smallest
// roster a gang op was sized to (0: none yet), the current instance's roster,
// relaunches after an idle exit, and the host ns they took (reap + launch), then
// over every start: ns choosing a lane, ns in the launch call, starts}.
// Then: 1 if the lanes are AQL queues of the library's own (0: HIP streams),
// gang ops that replaced a lone lead with a full instance, 1 if the running
// instance's lead is alone (its members left), and the lanes created.
// Then the longest wait for a lane to drain (ns) and where it happened
// (1 lane pick at a start, 2 park, 3 shutdown, 4 abort, 5 re-post after an exit),
// the instances dispatched beside a previous lead that had not left yet, and 1
// while an instance is resident (started and not yet left), and 1 + the XCD of
// the running instance's lead (0: unknown). Then the ops that started an instance
// and their split: host ns from the dispatch to seeing the lead's start stamp, GPU
// ticks (100 MHz) from the lead's start to its first request seen, host ns in total;
// then the library's AQL queues (lanes) and the HIP streams it created.
void ocm_x_service_health(uint64_t out[29]) {
    State &s = S();
    std::lock_guard<std::recursive_mutex> lk(s.mu);
    const bool run = s.svc && s.svc_running;
    out[0] = s.svc_degraded;
    out[1] = s.svc_incomplete_exits;
    out[2] = s.svc_aborts;
    out[3] = s.svc_wedged ? 1 : 0;
    out[4] = s.svc_roster_min == ~0ull ? 0 : s.svc_roster_min;
    out[5] = run ? service_untag(s.svc_epoch, __atomic_load_n(&s.svc->roster, __ATOMIC_ACQUIRE)) : 0;
    out[6] = s.svc_relaunches;
    out[7] = s.svc_ns_relaunch;
    out[8] = s.svc_ns_pick;
    out[9] = s.svc_ns_launch;
    out[10] = s.svc_epoch_starts;
    out[11] = s.svc_aql ? 1 : 0;
    out[12] = s.svc_promotions;
    out[13] = (run && service_untag(s.svc_epoch, __atomic_load_n(&s.svc->lone, __ATOMIC_ACQUIRE)) != 0) ? 1 : 0;
    out[14] = s.svc_drain_max_ns;
    out[15] = s.svc_drain_max_site;
    out[16] = s.svc_overlaps;
    out[17] = (run && service_untag(s.svc_epoch, __atomic_load_n(&s.svc->exited, __ATOMIC_ACQUIRE)) == 0) ? 1 : 0;
    out[18] = run ? service_untag(s.svc_epoch, __atomic_load_n(&s.svc->lead_xcd, __ATOMIC_ACQUIRE)) : 0;
    out[19] = s.svc_cold_ops;
    out[20] = s.svc_cold_ns_to_start;
    out[21] = s.svc_cold_ticks_to_seen;
    out[22] = s.svc_cold_ns_total;
    // hardware queues this process's library holds: its own AQL
    // queues, and HIP streams (HIP maps those onto at most GPU_MAX_HW_QUEUES queues)
    uint64_t aql = 0, hip = 0;
    for (const State::SvcLane &l : s.svc_lanes) (l.aql ? aql : hip)++;
    hip += s.lanes.size() + (s.stream ? 1 : 0);
    for (const auto &kv : s.push) hip += kv.second.stream ? 1 : 0;
    out[23] = aql;
    out[24] = hip;
    out[25] = s.svc_arms;   // instances pre-armed while the service was idle
    out[26] = s.svc_fires;  // starts that fired one
    out[27] = s.svc_disarms;  // armed instances cancelled at the end of OCM_SERVICE_PREARM_MS
    out[28] = s.svc_inline_starts;  // starts that carried their first (solo) request inline
}

// The copy service's cold starts one by one (the last State::kColdRing ops that had to
// start an instance), out[24]:
//   0 samples; 1-4 dispatch -> the host sees the lead's start stamp, ns: p50, p99, max,
//   and the seq of the op with that max; 5-8 the whole op (entry -> done seen), ns:
//   p50, p99, max, seq of the max; 9-10 the lead's start -> first request seen, GPU
//   ticks (100 MHz): p50, max; 11-12 ops whose start fired a pre-armed instance, and
//   their whole-op p50 (ns); 13-14 the same for starts that dispatched a new packet;
//   15-17 lane drains: count, total ns, over 1 ms; 18 the longest drain (ns) and 19 where.
// Percentiles are nearest-rank over the samples held.
void ocm_x_service_cold(uint64_t out[24]) {
    State &s = S();
    std::lock_guard<std::recursive_mutex> lk(s.mu);
    std::memset(out, 0, 24 * sizeof(uint64_t));
    const size_t n = (size_t)std::min<uint64_t>(s.svc_cold_next, State::kColdRing);
    std::vector<State::ColdSample> v(s.svc_cold_ring.begin(), s.svc_cold_ring.begin() + (long)n);
    auto pct = [](std::vector<uint64_t> &x, double q) -> uint64_t {
        if (x.empty()) return 0;
        std::sort(x.begin(), x.end());
        size_t i = (size_t)std::ceil(q * (double)x.size());
        return x[std::min(x.size(), std::max<size_t>(i, 1)) - 1];
    };
    std::vector<uint64_t> a, b, c, fired, cold;
    uint64_t amax_seq = 0, bmax_seq = 0, amax = 0, bmax = 0;
    for (const auto &x : v) {
        a.push_back(x.to_start_ns);
        b.push_back(x.total_ns);
        c.push_back(x.seen_ticks);
        (x.fired ? fired : cold).push_back(x.total_ns);
        if (x.to_start_ns >= amax) amax = x.to_start_ns, amax_seq = x.seq;
        if (x.total_ns >= bmax) bmax = x.total_ns, bmax_seq = x.seq;
    }
    out[0] = n;
    out[1] = pct(a, 0.50);
    out[2] = pct(a, 0.99);
    out[3] = amax;
    out[4] = amax_seq;
    out[5] = pct(b, 0.50);
    out[6] = pct(b, 0.99);
    out[7] = bmax;
    out[8] = bmax_seq;
    out[9] = pct(c, 0.50);
    out[10] = c.empty() ? 0 : *std::max_element(c.begin(), c.end());
    out[11] = fired.size();
    out[12] = pct(fired, 0.50);
    out[13] = cold.size();
    out[14] = pct(cold, 0.50);
    out[15] = s.svc_drains;
    out[16] = s.svc_drain_ns_total;
    out[17] = s.svc_drains_over_1ms;
    out[18] = s.svc_drain_max_ns;
    out[19] = s.svc_drain_max_site;
}

// Forget the cold-start samples and the drain counters (per-test windows).
void ocm_x_service_cold_reset(void) {
    State &s = S();
    std::lock_guard<std::recursive_mutex> lk(s.mu);
    s.svc_cold_next = 0;
    s.svc_drains = s.svc_drain_ns_total = s.svc_drains_over_1ms = 0;
    s.svc_drain_max_ns = 0;
    s.svc_drain_max_site = 0;
}

// OCM_SERVICE_PREARM at run time (A/B in one process): 0 stops arming (an instance
// armed already is cancelled by the next dispatch on its lane, ocm/aql.h), 1 resumes.
// Returns the previous setting.
int ocm_x_set_prearm(int on) {
    State &s = S();
    std::lock_guard<std::recursive_mutex> lk(s.mu);
    const int was = s.cfg.svc_prearm ? 1 : 0;
    s.cfg.svc_prearm = on != 0;
    return was;
}

// OCM_SERVICE_PREARM_MS at run time: how long an armed instance may wait for an op
// before the armer cancels it (0: until the next op). Returns the previous value (ms).
int ocm_x_set_prearm_window(int ms) {
    State &s = S();
    std::lock_guard<std::recursive_mutex> lk(s.mu);
    const int was = (int)(s.svc_arm_window_ns.load() / 1000000ull);
    s.svc_arm_window_ns.store((uint64_t)std::max(0, ms) * 1000000ull);
    return was;
}

// Copy-service phase stamps of the last request (OCM_SERVICE_PROTO with the
// TRACE bit): 4 GPU-clock words per workgroup for the first n workgroups.
int ocm_x_service_trace(uint64_t *out, int n_wgs) {
    State &s = S();
    std::lock_guard<std::recursive_mutex> lk(s.mu);
    if (!s.svc_box || n_wgs < 1 || n_wgs > kServiceTraceWgs) return -1;
    DeviceGuard g(s.device);
    if (hipMemcpy(out, s.svc_box->trace, (size_t)n_wgs * 4 * sizeof(uint64_t), hipMemcpyDeviceToHost) != hipSuccess) {
        (void)hipGetLastError();
        return -1;
    }
    return 0;
}

// Per-op stamps of the last n ops through the copy service (OCM_SERVICE_PROTO with
// the TRACE bit), oldest first, 9 words each: seq, host entry / posted / done-seen
// (now_ns), lane, flags (1: the op started an instance), gang width, and the lead's
// seen / done stamps (GPU clock, 100 MHz; 0 when the lane's ring no longer holds
// the seq). The two clocks are not aligned: tools/small_op_trace.py fits the offset.
int ocm_x_service_optrace(uint64_t *out, int n) {
    State &s = S();
    std::lock_guard<std::recursive_mutex> lk(s.mu);
    if (n < 1 || n > kServiceOpTrace || s.svc_optrace.empty()) return -1;
    DeviceGuard g(s.device);
    std::vector<std::vector<unsigned long long>> boxes(s.svc_lanes.size());
    for (size_t i = 0; i < s.svc_lanes.size(); i++) {
        if (!s.svc_lanes[i].box) continue;
        boxes[i].resize((size_t)kServiceOpTrace * 4);
        if (hipMemcpy(boxes[i].data(), s.svc_lanes[i].box->optrace, boxes[i].size() * 8, hipMemcpyDeviceToHost) !=
            hipSuccess) {
            (void)hipGetLastError();
            return -1;
        }
    }
    int rows = 0;
    const unsigned long long last = s.svc_seq;
    for (unsigned long long q = last >= (unsigned long long)n ? last - n + 1 : 1; q <= last; q++) {
        const auto &h = s.svc_optrace[q & (kServiceOpTrace - 1)];
        if (h[0] != q) continue;  // not an op through the service (or a re-posted seq)
        uint64_t *o = out + (size_t)rows * 9;
        for (int k = 0; k < 7; k++) o[k] = h[k];
        o[7] = o[8] = 0;
        const size_t lane = (size_t)h[4];
        if (lane < boxes.size() && !boxes[lane].empty()) {
            const unsigned long long *b = &boxes[lane][(size_t)(q & (kServiceOpTrace - 1)) * 4];
            if (b[0] == q) {
                o[7] = b[1];
                o[8] = b[2];
            }
        }
        rows++;
    }
    return rows;
}

// Every thread's native stack on stderr (hang diagnosis; ocm/stackdump.h). The same
// dump runs by itself when a blocking call has been in flight OCM_HANG_DUMP_S seconds.
void ocm_x_dump_stacks(const char *why) { dump_all_stacks(2, why ? why : "ocm_x_dump_stacks"); }

// A daemon embedded in this process (libocmd.so ocmd_embed_slab_ptr): HBM slabs it
// exported map to its own pointers instead of IPC imports. Null removes it.
void ocm_x_set_slab_resolver(void *fn) {
    State &s = S();
    std::lock_guard<std::recursive_mutex> lk(s.mu);
    s.slab_resolver = reinterpret_cast<void *(*)(const unsigned char *)>(fn);
}

// Host addresses behind the copy service's hand-off (diagnostics: which NUMA node
// holds them): the request record pages, the status slot, and extent 0's host
// mapping of `a` (0 where there is none).
int ocm_x_service_pages(ocm_alloc_t a, uint64_t out[3]) {
    State &s = S();
    std::lock_guard<std::recursive_mutex> lk(s.mu);
    out[0] = reinterpret_cast<uint64_t>(s.svc_rec_pages);
    out[1] = reinterpret_cast<uint64_t>(s.svc);
    out[2] = (a && !a->ext.empty()) ? reinterpret_cast<uint64_t>(a->ext[0].hptr) : 0;
    return s.svc ? 0 : -1;
}

// Transfer tuning at runtime (benchmarks): variant 0 auto / 1 reg / 2 lds,
// blocks 0 = per-path default, nt = nontemporal destination stores.
void ocm_x_set_tuning(int variant, int blocks, int nt) {
    State &s = S();
    std::lock_guard<std::recursive_mutex> lk(s.mu);
    s.tuning = tuning_of(variant, blocks, nt);
    s.dir_tuning[0] = s.dir_tuning[1] = XferTuning{};
}

// Per-direction override of one-sided kernel ops (dir 0 get, 1 put), e.g. the
// winner of an autotune over the xGMI links; variant 0 clears it.
int ocm_x_set_tuning_dir(int dir, int variant, int blocks, int nt) {
    if (dir != 0 && dir != 1) return -1;
    if (variant < XFER_AUTO || variant > XFER_PUSH || blocks < 0) return -1;
    State &s = S();
    std::lock_guard<std::recursive_mutex> lk(s.mu);
    s.dir_tuning[dir] = tuning_of(variant, blocks, nt);
    return 0;
}

// Link type (hipExtLinkType) and hop count between two devices; -1 on error.
int ocm_x_link_info(int dev, int peer, uint32_t *type, uint32_t *hops) {
    if (hipExtGetLinkTypeAndHopCount(dev, peer, type, hops) != hipSuccess) {
        (void)hipGetLastError();
        return -1;
    }
    return 0;
}

void ocm_x_layout(uint64_t out[8]) {
    out[0] = sizeof(Msg);
    out[1] = sizeof(struct ocm_params);
    out[2] = sizeof(struct ocm_alloc_params);
    out[3] = offsetof(Msg, u);
    out[4] = sizeof(Region);
    out[5] = sizeof(NodeConfig);
    out[6] = sizeof(AllocReq);
    out[7] = kHandleBytes;
}
}  // extern "C"
