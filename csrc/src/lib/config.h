// libocm's knobs: everything ocm_init takes from the environment, parsed in one place
// (config.cpp: no HIP runtime call, so it links and is tested without a GPU or a daemon;
// csrc/tools/ocm_config_tests.cpp). Every default is written once, at its field.
#pragma once
#include <cstdint>

#include "ocm/xfer.h"

struct lib_alloc;

namespace ocmlib {
using namespace ocm;
#pragma GCC visibility push(hidden)

// Resident copy service defaults (OCM_SERVICE_MAX / _BLOCKS / _SOLO_TILES).
// Measured (profiles/svc_probe_r01.json): a 32-workgroup gang beats a kernel
// launch + sync (13.7-14.9 us) up to 4 MiB on HBM pairs: 8.8 us at 128 KiB-1 MiB,
// 11.8 us at 4 MiB; requests of <= 2 tiles (64 KiB) stay on workgroup 0 (4.6 us at 4 KiB).
constexpr uint64_t kServiceMaxDefault = 4ull << 20;
// Pairs whose remote half is all host tier: the gang stays ahead of the DMA
// engines up to 16 MiB (8 MiB 152/155 us against 164/164, 16 MiB 300/303 against
// 312/312 put/get; profiles/svc_max_ab_r02.json). OCM_SERVICE_MAX_HOST.
constexpr uint64_t kServiceMaxHostDefault = 16ull << 20;
// 128 workgroups: with the direct gang record only 16 of them poll host memory,
// so the width costs small ops nothing, and HBM gangs of 4-64 MiB run 1.5-7 us
// faster than 32 (or a launch); host-tier gangs stay at 32, since wider ones
// lose at 8-16 MiB (188 vs 153 us; profiles/svc_blocks_r02.json).
constexpr int kServiceBlocksDefault = 128;
constexpr unsigned kServiceGangHostDefault = 32;
// Pairs wholly in this GPU's HBM keep blocking ops up to 64 MiB on the service
// (64 MiB: 23.5-24 vs 30.5 us for launch + completion); peer HBM over xGMI
// keeps kServiceMaxDefault, above which the autotuned launches take over.
constexpr uint64_t kServiceMaxLocalDefault = 64ull << 20;
constexpr int kServiceSoloTilesDefault = 2;
constexpr int kServiceIdleUsDefault = 50;
constexpr int kServiceLoneUsDefault = 2000;
// Write-through hand-offs, the records in write-combined memory, and gang
// requests polled directly by the first 16 workgroups: small ops -0.1/-0.2 us,
// host-tier 128 KiB-4 MiB and HBM 256 KiB-1 MiB gangs 1-1.5 us faster than the
// relay (profiles/svc_direct_gang_ab_r02.json, svc_direct_hybrid_r02.json).
// Round 3: gangs complete through per-workgroup done words (WGDONE) instead of a
// device-scope counter: host-tier 64-128 KiB ops 0.2-0.3 us faster, 256 KiB-4 MiB
// 0.1 us, small ops unchanged (profiles/svc_wgdone_ab_r03.json).
// Round 5: the lead keeps 8 polls in flight (PIPE). With one poll per PCIe round
// trip, every process fell into a slow mode after a fresh instance (4 KiB get
// 6.6-6.8 us vs 5.6-5.8 hot, 25 of 25 rows per 5 processes); per-op stamps put all
// of the +1.15 us between the host's post and the lead seeing it, none in the copy
// or the way back. PIPE: 5.8-6.1 (+0.27 us) after quiesce, hot rows unchanged
// (profiles/small_op_modes_r05a.json, small_op_trace_r05a.json).
constexpr unsigned kServiceProtoDefault =
    kServiceProtoWT | kServiceProtoGangRec | kServiceProtoWCReq | kServiceProtoWgDone | kServiceProtoPipe;
// PIPE start jitter (a mask of s_sleep(1) units; 0 = off): after a quiesce, 4 KiB gets
// 5.82-6.02 us with 3 against 6.07-6.39 without, hot 5.7-5.9 (profiles/small_op_modes_jitter_r05n.json)
constexpr int kServicePollJitterDefault = 3;
constexpr int kServiceDirectDefault = 16;
// Direct gangs (at most kServiceDirectDefault workgroups) for ops up to these
// sizes; wider relayed gangs above, where 16 workgroups copy too slowly
// (host-tier 16 MiB get 310-320 vs 302 us; HBM 4 MiB 10.9 vs 9.1 us).
constexpr uint64_t kServiceDirectMaxHost = 4ull << 20;
constexpr uint64_t kServiceDirectMaxHbm = 1ull << 20;
// Kernel-published completion of blocking launches (XferDone) up to this size.
// Measured on HBM pairs (profiles/launch_flag_r01.json): 9.1-13.4 us against
// 13.0-14.6 us with the runtime event up to 4 MiB; above that the per-workgroup
// system-scope writeback costs more than it saves (16 MiB: 30.9 against 15.8 us).
constexpr uint64_t kLaunchFlagMaxDefault = 4ull << 20;

struct Config {
    int rpc_timeout_ms = 60000;        // OCM_RPC_TIMEOUT_MS
    uint64_t rpc_spin_ns = 50 * 1000;  // OCM_RPC_SPIN_US: poll for a reply this long before sleeping
    int connect_timeout_ms = 10000;    // OCM_CONNECT_TIMEOUT_MS
    bool shm_link = true;              // OCM_SHM_LINK=0: the mailbox alone
    bool no_gpu = false;               // OCM_NO_GPU set (to anything): the library asks HIP for no device
    // network tier
    int net_streams = 4;                  // OCM_NET_STREAMS: parallel connections per owner (1..64)
    uint64_t net_split_min = 1ull << 20;  // OCM_NET_SPLIT_MIN: smallest part worth its own stream (>= 4 KiB)
    int sync_mode = 1;                    // OCM_SYNC_MODE: 0 stream sync, 1 spin on an event, 2 blocking event sync
    int n_lanes = 4;                      // OCM_ASYNC_LANES
    uint64_t pinned_keep = 2ull << 30;    // OCM_PINNED_KEEP: idle pinned chunks kept for reuse
    uint64_t dev_cache_cap = 1ull << 30;  // OCM_LOCAL_CACHE: freed pool blocks kept for an exact-size reuse (0 = off)
    // Host-tier pairs: the PCIe streaming kernel (default), or with OCM_HOST_ENGINE=sdma
    // the runtime's copy engines above host_kernel_max (the measured baseline).
    bool host_engine_kernel = true;
    uint64_t host_kernel_max = 0;  // OCM_HOST_KERNEL_MAX
    bool launch_flags = true;      // OCM_LAUNCH_FLAG=0 waits on the runtime event instead (cleared when the flags cannot be allocated)
    uint64_t launch_flag_max = kLaunchFlagMaxDefault;  // OCM_LAUNCH_FLAG_MAX

    // ---- persistent copy service (small blocking one-sided ops)
    bool svc_eager = true;                           // OCM_SERVICE_EAGER: set it up at ocm_init
    uint64_t svc_max = kServiceMaxDefault;           // 0: the service is off (or failed)
    uint64_t svc_max_host = kServiceMaxHostDefault;  // the same bound for host-tier-only pairs (unset: an explicit OCM_SERVICE_MAX)
    uint64_t svc_max_local = kServiceMaxLocalDefault;  // ... for pairs wholly in this GPU's HBM (OCM_SERVICE_MAX_LOCAL)
    uint64_t svc_limit(const lib_alloc *a) const;  // largest blocking op the service takes for this pair (internal.h)
    // OCM_SERVICE_QUEUE=aql (default): lanes are AQL queues when the embedded code
    // object loads (State::svc_aql), =hip: HIP streams.
    bool svc_queue_aql = true;
    unsigned svc_lanes_max = 4;                          // OCM_SERVICE_STREAMS (1..16)
    unsigned svc_blocks = kServiceBlocksDefault;         // gang size (OCM_SERVICE_BLOCKS, 1..1024)
    unsigned svc_gang_host = kServiceGangHostDefault;    // widest gang for host-tier ops (OCM_SERVICE_GANG_HOST)
    unsigned svc_solo_tiles = kServiceSoloTilesDefault;  // requests of <= this many tiles stay on workgroup 0
    unsigned svc_solo_tiles_host_get = 1;  // ... for gets from the host tier (OCM_SERVICE_SOLO_TILES_HOST_GET)
    // Hand-off protocol bits (OCM_SERVICE_PROTO) with the PIPE spacing (OCM_SERVICE_POLL_SLEEP,
    // 0..254 s_sleep(1) units, stored + 1) and start jitter (OCM_SERVICE_POLL_JITTER, 1..15) packed in.
    unsigned svc_proto = kServiceProtoDefault | (unsigned)kServicePollJitterDefault << kServicePollJitterShift;
    // OCM_SERVICE_STRICT=1 (measurements, tests): every request takes the STRICT
    // (peer-HBM) hand-off, so its cost shows on a one-GPU box
    bool svc_force_strict = false;
    unsigned svc_direct = kServiceDirectDefault;           // GANGREC direct pollers (OCM_SERVICE_DIRECT; above kServiceGangCopiesMax: no COPIES)
    uint64_t svc_direct_max_host = kServiceDirectMaxHost;  // OCM_SERVICE_DIRECT_MAX_HOST
    uint64_t svc_direct_max_hbm = kServiceDirectMaxHbm;    // OCM_SERVICE_DIRECT_MAX_HBM
    // Smaller tiles for host-tier ops of svc_host_tile_min..max bytes (0: the 32 KiB
    // default), so a direct gang spreads them over more CUs' miss queues. Gets use
    // 16 KiB tiles there: 64/128/256 KiB 6.9/7.75/9.86 vs 7.6/8.3/10.4 us; 8 and 4 KiB
    // tiles lose, and so do puts and a 32 KiB get as a gang of two
    // (profiles/svc_host_tile_ab_r02.json). Puts take 16 KiB tiles there too since round 4:
    // with WGDONE completion and the roster a 64 KiB put as a gang of four beats it solo,
    // 64/128/256 KiB 6.2-6.4/6.9-7.3/9.2-9.3 vs 7.5-7.6/7.2-7.5/9.6-9.7 us in six interleaved
    // runs (profiles/host_mid_ab_r04p.json, profiles/host_put_ab_r04q.json).
    unsigned svc_host_tile_shift_get = 14, svc_host_tile_shift_put = 14;  // OCM_SERVICE_HOST_TILE_SHIFT_GET/_PUT
    uint64_t svc_host_tile_min = 64ull << 10;                             // OCM_SERVICE_HOST_TILE_MIN
    uint64_t svc_host_tile_max = 256ull << 10;                            // OCM_SERVICE_HOST_TILE_MAX
    // Host-tier gets of at least svc_host_get_narrow_min bytes go to at most
    // svc_host_get_width members: fewer reads in flight over PCIe end closer together.
    // 1/2/4 MiB gets 24.5-24.6/43.3/79.9 us with 12 members against 25.8-26.1/44.7-45.1/
    // 81.8-82.1 with 16; 512 KiB keeps 16 (14.9-15.0 against 15.2-15.4 with 12), and 8 or
    // 4 members lose (profiles/host_wide_ab_r04q.json).
    uint64_t svc_host_get_narrow_min = 1ull << 20;  // OCM_SERVICE_HOST_GET_NARROW_MIN
    unsigned svc_host_get_width = 12;               // OCM_SERVICE_HOST_GET_WIDTH (1..1024)
    bool svc_park_kernel = false;  // park the service during kernel transfers above svc_max (OCM_SERVICE_PARK_KERNEL)
    // Idle exit after OCM_SERVICE_IDLE_US (50 us; 100 MHz ticks): long enough to
    // stay resident through a burst of blocking ops, short enough that a
    // device-wide synchronize right after one (torch.cuda.synchronize) does not
    // wait long for the persistent kernel to leave.
    uint64_t svc_idle_ticks = 100ull * kServiceIdleUsDefault;
    uint64_t svc_degraded_idle_ticks = 100ull * 5000;  // OCM_SERVICE_DEGRADED_IDLE_US (5 ms)
    // Lone lead (ocm/xfer.h): the lead stays resident alone this long after the
    // members left (OCM_SERVICE_LONE_US; AQL lanes only, 100 MHz ticks). 2 ms: a
    // 4 KiB op after a 1 ms pause stays hot (6.4-6.8 us against 17 us through a
    // relaunch), while any resident workgroup delays a full-GPU GEMM launched
    // meanwhile by ~45% (bf16 8192^3: 0.93 -> 1.38 ms: the CU it holds runs its
    // tile late), so the window stays short (profiles/lone_sweep_r04.json).
    uint64_t svc_lone_ticks = 100ull * kServiceLoneUsDefault;
    // Roster (ocm/xfer.h): gangs are sized to the members already running. Right
    // after a launch a gang op waits up to svc_roster_wait_ns for the grid to check
    // in before it settles for fewer members (OCM_SERVICE_ROSTER_WAIT_US).
    uint64_t svc_roster_wait_ns = 200 * 1000ull;
    uint64_t svc_timeout_ns = 10000 * 1000000ull;  // OCM_SERVICE_TIMEOUT_MS
    uint64_t svc_drain_ns = 10000 * 1000000ull;    // OCM_SERVICE_DRAIN_MS: bound on the STOP drain after a timeout
    // A lane's gang box is zeroed only when it must be (ocm/xfer.h): at its first
    // launch, after an instance left a request unfinished, or always with
    // OCM_SERVICE_BOX_RESET=1. Otherwise the next instance's check-in tickets start
    // at the lane's `checkins` (every workgroup of every earlier instance took one).
    bool svc_box_reset_always = false;
    bool svc_relaunch_query = false;  // OCM_SERVICE_RELAUNCH_QUERY=1: always ask the runtime which lane drained
    // OCM_SERVICE_PREARM (round 5): once the service has been idle past its idle and lone
    // windows (the instance has left), a helper thread pre-arms the next instance on the
    // lane (ocm/aql.h aql_arm) and the next start fires it. Armed only while idle: a
    // barrier packet armed beside a running instance cost host-tier 64 KiB-1 MiB gets
    // 2.5-3 % (profiles/bench_n1_arm*_r05g.json), the packet processor polling its gate.
    // Round 6: that polling taxes the process's OTHER queues too, for as long as the
    // instance stays armed: a one-element kernel replayed in a HIP graph 1.55 -> 2.9 us,
    // a launch + sync +1.4 us, the control plane's tick hop p50 +2.5 us, whatever the
    // queue's priority (profiles/arm_launch_r06*.json, ctrl_noarm_r06l.json). Off by
    // default since; when on, the armer cancels an instance still armed
    // OCM_SERVICE_PREARM_MS after it was armed (State::svc_arm_window_ns starts from
    // svc_arm_window_ns here, 0: never). ocm_x_set_prearm writes svc_prearm under the lock.
    bool svc_prearm = false;
    uint64_t svc_arm_window_ns = 20 * 1000000ull;
    bool svc_inline = true;  // OCM_SERVICE_INLINE: a cold start carries its solo request in the kernel arguments

    // ---- fused Adam (ocm/optim.h: adam_launch_shape takes these as AdamKnobs)
    // Host-tier state in one extent, every offset within 4 GiB of its base: the PCIe
    // variant of the kernel (OCM_ADAM_HOST=0 keeps the generic one).
    bool adam_host = true;
    // 128 workgroups: 91 GiB/s of state (both directions of the link at once) against
    // 82 for the HBM-tuned full-chip grid; 64-160 are equal, 192 and up lose
    // (profiles/adam_host_probe_r03.json). OCM_ADAM_HOST_GRID; 0: the HBM grid rule.
    int adam_host_grid = 128;
    // Vectors in flight per lane of the fp32 PCIe variant (OCM_ADAM_HOST_VEC: 2, 8, anything
    // else 4). On HBM state, 4 vectors per lane and 2 workgroups per CU are the fastest
    // (1.40 ms for 256 Mi params; 8 vectors per lane is 4x slower: profiles/optim_offload_r01.json
    // "adam_kernel_sweep"), and the generic variant is built with those alone.
    int adam_host_vec = 4;
    int adam_grid = 0;  // OCM_ADAM_GRID > 0: this many workgroups per tensor on every variant (measurements)
};

// The configuration the environment asks for: a pure function of it, so a second
// ocm_init in a process carries nothing over from the first.
Config config_from_env();
int env_int(const char *k, int dflt);

#pragma GCC visibility pop
}  // namespace ocmlib
