// The environment, read once per ocm_init into a Config (config.h). Unset or empty
// variables leave a field at its default; no HIP runtime call here.
#include "config.h"

#include <algorithm>
#include <climits>
#include <cstdlib>
#include <cstring>

namespace ocmlib {

int env_int(const char *k, int dflt) {
    const char *v = std::getenv(k);
    return (v && *v) ? std::atoi(v) : dflt;
}

static uint64_t env_u64(const char *k, uint64_t dflt) {
    const char *v = std::getenv(k);
    return (v && *v) ? std::strtoull(v, nullptr, 0) : dflt;
}

static int env_clamped(const char *k, int dflt, int lo, int hi = INT_MAX) {
    return std::max(lo, std::min(env_int(k, dflt), hi));
}

static bool env_bool(const char *k, bool dflt) { return env_int(k, dflt ? 1 : 0) != 0; }

// A duration given in the variable's unit (us, ms), kept in the field's (`per` ticks or ns each), at least `lo`.
static uint64_t env_scaled(const char *k, uint64_t dflt, uint64_t per, int lo) {
    return per * (uint64_t)env_clamped(k, (int)(dflt / per), lo);
}

Config config_from_env() {
    Config c;
    c.rpc_timeout_ms = env_int("OCM_RPC_TIMEOUT_MS", c.rpc_timeout_ms);
    c.rpc_spin_ns = env_scaled("OCM_RPC_SPIN_US", c.rpc_spin_ns, 1000, 0);
    c.connect_timeout_ms = env_int("OCM_CONNECT_TIMEOUT_MS", c.connect_timeout_ms);
    c.shm_link = env_bool("OCM_SHM_LINK", c.shm_link);
    c.no_gpu = std::getenv("OCM_NO_GPU") != nullptr;
    c.net_streams = env_clamped("OCM_NET_STREAMS", c.net_streams, 1, 64);
    c.net_split_min = std::max<uint64_t>(4096, env_u64("OCM_NET_SPLIT_MIN", c.net_split_min));
    c.sync_mode = env_int("OCM_SYNC_MODE", c.sync_mode);
    c.n_lanes = env_int("OCM_ASYNC_LANES", c.n_lanes);
    c.pinned_keep = env_u64("OCM_PINNED_KEEP", c.pinned_keep);
    c.dev_cache_cap = env_u64("OCM_LOCAL_CACHE", c.dev_cache_cap);
    const char *he = std::getenv("OCM_HOST_ENGINE");
    c.host_engine_kernel = !(he && !std::strcmp(he, "sdma"));  // the PCIe streaming kernel unless asked for SDMA
    c.host_kernel_max = env_u64("OCM_HOST_KERNEL_MAX", c.host_engine_kernel ? c.host_kernel_max : 0);
    c.launch_flags = env_bool("OCM_LAUNCH_FLAG", c.launch_flags);
    c.launch_flag_max = env_u64("OCM_LAUNCH_FLAG_MAX", c.launch_flag_max);

    c.svc_eager = env_bool("OCM_SERVICE_EAGER", c.svc_eager);
    const char *sm = std::getenv("OCM_SERVICE_MAX");
    c.svc_max = env_u64("OCM_SERVICE_MAX", c.svc_max);
    c.svc_max_host = env_u64("OCM_SERVICE_MAX_HOST", sm && *sm ? c.svc_max : c.svc_max_host);
    c.svc_max_local = env_u64("OCM_SERVICE_MAX_LOCAL", c.svc_max_local);
    const char *q = std::getenv("OCM_SERVICE_QUEUE");
    c.svc_queue_aql = !(q && std::strcmp(q, "hip") == 0);
    c.svc_lanes_max = (unsigned)env_clamped("OCM_SERVICE_STREAMS", (int)c.svc_lanes_max, 1, 16);
    c.svc_blocks = (unsigned)env_clamped("OCM_SERVICE_BLOCKS", (int)c.svc_blocks, 1, 1024);
    c.svc_gang_host = (unsigned)env_clamped("OCM_SERVICE_GANG_HOST", (int)c.svc_gang_host, 1, 1024);
    c.svc_solo_tiles = (unsigned)env_clamped("OCM_SERVICE_SOLO_TILES", (int)c.svc_solo_tiles, 0);
    c.svc_solo_tiles_host_get = (unsigned)env_clamped("OCM_SERVICE_SOLO_TILES_HOST_GET", (int)c.svc_solo_tiles_host_get, 0);
    c.svc_proto = (unsigned)env_int("OCM_SERVICE_PROTO", (int)kServiceProtoDefault) & kServiceProtoMask;
    if (const int ps = env_int("OCM_SERVICE_POLL_SLEEP", -1); ps >= 0 && ps < 255)  // PIPE spacing, s_sleep(1) units
        c.svc_proto |= (unsigned)(ps + 1) << kServicePollSleepShift;
    if (const int pj = env_int("OCM_SERVICE_POLL_JITTER", kServicePollJitterDefault); pj > 0 && pj < 16)
        c.svc_proto |= (unsigned)pj << kServicePollJitterShift;
    c.svc_force_strict = env_bool("OCM_SERVICE_STRICT", c.svc_force_strict);
    c.svc_direct = (unsigned)env_clamped("OCM_SERVICE_DIRECT", (int)c.svc_direct, 1, 1024);
    if (c.svc_direct > (unsigned)kServiceGangCopiesMax) c.svc_proto &= ~kServiceProtoCopies;  // one page of copies
    c.svc_direct_max_host = env_u64("OCM_SERVICE_DIRECT_MAX_HOST", c.svc_direct_max_host);
    c.svc_direct_max_hbm = env_u64("OCM_SERVICE_DIRECT_MAX_HBM", c.svc_direct_max_hbm);
    c.svc_host_tile_shift_get = (unsigned)env_clamped("OCM_SERVICE_HOST_TILE_SHIFT_GET", (int)c.svc_host_tile_shift_get, 0);
    c.svc_host_tile_shift_put = (unsigned)env_clamped("OCM_SERVICE_HOST_TILE_SHIFT_PUT", (int)c.svc_host_tile_shift_put, 0);
    c.svc_host_tile_min = env_u64("OCM_SERVICE_HOST_TILE_MIN", c.svc_host_tile_min);
    c.svc_host_tile_max = env_u64("OCM_SERVICE_HOST_TILE_MAX", c.svc_host_tile_max);
    c.svc_host_get_narrow_min = env_u64("OCM_SERVICE_HOST_GET_NARROW_MIN", c.svc_host_get_narrow_min);
    c.svc_host_get_width = (unsigned)env_clamped("OCM_SERVICE_HOST_GET_WIDTH", (int)c.svc_host_get_width, 1, 1024);
    c.svc_park_kernel = env_bool("OCM_SERVICE_PARK_KERNEL", c.svc_park_kernel);
    c.svc_idle_ticks = env_scaled("OCM_SERVICE_IDLE_US", c.svc_idle_ticks, 100, 1);  // 100 MHz clock
    c.svc_degraded_idle_ticks = env_scaled("OCM_SERVICE_DEGRADED_IDLE_US", c.svc_degraded_idle_ticks, 100, 1);
    c.svc_lone_ticks = env_scaled("OCM_SERVICE_LONE_US", c.svc_lone_ticks, 100, 0);
    c.svc_roster_wait_ns = env_scaled("OCM_SERVICE_ROSTER_WAIT_US", c.svc_roster_wait_ns, 1000, 0);
    c.svc_timeout_ns = env_scaled("OCM_SERVICE_TIMEOUT_MS", c.svc_timeout_ns, 1000000, 1);
    c.svc_drain_ns = env_scaled("OCM_SERVICE_DRAIN_MS", c.svc_drain_ns, 1000000, 1);
    c.svc_box_reset_always = env_bool("OCM_SERVICE_BOX_RESET", c.svc_box_reset_always);
    c.svc_relaunch_query = env_bool("OCM_SERVICE_RELAUNCH_QUERY", c.svc_relaunch_query);
    c.svc_prearm = env_bool("OCM_SERVICE_PREARM", c.svc_prearm);
    c.svc_arm_window_ns = env_scaled("OCM_SERVICE_PREARM_MS", c.svc_arm_window_ns, 1000000, 0);
    c.svc_inline = env_bool("OCM_SERVICE_INLINE", c.svc_inline);

    c.adam_host = env_bool("OCM_ADAM_HOST", c.adam_host);
    c.adam_host_grid = env_int("OCM_ADAM_HOST_GRID", c.adam_host_grid);
    c.adam_host_vec = env_int("OCM_ADAM_HOST_VEC", c.adam_host_vec);
    c.adam_grid = env_int("OCM_ADAM_GRID", c.adam_grid);
    return c;
}

}  // namespace ocmlib
