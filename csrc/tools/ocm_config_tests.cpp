// The library's knobs as config_from_env() reads them (csrc/src/lib/config.h): the
// defaults, the clamps at both ends, the couplings between variables, and that a parse
// keeps nothing from the one before it. The expected values are written out here as
// numbers (the README's environment table and the kService* constants), not taken from
// the code under test. Stand-alone: no GPU, no daemon, nothing of HIP linked, so the
// build also makes an ASan + UBSan copy of it.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <utility>
#include <vector>

#include "config.h"

using namespace ocmlib;

namespace {

int failures = 0;

#define CHECK(cond, ...)                  \
    do {                                  \
        if (!(cond)) {                    \
            if (failures++ < 20) {        \
                std::printf("FAIL: ");    \
                std::printf(__VA_ARGS__); \
                std::printf("\n");        \
            }                             \
        }                                 \
    } while (0)

const char *const kVars[] = {
    "OCM_RPC_TIMEOUT_MS", "OCM_RPC_SPIN_US", "OCM_CONNECT_TIMEOUT_MS", "OCM_SHM_LINK", "OCM_NO_GPU", "OCM_NET_STREAMS",
    "OCM_NET_SPLIT_MIN", "OCM_SYNC_MODE", "OCM_ASYNC_LANES", "OCM_PINNED_KEEP", "OCM_LOCAL_CACHE", "OCM_HOST_ENGINE",
    "OCM_HOST_KERNEL_MAX", "OCM_LAUNCH_FLAG", "OCM_LAUNCH_FLAG_MAX", "OCM_SERVICE_EAGER", "OCM_SERVICE_MAX",
    "OCM_SERVICE_MAX_HOST", "OCM_SERVICE_MAX_LOCAL", "OCM_SERVICE_QUEUE", "OCM_SERVICE_STREAMS", "OCM_SERVICE_BLOCKS",
    "OCM_SERVICE_GANG_HOST", "OCM_SERVICE_SOLO_TILES", "OCM_SERVICE_SOLO_TILES_HOST_GET", "OCM_SERVICE_PROTO",
    "OCM_SERVICE_POLL_SLEEP", "OCM_SERVICE_POLL_JITTER", "OCM_SERVICE_STRICT", "OCM_SERVICE_DIRECT",
    "OCM_SERVICE_DIRECT_MAX_HOST", "OCM_SERVICE_DIRECT_MAX_HBM", "OCM_SERVICE_HOST_TILE_SHIFT_GET",
    "OCM_SERVICE_HOST_TILE_SHIFT_PUT", "OCM_SERVICE_HOST_TILE_MIN", "OCM_SERVICE_HOST_TILE_MAX",
    "OCM_SERVICE_HOST_GET_NARROW_MIN", "OCM_SERVICE_HOST_GET_WIDTH", "OCM_SERVICE_PARK_KERNEL", "OCM_SERVICE_IDLE_US",
    "OCM_SERVICE_DEGRADED_IDLE_US", "OCM_SERVICE_LONE_US", "OCM_SERVICE_ROSTER_WAIT_US", "OCM_SERVICE_TIMEOUT_MS",
    "OCM_SERVICE_DRAIN_MS", "OCM_SERVICE_BOX_RESET", "OCM_SERVICE_RELAUNCH_QUERY", "OCM_SERVICE_PREARM",
    "OCM_SERVICE_PREARM_MS", "OCM_SERVICE_INLINE", "OCM_ADAM_HOST", "OCM_ADAM_HOST_GRID", "OCM_ADAM_HOST_VEC",
    "OCM_ADAM_GRID"};

void clear_env() {
    for (const char *k : kVars) unsetenv(k);
}

// config_from_env() with exactly these variables set.
Config parse(std::initializer_list<std::pair<const char *, const char *>> env = {}) {
    clear_env();
    for (const auto &kv : env) setenv(kv.first, kv.second, 1);
    const Config c = config_from_env();
    clear_env();
    return c;
}

using Fields = std::vector<std::pair<const char *, uint64_t>>;

// Every field of a Config, by name.
Fields fields(const Config &c) {
#define F(x) {#x, (uint64_t)c.x}
    return {F(rpc_timeout_ms), F(rpc_spin_ns), F(connect_timeout_ms), F(shm_link), F(no_gpu), F(net_streams),
            F(net_split_min), F(sync_mode), F(n_lanes), F(pinned_keep), F(dev_cache_cap), F(host_engine_kernel),
            F(host_kernel_max), F(launch_flags), F(launch_flag_max), F(svc_eager), F(svc_max), F(svc_max_host),
            F(svc_max_local), F(svc_queue_aql), F(svc_lanes_max), F(svc_blocks), F(svc_gang_host), F(svc_solo_tiles),
            F(svc_solo_tiles_host_get), F(svc_proto), F(svc_force_strict), F(svc_direct), F(svc_direct_max_host),
            F(svc_direct_max_hbm), F(svc_host_tile_shift_get), F(svc_host_tile_shift_put), F(svc_host_tile_min),
            F(svc_host_tile_max), F(svc_host_get_narrow_min), F(svc_host_get_width), F(svc_park_kernel),
            F(svc_idle_ticks), F(svc_degraded_idle_ticks), F(svc_lone_ticks), F(svc_roster_wait_ns), F(svc_timeout_ns),
            F(svc_drain_ns), F(svc_box_reset_always), F(svc_relaunch_query), F(svc_prearm), F(svc_arm_window_ns),
            F(svc_inline), F(adam_host), F(adam_host_grid), F(adam_host_vec), F(adam_grid)};
#undef F
}

// The defaults, as numbers. svc_proto: WT | GANGREC | WCREQ | WGDONE | PIPE = 1 + 2 + 4 + 8 + 128,
// no poll spacing (bits 16-23), start jitter 3 (bits 24-27).
const Fields kDefaults = {
    {"rpc_timeout_ms", 60000}, {"rpc_spin_ns", 50000}, {"connect_timeout_ms", 10000}, {"shm_link", 1}, {"no_gpu", 0},
    {"net_streams", 4}, {"net_split_min", 1ull << 20}, {"sync_mode", 1}, {"n_lanes", 4}, {"pinned_keep", 2ull << 30},
    {"dev_cache_cap", 1ull << 30}, {"host_engine_kernel", 1}, {"host_kernel_max", 0}, {"launch_flags", 1},
    {"launch_flag_max", 4ull << 20}, {"svc_eager", 1}, {"svc_max", 4ull << 20}, {"svc_max_host", 16ull << 20},
    {"svc_max_local", 64ull << 20}, {"svc_queue_aql", 1}, {"svc_lanes_max", 4}, {"svc_blocks", 128},
    {"svc_gang_host", 32}, {"svc_solo_tiles", 2}, {"svc_solo_tiles_host_get", 1}, {"svc_proto", 143u | 3u << 24},
    {"svc_force_strict", 0}, {"svc_direct", 16}, {"svc_direct_max_host", 4ull << 20}, {"svc_direct_max_hbm", 1ull << 20},
    {"svc_host_tile_shift_get", 14}, {"svc_host_tile_shift_put", 14}, {"svc_host_tile_min", 64ull << 10},
    {"svc_host_tile_max", 256ull << 10}, {"svc_host_get_narrow_min", 1ull << 20}, {"svc_host_get_width", 12},
    {"svc_park_kernel", 0}, {"svc_idle_ticks", 100 * 50}, {"svc_degraded_idle_ticks", 100 * 5000},
    {"svc_lone_ticks", 100 * 2000}, {"svc_roster_wait_ns", 200000}, {"svc_timeout_ns", 10000000000ull},
    {"svc_drain_ns", 10000000000ull}, {"svc_box_reset_always", 0}, {"svc_relaunch_query", 0}, {"svc_prearm", 0},
    {"svc_arm_window_ns", 20000000}, {"svc_inline", 1}, {"adam_host", 1}, {"adam_host_grid", 128}, {"adam_host_vec", 4},
    {"adam_grid", 0}};

void expect_fields(const char *what, const Config &c, const Fields &want) {
    const Fields got = fields(c);
    CHECK(got.size() == want.size(), "%s: %zu fields listed, %zu expected", what, got.size(), want.size());
    for (size_t i = 0; i < got.size() && i < want.size(); i++) {
        CHECK(std::string(got[i].first) == want[i].first, "%s: field %zu is %s, expected %s", what, i, got[i].first,
              want[i].first);
        CHECK(got[i].second == want[i].second, "%s: %s = %llu, expected %llu", what, got[i].first,
              (unsigned long long)got[i].second, (unsigned long long)want[i].second);
    }
}

void test_defaults() {
    const int before = failures;
    expect_fields("nothing set", parse(), kDefaults);
    expect_fields("Config{}", Config{}, kDefaults);
    // an empty variable counts as unset
    expect_fields("empty variables",
                  parse({{"OCM_SERVICE_MAX", ""}, {"OCM_PINNED_KEEP", ""}, {"OCM_SERVICE_BLOCKS", ""}, {"OCM_ADAM_HOST", ""},
                         {"OCM_ADAM_HOST_GRID", ""}, {"OCM_ADAM_HOST_VEC", ""}, {"OCM_ADAM_GRID", ""}}),
                  kDefaults);
    if (failures == before) std::printf("PASS defaults\n");
}

void test_clamps() {
    const int before = failures;
    CHECK(parse({{"OCM_SERVICE_BLOCKS", "0"}}).svc_blocks == 1, "OCM_SERVICE_BLOCKS=0");
    CHECK(parse({{"OCM_SERVICE_BLOCKS", "5000"}}).svc_blocks == 1024, "OCM_SERVICE_BLOCKS=5000");
    CHECK(parse({{"OCM_SERVICE_BLOCKS", "64"}}).svc_blocks == 64, "OCM_SERVICE_BLOCKS=64");
    CHECK(parse({{"OCM_NET_STREAMS", "0"}}).net_streams == 1, "OCM_NET_STREAMS=0");
    CHECK(parse({{"OCM_NET_STREAMS", "100"}}).net_streams == 64, "OCM_NET_STREAMS=100");
    CHECK(parse({{"OCM_NET_SPLIT_MIN", "1"}}).net_split_min == 4096, "OCM_NET_SPLIT_MIN=1");
    CHECK(parse({{"OCM_NET_SPLIT_MIN", "0x800000"}}).net_split_min == 8ull << 20, "OCM_NET_SPLIT_MIN=0x800000");
    CHECK(parse({{"OCM_SERVICE_STREAMS", "99"}}).svc_lanes_max == 16, "OCM_SERVICE_STREAMS=99");
    CHECK(parse({{"OCM_SERVICE_STREAMS", "0"}}).svc_lanes_max == 1, "OCM_SERVICE_STREAMS=0");
    CHECK(parse({{"OCM_SERVICE_GANG_HOST", "0"}}).svc_gang_host == 1, "OCM_SERVICE_GANG_HOST=0");
    CHECK(parse({{"OCM_SERVICE_GANG_HOST", "4096"}}).svc_gang_host == 1024, "OCM_SERVICE_GANG_HOST=4096");
    CHECK(parse({{"OCM_SERVICE_HOST_GET_WIDTH", "0"}}).svc_host_get_width == 1, "OCM_SERVICE_HOST_GET_WIDTH=0");
    CHECK(parse({{"OCM_SERVICE_HOST_GET_WIDTH", "2000"}}).svc_host_get_width == 1024, "OCM_SERVICE_HOST_GET_WIDTH=2000");
    CHECK(parse({{"OCM_SERVICE_SOLO_TILES", "-3"}}).svc_solo_tiles == 0, "OCM_SERVICE_SOLO_TILES=-3");
    CHECK(parse({{"OCM_SERVICE_HOST_TILE_SHIFT_GET", "-1"}}).svc_host_tile_shift_get == 0, "HOST_TILE_SHIFT_GET=-1");
    // the unit conversions and their floors: us -> 100 MHz ticks, us / ms -> ns
    CHECK(parse({{"OCM_SERVICE_IDLE_US", "0"}}).svc_idle_ticks == 100, "OCM_SERVICE_IDLE_US=0");
    CHECK(parse({{"OCM_SERVICE_IDLE_US", "7"}}).svc_idle_ticks == 700, "OCM_SERVICE_IDLE_US=7");
    CHECK(parse({{"OCM_SERVICE_DEGRADED_IDLE_US", "0"}}).svc_degraded_idle_ticks == 100, "DEGRADED_IDLE_US=0");
    CHECK(parse({{"OCM_SERVICE_LONE_US", "-5"}}).svc_lone_ticks == 0, "OCM_SERVICE_LONE_US=-5");
    CHECK(parse({{"OCM_SERVICE_LONE_US", "30"}}).svc_lone_ticks == 3000, "OCM_SERVICE_LONE_US=30");
    CHECK(parse({{"OCM_SERVICE_ROSTER_WAIT_US", "-1"}}).svc_roster_wait_ns == 0, "OCM_SERVICE_ROSTER_WAIT_US=-1");
    CHECK(parse({{"OCM_SERVICE_ROSTER_WAIT_US", "5"}}).svc_roster_wait_ns == 5000, "OCM_SERVICE_ROSTER_WAIT_US=5");
    CHECK(parse({{"OCM_SERVICE_TIMEOUT_MS", "0"}}).svc_timeout_ns == 1000000, "OCM_SERVICE_TIMEOUT_MS=0");
    CHECK(parse({{"OCM_SERVICE_DRAIN_MS", "250"}}).svc_drain_ns == 250000000, "OCM_SERVICE_DRAIN_MS=250");
    CHECK(parse({{"OCM_SERVICE_PREARM_MS", "-2"}}).svc_arm_window_ns == 0, "OCM_SERVICE_PREARM_MS=-2");
    CHECK(parse({{"OCM_SERVICE_PREARM_MS", "3"}}).svc_arm_window_ns == 3000000, "OCM_SERVICE_PREARM_MS=3");
    CHECK(parse({{"OCM_RPC_SPIN_US", "-1"}}).rpc_spin_ns == 0, "OCM_RPC_SPIN_US=-1");
    CHECK(parse({{"OCM_RPC_SPIN_US", "9"}}).rpc_spin_ns == 9000, "OCM_RPC_SPIN_US=9");
    if (failures == before) std::printf("PASS clamps\n");
}

void test_couplings() {
    const int before = failures;
    // OCM_SERVICE_MAX_HOST follows an explicit OCM_SERVICE_MAX, unless it is set itself
    Config c = parse({{"OCM_SERVICE_MAX", "65536"}});
    CHECK(c.svc_max == 65536 && c.svc_max_host == 65536, "OCM_SERVICE_MAX=65536: host %llu", (unsigned long long)c.svc_max_host);
    c = parse({{"OCM_SERVICE_MAX", "0"}});
    CHECK(c.svc_max == 0 && c.svc_max_host == 0, "OCM_SERVICE_MAX=0: host %llu", (unsigned long long)c.svc_max_host);
    c = parse({{"OCM_SERVICE_MAX", "65536"}, {"OCM_SERVICE_MAX_HOST", "131072"}});
    CHECK(c.svc_max == 65536 && c.svc_max_host == 131072, "both set: host %llu", (unsigned long long)c.svc_max_host);
    c = parse({{"OCM_SERVICE_MAX_HOST", "131072"}});
    CHECK(c.svc_max == 4ull << 20 && c.svc_max_host == 131072, "OCM_SERVICE_MAX_HOST alone: max %llu", (unsigned long long)c.svc_max);
    // the poll spacing is stored + 1 in bits 16-23 (0..254), the jitter in bits 24-27 (1..15; 0 and 16 up: none)
    const unsigned base = 143u, jit3 = 3u << 24;
    CHECK(parse({{"OCM_SERVICE_POLL_SLEEP", "0"}}).svc_proto == (base | 1u << 16 | jit3), "OCM_SERVICE_POLL_SLEEP=0");
    CHECK(parse({{"OCM_SERVICE_POLL_SLEEP", "254"}}).svc_proto == (base | 255u << 16 | jit3), "OCM_SERVICE_POLL_SLEEP=254");
    CHECK(parse({{"OCM_SERVICE_POLL_SLEEP", "255"}}).svc_proto == (base | jit3), "OCM_SERVICE_POLL_SLEEP=255");
    CHECK(parse({{"OCM_SERVICE_POLL_JITTER", "0"}}).svc_proto == base, "OCM_SERVICE_POLL_JITTER=0");
    CHECK(parse({{"OCM_SERVICE_POLL_JITTER", "15"}}).svc_proto == (base | 15u << 24), "OCM_SERVICE_POLL_JITTER=15");
    CHECK(parse({{"OCM_SERVICE_POLL_JITTER", "16"}}).svc_proto == base, "OCM_SERVICE_POLL_JITTER=16");
    // OCM_SERVICE_PROTO keeps its low 8 bits; COPIES (64) survives up to 32 direct pollers (one page of 128-byte copies)
    CHECK(parse({{"OCM_SERVICE_PROTO", "511"}}).svc_proto == (255u | jit3), "OCM_SERVICE_PROTO=511");
    c = parse({{"OCM_SERVICE_PROTO", "207"}, {"OCM_SERVICE_DIRECT", "32"}});
    CHECK(c.svc_direct == 32 && c.svc_proto == (207u | jit3), "OCM_SERVICE_DIRECT=32: proto %u", c.svc_proto);
    c = parse({{"OCM_SERVICE_PROTO", "207"}, {"OCM_SERVICE_DIRECT", "33"}});
    CHECK(c.svc_direct == 33 && c.svc_proto == (143u | jit3), "OCM_SERVICE_DIRECT=33: proto %u", c.svc_proto);
    // OCM_HOST_ENGINE=sdma zeroes the kernel max; OCM_HOST_KERNEL_MAX then overrides it
    c = parse({{"OCM_HOST_ENGINE", "sdma"}});
    CHECK(!c.host_engine_kernel && c.host_kernel_max == 0, "sdma: kernel max %llu", (unsigned long long)c.host_kernel_max);
    c = parse({{"OCM_HOST_ENGINE", "sdma"}, {"OCM_HOST_KERNEL_MAX", "1048576"}});
    CHECK(!c.host_engine_kernel && c.host_kernel_max == 1048576, "sdma + max: %llu", (unsigned long long)c.host_kernel_max);
    c = parse({{"OCM_HOST_ENGINE", "kernel"}, {"OCM_HOST_KERNEL_MAX", "4096"}});
    CHECK(c.host_engine_kernel && c.host_kernel_max == 4096, "kernel + max: %llu", (unsigned long long)c.host_kernel_max);
    // OCM_SERVICE_QUEUE: only "hip" leaves the AQL queues
    CHECK(!parse({{"OCM_SERVICE_QUEUE", "hip"}}).svc_queue_aql, "OCM_SERVICE_QUEUE=hip");
    CHECK(parse({{"OCM_SERVICE_QUEUE", "aql"}}).svc_queue_aql, "OCM_SERVICE_QUEUE=aql");
    CHECK(parse({{"OCM_SERVICE_QUEUE", "other"}}).svc_queue_aql, "OCM_SERVICE_QUEUE=other");
    CHECK(parse({{"OCM_NO_GPU", ""}}).no_gpu, "OCM_NO_GPU set and empty");
    if (failures == before) std::printf("PASS couplings\n");
}

// The knobs an earlier init used to leave behind: set to something else, parsed, unset, parsed again.
void test_determinism() {
    const int before = failures;
    const Config c = parse({{"OCM_SERVICE_MAX_LOCAL", "1"}, {"OCM_SERVICE_DIRECT_MAX_HOST", "2"},
                            {"OCM_SERVICE_DIRECT_MAX_HBM", "3"}, {"OCM_SERVICE_HOST_TILE_MIN", "4"},
                            {"OCM_SERVICE_HOST_TILE_MAX", "5"}, {"OCM_SERVICE_HOST_GET_NARROW_MIN", "6"},
                            {"OCM_PINNED_KEEP", "7"}, {"OCM_LOCAL_CACHE", "8"}, {"OCM_NET_SPLIT_MIN", "8192"},
                            {"OCM_HOST_KERNEL_MAX", "10"}, {"OCM_SERVICE_GANG_HOST", "11"},
                            {"OCM_SERVICE_HOST_TILE_SHIFT_GET", "12"}, {"OCM_SERVICE_HOST_TILE_SHIFT_PUT", "13"},
                            {"OCM_SERVICE_QUEUE", "hip"}});
    CHECK(c.svc_max_local == 1 && c.svc_direct_max_host == 2 && c.svc_direct_max_hbm == 3 && c.svc_host_tile_min == 4 &&
              c.svc_host_tile_max == 5 && c.svc_host_get_narrow_min == 6 && c.pinned_keep == 7 && c.dev_cache_cap == 8 &&
              c.net_split_min == 8192 && c.host_kernel_max == 10 && c.svc_gang_host == 11 &&
              c.svc_host_tile_shift_get == 12 && c.svc_host_tile_shift_put == 13 && !c.svc_queue_aql,
          "the variables set were not all taken");
    expect_fields("after unsetting them", parse(), kDefaults);
    // the fused Adam knobs, which the launcher used to read once per process
    Config d = parse({{"OCM_ADAM_HOST", "0"}, {"OCM_ADAM_HOST_GRID", "64"}, {"OCM_ADAM_HOST_VEC", "8"}, {"OCM_ADAM_GRID", "7"}});
    CHECK(!d.adam_host && d.adam_host_grid == 64 && d.adam_host_vec == 8 && d.adam_grid == 7, "OCM_ADAM_*: first parse");
    d = parse({{"OCM_ADAM_HOST", "1"}, {"OCM_ADAM_HOST_GRID", "0"}, {"OCM_ADAM_HOST_VEC", "2"}});
    CHECK(d.adam_host && d.adam_host_grid == 0 && d.adam_host_vec == 2 && d.adam_grid == 0, "OCM_ADAM_*: second parse");
    if (failures == before) std::printf("PASS determinism\n");
}

}  // namespace

int main() {
    test_defaults();
    test_clamps();
    test_couplings();
    test_determinism();
    std::printf("%d failure(s)\n", failures);
    return failures ? 1 : 0;
}
