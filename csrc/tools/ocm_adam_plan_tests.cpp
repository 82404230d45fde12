// The fused Adam launch shape (ocm/optim.h: adam_launch_shape): grid, kernel variant,
// host span and vectors per lane for lists of tensors, where the state lives and the knobs;
// and the state space the optimizer kernels share (ocm/state_space.h): the launch-time check
// at its edges and the address arithmetic against its plain definition.
// The expected values are written out here as numbers, worked out with the arithmetic the
// launcher used before this function existed, not taken from the code under test.
// Stand-alone: it sees the HIP headers through ocm/optim.h and links nothing of HIP, so
// the build also makes an ASan + UBSan copy of it.
#include <cstdio>
#include <random>
#include <set>
#include <utility>
#include <vector>

#include "ocm/optim.h"

using namespace ocm;

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

constexpr int kCus = 256;
constexpr AdamKnobs kDefault{true, 128, 4, 0};
constexpr uint64_t k4G = 1ull << 32;

AdamTensor tensor(uint64_t n, uint64_t m_off, uint64_t v_off, uint64_t w_off = 0) {
    return AdamTensor{nullptr, nullptr, n, w_off, m_off, v_off};
}

// `big` elements and then k tensors of `small`, exp_avg and exp_avg_sq of each back to back.
std::vector<AdamTensor> mix(uint64_t big, uint64_t small, int k) {
    std::vector<AdamTensor> ts;
    uint64_t off = 0;
    for (int i = 0; i <= k; i++) {
        const uint64_t n = i ? small : big;
        ts.push_back(tensor(n, off, off + 4 * n));
        off += 8 * n;
    }
    return ts;
}

struct Where {
    bool bf16, host_state;
    uint32_t n_ext = 1;
    int cus = kCus;
};

void expect(const char *what, const std::vector<AdamTensor> &ts, Where w, const AdamKnobs &k, uint32_t gx, bool host,
            uint64_t span, int kV) {
    const AdamShape s = adam_launch_shape(ts.data(), (uint32_t)ts.size(), w.bf16, w.host_state, w.n_ext, w.cus, k);
    CHECK(s.gx == gx && s.host == host && s.span == span && s.kV == kV,
          "%s: gx %u host %d span %llu kV %d, expected %u %d %llu %d", what, s.gx, (int)s.host,
          (unsigned long long)s.span, s.kV, gx, (int)host, (unsigned long long)span, kV);
}

const Where kHbm{false, false}, kHost{false, true};
const std::vector<AdamTensor> kOne26 = {tensor(1ull << 26, 0, 1ull << 28)};             // fp32, 2^26 elements
const std::vector<AdamTensor> kOne26W = {tensor(1ull << 26, 0, 1ull << 28, 1ull << 29)};  // with a master array

void test_one_tensor() {
    const int before = failures;
    // the grids the single-tensor launcher gave: 2 workgroups per CU, 128 on host state, capped by the work
    expect("2^28 hbm", {tensor(1ull << 28, 0, 1ull << 30)}, kHbm, kDefault, 512, false, 1ull << 31, 4);
    expect("2^26 host", kOne26, kHost, kDefault, 128, true, (1ull << 28) + (1ull << 28), 4);
    expect("2^26 bf16 host", kOne26W, {true, true}, kDefault, 128, true, (1ull << 29) + (1ull << 28), 4);
    expect("n = 3 (nvec = 0)", {tensor(3, 0, 16)}, kHbm, kDefault, 1, false, 16, 4);
    expect("n = 3 host", {tensor(3, 0, 16)}, kHost, kDefault, 1, true, 16, 4);
    expect("n = 5", {tensor(5, 0, 32)}, kHbm, kDefault, 1, false, 48, 4);
    expect("n = 5 host", {tensor(5, 0, 32)}, kHost, kDefault, 1, true, 48, 4);
    expect("n = 1027 host", {tensor(1027, 0, 8192)}, kHost, kDefault, 1, true, 12288, 4);
    // nothing to do: no workgroups
    expect("n = 0", {tensor(0, 0, 0)}, kHbm, kDefault, 0, false, 0, 4);
    expect("no tensors", {}, kHbm, kDefault, 0, false, 0, 4);
    if (failures == before) std::printf("PASS one_tensor\n");
}

void test_lists() {
    const int before = failures;
    expect("32 x 4096 hbm", mix(4096, 4096, 31), kHbm, kDefault, 1, false, 1048576, 4);   // want 1, cap 16
    expect("32 x 4096 host", mix(4096, 4096, 31), kHost, kDefault, 1, true, 1048576, 4);
    // want = 256, cap = 497; host: 128 * 2^20 / (2^20 + 31 * 1024) + 0.999 = 125.3
    expect("2^20 + 31 x 1024 hbm", mix(1 << 20, 1024, 31), kHbm, kDefault, 256, false, 8642560, 4);
    expect("2^20 + 31 x 1024 host", mix(1 << 20, 1024, 31), kHost, kDefault, 125, true, 8642560, 4);
    // want = 4096; cap = 512 * 0.9981 + 0.999 = 512.03, host 128 * 0.9981 + 0.999 = 128.8
    expect("2^24 + 31 x 1024 hbm", mix(1 << 24, 1024, 31), kHbm, kDefault, 512, false, 134471680, 4);
    expect("2^24 + 31 x 1024 host", mix(1 << 24, 1024, 31), kHost, kDefault, 128, true, 134471680, 4);
    expect("2^24 + 31 x 1024 hbm, 304 CUs", mix(1 << 24, 1024, 31), {false, false, 1, 304}, kDefault, 607, false,
           134471680, 4);
    // equal tensors split the grid evenly
    expect("2 x 2^24 hbm", mix(1 << 24, 1 << 24, 1), kHbm, kDefault, 256, false, 268435456, 4);
    expect("2 x 2^24 host", mix(1 << 24, 1 << 24, 1), kHost, kDefault, 64, true, 268435456, 4);
    expect("an empty tensor beside n = 5", {tensor(0, 0, 0), tensor(5, 64, 128)}, kHbm, kDefault, 1, false, 144, 4);
    if (failures == before) std::printf("PASS lists\n");
}

void test_host_variant() {
    const int before = failures;
    // the span reaches exactly 2^32: generic; one vector less: host
    expect("span 2^32", {tensor(1024, 0, k4G - 4096)}, kHost, kDefault, 1, false, k4G, 4);
    expect("span 2^32 - 16", {tensor(1020, 0, k4G - 4096)}, kHost, kDefault, 1, true, k4G - 16, 4);
    // bf16: the master array alone pushes the span past 2^32; the same offsets as fp32 do not count it
    expect("bf16 w_off", {tensor(1024, 0, 4096, k4G - 4096)}, {true, true}, kDefault, 1, false, k4G, 4);
    expect("fp32 ignores w_off", {tensor(1024, 0, 4096, k4G - 4096)}, kHost, kDefault, 1, true, 8192, 4);
    // a tail-only tensor (n < 4) adds no bytes to the span; one vector does
    expect("tail-only at 2^32 - 16", {tensor(4096, 0, 16384), tensor(3, k4G - 16, 64)}, kHost, kDefault, 1, true,
           k4G - 16, 4);
    expect("one vector at 2^32 - 16", {tensor(4096, 0, 16384), tensor(4, k4G - 16, 64)}, kHost, kDefault, 1, false, k4G,
           4);
    expect("two extents", kOne26, {false, true, 2}, kDefault, 512, false, 1ull << 29, 4);
    expect("HBM state", kOne26, kHbm, kDefault, 512, false, 1ull << 29, 4);
    if (failures == before) std::printf("PASS host_variant\n");
}

void test_knobs() {
    const int before = failures;
    expect("OCM_ADAM_HOST=0", kOne26, kHost, {false, 128, 4, 0}, 512, false, 1ull << 29, 4);
    expect("OCM_ADAM_GRID=7 hbm", kOne26, kHbm, {true, 128, 4, 7}, 7, false, 1ull << 29, 4);
    expect("OCM_ADAM_GRID=7 host", kOne26, kHost, {true, 128, 4, 7}, 7, true, 1ull << 29, 4);
    expect("OCM_ADAM_HOST_GRID=64", kOne26, kHost, {true, 64, 4, 0}, 64, true, 1ull << 29, 4);
    expect("OCM_ADAM_HOST_GRID=0", kOne26, kHost, {true, 0, 4, 0}, 512, true, 1ull << 29, 4);  // the HBM rule
    const int vec[3][2] = {{2, 2}, {8, 8}, {3, 4}};
    for (const auto &v : vec) {
        expect("OCM_ADAM_HOST_VEC fp32", kOne26, kHost, {true, 128, v[0], 0}, 128, true, 1ull << 29, v[1]);
        expect("OCM_ADAM_HOST_VEC bf16", kOne26W, {true, true}, {true, 128, v[0], 0}, 128, true, 3ull << 28, 4);
        expect("OCM_ADAM_HOST_VEC hbm", kOne26, kHbm, {true, 128, v[0], 0}, 512, false, 1ull << 29, 4);
    }
    if (failures == before) std::printf("PASS knobs\n");
}

StateSpace space(uint32_t n_ext, uint32_t unit_shift) {
    StateSpace s{};
    s.n_ext = n_ext;
    s.unit_shift = unit_shift;
    return s;
}

void test_space() {
    const int before = failures;
    // state_space_ok: 1 .. kXferMaxExtents (8) extents; a striped space needs 4 <= shift < 64
    for (const uint32_t shift : {0u, 3u, 4u, 63u, 64u}) {
        CHECK(!state_space_ok(space(0, shift)), "no extents, shift %u: accepted", shift);
        CHECK(state_space_ok(space(1, shift)), "one extent, shift %u: refused (not striped: the shift is unused)", shift);
        CHECK(!state_space_ok(space(9, shift)), "9 extents, shift %u: accepted", shift);
        const bool want = shift >= 4 && shift < 64;
        CHECK(state_space_ok(space(2, shift)) == want, "2 extents, shift %u: expected %d", shift, (int)want);
        CHECK(state_space_ok(space(8, shift)) == want, "8 extents, shift %u: expected %d", shift, (int)want);
    }
    // state_place against the definition: unit u = x >> shift lives on extent u % n at
    // ((u / n) << shift) | (x & mask), in plain 64-bit arithmetic
    std::mt19937_64 rng(20261020);
    for (const uint32_t n : {1u, 2u, 3u, 5u, 6u, 7u, 8u})
        for (const uint32_t shift : {4u, 12u, 21u}) {
            const uint64_t unit = 1ull << shift;
            std::vector<uint64_t> xs;
            // around unit boundaries: the first byte, the last 16-byte vector of a unit, the first of the next;
            // around unit 2^32, where the 32-bit arithmetic hands over to the 64-bit
            const uint64_t n64 = n, k4g = 1ull << 32;
            for (const uint64_t u : {n64 - 1, n64, n64 + 1, n64 + 2, 1000003 * n64, k4g - 2, k4g - 1, k4g, k4g + 1, k4g + n64})
                for (const uint64_t in : {uint64_t{0}, unit - 16})
                    xs.push_back((u << shift) + in);
            // 16-byte aligned, below 2^60; every other one below unit 2^32, for the 32-bit arithmetic
            for (int i = 0; i < 4096; i++) xs.push_back(((i & 1) ? rng() >> 4 : rng() >> (32 - shift)) & ~15ull);
            std::set<std::pair<uint32_t, uint64_t>> seen;
            std::set<uint64_t> distinct(xs.begin(), xs.end());
            for (const uint64_t x : distinct) {
                const uint64_t u = x >> shift;
                const StatePlace p = state_place(n, shift, x);
                CHECK(p.index == u % n && p.off == (((u / n) << shift) | (x & (unit - 1))),
                      "n_ext %u shift %u x %llu: extent %u offset %llu", n, shift, (unsigned long long)x, p.index,
                      (unsigned long long)p.off);
                // a byte inside the vector stays with it
                const StatePlace q = state_place(n, shift, x + 15);
                CHECK(q.index == p.index && q.off == p.off + 15, "n_ext %u shift %u x %llu: the vector is split", n, shift,
                      (unsigned long long)x);
                CHECK(seen.insert({p.index, p.off}).second, "n_ext %u shift %u x %llu: a place taken twice", n, shift,
                      (unsigned long long)x);
            }
        }
    if (failures == before) std::printf("PASS space\n");
}

}  // namespace

int main() {
    test_one_tensor();
    test_lists();
    test_host_variant();
    test_knobs();
    test_space();
    std::printf("%d failure(s)\n", failures);
    return failures ? 1 : 0;
}
