// The accumulator side of the fused Adam (ocm/optim.h): the per-tensor validator
// adam_acc_check, each rule accepted at its edge and refused one past it, and the launch
// shape adam_acc_launch_shape (kernel variant, span of each space, grid) for every
// placement of the two spaces and under the knobs. The expected values are written out as
// numbers. Stand-alone: it sees the HIP headers through ocm/optim.h and links nothing of
// HIP, so the build also makes an ASan + UBSan copy of it.
#include <cmath>
#include <cstdio>
#include <limits>
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
constexpr uint64_t kHalf = 1ull << 20;  // bytes of the gradient allocation's remote half

AdamTensor tensor(uint64_t n, uint64_t m_off, uint64_t v_off, uint64_t w_off = 0) {
    return AdamTensor{nullptr, nullptr, n, w_off, m_off, v_off};
}

void verdict(const char *what, AdamAccBad got, AdamAccBad want) {
    CHECK(got == want, "%s: %d (%s), expected %d", what, (int)got, adam_acc_why(got), (int)want);
}

AdamAccBad check(const AdamTensor &t, uint64_t g_off, float gscale = 1.f, uint32_t flags = OCM_ADAM_ACC_ZERO,
                 bool bf16 = false, bool same = false, uint64_t half = kHalf) {
    return adam_acc_check(t, g_off, half, gscale, flags, bf16, same);
}

void test_validator() {
    const int before = failures;
    const AdamTensor t = tensor(1024, 0, 4096);
    verdict("g_off 16", check(t, 16), ADAM_ACC_OK);
    verdict("g_off 8", check(t, 8), ADAM_ACC_ALIGN);
    verdict("g_off 0", check(t, 0), ADAM_ACC_OK);
    // the range ends at the half's last byte; one word beyond
    verdict("ends at the last byte", check(t, kHalf - 4096), ADAM_ACC_OK);
    verdict("one word beyond", check(tensor(1025, 0, 8192), kHalf - 4096), ADAM_ACC_RANGE);
    verdict("one vector beyond", check(t, kHalf - 4096 + 16), ADAM_ACC_RANGE);
    verdict("g_off at the end, n = 0", check(tensor(0, 0, 0), kHalf), ADAM_ACC_OK);
    verdict("g_off past the end, n = 0", check(tensor(0, 0, 0), kHalf + 16), ADAM_ACC_RANGE);
    // 4 n wraps for n >= 2^62; n near 2^61 must not slip through either, whatever the half
    const uint64_t huge = (1ull << 63) - 4;  // bytes of 2^61 - 1 words
    verdict("n = 2^61 - 1, largest half", check(tensor((1ull << 61) - 1, 0, 0), 0, 1.f, 0, false, false, huge),
            ADAM_ACC_OK);
    verdict("n = 2^61 - 1 behind g_off 16", check(tensor((1ull << 61) - 1, 0, 0), 16, 1.f, 0, false, false, huge),
            ADAM_ACC_RANGE);
    verdict("n = 2^61", check(tensor(1ull << 61, 0, 0), 0, 1.f, 0, false, false, huge), ADAM_ACC_RANGE);
    verdict("n = 2^62 (4 n wraps to 0)", check(tensor(1ull << 62, 0, 0), 0), ADAM_ACC_RANGE);
    verdict("n = 2^62 + 4 (4 n wraps to 16)", check(tensor((1ull << 62) + 4, 0, 0), 0), ADAM_ACC_RANGE);
    verdict("n = 2^61 + 1 in a small half", check(tensor((1ull << 61) + 1, 0, 0), 0), ADAM_ACC_RANGE);
    // the scale
    verdict("gscale 0.25", check(t, 0, 0.25f), ADAM_ACC_OK);
    verdict("gscale 0", check(t, 0, 0.f), ADAM_ACC_OK);
    verdict("gscale largest finite", check(t, 0, std::numeric_limits<float>::max()), ADAM_ACC_OK);
    verdict("gscale subnormal", check(t, 0, 1e-40f), ADAM_ACC_OK);
    verdict("gscale inf", check(t, 0, INFINITY), ADAM_ACC_SCALE);
    verdict("gscale -inf", check(t, 0, -INFINITY), ADAM_ACC_SCALE);
    verdict("gscale NaN", check(t, 0, NAN), ADAM_ACC_SCALE);
    // the flags
    verdict("flags 0", check(t, 0, 1.f, 0), ADAM_ACC_OK);
    verdict("flags ZERO", check(t, 0, 1.f, OCM_ADAM_ACC_ZERO), ADAM_ACC_OK);
    verdict("flags 2", check(t, 0, 1.f, 2u), ADAM_ACC_FLAGS);
    verdict("flags ZERO | 2^31", check(t, 0, 1.f, OCM_ADAM_ACC_ZERO | 0x80000000u), ADAM_ACC_FLAGS);
    if (failures == before) std::printf("PASS validator\n");
}

void test_overlap() {
    const int before = failures;
    // m at [4096, 8192), v at [16384, 20480), w at [32768, 36864): 1024 elements each
    const AdamTensor t = tensor(1024, 4096, 16384, 32768);
    const struct {
        const char *what;
        uint64_t g_off;
        bool hits_fp32, hits_bf16;
    } cases[] = {
        {"before m, touching", 0, false, false},
        {"last vector inside m", 16, true, true},
        {"on m", 4096, true, true},
        {"first vector inside m's last", 8192 - 16, true, true},
        {"behind m, touching", 8192, false, false},
        {"last vector inside v", 16384 - 4096 + 16, true, true},
        {"on v", 16384, true, true},
        {"behind v, touching", 20480, false, false},
        {"last vector inside w", 32768 - 4096 + 16, false, true},
        {"on w", 32768, false, true},
        {"behind w, touching", 36864, false, false},
    };
    for (const auto &c : cases) {
        verdict(c.what, check(t, c.g_off, 1.f, 0, false, true), c.hits_fp32 ? ADAM_ACC_OVERLAP : ADAM_ACC_OK);
        verdict(c.what, check(t, c.g_off, 1.f, 0, true, true), c.hits_bf16 ? ADAM_ACC_OVERLAP : ADAM_ACC_OK);
        // another allocation: the same numbers name other memory
        verdict(c.what, check(t, c.g_off, 1.f, 0, false, false), ADAM_ACC_OK);
        verdict(c.what, check(t, c.g_off, 1.f, 0, true, false), ADAM_ACC_OK);
    }
    // an empty tensor overlaps nothing
    verdict("n = 0 on m", check(tensor(0, 4096, 16384), 4096, 1.f, 0, false, true), ADAM_ACC_OK);
    // one element: its own word only
    verdict("n = 1 on m", check(tensor(1, 4096, 16384), 4096, 1.f, 0, false, true), ADAM_ACC_OVERLAP);
    verdict("n = 1 one vector behind m", check(tensor(1, 4096, 16384), 4112, 1.f, 0, false, true), ADAM_ACC_OK);
    if (failures == before) std::printf("PASS overlap\n");
}

struct Where {
    bool bf16, host_state, host_acc;
    uint32_t n_ext = 1, acc_n_ext = 1;
};

void expect(const char *what, const std::vector<AdamTensor> &ts, const std::vector<uint64_t> &g, Where w,
            const AdamKnobs &k, uint32_t gx, bool host, uint64_t span, uint64_t acc_span, int kV) {
    const AdamAccShape a = adam_acc_launch_shape(ts.data(), g.data(), (uint32_t)ts.size(), w.bf16, w.host_state,
                                                 w.n_ext, w.host_acc, w.acc_n_ext, kCus, k);
    CHECK(a.s.gx == gx && a.s.host == host && a.s.span == span && a.acc_span == acc_span && a.s.kV == kV,
          "%s: gx %u host %d span %llu acc span %llu kV %d, expected %u %d %llu %llu %d", what, a.s.gx, (int)a.s.host,
          (unsigned long long)a.s.span, (unsigned long long)a.acc_span, a.s.kV, gx, (int)host,
          (unsigned long long)span, (unsigned long long)acc_span, kV);
}

const std::vector<AdamTensor> kOne26 = {tensor(1ull << 26, 0, 1ull << 28)};  // fp32, 2^26 elements
const Where kHostHost{false, true, true}, kHbmHbm{false, false, false}, kHbmHost{false, false, true},
    kHostHbm{false, true, false};

void test_variant() {
    const int before = failures;
    // both spaces one host extent: the PCIe variant on its grid; anything else: generic, 2 workgroups per CU
    expect("host / host", kOne26, {256}, kHostHost, kDefault, 128, true, 1ull << 29, 256 + (1ull << 28), 4);
    expect("hbm / hbm", kOne26, {256}, kHbmHbm, kDefault, 512, false, 1ull << 29, 256 + (1ull << 28), 4);
    expect("hbm state, host accumulators", kOne26, {256}, kHbmHost, kDefault, 512, false, 1ull << 29,
           256 + (1ull << 28), 4);
    expect("host state, hbm accumulators", kOne26, {256}, kHostHbm, kDefault, 512, false, 1ull << 29,
           256 + (1ull << 28), 4);
    expect("host state in two extents", kOne26, {0}, {false, true, true, 2, 1}, kDefault, 512, false, 1ull << 29,
           1ull << 28, 4);
    expect("host accumulators in two extents", kOne26, {0}, {false, true, true, 1, 2}, kDefault, 512, false, 1ull << 29,
           1ull << 28, 4);
    expect("bf16 host / host", {tensor(1ull << 26, 0, 1ull << 28, 1ull << 29)}, {0}, {true, true, true}, kDefault, 128,
           true, 3ull << 28, 1ull << 28, 4);
    // the accumulator span alone reaches 2^32: generic; one vector less: host
    expect("acc span 2^32", {tensor(1024, 0, 4096)}, {k4G - 4096}, kHostHost, kDefault, 1, false, 8192, k4G, 4);
    expect("acc span 2^32 - 16", {tensor(1020, 0, 4096)}, {k4G - 4096}, kHostHost, kDefault, 1, true, 8176, k4G - 16, 4);
    expect("state span 2^32", {tensor(1024, 0, k4G - 4096)}, {0}, kHostHost, kDefault, 1, false, k4G, 4096, 4);
    // the tail (n % 4) goes through 64-bit addresses and adds nothing to either span
    expect("n = 1027", {tensor(1027, 0, 8192)}, {16384}, kHostHost, kDefault, 1, true, 12288, 16384 + 4096, 4);
    expect("tail-only tensor at 2^32 - 16", {tensor(4096, 0, 16384), tensor(3, 64, 128)}, {0, k4G - 16}, kHostHost,
           kDefault, 1, true, 32768, k4G - 16, 4);
    // the span is the farthest tensor's, wherever it stands in the list
    expect("span over a list", {tensor(8, 0, 64), tensor(1024, 4096, 8192), tensor(4, 128, 192)}, {65536, 1024, 16},
           kHostHost, kDefault, 1, true, 12288, 65536 + 32, 4);
    expect("no tensors", {}, {}, kHostHost, kDefault, 0, false, 0, 0, 4);
    if (failures == before) std::printf("PASS variant\n");
}

void test_knobs() {
    const int before = failures;
    expect("OCM_ADAM_HOST=0", kOne26, {0}, kHostHost, {false, 128, 4, 0}, 512, false, 1ull << 29, 1ull << 28, 4);
    expect("OCM_ADAM_GRID=7 host / host", kOne26, {0}, kHostHost, {true, 128, 4, 7}, 7, true, 1ull << 29, 1ull << 28, 4);
    expect("OCM_ADAM_GRID=7 mixed", kOne26, {0}, kHostHbm, {true, 128, 4, 7}, 7, false, 1ull << 29, 1ull << 28, 4);
    expect("OCM_ADAM_HOST_GRID=64", kOne26, {0}, kHostHost, {true, 64, 4, 0}, 64, true, 1ull << 29, 1ull << 28, 4);
    expect("OCM_ADAM_HOST_GRID=64 mixed", kOne26, {0}, kHbmHost, {true, 64, 4, 0}, 512, false, 1ull << 29, 1ull << 28, 4);
    const int vec[3][2] = {{2, 2}, {8, 8}, {3, 4}};
    for (const auto &v : vec) {
        expect("OCM_ADAM_HOST_VEC host / host", kOne26, {0}, kHostHost, {true, 128, v[0], 0}, 128, true, 1ull << 29,
               1ull << 28, v[1]);
        expect("OCM_ADAM_HOST_VEC mixed", kOne26, {0}, kHostHbm, {true, 128, v[0], 0}, 512, false, 1ull << 29, 1ull << 28,
               4);
        expect("OCM_ADAM_HOST_VEC bf16", {tensor(1ull << 26, 0, 1ull << 28, 1ull << 29)}, {0}, {true, true, true},
               {true, 128, v[0], 0}, 128, true, 3ull << 28, 1ull << 28, 4);
    }
    if (failures == before) std::printf("PASS knobs\n");
}

// Without an accumulator space (g_off null) the answer is adam_launch_shape's, field for field.
void test_agrees_without_accumulators() {
    const int before = failures;
    const std::vector<std::vector<AdamTensor>> lists = {
        kOne26,
        {tensor(3, 0, 16)},
        {tensor(1027, 0, 8192)},
        {tensor(1 << 20, 0, 4 << 20), tensor(1024, 8 << 20, (8 << 20) + 4096), tensor(0, 0, 0)},
        {tensor(1024, 0, k4G - 4096)},
        {}};
    const AdamKnobs knobs[] = {kDefault, {false, 128, 4, 0}, {true, 64, 8, 0}, {true, 0, 2, 0}, {true, 128, 4, 7}};
    for (const auto &ts : lists)
        for (const auto &k : knobs)
            for (int bits = 0; bits < 16; bits++) {
                const bool bf16 = bits & 1, host_state = bits & 2, host_acc = bits & 4;
                const uint32_t n_ext = bits & 8 ? 3 : 1;
                const AdamShape want = adam_launch_shape(ts.data(), (uint32_t)ts.size(), bf16, host_state, n_ext, kCus, k);
                const AdamAccShape got = adam_acc_launch_shape(ts.data(), nullptr, (uint32_t)ts.size(), bf16, host_state,
                                                               n_ext, host_acc, 1, kCus, k);
                CHECK(got.s.gx == want.gx && got.s.host == want.host && got.s.span == want.span && got.s.kV == want.kV &&
                          got.acc_span == 0,
                      "no accumulators, bits %d: gx %u / %u host %d / %d", bits, got.s.gx, want.gx, (int)got.s.host,
                      (int)want.host);
            }
    if (failures == before) std::printf("PASS agrees_without_accumulators\n");
}

}  // namespace

int main() {
    test_validator();
    test_overlap();
    test_variant();
    test_knobs();
    test_agrees_without_accumulators();
    std::printf("%d failure(s)\n", failures);
    return failures ? 1 : 0;
}
