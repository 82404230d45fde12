// The gradient-norm reduction over remote accumulators (ocm/acc_norm.h): the per-tensor
// validator acc_norm_check, each rule accepted at its edge and refused one past it; the launch
// shape acc_norm_launch_shape (kernel variant, grid, span) under the knobs, and the workspace
// bound; the C++ reference of the reduction on integer-valued inputs, where the sum is exact;
// the non-finite count on bit patterns; and the clip rule. The expected values are written out
// as numbers. Stand-alone: it sees the HIP headers through ocm/optim.h and links nothing of HIP,
// so the build also makes an ASan + UBSan copy of it.
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "ocm/acc_norm.h"

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
constexpr uint64_t kHalf = 1ull << 20;  // bytes of the allocation's remote half

float from_bits(uint32_t b) {
    float f;
    std::memcpy(&f, &b, 4);
    return f;
}

void verdict(const char *what, AccNormBad got, AccNormBad want) {
    CHECK(got == want, "%s: %d (%s), expected %d", what, (int)got, acc_norm_why(got), (int)want);
}

void test_validator() {
    const int before = failures;
    verdict("g_off 16", acc_norm_check(1024, 16, kHalf), ACC_NORM_OK);
    verdict("g_off 8", acc_norm_check(1024, 8, kHalf), ACC_NORM_ALIGN);
    verdict("g_off 4", acc_norm_check(0, 4, kHalf), ACC_NORM_ALIGN);
    verdict("g_off 0", acc_norm_check(1024, 0, kHalf), ACC_NORM_OK);
    // the range ends at the half's last byte; one word, one vector beyond
    verdict("ends at the last byte", acc_norm_check(1024, kHalf - 4096, kHalf), ACC_NORM_OK);
    verdict("one word beyond", acc_norm_check(1025, kHalf - 4096, kHalf), ACC_NORM_RANGE);
    verdict("one vector beyond", acc_norm_check(1024, kHalf - 4096 + 16, kHalf), ACC_NORM_RANGE);
    verdict("g_off at the end, n = 0", acc_norm_check(0, kHalf, kHalf), ACC_NORM_OK);
    verdict("g_off past the end, n = 0", acc_norm_check(0, kHalf + 16, kHalf), ACC_NORM_RANGE);
    // g_off + 4 n: 4 n wraps for n >= 2^62, and n near 2^61 must not slip through either
    const uint64_t huge = (1ull << 63) - 4;  // bytes of 2^61 - 1 words
    verdict("n = 2^61 - 1, largest half", acc_norm_check((1ull << 61) - 1, 0, huge), ACC_NORM_OK);
    verdict("n = 2^61 - 1 behind g_off 16", acc_norm_check((1ull << 61) - 1, 16, huge), ACC_NORM_RANGE);
    verdict("n = 2^61", acc_norm_check(1ull << 61, 0, huge), ACC_NORM_RANGE);
    verdict("n = 2^62 (4 n wraps to 0)", acc_norm_check(1ull << 62, 0, kHalf), ACC_NORM_RANGE);
    verdict("n = 2^62 + 4 (4 n wraps to 16)", acc_norm_check((1ull << 62) + 4, 0, kHalf), ACC_NORM_RANGE);
    verdict("g_off + 4 n wraps", acc_norm_check(8, UINT64_MAX - 15, UINT64_MAX), ACC_NORM_RANGE);
    // the list: the count, and the first tensor at fault
    const uint64_t n[3] = {64, 1025, 64}, off[3] = {0, kHalf - 4096, 8};
    int at = 7;
    verdict("count -1", acc_norm_check_list(-1, n, off, kHalf, &at), ACC_NORM_COUNT);
    CHECK(at == -1, "count -1 names tensor %d", at);
    verdict("count 0", acc_norm_check_list(0, nullptr, nullptr, kHalf, &at), ACC_NORM_OK);
    verdict("count 1", acc_norm_check_list(1, n, off, kHalf, &at), ACC_NORM_OK);
    CHECK(at == -1, "a good list names tensor %d", at);
    verdict("count 3", acc_norm_check_list(3, n, off, kHalf, &at), ACC_NORM_RANGE);
    CHECK(at == 1, "the first bad tensor is 1, got %d", at);
    if (failures == before) std::printf("PASS validator\n");
}

void expect(const char *what, const std::vector<uint64_t> &n, const std::vector<uint64_t> &g, bool host_acc,
            uint32_t n_ext, const AdamKnobs &k, uint32_t gx, bool host, uint64_t span) {
    const AccNormShape s = acc_norm_launch_shape(n.data(), g.data(), (uint32_t)n.size(), host_acc, n_ext, kCus, k);
    CHECK(s.gx == gx && s.host == host && s.span == span, "%s: gx %u host %d span %llu, expected %u %d %llu", what, s.gx,
          (int)s.host, (unsigned long long)s.span, gx, (int)host, (unsigned long long)span);
    CHECK(s.gx <= acc_norm_max_gx(kCus, k), "%s: gx %u above the workspace bound %u", what, s.gx,
          acc_norm_max_gx(kCus, k));
}

void test_shape() {
    const int before = failures;
    const uint64_t n26 = 1ull << 26;
    // the host variant only for one host extent within 32 bits, on the host grid
    expect("host, one extent", {n26}, {256}, true, 1, kDefault, 128, true, 256 + (1ull << 28));
    expect("hbm", {n26}, {256}, false, 1, kDefault, 512, false, 256 + (1ull << 28));
    expect("host, two extents", {n26}, {0}, true, 2, kDefault, 512, false, 1ull << 28);
    expect("striped hbm", {n26}, {0}, false, 3, kDefault, 512, false, 1ull << 28);
    expect("span 2^32", {1024}, {k4G - 4096}, true, 1, kDefault, 1, false, k4G);
    expect("span 2^32 - 16", {1020}, {k4G - 4096}, true, 1, kDefault, 1, true, k4G - 16);
    // the tail (n % 4) goes through 64-bit addresses and adds nothing to the span
    expect("n = 1027", {1027}, {16384}, true, 1, kDefault, 1, true, 16384 + 4096);
    expect("tail-only tensor at 2^32 - 16", {4096, 3}, {0, k4G - 16}, true, 1, kDefault, 1, true, k4G - 16);
    // the proportional split: equal tensors share the grid, one long among tiny ones gets nearly all
    expect("four equal, hbm", {n26, n26, n26, n26}, {0, 1ull << 28, 2ull << 28, 3ull << 28}, false, 1, kDefault, 128,
           false, 4ull << 28);
    expect("four equal, host", {1 << 24, 1 << 24, 1 << 24, 1 << 24}, {0, 1 << 26, 2 << 26, 3 << 26}, true, 1, kDefault,
           32, true, 4 << 26);
    expect("one long among tiny, hbm", {n26, 4, 4, 4}, {0, 1ull << 28, (1ull << 28) + 16, (1ull << 28) + 32}, false, 1,
           kDefault, 512, false, (1ull << 28) + 48);
    expect("short tensor", {5000}, {0}, false, 1, kDefault, 2, false, 20000);
    // the knobs
    expect("host variant off", {n26}, {0}, true, 1, {false, 128, 4, 0}, 512, false, 1ull << 28);
    expect("host grid 64", {n26}, {0}, true, 1, {true, 64, 4, 0}, 64, true, 1ull << 28);
    expect("host grid 0: the HBM rule", {n26}, {0}, true, 1, {true, 0, 4, 0}, 512, true, 1ull << 28);
    expect("grid forced, host", {n26}, {0}, true, 1, {true, 128, 4, 7}, 7, true, 1ull << 28);
    expect("grid forced, hbm", {n26, 4}, {0, 1ull << 28}, false, 1, {true, 128, 4, 7}, 7, false, (1ull << 28) + 16);
    // vectors in flight are not a knob here
    expect("host_vec 8", {n26}, {0}, true, 1, {true, 128, 8, 0}, 128, true, 1ull << 28);
    // no work for all-empty lists
    expect("no tensors", {}, {}, true, 1, kDefault, 0, false, 0);
    expect("empty tensors", {0, 0, 0}, {0, 16, 4096}, false, 1, kDefault, 0, false, 4096);
    expect("empty tensors, grid forced", {0, 0}, {0, 16}, false, 1, {true, 128, 4, 7}, 0, false, 16);
    // the workspace: one partial per (tensor, workgroup) of the largest launch
    CHECK(acc_norm_work_bytes(0, kCus, kDefault) == 0, "an empty list needs no workspace");
    CHECK(acc_norm_work_bytes(1, kCus, kDefault) == 512 * 16, "work bytes of 1 tensor");
    CHECK(acc_norm_work_bytes(32, kCus, kDefault) == 32 * 512 * 16, "work bytes of 32 tensors");
    CHECK(acc_norm_work_bytes(37, kCus, kDefault) == 32 * 512 * 16, "work bytes of 37 tensors");
    CHECK(acc_norm_work_bytes(2, 32, kDefault) == 2 * 128 * 16, "few CUs: the host grid is the larger");
    CHECK(acc_norm_work_bytes(2, kCus, {true, 128, 4, 7}) == 2 * 7 * 16, "grid forced");
    if (failures == before) std::printf("PASS shape\n");
}

void test_reference() {
    const int before = failures;
    // integers: every square and every partial sum is an integer below 2^53, so the sum is exact
    std::vector<float> v;
    unsigned long long want = 0;
    for (int j = 0; j < 4099; j++) {
        const long long x = (j * 37) % 2001 - 1000;
        v.push_back((float)x);
        want += (unsigned long long)(x * x);
    }
    double s = -1.0;
    uint64_t bad = 99;
    acc_norm_reference(v.data(), v.size(), &s, &bad);
    CHECK(s == (double)want && bad == 0, "integers: %.17g and %llu non-finite, expected %llu and 0", s,
          (unsigned long long)bad, want);
    acc_norm_reference(v.data(), 0, &s, &bad);
    CHECK(s == 0.0 && !std::signbit(s) && bad == 0, "no words: %.17g, %llu", s, (unsigned long long)bad);
    // squares past FLT_MAX (2^128): small integers times 2^100, so the sum is an integer times 2^200
    const std::vector<float> big = {0x1p100f, -0x1p100f, 0x1p101f, 0x3p100f};
    acc_norm_reference(big.data(), big.size(), &s, &bad);
    CHECK(s == 15.0 * 0x1p200 && bad == 0, "(1 + 1 + 4 + 9) * 2^200: %.17g", s);
    const float fmax[1] = {FLT_MAX};  // the largest square there is: finite, and exactly the double product
    acc_norm_reference(fmax, 1, &s, &bad);
    CHECK(s == (double)FLT_MAX * (double)FLT_MAX && std::isfinite(s) && s > 1e77 && bad == 0, "FLT_MAX^2: %.17g", s);
    // fp32 subnormals: the square of 2^-149 is 2^-298, a normal double
    const std::vector<float> tiny = {from_bits(1), from_bits(0x80000001u), from_bits(2), from_bits(0x007fffffu)};
    acc_norm_reference(tiny.data(), tiny.size(), &s, &bad);
    const double m = 8388607.0;  // 2^23 - 1: its square is below 2^46, exact
    CHECK(s == (1.0 + 1.0 + 4.0 + m * m) * 0x1p-298 && bad == 0, "subnormals: %.17g", s);
    // the totals: index order, at index count
    double ss[4] = {1.0, 0x1p60, 3.0, -1.0};
    uint64_t bb[4] = {1, 0, 5, 77};
    acc_norm_totals(ss, bb, 3);
    CHECK(ss[3] == (1.0 + 0x1p60) + 3.0 && bb[3] == 6, "totals: %.17g, %llu", ss[3], (unsigned long long)bb[3]);
    acc_norm_totals(ss, bb, 0);
    CHECK(ss[0] == 0.0 && bb[0] == 0, "totals of nothing");
    if (failures == before) std::printf("PASS reference\n");
}

void test_nonfinite() {
    const int before = failures;
    const struct {
        uint32_t bits;
        bool counted;
    } words[] = {
        {0x7f800000u, true},   // +inf
        {0xff800000u, true},   // -inf
        {0x7fc00000u, true},   // quiet NaN
        {0xffc00001u, true},   // quiet NaN, negative, payload
        {0x7f800001u, true},   // signalling NaN, smallest payload
        {0x7fbfffffu, true},   // signalling NaN, largest payload
        {0xffa5c3e1u, true},   // a NaN with a payload
        {0x7f7fffffu, false},  // FLT_MAX
        {0xff7fffffu, false},  // -FLT_MAX
        {0x00000001u, false},  // the smallest subnormal
        {0x807fffffu, false},  // the largest subnormal, negative
        {0x00800000u, false},  // FLT_MIN
        {0x00000000u, false},
        {0x80000000u, false},
        {0x3f800000u, false},
    };
    std::vector<float> v;
    uint64_t want = 0;
    for (const auto &w : words) {
        CHECK(acc_norm_nonfinite(w.bits) == w.counted, "0x%08x counted %d", w.bits, (int)!w.counted);
        v.push_back(from_bits(w.bits));
        want += w.counted ? 1 : 0;
    }
    double s;
    uint64_t bad;
    acc_norm_reference(v.data(), v.size(), &s, &bad);
    CHECK(bad == want && want == 7 && std::isnan(s), "the list: %llu counted, sum %.17g", (unsigned long long)bad, s);
    acc_norm_reference(v.data(), 2, &s, &bad);  // infinities only
    CHECK(bad == 2 && std::isinf(s) && s > 0, "infinities: %llu counted, sum %.17g", (unsigned long long)bad, s);
    acc_norm_reference(v.data() + 7, 8, &s, &bad);  // the finite ones
    CHECK(bad == 0 && std::isfinite(s), "finite words: %llu counted, sum %.17g", (unsigned long long)bad, s);
    if (failures == before) std::printf("PASS nonfinite\n");
}

void test_clip_rule() {
    const int before = failures;
    // norm 5 (sumsq 25): at and below max_norm the coefficient is 1 and the scale comes back as it is
    CHECK(clip_scale(25.0, 1.0, 5.000001) == 1.0, "at max_norm (with torch's 1e-6): %.17g", clip_scale(25.0, 1.0, 5.000001));
    CHECK(clip_scale(25.0, 1.0, 6.0) == 1.0, "below max_norm");
    CHECK(clip_scale(25.0, 0.25, 1.25 + 1e-6) == 0.25, "scaled norm 1.25 at max_norm");
    CHECK(clip_scale(25.0, 1.0, 1e300) == 1.0, "far below max_norm");
    // torch's 1e-6 in the denominator clips a norm that equals max_norm by that much
    CHECK(clip_scale(25.0, 1.0, 5.0) == 5.0 / (5.0 + 1e-6), "norm == max_norm: %.17g", clip_scale(25.0, 1.0, 5.0));
    // above: scale * max_norm / (norm + 1e-6)
    CHECK(clip_scale(25.0, 1.0, 1.0) == 1.0 / (5.0 + 1e-6), "norm 5 to 1: %.17g", clip_scale(25.0, 1.0, 1.0));
    CHECK(clip_scale(25.0, 0.5, 1.0) == 0.5 * (1.0 / (2.5 + 1e-6)), "scale 0.5: %.17g", clip_scale(25.0, 0.5, 1.0));
    // a negative scale: the norm takes |scale|, the result keeps the sign
    CHECK(clip_scale(25.0, -0.5, 1.0) == -0.5 * (1.0 / (2.5 + 1e-6)), "scale -0.5: %.17g", clip_scale(25.0, -0.5, 1.0));
    CHECK(clip_scale(25.0, -0.5, 10.0) == -0.5, "scale -0.5 below max_norm");
    // zero norm: max_norm / 1e-6 is far above 1
    CHECK(clip_scale(0.0, 1.0, 1.0) == 1.0, "zero norm");
    CHECK(clip_scale(0.0, 0.125, 1e-3) == 0.125, "zero norm, small max_norm");
    CHECK(clip_scale(25.0, 0.0, 1.0) == 0.0, "zero scale");
    // a sum of squares past fp32's range, and the non-finite norms
    CHECK(clip_scale(1e60, 1.0, 1.0) == 1.0 / (1e30 + 1e-6), "norm 1e30");
    CHECK(clip_scale(INFINITY, 1.0, 1.0) == 0.0, "infinite norm: %.17g", clip_scale(INFINITY, 1.0, 1.0));
    CHECK(std::isnan(clip_scale(NAN, 1.0, 1.0)), "NaN norm: %.17g", clip_scale(NAN, 1.0, 1.0));
    if (failures == before) std::printf("PASS clip_rule\n");
}

}  // namespace

int main() {
    test_validator();
    test_shape();
    test_reference();
    test_nonfinite();
    test_clip_rule();
    std::printf("%d failure(s)\n", failures);
    return failures ? 1 : 0;
}
