// The MXFP8 host codec (ocm/mx8.h) on fixed groups with hard-coded expected bytes
// (taken from the torch oracle, oncilla_amd/ops/quant.py). Stand-alone: it links
// nothing of the library, so the build also makes an ASan + UBSan copy of it.
#include <cstdio>
#include <cstring>
#include <vector>

#include "ocm/mx8.h"

using namespace ocm;

namespace {

int failures = 0;

struct Case {
    const char *name;
    uint32_t dtype;
    uint16_t src[8];  // elements 0..7 of the group, the other 24 are +0
    uint8_t codes[8];
    uint8_t scale;
    uint16_t dec[8];
};

const Case kCases[] = {
    // an all-zero group with a -0.0
    {"zero bf16", kMx8Bf16, {0, 0x8000}, {0, 0x80}, 127, {0, 0x8000}},
    {"zero fp16", kMx8Fp16, {0, 0x8000}, {0, 0x80}, 127, {0, 0x8000}},
    // amax = 3.5 = 0.875 * 2^2: m == 0.875 exactly, scaled to 448
    {"m875 bf16", kMx8Bf16, {0x4060, 0x3f80, 0xbf00}, {0x7e, 0x70, 0xe8}, 120, {0x4060, 0x3f80, 0xbf00}},
    {"m875 fp16", kMx8Fp16, {0x4300, 0x3c00, 0xb800}, {0x7e, 0x70, 0xe8}, 120, {0x4300, 0x3c00, 0xb800}},
    // the next representable amax above it: one exponent up, scaled to just over 224
    {"m875+ bf16", kMx8Bf16, {0x4061, 0x3f80, 0xbf00}, {0x76, 0x68, 0xe0}, 121, {0x4060, 0x3f80, 0xbf00}},
    {"m875+ fp16", kMx8Fp16, {0x4301, 0x3c00, 0xb800}, {0x76, 0x68, 0xe0}, 121, {0x4300, 0x3c00, 0xb800}},
    // amax 448 (e = 0); small members land in fp8 subnormals: 2^-9, 3 * 2^-9, -2^-10 (a tie, to
    // even: -0), 1.5 * 2^-10, 2^-11, 7.5 * 2^-9 (a tie, to even: the smallest normal)
    {"subnormals bf16", kMx8Bf16, {0x43e0, 0x3b00, 0x3bc0, 0xba80, 0x3ac0, 0x3a00, 0x3c70},
     {0x7e, 0x01, 0x03, 0x80, 0x01, 0x00, 0x08}, 127, {0x43e0, 0x3b00, 0x3bc0, 0x8000, 0x3b00, 0x0000, 0x3c80}},
    {"subnormals fp16", kMx8Fp16, {0x5f00, 0x1800, 0x1e00, 0x9400, 0x1600, 0x1000, 0x2380},
     {0x7e, 0x01, 0x03, 0x80, 0x01, 0x00, 0x08}, 127, {0x5f00, 0x1800, 0x1e00, 0x8000, 0x1800, 0x0000, 0x2400}},
    // ties on [16, 32), where e4m3fn steps by 2: 17 -> 16, 19 -> 20, 21 -> 20, -17 -> -16, 23 -> 24
    {"ties bf16", kMx8Bf16, {0x43e0, 0x4188, 0x4198, 0x41a8, 0xc188, 0x41b8}, {0x7e, 0x58, 0x5a, 0x5a, 0xd8, 0x5c}, 127,
     {0x43e0, 0x4180, 0x41a0, 0x41a0, 0xc180, 0x41c0}},
    {"ties fp16", kMx8Fp16, {0x5f00, 0x4c40, 0x4cc0, 0x4d40, 0xcc40, 0x4dc0}, {0x7e, 0x58, 0x5a, 0x5a, 0xd8, 0x5c}, 127,
     {0x5f00, 0x4c00, 0x4d00, 0x4d00, 0xcc00, 0x4e00}},
    // the smallest bf16 subnormal as amax: e = -141 clamps to -127
    {"clamp bf16", kMx8Bf16, {0x0001, 0x8001}, {0x08, 0x88}, 0, {0x0001, 0x8001}},
    // fp16 subnormals; and the largest fp16, which decodes past it to infinity
    {"subnormal fp16", kMx8Fp16, {0x0001, 0x0003}, {0x70, 0x7c}, 96, {0x0001, 0x0003}},
    {"max fp16", kMx8Fp16, {0x7bff, 0xfbff, 0x63d0}, {0x78, 0xf8, 0x48}, 135, {0x7c00, 0xfc00, 0x6400}},
};

void check(bool ok, const char *name, const char *what, int i, unsigned got, unsigned want) {
    if (ok) return;
    failures++;
    std::printf("FAIL %s: %s[%d] = 0x%x, expected 0x%x\n", name, what, i, got, want);
}

void run_case(const Case &c) {
    uint16_t src[kMx8Group] = {};
    std::memcpy(src, c.src, sizeof(c.src));
    std::vector<uint8_t> rec(mx8_record_bytes(kMx8Group), 0xaa);
    mx8_encode(src, kMx8Group, c.dtype, rec.data());
    for (int i = 0; i < kMx8Group; i++) check(rec[i] == (i < 8 ? c.codes[i] : 0), c.name, "code", i, rec[i], i < 8 ? c.codes[i] : 0);
    check(rec[kMx8Group] == c.scale, c.name, "scale", 0, rec[kMx8Group], c.scale);
    std::vector<uint16_t> out(kMx8Group, 0xaaaa);
    mx8_decode(rec.data(), kMx8Group, c.dtype, out.data());
    for (int i = 0; i < kMx8Group; i++) check(out[i] == (i < 8 ? c.dec[i] : 0), c.name, "decoded", i, out[i], i < 8 ? c.dec[i] : 0);
}

// Properties over every finite bf16 magnitude as a group's amax: the scaled maximum lies in
// (224, 448] unless e was clamped, and it never encodes to a NaN code.
void sweep_amax() {
    for (uint32_t h = 1; h < 0x7f80u; h++) {
        uint16_t src[kMx8Group] = {};
        src[5] = (uint16_t)h;
        src[6] = (uint16_t)(h | 0x8000u);
        uint8_t rec[kMx8Group + 1];
        mx8_encode(src, kMx8Group, kMx8Bf16, rec);
        const int e = (int)rec[kMx8Group] - kMx8ScaleBias;
        const double scaled = std::ldexp((double)mx8_bf16_to_f32((uint16_t)h), -e);
        const bool ok = e == -127 ? scaled <= 448.0 : (scaled > 224.0 && scaled <= 448.0);
        check(ok, "sweep", "scaled amax out of (224, 448] at bf16", (int)h, (unsigned)scaled, 448);
        check((rec[5] & 0x7f) != 0x7f && rec[6] == (rec[5] | 0x80), "sweep", "code", (int)h, rec[5], 0);
        check(rec[kMx8Group] != 255, "sweep", "scale", (int)h, rec[kMx8Group], 254);
        // the decoded value, before it is narrowed (the largest bf16 values round up past the
        // format's finite range), is within half an fp8 step of 16 * 2^e: amax / 14
        const double x = mx8_bf16_to_f32((uint16_t)h), back = std::ldexp((double)mx8_e4m3_to_f32(rec[5]), e);
        check(std::fabs(back - x) <= x / 14.0 || e == -127, "sweep", "round trip", (int)h, rec[5], h);
    }
}

// fp16 <-> fp32 over every fp16 bit pattern that is not a NaN: widening and narrowing are inverse.
void sweep_fp16() {
    for (uint32_t h = 0; h < 0x10000u; h++) {
        if ((h & 0x7fffu) > 0x7c00u) continue;
        const uint16_t back = mx8_f32_to_fp16(mx8_fp16_to_f32((uint16_t)h));
        check(back == h, "fp16", "round trip", (int)h, back, h);
    }
    // ties to even and the overflow threshold
    check(mx8_f32_to_fp16(1.0f + 0x1p-11f) == 0x3c00, "fp16", "tie down", 0, mx8_f32_to_fp16(1.0f + 0x1p-11f), 0x3c00);
    check(mx8_f32_to_fp16(1.0f + 3 * 0x1p-11f) == 0x3c02, "fp16", "tie up", 0, mx8_f32_to_fp16(1.0f + 3 * 0x1p-11f), 0x3c02);
    check(mx8_f32_to_fp16(65519.0f) == 0x7bff, "fp16", "below overflow", 0, mx8_f32_to_fp16(65519.0f), 0x7bff);
    check(mx8_f32_to_fp16(65520.0f) == 0x7c00, "fp16", "overflow", 0, mx8_f32_to_fp16(65520.0f), 0x7c00);
    check(mx8_f32_to_fp16(0x1p-25f) == 0, "fp16", "tiny tie", 0, mx8_f32_to_fp16(0x1p-25f), 0);
    check(mx8_f32_to_fp16(3 * 0x1p-25f) == 2, "fp16", "tiny tie up", 0, mx8_f32_to_fp16(3 * 0x1p-25f), 2);
}

// Every e4m3fn code but the two NaNs survives decode -> encode.
void sweep_codes() {
    for (uint32_t c = 0; c < 256; c++) {
        if ((c & 0x7f) == 0x7f) continue;
        const uint8_t back = mx8_f32_to_e4m3(mx8_e4m3_to_f32((uint8_t)c));
        check(back == c, "e4m3", "round trip", (int)c, back, c);
    }
}

// A record of several groups: codes first, then the scale bytes, nothing written past the end.
void multi_group() {
    const uint64_t n = 5 * kMx8Group;
    std::vector<uint16_t> src(n);
    for (uint64_t i = 0; i < n; i++) src[i] = mx8_f32_to_bf16((float)((int)(i * 37 % 101) - 50) * (float)(1 + i / 32));
    std::vector<uint8_t> rec(mx8_record_bytes(n) + 8, 0x5a);
    mx8_encode(src.data(), n, kMx8Bf16, rec.data());
    for (int i = 0; i < 8; i++) check(rec[mx8_record_bytes(n) + i] == 0x5a, "multi", "guard", i, rec[mx8_record_bytes(n) + i], 0x5a);
    check(mx8_record_bytes(n) == 165, "multi", "record bytes", 0, (unsigned)mx8_record_bytes(n), 165);
    for (uint64_t g = 0; g < 5; g++) {
        uint8_t one[kMx8Group + 1];
        mx8_encode(src.data() + g * kMx8Group, kMx8Group, kMx8Bf16, one);
        check(std::memcmp(one, rec.data() + g * kMx8Group, kMx8Group) == 0, "multi", "codes of group", (int)g, 0, 0);
        check(one[kMx8Group] == rec[n + g], "multi", "scale of group", (int)g, rec[n + g], one[kMx8Group]);
    }
}

}  // namespace

int main() {
    for (const Case &c : kCases) run_case(c);
    if (!failures) std::printf("PASS edge_groups\n");
    int before = failures;
    sweep_amax();
    if (failures == before) std::printf("PASS amax_sweep\n");
    before = failures;
    sweep_fp16();
    if (failures == before) std::printf("PASS fp16_convert\n");
    before = failures;
    sweep_codes();
    if (failures == before) std::printf("PASS e4m3_codes\n");
    before = failures;
    multi_group();
    if (failures == before) std::printf("PASS record_layout\n");
    std::printf("%s (%d failures)\n", failures ? "FAILED" : "OK", failures);
    return failures ? 1 : 0;
}
