// The accumulate element rule, validator and tile count (ocm/acc.h) on fixed vectors with
// the expected bit patterns written out (two fp32 roundings, as the torch oracle
// oncilla_amd.ops.accumulate_reference computes them). Stand-alone: it links nothing of
// the library, so the build also makes an ASan + UBSan copy of it.
#include <cstdio>
#include <cstring>
#include <vector>

#include "ocm/acc.h"

using namespace ocm;

namespace {

int failures = 0;

void check(bool ok, const char *part, const char *name, unsigned long long got, unsigned long long want) {
    if (ok) return;
    failures++;
    std::printf("FAIL %s: %s = 0x%llx, expected 0x%llx\n", part, name, got, want);
}

struct RuleCase {
    const char *name;
    uint32_t acc, x, scale, want;  // fp32 bit patterns
};

const RuleCase kRule[] = {
    {"pos zeros", 0x00000000u, 0x00000000u, 0x3f800000u, 0x00000000u},
    {"neg zeros", 0x80000000u, 0x80000000u, 0x3f800000u, 0x80000000u},
    {"mixed zeros", 0x00000000u, 0x80000000u, 0x3f800000u, 0x00000000u},
    {"neg scale zero", 0x80000000u, 0x00000000u, 0xbf800000u, 0x80000000u},
    // 2^-140 + 2^-141: subnormals are kept
    {"subnormal sum", 0x00000200u, 0x00000100u, 0x3f800000u, 0x00000300u},
    // 2^-120 * 2^-25 = 2^-145: a subnormal product
    {"subnormal product", 0x00000000u, 0x03800000u, 0x33000000u, 0x00000010u},
    // scale = 1/3: the product itself rounds
    {"third of one", 0x3f800000u, 0x3f800000u, 0x3eaaaaabu, 0x3faaaaabu},
    {"third of three", 0x3f800000u, 0x40400000u, 0x3eaaaaabu, 0x40000000u},
    {"third of seven", 0xc0000000u, 0x40e00000u, 0x3eaaaaabu, 0x3eaaaab0u},
    // (1 + 2^-12)^2 = 1 + 2^-11 + 2^-24 rounds (a tie, to even) to 1 + 2^-11, and the sum
    // with -(1 + 2^-11) is +0; a fused multiply-add would give 2^-24 (0x33800000)
    {"fusion tell-tale", 0xbf801000u, 0x3f800800u, 0x3f800800u, 0x00000000u},
    {"absorbed", 0x4b800000u, 0x3f800000u, 0x3f800000u, 0x4b800000u},
    {"cancel", 0x3fc00000u, 0xbfc00000u, 0x3f800000u, 0x00000000u},
    {"inf plus finite", 0x7f800000u, 0xc2c80000u, 0x40000000u, 0x7f800000u},
    {"largest overflow", 0x7f7fffffu, 0x7f7fffffu, 0x3f800000u, 0x7f800000u},
    {"largest cancel", 0x7f7fffffu, 0xff7fffffu, 0x3f800000u, 0x00000000u},
    {"product overflow", 0x00000000u, 0x7f7fffffu, 0x40000000u, 0x7f800000u},
};

bool is_nan(uint32_t b) { return (b & 0x7fffffffu) > 0x7f800000u; }

void element_rule() {
    const int before = failures;
    for (const RuleCase &c : kRule) {
        const uint32_t got = acc_float_bits(acc_rule(acc_bits_float(c.acc), acc_bits_float(c.x), acc_bits_float(c.scale)));
        check(got == c.want, "element_rule", c.name, got, c.want);
    }
    // inf + -inf, and a NaN element: some NaN
    const uint32_t n1 = acc_float_bits(acc_rule(acc_bits_float(0x7f800000u), acc_bits_float(0xff800000u), 1.0f));
    const uint32_t n2 = acc_float_bits(acc_rule(1.0f, acc_bits_float(0x7fc00001u), 2.0f));
    check(is_nan(n1), "element_rule", "inf + -inf is NaN", n1, 0x7fc00000u);
    check(is_nan(n2), "element_rule", "NaN element stays NaN", n2, 0x7fc00000u);
    if (failures == before) std::printf("PASS element_rule\n");
}

void widen16() {
    const int before = failures;
    const struct {
        uint16_t h;
        bool bf16;
        uint32_t want;
    } cases[] = {
        {0x0001, false, 0x33800000u},  // the smallest fp16 subnormal, 2^-24
        {0x83ff, false, 0xb87fc000u},  // the largest one, negative
        {0x0400, false, 0x38800000u},  // the smallest normal
        {0x7bff, false, 0x477fe000u},  // 65504
        {0xfc00, false, 0xff800000u},
        {0x8000, false, 0x80000000u},
        {0x3c00, false, 0x3f800000u},
        {0x0001, true, 0x00010000u},   // a bf16 subnormal is an fp32 subnormal
        {0x807f, true, 0x807f0000u},
        {0x7f7f, true, 0x7f7f0000u},
        {0xff80, true, 0xff800000u},
        {0x8000, true, 0x80000000u},
    };
    for (const auto &c : cases) {
        const uint32_t got = acc_float_bits(acc_widen16(c.h, c.bf16));
        check(got == c.want, "widen16", c.bf16 ? "bf16" : "fp16", got, c.want);
    }
    check(is_nan(acc_float_bits(acc_widen16(0x7e01, false))), "widen16", "fp16 NaN", 0, 1);
    // every finite fp16 against the compiler's own conversion
    for (uint32_t h = 0; h < 0x10000u; h++) {
        if (((h >> 10) & 31u) == 31u) continue;
        _Float16 f;
        const uint16_t hh = (uint16_t)h;
        std::memcpy(&f, &hh, 2);
        const uint32_t want = acc_float_bits((float)f), got = acc_float_bits(acc_widen16(h, false));
        if (got != want) {
            check(false, "widen16", "fp16 sweep", got, want);
            break;
        }
    }
    if (failures == before) std::printf("PASS widen16\n");
}

// acc_apply_host over heap arrays of every type, sizes around the tile: element i of the
// result is the rule on element i, and nothing outside [0, n) is read or written.
void apply_host() {
    const int before = failures;
    for (uint64_t n : {0ull, 4ull, 1020ull, 1024ull, 1028ull}) {
        for (uint32_t dt : {kAccF32, kAccBf16, kAccFp16}) {
            std::vector<float> acc(n), want(n);
            std::vector<uint32_t> x32(n);
            std::vector<uint16_t> x16(n);
            const float scale = acc_bits_float(0x3eaaaaabu);
            for (uint64_t i = 0; i < n; i++) {
                acc[i] = (float)i * 0.25f - 100.0f;
                const float x = (float)((i * 37) % 129) - 64.0f;  // exact in every type
                x32[i] = acc_float_bits(x);
                uint16_t h = (uint16_t)(x32[i] >> 16);             // exact bf16: 8 significant bits
                if (dt == kAccFp16) {
                    _Float16 f = (_Float16)x;
                    std::memcpy(&h, &f, 2);
                }
                x16[i] = h;
                want[i] = acc_rule(acc[i], x, scale);
            }
            acc_apply_host(acc.data(), dt == kAccF32 ? (const void *)x32.data() : (const void *)x16.data(), n, dt, scale);
            for (uint64_t i = 0; i < n; i++)
                if (acc_float_bits(acc[i]) != acc_float_bits(want[i])) {
                    check(false, "apply_host", "element", acc_float_bits(acc[i]), acc_float_bits(want[i]));
                    break;
                }
        }
    }
    if (failures == before) std::printf("PASS apply_host\n");
}

ocm_acc_params op(uint64_t lo, uint64_t ro, uint64_t elems, uint32_t dtype, float scale) {
    ocm_acc_params p;
    p.local_offset = lo;
    p.remote_offset = ro;
    p.elems = elems;
    p.dtype = dtype;
    p.scale = scale;
    return p;
}

void expect(const ocm_acc_params &p, uint64_t lb, uint64_t rb, int want_rc, const char *needle, uint64_t want_bytes,
            const char *name) {
    char why[192] = "";
    uint64_t bytes = 77;
    const int rc = acc_check_op(p, lb, rb, &bytes, why, sizeof(why));
    check(rc == want_rc, "validator", name, (unsigned)rc, (unsigned)want_rc);
    if (want_rc == 0)
        check(bytes == want_bytes, "validator", name, bytes, want_bytes);
    else if (!std::strstr(why, needle)) {
        failures++;
        std::printf("FAIL validator: %s says \"%s\", expected \"%s\"\n", name, why, needle);
    }
}

void validator() {
    const int before = failures;
    const float inf = acc_bits_float(0x7f800000u), nan = acc_bits_float(0x7fc00000u);
    expect(op(0, 0, 1024, kAccF32, 1.0f), 4096, 4096, 0, "", 4096, "exact fit fp32");
    expect(op(0, 0, 1024, kAccBf16, 1.0f), 2048, 4096, 0, "", 4096, "exact fit bf16");
    expect(op(16, 16, 1020, kAccFp16, -0.5f), 2056, 4096, 0, "", 4080, "offset fit");
    expect(op(4096, 4096, 0, kAccF32, 1.0f), 4096, 4096, 0, "", 0, "empty op at the very end");
    expect(op(0, 0, 4, 0, 1.0f), 4096, 4096, -1, "unknown element type 0", 0, "dtype 0");
    expect(op(0, 0, 4, 4, 1.0f), 4096, 4096, -1, "unknown element type 4", 0, "dtype 4");
    expect(op(0, 0, 4, kAccF32, inf), 4096, 4096, -1, "not finite", 0, "inf scale");
    expect(op(0, 0, 4, kAccF32, -inf), 4096, 4096, -1, "not finite", 0, "-inf scale");
    expect(op(0, 0, 4, kAccF32, nan), 4096, 4096, -1, "not finite", 0, "NaN scale");
    expect(op(0, 0, 6, kAccF32, 1.0f), 4096, 4096, -1, "multiple of 4", 0, "elems % 4");
    expect(op(0, 0, 1ull << 31, kAccBf16, 1.0f), ~0ull, ~0ull, -1, "below 2^31", 0, "2^31 elements");
    expect(op(8, 0, 4, kAccF32, 1.0f), 4096, 4096, -1, "local offset 8", 0, "local misaligned");
    expect(op(0, 24, 4, kAccF32, 1.0f), 4096, 4096, -1, "remote offset 24", 0, "remote misaligned");
    expect(op(4096 - 16, 0, 8, kAccF32, 1.0f), 4096, 4096, -1, "local range", 0, "local range");
    expect(op(4112, 0, 0, kAccF32, 1.0f), 4096, 4096, -1, "local range", 0, "local offset past the end");
    expect(op(0, 4096 - 16, 8, kAccBf16, 1.0f), 4096, 4096, -1, "remote range", 0, "remote range");
    expect(op(2048 - 16, 0, 12, kAccBf16, 1.0f), 2048, 4096, -1, "local range", 0, "16-bit local range");
    expect(op(2048 - 16, 0, 8, kAccBf16, 1.0f), 2048, 4096, 0, "", 32, "16-bit local range, exact");
    // nothing overflows: offsets at the top of the address space, the most elements against small halves
    expect(op(~0ull - 15, 0, 4, kAccF32, 1.0f), 4096, 4096, -1, "local range", 0, "local offset 2^64 - 16");
    expect(op(0, ~0ull - 15, 4, kAccF32, 1.0f), 4096, 4096, -1, "remote range", 0, "remote offset 2^64 - 16");
    expect(op(~0ull - 15, ~0ull - 15, (1ull << 31) - 4, kAccF32, 1.0f), ~0ull, ~0ull, -1, "local range", 0,
           "both at the top of huge halves");
    expect(op(0, 0, (1ull << 31) - 4, kAccF32, 1.0f), 4096, 4096, -1, "local range", 0, "2^31 - 4 elements, small halves");
    expect(op(0, 0, (1ull << 31) - 4, kAccBf16, 1.0f), 1ull << 33, 4096, -1, "remote range", 0, "2^31 - 4 elements, small remote");
    expect(op(0, 0, (1ull << 31) - 4, kAccF32, 1.0f), 1ull << 33, 1ull << 33, 0, "", ((1ull << 31) - 4) * 4, "2^31 - 4 elements fit");
    if (failures == before) std::printf("PASS validator\n");
}

struct Desc {  // the fields of XferBatchOp that acc_pack and acc_plan touch
    uint64_t lin_off, rem_off, len, first_tile;
    uint32_t put, pad;
};

void tile_counts() {
    const int before = failures;
    const struct {
        uint64_t elems, tiles;
    } cases[] = {{0, 0}, {4, 1}, {1020, 1}, {1024, 1}, {1028, 2}, {2048, 2}, {(1ull << 31) - 4, 1ull << 21}};
    for (const auto &c : cases) check(acc_tile_count(c.elems) == c.tiles, "tile_counts", "tiles", acc_tile_count(c.elems), c.tiles);
    Desc d[5] = {};
    const uint64_t elems[5] = {0, 4, 1020, 1024, 1028};
    for (int i = 0; i < 5; i++) acc_pack(op(16 * i, 32 * i, elems[i], kAccBf16, -2.0f), &d[i]);
    check(acc_plan(d, 5) == 5, "tile_counts", "total", acc_plan(d, 5), 5);
    const uint64_t first[5] = {0, 0, 1, 2, 3};
    for (int i = 0; i < 5; i++) {
        check(d[i].first_tile == first[i], "tile_counts", "first_tile", d[i].first_tile, first[i]);
        check(d[i].len == elems[i] && d[i].pad == kAccBf16 && d[i].put == 0xc0000000u && d[i].lin_off == 16u * i &&
                  d[i].rem_off == 32u * i,
              "tile_counts", "packing", d[i].put, 0xc0000000u);
    }
    if (failures == before) std::printf("PASS tile_counts\n");
}

}  // namespace

int main() {
    static_assert(sizeof(ocm_acc_params) == 32, "ocm_acc_params layout");
    element_rule();
    widen16();
    apply_host();
    validator();
    tile_counts();
    if (failures) {
        std::printf("%d failure(s)\n", failures);
        return 1;
    }
    std::printf("all accumulate tests passed\n");
    return 0;
}
