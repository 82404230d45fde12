// The MXFP4 host codec (ocm/mx4.h) on fixed groups with hard-coded expected bytes (taken
// from the torch oracle, oncilla_amd/ops/quant.py), the exponent and code rules the kernel
// shares with it, and where the strided kernel finds an MXFP4 tile (ocm/quant_strided.h).
// Stand-alone: it links nothing of the library, so the build also makes an ASan + UBSan
// copy of it.
#include <cstdio>
#include <cstring>
#include <vector>

#include "ocm/mx4.h"
#include "ocm/quant_strided.h"

using namespace ocm;

namespace {

int failures = 0;

struct Case {
    const char *name;
    uint32_t dtype;
    uint16_t src[8];   // elements 0..7 of the group, the other 24 are +0
    uint8_t codes[4];  // their code bytes, the other 12 are 0
    uint8_t scale;
    uint16_t dec[8];
};

const Case kCases[] = {
    // an all-zero group with a -0.0
    {"zero bf16", kMx8Bf16, {0x0000, 0x8000}, {0x80}, 127, {0x0000, 0x8000}},
    {"zero fp16", kMx8Fp16, {0x0000, 0x8000}, {0x80}, 127, {0x0000, 0x8000}},
    // amax = 6 = 0.75 * 2^3: m == 0.75 exactly, e = 0; with 1, -0.5, 3, -6 and the ties 0.25, 0.75, 5
    {"m075 bf16", kMx8Bf16, {0x40c0, 0x3f80, 0xbf00, 0x4040, 0xc0c0, 0x3e80, 0x3f40, 0x40a0}, {0x27, 0x59, 0x0f, 0x62}, 127,
     {0x40c0, 0x3f80, 0xbf00, 0x4040, 0xc0c0, 0x0000, 0x3f80, 0x4080}},
    {"m075 fp16", kMx8Fp16, {0x4600, 0x3c00, 0xb800, 0x4200, 0xc600, 0x3400, 0x3a00, 0x4500}, {0x27, 0x59, 0x0f, 0x62}, 127,
     {0x4600, 0x3c00, 0xb800, 0x4200, 0xc600, 0x0000, 0x3c00, 0x4400}},
    // the next representable amax above it: one exponent up, scaled to just over 3
    {"m075+ bf16", kMx8Bf16, {0x40c1, 0x3f80, 0xbf00, 0x4040, 0xc0c0, 0x3f00, 0x3fc0, 0x40a0}, {0x15, 0x38, 0x0d, 0x42}, 128,
     {0x40c0, 0x3f80, 0x8000, 0x4040, 0xc0c0, 0x0000, 0x4000, 0x4080}},
    {"m075+ fp16", kMx8Fp16, {0x4601, 0x3c00, 0xb800, 0x4200, 0xc600, 0x3800, 0x3e00, 0x4500}, {0x15, 0x38, 0x0d, 0x42}, 128,
     {0x4600, 0x3c00, 0x8000, 0x4200, 0xc600, 0x0000, 0x4000, 0x4400}},
    // every tie in a group whose amax is 6: 0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5 go to the even codes
    {"ties bf16", kMx8Bf16, {0x40c0, 0x3e80, 0x3f40, 0x3fa0, 0x3fe0, 0x4020, 0x4060, 0x40a0}, {0x07, 0x22, 0x44, 0x66}, 127,
     {0x40c0, 0x0000, 0x3f80, 0x3f80, 0x4000, 0x4000, 0x4080, 0x4080}},
    {"ties fp16", kMx8Fp16, {0x4600, 0x3400, 0x3a00, 0x3d00, 0x3f00, 0x4100, 0x4300, 0x4500}, {0x07, 0x22, 0x44, 0x66}, 127,
     {0x4600, 0x0000, 0x3c00, 0x3c00, 0x4000, 0x4000, 0x4400, 0x4400}},
    {"ties- bf16", kMx8Bf16, {0xc0c0, 0xbe80, 0xbf40, 0xbfa0, 0xbfe0, 0xc020, 0xc060, 0xc0a0}, {0x8f, 0xaa, 0xcc, 0xee}, 127,
     {0xc0c0, 0x8000, 0xbf80, 0xbf80, 0xc000, 0xc000, 0xc080, 0xc080}},
    {"ties- fp16", kMx8Fp16, {0xc600, 0xb400, 0xba00, 0xbd00, 0xbf00, 0xc100, 0xc300, 0xc500}, {0x8f, 0xaa, 0xcc, 0xee}, 127,
     {0xc600, 0x8000, 0xbc00, 0xbc00, 0xc000, 0xc000, 0xc400, 0xc400}},
    // values that round to 0 (keeping their sign) and to 0.5
    {"small bf16", kMx8Bf16, {0x40c0, 0x3e00, 0xbe00, 0x3e81, 0x3e9a, 0x3f33, 0x3f43, 0xbe76}, {0x07, 0x18, 0x11, 0x82}, 127,
     {0x40c0, 0x0000, 0x8000, 0x3f00, 0x3f00, 0x3f00, 0x3f80, 0x8000}},
    {"small fp16", kMx8Fp16, {0x4600, 0x3000, 0xb000, 0x3400, 0x34cd, 0x399a, 0x3a14, 0xb3ae}, {0x07, 0x08, 0x11, 0x82}, 127,
     {0x4600, 0x0000, 0x8000, 0x0000, 0x3800, 0x3800, 0x3c00, 0x8000}},
    // the smallest subnormal as amax: bf16's wants e = -135 and gets -127, its code rounds to 0
    {"clamp bf16", kMx8Bf16, {0x0001, 0x8001}, {0x80}, 0, {0x0000, 0x8000}},
    {"clamp fp16", kMx8Fp16, {0x0001, 0x8001}, {0xe6}, 101, {0x0001, 0x8001}},
    // the largest finite value encodes as 4 * 2^e (RNE of 3.98 and 3.99) and decodes past the range
    {"largest bf16", kMx8Bf16, {0x7f7f, 0xff7f, 0x7f00, 0x4000}, {0xe6, 0x04}, 253, {0x7f80, 0xff80, 0x7f00, 0x0000}},
    {"largest fp16", kMx8Fp16, {0x7bff, 0xfbff, 0x63d0, 0x4000}, {0xe6, 0x00}, 141, {0x7c00, 0xfc00, 0x0000, 0x0000}},
};

void check(bool ok, const char *name, const char *what, long i, unsigned got, unsigned want) {
    if (ok) return;
    failures++;
    std::printf("FAIL %s: %s[%ld] = 0x%x, expected 0x%x\n", name, what, i, got, want);
}

void run_case(const Case &c) {
    uint16_t src[kMx8Group] = {};
    std::memcpy(src, c.src, sizeof(c.src));
    std::vector<uint8_t> rec(mx4_record_bytes(kMx8Group) + 4, 0xaa);
    mx4_encode(src, kMx8Group, c.dtype, rec.data());
    for (int i = 0; i < 16; i++) check(rec[i] == (i < 4 ? c.codes[i] : 0), c.name, "code byte", i, rec[i], i < 4 ? c.codes[i] : 0);
    check(rec[16] == c.scale, c.name, "scale", 0, rec[16], c.scale);
    for (int i = 17; i < 21; i++) check(rec[i] == 0xaa, c.name, "guard", i, rec[i], 0xaa);
    std::vector<uint16_t> out(kMx8Group, 0xaaaa);
    mx4_decode(rec.data(), kMx8Group, c.dtype, out.data());
    for (int i = 0; i < kMx8Group; i++) check(out[i] == (i < 8 ? c.dec[i] : 0), c.name, "decoded", i, out[i], i < 8 ? c.dec[i] : 0);
}

// The exponent rule at every binade of fp32, subnormal ones included: at m == 0.75 the
// scaled maximum is exactly 6, at the next value above it e is one more, and in between the
// scaled maximum lies in (3, 6] unless e was clamped. Then every finite bf16 as a group's amax.
void sweep_amax() {
    for (int ex = -148; ex <= 128; ex++) {  // amax = m * 2^ex
        const float lo = std::ldexp(0.5f, ex), mid = std::ldexp(0.75f, ex);
        const float up = mx8_bits_float(mx8_float_bits(mid) + 1), top = mx8_bits_float(mx8_float_bits(std::ldexp(0.5f, ex + 1)) - 1);
        const int want_lo = ex - 3 < -127 ? -127 : ex - 3, want_hi = ex - 2 < -127 ? -127 : ex - 2 > 127 ? 127 : ex - 2;
        check(mx4_group_exp(mx8_float_bits(lo)) == want_lo, "amax", "e at m = 0.5, ex", ex, mx4_group_exp(mx8_float_bits(lo)), want_lo);
        if (ex >= -147) {  // below that m = 0.75 is no fp32 value
            check(mx4_group_exp(mx8_float_bits(mid)) == want_lo, "amax", "e at m = 0.75, ex", ex, mx4_group_exp(mx8_float_bits(mid)), want_lo);
            if (ex - 3 >= -127) check(std::ldexp(mid, -want_lo) == 6.0f, "amax", "scaled m = 0.75, ex", ex, 0, 6);
        }
        if (ex >= -125 && ex < 128) {  // normal numbers: the next value above m = 0.75 is in the same binade
            check(mx4_group_exp(mx8_float_bits(up)) == want_hi, "amax", "e above m = 0.75, ex", ex, mx4_group_exp(mx8_float_bits(up)), want_hi);
            check(mx4_group_exp(mx8_float_bits(top)) == want_hi, "amax", "e below m = 1, ex", ex, mx4_group_exp(mx8_float_bits(top)), want_hi);
            check(std::ldexp(up, -want_hi) > 3.0f && std::ldexp(top, -want_hi) < 6.0f, "amax", "scaled above m = 0.75, ex", ex, 0, 0);
        }
    }
    check(mx4_group_exp(0) == 0, "amax", "e of zero", 0, mx4_group_exp(0), 0);
    for (uint32_t h = 1; h < 0x7f80u; h++) {
        uint16_t src[kMx8Group] = {};
        src[5] = (uint16_t)h;
        src[6] = (uint16_t)(h | 0x8000u);
        uint8_t rec[17];
        mx4_encode(src, kMx8Group, kMx8Bf16, rec);
        const int e = (int)rec[16] - kMx8ScaleBias;
        const double scaled = std::ldexp((double)mx8_bf16_to_f32((uint16_t)h), -e);
        const bool ok = e == -127 ? scaled <= 6.0 : (scaled > 3.0 && scaled <= 6.0);
        check(ok, "sweep", "scaled amax out of (3, 6] at bf16", h, (unsigned)scaled, 6);
        check(rec[16] != 255, "sweep", "scale", h, rec[16], 254);
        const unsigned lo = rec[2] >> 4, hi = rec[3] & 15u;  // elements 5 and 6
        check(hi == (lo | 8u) && (e == -127 || (lo & 7u) >= 5u), "sweep", "code", h, lo, hi);
        // decoded, before it is narrowed, within half a code step of the amax: the steps up there are 1 and 2
        const double back = std::ldexp((double)mx8_bits_float(mx4_e2m1_to_f32_bits(lo)), e);
        check(std::fabs(std::ldexp(back, -e) - scaled) <= (scaled > 4.0 ? 1.0 : 0.5), "sweep", "round trip", h, lo, 0);
    }
}

// All 16 codes decode to their values and encode again; every tie point goes to the even
// code, the value just below it to the code below and the value just above to the code above,
// in both signs; and what lies past 6 saturates.
void sweep_codes() {
    const float values[8] = {0.0f, 0.5f, 1.0f, 1.5f, 2.0f, 3.0f, 4.0f, 6.0f};
    for (uint32_t c = 0; c < 16; c++) {
        const float v = mx8_bits_float(mx4_e2m1_to_f32_bits(c));
        const float want = (c & 8u) ? -values[c & 7u] : values[c & 7u];
        check(mx8_float_bits(v) == mx8_float_bits(want), "e2m1", "value", c, mx8_float_bits(v), mx8_float_bits(want));
        check(mx4_f32_to_e2m1(mx8_float_bits(v)) == c, "e2m1", "round trip", c, mx4_f32_to_e2m1(mx8_float_bits(v)), c);
    }
    for (uint32_t m = 0; m < 7; m++) {
        const float tie = 0.5f * (values[m] + values[m + 1]);
        const uint32_t even = (m & 1u) ? m + 1 : m, tb = mx8_float_bits(tie);
        for (uint32_t sign = 0; sign < 2; sign++) {
            const uint32_t sb = sign << 31, sc = sign << 3;
            check(mx4_f32_to_e2m1(sb | tb) == (sc | even), "e2m1", "tie", m, mx4_f32_to_e2m1(sb | tb), sc | even);
            check(mx4_f32_to_e2m1(sb | (tb - 1)) == (sc | m), "e2m1", "below tie", m, mx4_f32_to_e2m1(sb | (tb - 1)), sc | m);
            check(mx4_f32_to_e2m1(sb | (tb + 1)) == (sc | (m + 1)), "e2m1", "above tie", m, mx4_f32_to_e2m1(sb | (tb + 1)), sc | (m + 1));
        }
    }
    check(mx4_f32_to_e2m1(mx8_float_bits(6.5f)) == 7 && mx4_f32_to_e2m1(mx8_float_bits(-1e30f)) == 15, "e2m1", "saturate", 0, 0, 7);
    check(mx4_f32_to_e2m1(0x7f800000u) == 7 && mx4_f32_to_e2m1(0xffc00000u) == 15, "e2m1", "inf and nan", 0, 0, 7);
    check(mx4_f32_to_e2m1(1) == 0 && mx4_f32_to_e2m1(0x80000001u) == 8, "e2m1", "tiny", 0, 0, 0);
}

// A record of several groups: element 2i in the low nibble of code byte i, element 2i + 1 in
// the high one, the scale bytes behind all code bytes, nothing written past the end.
void record_layout() {
    const uint64_t n = 5 * kMx8Group;
    std::vector<uint16_t> src(n);
    for (uint64_t i = 0; i < n; i++) src[i] = mx8_f32_to_bf16((float)((int)(i * 37 % 101) - 50) * (float)(1 + i / 32));
    const size_t rb = mx4_record_bytes(n);
    check(rb == 85 && quant_record_bytes(n, kQuantFmtMx4 | kMx8Bf16) == 85 && quant_record_bytes(n, kMx8Bf16) == 165, "layout",
          "record bytes", 0, (unsigned)rb, 85);
    std::vector<uint8_t> rec(rb + 8, 0x5a);
    mx4_encode(src.data(), n, kMx8Bf16, rec.data());
    for (int i = 0; i < 8; i++) check(rec[rb + i] == 0x5a, "layout", "guard", i, rec[rb + i], 0x5a);
    for (uint64_t g = 0; g < 5; g++) {
        uint8_t one[17];
        mx4_encode(src.data() + g * kMx8Group, kMx8Group, kMx8Bf16, one);
        check(std::memcmp(one, rec.data() + g * 16, 16) == 0, "layout", "codes of group", (long)g, 0, 0);
        check(one[16] == rec[n / 2 + g], "layout", "scale of group", (long)g, rec[n / 2 + g], one[16]);
    }
    // nibble order: only element 1 of group 0 and element 32 + 6 of group 1 are not zero
    std::vector<uint16_t> two(2 * kMx8Group, 0);
    two[1] = mx8_f32_to_bf16(6.0f);
    two[kMx8Group + 6] = mx8_f32_to_bf16(-1.0f);
    std::vector<uint8_t> r2(mx4_record_bytes(two.size()));
    mx4_encode(two.data(), two.size(), kMx8Bf16, r2.data());
    for (size_t i = 0; i < 32; i++) {
        const uint8_t want = i == 0 ? 0x70 : i == 19 ? 0x0e : 0;  // 6: code 7, high nibble; -1 = -4 * 2^-2: code 14, low nibble
        check(r2[i] == want, "layout", "nibble", (long)i, r2[i], want);
    }
    check(r2[32] == 127 && r2[33] == 125, "layout", "scales behind the codes", 0, r2[33], 125);
    std::vector<uint16_t> back(two.size());
    mx4_decode(r2.data(), two.size(), kMx8Bf16, back.data());
    check(back == two, "layout", "decoded", 0, 0, 0);
    // the dtype word
    char why[96];
    check(quant_check_dtype(kMx8Bf16, why, sizeof(why)) == 0 && quant_check_dtype(kQuantFmtMx4 | kMx8Fp16, why, sizeof(why)) == 0,
          "layout", "dtype word", 0, 0, 0);
    check(quant_check_dtype(7, why, sizeof(why)) == -1 && std::strcmp(why, "unknown element type 7") == 0, "layout", "dtype 7", 0, 0, 0);
    check(quant_check_dtype(0x201, why, sizeof(why)) == -1 && std::strstr(why, "format 0x200"), "layout", "format", 0, 0, 0);
    check(quant_check_dtype(0x10101, why, sizeof(why)) == -1 && std::strstr(why, "0x10101"), "layout", "stray bits", 0, 0, 0);
}

// Where the strided kernel finds the tiles of MXFP4 rows: piece k of a row is the tile k of
// the row's plain op (codes at rem_off + e0 / 2, scale bytes at rem_off + len / 2 + e0 / 32),
// whole 16-byte vectors, inside the row's record, and rows' records do not meet.
void strided_tile_location() {
    for (uint32_t row_elems : {32u, 2016u, 2048u, 2080u, 4128u, 10240u}) {
        ocm_quant_strided_params p{};
        p.local_offset = 64;
        p.remote_offset = 96;
        p.row_elems = row_elems;
        p.rows = 3;
        p.local_stride = 2 * row_elems + 32;
        p.remote_stride = (mx4_record_bytes(row_elems) + 31) / 32 * 32 + 64;
        p.op_flag = 1;
        p.dtype = OCM_QUANT_FP16 | OCM_QUANT_MXFP4;
        uint64_t src = 0, wire = 0;
        char why[192];
        const int rc = quant_strided_check_op(p, 1 << 20, 1 << 20, &src, &wire, why, sizeof(why));
        check(rc == 0 && src == 3ull * 2 * row_elems && wire == 3 * mx4_record_bytes(row_elems), "strided", "check_op", row_elems,
              (unsigned)wire, (unsigned)(3 * mx4_record_bytes(row_elems)));
        XferQuantStridedOp op = quant_strided_op(p);
        const uint64_t total = xfer_quant_strided_plan(&op, 1, kQuantTileShift);
        check(total == 3 * quant_tile_count(row_elems), "strided", "tiles", row_elems, (unsigned)total, 0);
        const uint32_t cs = quant_code_shift(op.dtype);
        check(cs == 1 && quant_code_shift(OCM_QUANT_FP16) == 0, "strided", "code shift", row_elems, cs, 1);
        uint64_t elems_seen = 0;
        for (uint64_t t = 0; t < total; t++) {
            uint64_t row;
            uint32_t k;
            list_locate(op.tiles_per_row, t, &row, &k);
            const QuantTileLoc q = quant_strided_tile(op, row, k, cs);
            const uint64_t rec = p.remote_offset + row * p.remote_stride, e0 = (uint64_t)k << kQuantTileShift;
            check(q.lin_off == p.local_offset + row * p.local_stride + 2 * e0, "strided", "elements of tile", (long)t, (unsigned)q.lin_off, 0);
            check(q.codes == rec + e0 / 2, "strided", "codes of tile", (long)t, (unsigned)q.codes, (unsigned)(rec + e0 / 2));
            check(q.scales == rec + row_elems / 2 + e0 / 32, "strided", "scale bytes of tile", (long)t, (unsigned)q.scales, 0);
            check(q.ne > 0 && q.ne % 32 == 0 && q.ne == (row_elems - e0 < kQuantTileElems ? row_elems - e0 : kQuantTileElems), "strided",
                  "elements in tile", (long)t, q.ne, 0);
            check(q.lin_off % 16 == 0 && q.codes % 16 == 0 && q.scales % 16 == 0, "strided", "unaligned vectors of tile", (long)t, 0, 0);
            check(q.codes + q.ne / 2 <= rec + row_elems / 2 && q.scales + q.ne / 32 <= rec + mx4_record_bytes(row_elems) &&
                      rec + mx4_record_bytes(row_elems) <= rec + p.remote_stride,
                  "strided", "tile leaves its record", (long)t, 0, 0);
            elems_seen += q.ne;
        }
        check(elems_seen == 3ull * row_elems, "strided", "elements covered", row_elems, (unsigned)elems_seen, 3 * row_elems);
        // one byte less of stride and rows would overlap
        p.remote_stride = (mx4_record_bytes(row_elems) + 31) / 32 * 32 - 32;
        if (p.remote_stride < mx4_record_bytes(row_elems))
            check(quant_strided_check_op(p, 1 << 20, 1 << 20, &src, &wire, why, sizeof(why)) == -1 && std::strstr(why, "remote stride"),
                  "strided", "small stride accepted", row_elems, 0, 0);
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
    sweep_codes();
    if (failures == before) std::printf("PASS e2m1_codes\n");
    before = failures;
    record_layout();
    if (failures == before) std::printf("PASS record_layout\n");
    before = failures;
    strided_tile_location();
    if (failures == before) std::printf("PASS strided_tile_location\n");
    std::printf("%s (%d failures)\n", failures ? "FAILED" : "OK", failures);
    return failures ? 1 : 0;
}
