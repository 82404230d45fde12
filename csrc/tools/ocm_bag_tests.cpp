// The pooled lookup's shared header (ocm/bag.h) on the CPU: the functions the kernel and
// the host path call. Every rule of the validator, violated once and met just inside, the
// tile count and the plan, and the rule itself on crafted values: bag bounds, the order of
// the sum, two roundings and no fma, the mean's divisor and the narrowing at ties.
// Stand-alone: it links nothing of the library, so the build also makes an ASan + UBSan
// copy of it.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "ocm/bag.h"

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

constexpr uint64_t LB = 1 << 16, RB = 1 << 20;  // the halves the validator cases are checked against

// An op that is fine: 8 bags of 64-byte rows at the start of the local half, a table of 100
// rows, 40 ids at 4096, offsets at 8192, no weights.
ocm_bag_params good() {
    ocm_bag_params p{};
    p.local_offset = 0;
    p.remote_offset = 0;
    p.row_elems = 16;
    p.bags = 8;
    p.ids = 40;
    p.local_stride = 64;
    p.remote_stride = 64;
    p.remote_rows = 100;
    p.index_offset = 4096;
    p.offsets_offset = 8192;
    p.weights_offset = OCM_INDEX_NONE;
    p.index_type = OCM_INDEX_I32;
    p.dtype = OCM_ACC_F32;
    p.mode = OCM_BAG_SUM;
    return p;
}

int check(const ocm_bag_params &p, uint64_t lb, uint64_t rb, char *why, size_t n, uint64_t *moved = nullptr) {
    uint64_t m = 0;
    why[0] = 0;
    const int rc = bag_check_op(p, lb, rb, &m, why, n);
    if (moved) *moved = m;
    return rc;
}

void accepts(const char *what, const ocm_bag_params &p, uint64_t lb = LB, uint64_t rb = RB) {
    char why[256];
    CHECK(check(p, lb, rb, why, sizeof(why)) == 0, "%s: rejected (%s)", what, why);
}

void rejects(const char *what, const ocm_bag_params &p, const char *needle, uint64_t lb = LB, uint64_t rb = RB) {
    char why[256];
    const int rc = check(p, lb, rb, why, sizeof(why));
    CHECK(rc == -1 && std::strstr(why, needle), "%s: rc %d, why '%s' (wanted '%s')", what, rc, why, needle);
}

void test_validator() {
    char why[256];
    uint64_t moved = 0;
    ocm_bag_params p = good();
    CHECK(check(p, LB, RB, why, sizeof(why), &moved) == 0 && moved == 40 * 64, "the good op: %s, %llu", why,
          (unsigned long long)moved);
    // known index_type, dtype and mode; reserved; no weights with the mean
    for (uint32_t t : {0u, 3u, 7u}) {
        p = good(), p.index_type = t;
        rejects("index_type", p, "index_type");
    }
    p = good(), p.index_type = OCM_INDEX_I64;
    accepts("int64", p);
    for (uint32_t t : {0u, 4u}) {
        p = good(), p.dtype = t;
        rejects("dtype", p, "element type");
    }
    p = good(), p.mode = 2;
    rejects("mode", p, "mode 2");
    p = good(), p.mode = OCM_BAG_MEAN;
    accepts("mean", p);
    p.weights_offset = 12288;
    rejects("mean with weights", p, "weights");
    p.mode = OCM_BAG_SUM;
    accepts("sum with weights", p);
    p = good(), p.reserved = 1;
    rejects("reserved", p, "reserved");
    // row bytes: a positive multiple of 16 below 2^32
    p = good(), p.row_elems = 0;
    rejects("no elements", p, "multiple of 16");
    p = good(), p.row_elems = 6;
    rejects("24-byte rows", p, "multiple of 16");
    p = good(), p.dtype = OCM_ACC_BF16, p.row_elems = 12;
    rejects("24-byte bf16 rows", p, "multiple of 16");
    p.row_elems = 8;
    accepts("16-byte bf16 rows", p);
    p = good(), p.row_elems = 1ull << 30, p.local_stride = p.remote_stride = 1ull << 32;
    rejects("2^32-byte rows", p, "below 2^32");
    p.row_elems = (1ull << 30) - 4, p.bags = 1, p.remote_rows = 1;
    p.index_offset = 1ull << 33, p.offsets_offset = (1ull << 33) + 4096;  // behind the 4 GiB output row
    accepts("rows 16 bytes below 2^32", p, 1ull << 40, 1ull << 40);
    p = good(), p.row_elems = (1ull << 62) + 4;  // times 4 wraps to 16
    rejects("row bytes that wrap", p, "below 2^32");
    // counts below 2^32
    p = good(), p.bags = 1ull << 32;
    rejects("bags", p, "2^32");
    p = good(), p.ids = 1ull << 32;
    rejects("ids", p, "2^32");
    p = good(), p.remote_rows = 1ull << 32;
    rejects("remote rows", p, "remote table of");
    // offsets and strides multiples of 16
    p = good(), p.local_offset = 8;
    rejects("local offset", p, "local offset");
    p = good(), p.remote_offset = 24;
    rejects("remote offset", p, "remote offset");
    p = good(), p.local_stride = 72;
    rejects("local stride", p, "multiple of 16");
    p = good(), p.remote_stride = 68;
    rejects("remote stride", p, "multiple of 16");
    // rows do not overlap; each table's last row inside its half
    p = good(), p.local_stride = 48;
    rejects("local rows overlap", p, "local stride");
    p = good(), p.remote_stride = 48;
    rejects("remote rows overlap", p, "remote stride");
    p = good(), p.local_offset = LB - 8 * 64;
    p.index_offset = 0, p.offsets_offset = 4096;
    accepts("the output ends with its half", p);
    p.local_offset += 16;
    rejects("the output's last row leaves its half", p, "local table");
    p = good(), p.remote_offset = RB - 100 * 64;
    accepts("the table ends with its half", p);
    p.remote_offset += 16;
    rejects("the table's last row leaves its half", p, "remote table");
    p = good(), p.remote_rows = 0;
    accepts("a table of no rows", p);
    // sizes near 2^64: the overflow-free forms
    p = good(), p.remote_stride = 1ull << 62, p.remote_rows = 5;  // 4 * 2^62 wraps to 0
    rejects("remote stride that wraps", p, "remote table");
    p = good(), p.local_stride = 1ull << 63, p.bags = 3;
    rejects("local stride that wraps", p, "local table");
    p = good(), p.remote_offset = ~0ull - 15;  // offset + row bytes wraps
    rejects("remote offset that wraps", p, "remote table");
    p = good(), p.local_offset = ~0ull - 15, p.bags = 1;
    rejects("local offset that wraps", p, "local table");
    // the arrays: aligned, inside the local half, outside the output table
    p = good(), p.index_offset = 4098;
    rejects("ids alignment", p, "not a multiple");
    p = good(), p.index_type = OCM_INDEX_I64, p.offsets_offset = 8196;
    rejects("offsets alignment", p, "not a multiple");
    p = good(), p.weights_offset = 12290;
    rejects("weights alignment", p, "not a multiple");
    p = good(), p.index_offset = LB - 40 * 4;
    accepts("ids end with the half", p);
    p.index_offset += 4;
    rejects("ids leave the half", p, "ids index array");
    p = good(), p.offsets_offset = LB - 9 * 4;
    accepts("offsets end with the half", p);
    p.offsets_offset += 4;
    rejects("offsets leave the half (bags + 1 entries)", p, "offsets index array");
    p = good(), p.weights_offset = LB - 40 * 4 + 4;
    rejects("weights leave the half", p, "weights index array");
    p = good(), p.index_offset = ~0ull - 7, p.index_type = OCM_INDEX_I64;
    rejects("ids offset near 2^64", p, "ids index array");
    p = good(), p.index_offset = OCM_INDEX_NONE;
    rejects("no id array", p, "ids index");
    p = good(), p.index_offset = 8 * 64 - 4;
    rejects("ids overlap the output", p, "overlaps");
    p.index_offset = 8 * 64;
    accepts("ids right behind the output", p);
    p = good(), p.local_offset = 4096 + 40 * 4 + 12, p.local_offset &= ~15ull;  // 4256: the ids end at 4256
    accepts("the output right behind the ids", p);
    p.local_offset -= 16;
    rejects("the output overlaps the ids", p, "overlaps");
    p = good(), p.offsets_offset = 64;
    rejects("offsets overlap the output", p, "overlaps");
    p = good(), p.weights_offset = 448;
    rejects("weights overlap the output", p, "overlaps");
    // an op without bags does nothing, whatever else it says; one without ids writes zeros
    p = good(), p.bags = 0, p.index_type = 9, p.dtype = 9, p.local_offset = 3, p.ids = 1ull << 40;
    CHECK(check(p, LB, RB, why, sizeof(why), &moved) == 0 && moved == 0, "an op without bags: %s", why);
    p = good(), p.ids = 0, p.index_offset = 3, p.weights_offset = 5;  // neither array is read
    CHECK(check(p, LB, RB, why, sizeof(why), &moved) == 0 && moved == 0, "an op without ids: %s", why);
    // the natural way to say "no ids": no array at all, also over a table with fewer rows than the op has bags
    p = good(), p.ids = 0, p.index_offset = OCM_INDEX_NONE, p.remote_rows = 3;
    CHECK(check(p, LB, RB, why, sizeof(why), &moved) == 0 && moved == 0, "an op without ids and without an id array: %s", why);
    p.remote_rows = 0;
    CHECK(check(p, LB, RB, why, sizeof(why), &moved) == 0, "... over a table of no rows: %s", why);
    const XferBagOp o = bag_op(p);
    CHECK(o.bags == 8 && o.ids == 0 && o.w_off == OCM_INDEX_NONE, "descriptor of an op without ids");
    if (!failures) std::printf("PASS validator\n");
}

void test_plan() {
    const int before = failures;
    CHECK(bag_tiles_per_row(16) == 1 && bag_tiles_per_row(1024) == 1 && bag_tiles_per_row(1040) == 2 &&
              bag_tiles_per_row(4112) == 5 && bag_tiles_per_row((1ull << 32) - 16) == (1ull << 22),
          "tiles per row");
    ocm_bag_params p = good();
    std::vector<XferBagOp> ops;
    const uint64_t rows[] = {4, 0, 256, 260, 1028, 0};  // elements of fp32 rows; 0: an op without bags
    const uint64_t bags[] = {1, 0, 37, 2, 3, 0};
    uint64_t want = 0;
    std::vector<uint64_t> first;
    for (int i = 0; i < 6; i++) {
        p.row_elems = rows[i] ? rows[i] : 4;
        p.bags = bags[i];
        ops.push_back(bag_op(p));
        first.push_back(want);
        want += bags[i] * bag_tiles_per_row(4 * p.row_elems);
    }
    const uint64_t total = xfer_bag_plan(ops.data(), (uint32_t)ops.size(), kBagTileShift);
    CHECK(total == want && total == 1 + 37 + 2 * 2 + 3 * 5, "total tiles %llu", (unsigned long long)total);
    for (size_t i = 0; i < ops.size(); i++) {
        CHECK(ops[i].first_tile == first[i], "first tile of op %zu", i);
        CHECK(bag_tile_count(ops[i]) == bags[i] * ops[i].tiles_per_row, "tile count of op %zu", i);
    }
    // the walk: from any first tile, list_enter_op and list_locate find the op, the bag and the piece
    for (uint64_t t = 0; t < total; t++) {
        uint32_t i = 0;
        const uint64_t next = list_enter_op(ops.data(), (uint32_t)ops.size(), t, &i);
        uint64_t b, k;
        list_locate(ops[i].tiles_per_row, t - ops[i].first_tile, &b, &k);
        CHECK(ops[i].bags != 0 && t >= ops[i].first_tile && t < next && b < ops[i].bags && k < ops[i].tiles_per_row,
              "tile %llu: op %u bag %llu piece %llu", (unsigned long long)t, i, (unsigned long long)b, (unsigned long long)k);
        CHECK((k << kBagTileShift) < ops[i].row_bytes, "tile %llu: piece past the row", (unsigned long long)t);
    }
    // the wave table of a grid: every wave starts in the op of its first tile
    std::vector<uint32_t> wave_op(3 * kListWaves);
    list_wave_ops(ops.data(), (uint32_t)ops.size(), total, 3, wave_op.data());
    for (uint32_t w = 0; w < 3 * kListWaves; w++) {
        uint64_t t0, t1;
        list_wave_range(w, 3, total, &t0, &t1);
        if (t0 >= t1) continue;
        uint32_t i = wave_op[w];
        list_enter_op(ops.data(), (uint32_t)ops.size(), t0, &i);
        CHECK(ops[i].first_tile <= t0 && t0 < ops[i].first_tile + bag_tile_count(ops[i]), "wave %u starts in op %u", w, i);
    }
    if (failures == before) std::printf("PASS plan\n");
}

float f32(uint32_t bits) { return acc_bits_float(bits); }

void test_rule() {
    const int before = failures;
    uint32_t lo, hi;
    bag_bounds(2, 5, 10, &lo, &hi);
    CHECK(lo == 2 && hi == 5, "bounds inside");
    bag_bounds(5, 20, 10, &lo, &hi);
    CHECK(lo == 5 && hi == 10, "an offset above ids is clamped");
    bag_bounds(7, 3, 10, &lo, &hi);
    CHECK(lo == 7 && hi == 7, "a decreasing pair is an empty bag");
    bag_bounds(indexed_widen32(0xffffffffu), 4, 10, &lo, &hi);  // -1 as int32: 2^64 - 1
    CHECK(lo == 10 && hi == 10, "a negative offset is past the array");
    bag_bounds(0, 0, 0, &lo, &hi);
    CHECK(lo == 0 && hi == 0, "no ids");
    // the order of the sum: 2^25, 1, -2^25, 1 in order is 1; reversed it is 0
    const float xs[4] = {33554432.0f, 1.0f, -33554432.0f, 1.0f};
    float acc = 0.0f, rev = 0.0f;
    for (int i = 0; i < 4; i++) bag_add_row_host(&acc, &xs[i], 1, kAccF32, 1.0f);
    for (int i = 3; i >= 0; i--) bag_add_row_host(&rev, &xs[i], 1, kAccF32, 1.0f);
    CHECK(acc == 1.0f && rev == 0.0f, "in-order sum %g, reversed %g", acc, rev);
    // two roundings: w * x rounds away the bit an fma would keep
    const float w = f32(0x3f800001u), x = f32(0x3f800001u);  // (1 + 2^-23)^2 = 1 + 2^-22 + 2^-46
    acc = -f32(0x3f800002u);                                  // -(1 + 2^-22)
    const float fused = std::fmaf(w, x, acc);
    bag_add_row_host(&acc, &x, 1, kAccF32, w);
    CHECK(acc == 0.0f && fused == f32(0x28800000u), "two roundings give %a, an fma %a", acc, fused);
    // 16-bit rows widen exactly
    const uint16_t hb[2] = {0x3f80, 0xc000}, hf[2] = {0x3c00, 0x0001};  // bf16 1, -2; fp16 1, 2^-24
    float a2[2] = {0.0f, 0.0f};
    bag_add_row_host(a2, hb, 2, kAccBf16, 2.0f);
    CHECK(a2[0] == 2.0f && a2[1] == -4.0f, "bf16 rows");
    a2[0] = a2[1] = 0.0f;
    bag_add_row_host(a2, hf, 2, kAccFp16, 1.0f);
    CHECK(a2[0] == 1.0f && a2[1] == 5.9604644775390625e-8f, "fp16 rows");
    // the mean: one division by hi - lo; no division for an empty bag
    const float sums[2] = {1.0f, 10.0f};
    float out[2];
    bag_finish_host(sums, out, 2, kAccF32, OCM_BAG_MEAN, 3);
    CHECK(out[0] == 1.0f / 3.0f && out[1] == 10.0f / 3.0f, "mean of 3");
    bag_finish_host(sums, out, 2, kAccF32, OCM_BAG_MEAN, 0);
    CHECK(out[0] == 1.0f && out[1] == 10.0f, "mean of an empty bag");
    bag_finish_host(sums, out, 2, kAccF32, OCM_BAG_SUM, 7);
    CHECK(out[0] == 1.0f && out[1] == 10.0f, "sum");
    // narrowing, to nearest even: bf16 ties at 2^-8, fp16 ties at 2^-11
    CHECK(bag_narrow16(f32(0x3f808000u), true) == 0x3f80 && bag_narrow16(f32(0x3f818000u), true) == 0x3f82 &&
              bag_narrow16(f32(0x3f808001u), true) == 0x3f81 && bag_narrow16(f32(0xbf818000u), true) == 0xbf82,
          "bf16 ties");
    CHECK(bag_narrow16(f32(0x7f7fffffu), true) == 0x7f80 && (bag_narrow16(f32(0x7fc00001u), true) & 0x7fff) > 0x7f80, "bf16 overflow and NaN");
    CHECK(bag_narrow16(1.0f + 1.0f / 2048, false) == 0x3c00 && bag_narrow16(1.0f + 3.0f / 2048, false) == 0x3c02 &&
              bag_narrow16(f32(0x3f801001u), false) == 0x3c01 && bag_narrow16(-1.0f - 3.0f / 2048, false) == 0xbc02,
          "fp16 ties");
    CHECK(bag_narrow16(65504.0f, false) == 0x7bff && bag_narrow16(65519.0f, false) == 0x7bff && bag_narrow16(65520.0f, false) == 0x7c00 &&
              bag_narrow16(-1e9f, false) == 0xfc00 && (bag_narrow16(f32(0x7fc00000u), false) & 0x7fff) > 0x7c00,
          "fp16 overflow and NaN");
    // fp16 subnormals: multiples of 2^-24, ties to even, and the step to the smallest normal
    const float q = 5.9604644775390625e-8f;  // 2^-24
    CHECK(bag_narrow16(q, false) == 1 && bag_narrow16(0.5f * q, false) == 0 && bag_narrow16(1.5f * q, false) == 2 &&
              bag_narrow16(0.75f * q, false) == 1 && bag_narrow16(1023.5f * q, false) == 0x400 &&
              bag_narrow16(1024.0f * q, false) == 0x400 && bag_narrow16(-2.5f * q, false) == 0x8002 && bag_narrow16(0.0f, false) == 0 &&
              bag_narrow16(-0.0f, false) == 0x8000,
          "fp16 subnormals");
    // every fp16 value survives widening and narrowing
    for (uint32_t h = 0; h < 0x10000; h++) {
        if ((h & 0x7c00) == 0x7c00 && (h & 0x3ff)) continue;  // NaNs: some NaN
        CHECK(bag_narrow16(acc_widen16(h, false), false) == h, "fp16 0x%04x round trip", h);
        CHECK(bag_narrow16(acc_widen16(h, true), true) == h, "bf16 0x%04x round trip", h);
    }
    // a bag with a 16-bit output that lands on a tie
    const uint16_t rows16[2] = {0x3f80, 0x3b80};  // bf16 1 and 2^-8: the sum ties between 1 and 1 + 2^-7
    float a1 = 0.0f;
    uint16_t o16;
    bag_add_row_host(&a1, &rows16[0], 1, kAccBf16, 1.0f);
    bag_add_row_host(&a1, &rows16[1], 1, kAccBf16, 1.0f);
    bag_finish_host(&a1, &o16, 1, kAccBf16, OCM_BAG_SUM, 2);
    CHECK(a1 == 1.00390625f && o16 == 0x3f80, "a bf16 sum on a tie: 0x%04x", o16);
    if (failures == before) std::printf("PASS rule\n");
}

}  // namespace

int main() {
    test_validator();
    test_plan();
    test_rule();
    if (failures) {
        std::printf("%d failure(s)\n", failures);
        return 1;
    }
    std::printf("all bag tests passed\n");
    return 0;
}
