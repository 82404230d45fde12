// The row-sparse fused Adam's shared header (ocm/adam_rows.h): the validator, every refusal
// beside its nearest accepted neighbour; the hyper-parameter rule; the bounds rule; and the
// walk of the kernel replayed on the host, wave by wave, from the header's launch shape,
// wave ranges and locate function. Stand-alone: it sees the HIP headers through ocm/optim.h
// and links nothing of HIP, so the build also makes an ASan + UBSan copy of it.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "ocm/adam_rows.h"

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

constexpr uint64_t kHalf = 1ull << 20;

// 37 rows of 64 elements: fp32 rows of 256 bytes at stride 272; the table, exp_avg, exp_avg_sq
// and the master one behind the other with 16 bytes between them.
constexpr uint64_t kRows = 37, kDim = 64, kStride = 272;
constexpr uint64_t kSpan = (kRows - 1) * kStride + 4 * kDim;  // bytes from a table's first to its last

ocm_adam_rows good(bool bf16) {
    ocm_adam_rows d{};
    d.rows = 5;
    d.dim = kDim;
    d.table_rows = kRows;
    d.index_type = OCM_INDEX_I64;
    d.bf16 = bf16;
    d.table_off = 0;
    d.table_stride = kStride;
    d.m_off = kSpan + 16;
    d.m_stride = kStride;
    d.v_off = 2 * (kSpan + 16);
    d.v_stride = kStride;
    d.w_off = 3 * (kSpan + 16);
    d.w_stride = kStride;
    d.g_stride = kDim;
    return d;
}

bool accepts(const ocm_adam_rows &d, bool same = true, uint64_t table_bytes = kHalf, uint64_t state_bytes = kHalf) {
    char why[256] = "";
    const int rc = adam_rows_check(d, table_bytes, state_bytes, same, why, sizeof(why));
    if (rc != 0 && why[0] == 0) CHECK(false, "a refusal without a reason");
    return rc == 0;
}

#define ACCEPT(...) CHECK(accepts(__VA_ARGS__), "refused: %s", #__VA_ARGS__)
#define REFUSE(...) CHECK(!accepts(__VA_ARGS__), "accepted: %s", #__VA_ARGS__)

template <class F>
ocm_adam_rows with(ocm_adam_rows d, F f) {
    f(d);
    return d;
}

void test_validator() {
    const int before = failures;
    for (int bf16 = 0; bf16 < 2; bf16++) {
        const ocm_adam_rows d = good(bf16 != 0);
        ACCEPT(d);
        ACCEPT(d, false);
        // dim
        REFUSE(with(d, [](ocm_adam_rows &x) { x.dim = 6; x.g_stride = 8; }));
        REFUSE(with(d, [](ocm_adam_rows &x) { x.dim = 0; }));
        REFUSE(with(d, [](ocm_adam_rows &x) { x.dim = 62; }));
        ACCEPT(with(d, [](ocm_adam_rows &x) { x.dim = 60; }));
        ACCEPT(with(d, [](ocm_adam_rows &x) { x.dim = 4; }));
        // index type
        ACCEPT(with(d, [](ocm_adam_rows &x) { x.index_type = OCM_INDEX_I32; }));
        REFUSE(with(d, [](ocm_adam_rows &x) { x.index_type = 0; }));
        REFUSE(with(d, [](ocm_adam_rows &x) { x.index_type = 3; }));
        REFUSE(with(d, [](ocm_adam_rows &x) { x.bf16 = 2; }));
        // counts
        ACCEPT(with(d, [](ocm_adam_rows &x) { x.rows = (1ull << 32) - 1; }));
        REFUSE(with(d, [](ocm_adam_rows &x) { x.rows = 1ull << 32; }));
        ACCEPT(with(d, [](ocm_adam_rows &x) { x.rows = 0; }));
        REFUSE(with(d, [](ocm_adam_rows &x) { x.table_rows = 1ull << 32; }));
        REFUSE(with(d, [](ocm_adam_rows &x) { x.table_rows = (1ull << 32) - 1; }));  // bounded, and does not fit
        REFUSE(with(d, [](ocm_adam_rows &x) { x.table_rows = ~0ull; }));
        // the gradient stride
        ACCEPT(with(d, [](ocm_adam_rows &x) { x.g_stride = kDim + 4; }));
        REFUSE(with(d, [](ocm_adam_rows &x) { x.g_stride = kDim + 2; }));
        REFUSE(with(d, [](ocm_adam_rows &x) { x.g_stride = kDim - 4; }));
        ACCEPT(with(d, [](ocm_adam_rows &x) { x.g_stride = 0; x.rows = 1; }));  // one row: the stride is not used
        ACCEPT(with(d, [](ocm_adam_rows &x) { x.g_stride = (1ull << 30) - 4; }));
        REFUSE(with(d, [](ocm_adam_rows &x) { x.g_stride = 1ull << 30; }));
        // alignment: 16 for fp32 tables, 8 for a bf16 table
        REFUSE(with(d, [](ocm_adam_rows &x) { x.m_off += 8; }));
        REFUSE(with(d, [](ocm_adam_rows &x) { x.v_off += 4; }));
        REFUSE(with(d, [](ocm_adam_rows &x) { x.m_stride += 8; }));
        REFUSE(with(d, [](ocm_adam_rows &x) { x.v_stride += 8; }));
        ACCEPT(with(d, [](ocm_adam_rows &x) { x.m_stride += 16; x.v_off += 36 * 16; x.w_off += 36 * 16; }));
        if (bf16) {
            REFUSE(with(d, [](ocm_adam_rows &x) { x.w_off += 8; }));
            REFUSE(with(d, [](ocm_adam_rows &x) { x.w_stride += 8; }));
            ACCEPT(with(d, [](ocm_adam_rows &x) { x.table_off = 8; }));
            REFUSE(with(d, [](ocm_adam_rows &x) { x.table_off = 4; }));
            ACCEPT(with(d, [](ocm_adam_rows &x) { x.table_stride = 2 * kDim + 8; }));
            REFUSE(with(d, [](ocm_adam_rows &x) { x.table_stride = 2 * kDim + 4; }));
        } else {
            // the master is not read for an fp32 table: whatever it says
            ACCEPT(with(d, [](ocm_adam_rows &x) { x.w_off = 3; x.w_stride = 1; }));
            REFUSE(with(d, [](ocm_adam_rows &x) { x.table_off = 8; }));
            REFUSE(with(d, [](ocm_adam_rows &x) { x.table_stride += 8; }));
        }
        // the stride against the row: exactly fitting, and 16 (8) bytes short
        const uint64_t trow = bf16 ? 2 * kDim : 4 * kDim, tal = bf16 ? 8 : 16;
        ACCEPT(with(d, [&](ocm_adam_rows &x) { x.table_stride = trow; }));
        REFUSE(with(d, [&](ocm_adam_rows &x) { x.table_stride = trow - tal; }));
        ACCEPT(with(d, [](ocm_adam_rows &x) { x.m_stride = 4 * kDim; }));
        REFUSE(with(d, [](ocm_adam_rows &x) { x.m_stride = 4 * kDim - 16; }));
        ACCEPT(with(d, [&](ocm_adam_rows &x) { x.table_stride = 0; x.table_rows = 1; }));  // one row: no stride
        REFUSE(with(d, [&](ocm_adam_rows &x) { x.table_stride = 0; x.table_rows = 2; }));
        // every table fits its half: ending at the last byte, and one vector beyond
        const uint64_t tspan = (kRows - 1) * kStride + trow;
        ACCEPT(with(d, [&](ocm_adam_rows &x) { x.table_off = kHalf - tspan; }), false);
        REFUSE(with(d, [&](ocm_adam_rows &x) { x.table_off = kHalf - tspan + tal; }), false);
        ACCEPT(d, false, tspan, kHalf);
        REFUSE(d, false, tspan - 1, kHalf);
        const uint64_t send = (bf16 ? d.w_off : d.v_off) + kSpan;  // the state's last byte, plus one
        ACCEPT(d, false, kHalf, send);
        REFUSE(d, false, kHalf, send - 1);
        ACCEPT(with(d, [&](ocm_adam_rows &x) { x.v_off = kHalf - kSpan; }), false);
        REFUSE(with(d, [&](ocm_adam_rows &x) { x.v_off = kHalf - kSpan + 16; }), false);
        // an offset exactly at the end holds no row; a table of no rows holds no byte
        REFUSE(with(d, [](ocm_adam_rows &x) { x.m_off = kHalf; }), false);
        ACCEPT(with(d, [](ocm_adam_rows &x) { x.m_off = kHalf; x.table_rows = 0; }), false);
        // offsets and strides near 2^64 must not wrap into the half
        REFUSE(with(d, [](ocm_adam_rows &x) { x.m_off = ~0ull - 15; }), false);
        REFUSE(with(d, [](ocm_adam_rows &x) { x.m_stride = ~0ull - 15; }), false);
        REFUSE(with(d, [](ocm_adam_rows &x) { x.table_stride = (1ull << 63); }), false);
        // overlap in a shared pair: touching is fine, one vector inside is not; another pair: other memory
        ACCEPT(with(d, [&](ocm_adam_rows &x) { x.m_off = tspan + (tal == 8 && tspan % 16 ? 8 : 0); }));
        REFUSE(with(d, [&](ocm_adam_rows &x) { x.m_off = (tspan - 16) / 16 * 16; }));
        ACCEPT(with(d, [&](ocm_adam_rows &x) { x.m_off = (tspan - 16) / 16 * 16; }), false);
        REFUSE(with(d, [](ocm_adam_rows &x) { x.m_off = 0; }));
        ACCEPT(with(d, [](ocm_adam_rows &x) { x.m_off = 0; }), false);
        // the state tables keep clear of each other whichever pair the table is in
        ACCEPT(with(d, [](ocm_adam_rows &x) { x.v_off = x.m_off + kSpan; }), false);
        REFUSE(with(d, [](ocm_adam_rows &x) { x.v_off = x.m_off + kSpan - 16; }), false);
        REFUSE(with(d, [](ocm_adam_rows &x) { x.v_off = x.m_off; }), false);
        REFUSE(with(d, [](ocm_adam_rows &x) { x.m_off = x.v_off + kSpan - 16; x.w_off = 5 * kSpan; }), false);
        if (bf16) {
            ACCEPT(with(d, [](ocm_adam_rows &x) { x.w_off = x.v_off + kSpan; }));
            REFUSE(with(d, [](ocm_adam_rows &x) { x.w_off = x.v_off + kSpan - 16; }));
            REFUSE(with(d, [](ocm_adam_rows &x) { x.w_off = x.m_off + 16; }), false);
            REFUSE(with(d, [](ocm_adam_rows &x) { x.w_off = 0; }));
            ACCEPT(with(d, [](ocm_adam_rows &x) { x.w_off = 0; x.table_off = 4 * (kSpan + 16); }));
        }
        // interleaved rows (exp_avg_sq rows in the gaps of exp_avg's): the whole ranges overlap
        REFUSE(with(d, [](ocm_adam_rows &x) { x.m_stride = x.v_stride = 8 * kDim; x.v_off = x.m_off + 4 * kDim; x.w_off = 1ull << 19; }),
               false);
    }
    if (failures == before) std::printf("PASS validator\n");
}

void test_hyper() {
    const int before = failures;
    char why[256];
    float hp[9] = {0.9f, 0.999f, 1e-8f, 0.f, 1e-2f, 31.6f, NAN, 0.1f, 0.001f};
    CHECK(adam_rows_check_hp(hp, 1.f, why, sizeof(why)) == 0, "plain Adam refused");
    CHECK(adam_rows_check_hp(hp, 0.f, why, sizeof(why)) == 0, "gscale 0 refused");
    CHECK(adam_rows_check_hp(hp, 1e-40f, why, sizeof(why)) == 0, "subnormal gscale refused");
    CHECK(adam_rows_check_hp(hp, INFINITY, why, sizeof(why)) != 0, "gscale inf accepted");
    CHECK(adam_rows_check_hp(hp, -INFINITY, why, sizeof(why)) != 0, "gscale -inf accepted");
    CHECK(adam_rows_check_hp(hp, NAN, why, sizeof(why)) != 0, "gscale NaN accepted");
    hp[3] = 0.01f;
    CHECK(adam_rows_check_hp(hp, 1.f, why, sizeof(why)) != 0 && std::strstr(why, "weight decay"), "L2 accepted");
    hp[3] = -0.f;
    CHECK(adam_rows_check_hp(hp, 1.f, why, sizeof(why)) == 0, "wd -0 refused");
    hp[6] = 0.999f;
    CHECK(adam_rows_check_hp(hp, 1.f, why, sizeof(why)) != 0 && std::strstr(why, "weight decay"), "AdamW accepted");
    hp[6] = 1.f;  // a multiplier of 1 is still AdamW's path
    CHECK(adam_rows_check_hp(hp, 1.f, why, sizeof(why)) != 0, "AdamW with decay 1 accepted");
    if (failures == before) std::printf("PASS hyper\n");
}

void test_bounds() {
    const int before = failures;
    CHECK(adam_rows_picks(0, 37) && adam_rows_picks(36, 37) && !adam_rows_picks(37, 37), "the table's edges");
    CHECK(!adam_rows_picks(indexed_widen32(0xFFFFFFFFu), 37), "int32 -1");
    CHECK(!adam_rows_picks(indexed_widen32(0x7FFFFFFFu), 37), "int32 2^31 - 1");
    CHECK(!adam_rows_picks(indexed_widen32(0x80000000u), 0xFFFFFFFFull), "int32 -2^31 in the largest table");
    CHECK(!adam_rows_picks(1ull << 40, 37) && !adam_rows_picks(~0ull, 37), "int64 2^40 and -1");
    CHECK(!adam_rows_picks(0, 0), "a table of no rows");
    if (failures == before) std::printf("PASS bounds\n");
}

// The kernel's walk of one wave, with its kAdamRowsInFlight slots a round, on the host.
void test_walk() {
    const int before = failures;
    const uint64_t dims[] = {4, 252, 256, 260, 1028}, ks[] = {1, 5, 37, 4093};
    const uint64_t unit = 4096;
    uint64_t shapes = 0;
    for (uint64_t dim : dims)
        for (uint64_t rows : ks) {
            const uint64_t tpr = adam_rows_tiles_per_row(dim), total = rows * tpr;
            CHECK(tpr == (dim + 255) / 256, "tiles per row of dim %llu", (unsigned long long)dim);
            // grids from one wave's workgroup to more waves than tiles, and the header's own
            std::vector<uint32_t> grids = {1, 2, 3, 7, (uint32_t)(total / kListWaves + 1), (uint32_t)(total + 3)};
            for (int cus : {1, 8, 256}) grids.push_back(adam_rows_launch_shape(rows, dim, cus, AdamKnobs{true, 128, 4, 0}).grid);
            grids.push_back(adam_rows_launch_shape(rows, dim, 256, AdamKnobs{true, 128, 4, 5}).grid);
            for (uint32_t grid : grids) {
                CHECK(grid >= 1, "grid 0 for %llu rows", (unsigned long long)rows);
                if (grid == 0) continue;
                std::vector<uint8_t> seen(total, 0);
                for (uint64_t w = 0; w < (uint64_t)grid * kListWaves; w++) {
                    uint64_t t, t1;
                    list_wave_range(w, grid, total, &t, &t1);
                    if (t >= t1) continue;
                    CHECK(t1 <= total, "wave range past the tiles");
                    uint64_t j, k;
                    list_locate(tpr, t, &j, &k);
                    for (; t < t1; t += kAdamRowsInFlight)
                        for (int u = 0; u < kAdamRowsInFlight && t + u < t1; u++) {
                            CHECK(j < rows && k < tpr && j * tpr + k == t + u, "tile %llu is not (%llu, %llu)",
                                  (unsigned long long)(t + u), (unsigned long long)j, (unsigned long long)k);
                            if (j < rows && k < tpr) seen[j * tpr + k]++;
                            // the vectors of the piece: inside the row, and never across a stripe unit,
                            // at any 16-byte (bf16 table: 8-byte) aligned place of the row
                            for (uint32_t lane = 0; lane < 64; lane++) {
                                const uint64_t e = adam_rows_elem(k, lane);
                                if (e >= dim) continue;
                                CHECK(e + 4 <= dim, "a vector past the row's end");
                                for (uint64_t off : {0ull, 16ull, 4080ull, 272ull * j}) {
                                    const uint64_t x = off + 4 * e, y = (off >> 1) + 2 * e;
                                    CHECK(x / unit == (x + 15) / unit, "an fp32 vector crosses a stripe unit");
                                    CHECK(y % 8 == 0 && y / unit == (y + 7) / unit, "a bf16 vector crosses a stripe unit");
                                }
                            }
                            if (++k == tpr) {
                                k = 0;
                                j++;
                            }
                        }
                }
                for (uint64_t i = 0; i < total; i++)
                    CHECK(seen[i] == 1, "dim %llu rows %llu grid %u: tile %llu visited %d times", (unsigned long long)dim,
                          (unsigned long long)rows, grid, (unsigned long long)i, (int)seen[i]);
                shapes++;
            }
            // every element of a row belongs to exactly one live vector
            uint64_t covered = 0;
            for (uint64_t k = 0; k < tpr; k++)
                for (uint32_t lane = 0; lane < 64; lane++)
                    if (adam_rows_elem(k, lane) < dim) covered += 4;
            CHECK(covered == dim, "dim %llu: %llu elements covered", (unsigned long long)dim, (unsigned long long)covered);
        }
    CHECK(shapes == 5 * 4 * 10, "%llu shapes walked", (unsigned long long)shapes);
    if (failures == before) std::printf("PASS walk\n");
}

void test_shape() {
    const int before = failures;
    const AdamKnobs none{true, 128, 4, 0};
    auto shape = [&](uint64_t rows, uint64_t dim, int cus, AdamKnobs k) { return adam_rows_launch_shape(rows, dim, cus, k); };
    CHECK(shape(0, 64, 256, none).grid == 0 && shape(0, 64, 256, none).total_tiles == 0, "no rows");
    CHECK(shape(1, 4, 256, none).grid == 1, "one tile");
    CHECK(shape(16, 64, 256, none).grid == 1 && shape(17, 64, 256, none).grid == 2, "16 tiles a workgroup");
    CHECK(shape(4096, 1024, 256, none).total_tiles == 16384 && shape(4096, 1024, 256, none).grid == 1024, "4 tiles a row");
    CHECK(shape(65536, 64, 256, none).grid == 1024 && shape(65536, 64, 8, none).grid == 32, "the cap: 4 workgroups a CU");
    CHECK(shape(65536, 64, 256, AdamKnobs{true, 128, 4, 7}).grid == 7, "the grid knob");
    // the second round of the GPU suite: the capped grid's waves own 5 tiles, one more than they keep in flight
    const uint64_t k2 = 1024ull * kListWaves * kAdamRowsInFlight + 7;
    const AdamRowsShape s = shape(k2, 8, 256, none);
    uint64_t t0, t1;
    list_wave_range(0, s.grid, s.total_tiles, &t0, &t1);
    CHECK(s.grid == 1024 && t1 - t0 == 5, "second round: grid %u, %llu tiles", s.grid, (unsigned long long)(t1 - t0));
    if (failures == before) std::printf("PASS shape\n");
}

}  // namespace

int main() {
    test_validator();
    test_hyper();
    test_bounds();
    test_walk();
    test_shape();
    std::printf("%d failure(s)\n", failures);
    return failures ? 1 : 0;
}
