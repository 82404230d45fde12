// The strided converting tile rule, validator and plan (ocm/quant_strided.h) on the
// CPU: the functions the kernel and the host side call, over a grid of row sizes, row
// counts and strides, against the plain converting ops the call is defined by (one per
// row). Stand-alone: it links nothing of the library, so the build also makes an
// ASan + UBSan copy of it.
#include <cstdio>
#include <cstring>
#include <vector>

#include "ocm/quant_strided.h"

using namespace ocm;

namespace {

int failures = 0;

#define CHECK(cond, ...)                 \
    do {                                 \
        if (!(cond)) {                   \
            if (failures++ < 20) {       \
                std::printf("FAIL: ");   \
                std::printf(__VA_ARGS__); \
                std::printf("\n");       \
            }                            \
        }                                \
    } while (0)

using ull = unsigned long long;

const uint64_t kRowElems[] = {32, 1024, 1056, 2048, 2080, 4128};
const uint32_t kRows[] = {1, 2, 5};

uint64_t record_up32(uint64_t elems) { return (mx8_record_bytes(elems) + 31) / 32 * 32; }

ocm_quant_strided_params P(uint64_t lo, uint64_t ro, uint64_t re, uint64_t rows, uint64_t ls, uint64_t rs,
                           uint32_t dtype = OCM_QUANT_FP16) {
    ocm_quant_strided_params p{};
    p.local_offset = lo;
    p.remote_offset = ro;
    p.row_elems = re;
    p.rows = rows;
    p.local_stride = ls;
    p.remote_stride = rs;
    p.op_flag = 1;
    p.dtype = dtype;
    return p;
}

// Every tile of `op`: the tiles of a row partition its elements exactly once, and each
// one lies where tile k of the row's plain converting op (xfer_quant_kernel's rule:
// e0 = k << kQuantTileShift, elements at lin_off + 2 e0, codes at rem_off + e0, scale
// bytes at rem_off + len + e0 / 32) lies. Then the walk the kernel makes (locate once,
// count afterwards) from several first tiles.
void check_op(XferQuantStridedOp op, uint64_t *tiles_seen) {
    const uint64_t total = xfer_quant_strided_plan(&op, 1, kQuantTileShift);
    CHECK(op.first_tile == 0 && total == (uint64_t)op.rows * quant_tile_count(op.row_elems), "plan");
    CHECK(op.tiles_per_row == (op.row_elems + kQuantTileElems - 1) / kQuantTileElems, "tiles_per_row %u for %u elements",
          op.tiles_per_row, op.row_elems);
    std::vector<uint8_t> cover((size_t)op.rows * op.row_elems, 0);  // how often element e of row r was converted
    for (uint64_t t = 0; t < total; t++) {
        uint64_t row;
        uint32_t k;
        list_locate(op.tiles_per_row, t, &row, &k);
        CHECK(row == t / op.tiles_per_row && k == t % op.tiles_per_row, "tile %llu located at row %llu piece %u", (ull)t,
              (ull)row, k);
        const QuantTileLoc q = quant_strided_tile(op, row, k, 0);  // MXFP8: one code byte per element
        (*tiles_seen)++;
        // the plain op of this row, cut as xfer_quant_kernel cuts it
        const uint64_t lin_off = op.lin_off + row * op.lin_stride, rem_off = op.rem_off + row * op.rem_stride;
        const uint64_t len = op.row_elems, e0 = (uint64_t)k << kQuantTileShift;
        const uint64_t ne = len - e0 < kQuantTileElems ? len - e0 : kQuantTileElems;
        CHECK(q.ne == ne && q.ne > 0 && q.ne % 32 == 0, "tile %llu: %u elements, the plain op has %llu", (ull)t, q.ne, (ull)ne);
        CHECK(q.lin_off == lin_off + 2 * e0, "tile %llu: elements at %llu", (ull)t, (ull)q.lin_off);
        CHECK(q.codes == rem_off + e0, "tile %llu: codes at %llu", (ull)t, (ull)q.codes);
        CHECK(q.scales == rem_off + len + (e0 >> 5), "tile %llu: scale bytes at %llu", (ull)t, (ull)q.scales);
        // what the tile bodies rest on: 16-byte vectors of source, codes and scale bytes
        CHECK(q.lin_off % 16 == 0 && q.codes % 16 == 0 && q.scales % 16 == 0, "tile %llu: unaligned vectors", (ull)t);
        // inside the row's record: codes in [0, len), scale bytes in [len, len + len / 32)
        CHECK(q.codes + q.ne <= rem_off + len && q.scales + q.ne / 32 <= rem_off + mx8_record_bytes(len),
              "tile %llu leaves its record", (ull)t);
        if (e0 + q.ne <= len)
            for (uint64_t e = 0; e < q.ne; e++) cover[(size_t)(row * op.row_elems + e0 + e)]++;
    }
    size_t bad = 0;
    for (uint8_t c : cover) bad += c != 1;
    CHECK(bad == 0, "%zu elements not converted exactly once (rows %u x %u)", bad, op.rows, op.row_elems);
    for (uint64_t start : {(uint64_t)0, total / 3, total - 1}) {
        uint64_t row;
        uint32_t k;
        list_locate(op.tiles_per_row, start, &row, &k);
        for (uint64_t t = start; t < total; t++) {
            CHECK(row == t / op.tiles_per_row && k == t % op.tiles_per_row, "walk differs at tile %llu", (ull)t);
            list_next_piece(op.tiles_per_row, &row, &k);
        }
    }
}

void test_tile_rule() {
    uint64_t ops = 0, tiles = 0;
    for (uint64_t re : kRowElems)
        for (uint32_t nr : kRows) {
            // local strides: dense, padded by 16, a cache apart; remote: dense (the record rounded
            // up to 32), padded by 32 and by 96
            const uint64_t lstrides[] = {2 * re, 2 * re + 16, 12 * 2 * re};
            const uint64_t rstrides[] = {record_up32(re), record_up32(re) + 32, record_up32(re) + 96};
            for (uint64_t ls : lstrides)
                for (uint64_t rs : rstrides)
                    for (uint64_t ro : {(uint64_t)0, (uint64_t)2 * 4096 - 64, (uint64_t)5 * 4096 - 2080}) {
                        const ocm_quant_strided_params p = P(48, ro, re, nr, ls, rs);
                        uint64_t src = 0, wire = 0;
                        char why[192] = "";
                        CHECK(quant_strided_check_op(p, 1ull << 30, 1ull << 30, &src, &wire, why, sizeof(why)) == 0, "%s", why);
                        CHECK(src == 2 * re * nr && wire == mx8_record_bytes(re) * nr, "src %llu wire %llu", (ull)src, (ull)wire);
                        const XferQuantStridedOp op = quant_strided_op(p);
                        CHECK(op.rows == nr && op.row_elems == re && op.put == 1 && op.dtype == OCM_QUANT_FP16, "descriptor");
                        check_op(op, &tiles);
                        ops++;
                    }
        }
    std::printf("tile_rule: %llu ops, %llu tiles\n", (ull)ops, (ull)tiles);
}

// A list: first_tile is the prefix sum, empty ops take no tiles, and every wave's
// starting op is the op of its first tile.
void test_plan() {
    const uint64_t re[] = {4128, 0, 32, 2048, 2080, 1024, 0};
    const uint64_t nr[] = {3, 4, 0, 2, 7, 1, 2};
    std::vector<XferQuantStridedOp> v;
    for (size_t i = 0; i < 7; i++) v.push_back(quant_strided_op(P(0, 0, re[i], nr[i], 2 * re[i], record_up32(re[i]))));
    CHECK(v[1].rows == 0 && v[1].row_elems == 0 && v[2].rows == 0 && v[2].row_elems == 0, "empty ops keep nothing");
    const uint64_t total = xfer_quant_strided_plan(v.data(), (uint32_t)v.size(), kQuantTileShift);
    CHECK(total == 3 * 3 + 0 + 0 + 2 * 1 + 7 * 2 + 1 + 0, "total %llu", (ull)total);
    const uint64_t want_first[] = {0, 9, 9, 9, 11, 25, 26};
    for (size_t i = 0; i < v.size(); i++) CHECK(v[i].first_tile == want_first[i], "first_tile of op %zu", i);
    for (uint32_t grid : {1u, 2u, 3u, 5u}) {
        std::vector<uint32_t> w(grid * 4);
        list_wave_ops(v.data(), (uint32_t)v.size(), total, grid, w.data());
        for (uint32_t k = 0; k < grid * 4; k++) {
            uint64_t t0, t1;
            list_wave_range(k, grid, total, &t0, &t1);
            if (t0 >= t1) continue;
            const XferQuantStridedOp &op = v[w[k]];
            CHECK(op.first_tile <= t0 && t0 < op.first_tile + quant_strided_tile_count(op), "wave %u of grid %u starts in op %u",
                  k, grid, w[k]);
        }
    }
}

int check(const ocm_quant_strided_params &p, uint64_t lb, uint64_t rb, const char *want_in_msg, uint64_t want_src = 0,
          uint64_t want_wire = 0) {
    char why[192] = "";
    uint64_t src = 77, wire = 77;
    const int rc = quant_strided_check_op(p, lb, rb, &src, &wire, why, sizeof(why));
    if (want_in_msg) {
        CHECK(rc == -1 && std::strstr(why, want_in_msg), "wanted an error with '%s', got rc %d '%s'", want_in_msg, rc, why);
    } else {
        CHECK(rc == 0 && src == want_src && wire == want_wire, "wanted success with %llu / %llu bytes, got rc %d '%s' %llu / %llu",
              (ull)want_src, (ull)want_wire, rc, why, (ull)src, (ull)wire);
    }
    return rc;
}

void test_validator() {
    const uint64_t MiB = 1ull << 20, big = 1ull << 63, max32 = (1ull << 32) - 1;
    // exact fits (4 rows of 64 elements: 128 local bytes, 66 record bytes), and one step too far
    check(P(0, 0, 64, 4, 128, 96), 512, 3 * 96 + 66, nullptr, 512, 4 * 66);
    check(P(16, 0, 64, 4, 128, 96), 512, 3 * 96 + 66, "local range");
    check(P(0, 32, 64, 4, 128, 96), 512, 3 * 96 + 66 + 31, "remote range");
    check(P(0, 0, 64, 4, 144, 96), 512, MiB, "local range");
    check(P(0, 0, 64, 4, 128, 96), 512, 3 * 96 + 65, "remote range");
    check(P(0, 0, 64, 1, 0, 0), 128, 66, nullptr, 128, 66);  // one row, stride 0
    check(P(MiB, 0, 32, 1, 0, 0), MiB, MiB, "local range");
    check(P(0, ~0ull - 31, 32, 1, 0, 0), MiB, MiB, "remote range");
    // element type, row size, rows
    check(P(0, 0, 64, 1, 128, 96, 0), MiB, MiB, "element type");
    check(P(0, 0, 64, 1, 128, 96, 3), MiB, MiB, "element type");
    check(P(0, 0, 64, 1, 128, 96, OCM_QUANT_BF16), MiB, MiB, nullptr, 128, 66);
    check(P(0, 0, 33, 1, 128, 96), MiB, MiB, "multiple of 32");
    check(P(0, 0, 1ull << 31, 1, 0, 0), ~0ull, ~0ull, "2^31");
    check(P(0, 0, (1ull << 31) - 32, 1, 0, 0), ~0ull, ~0ull, nullptr, (1ull << 32) - 64, (1ull << 31) - 32 + (1ull << 26) - 1);
    check(P(0, 0, 32, 1ull << 32, 64, 64), ~0ull, ~0ull, "2^32");
    check(P(0, 0, 32, ~0ull, 64, 64), ~0ull, ~0ull, "2^32");
    // alignment: 16 on the local side, 32 on the remote side
    check(P(8, 0, 32, 2, 64, 64), MiB, MiB, "local offset");
    check(P(0, 16, 32, 2, 64, 64), MiB, MiB, "remote offset");
    check(P(0, 0, 32, 2, 72, 64), MiB, MiB, "local stride");
    check(P(0, 0, 32, 2, 64, 80), MiB, MiB, "remote stride");
    check(P(16, 32, 32, 2, 80, 96), MiB, MiB, nullptr, 128, 66);
    // strides below the row: 2 * row_elems local bytes, row_elems + row_elems / 32 record bytes
    check(P(0, 0, 64, 2, 112, 96), MiB, MiB, "local stride");
    check(P(0, 0, 64, 2, 128, 64), MiB, MiB, "remote stride");  // 64 < 66
    check(P(0, 0, 1024, 2, 2048, 1024), MiB, MiB, "remote stride");
    check(P(0, 0, 1024, 2, 2048, 1056), MiB, MiB, nullptr, 4096, 2112);
    // sums and products that wrap 64 bits must not pass
    check(P(0, 0, 32, max32, big, 64), MiB, 1ull << 40, "local range");   // (2^32 - 2) * 2^63 wraps to 0
    check(P(0, 0, 32, max32, 64, big), 1ull << 40, MiB, "remote range");
    check(P(0, 0, 32, 3, big + 64, 64), MiB, MiB, "local range");          // 2 * (2^63 + 64) wraps to 128
    check(P(0, 0, 32, 3, 64, big + 64), MiB, MiB, "remote range");
    check(P(0, 0, 32, 5, big / 2, 64), MiB, MiB, "local range");           // 4 * 2^62 wraps to 0
    check(P(0, 0, 32, 5, 64, big / 2), MiB, MiB, "remote range");
    check(P(16, 32, 32, max32, ~0ull - 15, ~0ull - 31), ~0ull, ~0ull, "local range");
    check(P(0, 0, 32, max32, 64, 64), max32 * 64, (max32 - 1) * 64 + 33, nullptr, max32 * 64, max32 * 33);  // the most rows
    check(P(0, 0, 32, max32, 64, 64), max32 * 64 - 1, max32 * 64, "local range");
    check(P(0, 0, 32, max32, 64, 64), max32 * 64, (max32 - 1) * 64 + 32, "remote range");
    // empty ops: fine wherever they point
    check(P(~0ull, ~0ull, 0, 9, 1, 1), MiB, MiB, nullptr, 0, 0);
    check(P(~0ull, ~0ull, 64, 0, 1, 1), MiB, MiB, nullptr, 0, 0);
    check(P(0, 0, 0, max32, big, big), 0, 0, nullptr, 0, 0);
}

}  // namespace

int main() {
    struct {
        const char *name;
        void (*fn)();
    } parts[] = {{"tile_rule", test_tile_rule}, {"plan", test_plan}, {"validator", test_validator}};
    for (auto &p : parts) {
        const int before = failures;
        p.fn();
        std::printf("%s %s\n", failures == before ? "PASS" : "FAILED", p.name);
    }
    std::printf("%d failure(s)\n", failures);
    return failures ? 1 : 0;
}
