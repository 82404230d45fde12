// The strided tile geometry and validator (ocm/strided.h) on the CPU: the functions
// the kernel calls, over every tile of a grid of layouts. Stand-alone: it links
// nothing of the library, so the build also makes an ASan + UBSan copy of it.
#include <cstdio>
#include <cstring>
#include <vector>

#include "ocm/strided.h"

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

// The library's rule (xfer_batch_tile_shift): 4 KiB wave-tiles, or the stripe unit when smaller.
uint32_t batch_tile_shift(uint32_t n_ext, uint32_t unit_shift) { return (n_ext > 1 && unit_shift < 12) ? unit_shift : 12; }

struct Layout {
    uint32_t n_ext, unit_shift, tile_shift;
};

// Every tile of `op`: the pieces partition each row exactly once, stay inside the row,
// keep both sides at the same offset in the row, and never cross a stripe unit. Then
// the walk the kernel makes (list_locate once, list_next_piece afterwards) from several first tiles.
void check_op(XferStridedOp op, const Layout &L, uint64_t *pieces_seen, uint64_t *split_seen) {
    const uint64_t total = xfer_strided_plan(&op, 1, L.tile_shift);
    CHECK(op.first_tile == 0 && total == (uint64_t)op.rows * strided_tiles_per_row(op.row_bytes, L.tile_shift), "plan");
    CHECK(op.tiles_per_row * (1ull << L.tile_shift) >= op.row_bytes &&
              (op.tiles_per_row - 1) * (1ull << L.tile_shift) < op.row_bytes,
          "tiles_per_row %llu for %llu bytes", (unsigned long long)op.tiles_per_row, (unsigned long long)op.row_bytes);
    // cover[r * row_bytes + b]: how often byte b of row r was moved
    std::vector<uint8_t> cover((size_t)(op.rows * op.row_bytes), 0);
    for (uint64_t t = 0; t < total; t++) {
        StridedPiece p[2];
        const int np = strided_tile_pieces(op, t, L.n_ext, L.unit_shift, L.tile_shift, p);
        CHECK(np == 1 || np == 2, "tile %llu: %d pieces", (unsigned long long)t, np);
        const uint64_t row = t / op.tiles_per_row;  // the issue's rule, worked out apart from list_locate
        const uint64_t l0 = op.lin_off + row * op.lin_stride, r0 = op.rem_off + row * op.rem_stride;
        uint64_t tile_bytes = 0;
        for (int j = 0; j < np; j++) {
            (*pieces_seen)++;
            CHECK(p[j].n > 0 && p[j].n <= (1ull << L.tile_shift), "tile %llu piece %d: %llu bytes", (unsigned long long)t, j,
                  (unsigned long long)p[j].n);
            CHECK(p[j].lin_off >= l0 && p[j].rem_off >= r0 && p[j].lin_off - l0 == p[j].rem_off - r0,
                  "tile %llu piece %d: sides disagree", (unsigned long long)t, j);
            const uint64_t x = p[j].lin_off - l0;
            CHECK(x + p[j].n <= op.row_bytes, "tile %llu piece %d leaves its row", (unsigned long long)t, j);
            if (L.n_ext > 1)
                CHECK((p[j].rem_off >> L.unit_shift) == ((p[j].rem_off + p[j].n - 1) >> L.unit_shift),
                      "tile %llu piece %d crosses a stripe unit", (unsigned long long)t, j);
            if (x + p[j].n <= op.row_bytes)
                for (uint64_t b = 0; b < p[j].n; b++) cover[(size_t)(row * op.row_bytes + x + b)]++;
            tile_bytes += p[j].n;
        }
        if (np == 2) {
            (*split_seen)++;
            CHECK(p[1].lin_off == p[0].lin_off + p[0].n && p[1].rem_off == p[0].rem_off + p[0].n, "split not adjacent");
            CHECK((p[1].rem_off & ((1ull << L.unit_shift) - 1)) == 0, "second piece not at a unit boundary");
        }
        CHECK(tile_bytes <= (1ull << L.tile_shift), "tile %llu: %llu bytes", (unsigned long long)t, (unsigned long long)tile_bytes);
    }
    size_t bad = 0;
    for (uint8_t c : cover) bad += c != 1;
    CHECK(bad == 0, "%zu bytes not moved exactly once (rows %u x %llu, unit 2^%u, tile 2^%u, n_ext %u, rem_off %llu)", bad,
          op.rows, (unsigned long long)op.row_bytes, L.unit_shift, L.tile_shift, L.n_ext, (unsigned long long)op.rem_off);
    // the kernel's walk, by the functions it calls (ocm/list.h): list_locate at a wave's first
    // tile, then list_next_piece
    for (uint64_t start : {(uint64_t)0, total / 3, total - 1}) {
        uint64_t row, k;
        list_locate(op.tiles_per_row, start, &row, &k);
        for (uint64_t t = start; t < total; t++) {
            StridedPiece a[2], b[2];
            const int na = strided_row_pieces(op, row, k, L.n_ext, L.unit_shift, L.tile_shift, a);
            const int nb = strided_tile_pieces(op, t, L.n_ext, L.unit_shift, L.tile_shift, b);
            CHECK(na == nb && std::memcmp(a, b, sizeof(StridedPiece) * (size_t)na) == 0, "walk differs at tile %llu",
                  (unsigned long long)t);
            list_next_piece(op.tiles_per_row, &row, &k);
        }
    }
}

void test_geometry() {
    const uint64_t units[] = {16, 256, 4096, 1ull << 20};
    const uint64_t row_bytes[] = {1, 15, 16, 17, 4095, 4096, 4097, 12291};
    const uint32_t rows[] = {1, 2, 5};
    uint64_t ops = 0, pieces = 0, splits = 0;
    for (uint32_t n_ext : {1u, 3u})
        for (uint64_t unit : units) {
            const uint32_t us = (uint32_t)__builtin_ctzll(unit);
            // the library's tile, and 16-byte tiles (rows of many pieces)
            for (uint32_t ts : {batch_tile_shift(n_ext, us), 4u}) {
                const Layout L{n_ext, us, ts};
                for (uint64_t rb : row_bytes)
                    for (uint32_t nr : rows) {
                        // remote offsets: a multiple of the unit, of 16 only, of neither, and just under a boundary
                        const uint64_t roffs[] = {2 * unit, 2 * unit + 16, 2 * unit + 5, 3 * unit - 7};
                        // remote strides: dense, padded to whole units, padded by an odd amount
                        const uint64_t rstrides[] = {rb, (rb + unit - 1) / unit * unit + unit, rb + 13};
                        for (uint64_t ro : roffs)
                            for (uint64_t rs : rstrides)
                                for (int lv = 0; lv < 2; lv++) {
                                    XferStridedOp op{};
                                    op.lin_off = lv ? 3 : 64;
                                    op.lin_stride = lv ? rb + 1 : (rb + 15) / 16 * 16;
                                    op.rem_off = ro;
                                    op.rem_stride = rs;
                                    op.row_bytes = rb;
                                    op.rows = nr;
                                    op.put = (uint32_t)lv;
                                    check_op(op, L, &pieces, &splits);
                                    ops++;
                                }
                    }
            }
        }
    CHECK(splits > 0 && pieces > ops, "the grid never split a tile");
    std::printf("geometry: %llu ops, %llu pieces, %llu tiles in two spans\n", (unsigned long long)ops,
                (unsigned long long)pieces, (unsigned long long)splits);
}

// A list: first_tile is the prefix sum, empty ops take no tiles, and every wave's
// starting op is the op of its first tile.
void test_plan() {
    std::vector<XferStridedOp> v(7, XferStridedOp{});
    const uint64_t rb[] = {4097, 0, 100, 8192, 5, 1, 0};
    const uint32_t nr[] = {3, 4, 0, 2, 7, 1, 2};
    for (size_t i = 0; i < v.size(); i++) {
        v[i].row_bytes = nr[i] ? rb[i] : 0;
        v[i].rows = rb[i] ? nr[i] : 0;
    }
    const uint64_t total = xfer_strided_plan(v.data(), (uint32_t)v.size(), 12);
    CHECK(total == 3 * 2 + 0 + 0 + 2 * 2 + 7 + 1 + 0, "total %llu", (unsigned long long)total);
    const uint64_t want_first[] = {0, 6, 6, 6, 10, 17, 18};
    for (size_t i = 0; i < v.size(); i++) CHECK(v[i].first_tile == want_first[i], "first_tile of op %zu", i);
    for (uint32_t grid : {1u, 2u, 3u, 5u}) {
        std::vector<uint32_t> w(grid * 4);
        list_wave_ops(v.data(), (uint32_t)v.size(), total, grid, w.data());
        const uint64_t per = (total + grid * 4 - 1) / (grid * 4);
        for (uint32_t k = 0; k < grid * 4; k++) {
            const uint64_t t = k * per;
            if (t >= total) continue;
            const XferStridedOp &op = v[w[k]];
            CHECK(op.first_tile <= t && t < op.first_tile + strided_tile_count(op), "wave %u of grid %u starts in op %u", k,
                  grid, w[k]);
        }
    }
}

int check(const ocm_strided_params &p, uint64_t lb, uint64_t rb, const char *want_in_msg, uint64_t want_moved = 0) {
    char why[192] = "";
    uint64_t moved = 77;
    const int rc = strided_check_op(p, lb, rb, &moved, why, sizeof(why));
    if (want_in_msg) {
        CHECK(rc == -1 && std::strstr(why, want_in_msg), "wanted an error with '%s', got rc %d '%s'", want_in_msg, rc, why);
    } else {
        CHECK(rc == 0 && moved == want_moved, "wanted success moving %llu, got rc %d '%s' moved %llu",
              (unsigned long long)want_moved, rc, why, (unsigned long long)moved);
    }
    return rc;
}

ocm_strided_params P(uint64_t lo, uint64_t ro, uint64_t rb, uint64_t rows, uint64_t ls, uint64_t rs) {
    ocm_strided_params p{};
    p.local_offset = lo;
    p.remote_offset = ro;
    p.row_bytes = rb;
    p.rows = rows;
    p.local_stride = ls;
    p.remote_stride = rs;
    p.op_flag = 1;
    return p;
}

void test_validator() {
    const uint64_t MiB = 1ull << 20, big = 1ull << 63, max32 = (1ull << 32) - 1;
    // exact fits, and one byte too many on either side
    check(P(0, 0, 100, 4, 100, 256), 400, 3 * 256 + 100, nullptr, 400);
    check(P(1, 0, 100, 4, 100, 256), 400, 3 * 256 + 100, "local range");
    check(P(0, 1, 100, 4, 100, 256), 400, 3 * 256 + 100, "remote range");
    check(P(0, 0, 100, 4, 101, 256), 400, MiB, "local range");
    check(P(7, 9, MiB - 9, 1, 0, 0), MiB, MiB, nullptr, MiB - 9);  // one row: the strides are not read
    check(P(MiB, 0, 1, 1, 0, 0), MiB, MiB, "local range");
    check(P(0, ~0ull, 1, 1, 0, 0), MiB, MiB, "remote range");
    check(P(0, 0, ~0ull, 1, 0, 0), MiB, MiB, "local range");
    // sums and products that wrap 64 bits must not pass
    check(P(0, 0, 1, max32, big, 1), MiB, 1ull << 40, "local range");   // (2^32 - 2) * 2^63 wraps to 0
    check(P(0, 0, 1, max32, 1, big), 1ull << 40, MiB, "remote range");
    check(P(0, 0, 8, 3, big + 8, 8), MiB, MiB, "local range");           // 2 * (2^63 + 8) wraps to 16
    check(P(0, 0, 8, 3, 8, big + 8), MiB, MiB, "remote range");
    check(P(0, 0, 8, 5, big / 2, 8), MiB, MiB, "local range");           // 4 * 2^62 wraps to 0
    check(P(16, 16, 16, max32, ~0ull, ~0ull), ~0ull, ~0ull, "local range");
    check(P(0, 0, 1, max32, 1, 1), max32, max32, nullptr, max32);        // the most rows, dense: fits exactly
    check(P(0, 0, 1, max32, 1, 1), max32 - 1, max32, "local range");
    // rows
    check(P(0, 0, 1, 1ull << 32, 1, 1), ~0ull, ~0ull, "2^32");
    check(P(0, 0, 1, ~0ull, 1, 1), ~0ull, ~0ull, "2^32");
    // strides below the row
    check(P(0, 0, 100, 2, 99, 100), MiB, MiB, "local stride");
    check(P(0, 0, 100, 2, 100, 0), MiB, MiB, "remote stride");
    check(P(0, 0, 100, 1, 0, 0), MiB, MiB, nullptr, 100);
    // reserved
    ocm_strided_params r = P(0, 0, 1, 1, 1, 1);
    r.reserved = 5;
    check(r, MiB, MiB, "reserved");
    // empty ops: fine wherever they point
    check(P(~0ull, ~0ull, 0, 9, 0, 0), MiB, MiB, nullptr, 0);
    check(P(~0ull, ~0ull, 9, 0, 0, 0), MiB, MiB, nullptr, 0);
    check(P(0, 0, 0, max32, big, big), 0, 0, nullptr, 0);
}

}  // namespace

int main() {
    struct {
        const char *name;
        void (*fn)();
    } parts[] = {{"geometry", test_geometry}, {"plan", test_plan}, {"validator", test_validator}};
    for (auto &p : parts) {
        const int before = failures;
        p.fn();
        std::printf("%s %s\n", failures == before ? "PASS" : "FAILED", p.name);
    }
    std::printf("%d failure(s)\n", failures);
    return failures ? 1 : 0;
}
