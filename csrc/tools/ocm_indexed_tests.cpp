// The indexed ops' shared header (ocm/indexed.h) on the CPU: the functions the kernel
// and the host path call. Tile geometry under index arrays over a grid of layouts, the
// bounds rule at its edge values, every rule of the validator and the plan. Stand-alone:
// it links nothing of the library, so the build also makes an ASan + UBSan copy of it.
#include <climits>
#include <cstdio>
#include <cstring>
#include <vector>

#include "ocm/indexed.h"

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

// The kernel's walk over every tile of `op` with the index arrays lidx / ridx (empty:
// that side has none), from one first tile per "wave": each selected row is reassembled
// exactly once on both sides, pieces stay inside their rows and inside one stripe unit,
// and rows with an index outside its table move nothing and are counted once.
void check_op(XferIndexedOp op, const std::vector<int64_t> &lidx, const std::vector<int64_t> &ridx, const Layout &L,
              uint64_t *pieces_seen, uint64_t *split_seen, uint64_t *skips_seen) {
    const uint64_t total = xfer_indexed_plan(&op, 1, L.tile_shift);
    CHECK(op.first_tile == 0 && total == (uint64_t)op.rows * strided_tiles_per_row(op.row_bytes, L.tile_shift), "plan");
    // cover[j * row_bytes + b]: how often byte b of the op's row j was moved
    std::vector<uint8_t> cover((size_t)(op.rows * op.row_bytes), 0);
    std::vector<uint8_t> counted(op.rows, 0);
    // three waves with contiguous tile ranges, each entering its first row as the kernel does
    const uint64_t cuts[4] = {0, total / 3, total - total / 4, total};
    for (int wv = 0; wv < 3; wv++) {
        uint64_t j = 0, k = 0, lr = 0, rr = 0;
        bool enter = true, ok = false;
        if (cuts[wv] < cuts[wv + 1]) list_locate(op.tiles_per_row, cuts[wv], &j, &k);
        for (uint64_t t = cuts[wv]; t < cuts[wv + 1]; t++) {
            CHECK(j == t / op.tiles_per_row && k == t % op.tiles_per_row, "tile %llu is not row %llu piece %llu",
                  (unsigned long long)t, (unsigned long long)j, (unsigned long long)k);
            if (enter) {
                enter = false;
                lr = lidx.empty() ? j : (uint64_t)lidx[(size_t)j];
                rr = ridx.empty() ? j : (uint64_t)ridx[(size_t)j];
                ok = indexed_in_range(lr, op.lin_rows) && indexed_in_range(rr, op.rem_rows);
                if (!ok && k == 0) counted[(size_t)j]++;
            }
            if (ok) {
                StridedPiece p[2];
                const int np = strided_row_pieces(op, lr, rr, k, L.n_ext, L.unit_shift, L.tile_shift, p);
                CHECK(np == 1 || np == 2, "tile %llu: %d pieces", (unsigned long long)t, np);
                const uint64_t l0 = op.lin_off + lr * op.lin_stride, r0 = op.rem_off + rr * op.rem_stride;
                for (int q = 0; q < np; q++) {
                    (*pieces_seen)++;
                    CHECK(p[q].n > 0 && p[q].n <= (1ull << L.tile_shift), "tile %llu piece %d: %llu bytes", (unsigned long long)t,
                          q, (unsigned long long)p[q].n);
                    CHECK(p[q].lin_off >= l0 && p[q].rem_off >= r0 && p[q].lin_off - l0 == p[q].rem_off - r0,
                          "tile %llu piece %d: sides disagree", (unsigned long long)t, q);
                    const uint64_t x = p[q].lin_off - l0;
                    CHECK(x + p[q].n <= op.row_bytes, "tile %llu piece %d leaves its row", (unsigned long long)t, q);
                    if (L.n_ext > 1)
                        CHECK((p[q].rem_off >> L.unit_shift) == ((p[q].rem_off + p[q].n - 1) >> L.unit_shift),
                              "tile %llu piece %d crosses a stripe unit", (unsigned long long)t, q);
                    if (x + p[q].n <= op.row_bytes)
                        for (uint64_t b = 0; b < p[q].n; b++) cover[(size_t)(j * op.row_bytes + x + b)]++;
                }
                if (np == 2) {
                    (*split_seen)++;
                    CHECK(p[1].lin_off == p[0].lin_off + p[0].n && p[1].rem_off == p[0].rem_off + p[0].n, "split not adjacent");
                    CHECK((p[1].rem_off & ((1ull << L.unit_shift) - 1)) == 0, "second piece not at a unit boundary");
                }
            }
            if (list_next_piece(op.tiles_per_row, &j, &k)) enter = true;
        }
    }
    for (uint32_t j = 0; j < op.rows; j++) {
        const uint64_t lr = lidx.empty() ? j : (uint64_t)lidx[j], rr = ridx.empty() ? j : (uint64_t)ridx[j];
        const bool ok = lr < op.lin_rows && rr < op.rem_rows;  // the issue's rule, written apart from indexed_in_range
        size_t bad = 0;
        for (uint64_t b = 0; b < op.row_bytes; b++) bad += cover[(size_t)(j * op.row_bytes + b)] != (ok ? 1 : 0);
        CHECK(bad == 0, "row %u (%s): %zu bytes not moved exactly %d time(s)", j, ok ? "in range" : "out of range", bad, ok ? 1 : 0);
        CHECK(counted[j] == (ok ? 0 : 1), "row %u counted as skipped %u time(s)", j, counted[j]);
        *skips_seen += !ok;
    }
}

void test_geometry() {
    const uint64_t units[] = {16, 256, 4096, 1ull << 20};
    const uint64_t row_bytes[] = {1, 15, 16, 17, 4095, 4096, 4097, 12291};
    uint64_t ops = 0, pieces = 0, splits = 0, skips = 0;
    // five rows out of tables of seven: a permutation, duplicates, and out-of-range values among good ones
    const std::vector<int64_t> perm = {4, 0, 6, 2, 5}, dup = {3, 3, 0, 3, 6}, none = {};
    const std::vector<int64_t> bad = {-1, 6, 7, 2, (int64_t)1 << 40};
    const std::vector<int64_t> *pairs[][2] = {{&none, &perm}, {&perm, &none}, {&dup, &perm}, {&none, &bad}, {&bad, &dup}, {&perm, &bad}};
    for (uint32_t n_ext : {1u, 3u})
        for (uint64_t unit : units) {
            const uint32_t us = (uint32_t)__builtin_ctzll(unit);
            for (uint32_t ts : {batch_tile_shift(n_ext, us), 4u}) {
                const Layout L{n_ext, us, ts};
                for (uint64_t rb : row_bytes) {
                    const uint64_t roffs[] = {2 * unit, 2 * unit + 5, 3 * unit - 7};
                    const uint64_t rstrides[] = {rb, (rb + unit - 1) / unit * unit + unit, rb + 13};
                    for (uint64_t ro : roffs)
                        for (uint64_t rs : rstrides)
                            for (auto &pr : pairs) {
                                XferIndexedOp op{};
                                op.lin_off = ops % 2 ? 3 : 64;
                                op.lin_stride = ops % 2 ? rb + 1 : (rb + 15) / 16 * 16;
                                op.rem_off = ro;
                                op.rem_stride = rs;
                                op.row_bytes = rb;
                                op.rows = 5;
                                op.lin_rows = op.rem_rows = 7;
                                op.index_type = OCM_INDEX_I64;
                                op.put = (uint32_t)(ops % 2);
                                check_op(op, *pr[0], *pr[1], L, &pieces, &splits, &skips);
                                ops++;
                            }
                }
            }
        }
    CHECK(splits > 0 && pieces > ops && skips > 0, "the grid never split a tile or never skipped a row");
    std::printf("geometry: %llu ops, %llu pieces, %llu tiles in two spans, %llu rows skipped\n", (unsigned long long)ops,
                (unsigned long long)pieces, (unsigned long long)splits, (unsigned long long)skips);
}

// The in-range predicate on the values as they lie in memory, through the loader the host path uses.
void test_bounds() {
    const uint64_t table = 1000;
    struct {
        int64_t v;
        bool fits32;
    } vals[] = {{-1, true},       {INT32_MIN, true}, {(int64_t)table - 1, true}, {(int64_t)table, true}, {INT32_MAX, true},
                {0, true},        {1ll << 40, false}, {INT64_MIN, false},         {1ll << 32, false}};
    for (auto &x : vals) {
        const bool want = x.v >= 0 && (uint64_t)x.v < table;
        int64_t a64[2] = {0, x.v};
        CHECK(indexed_in_range(indexed_load_host(reinterpret_cast<const char *>(a64), 0, OCM_INDEX_I64, 1), table) == want,
              "int64 %lld against %llu rows", (long long)x.v, (unsigned long long)table);
        if (x.fits32) {
            int32_t a32[2] = {0, (int32_t)x.v};
            CHECK(indexed_in_range(indexed_load_host(reinterpret_cast<const char *>(a32), 0, OCM_INDEX_I32, 1), table) == want,
                  "int32 %lld against %llu rows", (long long)x.v, (unsigned long long)table);
            CHECK(indexed_in_range(indexed_widen32((uint32_t)(int32_t)x.v), table) == want, "widen32 %lld", (long long)x.v);
        }
    }
    // 2^32 as an int64 index must not be taken for row 0, nor anything for a row of an empty table
    CHECK(!indexed_in_range(1ull << 32, 1) && !indexed_in_range(0, 0), "2^32 or an empty table");
    // the largest table: 2^32 - 1 rows
    CHECK(indexed_in_range((1ull << 32) - 2, (1ull << 32) - 1) && !indexed_in_range((1ull << 32) - 1, (1ull << 32) - 1), "largest table");
    CHECK(indexed_in_range(indexed_widen32(INT32_MAX), (1ull << 32) - 1) && !indexed_in_range(indexed_widen32(0x80000000u), (1ull << 32) - 1),
          "int32 against the largest table");
}

int check(const ocm_indexed_params &p, uint64_t lb, uint64_t rb, const char *want_in_msg, uint64_t want_moved = 0) {
    char why[256] = "";
    uint64_t moved = 77;
    const int rc = indexed_check_op(p, lb, rb, &moved, why, sizeof(why));
    if (want_in_msg) {
        CHECK(rc == -1 && std::strstr(why, want_in_msg), "wanted an error with '%s', got rc %d '%s'", want_in_msg, rc, why);
    } else {
        CHECK(rc == 0 && moved == want_moved, "wanted success moving %llu, got rc %d '%s' moved %llu",
              (unsigned long long)want_moved, rc, why, (unsigned long long)moved);
    }
    return rc;
}

// A gather (get) of `rows` rows: remote table of rr rows indexed from ridx_off, local table of lr rows in order.
ocm_indexed_params P(uint64_t lo, uint64_t ro, uint64_t rb, uint64_t rows, uint64_t ls, uint64_t rs, uint64_t lidx,
                     uint64_t ridx, uint64_t lr, uint64_t rr, int put = 0, uint32_t type = OCM_INDEX_I32) {
    ocm_indexed_params p{};
    p.local_offset = lo;
    p.remote_offset = ro;
    p.row_bytes = rb;
    p.rows = rows;
    p.local_stride = ls;
    p.remote_stride = rs;
    p.local_index_offset = lidx;
    p.remote_index_offset = ridx;
    p.local_rows = lr;
    p.remote_rows = rr;
    p.op_flag = put;
    p.index_type = type;
    return p;
}

void test_validator() {
    const uint64_t MiB = 1ull << 20, big = 1ull << 63, max32 = (1ull << 32) - 1, NONE = OCM_INDEX_NONE;
    // a plain gather: 4 rows of 100 bytes out of 8, ids at the end of the local half
    check(P(0, 0, 100, 4, 100, 256, NONE, 400, 4, 8), 416, 7 * 256 + 100, nullptr, 400);
    check(P(0, 0, 100, 4, 100, 256, NONE, 400, 4, 8), 416, 7 * 256 + 99, "remote table");   // the table's last row, not the op's
    check(P(5, 0, 100, 4, 100, 256, NONE, 404, 4, 8), 420, MiB, "overlaps");               // the get would write ids
    check(P(0, 0, 100, 4, 100, 256, NONE, 400, 4, 8), 415, MiB, "index array");
    // index type and presence
    check(P(0, 0, 100, 4, 100, 256, NONE, 400, 4, 8, 0, 0), MiB, MiB, "index_type");
    check(P(0, 0, 100, 4, 100, 256, NONE, 400, 4, 8, 0, 3), MiB, MiB, "index_type");
    check(P(0, 0, 100, 4, 100, 256, NONE, NONE, 4, 8), MiB, MiB, "no index on either side");
    // counts of 2^32 and more
    check(P(0, 0, 1, 1ull << 32, 1, 1, NONE, 0, max32, 8, 1), ~0ull, ~0ull, "2^32");
    check(P(0, 0, 1, ~0ull, 1, 1, NONE, 0, max32, 8, 1), ~0ull, ~0ull, "2^32");
    check(P(0, 0, 1, 4, 1, 1, 4096, NONE, 1ull << 32, 8, 1), ~0ull, ~0ull, "local table of");
    check(P(0, 0, 1, 4, 1, 1, NONE, 4096, 8, 1ull << 32, 1), ~0ull, ~0ull, "remote table of");
    // strides below the row, read only for tables of more than one row
    check(P(0, 0, 100, 2, 99, 100, NONE, 4096, 2, 2, 1), MiB, MiB, "local stride");
    check(P(0, 0, 100, 2, 100, 0, NONE, 4096, 2, 2, 1), MiB, MiB, "remote stride");
    check(P(0, 0, 100, 1, 0, 0, NONE, 4096, 1, 1, 1), MiB, MiB, nullptr, 100);
    // the table's last row: exact fits, one byte too many, and no overflow
    check(P(0, 0, 100, 2, 100, 100, 4096, NONE, 40, 2, 1), 4096 + 8, 200, nullptr, 200);
    check(P(105, 0, 100, 2, 100, 100, 4096, NONE, 40, 2, 1), 4096 + 8, 200, "local table");
    check(P(0, 1, 100, 2, 100, 100, 4096, NONE, 40, 2, 1), 4096 + 8, 200, "remote table");
    check(P(MiB, 0, 1, 1, 0, 0, 0, NONE, 1, 1, 1), MiB, MiB, "local table");
    check(P(0, ~0ull, 1, 1, 0, 0, 0, NONE, 1, 1, 1), MiB, MiB, "remote table");
    check(P(0, ~0ull - 3, 8, 1, 0, 0, 0, NONE, 1, 1, 1), MiB, ~0ull, "remote table");   // offset + row_bytes wraps
    check(P(0, 0, ~0ull, 1, 0, 0, 8, NONE, 1, 1, 1), MiB, MiB, "local table");
    check(P(0, 0, 1, 1, big, 1, 8192, NONE, max32, 1, 1), MiB, MiB, "local table");       // (2^32 - 2) * 2^63 wraps to 0
    check(P(0, 0, 1, 1, 1, big, NONE, 8192, 1, max32, 1), MiB, MiB, "remote table");
    check(P(0, 0, 8, 1, big + 8, 8, 8192, NONE, 3, 1, 1), MiB, MiB, "local table");       // 2 * (2^63 + 8) wraps to 16
    check(P(0, 0, 8, 1, 8, big / 2, NONE, 8192, 1, 5, 1), MiB, MiB, "remote table");      // 4 * 2^62 wraps to 0
    check(P(16, 16, 16, 1, ~0ull, ~0ull, 0, 8, max32, max32, 1), ~0ull, ~0ull, "local table");
    // a side without an index needs a table of at least `rows` rows
    check(P(0, 0, 16, 5, 16, 16, NONE, 4096, 4, 8, 1), MiB, MiB, "local side has no index");
    check(P(0, 0, 16, 5, 16, 16, 4096, NONE, 8, 4, 1), MiB, MiB, "remote side has no index");
    check(P(0, 0, 16, 5, 16, 16, 4096, 8192, 4, 4, 1), MiB, MiB, nullptr, 80);            // both indexed: any table size
    // index arrays: alignment to the element size, and inside the local half without overflow
    check(P(0, 0, 16, 4, 16, 16, NONE, 4098, 4, 8, 1), MiB, MiB, "not a multiple");
    check(P(0, 0, 16, 4, 16, 16, NONE, 4100, 4, 8, 1, OCM_INDEX_I64), MiB, MiB, "not a multiple");
    check(P(0, 0, 16, 4, 16, 16, NONE, 4100, 4, 8, 1, OCM_INDEX_I32), MiB, MiB, nullptr, 64);
    check(P(0, 0, 16, 4, 16, 16, 4092, NONE, 8, 4, 1), MiB, MiB, nullptr, 64);
    check(P(0, 0, 16, 4, 16, 16, NONE, MiB - 12, 4, 8, 1), MiB, MiB, "index array");
    check(P(0, 0, 16, 4, 16, 16, NONE, MiB - 16, 4, 8, 1), MiB, MiB, nullptr, 64);
    check(P(0, 0, 16, 4, 16, 16, NONE, MiB - 24, 4, 8, 1, OCM_INDEX_I64), MiB, MiB, "index array");
    check(P(0, 0, 16, 4, 16, 16, ~0ull - 7, NONE, 8, 4, 1, OCM_INDEX_I64), MiB, MiB, "index array");   // off + rows * 8 wraps
    check(P(0, 0, 1, max32, 1, 1, NONE, 1ull << 62, max32, 8, 1, OCM_INDEX_I64), ~0ull - 1, ~0ull, nullptr, max32);
    check(P(0, 0, 1, max32, 1, 1, NONE, ~0ull - 15, max32, 8, 1, OCM_INDEX_I64), ~0ull - 1, ~0ull, "index array");
    // a get writes its local table: neither array may lie in it; a put only reads
    check(P(0, 0, 16, 4, 16, 16, NONE, 60, 4, 8, 0), MiB, MiB, "overlaps");
    check(P(0, 0, 16, 4, 16, 16, NONE, 64, 4, 8, 0), MiB, MiB, nullptr, 64);
    check(P(64, 0, 16, 4, 16, 16, NONE, 48, 4, 8, 0), MiB, MiB, nullptr, 64);
    check(P(64, 0, 16, 4, 16, 16, NONE, 52, 4, 8, 0), MiB, MiB, "overlaps");
    check(P(64, 0, 16, 4, 32, 16, 4096, 128, 8, 8, 0), MiB, MiB, "remote index array");  // between rows of a padded table: still its range
    check(P(64, 0, 16, 4, 32, 16, 100, 4096, 8, 8, 0), MiB, MiB, "local index array");
    check(P(0, 0, 16, 4, 16, 16, NONE, 60, 4, 8, 1), MiB, MiB, nullptr, 64);
    // empty ops: fine whatever else they say
    check(P(~0ull, ~0ull, 0, 9, 0, 0, 3, 3, ~0ull, ~0ull, 0, 9), MiB, MiB, nullptr, 0);
    check(P(~0ull, ~0ull, 9, 0, 0, 0, NONE, NONE, ~0ull, ~0ull, 1, 0), MiB, MiB, nullptr, 0);
    // the descriptor of an empty op takes no tiles
    XferIndexedOp e = indexed_op(P(1, 2, 0, 9, 0, 0, 3, 3, 5, 5));
    CHECK(e.rows == 0 && e.row_bytes == 0 && xfer_indexed_plan(&e, 1, 12) == 0, "empty op's descriptor");
    const XferIndexedOp d = indexed_op(P(1, 2, 3, 4, 5, 6, NONE, 8, 9, 10, 1, OCM_INDEX_I64));
    CHECK(d.lin_off == 1 && d.rem_off == 2 && d.row_bytes == 3 && d.rows == 4 && d.lin_stride == 5 && d.rem_stride == 6 &&
              d.lin_idx_off == NONE && d.rem_idx_off == 8 && d.lin_rows == 9 && d.rem_rows == 10 && d.put == 1 &&
              d.index_type == OCM_INDEX_I64,
          "descriptor fields");
}

// A list: first_tile is the prefix sum, empty ops take no tiles, and every wave's
// starting op is the op of its first tile.
void test_plan() {
    std::vector<XferIndexedOp> v(7, XferIndexedOp{});
    const uint64_t rb[] = {4097, 0, 100, 8192, 5, 1, 0};
    const uint32_t nr[] = {3, 4, 0, 2, 7, 1, 2};
    for (size_t i = 0; i < v.size(); i++) {
        v[i].row_bytes = nr[i] ? rb[i] : 0;
        v[i].rows = rb[i] ? nr[i] : 0;
    }
    const uint64_t total = xfer_indexed_plan(v.data(), (uint32_t)v.size(), 12);
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
            const XferIndexedOp &op = v[w[k]];
            CHECK(op.first_tile <= t && t < op.first_tile + indexed_tile_count(op), "wave %u of grid %u starts in op %u", k, grid,
                  w[k]);
        }
    }
    CHECK(sizeof(XferIndexedArgs::inline_ops) / sizeof(XferIndexedOp) == kIndexedInlineOps && kIndexedInlineOps == 16, "inline ops");
}

}  // namespace

int main() {
    struct {
        const char *name;
        void (*fn)();
    } parts[] = {{"geometry", test_geometry}, {"bounds", test_bounds}, {"validator", test_validator}, {"plan", test_plan}};
    for (auto &p : parts) {
        const int before = failures;
        p.fn();
        std::printf("%s %s\n", failures == before ? "PASS" : "FAILED", p.name);
    }
    std::printf("%d failure(s)\n", failures);
    return failures ? 1 : 0;
}
