// The indexed converting ops' shared header (ocm/quant_indexed.h) on the CPU: the
// functions the kernel and the host side call. The tiles the descriptor yields for picked
// rows against the plain converting ops the call is defined by (one per in-range row),
// the plan, every rule of the validator with its boundaries and overflow probes, and the
// host path's reading of index arrays against a brute-force expansion. Stand-alone: it
// links nothing of the library, so the build also makes an ASan + UBSan copy of it.
#include <climits>
#include <cstdio>
#include <cstring>
#include <vector>

#include "ocm/quant_indexed.h"

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
const uint32_t kFormats[] = {OCM_QUANT_MXFP8, OCM_QUANT_MXFP4};
const uint64_t NONE = OCM_INDEX_NONE;

uint64_t record_up32(uint64_t elems, uint32_t fmt) { return (quant_record_bytes(elems, fmt) + 31) / 32 * 32; }

ocm_quant_indexed_params P(uint64_t lo, uint64_t ro, uint64_t re, uint64_t rows, uint64_t ls, uint64_t rs, uint64_t lidx,
                           uint64_t ridx, uint64_t lr, uint64_t rr, int put = 0, uint32_t type = OCM_INDEX_I32,
                           uint32_t dtype = OCM_QUANT_FP16) {
    ocm_quant_indexed_params p{};
    p.local_offset = lo;
    p.remote_offset = ro;
    p.row_elems = re;
    p.rows = rows;
    p.local_stride = ls;
    p.remote_stride = rs;
    p.local_index_offset = lidx;
    p.remote_index_offset = ridx;
    p.local_rows = lr;
    p.remote_rows = rr;
    p.op_flag = put;
    p.index_type = type;
    p.dtype = dtype;
    return p;
}

// The kernel's walk over every tile of `op` with the index arrays lidx / ridx (empty: that
// side has none), from one first tile per "wave": every tile of an in-range row is tile k
// of the row's plain converting op, cut as xfer_quant_kernel cuts it (e0 = k <<
// kQuantTileShift, elements at lin_off + 2 e0, codes at rem_off + (e0 >> code_shift), scale
// bytes at rem_off + (len >> code_shift) + e0 / 32); every element of such a row is
// converted once, and rows with an index outside its table yield no tile and are counted once.
void check_op(XferQuantIndexedOp op, const std::vector<int64_t> &lidx, const std::vector<int64_t> &ridx, uint64_t *tiles_seen,
              uint64_t *skips_seen) {
    const uint32_t cs = quant_code_shift(op.dtype);
    const uint64_t total = xfer_quant_indexed_plan(&op, 1, kQuantTileShift);
    CHECK(op.first_tile == 0 && total == (uint64_t)op.rows * quant_tile_count(op.row_elems), "plan");
    CHECK(op.tiles_per_row == (op.row_elems + kQuantTileElems - 1) / kQuantTileElems, "tiles_per_row %u for %u elements",
          op.tiles_per_row, op.row_elems);
    std::vector<uint8_t> cover((size_t)op.rows * op.row_elems, 0);  // how often element e of the op's row j was converted
    std::vector<uint8_t> counted(op.rows, 0);
    const uint64_t cuts[4] = {0, total / 3, total - total / 4, total};
    for (int wv = 0; wv < 3; wv++) {
        uint64_t j = 0, lr = 0, rr = 0;
        uint32_t k = 0;
        bool enter = true, ok = false;
        if (cuts[wv] < cuts[wv + 1]) list_locate(op.tiles_per_row, cuts[wv], &j, &k);
        for (uint64_t t = cuts[wv]; t < cuts[wv + 1]; t++) {
            CHECK(j == t / op.tiles_per_row && k == t % op.tiles_per_row, "tile %llu is not row %llu piece %u", (ull)t, (ull)j, k);
            if (enter) {
                enter = false;
                lr = lidx.empty() ? j : (uint64_t)lidx[(size_t)j];
                rr = ridx.empty() ? j : (uint64_t)ridx[(size_t)j];
                ok = indexed_in_range(lr, op.lin_rows) && indexed_in_range(rr, op.rem_rows);
                if (!ok && k == 0) counted[(size_t)j]++;
            }
            if (ok) {
                const QuantTileLoc q = quant_indexed_tile(op, lr, rr, k, cs);
                (*tiles_seen)++;
                // the plain converting op of this row
                const uint64_t lin_off = op.lin_off + lr * op.lin_stride, rem_off = op.rem_off + rr * op.rem_stride;
                const uint64_t len = op.row_elems, e0 = (uint64_t)k << kQuantTileShift;
                const uint64_t ne = len - e0 < kQuantTileElems ? len - e0 : kQuantTileElems;
                CHECK(q.ne == ne && q.ne > 0 && q.ne % 32 == 0, "tile %llu: %u elements, the plain op has %llu", (ull)t, q.ne, (ull)ne);
                CHECK(q.lin_off == lin_off + 2 * e0, "tile %llu: elements at %llu", (ull)t, (ull)q.lin_off);
                CHECK(q.codes == rem_off + (e0 >> cs), "tile %llu: codes at %llu", (ull)t, (ull)q.codes);
                CHECK(q.scales == rem_off + (len >> cs) + (e0 >> 5), "tile %llu: scale bytes at %llu", (ull)t, (ull)q.scales);
                // the same place the strided rule gives for that row of a strided op with these tables
                XferQuantStridedOp so{};
                so.lin_off = lin_off;
                so.rem_off = rem_off;
                so.row_elems = op.row_elems;
                const QuantTileLoc s = quant_strided_tile(so, 0, k, cs);
                CHECK(s.ne == q.ne && s.lin_off == q.lin_off && s.codes == q.codes && s.scales == q.scales,
                      "tile %llu differs from the strided rule", (ull)t);
                // what the tile bodies rest on: 16-byte vectors of source and codes
                CHECK(q.lin_off % 16 == 0 && q.codes % 16 == 0, "tile %llu: unaligned vectors", (ull)t);
                // inside the row's record
                CHECK(q.codes + (q.ne >> cs) <= rem_off + (len >> cs) && q.scales + q.ne / 32 <= rem_off + quant_record_bytes(len, op.dtype),
                      "tile %llu leaves its record", (ull)t);
                if (e0 + q.ne <= len)
                    for (uint64_t e = 0; e < q.ne; e++) cover[(size_t)(j * op.row_elems + e0 + e)]++;
            }
            if (list_next_piece(op.tiles_per_row, &j, &k)) enter = true;
        }
    }
    for (uint32_t j = 0; j < op.rows; j++) {
        const uint64_t lr = lidx.empty() ? j : (uint64_t)lidx[j], rr = ridx.empty() ? j : (uint64_t)ridx[j];
        const bool ok = lr < op.lin_rows && rr < op.rem_rows;  // the rule, written apart from indexed_in_range
        size_t bad = 0;
        for (uint64_t e = 0; e < op.row_elems; e++) bad += cover[(size_t)(j * op.row_elems + e)] != (ok ? 1 : 0);
        CHECK(bad == 0, "row %u (%s): %zu elements not converted exactly %d time(s)", j, ok ? "in range" : "out of range", bad,
              ok ? 1 : 0);
        CHECK(counted[j] == (ok ? 0 : 1), "row %u counted as skipped %u time(s)", j, counted[j]);
        *skips_seen += !ok;
    }
}

void test_tile_rule() {
    uint64_t ops = 0, tiles = 0, skips = 0;
    // five rows out of tables of seven: a permutation, duplicates, and out-of-range values among good ones
    const std::vector<int64_t> perm = {4, 0, 6, 2, 5}, dup = {3, 3, 0, 3, 6}, none = {};
    const std::vector<int64_t> bad = {-1, 6, 7, 2, (int64_t)1 << 40};
    const std::vector<int64_t> *pairs[][2] = {{&none, &perm}, {&perm, &none}, {&dup, &perm}, {&none, &bad}, {&bad, &dup}, {&perm, &bad}};
    for (uint32_t fmt : kFormats)
        for (uint64_t re : kRowElems) {
            const uint64_t rec = record_up32(re, fmt);
            const uint64_t lstrides[] = {2 * re, 2 * re + 16};
            const uint64_t rstrides[] = {rec, rec + 32, rec + 96};
            for (uint64_t ls : lstrides)
                for (uint64_t rs : rstrides)
                    for (uint64_t ro : {(uint64_t)0, (uint64_t)2 * 4096 - 64, (uint64_t)5 * 4096 - 2080})
                        for (auto &pr : pairs) {
                            const uint64_t lidx = pr[0]->empty() ? NONE : (1ull << 29), ridx = pr[1]->empty() ? NONE : (1ull << 29) + 64;
                            const ocm_quant_indexed_params p =
                                P(48, ro, re, 5, ls, rs, lidx, ridx, 7, 7, (int)(ops % 2), OCM_INDEX_I64, OCM_QUANT_FP16 | fmt);
                            uint64_t src = 0, wire = 0;
                            char why[256] = "";
                            CHECK(quant_indexed_check_op(p, 1ull << 30, 1ull << 30, &src, &wire, why, sizeof(why)) == 0, "%s", why);
                            CHECK(src == 2 * re * 5 && wire == quant_record_bytes(re, fmt) * 5, "src %llu wire %llu", (ull)src, (ull)wire);
                            const XferQuantIndexedOp op = quant_indexed_op(p);
                            CHECK(op.rows == 5 && op.row_elems == re && op.put == ops % 2 && op.dtype == (OCM_QUANT_FP16 | fmt) &&
                                      op.lin_rows == 7 && op.rem_rows == 7 && op.lin_idx_off == lidx && op.rem_idx_off == ridx &&
                                      op.index_type == OCM_INDEX_I64 && op.lin_off == 48 && op.rem_off == ro && op.lin_stride == ls &&
                                      op.rem_stride == rs,
                                  "descriptor");
                            check_op(op, *pr[0], *pr[1], &tiles, &skips);
                            ops++;
                        }
        }
    CHECK(tiles > ops && skips > 0, "the grid never cut a row in tiles or never skipped a row");
    std::printf("tile_rule: %llu ops, %llu tiles, %llu rows skipped\n", (ull)ops, (ull)tiles, (ull)skips);
}

// A list: first_tile is the prefix sum, empty ops take no tiles, and every wave's
// starting op is the op of its first tile.
void test_plan() {
    const uint64_t re[] = {4128, 0, 32, 2048, 2080, 1024, 0};
    const uint64_t nr[] = {3, 4, 0, 2, 7, 1, 2};
    std::vector<XferQuantIndexedOp> v;
    for (size_t i = 0; i < 7; i++)
        v.push_back(quant_indexed_op(P(0, 0, re[i], nr[i], 2 * re[i], record_up32(re[i], 0), NONE, 1 << 20, 8, 8)));
    CHECK(v[1].rows == 0 && v[1].row_elems == 0 && v[1].rem_rows == 0 && v[2].rows == 0 && v[2].row_elems == 0, "empty ops keep nothing");
    const uint64_t total = xfer_quant_indexed_plan(v.data(), (uint32_t)v.size(), kQuantTileShift);
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
            const XferQuantIndexedOp &op = v[w[k]];
            CHECK(op.first_tile <= t0 && t0 < op.first_tile + quant_indexed_tile_count(op), "wave %u of grid %u starts in op %u", k,
                  grid, w[k]);
        }
    }
    // the inline capacity is the most the kernel arguments hold
    CHECK(sizeof(XferQuantIndexedArgs::inline_ops) / sizeof(XferQuantIndexedOp) == kQuantIndexedInlineOps, "inline ops");
    CHECK(sizeof(XferQuantIndexedArgs) <= kKernargLimit && sizeof(XferQuantIndexedArgs) + sizeof(XferQuantIndexedOp) > kKernargLimit,
          "the launch arguments take %zu bytes", sizeof(XferQuantIndexedArgs));
}

int check(const ocm_quant_indexed_params &p, uint64_t lb, uint64_t rb, const char *want_in_msg, uint64_t want_src = 0,
          uint64_t want_wire = 0) {
    char why[256] = "";
    uint64_t src = 77, wire = 77;
    const int rc = quant_indexed_check_op(p, lb, rb, &src, &wire, why, sizeof(why));
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
    // a plain lookup: 4 rows of 64 elements (128 local bytes, 66 record bytes at stride 96) out of 8, ids behind the rows.
    // The remote table's last row ends exactly at the half's end, and so does the index array.
    check(P(0, 0, 64, 4, 128, 96, NONE, 512, 4, 8), 528, 7 * 96 + 66, nullptr, 512, 4 * 66);
    check(P(0, 0, 64, 4, 128, 96, NONE, 512, 4, 8), 528, 7 * 96 + 65, "remote table");  // the table's last row, not the op's
    check(P(0, 0, 64, 4, 128, 96, NONE, 512, 4, 8), 527, MiB, "remote index array");
    check(P(0, 0, 64, 4, 128, 96, NONE, 512, 4, 8, 0, OCM_INDEX_I64), 543, MiB, "remote index array");
    check(P(0, 0, 64, 4, 128, 96, NONE, 512, 4, 8, 0, OCM_INDEX_I64), 544, MiB, nullptr, 512, 4 * 66);
    check(P(0, 0, 64, 4, 128, 96, NONE, 512, 4, 8, 0, OCM_INDEX_I32, OCM_QUANT_FP16 | OCM_QUANT_MXFP4), 528, 7 * 96 + 34, nullptr, 512, 4 * 34);
    check(P(0, 0, 64, 4, 128, 96, NONE, 512, 4, 8, 0, OCM_INDEX_I32, OCM_QUANT_FP16 | OCM_QUANT_MXFP4), 528, 7 * 96 + 33, "remote table");
    // a scatter whose local table's last row ends exactly at the half's end
    check(P(64, 0, 64, 2, 128, 96, 0, NONE, 4, 2, 1), 64 + 3 * 128 + 128, 96 + 66, nullptr, 256, 2 * 66);
    check(P(64, 0, 64, 2, 128, 96, 0, NONE, 4, 2, 1), 64 + 3 * 128 + 127, 96 + 66, "local table");
    // dtype bits, reserved, row size
    check(P(0, 0, 64, 1, 128, 96, NONE, 512, 1, 8, 0, OCM_INDEX_I32, 0), MiB, MiB, "element type");
    check(P(0, 0, 64, 1, 128, 96, NONE, 512, 1, 8, 0, OCM_INDEX_I32, 3), MiB, MiB, "element type");
    check(P(0, 0, 64, 1, 128, 96, NONE, 512, 1, 8, 0, OCM_INDEX_I32, OCM_QUANT_FP16 | 0x200), MiB, MiB, "format");
    check(P(0, 0, 64, 1, 128, 96, NONE, 512, 1, 8, 0, OCM_INDEX_I32, OCM_QUANT_FP16 | 0x10000), MiB, MiB, "dtype");
    check(P(0, 0, 64, 1, 128, 96, NONE, 512, 1, 8, 0, OCM_INDEX_I32, OCM_QUANT_BF16), MiB, MiB, nullptr, 128, 66);
    {
        ocm_quant_indexed_params p = P(0, 0, 64, 1, 128, 96, NONE, 512, 1, 8);
        p.reserved = 1;
        check(p, MiB, MiB, "reserved");
    }
    check(P(0, 0, 33, 1, 128, 96, NONE, 512, 1, 8), MiB, MiB, "multiple of 32");
    check(P(0, 0, 1ull << 31, 1, 0, 0, NONE, 0, 1, 1, 1), ~0ull, ~0ull, "2^31");
    check(P(0, 0, (1ull << 31) - 32, 1, 0, 0, NONE, 1ull << 33, 1, 1, 1), ~0ull, ~0ull, nullptr, (1ull << 32) - 64,
          (1ull << 31) - 32 + (1ull << 26) - 1);
    // index type and presence
    check(P(0, 0, 64, 4, 128, 96, NONE, 512, 4, 8, 0, 0), MiB, MiB, "index_type");
    check(P(0, 0, 64, 4, 128, 96, NONE, 512, 4, 8, 0, 3), MiB, MiB, "index_type");
    check(P(0, 0, 64, 4, 128, 96, NONE, NONE, 4, 8), MiB, MiB, "no index on either side");
    // counts of 2^32 and more
    check(P(0, 0, 32, 1ull << 32, 64, 64, NONE, 0, max32, 8, 1), ~0ull, ~0ull, "2^32");
    check(P(0, 0, 32, ~0ull, 64, 64, NONE, 0, max32, 8, 1), ~0ull, ~0ull, "2^32");
    check(P(0, 0, 32, 4, 64, 64, 4096, NONE, 1ull << 32, 8, 1), ~0ull, ~0ull, "local table of");
    check(P(0, 0, 32, 4, 64, 64, NONE, 4096, 8, 1ull << 32, 1), ~0ull, ~0ull, "remote table of");
    // alignment: 16 on the local side, 32 on the remote side
    check(P(8, 0, 32, 2, 64, 64, NONE, 4096, 2, 2, 1), MiB, MiB, "local offset");
    check(P(0, 16, 32, 2, 64, 64, NONE, 4096, 2, 2, 1), MiB, MiB, "remote offset");
    check(P(0, 0, 32, 2, 72, 64, NONE, 4096, 2, 2, 1), MiB, MiB, "local stride");
    check(P(0, 0, 32, 2, 64, 80, NONE, 4096, 2, 2, 1), MiB, MiB, "remote stride");
    check(P(16, 32, 32, 2, 80, 96, NONE, 4096, 2, 2, 1), MiB, MiB, nullptr, 128, 66);
    // strides below the row (2 * row_elems local bytes, the record's remote bytes), read only for tables of more than one row
    check(P(0, 0, 64, 2, 112, 96, NONE, 4096, 2, 2, 1), MiB, MiB, "local stride");
    check(P(0, 0, 64, 2, 128, 64, NONE, 4096, 2, 2, 1), MiB, MiB, "remote stride");  // 64 < 66
    check(P(0, 0, 64, 2, 128, 64, NONE, 4096, 2, 2, 1, OCM_INDEX_I32, OCM_QUANT_FP16 | OCM_QUANT_MXFP4), MiB, MiB, nullptr, 256, 68);  // 64 >= 34
    check(P(0, 0, 64, 2, 128, 32, NONE, 4096, 2, 2, 1, OCM_INDEX_I32, OCM_QUANT_FP16 | OCM_QUANT_MXFP4), MiB, MiB, "remote stride");
    check(P(0, 0, 1024, 2, 2048, 1024, NONE, 8192, 2, 2, 1), MiB, MiB, "remote stride");
    check(P(0, 0, 1024, 2, 2048, 1056, NONE, 8192, 2, 2, 1), MiB, MiB, nullptr, 4096, 2112);
    check(P(0, 0, 64, 1, 0, 0, NONE, 4096, 1, 1, 1), 4100, 66, nullptr, 128, 66);  // one-row tables, stride 0
    check(P(0, 0, 64, 3, 0, 0, 4096, 8192, 1, 1, 1), MiB, 66, nullptr, 384, 198);  // three rows naming the one row there is
    // the table's last row: one byte too many, and sums and products that wrap 64 bits
    check(P(16, 0, 64, 2, 128, 96, 4096, NONE, 32, 2, 1), 4096 + 8, 96 + 66, "local table");
    check(P(0, 32, 64, 2, 128, 96, 4096, NONE, 31, 2, 1), 4096 + 8, 96 + 66 + 31, "remote table");
    check(P(MiB, 0, 32, 1, 0, 0, 0, NONE, 1, 1, 1), MiB, MiB, "local table");
    check(P(0, ~0ull - 31, 32, 1, 0, 0, 0, NONE, 1, 1, 1), MiB, MiB, "remote table");
    check(P(0, ~0ull - 31, 32, 1, 0, 0, 0, NONE, 1, 1, 1), MiB, ~0ull, "remote table");  // offset + record bytes wraps
    check(P(~0ull - 15, 0, 32, 1, 0, 0, 0, NONE, 1, 1, 1), ~0ull, MiB, "local table");
    check(P(0, 0, 32, 1, big, 64, 8192, NONE, max32, 1, 1), MiB, MiB, "local table");   // (2^32 - 2) * 2^63 wraps to 0
    check(P(0, 0, 32, 1, 64, big, NONE, 8192, 1, max32, 1), MiB, MiB, "remote table");
    check(P(0, 0, 32, 1, big + 64, 64, 8192, NONE, 3, 1, 1), MiB, MiB, "local table");  // 2 * (2^63 + 64) wraps to 128
    check(P(0, 0, 32, 1, 64, big + 64, NONE, 8192, 1, 3, 1), MiB, MiB, "remote table");
    check(P(0, 0, 32, 1, big / 2, 64, 8192, NONE, 5, 1, 1), MiB, MiB, "local table");   // 4 * 2^62 wraps to 0
    check(P(0, 0, 32, 1, 64, big / 2, NONE, 8192, 1, 5, 1), MiB, MiB, "remote table");
    check(P(16, 32, 32, 1, ~0ull - 15, ~0ull - 31, 0, 8, max32, max32, 1), ~0ull, ~0ull, "local table");
    check(P(0, 0, 32, 4, 64, 64, NONE, 1ull << 20, max32, max32, 1), max32 * 64, (max32 - 1) * 64 + 33, nullptr, 256, 132);  // the largest tables
    check(P(0, 0, 32, 4, 64, 64, NONE, 1ull << 20, max32, max32, 1), max32 * 64 - 1, max32 * 64, "local table");
    check(P(0, 0, 32, 4, 64, 64, NONE, 1ull << 20, max32, max32, 1), max32 * 64, (max32 - 1) * 64 + 32, "remote table");
    // a side without an index needs a table of at least `rows` rows
    check(P(0, 0, 32, 5, 64, 64, NONE, 4096, 4, 8, 1), MiB, MiB, "local side has no index");
    check(P(0, 0, 32, 5, 64, 64, 4096, NONE, 8, 4, 1), MiB, MiB, "remote side has no index");
    check(P(0, 0, 32, 5, 64, 64, 4096, 8192, 4, 4, 1), MiB, MiB, nullptr, 320, 165);  // both indexed: any table size
    // index arrays: alignment to the element size, and inside the local half without overflow
    check(P(0, 0, 32, 4, 64, 64, NONE, 4098, 4, 8, 1), MiB, MiB, "not a multiple");
    check(P(0, 0, 32, 4, 64, 64, NONE, 4100, 4, 8, 1, OCM_INDEX_I64), MiB, MiB, "not a multiple");
    check(P(0, 0, 32, 4, 64, 64, NONE, 4100, 4, 8, 1, OCM_INDEX_I32), MiB, MiB, nullptr, 256, 132);
    check(P(0, 0, 32, 4, 64, 64, NONE, MiB - 12, 4, 8, 1), MiB, MiB, "remote index array");
    check(P(0, 0, 32, 4, 64, 64, NONE, MiB - 16, 4, 8, 1), MiB, MiB, nullptr, 256, 132);  // ends exactly at the half's end
    check(P(0, 0, 32, 4, 64, 64, MiB - 24, NONE, 8, 4, 1, OCM_INDEX_I64), MiB, MiB, "local index array");
    check(P(0, 0, 32, 4, 64, 64, ~0ull - 7, NONE, 8, 4, 1, OCM_INDEX_I64), MiB, MiB, "local index array");  // off + rows * 8 wraps
    check(P(0, 0, 32, max32, 64, 64, NONE, ~0ull - 15, max32, 8, 1, OCM_INDEX_I64), ~0ull - 1, ~0ull, "remote index array");
    check(P(0, 0, 32, max32, 64, 64, NONE, 1ull << 62, max32, 8, 1, OCM_INDEX_I64), ~0ull - 1, ~0ull, nullptr, max32 * 64, max32 * 33);
    // a get writes its local table: neither array may lie in it; a put only reads
    check(P(0, 0, 32, 4, 64, 64, NONE, 252, 4, 8, 0), MiB, MiB, "overlaps");
    check(P(0, 0, 32, 4, 64, 64, NONE, 256, 4, 8, 0), MiB, MiB, nullptr, 256, 132);
    check(P(64, 0, 32, 4, 64, 64, NONE, 48, 4, 8, 0), MiB, MiB, nullptr, 256, 132);
    check(P(64, 0, 32, 4, 64, 64, NONE, 52, 4, 8, 0), MiB, MiB, "overlaps");
    check(P(64, 0, 32, 4, 128, 64, 4096, 128, 8, 8, 0), MiB, MiB, "remote index array");  // between rows of a padded table: still its range
    check(P(64, 0, 32, 4, 128, 64, 132, 4096, 8, 8, 0), MiB, MiB, "local index array");
    check(P(0, 0, 32, 4, 64, 64, NONE, 252, 4, 8, 1), MiB, MiB, nullptr, 256, 132);
    // empty ops: fine wherever they point (the dtype, reserved and the row size are still read)
    check(P(~0ull, ~0ull, 0, 9, 1, 1, 3, 3, ~0ull, ~0ull, 0, 9), MiB, MiB, nullptr, 0, 0);
    check(P(~0ull, ~0ull, 64, 0, 1, 1, NONE, NONE, ~0ull, ~0ull, 1, 0), MiB, MiB, nullptr, 0, 0);
    check(P(~0ull, ~0ull, 0, 9, 1, 1, 3, 3, ~0ull, ~0ull, 0, 9, 7), MiB, MiB, "element type");
    // the descriptor of an empty op takes no tiles
    XferQuantIndexedOp e = quant_indexed_op(P(16, 32, 0, 9, 0, 0, 3, 3, 5, 5));
    CHECK(e.rows == 0 && e.row_elems == 0 && xfer_quant_indexed_plan(&e, 1, kQuantTileShift) == 0, "empty op's descriptor");
}

// What the host path does with the index arrays as they lie in memory
// (quant_indexed_host_row: indexed_load_host, indexed_in_range, then one plain converting
// op per row that passed), against an
// expansion that works on the values as signed integers.
void test_host_model() {
    const int64_t vals64[] = {3, -1, 0, 7, 8, INT64_MIN, 1ll << 32, 5, (1ll << 40) + 2, 6};
    const int32_t vals32[] = {3, -1, 0, 7, 8, INT32_MIN, INT32_MAX, 5, -4, 6};
    const uint64_t rows = 10;
    // the local half: the local-side indices at 0, the remote-side ones (the same values, reversed) at 256
    std::vector<char> half(1024, 0);
    for (uint32_t type : {(uint32_t)OCM_INDEX_I32, (uint32_t)OCM_INDEX_I64})
        for (int which = 0; which < 3; which++) {  // remote index only, local only, both
            std::vector<int64_t> v(rows);
            for (uint64_t j = 0; j < rows; j++) v[j] = type == OCM_INDEX_I64 ? vals64[j] : (int64_t)vals32[j];
            for (uint64_t j = 0; j < rows; j++) {
                if (type == OCM_INDEX_I64) {
                    std::memcpy(half.data() + 8 * j, &v[j], 8);
                    std::memcpy(half.data() + 256 + 8 * j, &v[rows - 1 - j], 8);
                } else {
                    const int32_t a = (int32_t)v[j], b = (int32_t)v[rows - 1 - j];
                    std::memcpy(half.data() + 4 * j, &a, 4);
                    std::memcpy(half.data() + 256 + 4 * j, &b, 4);
                }
            }
            const uint64_t lrows = which == 0 ? 16 : 8, rrows = which == 1 ? 16 : 7;
            const ocm_quant_indexed_params p = P(512, 64, 32, rows, 64, 96, which == 0 ? NONE : 0, which == 1 ? NONE : 256, lrows, rrows, 1, type);
            // the host path
            std::vector<ocm_quant_params> got;
            uint64_t skipped = 0;
            for (uint64_t j = 0; j < rows; j++) {
                ocm_quant_params q;
                if (quant_indexed_host_row(p, half.data(), j, &q))
                    got.push_back(q);
                else
                    skipped++;
            }
            // brute force, on signed values
            std::vector<ocm_quant_params> want;
            uint64_t want_skipped = 0;
            for (uint64_t j = 0; j < rows; j++) {
                const int64_t lr = which == 0 ? (int64_t)j : v[j], rr = which == 1 ? (int64_t)j : v[rows - 1 - j];
                if (lr < 0 || lr >= (int64_t)lrows || rr < 0 || rr >= (int64_t)rrows) {
                    want_skipped++;
                    continue;
                }
                want.push_back({512 + (uint64_t)lr * 64, 64 + (uint64_t)rr * 96, 32, 1, OCM_QUANT_FP16});
            }
            CHECK(skipped == want_skipped && got.size() == want.size(), "type %u case %d: %llu skipped, %zu moved; want %llu, %zu", type,
                  which, (ull)skipped, got.size(), (ull)want_skipped, want.size());
            CHECK(want_skipped > 0 && !want.empty(), "type %u case %d checks nothing", type, which);
            for (size_t n = 0; n < got.size() && n < want.size(); n++)
                CHECK(got[n].local_offset == want[n].local_offset && got[n].remote_offset == want[n].remote_offset &&
                          got[n].elems == want[n].elems && got[n].op_flag == want[n].op_flag && got[n].dtype == want[n].dtype,
                      "type %u case %d: plain op %zu differs", type, which, n);
        }
}

}  // namespace

int main() {
    struct {
        const char *name;
        void (*fn)();
    } parts[] = {{"tile_rule", test_tile_rule}, {"plan", test_plan}, {"validator", test_validator}, {"host_model", test_host_model}};
    for (auto &p : parts) {
        const int before = failures;
        p.fn();
        std::printf("%s %s\n", failures == before ? "PASS" : "FAILED", p.name);
    }
    std::printf("%d failure(s)\n", failures);
    return failures ? 1 : 0;
}
