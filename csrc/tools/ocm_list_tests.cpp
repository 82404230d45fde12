// The plan every descriptor list shares (ocm/list.h: list_plan, list_wave_ops,
// list_wave_range) under each kind's tile-count rule, as the library calls it
// (xfer_batch_plan, xfer_quant_plan, xfer_strided_plan, acc_plan), against a brute-force
// walk of every tile; and the walk the row kernels make through a list (list_enter_op,
// list_locate, list_next_piece: the functions they call) against the enumeration of its
// ops, rows and pieces. Stand-alone: it links nothing of the library, so the build also
// makes an ASan + UBSan copy of it.
#include <cstdio>
#include <vector>

#include "ocm/acc.h"
#include "ocm/list.h"
#include "ocm/quant.h"
#include "ocm/strided.h"
#include "ocm/xfer.h"

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

uint64_t rng_state = 1;
uint64_t rnd(uint64_t below) {  // a fixed sequence
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (rng_state >> 33) % below;
}

const uint32_t kCounts[] = {1, 2, 24, 25, 48, 49, 300};
const uint32_t kGrids[] = {1, 2, 3, 128, 2048};

// Which ops of a list of n are forced empty: none; the first, the last and two adjacent
// ones in the middle; the first only; the last only.
bool forced_empty(int variant, uint32_t i, uint32_t n) {
    const bool first = i == 0, last = i == n - 1, mid = i == n / 2 || i == n / 2 + 1;
    return variant == 1 ? (first || last || mid) : variant == 2 ? first : variant == 3 ? last : false;
}

// Pieces of `step` units, aligned to multiples of `step`, that [from, from + len) touches,
// counted one by one (from == 0: pieces cut from the op's own start).
uint64_t walk_aligned(uint64_t from, uint64_t len, uint64_t step) {
    uint64_t n = 0;
    for (uint64_t b = from; b < from + len; b = (b / step + 1) * step) n++;
    return n;
}

// One planned list against the brute force: `tiles[i]` is what a walk counted for op i.
template <class Op>
void check_list(const char *kind, const std::vector<Op> &v, uint64_t total, const std::vector<uint64_t> &tiles) {
    const uint32_t n = (uint32_t)v.size();
    // first_tile is the exclusive prefix sum, and tile -> op by brute force
    std::vector<uint32_t> op_of;
    uint64_t sum = 0;
    for (uint32_t i = 0; i < n; i++) {
        CHECK(v[i].first_tile == sum, "%s: first_tile of op %u of %u is %llu, the walk says %llu", kind, i, n,
              (unsigned long long)v[i].first_tile, (unsigned long long)sum);
        sum += tiles[i];
        op_of.insert(op_of.end(), (size_t)tiles[i], i);
    }
    CHECK(total == sum, "%s: total %llu of %u ops, the walk says %llu", kind, (unsigned long long)total, n,
          (unsigned long long)sum);
    if (total != sum) return;
    for (uint32_t grid : kGrids) {
        const uint32_t waves = grid * kListWaves;
        std::vector<uint32_t> start(waves, ~0u);
        list_wave_ops(v.data(), n, total, grid, start.data());
        std::vector<uint8_t> owners((size_t)total, 0);
        uint64_t cursor = 0;
        for (uint32_t w = 0; w < waves; w++) {
            uint64_t t0, t1;
            list_wave_range(w, grid, total, &t0, &t1);
            CHECK(start[w] < n, "%s: wave %u of grid %u starts in op %u of %u", kind, w, grid, start[w], n);
            if (t0 >= t1 || start[w] >= n) continue;
            CHECK(t0 == cursor && t1 <= total, "%s: wave %u of grid %u has [%llu, %llu), the tiles before it end at %llu", kind,
                  w, grid, (unsigned long long)t0, (unsigned long long)t1, (unsigned long long)cursor);
            if (t0 != cursor || t1 > total) return;
            cursor = t1;
            // the starting op contains the wave's first tile
            const Op &op = v[start[w]];
            CHECK(op.first_tile <= t0 && t0 < op.first_tile + tiles[start[w]], "%s: wave %u of grid %u (tile %llu) starts in op %u",
                  kind, w, grid, (unsigned long long)t0, start[w]);
            // the kernels' walks from there find the op of every tile of the range: the advance of
            // the kernels without rows, and list_enter_op as the row kernels call it
            uint32_t i = start[w], ir = start[w];
            uint64_t next = 0;
            for (uint64_t t = t0; t < t1; t++) {
                while (i + 1 < n && v[i + 1].first_tile <= t) i++;
                if (t >= next) next = list_enter_op(v.data(), n, t, &ir);
                CHECK(i == op_of[(size_t)t] && ir == i, "%s: grid %u tile %llu: the walks are in ops %u and %u, the tile belongs to op %u",
                      kind, grid, (unsigned long long)t, i, ir, op_of[(size_t)t]);
                CHECK(next > t && (ir + 1 == n ? next == ~0ull : next == v[ir + 1].first_tile),
                      "%s: grid %u tile %llu: the op after op %u is said to start at %llu", kind, grid, (unsigned long long)t, ir,
                      (unsigned long long)next);
                owners[(size_t)t]++;
            }
        }
        CHECK(cursor == total, "%s: grid %u: the ranges end at %llu of %llu tiles", kind, grid, (unsigned long long)cursor,
              (unsigned long long)total);
        size_t bad = 0;
        for (uint8_t c : owners) bad += c != 1;
        CHECK(bad == 0, "%s: grid %u: %zu of %llu tiles not in exactly one wave's range", kind, grid, bad,
              (unsigned long long)total);
    }
}

// Runs `make(i, empty)` for every list size and pattern of empty ops, then plan(v) and the checks.
template <class Op, class Make, class Plan, class Walk>
void each_list(const char *kind, Make make, Plan plan, Walk walk) {
    const int before = failures;
    uint64_t lists = 0, all_tiles = 0;
    for (uint32_t n : kCounts)
        for (int variant = 0; variant < 4; variant++) {
            std::vector<Op> v(n, Op{});
            for (uint32_t i = 0; i < n; i++) {
                make(&v[i], forced_empty(variant, i, n));
                v[i].first_tile = 0xdeadbeefull;  // the plan must write every one
            }
            const uint64_t total = plan(v.data(), n);
            std::vector<uint64_t> tiles(n);
            for (uint32_t i = 0; i < n; i++) tiles[i] = walk(v[i]);
            check_list(kind, v, total, tiles);
            lists++;
            all_tiles += total;
        }
    std::printf("%s: %llu lists, %llu tiles\n", kind, (unsigned long long)lists, (unsigned long long)all_tiles);
    if (failures == before) std::printf("PASS %s\n", kind);
}

// Byte copies: tiles aligned in striped coordinates (xfer_tile_count), none for an empty op.
void test_batch() {
    for (uint32_t shift : {12u, 8u}) {  // 4 KiB wave-tiles; a 256-byte stripe unit
        each_list<XferBatchOp>(
            shift == 12 ? "batch" : "batch_unit256",
            [](XferBatchOp *o, bool empty) {
                o->rem_off = rnd(1 << 20);  // unaligned, also for an empty op
                o->lin_off = rnd(1 << 20);
                o->len = empty || rnd(8) == 0 ? 0 : 1 + rnd(rnd(2) ? 20000 : 300);
                o->put = (uint32_t)rnd(2);
            },
            [shift](XferBatchOp *v, uint32_t n) { return xfer_batch_plan(v, n, shift); },
            [shift](const XferBatchOp &o) { return walk_aligned(o.rem_off, o.len, 1ull << shift); });
    }
}

// Converting ops: tiles of kQuantTileElems elements from the op's start.
void test_quant() {
    each_list<XferBatchOp>(
        "quant",
        [](XferBatchOp *o, bool empty) {
            o->rem_off = 32 * rnd(1 << 12);
            o->len = empty || rnd(8) == 0 ? 0 : 32 * (1 + rnd(rnd(2) ? 400 : 3));  // elements
            o->put = (uint32_t)rnd(2);
        },
        [](XferBatchOp *v, uint32_t n) { return xfer_quant_plan(v, n); },
        [](const XferBatchOp &o) { return walk_aligned(0, o.len, kQuantTileElems); });
}

// Accumulates: tiles of kAccTileElems elements from the op's start.
void test_acc() {
    each_list<XferBatchOp>(
        "acc",
        [](XferBatchOp *o, bool empty) {
            o->rem_off = 16 * rnd(1 << 12);
            o->len = empty || rnd(8) == 0 ? 0 : 4 * (1 + rnd(rnd(2) ? 1500 : 300));  // elements
            o->pad = kAccBf16;
        },
        [](XferBatchOp *v, uint32_t n) { return acc_plan(v, n); },
        [](const XferBatchOp &o) { return walk_aligned(0, o.len, kAccTileElems); });
}

// Strided ops: every row cut from its own start, rows * tiles_per_row (the plan fills tiles_per_row).
void test_strided() {
    const uint32_t shift = 12;
    each_list<XferStridedOp>(
        "strided",
        [](XferStridedOp *o, bool empty) {
            const bool e = empty || rnd(8) == 0;
            o->rem_off = rnd(1 << 20);
            o->row_bytes = e ? 0 : 1 + rnd(rnd(2) ? 9000 : 64);
            o->rows = e ? 0 : 1 + (uint32_t)rnd(5);
            o->lin_stride = o->rem_stride = o->row_bytes + rnd(100);
            o->tiles_per_row = 0xdeadbeefull;
        },
        [](XferStridedOp *v, uint32_t n) { return xfer_strided_plan(v, n, shift); },
        [](const XferStridedOp &o) {
            uint64_t tiles = 0;
            for (uint32_t r = 0; r < o.rows; r++) tiles += walk_aligned(0, o.row_bytes, 1ull << shift);
            return tiles;
        });
}

// The walk of the kernels whose ops have rows, by the functions they call (list_enter_op,
// list_locate, list_next_piece), as a wave makes it: for every wave of a grid, the (op, row,
// piece) of each of its tiles, against the enumeration of ops, rows and pieces in order.
// K: the width the kernel keeps the piece number in (the converting kernel: 32 bits).
// Rows of 1, 2 and 3 tiles, ops of 0, 1 and 3 rows and small grids make waves start
// mid-row and mid-op and cross empty ops.
template <class K>
void row_walk(const std::vector<XferStridedOp> &v, uint64_t total, int *walked) {
    struct Tile {
        uint32_t op;
        uint64_t row, k;
    };
    const uint32_t n = (uint32_t)v.size();
    std::vector<Tile> want;
    for (uint32_t i = 0; i < n; i++)
        for (uint64_t r = 0; r < v[i].rows; r++)
            for (uint64_t k = 0; k < v[i].tiles_per_row; k++) want.push_back(Tile{i, r, k});
    CHECK(want.size() == total, "row_walk: %zu tiles enumerated, the plan has %llu", want.size(), (unsigned long long)total);
    if (want.size() != total) return;
    for (uint32_t grid : {1u, 2u, 5u}) {
        const uint32_t waves = grid * kListWaves;
        std::vector<uint32_t> start(waves);
        list_wave_ops(v.data(), n, total, grid, start.data());
        uint64_t seen = 0;
        for (uint32_t w = 0; w < waves; w++) {
            uint64_t t, t1;
            list_wave_range(w, grid, total, &t, &t1);
            if (t >= t1) continue;
            CHECK(t == seen, "row_walk: wave %u of grid %u starts at tile %llu, not %llu", w, grid, (unsigned long long)t,
                  (unsigned long long)seen);
            uint32_t i = start[w];
            uint64_t next = 0, row = 0;
            K k = 0;
            for (; t < t1; t++, seen++) {
                if (t >= next) {  // as the kernels enter an op
                    next = list_enter_op(v.data(), n, t, &i);
                    list_locate(v[i].tiles_per_row, t - v[i].first_tile, &row, &k);
                }
                const Tile &x = want[(size_t)t];
                CHECK(i == x.op && row == x.row && k == x.k,
                      "row_walk: grid %u wave %u tile %llu of %u ops: the walk says (%u, %llu, %llu), the enumeration (%u, %llu, %llu)",
                      grid, w, (unsigned long long)t, n, i, (unsigned long long)row, (unsigned long long)k, x.op,
                      (unsigned long long)x.row, (unsigned long long)x.k);
                const bool new_row = list_next_piece((K)v[i].tiles_per_row, &row, &k);
                CHECK(new_row == (x.k + 1 == v[i].tiles_per_row), "row_walk: tile %llu: a new row after piece %llu of %llu",
                      (unsigned long long)t, (unsigned long long)x.k, (unsigned long long)v[i].tiles_per_row);
                (*walked)++;
            }
        }
        CHECK(seen == total, "row_walk: grid %u: the waves walked %llu of %llu tiles", grid, (unsigned long long)seen,
              (unsigned long long)total);
    }
}

void test_row_walk() {
    const int before = failures;
    const uint32_t shift = 12, kRows[] = {0, 1, 3};
    int walked = 0;
    for (uint32_t n : kCounts)
        for (int variant = 0; variant < 4; variant++)
            for (uint32_t phase = 0; phase < 9; phase++) {  // every (tiles_per_row, rows) pair in every place of the list
                std::vector<XferStridedOp> v(n, XferStridedOp{});
                for (uint32_t i = 0; i < n; i++) {
                    const uint32_t tpr = 1 + (i + phase) % 3, rows = forced_empty(variant, i, n) ? 0 : kRows[(i + phase) / 3 % 3];
                    v[i].rows = rows;
                    v[i].row_bytes = rows ? ((uint64_t)tpr << shift) - 48 : 0;  // the last piece of a row is partial
                    v[i].lin_stride = v[i].rem_stride = v[i].row_bytes;
                }
                const uint64_t total = xfer_strided_plan(v.data(), n, shift);
                for (uint32_t i = 0; i < n; i++)
                    CHECK(v[i].tiles_per_row == (v[i].rows ? 1 + (i + phase) % 3 : 0), "row_walk: op %u has %llu tiles a row", i,
                          (unsigned long long)v[i].tiles_per_row);
                row_walk<uint64_t>(v, total, &walked);
                row_walk<uint32_t>(v, total, &walked);
            }
    CHECK(walked > 100000, "row_walk: only %d tiles walked", walked);
    std::printf("row_walk: %d tiles walked\n", walked);
    if (failures == before) std::printf("PASS row_walk\n");
}

// list_wave_range on its own: the ranges tile [0, total) in wave order, with fewer tiles
// than waves and with totals that are no multiple of the wave count.
void test_wave_range() {
    const int before = failures;
    const uint64_t totals[] = {0, 1, 3, 4, 5, 7, 8, 9, 511, 512, 513, 8191, 8192, 8193, 1000003};
    for (uint32_t grid : kGrids)
        for (uint64_t total : totals) {
            const uint64_t waves = (uint64_t)grid * kListWaves;
            uint64_t cursor = 0, longest = 0, busy = 0;
            for (uint64_t w = 0; w < waves; w++) {
                uint64_t t0 = ~0ull, t1 = ~0ull;
                list_wave_range(w, grid, total, &t0, &t1);
                CHECK(t1 <= total, "grid %u total %llu wave %llu ends at %llu", grid, (unsigned long long)total,
                      (unsigned long long)w, (unsigned long long)t1);
                if (t0 >= t1) continue;
                CHECK(t0 == cursor, "grid %u total %llu wave %llu starts at %llu, the tiles before it end at %llu", grid,
                      (unsigned long long)total, (unsigned long long)w, (unsigned long long)t0, (unsigned long long)cursor);
                cursor = t1;
                busy++;
                if (t1 - t0 > longest) longest = t1 - t0;
            }
            CHECK(cursor == total, "grid %u total %llu: the ranges end at %llu", grid, (unsigned long long)total,
                  (unsigned long long)cursor);
            // equal shares, rounded up: no wave has more, and with fewer tiles than waves one tile each
            CHECK(longest == (total + waves - 1) / waves, "grid %u total %llu: longest range %llu", grid,
                  (unsigned long long)total, (unsigned long long)longest);
            if (total < waves) CHECK(busy == total, "grid %u total %llu: %llu waves busy", grid, (unsigned long long)total,
                                     (unsigned long long)busy);
        }
    if (failures == before) std::printf("PASS wave_range\n");
}

}  // namespace

int main() {
    static_assert(kListWaves == 4, "the wave table has four entries a workgroup");
    test_batch();
    test_quant();
    test_strided();
    test_acc();
    test_row_walk();
    test_wave_range();
    std::printf("%d failure(s)\n", failures);
    return failures ? 1 : 0;
}
