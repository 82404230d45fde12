/*
 * oncillamem.h — public C ABI of libocm (MI355X-native OncillaMem).
 *
 * Parity: same entry points, enum values and struct layouts as the reference
 * app interface (reference inc/oncillamem.h:24-89):
 *   - enum ocm_kind values OCM_LOCAL_HOST=1 .. OCM_REMOTE_GPU=7
 *   - struct ocm_params       (48 B)  src/dest offsets, *_2 offsets, bytes, op_flag
 *   - struct ocm_alloc_params (24 B)  local_alloc_bytes, rem_alloc_bytes, kind
 *
 * What the kinds mean on MI355X (one backend, not a dispatch layer):
 *   OCM_LOCAL_HOST   page-aligned host memory of the calling process
 *   OCM_LOCAL_GPU    HBM of the calling process' GPU
 *   OCM_REMOTE_GPU   pair: local half in the app GPU's HBM, remote half in the
 *                    HBM of a peer MI355X (placed by rank0) reached over xGMI,
 *                    or in a daemon's pinned host tier when HBM is exhausted
 *   OCM_REMOTE_RDMA  pair whose local half is pinned host memory (CPU-visible,
 *   OCM_REMOTE_RMA   like the reference's malloc'd IB/EXTOLL bounce buffer);
 *                    remote half placed exactly like OCM_REMOTE_GPU
 *   OCM_LOCAL_RDMA / OCM_LOCAL_RMA  accepted as OCM_LOCAL_HOST (the reference
 *                    never implemented them).
 *
 * Functions added for MI355X (async put/get, striping, explicit placement,
 * daemon statistics) are declared after the reference block.
 */
#ifndef ONCILLAMEM_H
#define ONCILLAMEM_H

#include <stdbool.h>
#include <stddef.h>
#include <stdint.h>
#include <sys/types.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct lib_alloc *ocm_alloc_t;

enum ocm_kind {
    OCM_LOCAL_HOST = 1,
    OCM_LOCAL_RMA,
    OCM_REMOTE_RMA,
    OCM_LOCAL_RDMA,
    OCM_REMOTE_RDMA,
    OCM_LOCAL_GPU,
    OCM_REMOTE_GPU,
};

/* General parameters for one-sided / two-sided copies.
 * op_flag: read = 0, write = 1. */
struct ocm_params {
    uint64_t src_offset;
    uint64_t dest_offset;
    uint64_t src_offset_2;
    uint64_t dest_offset_2;
    uint64_t bytes;
    int op_flag;
};
typedef struct ocm_params *ocm_param_t;

struct ocm_alloc_params {
    uint64_t local_alloc_bytes;
    uint64_t rem_alloc_bytes;
    enum ocm_kind kind;
};
typedef struct ocm_alloc_params *ocm_alloc_param_t;

/* ---------------- reference API (inc/oncillamem.h:69-89) ---------------- */
int ocm_init(void);
int ocm_tini(void);
ocm_alloc_t ocm_alloc(ocm_alloc_param_t alloc_param);
int ocm_free(ocm_alloc_t a);
int ocm_localbuf(ocm_alloc_t a, void **buf, size_t *len);
bool ocm_is_remote(ocm_alloc_t a);
enum ocm_kind ocm_alloc_kind(ocm_alloc_t a);
int ocm_remote_sz(ocm_alloc_t a, size_t *len);
/* Implemented (stubs in the reference, src/lib.c:491-499):
 * copy_in  writes min(local,remote) bytes from `src` into the allocation
 *          (remote half for pairs, the buffer itself for local kinds);
 * copy_out reads them back into `dst`. Host or device pointers accepted. */
int ocm_copy_out(void *dst, ocm_alloc_t src);
int ocm_copy_in(ocm_alloc_t dst, void *src);
int ocm_copy(ocm_alloc_t dst, ocm_alloc_t src, ocm_param_t options);
int ocm_copy_onesided(ocm_alloc_t src, ocm_param_t options);

/* ---------------- MI355X extensions ---------------- */

enum ocm_alloc_flags {
    OCM_ALLOC_STRIPE      = 1u << 0, /* stripe the remote half over several peers (xGMI links) */
    OCM_ALLOC_HOST_TIER   = 1u << 1, /* place the remote half in a daemon's pinned host tier */
    OCM_ALLOC_NO_SPILL    = 1u << 2, /* fail instead of spilling to the host tier */
    OCM_ALLOC_ZERO        = 1u << 3, /* zero the remote half before returning */
    OCM_ALLOC_LOOPBACK    = 1u << 4, /* remote half in the origin daemon's own HBM */
};

struct ocm_alloc_ex_params {
    int32_t  remote_rank;   /* -1: rank0 places; >=0: honour this owner (reference field was unused) */
    uint32_t flags;         /* enum ocm_alloc_flags */
    uint32_t stripe_width;  /* 0: all peers; else max number of owners */
    uint32_t reserved;
    uint64_t stripe_unit;   /* bytes per stripe unit, 0: default (OCM_STRIPE_UNIT or 1 MiB) */
};

enum ocm_tier { OCM_TIER_NONE = 0, OCM_TIER_HOST = 1, OCM_TIER_GPU = 2 };

#define OCM_MAX_EXTENTS 8

struct ocm_remote_info {
    uint32_t n_extents;
    uint32_t tier[OCM_MAX_EXTENTS];       /* enum ocm_tier per extent */
    int32_t  owner_rank[OCM_MAX_EXTENTS];
    int32_t  owner_gpu[OCM_MAX_EXTENTS];  /* device ordinal on the node, -1 for host */
    uint64_t extent_bytes[OCM_MAX_EXTENTS];
    uint64_t stripe_unit;
    uint64_t alloc_id;
    uint64_t remote_bytes;
    uint32_t net_mask;   /* bit i: extent i is on another node (network tier) */
    uint32_t reserved;
};

struct ocm_daemon_stats {
    int32_t  rank;
    int32_t  gpu;
    int32_t  num_nodes;
    int32_t  num_apps;
    uint64_t gpu_capacity, gpu_used;
    uint64_t host_capacity, host_used;
    uint64_t n_alloc, n_free, n_reclaimed, n_spilled;
    uint64_t n_slabs;
    uint64_t ctrl_ticks;   /* allgather ticks of the RCCL/socket control transport (0 on TCP) */
    uint64_t n_leases;     /* capacity leases held on peers */
    uint64_t lease_allocs; /* allocations carved from them without a mesh round trip */
    uint32_t xgmi_peers;   /* GPUs on the node this daemon's GPU reaches over xGMI */
    uint16_t min_hops;     /* xGMI hop count over those links (0 when none) */
    uint16_t max_hops;
    uint32_t ctrl_transport; /* daemon<->daemon records: 0 TCP, 1 socket ticks, 2 RCCL ticks,
                                3 TCP after leaving a tick transport, 4 tick transport starting */
    uint32_t reserved;
};

ocm_alloc_t ocm_alloc_ex(ocm_alloc_param_t alloc_param, const struct ocm_alloc_ex_params *ex);
/* Non-blocking variants: enqueue on the allocation's stream; ocm_wait() completes them. */
int ocm_copy_onesided_async(ocm_alloc_t a, ocm_param_t options);
int ocm_wait(ocm_alloc_t a);
/* Batched one-sided copies on one remote pair: n_ops records with the
 * ocm_copy_onesided meaning (op_flag 1 = put local[src_offset] -> remote[dest_offset],
 * 0 = get), puts and gets mixed, run as ONE gfx950 kernel launch (scatter/gather
 * lists). Ops of one batch run concurrently: overlapping destinations have no
 * defined order. flags: OCM_BATCH_ASYNC completes later (ocm_wait). */
#define OCM_BATCH_ASYNC 1
int ocm_copy_onesided_batch(ocm_alloc_t a, const struct ocm_params *ops, int n_ops, int flags);
/* Converting one-sided copies: the local half holds 16-bit elements, the remote half
 * MXFP8 records, 33/64 of the bytes. A put (op_flag 1) reads `elems` elements at
 * local_offset and writes their record at remote_offset; a get (op_flag 0) reads the
 * record and widens it. A record is contiguous: `elems` OCP e4m3fn code bytes, then
 * elems / 32 scale bytes, one per group of 32 consecutive elements: e + 127, where
 * 2^e is the group's shared power-of-two scale (the smallest with
 * max|x| * 2^-e <= 448). Decoding gives float(code) * 2^e rounded to nearest even
 * (docs/API.md has the exact rule). Constraints per op: elems % 32 == 0 and
 * elems < 2^31, local_offset % 16 == 0, remote_offset % 32 == 0, both ranges inside
 * their halves. Ops of one call run concurrently, puts and gets mixed, as ONE gfx950
 * launch when the local half is device memory; flags and ordering as for
 * ocm_copy_onesided_batch (OCM_BATCH_ASYNC, ocm_wait, ocm_stream_wait/signal).
 *
 * The record format is chosen per op: dtype = element type | record format, the element
 * type (enum ocm_quant_dtype) in the low byte and the format (enum ocm_quant_format) in
 * bits 8 to 15; any other bit and any unknown format is rejected. A bare element type is
 * MXFP8, as above. OCM_QUANT_MXFP4 records take 17/64 of the bytes: elems / 2 code bytes
 * of OCP E2M1 codes (element 2i in the low nibble of byte i, element 2i + 1 in the high
 * one), then elems / 32 scale bytes, with 2^e the smallest scale with max|x| * 2^-e <= 6.
 * The constraints per op are the same. Ops of both formats may be mixed in one list. */
enum ocm_quant_dtype { OCM_QUANT_BF16 = 1, OCM_QUANT_FP16 = 2 };
enum ocm_quant_format { OCM_QUANT_MXFP8 = 0, OCM_QUANT_MXFP4 = 0x100 };
struct ocm_quant_params {
    uint64_t local_offset;  /* bytes into the local half */
    uint64_t remote_offset; /* first byte of the record in the remote half */
    uint64_t elems;         /* 16-bit elements */
    int32_t  op_flag;       /* 1 = put (encode), 0 = get (decode) */
    uint32_t dtype;         /* enum ocm_quant_dtype | enum ocm_quant_format */
};
/* Bytes of the MXFP8 record of `elems` elements: elems + elems / 32. */
size_t ocm_quant_bytes(uint64_t elems);
/* Bytes of the record of `elems` elements in `format` (enum ocm_quant_format): MXFP8 as
 * ocm_quant_bytes, MXFP4 elems / 2 + elems / 32; 0 for an unknown format. */
size_t ocm_quant_bytes_fmt(uint64_t elems, uint32_t format);
int ocm_copy_onesided_quant(ocm_alloc_t a, const struct ocm_quant_params *ops, int n_ops, int flags);
/* Strided converting copies (layer-major KV caches): by definition the
 * ocm_copy_onesided_quant list with one op per row. Row r of an op is the converting op
 * (local_offset + r * local_stride, remote_offset + r * remote_stride, row_elems,
 * op_flag, dtype), r = 0 .. rows - 1: every row has a record of its own, its codes and
 * then its scale bytes, so a later ocm_copy_onesided_quant get can read one row of what
 * a strided put wrote. Ops of one call and rows of one op run concurrently, puts and
 * gets mixed, as ONE gfx950 launch when the local half is device memory. Per op: dtype
 * known, row_elems % 32 == 0 and row_elems < 2^31, rows < 2^32, local_offset and
 * local_stride multiples of 16, remote_offset and remote_stride multiples of 32, with
 * rows > 1 local_stride >= 2 * row_elems and remote_stride >= the row's record bytes
 * (ocm_quant_bytes_fmt: row_elems + row_elems / 32, or row_elems / 2 + row_elems / 32
 * for OCM_QUANT_MXFP4), and the last row's end inside its half on both sides; an op with rows == 0 or
 * row_elems == 0 does nothing. flags and ordering as for ocm_copy_onesided_batch
 * (OCM_BATCH_ASYNC, ocm_wait, ocm_stream_wait/signal). */
struct ocm_quant_strided_params {
    uint64_t local_offset;   /* first element of row 0 in the local half (bytes) */
    uint64_t remote_offset;  /* first byte of row 0's record in the remote half */
    uint64_t row_elems;      /* 16-bit elements per row */
    uint64_t rows;
    uint64_t local_stride;   /* bytes from one row's start to the next, local side */
    uint64_t remote_stride;  /* bytes from one row's record to the next, remote side */
    int32_t  op_flag;        /* 1 = put (encode), 0 = get (decode) */
    uint32_t dtype;          /* enum ocm_quant_dtype | enum ocm_quant_format */
};
int ocm_copy_onesided_quant_strided(ocm_alloc_t a, const struct ocm_quant_strided_params *ops, int n_ops, int flags);
/* Strided one-sided copies (2-D put / get): row r of an op moves row_bytes bytes between
 * local[local_offset + r * local_stride] and remote[remote_offset + r * remote_stride],
 * r = 0 .. rows - 1, in the direction of ocm_copy_onesided (op_flag 1 = put). Ops of one
 * call and rows of one op run concurrently, puts and gets mixed, as ONE gfx950 launch
 * when the local half is device memory: overlapping destinations have no defined order.
 * No alignment is asked of offsets, strides or row_bytes. Per op: reserved == 0,
 * rows < 2^32, with rows > 1 both strides >= row_bytes, and the last row's end inside
 * its half on both sides; an op with rows == 0 or row_bytes == 0 does nothing. flags and
 * ordering as for ocm_copy_onesided_batch (OCM_BATCH_ASYNC, ocm_wait,
 * ocm_stream_wait/signal). Transfer plans (ocm_plan_add) take ocm_params only. */
struct ocm_strided_params {
    uint64_t local_offset;   /* first byte of row 0 in the local half  */
    uint64_t remote_offset;  /* first byte of row 0 in the remote half */
    uint64_t row_bytes;      /* bytes per row (any value, 0 = empty op) */
    uint64_t rows;           /* number of rows, < 2^32 */
    uint64_t local_stride;   /* bytes from one row's start to the next, local half  */
    uint64_t remote_stride;  /* same, remote half */
    int32_t  op_flag;        /* 1 = put, 0 = get */
    uint32_t reserved;       /* must be 0 */
};
int ocm_copy_onesided_strided(ocm_alloc_t a, const struct ocm_strided_params *ops, int n_ops, int flags);
/* Indexed one-sided copies (gather / scatter by row number): each side is a table of
 * rows (offset, stride, number of rows), and which row of it row j of the op is comes
 * from an index array. For j = 0 .. rows - 1, with lr = lidx[j] when the local side has
 * an index and j when it has none, and rr likewise for the remote side, the op moves
 * row_bytes bytes between local[local_offset + lr * local_stride] and
 * remote[remote_offset + rr * remote_stride], in the direction of ocm_copy_onesided
 * (op_flag 1 = put). Both index arrays, `rows` entries of index_type each, live in the
 * LOCAL half (device memory on the kernel path) at local_index_offset and
 * remote_index_offset; OCM_INDEX_NONE: that side has no index. They are read when the
 * transfer runs, so they may be written on the GPU just before it (order the op after
 * that work with ocm_stream_wait, as for any data of the local half). Ops of one call and
 * rows of one op run concurrently, puts and gets mixed, as ONE gfx950 launch when the
 * local half is device memory. No alignment is asked of offsets, strides or row_bytes.
 *
 * Out-of-range indices: row j is skipped, moving nothing on either side, when either of
 * its indices is outside [0, table rows) of its side; indices are compared as unsigned, so
 * negative ones are out of range. Skipped rows are counted once each. A blocking call
 * that skipped k > 0 rows still moves every other row, then returns -1 and
 * ocm_last_error() names k; after an OCM_BATCH_ASYNC call the next ocm_wait(a) returns -1
 * once in the same way. Later ops on the allocation are unaffected.
 *
 * Duplicate destination rows (duplicates in the index of the side being written, or rows
 * written by two ops of a call) have no defined result: which source wins is undefined
 * and pieces of different sources may mix. Duplicates on the side being read are fine
 * (an embedding lookup).
 *
 * Per op (checked at the call): index_type known and at least one index; rows,
 * local_rows and remote_rows < 2^32; per side with more than one table row, stride >=
 * row_bytes; per side, the table's last row ends inside its half; a side without an
 * index has at least `rows` table rows; each index array is aligned to its element size
 * and lies inside the local half; for a get, no index array overlaps the op's local
 * table. An op with rows == 0 or row_bytes == 0 does nothing, whatever else it says.
 * flags and ordering as for ocm_copy_onesided_batch (OCM_BATCH_ASYNC, ocm_wait,
 * ocm_stream_wait/signal). Out of scope: transfer plans (ocm_plan_add takes ocm_params
 * only), the copy service, put-side accumulate variants, index-times-stride (layer-major)
 * ops and scatter-add. The converting (MX) variant is ocm_copy_onesided_quant_indexed, the
 * gather that sums the rows of a bag ocm_copy_onesided_bag, both below. */
#define OCM_INDEX_NONE (~0ull)
enum ocm_index_type { OCM_INDEX_I32 = 1, OCM_INDEX_I64 = 2 };
struct ocm_indexed_params {        /* 88 bytes */
    uint64_t local_offset;         /* first byte of local table row 0 */
    uint64_t remote_offset;        /* first byte of remote table row 0 */
    uint64_t row_bytes;            /* any value; 0 = empty op */
    uint64_t rows;                 /* rows moved = entries of each index array, < 2^32; 0 = empty op */
    uint64_t local_stride;         /* bytes between local table rows */
    uint64_t remote_stride;        /* bytes between remote table rows */
    uint64_t local_index_offset;   /* byte offset IN THE LOCAL HALF of `rows` indices, or OCM_INDEX_NONE */
    uint64_t remote_index_offset;  /* same, for the remote side */
    uint64_t local_rows;           /* rows the local table has  (< 2^32) */
    uint64_t remote_rows;          /* rows the remote table has (< 2^32) */
    int32_t  op_flag;              /* 1 = put, 0 = get */
    uint32_t index_type;           /* enum ocm_index_type, both arrays alike */
};
int ocm_copy_onesided_indexed(ocm_alloc_t a, const struct ocm_indexed_params *ops, int n_ops, int flags);
/* Indexed converting copies (embedding tables kept as MX records): the local side is a
 * table of rows of row_elems 16-bit elements, the remote side a table of records, one
 * MXFP8 or MXFP4 record per row (its codes, then its scale bytes, as for
 * ocm_copy_onesided_quant), and which row of either table row j of the op is comes from
 * an index array, as for ocm_copy_onesided_indexed. For j = 0 .. rows - 1, with
 * lr = lidx[j] when the local side has an index and j when it has none, and rr likewise
 * for the remote side: when both are in range, row j is exactly the converting op
 * (local_offset + lr * local_stride, remote_offset + rr * remote_stride, row_elems,
 * op_flag, dtype). By definition the call is the ocm_copy_onesided_quant list with one op
 * per in-range row, so a plain or strided converting get can read what an indexed put
 * wrote. Both index arrays, `rows` entries of index_type each, live in the LOCAL half at
 * local_index_offset and remote_index_offset (OCM_INDEX_NONE: that side has no index) and
 * are read when the transfer runs. Ops of one call and rows of one op run concurrently,
 * puts and gets and both record formats mixed, as ONE gfx950 launch when the local half
 * is device memory.
 *
 * Out-of-range indices follow the rule of ocm_copy_onesided_indexed unchanged: indices
 * are compared as unsigned; a row with either index outside [0, table rows) of its side
 * is skipped whole on both sides and counted once; a blocking call that skipped k > 0
 * rows still moves every other row, then returns -1 and ocm_last_error() says
 * "indexed ops skipped k row(s)"; after an OCM_BATCH_ASYNC call the next ocm_wait(a)
 * returns -1 once in the same way. The count goes to the allocation's one pair of skip
 * words, so ocm_wait has one path for both calls and the n_indexed_skipped counter counts
 * rows skipped by either.
 *
 * Duplicate destination rows have no defined result, as for the indexed op; duplicates on
 * the side being read are fine (an embedding lookup).
 *
 * Per op (checked at the call): dtype known; reserved == 0; row_elems % 32 == 0 and
 * row_elems < 2^31; index_type known and at least one index; rows, local_rows and
 * remote_rows < 2^32; local_offset and local_stride multiples of 16, remote_offset and
 * remote_stride multiples of 32; per side with more than one table row, stride >= the
 * row's bytes (2 * row_elems local, ocm_quant_bytes_fmt(row_elems, format) remote); per
 * side, the table's last row ends inside its half; a side without an index has at least
 * `rows` table rows; each index array is aligned to its element size and lies inside the
 * local half; for a get, no index array overlaps the op's local table. An op with
 * rows == 0 or row_elems == 0 does nothing. flags and ordering as for
 * ocm_copy_onesided_batch (OCM_BATCH_ASYNC, ocm_wait, ocm_stream_wait/signal). Out of
 * scope: transfer plans (ocm_plan_add takes ocm_params only), the copy service,
 * index-times-stride (layer-major) ops and scatter-add. */
struct ocm_quant_indexed_params {   /* 96 bytes */
    uint64_t local_offset;          /* first element of local table row 0 (bytes), multiple of 16 */
    uint64_t remote_offset;         /* first byte of remote table row 0's record, multiple of 32 */
    uint64_t row_elems;             /* 16-bit elements per row: multiple of 32, < 2^31; 0 = empty op */
    uint64_t rows;                  /* rows moved = entries of each index array, < 2^32; 0 = empty op */
    uint64_t local_stride;          /* multiple of 16 */
    uint64_t remote_stride;         /* multiple of 32 */
    uint64_t local_index_offset;    /* in the LOCAL half, or OCM_INDEX_NONE */
    uint64_t remote_index_offset;
    uint64_t local_rows;            /* rows each table has, < 2^32 */
    uint64_t remote_rows;
    int32_t  op_flag;               /* 1 = put (encode), 0 = get (decode) */
    uint32_t index_type;            /* enum ocm_index_type */
    uint32_t dtype;                 /* enum ocm_quant_dtype | enum ocm_quant_format */
    uint32_t reserved;              /* must be 0 */
};
int ocm_copy_onesided_quant_indexed(ocm_alloc_t a, const struct ocm_quant_indexed_params *ops, int n_ops, int flags);
/* Pooled embedding lookup (nn.EmbeddingBag's forward; a get only): the remote half holds a
 * table of remote_rows rows of row_elems elements of `dtype` (enum ocm_acc_dtype, below),
 * the local half an array of `ids` row numbers cut into `bags` bags by an offsets array of
 * bags + 1 entries (include-last-offset form), optionally one fp32 weight per id, and an
 * output table of `bags` rows of the same elements, written in bag order. All three arrays
 * live in the LOCAL half and are read when the transfer runs, as the index arrays of
 * ocm_copy_onesided_indexed are. The result is defined bit for bit (ocm/bag.h). For bag b:
 *   lo = min(off[b], ids), hi = min(off[b + 1], ids), compared as unsigned after int32
 *   values are sign-extended; hi < lo is an empty bag;
 *   acc[e] = +0, then for j = lo .. hi - 1 in that order
 *       acc[e] = fl32(acc[e] + fl32(w[j] * widen(table[id[j]][e])))
 *   (two roundings, never an fma; without weights fl32(acc[e] + widen(x))) when id[j] is
 *   inside [0, remote_rows) compared as unsigned; otherwise entry j adds nothing;
 *   OCM_BAG_MEAN: acc[e] = fl32(acc[e] / (float)(hi - lo)) when hi > lo;
 *   out[b][e] = acc[e] narrowed to dtype, round to nearest even. An empty bag writes zeros.
 * Duplicate ids in a bag add twice. The remote half is only read. Ops of one call and bags
 * of one op run concurrently, as ONE gfx950 launch when the local half is device memory.
 *
 * Out-of-range ids are counted once per entry and reported exactly as the indexed ops'
 * skipped rows are: the call still writes every bag, then returns -1 and ocm_last_error()
 * says "indexed ops skipped k row(s)"; after an OCM_BATCH_ASYNC call the next ocm_wait(a)
 * returns -1 once in the same way. The count goes to the allocation's one pair of skip
 * words and to the n_indexed_skipped counter. A mean divides by hi - lo, skipped entries
 * included.
 *
 * Per op (checked at the call): index_type, dtype and mode known, reserved == 0; no weights
 * with OCM_BAG_MEAN; row_elems * size(dtype) a positive multiple of 16 below 2^32; bags, ids
 * and remote_rows < 2^32; offsets and strides of both tables multiples of 16; per table with
 * more than one row, stride >= the row's bytes, and the table's last row ends inside its
 * half; each array is aligned to its element size, lies inside the local half and does not
 * overlap the output table. An op with bags == 0 does nothing; one with ids == 0 writes
 * zeros to every bag. flags and ordering as for ocm_copy_onesided_batch (OCM_BATCH_ASYNC,
 * ocm_wait, ocm_stream_wait/signal). Out of scope: a max mode, MX-compressed tables,
 * transfer plans, and scatter-add into remote memory. */
enum ocm_bag_mode { OCM_BAG_SUM = 0, OCM_BAG_MEAN = 1 };
struct ocm_bag_params {            /* 104 bytes */
    uint64_t local_offset;         /* first byte of bag 0's output row, multiple of 16 */
    uint64_t remote_offset;        /* first byte of remote table row 0, multiple of 16 */
    uint64_t row_elems;            /* elements per row of both tables */
    uint64_t bags;                 /* output rows, < 2^32; 0 = empty op */
    uint64_t ids;                  /* entries of the id array (and of the weights), < 2^32 */
    uint64_t local_stride;         /* bytes between output rows, multiple of 16 */
    uint64_t remote_stride;        /* bytes between table rows, multiple of 16 */
    uint64_t remote_rows;          /* rows the remote table has, < 2^32 */
    uint64_t index_offset;         /* byte offset IN THE LOCAL HALF of `ids` entries of index_type */
    uint64_t offsets_offset;       /* same, of bags + 1 entries of index_type */
    uint64_t weights_offset;       /* same, of `ids` fp32 weights, or OCM_INDEX_NONE */
    uint32_t index_type;           /* enum ocm_index_type, ids and offsets alike */
    uint32_t dtype;                /* enum ocm_acc_dtype, both tables alike */
    uint32_t mode;                 /* enum ocm_bag_mode */
    uint32_t reserved;             /* must be 0 */
};
int ocm_copy_onesided_bag(ocm_alloc_t a, const struct ocm_bag_params *ops, int n_ops, int flags);
/* One-sided accumulate (the counterpart of MPI_Accumulate): the remote half holds fp32
 * accumulators, the local half elements of `dtype`, and for every element i of every op
 *     remote_f32[i] = remote_f32[i] + scale * widen(local[i]).
 * The result is defined bit for bit (ocm/acc.h): two IEEE fp32 operations, each rounded
 * to nearest even, p = scale * x then r = acc + p, never fused into one; subnormals are
 * kept; bf16 and fp16 elements widen exactly; a NaN result is some NaN. The local half
 * is only read. Ops of one call run concurrently, as ONE gfx950 launch when the local
 * half is device memory; no atomics are used, so overlapping remote ranges within one
 * call have no defined result. Two calls on one allocation are ordered, as batches are.
 * Per op: dtype known, scale finite, both offsets multiples of 16, elems % 4 == 0 and
 * elems < 2^31 (0 = empty op), elems * size(dtype) bytes inside the local half and
 * 4 * elems inside the remote half. flags and ordering as for ocm_copy_onesided_batch
 * (OCM_BATCH_ASYNC, ocm_wait, ocm_stream_wait/signal). Out of scope: transfer plans
 * (ocm_plan_add takes ocm_params only), the copy service, a get-side accumulate
 * (local += remote) and integer element types. */
enum ocm_acc_dtype { OCM_ACC_F32 = 1, OCM_ACC_BF16 = 2, OCM_ACC_FP16 = 3 };
struct ocm_acc_params {      /* 32 bytes */
    uint64_t local_offset;   /* bytes into the local half, multiple of 16 */
    uint64_t remote_offset;  /* bytes into the remote half (fp32 accumulators), multiple of 16 */
    uint64_t elems;          /* multiple of 4, below 2^31; 0 = empty op */
    uint32_t dtype;          /* enum ocm_acc_dtype: element type of the LOCAL half */
    float    scale;          /* finite */
};
int ocm_copy_onesided_accumulate(ocm_alloc_t a, const struct ocm_acc_params *ops, int n_ops, int flags);
/* Stream interop (hipStream_t passed as void*, NULL = legacy default stream):
 * ocm_stream_wait:   a's next one-sided op starts after the work already queued on `stream`
 *                    (e.g. torch kernels that wrote the local half).
 * ocm_stream_signal: work queued on `stream` afterwards starts after a's queued async ops. */
int ocm_stream_wait(ocm_alloc_t a, void *stream);
int ocm_stream_signal(ocm_alloc_t a, void *stream);

/* Transfer plans: a fixed sequence of batch stages (each stage = one
 * ocm_copy_onesided_batch list on one allocation, run after the previous
 * stage), validated, planned and uploaded once, then captured into a HIP
 * graph. Every ocm_plan_launch replays the whole schedule as one graph launch
 * (data is read at replay time; the op lists are fixed). stream NULL: the
 * library stream, blocking; otherwise queued on `stream` (hipStream_t).
 * Allocations used by a plan cannot be freed before ocm_plan_destroy. */
typedef struct ocm_plan *ocm_plan_t;
ocm_plan_t ocm_plan_create(void);
int ocm_plan_add(ocm_plan_t p, ocm_alloc_t a, const struct ocm_params *ops, int n_ops);
int ocm_plan_launch(ocm_plan_t p, void *stream);
int ocm_plan_destroy(ocm_plan_t p);
int ocm_remote_info(ocm_alloc_t a, struct ocm_remote_info *info);
/* Device pointer of the remote half when it is a single extent (NULL if striped). */
void *ocm_remotebuf(ocm_alloc_t a);
int ocm_stats(int rank, struct ocm_daemon_stats *out); /* rank -1: local daemon */
int ocm_rank(void);        /* rank of the daemon this process is attached to */
int ocm_num_nodes(void);   /* daemons in the mesh */
int ocm_device(void);      /* HIP device the library copies on, -1 when CPU-only */
const char *ocm_last_error(void);

/* PyTorch pluggable-allocator hooks (torch.cuda.memory.CUDAPluggableAllocator;
 * Python wrapper: oncilla_amd.torch_pool.RemoteMemPool). A block is the remote
 * half of a single-extent pair with no local half, placed per
 * ocm_x_torch_pool_config (remote_rank -1: rank0 places; flags: enum
 * ocm_alloc_flags) and addressed in place by the caller's GPU. The process must
 * have called ocm_init; `device` must be the library's device. */
void *ocm_torch_alloc(ssize_t size, int device, void *stream);
void ocm_torch_free(void *ptr, ssize_t size, int device, void *stream);
void ocm_x_torch_pool_config(int remote_rank, uint32_t flags);

#ifdef __cplusplus
}
#endif
#endif /* ONCILLAMEM_H */
