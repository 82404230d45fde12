// What the kinds of descriptor list share on the host (batches in batch.cpp, converting
// ops in quant.cpp, strided ops in strided.cpp, strided converting ops in
// quant_strided.cpp, indexed ops in indexed.cpp, indexed converting ops in
// quant_indexed.cpp, accumulates in acc.cpp): how a
// call is entered and accounted, how launch arguments are filled from the pair and the
// plan (ocm/list.h), how a large list's descriptors and wave table are packed for the
// device, and the upload, launch and completion of one list (run_list). A kind brings
// its argument check, its descriptors, its plan and its launch function.
#pragma once
#include <functional>

#include "internal.h"

namespace ocmlib {
#pragma GCC visibility push(hidden)

// What a kind of list call says about itself.
struct ListNames {
    const char *fn;     // the ABI function, in argument errors
    const char *what;   // "<what> need a remote pair"
    const char *range;  // the trace range
    const char *op;     // the name trace_op records
    bool kernel_only;   // no host path for a device local half: fail when no kernel reaches every extent
};

// One kernel can serve this pair: device local half, every extent device-accessible (batch.cpp).
bool batch_device_path(const lib_alloc *a);

// Where an entered call goes; PATH_NONE: nothing to do, the call has succeeded.
enum ListPath : int { PATH_NONE = 0, PATH_HOST = 1, PATH_DEVICE = 2 };

// The start of every list call: takes the library lock into `lk` (held until the caller
// returns), checks the arguments, runs the kind's own check of the ops (-1: failed,
// 0: nothing to move, 1: work) and picks the path. -1: failed (the error is set).
template <class Check>
int list_enter(const ListNames &k, std::unique_lock<std::recursive_mutex> &lk, lib_alloc *a, const void *ops, int n_ops,
               Check check) {
    State &s = S();
    lk = std::unique_lock<std::recursive_mutex>(s.mu);
    if (!a || (!ops && n_ops)) OCM_FAIL(-1, "%s: NULL argument", k.fn);
    if (!s.allocs.count(a)) OCM_FAIL(-1, "%s: unknown allocation", k.fn);
    if (!a->remote) OCM_FAIL(-1, "%s need a remote pair (kind %d)", k.what, (int)a->kind);
    if (n_ops < 0) OCM_FAIL(-1, "%s: n_ops < 0", k.fn);
    const int work = check();
    if (work < 0) return -1;
    if (n_ops == 0 || work == 0) return PATH_NONE;
    if (batch_device_path(a)) return PATH_DEVICE;
    if (k.kernel_only && a->loc == LOC_DEVICE)
        OCM_FAIL(-1, "%s: a device local half needs every extent reachable by a kernel "
                     "(no network tier, stripe unit >= 16 bytes)", k.fn);
    return PATH_HOST;
}

// The ABI side of every list call (abi_call, unwatched): the kind's counters move after a
// success (count(counters, ns)), and the op log records `traced` bytes.
template <class Impl, class Count>
int list_call(const ListNames &k, const uint64_t &traced, Impl impl, Count count) {
    return abi_call(k.range, false, k.op, traced, impl, [&](OpCounters &c, uint64_t ns, bool ok) {
        if (ok) count(c, ns);
    });
}

// The plan's side of launch arguments (the head every kind shares, ocm/list.h) whose
// pair's side is set: the descriptors `v` planned by plan(ops, n, tile_shift) (first_tile
// filled in), the grid, and the descriptors themselves when they travel in the kernel
// arguments.
template <class Op, int INLINE, class Plan>
void list_plan_args(ListArgs<Op, INLINE> *args, std::vector<Op> &v, Plan plan) {
    args->n_ops = (uint32_t)v.size();
    args->total_tiles = plan(v.data(), (uint32_t)v.size(), args->tile_shift);
    args->grid = args->total_tiles ? xfer_batch_grid(args->total_tiles, args->host_tier != 0) : 0;
    if (v.size() <= (size_t)INLINE) std::memcpy(args->inline_ops, v.data(), v.size() * sizeof(Op));
}

// Launch arguments of a list on `a`: a kind's `Args` (the head, or a struct derived from
// it) zeroed, the kind's own fields included; then the head's pair side (the linear base,
// the extents and how they stripe) and its plan side (list_plan_args). elem_shift: the tile
// shift of a kind that cuts tiles in elements; 0: byte tiles, xfer_batch_tile_shift of the
// pair. -1: the pair's stripe unit is unusable (the error is set).
template <class Args, class Plan>
int list_fill_args(lib_alloc *a, std::vector<typename Args::Op> &v, uint32_t elem_shift, Plan plan, Args *args) {
    std::memset(args, 0, sizeof(*args));
    ListArgs<typename Args::Op, Args::kInline> *head = args;
    head->lin = static_cast<char *>(a->local);
    if (pair_side(a, 0, head) < 0)
        OCM_FAIL(-1, "stripe unit %llu is not a power of two", (unsigned long long)a->stripe_unit);
    head->host_tier = (!a->any_gpu && !a->any_net) ? 1u : 0u;
    head->tile_shift = elem_shift ? elem_shift : xfer_batch_tile_shift(head->n_ext, head->unit_shift);
    list_plan_args(head, v, plan);
    return 0;
}

// A large list's upload: the descriptors, then the wave table.
template <class Op>
size_t list_upload_bytes(size_t n_ops, uint32_t grid) {
    return n_ops * sizeof(Op) + (size_t)grid * kListWaves * sizeof(uint32_t);
}
// Packs it into `up` (list_upload_bytes long) and points `args` at where it will lie in
// device memory, `dev`.
template <class Op, int INLINE>
void list_pack(ListArgs<Op, INLINE> *args, const std::vector<Op> &v, void *up, void *dev) {
    const size_t dbytes = v.size() * sizeof(Op);
    std::memcpy(up, v.data(), dbytes);
    list_wave_ops(v.data(), (uint32_t)v.size(), args->total_tiles, args->grid,
                  reinterpret_cast<uint32_t *>(static_cast<char *>(up) + dbytes));
    args->ops = static_cast<const Op *>(dev);
    args->wave_op = reinterpret_cast<const uint32_t *>(static_cast<char *>(dev) + dbytes);
}

// The pair's staging for large lists, at least `need` bytes of pinned host and device
// memory (allocated on `st`), free again for the next upload (batch.cpp).
int list_staging(lib_alloc *a, size_t need, hipStream_t st);

// Upload (large lists), launch and complete one planned list on `a`: the staging buffer,
// its batch_up event and the completion every kind shares. n_launches: counted after a
// launch (batches count n_batch_launches).
template <class Args, class Op = typename Args::Op>
int run_list(lib_alloc *a, Args &args, const std::vector<Op> &v,
             hipError_t (*launch)(const Args &, const XferTuning &, hipStream_t), bool async, uint64_t *n_launches = nullptr) {
    State &s = S();
    DeviceGuard guard(s.device);
    if (!async && wait_alloc(a) != 0) return -1;
    hipStream_t st = async ? lane_stream(a) : s.stream;
    if (honor_dep(a, st, false) != 0) return -1;
    hipError_t err = hipSuccess;
    if (v.size() > (size_t)Args::kInline) {
        const size_t need = list_upload_bytes<Op>(v.size(), args.grid);
        if (list_staging(a, need, st) != 0) return -1;
        list_pack(&args, v, a->batch_host, a->batch_dev);
        // Pinned source: a real async DMA; batch_up tells the next batch when the staging is free.
        err = hipMemcpyAsync(a->batch_dev, a->batch_host, need, hipMemcpyHostToDevice, st);
        if (err == hipSuccess) err = hipEventRecord(a->batch_up, st);
        if (err != hipSuccess) OCM_FAIL(-1, "batch descriptor upload: %s", hipGetErrorString(err));
    }
    before_launch();
    err = launch(args, s.tuning, st);
    if (err != hipSuccess) OCM_FAIL(-1, "batch launch failed: %s", hipGetErrorString(err));
    if (n_launches) (*n_launches)++;
    return async ? async_done(a, st) : sync_stream();
}

// The host path of converting ops (quant.cpp): a CPU app, a host local half, the network
// tier. Encodes or decodes the plain ops `next` yields (false: no more), in order, on this
// thread and moves each record with xfer(). Converting lists yield their ops, strided
// converting lists (quant_strided.cpp) one op per row, indexed converting lists
// (quant_indexed.cpp) one op per row whose indices are in range.
int quant_host(lib_alloc *a, const std::function<bool(ocm_quant_params *)> &next);

// Copy absolute device ranges (op.lin_off = address) into dst's remote half, one launch.
int batch_put_abs(lib_alloc *dst, std::vector<XferBatchOp> &v);

#pragma GCC visibility pop
}  // namespace ocmlib
