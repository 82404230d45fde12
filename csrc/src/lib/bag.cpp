// libocm pooled embedding lookup (ocm_copy_onesided_bag): every bag's table rows read out
// of the remote half and summed, the sum written to the local half (ocm/bag.h has the
// rule, bit for bit). A pair with a device-side path takes one kernel launch per list,
// uploaded and ordered like a batch (run_list); the kernel reads the offsets, the ids and
// the weights, steps over ids outside the table and counts them into the allocation's
// skip words, the ones the indexed ops count into (indexed.cpp), so ocm_wait and the
// n_indexed_skipped counter have one path for all of them. Every other pair (a CPU app, a
// host local half, the network tier) brings the three arrays to host memory and goes op by
// op, bag by bag, id by id, in order: each in-range row through xfer() into a staging row,
// then the same rule in plain C++.
#include "lists.h"
#include "ocm/bag.h"

using namespace ocm;
using namespace ocmlib;

static const ListNames kBag = {"ocm_copy_onesided_bag", "pooled lookups", "ocm_bag", "bag", false};

// What a call names: bags and ids of its non-empty ops, and the nominal bytes read.
struct BagNamed {
    uint64_t bags = 0, ids = 0, bytes = 0;
    bool work = false;  // some op has a bag to write
};

// Every op against the pair (bag_check_op). Adds to *n.
static int check_bag_ops(lib_alloc *a, const struct ocm_bag_params *ops, int n_ops, BagNamed *n) {
    char why[256];
    for (int i = 0; i < n_ops; i++) {
        uint64_t moved = 0;
        if (bag_check_op(ops[i], a->local_bytes, a->remote_bytes, &moved, why, sizeof(why)) != 0)
            OCM_FAIL(-1, "bag op %d: %s", i, why);
        if (ops[i].bags == 0) continue;
        n->work = true;
        n->bags += ops[i].bags;
        n->ids += ops[i].ids;
        n->bytes += moved;
    }
    return 0;
}

// `n` bytes at byte `off` of the local half, in host memory: where they lie, or copied into `keep`.
static const char *local_on_host(lib_alloc *a, uint64_t off, uint64_t n, std::vector<char> &keep) {
    const char *src = static_cast<const char *>(a->local) + off;
    if (a->loc != LOC_DEVICE) return src;
    keep.resize((size_t)n);
    if (n != 0 && copy_local(keep.data(), LOC_HOST, src, LOC_DEVICE, (size_t)n) != 0) return nullptr;
    return keep.data();
}

// The host path. *skipped: entries whose id was outside the table.
static int bag_host(lib_alloc *a, const struct ocm_bag_params *ops, int n_ops, uint64_t *skipped) {
    // the arrays are read now: after the allocation's queued work and what ocm_stream_wait named
    if (wait_alloc(a) != 0 || honor_dep(a, nullptr, true) != 0) return -1;
    std::vector<char> idx_keep, off_keep, w_keep, row, out;
    std::vector<float> acc;
    for (int i = 0; i < n_ops; i++) {
        const ocm_bag_params &p = ops[i];
        if (p.bags == 0) continue;
        const uint64_t isz = indexed_index_bytes(p.index_type), row_bytes = p.row_elems * acc_elem_size(p.dtype);
        const bool weighted = p.ids != 0 && p.weights_offset != OCM_INDEX_NONE;
        const char *offs = local_on_host(a, p.offsets_offset, (p.bags + 1) * isz, off_keep);
        const char *idx = p.ids ? local_on_host(a, p.index_offset, p.ids * isz, idx_keep) : nullptr;
        const char *wts = weighted ? local_on_host(a, p.weights_offset, p.ids * 4, w_keep) : nullptr;
        if (!offs || (p.ids && !idx) || (weighted && !wts)) return -1;
        acc.resize((size_t)p.row_elems);
        row.resize((size_t)row_bytes);
        out.resize((size_t)row_bytes);
        for (uint64_t b = 0; b < p.bags; b++) {
            uint32_t lo, hi;
            bag_bounds(indexed_load_host(offs, 0, p.index_type, b), indexed_load_host(offs, 0, p.index_type, b + 1),
                       (uint32_t)p.ids, &lo, &hi);
            std::fill(acc.begin(), acc.end(), 0.0f);
            for (uint32_t j = lo; j < hi; j++) {
                const uint64_t id = indexed_load_host(idx, 0, p.index_type, j);
                if (!indexed_in_range(id, p.remote_rows)) {
                    (*skipped)++;
                    continue;
                }
                if (xfer(a, false, row.data(), LOC_HOST, p.remote_offset + id * p.remote_stride, row_bytes, false) != 0) return -1;
                float w = 1.0f;
                if (weighted) std::memcpy(&w, wts + 4ull * j, 4);
                bag_add_row_host(acc.data(), row.data(), p.row_elems, p.dtype, w);
            }
            bag_finish_host(acc.data(), out.data(), p.row_elems, p.dtype, p.mode, hi - lo);
            char *dst = static_cast<char *>(a->local) + p.local_offset + b * p.local_stride;
            if (copy_local(dst, a->loc, out.data(), LOC_HOST, (size_t)row_bytes) != 0) return -1;
        }
    }
    return 0;
}

// *ran: the lookup was made (entries may have been skipped, which fails the call all the same).
static int bag_impl(ocm_alloc_t a, const struct ocm_bag_params *ops, int n_ops, int flags, BagNamed *named, bool *ran) {
    std::unique_lock<std::recursive_mutex> lk;
    const int path = list_enter(kBag, lk, a, ops, n_ops, [&] { return check_bag_ops(a, ops, n_ops, named) != 0 ? -1 : named->work; });
    if (path <= PATH_NONE) {
        *ran = path == PATH_NONE;
        return path;
    }
    State &s = S();
    const bool async = (flags & OCM_BATCH_ASYNC) != 0;
    if (path == PATH_HOST) {
        uint64_t skipped = 0;
        if (bag_host(a, ops, n_ops, &skipped) != 0) return -1;
        *ran = true;
        if (skipped == 0) return 0;
        if (async) {  // the next ocm_wait reports them
            a->skip_host_path += skipped;
            return 0;
        }
        return indexed_fail_skips(skipped);
    }
    DeviceGuard guard(s.device);
    std::vector<XferBagOp> v((size_t)n_ops);
    for (int i = 0; i < n_ops; i++) v[i] = bag_op(ops[i]);
    XferBagArgs args;
    if (list_fill_args(a, v, kBagTileShift, xfer_bag_plan, &args) != 0) return -1;
    // a blocking call reports its own entries only: what queued async lists skipped stays for ocm_wait
    if (!async && wait_alloc(a) != 0) return -1;
    if (skip_words(a, async ? lane_stream(a) : s.stream) != 0) return -1;
    const uint64_t base = __atomic_load_n(a->skip_host, __ATOMIC_ACQUIRE);
    args.skipped = a->skip_dev;
    args.skipped_host = a->skip_host;
    if (run_list(a, args, v, xfer_bag_launch, async) != 0) return -1;
    *ran = true;
    if (async) return 0;
    const uint64_t k = __atomic_load_n(a->skip_host, __ATOMIC_ACQUIRE) - base;
    a->skip_seen += k;
    return indexed_fail_skips(k);
}

extern "C" {

int ocm_copy_onesided_bag(ocm_alloc_t a, const struct ocm_bag_params *ops, int n_ops, int flags) {
    BagNamed named;
    bool ran = false;
    return abi_call(kBag.range, false, kBag.op, named.bytes, [&] { return bag_impl(a, ops, n_ops, flags, &named, &ran); },
                    [&](OpCounters &c, uint64_t, bool) {
                        if (!ran) return;
                        c.n_bag++;
                        c.n_bag_ops += (uint64_t)n_ops;
                        c.n_bag_bags += named.bags;
                        c.n_bag_ids += named.ids;
                        c.bytes_bag += named.bytes;
                    });
}

}  // extern "C"
