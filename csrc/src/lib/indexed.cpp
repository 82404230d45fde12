// libocm indexed one-sided ops (ocm_copy_onesided_indexed): rows picked on either side by
// index arrays in the local half (ocm/indexed.h). A pair with a device-side path takes
// one kernel launch per list, uploaded and ordered like a batch (run_list); the kernel
// reads the indices, skips rows whose index is outside its table and counts them. Every
// other pair (a CPU app, a host local half, the network tier) brings the indices to host
// memory and goes op by op, row by row, in order, through xfer(), with the same rule.
//
// How skipped rows come back: the allocation has a device word that kernels only count
// up, and after each launch, on the same stream, the word is copied to a pinned host
// word. What the host has already reported is kept in skip_seen, so nothing is reset
// between launches and two async lists in a row add up. A blocking call reports its own
// rows after the stream sync; async calls are reported by the next ocm_wait.
#include "lists.h"
#include "ocm/indexed.h"

using namespace ocm;
using namespace ocmlib;

static const ListNames kIndexed = {"ocm_copy_onesided_indexed", "indexed one-sided copies", "ocm_indexed", "indexed", false};

// Every op against the pair (indexed_check_op). Adds to *rows and *moved.
static int check_indexed_ops(lib_alloc *a, const struct ocm_indexed_params *ops, int n_ops, uint64_t *rows, uint64_t *moved) {
    char why[256];
    for (int i = 0; i < n_ops; i++) {
        uint64_t n = 0;
        if (indexed_check_op(ops[i], a->local_bytes, a->remote_bytes, &n, why, sizeof(why)) != 0)
            OCM_FAIL(-1, "indexed op %d: %s", i, why);
        *moved += n;
        if (n) *rows += ops[i].rows;
    }
    return 0;
}

namespace ocmlib {

// The allocation's skip words, made on first use (the device word zeroed on `st`, which
// every later op of the allocation is ordered after).
int skip_words(lib_alloc *a, hipStream_t st) {
    if (a->skip_dev) return 0;
    State &s = S();
    void *dev = nullptr, *host = nullptr;
    hipError_t err = local_pool() ? hipMallocFromPoolAsync(&dev, 8, s.pool, st) : hipMallocAsync(&dev, 8, st);
    if (err == hipSuccess) err = hipMemsetAsync(dev, 0, 8, st);
    if (err == hipSuccess) err = hipHostMalloc(&host, 8, hipHostMallocDefault);
    if (err != hipSuccess) {
        (void)hipGetLastError();
        if (dev) (void)hipFreeAsync(dev, st);
        OCM_FAIL(-1, "indexed skip counter: %s", hipGetErrorString(err));
    }
    a->skip_dev = static_cast<unsigned long long *>(dev);
    a->skip_host = static_cast<unsigned long long *>(host);
    *a->skip_host = 0;
    a->skip_seen = 0;
    return 0;
}

int indexed_take_skips(lib_alloc *a) {
    uint64_t k = a->skip_host_path;
    a->skip_host_path = 0;
    if (a->skip_host) {
        const uint64_t now = __atomic_load_n(a->skip_host, __ATOMIC_ACQUIRE);
        k += now - a->skip_seen;
        a->skip_seen = now;
    }
    return indexed_fail_skips(k);
}

int indexed_fail_skips(uint64_t k) {
    if (k == 0) return 0;
    S().ctr.n_indexed_skipped += k;
    OCM_FAIL(-1, "indexed ops skipped %llu row(s): index outside its table", (unsigned long long)k);
}

void indexed_release(lib_alloc *a) {
    if (!a->skip_dev && !a->skip_host) return;
    State &s = S();
    DeviceGuard g(s.device);
    if (a->skip_dev) (void)hipFreeAsync(a->skip_dev, s.stream);
    if (a->skip_host) (void)hipHostFree(a->skip_host);
    a->skip_dev = a->skip_host = nullptr;
}

}  // namespace ocmlib

// The host path: indices in host memory, rows through xfer(). *skipped: rows not moved.
static int indexed_host(lib_alloc *a, const struct ocm_indexed_params *ops, int n_ops, bool async, uint64_t *skipped) {
    // the indices are read now: after the allocation's queued work and what ocm_stream_wait named
    if (wait_alloc(a) != 0 || honor_dep(a, nullptr, true) != 0) return -1;
    std::vector<char> idx;
    for (int i = 0; i < n_ops; i++) {
        const ocm_indexed_params &p = ops[i];
        if (p.rows == 0 || p.row_bytes == 0) continue;
        const uint64_t isz = indexed_index_bytes(p.index_type), bytes = p.rows * isz;
        const uint64_t offs[2] = {p.local_index_offset, p.remote_index_offset};
        const char *arr[2] = {nullptr, nullptr};  // per side: the array, in host memory
        if (a->loc == LOC_DEVICE) idx.resize((size_t)(2 * bytes));
        for (int sd = 0; sd < 2; sd++) {
            if (offs[sd] == OCM_INDEX_NONE) continue;
            const char *src = static_cast<const char *>(a->local) + offs[sd];
            if (a->loc == LOC_DEVICE) {
                char *dst = idx.data() + sd * bytes;
                if (copy_local(dst, LOC_HOST, src, LOC_DEVICE, (size_t)bytes) != 0) return -1;
                src = dst;
            }
            arr[sd] = src;
        }
        for (uint64_t j = 0; j < p.rows; j++) {
            const uint64_t lr = arr[0] ? indexed_load_host(arr[0], 0, p.index_type, j) : j;
            const uint64_t rr = arr[1] ? indexed_load_host(arr[1], 0, p.index_type, j) : j;
            if (!indexed_in_range(lr, p.local_rows) || !indexed_in_range(rr, p.remote_rows)) {
                (*skipped)++;
                continue;
            }
            if (xfer(a, p.op_flag != 0, static_cast<char *>(a->local) + p.local_offset + lr * p.local_stride, a->loc,
                     p.remote_offset + rr * p.remote_stride, p.row_bytes, async) != 0)
                return -1;
        }
    }
    return 0;
}

// *ran: the transfer was made (rows may have been skipped, which fails the call all the same).
static int indexed_impl(ocm_alloc_t a, const struct ocm_indexed_params *ops, int n_ops, int flags, uint64_t *rows,
                        uint64_t *moved, bool *ran) {
    std::unique_lock<std::recursive_mutex> lk;
    const int path = list_enter(kIndexed, lk, a, ops, n_ops,
                                [&] { return check_indexed_ops(a, ops, n_ops, rows, moved) != 0 ? -1 : *moved != 0; });
    if (path <= PATH_NONE) {
        *ran = path == PATH_NONE;
        return path;
    }
    State &s = S();
    const bool async = (flags & OCM_BATCH_ASYNC) != 0;
    if (path == PATH_HOST) {
        uint64_t skipped = 0;
        if (indexed_host(a, ops, n_ops, async, &skipped) != 0) return -1;
        *ran = true;
        if (skipped == 0) return 0;
        if (async) {  // the next ocm_wait reports them
            a->skip_host_path += skipped;
            return 0;
        }
        return indexed_fail_skips(skipped);
    }
    DeviceGuard guard(s.device);
    std::vector<XferIndexedOp> v((size_t)n_ops);
    for (int i = 0; i < n_ops; i++) v[i] = indexed_op(ops[i]);
    XferIndexedArgs args;
    if (list_fill_args(a, v, 0, xfer_indexed_plan, &args) != 0) return -1;
    // a blocking call reports its own rows only: what queued async lists skipped stays for ocm_wait
    if (!async && wait_alloc(a) != 0) return -1;
    if (skip_words(a, async ? lane_stream(a) : s.stream) != 0) return -1;
    const uint64_t base = __atomic_load_n(a->skip_host, __ATOMIC_ACQUIRE);
    args.skipped = a->skip_dev;
    args.skipped_host = a->skip_host;
    if (run_list(a, args, v, xfer_indexed_launch, async) != 0) return -1;
    *ran = true;
    if (async) return 0;
    const uint64_t k = __atomic_load_n(a->skip_host, __ATOMIC_ACQUIRE) - base;
    a->skip_seen += k;
    return indexed_fail_skips(k);
}

extern "C" {

int ocm_copy_onesided_indexed(ocm_alloc_t a, const struct ocm_indexed_params *ops, int n_ops, int flags) {
    uint64_t rows = 0, moved = 0;
    bool ran = false;
    return abi_call(kIndexed.range, false, kIndexed.op, moved, [&] { return indexed_impl(a, ops, n_ops, flags, &rows, &moved, &ran); },
                    [&](OpCounters &c, uint64_t, bool) {
                        if (!ran) return;
                        c.n_indexed++;
                        c.n_indexed_ops += (uint64_t)n_ops;
                        c.n_indexed_rows += rows;
                        c.bytes_indexed += moved;
                    });
}

}  // extern "C"
