// libocm strided one-sided ops (ocm_copy_onesided_strided): rows of row_bytes, one
// stride per side (ocm/strided.h). A pair with a device-side path takes one kernel
// launch per list, uploaded and ordered like a batch (run_list); every other pair (a
// CPU app, a host local half, the network tier) goes op by op, row by row, in order,
// through xfer(), as the batch fallback does.
#include "lists.h"
#include "ocm/strided.h"

using namespace ocm;
using namespace ocmlib;

static const ListNames kStrided = {"ocm_copy_onesided_strided", "strided one-sided copies", "ocm_strided", "strided", false};

// Every op against the pair (strided_check_op). Adds the bytes to *moved.
static int check_strided_ops(lib_alloc *a, const struct ocm_strided_params *ops, int n_ops, uint64_t *moved) {
    char why[192];
    for (int i = 0; i < n_ops; i++) {
        uint64_t n = 0;
        if (strided_check_op(ops[i], a->local_bytes, a->remote_bytes, &n, why, sizeof(why)) != 0)
            OCM_FAIL(-1, "strided op %d: %s", i, why);
        *moved += n;
    }
    return 0;
}

static int strided_impl(ocm_alloc_t a, const struct ocm_strided_params *ops, int n_ops, int flags, uint64_t *moved) {
    std::unique_lock<std::recursive_mutex> lk;
    const int path = list_enter(kStrided, lk, a, ops, n_ops,
                                [&] { return check_strided_ops(a, ops, n_ops, moved) != 0 ? -1 : *moved != 0; });
    if (path <= PATH_NONE) return path;
    const bool async = (flags & OCM_BATCH_ASYNC) != 0;
    if (path == PATH_HOST) {
        for (int i = 0; i < n_ops; i++) {
            const ocm_strided_params &p = ops[i];
            if (p.row_bytes == 0) continue;
            for (uint64_t r = 0; r < p.rows; r++)
                if (xfer(a, p.op_flag != 0, static_cast<char *>(a->local) + p.local_offset + r * p.local_stride, a->loc,
                         p.remote_offset + r * p.remote_stride, p.row_bytes, async) != 0)
                    return -1;
        }
        return 0;
    }
    DeviceGuard guard(S().device);
    std::vector<XferStridedOp> v((size_t)n_ops, XferStridedOp{});
    for (int i = 0; i < n_ops; i++) {
        const bool empty = ops[i].rows == 0 || ops[i].row_bytes == 0;  // no tiles, whatever its other fields say
        v[i].lin_off = ops[i].local_offset;
        v[i].rem_off = ops[i].remote_offset;
        v[i].row_bytes = empty ? 0 : ops[i].row_bytes;
        v[i].rows = empty ? 0 : (uint32_t)ops[i].rows;
        v[i].lin_stride = ops[i].local_stride;
        v[i].rem_stride = ops[i].remote_stride;
        v[i].put = ops[i].op_flag != 0;
    }
    XferStridedArgs args;
    if (list_fill_args(a, v, 0, xfer_strided_plan, &args) != 0) return -1;
    return run_list(a, args, v, xfer_strided_launch, async);
}

extern "C" {

int ocm_copy_onesided_strided(ocm_alloc_t a, const struct ocm_strided_params *ops, int n_ops, int flags) {
    uint64_t moved = 0;
    return list_call(kStrided, moved, [&] { return strided_impl(a, ops, n_ops, flags, &moved); },
                     [&](OpCounters &c, uint64_t) {
                         c.n_strided++;
                         c.n_strided_ops += (uint64_t)n_ops;
                         c.bytes_strided += moved;
                     });
}

}  // extern "C"
