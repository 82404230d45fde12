// libocm strided converting ops (ocm_copy_onesided_quant_strided): rows of 16-bit
// elements in the local half, one MXFP8 or MXFP4 record per row in the remote half, one stride
// per side (ocm/quant_strided.h). A device local half takes one kernel launch per list,
// uploaded and ordered like a batch (run_list); a host local half (a CPU app,
// OCM_REMOTE_RDMA / _RMA pairs, the network tier) goes op by op, row by row, in order,
// through the converting host path (quant_host): each row is a plain converting op.
#include "lists.h"
#include "ocm/quant_strided.h"

using namespace ocm;
using namespace ocmlib;

static const ListNames kQuantStrided = {"ocm_copy_onesided_quant_strided", "strided converting one-sided copies",
                                        "ocm_quant_strided", "quant_strided", true};

// Every op against the pair (quant_strided_check_op). Adds to *src / *wire.
static int check_ops(lib_alloc *a, const struct ocm_quant_strided_params *ops, int n_ops, uint64_t *src, uint64_t *wire) {
    char why[192];
    for (int i = 0; i < n_ops; i++) {
        uint64_t s = 0, w = 0;
        if (quant_strided_check_op(ops[i], a->local_bytes, a->remote_bytes, &s, &w, why, sizeof(why)) != 0)
            OCM_FAIL(-1, "quant_strided op %d: %s", i, why);
        *src += s;
        *wire += w;
    }
    return 0;
}

static int quant_strided_impl(ocm_alloc_t a, const struct ocm_quant_strided_params *ops, int n_ops, int flags, uint64_t *src,
                              uint64_t *wire) {
    std::unique_lock<std::recursive_mutex> lk;
    const int path = list_enter(kQuantStrided, lk, a, ops, n_ops,
                                [&] { return check_ops(a, ops, n_ops, src, wire) != 0 ? -1 : *src != 0; });
    if (path <= PATH_NONE) return path;
    if (path == PATH_HOST) {
        int i = 0;
        uint64_t r = 0;
        return quant_host(a, [&](ocm_quant_params *q) {
            while (i < n_ops && (ops[i].row_elems == 0 || r == ops[i].rows)) i++, r = 0;  // past empty and finished ops
            if (i == n_ops) return false;
            const ocm_quant_strided_params &p = ops[i];
            *q = {p.local_offset + r * p.local_stride, p.remote_offset + r * p.remote_stride, p.row_elems, p.op_flag, p.dtype};
            r++;
            return true;
        });
    }
    DeviceGuard guard(S().device);
    std::vector<XferQuantStridedOp> v((size_t)n_ops);
    for (int i = 0; i < n_ops; i++) v[i] = quant_strided_op(ops[i]);
    XferQuantStridedArgs args;
    if (list_fill_args(a, v, kQuantTileShift, xfer_quant_strided_plan, &args) != 0) return -1;
    return run_list(a, args, v, xfer_quant_strided_launch, (flags & OCM_BATCH_ASYNC) != 0);
}

extern "C" {

int ocm_copy_onesided_quant_strided(ocm_alloc_t a, const struct ocm_quant_strided_params *ops, int n_ops, int flags) {
    uint64_t src = 0, wire = 0;
    return list_call(kQuantStrided, wire, [&] { return quant_strided_impl(a, ops, n_ops, flags, &src, &wire); },
                     [&](OpCounters &c, uint64_t) {
                         c.n_quant_strided++;
                         c.n_quant_strided_ops += (uint64_t)n_ops;
                         c.bytes_quant_strided_src += src;
                         c.bytes_quant_strided_wire += wire;
                     });
}

}  // extern "C"
