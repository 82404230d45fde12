// libocm indexed converting ops (ocm_copy_onesided_quant_indexed): rows of 16-bit elements
// out of a table in the local half, one MXFP8 or MXFP4 record per row out of a table of
// records in the remote half, the row on either side picked by index arrays in the local
// half (ocm/quant_indexed.h). A device local half takes one kernel launch per list,
// uploaded and ordered like a batch (run_list); the kernel reads the indices, skips rows
// whose index is outside its table and counts them into the allocation's skip words, the
// ones the indexed op counts into (indexed.cpp), so ocm_wait and the n_indexed_skipped
// counter see the rows skipped by either call. A host local half (a CPU app,
// OCM_REMOTE_RDMA / _RMA pairs, the network tier) has its index arrays in host memory
// already, as every converting host path has its elements: it goes op by op, row by row,
// in order, each in-range row a plain converting op through quant_host, with the same
// rule.
#include "lists.h"
#include "ocm/quant_indexed.h"

using namespace ocm;
using namespace ocmlib;

static const ListNames kQuantIndexed = {"ocm_copy_onesided_quant_indexed", "indexed converting one-sided copies",
                                        "ocm_quant_indexed", "quant_indexed", true};

// What a call names, nominal: every row of every non-empty op, in range or not.
struct Named {
    uint64_t rows = 0, src = 0, wire = 0;
};

// Every op against the pair (quant_indexed_check_op). Adds to *n.
static int check_ops(lib_alloc *a, const struct ocm_quant_indexed_params *ops, int n_ops, Named *n) {
    char why[256];
    for (int i = 0; i < n_ops; i++) {
        uint64_t s = 0, w = 0;
        if (quant_indexed_check_op(ops[i], a->local_bytes, a->remote_bytes, &s, &w, why, sizeof(why)) != 0)
            OCM_FAIL(-1, "quant_indexed op %d: %s", i, why);
        n->src += s;
        n->wire += w;
        if (s) n->rows += ops[i].rows;
    }
    return 0;
}

// The host path: the indices are read where they lie, after the allocation's queued work
// and what ocm_stream_wait named (quant_host waits before it asks for the first op).
// *skipped: rows not moved.
static int quant_indexed_host(lib_alloc *a, const struct ocm_quant_indexed_params *ops, int n_ops, uint64_t *skipped) {
    const char *base = static_cast<const char *>(a->local);
    int i = 0;
    uint64_t j = 0;
    return quant_host(a, [&](ocm_quant_params *q) {
        for (;;) {
            while (i < n_ops && (ops[i].row_elems == 0 || j == ops[i].rows)) i++, j = 0;  // past empty and finished ops
            if (i == n_ops) return false;
            if (quant_indexed_host_row(ops[i], base, j++, q)) return true;
            (*skipped)++;
        }
    });
}

// *ran: the transfer was made (rows may have been skipped, which fails the call all the same).
static int quant_indexed_impl(ocm_alloc_t a, const struct ocm_quant_indexed_params *ops, int n_ops, int flags, Named *named,
                              bool *ran) {
    std::unique_lock<std::recursive_mutex> lk;
    const int path = list_enter(kQuantIndexed, lk, a, ops, n_ops,
                                [&] { return check_ops(a, ops, n_ops, named) != 0 ? -1 : named->src != 0; });
    if (path <= PATH_NONE) {
        *ran = path == PATH_NONE;
        return path;
    }
    State &s = S();
    const bool async = (flags & OCM_BATCH_ASYNC) != 0;
    if (path == PATH_HOST) {
        uint64_t skipped = 0;
        if (quant_indexed_host(a, ops, n_ops, &skipped) != 0) return -1;
        *ran = true;
        if (skipped == 0) return 0;
        if (async) {  // the next ocm_wait reports them
            a->skip_host_path += skipped;
            return 0;
        }
        return indexed_fail_skips(skipped);
    }
    DeviceGuard guard(s.device);
    std::vector<XferQuantIndexedOp> v((size_t)n_ops);
    for (int i = 0; i < n_ops; i++) v[i] = quant_indexed_op(ops[i]);
    XferQuantIndexedArgs args;
    if (list_fill_args(a, v, kQuantTileShift, xfer_quant_indexed_plan, &args) != 0) return -1;
    // a blocking call reports its own rows only: what queued async lists skipped stays for ocm_wait
    if (!async && wait_alloc(a) != 0) return -1;
    if (skip_words(a, async ? lane_stream(a) : s.stream) != 0) return -1;
    const uint64_t base = __atomic_load_n(a->skip_host, __ATOMIC_ACQUIRE);
    args.skipped = a->skip_dev;
    args.skipped_host = a->skip_host;
    if (run_list(a, args, v, xfer_quant_indexed_launch, async) != 0) return -1;
    *ran = true;
    if (async) return 0;
    const uint64_t k = __atomic_load_n(a->skip_host, __ATOMIC_ACQUIRE) - base;
    a->skip_seen += k;
    return indexed_fail_skips(k);
}

extern "C" {

int ocm_copy_onesided_quant_indexed(ocm_alloc_t a, const struct ocm_quant_indexed_params *ops, int n_ops, int flags) {
    Named named;
    bool ran = false;
    return abi_call(kQuantIndexed.range, false, kQuantIndexed.op, named.wire,
                    [&] { return quant_indexed_impl(a, ops, n_ops, flags, &named, &ran); },
                    [&](OpCounters &c, uint64_t, bool) {
                        if (!ran) return;
                        c.n_quant_indexed++;
                        c.n_quant_indexed_ops += (uint64_t)n_ops;
                        c.n_quant_indexed_rows += named.rows;
                        c.bytes_quant_indexed_src += named.src;
                        c.bytes_quant_indexed_wire += named.wire;
                    });
}

}  // extern "C"
