// libocm converting one-sided ops (ocm_copy_onesided_quant): 16-bit elements in
// the local half, MXFP8 or MXFP4 records (ocm/mx8.h, ocm/mx4.h; the op's dtype word
// says which) in the remote half. A device local
// half takes one kernel launch per list (ocm/quant.h), ordered like a batch; a
// host local half (a CPU app, OCM_REMOTE_RDMA / _RMA pairs, the network tier)
// encodes and decodes on this thread and moves each record with xfer().
#include "lists.h"
#include "ocm/mx4.h"

using namespace ocm;
using namespace ocmlib;

static const ListNames kQuant = {"ocm_copy_onesided_quant", "converting one-sided copies", "ocm_quant", "quant", true};

// Every op against the pair and the format's constraints. Adds to *src / *wire.
static int check_quant_ops(lib_alloc *a, const struct ocm_quant_params *ops, int n_ops, uint64_t *src, uint64_t *wire) {
    for (int i = 0; i < n_ops; i++) {
        const ocm_quant_params &p = ops[i];
        char why[96];
        if (quant_check_dtype(p.dtype, why, sizeof(why)) != 0) OCM_FAIL(-1, "quant op %d: %s", i, why);
        if (p.elems % kMx8Group != 0 || p.elems >= (1ull << 31))
            OCM_FAIL(-1, "quant op %d: %llu elements (a multiple of 32 below 2^31 is needed)", i,
                     (unsigned long long)p.elems);
        if (p.local_offset % 16 != 0)
            OCM_FAIL(-1, "quant op %d: local offset %llu is not a multiple of 16", i, (unsigned long long)p.local_offset);
        if (p.remote_offset % 32 != 0)
            OCM_FAIL(-1, "quant op %d: remote offset %llu is not a multiple of 32", i,
                     (unsigned long long)p.remote_offset);
        const uint64_t lbytes = 2 * p.elems, rbytes = quant_record_bytes(p.elems, p.dtype);
        if (p.local_offset > a->local_bytes || lbytes > a->local_bytes - p.local_offset)
            OCM_FAIL(-1, "quant op %d: local range [%llu,+%llu) exceeds %zu bytes", i,
                     (unsigned long long)p.local_offset, (unsigned long long)lbytes, a->local_bytes);
        if (p.remote_offset > a->remote_bytes || rbytes > a->remote_bytes - p.remote_offset)
            OCM_FAIL(-1, "quant op %d: remote range [%llu,+%llu) exceeds %zu bytes", i,
                     (unsigned long long)p.remote_offset, (unsigned long long)rbytes, a->remote_bytes);
        *src += lbytes;
        *wire += rbytes;
    }
    return 0;
}

// Host local half: record by record, in the order `next` yields them; a record is
// contiguous on the remote side.
int ocmlib::quant_host(lib_alloc *a, const std::function<bool(ocm_quant_params *)> &next) {
    State &s = S();
    if (s.device >= 0) {
        // the CPU reads and writes the local half: after queued async ops and stream dependencies
        DeviceGuard guard(s.device);
        if (wait_alloc(a) != 0) return -1;
        if (honor_dep(a, nullptr, true) != 0) return -1;
    }
    std::vector<uint8_t> rec;
    for (ocm_quant_params p; next(&p);) {
        if (p.elems == 0) continue;
        uint16_t *loc = reinterpret_cast<uint16_t *>(static_cast<char *>(a->local) + p.local_offset);
        const size_t rbytes = quant_record_bytes(p.elems, p.dtype);
        rec.resize(rbytes);
        if (p.op_flag != 0) quant_encode(loc, p.elems, p.dtype, rec.data());
        if (xfer(a, p.op_flag != 0, reinterpret_cast<char *>(rec.data()), LOC_HOST, p.remote_offset, rbytes, false) != 0)
            return -1;
        if (p.op_flag == 0) quant_decode(rec.data(), p.elems, p.dtype, loc);
    }
    return 0;
}

static int quant_impl(ocm_alloc_t a, const struct ocm_quant_params *ops, int n_ops, int flags, uint64_t *src,
                      uint64_t *wire) {
    std::unique_lock<std::recursive_mutex> lk;
    const int path = list_enter(kQuant, lk, a, ops, n_ops,
                                [&] { return check_quant_ops(a, ops, n_ops, src, wire) != 0 ? -1 : *src != 0; });
    if (path <= PATH_NONE) return path;
    if (path == PATH_HOST) {
        int i = 0;
        return quant_host(a, [&](ocm_quant_params *p) { return i < n_ops ? (*p = ops[i++], true) : false; });
    }
    DeviceGuard guard(S().device);
    std::vector<XferBatchOp> v((size_t)n_ops, XferBatchOp{});
    for (int i = 0; i < n_ops; i++) {
        v[i].lin_off = ops[i].local_offset;
        v[i].rem_off = ops[i].remote_offset;
        v[i].len = ops[i].elems;
        v[i].put = ops[i].op_flag != 0;
        v[i].pad = ops[i].dtype;
    }
    XferBatchArgs args;
    if (list_fill_args(a, v, kQuantTileShift, [](XferBatchOp *o, uint32_t n, uint32_t) { return xfer_quant_plan(o, n); }, &args) != 0) return -1;
    return run_list(a, args, v, xfer_quant_launch, (flags & OCM_BATCH_ASYNC) != 0);
}

extern "C" {

size_t ocm_quant_bytes(uint64_t elems) { return mx8_record_bytes(elems); }

size_t ocm_quant_bytes_fmt(uint64_t elems, uint32_t format) {
    return format == OCM_QUANT_MXFP8 || format == OCM_QUANT_MXFP4 ? quant_record_bytes(elems, format) : 0;
}

int ocm_copy_onesided_quant(ocm_alloc_t a, const struct ocm_quant_params *ops, int n_ops, int flags) {
    uint64_t src = 0, wire = 0;
    return list_call(kQuant, wire, [&] { return quant_impl(a, ops, n_ops, flags, &src, &wire); },
                     [&](OpCounters &c, uint64_t) {
                         c.n_quant++;
                         c.n_quant_ops += (uint64_t)n_ops;
                         c.bytes_quant_src += src;
                         c.bytes_quant_wire += wire;
                     });
}

}  // extern "C"
