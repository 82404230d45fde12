// libocm strided one-sided ops (ocm_copy_onesided_strided): rows of row_bytes, one
// stride per side (ocm/strided.h). A pair with a device-side path takes one kernel
// launch per list, uploaded and ordered like a batch (run_list); every other pair (a
// CPU app, a host local half, the network tier) goes op by op, row by row, in order,
// through xfer(), as the batch fallback does.
#include "internal.h"
#include "ocm/strided.h"

using namespace ocm;
using namespace ocmlib;

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
    State &s = S();
    std::lock_guard<std::recursive_mutex> lk(s.mu);
    if (!a || (!ops && n_ops)) OCM_FAIL(-1, "ocm_copy_onesided_strided: NULL argument");
    if (!s.allocs.count(a)) OCM_FAIL(-1, "ocm_copy_onesided_strided: unknown allocation");
    if (!a->remote) OCM_FAIL(-1, "strided one-sided copies need a remote pair (kind %d)", (int)a->kind);
    if (n_ops < 0) OCM_FAIL(-1, "ocm_copy_onesided_strided: n_ops < 0");
    const bool async = (flags & OCM_BATCH_ASYNC) != 0;
    if (check_strided_ops(a, ops, n_ops, moved) != 0) return -1;
    if (n_ops == 0 || *moved == 0) return 0;
    if (!batch_device_path(a)) {
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
    DeviceGuard guard(s.device);
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
    struct Ctx {
        XferStridedArgs args;
        std::vector<XferStridedOp> &v;
    } ctx{{}, v};
    XferStridedArgs &args = ctx.args;
    XferBatchArgs lay;  // the pair's side: the linear base, the extents and how they stripe
    batch_layout_args(a, false, &lay);
    args.lin = lay.lin;
    static_assert(sizeof(args.ext) == sizeof(lay.ext), "extent table of a pair");
    std::memcpy(args.ext, lay.ext, sizeof(args.ext));
    args.unit_shift = lay.unit_shift;
    args.n_ext = lay.n_ext;
    args.host_tier = lay.host_tier;
    args.tile_shift = xfer_batch_tile_shift(args.n_ext, args.unit_shift);
    args.n_ops = (uint32_t)v.size();
    args.total_tiles = xfer_strided_plan(v.data(), (uint32_t)v.size(), args.tile_shift);
    args.grid = xfer_batch_grid(args.total_tiles, args.host_tier != 0);
    BatchList list;
    list.desc = v.data();
    list.desc_bytes = v.size() * sizeof(XferStridedOp);
    list.large = v.size() > (size_t)kStridedInlineOps;
    list.grid = args.grid;
    list.ctx = &ctx;
    if (!list.large) std::memcpy(args.inline_ops, v.data(), list.desc_bytes);
    list.wave_ops = [](void *p, uint32_t *out) {
        Ctx &c = *static_cast<Ctx *>(p);
        xfer_strided_wave_ops(c.v.data(), (uint32_t)c.v.size(), c.args.total_tiles, c.args.grid, out);
    };
    list.launch = [](void *p, const void *dev_desc, const uint32_t *dev_wave, hipStream_t st) {
        Ctx &c = *static_cast<Ctx *>(p);
        c.args.ops = static_cast<const XferStridedOp *>(dev_desc);
        c.args.wave_op = dev_wave;
        return xfer_strided_launch(c.args, S().tuning, st);
    };
    return run_list(a, list, async);
}

extern "C" {

int ocm_copy_onesided_strided(ocm_alloc_t a, const struct ocm_strided_params *ops, int n_ops, int flags) {
    TraceRange tr("ocm_strided");
    const uint64_t t0 = now_ns();
    uint64_t moved = 0;
    const int rc = strided_impl(a, ops, n_ops, flags, &moved);
    const uint64_t t1 = now_ns();
    if (rc == 0) {
        OpCounters &c = S().ctr;
        c.n_strided++;
        c.n_strided_ops += (uint64_t)n_ops;
        c.bytes_strided += moved;
    }
    trace_op("strided", moved, t0, t1, rc);
    return rc;
}

}  // extern "C"
