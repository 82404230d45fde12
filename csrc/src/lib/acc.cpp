// libocm one-sided accumulate (ocm_copy_onesided_accumulate): fp32 accumulators in the
// remote half, remote += scale * local (ocm/acc.h has the element rule). A pair with a
// device-side path takes one kernel launch per list, uploaded and ordered like a batch;
// every other pair (a CPU app, a host local half, the network tier) goes op by op on this
// thread: a get into a bounce buffer, the same rule on the CPU, a put back.
#include "internal.h"
#include "ocm/acc.h"

using namespace ocm;
using namespace ocmlib;

// Every op against the pair (acc_check_op). Adds the accumulator bytes to *bytes.
static int check_acc_ops(lib_alloc *a, const struct ocm_acc_params *ops, int n_ops, uint64_t *bytes) {
    char why[192];
    for (int i = 0; i < n_ops; i++) {
        uint64_t n = 0;
        if (acc_check_op(ops[i], a->local_bytes, a->remote_bytes, &n, why, sizeof(why)) != 0)
            OCM_FAIL(-1, "accumulate op %d: %s", i, why);
        *bytes += n;
    }
    return 0;
}

// No device-side path: op by op, in chunks of at most 1 MiB of accumulators, blocking.
static int acc_host(lib_alloc *a, const struct ocm_acc_params *ops, int n_ops) {
    State &s = S();
    if (s.device >= 0) {
        // the CPU reads the local half: after queued async ops and stream dependencies
        DeviceGuard guard(s.device);
        if (wait_alloc(a) != 0) return -1;
        if (honor_dep(a, nullptr, true) != 0) return -1;
    }
    constexpr uint64_t kChunkElems = (1ull << 20) / 4;
    std::vector<float> bounce;
    for (int i = 0; i < n_ops; i++) {
        const ocm_acc_params &p = ops[i];
        const uint32_t esize = acc_elem_size(p.dtype);
        const char *loc = static_cast<const char *>(a->local) + p.local_offset;
        for (uint64_t done = 0; done < p.elems; done += kChunkElems) {
            const uint64_t n = std::min(kChunkElems, p.elems - done);
            bounce.resize(n);
            char *b = reinterpret_cast<char *>(bounce.data());
            if (xfer(a, false, b, LOC_HOST, p.remote_offset + 4 * done, 4 * n, false) != 0) return -1;
            acc_apply_host(bounce.data(), loc + done * esize, n, p.dtype, p.scale);
            if (xfer(a, true, b, LOC_HOST, p.remote_offset + 4 * done, 4 * n, false) != 0) return -1;
        }
    }
    return 0;
}

static int acc_impl(ocm_alloc_t a, const struct ocm_acc_params *ops, int n_ops, int flags, uint64_t *bytes) {
    State &s = S();
    std::lock_guard<std::recursive_mutex> lk(s.mu);
    if (!a || (!ops && n_ops)) OCM_FAIL(-1, "ocm_copy_onesided_accumulate: NULL argument");
    if (!s.allocs.count(a)) OCM_FAIL(-1, "ocm_copy_onesided_accumulate: unknown allocation");
    if (!a->remote) OCM_FAIL(-1, "one-sided accumulates need a remote pair (kind %d)", (int)a->kind);
    if (n_ops < 0) OCM_FAIL(-1, "ocm_copy_onesided_accumulate: n_ops < 0");
    if (check_acc_ops(a, ops, n_ops, bytes) != 0) return -1;
    if (n_ops == 0 || *bytes == 0) return 0;
    if (!batch_device_path(a)) {
        if (a->loc == LOC_DEVICE)
            OCM_FAIL(-1, "ocm_copy_onesided_accumulate: a device local half needs every extent reachable by a kernel "
                         "(no network tier, stripe unit >= 16 bytes)");
        return acc_host(a, ops, n_ops);
    }
    DeviceGuard guard(s.device);
    XferBatchArgs args;
    std::vector<XferBatchOp> v((size_t)n_ops, XferBatchOp{});
    for (int i = 0; i < n_ops; i++) acc_pack(ops[i], &v[i]);
    batch_layout_args(a, false, &args);
    args.tile_shift = kAccTileShift;
    args.n_ops = (uint32_t)v.size();
    args.total_tiles = acc_plan(v.data(), (uint32_t)v.size());
    args.grid = xfer_batch_grid(args.total_tiles, args.host_tier != 0);
    if (v.size() <= (size_t)kXferInlineOps) std::memcpy(args.inline_ops, v.data(), v.size() * sizeof(XferBatchOp));
    return run_batch(a, args, v, (flags & OCM_BATCH_ASYNC) != 0, LIST_ACC);
}

extern "C" {

int ocm_copy_onesided_accumulate(ocm_alloc_t a, const struct ocm_acc_params *ops, int n_ops, int flags) {
    TraceRange tr("ocm_accumulate");
    const uint64_t t0 = now_ns();
    uint64_t bytes = 0;
    const int rc = acc_impl(a, ops, n_ops, flags, &bytes);
    const uint64_t t1 = now_ns();
    if (rc == 0) {
        OpCounters &c = S().ctr;
        c.n_acc++;
        c.n_acc_ops += (uint64_t)n_ops;
        c.bytes_acc += bytes;
    }
    trace_op("acc", bytes, t0, t1, rc);
    return rc;
}

}  // extern "C"
