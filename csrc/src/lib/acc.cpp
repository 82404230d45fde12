// libocm one-sided accumulate (ocm_copy_onesided_accumulate): fp32 accumulators in the
// remote half, remote += scale * local (ocm/acc.h has the element rule). A pair with a
// device-side path takes one kernel launch per list, uploaded and ordered like a batch;
// every other pair (a CPU app, a host local half, the network tier) goes op by op on this
// thread: a get into a bounce buffer, the same rule on the CPU, a put back.
#include "lists.h"
#include "ocm/acc.h"

using namespace ocm;
using namespace ocmlib;

static const ListNames kAcc = {"ocm_copy_onesided_accumulate", "one-sided accumulates", "ocm_accumulate", "acc", true};

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
    std::unique_lock<std::recursive_mutex> lk;
    const int path = list_enter(kAcc, lk, a, ops, n_ops, [&] { return check_acc_ops(a, ops, n_ops, bytes) != 0 ? -1 : *bytes != 0; });
    if (path <= PATH_NONE) return path;
    if (path == PATH_HOST) return acc_host(a, ops, n_ops);
    DeviceGuard guard(S().device);
    std::vector<XferBatchOp> v((size_t)n_ops, XferBatchOp{});
    for (int i = 0; i < n_ops; i++) acc_pack(ops[i], &v[i]);
    XferBatchArgs args;
    if (list_fill_args(a, v, kAccTileShift, [](XferBatchOp *o, uint32_t n, uint32_t) { return acc_plan(o, n); }, &args) != 0) return -1;
    return run_list(a, args, v, xfer_acc_launch, (flags & OCM_BATCH_ASYNC) != 0);
}

extern "C" {

int ocm_copy_onesided_accumulate(ocm_alloc_t a, const struct ocm_acc_params *ops, int n_ops, int flags) {
    uint64_t bytes = 0;
    return list_call(kAcc, bytes, [&] { return acc_impl(a, ops, n_ops, flags, &bytes); },
                     [&](OpCounters &c, uint64_t) {
                         c.n_acc++;
                         c.n_acc_ops += (uint64_t)n_ops;
                         c.bytes_acc += bytes;
                     });
}

}  // extern "C"
