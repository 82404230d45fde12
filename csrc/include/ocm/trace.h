// Tracing: roctx ranges (visible to rocprofv3 --marker-trace) around every
// control and data-plane operation, per-process counters, and an optional
// JSON-lines op log (OCM_TRACE_FILE=<path>, written at ocm_tini / daemon exit).
// The reference had no tracing at all; its comments only noted
// where timing would go (test/ib_client.c:24, src/extoll.c:148).
#pragma once
#include <cstdint>
#include <string>

namespace ocm {

struct OpCounters {
    uint64_t n_put = 0, n_get = 0, bytes_put = 0, bytes_get = 0;
    uint64_t n_alloc = 0, n_free = 0, n_copy = 0, bytes_copy = 0;
    uint64_t ns_put = 0, ns_get = 0, ns_alloc = 0, ns_free = 0;
    uint64_t n_batch = 0, n_batch_ops = 0, bytes_batch = 0, ns_batch = 0;
    uint64_t n_batch_launches = 0;  // batch kernels launched outside plans (batches, remote->remote copies)
    // converting ops (ocm_copy_onesided_quant): calls, ops, 16-bit source bytes, record bytes on the wire
    uint64_t n_quant = 0, n_quant_ops = 0, bytes_quant_src = 0, bytes_quant_wire = 0;
    uint64_t n_slab_fd = 0;         // host-tier slabs imported through an fd from their owner (SCM_RIGHTS)
    uint64_t n_slab_path = 0;       // ... through the /proc/<pid>/fd path fallback
    uint64_t n_link_rpc = 0;        // RPCs posted on the shared-memory link (ocm/shmlink.h)
    uint64_t n_link_wake = 0;       // ... of which had to wake the daemon over the socket
    // strided ops (ocm_copy_onesided_strided): calls, ops, bytes moved (rows * row_bytes)
    uint64_t n_strided = 0, n_strided_ops = 0, bytes_strided = 0;
    // accumulates (ocm_copy_onesided_accumulate): calls, ops, accumulator bytes updated (4 * elems)
    uint64_t n_acc = 0, n_acc_ops = 0, bytes_acc = 0;
    // strided converting ops (ocm_copy_onesided_quant_strided): calls, ops, 16-bit source bytes, record bytes
    uint64_t n_quant_strided = 0, n_quant_strided_ops = 0, bytes_quant_strided_src = 0, bytes_quant_strided_wire = 0;
    // indexed ops (ocm_copy_onesided_indexed): calls, ops, rows named, nominal bytes (rows * row_bytes),
    // rows skipped for an index outside its table (counted when their count is reported)
    uint64_t n_indexed = 0, n_indexed_ops = 0, n_indexed_rows = 0, bytes_indexed = 0, n_indexed_skipped = 0;
    // indexed converting ops (ocm_copy_onesided_quant_indexed): calls, ops, rows named, their 16-bit source
    // bytes and record bytes (nominal: every named row of every non-empty op); the rows they skip are
    // counted in n_indexed_skipped, with the indexed ops'
    uint64_t n_quant_indexed = 0, n_quant_indexed_ops = 0, n_quant_indexed_rows = 0, bytes_quant_indexed_src = 0,
             bytes_quant_indexed_wire = 0;
    // pooled lookups (ocm_copy_onesided_bag): calls, ops, bags and ids named, nominal bytes read
    // (ids * row bytes); the entries they skip are counted in n_indexed_skipped, with the indexed ops'
    uint64_t n_bag = 0, n_bag_ops = 0, n_bag_bags = 0, n_bag_ids = 0, bytes_bag = 0;
};

bool trace_enabled();  // OCM_TRACE=0 disables the roctx ranges
uint64_t now_ns();
// Record one finished operation into the bounded in-memory log (if enabled).
void trace_op(const char *op, uint64_t bytes, uint64_t t0_ns, uint64_t t1_ns, int rc);
// Write the op log to OCM_TRACE_FILE (append). Returns records written.
int trace_flush(const char *who);

class TraceRange {
public:
    explicit TraceRange(const char *name);
    ~TraceRange();
    TraceRange(const TraceRange &) = delete;
    TraceRange &operator=(const TraceRange &) = delete;

private:
    bool on_;
};

}  // namespace ocm
