// Kernel dispatch on user-mode AQL queues owned by libocm (HSA runtime), next
// to HIP's streams.
//
// The resident copy service lives on such a queue. HIP does not know it, so a
// device-wide synchronize (hipDeviceSynchronize, torch.cuda.synchronize) never
// waits for the persistent kernel, and the service can stay resident across an
// application's compute phases instead of leaving after 50 us (the round-3
// design, which made every small op after an idle gap pay a relaunch). A
// dispatch is one 64-byte packet and a doorbell store: 0.04 us of host time
// against 2.2 us for hipLaunchKernelGGL (profiles/hsa_dispatch_probe_r04.json).
//
// The kernels come from a gfx950 device code object embedded in libocm at build
// time (the same xfer_service.hip source the HIP fat binary is built from), loaded into
// an HSA executable for the agent whose PCI location matches the HIP device.
#pragma once
#include <cstddef>
#include <cstdint>

namespace ocm {

struct AqlKernel {
    uint64_t object = 0;         // kernel descriptor address
    uint32_t kernarg_bytes = 0;  // explicit + hidden arguments
    uint32_t group_bytes = 0;    // static LDS
    uint32_t private_bytes = 0;  // scratch per work-item
};

// One queue, its completion signal (the dispatches still running: every
// dispatch adds one, the packet processor subtracts one when it completes) and
// kernarg slots used in turn, so a dispatch may follow one that is still
// running (the packets carry no barrier bit: the second starts as soon as every
// workgroup of the first has been dispatched).
struct AqlLane {
    void *queue = nullptr;  // hsa_queue_t *
    uint64_t signal = 0;    // hsa_signal_t handle
    void *kernarg = nullptr;
    unsigned slot = 0;      // kernarg slot of the last dispatch
    bool busy = false;      // a dispatch was issued and not yet seen complete
    bool kernarg_wc = false;  // kernarg buffer in write-combined host memory (else the runtime's pool)
    // Pre-armed dispatch (OCM_SERVICE_PREARM, round 5): a barrier-AND packet gated on
    // one of `gates`, then a dispatch whose arguments are written when it is fired. A
    // gate is closed again (set to 1) only for a barrier the packet processor has not
    // reached yet, and only once it has consumed the last barrier on that gate: the
    // packet processor may look at an opened gate some time after the host's store, and
    // re-closing it first (one gate for every arm) left the fired dispatch waiting.
    static constexpr int kGates = 4;
    uint64_t gates[kGates] = {};     // hsa_signal_t handles (1: closed)
    uint64_t gate_pkt[kGates] = {};  // queue index + 1 of the last barrier on each gate (0: none)
    unsigned gate_cur = 0;
    bool armed = false;
    unsigned armed_slot = 0;
    uint32_t armed_nargs = 0;
};

// Load the embedded code object for HIP device `hip_device` (idempotent per
// process). 0 on success; -1 with *why set when the HSA path is unusable.
int aql_open(int hip_device, const char **why);
// The kernel named `symbol` in the embedded code object (after aql_open).
int aql_kernel(const char *symbol, AqlKernel *k);
int aql_lane_create(AqlLane *l, bool high_priority);
void aql_lane_destroy(AqlLane *l);
// One 1-D dispatch of `blocks` x `threads`: `args` (the explicit kernel
// arguments, `nargs` bytes) followed by the hidden arguments the code object
// reads (block count, group size, grid dimensions). The lane must be idle unless
// `overlap`: then at most one dispatch may still run (its kernel must have read
// its arguments already), and the new one starts once all of its workgroups
// have been dispatched. `barrier`: the new one starts only once every earlier
// dispatch of the lane has completed (the packet's barrier bit).
int aql_dispatch(AqlLane *l, const AqlKernel &k, const void *args, size_t nargs, unsigned blocks, unsigned threads,
                 bool overlap = false, bool barrier = false);
// Pre-arm the lane's next dispatch (a relaunch after an idle gap
// costs ~12 us more than a hot op): queue a barrier-AND packet gated on the lane's gate
// signal and behind it a dispatch of `k` (`blocks` x `threads`, explicit arguments of
// `nargs` bytes, all zero until fired). aql_fire writes the arguments and opens the gate:
// one store, no packet to write or doorbell to ring, and the packet processor has both
// packets already. A dispatch fired with all-zero arguments is cancelled (the kernel
// must return at once on them). An armed dispatch does not count as running.
int aql_arm(AqlLane *l, const AqlKernel &k, size_t nargs, unsigned blocks, unsigned threads);
int aql_fire(AqlLane *l, const void *args, size_t nargs);
// Fire the armed dispatch with zero arguments (cancelled), if one is armed.
void aql_disarm(AqlLane *l);
// Whether the lane's dispatches have completed (a load of its signal).
bool aql_lane_idle(AqlLane *l);
// Dispatches of the lane still running.
long aql_lane_inflight(AqlLane *l);
// Wait up to timeout_ns for the lane's dispatch to complete. 0: idle.
int aql_lane_wait(AqlLane *l, uint64_t timeout_ns);

}  // namespace ocm
