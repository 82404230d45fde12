// Fused optimizer kernel that updates parameters in place while their state
// lives in a remote (striped) oncilla allocation: the kernel reads and writes
// the state straight from peer HBM over xGMI (or the pinned host tier), with
// no staging copy. See csrc/src/kernels/optim.hip.
#pragma once

#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstdint>

#include "ocm/xfer.h"

namespace ocm {

// What every tensor of a launch shares.
struct AdamArgs {
    char *ext[kXferMaxExtents];      // extent bases of the striped state space
    uint32_t n_ext;
    uint32_t unit_shift;             // log2(stripe unit) when n_ext > 1
    float b1, b2, eps, wd;           // betas, eps, L2 weight decay
    float omb1, omb2;                // 1 - b1, 1 - b2: computed in double by the caller, rounded once
    float step_size;                 // lr / (1 - b1^t)
    float inv_sqrt_bc2;              // 1 / sqrt(1 - b2^t)
    uint32_t bf16;                   // 1: p and g are bf16; fp32 master weights at w_off in the state
    uint32_t decoupled;              // 1: AdamW (p *= decay before the step; wd unused)
    float decay;                     // 1 - lr * weight_decay (AdamW)
    uint32_t host_state;             // 1: the state is all in the pinned host tier (PCIe-bound launch shape)
    uint32_t host_span;              // (set by the launcher) bytes of the host extent the kernel may touch
};

// One to kAdamMaxTensors parameters in one launch: blockIdx.y picks the tensor
// (descriptors ride in the kernarg segment), blockIdx.x strides within it.
struct AdamTensor {
    void *p;                         // parameters (this GPU), n elements, fp32 16-byte aligned or bf16 8-byte
    const void *g;                   // gradients (this GPU), like p
    uint64_t n;                      // elements
    uint64_t w_off, m_off, v_off;    // byte offsets of element 0's master weight (bf16 only), exp_avg and
                                     // exp_avg_sq in the state space (16-byte aligned)
};
constexpr int kAdamMaxTensors = 32;
struct AdamMultiArgs {
    AdamArgs c;
    uint32_t count;
    AdamTensor t[kAdamMaxTensors];
};
static_assert(sizeof(AdamMultiArgs) < 4096, "kernarg segment limit");

// ---- launch shape ----
// Which kernel variant runs, and on what grid: a pure function of the tensors, where the
// state lives, the CU count and the knobs, shared by the launcher and the stand-alone
// test program (csrc/tools/ocm_adam_plan_tests.cpp); it calls nothing of HIP.
constexpr int kAdamThreads = 256;    // lanes per workgroup, 4 vectors of 4 elements each per pass

struct AdamKnobs {                   // ocmlib::Config's adam_* fields (defaults and measurements there)
    bool host;                       // host-tier state in one extent takes the PCIe variant
    int host_grid;                   // its workgroups (0: the HBM grid rule)
    int host_vec;                    // its vectors in flight per lane, fp32: 2, 8, anything else 4
    int grid;                        // > 0: this many workgroups per tensor, whatever the rule says
};

struct AdamShape {
    uint32_t gx;                     // workgroups per tensor (grid.x; grid.y is the tensor count); 0: no work
    bool host;                       // the PCIe variant: buffer loads, write-through stores
    uint64_t span;                   // bytes from the extent's base that the vector part reaches
    int kV;                          // vectors in flight per lane
};

inline AdamShape adam_launch_shape(const AdamTensor *t, uint32_t count, bool bf16, bool host_state, uint32_t n_ext,
                                   int cus, const AdamKnobs &k) {
    uint64_t biggest = 0, total = 0, span = 0;
    for (uint32_t i = 0; i < count; i++) {
        biggest = std::max(biggest, t[i].n);
        total += t[i].n;
        const uint64_t bytes = (t[i].n & ~3ull) * 4;  // the tail goes through 64-bit addresses
        span = std::max(span, std::max(t[i].m_off, t[i].v_off) + bytes);
        if (bf16) span = std::max(span, t[i].w_off + bytes);
    }
    if (biggest == 0) return AdamShape{0, false, span, 4};
    // Blocks per tensor (uniform over blockIdx.y): the tuned total of 2 workgroups
    // per CU, shared in proportion to the biggest tensor's part of the work, so
    // equal tensors split it evenly and one big tensor among small ones gets
    // nearly all of it; the extra blocks of small tensors exit at once.
    const uint64_t want = std::max<uint64_t>(1, ((biggest >> 2) + kAdamThreads * 4 - 1) / (kAdamThreads * 4));
    const uint64_t cap = std::max<uint64_t>(1, (uint64_t)((double)cus * 2.0 * (double)biggest / (double)total + 0.999));
    AdamShape s{(uint32_t)std::min(want, cap), false, span, 4};
    // Host-tier state in one extent whose every offset fits 32 bits: the PCIe variant.
    s.host = host_state && k.host && n_ext == 1 && span < (1ull << 32);
    if (s.host && k.host_grid > 0) {
        // the host grid shared like the HBM one: in proportion to the biggest tensor's part
        const uint64_t hg = (uint64_t)((double)k.host_grid * (double)biggest / (double)total + 0.999);
        s.gx = (uint32_t)std::max<uint64_t>(1, std::min(hg, want));
    }
    if (k.grid > 0) s.gx = (uint32_t)k.grid;
    if (s.host && !bf16 && (k.host_vec == 2 || k.host_vec == 8)) s.kV = k.host_vec;
    return s;
}

// torch.optim.Adam's update (L2 weight decay, bias correction), or AdamW's
// (decoupled weight decay) with `decoupled`, one pass over every tensor:
// reads p, g (local) and m, v (remote), writes p (local) and m, v (remote).
// bf16 mode: the update runs on the fp32 master weights (remote) and p gets
// their bf16 rounding (round to nearest even).
hipError_t adam_remote_launch(const AdamMultiArgs &a, const AdamKnobs &knobs, hipStream_t stream);

}  // namespace ocm
