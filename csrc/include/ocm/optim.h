// Fused optimizer kernel that updates parameters in place while their state
// lives in a remote (striped) oncilla allocation: the kernel reads and writes
// the state straight from peer HBM over xGMI (or the pinned host tier), with
// no staging copy. See csrc/src/kernels/optim.hip.
#pragma once

#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstdint>
#include <cstring>

#include "ocm/state_space.h"

namespace ocm {

// What every tensor of a launch shares: the element rule's constants, and where the state lives.
struct AdamHyper {
    float b1, b2, eps, wd;           // betas, eps, L2 weight decay
    float omb1, omb2;                // 1 - b1, 1 - b2: computed in double by the caller, rounded once
    float step_size;                 // lr / (1 - b1^t)
    float inv_sqrt_bc2;              // 1 / sqrt(1 - b2^t)
    uint32_t bf16;                   // 1: p and g are bf16; fp32 master weights at w_off in the state
    uint32_t decoupled;              // 1: AdamW (p *= decay before the step; wd unused)
    float decay;                     // 1 - lr * weight_decay (AdamW)
};
struct AdamArgs {
    StateSpace state;                // exp_avg, exp_avg_sq and (bf16) the master weights
    AdamHyper h;
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

// The gradient source of ocm_x_adam_multi_acc, appended to the launch arguments: fp32
// accumulators in the remote half of a pair of their own (usually not the one that holds
// the moments), a second state space with its own extent table and stripe shift. Element i
// of tensor k is the word at g_off[k] + 4 i; the gradient is gscale * that word, one fp32
// multiply rounded on its own. AdamTensor::g is not read.
#define OCM_ADAM_ACC_ZERO 1u         // store +0.0f over every accumulator word that was read
struct AdamAccArgs {
    StateSpace space;                // the accumulators
    float gscale;
    uint32_t flags;                  // OCM_ADAM_ACC_*
    uint64_t g_off[kAdamMaxTensors]; // byte offset of element 0's accumulator (16-byte aligned), per tensor
};
struct AdamMultiArgs {
    AdamArgs c;
    uint32_t count;
    AdamTensor t[kAdamMaxTensors];
    AdamAccArgs acc;                 // read by the accumulator instantiations only
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

// The same with the gradient read from accumulators (g_off: one offset per tensor; null:
// no accumulator space is involved and the answer is adam_launch_shape's). The PCIe
// variant addresses each space through a buffer resource of its own, so it runs only when
// both spaces are one pinned host-tier extent whose reach fits 32 bits; any mixed
// placement takes the generic variant, on the HBM grid rule.
struct AdamAccShape {
    AdamShape s;
    uint64_t acc_span;               // bytes from the accumulator extent's base that the vector part reaches
};

inline AdamAccShape adam_acc_launch_shape(const AdamTensor *t, const uint64_t *g_off, uint32_t count, bool bf16,
                                          bool host_state, uint32_t n_ext, bool host_acc, uint32_t acc_n_ext, int cus,
                                          const AdamKnobs &k) {
    if (!g_off) return AdamAccShape{adam_launch_shape(t, count, bf16, host_state, n_ext, cus, k), 0};
    uint64_t span = 0;
    for (uint32_t i = 0; i < count; i++) span = std::max<uint64_t>(span, g_off[i] + (t[i].n & ~3ull) * 4);
    const bool acc_fits = host_acc && acc_n_ext == 1 && span < (1ull << 32);
    return AdamAccShape{adam_launch_shape(t, count, bf16, host_state && acc_fits, n_ext, cus, k), span};
}

// ---- the accumulator side of one tensor, checked before any launch ----
// Shared by the host path (csrc/src/lib/optim.cpp) and the stand-alone test program
// (csrc/tools/ocm_adam_acc_tests.cpp). acc_bytes: the gradient allocation's remote half.
// same_alloc: it is the allocation that holds the state, so the accumulators must keep clear
// of this tensor's exp_avg, exp_avg_sq and (bf16) master weights. Every range is tested as
// bytes <= size - offset with n bounded first, so nothing here can overflow.
enum AdamAccBad { ADAM_ACC_OK = 0, ADAM_ACC_ALIGN, ADAM_ACC_RANGE, ADAM_ACC_SCALE, ADAM_ACC_FLAGS, ADAM_ACC_OVERLAP };

inline AdamAccBad adam_acc_check(const AdamTensor &t, uint64_t g_off, uint64_t acc_bytes, float gscale, uint32_t flags,
                                 bool bf16, bool same_alloc) {
    uint32_t bits;
    std::memcpy(&bits, &gscale, 4);
    if ((bits & 0x7f800000u) == 0x7f800000u) return ADAM_ACC_SCALE;
    if (flags & ~OCM_ADAM_ACC_ZERO) return ADAM_ACC_FLAGS;
    if (g_off % 16 != 0) return ADAM_ACC_ALIGN;
    if (t.n > (UINT64_MAX >> 3) || g_off > acc_bytes || 4 * t.n > acc_bytes - g_off) return ADAM_ACC_RANGE;
    if (same_alloc && t.n) {
        // two arrays of the same length overlap when their starts are closer than that length
        const uint64_t bytes = 4 * t.n;
        auto hits = [&](uint64_t off) { return (off > g_off ? off - g_off : g_off - off) < bytes; };
        if (hits(t.m_off) || hits(t.v_off) || (bf16 && hits(t.w_off))) return ADAM_ACC_OVERLAP;
    }
    return ADAM_ACC_OK;
}

inline const char *adam_acc_why(AdamAccBad b) {
    switch (b) {
    case ADAM_ACC_ALIGN: return "accumulator offset is not a multiple of 16";
    case ADAM_ACC_RANGE: return "accumulator range exceeds the gradient allocation's remote half";
    case ADAM_ACC_SCALE: return "gscale is not finite";
    case ADAM_ACC_FLAGS: return "unknown flag bit";
    case ADAM_ACC_OVERLAP: return "accumulator range overlaps the tensor's state";
    case ADAM_ACC_OK: break;
    }
    return "ok";
}

// torch.optim.Adam's update (L2 weight decay, bias correction), or AdamW's
// (decoupled weight decay) with `decoupled`, one pass over every tensor:
// reads p, g (local) and m, v (remote), writes p (local) and m, v (remote).
// bf16 mode: the update runs on the fp32 master weights (remote) and p gets
// their bf16 rounding (round to nearest even).
// from_acc: the gradient is gscale * the fp32 accumulators of a.acc (remote), which the same
// pass zeroes when a.acc.flags has OCM_ADAM_ACC_ZERO; t[].g is not read.
hipError_t adam_remote_launch(const AdamMultiArgs &a, const AdamKnobs &knobs, hipStream_t stream,
                              bool from_acc = false);
// The CU count the launch shapes of the optimizer kernels are made for (256 when it cannot be asked).
int optim_cus();

}  // namespace ocm
