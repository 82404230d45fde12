// Global gradient norm over fp32 accumulators where they live: the remote half of a pair
// (ocm/optim.h: the accumulators ocm_x_adam_multi_acc reads). One read-only pass yields, per
// tensor, the sum of squares and the number of non-finite words; the host turns the total into
// the gscale of the fused Adam (clip_scale). See csrc/src/kernels/acc_norm.hip.
//
// The rule, for tensor i with n[i] words at byte offset g_off[i]:
//   sumsq[i]     = sum over j of (double)acc[j] * (double)acc[j], accumulated in fp64. The
//                  product of two fp32 values is exact in fp64 (48 significant bits), cannot
//                  overflow (FLT_MAX^2 ~ 1.2e77) and cannot go subnormal ((2^-149)^2 = 2^-298),
//                  so the only rounding is in the additions of non-negative terms: any order
//                  of them is within (n - 1) * 2^-53 relative of the exact sum.
//   nonfinite[i] = the number of words with (bits & 0x7f800000) == 0x7f800000, exact.
//   index count  = the sum of sumsq[0 .. count) in index order, and the sum of the counts.
// The order of the additions is a function of the tensor list and the launch shape only (no
// floating-point atomics), so two runs over the same data give the same bits.
//
// This header is what the kernel, the host path (csrc/src/lib/optim.cpp) and the stand-alone
// test program (csrc/tools/ocm_acc_norm_tests.cpp) share; what it adds to ocm/optim.h calls
// nothing of HIP.
#pragma once

#include <cmath>
#include <cstdint>
#include <cstring>

#include "ocm/optim.h"

namespace ocm {

// What one workgroup leaves for the finishing kernel, and what that kernel adds up.
struct AccNormPartial {
    double sumsq;
    uint64_t nonfinite;
};
static_assert(sizeof(AccNormPartial) == 16, "one 16-byte store per workgroup");

// One launch: up to kAdamMaxTensors tensors, blockIdx.y picks one (descriptors in the kernarg
// segment, as AdamMultiArgs).
struct AccNormArgs {
    StateSpace space;                // the accumulators
    uint32_t count;
    AccNormPartial *work;            // count * gridDim.x partials, tensor-major (device memory)
    uint64_t n[kAdamMaxTensors];     // words
    uint64_t g_off[kAdamMaxTensors]; // byte offset of word 0 (16-byte aligned)
};
static_assert(sizeof(AccNormArgs) < 4096, "kernarg segment limit");

// The finishing kernel's: partials of `count` tensors, gx each, into sumsq / nonfinite (this
// launch's first tensor); with `totals`, then the sums over all_sumsq / all_nonfinite[0 .. total_count)
// in index order into their element total_count.
struct AccNormFinishArgs {
    const AccNormPartial *work;
    uint32_t count, gx;
    double *sumsq;
    uint64_t *nonfinite;
    uint32_t totals, total_count;
    double *all_sumsq;
    uint64_t *all_nonfinite;
};

// ---- the element rule ----
OCM_LIST_HD inline bool acc_norm_nonfinite(uint32_t bits) { return (bits & 0x7f800000u) == 0x7f800000u; }

// ---- one tensor, checked before any launch ----
// acc_bytes: the allocation's remote half. n is bounded first and the range tested as
// bytes <= size - offset (adam_acc_check's way), so nothing here can overflow.
enum AccNormBad { ACC_NORM_OK = 0, ACC_NORM_COUNT, ACC_NORM_ALIGN, ACC_NORM_RANGE };

inline AccNormBad acc_norm_check(uint64_t n, uint64_t g_off, uint64_t acc_bytes) {
    if (g_off % 16 != 0) return ACC_NORM_ALIGN;
    if (n > (UINT64_MAX >> 3) || g_off > acc_bytes || 4 * n > acc_bytes - g_off) return ACC_NORM_RANGE;
    return ACC_NORM_OK;
}
// The whole list: a negative count, or the first tensor at fault (*at).
inline AccNormBad acc_norm_check_list(int count, const uint64_t *n, const uint64_t *g_off, uint64_t acc_bytes, int *at) {
    *at = -1;
    if (count < 0) return ACC_NORM_COUNT;
    for (int i = 0; i < count; i++)
        if (const AccNormBad bad = acc_norm_check(n[i], g_off[i], acc_bytes)) {
            *at = i;
            return bad;
        }
    return ACC_NORM_OK;
}

inline const char *acc_norm_why(AccNormBad b) {
    switch (b) {
    case ACC_NORM_COUNT: return "negative tensor count";
    case ACC_NORM_ALIGN: return adam_acc_why(ADAM_ACC_ALIGN);
    case ACC_NORM_RANGE: return adam_acc_why(ADAM_ACC_RANGE);
    case ACC_NORM_OK: break;
    }
    return "ok";
}

// ---- launch shape ----
// The fused Adam's (adam_launch_shape: the proportional split, the host grid, AdamKnobs'
// host / host_grid / grid) over one space: the buffer-resource variant on the host grid only
// when the accumulators are one pinned host-tier extent whose reach fits 32 bits.
struct AccNormShape {
    uint32_t gx;                     // workgroups per tensor (grid.y: the tensor count); 0: nothing to read
    bool host;
    uint64_t span;                   // bytes from the extent's base that the vector part reaches
};

inline AccNormShape acc_norm_launch_shape(const uint64_t *n, const uint64_t *g_off, uint32_t count, bool host_acc,
                                          uint32_t n_ext, int cus, const AdamKnobs &k) {
    AdamTensor t[kAdamMaxTensors];
    if (count > (uint32_t)kAdamMaxTensors) count = kAdamMaxTensors;
    for (uint32_t i = 0; i < count; i++) t[i] = AdamTensor{nullptr, nullptr, n[i], 0, g_off[i], g_off[i]};
    const AdamShape s = adam_launch_shape(t, count, false, host_acc, n_ext, cus, k);
    return AccNormShape{s.gx, s.host, s.span};
}

// The most workgroups per tensor any list can get: what the caller's workspace is sized for.
inline uint32_t acc_norm_max_gx(int cus, const AdamKnobs &k) {
    if (k.grid > 0) return (uint32_t)k.grid;
    return (uint32_t)std::max(1, std::max(2 * cus, k.host_grid));
}
inline uint64_t acc_norm_work_bytes(int count, int cus, const AdamKnobs &k) {
    if (count <= 0) return 0;  // an empty list has no partials
    const uint64_t per_launch = (uint64_t)std::min(count, kAdamMaxTensors);
    return per_launch * acc_norm_max_gx(cus, k) * sizeof(AccNormPartial);
}

// ---- clipping ----
// torch.nn.utils.clip_grad_norm_'s rule in double: the gradient is scale * acc, its norm
// |scale| * sqrt(sumsq_total), the coefficient min(1, max_norm / (norm + 1e-6)). Returns
// scale * coefficient, which the caller rounds to fp32 once, where it becomes gscale. A NaN
// norm gives NaN, as torch's clamp does (the fused Adam then refuses the step).
inline double clip_scale(double sumsq_total, double scale, double max_norm) {
    const double norm = std::fabs(scale) * std::sqrt(sumsq_total);
    const double ratio = max_norm / (norm + 1e-6);
    const double coef = ratio < 1.0 ? ratio : (ratio != ratio ? ratio : 1.0);
    return scale * coef;
}

// ---- a plain C++ reference of the reduction ----
// One tensor, words in index order.
inline void acc_norm_reference(const float *acc, uint64_t n, double *sumsq, uint64_t *nonfinite) {
    double s = 0.0;
    uint64_t bad = 0;
    for (uint64_t j = 0; j < n; j++) {
        uint32_t bits;
        std::memcpy(&bits, &acc[j], 4);
        s += (double)acc[j] * (double)acc[j];
        bad += acc_norm_nonfinite(bits) ? 1u : 0u;
    }
    *sumsq = s;
    *nonfinite = bad;
}
// The totals at index count, from sumsq / nonfinite[0 .. count) in index order.
inline void acc_norm_totals(double *sumsq, uint64_t *nonfinite, uint32_t count) {
    double s = 0.0;
    uint64_t bad = 0;
    for (uint32_t i = 0; i < count; i++) {
        s += sumsq[i];
        bad += nonfinite[i];
    }
    sumsq[count] = s;
    nonfinite[count] = bad;
}

// Queues the reduction of one launch's tensors (a.count <= kAdamMaxTensors) and its finishing
// kernel on `stream`; `f` names the outputs (f.work, f.count and f.gx are set here). work_bytes:
// what a.work holds. Defined in csrc/src/kernels/acc_norm.hip.
hipError_t acc_norm_launch(const AccNormArgs &a, AccNormFinishArgs f, uint64_t work_bytes, const AdamKnobs &knobs,
                           hipStream_t stream);

}  // namespace ocm
