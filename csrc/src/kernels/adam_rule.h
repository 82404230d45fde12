// The Adam element rule and what goes with it, shared by the dense kernel (optim.hip) and
// the row-sparse one (optim_rows.hip): the project keeps one rule.
#pragma once
#include <hip/hip_runtime.h>

#include "ocm/optim.h"

namespace ocm {

__device__ __forceinline__ float adam1(float &p, float g, float &m, float &v, const AdamHyper &a) {
    if (a.decoupled)
        p = p * a.decay;  // AdamW: p *= 1 - lr * weight_decay, gradient untouched
    else if (a.wd != 0.f)
        g = g + a.wd * p;  // Adam: L2 term in the gradient
    // omb1 / omb2: 1 - beta rounded once from double on the host. Subtracting the
    // already rounded fp32 beta here loses 1.3e-5 of 1 - 0.999 (1.7e-4 of 1 - 0.9999).
    m = m + a.omb1 * (g - m);  // torch: exp_avg.lerp_(grad, 1 - beta1)
    v = a.b2 * v + a.omb2 * g * g;
    const float denom = sqrtf(v) * a.inv_sqrt_bc2 + a.eps;
    p = p - a.step_size * (m / denom);
    return p;
}

// The accumulator gradient: one IEEE fp32 multiply, rounded on its own. Contraction is off
// here whatever -ffp-contract says, so the product never fuses with adam1's g - m or
// g + wd * p (an fma would round once; gscale == 1 must give acc's bits).
__device__ __forceinline__ float acc_grad(float gscale, float acc) {
#pragma clang fp contract(off)
    return gscale * acc;
}

// ---- mixed precision: bf16 parameters and gradients here, fp32 master
// weights and moments in the remote half. Local footprint 4 bytes/parameter
// (bf16 p + g), remote 12; one pass updates the master, the moments and the
// bf16 copy (round to nearest even, like torch's .to(torch.bfloat16)).
typedef unsigned short u16x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float bf16_to_f32(unsigned short h) { return __uint_as_float((unsigned)h << 16); }

__device__ __forceinline__ unsigned short f32_to_bf16(float f) {
    unsigned u = __float_as_uint(f);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (unsigned short)((u >> 16) | 0x40u);  // quiet NaN
    u += 0x7fffu + ((u >> 16) & 1u);
    return (unsigned short)(u >> 16);
}

}  // namespace ocm
