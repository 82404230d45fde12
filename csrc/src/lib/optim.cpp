// Fused Adam over optimizer state kept in the remote half of a pair (ocm/optim.h; hooks,
// not part of the ABI): p/g are this GPU's parameters and gradients (n floats),
// exp_avg / exp_avg_sq of element 0 sit at byte offsets m_off / v_off of the
// remote half. hp = {b1, b2, eps, weight_decay, step_size, 1/sqrt(bias_correction2),
// adamw_decay, 1 - b1, 1 - b2}: adamw_decay = 1 - lr * weight_decay selects AdamW
// (decoupled decay; weight_decay then unused), NaN selects Adam with the L2 term. The two
// complements are the caller's, computed in double from the exact betas like the bias
// corrections: 1.f - float(0.999) is 1.3e-5 short of float(0.001).
// Queued on `stream` (e.g. torch's current stream); no host wait.
#include <cmath>

#include "internal.h"
#include "ocm/optim.h"

using namespace ocm;
using namespace ocmlib;

namespace {

// What both entry points do before they launch: check that a kernel on this GPU can
// address the pair's remote half, and fill the fields every launch shares (the extent
// table and stripe shift, the hyper-parameters, where the state lives). The callers
// word the errors, under their own names.
enum AdamBad { ADAM_OK = 0, ADAM_NO_GPU, ADAM_NO_PAIR, ADAM_EXTENTS, ADAM_STRIPE };

AdamBad adam_prepare(ocm_alloc_t a, const float hp[9], bool bf16, AdamArgs *x) {
    if (S().device < 0) return ADAM_NO_GPU;
    if (!is_pair(a->kind) || a->ext.empty() || !a->all_dev_ok) return ADAM_NO_PAIR;
    if (a->ext.size() > (size_t)kXferMaxExtents) return ADAM_EXTENTS;
    std::memset(x, 0, sizeof(*x));
    if (pair_side(a, 4, x) < 0) return ADAM_STRIPE;
    x->b1 = hp[0];
    x->b2 = hp[1];
    x->eps = hp[2];
    x->wd = hp[3];
    x->step_size = hp[4];
    x->inv_sqrt_bc2 = hp[5];
    x->decoupled = std::isnan(hp[6]) ? 0u : 1u;  // NaN: L2 Adam; else AdamW's weight multiplier
    x->decay = hp[6];
    x->omb1 = hp[7];
    x->omb2 = hp[8];
    x->host_state = (!a->any_gpu && !a->any_net) ? 1u : 0u;
    x->bf16 = bf16 ? 1u : 0u;
    return ADAM_OK;
}

// n fp32 state elements at byte offset `off` lie inside the remote half.
bool fits(ocm_alloc_t a, uint64_t off, uint64_t n) {
    return n <= (UINT64_MAX >> 3) && off <= a->remote_bytes && 4 * n <= a->remote_bytes - off;
}

int adam_common(ocm_alloc_t a, void *p, const void *g, uint64_t n, uint64_t w_off, uint64_t m_off, uint64_t v_off,
                const float hp[9], void *stream, bool bf16) {
    State &s = S();
    if (!a || !p || !g || !hp) OCM_FAIL(-1, "ocm_x_adam: null argument");
    AdamArgs x;
    switch (adam_prepare(a, hp, bf16, &x)) {
    case ADAM_NO_GPU: OCM_FAIL(-1, "ocm_x_adam needs a GPU");
    case ADAM_NO_PAIR:
        OCM_FAIL(-1, "ocm_x_adam needs a remote half this GPU can address (HBM or host tier, not another node)");
    case ADAM_EXTENTS: OCM_FAIL(-1, "ocm_x_adam: too many extents");
    case ADAM_STRIPE: OCM_FAIL(-1, "ocm_x_adam: stripe unit %llu unusable", (unsigned long long)a->stripe_unit);
    case ADAM_OK: break;
    }
    if (!fits(a, m_off, n) || !fits(a, v_off, n) || (bf16 && !fits(a, w_off, n)))
        OCM_FAIL(-1, "ocm_x_adam: state range exceeds the remote half (%zu bytes)", a->remote_bytes);
    x.p = static_cast<float *>(p);
    x.g = static_cast<const float *>(g);
    x.w_off = w_off;
    x.m_off = m_off;
    x.v_off = v_off;
    x.n = n;
    std::lock_guard<std::recursive_mutex> lk(s.mu);
    if (wait_alloc(a) != 0) return -1;  // queued async ops on this allocation come first
    DeviceGuard dg(s.device);
    before_launch();
    const hipError_t e = adam_remote_launch(x, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) OCM_FAIL(-1, "ocm_x_adam launch: %s", hipGetErrorString(e));
    return 0;
}

}  // namespace

extern "C" {

int ocm_x_adam(ocm_alloc_t a, float *p, const float *g, uint64_t n, uint64_t m_off, uint64_t v_off,
               const float hp[9], void *stream) {
    return adam_common(a, p, g, n, 0, m_off, v_off, hp, stream, false);
}

// Mixed precision: p / g are bf16 on this GPU, the fp32 master weights sit at
// byte offset w_off of the remote half next to the moments.
int ocm_x_adam_bf16(ocm_alloc_t a, void *p, const void *g, uint64_t n, uint64_t w_off, uint64_t m_off,
                    uint64_t v_off, const float hp[9], void *stream) {
    return adam_common(a, p, g, n, w_off, m_off, v_off, hp, stream, true);
}

// Many parameters per launch (32 per kernel, descriptors in the kernarg
// segment): p[i] / g[i] of n[i] elements, state at w_off[i] (bf16 only),
// m_off[i], v_off[i] of the remote half. Same hp as ocm_x_adam.
int ocm_x_adam_multi(ocm_alloc_t a, int count, void *const *p, const void *const *g, const uint64_t *n,
                     const uint64_t *w_off, const uint64_t *m_off, const uint64_t *v_off, const float hp[9],
                     int bf16, void *stream) {
    State &s = S();
    if (!a || count < 0 || (count && (!p || !g || !n || !m_off || !v_off || (bf16 && !w_off))) || !hp)
        OCM_FAIL(-1, "ocm_x_adam_multi: null argument");
    AdamMultiArgs x;
    std::memset(&x, 0, sizeof(x));
    switch (adam_prepare(a, hp, bf16 != 0, &x.c)) {
    case ADAM_NO_GPU: OCM_FAIL(-1, "ocm_x_adam_multi needs a GPU");
    case ADAM_NO_PAIR:
    case ADAM_EXTENTS: OCM_FAIL(-1, "ocm_x_adam_multi needs a remote half this GPU can address");
    case ADAM_STRIPE: OCM_FAIL(-1, "ocm_x_adam_multi: stripe unit unusable");
    case ADAM_OK: break;
    }
    // Every tensor is checked before the first launch: a bad one never leaves
    // some parameters a step ahead of the others.
    for (int i = 0; i < count; i++) {
        if (!p[i] || !g[i]) OCM_FAIL(-1, "ocm_x_adam_multi: tensor %d has no data", i);
        if (!fits(a, m_off[i], n[i]) || !fits(a, v_off[i], n[i]) || (bf16 && !fits(a, w_off[i], n[i])))
            OCM_FAIL(-1, "ocm_x_adam_multi: tensor %d state range exceeds the remote half", i);
    }
    std::lock_guard<std::recursive_mutex> lk(s.mu);
    if (wait_alloc(a) != 0) return -1;
    DeviceGuard dg(s.device);
    before_launch();
    for (int k0 = 0; k0 < count; k0 += kAdamMaxTensors) {
        x.count = (uint32_t)std::min(count - k0, kAdamMaxTensors);
        for (uint32_t j = 0; j < x.count; j++) {
            const int i = k0 + (int)j;
            x.t[j] = AdamTensor{p[i], g[i], n[i], bf16 ? w_off[i] : 0, m_off[i], v_off[i]};
        }
        const hipError_t e = adam_remote_multi_launch(x, static_cast<hipStream_t>(stream));
        if (e != hipSuccess) OCM_FAIL(-1, "ocm_x_adam_multi launch: %s", hipGetErrorString(e));
    }
    return 0;
}

}  // extern "C"
