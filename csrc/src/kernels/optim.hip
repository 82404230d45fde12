// gfx950 fused Adam over remote optimizer state (see ocm/optim.h): one kernel,
// adam_multi_kernel, for one to kAdamMaxTensors parameters per launch.
//
// Each lane owns 4 consecutive elements: 16-byte loads of p and g from local
// HBM and of exp_avg / exp_avg_sq from the state's extents (peer HBM over
// xGMI, or pinned host memory over PCIe), the update in registers, 16-byte
// stores back. A 16-byte vector never crosses a stripe unit (units are powers
// of two >= 16 and the offsets are 16-byte aligned), so the extent math runs
// once per vector. Lanes keep kV (4) vectors in flight before the first use,
// which covers the xGMI round trip. The tail (n % 4) is done by lane 0 of
// the tensor's last workgroup, element by element.
//
// kAcc: the gradient is not a local tensor but gscale * fp32 accumulators in a second
// remote space (AdamAccArgs), loaded in the same first loop with the same kV vectors in
// flight and, with OCM_ADAM_ACC_ZERO, overwritten with +0 beside the moment stores.
#include <hip/hip_runtime.h>

#include "adam_rule.h"
#include "ocm/optim.h"
#include "state_space.h"

namespace ocm {

namespace {

constexpr int kThreads = kAdamThreads;

// state_ptr (state_space.h): where byte x of a state space lies, the moments' and master
// weights' or the gradient accumulators', each with its own extent table and stripe shift.
// adam1, acc_grad, bf16_to_f32, f32_to_bf16 (adam_rule.h): the element rule, shared with optim_rows.hip.

// One launch for up to kAdamMaxTensors parameters (see AdamMultiArgs).
// kHost: the state is one pinned host-tier extent whose offsets fit 32 bits: host_ld / host_st
// (state_space.h) on a grid of its own (adam_launch_shape), as PCIe reads want fewer streams than
// HBM. With kAcc the accumulators are such an extent too, behind a buffer resource of their own.
template <bool kBf16, bool kHost, int kV = 4, bool kAcc = false>
__global__ __launch_bounds__(kThreads) void adam_multi_kernel(AdamMultiArgs a) {
    const AdamTensor &T = a.t[blockIdx.y];  // uniform: scalar loads from the kernarg segment
    const StateSpace &c = a.c.state, &ga = a.acc.space;
    const AdamHyper &h = a.c.h;
    const uint64_t g_off = kAcc ? a.acc.g_off[blockIdx.y] : 0;
    const bool zero = kAcc && (a.acc.flags & OCM_ADAM_ACC_ZERO);
    const uint64_t nvec = T.n >> 2;
    const uint64_t lanes = (uint64_t)gridDim.x * kThreads;
    const uint64_t tid = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
    __amdgpu_buffer_rsrc_t rs, grs;
    if constexpr (kHost) rs = host_rsrc(c);
    if constexpr (kHost && kAcc) grs = host_rsrc(ga);
    for (uint64_t base = tid; base < nvec; base += lanes * kV) {
        f32x4 w[kV], m[kV], v[kV], g[kV];
        f32x4 *wp[kV], *mp[kV], *vp[kV], *gp[kV];
#pragma unroll
        for (int k = 0; k < kV; k++) {
            const uint64_t i = base + (uint64_t)k * lanes;
            if (i < nvec) {
                if constexpr (kHost) {
                    m[k] = host_ld(rs, T.m_off + (i << 4));
                    v[k] = host_ld(rs, T.v_off + (i << 4));
                    if constexpr (kAcc) g[k] = host_ld(grs, g_off + (i << 4));
                } else {
                    mp[k] = reinterpret_cast<f32x4 *>(state_ptr(c, T.m_off + (i << 4)));
                    vp[k] = reinterpret_cast<f32x4 *>(state_ptr(c, T.v_off + (i << 4)));
                    m[k] = __builtin_nontemporal_load(mp[k]);
                    v[k] = __builtin_nontemporal_load(vp[k]);
                    if constexpr (kAcc) {
                        gp[k] = reinterpret_cast<f32x4 *>(state_ptr(ga, g_off + (i << 4)));
                        g[k] = __builtin_nontemporal_load(gp[k]);
                    }
                }
                if constexpr (kBf16) {
                    if constexpr (kHost) {
                        w[k] = host_ld(rs, T.w_off + (i << 4));
                    } else {
                        wp[k] = reinterpret_cast<f32x4 *>(state_ptr(c, T.w_off + (i << 4)));
                        w[k] = __builtin_nontemporal_load(wp[k]);
                    }
                    if constexpr (!kAcc) {
                        const u16x4 gh = __builtin_nontemporal_load(reinterpret_cast<const u16x4 *>(T.g) + i);
#pragma unroll
                        for (int j = 0; j < 4; j++) g[k][j] = bf16_to_f32(gh[j]);
                    }
                } else {
                    w[k] = reinterpret_cast<const f32x4 *>(T.p)[i];
                    if constexpr (!kAcc) g[k] = __builtin_nontemporal_load(reinterpret_cast<const f32x4 *>(T.g) + i);
                }
            }
        }
#pragma unroll
        for (int k = 0; k < kV; k++) {
            const uint64_t i = base + (uint64_t)k * lanes;
            if (i < nvec) {
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    float wj = w[k][j], mj = m[k][j], vj = v[k][j];
                    adam1(wj, kAcc ? acc_grad(a.acc.gscale, g[k][j]) : g[k][j], mj, vj, h);
                    w[k][j] = wj;
                    m[k][j] = mj;
                    v[k][j] = vj;
                }
                if constexpr (kBf16) {
                    u16x4 out;
#pragma unroll
                    for (int j = 0; j < 4; j++) out[j] = f32_to_bf16(w[k][j]);
                    reinterpret_cast<u16x4 *>(T.p)[i] = out;
                    if constexpr (kHost)
                        host_st(rs, T.w_off + (i << 4), w[k]);
                    else
                        __builtin_nontemporal_store(w[k], wp[k]);
                } else {
                    reinterpret_cast<f32x4 *>(T.p)[i] = w[k];
                }
                if constexpr (kHost) {
                    host_st(rs, T.m_off + (i << 4), m[k]);
                    host_st(rs, T.v_off + (i << 4), v[k]);
                    if constexpr (kAcc)
                        if (zero) host_st(grs, g_off + (i << 4), f32x4{0.f, 0.f, 0.f, 0.f});
                } else {
                    __builtin_nontemporal_store(m[k], mp[k]);
                    __builtin_nontemporal_store(v[k], vp[k]);
                    if constexpr (kAcc)
                        if (zero) __builtin_nontemporal_store(f32x4{0.f, 0.f, 0.f, 0.f}, gp[k]);
                }
            }
        }
    }
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) {
        for (uint64_t i = nvec << 2; i < T.n; i++) {
            float *mq = reinterpret_cast<float *>(state_ptr(c, T.m_off + 4 * i));
            float *vq = reinterpret_cast<float *>(state_ptr(c, T.v_off + 4 * i));
            float mj = *mq, vj = *vq, wj, gj;
            if constexpr (kBf16)
                wj = *reinterpret_cast<float *>(state_ptr(c, T.w_off + 4 * i));
            else
                wj = static_cast<float *>(T.p)[i];
            if constexpr (kAcc) {
                float *gq = reinterpret_cast<float *>(state_ptr(ga, g_off + 4 * i));
                gj = acc_grad(a.acc.gscale, *gq);
                if (zero) *gq = 0.f;
            } else if constexpr (kBf16) {
                gj = bf16_to_f32(static_cast<const unsigned short *>(T.g)[i]);
            } else {
                gj = static_cast<const float *>(T.g)[i];
            }
            adam1(wj, gj, mj, vj, h);
            *mq = mj;
            *vq = vj;
            if constexpr (kBf16) {
                *reinterpret_cast<float *>(state_ptr(c, T.w_off + 4 * i)) = wj;
                static_cast<unsigned short *>(T.p)[i] = f32_to_bf16(wj);
            } else {
                static_cast<float *>(T.p)[i] = wj;
            }
        }
    }
}

// The instantiation for a shape: every variant has a twin that reads accumulators.
template <bool kAcc>
auto adam_kernel_for(bool bf16, const AdamShape &s) -> void (*)(AdamMultiArgs) {
    if (bf16) return s.host ? adam_multi_kernel<true, true, 4, kAcc> : adam_multi_kernel<true, false, 4, kAcc>;
    if (!s.host) return adam_multi_kernel<false, false, 4, kAcc>;
    return s.kV == 2   ? adam_multi_kernel<false, true, 2, kAcc>
           : s.kV == 8 ? adam_multi_kernel<false, true, 8, kAcc>
                       : adam_multi_kernel<false, true, 4, kAcc>;
}

}  // namespace

int optim_cus() {
    int dev = 0, cus = 256;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0)
        cus = 256;
    return cus;
}

hipError_t adam_remote_launch(const AdamMultiArgs &a, const AdamKnobs &knobs, hipStream_t stream, bool from_acc) {
    const StateSpace &state = a.c.state, &accs = a.acc.space;
    const bool bf16 = a.c.h.bf16 != 0;
    if (a.count == 0) return hipSuccess;
    if (a.count > (uint32_t)kAdamMaxTensors) return hipErrorInvalidValue;
    if (!state_space_ok(state) || (from_acc && !state_space_ok(accs))) return hipErrorInvalidValue;
    for (uint32_t k = 0; k < a.count; k++) {
        const AdamTensor &t = a.t[k];
        const uintptr_t pal = bf16 ? 7u : 15u;
        const uintptr_t g = from_acc ? (uintptr_t)a.acc.g_off[k] & 15u : (uintptr_t)t.g & pal;
        if (((uintptr_t)t.p & pal) || g || ((t.m_off | t.v_off | (bf16 ? t.w_off : 0)) & 15u))
            return hipErrorInvalidValue;
    }
    const AdamAccShape as = adam_acc_launch_shape(a.t, from_acc ? a.acc.g_off : nullptr, a.count, bf16, state.host,
                                                  state.n_ext, accs.host, accs.n_ext, optim_cus(), knobs);
    const AdamShape &s = as.s;
    if (s.gx == 0) return hipSuccess;
    void (*kernel)(AdamMultiArgs) = from_acc ? adam_kernel_for<true>(bf16, s) : adam_kernel_for<false>(bf16, s);
    return state_launch(kernel, dim3(s.gx, a.count), stream, a, s.host, [&](AdamMultiArgs &x) {
        x.c.state.host_span = (uint32_t)s.span;
        x.acc.space.host_span = (uint32_t)as.acc_span;
    });
}

}  // namespace ocm
