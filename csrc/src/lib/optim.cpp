// Fused Adam over optimizer state kept in the remote half of a pair (ocm/optim.h; hooks,
// not part of the ABI): p/g are this GPU's parameters and gradients (n floats),
// exp_avg / exp_avg_sq of element 0 sit at byte offsets m_off / v_off of the
// remote half. hp = {b1, b2, eps, weight_decay, step_size, 1/sqrt(bias_correction2),
// adamw_decay, 1 - b1, 1 - b2}: adamw_decay = 1 - lr * weight_decay selects AdamW
// (decoupled decay; weight_decay then unused), NaN selects Adam with the L2 term. The two
// complements are the caller's, computed in double from the exact betas like the bias
// corrections: 1.f - float(0.999) is 1.3e-5 short of float(0.001).
// Queued on `stream` (e.g. torch's current stream); no host wait.
// ocm_x_adam_multi_acc takes the gradient from fp32 accumulators in the remote half of a
// second pair instead (ocm/optim.h: AdamAccArgs), scaled, and can zero them in the same pass.
// ocm_x_acc_sumsq reduces such accumulators to their sum of squares and non-finite count
// (ocm/acc_norm.h), from which ocm_x_clip_scale makes that scale for a clipped step.
// ocm_x_adam_rows is the row-sparse step of an embedding table that itself lives in a remote
// half (ocm/adam_rows.h): ids on the GPU pick the rows, nothing else is read or written.
#include <cmath>

#include "internal.h"
#include "ocm/acc_norm.h"
#include "ocm/adam_rows.h"
#include "ocm/optim.h"

using namespace ocm;
using namespace ocmlib;

namespace {

// The start of every hook, after its null checks (lists.h: list_enter): takes the library lock
// into `lk` (held until the caller returns), refuses a handle that is not a live allocation
// before anything of it is read, and fills the state space `xa` of `a` and, unless `b` is null
// (`xb` is then left alone), `xb` of `b`, or says why a kernel here cannot address one (`single`:
// in ocm_x_adam's own words).
int optim_enter(std::unique_lock<std::recursive_mutex> &lk, const char *who, bool single, ocm_alloc_t a, StateSpace *xa,
                ocm_alloc_t b = nullptr, StateSpace *xb = nullptr) {
    State &s = S();
    lk = std::unique_lock<std::recursive_mutex>(s.mu);
    if (!s.allocs.count(a) || (b && !s.allocs.count(b))) OCM_FAIL(-1, "%s: unknown allocation", who);
    if (s.device < 0) OCM_FAIL(-1, "%s needs a GPU", who);
    const std::pair<ocm_alloc_t, StateSpace *> sides[2] = {{a, xa}, {b, xb}};
    for (const auto &[h, x] : sides) {
        if (!h) continue;
        const bool many = h->ext.size() > (size_t)kXferMaxExtents;
        if (!is_pair(h->kind) || h->ext.empty() || !h->all_dev_ok || (many && !single))
            OCM_FAIL(-1, "%s needs a remote half this GPU can address%s", who,
                     single ? " (HBM or host tier, not another node)" : "");
        if (many) OCM_FAIL(-1, "%s: too many extents", who);
        std::memset(x, 0, sizeof(*x));
        if (pair_side(h, 4, x) < 0) {
            if (single) OCM_FAIL(-1, "%s: stripe unit %llu unusable", who, (unsigned long long)h->stripe_unit);
            OCM_FAIL(-1, "%s: stripe unit unusable", who);
        }
        x->host = (!h->any_gpu && !h->any_net) ? 1u : 0u;
    }
    return 0;
}

AdamKnobs adam_knobs(const Config &c) { return AdamKnobs{c.adam_host, c.adam_host_grid, c.adam_host_vec, c.adam_grid}; }

// The end of every hook, under the lock, every check made: queued async ops on the allocations
// come first, then `launch` (which may queue several kernels) on the library's GPU, with the knobs.
template <class Launch>
int optim_launch(const char *who, ocm_alloc_t a, ocm_alloc_t b, Launch launch) {
    if (wait_alloc(a) != 0) return -1;
    if (b && b != a && wait_alloc(b) != 0) return -1;
    DeviceGuard dg(S().device);
    before_launch();
    const hipError_t e = launch(adam_knobs(S().cfg));
    if (e != hipSuccess) OCM_FAIL(-1, "%s launch: %s", who, hipGetErrorString(e));
    return 0;
}

AdamHyper adam_hyper(const float hp[9], bool bf16) {
    AdamHyper h{};
    h.b1 = hp[0];
    h.b2 = hp[1];
    h.eps = hp[2];
    h.wd = hp[3];
    h.step_size = hp[4];
    h.inv_sqrt_bc2 = hp[5];
    h.decoupled = std::isnan(hp[6]) ? 0u : 1u;  // NaN: L2 Adam; else AdamW's weight multiplier
    h.decay = hp[6];
    h.omb1 = hp[7];
    h.omb2 = hp[8];
    h.bf16 = bf16 ? 1u : 0u;
    return h;
}

// n fp32 state elements at byte offset `off` lie inside the remote half.
bool fits(ocm_alloc_t a, uint64_t off, uint64_t n) {
    return n <= (UINT64_MAX >> 3) && off <= a->remote_bytes && 4 * n <= a->remote_bytes - off;
}

// Where the gradient comes from when it is not a local tensor (ocm_x_adam_multi_acc).
struct AdamAccSource {
    ocm_alloc_t grads;
    const uint64_t *g_off;
    float gscale;
    uint32_t flags;
};

// The one path behind the four dense entry points: `count` tensors, kAdamMaxTensors per launch.
// The list entry points (`multi`) name the tensor at fault. `acc`: the gradients are
// accumulators (`g` is then unused). Every tensor is checked before the first launch: a bad
// one never leaves some parameters a step ahead of the others.
int adam_run(const char *who, bool multi, ocm_alloc_t a, int count, void *const *p, const void *const *g,
             const uint64_t *n, const uint64_t *w_off, const uint64_t *m_off, const uint64_t *v_off, const float hp[9],
             bool bf16, void *stream, const AdamAccSource *acc = nullptr) {
    if (!a || count < 0 || (count && (!p || (!acc && !g) || !n || !m_off || !v_off || (bf16 && !w_off))) || !hp ||
        (!multi && (!p[0] || !g[0])) || (acc && (!acc->grads || (count && !acc->g_off))))
        OCM_FAIL(-1, "%s: null argument", who);
    AdamMultiArgs x{};
    std::unique_lock<std::recursive_mutex> lk;
    if (optim_enter(lk, who, !multi, a, &x.c.state, acc ? acc->grads : nullptr, &x.acc.space) != 0) return -1;
    x.c.h = adam_hyper(hp, bf16);
    if (acc) {
        x.acc.gscale = acc->gscale;
        x.acc.flags = acc->flags;
    }
    for (int i = 0; i < count; i++) {
        if (!p[i] || (!acc && !g[i])) OCM_FAIL(-1, "%s: tensor %d has no data", who, i);
        if (!(fits(a, m_off[i], n[i]) && fits(a, v_off[i], n[i]) && (!bf16 || fits(a, w_off[i], n[i])))) {
            if (multi) OCM_FAIL(-1, "%s: tensor %d state range exceeds the remote half", who, i);
            OCM_FAIL(-1, "%s: state range exceeds the remote half (%zu bytes)", who, a->remote_bytes);
        }
        if (!acc) continue;
        const AdamTensor t{p[i], nullptr, n[i], bf16 ? w_off[i] : 0, m_off[i], v_off[i]};
        const AdamAccBad why = adam_acc_check(t, acc->g_off[i], acc->grads->remote_bytes, acc->gscale, acc->flags, bf16,
                                              acc->grads == a);
        if (why != ADAM_ACC_OK) OCM_FAIL(-1, "%s: tensor %d: %s", who, i, adam_acc_why(why));
    }
    return optim_launch(who, a, acc ? acc->grads : nullptr, [&](const AdamKnobs &knobs) {
        hipError_t e = hipSuccess;
        for (int k0 = 0; k0 < count && e == hipSuccess; k0 += kAdamMaxTensors) {
            x.count = (uint32_t)std::min(count - k0, kAdamMaxTensors);
            for (uint32_t j = 0; j < x.count; j++) {
                const int i = k0 + (int)j;
                x.t[j] = AdamTensor{p[i], acc ? nullptr : g[i], n[i], bf16 ? w_off[i] : 0, m_off[i], v_off[i]};
                if (acc) x.acc.g_off[j] = acc->g_off[i];
            }
            e = adam_remote_launch(x, knobs, static_cast<hipStream_t>(stream), acc != nullptr);
        }
        return e;
    });
}

// The sum of squares and the non-finite count of `count` accumulator tensors of `grads`' remote
// half (ocm/acc_norm.h), kAdamMaxTensors per launch pair, the totals formed once by the last
// finishing kernel. Every tensor is checked before the first launch: a refusal writes nothing.
int acc_norm_run(const char *who, ocm_alloc_t grads, int count, const uint64_t *n, const uint64_t *g_off, double *sumsq,
                 uint64_t *nonfinite, void *work, uint64_t work_bytes, void *stream) {
    if (!grads || (count > 0 && (!n || !g_off || !work)) || !sumsq || !nonfinite) OCM_FAIL(-1, "%s: null argument", who);
    AccNormArgs x{};
    std::unique_lock<std::recursive_mutex> lk;
    if (optim_enter(lk, who, false, grads, &x.space) != 0) return -1;
    int at = -1;
    if (const AccNormBad why = acc_norm_check_list(count, n, g_off, grads->remote_bytes, &at)) {
        if (at < 0) OCM_FAIL(-1, "%s: %s", who, acc_norm_why(why));
        OCM_FAIL(-1, "%s: tensor %d: %s", who, at, acc_norm_why(why));
    }
    uint64_t need;
    {
        DeviceGuard dg(S().device);  // optim_cus asks the current device
        need = acc_norm_work_bytes(count, optim_cus(), adam_knobs(S().cfg));
    }
    if (work_bytes < need)
        OCM_FAIL(-1, "%s: workspace of %llu bytes is short of %llu", who, (unsigned long long)work_bytes,
                 (unsigned long long)need);
    x.work = static_cast<AccNormPartial *>(work);
    return optim_launch(who, grads, nullptr, [&](const AdamKnobs &knobs) {
        hipError_t e = hipSuccess;
        int k0 = 0;
        do {  // count == 0: the finishing kernel alone, for the zero totals
            x.count = (uint32_t)std::min(count - k0, kAdamMaxTensors);
            for (uint32_t j = 0; j < x.count; j++) {
                x.n[j] = n[k0 + (int)j];
                x.g_off[j] = g_off[k0 + (int)j];
            }
            AccNormFinishArgs f{};
            f.sumsq = sumsq + k0;
            f.nonfinite = nonfinite + k0;
            k0 += (int)x.count;
            f.totals = k0 >= count ? 1u : 0u;
            f.total_count = (uint32_t)count;
            f.all_sumsq = sumsq;
            f.all_nonfinite = nonfinite;
            e = acc_norm_launch(x, f, work_bytes, knobs, static_cast<hipStream_t>(stream));
        } while (k0 < count && e == hipSuccess);
        return e;
    });
}

// The row-sparse step (ocm/adam_rows.h): the spaces of both pairs are prepared and every check
// is made before the launch, so a refusal writes nothing.
int adam_rows_run(const char *who, ocm_alloc_t table, ocm_alloc_t state, const ocm_adam_rows *d, const void *ids,
                  const void *g, const float hp[9], float gscale, unsigned long long *skipped, void *stream) {
    if (!table || !state || !d || !hp || (d->rows && (!ids || !g))) OCM_FAIL(-1, "%s: null argument", who);
    AdamRowsArgs x{};
    std::unique_lock<std::recursive_mutex> lk;
    if (optim_enter(lk, who, false, state, &x.c.state, table, &x.table) != 0) return -1;
    x.c.h = adam_hyper(hp, d->bf16 != 0);
    char why[256];
    if (adam_rows_check_hp(hp, gscale, why, sizeof(why)) != 0 ||
        adam_rows_check(*d, table->remote_bytes, state->remote_bytes, table == state, why, sizeof(why)) != 0)
        OCM_FAIL(-1, "%s: %s", who, why);
    if (d->rows == 0) return 0;
    x.d = *d;
    x.ids = ids;
    x.g = g;
    x.skipped = skipped;
    x.gscale = gscale;
    return optim_launch(who, table, state,
                        [&](const AdamKnobs &knobs) { return adam_rows_launch(x, knobs, static_cast<hipStream_t>(stream)); });
}

}  // namespace

extern "C" {

// Row-sparse ("lazy") Adam on an embedding table in `table`'s remote half with exp_avg,
// exp_avg_sq and (bf16 tables) fp32 master rows in `state`'s, which may be `table`: the d->rows
// ids at `ids` (device memory) pick the rows, row j of the gradient `g` (device memory, the
// table's dtype) is fl32(gscale * g) of row ids[j]. hp as for ocm_x_adam, with no weight decay of
// either kind. Rows whose id is outside [0, d->table_rows) are left alone and counted up in
// *skipped (a device word, or null). Duplicate ids have no defined result. Queued on `stream`
// behind the async ops queued on both allocations; no host wait.
int ocm_x_adam_rows(ocm_alloc_t table, ocm_alloc_t state, const struct ocm_adam_rows *d, const void *ids, const void *g,
                    const float hp[9], float gscale, unsigned long long *skipped, void *stream) {
    return adam_rows_run("ocm_x_adam_rows", table, state, d, ids, g, hp, gscale, skipped, stream);
}

// The global gradient norm's raw material, computed where the accumulators live: for tensor i
// of n[i] fp32 words at byte offset g_off[i] of `grads`' remote half, sumsq[i] (fp64) and
// nonfinite[i] (words that are inf or NaN), and at index `count` their totals in index order.
// sumsq / nonfinite: count + 1 elements of device memory; work: ocm_x_acc_sumsq_work_bytes(count)
// bytes of device memory, the caller's (two streams never share scratch of the library's).
// Queued on `stream` behind the async ops queued on `grads`; the accumulators are only read.
int ocm_x_acc_sumsq(ocm_alloc_t grads, int count, const uint64_t *n, const uint64_t *g_off, double *sumsq,
                    uint64_t *nonfinite, void *work, uint64_t work_bytes, void *stream) {
    return acc_norm_run("ocm_x_acc_sumsq", grads, count, n, g_off, sumsq, nonfinite, work, work_bytes, stream);
}

// Bytes of workspace a list of `count` tensors needs on this GPU (0: none, or no GPU).
uint64_t ocm_x_acc_sumsq_work_bytes(int count) {
    State &s = S();
    if (s.device < 0 || count <= 0) return 0;
    std::lock_guard<std::recursive_mutex> lk(s.mu);
    DeviceGuard dg(s.device);
    return acc_norm_work_bytes(count, optim_cus(), adam_knobs(s.cfg));
}

// ocm/acc_norm.h's clip_scale: the gscale of a step clipped to max_norm, in double.
double ocm_x_clip_scale(double sumsq_total, double scale, double max_norm) {
    return clip_scale(sumsq_total, scale, max_norm);
}

// One tensor: the count = 1 case of ocm_x_adam_multi, under its own name.
int ocm_x_adam(ocm_alloc_t a, float *p, const float *g, uint64_t n, uint64_t m_off, uint64_t v_off,
               const float hp[9], void *stream) {
    void *const pp = p;
    const void *const gp = g;
    return adam_run("ocm_x_adam", false, a, 1, &pp, &gp, &n, nullptr, &m_off, &v_off, hp, false, stream);
}

// Mixed precision: p / g are bf16 on this GPU, the fp32 master weights sit at
// byte offset w_off of the remote half next to the moments.
int ocm_x_adam_bf16(ocm_alloc_t a, void *p, const void *g, uint64_t n, uint64_t w_off, uint64_t m_off,
                    uint64_t v_off, const float hp[9], void *stream) {
    return adam_run("ocm_x_adam", false, a, 1, &p, &g, &n, &w_off, &m_off, &v_off, hp, true, stream);
}

// Many parameters per launch (32 per kernel, descriptors in the kernarg
// segment): p[i] / g[i] of n[i] elements, state at w_off[i] (bf16 only),
// m_off[i], v_off[i] of the remote half. Same hp as ocm_x_adam.
int ocm_x_adam_multi(ocm_alloc_t a, int count, void *const *p, const void *const *g, const uint64_t *n,
                     const uint64_t *w_off, const uint64_t *m_off, const uint64_t *v_off, const float hp[9],
                     int bf16, void *stream) {
    return adam_run("ocm_x_adam_multi", true, a, count, p, g, n, w_off, m_off, v_off, hp, bf16 != 0, stream);
}

// The same with every gradient read from the fp32 accumulators of `grads`' remote half
// (tensor i's at byte offset g_off[i]) as gscale * acc, one fp32 multiply rounded on its own;
// flags & OCM_ADAM_ACC_ZERO stores +0 over the accumulators in the same pass. `grads` may be
// `state` itself when the ranges keep clear of each other.
int ocm_x_adam_multi_acc(ocm_alloc_t state, ocm_alloc_t grads, int count, void *const *p, const uint64_t *n,
                         const uint64_t *w_off, const uint64_t *m_off, const uint64_t *v_off, const uint64_t *g_off,
                         const float hp[9], float gscale, uint32_t flags, int bf16, void *stream) {
    const AdamAccSource acc{grads, g_off, gscale, flags};
    return adam_run("ocm_x_adam_multi_acc", true, state, count, p, nullptr, n, w_off, m_off, v_off, hp, bf16 != 0,
                    stream, &acc);
}

}  // extern "C"
