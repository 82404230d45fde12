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

// Before any launch: check that a kernel on this GPU can address the pair's remote
// half, and fill the fields every launch shares (the extent table and stripe shift,
// the hyper-parameters, where the state lives). adam_run words the errors.
enum AdamBad { ADAM_OK = 0, ADAM_NO_GPU, ADAM_NO_PAIR, ADAM_EXTENTS, ADAM_STRIPE };

// One state space (the moments' pair or the accumulators'): Space is AdamArgs or AdamAccArgs.
template <class Space>
AdamBad adam_space(ocm_alloc_t a, Space *x) {
    if (S().device < 0) return ADAM_NO_GPU;
    if (!is_pair(a->kind) || a->ext.empty() || !a->all_dev_ok) return ADAM_NO_PAIR;
    if (a->ext.size() > (size_t)kXferMaxExtents) return ADAM_EXTENTS;
    std::memset(x, 0, sizeof(*x));
    if (pair_side(a, 4, x) < 0) return ADAM_STRIPE;
    return ADAM_OK;
}

bool host_tier(ocm_alloc_t a) { return !a->any_gpu && !a->any_net; }

AdamBad adam_prepare(ocm_alloc_t a, const float hp[9], bool bf16, AdamArgs *x) {
    if (const AdamBad bad = adam_space(a, x)) return bad;
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
    x->host_state = host_tier(a) ? 1u : 0u;
    x->bf16 = bf16 ? 1u : 0u;
    return ADAM_OK;
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

// The one path behind the four entry points: `count` tensors, kAdamMaxTensors per launch.
// `who` names the caller in the messages; the list entry points (`multi`) word some of them
// their own way and name the tensor at fault. `acc`: the gradients are accumulators (`g` is
// then unused). Every tensor is checked before the first launch: a bad one never leaves
// some parameters a step ahead of the others.
int adam_run(const char *who, bool multi, ocm_alloc_t a, int count, void *const *p, const void *const *g,
             const uint64_t *n, const uint64_t *w_off, const uint64_t *m_off, const uint64_t *v_off, const float hp[9],
             bool bf16, void *stream, const AdamAccSource *acc = nullptr) {
    State &s = S();
    if (!a || count < 0 || (count && (!p || (!acc && !g) || !n || !m_off || !v_off || (bf16 && !w_off))) || !hp ||
        (!multi && (!p[0] || !g[0])) || (acc && (!acc->grads || (count && !acc->g_off))))
        OCM_FAIL(-1, "%s: null argument", who);
    AdamMultiArgs x;
    std::memset(&x, 0, sizeof(x));
    const char *const which = multi ? "" : " (HBM or host tier, not another node)";
    AdamBad bad = adam_prepare(a, hp, bf16, &x.c);
    if (bad == ADAM_OK && acc) {  // the same checks, the same wording, for the gradient allocation
        bad = adam_space(acc->grads, &x.acc);
        x.acc.gscale = acc->gscale;
        x.acc.flags = acc->flags;
        x.acc.host_acc = host_tier(acc->grads) ? 1u : 0u;
    }
    switch (bad) {
    case ADAM_NO_GPU: OCM_FAIL(-1, "%s needs a GPU", who);
    case ADAM_EXTENTS:
        if (!multi) OCM_FAIL(-1, "%s: too many extents", who);
        [[fallthrough]];
    case ADAM_NO_PAIR: OCM_FAIL(-1, "%s needs a remote half this GPU can address%s", who, which);
    case ADAM_STRIPE:
        if (multi) OCM_FAIL(-1, "%s: stripe unit unusable", who);
        OCM_FAIL(-1, "%s: stripe unit %llu unusable", who, (unsigned long long)a->stripe_unit);
    case ADAM_OK: break;
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
    std::lock_guard<std::recursive_mutex> lk(s.mu);
    const AdamKnobs knobs{s.cfg.adam_host, s.cfg.adam_host_grid, s.cfg.adam_host_vec, s.cfg.adam_grid};
    if (wait_alloc(a) != 0) return -1;  // queued async ops on this allocation come first
    if (acc && acc->grads != a && wait_alloc(acc->grads) != 0) return -1;  // the accumulates, for one
    DeviceGuard dg(s.device);
    before_launch();
    for (int k0 = 0; k0 < count; k0 += kAdamMaxTensors) {
        x.count = (uint32_t)std::min(count - k0, kAdamMaxTensors);
        for (uint32_t j = 0; j < x.count; j++) {
            const int i = k0 + (int)j;
            x.t[j] = AdamTensor{p[i], acc ? nullptr : g[i], n[i], bf16 ? w_off[i] : 0, m_off[i], v_off[i]};
            if (acc) x.acc.g_off[j] = acc->g_off[i];
        }
        const hipError_t e = adam_remote_launch(x, knobs, static_cast<hipStream_t>(stream), acc != nullptr);
        if (e != hipSuccess) OCM_FAIL(-1, "%s launch: %s", who, hipGetErrorString(e));
    }
    return 0;
}

// The sum of squares and the non-finite count of `count` accumulator tensors of `grads`' remote
// half (ocm/acc_norm.h), kAdamMaxTensors per launch pair, the totals formed once by the last
// finishing kernel. Every tensor is checked before the first launch: a refusal writes nothing.
int acc_norm_run(const char *who, ocm_alloc_t grads, int count, const uint64_t *n, const uint64_t *g_off, double *sumsq,
                 uint64_t *nonfinite, void *work, uint64_t work_bytes, void *stream) {
    State &s = S();
    if (!grads || (count > 0 && (!n || !g_off || !work)) || !sumsq || !nonfinite) OCM_FAIL(-1, "%s: null argument", who);
    AccNormArgs x;
    switch (adam_space(grads, &x)) {  // the Adam hooks' checks, the Adam hooks' wording
    case ADAM_NO_GPU: OCM_FAIL(-1, "%s needs a GPU", who);
    case ADAM_EXTENTS:
    case ADAM_NO_PAIR: OCM_FAIL(-1, "%s needs a remote half this GPU can address", who);
    case ADAM_STRIPE: OCM_FAIL(-1, "%s: stripe unit unusable", who);
    case ADAM_OK: break;
    }
    x.host_acc = host_tier(grads) ? 1u : 0u;
    int at = -1;
    if (const AccNormBad why = acc_norm_check_list(count, n, g_off, grads->remote_bytes, &at)) {
        if (at < 0) OCM_FAIL(-1, "%s: %s", who, acc_norm_why(why));
        OCM_FAIL(-1, "%s: tensor %d: %s", who, at, acc_norm_why(why));
    }
    std::lock_guard<std::recursive_mutex> lk(s.mu);
    const AdamKnobs knobs{s.cfg.adam_host, s.cfg.adam_host_grid, s.cfg.adam_host_vec, s.cfg.adam_grid};
    DeviceGuard dg(s.device);
    const uint64_t need = acc_norm_work_bytes(count, acc_norm_cus(), knobs);
    if (work_bytes < need)
        OCM_FAIL(-1, "%s: workspace of %llu bytes is short of %llu", who, (unsigned long long)work_bytes,
                 (unsigned long long)need);
    if (wait_alloc(grads) != 0) return -1;  // queued async ops on this allocation (the accumulates) come first
    before_launch();
    x.work = static_cast<AccNormPartial *>(work);
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
        const hipError_t e = acc_norm_launch(x, f, work_bytes, knobs, static_cast<hipStream_t>(stream));
        if (e != hipSuccess) OCM_FAIL(-1, "%s launch: %s", who, hipGetErrorString(e));
    } while (k0 < count);
    return 0;
}


// The row-sparse step (ocm/adam_rows.h): the spaces of both pairs are prepared and every check
// is made before the launch, so a refusal writes nothing.
int adam_rows_run(const char *who, ocm_alloc_t table, ocm_alloc_t state, const ocm_adam_rows *d, const void *ids,
                  const void *g, const float hp[9], float gscale, unsigned long long *skipped, void *stream) {
    State &s = S();
    if (!table || !state || !d || !hp || (d->rows && (!ids || !g))) OCM_FAIL(-1, "%s: null argument", who);
    AdamRowsArgs x;
    std::memset(&x, 0, sizeof(x));
    AdamBad bad = adam_prepare(state, hp, d->bf16 != 0, &x.c);
    if (bad == ADAM_OK) bad = adam_space(table, &x.table);  // the same checks, the same wording, for the table's pair
    switch (bad) {
    case ADAM_NO_GPU: OCM_FAIL(-1, "%s needs a GPU", who);
    case ADAM_EXTENTS:
    case ADAM_NO_PAIR: OCM_FAIL(-1, "%s needs a remote half this GPU can address", who);
    case ADAM_STRIPE: OCM_FAIL(-1, "%s: stripe unit unusable", who);
    case ADAM_OK: break;
    }
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
    std::lock_guard<std::recursive_mutex> lk(s.mu);
    const AdamKnobs knobs{s.cfg.adam_host, s.cfg.adam_host_grid, s.cfg.adam_host_vec, s.cfg.adam_grid};
    if (wait_alloc(table) != 0) return -1;  // queued async ops on either allocation come first
    if (state != table && wait_alloc(state) != 0) return -1;
    DeviceGuard dg(s.device);
    before_launch();
    const hipError_t e = adam_rows_launch(x, knobs, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) OCM_FAIL(-1, "%s launch: %s", who, hipGetErrorString(e));
    return 0;
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
    const AdamKnobs knobs{s.cfg.adam_host, s.cfg.adam_host_grid, s.cfg.adam_host_vec, s.cfg.adam_grid};
    DeviceGuard dg(s.device);
    return acc_norm_work_bytes(count, acc_norm_cus(), knobs);
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
