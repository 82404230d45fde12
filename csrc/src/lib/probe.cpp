// Probe and benchmark hooks over raw pointers or timed inside the library (not part of
// the ABI): the kernels on raw device pointers, timing loops without Python in them, the
// word pattern, and the owner-side helpers.
#include "lists.h"

using namespace ocm;
using namespace ocmlib;

extern "C" {

// Striped transfer between raw device pointers on `device` (kernel numerics tests).
int ocm_x_xfer(int device, void *lin, void **ext, int n_ext, uint64_t unit, uint64_t rem_off, uint64_t len, int put,
               int variant, int blocks, int sync) {
    if (n_ext < 1 || n_ext > kXferMaxExtents) return -1;
    DeviceGuard g(device);
    XferArgs x;
    std::memset(&x, 0, sizeof(x));
    x.lin = static_cast<char *>(lin);
    x.rem_off = rem_off;
    x.len = len;
    x.put = (uint32_t)put;
    if (pair_side(ext, n_ext, unit, 4, &x) < 0) return -1;
    XferTuning t = xfer_tuning_from_env();
    if (variant) t.variant = variant;
    if (blocks) t.max_blocks = blocks;
    if (t.variant == XFER_PUSH && !put) {
        // the push-get kernel, every extent in the mask (numerics tests); the
        // same kernel a push get launches on each owner's GPU
        const uint32_t all = (uint32_t)((1ull << n_ext) - 1);
        if (xfer_push_launch(x, all, blocks, nullptr) != hipSuccess) return -1;
    } else if (xfer_launch(x, t, nullptr) != hipSuccess) {
        return -1;
    }
    if (!sync) return 0;  // caller orders it on the null stream
    return hipDeviceSynchronize() == hipSuccess ? 0 : -1;
}

// Batched transfer between raw device pointers (kernel numerics tests / PMC
// profiles without daemons). ops: n x {lin_off, rem_off, len, put} (u64 each).
// Returns 0, or -1 on bad arguments; iters > 1 repeats the launch (profiling).
int ocm_x_batch(int device, void *lin, void **ext, int n_ext, uint64_t unit, const uint64_t *ops, int n_ops, int iters) {
    if (n_ext < 1 || n_ext > kXferMaxExtents || n_ops < 1 || !ops) return -1;
    DeviceGuard g(device);
    XferBatchArgs args;
    std::memset(&args, 0, sizeof(args));
    args.lin = static_cast<char *>(lin);
    if (pair_side(ext, n_ext, unit, 4, &args) < 0) return -1;
    args.tile_shift = xfer_batch_tile_shift(args.n_ext, args.unit_shift);
    std::vector<XferBatchOp> v((size_t)n_ops);
    for (int i = 0; i < n_ops; i++) {
        v[i].lin_off = ops[4 * i];
        v[i].rem_off = ops[4 * i + 1];
        v[i].len = ops[4 * i + 2];
        v[i].put = ops[4 * i + 3] != 0;
    }
    list_plan_args(&args, v, xfer_batch_plan);  // as ocm_copy_onesided_batch plans
    if (!args.total_tiles) return 0;
    void *dev = nullptr;
    if (n_ops > kXferInlineOps) {
        const size_t need = list_upload_bytes<XferBatchOp>(v.size(), args.grid);
        std::vector<char> up(need);
        if (hipMalloc(&dev, need) != hipSuccess) return -1;
        list_pack(&args, v, up.data(), dev);
        if (hipMemcpy(dev, up.data(), need, hipMemcpyHostToDevice) != hipSuccess) {
            (void)hipFree(dev);
            return -1;
        }
    }
    XferTuning t = xfer_tuning_from_env();
    int rc = 0;
    for (int k = 0; k < std::max(1, iters) && rc == 0; k++)
        rc = xfer_batch_launch(args, t, nullptr) == hipSuccess ? 0 : -1;
    if (hipDeviceSynchronize() != hipSuccess) rc = -1;
    if (dev) (void)hipFree(dev);
    return rc;
}

// Time `iters` back-to-back device copies (seconds per copy, event-timed).
double ocm_x_time_device_copy(int device, void *dst, const void *src, uint64_t bytes, int variant, int blocks,
                              int nt, int iters) {
    DeviceGuard g(device);
    const XferTuning t = tuning_of(variant, blocks, nt);
    hipEvent_t e0, e1;
    (void)hipEventCreate(&e0);
    (void)hipEventCreate(&e1);
    (void)xfer_copy(dst, src, bytes, t, nullptr);  // warm
    (void)hipEventRecord(e0, nullptr);
    for (int i = 0; i < iters; i++) (void)xfer_copy(dst, src, bytes, t, nullptr);
    (void)hipEventRecord(e1, nullptr);
    (void)hipEventSynchronize(e1);
    float ms = 0;
    (void)hipEventElapsedTime(&ms, e0, e1);
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    return (double)ms / 1e3 / (iters > 0 ? iters : 1);
}

// Wall-clock seconds per blocking one-sided op, measured inside the library
// (no Python in the loop): the sweep primitive of bench.py.
// Per-sample wall time (seconds) of ocm_alloc_ex and the matching ocm_free,
// timed in C so callers (bench.py) report the API's latency, not their FFI's.
// Returns the number of samples taken (< samples on the first failure).
int ocm_x_alloc_latency(ocm_alloc_param_t ap, const struct ocm_alloc_ex_params *ex, int samples, double *alloc_s,
                        double *free_s) {
    for (int i = 0; i < samples; i++) {
        struct timespec t0, t1, t2;
        clock_gettime(CLOCK_MONOTONIC, &t0);
        ocm_alloc_t a = ocm_alloc_ex(ap, ex);
        clock_gettime(CLOCK_MONOTONIC, &t1);
        if (!a) return i;
        const int rc = ocm_free(a);
        clock_gettime(CLOCK_MONOTONIC, &t2);
        if (rc != 0) return i;
        alloc_s[i] = (double)(t1.tv_sec - t0.tv_sec) + (double)(t1.tv_nsec - t0.tv_nsec) * 1e-9;
        free_s[i] = (double)(t2.tv_sec - t1.tv_sec) + (double)(t2.tv_nsec - t1.tv_nsec) * 1e-9;
    }
    return samples;
}

double ocm_x_time_onesided(ocm_alloc_t a, ocm_param_t p, int iters) {
    struct timespec t0, t1;
    clock_gettime(CLOCK_MONOTONIC, &t0);
    for (int i = 0; i < iters; i++)
        if (ocm_copy_onesided(a, p) != 0) return -1.0;
    clock_gettime(CLOCK_MONOTONIC, &t1);
    double dt = (double)(t1.tv_sec - t0.tv_sec) + (double)(t1.tv_nsec - t0.tv_nsec) * 1e-9;
    return dt / (iters > 0 ? iters : 1);
}

// Per-op samples of a blocking one-sided op, each timed on its own: up to
// `iters` ops, stopping early once `cap_ns` have passed (at least `min_iters`
// ops). Before each op the calling thread stays busy for `gap_ns` without
// touching the library (an application computing between small ops), so the
// samples include whatever an idle gap costs the next op (the copy service's
// idle exit and relaunch). out[i] = seconds of op i; *relaunches = copy-service
// relaunches during the run. Returns the number of samples, -1 on an op failure.
int ocm_x_time_onesided_samples(ocm_alloc_t a, ocm_param_t p, int iters, int min_iters, uint64_t gap_ns,
                                uint64_t cap_ns, double *out, uint64_t *relaunches) {
    uint64_t r0 = 0;
    {
        std::lock_guard<std::recursive_mutex> lk(S().mu);
        r0 = S().svc_relaunches;
    }
    const uint64_t start = now_ns();
    int n = 0;
    for (; n < iters; n++) {
        if (n >= min_iters && now_ns() - start > cap_ns) break;
        if (gap_ns) {
            const uint64_t g0 = now_ns();
            while (now_ns() - g0 < gap_ns) __builtin_ia32_pause();
        }
        const uint64_t t0 = now_ns();
        if (ocm_copy_onesided(a, p) != 0) return -1;
        out[n] = (double)(now_ns() - t0) * 1e-9;
    }
    if (relaunches) {
        std::lock_guard<std::recursive_mutex> lk(S().mu);
        *relaunches = S().svc_relaunches - r0;
    }
    return n;
}

// Fill / check the deterministic word pattern on device or host memory.
// `words` 32-bit words starting at pattern index `first`; returns mismatches (check) or 0 / -1.
long long ocm_x_pattern(void *p, uint64_t words, uint64_t first, uint32_t seed, int check) {
    State &s = S();
    Loc l = pointer_loc(p);
    if (s.device < 0 || l == LOC_HOST) {
        uint32_t *w = static_cast<uint32_t *>(p);
        long long bad = 0;
        for (uint64_t i = 0; i < words; i++) {
            if (check)
                bad += w[i] != pattern_word_host(first + i, seed);
            else
                w[i] = pattern_word_host(first + i, seed);
        }
        return bad;
    }
    std::lock_guard<std::recursive_mutex> lk(s.mu);  // the library stream and its event are shared
    DeviceGuard g(s.device);
    if (!check) {
        if (pattern_fill(p, words, first, seed, s.stream) != hipSuccess) return -1;
        return sync_stream() == 0 ? 0 : -1;
    }
    // One counter kept for the process: hipFree synchronizes the whole device,
    // which would also wait for the resident copy service's idle exit.
    if (!s.pattern_bad && hipMalloc(reinterpret_cast<void **>(&s.pattern_bad), sizeof(unsigned long long)) != hipSuccess) {
        s.pattern_bad = nullptr;
        return -1;
    }
    unsigned long long bad = 0;
    (void)hipMemsetAsync(s.pattern_bad, 0, sizeof(bad), s.stream);
    hipError_t e = pattern_check(p, words, first, seed, s.pattern_bad, s.stream);
    if (e == hipSuccess) e = hipMemcpyAsync(&bad, s.pattern_bad, sizeof(bad), hipMemcpyDeviceToHost, s.stream);
    int rc = sync_stream();
    return (e == hipSuccess && rc == 0) ? (long long)bad : -1;
}

// Owner-side helpers that need no ocm_init (a verifier process on the owner's
// GPU): open an exported HBM slab on `device`, and fill / check the word
// pattern there with the same gfx950 kernels on that device's null stream.
int ocm_x_ipc_open(int device, const uint8_t *handle, void **out) {
    if (!handle || !out || hipSetDevice(device) != hipSuccess) return -1;
    hipIpcMemHandle_t h;
    std::memcpy(&h, handle, sizeof(h));
    if (hipIpcOpenMemHandle(out, h, hipIpcMemLazyEnablePeerAccess) != hipSuccess) {
        (void)hipGetLastError();
        return -1;
    }
    return 0;
}

int ocm_x_ipc_close(int device, void *p) {
    if (hipSetDevice(device) != hipSuccess) return -1;
    return hipIpcCloseMemHandle(p) == hipSuccess ? 0 : -1;
}

long long ocm_x_pattern_dev(int device, void *p, uint64_t words, uint64_t first, uint32_t seed, int check) {
    if (!p || hipSetDevice(device) != hipSuccess) return -1;
    unsigned long long *bad_dev = nullptr, bad = 0;
    hipError_t e = hipSuccess;
    if (check) {
        e = hipMalloc(reinterpret_cast<void **>(&bad_dev), sizeof(bad));
        if (e == hipSuccess) e = hipMemset(bad_dev, 0, sizeof(bad));
        if (e == hipSuccess) e = pattern_check(p, words, first, seed, bad_dev, nullptr);
        if (e == hipSuccess) e = hipMemcpy(&bad, bad_dev, sizeof(bad), hipMemcpyDeviceToHost);
        if (bad_dev) (void)hipFree(bad_dev);
    } else {
        e = pattern_fill(p, words, first, seed, nullptr);
        if (e == hipSuccess) e = hipDeviceSynchronize();
    }
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return -1;
    }
    return (long long)bad;
}
}  // extern "C"
