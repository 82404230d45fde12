// One-sided accumulate (ocm_copy_onesided_accumulate): the remote half holds fp32
// accumulators, the local half elements of ocm_acc_dtype, and every element becomes
//     remote[i] = remote[i] + scale * widen(local[i]).
// One launch serves a whole list, planned as every descriptor list is (ocm/list.h): the
// list is cut into wave-tiles of kAccTileElems elements in op-relative coordinates
// (4 KiB of accumulators), the host prefix-sums each op's tile count into `first_tile`,
// and every wave walks a contiguous tile range.
//
// The element rule is defined bit for bit, so that the kernel, the host path and the
// torch oracle agree whatever the pair: two IEEE fp32 operations, each rounded to
// nearest even, p = scale * x and then r = acc + p. They are never fused: an fma rounds
// once, and a path that fused (hipcc contracts a + b * c by default) would differ from
// one that cannot in the last bit. Subnormals are kept. bf16 and fp16 widen exactly. A
// NaN result is some NaN; its payload is not specified.
//
// The descriptors are XferBatchOp records read differently: len counts elements, pad
// holds the element type, put the scale's bits. XferBatchArgs carries them unchanged
// (tile_shift is unused), so large lists take the batch path's staged upload.
//
// This header is what the kernel (xfer_acc.hip), the host path (acc.cpp) and the
// stand-alone test program (ocm_acc_tests.cpp) share; it needs no HIP. Transfer plans,
// the copy service, a get-side accumulate (local += remote) and integer element types
// are out of scope.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "ocm/list.h"
#include "oncillamem.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define OCM_ACC_HD __host__ __device__
#else
#define OCM_ACC_HD
#endif

// Contraction off for acc_rule, whatever -ffp-contract says.
#if defined(__clang__)
#define OCM_ACC_NO_CONTRACT_ATTR
#define OCM_ACC_NO_CONTRACT_PRAGMA _Pragma("clang fp contract(off)")
#elif defined(__GNUC__)
#define OCM_ACC_NO_CONTRACT_ATTR __attribute__((optimize("fp-contract=off")))
#define OCM_ACC_NO_CONTRACT_PRAGMA
#else
#define OCM_ACC_NO_CONTRACT_ATTR
#define OCM_ACC_NO_CONTRACT_PRAGMA
#endif

namespace ocm {

constexpr uint32_t kAccTileShift = 10;  // 1024 elements: 4 KiB of accumulators, 256 16-byte vectors
constexpr uint32_t kAccTileElems = 1u << kAccTileShift;
constexpr uint32_t kAccF32 = OCM_ACC_F32, kAccBf16 = OCM_ACC_BF16, kAccFp16 = OCM_ACC_FP16;

// ---- the element rule ----
// r = acc + scale * x as two roundings.
OCM_ACC_HD OCM_ACC_NO_CONTRACT_ATTR inline float acc_rule(float acc, float x, float scale) {
    OCM_ACC_NO_CONTRACT_PRAGMA
    const float p = scale * x;
    return acc + p;
}

OCM_ACC_HD inline float acc_bits_float(uint32_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_bit_cast(float, b);
#else
    float f;
    std::memcpy(&f, &b, 4);
    return f;
#endif
}
OCM_ACC_HD inline uint32_t acc_float_bits(float f) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_bit_cast(uint32_t, f);
#else
    uint32_t b;
    std::memcpy(&b, &f, 4);
    return b;
#endif
}

// A 16-bit element widened to fp32, exactly (fp16 subnormals included).
OCM_ACC_HD inline float acc_widen16(uint32_t h, bool bf16) {
    if (bf16) return acc_bits_float(h << 16);
#if defined(__HIP_DEVICE_COMPILE__)
    return (float)__builtin_bit_cast(_Float16, (uint16_t)h);
#else
    const uint32_t sign = (h & 0x8000u) << 16, ex = (h >> 10) & 31u, man = h & 0x3ffu;
    if (ex == 31u) return acc_bits_float(sign | 0x7f800000u | (man << 13));
    if (ex == 0) {
        const float v = (float)man * 5.9604644775390625e-8f;  // man * 2^-24, exact
        return sign ? -v : v;
    }
    return acc_bits_float(sign | ((ex + 112u) << 23) | (man << 13));
#endif
}

// Bytes of one element of the local half (0: unknown type).
OCM_ACC_HD inline uint32_t acc_elem_size(uint32_t dtype) {
    return dtype == kAccF32 ? 4u : (dtype == kAccBf16 || dtype == kAccFp16) ? 2u : 0u;
}

// ---- tiles ----
OCM_ACC_HD inline uint64_t acc_tile_count(uint64_t elems) { return (elems + kAccTileElems - 1) >> kAccTileShift; }

// ---- descriptor packing (Op: XferBatchOp) ----
template <class Op>
inline void acc_pack(const struct ocm_acc_params &p, Op *o) {
    o->lin_off = p.local_offset;
    o->rem_off = p.remote_offset;
    o->len = p.elems;
    o->pad = p.dtype;
    o->put = acc_float_bits(p.scale);
}
// Fills first_tile, returns total tiles.
template <class Op>
inline uint64_t acc_plan(Op *ops, uint32_t n) {
    return list_plan(ops, n, [](const Op &op) { return acc_tile_count(op.len); });
}

#if !defined(__HIP_DEVICE_COMPILE__)
// n elements on the CPU: acc[i] = rule(acc[i], widen(local[i]), scale). `local` points at
// the first element, whatever its type.
inline void acc_apply_host(float *acc, const void *local, uint64_t n, uint32_t dtype, float scale) {
    if (dtype == kAccF32) {
        const float *x = static_cast<const float *>(local);
        for (uint64_t i = 0; i < n; i++) acc[i] = acc_rule(acc[i], x[i], scale);
    } else {
        const uint16_t *x = static_cast<const uint16_t *>(local);
        const bool bf16 = dtype == kAccBf16;
        for (uint64_t i = 0; i < n; i++) acc[i] = acc_rule(acc[i], acc_widen16(x[i], bf16), scale);
    }
}

// One op against halves of local_bytes / remote_bytes. 0: fine (*acc_bytes = the
// accumulator bytes it updates, 0 for an empty op); -1: `why` says what is wrong. elems is
// below 2^31 before it is multiplied, and every range is tested as bytes <= size - offset,
// so nothing here can overflow.
inline int acc_check_op(const struct ocm_acc_params &p, uint64_t local_bytes, uint64_t remote_bytes, uint64_t *acc_bytes,
                        char *why, size_t why_len) {
    *acc_bytes = 0;
    const uint32_t esize = acc_elem_size(p.dtype);
    if (esize == 0) {
        std::snprintf(why, why_len, "unknown element type %u", p.dtype);
        return -1;
    }
    if ((acc_float_bits(p.scale) & 0x7f800000u) == 0x7f800000u) {
        std::snprintf(why, why_len, "scale is not finite (bits 0x%08x)", acc_float_bits(p.scale));
        return -1;
    }
    if (p.elems % 4 != 0 || p.elems >= (1ull << 31)) {
        std::snprintf(why, why_len, "%llu elements (a multiple of 4 below 2^31 is needed)", (unsigned long long)p.elems);
        return -1;
    }
    if (p.local_offset % 16 != 0) {
        std::snprintf(why, why_len, "local offset %llu is not a multiple of 16", (unsigned long long)p.local_offset);
        return -1;
    }
    if (p.remote_offset % 16 != 0) {
        std::snprintf(why, why_len, "remote offset %llu is not a multiple of 16", (unsigned long long)p.remote_offset);
        return -1;
    }
    const uint64_t lbytes = p.elems * esize, rbytes = p.elems * 4;
    if (p.local_offset > local_bytes || lbytes > local_bytes - p.local_offset) {
        std::snprintf(why, why_len, "local range [%llu,+%llu) exceeds %llu bytes", (unsigned long long)p.local_offset,
                      (unsigned long long)lbytes, (unsigned long long)local_bytes);
        return -1;
    }
    if (p.remote_offset > remote_bytes || rbytes > remote_bytes - p.remote_offset) {
        std::snprintf(why, why_len, "remote range [%llu,+%llu) exceeds %llu bytes", (unsigned long long)p.remote_offset,
                      (unsigned long long)rbytes, (unsigned long long)remote_bytes);
        return -1;
    }
    *acc_bytes = rbytes;
    return 0;
}
#endif

}  // namespace ocm
