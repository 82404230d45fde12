// MXFP8 record codec (ocm_copy_onesided_quant): OCP e4m3fn codes plus one shared
// power-of-two scale byte (E8M0) per group of 32 elements.
//
// Per group, with every element widened exactly to fp32:
//   amax = max |x|; amax == 0 -> e = 0; else amax = m * 2^ex, m in [0.5, 1), and
//   e = ex - 9 if m <= 0.875 else ex - 8: the smallest e with amax * 2^-e <= 448
//   (e4m3fn's largest finite value), clamped to [-127, 127]. Scale byte = e + 127.
//   code = RNE(clamp(x * 2^-e, -448, 448)) to e4m3fn, fp8 subnormals kept.
// Decode: float(code) * 2^e in fp32, rounded to nearest even into the element type.
// The scaling is exact (a power of two), so the gfx950 kernel (xfer_quant.hip, the
// packed fp8 converts), this host codec and the torch oracle
// (oncilla_amd/ops/quant.py) agree byte for byte.
//
// mx8_group_exp is the one copy of the exponent rule: the kernel and the host
// codec both call it. The rest of the header is the plain C++ codec (host path of
// the library, tests).
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define OCM_MX8_HD __host__ __device__
#else
#define OCM_MX8_HD
#endif

namespace ocm {

constexpr int kMx8Group = 32;       // elements per scale byte
constexpr int kMx8ScaleBias = 127;  // E8M0

// Group exponent e from the fp32 bit pattern of amax (sign bit clear). Integer
// only, fp32 subnormals included (a bf16 subnormal widens to one). Inf / NaN
// patterns give some e in range: no fault, codes unspecified.
OCM_MX8_HD inline int mx8_group_exp(uint32_t amax_bits) {
    if (amax_bits == 0) return 0;
    uint32_t man = amax_bits & 0x7fffffu;
    int ex;  // amax = m * 2^ex, m in [0.5, 1)
    const uint32_t bexp = amax_bits >> 23;
    if (bexp) {
        ex = (int)bexp - 126;
    } else {
        const int hb = 31 - __builtin_clz(man);  // top set bit, 0..22
        ex = hb - 148;
        man = (man << (23 - hb)) & 0x7fffffu;
    }
    // m <= 0.875  <=>  1.man <= 1.75
    int e = ex - (man <= 0x600000u ? 9 : 8);
    return e < -127 ? -127 : e > 127 ? 127 : e;
}

// 2^k as an fp32 bit pattern, k in [-126, 127] (every -e the rule can produce).
OCM_MX8_HD inline uint32_t mx8_pow2_bits(int k) { return (uint32_t)(k + 127) << 23; }

inline size_t mx8_record_bytes(uint64_t elems) { return (size_t)(elems + elems / kMx8Group); }

// The wave-tile of the converting kernels (ocm/quant.h, ocm/quant_strided.h): 2048
// elements, 4 KiB of source, 2 KiB of codes, 64 scale bytes.
constexpr uint32_t kQuantTileShift = 11;
constexpr uint32_t kQuantTileElems = 1u << kQuantTileShift;
OCM_MX8_HD inline uint64_t quant_tile_count(uint64_t elems) { return (elems + kQuantTileElems - 1) >> kQuantTileShift; }

// ---- plain C++ codec ----

inline float mx8_bits_float(uint32_t b) {
    float f;
    std::memcpy(&f, &b, 4);
    return f;
}
inline uint32_t mx8_float_bits(float f) {
    uint32_t b;
    std::memcpy(&b, &f, 4);
    return b;
}

// fp32 (|y| <= 448) -> e4m3fn, round to nearest even, subnormals kept. NaN -> 0x7f.
inline uint8_t mx8_f32_to_e4m3(float y) {
    const uint32_t bits = mx8_float_bits(y);
    const uint8_t sign = (uint8_t)((bits >> 24) & 0x80u);
    const uint32_t abits = bits & 0x7fffffffu;
    if (abits > 0x7f800000u) return (uint8_t)(sign | 0x7fu);
    const float a = mx8_bits_float(abits);
    if (a < 0.015625f) {
        // below 2^-6: multiples of 2^-9; q == 8 is the smallest normal's code as it stands
        const float t = a * 512.0f;
        int q = (int)t;
        const float fr = t - (float)q;
        if (fr > 0.5f || (fr == 0.5f && (q & 1))) q++;
        return (uint8_t)(sign | q);
    }
    if (abits >= 0x43e00000u) return (uint8_t)(sign | 0x7eu);  // >= 448: saturate
    const uint32_t r = (abits + 0x7ffffu + ((abits >> 20) & 1u)) >> 20;  // exponent | 3 mantissa bits, carry included
    return (uint8_t)(sign | (r - ((127u - 7u) << 3)));
}

inline float mx8_e4m3_to_f32(uint8_t c) {
    const uint32_t ex = (c >> 3) & 15u, man = c & 7u;
    float v;
    if (ex == 15u && man == 7u)
        v = NAN;
    else if (ex == 0)
        v = (float)man * 0.001953125f;  // man * 2^-9
    else
        v = mx8_bits_float(((ex + 120u) << 23) | (man << 20));
    return (c & 0x80u) ? -v : v;
}

inline float mx8_bf16_to_f32(uint16_t h) { return mx8_bits_float((uint32_t)h << 16); }
inline uint16_t mx8_f32_to_bf16(float f) {
    const uint32_t b = mx8_float_bits(f);
    if ((b & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((b >> 16) | 0x40u);  // NaN stays NaN
    return (uint16_t)((b + 0x7fffu + ((b >> 16) & 1u)) >> 16);
}

inline float mx8_fp16_to_f32(uint16_t h) {
    const uint32_t sign = (uint32_t)(h & 0x8000u) << 16, ex = (h >> 10) & 31u, man = h & 0x3ffu;
    if (ex == 31u) return mx8_bits_float(sign | 0x7f800000u | (man << 13));
    if (ex == 0) {
        const float v = (float)man * 5.9604644775390625e-8f;  // man * 2^-24, exact
        return sign ? -v : v;
    }
    return mx8_bits_float(sign | ((ex + 112u) << 23) | (man << 13));
}
inline uint16_t mx8_f32_to_fp16(float f) {
    const uint32_t b = mx8_float_bits(f);
    const uint16_t sign = (uint16_t)((b >> 16) & 0x8000u);
    const uint32_t a = b & 0x7fffffffu;
    if (a > 0x7f800000u) return (uint16_t)(sign | 0x7e00u);
    if (a >= 0x477ff000u) return (uint16_t)(sign | 0x7c00u);  // >= 65520 rounds to inf
    if (a < 0x38800000u) {
        // below 2^-14: multiples of 2^-24; 1024 is the smallest normal's code as it stands
        const float t = mx8_bits_float(a) * 16777216.0f;
        int q = (int)t;
        const float fr = t - (float)q;
        if (fr > 0.5f || (fr == 0.5f && (q & 1))) q++;
        return (uint16_t)(sign | q);
    }
    const uint32_t r = (a + 0xfffu + ((a >> 13) & 1u)) >> 13;  // exponent | 10 mantissa bits, carry included
    return (uint16_t)(sign | (r - (112u << 10)));
}

// Element types as in enum ocm_quant_dtype (oncillamem.h).
constexpr uint32_t kMx8Bf16 = 1, kMx8Fp16 = 2;

inline float mx8_widen(uint16_t h, uint32_t dtype) { return dtype == kMx8Bf16 ? mx8_bf16_to_f32(h) : mx8_fp16_to_f32(h); }
inline uint16_t mx8_narrow(float f, uint32_t dtype) { return dtype == kMx8Bf16 ? mx8_f32_to_bf16(f) : mx8_f32_to_fp16(f); }

// Encode `elems` (a multiple of 32) 16-bit elements into a record: `elems` code
// bytes, then elems / 32 scale bytes.
inline void mx8_encode(const uint16_t *src, uint64_t elems, uint32_t dtype, uint8_t *record) {
    uint8_t *codes = record, *scales = record + elems;
    for (uint64_t g = 0; g < elems / kMx8Group; g++) {
        float x[kMx8Group];
        uint32_t amax = 0;
        for (int i = 0; i < kMx8Group; i++) {
            x[i] = mx8_widen(src[g * kMx8Group + i], dtype);
            const uint32_t ab = mx8_float_bits(x[i]) & 0x7fffffffu;
            amax = ab > amax ? ab : amax;
        }
        const int e = mx8_group_exp(amax);
        const float inv = mx8_bits_float(mx8_pow2_bits(-e));
        scales[g] = (uint8_t)(e + kMx8ScaleBias);
        for (int i = 0; i < kMx8Group; i++) {
            float y = x[i] * inv;
            y = y > 448.0f ? 448.0f : y < -448.0f ? -448.0f : y;
            codes[g * kMx8Group + i] = mx8_f32_to_e4m3(y);
        }
    }
}

inline void mx8_decode(const uint8_t *record, uint64_t elems, uint32_t dtype, uint16_t *dst) {
    const uint8_t *codes = record, *scales = record + elems;
    for (uint64_t g = 0; g < elems / kMx8Group; g++) {
        const int e = (int)scales[g] - kMx8ScaleBias;
        for (int i = 0; i < kMx8Group; i++)
            dst[g * kMx8Group + i] = mx8_narrow(std::ldexp(mx8_e4m3_to_f32(codes[g * kMx8Group + i]), e), dtype);
    }
}

}  // namespace ocm
