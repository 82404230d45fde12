// MXFP4 record codec (ocm_copy_onesided_quant with OCM_QUANT_MXFP4): OCP E2M1 codes,
// two to a byte, plus one shared power-of-two scale byte (E8M0) per group of 32 elements.
//
// Per group, with every element widened exactly to fp32:
//   amax = max |x|; amax == 0 -> e = 0; else amax = m * 2^ex, m in [0.5, 1), and
//   e = ex - 3 if m <= 0.75 else ex - 2: the smallest e with amax * 2^-e <= 6 (E2M1's
//   largest value), clamped to [-127, 127]. Scale byte = e + 127.
//   code = RNE(clamp(x * 2^-e, -6, 6)) to E2M1: bit 3 the sign, magnitudes 0, 0.5, 1,
//   1.5, 2, 3, 4, 6 as codes 0 to 7, ties to the even code, -0 (and what rounds to it)
//   keeps its sign.
// Decode: value(code) * 2^e in fp32 (always exact), rounded to nearest even into the
// element type.
// A record of `elems` elements is elems / 2 code bytes (element 2i the low nibble of
// byte i, element 2i + 1 the high one), then elems / 32 scale bytes.
//
// mx4_group_exp is the one copy of the exponent rule: the kernel (quant_tile.h) and the
// host codec both call it. mx4_f32_to_e2m1 and mx4_e2m1_to_f32_bits are the code rule in
// integer arithmetic, callable from both sides too. The rest of the header is the plain
// C++ codec (host path of the library, tests); the 16-bit widen and narrow helpers are
// those of ocm/mx8.h.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdio>

#include "ocm/mx8.h"

namespace ocm {

// The record format of a converting op: bits 8 to 15 of its dtype word, as in
// enum ocm_quant_format (oncillamem.h). The low byte is the element type.
constexpr uint32_t kQuantFmtMx8 = 0, kQuantFmtMx4 = 0x100;
constexpr uint32_t kQuantElemMask = 0xffu, kQuantFmtMask = 0xff00u;

// log2 of the elements one code byte holds: 0 (MXFP8) or 1 (MXFP4). Known formats only.
OCM_MX8_HD inline uint32_t quant_code_shift(uint32_t dtype_word) { return (dtype_word & kQuantFmtMask) == kQuantFmtMx4; }

// Record bytes of `elems` elements in the format of `dtype_word` (a known one).
inline size_t quant_record_bytes(uint64_t elems, uint32_t dtype_word) {
    return (size_t)((elems >> quant_code_shift(dtype_word)) + elems / kMx8Group);
}
inline size_t mx4_record_bytes(uint64_t elems) { return (size_t)(elems / 2 + elems / kMx8Group); }

// Group exponent e from the fp32 bit pattern of amax (sign bit clear). Integer only,
// fp32 subnormals included. Inf / NaN patterns give some e in range: no fault, codes
// unspecified.
OCM_MX8_HD inline int mx4_group_exp(uint32_t amax_bits) {
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
    // m <= 0.75  <=>  1.man <= 1.5
    int e = ex - (man <= 0x400000u ? 3 : 2);
    return e < -127 ? -127 : e > 127 ? 127 : e;
}

// fp32 bit pattern of y -> E2M1 code, round to nearest even, saturating at 6 (the clamp
// of the rule; Inf and NaN saturate too).
OCM_MX8_HD inline uint32_t mx4_f32_to_e2m1(uint32_t bits) {
    const uint32_t sign = (bits >> 28) & 8u, a = bits & 0x7fffffffu;
    uint32_t m;
    if (a < 0x3f800000u) {
        // below 1: multiples of 0.5; the ties 0.25 and 0.75 go to the even codes 0 and 2
        m = (a > 0x3e800000u) + (a >= 0x3f400000u);
    } else {
        m = ((a + 0x1fffffu + ((a >> 22) & 1u)) >> 22) - 252u;  // exponent | 1 mantissa bit, carry included
        m = m > 7u ? 7u : m;
    }
    return sign | m;
}

// E2M1 code -> the fp32 bit pattern of its value.
OCM_MX8_HD inline uint32_t mx4_e2m1_to_f32_bits(uint32_t c) {
    const uint32_t m = c & 7u;
    const uint32_t mag = m < 2u ? m * 0x3f000000u : (((m >> 1) + 126u) << 23) | ((m & 1u) << 22);
    return ((c & 8u) << 28) | mag;
}

// ---- plain C++ codec ----

inline void mx4_encode(const uint16_t *src, uint64_t elems, uint32_t dtype, uint8_t *record) {
    uint8_t *codes = record, *scales = record + elems / 2;
    for (uint64_t g = 0; g < elems / kMx8Group; g++) {
        float x[kMx8Group];
        uint32_t amax = 0;
        for (int i = 0; i < kMx8Group; i++) {
            x[i] = mx8_widen(src[g * kMx8Group + i], dtype);
            const uint32_t ab = mx8_float_bits(x[i]) & 0x7fffffffu;
            amax = ab > amax ? ab : amax;
        }
        const int e = mx4_group_exp(amax);
        const float inv = mx8_bits_float(mx8_pow2_bits(-e));
        scales[g] = (uint8_t)(e + kMx8ScaleBias);
        for (int i = 0; i < kMx8Group; i += 2) {
            const uint32_t lo = mx4_f32_to_e2m1(mx8_float_bits(x[i] * inv)), hi = mx4_f32_to_e2m1(mx8_float_bits(x[i + 1] * inv));
            codes[(g * kMx8Group + i) / 2] = (uint8_t)(lo | (hi << 4));
        }
    }
}

inline void mx4_decode(const uint8_t *record, uint64_t elems, uint32_t dtype, uint16_t *dst) {
    const uint8_t *codes = record, *scales = record + elems / 2;
    for (uint64_t g = 0; g < elems / kMx8Group; g++) {
        const int e = (int)scales[g] - kMx8ScaleBias;
        for (int i = 0; i < kMx8Group; i++) {
            const uint64_t el = g * kMx8Group + i;
            const uint32_t c = (codes[el / 2] >> (4 * (el & 1))) & 15u;
            dst[el] = mx8_narrow(std::ldexp(mx8_bits_float(mx4_e2m1_to_f32_bits(c)), e), dtype);
        }
    }
}

// Either format by the op's dtype word (element | format), for the host path.
inline void quant_encode(const uint16_t *src, uint64_t elems, uint32_t dtype_word, uint8_t *record) {
    if (quant_code_shift(dtype_word))
        mx4_encode(src, elems, dtype_word & kQuantElemMask, record);
    else
        mx8_encode(src, elems, dtype_word & kQuantElemMask, record);
}
inline void quant_decode(const uint8_t *record, uint64_t elems, uint32_t dtype_word, uint16_t *dst) {
    if (quant_code_shift(dtype_word))
        mx4_decode(record, elems, dtype_word & kQuantElemMask, dst);
    else
        mx8_decode(record, elems, dtype_word & kQuantElemMask, dst);
}

// The dtype word of an op: 0 if fine; else -1 with `why` (at least 64 bytes) saying what
// is wrong. A word with only low-byte bits is an element type alone, as before formats.
inline int quant_check_dtype(uint32_t dtype_word, char *why, size_t why_len) {
    const uint32_t el = dtype_word & kQuantElemMask, fmt = dtype_word & kQuantFmtMask;
    if (dtype_word & ~(kQuantElemMask | kQuantFmtMask)) {
        std::snprintf(why, why_len, "stray bits in dtype 0x%x (element type | record format is needed)", dtype_word);
        return -1;
    }
    if (fmt != kQuantFmtMx8 && fmt != kQuantFmtMx4) {
        std::snprintf(why, why_len, "unknown record format 0x%x", fmt);
        return -1;
    }
    if (el != kMx8Bf16 && el != kMx8Fp16) {
        std::snprintf(why, why_len, "unknown element type %u", el);
        return -1;
    }
    return 0;
}

}  // namespace ocm
