// The tile bodies of the converting kernels (xfer_quant.hip, xfer_quant_strided.hip,
// xfer_quant_indexed.hip):
// one wave encodes (put_tile) or decodes (get_tile) one wave-tile of at most
// kQuantTileElems elements, given where its elements, its codes and its scale bytes
// lie. How a kernel finds those three places is its own rule (ocm/quant.h: a tile of a
// record; ocm/quant_strided.h: a piece of a row's record). `A` is the launch arguments,
// read in place for the extent table (stripe_ptr). Device only: include from a HIP
// translation unit, inside no namespace.
//
// MXFP8 (put_tile, get_tile): two rounds of 1024 elements, a lane owns 16 elements, a
// group is a lane pair. MXFP4 (put_tile_mx4, get_tile_mx4): one round, a lane owns a
// whole group of 32 elements, 64 bytes of source and one 16-byte vector of codes, so
// there is no cross-lane step and code stores and loads stay whole vectors. Both hand
// the tile's scale bytes over through the wave's 64 bytes of LDS (store_scales).
#pragma once
#include <hip/hip_runtime.h>

#include "ocm/mx4.h"
#include "xfer_copy.h"

namespace ocm {

namespace {

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));

constexpr uint32_t kRoundElems = 1024;  // 64 lanes x 16 elements

template <bool BF16>
__device__ __forceinline__ float widen16(uint32_t h) {
    if constexpr (BF16)
        return __builtin_bit_cast(float, h << 16);
    else
        return (float)__builtin_bit_cast(_Float16, (uint16_t)h);
}

// Round to nearest even into the element type.
template <bool BF16>
__device__ __forceinline__ uint32_t narrow16(float f) {
    if constexpr (BF16) {
        const uint32_t b = __builtin_bit_cast(uint32_t, f);
        if ((b & 0x7fffffffu) > 0x7f800000u) return (b >> 16) | 0x40u;
        return (b + 0x7fffu + ((b >> 16) & 1u)) >> 16;
    } else {
        return (uint32_t)__builtin_bit_cast(uint16_t, (_Float16)f);
    }
}

// The tile's ne / 32 scale bytes, which the lanes have just written to sw, to striped
// offset `scales`: whole vectors, a partial last one byte by byte.
template <bool NT, class A>
__device__ __forceinline__ void store_scales(const A &a, uint64_t scales, uint32_t ne, uint32_t lane, uint8_t *sw) {
    // the wave's own LDS bytes: written by the caller, read below by other lanes of the same wave
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const uint32_t ng = ne >> 5;  // scale bytes of this tile, 1..64
    if (lane < 4 && lane * 16 < ng) {
        const uint32_t nb = ng - lane * 16;
        if (nb >= 16) {
            store16<NT>(reinterpret_cast<u32x4 *>(stripe_ptr(a, a.n_ext, a.unit_shift, scales + lane * 16)),
                        *reinterpret_cast<const u32x4 *>(sw + lane * 16));
        } else {
            for (uint32_t j = 0; j < nb; j++)
                *stripe_ptr(a, a.n_ext, a.unit_shift, scales + lane * 16 + j) = (char)sw[lane * 16 + j];
        }
    }
    // the next tile writes sw again: not before these reads
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// One put tile: `ne` elements (a multiple of 32, at most 2048) from `lin` into codes
// at striped offset `codes` and scale bytes at `scales`. sw: this wave's 64 bytes of LDS.
template <bool BF16, bool NT, class A>
__device__ __forceinline__ void put_tile(const A &a, const char *lin, uint64_t codes, uint64_t scales,
                                         uint32_t ne, uint32_t lane, uint8_t *sw) {
#pragma unroll
    for (uint32_t r = 0; r < 2; r++) {
        const uint32_t el = r * kRoundElems + lane * 16;
        const bool active = el < ne;  // a lane pair (one group) is in or out together
        u32x4 v[2] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
        if (active) {
            const u32x4 *s = reinterpret_cast<const u32x4 *>(lin + 2ull * el);
            v[0] = __builtin_nontemporal_load(s);
            v[1] = __builtin_nontemporal_load(s + 1);
        }
        float x[16];
        uint32_t amax = 0;
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const uint32_t w = v[k >> 2][k & 3];
            x[2 * k] = widen16<BF16>(w & 0xffffu);
            x[2 * k + 1] = widen16<BF16>(w >> 16);
        }
#pragma unroll
        for (int k = 0; k < 16; k++) {
            const uint32_t ab = __builtin_bit_cast(uint32_t, x[k]) & 0x7fffffffu;
            amax = ab > amax ? ab : amax;
        }
        const uint32_t other = (uint32_t)__shfl_xor((int)amax, 1);
        amax = other > amax ? other : amax;
        const int e = mx8_group_exp(amax);
        const float inv = __builtin_bit_cast(float, mx8_pow2_bits(-e));
        u32x4 c;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            float y[4];
#pragma unroll
            for (int j = 0; j < 4; j++) y[j] = __builtin_fminf(__builtin_fmaxf(x[4 * k + j] * inv, -448.0f), 448.0f);
            int d = __builtin_amdgcn_cvt_pk_fp8_f32(y[0], y[1], 0, false);
            d = __builtin_amdgcn_cvt_pk_fp8_f32(y[2], y[3], d, true);
            c[k] = (uint32_t)d;
        }
        if (active) store16<NT>(reinterpret_cast<u32x4 *>(stripe_ptr(a, a.n_ext, a.unit_shift, codes + el)), c);
        if ((lane & 1u) == 0) sw[r * 32 + (lane >> 1)] = (uint8_t)(e + kMx8ScaleBias);
    }
    store_scales<NT>(a, scales, ne, lane, sw);
}

// One get tile: the reverse; local stores are nontemporal.
template <bool BF16, class A>
__device__ __forceinline__ void get_tile(const A &a, char *lin, uint64_t codes, uint64_t scales,
                                         uint32_t ne, uint32_t lane) {
#pragma unroll
    for (uint32_t r = 0; r < 2; r++) {
        const uint32_t el = r * kRoundElems + lane * 16;
        if (el >= ne) continue;
        const u32x4 c = __builtin_nontemporal_load(
            reinterpret_cast<const u32x4 *>(stripe_ptr(a, a.n_ext, a.unit_shift, codes + el)));
        const uint8_t sb = *reinterpret_cast<const uint8_t *>(stripe_ptr(a, a.n_ext, a.unit_shift, scales + (el >> 5)));
        const int e = (int)sb - kMx8ScaleBias;
        u32x4 o[2];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)c[k], false);
            const f32x2 hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)c[k], true);
            const uint32_t h0 = narrow16<BF16>(__builtin_ldexpf(lo[0], e)), h1 = narrow16<BF16>(__builtin_ldexpf(lo[1], e));
            const uint32_t h2 = narrow16<BF16>(__builtin_ldexpf(hi[0], e)), h3 = narrow16<BF16>(__builtin_ldexpf(hi[1], e));
            o[k >> 1][(k & 1) * 2] = (h0 & 0xffffu) | (h1 << 16);
            o[k >> 1][(k & 1) * 2 + 1] = (h2 & 0xffffu) | (h3 << 16);
        }
        u32x4 *d = reinterpret_cast<u32x4 *>(lin + 2ull * el);
        store16<true>(d, o[0]);
        store16<true>(d + 1, o[1]);
    }
}

// ---- MXFP4 ----

// 2^e as the scale operand of the packed fp4 converts: they read the exponent field as
// E8M0, so e = -127 (field 0) is a scale too.
__device__ __forceinline__ float mx4_scale_operand(int e) {
    return __builtin_bit_cast(float, (uint32_t)(e + kMx8ScaleBias) << 23);
}

// Eight elements, as the four dwords of element pairs they arrive in, to the eight E2M1
// codes of one dword, element 0 in the lowest nibble: RNE(clamp(x * 2^-e, -6, 6)), all of
// it in the converts that take the 16-bit pairs as they are (they scale, round and saturate).
template <bool BF16>
__device__ __forceinline__ uint32_t mx4_pack8(uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3, float scale) {
    uint32_t d = 0;
    if constexpr (BF16) {
        d = __builtin_amdgcn_cvt_scalef32_pk_fp4_bf16(d, __builtin_bit_cast(bf16x2, w0), scale, 0);
        d = __builtin_amdgcn_cvt_scalef32_pk_fp4_bf16(d, __builtin_bit_cast(bf16x2, w1), scale, 1);
        d = __builtin_amdgcn_cvt_scalef32_pk_fp4_bf16(d, __builtin_bit_cast(bf16x2, w2), scale, 2);
        d = __builtin_amdgcn_cvt_scalef32_pk_fp4_bf16(d, __builtin_bit_cast(bf16x2, w3), scale, 3);
    } else {
        d = __builtin_amdgcn_cvt_scalef32_pk_fp4_f16(d, __builtin_bit_cast(f16x2, w0), scale, 0);
        d = __builtin_amdgcn_cvt_scalef32_pk_fp4_f16(d, __builtin_bit_cast(f16x2, w1), scale, 1);
        d = __builtin_amdgcn_cvt_scalef32_pk_fp4_f16(d, __builtin_bit_cast(f16x2, w2), scale, 2);
        d = __builtin_amdgcn_cvt_scalef32_pk_fp4_f16(d, __builtin_bit_cast(f16x2, w3), scale, 3);
    }
    return d;
}

// The reverse: value(code) * 2^e rounded to nearest even into the element type, four
// dwords of element pairs.
template <bool BF16>
__device__ __forceinline__ u32x4 mx4_unpack8(uint32_t c, float scale) {
    if constexpr (BF16)
        return u32x4{__builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(c, scale, 0)),
                     __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(c, scale, 1)),
                     __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(c, scale, 2)),
                     __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(c, scale, 3))};
    else
        return u32x4{__builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(c, scale, 0)),
                     __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(c, scale, 1)),
                     __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(c, scale, 2)),
                     __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(c, scale, 3))};
}

// One MXFP4 put tile: `ne` elements (a multiple of 32, at most 2048) from `lin` into ne / 2
// code bytes at striped offset `codes` and ne / 32 scale bytes at `scales`. Lane l owns
// group l: elements [32 l, 32 l + 32), code bytes [16 l, 16 l + 16).
template <bool BF16, bool NT, class A>
__device__ __forceinline__ void put_tile_mx4(const A &a, const char *lin, uint64_t codes, uint64_t scales,
                                             uint32_t ne, uint32_t lane, uint8_t *sw) {
    const uint32_t el = lane * 32;
    const bool active = el < ne;
    u32x4 v[4] = {{0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}};
    if (active) {
        const u32x4 *s = reinterpret_cast<const u32x4 *>(lin + 2ull * el);
#pragma unroll
        for (int k = 0; k < 4; k++) v[k] = __builtin_nontemporal_load(s + k);
    }
    // |x| orders as its 16-bit pattern does: the largest pattern, widened once, is amax
    uint32_t amax = 0;
#pragma unroll
    for (int k = 0; k < 16; k++) {
        const uint32_t w = v[k >> 2][k & 3], lo = w & 0x7fffu, hi = (w >> 16) & 0x7fffu;
        amax = lo > amax ? lo : amax;
        amax = hi > amax ? hi : amax;
    }
    const int e = mx4_group_exp(__builtin_bit_cast(uint32_t, widen16<BF16>(amax)));
    const float scale = mx4_scale_operand(e);
    u32x4 c;
#pragma unroll
    for (int k = 0; k < 4; k++) c[k] = mx4_pack8<BF16>(v[k][0], v[k][1], v[k][2], v[k][3], scale);
    if (active) store16<NT>(reinterpret_cast<u32x4 *>(stripe_ptr(a, a.n_ext, a.unit_shift, codes + lane * 16)), c);
    sw[lane] = (uint8_t)(e + kMx8ScaleBias);
    store_scales<NT>(a, scales, ne, lane, sw);
}

// One MXFP4 get tile: the reverse; local stores are nontemporal.
template <bool BF16, class A>
__device__ __forceinline__ void get_tile_mx4(const A &a, char *lin, uint64_t codes, uint64_t scales,
                                             uint32_t ne, uint32_t lane) {
    const uint32_t el = lane * 32;
    if (el >= ne) return;
    const u32x4 c = __builtin_nontemporal_load(
        reinterpret_cast<const u32x4 *>(stripe_ptr(a, a.n_ext, a.unit_shift, codes + lane * 16)));
    const uint8_t sb = *reinterpret_cast<const uint8_t *>(stripe_ptr(a, a.n_ext, a.unit_shift, scales + lane));
    const float scale = mx4_scale_operand((int)sb - kMx8ScaleBias);
    u32x4 *d = reinterpret_cast<u32x4 *>(lin + 2ull * el);
#pragma unroll
    for (int k = 0; k < 4; k++) store16<true>(d + k, mx4_unpack8<BF16>(c[k], scale));
}

// One tile of either format, direction and element type: `dtype` is the op's
// enum ocm_quant_dtype | enum ocm_quant_format word, `put` its direction, both wave-uniform.
template <bool PUT_NT, class A>
__device__ __forceinline__ void quant_tile(const A &a, char *lin, uint64_t codes, uint64_t scales, uint32_t ne,
                                           uint32_t dtype, uint32_t put, uint32_t lane, uint8_t *sw) {
    const bool bf16 = (dtype & kQuantElemMask) == kMx8Bf16;
    if (quant_code_shift(dtype)) {
        if (put) {
            if (bf16)
                put_tile_mx4<true, PUT_NT>(a, lin, codes, scales, ne, lane, sw);
            else
                put_tile_mx4<false, PUT_NT>(a, lin, codes, scales, ne, lane, sw);
        } else {
            if (bf16)
                get_tile_mx4<true>(a, lin, codes, scales, ne, lane);
            else
                get_tile_mx4<false>(a, lin, codes, scales, ne, lane);
        }
    } else if (put) {
        if (bf16)
            put_tile<true, PUT_NT>(a, lin, codes, scales, ne, lane, sw);
        else
            put_tile<false, PUT_NT>(a, lin, codes, scales, ne, lane, sw);
    } else {
        if (bf16)
            get_tile<true>(a, lin, codes, scales, ne, lane);
        else
            get_tile<false>(a, lin, codes, scales, ne, lane);
    }
}

}  // namespace

}  // namespace ocm
