// What the gfx950 packed fp4 converts do, against the MXFP4 rule of ocm/mx4.h (the host
// codec, which the torch oracle defines): rounding, saturation, the nibble order, which
// bits of the scale operand count, and the narrowing of the 16-bit forms.
//
//   fp4_cvt_probe [out.json]
//
// Encode, for every scale byte s = 0..254 (e = s - 127, operand s << 23) and every 16-bit
// pattern h that is finite in the element type: the code of h beside the code of 1.0, by
//   v_cvt_scalef32_pk_fp4_bf16 / _f16 (h as it is) and _f32 (h widened),
// against mx4_f32_to_e2m1(widen(h) * 2^-e). Mismatches are counted apart for inputs the
// rule can meet (|h * 2^-e| <= 6) and for those past it (the converts must only saturate).
// Decode, for every s and every code byte: both elements by
//   v_cvt_scalef32_pk_bf16_fp4 / _f16_fp4 / _f32_fp4 (the last narrowed by the host),
// against narrow(value(code) * 2^e). One JSON object per form; "ok" is the verdict the
// tile bodies (csrc/src/kernels/quant_tile.h) rest on.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <string>
#include <vector>

#include "ocm/mx4.h"

using namespace ocm;

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));

#define HIP_OK(x)                                                                  \
    do {                                                                           \
        hipError_t e_ = (x);                                                       \
        if (e_ != hipSuccess) {                                                    \
            std::fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_));          \
            return 2;                                                              \
        }                                                                          \
    } while (0)

constexpr uint32_t kScales = 255, kPatterns = 65536;
enum Form { kBf16 = 0, kF16 = 1, kF32FromBf16 = 2, kF32FromF16 = 3 };

__device__ inline float scale_operand(uint32_t s) { return __builtin_bit_cast(float, s << 23); }

// out[s * 65536 + h]: byte 1 of the result (sel 1) when h is the first element and 1.0 the second
// in the low byte of the entry; the high byte holds the swapped order, written with sel 2.
__global__ void encode_kernel(int form, uint16_t *out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= kScales * kPatterns) return;
    const uint32_t s = i >> 16, h = i & 0xffffu;
    const float scale = scale_operand(s);
    uint32_t d = 0xa5a5a5a5u;
    if (form == kBf16) {
        const uint32_t one = 0x3f80u;
        d = __builtin_amdgcn_cvt_scalef32_pk_fp4_bf16(d, __builtin_bit_cast(bf16x2, h | (one << 16)), scale, 1);
        d = __builtin_amdgcn_cvt_scalef32_pk_fp4_bf16(d, __builtin_bit_cast(bf16x2, one | (h << 16)), scale, 2);
    } else if (form == kF16) {
        const uint32_t one = 0x3c00u;
        d = __builtin_amdgcn_cvt_scalef32_pk_fp4_f16(d, __builtin_bit_cast(f16x2, h | (one << 16)), scale, 1);
        d = __builtin_amdgcn_cvt_scalef32_pk_fp4_f16(d, __builtin_bit_cast(f16x2, one | (h << 16)), scale, 2);
    } else {
        const float x = form == kF32FromBf16 ? __builtin_bit_cast(float, h << 16) : (float)__builtin_bit_cast(_Float16, (uint16_t)h);
        d = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(d, x, 1.0f, scale, 1);
        d = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(d, 1.0f, x, scale, 2);
    }
    // bytes 0 and 3 must be untouched
    out[i] = (d & 0xff0000ffu) == 0xa50000a5u ? (uint16_t)(d >> 8) : (uint16_t)0xffffu;
}

// out[(s * 256 + b) * 2 + k]: element k of code byte b (in byte 2 of the source, sel 2), as fp32 bits
// (form 2) or as the 16-bit pattern.
__global__ void decode_kernel(int form, uint32_t *out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= kScales * 256) return;
    const uint32_t s = i >> 8, b = i & 0xffu;
    const float scale = scale_operand(s);
    const uint32_t src = 0x5a00005au | (b << 16) | ((~b & 0xffu) << 8);
    if (form == kBf16) {
        const uint32_t r = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(src, scale, 2));
        out[2 * i] = r & 0xffffu;
        out[2 * i + 1] = r >> 16;
    } else if (form == kF16) {
        const uint32_t r = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(src, scale, 2));
        out[2 * i] = r & 0xffffu;
        out[2 * i + 1] = r >> 16;
    } else {
        const f32x2 r = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(src, scale, 2);
        out[2 * i] = __builtin_bit_cast(uint32_t, r[0]);
        out[2 * i + 1] = __builtin_bit_cast(uint32_t, r[1]);
    }
}

static bool finite16(uint32_t h, bool bf16) { return bf16 ? (h & 0x7f80u) != 0x7f80u : (h & 0x7c00u) != 0x7c00u; }

int main(int argc, char **argv) {
    const char *form_names[4] = {"pk_fp4_bf16", "pk_fp4_f16", "pk_fp4_f32(bf16 values)", "pk_fp4_f32(fp16 values)"};
    std::string json = "{\n";
    uint16_t *d_enc;
    uint32_t *d_dec;
    HIP_OK(hipMalloc(&d_enc, (size_t)kScales * kPatterns * 2));
    HIP_OK(hipMalloc(&d_dec, (size_t)kScales * 256 * 2 * 4));
    std::vector<uint16_t> enc((size_t)kScales * kPatterns);
    std::vector<uint32_t> dec((size_t)kScales * 256 * 2);
    bool all_ok = true;
    for (int form = 0; form < 4; form++) {
        hipLaunchKernelGGL(encode_kernel, dim3(kScales * kPatterns / 256), dim3(256), 0, 0, form, d_enc);
        HIP_OK(hipGetLastError());
        HIP_OK(hipMemcpy(enc.data(), d_enc, enc.size() * 2, hipMemcpyDeviceToHost));
        const bool bf16 = form == kBf16 || form == kF32FromBf16;
        const uint32_t dtype = bf16 ? kMx8Bf16 : kMx8Fp16;
        uint64_t bad_in = 0, bad_past = 0, bad_order = 0, n_in = 0;
        char first[256] = "";
        for (uint32_t s = 0; s < kScales; s++) {
            const int e = (int)s - kMx8ScaleBias;
            const uint32_t one = mx4_f32_to_e2m1(mx8_float_bits(std::ldexp(1.0f, -e)));
            for (uint32_t h = 0; h < kPatterns; h++) {
                if (!finite16(h, bf16)) continue;
                const float y = std::ldexp(mx8_widen((uint16_t)h, dtype), -e);  // exact, or rounded far below 0.25
                const uint32_t want = mx4_f32_to_e2m1(mx8_float_bits(y));
                const uint32_t got = enc[(size_t)s * kPatterns + h];
                const bool in_rule = std::fabs(y) <= 6.0f;
                n_in += in_rule;
                if (got == 0xffffu || (got & 0xf0u) != (one << 4) || ((got >> 8) & 0x0fu) != one || ((got >> 12) & 15u) != (got & 15u)) {
                    // the fixed 1.0 is not where the element order says, or the two orders disagree
                    bad_order++;
                }
                if ((got & 15u) != want) {
                    (in_rule ? bad_in : bad_past)++;
                    if (in_rule && !first[0])
                        std::snprintf(first, sizeof(first), "s=%u h=0x%04x y=%a got=%u want=%u", s, h, (double)y, got & 15u, want);
                }
            }
        }
        const bool ok = bad_in == 0 && bad_past == 0 && bad_order == 0;
        all_ok = all_ok && ok;
        char line[640];
        std::snprintf(line, sizeof(line),
                      " \"encode %s\": {\"ok\": %s, \"inputs_in_rule\": %llu, \"mismatch_in_rule\": %llu, \"mismatch_past_6\": %llu, "
                      "\"element_order_or_untouched_bytes_wrong\": %llu, \"first\": \"%s\"},\n",
                      form_names[form], ok ? "true" : "false", (unsigned long long)n_in, (unsigned long long)bad_in,
                      (unsigned long long)bad_past, (unsigned long long)bad_order, first);
        json += line;
    }
    const char *dec_names[3] = {"pk_bf16_fp4", "pk_f16_fp4", "pk_f32_fp4"};
    for (int form = 0; form < 3; form++) {
        hipLaunchKernelGGL(decode_kernel, dim3(kScales), dim3(256), 0, 0, form, d_dec);
        HIP_OK(hipGetLastError());
        HIP_OK(hipMemcpy(dec.data(), d_dec, dec.size() * 4, hipMemcpyDeviceToHost));
        uint64_t bad[2] = {0, 0};  // form 2: [as fp32, narrowed to bf16 and fp16]
        char first[256] = "";
        for (uint32_t s = 0; s < kScales; s++) {
            const int e = (int)s - kMx8ScaleBias;
            for (uint32_t b = 0; b < 256; b++)
                for (uint32_t k = 0; k < 2; k++) {
                    const float v = std::ldexp(mx8_bits_float(mx4_e2m1_to_f32_bits((b >> (4 * k)) & 15u)), e);
                    const uint32_t got = dec[((size_t)s * 256 + b) * 2 + k];
                    uint32_t want;
                    bool wrong;
                    if (form == 2) {
                        want = mx8_float_bits(v);
                        wrong = got != want;
                        const float g = mx8_bits_float(got);
                        bad[1] += mx8_f32_to_bf16(g) != mx8_f32_to_bf16(v) || mx8_f32_to_fp16(g) != mx8_f32_to_fp16(v);
                    } else {
                        want = mx8_narrow(v, form == kBf16 ? kMx8Bf16 : kMx8Fp16);
                        wrong = got != want;
                    }
                    bad[0] += wrong;
                    if (wrong && !first[0])
                        std::snprintf(first, sizeof(first), "s=%u byte=0x%02x element=%u got=0x%x want=0x%x", s, b, k, got, want);
                }
        }
        const bool ok = bad[0] == 0;
        all_ok = all_ok && ok;
        char line[512];
        std::snprintf(line, sizeof(line), " \"decode %s\": {\"ok\": %s, \"outputs\": %u, \"mismatch\": %llu%s, \"first\": \"%s\"},\n",
                      dec_names[form], ok ? "true" : "false", kScales * 512,
                      (unsigned long long)bad[0],
                      form == 2 ? (", \"mismatch_after_narrowing\": " + std::to_string(bad[1])).c_str() : "", first);
        json += line;
    }
    hipDeviceProp_t prop;
    HIP_OK(hipGetDeviceProperties(&prop, 0));
    json += std::string(" \"device\": \"") + prop.gcnArchName + "\",\n \"all_ok\": " + (all_ok ? "true" : "false") + "\n}\n";
    std::fputs(json.c_str(), stdout);
    if (argc > 1) {
        FILE *f = std::fopen(argv[1], "w");
        if (!f) return 2;
        std::fputs(json.c_str(), f);
        std::fclose(f);
    }
    HIP_OK(hipFree(d_enc));
    HIP_OK(hipFree(d_dec));
    return 0;
}
