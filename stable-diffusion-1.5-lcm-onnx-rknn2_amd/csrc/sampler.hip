// The step of the ordinary samplers (Euler, Euler a, DDIM, DPM++ 2M) as one linear form (include/lcm_hip.h, samplers):
//   x' = cx x + c0 x0 + c1 x0_prev + cn noise,   x0_prev <- x0
// with x0 from the model output by the prediction type.  The coefficients come from the host (samplers.py, float64 -> float32).
// One launch per step; under classifier-free guidance the new state goes to both halves in that launch.
#include "common.h"

#define LCM_PRED_EPSILON 0
#define LCM_PRED_V 1
#define LCM_PRED_SAMPLE 2

namespace {
struct SamplerCoef { float sa, sb, cx, c0, c1, cn; };

// One thread per latent pixel (b, pix), as scheduler_step_handover_kernel (sched.hip): the model output's four channels are one
// 16-byte NHWC load, the NCHW planes are coalesced 4-byte accesses across the wave.  Every operation is spelled with an
// intrinsic, in the order the header states; a pixel's value depends on its own operands only, so neither the batch size nor the
// position in the batch can change a request's bits.  c.c1 == 0 / c.cn == 0 are wave-uniform: x0_prev / noise are then not read.
template <int PRED>
__global__ void sampler_step_kernel(const float4* __restrict__ m, const float4* __restrict__ m_u, float guidance,
                                    float* __restrict__ lat, float* __restrict__ lat_dup, float* __restrict__ x0_prev,
                                    const float* __restrict__ noise, SamplerCoef c, int B, int hw) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;   // (b, pix)
    if (p >= B * hw) return;
    const int b = p / hw, pix = p - b * hw;
    const float4 m4 = m[p];
    float mv[4] = {m4.x, m4.y, m4.z, m4.w};
    if (m_u) {
        const float4 u4 = m_u[p];
        const float u[4] = {u4.x, u4.y, u4.z, u4.w};
#pragma unroll
        for (int ch = 0; ch < 4; ++ch) mv[ch] = __fmaf_rn(guidance, __fsub_rn(mv[ch], u[ch]), u[ch]);
    }
#pragma unroll
    for (int ch = 0; ch < 4; ++ch) {
        const long long i = ((long long)b * 4 + ch) * hw + pix;   // NCHW
        const float x = lat[i];
        const float x0 = PRED == LCM_PRED_EPSILON ? __fdiv_rn(__fmaf_rn(-c.sb, mv[ch], x), c.sa)
                       : PRED == LCM_PRED_V     ? __fmaf_rn(-c.sb, mv[ch], __fmul_rn(c.sa, x)) : mv[ch];
        float r = __fmaf_rn(c.cx, x, __fmul_rn(c.c0, x0));
        if (c.c1 != 0.0f) r = __fmaf_rn(c.c1, x0_prev[i], r);
        if (c.cn != 0.0f) r = __fmaf_rn(c.cn, noise[i], r);
        x0_prev[i] = x0;
        lat[i] = r;
        if (lat_dup) lat_dup[i] = r;
    }
}
}  // namespace

extern "C" int lcm_sampler_step(const void* eps, const void* eps_uncond, float guidance, void* lat, void* x0_prev, const void* noise,
                                float sa, float sb, float cx, float c0, float c1, float cn, int prediction_type, int B, int h, int w,
                                int dup, void* stream) {
    LCM_REQUIRE(prediction_type == LCM_PRED_EPSILON || prediction_type == LCM_PRED_V || prediction_type == LCM_PRED_SAMPLE,
                "sampler_step: unknown prediction type %d", prediction_type);
    LCM_REQUIRE(eps && lat && x0_prev, "sampler_step: null pointer");
    LCM_REQUIRE(cn == 0.0f || noise, "sampler_step: cn = %g needs a noise tensor", (double)cn);
    LCM_REQUIRE(B > 0 && h > 0 && w > 0 && (long long)B * 4 * h * w < (1ll << 30), "sampler_step: bad shape");
    LCM_REQUIRE(((uintptr_t)eps | (uintptr_t)eps_uncond) % 16 == 0, "sampler_step: model output must be 16-byte aligned");
    LCM_REQUIRE(((uintptr_t)lat | (uintptr_t)x0_prev | (uintptr_t)noise) % 4 == 0, "sampler_step: lat, x0_prev and noise must be 4-byte aligned");
    LCM_REQUIRE(prediction_type != LCM_PRED_EPSILON || sa != 0.0f, "sampler_step: sa = 0 with epsilon prediction");
    const SamplerCoef c = {sa, sb, cx, c0, c1, cn};
    const int hw = h * w, n = B * hw;
    auto kern = prediction_type == LCM_PRED_EPSILON ? sampler_step_kernel<LCM_PRED_EPSILON>
              : prediction_type == LCM_PRED_V     ? sampler_step_kernel<LCM_PRED_V>
                                                  : sampler_step_kernel<LCM_PRED_SAMPLE>;
    // dup: lat holds [other half | this half] (classifier-free guidance, rows [0,B) = negative prompt): the copy goes in front
    float* l = (float*)lat;
    hipLaunchKernelGGL(kern, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, (const float4*)eps, (const float4*)eps_uncond,
                       guidance, l, dup ? l - (long long)B * 4 * hw : (float*)nullptr, (float*)x0_prev, (const float*)noise, c, B, hw);
    LCM_CHECK_LAUNCH("sampler_step");
    return LCM_OK;
}
