// LCMScheduler.step for every prediction type of the model output (include/lcm_hip.h, lcm_scheduler_step_ex).
// The epsilon form is lcm_scheduler_step (misc.hip) itself, so its bits cannot change; this file adds the other two.
// Multi-pass refinement: lcm_latents_renoise and the hand-over form of the step, lcm_scheduler_step_handover.
#include "common.h"

#define LCM_PRED_EPSILON 0
#define LCM_PRED_V 1
#define LCM_PRED_SAMPLE 2

extern "C" int lcm_scheduler_step(const void* eps, const void* eps_uncond, float guidance, void* lat, const void* noise,
                                  const float* coef6, int last, int B, int h, int w, void* stream);

namespace {
struct StepCoef6 { float sa, sb, c_skip, c_out, sap, sbp; };

// m: fp32 NHWC model output (CFG first: m = m_u + g (m - m_u), as the epsilon kernel does); x0 from m by PRED; then
// den = c_out x0 + c_skip x and x <- last ? den : sap den + sbp noise.  lat / noise fp32 NCHW.
template <int PRED>
__global__ void scheduler_step_pred_kernel(const float* __restrict__ m, const float* __restrict__ m_u, float guidance,
                                           float* __restrict__ lat, const float* __restrict__ noise, StepCoef6 c, int last,
                                           int B, int h, int w) {
    static_assert(PRED == LCM_PRED_V || PRED == LCM_PRED_SAMPLE, "epsilon is lcm_scheduler_step");
    const int i = blockIdx.x * blockDim.x + threadIdx.x;   // NCHW index
    const int hw = h * w, n = B * 4 * hw;
    if (i >= n) return;
    const int pix = i % hw, ch = (i / hw) & 3, b = i / (4 * hw);
    const long long e = ((long long)b * hw + pix) * 4 + ch;   // NHWC
    float mv = m[e];
    if (m_u) { const float u = m_u[e]; mv = u + guidance * (mv - u); }
    const float x = lat[i];
    const float x0 = PRED == LCM_PRED_V ? c.sa * x - c.sb * mv : mv;
    const float den = c.c_out * x0 + c.c_skip * x;
    lat[i] = last ? den : c.sap * den + c.sbp * noise[i];
}

// x_t = sqrt_a x + sqrt_b n, one rounding for the product and one for the fused multiply-add: the expression is spelled with
// intrinsics so that the re-noise launch and the hand-over step give the same bits for the same operands (a refinement chain
// that starts from cached latents must equal the chain that ran through).
__device__ __forceinline__ float renoise1(float sa, float sb, float x, float n) { return __fmaf_rn(sb, n, __fmul_rn(sa, x)); }

// 16 bytes per lane; v counts float4.  lat_dup: second copy (the other classifier-free-guidance half) or null.
__global__ void latents_renoise_kernel(const float4* __restrict__ x0, const float4* __restrict__ noise, float sa, float sb,
                                       float4* __restrict__ lat, float4* __restrict__ lat_dup, int v) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= v) return;
    const float4 x = x0[i], n = noise[i];
    const float4 r = make_float4(renoise1(sa, sb, x.x, n.x), renoise1(sa, sb, x.y, n.y), renoise1(sa, sb, x.z, n.z),
                                 renoise1(sa, sb, x.w, n.w));
    lat[i] = r;
    if (lat_dup) lat_dup[i] = r;
}

// The last step of a refinement pass that another pass follows: den with the bits of the `last` form of the step kernels,
// stored to xk; lat <- re-noised den for the next pass's first timestep.  The step kernels leave the fusing of multiply and add
// to the compiler; what it chose there (guidance: fma(g, m - u, u); epsilon: fma(-sb, m, x) / sa; v: fma(-sb, m, sa x);
// den: fma(c_skip, x, c_out x0)) is spelled out here, so that a different choice in this kernel cannot change a chain's bits
// (tests/test_refine_gpu.py compares the two).  One thread per pixel: the model output's four channels are one 16-byte NHWC
// load, the NCHW planes are coalesced 4-byte accesses across the wave.
template <int PRED>
__global__ void scheduler_step_handover_kernel(const float4* __restrict__ m, const float4* __restrict__ m_u, float guidance,
                                               float* __restrict__ lat, float* __restrict__ lat_dup, const float* __restrict__ noise,
                                               float* __restrict__ xk, StepCoef6 c, float nsa, float nsb, int B, int hw) {
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
        const float x0 = PRED == LCM_PRED_EPSILON ? __fmaf_rn(-c.sb, mv[ch], x) / c.sa
                       : PRED == LCM_PRED_V     ? __fmaf_rn(-c.sb, mv[ch], __fmul_rn(c.sa, x)) : mv[ch];
        const float den = __fmaf_rn(c.c_skip, x, __fmul_rn(c.c_out, x0));
        xk[i] = den;
        const float r = renoise1(nsa, nsb, den, noise[i]);
        lat[i] = r;
        if (lat_dup) lat_dup[i] = r;
    }
}
}  // namespace

extern "C" int lcm_latents_renoise(const void* x0, const void* noise, float sqrt_a, float sqrt_b, void* lat_out, int B, int h,
                                   int w, int dup, void* stream) {
    LCM_REQUIRE(x0 && noise && lat_out, "latents_renoise: null pointer");
    LCM_REQUIRE(B > 0 && h > 0 && w > 0 && (long long)B * 4 * h * w < (1ll << 30), "latents_renoise: bad shape");
    LCM_REQUIRE(((uintptr_t)x0 | (uintptr_t)noise | (uintptr_t)lat_out) % 16 == 0, "latents_renoise: pointers must be 16-byte aligned");
    const int v = B * h * w;   // B * 4 * h * w floats as float4
    float4* lat = (float4*)lat_out;
    hipLaunchKernelGGL(latents_renoise_kernel, dim3((v + 255) / 256), dim3(256), 0, (hipStream_t)stream, (const float4*)x0,
                       (const float4*)noise, sqrt_a, sqrt_b, lat, dup ? lat + v : (float4*)nullptr, v);
    LCM_CHECK_LAUNCH("latents_renoise");
    return LCM_OK;
}

extern "C" int lcm_scheduler_step_handover(const void* eps, const void* eps_uncond, float guidance, void* lat, const void* noise,
                                           void* xk, const float* coef6, float next_sqrt_a, float next_sqrt_b, int prediction_type,
                                           int B, int h, int w, int dup, void* stream) {
    LCM_REQUIRE(prediction_type == LCM_PRED_EPSILON || prediction_type == LCM_PRED_V || prediction_type == LCM_PRED_SAMPLE,
                "scheduler_step_handover: unknown prediction type %d", prediction_type);
    LCM_REQUIRE(eps && lat && noise && xk && coef6, "scheduler_step_handover: null pointer");
    LCM_REQUIRE(B > 0 && h > 0 && w > 0 && (long long)B * 4 * h * w < (1ll << 30), "scheduler_step_handover: bad shape");
    LCM_REQUIRE(((uintptr_t)eps | (uintptr_t)eps_uncond) % 16 == 0, "scheduler_step_handover: model output must be 16-byte aligned");
    StepCoef6 c = {coef6[0], coef6[1], coef6[2], coef6[3], coef6[4], coef6[5]};
    const int hw = h * w, n = B * hw;
    auto kern = prediction_type == LCM_PRED_EPSILON ? scheduler_step_handover_kernel<LCM_PRED_EPSILON>
              : prediction_type == LCM_PRED_V     ? scheduler_step_handover_kernel<LCM_PRED_V>
                                                  : scheduler_step_handover_kernel<LCM_PRED_SAMPLE>;
    // dup: lat holds [other half | this half] (classifier-free guidance, rows [0,B) = negative prompt): the copy goes in front
    float* l = (float*)lat;
    hipLaunchKernelGGL(kern, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, (const float4*)eps, (const float4*)eps_uncond,
                       guidance, l, dup ? l - (long long)B * 4 * hw : (float*)nullptr, (const float*)noise, (float*)xk, c,
                       next_sqrt_a, next_sqrt_b, B, hw);
    LCM_CHECK_LAUNCH("scheduler_step_handover");
    return LCM_OK;
}

extern "C" int lcm_scheduler_step_ex(const void* eps, const void* eps_uncond, float guidance, void* lat, const void* noise,
                                     const float* coef6, int last, int prediction_type, int B, int h, int w, void* stream) {
    LCM_REQUIRE(prediction_type == LCM_PRED_EPSILON || prediction_type == LCM_PRED_V || prediction_type == LCM_PRED_SAMPLE,
                "scheduler_step: unknown prediction type %d", prediction_type);
    if (prediction_type == LCM_PRED_EPSILON)
        return lcm_scheduler_step(eps, eps_uncond, guidance, lat, noise, coef6, last, B, h, w, stream);
    LCM_REQUIRE(eps && lat && coef6 && (last || noise), "scheduler_step: null pointer");
    LCM_REQUIRE(B > 0 && h > 0 && w > 0, "scheduler_step: bad shape");
    StepCoef6 c = {coef6[0], coef6[1], coef6[2], coef6[3], coef6[4], coef6[5]};
    const int n = B * 4 * h * w;
    auto kern = prediction_type == LCM_PRED_V ? scheduler_step_pred_kernel<LCM_PRED_V> : scheduler_step_pred_kernel<LCM_PRED_SAMPLE>;
    hipLaunchKernelGGL(kern, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, (const float*)eps,
                       (const float*)eps_uncond, guidance, (float*)lat, (const float*)noise, c, last, B, h, w);
    LCM_CHECK_LAUNCH("scheduler_step");
    return LCM_OK;
}
