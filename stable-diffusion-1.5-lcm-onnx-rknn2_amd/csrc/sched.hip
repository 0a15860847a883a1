// LCMScheduler.step for every prediction type of the model output (include/lcm_hip.h, lcm_scheduler_step_ex).
// The epsilon form is lcm_scheduler_step (misc.hip) itself, so its bits cannot change; this file adds the other two.
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
}  // namespace

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
