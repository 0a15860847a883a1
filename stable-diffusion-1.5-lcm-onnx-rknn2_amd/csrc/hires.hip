// Hires fix, the hand-over between two sizes: the denoised latents of the low-resolution pass are
// upscaled with one of A1111's latent upscalers and re-noised to the first timestep of the second pass's strength-cut schedule,
// in one launch (include/lcm_hip.h, lcm_latents_upscale_renoise).
//
// What decides the numbers.  A source coordinate is the exact rational ((2 dst + 1) in - out) / (2 out) of torch's
// align_corners=False mapping (dst + 0.5) in / out - 0.5: its floor comes from integer division and its fraction is ONE
// correctly rounded fp32 division of two integers below 2^24, never a product with a rounded in / out.  Weights are therefore a
// function of (dst, in, out) alone -- not of the batch, the lane or the launch shape -- and every output element is computed
// by one thread from at most 4 x 4 taps in a fixed order.  The re-noise is lcm_latents_renoise's expression (one rounded
// product, one fused multiply-add): at H == h, W == w the weights are exactly 1 and 0, taps of weight 0 are left out, and
// the output has that launch's bits.
#include "common.h"

#define LCM_UPSCALE_BILINEAR 0
#define LCM_UPSCALE_BICUBIC 1
#define LCM_UPSCALE_NEAREST_EXACT 2

namespace {
// torch's cubic convolution coefficients (UpSampleKernel: A = -0.75)
__device__ __forceinline__ float cubic_near(float x) {   // |x| <= 1
    const float A = -0.75f;
    return ((A + 2.0f) * x - (A + 3.0f)) * x * x + 1.0f;
}
__device__ __forceinline__ float cubic_far(float x) {    // 1 < |x| < 2
    const float A = -0.75f;
    return ((A * x - 5.0f * A) * x + 8.0f * A) * x - 4.0f * A;
}

// taps of output index d along one axis: n source indices (clamped into [0, in)) and their weights
template <int MODE>
__device__ __forceinline__ int axis_taps(int d, int in, int out, int (&idx)[4], float (&wt)[4]) {
    const int den = 2 * out;
    if (MODE == LCM_UPSCALE_NEAREST_EXACT) {             // floor((dst + 0.5) in / out)
        idx[0] = min(((2 * d + 1) * in) / den, in - 1);
        wt[0] = 1.0f;
        return 1;
    }
    const int num = (2 * d + 1) * in - out;              // source coordinate = num / den
    if (MODE == LCM_UPSCALE_BILINEAR) {                  // the coordinate is clamped at 0
        const int i0 = num > 0 ? num / den : 0;
        const int r = num > 0 ? num - i0 * den : 0;
        const float t = __fdiv_rn((float)r, (float)den);
        idx[0] = min(i0, in - 1);
        idx[1] = min(i0 + 1, in - 1);
        wt[0] = 1.0f - t;
        wt[1] = t;
        return 2;
    }
    // bicubic: the coordinate is not clamped (num >= in - out > -den), the four indices are
    const int fl = num >= 0 ? num / den : -1;
    const float t = __fdiv_rn((float)(num - fl * den), (float)den);
#pragma unroll
    for (int k = 0; k < 4; ++k) idx[k] = min(max(fl - 1 + k, 0), in - 1);
    wt[0] = cubic_far(t + 1.0f);
    wt[1] = cubic_near(t);
    wt[2] = cubic_near(1.0f - t);
    wt[3] = cubic_far(2.0f - t);
    return 4;
}

// One thread per output element (fp32 NCHW, 4-byte accesses coalesced across the wave: W need not be a multiple of 4).
// n = B * 4 * H * W < 2^30.  lat_dup: the other classifier-free-guidance half or null; x_up: the upscaled clean latents or null.
template <int MODE>
__global__ void latents_upscale_renoise_kernel(const float* __restrict__ x0, int h, int w, const float* __restrict__ noise,
                                               float sa, float sb, float* __restrict__ x_up, float* __restrict__ lat,
                                               float* __restrict__ lat_dup, int H, int W, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int ox = i % W, oy = (i / W) % H, plane = i / (W * H);
    int ix[4], iy[4];
    float wx[4], wy[4];
    const int nx = axis_taps<MODE>(ox, w, W, ix, wx);
    const int ny = axis_taps<MODE>(oy, h, H, iy, wy);
    const float* src = x0 + (long long)plane * h * w;
    float acc = 0.0f;
    bool first = true;
#pragma unroll
    for (int y = 0; y < 4; ++y) {
        if (y >= ny || wy[y] == 0.0f) continue;
        const float* row = src + iy[y] * w;
        float r = 0.0f;
        bool rfirst = true;
#pragma unroll
        for (int x = 0; x < 4; ++x) {
            if (x >= nx || wx[x] == 0.0f) continue;
            const float v = row[ix[x]];
            r = rfirst ? __fmul_rn(wx[x], v) : __fmaf_rn(wx[x], v, r);
            rfirst = false;
        }
        acc = first ? __fmul_rn(wy[y], r) : __fmaf_rn(wy[y], r, acc);
        first = false;
    }
    if (x_up) x_up[i] = acc;
    const float out = __fmaf_rn(sb, noise[i], __fmul_rn(sa, acc));   // lcm_latents_renoise's expression
    lat[i] = out;
    if (lat_dup) lat_dup[i] = out;
}
}  // namespace

extern "C" int lcm_latents_upscale_renoise(const void* x0, int h, int w, const void* noise, float sqrt_a, float sqrt_b, int mode,
                                           void* x_up, void* lat_out, int B, int H, int W, int dup, void* stream) {
    LCM_REQUIRE(x0 && noise && lat_out, "latents_upscale_renoise: null pointer");
    LCM_REQUIRE(mode == LCM_UPSCALE_BILINEAR || mode == LCM_UPSCALE_BICUBIC || mode == LCM_UPSCALE_NEAREST_EXACT,
                "latents_upscale_renoise: unknown mode %d (0 bilinear, 1 bicubic, 2 nearest-exact)", mode);
    LCM_REQUIRE(B > 0 && h > 0 && w > 0, "latents_upscale_renoise: bad shape B=%d h=%d w=%d", B, h, w);
    LCM_REQUIRE(H >= h && W >= w && (long long)H <= 4ll * h && (long long)W <= 4ll * w,
                "latents_upscale_renoise: target %dx%d outside [1, 4] x the source %dx%d", H, W, h, w);
    LCM_REQUIRE(H <= 16384 && W <= 16384 && (long long)B * 4 * H * W < (1ll << 30), "latents_upscale_renoise: shape too large");
    const int n = B * 4 * H * W;
    float* lat = (float*)lat_out;
    auto kern = mode == LCM_UPSCALE_BILINEAR ? latents_upscale_renoise_kernel<LCM_UPSCALE_BILINEAR>
              : mode == LCM_UPSCALE_BICUBIC  ? latents_upscale_renoise_kernel<LCM_UPSCALE_BICUBIC>
                                             : latents_upscale_renoise_kernel<LCM_UPSCALE_NEAREST_EXACT>;
    hipLaunchKernelGGL(kern, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, (const float*)x0, h, w, (const float*)noise,
                       sqrt_a, sqrt_b, (float*)x_up, lat, dup ? lat + n : (float*)nullptr, H, W, n);
    LCM_CHECK_LAUNCH("latents_upscale_renoise");
    return LCM_OK;
}
