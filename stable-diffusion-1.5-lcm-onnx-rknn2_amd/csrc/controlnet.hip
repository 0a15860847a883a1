// The ControlNet hint stack on gfx950: ControlNetConditioningEmbedding of diffusers' ControlNetModel -- eight 3x3
// convolutions with 3 .. 256 input channels on the full-resolution hint image, SiLU after all but the last.
//
// These layers are too narrow for the implicit-GEMM tiles of igemm.hip (Cin, Cout multiples of 64): at 16 .. 96 channels a
// 128-wide N tile would be mostly padding, and the layers are bound by the activation traffic of the 512^2 / 256^2 levels, not
// by the matrix pipe.  Both kernels here follow conv_c4_kernel (misc.hip): the weights of the workgroup's output channels
// sit in LDS in fragment order, a wave owns 16 consecutive output pixels of the flattened (b, y, x) order and builds its B
// operand (the pixels' K slots, tap major / channel minor) in registers straight from global memory -- one 16-byte load per
// 8 slots, zero outside the image -- then walks the channel tiles with v_mfma_f32_16x16x32_f16:
//   A = weights (rows = output channels), lane (n, q) holds channel n, K slots 32 s + 8 q .. + 7
//   B = pixels,                           lane (n, q) holds pixel n,   K slots 32 s + 8 q .. + 7
//   D: lane (n, q) = pixel n, channels 4 q .. 4 q + 3  ->  one 8-byte store per 16 x 16 tile.
// fp16 operands, fp32 accumulation (one chain per output in slot order: no K split, so a pixel's bits depend on nothing but
// its own inputs), bias / SiLU in fp32 before the one fp16 rounding.  Stride 2 with padding 1 gives ceil(n / 2) outputs.
#include "common.h"

// ---------------------------------------------------------------------------------------------
// Layer 0: uint8 RGB [B,H,W,3] -> fp16 [B,H,W,Cout], x / 255 applied on the fly.  K = 27; the fp32 value x / 255 enters as
// fp16 hi + fp16 lo against the same weights (slots 0..26 hi, 27..53 lo, 54..63 zero): two MFMAs per 16 x 16 tile and the
// hint keeps ~22 bits, so no fp16 copy of the image exists anywhere and none of its rounding either.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void hint_conv_u8_kernel(const uint8_t* __restrict__ in, const half_t* __restrict__ W,
                                                           const half_t* __restrict__ bias, half_t* __restrict__ out,
                                                           int B, int H, int Wd, int Cout, int silu) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    for (int i = threadIdx.x; i < Cout * 8; i += 256) {
        const int sg = i / Cout, co = i - sg * Cout;
        half_t e[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int k = sg * 8 + j;
            e[j] = k < 54 ? W[co * 27 + (k >= 27 ? k - 27 : k)] : (half_t)0;
        }
        *reinterpret_cast<h8*>(smem + (sg * Cout + co) * 16) = (h8){e[0], e[1], e[2], e[3], e[4], e[5], e[6], e[7]};
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n = lane & 15, q = lane >> 4;
    const long long npix = (long long)B * H * Wd;
    const int ntile = (int)((npix + 15) >> 4), plane = H * Wd;
    for (int t = blockIdx.x * 4 + wave; t < ntile; t += gridDim.x * 4) {
        const long long pix = (long long)t * 16 + n;
        const bool live = pix < npix;
        const int b = (int)(pix / plane), rem = (int)(pix - (long long)b * plane);
        const int y = rem / Wd, x = rem - y * Wd;
        h8 xf[2];
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            half_t e[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int k = 32 * s + 8 * q + j;
                const int part = k >= 54 ? 2 : (k >= 27 ? 1 : 0), r = k - 27 * (k >= 54 ? 2 : (k >= 27 ? 1 : 0));
                const int tap = r / 3, c = r - 3 * tap;
                const int iy = y + tap / 3 - 1, ix = x + tap % 3 - 1;
                float v = 0.f;
                if (live && part < 2 && iy >= 0 && iy < H && ix >= 0 && ix < Wd)
                    v = (float)in[(((long long)b * H + iy) * Wd + ix) * 3 + c] / 255.0f;
                const half_t hi = (half_t)v;
                e[j] = part == 0 ? hi : (half_t)(v - (float)hi);
            }
            xf[s] = (h8){e[0], e[1], e[2], e[3], e[4], e[5], e[6], e[7]};
        }
        half_t* orow = out + pix * Cout + 4 * q;
        for (int ct = 0; ct < Cout; ct += 16) {
            f4 acc = {0.f, 0.f, 0.f, 0.f};
            if (bias) {
                const h4 b4 = *reinterpret_cast<const h4*>(bias + ct + 4 * q);
                acc = (f4){(float)b4[0], (float)b4[1], (float)b4[2], (float)b4[3]};
            }
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const h8 wf = *reinterpret_cast<const h8*>(smem + (((s * 4 + q) * Cout) + ct + n) * 16);
                acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf, xf[s], acc, 0, 0, 0);
            }
            if (live) {
                if (silu) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) acc[i] = silu_f(acc[i]);
                }
                *reinterpret_cast<h4*>(orow + ct) = (h4){(half_t)acc[0], (half_t)acc[1], (half_t)acc[2], (half_t)acc[3]};
            }
        }
    }
}

extern "C" int lcm_hint_conv_u8(const void* in, const void* W, const void* bias, void* out, int B, int H, int Wd, int Cout,
                                int silu, void* stream) {
    LCM_REQUIRE(in && W && out, "hint_conv_u8: null pointer");
    LCM_REQUIRE(B > 0 && H > 0 && Wd > 0 && Cout > 0 && Cout % 16 == 0 && Cout * 128 <= 64 * 1024, "hint_conv_u8: bad shape (Cout %d)", Cout);
    LCM_REQUIRE((long long)B * H * Wd < (1ll << 31) - 16, "hint_conv_u8: input too large");
    const long long ntile = ((long long)B * H * Wd + 15) / 16;
    const int grid = (int)((ntile + 3) / 4 < 2048 ? (ntile + 3) / 4 : 2048);
    hipLaunchKernelGGL(hint_conv_u8_kernel, dim3(grid), dim3(256), Cout * 128, (hipStream_t)stream, (const uint8_t*)in,
                       (const half_t*)W, (const half_t*)bias, (half_t*)out, B, H, Wd, Cout, silu);
    LCM_CHECK_LAUNCH("hint_conv_u8");
    return LCM_OK;
}

// ---------------------------------------------------------------------------------------------
// Layers 1 .. 6: fp16 [B,H,W,CIN] -> fp16 [B,Ho,Wo,Cout], CIN in {16, 32, 96}, stride 1 or 2.  K = 9 CIN padded to a multiple
// of 32 (CIN % 8 == 0: an 8-slot chunk never straddles a tap, and is either all real or all padding).  blockIdx.y picks CT of
// the Cout channels, so that their weights (CT x KP fp16) fit the default 64 KB of LDS; the pixel fragments (KP / 32 registers
// quads, 108 VGPRs at CIN = 96) are loaded once per tile and reused for every channel tile.
// ---------------------------------------------------------------------------------------------
template <int CIN>
__global__ __launch_bounds__(256) void hint_conv_kernel(const half_t* __restrict__ in, const half_t* __restrict__ W,
                                                        const half_t* __restrict__ bias, half_t* __restrict__ out,
                                                        int B, int H, int Wd, int Ho, int Wo, int Cout, int CT, int stride,
                                                        int silu) {
    constexpr int K = 9 * CIN, NS = (K + 31) / 32, NG = NS * 4;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int c_base = blockIdx.y * CT;
    for (int i = threadIdx.x; i < CT * NG; i += 256) {
        const int g = i / CT, co = i - g * CT;
        h8 v = {0, 0, 0, 0, 0, 0, 0, 0};
        if (8 * g < K) v = *reinterpret_cast<const h8*>(W + (long long)(c_base + co) * K + 8 * g);
        *reinterpret_cast<h8*>(smem + (g * CT + co) * 16) = v;
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n = lane & 15, q = lane >> 4;
    const long long npix = (long long)B * Ho * Wo;
    const int ntile = (int)((npix + 15) >> 4), plane = Ho * Wo;
    for (int t = blockIdx.x * 4 + wave; t < ntile; t += gridDim.x * 4) {
        const long long pix = (long long)t * 16 + n;
        const bool live = pix < npix;
        const int b = (int)(pix / plane), rem = (int)(pix - (long long)b * plane);
        const int yo = rem / Wo, xo = rem - yo * Wo;
        const int yc = yo * stride, xc = xo * stride;
        h8 xf[NS];
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const int k0 = 8 * (4 * s + q);
            const int tap = k0 / CIN, c0 = k0 - tap * CIN;
            const int iy = yc + tap / 3 - 1, ix = xc + tap % 3 - 1;
            h8 v = {0, 0, 0, 0, 0, 0, 0, 0};
            if (live && k0 < K && iy >= 0 && iy < H && ix >= 0 && ix < Wd)
                v = *reinterpret_cast<const h8*>(in + (((long long)b * H + iy) * Wd + ix) * CIN + c0);
            xf[s] = v;
        }
        half_t* orow = out + pix * Cout + c_base + 4 * q;
        for (int ct = 0; ct < CT; ct += 16) {
            f4 acc = {0.f, 0.f, 0.f, 0.f};
            if (bias) {
                const h4 b4 = *reinterpret_cast<const h4*>(bias + c_base + ct + 4 * q);
                acc = (f4){(float)b4[0], (float)b4[1], (float)b4[2], (float)b4[3]};
            }
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                const h8 wf = *reinterpret_cast<const h8*>(smem + (((s * 4 + q) * CT) + ct + n) * 16);
                acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf, xf[s], acc, 0, 0, 0);
            }
            if (live) {
                if (silu) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) acc[i] = silu_f(acc[i]);
                }
                *reinterpret_cast<h4*>(orow + ct) = (h4){(half_t)acc[0], (half_t)acc[1], (half_t)acc[2], (half_t)acc[3]};
            }
        }
    }
}

template <int CIN>
static int launch_hint_conv(const void* in, const void* W, const void* bias, void* out, int B, int H, int Wd, int Cout,
                            int stride, int silu, hipStream_t stream) {
    constexpr int KP = (9 * CIN + 31) / 32 * 32;
    int CT = 0;                       // the most channels per workgroup whose weights fit 64 KB: a function of the layer alone
    for (int c = Cout; c >= 16; c -= 16)
        if (Cout % c == 0 && c * KP * 2 <= 64 * 1024) { CT = c; break; }
    LCM_REQUIRE(CT > 0, "hint_conv: no channel split for Cin=%d Cout=%d", CIN, Cout);
    const int Ho = stride == 2 ? (H + 1) / 2 : H, Wo = stride == 2 ? (Wd + 1) / 2 : Wd;
    const long long ntile = ((long long)B * Ho * Wo + 15) / 16;
    const int grid = (int)((ntile + 3) / 4 < 2048 ? (ntile + 3) / 4 : 2048);
    hipLaunchKernelGGL(hint_conv_kernel<CIN>, dim3(grid, Cout / CT), dim3(256), CT * KP * 2, stream, (const half_t*)in,
                       (const half_t*)W, (const half_t*)bias, (half_t*)out, B, H, Wd, Ho, Wo, Cout, CT, stride, silu);
    LCM_CHECK_LAUNCH("hint_conv");
    return LCM_OK;
}

extern "C" int lcm_hint_conv_f16(const void* in, const void* W, const void* bias, void* out, int B, int H, int Wd, int Cin,
                                 int Cout, int stride, int silu, void* stream) {
    LCM_REQUIRE(in && W && out, "hint_conv: null pointer");
    LCM_REQUIRE(B > 0 && H > 0 && Wd > 0 && Cout > 0 && Cout % 16 == 0 && (stride == 1 || stride == 2),
                "hint_conv: bad shape (Cout %d, stride %d)", Cout, stride);
    LCM_REQUIRE((long long)B * H * Wd * Cin < (1ll << 40) && (long long)B * H * Wd < (1ll << 31) - 16, "hint_conv: input too large");
    switch (Cin) {
    case 16: return launch_hint_conv<16>(in, W, bias, out, B, H, Wd, Cout, stride, silu, (hipStream_t)stream);
    case 32: return launch_hint_conv<32>(in, W, bias, out, B, H, Wd, Cout, stride, silu, (hipStream_t)stream);
    case 96: return launch_hint_conv<96>(in, W, bias, out, B, H, Wd, Cout, stride, silu, (hipStream_t)stream);
    default:
        lcm_set_error("hint_conv: Cin=%d is none of the hint stack's widths (16, 32, 96); wider layers go through lcm_conv3x3_f16", Cin);
        return LCM_EINVAL;
    }
}

// ---------------------------------------------------------------------------------------------
// The ControlNet's conv_in: conv3x3 from the fp32 NCHW latents (Cin = 4) + bias + the hint embedding, one launch per step.
// conv_c4_kernel's scheme (misc.hip) without its pre-transform: the fp32 input enters as fp16 hi + lo parts (K slots 0..35 hi,
// 36..71 lo against the same weights, 72..95 zero; three MFMAs per 16 x 16 tile, ~22 bits of the input kept); the residual
// res fp16 [B,H,W,Cout] is added in fp32 before the one fp16 rounding of the output.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void conv_c4_res_kernel(const float* __restrict__ in, const half_t* __restrict__ W,
                                                          const half_t* __restrict__ bias, const half_t* __restrict__ res,
                                                          half_t* __restrict__ out, int B, int H, int Wd, int Cout) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    for (int i = threadIdx.x; i < Cout * 12; i += 256) {
        const int sg = i / Cout, co = i - sg * Cout;
        h4 v[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int s4 = sg * 2 + h;                       // 4-slot group: part = s4 / 9 (hi, lo, zero), tap = s4 % 9
            v[h] = (h4){0, 0, 0, 0};
            if (s4 < 18) v[h] = *reinterpret_cast<const h4*>(W + co * 36 + (s4 % 9) * 4);
        }
        *reinterpret_cast<h8*>(smem + (sg * Cout + co) * 16) = (h8){v[0][0], v[0][1], v[0][2], v[0][3], v[1][0], v[1][1], v[1][2], v[1][3]};
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n = lane & 15, q = lane >> 4;
    const int npix = B * H * Wd, ntile = (npix + 15) >> 4, plane = H * Wd;
    for (int t = blockIdx.x * 4 + wave; t < ntile; t += gridDim.x * 4) {
        const int pix = t * 16 + n;
        const bool live = pix < npix;
        const int b = pix / plane, rem = pix - b * plane;
        const int y = rem / Wd, x = rem - y * Wd;
        h8 xf[3];
#pragma unroll
        for (int s = 0; s < 3; ++s) {
            half_t e[8];
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int s4 = 8 * s + 2 * q + h;
                const int part = s4 >= 18 ? 2 : (s4 >= 9 ? 1 : 0), tap = s4 - 9 * part;
                const int iy = y + tap / 3 - 1, ix = x + tap % 3 - 1;
                float z[4] = {0.f, 0.f, 0.f, 0.f};
                if (live && part < 2 && iy >= 0 && iy < H && ix >= 0 && ix < Wd) {
#pragma unroll
                    for (int c = 0; c < 4; ++c) z[c] = in[((b * 4 + c) * H + iy) * Wd + ix];
                }
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const half_t hi = (half_t)z[c];
                    e[h * 4 + c] = part == 0 ? hi : (half_t)(z[c] - (float)hi);
                }
            }
            xf[s] = (h8){e[0], e[1], e[2], e[3], e[4], e[5], e[6], e[7]};
        }
        const long long o0 = (long long)pix * Cout + 4 * q;
        for (int ct = 0; ct < Cout; ct += 16) {
            f4 acc = {0.f, 0.f, 0.f, 0.f};
            if (bias) {
                const h4 b4 = *reinterpret_cast<const h4*>(bias + ct + 4 * q);
                acc = (f4){(float)b4[0], (float)b4[1], (float)b4[2], (float)b4[3]};
            }
#pragma unroll
            for (int s = 0; s < 3; ++s) {
                const h8 wf = *reinterpret_cast<const h8*>(smem + (((s * 4 + q) * Cout) + ct + n) * 16);
                acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf, xf[s], acc, 0, 0, 0);
            }
            if (live) {
                const h4 r4 = *reinterpret_cast<const h4*>(res + o0 + ct);
                *reinterpret_cast<h4*>(out + o0 + ct) = (h4){(half_t)(acc[0] + (float)r4[0]), (half_t)(acc[1] + (float)r4[1]),
                                                             (half_t)(acc[2] + (float)r4[2]), (half_t)(acc[3] + (float)r4[3])};
            }
        }
    }
}

extern "C" int lcm_conv3x3_c4_res_f32in(const void* in, const void* W, const void* bias, const void* res, void* out, int B,
                                        int H, int Wd, int Cout, void* stream) {
    LCM_REQUIRE(in && W && res && out, "conv_c4_res: null pointer");
    LCM_REQUIRE(B > 0 && H > 0 && Wd > 0 && Cout % 16 == 0 && Cout * 192 <= 160 * 1024, "conv_c4_res: bad shape (Cout %d)", Cout);
    LCM_REQUIRE((long long)B * 4 * H * Wd < (1ll << 31), "conv_c4_res: input too large");
    const int smem = Cout * 192;
    static LcmDevOnce attr_once;
    if (auto once_guard = attr_once.first()) {
        once_guard.check(hipFuncSetAttribute(reinterpret_cast<const void*>(&conv_c4_res_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    }
    const long long ntile = ((long long)B * H * Wd + 15) / 16;
    const int grid = (int)((ntile + 3) / 4 < 512 ? (ntile + 3) / 4 : 512);
    hipLaunchKernelGGL(conv_c4_res_kernel, dim3(grid), dim3(256), smem, (hipStream_t)stream, (const float*)in, (const half_t*)W,
                       (const half_t*)bias, (const half_t*)res, (half_t*)out, B, H, Wd, Cout);
    LCM_CHECK_LAUNCH("conv_c4_res");
    return LCM_OK;
}
