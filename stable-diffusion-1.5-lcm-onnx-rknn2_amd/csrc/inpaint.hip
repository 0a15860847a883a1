// Inpainting (include/lcm_hip.h): the mask on the device (separable integer Gaussian blur + the 8 x 8
// reduction to the binary latent mask), the LCM step with the per-cell select between the stepped latents and the init
// picture's re-noised latents, and the integer overlay of the decoded picture over the uploaded one.  The whole mask path is
// integer arithmetic: every result here is defined bit for bit by the header, and tests/test_inpaint_gpu.py compares for equality.
#include "common.h"

#define LCM_PRED_EPSILON 0
#define LCM_PRED_V 1
#define LCM_PRED_SAMPLE 2
#define LCM_INPAINT_MAX_RADIUS 80   // mask_blur <= 32: int(2.5 * 32 + 0.5)

namespace {
struct StepCoef6 { float sa, sb, c_skip, c_out, sap, sbp; };

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }

// Four pixels x .. x + 3 of one row as a dword (little endian: pixel x in the low byte), edge replicated.  fast: the row base
// is 4-byte aligned (W % 4 == 0) -- x is a multiple of 4 in every caller -- so an interior dword is one aligned 4-byte load.
__device__ __forceinline__ uint32_t load4_clamped(const uint8_t* __restrict__ row, int x, int W, bool fast) {
    if (fast && x >= 0 && x + 3 < W) return *reinterpret_cast<const uint32_t*>(row + x);
    uint32_t d = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) d |= (uint32_t)row[clampi(x + q, 0, W - 1)] << (8 * q);
    return d;
}

__device__ __forceinline__ void store4(uint8_t* __restrict__ row, int x, int W, bool fast, const uint32_t acc[4]) {
    uint32_t o[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = (acc[j] + 32768u) >> 16;
    if (fast && x + 3 < W) {
        *reinterpret_cast<uint32_t*>(row + x) = o[0] | (o[1] << 8) | (o[2] << 16) | (o[3] << 24);
        return;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (x + j < W) row[x + j] = (uint8_t)o[j];
}

// Horizontal pass: t[y,x] = (sum_k w_k m[y, clamp(x + k - r)] + 32768) >> 16.  A block is 64 lanes x 4 rows; a lane owns the four
// pixels x0 .. x0 + 3 (one dword store).  Each row is staged into LDS as dwords that start at x = tile_x0 - r4, r4 = r rounded up
// to a multiple of 4, so that the staging loads are aligned; the off = r4 - r surplus bytes in front meet `off` zero weights
// (q[] = off zeros | w_0 .. w_2r | zeros).  Per staged dword a lane reads 4 bytes of pixels and one broadcast uint4 of weights:
// byte p of its window (p = 4 i + b) is tap n = p - j of output j, so it needs q[4 i - 3 .. 4 i + 3], a sliding window of 7.
#define HB_LANES 64
#define HB_ROWS 4
__global__ void __launch_bounds__(HB_LANES * HB_ROWS)
mask_blur_h_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, const uint32_t* __restrict__ w, int r, int H, int W) {
    extern __shared__ uint4 smem4[];
    const int off = (4 - (r & 3)) & 3, r4 = r + off;
    const int nd = (2 * r + 4 + off + 3) / 4;                    // dwords of a lane's window
    const int nq = 4 * nd;                                       // padded weight count, a multiple of 4
    const int rowdw = HB_LANES + nd;                             // staged dwords per row (the last lane's window ends at 63 + nd)
    uint32_t* q = reinterpret_cast<uint32_t*>(smem4);
    uint32_t* pix = q + nq;
    const int tid = threadIdx.y * HB_LANES + threadIdx.x;
    const int b = blockIdx.z, y0 = blockIdx.y * HB_ROWS, tx0 = blockIdx.x * (HB_LANES * 4);
    const bool fast = (W & 3) == 0;
    for (int n = tid; n < nq; n += HB_LANES * HB_ROWS) q[n] = (n >= off && n - off <= 2 * r) ? w[n - off] : 0u;
    for (int n = tid; n < HB_ROWS * rowdw; n += HB_LANES * HB_ROWS) {
        const int row = n / rowdw, d = n - row * rowdw;
        const int y = min(y0 + row, H - 1);
        pix[n] = load4_clamped(src + ((long long)b * H + y) * W, tx0 - r4 + 4 * d, W, fast);
    }
    __syncthreads();
    const int y = y0 + threadIdx.y, x0 = tx0 + 4 * threadIdx.x;
    if (y >= H || x0 >= W) return;
    const uint32_t* mine = pix + threadIdx.y * rowdw + threadIdx.x;
    uint32_t acc[4] = {0u, 0u, 0u, 0u};
    uint32_t win[7] = {0u, 0u, 0u, 0u, 0u, 0u, 0u};              // q[4 i - 3 .. 4 i + 3]
    for (int i = 0; i < nd; ++i) {
        const uint4 nq4 = smem4[i];                              // q[4 i .. 4 i + 3], the same address in every lane
        win[3] = nq4.x, win[4] = nq4.y, win[5] = nq4.z, win[6] = nq4.w;
        const uint32_t d = mine[i];
#pragma unroll
        for (int bq = 0; bq < 4; ++bq) {
            const uint32_t v = (d >> (8 * bq)) & 255u;
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[j] += win[3 + bq - j] * v;
        }
        win[0] = win[4], win[1] = win[5], win[2] = win[6];
    }
    store4(dst + ((long long)b * H + y) * W, x0, W, fast, acc);
}

// Vertical pass: the same sum down a column.  A block is 16 lanes x 16 rows and owns 64 columns x 32 rows; TH + 2 r rows of 16
// dwords are staged (row clamped), so the four row groups of a wave read 64 consecutive dwords.  A lane owns the dword
// x0 .. x0 + 3 of the rows ty and ty + 16.
#define VB_LANES 16
#define VB_ROWS 16
#define VB_TH 32
__global__ void __launch_bounds__(VB_LANES * VB_ROWS)
mask_blur_v_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, const uint32_t* __restrict__ w, int r, int H, int W) {
    extern __shared__ uint4 smem4[];
    const int nw = 2 * r + 1, nq = (nw + 3) & ~3;
    uint32_t* q = reinterpret_cast<uint32_t*>(smem4);
    uint32_t* pix = q + nq;
    const int tid = threadIdx.y * VB_LANES + threadIdx.x;
    const int b = blockIdx.z, y0 = blockIdx.y * VB_TH, tx0 = blockIdx.x * (VB_LANES * 4);
    const bool fast = (W & 3) == 0;
    const int rows = VB_TH + 2 * r;
    for (int n = tid; n < nw; n += VB_LANES * VB_ROWS) q[n] = w[n];
    for (int n = tid; n < rows * VB_LANES; n += VB_LANES * VB_ROWS) {
        const int row = n / VB_LANES, d = n - row * VB_LANES;
        const int y = clampi(y0 - r + row, 0, H - 1), x = tx0 + 4 * d;
        pix[n] = x < W ? load4_clamped(src + ((long long)b * H + y) * W, x, W, fast) : 0u;
    }
    __syncthreads();
    const int x0 = tx0 + 4 * threadIdx.x;
    if (x0 >= W) return;
#pragma unroll
    for (int m = 0; m < VB_TH / VB_ROWS; ++m) {
        const int ly = threadIdx.y + VB_ROWS * m, y = y0 + ly;
        if (y >= H) break;
        const uint32_t* mine = pix + ly * VB_LANES + threadIdx.x;
        uint32_t acc[4] = {0u, 0u, 0u, 0u};
        for (int k = 0; k < nw; ++k) {
            const uint32_t wk = q[k], d = mine[k * VB_LANES];
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[j] += wk * ((d >> (8 * j)) & 255u);
        }
        store4(dst + ((long long)b * H + y) * W, x0, W, fast, acc);
    }
}

// M[b,y,x] = 2 * (sum of the 8 x 8 block of alpha) >= 64 * 255.  One lane per latent cell, eight aligned 8-byte loads (W % 8 == 0).
__global__ void latent_mask_kernel(const uint8_t* __restrict__ alpha, uint8_t* __restrict__ latmask, int B, int h, int w) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;   // (b, y, x)
    if (p >= B * h * w) return;
    const int x = p % w, by = p / w;                       // by = b * h + y: the rows of the images are contiguous
    const uint2* row = reinterpret_cast<const uint2*>(alpha + ((long long)by * 8) * (w * 8) + x * 8);
    uint32_t s = 0;
#pragma unroll
    for (int dy = 0; dy < 8; ++dy) {
        const uint2 v = row[(long long)dy * w];            // a row is w uint2
#pragma unroll
        for (int q = 0; q < 4; ++q) s += ((v.x >> (8 * q)) & 255u) + ((v.y >> (8 * q)) & 255u);
    }
    latmask[p] = 2u * s >= 64u * 255u ? 1 : 0;
}

// x_t = sqrt_a x + sqrt_b n with the bits of lcm_latents_renoise (sched.hip, renoise1).
__device__ __forceinline__ float renoise1(float sa, float sb, float x, float n) { return __fmaf_rn(sb, n, __fmul_rn(sa, x)); }

// The LCM step and the select in one launch, laid out like scheduler_step_handover_kernel (sched.hip): one thread per pixel, the
// model output's four channels as one 16-byte NHWC load, the NCHW planes as coalesced 4-byte accesses.  `stepped` spells out
// what the compiler chose in the step kernels (misc.hip scheduler_step_kernel, sched.hip scheduler_step_pred_kernel) --
// guidance: fma(g, m - u, u); epsilon: fma(-sb, m, x) / sa; v: fma(-sb, m, sa x); den: fma(c_skip, x, c_out x0); and the
// non-last form is NOT fused there: (sap den) + (sbp noise), two products and an add -- so a mask of ones gives their bits.
template <int PRED>
__global__ void scheduler_step_inpaint_kernel(const float4* __restrict__ m, const float4* __restrict__ m_u, float guidance,
                                              float* __restrict__ lat, float* __restrict__ lat_dup, const float* __restrict__ noise,
                                              const float* __restrict__ z, const float* __restrict__ e1,
                                              const uint8_t* __restrict__ latmask, StepCoef6 c, int last, float nsa, float nsb,
                                              int B, int hw) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;   // (b, pix): also the index into latmask [B,h,w]
    if (p >= B * hw) return;
    const int b = p / hw, pix = p - b * hw;
    const bool repaint = latmask[p] != 0;
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
        float stepped = den, kept = z[i];
        if (!last) {
            stepped = __fadd_rn(__fmul_rn(c.sap, den), __fmul_rn(c.sbp, noise[i]));
            kept = renoise1(nsa, nsb, kept, e1[i]);
        }
        const float r = repaint ? stepped : kept;
        lat[i] = r;
        if (lat_dup) lat_dup[i] = r;
    }
}

__device__ __forceinline__ uint32_t over1(uint32_t a, uint32_t g, uint32_t o) { return (a * g + (255u - a) * o + 127u) / 255u; }

// out = (alpha gen + (255 - alpha) init + 127) / 255 per pixel and channel, in place on gen.  A lane owns 16 pixels: 16 bytes of
// alpha and 48 bytes of each picture as three 16-byte accesses; the last pixels of a count that is no multiple of 16 go bytewise.
__global__ void inpaint_composite_kernel(uint8_t* __restrict__ rgb, const uint8_t* __restrict__ init, const uint8_t* __restrict__ alpha,
                                         long long npix) {
    const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long p0 = g * 16;
    if (p0 >= npix) return;
    if (p0 + 16 <= npix) {
        const uint4 a4 = *reinterpret_cast<const uint4*>(alpha + p0);
        const uint32_t a[4] = {a4.x, a4.y, a4.z, a4.w};
        uint4* gp = reinterpret_cast<uint4*>(rgb + p0 * 3);
        const uint4* ip = reinterpret_cast<const uint4*>(init + p0 * 3);
        uint32_t gv[12], iv[12];
#pragma unroll
        for (int v = 0; v < 3; ++v) {
            const uint4 x = gp[v], y = ip[v];
            gv[4 * v] = x.x, gv[4 * v + 1] = x.y, gv[4 * v + 2] = x.z, gv[4 * v + 3] = x.w;
            iv[4 * v] = y.x, iv[4 * v + 1] = y.y, iv[4 * v + 2] = y.z, iv[4 * v + 3] = y.w;
        }
#pragma unroll
        for (int d = 0; d < 12; ++d) {
            uint32_t o = 0;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int byte = 4 * d + q, px = byte / 3;          // compile-time after unrolling
                const uint32_t al = (a[px >> 2] >> (8 * (px & 3))) & 255u;
                o |= over1(al, (gv[d] >> (8 * q)) & 255u, (iv[d] >> (8 * q)) & 255u) << (8 * q);
            }
            gv[d] = o;
        }
#pragma unroll
        for (int v = 0; v < 3; ++v) gp[v] = make_uint4(gv[4 * v], gv[4 * v + 1], gv[4 * v + 2], gv[4 * v + 3]);
        return;
    }
    for (long long p = p0; p < npix; ++p) {
        const uint32_t al = alpha[p];
        for (int ch = 0; ch < 3; ++ch) rgb[p * 3 + ch] = (uint8_t)over1(al, rgb[p * 3 + ch], init[p * 3 + ch]);
    }
}
}  // namespace

extern "C" int lcm_inpaint_mask_prepare(const void* mask_u8, const void* weights_u32, int radius, void* alpha_u8_out, void* scratch_u8,
                                        void* latmask_out, int B, int H, int W, void* stream) {
    LCM_REQUIRE(mask_u8 && alpha_u8_out, "inpaint_mask_prepare: null pointer");
    LCM_REQUIRE(radius >= 0 && radius <= LCM_INPAINT_MAX_RADIUS, "inpaint_mask_prepare: blur radius %d outside [0, %d]", radius,
                LCM_INPAINT_MAX_RADIUS);
    LCM_REQUIRE(radius == 0 || (weights_u32 && scratch_u8), "inpaint_mask_prepare: a blur needs its weights and a scratch plane");
    LCM_REQUIRE(radius == 0 || (scratch_u8 != mask_u8 && scratch_u8 != alpha_u8_out), "inpaint_mask_prepare: scratch aliases a plane");
    LCM_REQUIRE(B > 0 && H > 0 && W > 0 && (long long)B * H * W < (1ll << 31) && B < 65536 && H <= 65535 * HB_ROWS,
                "inpaint_mask_prepare: bad shape");
    LCM_REQUIRE(!latmask_out || (H % 8 == 0 && W % 8 == 0), "inpaint_mask_prepare: the latent mask needs H and W divisible by 8, got %d and %d",
                H, W);
    LCM_REQUIRE(((uintptr_t)mask_u8 | (uintptr_t)alpha_u8_out | (uintptr_t)scratch_u8) % 8 == 0,
                "inpaint_mask_prepare: planes must be 8-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const uint8_t* m = (const uint8_t*)mask_u8;
    uint8_t* alpha = (uint8_t*)alpha_u8_out;
    if (radius == 0) {
        if (alpha != m) {
            hipError_t e = hipMemcpyAsync(alpha, m, (size_t)B * H * W, hipMemcpyDeviceToDevice, s);
            LCM_REQUIRE(e == hipSuccess, "inpaint_mask_prepare: copy failed: %s", hipGetErrorString(e));
        }
    } else {
        const uint32_t* w = (const uint32_t*)weights_u32;
        uint8_t* t = (uint8_t*)scratch_u8;
        const int off = (4 - (radius & 3)) & 3, nd = (2 * radius + 4 + off + 3) / 4;
        const size_t lds_h = sizeof(uint32_t) * (4 * nd + HB_ROWS * (HB_LANES + nd));
        hipLaunchKernelGGL(mask_blur_h_kernel, dim3((W + HB_LANES * 4 - 1) / (HB_LANES * 4), (H + HB_ROWS - 1) / HB_ROWS, B),
                           dim3(HB_LANES, HB_ROWS), lds_h, s, m, t, w, radius, H, W);
        LCM_CHECK_LAUNCH("inpaint_mask_prepare (horizontal)");
        const size_t lds_v = sizeof(uint32_t) * (((2 * radius + 1 + 3) & ~3) + (VB_TH + 2 * radius) * VB_LANES);
        hipLaunchKernelGGL(mask_blur_v_kernel, dim3((W + VB_LANES * 4 - 1) / (VB_LANES * 4), (H + VB_TH - 1) / VB_TH, B),
                           dim3(VB_LANES, VB_ROWS), lds_v, s, (const uint8_t*)t, alpha, w, radius, H, W);
        LCM_CHECK_LAUNCH("inpaint_mask_prepare (vertical)");
    }
    if (latmask_out) {
        const int n = B * (H / 8) * (W / 8);
        hipLaunchKernelGGL(latent_mask_kernel, dim3((n + 255) / 256), dim3(256), 0, s, (const uint8_t*)alpha, (uint8_t*)latmask_out, B,
                           H / 8, W / 8);
        LCM_CHECK_LAUNCH("inpaint_mask_prepare (latent mask)");
    }
    return LCM_OK;
}

extern "C" int lcm_scheduler_step_inpaint(const void* eps, const void* eps_uncond, float guidance, void* lat, const void* noise,
                                          const void* z, const void* e1, const void* latmask, const float* coef6, int last,
                                          float next_sqrt_a, float next_sqrt_b, int prediction_type, int B, int h, int w, int dup,
                                          void* stream) {
    LCM_REQUIRE(prediction_type == LCM_PRED_EPSILON || prediction_type == LCM_PRED_V || prediction_type == LCM_PRED_SAMPLE,
                "scheduler_step_inpaint: unknown prediction type %d", prediction_type);
    LCM_REQUIRE(eps && lat && z && latmask && coef6 && (last || (noise && e1)), "scheduler_step_inpaint: null pointer");
    LCM_REQUIRE(B > 0 && h > 0 && w > 0 && (long long)B * 4 * h * w < (1ll << 30), "scheduler_step_inpaint: bad shape");
    LCM_REQUIRE(((uintptr_t)eps | (uintptr_t)eps_uncond) % 16 == 0, "scheduler_step_inpaint: model output must be 16-byte aligned");
    StepCoef6 c = {coef6[0], coef6[1], coef6[2], coef6[3], coef6[4], coef6[5]};
    const int hw = h * w, n = B * hw;
    auto kern = prediction_type == LCM_PRED_EPSILON ? scheduler_step_inpaint_kernel<LCM_PRED_EPSILON>
              : prediction_type == LCM_PRED_V     ? scheduler_step_inpaint_kernel<LCM_PRED_V>
                                                  : scheduler_step_inpaint_kernel<LCM_PRED_SAMPLE>;
    // dup: lat holds [other half | this half] (classifier-free guidance, rows [0,B) = negative prompt): the copy goes in front
    float* l = (float*)lat;
    hipLaunchKernelGGL(kern, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, (const float4*)eps, (const float4*)eps_uncond,
                       guidance, l, dup ? l - (long long)B * 4 * hw : (float*)nullptr, (const float*)noise, (const float*)z,
                       (const float*)e1, (const uint8_t*)latmask, c, last ? 1 : 0, next_sqrt_a, next_sqrt_b, B, hw);
    LCM_CHECK_LAUNCH("scheduler_step_inpaint");
    return LCM_OK;
}

extern "C" int lcm_inpaint_composite_rgb8(void* rgb_inout, const void* init_u8, const void* alpha_u8, int B, int H, int W, void* stream) {
    LCM_REQUIRE(rgb_inout && init_u8 && alpha_u8, "inpaint_composite_rgb8: null pointer");
    LCM_REQUIRE(B > 0 && H > 0 && W > 0 && (long long)B * H * W * 3 < (1ll << 31), "inpaint_composite_rgb8: bad shape");
    LCM_REQUIRE(((uintptr_t)rgb_inout | (uintptr_t)init_u8 | (uintptr_t)alpha_u8) % 16 == 0,
                "inpaint_composite_rgb8: pointers must be 16-byte aligned");
    LCM_REQUIRE(rgb_inout != init_u8, "inpaint_composite_rgb8: the picture aliases the output");
    const long long npix = (long long)B * H * W, groups = (npix + 15) / 16;
    hipLaunchKernelGGL(inpaint_composite_kernel, dim3((unsigned)((groups + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       (uint8_t*)rgb_inout, (const uint8_t*)init_u8, (const uint8_t*)alpha_u8, npix);
    LCM_CHECK_LAUNCH("inpaint_composite_rgb8");
    return LCM_OK;
}
