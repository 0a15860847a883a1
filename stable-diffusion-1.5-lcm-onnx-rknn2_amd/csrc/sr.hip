// Super-resolution post-process (the server's SuperResWorker): the ONNX model zoo's super-resolution-10, an ESPCN-style
// sub-pixel CNN on the luma plane, run over independent square tiles of the image, plus PIL's bicubic x3 of the chroma planes
// and the YCbCr -> RGB merge.  Layouts and semantics: include/lcm_hip.h ("super-resolution").
//
//   lcm_sr_conv1          RGB8 -> PIL Y -> fp16 Y/255, gathered per tile (zero padded at each tile's border), conv1 5x5 1->64
//                         + bias + ReLU on the VALU (Cin = 1: 2.7 % of the FLOPs) -> fp16 NHWC [T][th][tw][64]
//   lcm_sr_conv3x3        conv2 (64->64) / conv3 (64->32), 3x3 pad 1 per tile, bias + ReLU: MFMA implicit GEMM, the halo of a
//                         16 x 32 output block and the whole weight matrix staged in LDS
//   lcm_sr_conv4_shuffle  conv4 (32->9) + bias, pixel shuffle x3, uint8(clip(255 y)) -- written only where the tile OWNS the
//                         pixel (the tile a row-major overwrite would leave on top), so every pixel is written exactly once
//   lcm_sr_chroma_h       RGB8 -> PIL Cb/Cr, horizontal bicubic x3 in PIL's 8-bit fixed point -> uint8 [H][3W][2]
//   lcm_sr_merge          vertical bicubic x3 of Cb/Cr, merge with the Y plane, PIL YCbCr -> RGB8
#include "common.h"

namespace {

constexpr int SR_R = 3;              // upscale factor of the network (conv4 has R*R outputs)
constexpr int C1 = 64, C3 = 32;      // channels after conv1/conv2 and after conv3

// ---- PIL's integer colour tables (ConvertYCbCr: 6 fraction bits).  Y uses rounded tables (matches PIL on all 2^24
// colours); the chroma and the inverse use truncated ones, which stay within 1 of PIL (the exact tables are not public
// API).  Every coefficient is the exact rational c * 64, so the tables are integer arithmetic in int32.
__host__ __device__ __forceinline__ int pil_y(int r, int g, int b) {
    return ((19136 * r + 500) / 1000 + (37568 * g + 500) / 1000 + (7296 * b + 500) / 1000) >> 6;
}
__host__ __device__ __forceinline__ int clamp_u8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }
__device__ __forceinline__ int pil_cb(int r, int g, int b) {
    return clamp_u8(((-(168736 * r) / 15625 + -(331264 * g) / 15625 + 32 * b) >> 6) + 128);
}
__device__ __forceinline__ int pil_cr(int r, int g, int b) {
    return clamp_u8(((32 * r + -(418688 * g) / 15625 + -(81312 * b) / 15625) >> 6) + 128);
}
__device__ __forceinline__ void pil_ycc_to_rgb(int y, int cb, int cr, uint8_t* o) {
    const int vb = cb - 128, vr = cr - 128;
    o[0] = (uint8_t)clamp_u8(y + ((11216 * vr / 125) >> 6));
    o[1] = (uint8_t)clamp_u8(y + ((-(344136 * vb) / 15625 + -(714136 * vr) / 15625) >> 6));
    o[2] = (uint8_t)clamp_u8(y + ((14176 * vb / 125) >> 6));
}

// ---- PIL's bicubic resampling of 8-bit planes (a = -0.5), for an upscale (filter scale 1, support 2, at most 5 taps):
// output o has centre (o + 0.5) * in/out, taps [trunc(centre - 1.5), trunc(centre + 2.5)) cut to the image, weights
// normalised in double and converted to 22-bit fixed point.  The double arithmetic follows PIL's operation order with
// contraction off, so the integer weights are PIL's.
constexpr int PIL_PREC = 22;
__device__ __forceinline__ double pil_bicubic(double x) {
#pragma clang fp contract(off)
    const double a = -0.5;
    if (x < 0.0) x = -x;
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
    if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
    return 0.0;
}
__device__ __forceinline__ int pil_coeffs(int o, int in_size, int out_size, int (&k)[5]) {
#pragma clang fp contract(off)
    const double scale = (double)in_size / (double)out_size;
    const double support = 2.0;
    const double center = (o + 0.5) * scale;
    int xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > in_size) xmax = in_size;
    xmax -= xmin;
    double w[5];
    double ww = 0.0;
#pragma unroll
    for (int x = 0; x < 5; ++x) {
        w[x] = x < xmax ? pil_bicubic(((double)(x + xmin) - center + 0.5) * 1.0) : 0.0;
        ww += w[x];
    }
#pragma unroll
    for (int x = 0; x < 5; ++x) {
        const double v = (x < xmax && ww != 0.0) ? w[x] / ww : 0.0;
        k[x] = v < 0 ? (int)(-0.5 + v * (1 << PIL_PREC)) : (int)(0.5 + v * (1 << PIL_PREC));
    }
    return xmin;
}
__device__ __forceinline__ int pil_clip8(int v) { return clamp_u8(v >> PIL_PREC); }

// ---- the tile plan (server/lcm_sr_server.py _plan_tiles): starts 0, t, 2t, ... while a whole tile fits, then size - t;
// i-th start = min(i t, size - t), count = ceil(size / t).  Row-major order with later tiles overwriting earlier ones
// leaves input pixel g to the tile with the largest covering start: the last one if g >= size - t, else g / t.
__device__ __forceinline__ int tile_start(int i, int t, int size) { return min(i * t, size - t); }
__device__ __forceinline__ int tile_owner(int g, int t, int size, int n) { return g >= size - t ? n - 1 : g / t; }

// ---------------------------------------------------------------------------------------------------------------------
// conv1: one thread per tile pixel (16 x 16 per workgroup), the 20 x 20 input halo and the weights in LDS
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sr_conv1_kernel(const uint8_t* __restrict__ rgb, int W, int H, int tw, int th, int nx,
                                                       int t0, int nbx, const half_t* __restrict__ w1, const float* __restrict__ b1,
                                                       half_t* __restrict__ out) {
    __shared__ float xin[20][20];
    __shared__ __align__(16) float wl[25][C1];
    __shared__ float bl[C1];
    const int t = t0 + blockIdx.y;
    const int x0 = tile_start(t % nx, tw, W), y0 = tile_start(t / nx, th, H);
    const int by = blockIdx.x / nbx, bx = blockIdx.x % nbx;
    const int oy0 = by * 16, ox0 = bx * 16;
    for (int i = threadIdx.x; i < 25 * C1; i += 256) wl[i / C1][i % C1] = (float)w1[i];
    if (threadIdx.x < C1) bl[threadIdx.x] = b1[threadIdx.x];
    for (int i = threadIdx.x; i < 400; i += 256) {
        const int hy = i / 20, hx = i % 20;
        const int ty = oy0 - 2 + hy, tx = ox0 - 2 + hx;              // tile coordinates: zero outside the tile
        float v = 0.f;
        if (ty >= 0 && ty < th && tx >= 0 && tx < tw) {
            const uint8_t* p = rgb + ((long long)(y0 + ty) * W + (x0 + tx)) * 3;
            v = (float)(half_t)((float)pil_y(p[0], p[1], p[2]) / 255.0f);
        }
        xin[hy][hx] = v;
    }
    __syncthreads();
    const int ly = threadIdx.x >> 4, lx = threadIdx.x & 15;
    const int ty = oy0 + ly, tx = ox0 + lx;
    if (ty >= th || tx >= tw) return;
    float acc[C1];
#pragma unroll
    for (int c = 0; c < C1; ++c) acc[c] = bl[c];
#pragma unroll 5
    for (int tap = 0; tap < 25; ++tap) {
        const float x = xin[ly + tap / 5][lx + tap % 5];
#pragma unroll
        for (int c = 0; c < C1; c += 4) {
            const f4 w = *reinterpret_cast<const f4*>(&wl[tap][c]);
            acc[c] = __builtin_fmaf(x, w[0], acc[c]);
            acc[c + 1] = __builtin_fmaf(x, w[1], acc[c + 1]);
            acc[c + 2] = __builtin_fmaf(x, w[2], acc[c + 2]);
            acc[c + 3] = __builtin_fmaf(x, w[3], acc[c + 3]);
        }
    }
    h8* o = reinterpret_cast<h8*>(out + (((long long)blockIdx.y * th + ty) * tw + tx) * C1);
#pragma unroll
    for (int q = 0; q < C1 / 8; ++q) {
        h8 v;
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = (half_t)fmaxf(acc[8 * q + j], 0.f);
        o[q] = v;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// conv2 / conv3: 3x3, Cin 64, pad 1 per tile, bias + ReLU.  Implicit GEMM M = pixels, N = COUT, K = 9 taps x 64 channels on
// v_mfma_f32_16x16x32_f16.  A workgroup (8 waves) owns a 16-row x 32-column output block of one tile; its 18 x 34 pixel halo
// (78 KB) and the whole [COUT][576] weight matrix (72 / 36 KB) sit in LDS.  Wave w computes rows 2w, 2w+1: four 16-pixel
// A fragments x COUT/16 B fragments per 32-deep K step.  16-byte chunks are XOR-swizzled by (row & 7) in both images so the
// fragment reads of 8 consecutive pixels / output channels fall on distinct banks.
// ---------------------------------------------------------------------------------------------------------------------
constexpr int CB_H = 16, CB_W = 32, HALO_H = CB_H + 2, HALO_W = CB_W + 2;
template <int COUT>
constexpr int conv3x3_lds() { return (HALO_H * HALO_W * 8 + COUT * 72) * 16; }

template <int COUT>
__global__ __launch_bounds__(512) void sr_conv3x3_kernel(const half_t* __restrict__ in, const half_t* __restrict__ w,
                                                         const float* __restrict__ bias, half_t* __restrict__ out, int th, int tw,
                                                         int nbx) {
    extern __shared__ __align__(16) char smem[];
    uint4* halo = reinterpret_cast<uint4*>(smem);              // chunk c of halo pixel p at p * 8 + (c ^ (p & 7))
    uint4* wl = halo + HALO_H * HALO_W * 8;                     // chunk c of weight row n at n * 72 + (c ^ (n & 7))
    constexpr int NF = COUT / 16;
    const long long img = (long long)blockIdx.y * th * tw;
    const int by = blockIdx.x / nbx, bx = blockIdx.x % nbx;
    const int oy0 = by * CB_H, ox0 = bx * CB_W;
    const uint4* wg = reinterpret_cast<const uint4*>(w);
    for (int i = threadIdx.x; i < COUT * 72; i += 512) {
        const int n = i / 72, c = i - n * 72;
        wl[n * 72 + (c ^ (n & 7))] = wg[i];
    }
    const uint4* ig = reinterpret_cast<const uint4*>(in);
    for (int i = threadIdx.x; i < HALO_H * HALO_W * 8; i += 512) {
        const int p = i >> 3, c = i & 7;
        const int hy = p / HALO_W, hx = p - hy * HALO_W;
        const int ty = oy0 - 1 + hy, tx = ox0 - 1 + hx;
        uint4 v = {0u, 0u, 0u, 0u};
        if (ty >= 0 && ty < th && tx >= 0 && tx < tw) v = ig[(img + (long long)ty * tw + tx) * 8 + c];
        halo[p * 8 + (c ^ (p & 7))] = v;
    }
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int li = lane & 15, lq = lane >> 4;
    f4 acc[4][NF];
#pragma unroll
    for (int f = 0; f < 4; ++f)
#pragma unroll
        for (int j = 0; j < NF; ++j) acc[f][j] = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
    for (int tap = 0; tap < 9; ++tap) {
        const int ky = tap / 3, kx = tap - 3 * (tap / 3);
#pragma unroll
        for (int kc = 0; kc < 2; ++kc) {
            h8 a[4], b[NF];
#pragma unroll
            for (int f = 0; f < 4; ++f) {
                const int p = (2 * wave + (f >> 1) + ky) * HALO_W + 16 * (f & 1) + li + kx;
                const uint4 v = halo[p * 8 + ((kc * 4 + lq) ^ (p & 7))];
                a[f] = *reinterpret_cast<const h8*>(&v);
            }
#pragma unroll
            for (int j = 0; j < NF; ++j) {
                const int n = 16 * j + li;
                const uint4 v = wl[n * 72 + ((tap * 8 + kc * 4 + lq) ^ (n & 7))];
                b[j] = *reinterpret_cast<const h8*>(&v);
            }
#pragma unroll
            for (int f = 0; f < 4; ++f)
#pragma unroll
                for (int j = 0; j < NF; ++j) acc[f][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[f], b[j], acc[f][j], 0, 0, 0);
        }
    }
    // D[m][n]: lane holds pixels 4 lq + i (i = 0..3) of the fragment, output channel 16 j + li
#pragma unroll
    for (int f = 0; f < 4; ++f) {
        const int ty = oy0 + 2 * wave + (f >> 1);
        if (ty >= th) continue;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int tx = ox0 + 16 * (f & 1) + 4 * lq + i;
            if (tx >= tw) continue;
            half_t* o = out + (img + (long long)ty * tw + tx) * COUT;
#pragma unroll
            for (int j = 0; j < NF; ++j) o[16 * j + li] = (half_t)fmaxf(acc[f][j][i] + bias[16 * j + li], 0.f);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// conv4 + pixel shuffle + uint8 Y: one thread per tile pixel; pixels the tile does not own return after the shared loads
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sr_conv4_shuffle_kernel(const half_t* __restrict__ in, int W, int H, int tw, int th, int nx,
                                                               int ny, int t0, int nbx, const half_t* __restrict__ w4,
                                                               const float* __restrict__ b4, uint8_t* __restrict__ y_out) {
    constexpr int RR = SR_R * SR_R;
    __shared__ __align__(16) half_t hal[18 * 18][C3];
    __shared__ float wl[9 * C3][RR];
    __shared__ float bl[RR];
    const int t = t0 + blockIdx.y;
    const int txi = t % nx, tyi = t / nx;
    const int x0 = tile_start(txi, tw, W), y0 = tile_start(tyi, th, H);
    const int by = blockIdx.x / nbx, bx = blockIdx.x % nbx;
    const int oy0 = by * 16, ox0 = bx * 16;
    for (int i = threadIdx.x; i < 9 * C3 * RR; i += 256) wl[i / RR][i % RR] = (float)w4[i];
    if (threadIdx.x < RR) bl[threadIdx.x] = b4[threadIdx.x];
    const long long img = (long long)blockIdx.y * th * tw;
    for (int i = threadIdx.x; i < 18 * 18 * (C3 / 8); i += 256) {
        const int p = i / (C3 / 8), c = i % (C3 / 8);
        const int ty = oy0 - 1 + p / 18, tx = ox0 - 1 + p % 18;
        h8 v = {};
        if (ty >= 0 && ty < th && tx >= 0 && tx < tw) v = reinterpret_cast<const h8*>(in + (img + (long long)ty * tw + tx) * C3)[c];
        reinterpret_cast<h8*>(&hal[p][0])[c] = v;
    }
    __syncthreads();
    const int ly = threadIdx.x >> 4, lx = threadIdx.x & 15;
    const int ty = oy0 + ly, tx = ox0 + lx;
    if (ty >= th || tx >= tw) return;
    const int gx = x0 + tx, gy = y0 + ty;
    if (tile_owner(gx, tw, W, nx) != txi || tile_owner(gy, th, H, ny) != tyi) return;
    float acc[RR];
#pragma unroll
    for (int o = 0; o < RR; ++o) acc[o] = bl[o];
#pragma unroll 1
    for (int tap = 0; tap < 9; ++tap) {
        const half_t* x = &hal[(ly + tap / 3) * 18 + lx + tap % 3][0];
#pragma unroll 8
        for (int c = 0; c < C3; ++c) {
            const float xv = (float)x[c];
#pragma unroll
            for (int o = 0; o < RR; ++o) acc[o] = __builtin_fmaf(xv, wl[tap * C3 + c][o], acc[o]);
        }
    }
    const long long OW = (long long)W * SR_R;
#pragma unroll
    for (int i = 0; i < SR_R; ++i)
#pragma unroll
        for (int j = 0; j < SR_R; ++j) {
            const float v = fminf(fmaxf(acc[i * SR_R + j] * 255.0f, 0.f), 255.f);
            y_out[((long long)gy * SR_R + i) * OW + (long long)gx * SR_R + j] = (uint8_t)(int)v;     // truncation
        }
}

// ---------------------------------------------------------------------------------------------------------------------
// chroma: horizontal pass (RGB8 -> Cb, Cr -> bicubic along x, clipped to uint8 as PIL stores its intermediate image)
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sr_chroma_h_kernel(const uint8_t* __restrict__ rgb, int W, int H, uint8_t* __restrict__ cc) {
    const int OW = W * SR_R;
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)OW * H) return;
    const int y = (int)(idx / OW), ox = (int)(idx - (long long)y * OW);
    int k[5];
    const int xmin = pil_coeffs(ox, W, OW, k);
    int sb = 1 << (PIL_PREC - 1), sr = 1 << (PIL_PREC - 1);
#pragma unroll
    for (int x = 0; x < 5; ++x) {
        if (k[x] == 0) continue;                                  // PIL's zero weights beyond the cut add nothing
        const uint8_t* p = rgb + ((long long)y * W + xmin + x) * 3;
        sb += pil_cb(p[0], p[1], p[2]) * k[x];
        sr += pil_cr(p[0], p[1], p[2]) * k[x];
    }
    cc[idx * 2] = (uint8_t)pil_clip8(sb);
    cc[idx * 2 + 1] = (uint8_t)pil_clip8(sr);
}

// merge: vertical pass of Cb/Cr + Y plane -> RGB8 [3H][3W][3]
__global__ __launch_bounds__(256) void sr_merge_kernel(const uint8_t* __restrict__ yp, const uint8_t* __restrict__ cc, int W, int H,
                                                       uint8_t* __restrict__ rgb) {
    const int OW = W * SR_R, OH = H * SR_R;
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)OW * OH) return;
    const int oy = (int)(idx / OW), ox = (int)(idx - (long long)oy * OW);
    int k[5];
    const int ymin = pil_coeffs(oy, H, OH, k);
    int sb = 1 << (PIL_PREC - 1), sr = 1 << (PIL_PREC - 1);
#pragma unroll
    for (int y = 0; y < 5; ++y) {
        if (k[y] == 0) continue;
        const uint8_t* p = cc + ((long long)(ymin + y) * OW + ox) * 2;
        sb += p[0] * k[y];
        sr += p[1] * k[y];
    }
    pil_ycc_to_rgb(yp[idx], pil_clip8(sb), pil_clip8(sr), rgb + idx * 3);
}

}  // namespace

// ---------------------------------------------------------------------------------------------------------------------
// C ABI (include/lcm_hip.h): every argument is checked before anything is enqueued
// ---------------------------------------------------------------------------------------------------------------------
static int sr_check_plan(const char* what, int W, int H, int tile_w, int tile_h, int t0, int ntiles) {
    LCM_REQUIRE(W >= 1 && H >= 1, "%s: image %dx%d must be at least 1x1", what, W, H);
    LCM_REQUIRE(tile_w >= 1 && tile_h >= 1, "%s: tile %dx%d must be at least 1x1", what, tile_w, tile_h);
    LCM_REQUIRE(tile_w <= W && tile_h <= H, "%s: tile %dx%d larger than the image %dx%d", what, tile_w, tile_h, W, H);
    LCM_REQUIRE((long long)W * SR_R * SR_R * H * 3 < (1ll << 40), "%s: image %dx%d too large", what, W, H);
    const long long nt = (long long)((W + tile_w - 1) / tile_w) * ((H + tile_h - 1) / tile_h);
    LCM_REQUIRE(ntiles >= 1 && ntiles <= 65535, "%s: ntiles=%d must be in 1..65535", what, ntiles);
    LCM_REQUIRE(t0 >= 0 && t0 + (long long)ntiles <= nt, "%s: tiles [%d, %d) outside the plan's %lld tiles", what, t0, t0 + ntiles, nt);
    return LCM_OK;
}

extern "C" int lcm_sr_conv1(const void* rgb, int W, int H, int tile_w, int tile_h, int t0, int ntiles, const void* w1,
                            const void* b1, void* out, void* stream) {
    LCM_REQUIRE(rgb && w1 && b1 && out, "sr_conv1: null pointer");
    if (int rc = sr_check_plan("sr_conv1", W, H, tile_w, tile_h, t0, ntiles)) return rc;
    const int nbx = (tile_w + 15) / 16, nby = (tile_h + 15) / 16;
    hipStream_t s = (hipStream_t)stream;
    lcm_prof_start("sr_conv1_kernel", s);
    hipLaunchKernelGGL(sr_conv1_kernel, dim3(nbx * nby, ntiles), dim3(256), 0, s, (const uint8_t*)rgb, W, H, tile_w, tile_h,
                       (W + tile_w - 1) / tile_w, t0, nbx, (const half_t*)w1, (const float*)b1, (half_t*)out);
    lcm_prof_stop(s);
    LCM_CHECK_LAUNCH("sr_conv1");
    return LCM_OK;
}

template <int COUT>
static int sr_conv3x3_launch(const void* in, int T, int th, int tw, const void* w, const void* bias, void* out, hipStream_t s) {
    constexpr int smem = conv3x3_lds<COUT>();
    static_assert(smem <= 160 * 1024, "conv3x3 halo + weights exceed LDS");
    static LcmDevOnce attr_once;
    if (auto once_guard = attr_once.first()) {
        once_guard.check(hipFuncSetAttribute(reinterpret_cast<const void*>(&sr_conv3x3_kernel<COUT>),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, smem));
    }
    const int nbx = (tw + CB_W - 1) / CB_W, nby = (th + CB_H - 1) / CB_H;
    lcm_prof_start(COUT == 64 ? "sr_conv3x3_kernel<64>" : "sr_conv3x3_kernel<32>", s);
    hipLaunchKernelGGL(sr_conv3x3_kernel<COUT>, dim3(nbx * nby, T), dim3(512), smem, s, (const half_t*)in, (const half_t*)w,
                       (const float*)bias, (half_t*)out, th, tw, nbx);
    lcm_prof_stop(s);
    LCM_CHECK_LAUNCH("sr_conv3x3");
    return LCM_OK;
}

extern "C" int lcm_sr_conv3x3(const void* in, int T, int th, int tw, int cout, const void* w, const void* bias, void* out, void* stream) {
    LCM_REQUIRE(in && w && bias && out, "sr_conv3x3: null pointer");
    LCM_REQUIRE(T >= 1 && T <= 65535, "sr_conv3x3: T=%d must be in 1..65535", T);
    LCM_REQUIRE(th >= 1 && tw >= 1, "sr_conv3x3: tile %dx%d must be at least 1x1", tw, th);
    LCM_REQUIRE(cout == 64 || cout == 32, "sr_conv3x3: cout=%d not supported (64 or 32)", cout);
    LCM_REQUIRE(((uintptr_t)in | (uintptr_t)w | (uintptr_t)out) % 16 == 0, "sr_conv3x3: pointers must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    return cout == 64 ? sr_conv3x3_launch<64>(in, T, th, tw, w, bias, out, s) : sr_conv3x3_launch<32>(in, T, th, tw, w, bias, out, s);
}

extern "C" int lcm_sr_conv4_shuffle(const void* in, int W, int H, int tile_w, int tile_h, int t0, int ntiles, const void* w4,
                                    const void* b4, int r, void* y_out, void* stream) {
    LCM_REQUIRE(in && w4 && b4 && y_out, "sr_conv4_shuffle: null pointer");
    LCM_REQUIRE(r == SR_R, "sr_conv4_shuffle: upscale factor %d not supported (the kernels implement %d)", r, SR_R);
    if (int rc = sr_check_plan("sr_conv4_shuffle", W, H, tile_w, tile_h, t0, ntiles)) return rc;
    LCM_REQUIRE((uintptr_t)in % 16 == 0, "sr_conv4_shuffle: input must be 16-byte aligned");
    const int nbx = (tile_w + 15) / 16, nby = (tile_h + 15) / 16;
    hipStream_t s = (hipStream_t)stream;
    lcm_prof_start("sr_conv4_shuffle_kernel", s);
    hipLaunchKernelGGL(sr_conv4_shuffle_kernel, dim3(nbx * nby, ntiles), dim3(256), 0, s, (const half_t*)in, W, H, tile_w, tile_h,
                       (W + tile_w - 1) / tile_w, (H + tile_h - 1) / tile_h, t0, nbx, (const half_t*)w4, (const float*)b4,
                       (uint8_t*)y_out);
    lcm_prof_stop(s);
    LCM_CHECK_LAUNCH("sr_conv4_shuffle");
    return LCM_OK;
}

extern "C" int lcm_sr_chroma_h(const void* rgb, int W, int H, int r, void* cbcr_h, void* stream) {
    LCM_REQUIRE(rgb && cbcr_h, "sr_chroma_h: null pointer");
    LCM_REQUIRE(r == SR_R, "sr_chroma_h: upscale factor %d not supported (the kernels implement %d)", r, SR_R);
    LCM_REQUIRE(W >= 1 && H >= 1 && (long long)W * H * SR_R * SR_R < (1ll << 31), "sr_chroma_h: image %dx%d out of range", W, H);
    const long long n = (long long)W * SR_R * H;
    hipStream_t s = (hipStream_t)stream;
    lcm_prof_start("sr_chroma_h_kernel", s);
    hipLaunchKernelGGL(sr_chroma_h_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (const uint8_t*)rgb, W, H,
                       (uint8_t*)cbcr_h);
    lcm_prof_stop(s);
    LCM_CHECK_LAUNCH("sr_chroma_h");
    return LCM_OK;
}

extern "C" int lcm_sr_merge(const void* y_plane, const void* cbcr_h, int W, int H, int r, void* rgb_out, void* stream) {
    LCM_REQUIRE(y_plane && cbcr_h && rgb_out, "sr_merge: null pointer");
    LCM_REQUIRE(r == SR_R, "sr_merge: upscale factor %d not supported (the kernels implement %d)", r, SR_R);
    LCM_REQUIRE(W >= 1 && H >= 1 && (long long)W * H * SR_R * SR_R < (1ll << 31), "sr_merge: image %dx%d out of range", W, H);
    const long long n = (long long)W * SR_R * H * SR_R;
    hipStream_t s = (hipStream_t)stream;
    lcm_prof_start("sr_merge_kernel", s);
    hipLaunchKernelGGL(sr_merge_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (const uint8_t*)y_plane,
                       (const uint8_t*)cbcr_h, W, H, (uint8_t*)rgb_out);
    lcm_prof_stop(s);
    LCM_CHECK_LAUNCH("sr_merge");
    return LCM_OK;
}
