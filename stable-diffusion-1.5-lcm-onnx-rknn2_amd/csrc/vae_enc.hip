// Image-to-image, the two ends of the AutoencoderKL encoder that no decoder kernel covers:
//   lcm_vae_enc_conv_in_u8      encoder.conv_in from the uploaded uint8 picture, x = 2 u8 / 255 - 1 formed in the kernel
//   lcm_conv3x3_down_f16        Downsample2D: F.pad(x, (0, 1, 0, 1)) -> conv3x3 stride 2, on the row-gather implicit GEMM
//   lcm_vae_posterior_renoise   quant_conv -> DiagonalGaussianDistribution.sample -> x scaling_factor -> LCMScheduler.add_noise,
//                               one launch that writes the clean latents z and the first state of the "from-state" plan
// Everything else runs on the decoder's kernels.
#include "igemm_common.h"

// ---------------------------------------------------------------------------------------------
// conv_in: uint8 RGB [B,H,W,3] -> fp16 [B,H,W,Cout].  hint_conv_u8_kernel's scheme (controlnet.hip): the weights sit in LDS in
// fragment order, a wave owns 16 consecutive pixels and builds its B operand in registers.  K = 27; the fp32 value
// x = 2 u8 / 255 - 1 enters as fp16 hi + fp16 lo against the same weights (slots 0..26 hi, 27..53 lo, 54..63 zero): two MFMAs per
// 16 x 16 tile, one fp32 chain per output in slot order, no K split.  The convolution pads the NORMALISED picture with zeros: a
// tap outside the image contributes 0, not the -1 that a zero byte would normalise to -- which is why the normalisation cannot
// be folded into the weights and the bias.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void vae_enc_conv_in_u8_kernel(const uint8_t* __restrict__ in, const half_t* __restrict__ W,
                                                                 const half_t* __restrict__ bias, half_t* __restrict__ out,
                                                                 int B, int H, int Wd, int Cout) {
#pragma clang fp contract(off)
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
                const int part = k >= 54 ? 2 : (k >= 27 ? 1 : 0), r = k - 27 * part;
                const int tap = r / 3, c = r - 3 * tap;
                const int iy = y + tap / 3 - 1, ix = x + tap % 3 - 1;
                float v = 0.f;                              // outside the picture: zero AFTER the normalisation
                if (live && part < 2 && iy >= 0 && iy < H && ix >= 0 && ix < Wd)
                    v = (2.0f * (float)in[(((long long)b * H + iy) * Wd + ix) * 3 + c]) / 255.0f - 1.0f;
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
            if (live)
                *reinterpret_cast<h4*>(orow + ct) = (h4){(half_t)acc[0], (half_t)acc[1], (half_t)acc[2], (half_t)acc[3]};
        }
    }
}

extern "C" int lcm_vae_enc_conv_in_u8(const void* in, const void* W, const void* bias, void* out, int B, int H, int Wd, int Cout,
                                      void* stream) {
    LCM_REQUIRE(in && W && out, "vae_enc_conv_in_u8: null pointer");
    LCM_REQUIRE(B > 0 && H > 0 && Wd > 0 && Cout > 0 && Cout % 16 == 0 && Cout * 128 <= 64 * 1024, "vae_enc_conv_in_u8: bad shape (Cout %d)", Cout);
    LCM_REQUIRE((long long)B * H * Wd < (1ll << 31) - 16, "vae_enc_conv_in_u8: input too large");
    const long long ntile = ((long long)B * H * Wd + 15) / 16;
    const int grid = (int)((ntile + 3) / 4 < 2048 ? (ntile + 3) / 4 : 2048);
    hipLaunchKernelGGL(vae_enc_conv_in_u8_kernel, dim3(grid), dim3(256), Cout * 128, (hipStream_t)stream, (const uint8_t*)in,
                       (const half_t*)W, (const half_t*)bias, (half_t*)out, B, H, Wd, Cout);
    LCM_CHECK_LAUNCH("vae_enc_conv_in_u8");
    return LCM_OK;
}

// ---------------------------------------------------------------------------------------------
// Posterior -> sampler state.  One thread per latent pixel: the 8 pre-quant_conv moments (two fp32 [B,h,w,4] tensors: the mean
// rows and the logvar rows of encoder.conv_out), quant_conv (8 x 8 + bias, fp32, one fused-multiply-add chain per output in
// input-channel order), then per latent channel c
//   z   = (mean_c + exp(0.5 clamp(logvar_c, -30, 20)) e0) scaling_factor
//   x_T = sqrt_a z + sqrt_b e1                       (lcm_latents_renoise's expression: one rounded product, one fma)
// z, x_T fp32 NCHW; dup: x_T is written to both halves of a [2B,4,h,w] state; moments: optional fp32 [B,8,h,w].
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void vae_posterior_renoise_kernel(const float* __restrict__ pre_m, const float* __restrict__ pre_l,
                                                                    const float* __restrict__ qw, const float* __restrict__ qb,
                                                                    const float* __restrict__ e0, const float* __restrict__ e1,
                                                                    float sf, float sa, float sb, float* __restrict__ z_out,
                                                                    float* __restrict__ lat, float* __restrict__ lat_dup,
                                                                    float* __restrict__ moments, int plane, int npix) {
    __shared__ float w_s[72];
    if (threadIdx.x < 64) w_s[threadIdx.x] = qw[threadIdx.x];
    else if (threadIdx.x < 72) w_s[threadIdx.x] = qb[threadIdx.x - 64];
    __syncthreads();
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= npix) return;
    const f4 a = *reinterpret_cast<const f4*>(pre_m + (long long)i * 4);
    const f4 l = *reinterpret_cast<const f4*>(pre_l + (long long)i * 4);
    const float in8[8] = {a[0], a[1], a[2], a[3], l[0], l[1], l[2], l[3]};
    float mom[8];
#pragma unroll
    for (int o = 0; o < 8; ++o) {
        float s = __fmul_rn(w_s[o * 8], in8[0]);
#pragma unroll
        for (int k = 1; k < 8; ++k) s = __fmaf_rn(w_s[o * 8 + k], in8[k], s);
        mom[o] = __fadd_rn(s, w_s[64 + o]);
    }
    const int b = i / plane, rem = i - b * plane;
    if (moments) {
#pragma unroll
        for (int o = 0; o < 8; ++o) moments[((long long)b * 8 + o) * plane + rem] = mom[o];
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const long long j = ((long long)b * 4 + c) * plane + rem;
        const float lv = fminf(fmaxf(mom[4 + c], -30.0f), 20.0f);
        const float sd = expf(__fmul_rn(0.5f, lv));
        const float z = __fmul_rn(__fmaf_rn(sd, e0[j], mom[c]), sf);
        z_out[j] = z;
        const float xt = __fmaf_rn(sb, e1[j], __fmul_rn(sa, z));
        lat[j] = xt;
        if (lat_dup) lat_dup[j] = xt;
    }
}

extern "C" int lcm_vae_posterior_renoise(const void* pre_mean, const void* pre_logvar, const void* quant_w, const void* quant_b,
                                         const void* e0, const void* e1, float scaling_factor, float sqrt_a, float sqrt_b,
                                         void* z_out, void* lat_out, void* moments_out, int B, int h, int w, int dup, void* stream) {
    LCM_REQUIRE(pre_mean && pre_logvar && quant_w && quant_b && e0 && e1 && z_out && lat_out, "vae_posterior_renoise: null pointer");
    LCM_REQUIRE(B > 0 && h > 0 && w > 0 && (long long)B * 8 * h * w < (1ll << 30), "vae_posterior_renoise: bad shape B=%d h=%d w=%d", B, h, w);
    const int plane = h * w, npix = B * plane;
    float* lat = (float*)lat_out;
    hipLaunchKernelGGL(vae_posterior_renoise_kernel, dim3((npix + 255) / 256), dim3(256), 0, (hipStream_t)stream,
                       (const float*)pre_mean, (const float*)pre_logvar, (const float*)quant_w, (const float*)quant_b,
                       (const float*)e0, (const float*)e1, scaling_factor, sqrt_a, sqrt_b, (float*)z_out, lat,
                       dup ? lat + (long long)npix * 4 : (float*)nullptr, (float*)moments_out, plane, npix);
    LCM_CHECK_LAUNCH("vae_posterior_renoise");
    return LCM_OK;
}

// ---------------------------------------------------------------------------------------------
// Downsample2D of the AutoencoderKL encoder: F.pad(x, (0, 1, 0, 1)) -> conv3x3(stride 2, padding 0).  One zero row below and one
// zero column right of the image only: output (oy, ox) reads input rows 2 oy .. 2 oy + 2 and Ho = (H + 1 - 3) / 2 + 1.
// lcm_conv3x3_f16 with stride 2 pads symmetrically (rows 2 oy - 1 .. 2 oy + 1, ceil(H / 2) outputs): another function, and no
// pointer offset turns one into the other (the row before an image's first is the previous image's last, not zero).
//
// The row-gather implicit GEMM of igemm.hip (igemm_kernel, MODE 1) with that one change in the row descriptors: the same
// 2 x 2 wave grid over a BM x BN tile, BK = 64, register-staged double buffer, XOR-swizzled 128-byte LDS rows, swapped
// v_mfma_f32_16x16x32_f16, and THE shared epilogue (igemm_common.h: split-K slab store | bias, fp16 store, statistics per
// canonical 32-row slab).  What decides the numbers is the K partition alone, and that is the library's canonical one for the
// PER-IMAGE shape (lcm_canonical_splits, kind 1: plan table entry or the deterministic heuristic): blockIdx.y owns its k-tiles,
// the parts are added in part order by splitk_reduce_kernel -- at every batch size, so a request has the same bits alone and in
// a batch.  The tile is a launch parameter (128 x 128 from 4096 output rows on, else 64 x 64).
// ---------------------------------------------------------------------------------------------
float* lcm_splitk_workspace(long long* bytes, hipStream_t s);
void lcm_launch_splitk_reduce(IgemmParams& p, hipStream_t s);
extern "C" int lcm_canonical_splits(int kind, int m_img, int N, int K, int aux, int ph);

template <int BM, int BN>
__global__ __launch_bounds__(256, 2) void conv_down_kernel(IgemmParams p) {
    constexpr int RA = BM / 32, RW = BN / 32;
    constexpr int TM = BM / 32, TN = BN / 32;
    constexpr int XBYTES = BM * 128, WBYTES = BN * 128, BUF = XBYTES + WBYTES;
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave & 1, wn = wave >> 1;
    const int tile = xcd_remap(blockIdx.x, p.mtiles * p.ntiles);
    const int mt = tile / p.ntiles, nt = tile - mt * p.ntiles;
    const int m_base = mt * BM, n_base = nt * BN;
    const half_t* __restrict__ Ab = p.A;
    const int chunk = tid & 7, row0 = tid >> 3;
    const int swz = (chunk ^ (row0 & 7)) << 4;

    bool a_ok[RA];
    int a_b[RA], a_y[RA], a_x[RA];
#pragma unroll
    for (int i = 0; i < RA; ++i) {
        const int m = m_base + row0 + 32 * i;
        a_ok[i] = m < p.M;
        const int hw = p.Hout * p.Wout;
        const int b = m / hw, rem = m - b * hw;
        const int oy = rem / p.Wout;
        a_b[i] = b; a_y[i] = oy * 2; a_x[i] = (rem - oy * p.Wout) * 2;      // no top / left padding
    }
    const half_t* wptr = p.W + (long long)(n_base + row0) * p.K + chunk * 8;

    h8 ra[RA], rw[RW];
    const int nk_all = p.K >> 6;
    const int kt0 = (int)((long long)blockIdx.y * nk_all / p.splits);
    const int kt1 = (int)((long long)(blockIdx.y + 1) * nk_all / p.splits);

    auto load_tile = [&](int kt) {
        const int cpt = p.Cin >> 6;
        const int tap = kt / cpt;
        const int c0 = ((kt - tap * cpt) << 6) + chunk * 8;
        const int dy = tap / 3, dx = tap - dy * 3;
#pragma unroll
        for (int i = 0; i < RA; ++i) {
            h8 v = {0, 0, 0, 0, 0, 0, 0, 0};
            const int iy = a_y[i] + dy, ix = a_x[i] + dx;                   // >= 0; past the last row / column: the zero padding
            if (a_ok[i] && iy < p.Hin && ix < p.Win) {
                const long long off = ((long long)(a_b[i] * p.Hin + iy) * p.Win + ix) * p.Cin + c0;
                v = *reinterpret_cast<const h8*>(Ab + off);
            }
            ra[i] = v;
        }
#pragma unroll
        for (int i = 0; i < RW; ++i)
            rw[i] = *reinterpret_cast<const h8*>(wptr + (long long)(32 * i) * p.K + (kt << 6));
    };
    auto store_tile = [&](int buf) {
        char* xs = smem + buf * BUF;
        char* ws = xs + XBYTES;
#pragma unroll
        for (int i = 0; i < RA; ++i) *reinterpret_cast<h8*>(xs + (row0 + 32 * i) * 128 + swz) = ra[i];
#pragma unroll
        for (int i = 0; i < RW; ++i) *reinterpret_cast<h8*>(ws + (row0 + 32 * i) * 128 + swz) = rw[i];
    };

    f4 acc[TN][TM];
#pragma unroll
    for (int a = 0; a < TN; ++a)
#pragma unroll
        for (int b = 0; b < TM; ++b) acc[a][b] = (f4){0.f, 0.f, 0.f, 0.f};

    const int frow = lane & 15, fq = lane >> 4;
    load_tile(kt0);
    store_tile(0);
    __syncthreads();
    for (int kt = kt0; kt < kt1; ++kt) {
        const int cur = (kt - kt0) & 1;
        if (kt + 1 < kt1) load_tile(kt + 1);
        const char* xs = smem + cur * BUF + (wm * (BM / 2)) * 128;
        const char* ws = smem + cur * BUF + XBYTES + (wn * (BN / 2)) * 128;
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            h8 xf[TM], wf[TN];
            const int c = kk * 4 + fq;
#pragma unroll
            for (int b = 0; b < TM; ++b) {
                const int r = b * 16 + frow;
                xf[b] = *reinterpret_cast<const h8*>(xs + r * 128 + ((c ^ (r & 7)) << 4));
            }
#pragma unroll
            for (int a = 0; a < TN; ++a) {
                const int r = a * 16 + frow;
                wf[a] = *reinterpret_cast<const h8*>(ws + r * 128 + ((c ^ (r & 7)) << 4));
            }
#pragma unroll
            for (int a = 0; a < TN; ++a)
#pragma unroll
                for (int b = 0; b < TM; ++b)
                    acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf[a], xf[b], acc[a][b], 0, 0, 0);
        }
        if (kt + 1 < kt1) store_tile(cur ^ 1);
        __syncthreads();
    }

    int m_of[TM];
#pragma unroll
    for (int b = 0; b < TM; ++b) {
        const int m = m_base + wm * (BM / 2) + b * 16 + frow;
        m_of[b] = m < p.M ? m : -1;
    }
    int slab_of[BM / 64];
#pragma unroll
    for (int bp = 0; bp < BM / 64; ++bp) {
        const int r = m_base + wm * (BM / 2) + bp * 32;
        slab_of[bp] = r < p.M ? (r >> 5) : -1;
    }
    igemm_epilogue<BM, BN>(p, acc, m_of, n_base + wn * (BN / 2), fq, 0, slab_of);
}

template <int BM, int BN>
static int launch_conv_down(IgemmParams& p, hipStream_t s) {
    constexpr int smem = 2 * (BM + BN) * 128;
    static LcmDevOnce attr_once;
    if (auto once_guard = attr_once.first()) {
        once_guard.check(hipFuncSetAttribute(reinterpret_cast<const void*>(&conv_down_kernel<BM, BN>),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, smem));
    }
    p.mtiles = (p.M + BM - 1) / BM;
    p.ntiles = p.N / BN;
    char nm[64];
    snprintf(nm, sizeof(nm), "conv_down_kernel<%d, %d>%s", BM, BN, p.splits > 1 ? " +splitk" : "");
    lcm_prof_start(nm, s);
    hipLaunchKernelGGL((conv_down_kernel<BM, BN>), dim3(p.mtiles * p.ntiles, p.splits, 1), dim3(256), smem, s, p);
    lcm_prof_stop(s);
    LCM_CHECK_LAUNCH("conv3x3_down");
    if (p.splits > 1) {
        lcm_launch_splitk_reduce(p, s);
        LCM_CHECK_LAUNCH("splitk_reduce");
    }
    return LCM_OK;
}

extern "C" int lcm_conv3x3_down_f16(const void* in, const void* W, const void* bias, void* out, int B, int Hin, int Win, int Cin,
                                    int Cout, void* stats_out, int64_t stats_bytes, int* slabs_per_image, void* stream) {
    LCM_REQUIRE(in && W && out, "conv3x3_down: null pointer");
    LCM_REQUIRE(B > 0 && Hin >= 2 && Win >= 2, "conv3x3_down: bad shape B=%d %dx%d (each side >= 2)", B, Hin, Win);
    LCM_REQUIRE(Cin % 64 == 0 && Cout % 64 == 0 && Cin > 0 && Cout > 0, "conv3x3_down: Cin=%d Cout=%d must be multiples of 64", Cin, Cout);
    LCM_REQUIRE((long long)B * Hin * Win < (1ll << 30), "conv3x3_down: input too large");
    LCM_REQUIRE(!stats_out || slabs_per_image, "conv3x3_down: stats_out needs slabs_per_image");
    hipStream_t s = (hipStream_t)stream;
    IgemmParams p = {};
    p.A = (const half_t*)in; p.W = (const half_t*)W; p.bias = (const half_t*)bias; p.out = (half_t*)out;
    p.Hin = Hin; p.Win = Win; p.Cin = Cin; p.stride = 2; p.ups = 0;
    p.Hout = (Hin + 1 - 3) / 2 + 1; p.Wout = (Win + 1 - 3) / 2 + 1;
    const int img_rows = p.Hout * p.Wout;
    p.M = B * img_rows; p.N = Cout; p.K = 9 * Cin;
    p.ldo = Cout; p.ldr = Cout; p.rows_per_batch = img_rows; p.img_rows = img_rows;
    p.epi = 0; p.out_scale = 1.0f; p.n_iters = 1; p.seg_parts = 1; p.rg_kind = 0;
    long long wsb = 0;
    p.ws = lcm_splitk_workspace(&wsb, s);
    p.splits = 1;
    if (p.ws) {                                   // no workspace registered: the library never splits
        const int sp = lcm_canonical_splits(1, img_rows, p.N, p.K, 1, 0);
        if (sp < 0) return sp;
        p.splits = sp;
    }
    if (p.splits > 1 && (long long)p.splits * p.M * p.N * 4 > wsb) {
        lcm_set_error("conv3x3_down: split-K workspace too small: %d x %d x %d fp32 slabs need %lld MB, have %lld MB "
                      "(lcm_set_workspace / LCM_SPLITK_WS_MB)", p.splits, p.M, p.N,
                      ((long long)p.splits * p.M * p.N * 4 + (1 << 20) - 1) >> 20, wsb >> 20);
        return LCM_EINVAL;
    }
    if (slabs_per_image) *slabs_per_image = 0;
    p.stats = (float*)stats_out; p.stats_cap = stats_bytes;
    if (p.stats) {
        if (p.N <= 2048 && img_rows % 32 == 0) {
            LCM_STATS_FIT(p, img_rows / 32, B, "conv3x3_down");
            *slabs_per_image = img_rows / 32;     // canonical 32-row slabs (igemm_epilogue / splitk_reduce_kernel)
        } else {
            p.stats = nullptr;
        }
    }
    if (p.M >= 4096 && p.N % 128 == 0) return launch_conv_down<128, 128>(p, s);
    return launch_conv_down<64, 64>(p, s);
}
