// Quantised JPEG coefficients on the device -> RGB8 pixels: everything of a JPEG decode after the entropy decoding (jpeg_dec.cpp
// does that on the host).  The arithmetic is integer and fixed (include/lcm_hip.h) and is the one libjpeg-turbo runs by default
// -- "slow integer" inverse DCT, "fancy" triangle chroma upsampling, 16-bit fixed point YCbCr -> RGB -- so the pixels equal
// ``PIL.Image.open(...).convert("RGB")`` byte for byte.  Two launches on the caller's stream:
//   1. jpeg_idct_kernel: a workgroup of 256 threads takes 32 consecutive blocks of the coefficient buffer.  Eight threads per
//      block: each loads 8 coefficients (one 16-byte load), multiplies them by their table entries and scatters them from
//      zigzag to natural order into an int32 LDS tile (block stride 72: the column reads of four blocks of a half-wave hit 32
//      different banks); column pass, row pass, +128, clamp; every thread stores one 8-sample row of its block (8 bytes) into
//      the component's sample plane in the caller's work buffer.  Planes are whole blocks wide and high.
//   2. jpeg_upsample_rgb_kernel: a thread makes 4 consecutive pixels of one row: 4 luma samples (one dword), the chroma samples
//      it needs from the planes (the filters reach one chroma sample left / right and one chroma row up / down, clamped to the
//      component's own last sample -- not to the padded block edge), colour conversion, and three dword stores (bytes where the
//      row is misaligned or the group is cut by the right edge).
// Two launches because the chroma filter reads samples of the neighbouring blocks and MCU rows: a single launch would have to
// redo the inverse DCT of the chroma blocks around every tile for that halo.
// Streaming work: 2 B per coefficient in, 3 B per pixel out, plus the planes once out and once in.  No atomics.
#include "common.h"
#include <string.h>

#include "../../include/lcm_hip.h"      // lcm_jpeg_info

namespace {

constexpr int DEC_THREADS = 256;
constexpr int DEC_BLOCKS = 32;               // blocks per workgroup
constexpr int T_STRIDE = 72;                 // ints per block in the LDS tile (64 + 8)

struct DecQuant { uint8_t q[192]; };         // table entries of the (up to) three components, natural order

// zigzag position -> natural index
__constant__ uint8_t DEC_ZZ[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                   41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                   30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// One 8-point pass of the "slow integer" inverse DCT (Loeffler, Ligtenberg, Moschytz; 13-bit constants): out = descale(.., SH).
// 32-bit two's complement arithmetic that wraps -- written in uint32_t so that it is defined -- with an arithmetic shift.
template <int SH>
__device__ __forceinline__ void idct8(const uint32_t* d, int* o) {
    constexpr uint32_t F0_298 = 2446, F0_390 = (uint32_t)-3196, F0_541 = 4433, F0_765 = 6270, F0_899 = (uint32_t)-7373, F1_175 = 9633,
                       F1_501 = 12299, F1_847 = (uint32_t)-15137, F1_961 = (uint32_t)-16069, F2_053 = 16819, F2_562 = (uint32_t)-20995,
                       F3_072 = 25172;
    uint32_t z1 = (d[2] + d[6]) * F0_541;
    const uint32_t e2 = z1 + d[6] * F1_847, e3 = z1 + d[2] * F0_765;
    const uint32_t e0 = (d[0] + d[4]) << 13, e1 = (d[0] - d[4]) << 13;
    const uint32_t a10 = e0 + e3, a13 = e0 - e3, a11 = e1 + e2, a12 = e1 - e2;
    uint32_t t0 = d[7], t1 = d[5], t2 = d[3], t3 = d[1];
    z1 = t0 + t3;
    uint32_t z2 = t1 + t2, z3 = t0 + t2, z4 = t1 + t3;
    const uint32_t z5 = (z3 + z4) * F1_175;
    t0 *= F0_298; t1 *= F2_053; t2 *= F3_072; t3 *= F1_501;
    z1 *= F0_899; z2 *= F2_562;
    z3 = z3 * F1_961 + z5;
    z4 = z4 * F0_390 + z5;
    t0 += z1 + z3; t1 += z2 + z4; t2 += z2 + z3; t3 += z1 + z4;
    constexpr uint32_t RND = 1u << (SH - 1);
    o[0] = (int)(a10 + t3 + RND) >> SH; o[7] = (int)(a10 - t3 + RND) >> SH;
    o[1] = (int)(a11 + t2 + RND) >> SH; o[6] = (int)(a11 - t2 + RND) >> SH;
    o[2] = (int)(a12 + t1 + RND) >> SH; o[5] = (int)(a12 - t1 + RND) >> SH;
    o[3] = (int)(a13 + t0 + RND) >> SH; o[4] = (int)(a13 - t0 + RND) >> SH;
}

__device__ __forceinline__ uint32_t clamp8(int v) { return (uint32_t)min(max(v, 0), 255); }

// hs, vs: luma blocks per MCU along x and y; ncomp 1 or 3; ys / cs: bytes per row of the luma / chroma planes
__global__ __launch_bounds__(DEC_THREADS) void jpeg_idct_kernel(const int16_t* __restrict__ coefs, long long nblocks, int mcus_x, int hs,
                                                                 int vs, int ncomp, DecQuant q, uint8_t* __restrict__ work, int ys,
                                                                 long long y_bytes, int cs, long long c_bytes) {
    __shared__ __attribute__((aligned(16))) uint32_t tile[DEC_BLOCKS * T_STRIDE];
    __shared__ uint8_t qs[192];
    __shared__ uint8_t zz[64];
    const int tid = threadIdx.x;
    if (tid < 192) qs[tid] = q.q[tid];
    if (tid < 64) zz[tid] = DEC_ZZ[tid];
    __syncthreads();

    const int bl = tid >> 3, part = tid & 7;
    const long long g = (long long)blockIdx.x * DEC_BLOCKS + bl;
    const bool live = g < nblocks;
    const int ny = ncomp == 1 ? 1 : hs * vs, bpm = ncomp == 1 ? 1 : ny + 2;
    const long long mcu = g / bpm;
    const int k = (int)(g - mcu * bpm);
    const int comp = k < ny ? 0 : k - ny + 1;
    uint32_t* t = tile + bl * T_STRIDE;
    if (live) {
        const uint4 v = *(const uint4*)(coefs + g * 64 + part * 8);
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
        const uint8_t* qc = qs + comp * 64;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int c = (int)(int16_t)(w[i >> 1] >> (16 * (i & 1)));
            const int nat = zz[part * 8 + i];
            t[nat] = (uint32_t)(c * (int)qc[nat]);
        }
    }
    __syncthreads();
    if (live) {                                  // columns: thread `part` owns column `part` of its block
        uint32_t d[8];
        int o[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) d[r] = t[r * 8 + part];
        idct8<11>(d, o);
#pragma unroll
        for (int r = 0; r < 8; ++r) t[r * 8 + part] = (uint32_t)o[r];
    }
    __syncthreads();
    if (live) {                                  // rows: thread `part` owns row `part`
        const uint4 lo = *(const uint4*)(t + part * 8), hi = *(const uint4*)(t + part * 8 + 4);
        const uint32_t d[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
        int o[8];
        idct8<18>(d, o);
        uint2 px;
        px.x = clamp8(o[0] + 128) | (clamp8(o[1] + 128) << 8) | (clamp8(o[2] + 128) << 16) | (clamp8(o[3] + 128) << 24);
        px.y = clamp8(o[4] + 128) | (clamp8(o[5] + 128) << 8) | (clamp8(o[6] + 128) << 16) | (clamp8(o[7] + 128) << 24);
        const int my = (int)(mcu / mcus_x), mx = (int)(mcu - (long long)my * mcus_x);
        uint8_t* dst;
        if (comp == 0) {
            const int bx = mx * hs + (ncomp == 1 ? 0 : k % hs), by = my * vs + (ncomp == 1 ? 0 : k / hs);
            dst = work + ((long long)by * 8 + part) * ys + bx * 8;
        } else {
            dst = work + y_bytes + (comp - 1) * c_bytes + ((long long)my * 8 + part) * cs + mx * 8;
        }
        *(uint2*)dst = px;
    }
}

// cw x ch: the chroma component's own samples (ceil(W h / hmax) x ceil(H v / vmax)); sampling as in lcm_jpeg_info
__global__ __launch_bounds__(DEC_THREADS) void jpeg_upsample_rgb_kernel(const uint8_t* __restrict__ work, int W, int H, int ncomp,
                                                                         int sampling, int ys, long long y_bytes, int cs,
                                                                         long long c_bytes, int cw, int ch, uint8_t* __restrict__ out,
                                                                         long long pitch) {
    const int x0 = (blockIdx.x * DEC_THREADS + threadIdx.x) * 4, y = blockIdx.y;
    if (x0 >= W) return;
    const uint32_t yw = *(const uint32_t*)(work + (long long)y * ys + x0);
    int Y[4], cb[4], cr[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) Y[i] = (yw >> (8 * i)) & 255;
    if (ncomp == 3) {
        const uint8_t* pb = work + y_bytes;
        const uint8_t* pr = pb + c_bytes;
        if (sampling == 0) {
            const uint32_t b = *(const uint32_t*)(pb + (long long)y * cs + x0), r = *(const uint32_t*)(pr + (long long)y * cs + x0);
#pragma unroll
            for (int i = 0; i < 4; ++i) { cb[i] = (b >> (8 * i)) & 255; cr[i] = (r >> (8 * i)) & 255; }
        } else {
            const bool fancy = cw > 2;           // libjpeg filters only components more than two samples wide
            const int c0 = x0 >> 1;
            // the four chroma columns c0 - 1 .. c0 + 2, clamped to the component, of one or two chroma rows
            int col[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) col[j] = min(max(c0 - 1 + j, 0), cw - 1);
            int sb[4], sr[4];                    // sampling 1: the samples; sampling 2: 3 * near row + far row
            if (sampling == 1) {
                const long long row = (long long)y * cs;
#pragma unroll
                for (int j = 0; j < 4; ++j) { sb[j] = pb[row + col[j]]; sr[j] = pr[row + col[j]]; }
            } else {
                const int cy = y >> 1, cn = (y & 1) ? min(cy + 1, ch - 1) : max(cy - 1, 0);
                const long long r0 = (long long)cy * cs, r1 = (long long)cn * cs;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int nb = pb[r0 + col[j]], nr = pr[r0 + col[j]];
                    sb[j] = fancy ? 3 * nb + pb[r1 + col[j]] : nb;
                    sr[j] = fancy ? 3 * nr + pr[r1 + col[j]] : nr;
                }
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int j = 1 + (i >> 1);      // this pixel's chroma column within col[]; its neighbour is j - 1 or j + 1
                const int c = c0 + (i >> 1);
                if (!fancy) {
                    cb[i] = sb[j]; cr[i] = sr[j];
                } else if (sampling == 1) {
                    if (i & 1) {
                        cb[i] = c >= cw - 1 ? sb[j] : (3 * sb[j] + sb[j + 1] + 2) >> 2;
                        cr[i] = c >= cw - 1 ? sr[j] : (3 * sr[j] + sr[j + 1] + 2) >> 2;
                    } else {
                        cb[i] = c == 0 ? sb[j] : (3 * sb[j] + sb[j - 1] + 1) >> 2;
                        cr[i] = c == 0 ? sr[j] : (3 * sr[j] + sr[j - 1] + 1) >> 2;
                    }
                } else {
                    if (i & 1) { cb[i] = (3 * sb[j] + sb[j + 1] + 7) >> 4; cr[i] = (3 * sr[j] + sr[j + 1] + 7) >> 4; }
                    else { cb[i] = (3 * sb[j] + sb[j - 1] + 8) >> 4; cr[i] = (3 * sr[j] + sr[j - 1] + 8) >> 4; }
                }
            }
        }
    }
    uint8_t px[12];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if (ncomp == 3) {
            const int b = cb[i] - 128, r = cr[i] - 128;
            px[3 * i] = (uint8_t)clamp8(Y[i] + ((91881 * r + 32768) >> 16));
            px[3 * i + 1] = (uint8_t)clamp8(Y[i] + ((-22554 * b - 46802 * r + 32768) >> 16));
            px[3 * i + 2] = (uint8_t)clamp8(Y[i] + ((116130 * b + 32768) >> 16));
        } else {
            px[3 * i] = px[3 * i + 1] = px[3 * i + 2] = (uint8_t)Y[i];
        }
    }
    uint8_t* dst = out + (long long)y * pitch + 3ll * x0;
    const int npx = min(4, W - x0);
    if (npx == 4 && ((uintptr_t)dst & 3) == 0) {
        uint32_t* d4 = (uint32_t*)dst;
#pragma unroll
        for (int j = 0; j < 3; ++j)
            d4[j] = (uint32_t)px[4 * j] | ((uint32_t)px[4 * j + 1] << 8) | ((uint32_t)px[4 * j + 2] << 16) | ((uint32_t)px[4 * j + 3] << 24);
    } else {
        for (int j = 0; j < 3 * npx; ++j) dst[j] = px[j];
    }
}

}  // namespace

extern "C" int lcm_jpeg_idct_rgb8(const void* coefs, long long coefs_bytes, const lcm_jpeg_info* info, void* work, long long work_bytes,
                                  void* rgb_out, long long pitch, void* stream) {
    LCM_REQUIRE(coefs && info && work && rgb_out, "jpeg_idct_rgb8: null pointer");
    const int W = info->width, H = info->height, nc = info->ncomp, sm = info->sampling;
    LCM_REQUIRE(W >= 1 && H >= 1 && W <= 65535 && H <= 65535, "jpeg_idct_rgb8: bad shape %dx%d (1..65535 each)", W, H);
    LCM_REQUIRE(nc == 1 || nc == 3, "jpeg_idct_rgb8: %d components (1 or 3)", nc);
    LCM_REQUIRE(sm >= 0 && sm <= 2 && (nc == 3 || sm == 0), "jpeg_idct_rgb8: bad sampling class %d for %d components", sm, nc);
    const int hs = sm >= 1 ? 2 : 1, vs = sm == 2 ? 2 : 1;
    const int mcus_x = (W + 8 * hs - 1) / (8 * hs), mcus_y = (H + 8 * vs - 1) / (8 * vs);
    const int bpm = nc == 1 ? 1 : hs * vs + 2;
    const long long nblocks = (long long)mcus_x * mcus_y * bpm;
    LCM_REQUIRE(coefs_bytes >= nblocks * 128, "jpeg_idct_rgb8: coefficient buffer %lld < %lld bytes", coefs_bytes, nblocks * 128);
    LCM_REQUIRE(work_bytes >= nblocks * 64, "jpeg_idct_rgb8: work buffer %lld < %lld bytes", work_bytes, nblocks * 64);
    LCM_REQUIRE(pitch >= 3ll * W, "jpeg_idct_rgb8: pitch %lld < 3 * width %d", pitch, W);
    LCM_REQUIRE(((uintptr_t)coefs & 15) == 0 && ((uintptr_t)work & 15) == 0, "jpeg_idct_rgb8: coefficient and work buffers must be 16-byte aligned");
    DecQuant q;
    memcpy(q.q, info->qt, 192);
    const int ys = mcus_x * hs * 8, cs = mcus_x * 8;
    const long long y_bytes = (long long)ys * mcus_y * vs * 8, c_bytes = (long long)cs * mcus_y * 8;
    const int cw = (W + hs - 1) / hs, ch = (H + vs - 1) / vs;
    hipStream_t s = (hipStream_t)stream;
    lcm_prof_start("jpeg_idct_kernel", s);
    hipLaunchKernelGGL(jpeg_idct_kernel, dim3((unsigned)((nblocks + DEC_BLOCKS - 1) / DEC_BLOCKS)), dim3(DEC_THREADS), 0, s,
                       (const int16_t*)coefs, nblocks, mcus_x, hs, vs, nc, q, (uint8_t*)work, ys, y_bytes, cs, c_bytes);
    lcm_prof_stop(s);
    LCM_CHECK_LAUNCH("jpeg_idct_rgb8 (idct)");
    lcm_prof_start("jpeg_upsample_rgb_kernel", s);
    hipLaunchKernelGGL(jpeg_upsample_rgb_kernel, dim3((unsigned)(((W + 3) / 4 + DEC_THREADS - 1) / DEC_THREADS), (unsigned)H),
                       dim3(DEC_THREADS), 0, s, (const uint8_t*)work, W, H, nc, sm, ys, y_bytes, cs, c_bytes, cw, ch, (uint8_t*)rgb_out,
                       pitch);
    lcm_prof_stop(s);
    LCM_CHECK_LAUNCH("jpeg_idct_rgb8 (upsample)");
    return LCM_OK;
}
