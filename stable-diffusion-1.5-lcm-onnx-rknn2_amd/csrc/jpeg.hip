// RGB8 image on the device -> quantised JPEG coefficients, one launch: everything of a baseline 4:2:0 JPEG except the entropy
// coding (jpeg.cpp does that on the host, one MCU row per restart interval).  The arithmetic is fixed (include/lcm_hip.h):
// libjpeg's 16-bit integer RGB -> YCbCr, h2v2 chroma means with the alternating bias, edge replication to whole 16x16 MCUs,
// level shift, separable fp32 8x8 DCT-II (even / odd halves), reciprocal-multiply quantisation with round to nearest, zigzag.
//
// A workgroup of 256 threads owns 16 consecutive MCUs of one MCU row (a 256 x 16 pixel strip, 12 KB of RGB):
//   1. the strip's rows come in as aligned 16-byte loads into LDS, at their own misalignment (any pitch, any base);
//   2. every thread turns 4 x 2 pixels (three dwords per row, re-aligned with v_alignbyte) into 8 luma bytes and 2 Cb / Cr
//      means; the planes stay in LDS as uint8, their rows padded so that the eight rows of a block fall on different banks;
//   3. 8 threads per block: row transform from the planes into an fp32 LDS tile (block stride 72 floats: the column reads
//      of four blocks of a half-wave hit 32 different banks), column transform, quantise, scatter to zigzag order in LDS;
//   4. the strip's 16 x 6 x 128 bytes leave as one contiguous run of 16-byte stores.
// The launch is memory-bound (3 B/pixel in, 3 B/pixel out); no atomics, no inter-workgroup traffic.
#include "common.h"

extern "C" int lcm_jpeg_quant_tables(int quality, uint8_t* out);       // jpeg.cpp
extern "C" long long lcm_jpeg_coef_bytes(int W, int H);

namespace {

constexpr int JPEG_NM = 16;                  // MCUs per workgroup
constexpr int JPEG_THREADS = 256;
constexpr int RAW_CHUNKS = 49;               // 16-byte chunks that cover 768 bytes at any misalignment
constexpr int RAW_STRIDE = 800;              // bytes per staged row: 49 chunks + the dword the re-alignment reads past them
constexpr int Y_STRIDE = 272;                // bytes per luma row in LDS (256 + 16: 68 dwords, rows 4 banks apart)
constexpr int C_STRIDE = 144;                // bytes per chroma row in LDS (128 + 16)
constexpr int T_STRIDE = 72;                 // floats per block in the transpose tile (64 + 8)

struct JpegQuant { float recip[128]; };      // 1 / table entry, natural order: luma, then chroma

// natural index -> position in the zigzag sequence
__constant__ uint8_t JPEG_ZPOS[64] = {0,  1,  5,  6,  14, 15, 27, 28, 2,  4,  7,  13, 16, 26, 29, 42, 3,  8,  12, 17, 25, 30,
                                      41, 43, 9,  11, 18, 24, 31, 40, 44, 53, 10, 19, 23, 32, 39, 45, 52, 54, 20, 22, 33, 38,
                                      46, 51, 55, 60, 21, 34, 37, 47, 50, 56, 59, 61, 35, 36, 48, 49, 57, 58, 62, 63};

// 8-point DCT-II, X(u) = C(u)/2 sum_i x(i) cos((2i+1) u pi / 16), C(0) = 1/sqrt(2): applied along both axes it is the JPEG
// forward transform (DC = sum / 8)
__device__ __forceinline__ void dct8(const float* x, float* X) {
    constexpr float A = 0.35355339059327379f;            // 1 / (2 sqrt 2)
    constexpr float C1 = 0.49039264020161522f, C2 = 0.46193976625564337f, C3 = 0.41573480615127262f;      // cos(k pi/16) / 2
    constexpr float C5 = 0.27778511650980111f, C6 = 0.19134171618254489f, C7 = 0.09754516100806413f;
    const float s0 = x[0] + x[7], s1 = x[1] + x[6], s2 = x[2] + x[5], s3 = x[3] + x[4];
    const float d0 = x[0] - x[7], d1 = x[1] - x[6], d2 = x[2] - x[5], d3 = x[3] - x[4];
    const float e0 = s0 + s3, e1 = s1 + s2, e2 = s0 - s3, e3 = s1 - s2;
    X[0] = A * (e0 + e1);
    X[4] = A * (e0 - e1);
    X[2] = C2 * e2 + C6 * e3;
    X[6] = C6 * e2 - C2 * e3;
    X[1] = C1 * d0 + C3 * d1 + C5 * d2 + C7 * d3;
    X[3] = C3 * d0 - C7 * d1 - C1 * d2 - C5 * d3;
    X[5] = C5 * d0 - C1 * d1 + C7 * d2 + C3 * d3;
    X[7] = C7 * d0 - C5 * d1 + C3 * d2 - C1 * d3;
}

__global__ __launch_bounds__(JPEG_THREADS) void jpeg_dct_rgb8_kernel(const uint8_t* __restrict__ rgb, int W, int H, long long pitch,
                                                                      JpegQuant q, int mcus_x, int16_t* __restrict__ coefs) {
    __shared__ __attribute__((aligned(16))) uint8_t raw[16 * RAW_STRIDE];        // staged RGB rows; later the zigzag output
    __shared__ __attribute__((aligned(16))) uint8_t yp[16 * Y_STRIDE];
    __shared__ __attribute__((aligned(16))) uint8_t cbp[8 * C_STRIDE];
    __shared__ __attribute__((aligned(16))) uint8_t crp[8 * C_STRIDE];
    __shared__ __attribute__((aligned(16))) float tile[JPEG_NM * 6 * T_STRIDE];
    __shared__ float qrecip[128];
    __shared__ uint8_t zpos[64];

    const int tid = threadIdx.x;
    const int mcu0 = blockIdx.x * JPEG_NM, mrow = blockIdx.y;
    const int nm = min(JPEG_NM, mcus_x - mcu0);          // MCUs of this strip
    const int x0 = mcu0 * 16, y0 = mrow * 16;
    const int npx = min(nm * 16, W - x0);                // pixels of the strip that exist; the rest replicate the last one
    const int nb = 3 * npx;
    const uintptr_t lo = (uintptr_t)rgb, hi = lo + (unsigned long long)(H - 1) * pitch + 3ull * W;

    if (tid < 128) qrecip[tid] = q.recip[tid];
    if (tid < 64) zpos[tid] = JPEG_ZPOS[tid];

    // 1. stage the rows: aligned 16-byte chunks, LDS byte i of a row = global byte (row start - m + i)
    for (int idx = tid; idx < 16 * RAW_CHUNKS; idx += JPEG_THREADS) {
        const int r = idx / RAW_CHUNKS, j = idx - r * RAW_CHUNKS;
        const uintptr_t p = lo + (unsigned long long)min(y0 + r, H - 1) * pitch + 3ull * x0;
        const int m = (int)(p & 15);
        if (16 * j < m + nb) {
            const uintptr_t ga = p - m + 16 * j;
            uint4 v;
            if (ga >= lo && ga + 16 <= hi) {
                v = *(const uint4*)ga;
            } else {                                     // a chunk that straddles the ends of the image: bytes, each one checked
                uint32_t w[4] = {0, 0, 0, 0};
                for (int k = 0; k < 16; ++k)
                    if (ga + k >= lo && ga + k < hi) w[k >> 2] |= (uint32_t)(*(const uint8_t*)(ga + k)) << (8 * (k & 3));
                v = make_uint4(w[0], w[1], w[2], w[3]);
            }
            *(uint4*)(raw + r * RAW_STRIDE + 16 * j) = v;
        }
    }
    __syncthreads();
    // replicate the last pixel to the right up to the MCU boundary (at most 15 pixels, only in the image's last strip)
    const int padb = 3 * (nm * 16 - npx);
    for (int idx = tid; idx < 16 * padb; idx += JPEG_THREADS) {
        const int r = idx / padb, k = idx - r * padb;
        const int m = (int)((lo + (unsigned long long)min(y0 + r, H - 1) * pitch + 3ull * x0) & 15);
        uint8_t* row = raw + r * RAW_STRIDE + m + 3 * (npx - 1);
        row[3 + k] = row[k % 3];
    }
    if (padb) __syncthreads();

    // 2. colour conversion and chroma sampling: 4 x 2 pixels per task
    const uint32_t* rawd = (const uint32_t*)raw;
    for (int t = tid; t < 8 * 64; t += JPEG_THREADS) {
        const int rp = t >> 6, gp = t & 63;
        if (gp * 4 >= nm * 16) continue;
        int cb[2][4], cr[2][4];
#pragma unroll
        for (int rr = 0; rr < 2; ++rr) {
            const int row = 2 * rp + rr;
            const int m = (int)((lo + (unsigned long long)min(y0 + row, H - 1) * pitch + 3ull * x0) & 15);
            const int off = row * RAW_STRIDE + m + 12 * gp;
            const uint32_t* d = rawd + (off >> 2);
            const uint32_t w0 = d[0], w1 = d[1], w2 = d[2], w3 = d[3];
            const uint32_t sh = (uint32_t)off & 3;
            const uint32_t pk[3] = {__builtin_amdgcn_alignbyte(w1, w0, sh), __builtin_amdgcn_alignbyte(w2, w1, sh),
                                    __builtin_amdgcn_alignbyte(w3, w2, sh)};
            uint32_t ypack = 0;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int R = (pk[(3 * i) >> 2] >> (8 * ((3 * i) & 3))) & 255;
                const int G = (pk[(3 * i + 1) >> 2] >> (8 * ((3 * i + 1) & 3))) & 255;
                const int B = (pk[(3 * i + 2) >> 2] >> (8 * ((3 * i + 2) & 3))) & 255;
                const int Y = (19595 * R + 38470 * G + 7471 * B + 32768) >> 16;
                cb[rr][i] = (-11059 * R - 21709 * G + 32768 * B + (128 << 16) + 32767) >> 16;
                cr[rr][i] = (32768 * R - 27439 * G - 5329 * B + (128 << 16) + 32767) >> 16;
                ypack |= (uint32_t)Y << (8 * i);
            }
            *(uint32_t*)(yp + row * Y_STRIDE + 4 * gp) = ypack;
        }
        // output columns 2 gp (even: bias 1) and 2 gp + 1 (odd: bias 2)
        const int b0 = (cb[0][0] + cb[0][1] + cb[1][0] + cb[1][1] + 1) >> 2, b1 = (cb[0][2] + cb[0][3] + cb[1][2] + cb[1][3] + 2) >> 2;
        const int r0 = (cr[0][0] + cr[0][1] + cr[1][0] + cr[1][1] + 1) >> 2, r1 = (cr[0][2] + cr[0][3] + cr[1][2] + cr[1][3] + 2) >> 2;
        *(uint16_t*)(cbp + rp * C_STRIDE + 2 * gp) = (uint16_t)(b0 | (b1 << 8));
        *(uint16_t*)(crp + rp * C_STRIDE + 2 * gp) = (uint16_t)(r0 | (r1 << 8));
    }
    __syncthreads();

    // 3a. rows: thread (block b, row r) -> tile[b][r][0..7]
    const int nblk = nm * 6;
    for (int t = tid; t < JPEG_NM * 6 * 8; t += JPEG_THREADS) {
        const int b = t >> 3, r = t & 7;
        if (b >= nblk) continue;
        const int mcu = b / 6, k = b - mcu * 6;
        const uint8_t* src = k < 4 ? yp + ((k >> 1) * 8 + r) * Y_STRIDE + mcu * 16 + (k & 1) * 8
                                   : (k == 4 ? cbp : crp) + r * C_STRIDE + mcu * 8;
        const uint2 v = *(const uint2*)src;
        float x[8], X[8];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            x[i] = (float)((int)((v.x >> (8 * i)) & 255) - 128);
            x[4 + i] = (float)((int)((v.y >> (8 * i)) & 255) - 128);
        }
        dct8(x, X);
        float4* dst = (float4*)(tile + b * T_STRIDE + r * 8);
        dst[0] = make_float4(X[0], X[1], X[2], X[3]);
        dst[1] = make_float4(X[4], X[5], X[6], X[7]);
    }
    __syncthreads();
    // 3b. columns: thread (block b, column c) -> quantised coefficients (v, c), v = 0..7, to their zigzag places
    int16_t* outb = (int16_t*)raw;
    for (int t = tid; t < JPEG_NM * 6 * 8; t += JPEG_THREADS) {
        const int b = t >> 3, c = t & 7;
        if (b >= nblk) continue;
        const int k = b % 6;
        const float* src = tile + b * T_STRIDE + c;
        float x[8], X[8];
#pragma unroll
        for (int v = 0; v < 8; ++v) x[v] = src[v * 8];
        dct8(x, X);
        const float* qr = qrecip + (k < 4 ? 0 : 64);
#pragma unroll
        for (int v = 0; v < 8; ++v) {
            const int n = v * 8 + c;
            const float lim = n == 0 ? 2047.0f : 1023.0f;
            const float val = fminf(fmaxf(rintf(X[v] * qr[n]), -lim), lim);
            outb[b * 64 + zpos[n]] = (int16_t)(int)val;
        }
    }
    __syncthreads();
    // 4. the strip's blocks are one contiguous run of the output
    uint4* dst = (uint4*)(coefs + ((long long)mrow * mcus_x + mcu0) * 384);
    const uint4* so = (const uint4*)raw;
    for (int idx = tid; idx < nm * 48; idx += JPEG_THREADS) dst[idx] = so[idx];
}

}  // namespace

extern "C" int lcm_jpeg_dct_rgb8(const void* rgb, int W, int H, long long pitch, int quality, void* coefs, long long coefs_bytes,
                                 void* stream) {
    LCM_REQUIRE(rgb && coefs, "jpeg_dct_rgb8: null pointer");
    LCM_REQUIRE(W >= 1 && H >= 1 && W <= 65535 && H <= 65535, "jpeg_dct_rgb8: bad shape %dx%d (1..65535 each)", W, H);
    LCM_REQUIRE(pitch >= 3ll * W, "jpeg_dct_rgb8: pitch %lld < 3 * width %d", pitch, W);
    LCM_REQUIRE(quality >= 1 && quality <= 100, "jpeg_dct_rgb8: quality %d outside 1..100", quality);
    LCM_REQUIRE(coefs_bytes >= lcm_jpeg_coef_bytes(W, H), "jpeg_dct_rgb8: coefficient buffer %lld < %lld bytes", coefs_bytes,
                lcm_jpeg_coef_bytes(W, H));
    LCM_REQUIRE(((uintptr_t)coefs & 15) == 0, "jpeg_dct_rgb8: coefficient buffer must be 16-byte aligned");
    uint8_t tab[128];
    if (lcm_jpeg_quant_tables(quality, tab) != LCM_OK) return LCM_EINVAL;
    JpegQuant q;
    for (int i = 0; i < 128; ++i) q.recip[i] = 1.0f / (float)tab[i];
    const int mcus_x = (W + 15) / 16, mcus_y = (H + 15) / 16;
    hipStream_t s = (hipStream_t)stream;
    lcm_prof_start("jpeg_dct_rgb8_kernel", s);
    hipLaunchKernelGGL(jpeg_dct_rgb8_kernel, dim3((unsigned)((mcus_x + JPEG_NM - 1) / JPEG_NM), (unsigned)mcus_y), dim3(JPEG_THREADS),
                       0, s, (const uint8_t*)rgb, W, H, pitch, q, mcus_x, (int16_t*)coefs);
    lcm_prof_stop(s);
    LCM_CHECK_LAUNCH("jpeg_dct_rgb8");
    return LCM_OK;
}
