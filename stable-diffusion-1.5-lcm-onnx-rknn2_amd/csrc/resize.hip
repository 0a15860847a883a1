// The Lanczos resampler on the device (include/lcm_hip.h "Lanczos resampler"): PIL's 8-bit
// ImagingResample as two integer passes over fixed-point tables that the host built (csrc/resize.cpp) -- horizontal into a
// rounded and clipped uint8 intermediate, then vertical -- so that a picture fitted here has the bytes of
// Image.resize(..., Image.LANCZOS).  Each pass is one launch; no workgroup waits for another and nothing is read back.
//
// A table holds, per output of the window, (first source index, taps) and `ksize` 22-bit coefficients.  A window position
// outside the full output grid was given the nearest output's row by the host, and a pass that maps rows or columns without
// resampling them (the axis keeps its size) clamps the same way: that is the edge replication of resize_mode 2.
#include "common.h"

extern "C" long long lcm_resize_table_bytes(int in, int out, int n);
extern "C" int lcm_resize_ksize(int in, int out);
extern "C" int lcm_resize_span(int in, int out, int o0, int n, int* first, int* last);
extern "C" int lcm_resize_max_span(int in, int out, int o0, int n, int tile);
extern "C" int lcm_resize_passes(int sw, int sh, int out_w, int out_h);

#define RS_BITS 22
#define RS_THREADS 256
#define RS_COEF_INTS 4096           // 16 KiB of coefficients per workgroup: tile columns x ksize
#define RS_PIX_BYTES 32768          // 32 KiB of staged source rows (a whole 8192-pixel RGB row is 24 KiB)
#define RS_MAX_TILE 64

namespace {

__device__ __forceinline__ int rs_clamp(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }
__device__ __forceinline__ uint8_t rs_clip8(int acc) { return (uint8_t)rs_clamp(acc >> RS_BITS, 0, 255); }

// Horizontal pass.  A workgroup owns TX neighbouring output columns of TY rows.  The source pixels those columns read are one
// contiguous byte range of each row (bounds do not decrease with the column): it is staged in LDS once, with the columns'
// coefficients (read from the table directly when ksize alone exceeds the LDS share: TX is 1 then).  Output row j reads source
// row clamp(j + yoff, 0, hsrc - 1).  The host sized TX and TY so that TY x span fits; a tile that would not is left alone.
template <int C>
__global__ void __launch_bounds__(RS_THREADS)
resize_h_kernel(const uint8_t* __restrict__ src, long long src_pitch, int yoff, int hsrc, const int* __restrict__ bounds,
                const int* __restrict__ kk, int ksize, uint8_t* __restrict__ dst, long long dst_pitch, int w, int rows, int TX,
                int TY, int stage_coefs) {
    __shared__ int kcoef[RS_COEF_INTS];
    __shared__ uint8_t pix[RS_PIX_BYTES];
    const int tid = threadIdx.x;
    const int i0 = blockIdx.x * TX, j0 = blockIdx.y * TY;
    const int ni = min(TX, w - i0), nj = min(TY, rows - j0);
    const int px0 = bounds[2 * i0];
    const int span = (bounds[2 * (i0 + ni - 1)] + bounds[2 * (i0 + ni - 1) + 1] - px0) * C;
    if (span <= 0 || (long long)span * nj > RS_PIX_BYTES) return;
    for (int n = tid; n < nj * span; n += RS_THREADS) {
        const int r = n / span, b = n - r * span;
        const int sy = rs_clamp(j0 + r + yoff, 0, hsrc - 1);
        pix[n] = src[(long long)sy * src_pitch + (long long)px0 * C + b];
    }
    if (stage_coefs)
        for (int n = tid; n < ni * ksize; n += RS_THREADS) kcoef[n] = kk[(long long)i0 * ksize + n];
    __syncthreads();
    for (int n = tid; n < nj * ni * C; n += RS_THREADS) {
        const int t = n / C, c = n - t * C;
        const int r = t / ni, i = t - r * ni;
        const int xmin = bounds[2 * (i0 + i)] - px0, cnt = bounds[2 * (i0 + i) + 1];
        const uint8_t* q = pix + r * span + xmin * C + c;
        int acc = 1 << (RS_BITS - 1);
        if (stage_coefs) {
            const int* k = kcoef + i * ksize;
#pragma unroll 4
            for (int x = 0; x < cnt; ++x) acc += (int)q[x * C] * k[x];
        } else {
            const int* k = kk + (long long)(i0 + i) * ksize;
#pragma unroll 4
            for (int x = 0; x < cnt; ++x) acc += (int)q[x * C] * k[x];
        }
        dst[(long long)(j0 + r) * dst_pitch + (i0 + i) * C + c] = rs_clip8(acc);
    }
}

// Vertical pass.  A workgroup owns 256 neighbouring bytes of one output row: lanes run along x * C, so every load is a
// coalesced row segment (rows need no alignment), and the row's bounds and coefficients are the same in every lane.  Output
// pixel x reads source column clamp(x + xoff, 0, wsrc - 1); source row y of the table is row y - r0 of src.
__global__ void __launch_bounds__(RS_THREADS)
resize_v_kernel(const uint8_t* __restrict__ src, long long src_pitch, int r0, int xoff, int wsrc, int C,
                const int* __restrict__ bounds, const int* __restrict__ kk, int ksize, uint8_t* __restrict__ dst,
                long long dst_pitch, int w) {
    const int j = blockIdx.y;
    const int col = blockIdx.x * RS_THREADS + threadIdx.x;
    if (col >= w * C) return;
    const int px = col / C, c = col - px * C;
    const int sx = rs_clamp(px + xoff, 0, wsrc - 1);
    const int ymin = bounds[2 * j] - r0, cnt = bounds[2 * j + 1];
    const uint8_t* p = src + (long long)ymin * src_pitch + sx * C + c;
    const int* k = kk + (long long)j * ksize;
    int acc = 1 << (RS_BITS - 1);
#pragma unroll 4
    for (int y = 0; y < cnt; ++y) acc += (int)p[(long long)y * src_pitch] * k[y];
    dst[(long long)j * dst_pitch + col] = rs_clip8(acc);
}

inline long long pad16(long long v) { return (v + 15) & ~15ll; }

struct Geo {
    int passes, r0, r1;               // r0 .. r1: the source rows the vertical pass reads (all rows of the window without it)
    long long tab_h, tab_v, tmp;
};

int geometry(const char* who, int C, int sw, int sh, int out_w, int out_h, int x0, int y0, int w, int h, Geo* g) {
    LCM_REQUIRE(C == 1 || C == 3, "%s: %d channels (1 or 3)", who, C);
    LCM_REQUIRE(sw >= 1 && sw <= 8192 && sh >= 1 && sh <= 8192, "%s: source %dx%d outside 1..8192", who, sw, sh);
    LCM_REQUIRE(out_w >= 1 && out_w <= 4096 && out_h >= 1 && out_h <= 4096, "%s: output %dx%d outside 1..4096", who, out_w, out_h);
    LCM_REQUIRE(w >= 1 && w <= 4096 && h >= 1 && h <= 4096, "%s: window %dx%d outside 1..4096", who, w, h);
    LCM_REQUIRE(x0 >= -4096 && x0 <= 4096 && y0 >= -4096 && y0 <= 4096, "%s: window origin %d,%d outside -4096..4096", who, x0, y0);
    g->passes = lcm_resize_passes(sw, sh, out_w, out_h);
    g->tab_h = (g->passes & 1) ? lcm_resize_table_bytes(sw, out_w, w) : 0;
    g->tab_v = (g->passes & 2) ? lcm_resize_table_bytes(sh, out_h, h) : 0;
    g->r0 = 0, g->r1 = 0, g->tmp = 0;
    if (g->passes == 3) {
        if (int rc = lcm_resize_span(sh, out_h, y0, h, &g->r0, &g->r1)) return rc;
        g->tmp = pad16((long long)(g->r1 - g->r0) * w * C);
    }
    return LCM_OK;
}

}  // namespace

extern "C" long long lcm_resize_ws_bytes(int C, int sw, int sh, int out_w, int out_h, int x0, int y0, int w, int h) {
    Geo g;
    if (geometry("resize_ws_bytes", C, sw, sh, out_w, out_h, x0, y0, w, h, &g)) return 0;
    return g.tab_h + g.tab_v + g.tmp;
}

extern "C" int lcm_resize_lanczos_u8(const void* src, long long src_stride, int C, int sw, int sh, int out_w, int out_h, int x0,
                                     int y0, int w, int h, void* dst, long long dst_stride, void* ws, long long ws_bytes,
                                     void* stream) {
    LCM_REQUIRE(src && dst && ws, "resize_lanczos_u8: null pointer");
    Geo g;
    if (int rc = geometry("resize_lanczos_u8", C, sw, sh, out_w, out_h, x0, y0, w, h, &g)) return rc;
    LCM_REQUIRE(src_stride >= (long long)sw * C, "resize_lanczos_u8: source stride %lld below a row of %d bytes", src_stride, sw * C);
    LCM_REQUIRE(dst_stride >= (long long)w * C, "resize_lanczos_u8: destination stride %lld below a row of %d bytes", dst_stride, w * C);
    const long long need = g.tab_h + g.tab_v + g.tmp;
    LCM_REQUIRE(ws_bytes >= need, "resize_lanczos_u8: workspace of %lld bytes, %lld needed", ws_bytes, need);
    LCM_REQUIRE((uintptr_t)ws % 16 == 0, "resize_lanczos_u8: the workspace must be 16-byte aligned");
    const uint8_t *s8 = (const uint8_t*)src, *w8 = (const uint8_t*)ws;
    uint8_t* d8 = (uint8_t*)dst;
    const long long src_len = (long long)(sh - 1) * src_stride + (long long)sw * C;
    const long long dst_len = (long long)(h - 1) * dst_stride + (long long)w * C;
    LCM_REQUIRE(s8 + src_len <= w8 || s8 >= w8 + need, "resize_lanczos_u8: the source overlaps the workspace");
    LCM_REQUIRE(d8 + dst_len <= w8 || d8 >= w8 + need, "resize_lanczos_u8: the destination overlaps the workspace");
    LCM_REQUIRE(d8 + dst_len <= s8 || d8 >= s8 + src_len, "resize_lanczos_u8: the destination overlaps the source");
    hipStream_t st = (hipStream_t)stream;
    const int* tab_h = (const int*)w8;
    const int* tab_v = (const int*)(w8 + g.tab_h);
    uint8_t* tmp = (uint8_t*)ws + g.tab_h + g.tab_v;
    if (g.passes & 1) {
        const int ksize = lcm_resize_ksize(sw, out_w);
        const bool both = g.passes == 3;
        const int rows = both ? g.r1 - g.r0 : h;
        const int stage = ksize <= RS_COEF_INTS;
        int TX = stage ? RS_COEF_INTS / ksize : 1;
        TX = TX > RS_MAX_TILE ? RS_MAX_TILE : TX;
        TX = TX > w ? w : TX;
        const int span = lcm_resize_max_span(sw, out_w, x0, w, TX);
        LCM_REQUIRE(span >= 1 && (long long)span * C <= RS_PIX_BYTES, "resize_lanczos_u8: a tile of %d columns reads %d source pixels", TX, span);
        int TY = RS_PIX_BYTES / (span * C);
        TY = TY > RS_MAX_TILE ? RS_MAX_TILE : TY;
        TY = TY > rows ? rows : TY;
        const dim3 grid((w + TX - 1) / TX, (rows + TY - 1) / TY);
        uint8_t* out = both ? tmp : d8;
        const long long out_pitch = both ? (long long)w * C : dst_stride;
        const int yoff = both ? g.r0 : y0;
        if (C == 3)
            hipLaunchKernelGGL(resize_h_kernel<3>, grid, dim3(RS_THREADS), 0, st, s8, src_stride, yoff, sh, tab_h, tab_h + 2 * w, ksize,
                               out, out_pitch, w, rows, TX, TY, stage);
        else
            hipLaunchKernelGGL(resize_h_kernel<1>, grid, dim3(RS_THREADS), 0, st, s8, src_stride, yoff, sh, tab_h, tab_h + 2 * w, ksize,
                               out, out_pitch, w, rows, TX, TY, stage);
        LCM_CHECK_LAUNCH("resize_lanczos_u8 (horizontal)");
    }
    if (g.passes & 2) {
        const int ksize = lcm_resize_ksize(sh, out_h);
        const bool both = g.passes == 3;
        const dim3 grid((w * C + RS_THREADS - 1) / RS_THREADS, h);
        hipLaunchKernelGGL(resize_v_kernel, grid, dim3(RS_THREADS), 0, st, both ? (const uint8_t*)tmp : s8,
                           both ? (long long)w * C : src_stride, both ? g.r0 : 0, both ? 0 : x0, both ? w : sw, C, tab_v,
                           tab_v + 2 * h, ksize, d8, dst_stride, w);
        LCM_CHECK_LAUNCH("resize_lanczos_u8 (vertical)");
    }
    return LCM_OK;
}
