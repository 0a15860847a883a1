// SD upscale's way back (include/lcm_hip.h, "tile grid combine"; DESIGN.md sections 3 and 6): the overlapping tiles of one request,
// blended into the W x H picture as A1111's combine_grid pastes them -- in one launch, as a pure gather.
//
// blockIdx.y is the output row, so which tile rows lie under it (the last hard cover and the blended rows after it) is wave-uniform
// and found once from the by-value ys.  A thread owns GP neighbouring pixels of that row: per pixel it finds its last hard column
// cover and the blended columns after it from xs, folds the row pictures forward from there and writes its 12 bytes with three
// dword stores (byte stores where the row's start is not dword-aligned or the group is cut by the row's end).  Lanes are
// neighbouring groups, so the byte loads of a wave walk one contiguous segment of a tile row.  No LDS, no workgroup waits for
// another, no atomics.  The launch moves W x H x 3 bytes out and little more in; nothing here is tuned for bandwidth (what it takes
// at 1024 x 1024 and 2048 x 2048: DESIGN.md section 7, tools/sdupscale_bench.py).
#include "common.h"

#include "../../include/lcm_hip.h"      // lcm_grid_desc

namespace {
constexpr int GC_THREADS = 256;
constexpr int GP = 4;                    // pixels per thread: 12 bytes, three dwords

__device__ __forceinline__ int div255(int a) {
    a += 128;
    return (a + (a >> 8)) >> 8;
}
__device__ __forceinline__ int blend8(int p, int t, int m) { return div255(p * (255 - m) + t * m); }

__global__ __launch_bounds__(GC_THREADS) void grid_combine_kernel(const uint8_t* __restrict__ tiles, uint8_t* __restrict__ out,
                                                                  const lcm_grid_desc d) {
    const int y = blockIdx.y;
    const int xg = (blockIdx.x * GC_THREADS + threadIdx.x) * GP;
    const int W = d.W, tw = d.tile_w, th = d.tile_h, ov = d.overlap, cols = d.cols, rows = d.rows;
    if (xg >= W) return;
    // rows under y (uniform): the last hard cover r_hard, then rows r_hard + 1 .. r_end - 1 blend in (their j is below ov: a later
    // row with j >= ov would have been the hard one)
    int r_hard = 0, r_end = 1;
    for (int r = 1; r < rows; ++r) {
        const int j = y - d.ys[r];
        if (j >= ov && j < th) r_hard = r;
        if (j >= 0) r_end = r + 1;
    }
    // the same per pixel along x
    int c_hard[GP], c_end[GP];
#pragma unroll
    for (int p = 0; p < GP; ++p) c_hard[p] = 0, c_end[p] = 1;
    for (int c = 1; c < cols; ++c) {
        const int xc = d.xs[c];
#pragma unroll
        for (int p = 0; p < GP; ++p) {
            const int i = xg + p - xc;
            if (i >= ov && i < tw) c_hard[p] = c;
            if (i >= 0) c_end[p] = c + 1;
        }
    }
    uint8_t px[GP * 3];
#pragma unroll
    for (int p = 0; p < GP; ++p) {
        const int x = xg + p;
        int v0 = 0, v1 = 0, v2 = 0;
        if (x < W) {
            for (int r = r_hard; r < r_end; ++r) {
                const int j = y - d.ys[r];                     // 0 <= j < th
                // the row picture R_r(x, j): the hard column, then the blended ones
                const uint8_t* row = tiles + ((size_t)(r * cols) * th + j) * tw * 3;
                const uint8_t* t = row + ((size_t)c_hard[p] * th * tw + (x - d.xs[c_hard[p]])) * 3;
                int q0 = t[0], q1 = t[1], q2 = t[2];
                for (int c = c_hard[p] + 1; c < c_end[p]; ++c) {
                    const int i = x - d.xs[c];                 // 0 <= i < ov
                    const int m = (255 * i) / ov;
                    const uint8_t* u = row + ((size_t)c * th * tw + i) * 3;
                    q0 = blend8(q0, u[0], m), q1 = blend8(q1, u[1], m), q2 = blend8(q2, u[2], m);
                }
                if (r == r_hard) {
                    v0 = q0, v1 = q1, v2 = q2;
                } else {
                    const int m = (255 * j) / ov;
                    v0 = blend8(v0, q0, m), v1 = blend8(v1, q1, m), v2 = blend8(v2, q2, m);
                }
            }
        }
        px[p * 3 + 0] = (uint8_t)v0, px[p * 3 + 1] = (uint8_t)v1, px[p * 3 + 2] = (uint8_t)v2;
    }
    uint8_t* dst = out + ((size_t)y * W + xg) * 3;
    if (xg + GP <= W && ((uintptr_t)dst & 3) == 0) {
        uint32_t* d32 = (uint32_t*)dst;
#pragma unroll
        for (int k = 0; k < 3; ++k)
            d32[k] = (uint32_t)px[4 * k] | ((uint32_t)px[4 * k + 1] << 8) | ((uint32_t)px[4 * k + 2] << 16) | ((uint32_t)px[4 * k + 3] << 24);
    } else {
#pragma unroll
        for (int p = 0; p < GP; ++p)
            if (xg + p < W) {
                dst[p * 3 + 0] = px[p * 3 + 0];
                dst[p * 3 + 1] = px[p * 3 + 1];
                dst[p * 3 + 2] = px[p * 3 + 2];
            }
    }
}

// the four facts of an axis' tile offsets (backends/sdupscale.py, geometry): they make every pixel hard-covered and every read
// inside its tile
bool axis_ok(const int* v, int n, int tile, int overlap, int size) {
    if (v[0] != 0 || v[n - 1] + tile != size) return false;
    for (int k = 1; k < n; ++k)
        if (v[k] <= v[k - 1] || v[k] - v[k - 1] > tile - overlap) return false;
    return true;
}
}  // namespace

extern "C" int lcm_grid_combine_rgb8(const void* tiles_u8, void* out_u8, const lcm_grid_desc* desc, void* stream) {
    LCM_REQUIRE(tiles_u8 && out_u8 && desc, "grid_combine: null pointer");
    const lcm_grid_desc d = *desc;
    LCM_REQUIRE(d.cols >= 1 && d.cols <= LCM_GRID_MAX_AXIS && d.rows >= 1 && d.rows <= LCM_GRID_MAX_AXIS,
                "grid_combine: %d x %d tiles, an axis holds 1..%d", d.cols, d.rows, LCM_GRID_MAX_AXIS);
    LCM_REQUIRE(d.tile_w >= 1 && d.tile_w <= 4096 && d.tile_h >= 1 && d.tile_h <= 4096, "grid_combine: tile %d x %d outside 1..4096",
                d.tile_w, d.tile_h);
    LCM_REQUIRE(d.W >= d.tile_w && d.W <= 4096 && d.H >= d.tile_h && d.H <= 4096,
                "grid_combine: picture %d x %d outside tile (%d x %d) .. 4096", d.W, d.H, d.tile_w, d.tile_h);
    LCM_REQUIRE(d.overlap >= 0 && d.overlap < (d.tile_w < d.tile_h ? d.tile_w : d.tile_h), "grid_combine: overlap %d outside 0 .. min(tile) - 1",
                d.overlap);
    LCM_REQUIRE(axis_ok(d.xs, d.cols, d.tile_w, d.overlap, d.W), "grid_combine: xs must start at 0, rise strictly by at most tile_w - overlap "
                "and end at W - tile_w");
    LCM_REQUIRE(axis_ok(d.ys, d.rows, d.tile_h, d.overlap, d.H), "grid_combine: ys must start at 0, rise strictly by at most tile_h - overlap "
                "and end at H - tile_h");
    LCM_REQUIRE((long long)d.rows * d.cols * d.tile_h * d.tile_w * 3 < (1ll << 31), "grid_combine: %d tiles of %d x %d pass 2^31 bytes",
                d.rows * d.cols, d.tile_w, d.tile_h);
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((d.W + GC_THREADS * GP - 1) / (GC_THREADS * GP), d.H);
    lcm_prof_start("grid_combine_kernel", s);
    hipLaunchKernelGGL(grid_combine_kernel, grid, dim3(GC_THREADS), 0, s, (const uint8_t*)tiles_u8, (uint8_t*)out_u8, d);
    lcm_prof_stop(s);
    LCM_CHECK_LAUNCH("grid_combine");
    return LCM_OK;
}
