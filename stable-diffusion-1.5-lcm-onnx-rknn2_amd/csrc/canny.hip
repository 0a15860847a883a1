// ControlNet preprocessors on the device (include/lcm_hip.h "Canny"): the Canny edge detector as integer
// arithmetic -- Sobel gradients, channel pick, non-maximum suppression and the double threshold in one LDS-haloed stencil
// launch (picture -> class map 0 / 1 / 2), then hysteresis as connected-component labelling by label equivalence in four
// launches (class map -> edge picture) -- and the byte inversion.  Every result is defined bit for bit by the header and
// tests/test_canny_gpu.py compares for equality with tests/canny_reference.py.
//
// Linking.  labels[] is a forest over the linear pixel index g = (b H + y) W + x with the invariant  labels[i] <= i  at every
// moment of every launch: a pixel starts as its own root, a parent is only ever replaced by a smaller value (integer min), and
// the flatten pass replaces it by the root, the smallest index of the component.  So every chain of parents strictly descends
// and ends at a pixel that is its own parent after at most i steps, whatever other threads do meanwhile: no loop below waits
// for another thread or workgroup, none can spin.  Workgroups never hand data to each other inside a launch other than through
// those monotone integer atomics; what one launch wrote is read by the next (the kernel boundary is the only fence relied on).
// min and or are commutative and idempotent, so the forest's roots, the marks and the picture do not depend on arrival order.
#include "common.h"

#define CANNY_TG22 13573            // tan(22.5 deg) * 2^15

// classes stage: a workgroup owns CT_W x CT_H pixels, one per thread
#define CT_W 32
#define CT_H 8
// link stage: a workgroup labels an LT x LT tile in LDS, one pixel per thread
#define LT 32

namespace {

__device__ __forceinline__ int clampc(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }

// Picture -> class map.  The tile plus a 2-pixel halo of pixels (border replicated) is staged in LDS; gradients and magnitudes
// are computed for the tile plus a 1-pixel halo (0 outside the picture), so that the suppression of a pixel reads its
// neighbours' magnitudes from LDS instead of a second pass through memory.
__global__ void __launch_bounds__(CT_W * CT_H)
canny_classes_kernel(const uint8_t* __restrict__ in, uint8_t* __restrict__ cls, int H, int W, int lo, int hi) {
    constexpr int PW = CT_W + 4, PH = CT_H + 4, MW = CT_W + 2, MH = CT_H + 2;
    __shared__ uint8_t pix[3][PH][PW];
    __shared__ short gdx[MH][MW], gdy[MH][MW], gm[MH][MW];
    const int tid = threadIdx.y * CT_W + threadIdx.x;
    const int b = blockIdx.z, y0 = blockIdx.y * CT_H, x0 = blockIdx.x * CT_W;
    const uint8_t* img = in + (size_t)b * H * W * 3;
    for (int n = tid; n < PH * PW; n += CT_W * CT_H) {
        const int ry = n / PW, rx = n - ry * PW;
        const int y = clampc(y0 - 2 + ry, 0, H - 1), x = clampc(x0 - 2 + rx, 0, W - 1);
        const uint8_t* p = img + ((size_t)y * W + x) * 3;
        pix[0][ry][rx] = p[0], pix[1][ry][rx] = p[1], pix[2][ry][rx] = p[2];
    }
    __syncthreads();
    for (int n = tid; n < MH * MW; n += CT_W * CT_H) {
        const int my = n / MW, mx = n - my * MW;
        const int y = y0 - 1 + my, x = x0 - 1 + mx;
        int bdx = 0, bdy = 0, bm = 0;
        if (y >= 0 && y < H && x >= 0 && x < W) {
            bm = -1;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const uint8_t(*q)[PW] = pix[c];              // q[my + 1][mx + 1] is the pixel itself
                const int a00 = q[my][mx], a01 = q[my][mx + 1], a02 = q[my][mx + 2];
                const int a10 = q[my + 1][mx], a12 = q[my + 1][mx + 2];
                const int a20 = q[my + 2][mx], a21 = q[my + 2][mx + 1], a22 = q[my + 2][mx + 2];
                const int dx = (a02 - a00) + 2 * (a12 - a10) + (a22 - a20);
                const int dy = (a20 - a00) + 2 * (a21 - a01) + (a22 - a02);
                const int m = abs(dx) + abs(dy);
                if (m > bm) bdx = dx, bdy = dy, bm = m;     // strictly larger: the lowest channel wins a tie
            }
        }
        gdx[my][mx] = (short)bdx, gdy[my][mx] = (short)bdy, gm[my][mx] = (short)bm;
    }
    __syncthreads();
    const int y = y0 + threadIdx.y, x = x0 + threadIdx.x;
    if (y >= H || x >= W) return;
    const int my = threadIdx.y + 1, mx = threadIdx.x + 1;
    const int dx = gdx[my][mx], dy = gdy[my][mx], m = gm[my][mx];
    const int ax = abs(dx), ay = abs(dy) << 15;
    const int t22 = ax * CANNY_TG22, t67 = t22 + (ax << 16);
    bool peak;
    if (ay < t22) peak = m > gm[my][mx - 1] && m >= gm[my][mx + 1];
    else if (ay > t67) peak = m > gm[my - 1][mx] && m >= gm[my + 1][mx];
    else {
        const int s = ((dx ^ dy) < 0) ? -1 : 1;
        peak = m > gm[my - 1][mx - s] && m > gm[my + 1][mx + s];
    }
    cls[((size_t)b * H + y) * W + x] = (peak && m > lo) ? (m > hi ? 2 : 1) : 0;
}

// ---- linking ---------------------------------------------------------------------------------------------------------
// Root of i in an LDS forest.  Terminates: L[x] <= x always, so x strictly descends until L[x] == x (at most x steps).
__device__ __forceinline__ int lds_find(const int* L, int i) {
    int x = i, p;
    while ((p = __hip_atomic_load(&L[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) != x) x = p;
    return x;
}
// Union in an LDS forest.  Terminates: each round either finishes or replaces the larger root by the value the min found
// there, which is smaller than that root (a parent never exceeds its child); the pair (a, b) strictly descends in a + b >= 0.
__device__ __forceinline__ void lds_union(int* L, int a, int b) {
    for (;;) {
        a = lds_find(L, a), b = lds_find(L, b);
        if (a == b) return;
        if (a > b) { const int t = a; a = b, b = t; }        // a < b: hang b under a
        const int old = atomicMin(&L[b], a);
        if (old == b) return;                                // b was a root and now points to a
        b = old;                                             // b had a parent already (old < b): unite that with a
    }
}

// The same two on the global forest, used by the seam pass, where workgroups update concurrently: every access is an
// agent-scope atomic, so no value is served from a cache that another workgroup's update has not reached.
__device__ __forceinline__ int g_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
// Terminates: labels[x] <= x, so x strictly descends.
__device__ __forceinline__ int g_find(const int* L, int i) {
    int x = i, p;
    while ((p = g_load(&L[x])) != x) x = p;
    return x;
}
// Terminates as lds_union does: the larger root is replaced by a strictly smaller value in every round that does not finish.
__device__ __forceinline__ void g_union(int* L, int a, int b) {
    for (;;) {
        a = g_find(L, a), b = g_find(L, b);
        if (a == b) return;
        if (a > b) { const int t = a; a = b, b = t; }
        const int old = __hip_atomic_fetch_min(&L[b], a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (old == b) return;
        b = old;
    }
}

// Pass 1: label each LT x LT tile by itself in LDS (row-major local index, so the smallest local index of a component is its
// smallest linear pixel index too), write labels[g] = linear index of the local root (g itself where the class is 0), and
// marks[g] = 1 where g is a local root whose local component holds a class-2 pixel, else 0.
__global__ void __launch_bounds__(LT * LT)
canny_label_tile_kernel(const uint8_t* __restrict__ cls, int* __restrict__ labels, int* __restrict__ marks, int H, int W) {
    __shared__ int L[LT * LT];
    __shared__ int strong[LT * LT];
    __shared__ uint8_t c[LT + 2][LT + 2];                    // the tile's classes with a ring (0 outside the tile: tile-local)
    const int lx = threadIdx.x, ly = threadIdx.y, i = ly * LT + lx;
    const int b = blockIdx.z, y = blockIdx.y * LT + ly, x = blockIdx.x * LT + lx;
    const bool inside = y < H && x < W;
    const int g = inside ? (b * H + y) * W + x : 0;
    const int me = inside ? cls[g] : 0;
    for (int n = i; n < (LT + 2) * (LT + 2); n += LT * LT) (&c[0][0])[n] = 0;
    L[i] = i, strong[i] = 0;
    __syncthreads();
    c[ly + 1][lx + 1] = (uint8_t)me;
    __syncthreads();
    if (me) {                                                // the four neighbours before me in row-major order
        if (c[ly + 1][lx]) lds_union(L, i, i - 1);
        if (c[ly][lx]) lds_union(L, i, i - LT - 1);
        if (c[ly][lx + 1]) lds_union(L, i, i - LT);
        if (c[ly][lx + 2]) lds_union(L, i, i - LT + 1);
    }
    __syncthreads();
    const int r = lds_find(L, i);
    if (me == 2) atomicOr(&strong[r], 1);
    __syncthreads();
    if (!inside) return;
    labels[g] = g + (r / LT - ly) * W + (r % LT - lx);
    marks[g] = strong[i];
}

// Pass 2: unite across tile borders.  A pixel on the border of its tile unites with those of its four neighbours before it
// in row-major order (W, NW, N, NE) that lie in another tile; every 8-adjacent pair that crosses a border is met once, from
// its later pixel.  Components never cross pictures: neighbours are taken inside the picture only.
__global__ void __launch_bounds__(256)
canny_seam_kernel(const uint8_t* __restrict__ cls, int* __restrict__ labels, int B, int H, int W) {
    // one thread per pixel of a tile's first row, first column and last column: 3 LT slots per tile
    const int tiles_x = (W + LT - 1) / LT, tiles_y = (H + LT - 1) / LT;
    const long long n = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long total = (long long)B * tiles_y * tiles_x * (3 * LT);
    if (n >= total) return;
    const int slot = (int)(n % (3 * LT));
    long long t = n / (3 * LT);
    const int tx = (int)(t % tiles_x);
    t /= tiles_x;
    const int ty = (int)(t % tiles_y), b = (int)(t / tiles_y);
    const int side = slot / LT, k = slot - side * LT;
    // side 0: first row, column k; side 1: first column, row k (k > 0); side 2: last column, row k (k > 0; its NE neighbour)
    if (side != 0 && k == 0) return;
    const int y = ty * LT + (side == 0 ? 0 : k), x = tx * LT + (side == 0 ? k : side == 1 ? 0 : LT - 1);
    if (y >= H || x >= W) return;
    const int g = (b * H + y) * W + x;
    if (!cls[g]) return;
    const bool first_row = side == 0, first_col = (x % LT) == 0, last_col = (x % LT) == LT - 1;
    // W: another tile iff first column
    if (first_col && x > 0 && cls[g - 1]) g_union(labels, g, g - 1);
    if (y > 0) {
        // NW: another tile iff first row or first column
        if ((first_row || first_col) && x > 0 && cls[g - W - 1]) g_union(labels, g, g - W - 1);
        // N: another tile iff first row
        if (first_row && cls[g - W]) g_union(labels, g, g - W);
        // NE: another tile iff first row or last column
        if ((first_row || last_col) && x + 1 < W && cls[g - W + 1]) g_union(labels, g, g - W + 1);
    }
}

// Pass 3: flatten (labels[g] = root of g) and carry the marks of the tile-local roots to the roots.  Roots are fixed in this
// launch (nobody writes a root's label), and every value labels[i] holds during it is either its parent from pass 2 or its
// root, both ancestors of i: the walk below ends at the root whichever it reads.  Terminates: labels[x] <= x, strictly descending.
__global__ void __launch_bounds__(256)
canny_flatten_kernel(const uint8_t* __restrict__ cls, int* __restrict__ labels, int* __restrict__ marks, int n) {
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= n || !cls[g]) return;
    int x = g, p;
    while ((p = g_load(&labels[x])) != x) x = p;
    if (x != g) {
        labels[g] = x;
        if (marks[g]) atomicOr(&marks[x], 1);               // g was a tile-local root with a strong pixel under it
    }
}

// Pass 4: the picture.  255 where the pixel has a class and its root is marked.  A thread owns four pixels = three dwords.
__global__ void __launch_bounds__(256)
canny_paint_kernel(const uint8_t* __restrict__ cls, const int* __restrict__ labels, const int* __restrict__ marks,
                   uint8_t* __restrict__ out, int n, int aligned) {
    const int g0 = (blockIdx.x * 256 + threadIdx.x) * 4;
    if (g0 >= n) return;
    uint32_t v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int g = g0 + j;
        v[j] = (g < n && cls[g] && marks[labels[g]]) ? 255u : 0u;
    }
    if (aligned && g0 + 3 < n) {
        uint32_t* o = reinterpret_cast<uint32_t*>(out + (size_t)g0 * 3);
        o[0] = v[0] * 0x010101u | v[1] << 24;
        o[1] = v[1] * 0x0101u | v[2] * 0x01010000u;
        o[2] = v[2] | v[3] * 0x01010100u;
        return;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (g0 + j < n) {
            uint8_t* o = out + (size_t)(g0 + j) * 3;
            o[0] = o[1] = o[2] = (uint8_t)v[j];
        }
}

__global__ void __launch_bounds__(256)
invert_u8_kernel(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, long long n, int aligned) {
    const long long i0 = ((long long)blockIdx.x * 256 + threadIdx.x) * 16;
    if (i0 >= n) return;
    if (aligned && i0 + 15 < n) {
        uint4 v = *reinterpret_cast<const uint4*>(in + i0);
        v.x = ~v.x, v.y = ~v.y, v.z = ~v.z, v.w = ~v.w;
        *reinterpret_cast<uint4*>(out + i0) = v;
        return;
    }
    for (long long i = i0; i < n && i < i0 + 16; ++i) out[i] = (uint8_t)(255 - in[i]);
}

inline long long pad16(long long v) { return (v + 15) & ~15ll; }

int check_shape(const char* who, int B, int H, int W) {
    LCM_REQUIRE(B >= 1 && H >= 1 && W >= 1, "%s: bad shape B=%d H=%d W=%d", who, B, H, W);
    LCM_REQUIRE((long long)B * H * W < (1ll << 29), "%s: %d x %d x %d pixels are more than 2^29", who, B, H, W);
    LCM_REQUIRE(B < 65536 && (H + CT_H - 1) / CT_H < 65536, "%s: B=%d or H=%d too large for one grid", who, B, H);
    return LCM_OK;
}
}  // namespace

extern "C" long long lcm_canny_ws_bytes(int B, int H, int W) {
    if (B < 1 || H < 1 || W < 1) return 0;
    const long long n = (long long)B * H * W;
    return pad16(n) + 2 * pad16(4 * n);                      // class map | labels | marks
}

extern "C" int lcm_canny_classes_u8(const void* in_rgb, void* cls_out, int B, int H, int W, int lo, int hi, void* stream) {
    LCM_REQUIRE(in_rgb && cls_out, "canny_classes_u8: null pointer");
    if (int rc = check_shape("canny_classes_u8", B, H, W)) return rc;
    LCM_REQUIRE(in_rgb != cls_out, "canny_classes_u8: the class map aliases the picture");
    if (lo > hi) { const int t = lo; lo = hi, hi = t; }
    hipLaunchKernelGGL(canny_classes_kernel, dim3((W + CT_W - 1) / CT_W, (H + CT_H - 1) / CT_H, B), dim3(CT_W, CT_H), 0,
                       (hipStream_t)stream, (const uint8_t*)in_rgb, (uint8_t*)cls_out, H, W, lo, hi);
    LCM_CHECK_LAUNCH("canny_classes_u8");
    return LCM_OK;
}

extern "C" int lcm_canny_link(const void* cls, void* out_rgb, void* ws, long long ws_bytes, int B, int H, int W, void* stream) {
    LCM_REQUIRE(cls && out_rgb && ws, "canny_link: null pointer");
    if (int rc = check_shape("canny_link", B, H, W)) return rc;
    LCM_REQUIRE(ws_bytes >= lcm_canny_ws_bytes(B, H, W), "canny_link: workspace of %lld bytes, %lld needed", ws_bytes,
                lcm_canny_ws_bytes(B, H, W));
    LCM_REQUIRE((uintptr_t)ws % 16 == 0, "canny_link: the workspace must be 16-byte aligned");
    const long long n = (long long)B * H * W;
    const uint8_t* c = (const uint8_t*)cls;
    LCM_REQUIRE((const uint8_t*)out_rgb + 3 * n <= c || (const uint8_t*)out_rgb >= c + n, "canny_link: the picture overlaps the class map");
    int* labels = (int*)((uint8_t*)ws + pad16(n));
    int* marks = (int*)((uint8_t*)ws + pad16(n) + pad16(4 * n));
    LCM_REQUIRE((const uint8_t*)out_rgb + 3 * n <= (const uint8_t*)labels || (const uint8_t*)out_rgb >= (const uint8_t*)ws + ws_bytes,
                "canny_link: the picture overlaps the workspace's labels");
    hipStream_t s = (hipStream_t)stream;
    const int tiles_x = (W + LT - 1) / LT, tiles_y = (H + LT - 1) / LT;
    LCM_REQUIRE(tiles_y < 65536, "canny_link: H=%d too large for one grid", H);
    hipLaunchKernelGGL(canny_label_tile_kernel, dim3(tiles_x, tiles_y, B), dim3(LT, LT), 0, s, c, labels, marks, H, W);
    LCM_CHECK_LAUNCH("canny_link (tiles)");
    const long long seam = (long long)B * tiles_y * tiles_x * (3 * LT);
    hipLaunchKernelGGL(canny_seam_kernel, dim3((unsigned)((seam + 255) / 256)), dim3(256), 0, s, c, labels, B, H, W);
    LCM_CHECK_LAUNCH("canny_link (seams)");
    hipLaunchKernelGGL(canny_flatten_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, c, labels, marks, (int)n);
    LCM_CHECK_LAUNCH("canny_link (flatten)");
    hipLaunchKernelGGL(canny_paint_kernel, dim3((unsigned)((n + 1023) / 1024)), dim3(256), 0, s, c, (const int*)labels,
                       (const int*)marks, (uint8_t*)out_rgb, (int)n, (int)((uintptr_t)out_rgb % 4 == 0));
    LCM_CHECK_LAUNCH("canny_link (paint)");
    return LCM_OK;
}

extern "C" int lcm_canny_rgb8(const void* in_rgb, void* out_rgb, void* ws, long long ws_bytes, int B, int H, int W, float low,
                              float high, void* stream) {
    LCM_REQUIRE(in_rgb && out_rgb && ws, "canny_rgb8: null pointer");
    if (int rc = check_shape("canny_rgb8", B, H, W)) return rc;
    LCM_REQUIRE(low == low && high == high && fabsf(low) < 1e9f && fabsf(high) < 1e9f, "canny_rgb8: thresholds %g, %g are not finite numbers below 1e9",
                (double)low, (double)high);
    LCM_REQUIRE(ws_bytes >= lcm_canny_ws_bytes(B, H, W), "canny_rgb8: workspace of %lld bytes, %lld needed", ws_bytes,
                lcm_canny_ws_bytes(B, H, W));
    LCM_REQUIRE((uintptr_t)ws % 16 == 0, "canny_rgb8: the workspace must be 16-byte aligned");
    const long long n = (long long)B * H * W;
    const uint8_t *i8 = (const uint8_t*)in_rgb, *o8 = (const uint8_t*)out_rgb, *w8 = (const uint8_t*)ws;
    LCM_REQUIRE(i8 + 3 * n <= w8 || i8 >= w8 + ws_bytes, "canny_rgb8: the picture overlaps the workspace");
    LCM_REQUIRE(o8 + 3 * n <= w8 || o8 >= w8 + ws_bytes, "canny_rgb8: the output overlaps the workspace");
    // in place (out_rgb == in_rgb) is fine: the picture is read by the first launch only, the output written by the last
    int rc = lcm_canny_classes_u8(in_rgb, ws, B, H, W, (int)floorf(low), (int)floorf(high), stream);
    if (rc) return rc;
    return lcm_canny_link(ws, out_rgb, ws, ws_bytes, B, H, W, stream);
}

extern "C" int lcm_invert_u8(const void* in, void* out, long long n, void* stream) {
    LCM_REQUIRE(in && out, "invert_u8: null pointer");
    LCM_REQUIRE(n >= 1 && n < (1ll << 40), "invert_u8: bad length %lld", n);
    const long long groups = (n + 15) / 16, blocks = (groups + 255) / 256;
    LCM_REQUIRE(blocks < (1ll << 31), "invert_u8: bad length %lld", n);
    hipLaunchKernelGGL(invert_u8_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (const uint8_t*)in, (uint8_t*)out, n,
                       (int)((((uintptr_t)in | (uintptr_t)out) % 16) == 0));
    LCM_CHECK_LAUNCH("invert_u8");
    return LCM_OK;
}
