// Variation seeds (include/lcm_hip.h, "variation seeds"; DESIGN.md sections 3 and 6): the subseed's noise blended into a request's
// initial latents on a per-column sphere, and the seed-resize paste of a source-shape blend into the target, in one launch for the
// whole batch.
//
// One wave per (slot, 64 (channel, column) pairs).  A thread owns one source column of one channel: it walks the column once for
// the three sums (y ascending, fma), decides its branch, and walks the pasted rows again for the blend.  Lanes are neighbouring
// columns, so every load and store of a wave is one contiguous row segment.  The per-slot descriptors travel by value in the
// kernel arguments; inactive slots and workgroups past a slot's columns return at once.  The launch moves at most 128 KiB per
// request at 512 x 512 and is bound by launch and load latency at every served size: nothing here is tuned for bandwidth.
#include "common.h"
#include <math.h>

#include "../../include/lcm_hip.h"      // lcm_variation_desc

namespace {
constexpr int NV_THREADS = 64;
constexpr int NV_ROWS = 8;               // rows of a column in flight per thread
constexpr float NV_DOT_LIMIT = 0.9995f;

struct VarSlot {
    const float* low;
    const float* high;
    int hs, ws;
    float t;
    int active;
};
struct VarArgs {
    VarSlot s[LCM_VARIATION_MAX_BATCH];
};

// floor((a - b) / 2) for any sign (Python's //)
__host__ __device__ inline int floor_half_diff(int a, int b) {
    const int d = a - b;
    return d >= 0 ? d / 2 : -((1 - d) / 2);
}

__global__ __launch_bounds__(NV_THREADS) void noise_variation_kernel(float* lat0, VarArgs args, int h, int w) {
    const int b = blockIdx.y;
    const VarSlot sl = args.s[b];
    if (!sl.active) return;
    const int hs = sl.hs, ws = sl.ws;
    // the window of the source that lands in the target, per axis
    const int dx = floor_half_diff(w, ws), dy = floor_half_diff(h, hs);
    const int cw = ws < w ? ws : w, ch = hs < h ? hs : h;
    const int sx0 = dx < 0 ? -dx : 0, tx0 = dx > 0 ? dx : 0;
    const int sy0 = dy < 0 ? -dy : 0, ty0 = dy > 0 ? dy : 0;
    const int i = blockIdx.x * NV_THREADS + threadIdx.x;         // (channel, column of the window)
    if (i >= 4 * cw) return;
    const int c = i / cw, xx = i - c * cw;
    // low may alias the slot (in place): no __restrict__ on these.  The thread owns the column, and every batch of rows below is
    // loaded before it is stored
    const long long col = ((long long)c * hs) * ws + sx0 + xx;
    const float* lo = sl.low + col;
    float* dst = lat0 + (((long long)b * 4 + c) * h + ty0) * w + tx0 + xx;
    const float t = sl.t;
    if (t == 0.f) {                                              // seed-resize alone: low is pasted, high is never read
        for (int y0 = 0; y0 < ch; y0 += NV_ROWS) {
            float l[NV_ROWS];
#pragma unroll
            for (int k = 0; k < NV_ROWS; ++k) l[k] = y0 + k < ch ? lo[(long long)(sy0 + y0 + k) * ws] : 0.f;
#pragma unroll
            for (int k = 0; k < NV_ROWS; ++k)
                if (y0 + k < ch) dst[(long long)(y0 + k) * w] = l[k];
        }
        return;
    }
    const float* hi = sl.high + col;
    float s_ll = 0.f, s_hh = 0.f, s_lh = 0.f;
#pragma unroll 8
    for (int y = 0; y < hs; ++y) {
        const float l = lo[(long long)y * ws], g = hi[(long long)y * ws];
        s_ll = __builtin_fmaf(l, l, s_ll);
        s_hh = __builtin_fmaf(g, g, s_hh);
        s_lh = __builtin_fmaf(l, g, s_lh);
    }
    float a = 1.0f - t, bb = t;
    const float d = s_lh / sqrtf(s_ll * s_hh);
    if (s_ll > 0.f && s_hh > 0.f && fabsf(d) <= NV_DOT_LIMIT) {  // false for a NaN: the linear weights stay
        const float om = acosf(d), so = sinf(om);
        a = sinf((1.0f - t) * om) / so;
        bb = sinf(t * om) / so;
    }
    for (int y0 = 0; y0 < ch; y0 += NV_ROWS) {
        float l[NV_ROWS], g[NV_ROWS];
#pragma unroll
        for (int k = 0; k < NV_ROWS; ++k) {
            const bool in = y0 + k < ch;
            l[k] = in ? lo[(long long)(sy0 + y0 + k) * ws] : 0.f;
            g[k] = in ? hi[(long long)(sy0 + y0 + k) * ws] : 0.f;
        }
#pragma unroll
        for (int k = 0; k < NV_ROWS; ++k)
            if (y0 + k < ch) dst[(long long)(y0 + k) * w] = __builtin_fmaf(a, l[k], bb * g[k]);
    }
}
}  // namespace

extern "C" int lcm_noise_variation_f32(void* lat0, int B, int h, int w, const lcm_variation_desc* descs, void* stream) {
    LCM_REQUIRE(lat0 && descs, "noise_variation: null pointer");
    LCM_REQUIRE(B >= 1 && B <= LCM_VARIATION_MAX_BATCH, "noise_variation: %d requests, one launch serves 1..%d", B, LCM_VARIATION_MAX_BATCH);
    LCM_REQUIRE(h >= 1 && h <= 256 && w >= 1 && w <= 256, "noise_variation: target shape %d x %d outside 1..256", h, w);
    LCM_REQUIRE(((uintptr_t)lat0 & 3) == 0, "noise_variation: misaligned latents");
    const uintptr_t all0 = (uintptr_t)lat0, slot_bytes = (uintptr_t)16 * h * w, all1 = all0 + (uintptr_t)B * slot_bytes;
    VarArgs args = {};
    int groups = 0;
    for (int b = 0; b < B; ++b) {
        const lcm_variation_desc& d = descs[b];
        if (!d.active) continue;
        LCM_REQUIRE(d.hs >= 1 && d.hs <= 256 && d.ws >= 1 && d.ws <= 256, "noise_variation: request %d: source shape %d x %d outside 1..256", b,
                    d.hs, d.ws);
        LCM_REQUIRE(d.t >= 0.f && d.t <= 1.f, "noise_variation: request %d: strength %g outside [0, 1]", b, (double)d.t);
        LCM_REQUIRE(d.low && (d.high || d.t == 0.f), "noise_variation: request %d: null pointer", b);
        LCM_REQUIRE((((uintptr_t)d.low | (uintptr_t)d.high) & 3) == 0, "noise_variation: request %d: misaligned pointer", b);
        const uintptr_t slot = all0 + (uintptr_t)b * slot_bytes, src_bytes = (uintptr_t)16 * d.hs * d.ws;
        const uintptr_t lo = (uintptr_t)d.low, hi = (uintptr_t)d.high;
        if (lo == slot)
            LCM_REQUIRE(d.hs == h && d.ws == w, "noise_variation: request %d: a blend in place needs the target's shape, got %d x %d for %d x %d",
                        b, d.hs, d.ws, h, w);
        else
            LCM_REQUIRE(lo + src_bytes <= all0 || lo >= all1, "noise_variation: request %d: low overlaps the latents without being its slot", b);
        LCM_REQUIRE(d.t == 0.f || hi + src_bytes <= all0 || hi >= all1, "noise_variation: request %d: high overlaps the latents", b);
        args.s[b] = {(const float*)d.low, (const float*)d.high, d.hs, d.ws, d.t, 1};
        const int cw = d.ws < w ? d.ws : w, g = (4 * cw + NV_THREADS - 1) / NV_THREADS;
        groups = g > groups ? g : groups;
    }
    if (groups == 0) return LCM_OK;
    hipStream_t s = (hipStream_t)stream;
    lcm_prof_start("noise_variation_kernel", s);
    hipLaunchKernelGGL(noise_variation_kernel, dim3(groups, B), dim3(NV_THREADS), 0, s, (float*)lat0, args, h, w);
    lcm_prof_stop(s);
    LCM_CHECK_LAUNCH("noise_variation");
    return LCM_OK;
}
