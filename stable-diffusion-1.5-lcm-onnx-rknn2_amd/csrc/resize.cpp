// Host side of the Lanczos resampler (include/lcm_hip.h "Lanczos resampler"): the coefficient tables of an
// axis in double precision with libm's sin, as PIL's ImagingResample builds them for 8-bit pixels, turned into 22-bit fixed
// point.  Compiled without fast-math and without the device tool chain's contraction: every operation below is one IEEE double
// operation in the order written, which is what makes the tables -- and so the device passes (csrc/resize.hip) -- equal to
// PIL's bit for bit.  tests/test_resize_cpu.py compares them with tests/resize_reference.py for equality.
#include <math.h>
#include <stdint.h>

#include <vector>

#define LCM_OK 0
#define LCM_EINVAL (-1)
void lcm_set_error(const char* fmt, ...);

namespace {

constexpr double kLanczosSupport = 3.0;
constexpr int kPrecisionBits = 22;

inline double sinc(double x) {
    if (x == 0.0) return 1.0;
    x = x * M_PI;
    return sin(x) / x;
}
inline double lanczos(double x) { return (-3.0 <= x && x < 3.0) ? sinc(x) * sinc(x / 3) : 0.0; }

struct Axis {
    double scale, fs, support;
    int ksize;
};
inline Axis axis_of(int in, int out) {
    Axis a;
    a.scale = (double)in / out;
    a.fs = a.scale < 1.0 ? 1.0 : a.scale;
    a.support = kLanczosSupport * a.fs;
    a.ksize = (int)ceil(a.support) * 2 + 1;
    return a;
}
inline void bounds_of(const Axis& a, int in, int xx, int* xmin, int* xmax) {
    const double center = (xx + 0.5) * a.scale;
    int lo = (int)(center - a.support + 0.5), hi = (int)(center + a.support + 0.5);
    *xmin = lo < 0 ? 0 : lo;
    *xmax = hi > in ? in : hi;
}
inline bool axis_ok(int in, int out) { return in >= 1 && in <= 8192 && out >= 1 && out <= 4096; }
inline int clampi(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }

}  // namespace

extern "C" int lcm_resize_ksize(int in, int out) { return axis_ok(in, out) ? axis_of(in, out).ksize : 0; }

extern "C" long long lcm_resize_table_bytes(int in, int out, int n) {
    if (!axis_ok(in, out) || n < 1 || n > 4096) return 0;
    const long long b = 4ll * n * (2 + axis_of(in, out).ksize);
    return (b + 15) & ~15ll;
}

// The source range [*first, *last) that the outputs o0 .. o0 + n - 1 (each clamped to [0, out)) read.  Bounds do not decrease
// with the output index, so the first and the last output give it.
extern "C" int lcm_resize_span(int in, int out, int o0, int n, int* first, int* last) {
    if (!axis_ok(in, out) || n < 1 || n > 4096 || !first || !last) {
        lcm_set_error("resize_span: bad axis in=%d out=%d window %d+%d", in, out, o0, n);
        return LCM_EINVAL;
    }
    const Axis a = axis_of(in, out);
    int lo, hi, t;
    bounds_of(a, in, clampi(o0, 0, out - 1), &lo, &t);
    bounds_of(a, in, clampi(o0 + n - 1, 0, out - 1), &t, &hi);
    *first = lo, *last = hi;
    return LCM_OK;
}

extern "C" int lcm_resize_tables(int in, int out, int o0, int n, void* dst, long long dst_bytes) {
    if (!axis_ok(in, out) || n < 1 || n > 4096 || !dst) {
        lcm_set_error("resize_tables: bad axis in=%d out=%d window %d+%d (source 1..8192, output 1..4096)", in, out, o0, n);
        return LCM_EINVAL;
    }
    if (dst_bytes < lcm_resize_table_bytes(in, out, n)) {
        lcm_set_error("resize_tables: table of %lld bytes, %lld needed", dst_bytes, lcm_resize_table_bytes(in, out, n));
        return LCM_EINVAL;
    }
    const Axis a = axis_of(in, out);
    const double ss = 1.0 / a.fs;
    int32_t* bounds = (int32_t*)dst;
    int32_t* kk = bounds + 2 * n;
    std::vector<double> w(a.ksize);
    for (int i = 0; i < n; ++i) {
        const int xx = clampi(o0 + i, 0, out - 1);
        const double center = (xx + 0.5) * a.scale;
        int xmin, xmax;
        bounds_of(a, in, xx, &xmin, &xmax);
        const int cnt = xmax - xmin;
        double ww = 0.0;
        for (int x = 0; x < cnt; ++x) {
            w[x] = lanczos((x + xmin - center + 0.5) * ss);
            ww += w[x];
        }
        int32_t* k = kk + (long long)i * a.ksize;
        for (int x = 0; x < cnt; ++x) {
            const double v = ww != 0.0 ? w[x] / ww : w[x];
            k[x] = v < 0 ? (int)(-0.5 + v * (1 << kPrecisionBits)) : (int)(0.5 + v * (1 << kPrecisionBits));
        }
        for (int x = cnt; x < a.ksize; ++x) k[x] = 0;
        bounds[2 * i] = xmin, bounds[2 * i + 1] = cnt;
    }
    return LCM_OK;
}

// The largest number of source pixels that `tile` neighbouring outputs of the window read together (what the horizontal pass
// stages per row).
extern "C" int lcm_resize_max_span(int in, int out, int o0, int n, int tile) {
    if (!axis_ok(in, out) || n < 1 || n > 4096 || tile < 1) return 0;
    const Axis a = axis_of(in, out);
    int best = 0;
    for (int i0 = 0; i0 < n; i0 += tile) {
        const int i1 = (i0 + tile < n ? i0 + tile : n) - 1;
        int lo, hi, t;
        bounds_of(a, in, clampi(o0 + i0, 0, out - 1), &lo, &t);
        bounds_of(a, in, clampi(o0 + i1, 0, out - 1), &t, &hi);
        if (hi - lo > best) best = hi - lo;
    }
    return best;
}

// Which passes a call runs: bit 0 the horizontal, bit 1 the vertical one.  A pass whose axis keeps its size does not run (its
// table would be the identity); when both keep it the horizontal pass copies the window.
extern "C" int lcm_resize_passes(int sw, int sh, int out_w, int out_h) {
    const int v = out_h != sh ? 2 : 0;
    return v | ((out_w != sw || !v) ? 1 : 0);
}

extern "C" long long lcm_resize_plan_table_bytes(int sw, int sh, int out_w, int out_h, int w, int h) {
    if (!axis_ok(sw, out_w) || !axis_ok(sh, out_h) || w < 1 || w > 4096 || h < 1 || h > 4096) return 0;
    const int p = lcm_resize_passes(sw, sh, out_w, out_h);
    return ((p & 1) ? lcm_resize_table_bytes(sw, out_w, w) : 0) + ((p & 2) ? lcm_resize_table_bytes(sh, out_h, h) : 0);
}

// The tables of a call, as the head of its workspace holds them: the horizontal pass's, then the vertical pass's, each only
// if the pass runs.
extern "C" int lcm_resize_plan_tables(int sw, int sh, int out_w, int out_h, int x0, int y0, int w, int h, void* dst,
                                      long long dst_bytes) {
    const long long need = lcm_resize_plan_table_bytes(sw, sh, out_w, out_h, w, h);
    if (need <= 0 || !dst || dst_bytes < need) {
        lcm_set_error("resize_plan_tables: bad geometry %dx%d -> %dx%d window %dx%d, or a table of %lld bytes where %lld are needed",
                      sw, sh, out_w, out_h, w, h, dst_bytes, need);
        return LCM_EINVAL;
    }
    const int p = lcm_resize_passes(sw, sh, out_w, out_h);
    uint8_t* d = (uint8_t*)dst;
    if (p & 1) {
        const long long b = lcm_resize_table_bytes(sw, out_w, w);
        if (int rc = lcm_resize_tables(sw, out_w, x0, w, d, b)) return rc;
        d += b;
    }
    if (p & 2) return lcm_resize_tables(sh, out_h, y0, h, d, lcm_resize_table_bytes(sh, out_h, h));
    return LCM_OK;
}
