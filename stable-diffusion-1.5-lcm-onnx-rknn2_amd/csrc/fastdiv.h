// Division by a launch-time constant as multiply-high + shift, shared by the host (which derives the magic number once per
// launch) and the kernels (which would otherwise run a v_rcp_iflag division chain -- about 25 dependent instructions for an
// unsigned 32-bit quotient, several times that for a signed 64-bit one -- in front of their first load).
//
//   FastDiv f = fastdiv_make(d);          1 <= d < 2^31
//   fastdiv(n, f) == n / d                for every 0 <= n < 2^31
//
// Round-up method (Granlund & Montgomery): with p = 31 + ceil(log2 d) and m = ceil(2^p / d) < 2^32,
// floor(n m / 2^p) = floor(n / d) for n < 2^31.  d = 1 would need m = 2^31 and a shift of -1: it is encoded as mul = 0.
// Plain C++ (the 64-bit product lowers to v_mul_hi_u32 / s_mul_hi_u32): one text for hipcc's host and device passes and for
// a host-only compiler (tests/test_entry_path_cpu.py builds this header into a stand-alone program).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LCM_HD __host__ __device__ __forceinline__
#else
#define LCM_HD inline
#endif

struct FastDiv {
    uint32_t mul;      // 0: divisor 1
    uint32_t shr;
};

inline FastDiv fastdiv_make(int d) {
    FastDiv f = {0u, 0u};
    if (d <= 1) return f;
    uint32_t l = 0;
    while ((1u << l) < (uint32_t)d) ++l;                       // ceil(log2 d), 1 .. 31
    const uint64_t p2 = (uint64_t)1 << (31 + l);
    f.mul = (uint32_t)((p2 + (uint32_t)d - 1) / (uint32_t)d);
    f.shr = l - 1;                                             // (31 + l) - 32
    return f;
}

LCM_HD int fastdiv(int n, FastDiv f) {
    const uint32_t hi = (uint32_t)(((uint64_t)(uint32_t)n * f.mul) >> 32);
    return f.mul ? (int)(hi >> f.shr) : n;
}

// blockIdx.y's share of nk k-tiles (or 64-channel chunks) split `splits` ways: [y nk / splits, (y + 1) nk / splits).
// y < splits <= 64 and nk < 2^24, so the products stay far below 2^31 and the 32-bit form equals the 64-bit one.
LCM_HD void split_bounds(int y, int nk, FastDiv splits, int& k0, int& k1) {
    k0 = fastdiv(y * nk, splits);
    k1 = fastdiv((y + 1) * nk, splits);
}

// Flattened (outer, inner) walk of a ring issue order: `inner` runs lo .. hi - 1, then wraps and `outer` advances -- the
// (t / n, t % n) of consecutive t without the division.
struct WrapCounter {
    int inner, outer;
};
LCM_HD void wrap_step(WrapCounter& c, int lo, int hi) {
    if (++c.inner == hi) { c.inner = lo; ++c.outer; }
}
