// Prompt emphasis (include/lcm_hip.h, "prompt emphasis"): the per-token weights of `(word:1.3)` applied to the
// text encoder's output, and the chunk's mean restored, in one launch that writes each chunk into its slot of the destination.
//
// One workgroup of 512 threads per 77-token chunk (8 waves, two per SIMD: up to 256 VGPRs each, so the chunk fits in registers
// without spilling; 1024 threads spilled at D >= 1024).  A chunk is 77 x D fp16 (116 - 193 KiB): every thread loads its 16-byte
// vectors ONCE (15 / 20 / 25 of them for D = 768 / 1024 / 1280) and keeps them in registers across the reduction, so the chunk is
// read from memory once for both sums and for the scaling.  The reduction order is fixed by the header and does not depend on the
// number of chunks or on the chunk's place in the launch: a chunk's bits are those of the same chunk launched alone.
#include "common.h"

namespace {
constexpr int PE_THREADS = 512, PE_WAVES = PE_THREADS / 64;

template <int D>
__global__ __launch_bounds__(PE_THREADS) void prompt_emphasis_kernel(const half_t* __restrict__ z, const float* __restrict__ w,
                                                                     half_t* __restrict__ out, long long ldo, int S) {
    constexpr int VPR = D / 8;                                   // 16-byte vectors per row
    constexpr int NV = (77 * VPR + PE_THREADS - 1) / PE_THREADS; // vectors per thread (S == 77, checked by the caller)
    __shared__ float part[2][PE_WAVES];
    const int tid = threadIdx.x, c = blockIdx.x;
    const int nvec = S * VPR;
    const half_t* zc = z + (long long)c * S * D;
    const float* wc = w + (long long)c * S;

    h8 v[NV];
    float wr[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int idx = tid + i * PE_THREADS;
        v[i] = (h8){0, 0, 0, 0, 0, 0, 0, 0};
        wr[i] = 0.f;
        if (idx < nvec) {
            v[i] = *reinterpret_cast<const h8*>(zc + (long long)idx * 8);
            wr[i] = wc[idx / VPR];
        }
    }
    // thread sums: elements 8 (tid + 512 i) + j, i ascending, then j ascending (vectors past the chunk add exact zeros)
    float s0 = 0.f, s1 = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float a = (float)v[i][j];
            s0 = s0 + a;
            s1 = __builtin_fmaf(a, wr[i], s1);
        }
    // wave: xor butterfly 32, 16, 8, 4, 2, 1; workgroup: the 8 wave sums added in wave order by every thread
    s0 = wave_sum(s0);
    s1 = wave_sum(s1);
    if ((tid & 63) == 0) { part[0][tid >> 6] = s0; part[1][tid >> 6] = s1; }
    __syncthreads();
    float t0 = 0.f, t1 = 0.f;
#pragma unroll
    for (int k = 0; k < PE_WAVES; ++k) { t0 += part[0][k]; t1 += part[1][k]; }
    const float r = t1 != 0.f ? t0 / t1 : 1.0f;                  // mean(z) / mean(z w): the counts cancel
    // (opaque: without it the compiler keeps the fp32 conversions of the reduction alive for the scaling, 8 registers per
    // vector instead of 4, and spills)
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        f4 t = __builtin_bit_cast(f4, v[i]);
        asm volatile("" : "+v"(t));
        v[i] = __builtin_bit_cast(h8, t);
    }

#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int idx = tid + i * PE_THREADS;
        if (idx < nvec) {
            const int row = idx / VPR, col = (idx - row * VPR) * 8;
            h8 o;
#pragma unroll
            for (int j = 0; j < 8; ++j) o[j] = (half_t)(((float)v[i][j] * wr[i]) * r);
            *reinterpret_cast<h8*>(out + ((long long)c * S + row) * ldo + col) = o;
        }
    }
}

template <int D>
int launch_emphasis(const void* z, const void* w, void* out, int ldo, int n_chunks, int S, hipStream_t s) {
    lcm_prof_start("prompt_emphasis_kernel", s);
    hipLaunchKernelGGL((prompt_emphasis_kernel<D>), dim3(n_chunks), dim3(PE_THREADS), 0, s, (const half_t*)z, (const float*)w,
                       (half_t*)out, (long long)ldo, S);
    lcm_prof_stop(s);
    LCM_CHECK_LAUNCH("prompt_emphasis");
    return LCM_OK;
}
}  // namespace

extern "C" int lcm_prompt_emphasis_f16(const void* z, const void* w, void* out, int ldo, int n_chunks, int S, int D, void* stream) {
    LCM_REQUIRE(z && w && out, "prompt_emphasis: null pointer");
    LCM_REQUIRE(n_chunks > 0, "prompt_emphasis: n_chunks %d must be positive", n_chunks);
    LCM_REQUIRE(S == 77, "prompt_emphasis: S = %d, a chunk is 77 tokens", S);
    LCM_REQUIRE(D == 768 || D == 1024 || D == 1280, "prompt_emphasis: D = %d, expected 768, 1024 or 1280", D);
    LCM_REQUIRE(ldo >= D && ldo % 8 == 0, "prompt_emphasis: ldo = %d must be a multiple of 8 and at least D = %d", ldo, D);
    LCM_REQUIRE(((uintptr_t)z & 15) == 0 && ((uintptr_t)out & 15) == 0 && ((uintptr_t)w & 3) == 0, "prompt_emphasis: misaligned pointer");
    hipStream_t s = (hipStream_t)stream;
    switch (D) {
        case 768: return launch_emphasis<768>(z, w, out, ldo, n_chunks, S, s);
        case 1024: return launch_emphasis<1024>(z, w, out, ldo, n_chunks, S, s);
        default: return launch_emphasis<1280>(z, w, out, ldo, n_chunks, S, s);
    }
}
