// Stand-alone host program around csrc/fastdiv.h (tests/test_entry_path_cpu.py builds and runs it): every multiply-shift or
// counter form the kernels now use, against the plain division it replaces.
//
//   entry_path_check [log2 of the dividend range, default 20]
//
// Exits 0 and prints "ok <comparisons>" when every comparison holds; prints the first mismatch and exits 1 otherwise.
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <thread>
#include <vector>

#include "fastdiv.h"

static std::atomic<long long> g_checked{0};
static std::atomic<int> g_bad{0};

static void fail(const char* what, long long a, long long b, long long got, long long want) {
    if (g_bad.fetch_add(1) == 0) std::fprintf(stderr, "MISMATCH %s: %lld / %lld -> %lld, want %lld\n", what, a, b, got, want);
}

// every dividend 0 .. nmax for the divisors d0, d0 + step, ... <= 4096.  The reference quotient is a counter (no division in
// the inner loop, so the whole 2^20 x 4096 sweep takes seconds); the counter itself is pinned to `/` at the range's end.
static void sweep(int d0, int step, int nmax) {
    long long n_checked = 0;
    for (int d = d0; d <= 4096; d += step) {
        const FastDiv f = fastdiv_make(d);
        int q = 0, r = 0;
        for (int n = 0; n <= nmax; ++n) {
            if (fastdiv(n, f) != q) { fail("sweep", n, d, fastdiv(n, f), q); return; }
            if (++r == d) { r = 0; ++q; }
        }
        if (q != (nmax + 1) / d) { fail("sweep reference", nmax + 1, d, q, (nmax + 1) / d); return; }
        n_checked += nmax + 1;
        // the ends of the range the header promises (dividends below 2^31), around multiples of d
        for (long long k : {1ll, 2ll, 3ll, (long long)(0x7fffffff / d) - 1, (long long)(0x7fffffff / d)})
            for (int e = -1; e <= 1; ++e) {
                const long long n = k * d + e;
                if (n < 0 || n > 0x7fffffffll) continue;
                if (fastdiv((int)n, f) != (int)(n / d)) { fail("edge", n, d, fastdiv((int)n, f), n / d); return; }
                ++n_checked;
            }
        if (fastdiv(0x7fffffff, f) != 0x7fffffff / d) { fail("edge", 0x7fffffff, d, fastdiv(0x7fffffff, f), 0x7fffffff / d); return; }
    }
    g_checked += n_checked;
}

int main(int argc, char** argv) {
    const int lg = argc > 1 ? std::atoi(argv[1]) : 20;
    const int nmax = 1 << lg;
    // 1. ntiles, n_iters / ngroups, splits, nkr, patch counts, image sides: every divisor 1 .. 4096, every dividend 0 .. 2^lg
    unsigned nt = std::thread::hardware_concurrency();
    nt = nt < 1 ? 1 : nt > 16 ? 16 : nt;
    std::vector<std::thread> th;
    for (unsigned t = 0; t < nt; ++t) th.emplace_back(sweep, 1 + (int)t, (int)nt, nmax);
    for (auto& t : th) t.join();

    // large divisors (rows per image, slab counts): powers of two and their neighbours, dividends spread over [0, 2^31)
    for (int l = 12; l <= 30; ++l)
        for (int e = -1; e <= 1; ++e) {
            const int d = (1 << l) + e;
            const FastDiv f = fastdiv_make(d);
            for (long long n = 0; n <= 0x7fffffffll; n += 104729) {
                if (fastdiv((int)n, f) != (int)(n / d)) fail("large", n, d, fastdiv((int)n, f), n / d);
                ++g_checked;
            }
            for (long long k = 1; k * d <= 0x7fffffffll && k < 64; ++k)
                for (int e2 = -1; e2 <= 0; ++e2) {
                    const long long n = k * d + e2;
                    if (fastdiv((int)n, f) != (int)(n / d)) fail("large edge", n, d, fastdiv((int)n, f), n / d);
                    ++g_checked;
                }
        }

    // 2. kt0 / kt1 (and the chunk bounds of the convolutions, and the part bounds of segmented accumulation): the 32-bit
    //    multiply-shift form against the 64-bit signed division of the parent kernels
    for (int nk = 1; nk <= 360; ++nk)
        for (int splits = 1; splits <= 16; ++splits) {
            const FastDiv f = fastdiv_make(splits);
            int prev_end = 0;
            for (int y = 0; y < splits; ++y) {
                int k0, k1;
                split_bounds(y, nk, f, k0, k1);
                const int w0 = (int)((long long)y * nk / splits), w1 = (int)((long long)(y + 1) * nk / splits);
                if (k0 != w0) fail("kt0", (long long)y * nk, splits, k0, w0);
                if (k1 != w1) fail("kt1", (long long)(y + 1) * nk, splits, k1, w1);
                if (k0 != prev_end) fail("kt ranges are not contiguous", y, splits, k0, prev_end);
                prev_end = k1;
                g_checked += 2;
            }
            if (prev_end != nk) fail("kt ranges do not cover K", nk, splits, prev_end, nk);
        }

    // 3. issue_tile's counters against t / nkr, t % nkr for every ring step of every (kt0, nkr, n_iters)
    for (int kt0 = 0; kt0 <= 7; kt0 += 7)
        for (int nkr = 1; nkr <= 360; ++nkr)
            for (int n_iters = 1; n_iters <= 5; ++n_iters) {
                WrapCounter c = {kt0, 0};
                for (int t = 0; t < nkr * n_iters; ++t) {
                    const int ni = t / nkr, kt = kt0 + (t - ni * nkr);
                    if (c.outer != ni) fail("issue counter ni", t, nkr, c.outer, ni);
                    if (c.inner != kt) fail("issue counter kt", t, nkr, c.inner, kt);
                    wrap_step(c, kt0, kt0 + nkr);
                    ++g_checked;
                }
            }

    // 4. the reduce's patch coordinates: shifts for the 16- and 8-wide patches against / and %
    for (int twl = 3; twl <= 4; ++twl) {
        const int TW = 1 << twl, RS = 32 / TW;
        for (int syi = 0; syi < 600; ++syi)
            for (int q = 0; q < 32; ++q) {
                if ((syi << (5 - twl)) + (q >> twl) != syi * RS + q / TW) fail("patch row", q, TW, (syi << (5 - twl)) + (q >> twl), syi * RS + q / TW);
                if ((syi << twl) + (q & (TW - 1)) != syi * TW + q % TW) fail("patch column", q, TW, (syi << twl) + (q & (TW - 1)), syi * TW + q % TW);
                g_checked += 2;
            }
    }
    if (g_bad.load()) return 1;
    std::printf("ok %lld\n", g_checked.load());
    return 0;
}
