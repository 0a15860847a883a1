// JFIF / JPEG file bytes -> quantised DCT coefficients on the host: the marker and entropy-decoding half of the JPEG *input* of
// the super-resolution worker (the reference's ``Image.open(io.BytesIO(image_bytes)).convert("RGB")``, server/lcm_sr_server.py).
// The dense half -- dequantisation, inverse DCT, chroma upsampling, colour conversion -- runs on the GPU (jpeg_dec.hip,
// lcm_jpeg_idct_rgb8) on the int16 [mcu_row][mcu_col][blocks per MCU][64] this file writes, every block in zigzag order as it
// is in the file: for 4:2:0 that is exactly the layout the encoder's front end produces (jpeg.hip / jpeg.cpp).  Here:
//   * lcm_jpeg_dec_info: walks the markers.  Baseline and extended sequential Huffman (SOF0, SOF1), 8 bit, one interleaved
//     scan, Y only or YCbCr at 4:4:4 / 4:2:2 / 4:2:0, any DHT, with or without DRI; anything else is LCM_EUNSUPPORTED and the
//     caller hands the file to PIL;
//   * lcm_jpeg_dec_coefs: the restart intervals are found by looking for FFD0..FFD7 (byte stuffing makes them unambiguous) and
//     decoded in parallel on the pool png.cpp owns, each from a DC predictor of 0 into its own run of MCUs, so the result does
//     not depend on the thread count.  A file without DRI is one interval on one thread.  Every read is bounded by the
//     interval: past its end the bit reader supplies zeros and counts them, and an interval that consumed one is an error.
// No GPU is touched.
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <vector>

#include "../../include/lcm_hip.h"      // lcm_jpeg_info, LCM_E*

void lcm_set_error(const char* fmt, ...);
void lcm_host_pool_for_each(size_t n, void (*fn)(void* ctx, size_t i), void* ctx);      // png.cpp

namespace {

// zigzag position -> natural index
const uint8_t ZZ[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                        41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                        30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

constexpr int LOOK = 10;       // bits of the first-level Huffman lookup

struct HuffDec {
    bool defined = false;
    uint16_t fast[1 << LOOK];  // (length << 8) | symbol for codes of <= LOOK bits, 0 = longer
    int32_t maxcode[18];       // largest code of each length, -1 = none (T.81 Annex F.2.2.3)
    int32_t valoff[17];        // symbol index of a code = code + valoff[length]
    uint8_t vals[256];
};

// T.81 Annex C code assignment; false if the counts do not describe a prefix code
bool build_huff(const uint8_t* bits, const uint8_t* vals, int nvals, HuffDec& t) {
    memset(t.fast, 0, sizeof(t.fast));
    memcpy(t.vals, vals, (size_t)nvals);
    int32_t code = 0;
    int k = 0;
    for (int l = 1; l <= 16; ++l) {
        t.valoff[l] = k - code;
        const int n = bits[l - 1];
        if (n) {
            if (code + n > (1 << l)) return false;
            for (int i = 0; i < n; ++i, ++k, ++code) {
                if (l <= LOOK) {
                    const int lo = code << (LOOK - l);
                    for (int j = 0; j < (1 << (LOOK - l)); ++j) t.fast[lo + j] = (uint16_t)((l << 8) | vals[k]);
                }
            }
            t.maxcode[l] = code - 1;
        } else {
            t.maxcode[l] = -1;
        }
        code <<= 1;
    }
    t.maxcode[17] = 0x7FFFFFFF;
    t.defined = true;
    return true;
}

struct Parsed {
    lcm_jpeg_info info;
    HuffDec dc[4], ac[4];
    int td[3], ta[3];                      // table selectors of the scan's components
    int comp_h[3], comp_v[3];
    long long scan_begin = 0;              // first byte of entropy-coded data
    std::vector<long long> iv_begin, iv_end;   // restart intervals, [begin, end)
    bool saw_eoi = false;
    int bad_rst = 0;                       // an RSTn out of sequence was met
};

inline int be16(const uint8_t* p) { return (p[0] << 8) | p[1]; }

// Fills P from the markers.  `why` receives a short reason for LCM_EINVAL / LCM_EUNSUPPORTED.
int parse(const uint8_t* d, long long len, Parsed& P, const char*& why) {
    if (len < 4 || d[0] != 0xFF || d[1] != 0xD8) { why = "no SOI marker"; return LCM_EINVAL; }
    uint8_t qtab[4][64];
    bool qdef[4] = {false, false, false, false};
    int comp_id[3] = {0, 0, 0}, comp_tq[3] = {0, 0, 0};
    bool sof = false, jfif = false, adobe = false;
    int adobe_transform = -1, ri = 0;
    lcm_jpeg_info& I = P.info;
    memset(&I, 0, sizeof(I));
    long long i = 2;
    for (;;) {
        if (i + 2 > len) { why = "file ends before the scan"; return LCM_EINVAL; }
        if (d[i] != 0xFF) { why = "marker expected"; return LCM_EINVAL; }
        while (i + 1 < len && d[i + 1] == 0xFF) ++i;              // fill bytes
        if (i + 2 > len) { why = "file ends before the scan"; return LCM_EINVAL; }
        const int mk = d[i + 1];
        i += 2;
        if (mk == 0x01 || (mk >= 0xD0 && mk <= 0xD7)) continue;   // stand-alone
        if (mk == 0xD9) { why = "EOI before any scan"; return LCM_EINVAL; }
        if (mk == 0xD8 || mk == 0x00) { why = "stray marker"; return LCM_EINVAL; }
        if (i + 2 > len) { why = "file ends inside a marker"; return LCM_EINVAL; }
        const int L = be16(d + i);
        if (L < 2 || i + L > len) { why = "file ends inside a marker"; return LCM_EINVAL; }
        const uint8_t* s = d + i + 2;
        const int n = L - 2;
        i += L;
        if (mk == 0xC0 || mk == 0xC1) {
            if (sof) { why = "two frame headers"; return LCM_EUNSUPPORTED; }
            if (n < 6) { why = "short SOF"; return LCM_EINVAL; }
            if (s[0] != 8) { why = "sample precision is not 8 bit"; return LCM_EUNSUPPORTED; }
            I.height = be16(s + 1);
            I.width = be16(s + 3);
            I.ncomp = s[5];
            if (I.ncomp != 1 && I.ncomp != 3) { why = "neither 1 nor 3 components"; return LCM_EUNSUPPORTED; }
            if (n != 6 + 3 * I.ncomp) { why = "bad SOF length"; return LCM_EINVAL; }
            if (I.height == 0) { why = "height given by DNL"; return LCM_EUNSUPPORTED; }
            if (I.width == 0) { why = "width 0"; return LCM_EINVAL; }
            for (int c = 0; c < I.ncomp; ++c) {
                comp_id[c] = s[6 + 3 * c];
                P.comp_h[c] = s[7 + 3 * c] >> 4;
                P.comp_v[c] = s[7 + 3 * c] & 15;
                comp_tq[c] = s[8 + 3 * c];
                if (comp_tq[c] > 3) { why = "quantisation table selector > 3"; return LCM_EINVAL; }
            }
            sof = true;
        } else if (mk >= 0xC2 && mk <= 0xCF && mk != 0xC4) {
            why = "not a sequential Huffman frame (progressive, lossless, arithmetic or hierarchical)";
            return LCM_EUNSUPPORTED;
        } else if (mk == 0xC4) {
            int j = 0;
            while (j < n) {
                if (j + 17 > n) { why = "short DHT"; return LCM_EINVAL; }
                const int tc = s[j] >> 4, th = s[j] & 15;
                int cnt = 0;
                for (int k = 0; k < 16; ++k) cnt += s[j + 1 + k];
                if (tc > 1 || th > 3 || cnt > 256 || j + 17 + cnt > n) { why = "bad DHT"; return LCM_EINVAL; }
                if (!build_huff(s + j + 1, s + j + 17, cnt, tc ? P.ac[th] : P.dc[th])) { why = "DHT is not a prefix code"; return LCM_EINVAL; }
                j += 17 + cnt;
            }
        } else if (mk == 0xDB) {
            int j = 0;
            while (j < n) {
                const int pq = s[j] >> 4, tq = s[j] & 15;
                if (tq > 3 || pq > 1) { why = "bad DQT"; return LCM_EINVAL; }
                if (pq == 1) { why = "16-bit quantisation table"; return LCM_EUNSUPPORTED; }
                if (j + 65 > n) { why = "short DQT"; return LCM_EINVAL; }
                for (int k = 0; k < 64; ++k) qtab[tq][ZZ[k]] = s[j + 1 + k];
                qdef[tq] = true;
                j += 65;
            }
        } else if (mk == 0xDD) {
            if (n != 2) { why = "bad DRI"; return LCM_EINVAL; }
            ri = be16(s);
        } else if (mk == 0xE0) {
            if (n >= 5 && memcmp(s, "JFIF", 5) == 0) jfif = true;
        } else if (mk == 0xEE) {
            if (n >= 12 && memcmp(s, "Adobe", 5) == 0) { adobe = true; adobe_transform = s[11]; }
        } else if (mk == 0xDA) {
            if (!sof) { why = "scan before the frame header"; return LCM_EINVAL; }
            if (n < 1) { why = "short SOS"; return LCM_EINVAL; }
            const int ns = s[0];
            if (ns < 1 || ns > 4 || n != 4 + 2 * ns) { why = "bad SOS length"; return LCM_EINVAL; }
            if (ns != I.ncomp) { why = "the scan does not interleave every component (several scans)"; return LCM_EUNSUPPORTED; }
            for (int c = 0; c < ns; ++c) {
                if (s[1 + 2 * c] != comp_id[c]) { why = "scan components are not in frame order"; return LCM_EUNSUPPORTED; }
                P.td[c] = s[2 + 2 * c] >> 4;
                P.ta[c] = s[2 + 2 * c] & 15;
                if (P.td[c] > 3 || P.ta[c] > 3) { why = "Huffman table selector > 3"; return LCM_EINVAL; }
                if (!P.dc[P.td[c]].defined || !P.ac[P.ta[c]].defined) { why = "the scan uses a Huffman table no DHT defined"; return LCM_EINVAL; }
            }
            if (s[1 + 2 * ns] != 0 || s[2 + 2 * ns] != 63 || s[3 + 2 * ns] != 0) { why = "not a full sequential scan (Ss, Se, Ah, Al)"; return LCM_EUNSUPPORTED; }
            break;
        }
        // every other segment (APPn, COM, ...) is skipped
    }
    P.scan_begin = i;

    // sampling class
    if (I.ncomp == 1) {
        if (P.comp_h[0] != 1 || P.comp_v[0] != 1) { why = "grayscale with sampling factors other than 1x1"; return LCM_EUNSUPPORTED; }
        I.sampling = 0;
    } else {
        if (P.comp_h[1] != 1 || P.comp_v[1] != 1 || P.comp_h[2] != 1 || P.comp_v[2] != 1) { why = "chroma sampling is not 1x1"; return LCM_EUNSUPPORTED; }
        const int h = P.comp_h[0], v = P.comp_v[0];
        if (h == 1 && v == 1) I.sampling = 0;
        else if (h == 2 && v == 1) I.sampling = 1;
        else if (h == 2 && v == 2) I.sampling = 2;
        else { why = "luma sampling is none of 1x1, 2x1, 2x2"; return LCM_EUNSUPPORTED; }
        // the colour space libjpeg would assume: JFIF -> YCbCr; Adobe -> by its transform flag; neither -> by the component ids
        if (adobe && adobe_transform != 1) { why = "Adobe marker: the components are not YCbCr"; return LCM_EUNSUPPORTED; }
        if (!jfif && !adobe && !(comp_id[0] == 1 && comp_id[1] == 2 && comp_id[2] == 3)) { why = "component ids other than 1, 2, 3 without a JFIF marker"; return LCM_EUNSUPPORTED; }
    }
    for (int c = 0; c < I.ncomp; ++c) {
        if (!qdef[comp_tq[c]]) { why = "a component uses a quantisation table no DQT defined"; return LCM_EINVAL; }
        memcpy(I.qt[c], qtab[comp_tq[c]], 64);
    }
    const int hmax = I.sampling >= 1 ? 2 : 1, vmax = I.sampling == 2 ? 2 : 1;
    I.mcus_x = (I.width + 8 * hmax - 1) / (8 * hmax);
    I.mcus_y = (I.height + 8 * vmax - 1) / (8 * vmax);
    I.blocks_per_mcu = I.ncomp == 1 ? 1 : hmax * vmax + 2;
    I.restart_interval = ri;
    const long long nm = (long long)I.mcus_x * I.mcus_y;
    I.coefs_bytes = nm * I.blocks_per_mcu * 128;
    I.work_bytes = nm * I.blocks_per_mcu * 64;              // one byte per sample of every block

    // the entropy-coded segment: cut at every marker
    long long start = i, pos = i;
    int nrst = 0;
    for (;;) {
        const uint8_t* f = pos < len ? (const uint8_t*)memchr(d + pos, 0xFF, (size_t)(len - pos)) : nullptr;
        if (!f || f + 1 >= d + len) {                                  // no marker ends the data
            P.iv_begin.push_back(start);
            P.iv_end.push_back(len);
            break;
        }
        const long long j = f - d;
        const int nx = d[j + 1];
        if (nx == 0) { pos = j + 2; continue; }
        if (nx == 0xFF) { pos = j + 1; continue; }
        P.iv_begin.push_back(start);
        P.iv_end.push_back(j);
        if (nx >= 0xD0 && nx <= 0xD7) {
            if (nx - 0xD0 != (nrst & 7)) P.bad_rst = 1;
            ++nrst;
            start = pos = j + 2;
            continue;
        }
        if (nx == 0xD9) { P.saw_eoi = true; break; }
        why = "a marker other than RSTn / EOI follows the scan (several scans, DNL, or tables between scans)";
        return LCM_EUNSUPPORTED;
    }
    return LCM_OK;
}

// MSB-first bit reader over one restart interval with the 0xFF 0x00 stuffing removed.  Past the end it supplies zero bits and
// counts them in `fake`.
struct BitReader {
    const uint8_t* p;
    const uint8_t* end;
    uint64_t acc = 0;          // the low n bits are unread, oldest highest
    int n = 0;
    int fake = 0;
    inline void refill() {     // afterwards n >= 32
        if (n <= 32 && end - p >= 4) {
            const uint32_t w = ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3];
            if ((w & 0x80808080u & ~(w + 0x01010101u)) == 0) {        // no byte of w is 0xFF (false positives take the slow way)
                acc = (acc << 32) | w;
                n += 32;
                p += 4;
                return;
            }
        }
        while (n <= 56) {
            uint8_t b = 0;
            if (p < end) {
                b = *p++;
                if (b == 0xFF) {
                    if (p < end && *p == 0) ++p;
                    else if (p < end) p = end;       // fill byte in front of the marker that ends the interval
                }
            } else {
                fake += 8;
            }
            acc = (acc << 8) | b;
            n += 8;
        }
    }
    inline uint32_t peek(int k) const { return (uint32_t)(acc >> (n - k)) & ((1u << k) - 1); }
    inline void skip(int k) { n -= k; }
    inline int get_extended(int s) {                                   // s bits as a signed value of category s (T.81 F.2.2.1)
        if (s == 0) return 0;
        const int v = (int)peek(s);
        n -= s;
        return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v;
    }
};

// next Huffman symbol, -1 if no code matches (16 one bits in a table without that code)
inline int decode_sym(BitReader& br, const HuffDec& t) {
    const uint32_t e = t.fast[br.peek(LOOK)];
    if (e) { br.skip((int)(e >> 8)); return (int)(e & 255); }
    int l = LOOK + 1;
    int32_t code = (int32_t)br.peek(l);
    while (l <= 16 && code > t.maxcode[l]) { ++l; code = (int32_t)br.peek(l); }
    if (l > 16) return -1;
    br.skip(l);
    return t.vals[(code + t.valoff[l]) & 255];
}

enum { E_NONE = 0, E_CODE, E_RUN, E_RANGE, E_SHORT, E_EXTRA };

struct Job {
    const uint8_t* data;
    const Parsed* P;
    int16_t* coefs;
    long long total_mcus, per_interval;
    size_t nint, chunk;
    std::atomic<size_t> next{0};
    std::atomic<int> err{E_NONE};
};

int decode_interval(const Job& j, size_t iv) {
    const Parsed& P = *j.P;
    const lcm_jpeg_info& I = P.info;
    const long long m0 = (long long)iv * j.per_interval;
    const long long nm = m0 + j.per_interval <= j.total_mcus ? j.per_interval : j.total_mcus - m0;
    const int bpm = I.blocks_per_mcu, ny = bpm == 1 ? 1 : bpm - 2;
    int16_t* c = j.coefs + m0 * bpm * 64;
    memset(c, 0, (size_t)nm * bpm * 128);
    BitReader br{j.data + P.iv_begin[iv], j.data + P.iv_end[iv]};
    int pred[3] = {0, 0, 0};
    for (long long m = 0; m < nm; ++m) {
        for (int b = 0; b < bpm; ++b, c += 64) {
            const int ci = b < ny ? 0 : b - ny + 1;
            const HuffDec& dc = P.dc[P.td[ci]];
            const HuffDec& ac = P.ac[P.ta[ci]];
            if (br.n < 32) br.refill();
            int s = decode_sym(br, dc);
            if (s < 0 || s > 11) return E_CODE;
            pred[ci] += br.get_extended(s);
            if (pred[ci] < -2047 || pred[ci] > 2047) return E_RANGE;
            c[0] = (int16_t)pred[ci];
            for (int k = 1; k < 64;) {
                if (br.n < 32) br.refill();
                const int rs = decode_sym(br, ac);
                if (rs < 0) return E_CODE;
                const int r = rs >> 4;
                s = rs & 15;
                if (s == 0) {
                    if (r == 15) { k += 16; continue; }
                    if (r != 0) return E_CODE;                          // EOBn belongs to progressive scans
                    break;
                }
                if (s > 10) return E_RANGE;
                k += r;
                if (k > 63) return E_RUN;
                c[k++] = (int16_t)br.get_extended(s);
            }
        }
        if (br.n < br.fake) return E_SHORT;
    }
    if (br.n < br.fake) return E_SHORT;
    if ((br.n - br.fake) + 8 * (long long)(br.end - br.p) >= 8) return E_EXTRA;
    return E_NONE;
}

void interval_worker(void* ctx, size_t) {
    Job& j = *(Job*)ctx;
    for (;;) {
        const size_t i0 = j.next.fetch_add(j.chunk, std::memory_order_relaxed);
        if (i0 >= j.nint || j.err.load(std::memory_order_relaxed) != E_NONE) return;
        const size_t i1 = i0 + j.chunk < j.nint ? i0 + j.chunk : j.nint;
        for (size_t i = i0; i < i1; ++i) {
            const int e = decode_interval(j, i);
            if (e != E_NONE) {
                int none = E_NONE;
                j.err.compare_exchange_strong(none, e);
                return;
            }
        }
    }
}

}  // namespace

extern "C" int lcm_jpeg_dec_info(const void* data, long long len, lcm_jpeg_info* info) {
    if (!data || !info) { lcm_set_error("jpeg_dec_info: null pointer"); return LCM_EINVAL; }
    Parsed P;
    const char* why = "";
    const int rc = parse((const uint8_t*)data, len, P, why);
    if (rc != LCM_OK) { lcm_set_error("jpeg_dec_info: %s", why); return rc; }
    *info = P.info;
    return LCM_OK;
}

extern "C" int lcm_jpeg_dec_coefs(const void* data, long long len, int threads, void* coefs, long long coefs_bytes) {
    if (!data || !coefs) { lcm_set_error("jpeg_dec_coefs: null pointer"); return LCM_EINVAL; }
    Parsed P;
    const char* why = "";
    const int rc = parse((const uint8_t*)data, len, P, why);
    if (rc != LCM_OK) { lcm_set_error("jpeg_dec_coefs: %s", why); return rc; }
    const lcm_jpeg_info& I = P.info;
    if (coefs_bytes < I.coefs_bytes) { lcm_set_error("jpeg_dec_coefs: coefficient buffer %lld < %lld bytes", coefs_bytes, I.coefs_bytes); return LCM_EINVAL; }
    if (!P.saw_eoi) { lcm_set_error("jpeg_dec_coefs: premature end of the file (no EOI)"); return LCM_EINVAL; }
    Job job;
    job.data = (const uint8_t*)data;
    job.P = &P;
    job.coefs = (int16_t*)coefs;
    job.total_mcus = (long long)I.mcus_x * I.mcus_y;
    job.per_interval = I.restart_interval ? I.restart_interval : job.total_mcus;
    job.nint = P.iv_begin.size();
    const long long want = (job.total_mcus + job.per_interval - 1) / job.per_interval;
    if ((long long)job.nint != want) {
        lcm_set_error("jpeg_dec_coefs: %lld restart intervals for %lld MCUs at a restart interval of %d (missing or surplus RSTn)",
                      (long long)job.nint, job.total_mcus, I.restart_interval);
        return LCM_EINVAL;
    }
    if (P.bad_rst) { lcm_set_error("jpeg_dec_coefs: RSTn markers out of sequence"); return LCM_EINVAL; }
    if (threads < 1) threads = 1;
    if ((size_t)threads > job.nint) threads = (int)job.nint;
    job.chunk = job.nint / ((size_t)threads * 8);
    if (job.chunk < 1) job.chunk = 1;
    if (threads == 1) interval_worker(&job, 0);
    else lcm_host_pool_for_each((size_t)threads, interval_worker, &job);
    static const char* const MSG[] = {"", "bad Huffman code", "zero run past the end of a block",
                                      "coefficient outside the 8-bit range (DC +-2047, AC +-1023)",
                                      "premature end of a restart interval", "extraneous bytes at the end of a restart interval"};
    const int e = job.err.load();
    if (e != E_NONE) { lcm_set_error("jpeg_dec_coefs: corrupt scan: %s", MSG[e]); return LCM_EINVAL; }
    return LCM_OK;
}
