// Quantised DCT coefficients -> baseline JFIF file bytes on the host: the entropy-coding half of the JPEG output of the
// super-resolution worker (the reference's ``img.save(buf, format="JPEG", quality=q)``, server/lcm_sr_server.py).  The dense
// half -- colour conversion, 4:2:0 sampling, DCT, quantisation, zigzag -- runs on the GPU (jpeg.hip, lcm_jpeg_dct_rgb8) and
// hands over int16 [mcu_row][mcu_col][6][64] with the blocks Y00 Y01 Y10 Y11 Cb Cr in zigzag order.  Here:
//   * header: SOI, APP0 (JFIF 1.01), two DQT, SOF0 (Y 2x2, Cb 1x1, Cr 1x1), four DHT (the Annex K tables, as libjpeg writes
//     them when it does not optimise), DRI, SOS; one interleaved scan; EOI;
//   * the restart interval is ONE MCU ROW, whatever the thread count: DC prediction starts from 0 in every interval, an
//     interval ends padded with 1 bits and RSTn (n = row mod 8), so a row is coded knowing nothing of its neighbours;
//   * rows are coded in parallel on the pool png.cpp owns (at most `threads` at a time), each into its own worst-case slice
//     of the caller's buffer, and moved down into place in order.
// Deterministic: the bytes depend on (coefficients, size, quality) only.  No GPU is touched.
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <mutex>
#include <vector>

#define LCM_OK 0
#define LCM_EINVAL (-1)
void lcm_set_error(const char* fmt, ...);
void lcm_host_pool_for_each(size_t n, void (*fn)(void* ctx, size_t i), void* ctx);      // png.cpp

namespace {

// ITU-T T.81 Annex K.1 / K.2 quantisation tables, natural (row-major) order
const uint8_t K_LUMA[64] = {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,  14, 13, 16, 24, 40,  57,
                            69, 56, 14, 17, 22,  29,  51,  87,  80, 62, 18, 22, 37,  56,  68,  109, 103, 77, 24, 35, 55,  64,
                            81, 104, 113, 92, 49, 64,  78,  87,  103, 121, 120, 101, 72, 92,  95,  98,  112, 100, 103, 99};
const uint8_t K_CHROMA[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99,
                              99, 99, 47, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
                              99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};
// zigzag position -> natural index
const uint8_t ZZ[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                        41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                        30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// Annex K.3 Huffman tables: number of codes of each length 1..16, then the symbols in code order
const uint8_t DC_LUMA_BITS[16] = {0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0};
const uint8_t DC_CHROMA_BITS[16] = {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0};
const uint8_t DC_VALS[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
const uint8_t AC_LUMA_BITS[16] = {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d};
const uint8_t AC_LUMA_VALS[162] = {
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81,
    0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18,
    0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
    0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75,
    0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99,
    0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
    0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5,
    0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};
const uint8_t AC_CHROMA_BITS[16] = {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77};
const uint8_t AC_CHROMA_VALS[162] = {
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08,
    0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25,
    0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47,
    0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74,
    0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97,
    0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
    0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4,
    0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};

// symbol -> code (right aligned) and length, by the procedure of Annex C
struct HuffTable { uint16_t code[256]; uint8_t len[256]; };
HuffTable g_dc[2], g_ac[2];
std::once_flag g_huff_once;
void derive(const uint8_t* bits, const uint8_t* vals, HuffTable& t) {
    memset(&t, 0, sizeof(t));
    uint32_t code = 0;
    int k = 0;
    for (int l = 1; l <= 16; ++l) {
        for (int i = 0; i < bits[l - 1]; ++i, ++k) {
            t.code[vals[k]] = (uint16_t)code++;
            t.len[vals[k]] = (uint8_t)l;
        }
        code <<= 1;
    }
}
void huff_init() {
    derive(DC_LUMA_BITS, DC_VALS, g_dc[0]);
    derive(DC_CHROMA_BITS, DC_VALS, g_dc[1]);
    derive(AC_LUMA_BITS, AC_LUMA_VALS, g_ac[0]);
    derive(AC_CHROMA_BITS, AC_CHROMA_VALS, g_ac[1]);
}

// MSB-first bit stream with 0xFF -> 0xFF 0x00 stuffing.  The caller's slice is a worst-case bound, so nothing is checked per byte.
struct BitWriter {
    uint8_t* p;
    uint64_t acc = 0;          // the low `nbits` bits are pending, oldest highest
    int nbits = 0;
    bool bad = false;          // a coefficient outside the baseline categories was met
    inline void put(uint32_t v, int n) {           // n <= 27, v < 2^n
        acc = (acc << n) | v;
        nbits += n;
        if (nbits >= 32) {
            const uint32_t w = (uint32_t)(acc >> (nbits - 32));
            nbits -= 32;
            if ((w & 0x80808080u & ~(w + 0x01010101u)) == 0) {      // no byte of w is 0xFF (false positives take the slow way)
                p[0] = (uint8_t)(w >> 24); p[1] = (uint8_t)(w >> 16); p[2] = (uint8_t)(w >> 8); p[3] = (uint8_t)w;
                p += 4;
            } else {
                for (int s = 24; s >= 0; s -= 8) {
                    const uint8_t b = (uint8_t)(w >> s);
                    *p++ = b;
                    if (b == 0xFF) *p++ = 0;
                }
            }
        }
    }
    inline void finish() {                          // pad the last byte with 1 bits
        while (nbits >= 8) {
            const uint8_t b = (uint8_t)(acc >> (nbits - 8));
            nbits -= 8;
            *p++ = b;
            if (b == 0xFF) *p++ = 0;
        }
        if (nbits > 0) {
            const uint8_t b = (uint8_t)(((acc << (8 - nbits)) | (0xFFu >> nbits)) & 0xFF);
            *p++ = b;
            if (b == 0xFF) *p++ = 0;
            nbits = 0;
        }
    }
};

inline int bit_size(int a) { return a ? 32 - __builtin_clz((unsigned)a) : 0; }      // a >= 0

// one 8x8 block in zigzag order; returns the DC value (the next block's predictor)
inline int encode_block(BitWriter& bw, const int16_t* c, int pred, const HuffTable& dc, const HuffTable& ac) {
    const int d = c[0] - pred;
    {
        const int a = d < 0 ? -d : d, n = bit_size(a);
        if (n > 11) { bw.bad = true; return c[0]; }
        const uint32_t bits = (uint32_t)(d < 0 ? d - 1 : d) & ((1u << n) - 1);
        bw.put(((uint32_t)dc.code[n] << n) | bits, dc.len[n] + n);
    }
    uint64_t nz = 0;
    for (int k = 1; k < 64; ++k) nz |= (uint64_t)(c[k] != 0) << k;
    int last = 0;
    while (nz) {
        const int k = __builtin_ctzll(nz);
        nz &= nz - 1;
        int run = k - last - 1;
        last = k;
        while (run >= 16) { bw.put(ac.code[0xF0], ac.len[0xF0]); run -= 16; }
        const int v = c[k], a = v < 0 ? -v : v, n = bit_size(a);
        if (n > 10) { bw.bad = true; return c[0]; }
        const uint32_t bits = (uint32_t)(v < 0 ? v - 1 : v) & ((1u << n) - 1);
        const int sym = (run << 4) | n;
        bw.put(((uint32_t)ac.code[sym] << n) | bits, ac.len[sym] + n);
    }
    if (last != 63) bw.put(ac.code[0], ac.len[0]);
    return c[0];
}

// worst case of one block: 64 x (16-bit code + 11 value bits) = 216 bytes, every one of them stuffed
constexpr long long BLOCK_BOUND = 432;
constexpr long long HEADER_BOUND = 1024;
inline long long row_bound(int mcus_x) { return 6 * BLOCK_BOUND * mcus_x + 16; }

struct Job {
    const int16_t* coefs;
    int mcus_x, mcus_y;
    uint8_t* base;             // slice of row r starts at base + r * row_bound
    long long* len;            // bytes of row r, its RSTn included
    std::atomic<int> next{0};
    std::atomic<bool> bad{false};
};

void encode_row(Job& j, int r) {
    uint8_t* const out = j.base + (long long)r * row_bound(j.mcus_x);
    BitWriter bw{out};
    const int16_t* c = j.coefs + (long long)r * j.mcus_x * 384;
    int py = 0, pb = 0, pr = 0;
    for (int m = 0; m < j.mcus_x; ++m, c += 384) {
        py = encode_block(bw, c, py, g_dc[0], g_ac[0]);
        py = encode_block(bw, c + 64, py, g_dc[0], g_ac[0]);
        py = encode_block(bw, c + 128, py, g_dc[0], g_ac[0]);
        py = encode_block(bw, c + 192, py, g_dc[0], g_ac[0]);
        pb = encode_block(bw, c + 256, pb, g_dc[1], g_ac[1]);
        pr = encode_block(bw, c + 320, pr, g_dc[1], g_ac[1]);
    }
    bw.finish();
    if (r != j.mcus_y - 1) { *bw.p++ = 0xFF; *bw.p++ = (uint8_t)(0xD0 + (r & 7)); }
    j.len[r] = (long long)(bw.p - out);
    if (bw.bad) j.bad.store(true, std::memory_order_relaxed);
}

// one of `threads` workers of a call: takes rows until none are left
void row_worker(void* ctx, size_t) {
    Job& j = *(Job*)ctx;
    for (;;) {
        const int r = j.next.fetch_add(1, std::memory_order_relaxed);
        if (r >= j.mcus_y) return;
        encode_row(j, r);
    }
}

inline uint8_t* put16(uint8_t* p, unsigned v) { p[0] = (uint8_t)(v >> 8); p[1] = (uint8_t)v; return p + 2; }
uint8_t* put_dht(uint8_t* p, int tc_th, const uint8_t* bits, const uint8_t* vals) {
    int n = 0;
    for (int i = 0; i < 16; ++i) n += bits[i];
    *p++ = 0xFF; *p++ = 0xC4;
    p = put16(p, 2 + 1 + 16 + n);
    *p++ = (uint8_t)tc_th;
    memcpy(p, bits, 16); p += 16;
    memcpy(p, vals, n); p += n;
    return p;
}

inline bool shape_ok(int W, int H) { return W >= 1 && H >= 1 && W <= 65535 && H <= 65535; }

}  // namespace

// bytes of the coefficient buffer of a W x H image: 6 blocks of 64 int16 per 16x16 MCU
extern "C" long long lcm_jpeg_coef_bytes(int W, int H) {
    if (!shape_ok(W, H)) return 0;
    return (long long)((W + 15) / 16) * ((H + 15) / 16) * 768;
}

// capacity lcm_jpeg_encode_coefs needs for its output (the worst case of every interval plus the header)
extern "C" long long lcm_jpeg_bound(int W, int H) {
    if (!shape_ok(W, H)) return 0;
    return HEADER_BOUND + row_bound((W + 15) / 16) * ((H + 15) / 16);
}

// out[0..63] luma, out[64..127] chroma, natural order: jpeg_set_quality(quality, force_baseline = TRUE)
extern "C" int lcm_jpeg_quant_tables(int quality, uint8_t* out) {
    if (!out) { lcm_set_error("jpeg_quant_tables: null pointer"); return LCM_EINVAL; }
    if (quality < 1 || quality > 100) { lcm_set_error("jpeg_quant_tables: quality %d outside 1..100", quality); return LCM_EINVAL; }
    const int s = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    for (int i = 0; i < 128; ++i) {
        const int base = i < 64 ? K_LUMA[i] : K_CHROMA[i - 64];
        int v = (base * s + 50) / 100;
        out[i] = (uint8_t)(v < 1 ? 1 : v > 255 ? 255 : v);
    }
    return LCM_OK;
}

extern "C" int lcm_jpeg_encode_coefs(const void* coefs, int W, int H, int quality, int threads, void* out, long long out_cap,
                                     long long* out_len) {
    if (!coefs || !out || !out_len) { lcm_set_error("jpeg_encode_coefs: null pointer"); return LCM_EINVAL; }
    if (!shape_ok(W, H)) { lcm_set_error("jpeg_encode_coefs: bad shape %dx%d (1..65535 each)", W, H); return LCM_EINVAL; }
    uint8_t q[128];
    if (lcm_jpeg_quant_tables(quality, q) != LCM_OK) return LCM_EINVAL;
    if (out_cap < lcm_jpeg_bound(W, H)) { lcm_set_error("jpeg_encode_coefs: output buffer %lld < bound %lld", out_cap, lcm_jpeg_bound(W, H)); return LCM_EINVAL; }
    std::call_once(g_huff_once, huff_init);
    const int mcus_x = (W + 15) / 16, mcus_y = (H + 15) / 16;

    uint8_t* p = (uint8_t*)out;
    *p++ = 0xFF; *p++ = 0xD8;                                                    // SOI
    static const uint8_t APP0[18] = {0xFF, 0xE0, 0, 16, 'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0};
    memcpy(p, APP0, 18); p += 18;
    for (int t = 0; t < 2; ++t) {                                                // DQT, 8-bit entries in zigzag order
        *p++ = 0xFF; *p++ = 0xDB;
        p = put16(p, 67);
        *p++ = (uint8_t)t;
        for (int k = 0; k < 64; ++k) *p++ = q[64 * t + ZZ[k]];
    }
    *p++ = 0xFF; *p++ = 0xC0;                                                    // SOF0
    p = put16(p, 17);
    *p++ = 8;
    p = put16(p, (unsigned)H); p = put16(p, (unsigned)W);
    *p++ = 3;
    *p++ = 1; *p++ = 0x22; *p++ = 0;
    *p++ = 2; *p++ = 0x11; *p++ = 1;
    *p++ = 3; *p++ = 0x11; *p++ = 1;
    p = put_dht(p, 0x00, DC_LUMA_BITS, DC_VALS);
    p = put_dht(p, 0x10, AC_LUMA_BITS, AC_LUMA_VALS);
    p = put_dht(p, 0x01, DC_CHROMA_BITS, DC_VALS);
    p = put_dht(p, 0x11, AC_CHROMA_BITS, AC_CHROMA_VALS);
    *p++ = 0xFF; *p++ = 0xDD;                                                    // DRI: one MCU row
    p = put16(p, 4); p = put16(p, (unsigned)mcus_x);
    *p++ = 0xFF; *p++ = 0xDA;                                                    // SOS
    p = put16(p, 12);
    *p++ = 3;
    *p++ = 1; *p++ = 0x00; *p++ = 2; *p++ = 0x11; *p++ = 3; *p++ = 0x11;
    *p++ = 0; *p++ = 63; *p++ = 0;

    Job job;
    job.coefs = (const int16_t*)coefs;
    job.mcus_x = mcus_x;
    job.mcus_y = mcus_y;
    job.base = (uint8_t*)out + HEADER_BOUND;
    std::vector<long long> lens(mcus_y);
    job.len = lens.data();
    if (threads < 1) threads = 1;
    if (threads > mcus_y) threads = mcus_y;
    if (threads == 1) row_worker(&job, 0);
    else lcm_host_pool_for_each((size_t)threads, row_worker, &job);

    if (job.bad.load()) {
        lcm_set_error("jpeg_encode_coefs: a coefficient is outside the baseline range (DC difference +-2047, AC +-1023)");
        return LCM_EINVAL;
    }
    for (int r = 0; r < mcus_y; ++r) {
        const uint8_t* src = job.base + (long long)r * row_bound(mcus_x);
        if (p != src) memmove(p, src, (size_t)lens[r]);
        p += lens[r];
    }
    *p++ = 0xFF; *p++ = 0xD9;                                                    // EOI
    *out_len = (long long)(p - (uint8_t*)out);
    return LCM_OK;
}
