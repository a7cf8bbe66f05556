// The coder of the device JPEG encoder (jpeg_encode.hip), as code that compiles for the host and for the device: the frame's
// geometry, colour conversion, chroma averaging, the forward DCT, quantisation, the Huffman coding of one block and its bit
// packing, the file's header.  Everything is 32-bit integer arithmetic, so the host build of these functions gives the device's
// bits: jpeg_host_encode() below walks the same intervals and blocks serially and its file is the kernels' byte for byte -- and
// both are what libjpeg writes (baseline, 4:2:0, the "islow" transform, the tables of T.81 Annex K, a restart interval of
// kJpegRestart MCUs), segment for segment and bit for bit in the scan.
//
// The file:  SOI | APP0 (JFIF) | DQT x 2 | SOF0 | DHT x 4 | DRI | SOS | interval 0 | RST0 | interval 1 | RST1 | ... | EOI
// An MCU is 16x16 pixels: four Y blocks (0,0) (0,1) (1,0) (1,1), Cb, Cr.  An interval is kJpegRestart MCUs in raster order; its
// bits begin and end on a byte (padded with 1-bits), every FF in it is followed by a stuffed 00, and the DC predictors start at 0,
// so intervals are coded independently of each other and concatenate by byte offsets.
#pragma once
#include <stdint.h>
#include <stddef.h>
#include <stdlib.h>
#include <string.h>
#include "jpeg_tables.h"

#if defined(__HIPCC__)
#define JPEG_HD __host__ __device__ inline
#else
#define JPEG_HD inline
#endif

constexpr int kJpegRestart = 8;                                     // MCUs of a restart interval
constexpr int kJpegMcuBlocks = 6;
constexpr int kJpegIntervalBlocks = kJpegRestart * kJpegMcuBlocks;  // 48: the lanes of one wave take a block each
// A block's code at its longest: the DC code (at most 11 bits in the chrominance table) and 11 value bits, then 63 coefficients of
// a 16-bit code and 10 value bits each, no end of block.
constexpr int kJpegBlockMaxBits = 22 + 63 * 26;
constexpr int kJpegBlockMaxBytes = (kJpegBlockMaxBits + 7) / 8;                                     // 208
constexpr int kJpegImgWords = (kJpegIntervalBlocks * kJpegBlockMaxBytes + 3) / 4 + 2;               // an interval's bits, unstuffed
constexpr int kJpegCoefStride = 66;                                 // int16s of a block in LDS: 33 words, odd
constexpr int kJpegHeaderBytes = 2 + 18 + 2 * 69 + 19 + 2 * (33 + 183) + 6 + 14;                    // SOI .. SOS
static_assert(kJpegIntervalBlocks <= 64, "one lane per block of an interval");
static_assert(kJpegHeaderBytes == 629, "the header's layout changed");

struct JpegDht {
    uint8_t tc_th, n;
    uint8_t counts[16];
    uint8_t symbols[JPEG_DHT_MAX_SYMBOLS];
};
struct JpegQuant {
    uint8_t q[2][64];       // luminance, chrominance; zigzag order
};

// ---- shapes ---------------------------------------------------------------------------------------------------------------
struct JpegGeom {
    int H, W;
    int ybw, ybh;           // the Y block grid; blocks of an MCU outside it are dummy blocks
    int mw, mh, nmcu;       // MCUs (the chroma block grid is mw x mh too)
    int nint;               // restart intervals
};
JPEG_HD JpegGeom jpeg_geom(int H, int W)
{
    JpegGeom g;
    g.H = H; g.W = W;
    g.ybw = (W + 7) / 8; g.ybh = (H + 7) / 8;
    g.mw = (W + 15) / 16; g.mh = (H + 15) / 16;
    g.nmcu = g.mw * g.mh;
    g.nint = (g.nmcu + kJpegRestart - 1) / kJpegRestart;
    return g;
}
// bytes an interval of `mcus` MCUs can take: every block at its longest, every byte stuffed, the restart marker (or EOI)
JPEG_HD uint64_t jpeg_interval_max(int mcus) { return 2ull * (uint64_t)(mcus * kJpegMcuBlocks) * kJpegBlockMaxBytes + 2; }
JPEG_HD bool jpeg_shape_ok(int H, int W) { return H >= 1 && W >= 1 && H <= 65535 && W <= 65535; }
// the capacity that always suffices; 0: unsupported shape, or 2^31 and above
JPEG_HD uint64_t jpeg_bound(int H, int W)
{
    if (!jpeg_shape_ok(H, W)) return 0;
    const uint64_t nmcu = (uint64_t)((W + 15) / 16) * (uint64_t)((H + 15) / 16);
    const uint64_t full = nmcu / kJpegRestart, rest = nmcu % kJpegRestart;
    const uint64_t b = kJpegHeaderBytes + full * jpeg_interval_max(kJpegRestart) + (rest ? jpeg_interval_max((int)rest) : 0);
    return b >= (1ull << 31) ? 0 : b;
}

// ---- pixels ---------------------------------------------------------------------------------------------------------------
// the reference's to8b (render_4DGS.py:44): uint8(255 * clip(x, 0, 1)), the product in float32, truncated
JPEG_HD int jpeg_to8b(float x)
{
    const float c = !(x > 0.f) ? 0.f : (x > 1.f ? 1.f : x);
    return (int)(255.0f * c);
}
struct JpegRgb8Src {            // [H][row_stride] bytes, R G B interleaved
    const uint8_t* p;
    size_t row_stride;
    JPEG_HD void operator()(int y, int x, int& r, int& g, int& b) const
    {
        const uint8_t* q = p + (size_t)y * row_stride + 3 * (size_t)x;
        r = q[0]; g = q[1]; b = q[2];
    }
};
struct JpegChwSrc {             // the window at (y0, x0) of a [3][IH][IW] float image, through to8b
    const float* img;
    int IH, IW, y0, x0;
    JPEG_HD void operator()(int y, int x, int& r, int& g, int& b) const
    {
        const size_t plane = (size_t)IH * IW, o = (size_t)(y0 + y) * IW + (size_t)(x0 + x);
        r = jpeg_to8b(img[o]); g = jpeg_to8b(img[plane + o]); b = jpeg_to8b(img[2 * plane + o]);
    }
};

#define JPEG_FIX(x) ((int)((x) * 65536.0 + 0.5))
JPEG_HD int jpeg_luma(int r, int g, int b) { return (JPEG_FIX(0.299) * r + JPEG_FIX(0.587) * g + JPEG_FIX(0.114) * b + 32768) >> 16; }
JPEG_HD int jpeg_cb(int r, int g, int b)
{
    return (-JPEG_FIX(0.16874) * r - JPEG_FIX(0.33126) * g + JPEG_FIX(0.5) * b + (128 << 16) + 32767) >> 16;
}
JPEG_HD int jpeg_cr(int r, int g, int b)
{
    return (JPEG_FIX(0.5) * r - JPEG_FIX(0.41869) * g - JPEG_FIX(0.08131) * b + (128 << 16) + 32767) >> 16;
}

// ---- the transform --------------------------------------------------------------------------------------------------------
JPEG_HD int jpeg_descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }
// One pass of the IJG "islow" forward DCT over eight values at d[0], d[s], ..: the outputs 0 and 4 are (t10 +- t11) * 2^up when
// up >= 0 and descaled by -up otherwise; the others are descaled by `down`.
template <int S>
JPEG_HD void jpeg_dct_pass(int* d, int up, int down)
{
    const int t0 = d[0] + d[7 * S], t7 = d[0] - d[7 * S], t1 = d[S] + d[6 * S], t6 = d[S] - d[6 * S];
    const int t2 = d[2 * S] + d[5 * S], t5 = d[2 * S] - d[5 * S], t3 = d[3 * S] + d[4 * S], t4 = d[3 * S] - d[4 * S];
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    d[0] = up >= 0 ? (t10 + t11) * (1 << up) : jpeg_descale(t10 + t11, -up);
    d[4 * S] = up >= 0 ? (t10 - t11) * (1 << up) : jpeg_descale(t10 - t11, -up);
    int z1 = (t12 + t13) * 4433;
    d[2 * S] = jpeg_descale(z1 + t13 * 6270, down);
    d[6 * S] = jpeg_descale(z1 - t12 * 15137, down);
    z1 = t4 + t7;
    int z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
    const int z5 = (z3 + z4) * 9633;
    const int a4 = t4 * 2446, a5 = t5 * 16819, a6 = t6 * 25172, a7 = t7 * 12299;
    z1 *= -7373;
    z2 *= -20995;
    z3 = z3 * -16069 + z5;
    z4 = z4 * -3196 + z5;
    d[7 * S] = jpeg_descale(a4 + z1 + z3, down);
    d[5 * S] = jpeg_descale(a5 + z2 + z4, down);
    d[3 * S] = jpeg_descale(a6 + z2 + z3, down);
    d[S] = jpeg_descale(a7 + z1 + z4, down);
}
// sign(x) * ((|x| + (q8 >> 1)) / q8), q8 = 8 q: the transform's outputs carry a factor of 8
JPEG_HD int jpeg_quantise(int x, int q)
{
    const unsigned q8 = (unsigned)q << 3, a = (unsigned)(x < 0 ? -x : x);
    const int v = (int)((a + (q8 >> 1)) / q8);
    return x < 0 ? -v : v;
}

// ---- samples -------------------------------------------------------------------------------------------------------------
// The Y sample at (y, x) of the padded image, less 128: the pixels right of the image repeat column W - 1, those below it row H - 1.
template <class Src>
JPEG_HD int jpeg_y_sample(const Src& src, const JpegGeom& g, int y, int x)
{
    int r, gg, bb;
    src(y < g.H ? y : g.H - 1, x < g.W ? x : g.W - 1, r, gg, bb);
    return jpeg_luma(r, gg, bb) - 128;
}
// The chroma samples at (cy, cx) of the padded, averaged planes, less 128.  Columns are padded before the average (column W - 1
// again); rows only for an odd H (row H - 1 again) -- the chroma rows below ceil(H / 2) repeat the last AVERAGED row.  The bias of
// the average is 1, 2, 1, 2, .. along a row.
template <class Src>
JPEG_HD void jpeg_c_sample(const Src& src, const JpegGeom& g, int cy, int cx, int& cb, int& cr)
{
    const int ch = (g.H + 1) / 2;
    cy = cy < ch ? cy : ch - 1;
    const int ya = 2 * cy < g.H ? 2 * cy : g.H - 1, yb = 2 * cy + 1 < g.H ? 2 * cy + 1 : g.H - 1;
    const int xa = 2 * cx < g.W ? 2 * cx : g.W - 1, xb = 2 * cx + 1 < g.W ? 2 * cx + 1 : g.W - 1;
    int sb = 1 + (cx & 1), sr = sb;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        int r, gg, bb;
        src(k & 2 ? yb : ya, k & 1 ? xb : xa, r, gg, bb);
        sb += jpeg_cb(r, gg, bb);
        sr += jpeg_cr(r, gg, bb);
    }
    cb = (sb >> 2) - 128;
    cr = (sr >> 2) - 128;
}
// A Y block of an MCU outside the Y block grid is a dummy block: it is coded with the DC of the last block in front of it in the
// MCU that is inside the grid (block 0 always is) and no AC, and no pixels are read for it.  Returns that block, b itself if b is
// inside the grid.
JPEG_HD int jpeg_dummy_source(const JpegGeom& g, int mx, int my, int b)
{
    while (b > 0 && b < 4 && (2 * my + (b >> 1) >= g.ybh || 2 * mx + (b & 1) >= g.ybw)) b--;
    return b;
}

// Block b (0..3 Y, 4 Cb, 5 Cr) of the MCU (mx, my): 64 quantised coefficients in zigzag order.  (The serial form; the kernel spreads
// an MCU's samples, passes and coefficients over a wave and calls the same functions.)
template <class Src>
inline void jpeg_block(const Src& src, const JpegGeom& g, int mx, int my, int b, const JpegQuant& qt, int16_t* out)
{
    constexpr uint8_t zigzag[64] = JPEG_ZIGZAG_INIT;
    int d[64];
    const int sb = jpeg_dummy_source(g, mx, my, b);
    for (int i = 0; i < 64; i++) {
        if (b < 4) {
            d[i] = jpeg_y_sample(src, g, (2 * my + (sb >> 1)) * 8 + (i >> 3), (2 * mx + (sb & 1)) * 8 + (i & 7));
        } else {
            int cb, cr;
            jpeg_c_sample(src, g, my * 8 + (i >> 3), mx * 8 + (i & 7), cb, cr);
            d[i] = b == 4 ? cb : cr;
        }
    }
    for (int r = 0; r < 8; r++) jpeg_dct_pass<1>(d + 8 * r, 2, 11);
    for (int c = 0; c < 8; c++) jpeg_dct_pass<8>(d + c, -2, 15);
    const uint8_t* q = qt.q[b < 4 ? 0 : 1];
    for (int k = 0; k < 64; k++) out[k] = (int16_t)((sb != b && k) ? 0 : jpeg_quantise(d[zigzag[k]], q[k]));
}

// ---- tables and the header ------------------------------------------------------------------------------------------------
// libjpeg's quality scaling of the base tables, clamped to a baseline file's 1..255
JPEG_HD int jpeg_scale_q(int base, int Q)
{
    const int s = Q < 50 ? 5000 / Q : 200 - 2 * Q, v = (base * s + 50) / 100;
    return v < 1 ? 1 : (v > 255 ? 255 : v);
}
JPEG_HD void jpeg_scale_quant(int Q, const uint8_t base[2][64], JpegQuant* out)
{
    for (int t = 0; t < 2; t++)
        for (int k = 0; k < 64; k++) out->q[t][k] = (uint8_t)jpeg_scale_q(base[t][k], Q);
}
// SOI .. SOS into p [kJpegHeaderBytes]
JPEG_HD void jpeg_write_header(uint8_t* p, int H, int W, int Q, const uint8_t base[2][64], const JpegDht* dht)
{
    const uint8_t app0[20] = {0xFF, 0xD8, 0xFF, 0xE0, 0, 16, 'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0};
    for (int i = 0; i < 20; i++) *p++ = app0[i];
    for (int t = 0; t < 2; t++) {
        *p++ = 0xFF; *p++ = 0xDB; *p++ = 0; *p++ = 67; *p++ = (uint8_t)t;
        for (int k = 0; k < 64; k++) *p++ = (uint8_t)jpeg_scale_q(base[t][k], Q);
    }
    const uint8_t sof[19] = {0xFF, 0xC0, 0, 17, 8, (uint8_t)(H >> 8), (uint8_t)H, (uint8_t)(W >> 8), (uint8_t)W, 3,
                             1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1};
    for (int i = 0; i < 19; i++) *p++ = sof[i];
    for (int t = 0; t < 4; t++) {
        const int n = dht[t].n;
        *p++ = 0xFF; *p++ = 0xC4; *p++ = 0; *p++ = (uint8_t)(19 + n); *p++ = dht[t].tc_th;
        for (int k = 0; k < 16; k++) *p++ = dht[t].counts[k];
        for (int k = 0; k < n; k++) *p++ = dht[t].symbols[k];
    }
    const uint8_t tail[20] = {0xFF, 0xDD, 0, 4, 0, kJpegRestart, 0xFF, 0xDA, 0, 12, 3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0};
    for (int i = 0; i < 20; i++) *p++ = tail[i];
}

// ---- entropy coding -------------------------------------------------------------------------------------------------------
JPEG_HD int jpeg_nbits(int v) { return v ? 32 - __builtin_clz((unsigned)v) : 0; }     // v >= 0

// The symbols of one block (T.81 F.1.2): put(bits, n) receives every code with its value bits behind it, n <= 26.
// coef(k): coefficient k in zigzag order; pred: the DC of the component's previous block in the interval, 0 for the first;
// dc / ac: code | length << 16 per symbol.
template <class Get, class Sink>
JPEG_HD void jpeg_walk_block(const Get& coef, int pred, const uint32_t* dc, const uint32_t* ac, Sink& sink)
{
    int t = coef(0) - pred, t2 = t;
    if (t < 0) { t = -t; t2--; }
    int n = jpeg_nbits(t);
    uint32_t c = dc[n];
    sink.put(((c & 0xFFFFu) << n) | ((uint32_t)t2 & ((1u << n) - 1u)), (int)(c >> 16) + n);
    int run = 0;
    for (int k = 1; k < 64; k++) {
        t = coef(k);
        if (t == 0) { run++; continue; }
        while (run > 15) {
            sink.put(ac[0xF0] & 0xFFFFu, (int)(ac[0xF0] >> 16));
            run -= 16;
        }
        t2 = t;
        if (t < 0) { t = -t; t2--; }
        n = jpeg_nbits(t);
        c = ac[(run << 4) + n];
        sink.put(((c & 0xFFFFu) << n) | ((uint32_t)t2 & ((1u << n) - 1u)), (int)(c >> 16) + n);
        run = 0;
    }
    if (run > 0) sink.put(ac[0] & 0xFFFFu, (int)(ac[0] >> 16));
}
struct JpegCount {
    uint32_t bits;
    JPEG_HD void put(uint32_t, int n) { bits += (uint32_t)n; }
};
// Bits go into words that hold four bytes of the file each, the first byte in the most significant place: or_word(w, v) ORs v into
// word w of an image that starts out zero.
template <class Or>
struct JpegEmit {
    Or or_word;
    uint32_t pos;           // bits in front of the next one
    JPEG_HD void put(uint32_t v, int n)
    {
        const uint64_t x = (uint64_t)v << (64 - (int)(pos & 31u) - n);
        or_word(pos >> 5, (uint32_t)(x >> 32));
        if ((uint32_t)x) or_word((pos >> 5) + 1, (uint32_t)x);
        pos += (uint32_t)n;
    }
};
JPEG_HD uint8_t jpeg_img_byte(const uint32_t* img, uint32_t k) { return (uint8_t)(img[k >> 2] >> (24 - 8 * (k & 3u))); }
// index, within the interval's blocks, of the block whose DC predicts block j's; -1: the predictor is 0
JPEG_HD int jpeg_pred_block(int j)
{
    const int b = j % kJpegMcuBlocks;
    if (b >= 1 && b <= 3) return j - 1;
    if (j < kJpegMcuBlocks) return -1;
    return b == 0 ? j - 3 : j - kJpegMcuBlocks;
}

// ---- the host form --------------------------------------------------------------------------------------------------------
struct JpegPlainOr {
    uint32_t* img;
    void operator()(uint32_t w, uint32_t v) const { if (w < (uint32_t)kJpegImgWords) img[w] |= v; }
};
struct JpegPlainGet {
    const int16_t* p;
    int operator()(int k) const { return p[k]; }
};
// The whole file into out (capacity >= jpeg_bound); returns its length.
template <class Src>
inline uint32_t jpeg_host_encode(const Src& src, int H, int W, int Q, const uint8_t base[2][64], const JpegDht* dht, const uint32_t (*huff)[256], uint8_t* out)
{
    const JpegGeom g = jpeg_geom(H, W);
    JpegQuant qt;
    jpeg_scale_quant(Q, base, &qt);
    jpeg_write_header(out, H, W, Q, base, dht);
    uint8_t* p = out + kJpegHeaderBytes;
    uint32_t* img = (uint32_t*)malloc(sizeof(uint32_t) * kJpegImgWords);
    int16_t* co = (int16_t*)malloc(sizeof(int16_t) * 64 * kJpegIntervalBlocks);
    for (int i = 0; i < g.nint; i++) {
        const int m0 = i * kJpegRestart, nm = g.nmcu - m0 < kJpegRestart ? g.nmcu - m0 : kJpegRestart, nblk = nm * kJpegMcuBlocks;
        for (int j = 0; j < nblk; j++) {
            const int m = m0 + j / kJpegMcuBlocks;
            jpeg_block(src, g, m % g.mw, m / g.mw, j % kJpegMcuBlocks, qt, co + 64 * j);
        }
        memset(img, 0, sizeof(uint32_t) * kJpegImgWords);
        JpegEmit<JpegPlainOr> e = {{img}, 0};
        for (int j = 0; j < nblk; j++) {
            const int b = j % kJpegMcuBlocks, jp = jpeg_pred_block(j);
            const JpegPlainGet get = {co + 64 * j};
            jpeg_walk_block(get, jp < 0 ? 0 : co[64 * jp], huff[b < 4 ? JPEG_DC_LUMA : JPEG_DC_CHROMA],
                            huff[b < 4 ? JPEG_AC_LUMA : JPEG_AC_CHROMA], e);
        }
        const int pad = (int)((0u - e.pos) & 7u);
        if (pad) e.put((1u << pad) - 1u, pad);
        for (uint32_t k = 0; k < e.pos >> 3; k++) {
            const uint8_t v = jpeg_img_byte(img, k);
            *p++ = v;
            if (v == 0xFF) *p++ = 0;
        }
        *p++ = 0xFF;
        *p++ = i == g.nint - 1 ? 0xD9 : (uint8_t)(0xD0 + (i & 7));
    }
    free(co);
    free(img);
    return (uint32_t)(p - out);
}
