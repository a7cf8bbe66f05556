// The coder of the device PNG encoder (png_encode.hip), as code that compiles for the host and for the device: PNG row filters,
// the choice of symbols of one lane's chunk (literals and run-length matches), their bit packing, the Adler-32 partial sums and
// their combination, the choice between the Huffman-coded and the stored form of a segment.  The kernels call these per lane;
// png_host_encode() below walks the same segments and chunks serially, in the kernels' order and with the same arithmetic, so its
// stream is the kernels' byte for byte -- which lets a machine without a GPU check the stream the kernels must reproduce.
//
// The stream (zlib, RFC 1950 / 1951):  78 01 | per segment of kPngRowsPerSegment rows: one block, BFINAL = 0 | 03 00 | Adler-32.
// A segment's block is the smaller of
//   coded:  <table header> <symbols of chunk 0> <symbols of chunk 1> ... <end of block> 000 <pad to a byte> 00 00 FF FF
//           (the empty stored block makes every segment's piece end on a byte, so pieces concatenate by byte offsets), the table
//           being the cheapest of png_tables.h's for this segment: every chunk is priced under all of them,
//   stored: ceil(n / 65535) stored blocks, 00 LEN NLEN <bytes>, already byte-aligned.
// A chunk is kPngChunk consecutive filtered bytes of the segment (rows are not chunk borders).  Matches never leave their chunk:
// a run of bytes that repeat the byte 1 back or, for C > 1, C back (the pixel size) becomes a match of its length if that is 3 or
// more, at most 258; everything else is literals (png_walk_chunk).
#pragma once
#include <stdint.h>
#include <stddef.h>
#include <stdlib.h>
#include <string.h>
#include "png_tables.h"

#if defined(__HIPCC__)
#define PNG_HD __host__ __device__ inline
#else
#define PNG_HD inline
#endif

constexpr int kPngRowsPerSegment = 4;
constexpr int kPngChunk = 288;                          // bytes of one lane's chunk: above the longest match, 72 words
constexpr int kPngLanes = 64;                           // the lanes of one wave walk a segment's chunks ...
constexpr int kPngThreads = 256;                        // ... in a workgroup of four waves that fetch and filter its bytes
constexpr int kPngBatch = 8;                            // loads a thread keeps in flight while it does
constexpr int kPngTileBytes = kPngChunk * kPngLanes;    // what a wave codes between two flushes of its LDS image
constexpr int kPngChunkStride = kPngChunk + 4;          // a chunk's stride in LDS: 73 words, odd, so the lanes' reads spread over the banks
constexpr uint32_t kPngAdlerMod = 65521;
constexpr int kPngStoredMax = 65535;                    // bytes of one stored block
constexpr int kPngFormStored = PNG_TABLE_COUNT;         // PngPlan::form: 0 .. PNG_TABLE_COUNT-1 is a table
static_assert(PNG_TABLE_COUNT == 4, "PngCost packs the chunk's price under four tables into two words");

struct PngTable {
    uint32_t lit[PNG_TABLE_NLIT];       // literal / length symbols: the code, bit-reversed, | bits << 16
    uint32_t dist[PNG_TABLE_NDIST];     // distance codes 0..3 (distances 1..4, no extra bits)
    uint32_t hdr_bits;                  // block header: BFINAL = 0, BTYPE and the dynamic tables
    uint32_t hdr[PNG_TABLE_HDR_WORDS];
};

// ---- shapes ---------------------------------------------------------------------------------------------------------------
PNG_HD uint64_t png_stored_len(uint64_t n) { return n + 5 * ((n + kPngStoredMax - 1) / kPngStoredMax); }
PNG_HD uint32_t png_coded_len(uint64_t bits) { return (uint32_t)((bits + 3 + 7) >> 3) + 4; }
PNG_HD int png_segments(int H) { return (H + kPngRowsPerSegment - 1) / kPngRowsPerSegment; }
PNG_HD bool png_shape_ok(int C, int H, int W) { return (C == 1 || C == 3 || C == 4) && H >= 1 && W >= 1; }
// 2 (zlib header) + every segment stored + 2 (the final empty block) + 4 (Adler-32); 0: unsupported shape or 2^31 and above
PNG_HD uint64_t png_bound(int C, int H, int W)
{
    if (!png_shape_ok(C, H, W)) return 0;
    const uint64_t rb = 1 + (uint64_t)W * C, full = (uint64_t)H / kPngRowsPerSegment, rest = (uint64_t)H % kPngRowsPerSegment;
    const uint64_t b = 2 + full * png_stored_len(kPngRowsPerSegment * rb) + (rest ? png_stored_len(rest * rb) : 0) + 2 + 4;
    return b >= (1ull << 31) ? 0 : b;
}

// ---- filters --------------------------------------------------------------------------------------------------------------
PNG_HD int png_abs(int v) { return v < 0 ? -v : v; }
PNG_HD int png_paeth(int a, int b, int c)
{
    const int p = a + b - c, pa = png_abs(p - a), pb = png_abs(p - b), pc = png_abs(p - c);
    return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}
// raw [H][WC]; byte x of row y and its neighbours: a left (one pixel), b above, c above left; 0 outside the image.  The three loads
// are unconditional, from addresses clamped into the image, and the zeros are selected afterwards: a branch around a load would keep
// the device from having the loads of several bytes in flight at once.
PNG_HD void png_neighbours(const uint8_t* raw, int WC, int C, int y, int x, int& v, int& a, int& b, int& c)
{
    const uint8_t* p = raw + (size_t)y * WC + x;
    const bool left = x >= C, up = y > 0;
    const ptrdiff_t da = left ? -(ptrdiff_t)C : 0, db = up ? -(ptrdiff_t)WC : 0;
    const int la = p[da], lb = p[db], lc = p[da + db];
    v = p[0];
    a = left ? la : 0;
    b = up ? lb : 0;
    c = (left && up) ? lc : 0;
}
PNG_HD uint8_t png_filtered(const uint8_t* raw, int WC, int C, int y, int x, int f)
{
    int v, a, b, c;
    png_neighbours(raw, WC, C, y, x, v, a, b, c);
    // masks, not a choice: with Paeth behind a branch the device compiler moves c's load there, and the loads no longer batch
    return (uint8_t)(v - ((a & -(int)(f == 1)) | (b & -(int)(f == 2)) | (png_paeth(a, b, c) & -(int)(f == 4))));
}
// the sums of |signed residual| of Sub, Up and Paeth grow by byte x's
PNG_HD void png_filter_costs(const uint8_t* raw, int WC, int C, int y, int x, uint32_t& s1, uint32_t& s2, uint32_t& s4)
{
    int v, a, b, c;
    png_neighbours(raw, WC, C, y, x, v, a, b, c);
    s1 += png_abs((int8_t)(uint8_t)(v - a));
    s2 += png_abs((int8_t)(uint8_t)(v - b));
    s4 += png_abs((int8_t)(uint8_t)(v - png_paeth(a, b, c)));
}
PNG_HD int png_choose_filter(uint32_t s1, uint32_t s2, uint32_t s4)
{
    int f = 1;
    uint32_t best = s1;
    if (s2 < best) { best = s2; f = 2; }
    if (s4 < best) f = 4;
    return f;
}

// ---- symbols of one chunk -------------------------------------------------------------------------------------------------
// length 3..258 -> symbol 257..285, its extra bits and their value (RFC 1951 3.2.5)
PNG_HD void png_length_symbol(int L, int& sym, int& nb, int& ev)
{
    const int l = L - 3;
    if (L == 258) { sym = 285; nb = 0; ev = 0; }
    else if (l < 8) { sym = 257 + l; nb = 0; ev = 0; }
    else {
        nb = 29 - __builtin_clz((unsigned)l);
        sym = 261 + 4 * nb + ((l >> nb) & 3);
        ev = l & ((1 << nb) - 1);
    }
}

// word(w): bytes 4w .. 4w+3 of the chunk, little-endian (bytes past len are ignored).  sink.lit(byte) / sink.match(length, distance)
// in stream order.  One byte per step and no inner loop, so that the lanes of a wave, each in its own chunk, stay in step: a
// candidate run is carried as state -- `pend` bytes, equal so far to the bytes 1 back (alive1) and / or C back (aliveC) -- and
// settled when the byte at hand continues neither or the run is 258 long: 3 and more become a match (distance 1 if both are
// alive), one or two become literals.
template <class Word, class Sink>
PNG_HD void png_walk_chunk(const Word& word, int len, int C, Sink& sink)
{
    int pend = 0;
    bool alive1 = false, aliveC = false;
    uint32_t p1 = 0, p2 = 0, p3 = 0, p4 = 0, w = 0;         // the four bytes before the one at hand
    for (int i = 0; i <= len; i++) {
        if ((i & 3) == 0 && i < len) w = word(i >> 2);
        const uint32_t b = w & 255u;
        w >>= 8;
        const bool last = i == len;                         // one step behind the chunk settles what is pending
        const bool e1 = !last && i >= 1 && b == p1;
        const bool eC = !last && C > 1 && i >= C && b == (C == 3 ? p3 : p4);
        bool fresh = !last;
        if (pend > 0) {
            const bool n1 = alive1 && e1, nC = aliveC && eC;
            if ((n1 || nC) && pend < 258) {
                alive1 = n1;
                aliveC = nC;
                pend++;
                fresh = false;
            } else {
                if (pend >= 3) sink.match(pend, alive1 ? 1 : C);
                else {
                    if (pend == 2) sink.lit((int)p2);
                    sink.lit((int)p1);
                }
                pend = 0;
            }
        }
        if (fresh) {
            if (e1 || eC) { alive1 = e1; aliveC = eC; pend = 1; }
            else sink.lit((int)b);
        }
        p4 = p3; p3 = p2; p2 = p1; p1 = b;
    }
}

// The price in bits of a chunk under all four tables at once.  lens4[s] holds the four code lengths of symbol s, a byte each; the
// sums run in 16-bit fields (a chunk costs at most kPngChunk * PNG_TABLE_MAX_BITS < 65536 bits): tables 0 and 2 in lo, 1 and 3 in hi.
struct PngCost {
    const uint32_t* lens4;
    const uint32_t* dlens4;
    uint32_t lo, hi, extra;
    PNG_HD void add(uint32_t p) { lo += p & 0x00FF00FFu; hi += (p >> 8) & 0x00FF00FFu; }
    PNG_HD void lit(int b) { add(lens4[b]); }
    PNG_HD void match(int L, int dist)
    {
        int sym, nb, ev;
        png_length_symbol(L, sym, nb, ev);
        add(lens4[sym]);
        add(dlens4[dist - 1]);
        extra += nb;
    }
    PNG_HD uint32_t bits(int t) const { return ((t & 1 ? hi : lo) >> (t & 2 ? 16 : 0) & 0xFFFFu) + extra; }
};
PNG_HD uint32_t png_lens4(const PngTable* tabs, int s)
{
    return (tabs[0].lit[s] >> 16) | (tabs[1].lit[s] >> 16) << 8 | (tabs[2].lit[s] >> 16) << 16 | (tabs[3].lit[s] >> 16) << 24;
}
PNG_HD uint32_t png_dlens4(const PngTable* tabs, int d)
{
    return (tabs[0].dist[d] >> 16) | (tabs[1].dist[d] >> 16) << 8 | (tabs[2].dist[d] >> 16) << 16 | (tabs[3].dist[d] >> 16) << 24;
}

// Bit packing of one chunk: words of the stream, least-significant bit first, OR-ed into an image of zeros at a bit offset.
// or_word(w, v): image word w |= v -- an LDS atomic on the device, where neighbouring chunks share their border words.
template <class Or>
struct PngEmit {
    const uint32_t* lit_tab;
    const uint32_t* dist_tab;
    const Or& or_word;
    uint64_t acc;
    int n;
    uint32_t w;
    PNG_HD PngEmit(const uint32_t* lit_, const uint32_t* dist_, const Or& o, uint64_t bit_offset)
        : lit_tab(lit_), dist_tab(dist_), or_word(o), acc(0), n((int)(bit_offset & 31)), w((uint32_t)(bit_offset >> 5)) {}
    PNG_HD void put(uint32_t v, int nb)
    {
        acc |= (uint64_t)v << n;
        n += nb;
        if (n >= 32) { or_word(w++, (uint32_t)acc); acc >>= 32; n -= 32; }
    }
    PNG_HD void code(uint32_t e) { put(e & 0xFFFFu, (int)(e >> 16)); }
    PNG_HD void lit(int b) { code(lit_tab[b]); }
    PNG_HD void match(int L, int d)
    {
        int sym, nb, ev;
        png_length_symbol(L, sym, nb, ev);
        code(lit_tab[sym]);
        if (nb) put((uint32_t)ev, nb);
        code(dist_tab[d - 1]);
    }
    PNG_HD void flush() { if (n > 0) or_word(w, (uint32_t)acc); }
};

// ---- Adler-32 -------------------------------------------------------------------------------------------------------------
// A block of len bytes d[i] has the partial sums A = sum d[i], B = sum (len - i) d[i]; behind a prefix whose state is (a, b) the
// state becomes (a + A, b + len a + B).  Blocks X then Y are one block with A = A_X + A_Y, B = B_X + B_Y + len_Y A_X, so the sums
// of a run of blocks are  A = sum A_k,  B = sum (B_k + A_k * (bytes behind block k)): plain sums, taken modulo 65521 at every step
// (a chunk's own sums stay below 2^25, products go through 64 bits).
PNG_HD uint32_t png_adler_weighted(uint32_t A, uint32_t B, uint64_t bytes_behind)
{
    return (uint32_t)((B % kPngAdlerMod + (uint64_t)(A % kPngAdlerMod) * (bytes_behind % kPngAdlerMod)) % kPngAdlerMod);
}

// ---- form of a segment ----------------------------------------------------------------------------------------------------
// bits[t]: the segment's chunks priced under table t (without header and end of block); n: its filtered bytes
PNG_HD void png_choose_form(const PngTable* tabs, const uint64_t* bits, uint64_t n, int& form, uint32_t& len)
{
    form = kPngFormStored;
    len = (uint32_t)png_stored_len(n);
    for (int t = 0; t < PNG_TABLE_COUNT; t++) {
        const uint32_t l = png_coded_len(tabs[t].hdr_bits + bits[t] + (tabs[t].lit[256] >> 16));
        if (l < len) { len = l; form = t; }
    }
}
// the stored form's byte k of the segment lands at
PNG_HD uint64_t png_stored_pos(uint64_t k) { return k + 5 * (k / kPngStoredMax + 1); }
PNG_HD void png_stored_header(uint8_t* dst, uint64_t n, uint64_t blk)
{
    const uint64_t left = n - blk * kPngStoredMax;
    const uint32_t len = (uint32_t)(left < kPngStoredMax ? left : kPngStoredMax);
    uint8_t* p = dst + blk * (kPngStoredMax + 5);
    p[0] = 0;
    p[1] = (uint8_t)len;
    p[2] = (uint8_t)(len >> 8);
    p[3] = (uint8_t)~len;
    p[4] = (uint8_t)(~len >> 8);
}

// ---- the whole stream on the host -------------------------------------------------------------------------------------------
// 0, or -1 when the two work buffers could not be allocated.  The caller has validated shape, pointers and capacity.
inline int png_host_encode(const PngTable* tabs, int C, int H, int W, const uint8_t* raw, uint8_t* out, uint32_t* out_size)
{
    const int WC = W * C, rb = WC + 1, S = png_segments(H);
    const uint64_t seg_full = (uint64_t)kPngRowsPerSegment * rb, n_total = (uint64_t)H * rb;
    uint8_t* seg = (uint8_t*)malloc(seg_full + 4);              // + 4: the walk reads whole words
    uint32_t* img = (uint32_t*)malloc(png_stored_len(seg_full) + 16);
    uint32_t lens4[PNG_TABLE_NLIT], dlens4[PNG_TABLE_NDIST];
    if (!seg || !img) { free(seg); free(img); return -1; }
    for (int s = 0; s < PNG_TABLE_NLIT; s++) lens4[s] = png_lens4(tabs, s);
    for (int d = 0; d < PNG_TABLE_NDIST; d++) dlens4[d] = png_dlens4(tabs, d);
    size_t pos = 0;
    out[pos++] = 0x78;
    out[pos++] = 0x01;
    uint32_t a = 1, b = (uint32_t)(n_total % kPngAdlerMod);            // the prefix "1" weighs on every byte
    for (int s = 0; s < S; s++) {
        const int y0 = s * kPngRowsPerSegment, rows = H - y0 < kPngRowsPerSegment ? H - y0 : kPngRowsPerSegment;
        const uint64_t n = (uint64_t)rows * rb;
        for (int r = 0; r < rows; r++) {
            uint32_t s1 = 0, s2 = 0, s4 = 0;
            for (int x = 0; x < WC; x++) png_filter_costs(raw, WC, C, y0 + r, x, s1, s2, s4);
            const int f = png_choose_filter(s1, s2, s4);
            uint8_t* row = seg + (size_t)r * rb;
            row[0] = (uint8_t)f;
            for (int x = 0; x < WC; x++) row[1 + x] = png_filtered(raw, WC, C, y0 + r, x, f);
        }
        const uint64_t nchunks = (n + kPngChunk - 1) / kPngChunk;
        uint64_t bits[PNG_TABLE_COUNT] = {0, 0, 0, 0};
        uint32_t A = 0, B = 0;
        for (uint64_t ch = 0; ch < nchunks; ch++) {
            const uint8_t* p = seg + ch * kPngChunk;
            const int len = (int)(n - ch * kPngChunk < (uint64_t)kPngChunk ? n - ch * kPngChunk : kPngChunk);
            PngCost cost = {lens4, dlens4, 0, 0, 0};
            png_walk_chunk([p](int i) { uint32_t v; memcpy(&v, p + 4 * i, 4); return v; }, len, C, cost);
            for (int t = 0; t < PNG_TABLE_COUNT; t++) bits[t] += cost.bits(t);
            uint32_t s1 = 0, s2 = 0;
            for (int i = 0; i < len; i++) { s1 += p[i]; s2 += s1; }
            A = (A + s1) % kPngAdlerMod;
            B = (B + png_adler_weighted(s1, s2, n - (ch * kPngChunk + len))) % kPngAdlerMod;
        }
        const uint64_t behind = s == S - 1 ? 0 : n_total - (uint64_t)(s + 1) * seg_full;
        a = (a + A) % kPngAdlerMod;
        b = (b + png_adler_weighted(A, B, behind)) % kPngAdlerMod;
        int form;
        uint32_t plen;
        png_choose_form(tabs, bits, n, form, plen);
        uint8_t* dst = out + pos;
        if (form == kPngFormStored) {
            for (uint64_t blk = 0; blk * kPngStoredMax < n; blk++) png_stored_header(dst, n, blk);
            for (uint64_t k = 0; k < n; k++) dst[png_stored_pos(k)] = seg[k];
        } else {
            const PngTable& T = tabs[form];
            memset(img, 0, ((size_t)plen + 7) & ~(size_t)3);
            for (int i = 0; i < PNG_TABLE_HDR_WORDS && 32u * i < T.hdr_bits; i++) img[i] = T.hdr[i];
            uint64_t base = T.hdr_bits;
            auto or_word = [img](uint32_t w, uint32_t v) { img[w] |= v; };
            for (uint64_t ch = 0; ch < nchunks; ch++) {
                const uint8_t* p = seg + ch * kPngChunk;
                const int len = (int)(n - ch * kPngChunk < (uint64_t)kPngChunk ? n - ch * kPngChunk : kPngChunk);
                PngEmit<decltype(or_word)> e(T.lit, T.dist, or_word, base);
                png_walk_chunk([p](int i) { uint32_t v; memcpy(&v, p + 4 * i, 4); return v; }, len, C, e);
                if (ch == nchunks - 1) e.code(T.lit[256]);
                e.flush();
                base = ((uint64_t)e.w << 5) + e.n;
            }
            const uint64_t tail = (base + 3 + 7) >> 3;                // 000, pad to a byte: LEN = 0 and NLEN = FFFF follow
            for (uint64_t k = 0; k < tail; k++) dst[k] = (uint8_t)(img[k >> 2] >> (8 * (k & 3)));
            dst[tail] = 0;
            dst[tail + 1] = 0;
            dst[tail + 2] = 0xFF;
            dst[tail + 3] = 0xFF;
            if (tail + 4 != plen) { free(seg); free(img); return -2; }     // the price and the packing disagree: never
        }
        pos += plen;
    }
    out[pos++] = 0x03;
    out[pos++] = 0x00;
    out[pos++] = (uint8_t)(b >> 8);
    out[pos++] = (uint8_t)b;
    out[pos++] = (uint8_t)(a >> 8);
    out[pos++] = (uint8_t)a;
    *out_size = (uint32_t)pos;
    free(seg);
    free(img);
    return 0;
}
