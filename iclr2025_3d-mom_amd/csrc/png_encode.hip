// The zlib stream of a PNG's IDAT, made on the device from the [H,W,C] bytes mom_image_to_rgb8 writes (render.AsyncPNGWriter,
// encoder="device"): row filters, deflate with constant Huffman tables and run-length matches, Adler-32.  The stream's layout and
// the per-chunk coder are png_dev.h's; this file is the parallel part.  Four launches on the caller's stream:
//   png_plan_kernel     a workgroup per segment: the rows' filters, every chunk priced under the four tables (kept for the next
//                       kernel), the chunks' Adler sums, then the segment's form and exact length
//   png_scan_kernel     one wave: exclusive scan of the lengths, the Adler-32 of the image, 78 01, the final block, *out_size
//   png_encode_kernel   a workgroup per segment: the chunks' bit offsets from a wave prefix sum of the kept prices, every lane of wave 0
//                       packs its chunk and ORs the words into an LDS image of the tile, the image goes to the segment's staging
//                       area (fixed stride, word-aligned) in coalesced stores; a partial last word is carried into the next tile
// A workgroup is four waves: a tile is the 64 chunks wave 0's lanes walk, and all four waves fetch and filter its bytes, kPngBatch
// rows of loads in flight per thread -- with one workgroup per compute unit nothing else hides the loads' latency.
//   png_compact_kernel  staging -> out at the scanned byte offsets, aligned words on the destination side
// No launch waits for another through memory: the order is the stream's.
#include "mom_common.h"
#include "png_dev.h"

static const PngTable h_png_tables[PNG_TABLE_COUNT] = PNG_TABLES_INIT;

namespace {
__device__ const PngTable d_png_tables[PNG_TABLE_COUNT] = PNG_TABLES_INIT;

// words of a tile's image: the tile's chunks at PNG_TABLE_MAX_BITS a byte (a match costs less per byte than that: png_tables.py),
// a table header, the carried word, the end of block and the empty stored block
constexpr int kImgWords = kPngTileBytes * PNG_TABLE_MAX_BITS / 32 + PNG_TABLE_HDR_WORDS + 8;

struct PngPlan {
    int32_t form;       // table, or kPngFormStored
    uint32_t len;       // bytes of the segment's piece
    uint32_t a, b;      // Adler sums of the segment's filtered bytes (png_dev.h), modulo 65521
};

struct PngScratch {
    PngPlan* plan;          // [S]
    uint32_t* off;          // [S] byte offset of the piece behind the zlib header
    uint8_t* filt;          // [H]
    uint4* chunk_bits;      // [S][cps] price of every chunk under the four tables
    uint8_t* staging;       // [S][stride]
    size_t stride;
    int S, cps;
};

size_t png_scratch_view(char* base, int C, int H, int W, PngScratch* v)
{
    const uint64_t seg_full = (uint64_t)kPngRowsPerSegment * (1 + (uint64_t)W * C);
    const size_t S = (size_t)png_segments(H), cps = (size_t)((seg_full + kPngChunk - 1) / kPngChunk);
    const size_t stride = (size_t)((png_stored_len(seg_full) + 8 + 15) & ~(uint64_t)15);
    size_t off = 0;
    const size_t o_plan = off; off = mom_align_up(off + S * sizeof(PngPlan));
    const size_t o_off = off; off = mom_align_up(off + S * 4);
    const size_t o_filt = off; off = mom_align_up(off + (size_t)H);
    const size_t o_bits = off; off = mom_align_up(off + S * cps * sizeof(uint4));
    const size_t o_stage = off; off = mom_align_up(off + S * stride);
    if (v) {
        v->plan = (PngPlan*)(base + o_plan);
        v->off = (uint32_t*)(base + o_off);
        v->filt = (uint8_t*)(base + o_filt);
        v->chunk_bits = (uint4*)(base + o_bits);
        v->staging = (uint8_t*)(base + o_stage);
        v->stride = stride;
        v->S = (int)S;
        v->cps = (int)cps;
    }
    return off + MOM_ALIGN;
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t v)
{
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    return v;
}
__device__ __forceinline__ uint64_t wave_sum64(uint64_t v)
{
    for (int d = 32; d >= 1; d >>= 1) v += (uint64_t)__shfl_xor((unsigned long long)v, d);
    return v;
}
// inclusive prefix sum over the wave's lanes
__device__ __forceinline__ uint32_t wave_scan(uint32_t v, int lane)
{
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = __shfl_up(v, d);
        if (lane >= d) v += o;
    }
    return v;
}

// Filtered byte k of the segment whose first row is y0 (filters: four bits per row).  No state from one byte to the next, and the
// row's filter-type byte is a select, not a branch: the caller batches these so that a thread has several rows of loads in flight.
__device__ __forceinline__ uint8_t png_segment_byte(const uint8_t* __restrict__ raw, int WC, int C, int y0, uint32_t filters, int k)
{
    const int rb = WC + 1;
    int r = 0;
#pragma unroll
    for (int i = 1; i < kPngRowsPerSegment; i++) r += k >= i * rb;
    const int col = k - r * rb, f = (int)((filters >> (4 * r)) & 15u);
    const uint8_t v = png_filtered(raw, WC, C, y0 + r, max(col - 1, 0), f);
    return col == 0 ? (uint8_t)f : v;
}
// fn(j, byte) for the filtered bytes k0 + j, j = tid, tid + kPngThreads, ... < nbytes (>= 1), kPngBatch of them loaded before the
// first is handed on: a lone workgroup per compute unit hides the loads' latency only by having many of them in flight
template <class Fn>
__device__ __forceinline__ void png_filtered_bytes(const uint8_t* __restrict__ raw, int WC, int C, int y0, uint32_t filters, int k0,
                                                   int nbytes, int tid, const Fn& fn)
{
    for (int j0 = tid; j0 < nbytes; j0 += kPngThreads * kPngBatch) {
        uint8_t v[kPngBatch];
#pragma unroll
        for (int u = 0; u < kPngBatch; u++) v[u] = png_segment_byte(raw, WC, C, y0, filters, k0 + min(j0 + u * kPngThreads, nbytes - 1));
#pragma unroll
        for (int u = 0; u < kPngBatch; u++)
            if (j0 + u * kPngThreads < nbytes) fn(j0 + u * kPngThreads, v[u]);
    }
}
// ... into the tile in LDS, chunk by chunk at kPngChunkStride
__device__ __forceinline__ void png_load_tile(uint8_t* tile, const uint8_t* __restrict__ raw, int WC, int C, int y0, uint32_t filters,
                                              int k0, int nbytes, int tid)
{
    png_filtered_bytes(raw, WC, C, y0, filters, k0, nbytes, tid, [tile](int j, uint8_t v) {
        const int ch = j / kPngChunk;
        tile[ch * kPngChunkStride + (j - ch * kPngChunk)] = v;
    });
}
struct LdsChunk {               // a lane's chunk in the tile, word-aligned
    const uint8_t* p;
    __device__ __forceinline__ uint32_t operator()(int w) const { return ((const uint32_t*)p)[w]; }
};
struct LdsOr {
    uint32_t* img;
    __device__ __forceinline__ void operator()(uint32_t w, uint32_t v) const
    {
        if (w < (uint32_t)kImgWords) atomicOr(&img[w], v);
    }
};
// Adler sums of a chunk in LDS (word-aligned): a full chunk word by word, so that the reads are independent of each other
__device__ __forceinline__ void png_chunk_adler(const uint8_t* p, int len, uint32_t& s1, uint32_t& s2)
{
    s1 = s2 = 0;
    if (len == kPngChunk) {
        const uint32_t* w = (const uint32_t*)p;
#pragma unroll 8
        for (int i = 0; i < kPngChunk / 4; i++) {
            const uint32_t x = w[i], b0 = x & 255u, b1 = (x >> 8) & 255u, b2 = (x >> 16) & 255u, b3 = x >> 24;
            s2 += 4 * s1 + 4 * b0 + 3 * b1 + 2 * b2 + b3;
            s1 += b0 + b1 + b2 + b3;
        }
    } else {
        for (int i = 0; i < len; i++) { s1 += p[i]; s2 += s1; }
    }
}

// Workgroups of four waves: all of them choose the filters and fill the tile (memory latency), wave 0's lanes walk the chunks.
__global__ void __launch_bounds__(kPngThreads) png_plan_kernel(int C, int H, int W, const uint8_t* __restrict__ raw,
                                                              PngPlan* __restrict__ plan, uint8_t* __restrict__ filt,
                                                              uint4* __restrict__ chunk_bits, int cps)
{
    __shared__ __attribute__((aligned(16))) uint8_t tile[kPngLanes * kPngChunkStride];
    __shared__ uint32_t lens4[PNG_TABLE_NLIT];
    __shared__ uint32_t dlens4[PNG_TABLE_NDIST];
    __shared__ uint32_t fcost[kPngRowsPerSegment][3];
    const int s = blockIdx.x, tid = threadIdx.x, lane = tid & (kPngLanes - 1);
    const int WC = W * C, rb = WC + 1, y0 = s * kPngRowsPerSegment, rows = min(kPngRowsPerSegment, H - y0), n = rows * rb;
    for (int i = tid; i < PNG_TABLE_NLIT; i += kPngThreads) lens4[i] = png_lens4(d_png_tables, i);
    if (tid < PNG_TABLE_NDIST) dlens4[tid] = png_dlens4(d_png_tables, tid);
    if (tid < kPngRowsPerSegment * 3) fcost[tid / 3][tid % 3] = 0;
    __syncthreads();

    for (int r = 0; r < rows; r++) {
        uint32_t s1 = 0, s2 = 0, s4 = 0;
#pragma unroll 4
        for (int x = tid; x < WC; x += kPngThreads) png_filter_costs(raw, WC, C, y0 + r, x, s1, s2, s4);
        s1 = wave_sum(s1);
        s2 = wave_sum(s2);
        s4 = wave_sum(s4);
        if (lane == 0) {
            atomicAdd(&fcost[r][0], s1);
            atomicAdd(&fcost[r][1], s2);
            atomicAdd(&fcost[r][2], s4);
        }
    }
    __syncthreads();
    uint32_t filters = 0;
    for (int r = 0; r < rows; r++) {
        const int f = png_choose_filter(fcost[r][0], fcost[r][1], fcost[r][2]);
        filters |= (uint32_t)f << (4 * r);
        if (tid == 0) filt[y0 + r] = (uint8_t)f;
    }

    const int nchunks = (n + kPngChunk - 1) / kPngChunk;
    uint64_t bits0 = 0, bits1 = 0, bits2 = 0, bits3 = 0;
    uint32_t A = 0, B = 0;
    for (int c0 = 0; c0 < nchunks; c0 += kPngLanes) {
        const int k0 = c0 * kPngChunk;
        __syncthreads();
        png_load_tile(tile, raw, WC, C, y0, filters, k0, min(n - k0, kPngTileBytes), tid);
        __syncthreads();
        const int ch = c0 + tid;
        if (tid < kPngLanes && ch < nchunks) {
            const int len = min(kPngChunk, n - ch * kPngChunk);
            const LdsChunk get = {tile + tid * kPngChunkStride};
            PngCost cost = {lens4, dlens4, 0, 0, 0};
            png_walk_chunk(get, len, C, cost);
            const uint4 b4 = make_uint4(cost.bits(0), cost.bits(1), cost.bits(2), cost.bits(3));
            chunk_bits[(size_t)s * cps + ch] = b4;
            bits0 += b4.x; bits1 += b4.y; bits2 += b4.z; bits3 += b4.w;
            uint32_t s1, s2;
            png_chunk_adler(get.p, len, s1, s2);
            A = (A + s1) % kPngAdlerMod;
            B = (B + png_adler_weighted(s1, s2, (uint64_t)(n - (ch * kPngChunk + len)))) % kPngAdlerMod;
        }
    }
    if (tid < kPngLanes) {
        const uint64_t bits[PNG_TABLE_COUNT] = {wave_sum64(bits0), wave_sum64(bits1), wave_sum64(bits2), wave_sum64(bits3)};
        A = wave_sum(A) % kPngAdlerMod;
        B = wave_sum(B) % kPngAdlerMod;
        if (tid == 0) {
            PngPlan p;
            png_choose_form(d_png_tables, bits, (uint64_t)n, p.form, p.len);
            p.a = A;
            p.b = B;
            plan[s] = p;
        }
    }
}

__global__ void __launch_bounds__(kPngLanes) png_scan_kernel(int S, int H, int rb, const PngPlan* __restrict__ plan,
                                                            uint32_t* __restrict__ off, uint8_t* __restrict__ out,
                                                            uint32_t* __restrict__ out_size)
{
    const int lane = threadIdx.x;
    const uint64_t n_total = (uint64_t)H * rb, seg_full = (uint64_t)kPngRowsPerSegment * rb;
    uint32_t running = 0, A = 0, B = 0;
    for (int s0 = 0; s0 < S; s0 += kPngLanes) {
        const int s = s0 + lane;
        PngPlan p = {0, 0, 0, 0};
        if (s < S) p = plan[s];
        const uint32_t incl = wave_scan(p.len, lane);
        if (s < S) {
            off[s] = running + incl - p.len;
            A = (A + p.a) % kPngAdlerMod;
            B = (B + png_adler_weighted(p.a, p.b, s == S - 1 ? 0 : n_total - (uint64_t)(s + 1) * seg_full)) % kPngAdlerMod;
        }
        running += __shfl(incl, kPngLanes - 1);
    }
    A = wave_sum(A) % kPngAdlerMod;
    B = wave_sum(B) % kPngAdlerMod;
    if (lane == 0) {
        const uint32_t a = (1 + A) % kPngAdlerMod, b = (uint32_t)((n_total % kPngAdlerMod + B) % kPngAdlerMod);
        uint8_t* t = out + 2 + running;
        out[0] = 0x78;
        out[1] = 0x01;
        t[0] = 0x03;
        t[1] = 0x00;
        t[2] = (uint8_t)(b >> 8);
        t[3] = (uint8_t)b;
        t[4] = (uint8_t)(a >> 8);
        t[5] = (uint8_t)a;
        *out_size = running + 8;
    }
}

__global__ void __launch_bounds__(kPngThreads) png_encode_kernel(int C, int H, int W, const uint8_t* __restrict__ raw,
                                                                const PngPlan* __restrict__ plan, const uint8_t* __restrict__ filt,
                                                                const uint4* __restrict__ chunk_bits, int cps,
                                                                uint8_t* __restrict__ staging, size_t stride)
{
    __shared__ __attribute__((aligned(16))) uint8_t tile[kPngLanes * kPngChunkStride];
    __shared__ uint32_t img[kImgWords];
    __shared__ uint32_t tab[PNG_TABLE_NLIT + PNG_TABLE_NDIST];
    const int s = blockIdx.x, tid = threadIdx.x, lane = tid & (kPngLanes - 1);
    const int WC = W * C, rb = WC + 1, y0 = s * kPngRowsPerSegment, rows = min(kPngRowsPerSegment, H - y0), n = rows * rb;
    const PngPlan p = plan[s];
    uint32_t filters = 0;
    for (int r = 0; r < rows; r++) filters |= (uint32_t)filt[y0 + r] << (4 * r);
    uint8_t* dst = staging + (size_t)s * stride;

    if (p.form < 0 || p.form >= PNG_TABLE_COUNT) {              // stored
        const int nblk = (n + kPngStoredMax - 1) / kPngStoredMax;
        for (int blk = tid; blk < nblk; blk += kPngThreads) png_stored_header(dst, (uint64_t)n, (uint64_t)blk);
        png_filtered_bytes(raw, WC, C, y0, filters, 0, n, tid, [dst](int k, uint8_t v) { dst[png_stored_pos((uint64_t)k)] = v; });
        return;
    }

    const PngTable& T = d_png_tables[p.form];
    for (int i = tid; i < PNG_TABLE_NLIT + PNG_TABLE_NDIST; i += kPngThreads)
        tab[i] = i < PNG_TABLE_NLIT ? T.lit[i] : T.dist[i - PNG_TABLE_NLIT];
    for (int i = tid; i < kImgWords; i += kPngThreads) img[i] = i < PNG_TABLE_HDR_WORDS ? T.hdr[i] : 0u;
    const uint32_t eob = T.lit[256];
    const int sel = p.form;
    const int nchunks = (n + kPngChunk - 1) / kPngChunk;
    const uint32_t stride_words = (uint32_t)(stride / 4);
    uint32_t* dst32 = (uint32_t*)dst;
    uint64_t base = T.hdr_bits;         // bits of the segment so far
    uint32_t wout = 0;                  // words of the segment already in staging: the image starts at bit 32 * wout
    const LdsOr or_word = {img};
    for (int c0 = 0; c0 < nchunks; c0 += kPngLanes) {
        const int k0 = c0 * kPngChunk;
        __syncthreads();
        png_load_tile(tile, raw, WC, C, y0, filters, k0, min(n - k0, kPngTileBytes), tid);
        __syncthreads();
        const int ch = c0 + lane;           // every wave scans the chunks' prices, so that all threads know where the tile ends
        uint32_t bits = 0;
        if (ch < nchunks) {
            const uint4 b4 = chunk_bits[(size_t)s * cps + ch];
            bits = sel == 0 ? b4.x : sel == 1 ? b4.y : sel == 2 ? b4.z : b4.w;
            if (ch == nchunks - 1) bits += eob >> 16;
        }
        const uint32_t incl = wave_scan(bits, lane);
        if (tid < kPngLanes && ch < nchunks) {
            const LdsChunk get = {tile + lane * kPngChunkStride};
            PngEmit<LdsOr> e(tab, tab + PNG_TABLE_NLIT, or_word, base - 32ull * wout + (incl - bits));
            png_walk_chunk(get, min(kPngChunk, n - ch * kPngChunk), C, e);
            if (ch == nchunks - 1) e.code(eob);
            e.flush();
        }
        base += __shfl(incl, kPngLanes - 1);
        __syncthreads();
        if (c0 + kPngLanes >= nchunks) {
            // 000 and the pad are zeros already; LEN = 0000, NLEN = FFFF
            const uint32_t rel = (uint32_t)(((base + 3 + 7) >> 3) - 4ull * wout) + 2;
            if (tid < 2) or_word((rel + tid) >> 2, 0xFFu << (8 * ((rel + tid) & 3)));
            __syncthreads();
            const uint32_t nw = (p.len - 4 * wout + 3) >> 2;
            for (uint32_t i = tid; i < nw && i < (uint32_t)kImgWords; i += kPngThreads)
                if (wout + i < stride_words) dst32[wout + i] = img[i];
        } else {
            const uint32_t nfull = (uint32_t)(base >> 5) - wout;
            for (uint32_t i = tid; i < nfull && i < (uint32_t)kImgWords; i += kPngThreads)
                if (wout + i < stride_words) dst32[wout + i] = img[i];
            const uint32_t carry = nfull < (uint32_t)kImgWords ? img[nfull] : 0u;
            __syncthreads();
            for (uint32_t i = tid; i <= nfull && i < (uint32_t)kImgWords; i += kPngThreads) img[i] = i == 0 ? carry : 0u;
            wout += nfull;
        }
    }
}

// grid (S): the segment's piece from its staging area to out + 2 + off[s].  Destination words are aligned; a source word pair is
// shifted into place.
__global__ void __launch_bounds__(256) png_compact_kernel(const PngPlan* __restrict__ plan, const uint32_t* __restrict__ off,
                                                          const uint8_t* __restrict__ staging, size_t stride,
                                                          uint8_t* __restrict__ out)
{
    const int s = blockIdx.x, tid = threadIdx.x;
    const uint32_t len = plan[s].len;
    const uint8_t* src = staging + (size_t)s * stride;
    uint8_t* dst = out + 2 + off[s];
    uint32_t head = (uint32_t)((4 - ((uintptr_t)dst & 3)) & 3);
    if (head > len) head = len;
    const uint32_t nw = (len - head) >> 2, tail0 = head + 4 * nw;
    if ((uint32_t)tid < head) dst[tid] = src[tid];
    const uint32_t* src32 = (const uint32_t*)src;
    uint32_t* dst32 = (uint32_t*)(dst + head);
    const uint32_t sh = 8 * (head & 3);
    for (uint32_t w = tid; w < nw; w += 256) {
        const uint32_t i = (head >> 2) + w;
        const uint32_t lo = src32[i];
        dst32[w] = sh ? (lo >> sh) | (src32[i + 1] << (32 - sh)) : lo;
    }
    if (tail0 + tid < len) dst[tail0 + tid] = src[tail0 + tid];
}
}  // namespace

extern "C" size_t mom_png_bound(int C, int H, int W) { return (size_t)png_bound(C, H, W); }

extern "C" size_t mom_png_scratch_bytes(int C, int H, int W)
{
    if (!png_bound(C, H, W)) return 0;
    return png_scratch_view(nullptr, C, H, W, nullptr);
}

extern "C" int mom_png_encode(int C, int H, int W, const uint8_t* rgb8, uint8_t* out, size_t capacity, uint32_t* out_size,
                              void* scratch, mom_stream_t stream)
{
    const uint64_t bound = png_bound(C, H, W);
    if (!bound || !rgb8 || !out || !out_size || !scratch || capacity < bound) return MOM_EINVAL;
    PngScratch v;
    png_scratch_view(mom_align_ptr(scratch), C, H, W, &v);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(png_plan_kernel, dim3(v.S), dim3(kPngThreads), 0, st, C, H, W, rgb8, v.plan, v.filt, v.chunk_bits, v.cps);
    hipLaunchKernelGGL(png_scan_kernel, dim3(1), dim3(kPngLanes), 0, st, v.S, H, 1 + W * C, v.plan, v.off, out, out_size);
    hipLaunchKernelGGL(png_encode_kernel, dim3(v.S), dim3(kPngThreads), 0, st, C, H, W, rgb8, v.plan, v.filt, v.chunk_bits, v.cps,
                       v.staging, v.stride);
    hipLaunchKernelGGL(png_compact_kernel, dim3(v.S), dim3(256), 0, st, v.plan, v.off, v.staging, v.stride, out);
    return hipGetLastError() == hipSuccess ? MOM_OK : MOM_ELAUNCH;
}

extern "C" int mom_png_encode_host(int C, int H, int W, const uint8_t* rgb8, uint8_t* out, size_t capacity, uint32_t* out_size)
{
    const uint64_t bound = png_bound(C, H, W);
    if (!bound || !rgb8 || !out || !out_size || capacity < bound) return MOM_EINVAL;
    return png_host_encode(h_png_tables, C, H, W, rgb8, out, out_size) == 0 ? MOM_OK : MOM_ECAPACITY;
}

extern "C" int mom_png_tables(int index, uint8_t* litlen, uint8_t* dist, uint8_t* header, int header_capacity, int* header_bits)
{
    if (index == -1) return PNG_TABLE_COUNT;
    if (index < 0 || index >= PNG_TABLE_COUNT || !litlen || !dist || !header || !header_bits) return MOM_EINVAL;
    const PngTable& T = h_png_tables[index];
    if (header_capacity < (int)((T.hdr_bits + 7) / 8)) return MOM_EINVAL;
    memset(litlen, 0, 288);
    memset(dist, 0, 32);
    for (int s = 0; s < PNG_TABLE_NLIT; s++) litlen[s] = (uint8_t)(T.lit[s] >> 16);
    for (int d = 0; d < PNG_TABLE_NDIST; d++) dist[d] = (uint8_t)(T.dist[d] >> 16);
    if (index == 0) {                   // the fixed code is defined over 288 and 32 symbols (RFC 1951 3.2.6); two and 28 are never sent
        litlen[286] = litlen[287] = 8;
        for (int d = 0; d < 32; d++) dist[d] = 5;
    }
    for (uint32_t k = 0; k < (T.hdr_bits + 7) / 8; k++) header[k] = (uint8_t)(T.hdr[k >> 2] >> (8 * (k & 3)));
    *header_bits = (int)T.hdr_bits;
    return PNG_TABLE_COUNT;
}
