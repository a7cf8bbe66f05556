// A baseline JPEG file made on the device from 8-bit RGB or from the crop window of a rendered float image
// (render.AsyncVideoWriter, encoder="device": the frames of vid_result/<name>.avi).  The file's layout and the per-block coder are
// jpeg_dev.h's; this file is the parallel part.  Three launches on the caller's stream:
//   jpeg_transform_kernel  a wave per 16x16 MCU, staged in LDS: to8b (float input), colour conversion, chroma average, forward DCT
//                          (a lane per row, then per column, of the six blocks), quantisation; 64 int16 coefficients in zigzag
//                          order per block to scratch, dummy blocks included
//   jpeg_entropy_kernel    a wave per restart interval, a lane per block: the interval's coefficients into LDS, every lane prices
//                          its block (the DC predecessor is a neighbour's coefficient 0), a wave prefix sum gives the bit offsets,
//                          the lanes OR their codes into an LDS image of the interval, the image is padded with 1-bits and goes to
//                          the interval's staging area byte by byte with the stuffed zeros, the restart marker behind it
//   jpeg_compact_kernel    a workgroup per interval: staging -> out at the summed byte offsets; the first one writes the header,
//                          the last one EOI and *out_size
// No launch waits for another through memory: the order is the stream's.
#include "mom_common.h"
#include "jpeg_dev.h"

static const uint8_t h_jpeg_base[2][64] = JPEG_QUANT_INIT;
static const uint8_t h_jpeg_zigzag[64] = JPEG_ZIGZAG_INIT;
static const JpegDht h_jpeg_dht[4] = JPEG_DHT_INIT;
static const uint32_t h_jpeg_huff[4][256] = JPEG_HUFF_INIT;

namespace {
__device__ const uint8_t d_jpeg_base[2][64] = JPEG_QUANT_INIT;
__device__ const uint8_t d_jpeg_zigzag[64] = JPEG_ZIGZAG_INIT;
__device__ const JpegDht d_jpeg_dht[4] = JPEG_DHT_INIT;
__device__ const uint32_t d_jpeg_huff[4][256] = JPEG_HUFF_INIT;

constexpr int kTransformThreads = 256;
constexpr int kTransformWaves = kTransformThreads / 64;
constexpr int kBlkStride = 8 * 9;
constexpr int kCompactThreads = 256;

struct JpegScratch {
    int16_t* coef;          // [blocks][64]
    uint32_t* len;          // [nint] bytes of the interval's piece, its marker included
    uint8_t* staging;       // [nint][stride]
    size_t stride;
};

size_t jpeg_scratch_view(char* base, const JpegGeom& g, JpegScratch* v)
{
    const size_t blocks = (size_t)g.nmcu * kJpegMcuBlocks;
    const size_t stride = (size_t)((jpeg_interval_max(kJpegRestart) + 16 + 15) & ~(uint64_t)15);
    size_t off = 0;
    const size_t o_coef = off; off = mom_align_up(off + blocks * 64 * sizeof(int16_t));
    const size_t o_len = off; off = mom_align_up(off + (size_t)g.nint * 4);
    const size_t o_stage = off; off = mom_align_up(off + (size_t)g.nint * stride);
    if (v) {
        v->coef = (int16_t*)(base + o_coef);
        v->len = (uint32_t*)(base + o_len);
        v->staging = (uint8_t*)(base + o_stage);
        v->stride = stride;
    }
    return off + MOM_ALIGN;
}

// A wave per MCU, four MCUs per workgroup.  `blk` holds the MCU's six blocks, a row of eight at a stride of nine words so that
// neither pass meets a bank twice: the lanes fill it (four Y samples each, then one averaged chroma pair each), 48 lanes run a row
// pass each, then a column pass each, and every lane quantises six coefficients -- lane k the coefficient k of every block, so a
// block's 128 bytes leave in one store.  A wave's LDS is its own, so the waves only meet at the barriers.
template <class Src>
__global__ void __launch_bounds__(kTransformThreads) jpeg_transform_kernel(Src src, JpegGeom g, int Q, int16_t* __restrict__ coef)
{
    __shared__ int blk_s[kTransformWaves][kJpegMcuBlocks][kBlkStride];
    __shared__ uint8_t q_s[2][64];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    if (tid < 128) q_s[tid >> 6][tid & 63] = (uint8_t)jpeg_scale_q(d_jpeg_base[tid >> 6][tid & 63], Q);
    const int m = blockIdx.x * kTransformWaves + wave;
    const bool live = m < g.nmcu;
    const int my = live ? m / g.mw : 0, mx = live ? m - my * g.mw : 0;
    int (*blk)[kBlkStride] = blk_s[wave];
    if (live) {
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int p = lane + 64 * j, y = p >> 4, x = p & 15, b = (y >> 3) * 2 + (x >> 3);
            // a dummy block's samples are never used: no pixels are read for it
            if (jpeg_dummy_source(g, mx, my, b) == b) blk[b][(y & 7) * 9 + (x & 7)] = jpeg_y_sample(src, g, my * 16 + y, mx * 16 + x);
        }
        int cb, cr;
        jpeg_c_sample(src, g, my * 8 + (lane >> 3), mx * 8 + (lane & 7), cb, cr);
        blk[4][(lane >> 3) * 9 + (lane & 7)] = cb;
        blk[5][(lane >> 3) * 9 + (lane & 7)] = cr;
    }
    __syncthreads();
    if (live && lane < 8 * kJpegMcuBlocks) jpeg_dct_pass<1>(&blk[lane >> 3][(lane & 7) * 9], 2, 11);
    __syncthreads();
    if (live && lane < 8 * kJpegMcuBlocks) jpeg_dct_pass<9>(&blk[lane >> 3][lane & 7], -2, 15);
    __syncthreads();
    if (!live) return;
    const int at = d_jpeg_zigzag[lane], pos = (at >> 3) * 9 + (at & 7);
    int16_t* dst = coef + (size_t)m * kJpegMcuBlocks * 64 + lane;
#pragma unroll
    for (int b = 0; b < kJpegMcuBlocks; b++) {
        const int sb = jpeg_dummy_source(g, mx, my, b);
        const int v = (sb != b && lane) ? 0 : jpeg_quantise(blk[sb][pos], q_s[b < 4 ? 0 : 1][lane]);
        dst[64 * b] = (int16_t)v;
    }
}

struct LdsCoef {
    const int16_t* p;
    __device__ __forceinline__ int operator()(int k) const { return p[k]; }
};
struct LdsOr {
    uint32_t* img;
    __device__ __forceinline__ void operator()(uint32_t w, uint32_t v) const
    {
        if (w < (uint32_t)kJpegImgWords) atomicOr(&img[w], v);
    }
};
// inclusive prefix sum over the wave's lanes
__device__ __forceinline__ uint32_t wave_scan(uint32_t v, int lane)
{
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = __shfl_up(v, d);
        if (lane >= d) v += o;
    }
    return v;
}

__global__ void __launch_bounds__(64) jpeg_entropy_kernel(int nmcu, int nint, const int16_t* __restrict__ coef,
                                                          uint8_t* __restrict__ staging, size_t stride, uint32_t* __restrict__ len)
{
    __shared__ __attribute__((aligned(4))) int16_t co[kJpegIntervalBlocks * kJpegCoefStride];
    __shared__ uint32_t img[kJpegImgWords];
    __shared__ uint32_t huff[4][256];
    const int i = blockIdx.x, lane = threadIdx.x;
    const int m0 = i * kJpegRestart, nblk = min(kJpegRestart, nmcu - m0) * kJpegMcuBlocks;
    const uint32_t* src = (const uint32_t*)(coef + (size_t)m0 * kJpegMcuBlocks * 64);
    uint32_t* co32 = (uint32_t*)co;
    for (int w = lane; w < nblk * 32; w += 64) co32[(w >> 5) * (kJpegCoefStride / 2) + (w & 31)] = src[w];
    for (int w = lane; w < kJpegImgWords; w += 64) img[w] = 0u;
    for (int w = lane; w < 4 * 256; w += 64) huff[w >> 8][w & 255] = d_jpeg_huff[w >> 8][w & 255];
    __syncthreads();

    const bool live = lane < nblk;
    const int b = lane % kJpegMcuBlocks, jp = jpeg_pred_block(lane);
    const LdsCoef get = {co + (live ? lane : 0) * kJpegCoefStride};
    const int pred = (live && jp >= 0) ? co[jp * kJpegCoefStride] : 0;
    const uint32_t* dc = huff[b < 4 ? JPEG_DC_LUMA : JPEG_DC_CHROMA];
    const uint32_t* ac = huff[b < 4 ? JPEG_AC_LUMA : JPEG_AC_CHROMA];
    JpegCount cost = {0};
    if (live) jpeg_walk_block(get, pred, dc, ac, cost);
    const uint32_t incl = wave_scan(cost.bits, lane);
    const uint32_t total = __shfl(incl, 63);
    if (live) {
        JpegEmit<LdsOr> e = {{img}, incl - cost.bits};
        jpeg_walk_block(get, pred, dc, ac, e);
    }
    const uint32_t pad = (0u - total) & 7u, nbytes = (total + pad) >> 3;
    if (lane == 0 && pad) {
        JpegEmit<LdsOr> e = {{img}, total};
        e.put((1u << pad) - 1u, (int)pad);
    }
    __syncthreads();

    uint8_t* dst = staging + (size_t)i * stride;
    uint32_t extra = 0;             // stuffed zeros so far
    for (uint32_t k0 = 0; k0 < nbytes; k0 += 64) {
        const uint32_t k = k0 + lane;
        const bool valid = k < nbytes && (k >> 2) < (uint32_t)kJpegImgWords;
        const uint8_t v = valid ? jpeg_img_byte(img, k) : 0;
        const bool ff = valid && v == 0xFF;
        const unsigned long long mask = __ballot(ff);
        const uint32_t at = k + extra + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
        if (valid && at < stride) dst[at] = v;
        if (ff && at + 1 < stride) dst[at + 1] = 0;
        extra += (uint32_t)__popcll(mask);
    }
    if (lane == 0) {
        // never above jpeg_interval_max, the marker (or the last interval's EOI) included: the bound is the sum of those
        const uint32_t most = (uint32_t)jpeg_interval_max(nblk / kJpegMcuBlocks) - 2;
        uint32_t n = min(nbytes + extra, most);
        if (i != nint - 1) {
            dst[n] = 0xFF;
            dst[n + 1] = (uint8_t)(0xD0 + (i & 7));
            n += 2;
        }
        len[i] = n;
    }
}

// grid (nint): the interval's piece from its staging area to out + kJpegHeaderBytes + the lengths in front of it.  Destination words
// are aligned; a source word pair is shifted into place.
__global__ void __launch_bounds__(kCompactThreads) jpeg_compact_kernel(int H, int W, int nint, int Q, const uint32_t* __restrict__ len,
                                                                       const uint8_t* __restrict__ staging, size_t stride,
                                                                       uint8_t* __restrict__ out, uint32_t* __restrict__ out_size)
{
    __shared__ uint32_t off_s;
    __shared__ uint8_t hdr[kJpegHeaderBytes];
    const int i = blockIdx.x, tid = threadIdx.x;
    if (tid == 0) off_s = 0;
    __syncthreads();
    uint32_t part = 0;
    for (int j = tid; j < i; j += kCompactThreads) part += len[j];
    for (int d = 32; d >= 1; d >>= 1) part += __shfl_xor(part, d);
    if ((tid & 63) == 0 && part) atomicAdd(&off_s, part);
    if (i == 0 && tid == 0) jpeg_write_header(hdr, H, W, Q, d_jpeg_base, d_jpeg_dht);
    __syncthreads();
    if (i == 0)
        for (int k = tid; k < kJpegHeaderBytes; k += kCompactThreads) out[k] = hdr[k];
    const uint32_t n = len[i];
    const uint8_t* src = staging + (size_t)i * stride;
    uint8_t* dst = out + kJpegHeaderBytes + off_s;
    uint32_t head = (uint32_t)((4 - ((uintptr_t)dst & 3)) & 3);
    if (head > n) head = n;
    const uint32_t nw = (n - head) >> 2, tail0 = head + 4 * nw;
    if ((uint32_t)tid < head) dst[tid] = src[tid];
    const uint32_t* src32 = (const uint32_t*)src;
    uint32_t* dst32 = (uint32_t*)(dst + head);
    const uint32_t sh = 8 * (head & 3);
    for (uint32_t w = tid; w < nw; w += kCompactThreads) {
        const uint32_t k = (head >> 2) + w;
        const uint32_t lo = src32[k];
        dst32[w] = sh ? (lo >> sh) | (src32[k + 1] << (32 - sh)) : lo;
    }
    if (tail0 + tid < n) dst[tail0 + tid] = src[tail0 + tid];
    if (i == nint - 1 && tid == 0) {
        dst[n] = 0xFF;
        dst[n + 1] = 0xD9;
        *out_size = kJpegHeaderBytes + off_s + n + 2;
    }
}

template <class Src>
int jpeg_launch(const Src& src, int H, int W, int Q, uint8_t* out, uint32_t* out_size, void* scratch, hipStream_t st)
{
    const JpegGeom g = jpeg_geom(H, W);
    JpegScratch v;
    jpeg_scratch_view(mom_align_ptr(scratch), g, &v);
    hipLaunchKernelGGL(jpeg_transform_kernel<Src>, dim3((g.nmcu + kTransformWaves - 1) / kTransformWaves), dim3(kTransformThreads), 0,
                       st, src, g, Q, v.coef);
    hipLaunchKernelGGL(jpeg_entropy_kernel, dim3(g.nint), dim3(64), 0, st, g.nmcu, g.nint, v.coef, v.staging, v.stride, v.len);
    hipLaunchKernelGGL(jpeg_compact_kernel, dim3(g.nint), dim3(kCompactThreads), 0, st, H, W, g.nint, Q, v.len, v.staging, v.stride, out,
                       out_size);
    return hipGetLastError() == hipSuccess ? MOM_OK : MOM_ELAUNCH;
}
}  // namespace

extern "C" size_t mom_jpeg_bound(int H, int W) { return (size_t)jpeg_bound(H, W); }

extern "C" size_t mom_jpeg_scratch_bytes(int H, int W)
{
    if (!jpeg_bound(H, W)) return 0;
    return jpeg_scratch_view(nullptr, jpeg_geom(H, W), nullptr);
}

extern "C" int mom_jpeg_encode(int H, int W, const uint8_t* rgb8, size_t row_stride, int Q, uint8_t* out, size_t capacity,
                               uint32_t* out_size, void* scratch, mom_stream_t stream)
{
    const uint64_t bound = jpeg_bound(H, W);
    if (!bound || Q < 1 || Q > 100 || !rgb8 || !out || !out_size || !scratch || capacity < bound || row_stride < 3 * (size_t)W)
        return MOM_EINVAL;
    const JpegRgb8Src src = {rgb8, row_stride};
    return jpeg_launch(src, H, W, Q, out, out_size, scratch, (hipStream_t)stream);
}

extern "C" int mom_jpeg_encode_chw(int IH, int IW, int y0, int x0, int H, int W, const float* image, int Q, uint8_t* out,
                                   size_t capacity, uint32_t* out_size, void* scratch, mom_stream_t stream)
{
    const uint64_t bound = jpeg_bound(H, W);
    if (!bound || Q < 1 || Q > 100 || !image || !out || !out_size || !scratch || capacity < bound) return MOM_EINVAL;
    if (IH < 1 || IW < 1 || y0 < 0 || x0 < 0 || (int64_t)y0 + H > IH || (int64_t)x0 + W > IW) return MOM_EINVAL;
    const JpegChwSrc src = {image, IH, IW, y0, x0};
    return jpeg_launch(src, H, W, Q, out, out_size, scratch, (hipStream_t)stream);
}

extern "C" int mom_jpeg_encode_host(int H, int W, const uint8_t* rgb8, size_t row_stride, int Q, uint8_t* out, size_t capacity,
                                    uint32_t* out_size)
{
    const uint64_t bound = jpeg_bound(H, W);
    if (!bound || Q < 1 || Q > 100 || !rgb8 || !out || !out_size || capacity < bound || row_stride < 3 * (size_t)W) return MOM_EINVAL;
    const JpegRgb8Src src = {rgb8, row_stride};
    *out_size = jpeg_host_encode(src, H, W, Q, h_jpeg_base, h_jpeg_dht, h_jpeg_huff, out);
    return MOM_OK;
}

extern "C" int mom_jpeg_tables(int Q, uint8_t* quant, uint8_t* dht_counts, uint8_t* dht_symbols, int* dht_nsymbols, int* restart_interval)
{
    if (Q < 1 || Q > 100 || !quant || !dht_counts || !dht_symbols || !dht_nsymbols || !restart_interval) return MOM_EINVAL;
    JpegQuant qt;
    jpeg_scale_quant(Q, h_jpeg_base, &qt);
    for (int t = 0; t < 2; t++)
        for (int k = 0; k < 64; k++) quant[64 * t + h_jpeg_zigzag[k]] = qt.q[t][k];
    memset(dht_symbols, 0, 4 * JPEG_DHT_MAX_SYMBOLS);
    for (int t = 0; t < 4; t++) {
        memcpy(dht_counts + 16 * t, h_jpeg_dht[t].counts, 16);
        memcpy(dht_symbols + JPEG_DHT_MAX_SYMBOLS * t, h_jpeg_dht[t].symbols, h_jpeg_dht[t].n);
        dht_nsymbols[t] = h_jpeg_dht[t].n;
    }
    *restart_interval = kJpegRestart;
    return MOM_OK;
}
