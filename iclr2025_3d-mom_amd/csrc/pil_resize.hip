// PIL's 8-bit bicubic resize (Image.resize(size, BICUBIC) of an "L" or "RGB" image), byte for byte, on the device.
//
// PIL resamples one axis at a time with integer arithmetic on coefficients it computes in double: per output index a window
// [xmin, xmin + n) of the input and n weights, normalised, then rounded to 22 fractional bits; a sample is
// clamp((2^21 + sum byte * k) >> 22, 0, 255).  The horizontal pass runs first and is rounded to bytes, the vertical pass runs on
// those bytes; an axis whose size does not change is skipped.  The coefficient tables are made on the host (mom_pil_resize_coeffs,
// this file, compiled without FMA contraction) and uploaded once per (in, out) by the caller; the kernels do the integer part.
//
// Two launches, not one: a vertical window is as tall as the scale asks (128 -> 5 rows has 105 taps), so one workgroup holding the
// horizontal result of its whole window in LDS would either redo the horizontal pass for every overlapping window or be limited in
// tap count.  The intermediate [N][H][pitch] bytes (pitch: OW C rounded up to 16) goes through memory instead -- 1.5 MB at
// 1024^2 -> 512^2, which stays in the L2 / Infinity Cache between the launches -- and its aligned rows are what lets the vertical
// pass read whole dwords with no staging at all.
//
//   hpass  one workgroup = 256 output pixels of one row.  The input span of those pixels is staged in LDS with aligned 16-byte
//          loads (groups that stick out of the buffer are read element by element), in pieces of 4096 pixels when it is longer, the
//          integer sums carrying over the pieces.  A lane produces the C bytes of one pixel into an LDS row, and the row leaves
//          through dwords.  The float form (to8b) stages (uint8)(x * 255.0f) of aligned float4 loads.
//   vpass  one workgroup = 512 byte columns of one output row.  Channels do not matter vertically: a lane owns four adjacent byte
//          columns, reads one aligned dword of each tap row and keeps four sums; the row again leaves through LDS and dwords,
//          because an output row of OW C bytes starts at any alignment.
//   copy   the staging and the store of hpass with nothing in between: the result when no axis changes, and the float -> byte
//          conversion into the intermediate when only the vertical axis does.
#include <math.h>
#include <string.h>
#include <vector>
#include "mom_common.h"

namespace {
constexpr int kPrecisionBits = 32 - 8 - 2;       // PIL's PRECISION_BITS
constexpr int kHThreads = 256;                   // hpass: output pixels per workgroup
constexpr int kChunkPx = 4096;                   // hpass: input pixels staged at a time
constexpr int kStageBytes = kChunkPx * 3 + 32;   // the staged piece and the bytes in front of it down to the 16-byte boundary
constexpr int kVThreads = 128;                   // vpass: dwords of one output row per workgroup
constexpr int kCopyBytes = 4096;                 // copy: bytes per workgroup

// ---- the coefficients (host) ---------------------------------------------------------------------------------------------
double bicubic(double x)
{
    const double a = -0.5;
    if (x < 0.0) x = -x;
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
    if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
    return 0.0;
}

int pil_ksize(int in, int out)
{
    double fs = (double)in / out;
    if (fs < 1.0) fs = 1.0;
    const double k = ceil(2.0 * fs) * 2 + 1;
    return k < 2147483647.0 ? (int)k : 0;
}

// bounds [out][2] = (xmin, n), kk [out][ksize], zero behind n.  The filter's argument is the product with 1 / fs, as PIL writes it.
void pil_coeffs(int in, int out, int ksize, int32_t* bounds, int32_t* kk)
{
    const double scale = (double)in / out;
    const double fs = scale < 1.0 ? 1.0 : scale;
    const double support = 2.0 * fs, ss = 1.0 / fs;
    std::vector<double> w((size_t)ksize);
    for (int xx = 0; xx < out; xx++) {
        const double center = (xx + 0.5) * scale;
        int xmin = (int)(center - support + 0.5);
        if (xmin < 0) xmin = 0;
        int xmax = (int)(center + support + 0.5);
        if (xmax > in) xmax = in;
        const int n = xmax - xmin;
        double ww = 0.0;
        for (int x = 0; x < n; x++) {
            w[x] = bicubic((x + xmin - center + 0.5) * ss);
            ww += w[x];
        }
        int32_t* k = kk + (size_t)xx * ksize;
        for (int x = 0; x < ksize; x++) {
            double v = x < n ? w[x] : 0.0;
            if (x < n && ww != 0.0) v /= ww;
            k[x] = v < 0 ? (int)(-0.5 + v * (1 << kPrecisionBits)) : (int)(0.5 + v * (1 << kPrecisionBits));
        }
        bounds[2 * xx] = xmin;
        bounds[2 * xx + 1] = n;
    }
}

__host__ __device__ inline uint8_t clip8(int s)
{
    s >>= kPrecisionBits;
    return (uint8_t)(s < 0 ? 0 : (s > 255 ? 255 : s));
}

// one axis on the host: `lines` lines of `in` samples of C bytes, `step` bytes between samples of a line, `line` between lines
void host_axis(const uint8_t* src, uint8_t* dst, int lines, int in, int out, int C, size_t s_step, size_t s_line, size_t d_step,
               size_t d_line, const int32_t* bounds, const int32_t* kk, int ksize)
{
    for (int l = 0; l < lines; l++)
        for (int xx = 0; xx < out; xx++) {
            const int xmin = bounds[2 * xx], n = bounds[2 * xx + 1];
            const int32_t* k = kk + (size_t)xx * ksize;
            for (int c = 0; c < C; c++) {
                int s = 1 << (kPrecisionBits - 1);
                for (int x = 0; x < n; x++) s += src[l * s_line + (size_t)(xmin + x) * s_step + c] * k[x];
                dst[l * d_line + xx * d_step + c] = clip8(s);
            }
        }
}

// ---- device ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t to8b(float x)
{
    // the float32 product, clamped while it is a float (a NaN gives 0), then truncated: inside (-1, 256) the clamp changes nothing
    return (uint32_t)(int)fminf(fmaxf(x * 255.0f, 0.0f), 255.0f);
}

// Source traits: a group is what one lane loads at once -- 16 bytes, aligned -- and the bytes it leaves in LDS.
template <typename T> struct Src;
template <> struct Src<uint8_t> {
    static constexpr int G = 16;                // elements per group = LDS bytes per group
    static __device__ __forceinline__ unsigned misalign(const uint8_t* p) { return (unsigned)((uintptr_t)p & 15); }
    static __device__ __forceinline__ void load(const uint8_t* p, uint8_t* lds) { *(uint4*)lds = *(const uint4*)p; }
    static __device__ __forceinline__ uint8_t one(const uint8_t* p) { return *p; }
};
template <> struct Src<float> {
    static constexpr int G = 4;
    static __device__ __forceinline__ unsigned misalign(const float* p) { return (unsigned)(((uintptr_t)p >> 2) & 3); }
    static __device__ __forceinline__ void load(const float* p, uint8_t* lds)
    {
        const float4 v = *(const float4*)p;
        *(uint32_t*)lds = to8b(v.x) | (to8b(v.y) << 8) | (to8b(v.z) << 16) | (to8b(v.w) << 24);
    }
    static __device__ __forceinline__ uint8_t one(const float* p) { return (uint8_t)to8b(*p); }
};

// Stages elements [e0, e0 + len) of src[0 .. total) as bytes: lds[d + i] = byte of element e0 + i, d returned (< G).  Whole aligned
// groups are loaded, so up to G - 1 elements on either side come along; a group that is not wholly inside the buffer is read element
// by element, the ones outside not at all.  lds: 16-byte aligned, (G - 1 + len) rounded up to G bytes.  No barrier inside.
template <typename T>
__device__ __forceinline__ int stage_span(uint8_t* lds, const T* src, long long total, long long e0, int len, int tid, int nthreads)
{
    constexpr int G = Src<T>::G;
    const long long pos = e0 + Src<T>::misalign(src);          // in elements from the aligned address in front of src
    const int d = (int)(pos & (G - 1));
    const long long g0 = e0 - d;                                // element of lds[0]; may lie in front of the buffer
    const int groups = (d + len + G - 1) / G;
    for (int j = tid; j < groups; j += nthreads) {
        const long long e = g0 + (long long)j * G;
        uint8_t* l = lds + j * G;
        if (e >= 0 && e + G <= total) {
            Src<T>::load(src + e, l);
        } else {
            for (int i = 0; i < G; i++)
                if (e + i >= 0 && e + i < total) l[i] = Src<T>::one(src + e + i);
        }
    }
    return d;
}

// lds[off .. off + len) -> dst[0 .. len): dwords where dst is aligned, bytes in front and behind.  Nothing outside [0, len) is written.
__device__ __forceinline__ void store_run(uint8_t* dst, const uint8_t* lds, int off, int len, int tid, int nthreads)
{
    const int head = min(len, (int)((4 - ((uintptr_t)dst & 3)) & 3));
    const int body = (len - head) >> 2;
    const int tail0 = head + 4 * body;
    uint32_t* d32 = (uint32_t*)(dst + head);
    const uint8_t* s = lds + off + head;
    if (((off + head) & 3) == 0) {
        for (int j = tid; j < body; j += nthreads) d32[j] = ((const uint32_t*)s)[j];
    } else {
        for (int j = tid; j < body; j += nthreads)
            d32[j] = (uint32_t)s[4 * j] | ((uint32_t)s[4 * j + 1] << 8) | ((uint32_t)s[4 * j + 2] << 16) | ((uint32_t)s[4 * j + 3] << 24);
    }
    if (tid < head) dst[tid] = lds[off + tid];
    if (tid < len - tail0) dst[tail0 + tid] = lds[off + tail0 + tid];
}

// Horizontal pass.  src [rows][W][C] elements (total of them), dst: row r at dst + r * d_pitch, OW * C bytes each.
// Workgroup b: row b / tiles, output pixels (b % tiles) * 256 ...
template <typename T, int C>
__global__ void __launch_bounds__(kHThreads)
pil_hpass_kernel(const T* __restrict__ src, long long total, int W, int OW, int tiles, const int* __restrict__ bounds,
                 const int* __restrict__ kk, int ksize, uint8_t* __restrict__ dst, size_t d_pitch)
{
    __shared__ uint4 stage4[kStageBytes / 16 + 1];
    __shared__ uint32_t orow4[kHThreads * C / 4 + 1];
    uint8_t* stage = (uint8_t*)stage4;
    uint8_t* orow = (uint8_t*)orow4;
    const int tid = threadIdx.x;
    const int row = blockIdx.x / tiles, x0 = (blockIdx.x % tiles) * kHThreads;
    const int cnt = min(kHThreads, OW - x0);
    // the tables are the caller's: every window is clamped to the row, whatever they hold
    const int xs = min(max(bounds[2 * x0], 0), W);
    const int xl = x0 + cnt - 1;
    const int le = min(max(bounds[2 * xl], 0), W);
    const int xe = le + min(max(bounds[2 * xl + 1], 0), min(ksize, W - le));
    int xmin = 0, n = 0;
    const int* k = kk;
    if (tid < cnt) {
        xmin = min(max(bounds[2 * (x0 + tid)], 0), W);
        n = min(max(bounds[2 * (x0 + tid) + 1], 0), min(ksize, W - xmin));
        k = kk + (size_t)(x0 + tid) * ksize;
    }
    int acc[C];
#pragma unroll
    for (int c = 0; c < C; c++) acc[c] = 1 << (kPrecisionBits - 1);
    for (int s = xs; s < xe; s += kChunkPx) {
        const int px = min(kChunkPx, xe - s);
        if (s != xs) __syncthreads();                          // the piece before this one has been read
        const int d = stage_span<T>(stage, src, total, ((long long)row * W + s) * C, px * C, tid, kHThreads);
        __syncthreads();
        const int lo = max(xmin, s), hi = min(xmin + n, s + px);
        for (int x = lo; x < hi; x++) {
            const int kv = k[x - xmin];
            const uint8_t* p = stage + d + (x - s) * C;
#pragma unroll
            for (int c = 0; c < C; c++) acc[c] += (int)p[c] * kv;
        }
    }
    if (tid < cnt) {
#pragma unroll
        for (int c = 0; c < C; c++) orow[tid * C + c] = clip8(acc[c]);
    }
    __syncthreads();
    store_run(dst + (size_t)row * d_pitch + (size_t)x0 * C, orow, 0, cnt * C, tid, kHThreads);
}

// Vertical pass over byte columns.  src: [imgs][H][pitch] bytes, pitch a multiple of 4 and src dword-aligned; dst [imgs][OH][RB].
// Workgroup b: image / output row b / tiles, byte columns (b % tiles) * 512 ...
__global__ void __launch_bounds__(kVThreads)
pil_vpass_kernel(const uint8_t* __restrict__ src, int H, size_t pitch, int OH, int RB, int tiles, const int* __restrict__ bounds,
                 const int* __restrict__ kk, int ksize, uint8_t* __restrict__ dst)
{
    __shared__ uint32_t orow[kVThreads];
    const int tid = threadIdx.x;
    const int line = blockIdx.x / tiles, c0 = (blockIdx.x % tiles) * (kVThreads * 4);
    const int img = line / OH, yy = line % OH;
    const int cnt = min(kVThreads * 4, RB - c0);
    const int ymin = min(max(bounds[2 * yy], 0), H);
    const int n = min(max(bounds[2 * yy + 1], 0), min(ksize, H - ymin));
    const int* k = kk + (size_t)yy * ksize;
    if (4 * tid < cnt) {                                       // the dword may reach into the row's padding, never past the pitch
        int a0, a1, a2, a3;
        a0 = a1 = a2 = a3 = 1 << (kPrecisionBits - 1);
        const uint8_t* p = src + ((size_t)img * H + ymin) * pitch + c0 + 4 * tid;
        for (int y = 0; y < n; y++) {
            const int kv = k[y];
            const uint32_t v = *(const uint32_t*)(p + (size_t)y * pitch);
            a0 += (int)(v & 255) * kv;
            a1 += (int)((v >> 8) & 255) * kv;
            a2 += (int)((v >> 16) & 255) * kv;
            a3 += (int)(v >> 24) * kv;
        }
        orow[tid] = clip8(a0) | ((uint32_t)clip8(a1) << 8) | ((uint32_t)clip8(a2) << 16) | ((uint32_t)clip8(a3) << 24);
    }
    __syncthreads();
    store_run(dst + (size_t)line * RB + c0, (const uint8_t*)orow, 0, cnt, tid, kVThreads);
}

// rows of `len` elements, contiguous in src, to bytes at dst + r * d_pitch.  Workgroup b: row b / tiles, elements (b % tiles) * 4096 ...
template <typename T>
__global__ void __launch_bounds__(256)
pil_copy_kernel(const T* __restrict__ src, long long total, long long len, int tiles, uint8_t* __restrict__ dst, size_t d_pitch)
{
    __shared__ uint4 stage4[(kCopyBytes + 32) / 16];
    uint8_t* stage = (uint8_t*)stage4;
    const int tid = threadIdx.x;
    const long long row = blockIdx.x / tiles, e = (long long)(blockIdx.x % tiles) * kCopyBytes;
    const int cnt = (int)min((long long)kCopyBytes, len - e);
    const int d = stage_span<T>(stage, src, total, row * len + e, cnt, tid, 256);
    __syncthreads();
    store_run(dst + (size_t)row * d_pitch + e, stage, d, cnt, tid, 256);
}

// ---- argument checks shared by the device and the host form --------------------------------------------------------------
constexpr long long kMaxBytes = 2147483647LL;    // the kernels count elements of one buffer in 32 bits where they can

bool shape_ok(int N, int H, int W, int C, int OH, int OW, int filter)
{
    if (filter != MOM_RESIZE_BICUBIC || (C != 1 && C != 3)) return false;
    if (N < 1 || H < 1 || W < 1 || OH < 1 || OW < 1) return false;
    // Image.resize of Pillow 11 and later shrinks an image more than 100 times as tall as wide along the vertical axis FIRST: other
    // bytes than the order built here gives, so such a shape is refused, not answered wrongly
    if (W != OW && OH < H && (long long)H > 100LL * W) return false;
    const long long in = (long long)N * H, out = (long long)N * OH;
    if (in > kMaxBytes / W / C || out > kMaxBytes / OW / C) return false;
    if (in > kMaxBytes / ((OW * (long long)C + 15) & ~15LL)) return false;         // the intermediate
    return (W == OW || pil_ksize(W, OW)) && (H == OH || pil_ksize(H, OH));
}

size_t inter_pitch(int C, int OW) { return ((size_t)OW * C + 15) & ~(size_t)15; }

template <typename T>
int resize_launch(int N, int H, int W, int C, const T* src, int OH, int OW, int filter, const int* bounds_x, const int* kk_x,
                  const int* bounds_y, const int* kk_y, uint8_t* out, void* scratch, size_t scratch_bytes, mom_stream_t stream)
{
    if (!shape_ok(N, H, W, C, OH, OW, filter) || !src || !out || ((uintptr_t)src & (sizeof(T) - 1))) return MOM_EINVAL;
    const bool need_h = W != OW, need_v = H != OH;
    if ((need_h && (!bounds_x || !kk_x)) || (need_v && (!bounds_y || !kk_y))) return MOM_EINVAL;
    const size_t need = mom_pil_resize_scratch_bytes(N, H, W, C, OH, OW);
    if (need && (!scratch || ((uintptr_t)scratch & 15) || scratch_bytes < need)) return MOM_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const long long total = (long long)N * H * W * C;
    const int RB = OW * C;
    uint8_t* hdst = need_v ? (uint8_t*)scratch : out;         // where the horizontal result (or the converted copy) goes
    const size_t hpitch = need_v ? inter_pitch(C, OW) : (size_t)RB;
    if (need_h) {
        const int tiles = (OW + kHThreads - 1) / kHThreads;
        const long long blocks = (long long)N * H * tiles;
        if (blocks > kMaxBytes) return MOM_EINVAL;
        const int ks = pil_ksize(W, OW);
        if (C == 3)
            hipLaunchKernelGGL((pil_hpass_kernel<T, 3>), dim3((unsigned)blocks), dim3(kHThreads), 0, st, src, total, W, OW, tiles,
                               bounds_x, kk_x, ks, hdst, hpitch);
        else
            hipLaunchKernelGGL((pil_hpass_kernel<T, 1>), dim3((unsigned)blocks), dim3(kHThreads), 0, st, src, total, W, OW, tiles,
                               bounds_x, kk_x, ks, hdst, hpitch);
    } else {
        // no axis changes: one row of everything; the vertical axis alone: the rows into the intermediate's pitch
        const long long rows = need_v ? (long long)N * H : 1, len = total / rows;
        const int tiles = (int)((len + kCopyBytes - 1) / kCopyBytes);
        if (rows * tiles > kMaxBytes) return MOM_EINVAL;
        hipLaunchKernelGGL(pil_copy_kernel<T>, dim3((unsigned)(rows * tiles)), dim3(256), 0, st, src, total, len, tiles, hdst, hpitch);
    }
    if (need_v) {
        const int tiles = (RB + kVThreads * 4 - 1) / (kVThreads * 4);
        const long long blocks = (long long)N * OH * tiles;
        if (blocks > kMaxBytes) return MOM_EINVAL;
        hipLaunchKernelGGL(pil_vpass_kernel, dim3((unsigned)blocks), dim3(kVThreads), 0, st, (const uint8_t*)scratch, H, hpitch, OH, RB,
                           tiles, bounds_y, kk_y, pil_ksize(H, OH), out);
    }
    return hipGetLastError() == hipSuccess ? MOM_OK : MOM_ELAUNCH;
}
}  // namespace

extern "C" int mom_pil_resize_ksize(int in_size, int out_size, int filter)
{
    if (filter != MOM_RESIZE_BICUBIC || in_size < 1 || out_size < 1) return MOM_EINVAL;
    const int k = pil_ksize(in_size, out_size);
    return k && (long long)k * out_size <= kMaxBytes / 4 ? k : MOM_EINVAL;
}

extern "C" int mom_pil_resize_coeffs(int in_size, int out_size, int filter, int* bounds, int* kk)
{
    const int ksize = mom_pil_resize_ksize(in_size, out_size, filter);
    if (ksize < 1 || !bounds || !kk) return MOM_EINVAL;
    pil_coeffs(in_size, out_size, ksize, bounds, kk);
    return MOM_OK;
}

extern "C" size_t mom_pil_resize_scratch_bytes(int N, int H, int W, int C, int OH, int OW)
{
    if (!shape_ok(N, H, W, C, OH, OW, MOM_RESIZE_BICUBIC) || H == OH) return 0;
    return (size_t)N * H * inter_pitch(C, OW);
}

extern "C" int mom_pil_resize(int N, int H, int W, int C, const uint8_t* src, int OH, int OW, int filter, const int* bounds_x,
                              const int* kk_x, const int* bounds_y, const int* kk_y, uint8_t* out, void* scratch, size_t scratch_bytes,
                              mom_stream_t stream)
{
    return resize_launch<uint8_t>(N, H, W, C, src, OH, OW, filter, bounds_x, kk_x, bounds_y, kk_y, out, scratch, scratch_bytes, stream);
}

extern "C" int mom_pil_resize_to8b(int N, int H, int W, int C, const float* src, int OH, int OW, int filter, const int* bounds_x,
                                   const int* kk_x, const int* bounds_y, const int* kk_y, uint8_t* out, void* scratch,
                                   size_t scratch_bytes, mom_stream_t stream)
{
    return resize_launch<float>(N, H, W, C, src, OH, OW, filter, bounds_x, kk_x, bounds_y, kk_y, out, scratch, scratch_bytes, stream);
}

extern "C" int mom_pil_resize_host(int N, int H, int W, int C, const uint8_t* src, int OH, int OW, int filter, uint8_t* out)
{
    if (!shape_ok(N, H, W, C, OH, OW, filter) || !src || !out) return MOM_EINVAL;
    const size_t in_px = (size_t)H * W, out_px = (size_t)OH * OW;
    std::vector<uint8_t> mid;
    std::vector<int32_t> bx, kx, by, ky;
    int ksx = 0, ksy = 0;
    if (W != OW) {
        ksx = mom_pil_resize_ksize(W, OW, filter);
        if (ksx < 1) return MOM_EINVAL;
        bx.resize((size_t)OW * 2), kx.resize((size_t)OW * ksx);
        pil_coeffs(W, OW, ksx, bx.data(), kx.data());
    }
    if (H != OH) {
        ksy = mom_pil_resize_ksize(H, OH, filter);
        if (ksy < 1) return MOM_EINVAL;
        by.resize((size_t)OH * 2), ky.resize((size_t)OH * ksy);
        pil_coeffs(H, OH, ksy, by.data(), ky.data());
    }
    if (ksx && ksy) mid.resize((size_t)H * OW * C);
    for (int i = 0; i < N; i++) {
        const uint8_t* s = src + i * in_px * C;
        uint8_t* o = out + i * out_px * C;
        if (!ksx && !ksy) { memcpy(o, s, in_px * C); continue; }
        const uint8_t* vs = s;
        if (ksx) {
            uint8_t* hd = ksy ? mid.data() : o;
            host_axis(s, hd, H, W, OW, C, C, (size_t)W * C, C, (size_t)OW * C, bx.data(), kx.data(), ksx);
            vs = hd;
        }
        // the vertical axis: a "line" is a column of pixels
        if (ksy) host_axis(vs, o, OW, H, OH, C, (size_t)OW * C, C, (size_t)OW * C, C, by.data(), ky.data(), ksy);
    }
    return MOM_OK;
}
