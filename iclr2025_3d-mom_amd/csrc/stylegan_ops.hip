// The two native ops of the StyleGAN2 that the reference's video generator is built on (thirdparty/StyleCineGAN/models/stylegan2/op,
// and the encoder's copy of it), gfx950:
//
//   mom_upfirdn2d        op/upfirdn2d.py:85-121, upfirdn2d_kernel.cu    up-sample by zero insertion, pad / crop, FIR, down-sample
//   mom_fused_bias_act   op/fused_act.py, fused_bias_act_kernel.cu      bias + leaky ReLU (or its gradient) + gain
//
// Both are streaming passes.  upfirdn2d: a workgroup stages the input tile of its 64 x 16 outputs (with the halo of the taps) and the
// flipped taps in LDS; each output is an fp32 sum in a fixed order (tap rows ascending, then tap columns), no atomics, so two runs
// give the same bits.  The six shapes the generator, the discriminator and the encoder call it with are compile-time instantiations
// (up / down / taps: 1/1/4x4, 1/1/3x3, 2/1/4x4, 2/1/2x2, 1/2/4x4, 1/2/2x2); an up-2 instantiation visits only the taps of its output
// phase (the inserted zeros are never multiplied).  Everything else with 1 <= kh, kw <= 32 takes the general kernel: taps in LDS,
// the input read from global memory with the same phase stepping.  The plane index is a grid axis that is looped.
#include "mom_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kTileW = 64, kTileH = 16, kRows = kTileH / (kThreads / kTileW);   // a thread computes kRows consecutive output rows
constexpr int kMaxTap = 32;
constexpr int kMaxPlanesY = 65535;           // the plane axis of the grid; the kernels loop beyond it
constexpr int64_t kLim = (int64_t)1 << 29;   // |pad|, down and H up stay below this: every coordinate the kernels form fits an int

struct Upfir {
    int M, H, W, kh, kw, up_x, up_y, down_x, down_y, pad_x0, pad_y0, out_h, out_w, tiles_x;
};

// smallest non-negative a with (v + a) divisible by n
__device__ __forceinline__ int phase(int v, int n) { const int r = v % n; return r > 0 ? n - r : -r; }
// ceil(v / n), n > 0, any sign of v
__device__ __forceinline__ int ceil_div(int v, int n) { const int q = v / n; return q * n < v ? q + 1 : q; }

template <int UP, int DOWN, int KH, int KW>
__global__ void __launch_bounds__(kThreads)
upfirdn2d_tile_kernel(Upfir p, const float* __restrict__ x, const float* __restrict__ k, float* __restrict__ out)
{
    // rows / columns of the input that the taps of a tile of outputs can touch
    constexpr int IN_H = ((kTileH - 1) * DOWN + KH - 1) / UP + 1, IN_W = ((kTileW - 1) * DOWN + KW - 1) / UP + 1;
    constexpr int LD = IN_W | 1;
    constexpr int TA = (KH + UP - 1) / UP, TB = (KW + UP - 1) / UP;     // the most taps of one phase, per axis
    __shared__ float taps[KH * KW];
    __shared__ float tile[IN_H * LD];
    const int ox0 = (int)(blockIdx.x % p.tiles_x) * kTileW, oy0 = (int)(blockIdx.x / p.tiles_x) * kTileH;
    const int ix_lo = ceil_div(ox0 * DOWN - p.pad_x0, UP), iy_lo = ceil_div(oy0 * DOWN - p.pad_y0, UP);
    if (threadIdx.x < KH * KW) taps[threadIdx.x] = k[KH * KW - 1 - threadIdx.x];       // taps[a][b] = k[kh-1-a][kw-1-b]
    const int lx = threadIdx.x % kTileW, ly = (threadIdx.x / kTileW) * kRows;
    const int ox = ox0 + lx, Xb = ox * DOWN - p.pad_x0, b0 = UP == 1 ? 0 : phase(Xb, UP);
    const int c0 = (Xb + b0) / UP - ix_lo;           // exact: Xb + b0 is a multiple of UP; 0 <= c0 + j, the last tap's column < IN_W
    const size_t in_plane = (size_t)p.H * p.W, out_plane = (size_t)p.out_h * p.out_w;
    for (int m = blockIdx.y; m < p.M; m += gridDim.y) {
        const float* __restrict__ xin = x + (size_t)m * in_plane;
        __syncthreads();                             // the taps are written / the last plane's tile has been read
        for (int i = threadIdx.x; i < IN_H * IN_W; i += kThreads) {
            const int r = i / IN_W, c = i % IN_W, iy = iy_lo + r, ix = ix_lo + c;
            tile[r * LD + c] = (iy >= 0 && iy < p.H && ix >= 0 && ix < p.W) ? xin[(size_t)iy * p.W + ix] : 0.0f;
        }
        __syncthreads();
        if (ox >= p.out_w) continue;
#pragma unroll
        for (int i = 0; i < kRows; i++) {
            const int oy = oy0 + ly + i;
            if (oy >= p.out_h) break;
            const int Yb = oy * DOWN - p.pad_y0, a0 = UP == 1 ? 0 : phase(Yb, UP);
            const int r0 = (Yb + a0) / UP - iy_lo;
            float acc = 0.0f;
#pragma unroll
            for (int ja = 0; ja < TA; ja++) {
                const int a = a0 + ja * UP;
                if (a >= KH) break;
#pragma unroll
                for (int jb = 0; jb < TB; jb++) {
                    const int b = b0 + jb * UP;
                    if (b >= KW) break;
                    acc += taps[a * KW + b] * tile[(r0 + ja) * LD + c0 + jb];
                }
            }
            out[(size_t)m * out_plane + (size_t)oy * p.out_w + ox] = acc;
        }
    }
}

// Any factors, pads and taps up to 32 x 32: one output per thread, the input read where it lies.
__global__ void __launch_bounds__(kThreads)
upfirdn2d_general_kernel(Upfir p, const float* __restrict__ x, const float* __restrict__ k, float* __restrict__ out)
{
    __shared__ float taps[kMaxTap * kMaxTap];
    const int nk = p.kh * p.kw;
    for (int i = threadIdx.x; i < nk; i += kThreads) taps[i] = k[nk - 1 - i];
    __syncthreads();
    const size_t in_plane = (size_t)p.H * p.W, out_plane = (size_t)p.out_h * p.out_w;
    const size_t o = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (o >= out_plane) return;
    const int oy = (int)(o / p.out_w), ox = (int)(o % p.out_w);
    const int Yb = oy * p.down_y - p.pad_y0, Xb = ox * p.down_x - p.pad_x0;
    const int a0 = phase(Yb, p.up_y), b0 = phase(Xb, p.up_x);
    for (int m = blockIdx.y; m < p.M; m += gridDim.y) {
        const float* __restrict__ xin = x + (size_t)m * in_plane;
        float acc = 0.0f;
        for (int a = a0; a < p.kh; a += p.up_y) {
            const int iy = (Yb + a) / p.up_y;
            if (iy < 0) continue;
            if (iy >= p.H) break;
            for (int b = b0; b < p.kw; b += p.up_x) {
                const int ix = (Xb + b) / p.up_x;
                if (ix < 0) continue;
                if (ix >= p.W) break;
                acc += taps[a * p.kw + b] * xin[(size_t)iy * p.W + ix];
            }
        }
        out[(size_t)m * out_plane + o] = acc;
    }
}

template <int UP, int DOWN, int KH, int KW>
void launch_tile(const Upfir& p, const float* x, const float* k, float* out, hipStream_t stream)
{
    const unsigned tiles = (unsigned)p.tiles_x * (unsigned)((p.out_h + kTileH - 1) / kTileH);
    hipLaunchKernelGGL((upfirdn2d_tile_kernel<UP, DOWN, KH, KW>), dim3(tiles, (unsigned)(p.M < kMaxPlanesY ? p.M : kMaxPlanesY)),
                       dim3(kThreads), 0, stream, p, x, k, out);
}

// ---- bias + activation + gain ------------------------------------------------------------------------------------------------------
constexpr int kVec = 4, kLoop = 4;                        // elements per thread and pass; passes per workgroup
constexpr unsigned kBlockElems = kThreads * kVec * kLoop;

// mode: act * 10 + grad, the reference's switch.  ALIGNED: x, ref and out are 16-byte aligned, full groups of four move as float4.
template <bool ALIGNED>
__global__ void __launch_bounds__(kThreads)
fused_bias_act_kernel(unsigned n, unsigned step_b, unsigned size_b, int mode, float alpha, float scale, const float* __restrict__ x,
                      const float* __restrict__ b, const float* __restrict__ ref, float* __restrict__ out)
{
#pragma clang fp contract(off)
    const bool use_ref = mode == 31;
    for (int pass = 0; pass < kLoop; pass++) {
        const unsigned i0 = blockIdx.x * kBlockElems + (unsigned)pass * (kThreads * kVec) + threadIdx.x * kVec;   // n < 2^31: no wrap
        if (i0 >= n) return;
        const unsigned cnt = n - i0 < (unsigned)kVec ? n - i0 : (unsigned)kVec;
        float v[kVec], r[kVec];
        if (ALIGNED && cnt == kVec) {
            const float4 t = *reinterpret_cast<const float4*>(x + i0);
            v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
            if (use_ref) {
                const float4 u = *reinterpret_cast<const float4*>(ref + i0);
                r[0] = u.x; r[1] = u.y; r[2] = u.z; r[3] = u.w;
            }
        } else {
            for (unsigned j = 0; j < (unsigned)kVec; j++) {
                v[j] = j < cnt ? x[i0 + j] : 0.0f;
                if (use_ref) r[j] = j < cnt ? ref[i0 + j] : 0.0f;
            }
        }
        if (b) {
            // b[(i / step_b) % size_b] with two divisions per four elements: the remainder and the bias index are carried along
            unsigned q = i0 / step_b, rem = i0 - q * step_b, bi = q % size_b;
            for (int j = 0; j < kVec; j++) {
                v[j] = v[j] + b[bi];
                if (++rem == step_b) { rem = 0; if (++bi == size_b) bi = 0; }
            }
        }
        for (int j = 0; j < kVec; j++) {
            float y;
            if (mode == 10 || mode == 11) y = v[j];
            else if (mode == 12 || mode == 32) y = 0.0f;
            else y = ((use_ref ? r[j] : v[j]) > 0.0f) ? v[j] : v[j] * alpha;
            v[j] = y * scale;
        }
        if (ALIGNED && cnt == kVec) {
            *reinterpret_cast<float4*>(out + i0) = make_float4(v[0], v[1], v[2], v[3]);
        } else {
            for (unsigned j = 0; j < cnt; j++) out[i0 + j] = v[j];
        }
    }
}

}  // namespace

extern "C" int mom_upfirdn2d(int M, int H, int W, int kh, int kw, int up_x, int up_y, int down_x, int down_y, int pad_x0, int pad_x1,
                             int pad_y0, int pad_y1, const float* x, const float* k, float* out, mom_stream_t stream)
{
    if (M < 1 || H < 1 || W < 1 || kh < 1 || kw < 1 || kh > kMaxTap || kw > kMaxTap || up_x < 1 || up_y < 1 || down_x < 1 ||
        down_y < 1 || !x || !k || !out)
        return MOM_EINVAL;
    const int64_t span_y = (int64_t)H * up_y, span_x = (int64_t)W * up_x;
    auto wide = [](int64_t v) { return v >= kLim || v <= -kLim; };
    if (wide(span_y) || wide(span_x) || wide(pad_x0) || wide(pad_x1) || wide(pad_y0) || wide(pad_y1) || wide(down_x) || wide(down_y))
        return MOM_EINVAL;
    const int64_t num_y = span_y + pad_y0 + pad_y1 - kh, num_x = span_x + pad_x0 + pad_x1 - kw;
    if (num_y < 0 || num_x < 0) return MOM_EINVAL;                       // out_h or out_w below 1
    const int64_t out_h = num_y / down_y + 1, out_w = num_x / down_x + 1;
    if ((int64_t)H * W >= ((int64_t)1 << 31) || out_h * out_w >= ((int64_t)1 << 31)) return MOM_EINVAL;
    // a grid axis holds fewer than 2^32 threads
    if (((out_w + kTileW - 1) / kTileW) * ((out_h + kTileH - 1) / kTileH) >= ((int64_t)1 << 24)) return MOM_EINVAL;
    Upfir p = {M, H, W, kh, kw, up_x, up_y, down_x, down_y, pad_x0, pad_y0, (int)out_h, (int)out_w, (int)((out_w + kTileW - 1) / kTileW)};
    hipStream_t s = (hipStream_t)stream;
    const int up = up_x == up_y ? up_x : 0, down = down_x == down_y ? down_x : 0;
    auto is = [&](int u, int d, int h, int w) { return up == u && down == d && kh == h && kw == w; };
    if (is(1, 1, 4, 4)) launch_tile<1, 1, 4, 4>(p, x, k, out, s);
    else if (is(1, 1, 3, 3)) launch_tile<1, 1, 3, 3>(p, x, k, out, s);
    else if (is(2, 1, 4, 4)) launch_tile<2, 1, 4, 4>(p, x, k, out, s);
    else if (is(2, 1, 2, 2)) launch_tile<2, 1, 2, 2>(p, x, k, out, s);
    else if (is(1, 2, 4, 4)) launch_tile<1, 2, 4, 4>(p, x, k, out, s);
    else if (is(1, 2, 2, 2)) launch_tile<1, 2, 2, 2>(p, x, k, out, s);
    else
        hipLaunchKernelGGL(upfirdn2d_general_kernel, dim3((unsigned)((out_h * out_w + kThreads - 1) / kThreads),
                                                          (unsigned)(M < kMaxPlanesY ? M : kMaxPlanesY)),
                           dim3(kThreads), 0, s, p, x, k, out);
    return hipGetLastError() == hipSuccess ? MOM_OK : MOM_ELAUNCH;
}

extern "C" int mom_fused_bias_act(size_t n, int step_b, int size_b, int act, int grad, float alpha, float scale, const float* x,
                                  const float* b, const float* ref, float* out, mom_stream_t stream)
{
    if ((act != 1 && act != 3) || grad < 0 || grad > 2 || n < 1 || n >= ((size_t)1 << 31) || step_b < 1 || (b && size_b < 1) || !x ||
        !out)
        return MOM_EINVAL;
    if (act == 3 && grad == 1 && !ref) return MOM_EINVAL;
    const unsigned blocks = (unsigned)((n + kBlockElems - 1) / kBlockElems);
    const bool aligned = (((uintptr_t)x | (uintptr_t)out | (uintptr_t)(act == 3 && grad == 1 ? ref : nullptr)) & 15) == 0;
    const unsigned sb = b ? (unsigned)size_b : 1u;
    if (aligned)
        hipLaunchKernelGGL(fused_bias_act_kernel<true>, dim3(blocks), dim3(kThreads), 0, (hipStream_t)stream, (unsigned)n,
                           (unsigned)step_b, sb, act * 10 + grad, alpha, scale, x, b, ref, out);
    else
        hipLaunchKernelGGL(fused_bias_act_kernel<false>, dim3(blocks), dim3(kThreads), 0, (hipStream_t)stream, (unsigned)n,
                           (unsigned)step_b, sb, act * 10 + grad, alpha, scale, x, b, ref, out);
    return hipGetLastError() == hipSuccess ? MOM_OK : MOM_ELAUNCH;
}
