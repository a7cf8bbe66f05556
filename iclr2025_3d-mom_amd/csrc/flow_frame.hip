// The arithmetic around stage 1's 2D flow estimator, for all V views of a scene in one call each (include/mom4d.h has the contract):
//   mom_hint_field   the dense hint field and the masks in front of the estimator (thirdparty/cinemagraphy/demo.py:77-103)
//   mom_flow_finish  the masking, blur, rescale and resize behind it (thirdparty/cinemagraphy/lib/renderer.py:598-606)
// The reference runs both on the CPU, once per view.  Everything is fp32 in the reference's order of operations, contracted only
// where torch's CPU kernels are (the bilinear resize), except the two places named in the header: expf is the device's, and the
// 15 x 15 box sum is formed as 15 row sums of 15 terms.
// No atomics anywhere: two calls give the same bits.
#include "mom_common.h"

namespace {
constexpr int kThreads = 256;
constexpr int kBoxR = 7;                          // box_blur(flow, (15, 15)): 7 on either side
constexpr int kBoxN = (2 * kBoxR + 1) * (2 * kBoxR + 1);
constexpr int kTile = 32;                         // outputs per side of a blur workgroup
constexpr int kTileIn = kTile + 2 * kBoxR;

// F.interpolate(..., mode='bilinear', align_corners=False) as torch's CPU kernels compute it, where the reference runs it: the source
// coordinate scale * (dst + 0.5) - 0.5 is ONE fused multiply-add in fp32 (scale = (float)in / out; negative sources clamp to 0), and
// so is each of the three sums of the interpolation.  With two roundings in the coordinate an output row or column whose source is
// an integer in exact arithmetic takes its neighbour's pixels.
struct Tap { int i0, i1; float l0, l1; };
__device__ __forceinline__ Tap bilinear_tap(int dst, int in, int out)
{
#pragma clang fp contract(off)
    const float scale = (float)in / (float)out;
    float src = __builtin_fmaf(scale, (float)dst + 0.5f, -0.5f);
    if (src < 0.f) src = 0.f;
    Tap t;
    t.i0 = min((int)src, in - 1);
    t.i1 = t.i0 + (t.i0 < in - 1 ? 1 : 0);
    t.l1 = src - (float)t.i0;
    t.l0 = 1.f - t.l1;
    return t;
}
__device__ __forceinline__ float bilinear_at(const float* __restrict__ plane, int in_w, Tap ty, Tap tx)
{
#pragma clang fp contract(off)
    const float* r0 = plane + (size_t)ty.i0 * in_w;
    const float* r1 = plane + (size_t)ty.i1 * in_w;
    const float top = __builtin_fmaf(tx.l0, r0[tx.i0], tx.l1 * r0[tx.i1]);
    const float bot = __builtin_fmaf(tx.l0, r1[tx.i0], tx.l1 * r1[tx.i1]);
    return __builtin_fmaf(ty.l0, top, ty.l1 * bot);
}

// ---- launch 1 of mom_hint_field: the dense field at the image's own size, masked and scaled (demo.py:77-101) ----
__global__ void __launch_bounds__(kThreads) hint_dense_kernel(int H, int W, int max_hints, const int* __restrict__ pos,
                                                              const double* __restrict__ start, const double* __restrict__ end,
                                                              const int* __restrict__ count, const float* __restrict__ sigma,
                                                              const uint8_t* __restrict__ mask, float scale_x, float scale_y,
                                                              float* __restrict__ dense)
{
#pragma clang fp contract(off)
    const int v = blockIdx.y;
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= H * W) return;
    const float x = (float)(i % W), y = (float)(i / W);
    const int n = min(max(count[v], 0), max_hints);
    const float sg = sigma[v];
    float mx = 0.f, my = 0.f, norm = 0.f;
    for (int k = 0; k < n; ++k) {
        const size_t h = ((size_t)v * max_hints + k) * 2;
        const float dx = x - (float)pos[h], dy = y - (float)pos[h + 1];
        const float dist = __fsqrt_rn(dx * dx + dy * dy);
        const float q = __fdiv_rn(dist, sg);
        const float w = expf(-(q * q));
        // hint_motion is float64 there, so `dense_motion += weight * hint_motion` adds in float64 and rounds to fp32 (demo.py:70,93)
        mx = (float)((double)mx + (double)w * ((end[h] - start[h]) / 50.));
        my = (float)((double)my + (double)w * ((end[h + 1] - start[h + 1]) / 50.));
        norm += w;
    }
    if (norm == 0.f) norm = 1.f;
    const float keep = mask[(size_t)v * H * W + i] ? 1.f : 0.f;
    float* out = dense + (size_t)v * 2 * H * W + i;
    out[0] = __fdiv_rn(mx, norm) * keep * scale_x;
    out[(size_t)H * W] = __fdiv_rn(my, norm) * keep * scale_y;
}

// ---- launch 2: per view three S x S planes -- the field's two channels resized bilinearly, and F.interpolate(mode='area') of
// mask != 0, which is adaptive_avg_pool2d: the window [floor(o in / out), ceil((o + 1) in / out)), the sum of the (exact) ones
// divided by the window's height and then by its width, as torch's CPU kernel divides (demo.py:102-103) ----
__global__ void __launch_bounds__(kThreads) hint_resize_kernel(int H, int W, int S, const float* __restrict__ dense,
                                                               const uint8_t* __restrict__ mask, float* __restrict__ hints,
                                                               float* __restrict__ mask_s)
{
#pragma clang fp contract(off)
    const int v = blockIdx.y / 3, p = blockIdx.y % 3;
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= S * S) return;
    const int ox = i % S, oy = i / S;
    if (p < 2) {
        hints[((size_t)v * 2 + p) * S * S + i] = bilinear_at(dense + ((size_t)v * 2 + p) * H * W, W, bilinear_tap(oy, H, S),
                                                            bilinear_tap(ox, W, S));
        return;
    }
    const int y0 = (int)(((int64_t)oy * H) / S), y1 = (int)((((int64_t)oy + 1) * H + S - 1) / S);
    const int x0 = (int)(((int64_t)ox * W) / S), x1 = (int)((((int64_t)ox + 1) * W + S - 1) / S);
    const uint8_t* m = mask + (size_t)v * H * W;
    int ones = 0;
    for (int yy = y0; yy < y1; ++yy)
        for (int xx = x0; xx < x1; ++xx) ones += m[(size_t)yy * W + xx] ? 1 : 0;
    mask_s[(size_t)v * S * S + i] = __fdiv_rn(__fdiv_rn((float)ones, (float)(y1 - y0)), (float)(x1 - x0));
}

// ---- launch 1 of mom_flow_finish: (box mean of pred * mask) * mask * scale at S x S (renderer.py:598-605) ----
// A workgroup makes a 32 x 32 tile: the 46 x 46 products it needs go to LDS (0 outside the image: border_type='constant'), then 15-term
// row sums, then 15-term column sums of those.
__global__ void __launch_bounds__(kThreads) flow_blur_kernel(int S, int tiles_x, const float* __restrict__ pred,
                                                             const float* __restrict__ mask_s, float scale_x, float scale_y,
                                                             float* __restrict__ blurred)
{
#pragma clang fp contract(off)
    __shared__ float in[kTileIn][kTileIn + 1];
    __shared__ float rows[kTileIn][kTile + 1];
    const int plane = blockIdx.y, v = plane >> 1;
    const int tx0 = (blockIdx.x % tiles_x) * kTile, ty0 = (blockIdx.x / tiles_x) * kTile;
    const float* pp = pred + (size_t)plane * S * S;
    const float* mm = mask_s + (size_t)v * S * S;
    for (int i = threadIdx.x; i < kTileIn * kTileIn; i += kThreads) {
        const int ly = i / kTileIn, lx = i % kTileIn;
        const int gy = ty0 + ly - kBoxR, gx = tx0 + lx - kBoxR;
        float val = 0.f;
        if (gy >= 0 && gy < S && gx >= 0 && gx < S) val = pp[(size_t)gy * S + gx] * mm[(size_t)gy * S + gx];
        in[ly][lx] = val;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < kTileIn * kTile; i += kThreads) {
        const int ly = i / kTile, lx = i % kTile;
        float s = 0.f;
#pragma unroll
        for (int k = 0; k <= 2 * kBoxR; ++k) s += in[ly][lx + k];
        rows[ly][lx] = s;
    }
    __syncthreads();
    const float scale = (plane & 1) ? scale_y : scale_x;
    for (int i = threadIdx.x; i < kTile * kTile; i += kThreads) {
        const int ly = i / kTile, lx = i % kTile;
        const int gy = ty0 + ly, gx = tx0 + lx;
        if (gy >= S || gx >= S) continue;
        float s = 0.f;
#pragma unroll
        for (int k = 0; k <= 2 * kBoxR; ++k) s += rows[ly + k][lx];
        blurred[(size_t)plane * S * S + (size_t)gy * S + gx] = __fdiv_rn(s, (float)kBoxN) * mm[(size_t)gy * S + gx] * scale;
    }
}

// ---- launch 2: M planes of [S,S] -> [H,W], bilinear (renderer.py:606) ----
__global__ void __launch_bounds__(kThreads) flow_resize_kernel(int S, int H, int W, const float* __restrict__ blurred,
                                                               float* __restrict__ flow)
{
    const int plane = blockIdx.y;
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= H * W) return;
    flow[(size_t)plane * H * W + i] = bilinear_at(blurred + (size_t)plane * S * S, S, bilinear_tap(i / W, S, H), bilinear_tap(i % W, S, W));
}

// V views of an h x w plane and of an S x S plane: every index fits an int, the view count fits a grid's y extent (3 planes a view)
bool shape_ok(int V, int h, int w, int S)
{
    if (V < 1 || V > 21845 || h < 1 || w < 1 || S < 1) return false;
    const int64_t lim = (int64_t)1 << 31;
    return (int64_t)h * w < lim && (int64_t)S * S < lim && (int64_t)V * 2 * h * w < lim && (int64_t)V * 2 * S * S < lim;
}
}  // namespace

extern "C" size_t mom_hint_field_scratch_bytes(int V, int H, int W)
{
    return shape_ok(V, H, W, 1) ? (size_t)V * 2 * H * W * sizeof(float) : 0;
}

extern "C" int mom_hint_field(int V, int H, int W, int S, int max_hints, const int* hint_pos, const double* hint_start,
                              const double* hint_end, const int* hint_count, const float* sigma, const uint8_t* mask, float* hints,
                              float* mask_s, void* scratch, size_t scratch_bytes, mom_stream_t stream)
{
    if (!shape_ok(V, H, W, S) || max_hints < 0 || max_hints > MOM_HINTS_MAX) return MOM_EINVAL;
    if (!hint_count || !sigma || !mask || !hints || !mask_s || !scratch) return MOM_EINVAL;
    if (max_hints > 0 && (!hint_pos || !hint_start || !hint_end)) return MOM_EINVAL;
    if (((uintptr_t)scratch & 3) || scratch_bytes < mom_hint_field_scratch_bytes(V, H, W)) return MOM_EINVAL;
    float* dense = (float*)scratch;
    const float scale_x = (float)((double)S / W), scale_y = (float)((double)S / H);      // torch.FloatTensor of Python floats
    hipLaunchKernelGGL(hint_dense_kernel, dim3((unsigned)(((int64_t)H * W + kThreads - 1) / kThreads), (unsigned)V), dim3(kThreads), 0,
                       (hipStream_t)stream, H, W, max_hints, hint_pos, hint_start, hint_end, hint_count, sigma, mask, scale_x, scale_y,
                       dense);
    if (hipGetLastError() != hipSuccess) return MOM_ELAUNCH;
    hipLaunchKernelGGL(hint_resize_kernel, dim3((unsigned)(((int64_t)S * S + kThreads - 1) / kThreads), (unsigned)(V * 3)),
                       dim3(kThreads), 0, (hipStream_t)stream, H, W, S, dense, mask, hints, mask_s);
    return hipGetLastError() == hipSuccess ? MOM_OK : MOM_ELAUNCH;
}

extern "C" size_t mom_flow_finish_scratch_bytes(int V, int S)
{
    return shape_ok(V, 1, 1, S) ? (size_t)V * 2 * S * S * sizeof(float) : 0;
}

extern "C" int mom_flow_finish(int V, int S, int H, int W, const float* pred, const float* mask_s, float* flow, void* scratch,
                               size_t scratch_bytes, mom_stream_t stream)
{
    if (!shape_ok(V, H, W, S) || !pred || !mask_s || !flow || !scratch) return MOM_EINVAL;
    if (((uintptr_t)scratch & 3) || scratch_bytes < mom_flow_finish_scratch_bytes(V, S)) return MOM_EINVAL;
    const int tiles_x = (S + kTile - 1) / kTile;
    if ((int64_t)tiles_x * tiles_x >= ((int64_t)1 << 31)) return MOM_EINVAL;
    float* blurred = (float*)scratch;
    const float scale_x = (float)((double)W / S), scale_y = (float)((double)H / S);
    hipLaunchKernelGGL(flow_blur_kernel, dim3((unsigned)(tiles_x * tiles_x), (unsigned)(V * 2)), dim3(kThreads), 0,
                       (hipStream_t)stream, S, tiles_x, pred, mask_s, scale_x, scale_y, blurred);
    if (hipGetLastError() != hipSuccess) return MOM_ELAUNCH;
    hipLaunchKernelGGL(flow_resize_kernel, dim3((unsigned)(((int64_t)H * W + kThreads - 1) / kThreads), (unsigned)(V * 2)),
                       dim3(kThreads), 0, (hipStream_t)stream, S, H, W, blurred, flow);
    return hipGetLastError() == hipSuccess ? MOM_OK : MOM_ELAUNCH;
}
