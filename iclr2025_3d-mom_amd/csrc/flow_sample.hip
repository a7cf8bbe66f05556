// The scene-flow fit's targets in one launch, gfx950: every view's 2D flow image sampled at that view's projected points.
//
// The reference (train_motion.py:117-121) calls scipy.interpolate.griddata(pixel grid, flow image, pixels, method="linear") once per
// view.  On a pixel grid that is linear interpolation inside one of the two triangles of the pixel's cell; which diagonal splits
// a cell is the triangulation's (Qhull's) choice, irregular, but a function of (H, W) alone.  The host triangulates the grid once
// (motion.grid_diagonals) and hands the choice over as one bit per cell; the kernel is then a gather: one thread per
// (view, point), the view on the slow grid axis so that a view's image stays in an XCD's L2 while its workgroups run.
//
//   flow    [V][H][W] float2    channel-last; the four corners of a cell are two 16-byte reads, one per image row
//   pix     [V][P] double2      the unflowed pixel (u, v) as the reference hands it to griddata: float64
//   valid   [ceil(V/32)][P]     the fit's bit words, word-major: a wave's 64 words are contiguous
//   diag    [ceil(cells/32)]    bit c % 32 of word c / 32, c = y (W-1) + x: set = the anti-diagonal (x+1,y)-(x,y+1) splits the cell
//   records [V][P] float4       {(float)u, (float)v, gt.x, gt.y}, what sceneflow_fit_kernel reads: one 16-byte store per lane
//
// Everything between the loads and the final rounding is float64 without contraction, in the order include/mom4d.h writes out,
// so that a float64 numpy evaluation of the same expressions gives the same bits.  An invalid pair writes four zeros, by selection
// on its bit; the cell indices are clamped as float64 BEFORE the conversion to int, so a NaN (maxnum keeps the other operand) or
// 1e300 in an invalid slot reaches no address outside the image.  No LDS, no barrier: the threads past P return at once.
#include "mom_common.h"

namespace {

constexpr int kThreads = 256;

struct __attribute__((aligned(8))) TexelPair { float ax, ay, bx, by; };      // texels (x, y) and (x+1, y): 16 bytes, 8-byte aligned

__device__ __forceinline__ double tri_sample(bool anti, double fx, double fy, double f00, double f10, double f01, double f11)
{
#pragma clang fp contract(off)
    if (anti) {
        return fx + fy <= 1.0 ? f00 + fx * (f10 - f00) + fy * (f01 - f00)
                              : f11 + (1.0 - fx) * (f01 - f11) + (1.0 - fy) * (f10 - f11);
    }
    return fx >= fy ? f00 + fx * (f10 - f00) + fy * (f11 - f10)
                    : f00 + fx * (f11 - f01) + fy * (f01 - f00);
}

__global__ void __launch_bounds__(kThreads)
flow_sample_kernel(int P, int H, int W, const float* __restrict__ flow, const double2* __restrict__ pix,
                   const uint32_t* __restrict__ valid, const uint32_t* __restrict__ diag, float4* __restrict__ rec)
{
#pragma clang fp contract(off)
    const size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= (size_t)P) return;
    const int j = blockIdx.y;
    const size_t at = (size_t)j * P + i;
    const bool ok = (valid[(size_t)(j >> 5) * P + i] >> (j & 31)) & 1u;
    const double2 p = pix[at];
    // x0 = clamp(floor(u), 0, W-2) in float64: in range (and 0 for a NaN) before it becomes an int
    const int x0 = (int)fmin(fmax(floor(p.x), 0.0), (double)(W - 2));
    const int y0 = (int)fmin(fmax(floor(p.y), 0.0), (double)(H - 2));
    const double fx = p.x - (double)x0, fy = p.y - (double)y0;
    const size_t cell = (size_t)y0 * (W - 1) + x0;
    const bool anti = (diag[cell >> 5] >> (cell & 31)) & 1u;
    const float* __restrict__ row = flow + (((size_t)j * H + y0) * W + x0) * 2;
    const TexelPair a = *(const TexelPair*)row, b = *(const TexelPair*)(row + 2 * (size_t)W);
    const double gx = tri_sample(anti, fx, fy, (double)a.ax, (double)a.bx, (double)b.ax, (double)b.bx);
    const double gy = tri_sample(anti, fx, fy, (double)a.ay, (double)a.by, (double)b.ay, (double)b.by);
    rec[at] = ok ? float4{(float)p.x, (float)p.y, (float)gx, (float)gy} : float4{0.0f, 0.0f, 0.0f, 0.0f};
}

}  // namespace

extern "C" int mom_flow_sample(int P, int V, int H, int W, const float* flow, const double* pix, const uint32_t* valid,
                               const uint32_t* diag, float* records, mom_stream_t stream)
{
    if (P < 0 || V <= 0 || V > 65535 || H < 2 || W < 2) return MOM_EINVAL;
    if (P == 0) return MOM_OK;
    if (!flow || !pix || !valid || !diag || !records) return MOM_EINVAL;
    if (((uintptr_t)records & 15) || ((uintptr_t)pix & 15) || ((uintptr_t)flow & 7)) return MOM_EINVAL;
    const size_t blocks = ((size_t)P + kThreads - 1) / kThreads;
    hipLaunchKernelGGL(flow_sample_kernel, dim3((unsigned)blocks, (unsigned)V), dim3(kThreads), 0, (hipStream_t)stream, P, H, W, flow,
                       (const double2*)pix, valid, diag, (float4*)records);
    return hipGetLastError() == hipSuccess ? MOM_OK : MOM_ELAUNCH;
}
