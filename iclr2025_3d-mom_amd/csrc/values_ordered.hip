// Ordered value reductions of the loss: the L1 sums, the fold of the SSIM block totals and the plane regularisers' value, gfx950.
//
// The atomic forms (optim_loss.hip l1_kernel and plane_reg_kernel, ssim.hip ssim_fwd_kernel) end every workgroup with a float or
// double atomicAdd into one or a few words, so the VALUE of a loss term depends on the order the workgroups arrive in (its gradient,
// formed per element, does not).  Here every workgroup STORES its total into a slot of its own, and one workgroup per result adds the
// slots up in the order include/mom4d.h documents ("ordered loss values"): no float atomic anywhere, and the order is a function of
// the problem size alone.
//
// THIS FILE IS COMPILED WITH -ffp-contract=off: the host twins at its end must multiply and add exactly as the kernels do.
#include "mom_common.h"

namespace {

constexpr int kBlock = 64;          // terms per block of the order
constexpr int kL1Share = 4096;      // elements per workgroup of the L1 pass: 256 lanes x 4 rounds x 4 consecutive elements
constexpr int kRegRows = 16;        // rows of H per workgroup of the regulariser, as plane_reg_kernel

// The 256 lane sums of a workgroup -> its total, in thread 0: blocks of 64 lanes (a wave), each added left to right from +0.0 by
// one thread out of LDS, then the four block sums left to right.
__device__ __forceinline__ float wg_fold(float v, float* s_lane /* [256] */, float* s_wave /* [4] */)
{
    s_lane[threadIdx.x] = v;
    __syncthreads();
    if (threadIdx.x < 4) {
        float b = 0.f;
        for (int i = 0; i < kBlock; i++) b += s_lane[threadIdx.x * kBlock + i];
        s_wave[threadIdx.x] = b;
    }
    __syncthreads();
    float t = 0.f;
    if (threadIdx.x == 0)
        for (int w = 0; w < 4; w++) t += s_wave[w];
    __syncthreads();                 // (the arrays may be reused by a second fold)
    return t;
}

// out[r] = fold of part[r * stride .. + n): blocks of 64 partials from the first, each left to right from +0.0 in T, then the block
// sums left to right.  One workgroup per result r; 256 blocks at a time meet in LDS, thread 0 carries the running total.
template <typename T>
__global__ void __launch_bounds__(256) fold_kernel(size_t n, const float* __restrict__ part, size_t stride, T* __restrict__ out)
{
    __shared__ T s_b[256];
    const float* __restrict__ p = part + (size_t)blockIdx.x * stride;
    T total = (T)0;
    for (size_t c0 = 0; c0 < n; c0 += (size_t)256 * kBlock) {
        const size_t j0 = c0 + (size_t)threadIdx.x * kBlock;
        T b = (T)0;
        if (j0 < n) {
            const size_t j1 = n - j0 < (size_t)kBlock ? n : j0 + kBlock;
            for (size_t i = j0; i < j1; i++) b += (T)p[i];
        }
        s_b[threadIdx.x] = b;
        __syncthreads();
        if (threadIdx.x == 0) {
            const size_t left = (n - c0 + kBlock - 1) / kBlock;
            const int nb = left < 256 ? (int)left : 256;
            for (int k = 0; k < nb; k++) total += s_b[k];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) out[blockIdx.x] = total;
}

template <typename T>
void fold_host(size_t n, const float* p, T* out)
{
    T total = (T)0;
    for (size_t j0 = 0; j0 < n; j0 += kBlock) {
        T b = (T)0;
        for (size_t i = j0; i < n && i < j0 + kBlock; i++) b += (T)p[i];
        total += b;
    }
    *out = total;
}

// ---------------------------------------------------------------- L1 sums
// the two terms of one element, added onto the lane's sums; returns the gradient, sign(d) / n as l1_kernel forms it
__host__ __device__ __forceinline__ float l1_one(float x, float y, float inv_n, float& a1, float& a2)
{
    const float d = x - y;
    a1 += fabsf(d);
    a2 += d * d;
    return d > 0.f ? inv_n : (d < 0.f ? -inv_n : 0.f);
}

__global__ void __launch_bounds__(256)
l1_ordered_kernel(size_t n, const float* __restrict__ img, const float* __restrict__ gt, float* __restrict__ dimg, float inv_n,
                  float* __restrict__ part /* [2][gridDim.x] */)
{
    __shared__ float s_lane[256], s_wave[4];
    // Workgroup g owns elements [4096 g, 4096 (g + 1)); lane t takes, for r = 0..3, the four elements 4096 g + 1024 r + 4 t + j,
    // j = 0..3, in that order: a lane's sixteen elements in ascending index.  16 bytes per lane where the pointers allow it and the
    // share is whole; the same elements in the same order one by one otherwise.
    const size_t base = (size_t)blockIdx.x * kL1Share;
    float a1 = 0.f, a2 = 0.f;
    const bool vec = ((reinterpret_cast<uintptr_t>(img) | reinterpret_cast<uintptr_t>(gt) | reinterpret_cast<uintptr_t>(dimg)) & 15) == 0 &&
                     n - base >= (size_t)kL1Share;
    if (vec) {
        const float4* __restrict__ img4 = reinterpret_cast<const float4*>(img + base);
        const float4* __restrict__ gt4 = reinterpret_cast<const float4*>(gt + base);
        float4* __restrict__ dimg4 = dimg ? reinterpret_cast<float4*>(dimg + base) : nullptr;
        float4 x[4], y[4];
#pragma unroll
        for (int r = 0; r < 4; r++) {
            x[r] = img4[r * 256 + threadIdx.x];
            y[r] = gt4[r * 256 + threadIdx.x];
        }
#pragma unroll
        for (int r = 0; r < 4; r++) {
            float4 g;
            g.x = l1_one(x[r].x, y[r].x, inv_n, a1, a2);
            g.y = l1_one(x[r].y, y[r].y, inv_n, a1, a2);
            g.z = l1_one(x[r].z, y[r].z, inv_n, a1, a2);
            g.w = l1_one(x[r].w, y[r].w, inv_n, a1, a2);
            if (dimg4) dimg4[r * 256 + threadIdx.x] = g;
        }
    } else {
        for (int r = 0; r < 4; r++)
            for (int j = 0; j < 4; j++) {
                const size_t i = base + (size_t)(r * 1024 + 4 * (int)threadIdx.x + j);
                if (i < n) {
                    const float g = l1_one(img[i], gt[i], inv_n, a1, a2);
                    if (dimg) dimg[i] = g;
                }
            }
    }
    const float t1 = wg_fold(a1, s_lane, s_wave);
    const float t2 = wg_fold(a2, s_lane, s_wave);
    if (threadIdx.x == 0) {
        part[blockIdx.x] = t1;
        part[(size_t)gridDim.x + blockIdx.x] = t2;
    }
}

// ---------------------------------------------------------------- plane regularisers' value
struct RegValueArgs {
    MomRegPlane p[MOM_REG_MAX_PLANES];
    unsigned block_start[MOM_REG_MAX_PLANES + 1];
    int count;
};

// the terms of one float column of a plane over rows [h_begin, h_end), added onto val in ascending h: the smoothness term of the
// row, then its |1 - p| term.  t(k) is the column's value in row h_begin + k (asked for only where that row exists)
template <typename Load>
__host__ __device__ __forceinline__ float reg_column(const MomRegPlane& P, int row, int h_begin, int h_end, Load t)
{
    const int H = P.H;
    const float cs = (H > 2 && P.w_smooth != 0.f) ? P.w_smooth / ((float)(H - 2) * (float)row) : 0.f;
    const float cl = P.w_l1 != 0.f ? P.w_l1 / ((float)H * (float)row) : 0.f;
    float val = 0.f;
#pragma unroll
    for (int k = 0; k < kRegRows; k++) {
        const int h = h_begin + k;
        if (h < h_end) {
            const float t0 = t(k);
            const float sh = h + 2 < H ? (t(k + 2) - 2.f * t(k + 1) + t0) : 0.f;
            val += cs * sh * sh;
            if (cl != 0.f) val += cl * fabsf(1.f - t0);
        }
    }
    return val;
}

__global__ void __launch_bounds__(256) reg_ordered_kernel(RegValueArgs a, float* __restrict__ part /* [gridDim.x] */)
{
    __shared__ float s_lane[256], s_wave[4];
    // plane_reg_kernel's mapping: workgroup `local` of a plane is (row block local / cblocks, column block local % cblocks), a lane
    // one float column of sixteen rows
    int pi = 0;
    while (pi + 1 < a.count && blockIdx.x >= a.block_start[pi + 1]) pi++;
    const MomRegPlane P = a.p[pi];
    const int row = P.W * 32;
    const int cblocks = (row + 255) / 256;
    const int local = blockIdx.x - a.block_start[pi];
    const int col = (local % cblocks) * 256 + threadIdx.x;
    const int h_begin = (local / cblocks) * kRegRows, h_end = min(P.H, h_begin + kRegRows);
    float val = 0.f;
    if (col < row) {
        const float* __restrict__ t = P.plane;
        float tv[kRegRows + 2];
#pragma unroll
        for (int k = 0; k < kRegRows + 2; k++) {
            const int h = h_begin + k;
            tv[k] = h < P.H ? t[(size_t)h * row + col] : 0.f;
        }
        val = reg_column(P, row, h_begin, h_end, [&](int k) { return tv[k]; });
    }
    const float tot = wg_fold(val, s_lane, s_wave);
    if (threadIdx.x == 0) part[blockIdx.x] = tot;
}

bool reg_plan(const MomRegPlane* planes, int count, RegValueArgs* a, unsigned* blocks_out)
{
    if (count < 0 || count > MOM_REG_MAX_PLANES || (count && !planes)) return false;
    unsigned blocks = 0;
    for (int i = 0; i < count; i++) {
        const MomRegPlane& p = planes[i];
        if (p.H < 1 || p.W < 1 || p.W > (1 << 24) || p.H > (1 << 24)) return false;
        if (a) { a->p[i] = p; a->block_start[i] = blocks; }
        const unsigned long long nb = (unsigned long long)((p.W * 32 + 255) / 256) * (unsigned long long)((p.H + kRegRows - 1) / kRegRows);
        if (nb + blocks > (1ull << 30)) return false;
        blocks += (unsigned)nb;
    }
    if (a) { a->block_start[count] = blocks; a->count = count; }
    *blocks_out = blocks;
    return true;
}

constexpr size_t kL1MaxN = (size_t)1 << 40;

bool scratch_ok(const void* scratch, size_t scratch_bytes, size_t need)
{
    return need == 0 || (scratch && (reinterpret_cast<uintptr_t>(scratch) & 3) == 0 && scratch_bytes >= need);
}

}  // namespace

extern "C" size_t mom_l1_loss_ordered_scratch_bytes(size_t n)
{
    return n > kL1MaxN ? 0 : 2 * ((n + kL1Share - 1) / kL1Share) * sizeof(float);
}

extern "C" int mom_l1_loss_ordered(size_t n, const float* img, const float* gt, float* dimg, float* sums2, void* scratch,
                                   size_t scratch_bytes, mom_stream_t stream)
{
    if (!img || !gt || !sums2 || n > kL1MaxN || !scratch_ok(scratch, scratch_bytes, mom_l1_loss_ordered_scratch_bytes(n))) return MOM_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const size_t groups = (n + kL1Share - 1) / kL1Share;
    float* part = static_cast<float*>(scratch);
    MomProfScope ps(MOM_P_L1, s);
    if (groups) {
        hipLaunchKernelGGL(l1_ordered_kernel, dim3((unsigned)groups), dim3(256), 0, s, n, img, gt, dimg, 1.0f / (float)n, part);
        if (hipGetLastError() != hipSuccess) return MOM_ELAUNCH;
    }
    hipLaunchKernelGGL(fold_kernel<float>, dim3(2), dim3(256), 0, s, groups, part, groups, sums2);     // (no group: +0.0 twice)
    return hipGetLastError() == hipSuccess ? MOM_OK : MOM_ELAUNCH;
}

extern "C" size_t mom_ssim_ordered_scratch_bytes(int C, int H, int W)
{
    if (C < 1 || H < 1 || W < 1) return 0;
    return (size_t)C * (size_t)((H + 15) / 16) * (size_t)((W + 15) / 16) * sizeof(float);
}

extern "C" int mom_ssim_sum_ordered(size_t blocks, const float* totals, double* sum, mom_stream_t stream)
{
    if (!sum || (blocks && !totals)) return MOM_EINVAL;
    hipLaunchKernelGGL(fold_kernel<double>, dim3(1), dim3(256), 0, (hipStream_t)stream, blocks, totals, blocks, sum);
    return hipGetLastError() == hipSuccess ? MOM_OK : MOM_ELAUNCH;
}

extern "C" size_t mom_plane_regulation_ordered_scratch_bytes(const MomRegPlane* planes, int count)
{
    unsigned blocks = 0;
    return reg_plan(planes, count, nullptr, &blocks) ? (size_t)blocks * sizeof(float) : 0;
}

extern "C" int mom_plane_regulation_ordered(const MomRegPlane* planes, int count, float* value, void* scratch, size_t scratch_bytes,
                                            mom_stream_t stream)
{
    RegValueArgs a;
    unsigned blocks = 0;
    if (!value || !reg_plan(planes, count, &a, &blocks)) return MOM_EINVAL;
    for (int i = 0; i < count; i++)
        if (!planes[i].plane) return MOM_EINVAL;
    if (!scratch_ok(scratch, scratch_bytes, (size_t)blocks * sizeof(float))) return MOM_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    float* part = static_cast<float*>(scratch);
    MomProfScope ps(MOM_P_REG, s);
    if (blocks) {
        hipLaunchKernelGGL(reg_ordered_kernel, dim3(blocks), dim3(256), 0, s, a, part);
        if (hipGetLastError() != hipSuccess) return MOM_ELAUNCH;
    }
    hipLaunchKernelGGL(fold_kernel<float>, dim3(1), dim3(256), 0, s, (size_t)blocks, part, (size_t)blocks, value);
    return hipGetLastError() == hipSuccess ? MOM_OK : MOM_ELAUNCH;
}

// ---------------------------------------------------------------- host twins (plain C++, no GPU)
extern "C" int mom_l1_loss_ordered_host(size_t n, const float* img, const float* gt, float* dimg, float* sums2)
{
    if (!img || !gt || !sums2 || n > kL1MaxN) return MOM_EINVAL;
    const size_t groups = (n + kL1Share - 1) / kL1Share;
    float* part = static_cast<float*>(malloc(sizeof(float) * (2 * groups + 1)));
    if (!part) return MOM_ECAPACITY;
    const float inv_n = 1.0f / (float)n;
    for (size_t g = 0; g < groups; g++) {
        float lane[2][256];
        for (int t = 0; t < 256; t++) {
            float a1 = 0.f, a2 = 0.f;
            for (int r = 0; r < 4; r++)
                for (int j = 0; j < 4; j++) {
                    const size_t i = g * kL1Share + (size_t)(r * 1024 + 4 * t + j);
                    if (i < n) {
                        const float gr = l1_one(img[i], gt[i], inv_n, a1, a2);
                        if (dimg) dimg[i] = gr;
                    }
                }
            lane[0][t] = a1;
            lane[1][t] = a2;
        }
        fold_host<float>(256, lane[0], &part[g]);
        fold_host<float>(256, lane[1], &part[groups + g]);
    }
    fold_host<float>(groups, part, &sums2[0]);
    fold_host<float>(groups, part + groups, &sums2[1]);
    free(part);
    return MOM_OK;
}

extern "C" int mom_ssim_sum_ordered_host(size_t blocks, const float* totals, double* sum)
{
    if (!sum || (blocks && !totals)) return MOM_EINVAL;
    fold_host<double>(blocks, totals, sum);
    return MOM_OK;
}

extern "C" int mom_plane_regulation_ordered_host(const MomRegPlane* planes, int count, float* value)
{
    RegValueArgs a;
    unsigned blocks = 0;
    if (!value || !reg_plan(planes, count, &a, &blocks)) return MOM_EINVAL;
    for (int i = 0; i < count; i++)
        if (!planes[i].plane) return MOM_EINVAL;
    float* part = static_cast<float*>(malloc(sizeof(float) * ((size_t)blocks + 1)));
    if (!part) return MOM_ECAPACITY;
    for (int pi = 0; pi < count; pi++) {
        const MomRegPlane& P = a.p[pi];
        const int row = P.W * 32, cblocks = (row + 255) / 256;
        for (unsigned b = a.block_start[pi]; b < a.block_start[pi + 1]; b++) {
            const int local = (int)(b - a.block_start[pi]);
            const int h_begin = (local / cblocks) * kRegRows, h_end = P.H < h_begin + kRegRows ? P.H : h_begin + kRegRows;
            float lane[256];
            for (int t = 0; t < 256; t++) {
                const int col = (local % cblocks) * 256 + t;
                lane[t] = col < row ? reg_column(P, row, h_begin, h_end, [&](int k) { return P.plane[(size_t)(h_begin + k) * row + col]; }) : 0.f;
            }
            fold_host<float>(256, lane, &part[b]);
        }
    }
    fold_host<float>(blocks, part, value);
    free(part);
    return MOM_OK;
}
