// The warp of the reference's video generator (thirdparty/StyleCineGAN), gfx950: Euler integration of a motion field, the summation
// splat, and the two of them fused with the blend, the normalisation, the hole filling and the crop of warp_one_level.
//
//   mom_euler_integrate   cinemagraph_utils.py:9-59     one launch, each lane walks its own pixel's chain
//   mom_softsplat_sum     softmax_splatting.py:8-53     the forward of _FunctionSoftsplat, the reference's [N,C,H,W] layout
//   mom_eulerian_blend    cinemagraph_utils.py:131-178 + joint_splatting.py:23-42: cut, reflection padding, both Euler chains, feature Z
//                         and Z of both halves splatted into ONE channel-last accumulator [P,P,C+1]
//   mom_eulerian_finish   softmax_splatting.py:341-344 + cinemagraph_utils.py:498-531, 77-83: divide, box mean at the blank pixels, crop
//
// All arithmetic is fp32 without contraction, operation by operation what the reference's torch ops and CUDA string compute, so the
// integrated displacements are the reference's bits and the splat differs from it by the order of the atomic adds alone.
//
// Where this file is deliberately NOT the reference (include/mom4d.h says the same):
//   * a chain that reaches a non-finite coordinate (NaN / inf motion) is invalid from that step on (displacement 0); the reference's
//     comparisons are all false for a NaN and it goes on to index with it.  Every gather index is clamped besides.
//   * a splat target whose coordinate is not below 2^30 in magnitude (or is NaN) is dropped before the conversion to int.
//
// The accumulator is channel-last so that the lanes of a wave add to contiguous bytes of one target texel: a wave-instruction of the
// blend covers runs of n consecutive floats, n = C+1 up to 64 channels and a balanced share of C+1 above (33 for C = 64: 132-byte runs).
#include "eulerian_dev.h"

namespace {

constexpr int kThreads = 256;
constexpr int kChunk = 32;            // channels the finish pass transposes at a time
constexpr int kBlendChunk = 64;       // the most accumulator channels the blend handles per pass (passes are balanced: 33 -> 33, 65 -> 33 + 32)

__global__ void __launch_bounds__(kThreads)
euler_integrate_kernel(int H, int W, int steps, int all_frames, const float* __restrict__ motion, float* __restrict__ disp)
{
    const size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x;
    const size_t plane = (size_t)H * W;
    if (i >= plane) return;
    const int px = (int)(i % W), py = (int)(i / W);
    auto fetch = [&](int ix, int iy, float& mx, float& my) {
        const size_t at = (size_t)iy * W + ix;
        mx = motion[at];
        my = motion[plane + at];
    };
    if (all_frames) {
        disp[i] = 0.0f;                // frame 0: the reference's zeros
        disp[plane + i] = 0.0f;
        walk_chain(px, py, W, H, steps, fetch, disp + i, 2 * plane, plane);
    } else {
        const float2 d = walk_chain(px, py, W, H, steps, fetch, (float*)nullptr, 0, 0);
        disp[i] = d.x;
        disp[plane + i] = d.y;
    }
}

__global__ void __launch_bounds__(kThreads)
softsplat_sum_kernel(size_t total, int C, int H, int W, const float* __restrict__ input, const float* __restrict__ flow,
                     float* __restrict__ output)
{
#pragma clang fp contract(off)
    const size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= total) return;
    const size_t plane = (size_t)H * W;
    const int x = (int)(i % W), y = (int)((i / W) % H);
    const size_t nc = i / plane, n = nc / C;
    const size_t pix = (size_t)y * W + x;
    const float ox = (float)x + flow[(n * 2) * plane + pix], oy = (float)y + flow[(n * 2 + 1) * plane + pix];
    const Corners c = corners(ox, oy, W, H);
    const float v = input[i];
    float* __restrict__ out = output + nc * plane;
    for (int k = 0; k < 4; k++)
        if (c.at[k] >= 0) atomicAdd(&out[c.at[k]], v * c.w[k]);
}

// ---- the fused blend -------------------------------------------------------------------------------------------------------------
// Geometry (eulerian_dev.h): the cut, the padding of the cut size s, the padded size P, where crop_padded_tensor starts.
struct Entry { int at[4]; float w[4]; float z; int src; };       // one (source pixel, half): 40 bytes

// Workgroup: kThreads / 2 consecutive source pixels of the padded domain, both halves; thread t walks the chain of pixel t / 2,
// half t % 2, and leaves its four targets in LDS.  Then the workgroup adds, per pass of up to kBlendChunk accumulator channels, every
// (entry, corner, channel) with the channel on the fastest lanes.  form 1 (small C): thread t adds its own entry's channels in a
// loop instead (no LDS round trip for the features; the lanes of a wave then add to neighbouring texels, one channel at a time).
template <int FORM>
__global__ void __launch_bounds__(kThreads)
eulerian_blend_kernel(int C, int S, Geometry g, int idx, int n_frames, float z_future, float z_past,
                      const float* __restrict__ feature, const float* __restrict__ motion, float* __restrict__ acc)
{
#pragma clang fp contract(off)
    __shared__ Entry entries[kThreads];
    __shared__ float tile[kBlendChunk][kThreads / 2 + 1];
    const int P = g.P, C1 = C + 1;
    const size_t npix = (size_t)P * P, plane = (size_t)S * S;
    const size_t pix = (size_t)blockIdx.x * (kThreads / 2) + threadIdx.x / 2;
    const int half = threadIdx.x & 1;
    Entry e;
    for (int k = 0; k < 4; k++) { e.at[k] = -1; e.w[k] = 0.0f; }
    e.z = half ? z_past : z_future;
    e.src = 0;
    if (pix < npix) {
        const int px = (int)(pix % P), py = (int)(pix / P);
        // joint_splatting.py:30-33: the second half's SOURCES lie P columns to the right with P taken off their x flow, so both halves
        // aim at columns [0, P) of the double canvas (blend_target reproduces the two fp32 roundings).  What lands in columns [P, 2P)
        // the reference crops away (output_size): dropped here like any target outside the canvas
        const float2 o = blend_target(px, py, half, S, g, idx, n_frames, motion);
        const Corners c = corners(o.x, o.y, P, P);
        for (int k = 0; k < 4; k++) { e.at[k] = c.at[k]; e.w[k] = c.w[k]; }
        e.src = (reflect(py - g.pad, g.s) + g.cut) * S + (reflect(px - g.pad, g.s) + g.cut);
    }
    if (FORM == 1) {
        if (pix >= npix) return;
        for (int c = 0; c < C1; c++) {
            const float v = (c < C ? feature[(size_t)c * plane + e.src] : 1.0f) * e.z;
            for (int k = 0; k < 4; k++)
                if (e.at[k] >= 0) atomicAdd(&acc[(size_t)e.at[k] * C1 + c], v * e.w[k]);
        }
        return;
    }
    entries[threadIdx.x] = e;
    const int passes = (C1 + kBlendChunk - 1) / kBlendChunk, width = (C1 + passes - 1) / passes;
    for (int c0 = 0; c0 < C1; c0 += width) {
        const int cn = C1 - c0 < width ? C1 - c0 : width;
        __syncthreads();                                          // entries written / the last pass has read the tile
        for (int i = threadIdx.x; i < cn * (kThreads / 2); i += kThreads) {
            const int p = i % (kThreads / 2), c = c0 + i / (kThreads / 2);
            tile[i / (kThreads / 2)][p] = c < C ? feature[(size_t)c * plane + entries[2 * p].src] : 1.0f;
        }
        __syncthreads();
        const int items = kThreads * 4 * cn;
        for (int i = threadIdx.x; i < items; i += kThreads) {
            const int c = i % cn, k = (i / cn) & 3, en = i / (cn * 4);
            const int at = entries[en].at[k];
            if (at >= 0) {
                const float v = tile[c][en >> 1] * entries[en].z;
                atomicAdd(&acc[(size_t)at * C1 + c0 + c], v * entries[en].w[k]);
            }
        }
    }
}

// ---- normalise, fill the blank pixels, crop --------------------------------------------------------------------------------------
// Workgroup: 64 consecutive pixels of one output row; per pass kChunk channels: read channel-fastest, write pixel-fastest through LDS.
__global__ void __launch_bounds__(kThreads)
eulerian_finish_kernel(int C, int P, int out0, int out_size, int inpaint, const float* __restrict__ acc, float* __restrict__ out,
                       uint8_t* __restrict__ blank)
{
#pragma clang fp contract(off)
    __shared__ float tile[64][kChunk + 1];
    const int C1 = C + 1;
    const int y = blockIdx.y, x0 = blockIdx.x * 64;
    const float w49 = 1.0f / 49.0f;
    for (int c0 = 0; c0 < C; c0 += kChunk) {
        const int cn = C - c0 < kChunk ? C - c0 : kChunk;
        __syncthreads();
        for (int i = threadIdx.x; i < 64 * kChunk; i += kThreads) {
            const int c = i % kChunk, p = i / kChunk, x = x0 + p;
            if (c >= cn || x >= out_size) continue;
            const int ay = y + out0, ax = x + out0;
            const size_t tex = ((size_t)ay * P + ax) * C1;
            const float m = acc[tex + C];
            float v;
            if (m != 0.0f) {
                v = acc[tex + c0 + c] / m;
            } else if (!inpaint) {
                v = acc[tex + c0 + c];                                // softmax_splatting.py:343: the divisor becomes 1
            } else {
                // feature_inpaint_conv: conv2d of the normalised map with 49 weights of 1/49, zero padding 3
                v = 0.0f;
                for (int dy = -3; dy <= 3; dy++) {
                    const int ny = ay + dy;
                    if (ny < 0 || ny >= P) continue;
                    for (int dx = -3; dx <= 3; dx++) {
                        const int nx = ax + dx;
                        if (nx < 0 || nx >= P) continue;
                        const size_t nt = ((size_t)ny * P + nx) * C1;
                        const float nm = acc[nt + C];
                        v = v + (acc[nt + c0 + c] / (nm == 0.0f ? 1.0f : nm)) * w49;
                    }
                }
            }
            tile[p][c] = v;
            if (blank && c0 == 0 && c == 0) blank[(size_t)y * out_size + x] = m == 0.0f;
        }
        __syncthreads();
        for (int i = threadIdx.x; i < 64 * cn; i += kThreads) {
            const int p = i % 64, c = i / 64, x = x0 + p;
            if (x < out_size) out[((size_t)(c0 + c) * out_size + y) * out_size + x] = tile[p][c];
        }
    }
}

}  // namespace

extern "C" int mom_euler_integrate(int H, int W, int steps, int all_frames, const float* motion, float* disp, mom_stream_t stream)
{
    if (H < 1 || W < 1 || steps < 0 || !motion || !disp) return MOM_EINVAL;
    if ((size_t)H * W >= ((size_t)1 << 31)) return MOM_EINVAL;
    const size_t blocks = ((size_t)H * W + kThreads - 1) / kThreads;
    hipLaunchKernelGGL(euler_integrate_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, (hipStream_t)stream, H, W, steps,
                       all_frames != 0, motion, disp);
    return hipGetLastError() == hipSuccess ? MOM_OK : MOM_ELAUNCH;
}

extern "C" int mom_softsplat_sum(int N, int C, int H, int W, const float* input, const float* flow, float* output, mom_stream_t stream)
{
    if (N < 1 || C < 1 || H < 1 || W < 1 || !input || !flow || !output) return MOM_EINVAL;
    if ((size_t)H * W >= ((size_t)1 << 31)) return MOM_EINVAL;
    const size_t total = (size_t)N * C * H * W, blocks = (total + kThreads - 1) / kThreads;
    if (blocks >= ((size_t)1 << 31)) return MOM_EINVAL;
    hipLaunchKernelGGL(softsplat_sum_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, (hipStream_t)stream, total, C, H, W, input,
                       flow, output);
    return hipGetLastError() == hipSuccess ? MOM_OK : MOM_ELAUNCH;
}

extern "C" int mom_eulerian_geometry(int S, int* cut, int* pad, int* padded, int* crop0)
{
    Geometry g;
    if (!geometry(S, &g)) return MOM_EINVAL;
    if (cut) *cut = g.cut;
    if (pad) *pad = g.pad;
    if (padded) *padded = g.P;
    if (crop0) *crop0 = g.crop0;
    return MOM_OK;
}

extern "C" int mom_eulerian_blend(int C, int H, int W, int idx, int n_frames, int form, const float* feature, const float* motion,
                                  float* acc, mom_stream_t stream)
{
    Geometry g;
    if (C < 1 || H != W || n_frames < 2 || idx < 0 || idx >= n_frames || form < 0 || form > 1 || !feature || !motion || !acc)
        return MOM_EINVAL;
    if (!geometry(H, &g)) return MOM_EINVAL;
    const size_t npix = (size_t)g.P * g.P;
    if (npix * (size_t)(C + 1) >= ((size_t)1 << 40)) return MOM_EINVAL;
    if (hipMemsetAsync(acc, 0, npix * (size_t)(C + 1) * sizeof(float), (hipStream_t)stream) != hipSuccess) return MOM_ELAUNCH;
    float z_future, z_past;
    blend_z(idx, n_frames, &z_future, &z_past);
    const size_t blocks = (npix + kThreads / 2 - 1) / (kThreads / 2);
    if (form == 1)
        hipLaunchKernelGGL(eulerian_blend_kernel<1>, dim3((unsigned)blocks), dim3(kThreads), 0, (hipStream_t)stream, C, H, g, idx,
                           n_frames, z_future, z_past, feature, motion, acc);
    else
        hipLaunchKernelGGL(eulerian_blend_kernel<0>, dim3((unsigned)blocks), dim3(kThreads), 0, (hipStream_t)stream, C, H, g, idx,
                           n_frames, z_future, z_past, feature, motion, acc);
    return hipGetLastError() == hipSuccess ? MOM_OK : MOM_ELAUNCH;
}

extern "C" int mom_eulerian_finish(int C, int S, int full, const float* acc, float* out, uint8_t* blank, mom_stream_t stream)
{
    Geometry g;
    if (C < 1 || !acc || !out) return MOM_EINVAL;
    if (!geometry(S, &g)) return MOM_EINVAL;
    const int out0 = full ? 0 : g.crop0, out_size = full ? g.P : S;
    if (out_size > 65535) return MOM_EINVAL;                      // the row is a grid axis
    hipLaunchKernelGGL(eulerian_finish_kernel, dim3((unsigned)((out_size + 63) / 64), (unsigned)out_size), dim3(kThreads), 0,
                       (hipStream_t)stream, C, g.P, out0, out_size, full ? 0 : 1, acc, out, blank);
    return hipGetLastError() == hipSuccess ? MOM_OK : MOM_ELAUNCH;
}
