// Device helpers of the fused deformation MLP with a 32-feature trunk, shared by deform_mlp32.hip (MLP on stored features) and
// deform_field16.hip (HexPlane gather fused in front of it): the weights' LDS image and the trunk layer.
#pragma once
#include "deform_mlp_dev.h"

namespace {

constexpr int kIn32 = 32;                            // trunk input features of this file's kernels

// load_weights (deform_mlp_dev.h) for a [64,32] trunk matrix: the same LDS map, W0 in rows 0..31 of its slot.  All of a thread's
// fetches are issued before its first LDS store, as there.
__device__ __forceinline__ void load_weights32(const MlpDev& m, float* __restrict__ lds)
{
    const int nth = (int)blockDim.x;
    constexpr int kQ0 = kHid * kIn32 / 4;                                    // 512 float4 of W0, then 3 x 1024 of the heads
    constexpr int kQuads = kQ0 + 3 * kHid * kHid / 4, kMaxPer = kQuads / 256;  // 3584 in all; <= 14 per thread
    float4 v[kMaxPer];
#pragma unroll
    for (int j = 0; j < kMaxPer; j++) {
        const int q = threadIdx.x + j * nth;
        if (q < kQuads) {
            const int qq = q - kQ0, L = qq >> 10;
            const float* src = q < kQ0 ? m.W0 : (L == 0 ? m.W1[0] : (L == 1 ? m.W1[1] : m.W1[2]));
            v[j] = reinterpret_cast<const float4*>(src)[q < kQ0 ? q : (qq & 1023)];
        }
    }
    const float* bs[4] = {m.b0, m.b1[0], m.b1[1], m.b1[2]};
    float bias = 0.f;                                              // workgroups have at least 4 * kHid = 256 threads
    if (threadIdx.x < 4 * kHid) bias = bs[threadIdx.x >> 6][threadIdx.x & 63];
#pragma unroll
    for (int j = 0; j < kMaxPer; j++) {
        const int q = threadIdx.x + j * nth;
        if (q < kQuads) {
            float* d;
            if (q < kQ0) {
                const int i = 4 * q, o = i >> 5, k = i & 31;                 // W0[out][in], 32 wide -> lds[in][out], stride 65
                d = lds + kLW + k * kWStride + o;
            } else {
                const int qq = q - kQ0, L = 1 + (qq >> 10), i = 4 * (qq & 1023), o = i >> 6, k = i & 63;
                d = lds + kLW + L * kWFloats + k * kWStride + o;
            }
            d[0] = v[j].x; d[kWStride] = v[j].y; d[2 * kWStride] = v[j].z; d[3 * kWStride] = v[j].w;
        }
    }
    if (threadIdx.x < 4 * kHid) lds[kLB + threadIdx.x] = bias;
    for (int i = threadIdx.x; i < 3 * 4 * kHid; i += nth) {
        const int head = i >> 8, n = (i >> 6) & 3, f = i & 63;
        const int nout = head == 2 ? 4 : 3;
        lds[kLW2 + i] = n < nout ? m.W2[head][n * kHid + f] : 0.f;
    }
    if (threadIdx.x < 12) {
        const int head = threadIdx.x >> 2, n = threadIdx.x & 3;
        const int nout = head == 2 ? 4 : 3;
        lds[kLB2 + threadIdx.x] = n < nout ? m.b2[head][n] : 0.f;
    }
}

// trunk layer, h0[mt] += W0 f: layer64<false> without its second K tile (the chain of k = 0..31 in the same order)
__device__ __forceinline__ void trunk32(const float* __restrict__ Wl, const f32x16& in, f32x16 (&out)[2], int col, int h)
{
#pragma unroll
    for (int mt = 0; mt < 2; mt++)
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const float a = Wl[fmap(r, h) * kWStride + 32 * mt + col];
            out[mt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, in[r], out[mt], 0, 0, 0);
            if (r == 15) __builtin_amdgcn_sched_barrier(0);
        }
}

}  // namespace
