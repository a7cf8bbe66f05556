// Device helpers of the fused deformation MLP (v_mfma_f32_32x32x2_f32 layers with the weights resident in LDS), shared by
// deform_mlp.hip (MLP on stored features) and deform_field16.hip (HexPlane gather fused in front of it); the bf16 kernels
// (deform_field.hip, deform_bwd_b3.hip) use its tile layout and loads.
//
// KT is the number of 32-feature tiles of the trunk's input: 2 for 64 features, 1 for 32 (dnerf/eulerian_150_16: two HexPlane
// levels of 16 channels).  Only the trunk layer depends on it: h0 = W0 f + b0 with W0 [64][32 KT]; everything after relu(h0) is
// one code.  A tile's 32 features are ONE f32x16 per lane half, and the chains run over k ascending, so a 64-feature call on 32
// features padded with zero columns computes the bits of the 32-feature call -- it only adds + 0 * 0 terms at the end of each chain.
#pragma once
#include "mom_common.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kHid = 64;
constexpr int kWStride = 65;                         // LDS row stride of a weight matrix ([in][out])
constexpr int kWFloats = kHid * kWStride;            // one layer
constexpr int kStageStride = 33;                     // staging rows: [feature][32 gaussians + 1 pad]
constexpr int kStageFloats = kHid * kStageStride + 4 * 32;       // sA | dout[32][4]
constexpr int kDxWaves = 8;                          // waves per workgroup of the dx kernel (they share one copy of the weights)

// LDS map (floats)
constexpr int kLW = 0;                               // [4][64][65]
constexpr int kLB = kLW + 4 * kWFloats;              // [4][64]
constexpr int kLW2 = kLB + 4 * kHid;                 // [3][4][64] (rows >= nout are zero)
constexpr int kLB2 = kLW2 + 3 * 4 * kHid;            // [3][4]
constexpr int kLFwdTotal = kLB2 + 16;
constexpr int kLStage = kLFwdTotal;                  // [kDxWaves][kStageFloats]   (backward only)
constexpr int kLBwdTotal = kLStage + kDxWaves * kStageFloats;

__device__ __forceinline__ int fmap(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

struct MlpDev {
    const float *W0, *b0, *W1[3], *b1[3], *W2[3], *b2[3];
    float *dW0, *db0, *dW1[3], *db1[3], *dW2[3], *db2[3];
};

// Cooperative load of all weights into LDS (any workgroup size that is a multiple of 64, at least 256).  The four matrices
// are fetched as float4 and ALL of a thread's fetches are issued before its first LDS store: written as a plain copy loop the
// prologue paid one memory latency per iteration (16 k cycles of the forward kernel's 150 k).  W0 is [64][32 KT]: it fills rows
// 0 .. 32 KT - 1 of the first 64x64 slot, so that the heads' matrices sit where the map puts them at either width.
template <int KT>
__device__ __forceinline__ void load_weights(const MlpDev& m, float* __restrict__ lds)
{
    const int nth = (int)blockDim.x;
    constexpr int kIn = 32 * KT, kQ0 = kHid * kIn / 4;                       // 1024 (512) float4 of W0, then 3 x 1024 of the heads
    constexpr int kQuads = kQ0 + 3 * kHid * kHid / 4, kMaxPer = kQuads / 256; // 4096 (3584) in all; <= 16 (14) per thread
    float4 v[kMaxPer];
    float bias = 0.f;                                              // workgroups have at least 4 * kHid = 256 threads
    // Quad q of a thread.  With four equal matrices the layer is q >> 10 and indexes a table; with the narrower W0 in front it
    // is one more case.  The two fetch phases are written out, each as its kernels were timed: the compiled prologue follows the
    // form of the selection and even the place of the two tables' declarations.  (The table form for both widths: 7 instructions
    // fewer in deform_field16_fwd_kernel; the case form for both: 213 more in deform_fwd_kernel<2>.  Neither is what was measured.)
    if constexpr (KT == 2) {
        const float* Ws[4] = {m.W0, m.W1[0], m.W1[1], m.W1[2]};
        const float* bs[4] = {m.b0, m.b1[0], m.b1[1], m.b1[2]};
#pragma unroll
        for (int j = 0; j < kMaxPer; j++) {
            const int q = threadIdx.x + j * nth;                   // quad q: layer q >> 10, floats 4 (q & 1023) .. + 3 of it
            if (q < kQuads) v[j] = reinterpret_cast<const float4*>(Ws[q >> 10])[q & 1023];
        }
        if (threadIdx.x < 4 * kHid) bias = bs[threadIdx.x >> 6][threadIdx.x & 63];
    } else {
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
        if (threadIdx.x < 4 * kHid) bias = bs[threadIdx.x >> 6][threadIdx.x & 63];
    }
#pragma unroll
    for (int j = 0; j < kMaxPer; j++) {
        const int q = threadIdx.x + j * nth;
        if (q < kQuads) {
            float* d;
            if constexpr (KT == 2) {
                const int L = q >> 10, i = 4 * (q & 1023), o = i >> 6, k = i & 63;       // W[out][in] row-major -> lds[in][out], stride 65
                d = lds + kLW + L * kWFloats + k * kWStride + o;
            } else if (q < kQ0) {
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

// out[mt] += sum_k A(mt,k) in[k].  TRANS=false: A = W (out = W in).  TRANS=true: A = W^T (din = W^T dout).  The tile counts come
// from the operands: 2 x 2 for a 64x64 layer; the 32-feature trunk is in[1] -> out[2] forward and in[2] -> out[1] transposed.
template <bool TRANS, int KT, int MT>
__device__ __forceinline__ void layer64(const float* __restrict__ Wl, const f32x16 (&in)[KT], f32x16 (&out)[MT], int col, int h)
{
#pragma unroll
    for (int mt = 0; mt < MT; mt++)
#pragma unroll
        for (int kt = 0; kt < KT; kt++)
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const int k = 32 * kt + fmap(r, h), mrow = 32 * mt + col;
                const float a = TRANS ? Wl[mrow * kWStride + k] : Wl[k * kWStride + mrow];
                out[mt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, in[kt][r], out[mt], 0, 0, 0);
                if (r == 15) __builtin_amdgcn_sched_barrier(0);   // bound the scheduler's look-ahead (register budget)
            }
}

__device__ __forceinline__ void init_bias(const float* __restrict__ b, f32x16 (&t)[2], int h)
{
#pragma unroll
    for (int mt = 0; mt < 2; mt++)
#pragma unroll
        for (int r = 0; r < 16; r++) t[mt][r] = b[32 * mt + fmap(r, h)];
}
template <int MT>
__device__ __forceinline__ void zero_tile(f32x16 (&t)[MT])
{
#pragma unroll
    for (int mt = 0; mt < MT; mt++)
#pragma unroll
        for (int r = 0; r < 16; r++) t[mt][r] = 0.f;
}
__device__ __forceinline__ void relu_tile(f32x16 (&t)[2])
{
#pragma unroll
    for (int mt = 0; mt < 2; mt++)
#pragma unroll
        for (int r = 0; r < 16; r++) t[mt][r] = fmaxf(t[mt][r], 0.f);
}

// feat [P][32 KT] row-major <-> T layout (lane = gaussian column, registers = features: register 4q+j of tile kt and lane half h
// is feature 32kt+8q+4h+j, fmap)
template <int KT>
__device__ __forceinline__ void load_feat(const float* __restrict__ feat, int g, bool ok, int h, f32x16 (&t)[KT])
{
    const float* row = feat + (size_t)(ok ? g : 0) * (32 * KT);
#pragma unroll
    for (int kt = 0; kt < KT; kt++)
#pragma unroll
        for (int q = 0; q < 4; q++) {
            float4 v = *reinterpret_cast<const float4*>(row + 32 * kt + 8 * q + 4 * h);
            if (!ok) v = make_float4(0.f, 0.f, 0.f, 0.f);
            t[kt][4 * q + 0] = v.x;
            t[kt][4 * q + 1] = v.y;
            t[kt][4 * q + 2] = v.z;
            t[kt][4 * q + 3] = v.w;
        }
}
template <int KT>
__device__ __forceinline__ void store_feat(float* __restrict__ feat, int g, bool ok, int h, const f32x16 (&t)[KT])
{
    if (!ok) return;
    float* row = feat + (size_t)g * (32 * KT);
#pragma unroll
    for (int kt = 0; kt < KT; kt++)
#pragma unroll
        for (int q = 0; q < 4; q++)
            *reinterpret_cast<float4*>(row + 32 * kt + 8 * q + 4 * h) =
                make_float4(t[kt][4 * q + 0], t[kt][4 * q + 1], t[kt][4 * q + 2], t[kt][4 * q + 3]);
}

// thin output layer on the VALU: o[n] = b2[n] + sum_f W2[n][f] a1[f]; the two lane halves hold complementary feature
// subsets of the same gaussian, so they exchange partial sums
__device__ __forceinline__ void out_layer(const float* __restrict__ W2l, const float* __restrict__ b2l, const f32x16 (&a1)[2], int h,
                                          float (&o)[4])
{
#pragma unroll
    for (int n = 0; n < 4; n++) {
        float p = 0.f;
#pragma unroll
        for (int mt = 0; mt < 2; mt++)
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const float4 w = *reinterpret_cast<const float4*>(W2l + n * kHid + 32 * mt + 8 * q + 4 * h);
                p += w.x * a1[mt][4 * q] + w.y * a1[mt][4 * q + 1] + w.z * a1[mt][4 * q + 2] + w.w * a1[mt][4 * q + 3];
            }
        o[n] = p + __shfl_xor(p, 32) + b2l[n];
    }
}

// Optional activated copies of the forward's outputs (mom_deform_forward_activated): exp(scales), rots / |rots|,
// sigmoid(opacity_raw) -- what mom_activations_forward computes from the stored outputs, without its launch.
struct ActOut {
    float *scales, *rots, *opacity;
    const float* opacity_raw;
};

// stage a T-layout tile as [feature][gaussian] rows
__device__ __forceinline__ void stage_tile(float* __restrict__ s, const f32x16 (&t)[2], int col, int h)
{
#pragma unroll
    for (int mt = 0; mt < 2; mt++)
#pragma unroll
        for (int r = 0; r < 16; r++) s[(32 * mt + fmap(r, h)) * kStageStride + col] = t[mt][r];
}

}  // namespace

static int fill_dev(const MomDeformMLP* w, MlpDev* d)
{
    if (!w || !w->W0 || !w->b0) return MOM_EINVAL;
    d->W0 = w->W0; d->b0 = w->b0;
    d->dW0 = w->dW0; d->db0 = w->db0;
    for (int i = 0; i < 3; i++) {
        if (!w->W1[i] || !w->b1[i] || !w->W2[i] || !w->b2[i]) return MOM_EINVAL;
        d->W1[i] = w->W1[i]; d->b1[i] = w->b1[i]; d->W2[i] = w->W2[i]; d->b2[i] = w->b2[i];
        d->dW1[i] = w->dW1[i]; d->db1[i] = w->db1[i]; d->dW2[i] = w->dW2[i]; d->db2[i] = w->db2[i];
    }
    return MOM_OK;
}

