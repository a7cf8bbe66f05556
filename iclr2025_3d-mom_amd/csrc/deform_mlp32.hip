// Fused deformation MLP with a 32-feature trunk (dnerf/eulerian_150_16: two HexPlane levels of 16 channels), fp32, gfx950.
//
// The network of deform_mlp.hip with one difference: the trunk layer reads 32 features,
//     h0 = W0 f + b0,   W0 [64,32], f [32]
// and everything after relu(h0) -- the three heads, the residual adds, the activated copies -- is that file's.  These are the
// counterparts of its three f32 kernels, in the same formulation: transposed MFMA (v_mfma_f32_32x32x2_f32, weights the A operand,
// the Gaussian on the lane), the same k-ascending fma chain (over k = 0..31 in the trunk layer: a tile's 32 features are ONE f32x16
// per lane half, and a 64-feature call on the same features padded with zero columns computes the same bits -- it only adds
// + 0 * 0 terms at the end of each chain), W0 in LDS as [32][64] with the 65-float row stride (the slot of the 64x64 trunk matrix,
// half used, so that the heads' matrices sit where deform_mlp_dev.h's map puts them), a0_save [P,64].
//
// Backward: the two-kernel f32 form only.  dx back-propagates dH0 through W0^T to dfeat [P,32]; dW forms dW0 [64,32] = dH0^T feat
// with feat [P,32].  There the B operand's lane is still the input feature and its lane half the K slot (one of two Gaussians):
// two consecutive 128-byte feature rows are ONE 256-byte load of all 64 lanes, so the trunk layer issues one operand load and two
// MFMAs per K step where the 64-feature kernel issues two and four, and no lane is masked.
//
// There is no bf16 one-kernel backward for this shape (deform_bwd_b3.hip is 64 features only): a 32-feature call runs the two f32
// kernels whatever MOM_MLP_BWD names -- unset, empty, "b3" or "split" -- and any other value is MOM_EINVAL as for 64 features.
//
// The entry points here are the *_n forms of the ABI (include/mom4d.h): in_features = 64 forwards to deform_mlp.hip's entry
// points unchanged, 32 runs the kernels below, anything else is MOM_EINVAL.
#include "deform_mlp32_dev.h"
#include <string.h>

namespace {

// its transpose, df += W0^T dH0: layer64<true> without its second M tile (the 32 input features are the tile's rows)
__device__ __forceinline__ void trunk32_t(const float* __restrict__ Wl, const f32x16 (&in)[2], f32x16& out, int col, int h)
{
#pragma unroll
    for (int kt = 0; kt < 2; kt++)
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const float a = Wl[col * kWStride + 32 * kt + fmap(r, h)];
            out = __builtin_amdgcn_mfma_f32_32x32x2f32(a, in[kt][r], out, 0, 0, 0);
            if (r == 15) __builtin_amdgcn_sched_barrier(0);
        }
}

// feat [P][32] row-major <-> T layout: register 4q+j of lane half h is feature 8q+4h+j (fmap)
__device__ __forceinline__ void load_feat32(const float* __restrict__ feat, int g, bool ok, int h, f32x16& t)
{
    const float* row = feat + (size_t)(ok ? g : 0) * kIn32;
#pragma unroll
    for (int q = 0; q < 4; q++) {
        float4 v = *reinterpret_cast<const float4*>(row + 8 * q + 4 * h);
        if (!ok) v = make_float4(0.f, 0.f, 0.f, 0.f);
        t[4 * q + 0] = v.x;
        t[4 * q + 1] = v.y;
        t[4 * q + 2] = v.z;
        t[4 * q + 3] = v.w;
    }
}
__device__ __forceinline__ void store_feat32(float* __restrict__ feat, int g, bool ok, int h, const f32x16& t)
{
    if (!ok) return;
    float* row = feat + (size_t)g * kIn32;
#pragma unroll
    for (int q = 0; q < 4; q++)
        *reinterpret_cast<float4*>(row + 8 * q + 4 * h) = make_float4(t[4 * q + 0], t[4 * q + 1], t[4 * q + 2], t[4 * q + 3]);
}

// deform_fwd_kernel with the 32-feature trunk: one workgroup of sixteen waves per CU around one copy of the weights
__global__ void __launch_bounds__(1024)
deform32_fwd_kernel(MlpDev m, int P, int tiles, const float* __restrict__ feat, const float* __restrict__ xyz,
                    const float* __restrict__ scaling, const float* __restrict__ rotation, const float* __restrict__ flow,
                    float flow_coef, float* __restrict__ pts, float* __restrict__ scales, float* __restrict__ rots,
                    float* __restrict__ a0_save, ActOut act)
{
    extern __shared__ float lds[];
    load_weights32(m, lds);
    __syncthreads();
    const int lane = threadIdx.x & 63, col = lane & 31, h = lane >> 5;
    // a contiguous, equal (+-1) share of the tiles per workgroup, dealt to its waves (see deform_fwd_kernel)
    const int t_begin = (int)((long long)tiles * blockIdx.x / gridDim.x), t_end = (int)((long long)tiles * (blockIdx.x + 1) / gridDim.x);
    const int t_first = t_begin + (int)(threadIdx.x >> 6), t_step = (int)(blockDim.x >> 6);
    for (int t = t_first; t < t_end; t += t_step) {
        const int g = t * 32 + col;
        const bool ok = g < P;
        f32x16 a0[2];
        {
            f32x16 x;
            load_feat32(feat, g, ok, h, x);
            init_bias(lds + kLB, a0, h);
            trunk32(lds + kLW, x, a0, col, h);
        }
        relu_tile(a0);
        if (a0_save) store_feat(a0_save, g, ok, h, a0);     // relu(h0) [P,64], reused by the backward kernels
#pragma nounroll
        for (int head = 0; head < 3; head++) {
            f32x16 h1[2];
            init_bias(lds + kLB + (1 + head) * kHid, h1, h);
            layer64<false>(lds + kLW + (1 + head) * kWFloats, a0, h1, col, h);
            relu_tile(h1);
            float o[4];
            out_layer(lds + kLW2 + head * 4 * kHid, lds + kLB2 + head * 4, h1, h, o);
            if (h == 0 && ok) {
                if (head == 0) {
#pragma unroll
                    for (int k = 0; k < 3; k++) pts[3 * g + k] = xyz[3 * g + k] + (o[k] + flow_coef * flow[3 * g + k]);
                } else if (head == 1) {
#pragma unroll
                    for (int k = 0; k < 3; k++) scales[3 * g + k] = scaling[3 * g + k] + o[k];
                } else {
#pragma unroll
                    for (int k = 0; k < 4; k++) rots[4 * g + k] = rotation[4 * g + k] + o[k];
                }
            }
        }
    }
    // activated copies after the tile loop, each lane re-reading what it stored itself (see deform_fwd_kernel)
    if (act.scales || act.rots || act.opacity) {
        for (int t = t_first; t < t_end; t += t_step) {
            const int g = t * 32 + col;
            if (h != 0 || g >= P) continue;
            if (act.scales) {
#pragma unroll
                for (int k = 0; k < 3; k++) act.scales[3 * g + k] = expf(scales[3 * g + k]);
            }
            if (act.rots) {
                const float4 q = *reinterpret_cast<const float4*>(rots + 4 * g);
                const float n = mom_quat_norm(q.x, q.y, q.z, q.w);
                *reinterpret_cast<float4*>(act.rots + 4 * g) = make_float4(q.x / n, q.y / n, q.z / n, q.w / n);
            }
            if (act.opacity) act.opacity[g] = mom_sigmoid(act.opacity_raw[g]);
        }
    }
}

// ---------------------------------------------------------------------------------------------- backward
// (A) deform_bwd_dx_kernel with the 32-feature trunk: dH for the four layers [4][P][64], dfeat [P,32], output-layer gradients
__global__ void __launch_bounds__(64 * kDxWaves)
deform32_bwd_dx_kernel(MlpDev m, int P, int tiles, const float* __restrict__ a0g, const float* __restrict__ dpts,
                       const float* __restrict__ dscales, const float* __restrict__ drots, float* __restrict__ dfeat,
                       float* __restrict__ dH /* [4][P][64] */)
{
    extern __shared__ float lds[];
    load_weights32(m, lds);
    __syncthreads();
    const int lane = threadIdx.x & 63, col = lane & 31, h = lane >> 5, wv = threadIdx.x >> 6;
    float* sA = lds + kLStage + wv * kStageFloats;
    float* sD = sA + kHid * kStageStride;              // dout[32 gaussians][4]
    const int t_begin = (int)((long long)tiles * blockIdx.x / gridDim.x), t_end = (int)((long long)tiles * (blockIdx.x + 1) / gridDim.x);
    const int t_first = t_begin + (int)(threadIdx.x >> 6), t_step = (int)(blockDim.x >> 6);
    const size_t PH = (size_t)P * kHid;
    float dW2[3][4], db2[3];                           // lane = feature; db2: lane n < 4 holds output n
#pragma unroll
    for (int k = 0; k < 3; k++) { db2[k] = 0.f; dW2[k][0] = dW2[k][1] = dW2[k][2] = dW2[k][3] = 0.f; }

    // the next tile's trunk activations are requested while this tile is worked on
    f32x16 a0n[2];
    if (t_first < t_end) load_feat(a0g, t_first * 32 + col, t_first * 32 + col < P, h, a0n);
    for (int t = t_first; t < t_end; t += t_step) {
        const int g = t * 32 + col;
        const bool ok = g < P;
        f32x16 a0[2], dA0[2];
        a0[0] = a0n[0];
        a0[1] = a0n[1];
        if (t + t_step < t_end) load_feat(a0g, (t + t_step) * 32 + col, (t + t_step) * 32 + col < P, h, a0n);
        zero_tile(dA0);
#pragma nounroll
        for (int head = 0; head < 3; head++) {   // rolled on purpose, as in deform_bwd_dx_kernel
            const int nout = head == 2 ? 4 : 3;
            f32x16 a1[2];
            init_bias(lds + kLB + (1 + head) * kHid, a1, h);
            layer64<false>(lds + kLW + (1 + head) * kWFloats, a0, a1, col, h);
            relu_tile(a1);
            const float* __restrict__ dsrc = head == 0 ? dpts : (head == 1 ? dscales : drots);
            float dout[4];
#pragma unroll
            for (int k = 0; k < 4; k++) dout[k] = (ok && k < nout) ? dsrc[nout * g + k] : 0.f;
            __builtin_amdgcn_wave_barrier();
            stage_tile(sA, a1, col, h);
            if (h == 0) *reinterpret_cast<float4*>(sD + 4 * col) = make_float4(dout[0], dout[1], dout[2], dout[3]);
            __builtin_amdgcn_wave_barrier();
            {   // output layer: dW2[n][f] += sum_g dout[n][g] a1[f][g]; db2[n] += sum_g dout[n][g]   (lane = f)
                float w0 = 0.f, w1 = 0.f, w2 = 0.f, w3 = 0.f, bsum = 0.f;
#pragma unroll
                for (int gg = 0; gg < 32; gg++) {
                    const float v = sA[lane * kStageStride + gg];
                    const float4 d = *reinterpret_cast<const float4*>(sD + 4 * gg);
                    w0 += d.x * v; w1 += d.y * v; w2 += d.z * v; w3 += d.w * v;
                    bsum += sD[4 * gg + (lane & 3)];
                }
                if (head == 0) { dW2[0][0] += w0; dW2[0][1] += w1; dW2[0][2] += w2; dW2[0][3] += w3; db2[0] += bsum; }
                else if (head == 1) { dW2[1][0] += w0; dW2[1][1] += w1; dW2[1][2] += w2; dW2[1][3] += w3; db2[1] += bsum; }
                else { dW2[2][0] += w0; dW2[2][1] += w1; dW2[2][2] += w2; dW2[2][3] += w3; db2[2] += bsum; }
            }
            // dH1 = relu'(h1) * W2^T dout, in place of a1
            const float* __restrict__ W2l = lds + kLW2 + head * 4 * kHid;
#pragma unroll
            for (int mt = 0; mt < 2; mt++)
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const float4 wa = *reinterpret_cast<const float4*>(W2l + 0 * kHid + 32 * mt + 8 * q + 4 * h);
                    const float4 wb = *reinterpret_cast<const float4*>(W2l + 1 * kHid + 32 * mt + 8 * q + 4 * h);
                    const float4 wc = *reinterpret_cast<const float4*>(W2l + 2 * kHid + 32 * mt + 8 * q + 4 * h);
                    const float4 wd = *reinterpret_cast<const float4*>(W2l + 3 * kHid + 32 * mt + 8 * q + 4 * h);
                    const float v0 = wa.x * dout[0] + wb.x * dout[1] + wc.x * dout[2] + wd.x * dout[3];
                    const float v1 = wa.y * dout[0] + wb.y * dout[1] + wc.y * dout[2] + wd.y * dout[3];
                    const float v2 = wa.z * dout[0] + wb.z * dout[1] + wc.z * dout[2] + wd.z * dout[3];
                    const float v3 = wa.w * dout[0] + wb.w * dout[1] + wc.w * dout[2] + wd.w * dout[3];
                    a1[mt][4 * q + 0] = a1[mt][4 * q + 0] > 0.f ? v0 : 0.f;
                    a1[mt][4 * q + 1] = a1[mt][4 * q + 1] > 0.f ? v1 : 0.f;
                    a1[mt][4 * q + 2] = a1[mt][4 * q + 2] > 0.f ? v2 : 0.f;
                    a1[mt][4 * q + 3] = a1[mt][4 * q + 3] > 0.f ? v3 : 0.f;
                }
            store_feat(dH + (size_t)(1 + head) * PH, g, ok, h, a1);
            layer64<true>(lds + kLW + (1 + head) * kWFloats, a1, dA0, col, h);   // dA0 += W1^T dH1
        }
        // through the ReLU between trunk and heads
#pragma unroll
        for (int mt = 0; mt < 2; mt++)
#pragma unroll
            for (int r = 0; r < 16; r++) dA0[mt][r] = a0[mt][r] > 0.f ? dA0[mt][r] : 0.f;
        store_feat(dH, g, ok, h, dA0);
        {
            f32x16 df;
#pragma unroll
            for (int r = 0; r < 16; r++) df[r] = 0.f;
            trunk32_t(lds + kLW, dA0, df, col, h);      // dfeat = W0^T dH0, 32 rows
            store_feat32(dfeat, g, ok, h, df);
        }
    }
    // output-layer gradients: combine the waves in LDS, one atomic per element per workgroup
    __syncthreads();
    float* R = lds;
    for (int i = threadIdx.x; i < 12 * kHid + 16; i += blockDim.x) R[i] = 0.f;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 3; k++) {
#pragma unroll
        for (int n = 0; n < 4; n++) atomicAdd(&R[(k * 4 + n) * kHid + lane], dW2[k][n]);
        if (lane < 4) atomicAdd(&R[12 * kHid + k * 4 + lane], db2[k]);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 12 * kHid; i += blockDim.x) {
        const int k = i >> 8, n = (i >> 6) & 3, f = i & 63;
        const int nout = k == 2 ? 4 : 3;
        const float v = R[i];
        if (n < nout && v != 0.f) atomicAdd(&m.dW2[k][n * kHid + f], v);
    }
    if (threadIdx.x < 12) {
        const int k = threadIdx.x >> 2, n = threadIdx.x & 3;
        const int nout = k == 2 ? 4 : 3;
        const float v = R[12 * kHid + threadIdx.x];
        if (n < nout && v != 0.f) atomicAdd(&m.db2[k][n], v);
    }
}

// (B) One layer's weight gradient over one wave's range of Gaussians: dW[o][i] = sum_g dH[g][o] X[g][i], db[o] = sum_g dH[g][o].
// KT = tiles of 32 input features: 2 for the heads (X = a0 [P,64], as deform_bwd_dw_kernel), 1 for the trunk (X = feat [P,32]).
// The B operand's lane half is the K slot, a Gaussian of the pair g0 + 2u + {0,1}: with KT = 1 the two halves read two consecutive
// 128-byte rows, one 256-byte load of the whole wave.
template <int KT>
__device__ __forceinline__ void dw_layer(const float* __restrict__ xa, const float* __restrict__ dHl, int g_begin, int g_end,
                                         float* __restrict__ dst, float* __restrict__ dbs, float* __restrict__ R)
{
    constexpr int kIn = 32 * KT;
    const int lane = threadIdx.x & 63, col = lane & 31, h = lane >> 5;
    f32x16 dW[2][KT];
    float db[2] = {0.f, 0.f};
#pragma unroll
    for (int mt = 0; mt < 2; mt++)
#pragma unroll
        for (int kt = 0; kt < KT; kt++)
#pragma unroll
            for (int r = 0; r < 16; r++) dW[mt][kt][r] = 0.f;
    // operand loads double buffered by hand and issued unconditionally (rows past the end are clamped and masked by `ok`), as in
    // deform_bwd_dw_kernel
    constexpr int UNR = 4;
    struct Operands {
        float x[UNR][KT], da[UNR][2];
        bool ok[UNR];
    };
    auto load = [&](Operands& o, int g0) {
#pragma unroll
        for (int u = 0; u < UNR; u++) {
            const int g = g0 + 2 * u + h;               // K slot of this lane half
            const bool ok = g < g_end;
            o.ok[u] = ok;
            const size_t row = (size_t)(ok ? g : g_begin);
#pragma unroll
            for (int kt = 0; kt < KT; kt++) o.x[u][kt] = xa[row * kIn + 32 * kt + col];
            o.da[u][0] = dHl[row * kHid + col];
            o.da[u][1] = dHl[row * kHid + 32 + col];
        }
    };
    auto compute = [&](const Operands& o) {
#pragma unroll
        for (int u = 0; u < UNR; u++) {
            const float a_lo = o.ok[u] ? o.da[u][0] : 0.f, a_hi = o.ok[u] ? o.da[u][1] : 0.f;
            db[0] += a_lo;
            db[1] += a_hi;
#pragma unroll
            for (int kt = 0; kt < KT; kt++) dW[0][kt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a_lo, o.x[u][kt], dW[0][kt], 0, 0, 0);
#pragma unroll
            for (int kt = 0; kt < KT; kt++) dW[1][kt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a_hi, o.x[u][kt], dW[1][kt], 0, 0, 0);
        }
    };
    if (g_begin < g_end) {
        Operands cur, nxt;
        load(cur, g_begin);
        for (int g0 = g_begin; g0 < g_end; g0 += 2 * UNR) {
            load(nxt, g0 + 2 * UNR);
            __builtin_amdgcn_sched_barrier(0);
            compute(cur);
            __builtin_amdgcn_sched_barrier(0);
            cur = nxt;
        }
    }
    // the four waves take turns on the shared tile with plain read-add-write, then one float atomic per weight per workgroup
    const int wv = threadIdx.x >> 6;
    const float b_lo = db[0] + __shfl_xor(db[0], 32), b_hi = db[1] + __shfl_xor(db[1], 32);
#pragma unroll 1
    for (int turn = 0; turn < 4; turn++) {
        __syncthreads();
        if (wv == turn) {
#pragma unroll
            for (int mt = 0; mt < 2; mt++)
#pragma unroll
                for (int kt = 0; kt < KT; kt++)
#pragma unroll
                    for (int r = 0; r < 16; r++) {     // tile row = out feature 32mt+fmap(r,h), column = in feature 32kt+col
                        float* a = &R[(32 * mt + fmap(r, h)) * kIn + 32 * kt + col];
                        *a = (turn == 0 ? 0.f : *a) + dW[mt][kt][r];
                    }
            if (h == 0) {
                float* a = &R[kHid * kIn + col];
                a[0] = (turn == 0 ? 0.f : a[0]) + b_lo;
                a[32] = (turn == 0 ? 0.f : a[32]) + b_hi;
            }
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < kHid * kIn; i += 256) {
        const float v = R[i];
        if (v != 0.f) atomicAdd(&dst[i], v);
    }
    if (threadIdx.x < kHid) {
        const float v = R[kHid * kIn + threadIdx.x];
        if (v != 0.f) atomicAdd(&dbs[threadIdx.x], v);
    }
}

// deform_bwd_dw_kernel with the 32-feature trunk: a wave takes ONE layer of its range of Gaussians, and the grid is numbered so
// that the four layers of a range land on the same XCD (see there).  Layer 0 (dW0 [64,32]) has half the MFMAs of the others.
__global__ void __launch_bounds__(256)
deform32_bwd_dw_kernel(MlpDev m, int P, int chunk, const float* __restrict__ feat, const float* __restrict__ a0g,
                       const float* __restrict__ dH, int ny)
{
    extern __shared__ float lds[];                     // [64][64] reduction scratch + [64] bias
    const int lin = blockIdx.x, run = 8 * ny;
    const int bx = (lin / run) * 8 + (lin % run) % 8, L = (lin % run) / 8;      // range of Gaussians, layer
    const int wave = (bx * 256 + threadIdx.x) >> 6;
    const int g_begin = wave * chunk, g_end = min(P, g_begin + chunk);   // chunk is even
    const float* __restrict__ dHl = dH + (size_t)L * P * kHid;
    if (L == 0)
        dw_layer<1>(feat, dHl, g_begin, g_end, m.dW0, m.db0, lds);
    else
        dw_layer<2>(a0g, dHl, g_begin, g_end, m.dW1[L - 1], m.db1[L - 1], lds);
}

int forward32(const MomDeformMLP* w, int P, const float* feat, const float* xyz, const float* scaling, const float* rotation,
              const float* scene_flow, float flow_coef, float* pts, float* scales, float* rots, float* a0_save, const float* opacity_raw,
              float* scales_act, float* rots_act, float* opacity_act, mom_stream_t stream)
{
    if (P < 0) return MOM_EINVAL;
    if (P == 0) return MOM_OK;
    if (!feat || !xyz || !scaling || !rotation || !scene_flow || !pts || !scales || !rots) return MOM_EINVAL;
    if ((opacity_act != nullptr) != (opacity_raw != nullptr)) return MOM_EINVAL;
    MlpDev d;
    int rc = fill_dev(w, &d);
    if (rc) return rc;
    const int tiles = (P + 31) / 32;
    const int block = 1024;                            // one workgroup per CU, sixteen waves around one copy of the weights
    const int blocks = tiles < 256 ? tiles : 256;      // never more workgroups than tiles: a small problem is spread over the CUs
    const size_t lds_bytes = sizeof(float) * kLFwdTotal;
    if (!mom_lds_limit<deform32_fwd_kernel>(lds_bytes)) return MOM_ELAUNCH;
    const ActOut act = {scales_act, rots_act, opacity_act, opacity_raw};
    MomProfScope ps(MOM_P_MLP_FWD, (hipStream_t)stream);
    hipLaunchKernelGGL(deform32_fwd_kernel, dim3(blocks), dim3(block), lds_bytes, (hipStream_t)stream, d, P, tiles, feat, xyz, scaling,
                       rotation, scene_flow, flow_coef, pts, scales, rots, a0_save, act);
    return hipGetLastError() == hipSuccess ? MOM_OK : MOM_ELAUNCH;
}

int backward32(const MomDeformMLP* w, int P, const float* feat, const float* a0, const float* dpts, const float* dscales,
               const float* drots, float* dfeat, void* scratch, mom_stream_t stream, mom_stream_t dw_stream)
{
    if (P < 0) return MOM_EINVAL;
    if (P == 0) return MOM_OK;
    if (!feat || !a0 || !dpts || !dscales || !drots || !dfeat || !scratch) return MOM_EINVAL;
    // MOM_MLP_BWD names a form of the 64-feature backward; this shape has the f32 form only, so every value that is valid there
    // (unset, empty, "b3", "split") runs it, and a value that is refused there is refused here
    const char* e = getenv("MOM_MLP_BWD");
    if (e && *e && strcmp(e, "b3") && strcmp(e, "split")) return MOM_EINVAL;
    MlpDev d;
    int rc = fill_dev(w, &d);
    if (rc) return rc;
    if (!d.dW0 || !d.db0) return MOM_EINVAL;
    for (int i = 0; i < 3; i++)
        if (!d.dW1[i] || !d.db1[i] || !d.dW2[i] || !d.db2[i]) return MOM_EINVAL;
    float* dH = (float*)scratch;                       // [4][P][64]: mom_deform_backward_scratch_bytes(P) holds it
    const int tiles = (P + 31) / 32;
    const int blocks = tiles < 256 ? tiles : 256;
    const size_t lds_a = sizeof(float) * kLBwdTotal;
    const size_t lds_b = sizeof(float) * (kHid * kHid + kHid);
    if (!mom_lds_limit<deform32_bwd_dx_kernel>(lds_a)) return MOM_ELAUNCH;
    MomProfScope ps(MOM_P_MLP_BWD, (hipStream_t)stream);
    hipLaunchKernelGGL(deform32_bwd_dx_kernel, dim3(blocks), dim3(64 * kDxWaves), lds_a, (hipStream_t)stream, d, P, tiles, a0, dpts,
                       dscales, drots, dfeat, dH);
    if (hipGetLastError() != hipSuccess) return MOM_ELAUNCH;
    hipStream_t ws = (hipStream_t)dw_stream;
    if (ws != (hipStream_t)stream) {                   // the weight-gradient kernel goes to the caller's second stream, behind dx
        static hipEvent_t dx_done = nullptr;
        if (!dx_done && hipEventCreateWithFlags(&dx_done, mom_order_event_flags()) != hipSuccess) return MOM_ELAUNCH;
        if (hipEventRecord(dx_done, (hipStream_t)stream) != hipSuccess) return MOM_ELAUNCH;
        if (hipStreamWaitEvent(ws, dx_done, 0) != hipSuccess) return MOM_ELAUNCH;
    }
    const int waves = 1024, layers = 4;                // 1024 waves per layer, each a contiguous (even-sized) range of Gaussians
    int chunk = (P + waves - 1) / waves;
    chunk += chunk & 1;
    hipLaunchKernelGGL(deform32_bwd_dw_kernel, dim3((waves / 4) * layers), dim3(256), lds_b, ws, d, P, chunk, feat, a0, dH, layers);
    return hipGetLastError() == hipSuccess ? MOM_OK : MOM_ELAUNCH;
}

}  // namespace

extern "C" int mom_deform_forward_n(const MomDeformMLP* w, int P, int in_features, const float* feat, const float* xyz,
                                    const float* scaling, const float* rotation, const float* scene_flow, float flow_coef, float* pts,
                                    float* scales, float* rots, float* a0_save, mom_stream_t stream)
{
    return mom_deform_forward_activated_n(w, P, in_features, feat, xyz, scaling, rotation, scene_flow, flow_coef, pts, scales, rots,
                                          a0_save, nullptr, nullptr, nullptr, nullptr, stream);
}

extern "C" int mom_deform_forward_activated_n(const MomDeformMLP* w, int P, int in_features, const float* feat, const float* xyz,
                                              const float* scaling, const float* rotation, const float* scene_flow, float flow_coef,
                                              float* pts, float* scales, float* rots, float* a0_save, const float* opacity_raw,
                                              float* scales_act, float* rots_act, float* opacity_act, mom_stream_t stream)
{
    if (in_features == kHid)
        return mom_deform_forward_activated(w, P, feat, xyz, scaling, rotation, scene_flow, flow_coef, pts, scales, rots, a0_save,
                                            opacity_raw, scales_act, rots_act, opacity_act, stream);
    if (in_features != kIn32) return MOM_EINVAL;
    return forward32(w, P, feat, xyz, scaling, rotation, scene_flow, flow_coef, pts, scales, rots, a0_save, opacity_raw, scales_act,
                     rots_act, opacity_act, stream);
}

extern "C" int mom_deform_backward_n(const MomDeformMLP* w, int P, int in_features, const float* feat, const float* a0,
                                     const float* dpts, const float* dscales, const float* drots, float* dfeat, void* scratch,
                                     mom_stream_t stream)
{
    return mom_deform_backward_split_n(w, P, in_features, feat, a0, dpts, dscales, drots, dfeat, scratch, stream, stream);
}

extern "C" int mom_deform_backward_split_n(const MomDeformMLP* w, int P, int in_features, const float* feat, const float* a0,
                                           const float* dpts, const float* dscales, const float* drots, float* dfeat, void* scratch,
                                           mom_stream_t stream, mom_stream_t dw_stream)
{
    if (in_features == kHid) return mom_deform_backward_split(w, P, feat, a0, dpts, dscales, drots, dfeat, scratch, stream, dw_stream);
    if (in_features != kIn32) return MOM_EINVAL;
    return backward32(w, P, feat, a0, dpts, dscales, drots, dfeat, scratch, stream, dw_stream);
}
