// Fused deformation MLP on the f32 matrix cores, forward and backward, gfx950.
//
// Replaces Deformation.forward_dynamic's 7 nn.Linear + ReLU + residual adds (reference
// scene/deformation.py:53-65,97-135 with the shipped config: W=64, D=0, heads pos/scales/rotations live,
// opacity/shs heads dead) and their autograd backward (14 GEMMs + elementwise):
//     h0 = W0 f + b0                        (feature_out, no activation after it)
//     for head in {pos, scales, rot}:  o = W2 relu(W1 relu(h0) + b1) + b2
//     pts = xyz + o_pos + c * scene_flow ; scales = s + o_scales ; rot = r + o_rot
//
// All 64x64 layers run on v_mfma_f32_32x32x2_f32 (exact fp32, k-ordered fma chain) in the TRANSPOSED form
// H^T = W X^T: weights are the A operand, activations the B operand with the Gaussian on the lane.  A 32x32
// accumulator tile then has exactly the register layout the next layer needs as ITS B operand (register r of lane
// half h is feature (r&3)+8(r>>2)+4h), so activations never leave registers between layers.
//
// The four 64x64 matrices live in LDS for the whole (persistent) kernel as [in][out] with a row stride of 65
// floats: the forward A fragment (lane = out) reads consecutive banks, the backward A fragment of W^T (lane = in)
// reads banks 65 apart -- both conflict-free from ONE copy.  The 64->{3,3,4} output layers are too thin for a
// 32-row tile and run on the VALU.  One wave owns 32 Gaussians per step of its persistent loop.
//
// Backward is two streaming kernels.  (A) deform_bwd_dx: reloads relu(h0) saved by the forward, recomputes each
// head's hidden layer, forms dH (gradient at every pre-activation), back-propagates through W^T down to d(features)
// and writes the four dH matrices [P][64]; the thin output layers' gradients are row sums over an LDS staging tile,
// kept in registers across the persistent loop.  (B) deform_bwd_dw: dW_L = dH_L^T X_L for the four 64x64 layers on
// the matrix cores with the Gaussian as the MFMA K index -- because dH and X are stored [gaussian][feature], both
// MFMA operands are plain coalesced 256-byte loads (lane = feature), every byte is read exactly once, the four
// 64x64 results live in 256 accumulator registers for the wave's whole range, and the bias gradients fall out of
// the A operands for free.  No atomics until one float atomic per weight per workgroup at the very end.
//
// The three kernels are templates on KT, the trunk's input in tiles of 32 features (deform_mlp_dev.h): 2 for the 64 features of
// two HexPlane levels of 32 channels, 1 for the 32 of two levels of 16 (dnerf/eulerian_150_16).  With KT = 1 the trunk layer reads
// W0 [64,32] and f [32] (a0_save stays [P,64]); dx back-propagates dH0 through W0^T to dfeat [P,32]; dW forms dW0 [64,32] = dH0^T
// feat with feat [P,32].  There the B operand's lane is still the input feature and its lane half the K slot (one of two
// Gaussians): two consecutive 128-byte feature rows are ONE 256-byte load of all 64 lanes, so the trunk layer issues one operand
// load and two MFMAs per K step where KT = 2 issues two and four, and no lane is masked.
//
// Ordered form (mom_deform_backward_ordered_n, include/mom4d.h "ordered MLP weight gradients"): the same two kernels instantiated with
// ORDERED = true store per-workgroup records where the default instantiations issue float atomics, and one more kernel adds the
// records in workgroup order; the default instantiations compile to the code they had.
//
// There is no bf16 one-kernel backward for 32 features (deform_bwd_b3.hip is 64 features only): such a call runs the two f32
// kernels whatever MOM_MLP_BWD names -- unset, empty, "b3" or "split" -- and any other value is MOM_EINVAL as for 64 features.
#include "deform_mlp_dev.h"
#include <string.h>

int mom_launch_deform_bwd_b3f(const MomDeformMLP* w, int P, const float* feat, const float* a0, const float* dpts, const float* dscales,
                              const float* drots, float* dfeat, void* scratch, hipStream_t s, hipStream_t dw_stream);      // deform_bwd_b3.hip
size_t mom_deform_bwd_b3f_scratch_bytes(void);

namespace {

constexpr int kOrdLayer = kHid * kHid + kHid;   // floats of one dW workgroup's record in the ordered form: [64][64] weights | 64 biases
constexpr int kOrdThin = 12 * kHid + 16;   // floats of one dx workgroup's record in the ordered form: [3 heads][4][64] weights | [3][4] biases | pad

// All threads of a workgroup share ONE copy of the weights in LDS (70 KB).  With 256 threads two workgroups = 8 waves fit per
// CU although the registers allow 16: a workgroup of up to 1024 threads gets up to 16 waves for the same LDS.
template <int KT>
__global__ void __launch_bounds__(1024)
deform_fwd_kernel(MlpDev m, int P, int tiles, const float* __restrict__ feat, const float* __restrict__ xyz,
                  const float* __restrict__ scaling, const float* __restrict__ rotation, const float* __restrict__ flow,
                  float flow_coef, float* __restrict__ pts, float* __restrict__ scales, float* __restrict__ rots,
                  float* __restrict__ a0_save, ActOut act)
{
    extern __shared__ float lds[];
    load_weights<KT>(m, lds);
    __syncthreads();
    const int lane = threadIdx.x & 63, col = lane & 31, h = lane >> 5;
    // Every workgroup takes a contiguous, equal (+-1) share of the tiles and deals it to its waves.  Dealing tiles to ALL the
    // launch's waves in turn left the remainder with the first workgroups only: at 6250 tiles on 4096 waves 134 CUs worked
    // through 8 tiles per SIMD while 122 had 4 -- the launch lasted 8 where the mean is 6.1.
    const int t_begin = (int)((long long)tiles * blockIdx.x / gridDim.x), t_end = (int)((long long)tiles * (blockIdx.x + 1) / gridDim.x);
    const int t_first = t_begin + (int)(threadIdx.x >> 6), t_step = (int)(blockDim.x >> 6);
    for (int t = t_first; t < t_end; t += t_step) {
        const int g = t * 32 + col;
        const bool ok = g < P;
        f32x16 a0[2];
        {
            f32x16 x[KT];
            load_feat(feat, g, ok, h, x);
            init_bias(lds + kLB, a0, h);
            layer64<false>(lds + kLW, x, a0, col, h);
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
    // Activated copies (mom_deform_forward_activated), after the tile loop: inside it their temporaries pushed the kernel over
    // its 128-register budget (100 bytes of scratch per lane, +15 us).  Each lane re-reads what it stored itself.
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
// (A) activations backward: dH for the four layers, d(features) [P][32 KT], output-layer weight gradients
// 512 threads: two waves per SIMD share one copy of the weights (142 KB of LDS with the staging tiles), so that one wave's vector
// and memory phases -- the thin output layers, the dH stores -- run under the other's MFMAs (4 waves: 288 us for dx + dW, 8: 276)
// ORDERED (mom_deform_backward_ordered_n): the waves meet in LDS by taking turns in wave order and the workgroup's result is STORED
// at m.dW2[0] + blockIdx.x * kOrdThin (the host points dW2[0] at the partials); deform_bwd_ordered_reduce_kernel adds the workgroups up.
template <int KT, bool ORDERED = false>
__global__ void __launch_bounds__(64 * kDxWaves)
deform_bwd_dx_kernel(MlpDev m, int P, int tiles, const float* __restrict__ a0g, const float* __restrict__ dpts,
                     const float* __restrict__ dscales, const float* __restrict__ drots, float* __restrict__ dfeat,
                     float* __restrict__ dH /* [4][P][64] */)
{
    extern __shared__ float lds[];
    load_weights<KT>(m, lds);
    __syncthreads();
    const int lane = threadIdx.x & 63, col = lane & 31, h = lane >> 5, wv = threadIdx.x >> 6;
    float* sA = lds + kLStage + wv * kStageFloats;
    float* sD = sA + kHid * kStageStride;              // dout[32 gaussians][4]
    // Every workgroup takes a contiguous, equal (+-1) share of the tiles and deals it to its waves.  Dealing tiles to ALL the
    // launch's waves in turn left the remainder with the first workgroups only: at 6250 tiles on 4096 waves 134 CUs worked
    // through 8 tiles per SIMD while 122 had 4 -- the launch lasted 8 where the mean is 6.1.
    const int t_begin = (int)((long long)tiles * blockIdx.x / gridDim.x), t_end = (int)((long long)tiles * (blockIdx.x + 1) / gridDim.x);
    const int t_first = t_begin + (int)(threadIdx.x >> 6), t_step = (int)(blockDim.x >> 6);
    const size_t PH = (size_t)P * kHid;
    float dW2[3][4], db2[3];                           // lane = feature; db2: lane n < 4 holds output n
#pragma unroll
    for (int k = 0; k < 3; k++) { db2[k] = 0.f; dW2[k][0] = dW2[k][1] = dW2[k][2] = dW2[k][3] = 0.f; }

    // the next tile's trunk activations are requested while this tile is worked on (a wave otherwise starts every tile with
    // a memory round trip, and its SIMD partner is not always in a matrix phase to cover it; mlp_bwd slot 177.4 -> 173.7 us)
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
        for (int head = 0; head < 3; head++) {   // rolled on purpose: unrolled, the scheduler interleaves the heads and spills
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
            f32x16 df[KT];
            zero_tile(df);
            layer64<true>(lds + kLW, dA0, df, col, h);  // dfeat = W0^T dH0, 32 KT rows
            store_feat(dfeat, g, ok, h, df);
        }
    }
    // output-layer gradients: combine the four waves in LDS, one atomic per element per workgroup
    __syncthreads();
    float* R = lds;
    if constexpr (ORDERED) {
#pragma unroll 1
        for (int turn = 0; turn < kDxWaves; turn++) {
            if (wv == turn) {
#pragma unroll
                for (int k = 0; k < 3; k++) {
#pragma unroll
                    for (int n = 0; n < 4; n++) {
                        float* a = &R[(k * 4 + n) * kHid + lane];
                        *a = (turn == 0 ? 0.f : *a) + dW2[k][n];
                    }
                    if (lane < 4) {
                        float* a = &R[12 * kHid + k * 4 + lane];
                        *a = (turn == 0 ? 0.f : *a) + db2[k];
                    }
                }
            }
            __syncthreads();
        }
        float* __restrict__ out = m.dW2[0] + (size_t)blockIdx.x * kOrdThin;
        for (int i = threadIdx.x; i < kOrdThin; i += blockDim.x) out[i] = i < 12 * kHid + 12 ? R[i] : 0.f;
        return;
    }
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

// One layer's weight gradient over one wave's range of Gaussians, for the 32-feature trunk's form of kernel (B) below:
// dW[o][i] = sum_g dH[g][o] X[g][i], db[o] = sum_g dH[g][o].
// KT = tiles of 32 input features: 2 for the heads (X = a0 [P,64], as deform_bwd_dw_kernel), 1 for the trunk (X = feat [P,32]).
// The B operand's lane half is the K slot, a Gaussian of the pair g0 + 2u + {0,1}: with KT = 1 the two halves read two consecutive
// 128-byte rows, one 256-byte load of the whole wave.
template <int KT, bool ORDERED = false>
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
    if constexpr (ORDERED) {
        // dst / dbs: this workgroup's record of the partials
        for (int i = threadIdx.x; i < kHid * kIn; i += 256) dst[i] = R[i];
        if (threadIdx.x < kHid) dbs[threadIdx.x] = R[kHid * kIn + threadIdx.x];
        return;
    }
    for (int i = threadIdx.x; i < kHid * kIn; i += 256) {
        const float v = R[i];
        if (v != 0.f) atomicAdd(&dst[i], v);
    }
    if (threadIdx.x < kHid) {
        const float v = R[kHid * kIn + threadIdx.x];
        if (v != 0.f) atomicAdd(&dbs[threadIdx.x], v);
    }
}

// (B) weight gradients: dW_L[o][i] = sum_g dH_L[g][o] X_L[g][i], db_L[o] = sum_g dH_L[g][o];  X_0 = feat, X_1..3 = a0
//
// The kernel streams dwords and is bound by how many cache misses a CU keeps in flight, not by the matrix pipe (SQ counters
// with all four layers in one wave: MFMA busy 30 % of the time, the rest issue stalls on VMEM).  So a wave takes ONE layer
// of its range of Gaussians: 64 accumulators, four waves per SIMD, four times the loads in flight of the form with all four
// layers (256 accumulators, one wave per SIMD); measured, dx + dW: 344 / 339 / 326 us for 4 / 2 / 1 layers per wave.  dH is
// still read exactly once overall; a0 is read once per layer 1..3.
//
// KT = 2 is the body below.  KT = 1 runs dw_layer above: layer 0 (dW0 [64,32], half the MFMAs of the others) at one K tile, layers
// 1..3 at two.  The two forms stay side by side because the body does not survive being called: as a __forceinline__ function or
// a generic lambda, at KT = 2, it compiles to 895 instructions where it has 991 here -- the same loop, another reduction (LDS stores
// merged in pairs, half the exec-mask regions) -- the way its NL comment warns, and the timings of this file are of these 991.
// ORDERED: a workgroup STORES its tile as record (layer, range) of the partials at m.dW0 (the host points it there), kOrdLayer floats
// each: [64][32 KT'] weights from the record's start, the 64 biases at kHid * kHid; deform_bwd_ordered_reduce_kernel adds the ranges up.
template <int KT, bool ORDERED = false>
__global__ void __launch_bounds__(256)
deform_bwd_dw_kernel(MlpDev m, int P, int chunk, const float* __restrict__ feat, const float* __restrict__ a0g,
                     const float* __restrict__ dH, int ny)
{
    extern __shared__ float lds[];                     // [64][64] reduction scratch + [64] bias
    if constexpr (KT == 2) {
        constexpr int NL = 1;                              // layers per wave; ny = 4 / NL layer groups (written out for NL = 1 the same
                                                           // source compiles to another schedule, so the loops over NL stay)
        const int lane = threadIdx.x & 63, col = lane & 31, h = lane >> 5;
        // One-dimensional grid of (ranges of Gaussians) x (ny layer groups), numbered so that the ny workgroups of one range are 8
        // ids apart inside a run of 8 ny ids: workgroup ids go to the eight XCDs in turn, so the layer groups of a range land on the
        // SAME XCD at about the same time, and the rows of a0 the three head layers all read come out of that XCD's L2 twice out of
        // three times (a two-dimensional grid ran all ranges of layer 0, then all of layer 1, ...: three trips to memory).
        const int lin = blockIdx.x, run = 8 * ny;
        const int bx = (lin / run) * 8 + (lin % run) % 8, by = (lin % run) / 8;
        const int wave = (bx * 256 + threadIdx.x) >> 6;
        const int L0 = NL * by;                            // first layer of this workgroup
        const size_t PH = (size_t)P * kHid;
        const int g_begin = wave * chunk, g_end = min(P, g_begin + chunk);   // chunk is even

        f32x16 dW[NL][2][2];
        float db[NL][2];
#pragma unroll
        for (int l = 0; l < NL; l++) {
            zero_tile(dW[l][0]);
            zero_tile(dW[l][1]);
            db[l][0] = db[l][1] = 0.f;
        }
        // Operand loads are double buffered by hand.  A trip is UNR K-steps (2 gaussians each); the loads of trip t+1 are issued
        // before the MFMAs of trip t.  They are issued UNCONDITIONALLY (rows past the end are clamped and masked by `ok`): vmcnt
        // retires in order, and a prefetch behind a branch would make the compiler wait for it too.
        constexpr int UNR = 4;
        struct Operands {
            float x[UNR][2], da[UNR][NL][2];
            bool ok[UNR];
        };
        const float* __restrict__ xa = L0 == 0 ? feat : a0g;      // layer L reads X = feat (L == 0) or a0 (L >= 1)
        auto load = [&](Operands& o, int g0) {
#pragma unroll
            for (int u = 0; u < UNR; u++) {
                const int g = g0 + 2 * u + h;               // K slot of this lane half
                const bool ok = g < g_end;
                o.ok[u] = ok;
                const size_t row = (size_t)(ok ? g : g_begin) * kHid;
#pragma unroll
                for (int kt = 0; kt < 2; kt++) o.x[u][kt] = xa[row + 32 * kt + col];
#pragma unroll
                for (int l = 0; l < NL; l++) {
                    const float* __restrict__ d = dH + (size_t)(L0 + l) * PH + row;
                    o.da[u][l][0] = d[col];
                    o.da[u][l][1] = d[32 + col];
                }
            }
        };
        auto compute = [&](const Operands& o) {
#pragma unroll
            for (int u = 0; u < UNR; u++) {
#pragma unroll
                for (int l = 0; l < NL; l++) {
                    const float a_lo = o.ok[u] ? o.da[u][l][0] : 0.f, a_hi = o.ok[u] ? o.da[u][l][1] : 0.f;
                    db[l][0] += a_lo;
                    db[l][1] += a_hi;
                    const float x0 = o.x[u][0], x1 = o.x[u][1];
                    dW[l][0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a_lo, x0, dW[l][0][0], 0, 0, 0);
                    dW[l][0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a_lo, x1, dW[l][0][1], 0, 0, 0);
                    dW[l][1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a_hi, x0, dW[l][1][0], 0, 0, 0);
                    dW[l][1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a_hi, x1, dW[l][1][1], 0, 0, 0);
                }
            }
        };
        if (g_begin < g_end) {
            // single rotation (compute(cur); cur = nxt): the two-phase form (A/B alternating in one body) made the register
            // allocator spill a whole operand buffer to scratch
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
        // Combine the four waves in LDS, then one float atomic per weight per workgroup.  The waves take TURNS on the shared
        // tile with plain read-add-write instead of LDS float atomics: ds_add_f32 runs at roughly 170 cycles per wave
        // instruction here, and 16 waves per CU each issuing 66 of them kept the CU's LDS busy for ~80 us -- more than the whole
        // MFMA loop (ablation: loop only 77 us, reduction only 88 us with every global atomic skipped, together 145 us).
        float* R = lds;
        const int wv = threadIdx.x >> 6;
#pragma unroll
        for (int l = 0; l < NL; l++) {
            const int L = L0 + l;
            // bias: the two lane halves hold different K slots of the same output feature
            const float b_lo = db[l][0] + __shfl_xor(db[l][0], 32), b_hi = db[l][1] + __shfl_xor(db[l][1], 32);
#pragma unroll 1
            for (int turn = 0; turn < 4; turn++) {
                __syncthreads();
                if (wv == turn) {
#pragma unroll
                    for (int mt = 0; mt < 2; mt++)
#pragma unroll
                        for (int kt = 0; kt < 2; kt++)
#pragma unroll
                            for (int r = 0; r < 16; r++) {     // tile row = out feature 32mt+fmap(r,h), column = in feature 32kt+col
                                float* a = &R[(32 * mt + fmap(r, h)) * kHid + 32 * kt + col];
                                *a = (turn == 0 ? 0.f : *a) + dW[l][mt][kt][r];
                            }
                    if (h == 0) {
                        float* a = &R[kHid * kHid + col];
                        a[0] = (turn == 0 ? 0.f : a[0]) + b_lo;
                        a[32] = (turn == 0 ? 0.f : a[32]) + b_hi;
                    }
                }
            }
            __syncthreads();
            if constexpr (ORDERED) {
                float* __restrict__ rec = m.dW0 + ((size_t)L * (gridDim.x / ny) + bx) * kOrdLayer;
                for (int i = threadIdx.x; i < kOrdLayer; i += 256) rec[i] = R[i];
                continue;
            }
            float* dst = L == 0 ? m.dW0 : m.dW1[L - 1];
            float* dbs = L == 0 ? m.db0 : m.db1[L - 1];
            for (int i = threadIdx.x; i < kHid * kHid; i += 256) {
                const float v = R[i];
                if (v != 0.f) atomicAdd(&dst[i], v);
            }
            if (threadIdx.x < kHid) {
                const float v = R[kHid * kHid + threadIdx.x];
                if (v != 0.f) atomicAdd(&dbs[threadIdx.x], v);
            }
        }
    } else {
        const int lin = blockIdx.x, run = 8 * ny;
        const int bx = (lin / run) * 8 + (lin % run) % 8, L = (lin % run) / 8;      // range of Gaussians, layer
        const int wave = (bx * 256 + threadIdx.x) >> 6;
        const int g_begin = wave * chunk, g_end = min(P, g_begin + chunk);   // chunk is even
        const float* __restrict__ dHl = dH + (size_t)L * P * kHid;
        if constexpr (ORDERED) {
            float* __restrict__ rec = m.dW0 + ((size_t)L * (gridDim.x / ny) + bx) * kOrdLayer;
            if (L == 0)
                dw_layer<1, true>(feat, dHl, g_begin, g_end, rec, rec + kHid * kHid, lds);
            else
                dw_layer<2, true>(a0g, dHl, g_begin, g_end, rec, rec + kHid * kHid, lds);
        } else {
            if (L == 0)
                dw_layer<1>(feat, dHl, g_begin, g_end, m.dW0, m.db0, lds);
            else
                dw_layer<2>(a0g, dHl, g_begin, g_end, m.dW1[L - 1], m.db1[L - 1], lds);
        }
    }
}

// The f32 backward's weight and bias gradients meet in a zeroed staging area at the head of `scratch` (the workgroups' float
// atomics land there) and reach the caller's buffers in ONE addition per element: the += of mom4d.h to one rounding of what the
// buffer held, as deform_bwd_reduce_kernel gives the bf16 form.  (Atomics straight onto the buffers rounded its content once per
// workgroup: 5 times at 33 Gaussians, ~200 at 8 k -- and once more per camera of a batch.)
//   [4 layers (W0, W1_0..2)][64*64 weights + 64 biases]  then  [3 heads][4*64 weights + 4 biases]
constexpr int kStgLayer = kHid * kHid + kHid;
static_assert(kStgLayer == kOrdLayer, "the ordered form's records have the staging area's layer layout");
constexpr int kStgThin = 4 * kHid + 4;
constexpr int kStgUsed = 4 * kStgLayer + 3 * kStgThin;
constexpr int kStgFloats = (kStgUsed + 63) / 64 * 64;            // dH behind it stays 256-byte aligned
// dst[i] += staged[i] for the elements first .. first + count - 1 of the map above; an element whose sum is zero is left alone
__global__ void __launch_bounds__(256) deform_bwd_add_kernel(MlpDev m, const float* __restrict__ staged, int n_in, int first, int count)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= count) return;
    const int i = first + t;
    if (i >= kStgUsed) return;
    const float v = staged[i];
    if (v == 0.f) return;
    float* dst = nullptr;
    if (i < 4 * kStgLayer) {
        const int L = i / kStgLayer, j = i - L * kStgLayer;
        if (j >= kHid * kHid) dst = (L == 0 ? m.db0 : m.db1[L - 1]) + (j - kHid * kHid);
        else if (L > 0) dst = m.dW1[L - 1] + j;
        else if (j < kHid * n_in) dst = m.dW0 + j;
    } else {
        const int k = (i - 4 * kStgLayer) / kStgThin, j = (i - 4 * kStgLayer) - k * kStgThin;
        const int nout = k == 2 ? 4 : 3;
        if (j < 4 * kHid) {
            if ((j >> 6) < nout) dst = m.dW2[k] + j;
        } else if (j - 4 * kHid < nout) dst = m.db2[k] + (j - 4 * kHid);
    }
    if (dst) *dst += v;
}

// The ordered form's reduction (include/mom4d.h, "ordered MLP weight gradients"): element i of the map above (first .. first + count - 1)
// takes the `nparts` workgroups' partials in ascending workgroup index, left to right from +0.0, then dst[i] += total -- ONE thread
// per element, so nothing but `nparts` decides the order.  Records are `stride` floats apart: element (layer L, j) lies at j of record
// (L, workgroup) [kOrdLayer floats], weight j of head k at 256 k + j and its bias n at 768 + 4 k + n of the workgroup's thin record [kOrdThin].
__global__ void __launch_bounds__(256)
deform_bwd_ordered_reduce_kernel(MlpDev m, const float* __restrict__ parts, int nparts, int n_in, int first, int count)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= count) return;
    const int i = first + t;
    if (i >= kStgUsed) return;
    float* dst = nullptr;
    const float* src;
    size_t stride;
    if (i < 4 * kStgLayer) {
        const int L = i / kStgLayer, j = i - L * kStgLayer;
        if (j >= kHid * kHid) dst = (L == 0 ? m.db0 : m.db1[L - 1]) + (j - kHid * kHid);
        else if (L > 0) dst = m.dW1[L - 1] + j;
        else if (j < kHid * n_in) dst = m.dW0 + j;
        src = parts + (size_t)L * nparts * kStgLayer + j;
        stride = kStgLayer;
    } else {
        const int k = (i - 4 * kStgLayer) / kStgThin, j = (i - 4 * kStgLayer) - k * kStgThin;
        const int nout = k == 2 ? 4 : 3;
        if (j < 4 * kHid) {
            if ((j >> 6) < nout) dst = m.dW2[k] + j;
            src = parts + k * 4 * kHid + j;
        } else {
            if (j - 4 * kHid < nout) dst = m.db2[k] + (j - 4 * kHid);
            src = parts + 12 * kHid + k * 4 + (j - 4 * kHid);
        }
        stride = kOrdThin;
    }
    if (!dst) return;
    float total = 0.f;
    for (int w0 = 0; w0 < nparts; w0 += 8) {               // eight loads in flight; the additions stay in record order
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; u++) v[u] = src[(size_t)min(w0 + u, nparts - 1) * stride];
#pragma unroll
        for (int u = 0; u < 8; u++)
            if (w0 + u < nparts) total = total + v[u];
    }
    *dst = *dst + total;
}

template <int KT>
int forward(const MomDeformMLP* w, int P, const float* feat, const float* xyz, const float* scaling, const float* rotation,
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
    // one workgroup per CU, the weights in its LDS (70 KB).  Sixteen waves: with 256 threads two workgroups = 8 waves fit per CU
    // beside their two copies of the weights although the registers allow 16; 1024 threads get all 16 for one copy
    const int block = 1024;
    // as many workgroups as CUs can hold at once, but never more than tiles: a small problem is spread over the CUs (one tile per
    // workgroup, 39 -> 21 us at 5 k Gaussians) instead of filling sixteen waves of a few workgroups
    const int blocks = tiles < 256 ? tiles : 256;
    const size_t lds_bytes = sizeof(float) * kLFwdTotal;
    if (!mom_lds_limit<deform_fwd_kernel<KT>>(lds_bytes)) return MOM_ELAUNCH;
    const ActOut act = {scales_act, rots_act, opacity_act, opacity_raw};
    MomProfScope ps(MOM_P_MLP_FWD, (hipStream_t)stream);
    hipLaunchKernelGGL(deform_fwd_kernel<KT>, dim3(blocks), dim3(block), lds_bytes, (hipStream_t)stream, d, P, tiles, feat, xyz, scaling,
                       rotation, scene_flow, flow_coef, pts, scales, rots, a0_save, act);
    return hipGetLastError() == hipSuccess ? MOM_OK : MOM_ELAUNCH;
}

// MOM_MLP_BWD (read per call so that tests can compare the forms): unset or "b3" -- the one-kernel backward on the bf16 pipe
// with role-specialised waves (deform_bwd_b3.hip; dfeat is complete on `stream`, the small reduction that completes the weight
// gradients runs on dw_stream); "split" -- the two f32 kernels above (dx on `stream`, dW on `dw_stream`).  Empty counts as
// unset, as for the integer switches; anything else is refused: a misspelt value must not quietly select a form.
enum BwdForm { kBwdB3, kBwdSplit, kBwdRefused };
BwdForm bwd_form()
{
    const char* e = getenv("MOM_MLP_BWD");
    if (!e || !*e || !strcmp(e, "b3")) return kBwdB3;
    return strcmp(e, "split") ? kBwdRefused : kBwdSplit;
}

template <int KT>
int backward(const MomDeformMLP* w, int P, const float* feat, const float* a0, const float* dpts, const float* dscales,
             const float* drots, float* dfeat, void* scratch, mom_stream_t stream, mom_stream_t dw_stream)
{
    if (P < 0) return MOM_EINVAL;
    if (P == 0) return MOM_OK;
    if (!feat || !a0 || !dpts || !dscales || !drots || !dfeat || !scratch) return MOM_EINVAL;
    // the bf16 form is 64 features only: at 32 every value that is valid there runs the f32 kernels, and a value that is refused
    // there is refused here
    const BwdForm form = bwd_form();
    if (form == kBwdRefused) return MOM_EINVAL;
    if (KT == 2 && form == kBwdB3)
        return mom_launch_deform_bwd_b3f(w, P, feat, a0, dpts, dscales, drots, dfeat, scratch, (hipStream_t)stream, (hipStream_t)dw_stream);
    MlpDev d;
    int rc = fill_dev(w, &d);
    if (rc) return rc;
    if (!d.dW0 || !d.db0) return MOM_EINVAL;
    for (int i = 0; i < 3; i++)
        if (!d.dW1[i] || !d.db1[i] || !d.dW2[i] || !d.db2[i]) return MOM_EINVAL;
    // mom_deform_backward_scratch_bytes(P) holds both: the staging area of the weight gradients, then dH [4][P][64]
    float* staged = (float*)scratch;
    float* dH = staged + kStgFloats;
    MlpDev g = d;                                       // the kernels' gradient pointers: into the staging area
    g.dW0 = staged;
    g.db0 = staged + kHid * kHid;
    for (int i = 0; i < 3; i++) {
        g.dW1[i] = staged + (1 + i) * kStgLayer;
        g.db1[i] = g.dW1[i] + kHid * kHid;
        g.dW2[i] = staged + 4 * kStgLayer + i * kStgThin;
        g.db2[i] = g.dW2[i] + 4 * kHid;
    }
    const int tiles = (P + 31) / 32;
    int blocks = tiles < 256 ? tiles : 256;             // persistent: one workgroup per CU; a small problem still uses every CU
    const size_t lds_a = sizeof(float) * kLBwdTotal;
    const size_t lds_b = sizeof(float) * (kHid * kHid + kHid);
    if (!mom_lds_limit<deform_bwd_dx_kernel<KT>>(lds_a)) return MOM_ELAUNCH;
    MomProfScope ps(MOM_P_MLP_BWD, (hipStream_t)stream);
    if (hipMemsetAsync(staged, 0, sizeof(float) * kStgFloats, (hipStream_t)stream) != hipSuccess) return MOM_ELAUNCH;
    hipLaunchKernelGGL(deform_bwd_dx_kernel<KT>, dim3(blocks), dim3(64 * kDxWaves), lds_a, (hipStream_t)stream, g, P, tiles, a0, dpts,
                       dscales, drots, dfeat, dH);
    if (hipGetLastError() != hipSuccess) return MOM_ELAUNCH;
    hipStream_t ws = (hipStream_t)dw_stream;
    if (ws != (hipStream_t)stream) {
        // the weight-gradient kernel reads what dx wrote (dH) and nothing behind it on `stream` depends on it: it goes to the
        // caller's second stream, behind an event, and overlaps whatever the caller enqueues on `stream` next
        static hipEvent_t dx_done = nullptr;
        if (!dx_done && hipEventCreateWithFlags(&dx_done, mom_order_event_flags()) != hipSuccess) return MOM_ELAUNCH;
        if (hipEventRecord(dx_done, (hipStream_t)stream) != hipSuccess) return MOM_ELAUNCH;
        if (hipStreamWaitEvent(ws, dx_done, 0) != hipSuccess) return MOM_ELAUNCH;
    }
    // weight gradients: 1024 waves per layer, each a contiguous (even-sized) range of gaussians
    const int waves = 1024, layers = 4;
    int chunk = (P + waves - 1) / waves;
    chunk += chunk & 1;
    // the thin output layers' gradients are complete in the staging area: into the caller's buffers on `stream` (mom4d.h), beside
    // the weight-gradient kernel
    hipLaunchKernelGGL(deform_bwd_add_kernel, dim3((3 * kStgThin + 255) / 256), dim3(256), 0, (hipStream_t)stream, d, staged, 32 * KT,
                       4 * kStgLayer, 3 * kStgThin);
    if (hipGetLastError() != hipSuccess) return MOM_ELAUNCH;
    // one-dimensional grid: the kernel deals (range, layer) to the XCDs itself
    hipLaunchKernelGGL(deform_bwd_dw_kernel<KT>, dim3((waves / 4) * layers), dim3(256), lds_b, ws, g, P, chunk, feat, a0, dH, layers);
    if (hipGetLastError() != hipSuccess) return MOM_ELAUNCH;
    hipLaunchKernelGGL(deform_bwd_add_kernel, dim3((4 * kStgLayer + 255) / 256), dim3(256), 0, ws, d, staged, 32 * KT, 0, 4 * kStgLayer);
    return hipGetLastError() == hipSuccess ? MOM_OK : MOM_ELAUNCH;
}

// scratch of the ordered form: dH [4][P][64] | the dx workgroups' records [256][kOrdThin] | the dW workgroups' records [4][256][kStgLayer]
constexpr int kOrdDxParts = 256, kOrdDwParts = 256;
size_t ordered_scratch_floats(int P, size_t* o_dx, size_t* o_dw)
{
    size_t off = ((size_t)4 * (size_t)(P > 0 ? P : 1) * kHid + 63) / 64 * 64;
    if (o_dx) *o_dx = off;
    off += (size_t)kOrdDxParts * kOrdThin;
    if (o_dw) *o_dw = off;
    off += (size_t)4 * kOrdDwParts * kStgLayer;
    return off;
}

// mom_deform_backward_ordered_n: the two f32 kernels in their ORDERED instantiations on one stream, then the reduction.  The grids are
// those of backward<KT>: min(tiles, 256) persistent workgroups, each a contiguous share of the tiles dealt to its waves by index, and
// 1024 wave ranges of a chunk that P alone fixes -- both mappings are arithmetic on blockIdx / threadIdx (deform_bwd_dx_kernel's t_begin /
// t_first, deform_bwd_dw_kernel's bx / wave), nothing is claimed at run time.
template <int KT>
int backward_ordered(const MomDeformMLP* w, int P, const float* feat, const float* a0, const float* dpts, const float* dscales,
                     const float* drots, float* dfeat, void* scratch, size_t scratch_bytes, mom_stream_t stream)
{
    if (P < 0) return MOM_EINVAL;
    if (P == 0) return MOM_OK;
    if (!feat || !a0 || !dpts || !dscales || !drots || !dfeat || !scratch) return MOM_EINVAL;
    size_t o_dx, o_dw;
    if (scratch_bytes < ordered_scratch_floats(P, &o_dx, &o_dw) * sizeof(float)) return MOM_EINVAL;
    MlpDev d;
    int rc = fill_dev(w, &d);
    if (rc) return rc;
    if (!d.dW0 || !d.db0) return MOM_EINVAL;
    for (int i = 0; i < 3; i++)
        if (!d.dW1[i] || !d.db1[i] || !d.dW2[i] || !d.db2[i]) return MOM_EINVAL;
    float* dH = (float*)scratch;
    float* parts_dx = dH + o_dx;
    float* parts_dw = dH + o_dw;
    MlpDev g = d;                                       // the ORDERED kernels read two of the gradient pointers only: their partials
    g.dW2[0] = parts_dx;
    g.dW0 = parts_dw;
    const int tiles = (P + 31) / 32;
    const int blocks = tiles < kOrdDxParts ? tiles : kOrdDxParts;
    const size_t lds_a = sizeof(float) * kLBwdTotal;
    const size_t lds_b = sizeof(float) * (kHid * kHid + kHid);
    if (!mom_lds_limit<deform_bwd_dx_kernel<KT, true>>(lds_a)) return MOM_ELAUNCH;
    hipStream_t s = (hipStream_t)stream;
    MomProfScope ps(MOM_P_MLP_BWD, s);
    hipLaunchKernelGGL((deform_bwd_dx_kernel<KT, true>), dim3(blocks), dim3(64 * kDxWaves), lds_a, s, g, P, tiles, a0, dpts, dscales, drots,
                       dfeat, dH);
    if (hipGetLastError() != hipSuccess) return MOM_ELAUNCH;
    const int waves = 4 * kOrdDwParts, layers = 4;
    int chunk = (P + waves - 1) / waves;
    chunk += chunk & 1;
    hipLaunchKernelGGL((deform_bwd_dw_kernel<KT, true>), dim3(kOrdDwParts * layers), dim3(256), lds_b, s, g, P, chunk, feat, a0, dH, layers);
    if (hipGetLastError() != hipSuccess) return MOM_ELAUNCH;
    hipLaunchKernelGGL(deform_bwd_ordered_reduce_kernel, dim3((3 * kStgThin + 255) / 256), dim3(256), 0, s, d, parts_dx, blocks, 32 * KT,
                       4 * kStgLayer, 3 * kStgThin);
    hipLaunchKernelGGL(deform_bwd_ordered_reduce_kernel, dim3((4 * kStgLayer + 255) / 256), dim3(256), 0, s, d, parts_dw, kOrdDwParts, 32 * KT, 0,
                       4 * kStgLayer);
    return hipGetLastError() == hipSuccess ? MOM_OK : MOM_ELAUNCH;
}

}  // namespace

extern "C" size_t mom_deform_backward_ordered_scratch_bytes(int P)
{
    return P < 0 ? 0 : ordered_scratch_floats(P, nullptr, nullptr) * sizeof(float);
}

extern "C" int mom_deform_backward_ordered_n(const MomDeformMLP* w, int P, int in_features, const float* feat, const float* a0,
                                             const float* dpts, const float* dscales, const float* drots, float* dfeat, void* scratch,
                                             size_t scratch_bytes, mom_stream_t stream)
{
    if (in_features != 64 && in_features != 32) return MOM_EINVAL;
    return (in_features == 64 ? backward_ordered<2> : backward_ordered<1>)(w, P, feat, a0, dpts, dscales, drots, dfeat, scratch,
                                                                           scratch_bytes, stream);
}

// The entry points with in_features (include/mom4d.h) are the ones that launch: 64 and 32 are the trunks there are.
extern "C" int mom_deform_forward_activated_n(const MomDeformMLP* w, int P, int in_features, const float* feat, const float* xyz,
                                              const float* scaling, const float* rotation, const float* scene_flow, float flow_coef,
                                              float* pts, float* scales, float* rots, float* a0_save, const float* opacity_raw,
                                              float* scales_act, float* rots_act, float* opacity_act, mom_stream_t stream)
{
    if (in_features != 64 && in_features != 32) return MOM_EINVAL;
    return (in_features == 64 ? forward<2> : forward<1>)(w, P, feat, xyz, scaling, rotation, scene_flow, flow_coef, pts, scales, rots,
                                                         a0_save, opacity_raw, scales_act, rots_act, opacity_act, stream);
}

extern "C" int mom_deform_backward_split_n(const MomDeformMLP* w, int P, int in_features, const float* feat, const float* a0,
                                           const float* dpts, const float* dscales, const float* drots, float* dfeat, void* scratch,
                                           mom_stream_t stream, mom_stream_t dw_stream)
{
    if (in_features != 64 && in_features != 32) return MOM_EINVAL;
    return (in_features == 64 ? backward<2> : backward<1>)(w, P, feat, a0, dpts, dscales, drots, dfeat, scratch, stream, dw_stream);
}

// the larger of what the two forms need: the two-kernel form's staging area and four [P,64] matrices, the one-kernel form's
// per-workgroup partial sums
extern "C" size_t mom_deform_backward_scratch_bytes(int P)
{
    const size_t a = ((size_t)kStgFloats + (size_t)4 * (size_t)(P > 0 ? P : 1) * kHid) * sizeof(float), b = mom_deform_bwd_b3f_scratch_bytes();
    return a > b ? a : b;
}

extern "C" int mom_deform_forward_n(const MomDeformMLP* w, int P, int in_features, const float* feat, const float* xyz,
                                    const float* scaling, const float* rotation, const float* scene_flow, float flow_coef, float* pts,
                                    float* scales, float* rots, float* a0_save, mom_stream_t stream)
{
    return mom_deform_forward_activated_n(w, P, in_features, feat, xyz, scaling, rotation, scene_flow, flow_coef, pts, scales, rots,
                                          a0_save, nullptr, nullptr, nullptr, nullptr, stream);
}

extern "C" int mom_deform_backward_n(const MomDeformMLP* w, int P, int in_features, const float* feat, const float* a0,
                                     const float* dpts, const float* dscales, const float* drots, float* dfeat, void* scratch,
                                     mom_stream_t stream)
{
    return mom_deform_backward_split_n(w, P, in_features, feat, a0, dpts, dscales, drots, dfeat, scratch, stream, stream);
}

extern "C" int mom_deform_forward(const MomDeformMLP* w, int P, const float* feat, const float* xyz, const float* scaling,
                                  const float* rotation, const float* scene_flow, float flow_coef, float* pts, float* scales,
                                  float* rots, float* a0_save, mom_stream_t stream)
{
    return mom_deform_forward_n(w, P, 64, feat, xyz, scaling, rotation, scene_flow, flow_coef, pts, scales, rots, a0_save, stream);
}

extern "C" int mom_deform_forward_activated(const MomDeformMLP* w, int P, const float* feat, const float* xyz, const float* scaling,
                                            const float* rotation, const float* scene_flow, float flow_coef, float* pts, float* scales,
                                            float* rots, float* a0_save, const float* opacity_raw, float* scales_act, float* rots_act,
                                            float* opacity_act, mom_stream_t stream)
{
    return mom_deform_forward_activated_n(w, P, 64, feat, xyz, scaling, rotation, scene_flow, flow_coef, pts, scales, rots, a0_save,
                                          opacity_raw, scales_act, rots_act, opacity_act, stream);
}

extern "C" int mom_deform_backward(const MomDeformMLP* w, int P, const float* feat, const float* a0, const float* dpts,
                                   const float* dscales, const float* drots, float* dfeat, void* scratch, mom_stream_t stream)
{
    return mom_deform_backward_n(w, P, 64, feat, a0, dpts, dscales, drots, dfeat, scratch, stream);
}

extern "C" int mom_deform_backward_split(const MomDeformMLP* w, int P, const float* feat, const float* a0, const float* dpts,
                                         const float* dscales, const float* drots, float* dfeat, void* scratch, mom_stream_t stream,
                                         mom_stream_t dw_stream)
{
    return mom_deform_backward_split_n(w, P, 64, feat, a0, dpts, dscales, drots, dfeat, scratch, stream, dw_stream);
}
