// The 3D motion optimisation module's fit in one launch, gfx950.
//
// The reference (train_motion.py:125-207 MotionOptimization.optimize_motion) holds one [3,P] tensor, the Eulerian scene flow, and
// runs SGD on it: every epoch projects the flowed points into every view, takes the mean L1 distance between the 2D flow that
// results and the view's estimated 2D flow, sums the views' means, divides by idx + 1 and steps once.  The normalisers come from the
// UNflowed points and never change, so the gradient of a point's flow depends on that point alone: here one thread owns one point,
// keeps its three flow components in registers and walks all E x V (epoch, view) pairs by itself.
//
//   records [V][P] float4  {pix0.x, pix0.y, gt.x, gt.y}: one 16-byte load per lane, a wave reads 1 KB contiguous
//   valid   [ceil(V/32)][P] one bit per (view, point), word-major so that a wave's 64 words are contiguous; a word is read when its
//           32 views begin (three 4-byte loads per point and epoch at V = 70 beside seventy 16-byte ones) -- held in registers for
//           the whole fit they would be an array indexed by a run-time value, which the compiler keeps in scratch memory
//   R [V][9], T [V][3], w [V]  indexed by the view alone: the same address in every lane
//
// Arithmetic order is the reference's where a sign depends on it: the rotation and the intrinsics are three-term sums accumulated
// with fused multiply-adds in term order (as the BLAS inner loop does for torch.matmul), d = ((u,v) - pix0) - gt in that order,
// sign(0) = 0.  Nothing guards h_z <= 0 for a valid point (the reference does not either); invalid entries are left out by
// selection, not by a zero factor, so whatever they hold -- a point behind the camera, unwritten record memory -- reaches nothing.
//
// The epoch's loss is summed per thread and per wave in double and stored per wave (partial[E][waves]); a second launch adds each
// epoch's row in a fixed order.  No atomics: the log is the same bits on every run.  No workgroup barrier in the fit kernel, so
// the threads past P simply carry no valid bit.
#include "mom_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWavesPerBlock = kThreads / MOM_WAVE;

__device__ __forceinline__ float sf_sign(float x) { return (float)((x > 0.0f) - (x < 0.0f)); }

template <bool LOSS>
__global__ void __launch_bounds__(kThreads)
sceneflow_fit_kernel(int P, int V, int E, const float* __restrict__ points, float fx, float fy, float cx, float cy,
                     const float* __restrict__ R, const float* __restrict__ T, const float* __restrict__ w,
                     const float4* __restrict__ rec, const uint32_t* __restrict__ valid, const float* __restrict__ lr,
                     float* __restrict__ flow, double* __restrict__ partial, int nwaves, float2* __restrict__ flow2d_last)
{
#pragma clang fp contract(off)
    const int i = blockIdx.x * kThreads + threadIdx.x;
    const bool live = i < P;
    const size_t ii = live ? i : P - 1;                  // (threads past P read the last point and keep nothing)
    const size_t sP = (size_t)P;
    const float px = points[ii], py = points[sP + ii], pz = points[2 * sP + ii];
    float f0 = flow[ii], f1 = flow[sP + ii], f2 = flow[2 * sP + ii];

    for (int e = 0; e < E; e++) {
        const bool last = flow2d_last != nullptr && e == E - 1;
        const float qx = px + f0, qy = py + f1, qz = pz + f2;
        float g0 = 0.0f, g1 = 0.0f, g2 = 0.0f;
        double ls = 0.0;
        for (int j0 = 0; j0 < V; j0 += 32) {
            const uint32_t bits = live ? valid[(size_t)(j0 >> 5) * sP + ii] : 0u;
            const int jn = min(32, V - j0);
#pragma unroll 4
            for (int k = 0; k < jn; k++) {
                const int j = j0 + k;
                const float4 r = rec[(size_t)j * sP + ii];
                const bool ok = (bits >> k) & 1u;
                const float* __restrict__ Rj = R + 9 * (size_t)j;
                const float* __restrict__ Tj = T + 3 * (size_t)j;
                const float wj = w[j];
                // c = R q + T,  h = K c
                const float c0 = __builtin_fmaf(Rj[2], qz, __builtin_fmaf(Rj[1], qy, Rj[0] * qx)) + Tj[0];
                const float c1 = __builtin_fmaf(Rj[5], qz, __builtin_fmaf(Rj[4], qy, Rj[3] * qx)) + Tj[1];
                const float c2 = __builtin_fmaf(Rj[8], qz, __builtin_fmaf(Rj[7], qy, Rj[6] * qx)) + Tj[2];
                const float hx = __builtin_fmaf(cx, c2, fx * c0);
                const float hy = __builtin_fmaf(cy, c2, fy * c1);
                // u = hx / c2, v = hy / c2: one division, then each quotient corrected by its own remainder
                const float rz = 1.0f / c2;
                float u = hx * rz, v = hy * rz;
                u = __builtin_fmaf(__builtin_fmaf(-u, c2, hx), rz, u);
                v = __builtin_fmaf(__builtin_fmaf(-v, c2, hy), rz, v);
                const float du = u - r.x, dv = v - r.y;
                const float dx = du - r.z, dy = dv - r.w;
                // backward of w_j (|dx| + |dy|) through the division, K and R
                const float gu = wj * sf_sign(dx), gv = wj * sf_sign(dy);
                const float ghx = gu * rz, ghy = gv * rz;
                const float ghz = -(gu * u + gv * v) * rz;
                const float gc0 = fx * ghx, gc1 = fy * ghy;
                const float gc2 = __builtin_fmaf(cy, ghy, cx * ghx) + ghz;
                const float t0 = __builtin_fmaf(Rj[6], gc2, __builtin_fmaf(Rj[3], gc1, Rj[0] * gc0));
                const float t1 = __builtin_fmaf(Rj[7], gc2, __builtin_fmaf(Rj[4], gc1, Rj[1] * gc0));
                const float t2 = __builtin_fmaf(Rj[8], gc2, __builtin_fmaf(Rj[5], gc1, Rj[2] * gc0));
                g0 += ok ? t0 : 0.0f;
                g1 += ok ? t1 : 0.0f;
                g2 += ok ? t2 : 0.0f;
                if (LOSS) ls += ok ? (double)(wj * (fabsf(dx) + fabsf(dy))) : 0.0;
                if (last && live) flow2d_last[(size_t)j * sP + ii] = ok ? float2{du, dv} : float2{0.0f, 0.0f};
            }
        }
        const float step = lr[e];
        f0 -= step * g0;
        f1 -= step * g1;
        f2 -= step * g2;
        if (LOSS) {
#pragma unroll
            for (int m = MOM_WAVE / 2; m > 0; m >>= 1) ls += __shfl_xor(ls, m, MOM_WAVE);
            if ((threadIdx.x & (MOM_WAVE - 1)) == 0)
                partial[(size_t)e * nwaves + blockIdx.x * kWavesPerBlock + threadIdx.x / MOM_WAVE] = ls;
        }
    }
    if (live) {
        flow[ii] = f0;
        flow[sP + ii] = f1;
        flow[2 * sP + ii] = f2;
    }
}

// loss[e] = the sum of partial[e][0 .. nwaves), always in the same order.  One workgroup per epoch; every thread reaches every barrier.
__global__ void __launch_bounds__(kThreads) sceneflow_loss_kernel(int nwaves, const double* __restrict__ partial, float* __restrict__ loss)
{
    __shared__ double s_sum[kThreads];
    const double* __restrict__ row = partial + (size_t)blockIdx.x * nwaves;
    double a = 0.0;
    for (int k = threadIdx.x; k < nwaves; k += kThreads) a += row[k];
    s_sum[threadIdx.x] = a;
    __syncthreads();
    for (int m = kThreads / 2; m > 0; m >>= 1) {
        if ((int)threadIdx.x < m) s_sum[threadIdx.x] += s_sum[threadIdx.x + m];
        __syncthreads();
    }
    if (threadIdx.x == 0) loss[blockIdx.x] = (float)s_sum[0];
}

inline size_t fit_blocks(int P) { return ((size_t)P + kThreads - 1) / kThreads; }

}  // namespace

extern "C" size_t mom_sceneflow_fit_scratch_bytes(int P, int V, int E)
{
    (void)V;
    if (P <= 0 || E <= 0) return MOM_ALIGN;
    return mom_align_up((size_t)E * fit_blocks(P) * kWavesPerBlock * sizeof(double)) + MOM_ALIGN;
}

extern "C" int mom_sceneflow_fit(int P, int V, int E, const float* points, const float* K, const float* R, const float* T,
                                 const float* w, const float* records, const uint32_t* valid, const float* lr, float* flow,
                                 float* loss, float* flow2d_last, void* scratch, size_t scratch_bytes, mom_stream_t stream)
{
    if (P < 0 || V <= 0 || E < 0) return MOM_EINVAL;
    if (P == 0) return MOM_OK;
    if (!points || !K || !R || !T || !w || !records || !valid || !flow || (E > 0 && !lr)) return MOM_EINVAL;
    if (((uintptr_t)records & 15) || ((uintptr_t)flow2d_last & 7)) return MOM_EINVAL;
    // K = [[fx, 0, cx], [0, fy, cy], [0, 0, 1]] (train_motion.py:58-62), read on the host
    if (K[1] != 0.0f || K[3] != 0.0f || K[6] != 0.0f || K[7] != 0.0f || K[8] != 1.0f) return MOM_EINVAL;
    if (loss && (!scratch || scratch_bytes < mom_sceneflow_fit_scratch_bytes(P, V, E))) return MOM_EINVAL;
    if (E == 0) return MOM_OK;
    hipStream_t s = (hipStream_t)stream;
    const size_t blocks = fit_blocks(P);
    const int nwaves = (int)(blocks * kWavesPerBlock);
    double* partial = loss ? (double*)mom_align_ptr(scratch) : nullptr;
    if (loss) {
        hipLaunchKernelGGL(sceneflow_fit_kernel<true>, dim3((unsigned)blocks), dim3(kThreads), 0, s, P, V, E, points, K[0], K[4], K[2],
                           K[5], R, T, w, (const float4*)records, valid, lr, flow, partial, nwaves, (float2*)flow2d_last);
        hipLaunchKernelGGL(sceneflow_loss_kernel, dim3((unsigned)E), dim3(kThreads), 0, s, nwaves, partial, loss);
    } else {
        hipLaunchKernelGGL(sceneflow_fit_kernel<false>, dim3((unsigned)blocks), dim3(kThreads), 0, s, P, V, E, points, K[0], K[4], K[2],
                           K[5], R, T, w, (const float4*)records, valid, lr, flow, partial, nwaves, (float2*)flow2d_last);
    }
    return hipGetLastError() == hipSuccess ? MOM_OK : MOM_ELAUNCH;
}
