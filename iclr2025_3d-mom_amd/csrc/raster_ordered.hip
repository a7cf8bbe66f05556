// The ordered backward reduction of the rasterizer (include/mom4d.h, "ordered backward reduction"), gfx950: the plan that gives every
// (Gaussian, tile of its rectangle) pair a slot, the reduction that adds a Gaussian's slots up in the documented order, and that
// order once more in plain C++ for the host.  The compositing kernel that fills the slots is render_bwd_kernel<., true>
// (raster_render.hip).  THIS FILE IS COMPILED WITH -ffp-contract=off: the host twin must add exactly as the kernel does.
#include "mom_common.h"
#include "scan_dev.h"

namespace {

// ---- plan: slot_base = exclusive scan of tiles_touched ---------------------------------------------------------------------------
// tiles_touched is word 3 of a Gaussian's record (0 for radius 0), written by the projection from getRect: the scan needs nothing
// else.  A workgroup owns kPlanChunk consecutive Gaussians, a thread sixteen consecutive ones.  Two launches: the chunks' sums, then
// every chunk adds the sums of the chunks in front of it (a few hundred at most: 245 for a million Gaussians) and scans its own.
constexpr int kPlanPer = 16, kPlanChunk = 256 * kPlanPer;

__device__ __forceinline__ uint32_t tiles_of(const float4* __restrict__ rec, int g, int P)
{
    return g < P ? __float_as_uint(rec[3 * (size_t)g].w) : 0u;
}

__global__ void __launch_bounds__(256) ordered_count_kernel(int P, const float4* __restrict__ rec, unsigned long long* __restrict__ chunk_sums)
{
    __shared__ int s_wave[4];
    const int g0 = blockIdx.x * kPlanChunk + threadIdx.x * kPlanPer;
    int mine = 0;
#pragma unroll
    for (int i = 0; i < kPlanPer; i++) mine += (int)tiles_of(rec, g0 + i, P);
    int total;
    block_exclusive_scan_256(mine, s_wave, total);
    if (threadIdx.x == 0) chunk_sums[blockIdx.x] = (unsigned long long)(uint32_t)total;
}
// A rectangle holds at most gx * gy tiles and the binning refuses grids above 2^16 tiles long before (kMaxLdsTiles and the tile
// scan's 36 k): a chunk's sum stays below 4096 x 2^16 = 2^28, an int.  The sum over the chunks is taken in 64 bits and a total that
// does not fit the 32-bit slot index is reported as 2^32 - 1, which nobody accepts as a slot count.
__global__ void __launch_bounds__(256) ordered_scan_kernel(int P, const float4* __restrict__ rec, const unsigned long long* __restrict__ chunk_sums,
                                                          uint32_t* __restrict__ slot_base, uint32_t* total_dev, uint32_t* total_host)
{
    __shared__ int s_wave[4];
    __shared__ unsigned long long s_front[256];
    unsigned long long front = 0;
    for (int c = threadIdx.x; c < (int)blockIdx.x; c += 256) front += chunk_sums[c];
    s_front[threadIdx.x] = front;
    __syncthreads();
    for (int d = 128; d >= 1; d >>= 1) {
        if ((int)threadIdx.x < d) s_front[threadIdx.x] += s_front[threadIdx.x + d];
        __syncthreads();
    }
    front = s_front[0];
    const int g0 = blockIdx.x * kPlanChunk + threadIdx.x * kPlanPer;
    uint32_t t[kPlanPer];
    int mine = 0;
#pragma unroll
    for (int i = 0; i < kPlanPer; i++) {
        t[i] = tiles_of(rec, g0 + i, P);
        mine += (int)t[i];
    }
    int total;
    unsigned long long at = front + (unsigned long long)block_exclusive_scan_256(mine, s_wave, total);
#pragma unroll
    for (int i = 0; i < kPlanPer; i++) {
        if (g0 + i < P) slot_base[g0 + i] = (uint32_t)at;
        at += t[i];
    }
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) {
        const unsigned long long all = front + (unsigned long long)total;
        const uint32_t v = all >= 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)all;
        slot_base[P] = v;
        if (total_dev) *total_dev = v;
        if (total_host) __hip_atomic_store(total_host, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// ---- reduction ------------------------------------------------------------------------------------------------------------------------
// One wave per Gaussian.  Lane = 16 r + k: value k (k < MOM_ORDERED_VALUES) of the interleaved sequence r = 0..3, which walks the slots
// r, r + 4, ... in increasing order; the four sequences meet as (a0 + a2) + (a1 + a3).  The lanes, the grid and the workgroup size
// decide WHO adds, never WHAT is added to what: the order is the one include/mom4d.h documents, a function of the slot count alone.
// A slot range that leaves the buffer (a plan of another frame) is cut at `slots` and MOM_ORDERED_CUT raised: nothing outside is read.
__global__ void __launch_bounds__(256) ordered_reduce_kernel(int P, const uint32_t* __restrict__ slot_base, const float* __restrict__ partials,
                                                            uint32_t slots, float* __restrict__ gacc, uint32_t* status)
{
    const int lane = threadIdx.x & 63, g = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (g >= P) return;
    const int r = lane >> 4, k = lane & 15;
    const uint32_t b0 = slot_base[g], b1 = slot_base[g + 1];
    uint32_t n = b1 >= b0 ? b1 - b0 : 0u;
    if (b1 < b0 || b0 > slots || n > slots - b0) {
        n = b0 > slots ? 0u : min(n, slots - b0);
        if (lane == 0) atomicOr(status, (uint32_t)MOM_ORDERED_CUT);
    }
    float acc = 0.f;
    if (k < MOM_ORDERED_VALUES) {
        const float* __restrict__ p = partials + (size_t)b0 * (4 * MOM_ORDERED_VALUES) + k;
        for (uint32_t s = (uint32_t)r; s < n; s += 4) {
            const float* q = p + (size_t)s * (4 * MOM_ORDERED_VALUES);
            const float t = (q[0] + q[MOM_ORDERED_VALUES]) + (q[2 * MOM_ORDERED_VALUES] + q[3 * MOM_ORDERED_VALUES]);
            acc = acc + t;
        }
    }
    acc = acc + __shfl_xor(acc, 32);          // a0 + a2 | a1 + a3 (an addition's two operands commute: both partners hold the same bits)
    acc = acc + __shfl_xor(acc, 16);          // (a0 + a2) + (a1 + a3)
    if (r == 0 && k < MOM_GACC_FLOATS) gacc[(size_t)g * MOM_GACC_FLOATS + k] = k < MOM_ORDERED_VALUES ? acc : 0.f;
}

}  // namespace

static_assert(MOM_ORDERED_SLOT_BYTES == 4 * MOM_ORDERED_VALUES * sizeof(float), "four waves of ten values per slot");
static_assert(MOM_GACC_FLOATS <= 16 && MOM_ORDERED_VALUES <= MOM_GACC_FLOATS, "the reduction's lane layout");

static inline int plan_chunks(int P) { return (P + kPlanChunk - 1) / kPlanChunk; }
// plan buffer: slot_base[P + 1] u32 | chunk_sums[chunks] u64
size_t mom_ordered_plan_view(char* base, int P, uint32_t** slot_base, unsigned long long** chunk_sums)
{
    size_t off = 0;
    const size_t o_b = off; off = mom_align_up(off + ((size_t)P + 1) * 4);
    const size_t o_c = off; off = mom_align_up(off + (size_t)plan_chunks(P) * 8);
    if (slot_base) *slot_base = (uint32_t*)(base + o_b);
    if (chunk_sums) *chunk_sums = (unsigned long long*)(base + o_c);
    return off + MOM_ALIGN;
}

int mom_launch_ordered_plan(int P, const GeomView& g, char* plan, uint32_t* total_dev, uint32_t* total_host, hipStream_t s)
{
    uint32_t* slot_base;
    unsigned long long* chunk_sums;
    mom_ordered_plan_view(plan, P, &slot_base, &chunk_sums);
    const int chunks = plan_chunks(P);
    hipLaunchKernelGGL(ordered_count_kernel, dim3(chunks), dim3(256), 0, s, P, g.rec, chunk_sums);
    hipLaunchKernelGGL(ordered_scan_kernel, dim3(chunks), dim3(256), 0, s, P, g.rec, chunk_sums, slot_base, total_dev, total_host);
    return hipGetLastError() == hipSuccess ? MOM_OK : MOM_ELAUNCH;
}

int mom_launch_ordered_reduce(int P, const GeomView& g, const uint32_t* slot_base, const float* partials, uint32_t slots, uint32_t* status,
                              hipStream_t s)
{
    hipLaunchKernelGGL(ordered_reduce_kernel, dim3((P + 3) / 4), dim3(256), 0, s, P, slot_base, partials, slots, g.gacc, status);
    return hipGetLastError() == hipSuccess ? MOM_OK : MOM_ELAUNCH;
}

extern "C" int mom_raster_ordered_sum_host(int P, const uint32_t* slot_base, const float* partials, float* gacc)
{
    if (P < 0) return MOM_EINVAL;
    if (P == 0) return MOM_OK;
    if (!slot_base || !gacc) return MOM_EINVAL;
    if (!partials && slot_base[P] != slot_base[0]) return MOM_EINVAL;
    for (int g = 0; g < P; g++) {
        if (slot_base[g + 1] < slot_base[g]) return MOM_EINVAL;
        const uint32_t n = slot_base[g + 1] - slot_base[g];
        float* out = gacc + (size_t)g * MOM_GACC_FLOATS;
        for (int k = 0; k < MOM_GACC_FLOATS; k++) out[k] = 0.f;
        for (int k = 0; k < MOM_ORDERED_VALUES; k++) {
            float a[4] = {0.f, 0.f, 0.f, 0.f};
            for (uint32_t s = 0; s < n; s++) {
                const float* q = partials + ((size_t)slot_base[g] + s) * (4 * MOM_ORDERED_VALUES) + k;
                const float t = (q[0] + q[MOM_ORDERED_VALUES]) + (q[2 * MOM_ORDERED_VALUES] + q[3 * MOM_ORDERED_VALUES]);
                a[s & 3] = a[s & 3] + t;
            }
            out[k] = (a[0] + a[2]) + (a[1] + a[3]);
        }
    }
    return MOM_OK;
}
