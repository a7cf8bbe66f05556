// One-pass densify round, gfx950.
//
// The reference's round (scene/gaussian_model.py:541-581 densify_and_clone / densify_and_split, with :461-482
// cat_tensors_to_optimizer, :484-509 densification_postfix and :511-539 the split's sampling and prune_points) appends the clones,
// appends two children per split parent and then removes the parents: three selections, two concatenations and a prune of every
// per-Gaussian tensor and both of its Adam moments.  Here the two masks are scanned ONCE into a plan and one kernel reads every
// source row once and writes it -- or its children -- where the reference's round leaves it:
//
//   rows 0 .. K-1            the rows that are not split, in order                (K = P - S)
//   rows K .. K+C-1          the clones, in order
//   rows K+C+b*S+j, b = 0,1  child b of the j-th split parent
//
// The masks themselves stay torch expressions on the caller's side: which class a row falls into must not depend on whose exp()
// rounds which way.
#include "mom_common.h"
#include "scan_dev.h"

namespace {

constexpr int kItems = 2048;       // rows per workgroup in the scan (256 threads x 8), as in select_rows.hip

__global__ void __launch_bounds__(256) densify_count_kernel(int n, const uint8_t* __restrict__ clone, const uint8_t* __restrict__ split,
                                                           int* __restrict__ bc_clone, int* __restrict__ bc_split)
{
    __shared__ int s_wave[4];
    const int base = blockIdx.x * kItems + threadIdx.x * 8;
    int c = 0, s = 0;
#pragma unroll
    for (int k = 0; k < 8; k++) {
        c += (base + k < n && clone[base + k]) ? 1 : 0;
        s += (base + k < n && split[base + k]) ? 1 : 0;
    }
    int tc, ts;
    block_exclusive_scan_256(c, s_wave, tc);
    block_exclusive_scan_256(s, s_wave, ts);
    if (threadIdx.x == 0) {
        bc_clone[blockIdx.x] = tc;
        bc_split[blockIdx.x] = ts;
    }
}

// exclusive scan of both rows of workgroup counts in place (one workgroup; any number of counts); counts = {n - S, C, S}
__global__ void __launch_bounds__(256) densify_scan_kernel(int n, int nblocks, int* __restrict__ bc_clone, int* __restrict__ bc_split,
                                                          int* __restrict__ counts_dev)
{
    __shared__ int s_wave[4];
    int carry_c = 0, carry_s = 0;
    for (int b0 = 0; b0 < nblocks; b0 += 256) {
        const int i = b0 + threadIdx.x;
        const int vc = i < nblocks ? bc_clone[i] : 0, vs = i < nblocks ? bc_split[i] : 0;
        int tc, ts;
        const int ec = block_exclusive_scan_256(vc, s_wave, tc);
        const int es = block_exclusive_scan_256(vs, s_wave, ts);
        if (i < nblocks) {
            bc_clone[i] = carry_c + ec;
            bc_split[i] = carry_s + es;
        }
        carry_c += tc;
        carry_s += ts;
    }
    if (threadIdx.x == 0) {
        counts_dev[0] = n - carry_s;
        counts_dev[1] = carry_c;
        counts_dev[2] = carry_s;
    }
}

__global__ void __launch_bounds__(256) densify_index_kernel(int n, const uint8_t* __restrict__ clone, const uint8_t* __restrict__ split,
                                                           const int* __restrict__ bo_clone, const int* __restrict__ bo_split,
                                                           int* __restrict__ kept_index, int* __restrict__ clone_rank,
                                                           int* __restrict__ split_rank)
{
    __shared__ int s_wave[4];
    const int base = blockIdx.x * kItems + threadIdx.x * 8;
    int c = 0, s = 0;
    bool c8[8], s8[8];
#pragma unroll
    for (int k = 0; k < 8; k++) {
        c8[k] = base + k < n && clone[base + k];
        s8[k] = base + k < n && split[base + k];
        c += c8[k] ? 1 : 0;
        s += s8[k] ? 1 : 0;
    }
    int total;
    int pc = bo_clone[blockIdx.x] + block_exclusive_scan_256(c, s_wave, total);
    int ps = bo_split[blockIdx.x] + block_exclusive_scan_256(s, s_wave, total);
#pragma unroll
    for (int k = 0; k < 8; k++)
        if (base + k < n) {
            kept_index[base + k] = s8[k] ? -1 : base + k - ps;      // the rows in front that are not split
            clone_rank[base + k] = c8[k] ? pc : -1;
            split_rank[base + k] = s8[k] ? ps : -1;
            pc += c8[k] ? 1 : 0;
            ps += s8[k] ? 1 : 0;
        }
}

struct DensifyArgs {
    MomDensifyTensor t[MOM_DENSIFY_MAX_TENSORS];
    const int* kept_index;
    const int* clone_rank;
    const int* split_rank;
    const float* xyz;          // the sources the children are made of (null when S == 0)
    const float* scaling;
    const float* rotation;
    const float* z;            // [2S,3] standard normals
    int P, K, C, S;
    float inv_split;           // 1 / (0.8 * 2), as torch forms it for a division by a host scalar
};

// Where source row i goes: d[0] among the kept rows, d[1] among the clones, d[2] and d[3] its two children; -1 = nowhere.
// The comparisons with the counts hold for every plan made by mom_densify_plan; they keep a caller's inconsistent counts from
// becoming a store outside the outputs.
struct RowDst {
    int kept, clone, child0, child1, srank;
};
__device__ __forceinline__ RowDst row_dst(const DensifyArgs& a, int i)
{
    const int ki = a.kept_index[i], cr = a.clone_rank[i], sr = a.split_rank[i];
    RowDst d;
    d.kept = (ki >= 0 && ki < a.K) ? ki : -1;
    d.clone = (cr >= 0 && cr < a.C) ? a.K + cr : -1;
    d.srank = (sr >= 0 && sr < a.S) ? sr : -1;
    d.child0 = d.srank >= 0 ? a.K + a.C + d.srank : -1;
    d.child1 = d.srank >= 0 ? a.K + a.C + a.S + d.srank : -1;
    return d;
}

// The split's children as torch evaluates them (scene/gaussian_model.py:517-526), every operation rounded on its own:
//   stds = exp(scaling);  samples = z * stds + 0;  R = build_rotation(rotation)   (utils/general_utils.py:84-105, the quaternion
//   divided by its norm);  xyz' = bmm(R, samples) + xyz;  scaling' = log(stds / (0.8 * 2)).
// The bmm's three-term sum is accumulated with fused multiply-adds in term order, as the BLAS inner loop does (on an MI355X
// torch.bmm of these shapes equals fma(R2, s2, fma(R1, s1, R0 * s0)) on every row tried, and no uncontracted order); everything
// else is element-wise torch arithmetic and must not contract.
__device__ __forceinline__ float child_xyz(const DensifyArgs& a, int i, int k, int zrow)
{
#pragma clang fp contract(off)
    const float* q4 = a.rotation + (size_t)i * 4;
    const float r0 = q4[0], r1 = q4[1], r2 = q4[2], r3 = q4[3];
    const float nrm = sqrtf((r0 * r0 + r1 * r1) + (r2 * r2 + r3 * r3));      // (torch sums the four squares in pairs)
    const float w = r0 / nrm, x = r1 / nrm, y = r2 / nrm, z = r3 / nrm;
    float m0, m1, m2;
    if (k == 0) {
        m0 = 1.0f - 2.0f * (y * y + z * z);
        m1 = 2.0f * (x * y - w * z);
        m2 = 2.0f * (x * z + w * y);
    } else if (k == 1) {
        m0 = 2.0f * (x * y + w * z);
        m1 = 1.0f - 2.0f * (x * x + z * z);
        m2 = 2.0f * (y * z - w * x);
    } else {
        m0 = 2.0f * (x * z - w * y);
        m1 = 2.0f * (y * z + w * x);
        m2 = 1.0f - 2.0f * (x * x + y * y);
    }
    const float* sc = a.scaling + (size_t)i * 3;
    const float* zz = a.z + (size_t)zrow * 3;
    const float s0 = zz[0] * expf(sc[0]) + 0.0f, s1 = zz[1] * expf(sc[1]) + 0.0f, s2 = zz[2] * expf(sc[2]) + 0.0f;
    float acc = m0 * s0;
    acc = __builtin_fmaf(m1, s1, acc);
    acc = __builtin_fmaf(m2, s2, acc);
    return acc + a.xyz[(size_t)i * 3 + k];
}
// The logarithm is taken in double and rounded once: this toolchain's logf measured up to 1.55 ulp where torch's log stays within
// 1.35, which put the children's scaling 2.05 times as far from float64 as the op-by-op round's; the correctly rounded value is
// never further than either.  Its argument is torch's, bit for bit (expf equals torch.exp on every input tried).
__device__ __forceinline__ float child_scaling(const DensifyArgs& a, float raw)
{
#pragma clang fp contract(off)
    const float x = expf(raw) * a.inv_split;
    return (float)log((double)x);
}

// blockIdx.y = tensor, blockIdx.x = chunk of 256 source rows.  The threads walk the chunk's words in order, so reads are coalesced
// and writes nearly so (each class of rows is contiguous in the output).  WORD = 16 or 4 when row size and alignment allow, else 1.
template <int WORD>
struct WordOf;
template <>
struct WordOf<16> { using T = uint4; };
template <>
struct WordOf<4> { using T = uint32_t; };
template <>
struct WordOf<1> { using T = uint8_t; };

template <int WORD>
__device__ __forceinline__ void copy_chunk(const DensifyArgs& a, const MomDensifyTensor& t)
{
    using T = typename WordOf<WORD>::T;
    const int row0 = blockIdx.x * 256, rows = min(256, a.P - row0);
    const unsigned rw = t.row_bytes / WORD;
    const unsigned words = (unsigned)rows * rw;        // (row_bytes <= MOM_DENSIFY_MAX_ROW_BYTES: no overflow)
    const bool moment = t.role == MOM_DENSIFY_MOMENT;
    const char* __restrict__ src = (const char*)t.src;
    char* __restrict__ dst = (char*)t.dst;
    for (unsigned w = threadIdx.x; w < words; w += 256) {
        const unsigned r = w / rw, c = w - r * rw;
        const int i = row0 + (int)r;
        const RowDst d = row_dst(a, i);
        const T v = *(const T*)(src + ((size_t)i * rw + c) * WORD);
        T fresh = v;                                   // what a clone or a child gets: the row, or zero moments
        if (moment) fresh = T{};
        if (d.kept >= 0) *(T*)(dst + ((size_t)d.kept * rw + c) * WORD) = v;
        if (d.clone >= 0) *(T*)(dst + ((size_t)d.clone * rw + c) * WORD) = fresh;
        if (d.child0 >= 0) {
            *(T*)(dst + ((size_t)d.child0 * rw + c) * WORD) = fresh;
            *(T*)(dst + ((size_t)d.child1 * rw + c) * WORD) = fresh;
        }
    }
}

// _xyz and _scaling: [P,3] floats; kept rows and clones copy, the children are computed
__device__ __forceinline__ void child_chunk(const DensifyArgs& a, const MomDensifyTensor& t)
{
    const int row0 = blockIdx.x * 256, rows = min(256, a.P - row0);
    const float* __restrict__ src = (const float*)t.src;
    float* __restrict__ dst = (float*)t.dst;
    const bool is_xyz = t.role == MOM_DENSIFY_XYZ;
    for (int w = threadIdx.x; w < rows * 3; w += 256) {
        const int r = w / 3, k = w - r * 3;
        const int i = row0 + r;
        const RowDst d = row_dst(a, i);
        const float v = src[(size_t)i * 3 + k];
        if (d.kept >= 0) dst[(size_t)d.kept * 3 + k] = v;
        if (d.clone >= 0) dst[(size_t)d.clone * 3 + k] = v;
        if (d.child0 >= 0) {
            float c0, c1;
            if (is_xyz) {
                c0 = child_xyz(a, i, k, d.srank);
                c1 = child_xyz(a, i, k, a.S + d.srank);
            } else {
                c0 = c1 = child_scaling(a, v);
            }
            dst[(size_t)d.child0 * 3 + k] = c0;
            dst[(size_t)d.child1 * 3 + k] = c1;
        }
    }
}

// a statistics tensor: zero at the new length.  blockIdx.x = chunk of 256 OUTPUT rows; a chunk starts at a multiple of 256 *
// row_bytes, so with a 16-byte aligned tensor every chunk starts 16-byte aligned and only the last one can have a tail.
__device__ __forceinline__ void zero_chunk(const DensifyArgs& a, const MomDensifyTensor& t)
{
    const int nout = a.K + a.C + 2 * a.S;
    const int row0 = blockIdx.x * 256;
    if (row0 >= nout) return;
    const size_t bytes = (size_t)min(256, nout - row0) * t.row_bytes;
    char* __restrict__ dst = (char*)t.dst + (size_t)row0 * t.row_bytes;
    size_t done = 0;
    if (((uintptr_t)t.dst & 15) == 0) {
        const size_t n16 = bytes / 16;
        for (size_t w = threadIdx.x; w < n16; w += 256) *(uint4*)(dst + w * 16) = uint4{0, 0, 0, 0};
        done = n16 * 16;
    }
    for (size_t b = done + threadIdx.x; b < bytes; b += 256) dst[b] = 0;
}

__global__ void __launch_bounds__(256) densify_apply_kernel(DensifyArgs a)
{
    const MomDensifyTensor t = a.t[blockIdx.y];
    if (t.row_bytes == 0) return;
    if (t.role == MOM_DENSIFY_ZERO) {
        zero_chunk(a, t);
        return;
    }
    if ((int)blockIdx.x * 256 >= a.P) return;          // (the grid covers the longer of the input and the output)
    if (t.role == MOM_DENSIFY_XYZ || t.role == MOM_DENSIFY_SCALING) {
        child_chunk(a, t);
        return;
    }
    const uintptr_t al = (uintptr_t)t.src | (uintptr_t)t.dst;
    if ((t.row_bytes & 15) == 0 && (al & 15) == 0) copy_chunk<16>(a, t);
    else if ((t.row_bytes & 3) == 0 && (al & 3) == 0) copy_chunk<4>(a, t);
    else copy_chunk<1>(a, t);
}

}  // namespace

extern "C" size_t mom_densify_scratch_bytes(int P)
{
    const size_t blocks = ((size_t)(P > 0 ? P : 1) + kItems - 1) / kItems;
    return 2 * mom_align_up(blocks * sizeof(int)) + MOM_ALIGN;
}

extern "C" int mom_densify_plan(int P, const uint8_t* clone_mask, const uint8_t* split_mask, int* kept_index, int* clone_rank,
                                int* split_rank, int* counts_dev, int* counts_host, void* scratch, mom_stream_t stream)
{
    if (P < 0) return MOM_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    if (P == 0) {                                       // nothing to scan: zero counts, and nothing is launched for the host's copy
        if (counts_host) counts_host[0] = counts_host[1] = counts_host[2] = 0;
        if (counts_dev && hipMemsetAsync(counts_dev, 0, 3 * sizeof(int), s) != hipSuccess) return MOM_ELAUNCH;
        return MOM_OK;
    }
    if (!clone_mask || !split_mask || !kept_index || !clone_rank || !split_rank || !counts_dev || !scratch) return MOM_EINVAL;
    const int blocks = (P + kItems - 1) / kItems;
    int* bc_clone = (int*)mom_align_ptr(scratch);
    int* bc_split = (int*)((char*)bc_clone + mom_align_up((size_t)blocks * sizeof(int)));
    hipLaunchKernelGGL(densify_count_kernel, dim3(blocks), dim3(256), 0, s, P, clone_mask, split_mask, bc_clone, bc_split);
    hipLaunchKernelGGL(densify_scan_kernel, dim3(1), dim3(256), 0, s, P, blocks, bc_clone, bc_split, counts_dev);
    hipLaunchKernelGGL(densify_index_kernel, dim3(blocks), dim3(256), 0, s, P, clone_mask, split_mask, bc_clone, bc_split, kept_index,
                       clone_rank, split_rank);
    if (hipGetLastError() != hipSuccess) return MOM_ELAUNCH;
    if (counts_host && hipMemcpyAsync(counts_host, counts_dev, 3 * sizeof(int), hipMemcpyDeviceToHost, s) != hipSuccess)
        return MOM_ELAUNCH;
    return MOM_OK;
}

extern "C" int mom_densify_apply(int P, const int* kept_index, const int* clone_rank, const int* split_rank, const int* counts,
                                 const float* z, const MomDensifyTensor* tensors, int count, size_t tensor_size, mom_stream_t stream)
{
    if (P < 0 || count < 0 || count > MOM_DENSIFY_MAX_TENSORS || (count && !tensors)) return MOM_EINVAL;
    if (tensor_size != sizeof(MomDensifyTensor)) return MOM_EINVAL;
    DensifyArgs a = {};
    if (P > 0) {
        if (!kept_index || !clone_rank || !split_rank || !counts) return MOM_EINVAL;
        a.K = counts[0], a.C = counts[1], a.S = counts[2];
        if (a.C < 0 || a.S < 0 || a.C > P || a.S > P || a.K != P - a.S) return MOM_EINVAL;
    }
    for (int i = 0; i < count; i++) {
        const MomDensifyTensor& t = tensors[i];
        a.t[i] = t;
        if (t.role < MOM_DENSIFY_COPY || t.role > MOM_DENSIFY_ZERO) return MOM_EINVAL;
        if (t.row_bytes == 0) continue;
        if (t.row_bytes > MOM_DENSIFY_MAX_ROW_BYTES) return MOM_EINVAL;
        if (!t.dst || (t.role != MOM_DENSIFY_ZERO && !t.src)) return MOM_EINVAL;
        const bool al4 = (((uintptr_t)t.src | (uintptr_t)t.dst) & 3) == 0;
        if (t.role == MOM_DENSIFY_XYZ) {
            if (t.row_bytes != 12 || !al4 || a.xyz) return MOM_EINVAL;
            a.xyz = (const float*)t.src;
        } else if (t.role == MOM_DENSIFY_SCALING) {
            if (t.row_bytes != 12 || !al4 || a.scaling) return MOM_EINVAL;
            a.scaling = (const float*)t.src;
        } else if (t.role == MOM_DENSIFY_ROTATION) {
            if (t.row_bytes != 16 || !al4 || a.rotation) return MOM_EINVAL;
            a.rotation = (const float*)t.src;
        }
    }
    // a split makes children of all three: an xyz or scaling row without the other two (or without the normals) is refused
    if (a.S > 0 && (!a.xyz || !a.scaling || !a.rotation || !z)) return MOM_EINVAL;
    if (count == 0) return MOM_OK;
    const long long nout = (long long)a.K + a.C + 2LL * a.S;
    if (nout > 0x7fffffffLL) return MOM_EINVAL;
    const long long longest = nout > P ? nout : P;
    if (longest == 0) return MOM_OK;
    a.kept_index = kept_index, a.clone_rank = clone_rank, a.split_rank = split_rank;
    a.z = z;
    a.P = P;
    a.inv_split = 1.0f / (float)(0.8 * 2);
    hipLaunchKernelGGL(densify_apply_kernel, dim3((unsigned)((longest + 255) / 256), count), dim3(256), 0, (hipStream_t)stream, a);
    return hipGetLastError() == hipSuccess ? MOM_OK : MOM_ELAUNCH;
}
