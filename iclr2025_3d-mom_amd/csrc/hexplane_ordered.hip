// The ordered HexPlane backward (include/mom4d.h, "ordered HexPlane backward"), gfx950: plane gradients and position gradients that
// are a function of their inputs, bit for bit.  A PULL form -- a texel's gradient is computed by the texel's owner from the points
// of the four cells around it -- with no float atomic anywhere:
//
//   gather     per (point, level): the six samples, gv(plane) = dfeat * (product of the other five) stored as one row per plane in
//              POINT order, and the level's share of the position gradient stored per level (the levels meet in ordered_dxyz_kernel);
//   orders     per (level, plane): key = texel cell y0 * W + x0 of every point, the four corner weights beside it, a stable LSD sort
//              of (key, g) from the identity (knn.hip: its only atomics count integers) -- so a cell's points are consecutive and
//              ascending in g -- the first sorted position of every cell by binary search, and an exclusive scan of the cells'
//              block counts (a block = 64 consecutive terms from the segment's start);
//   block sums one lane group per block, all blocks of a plane in parallel: the block's terms left to right, for the four corner
//              weights at once (a cell is the nw cell of one texel, the ne cell of the next, ...);
//   texels     one lane group per texel: the block sums of each of its four cells left to right, the four classes as
//              (nw + ne) + (sw + se), one add onto what the gradient buffer held.
//
// With one timestamp a space-time plane has W occupied cells of P / W points each: their ~P / 64 blocks are summed by as many
// lane groups at once, and a texel's owner only walks block sums (P / (64 W) rows per class), never the points.
// Lane = channel in every kernel that touches rows, so a row read is one coalesced 128- or 64-byte request.
// THIS FILE IS COMPILED WITH -ffp-contract=off: the host twin at its end must multiply and add exactly as the kernels do.
#include "hexplane_dev.h"
#include <vector>

int mom_sort_pairs_u32(int n, int bits, unsigned* keys[2], unsigned* vals[2], unsigned* counts, hipStream_t s);   // knn.hip
size_t mom_sort_pairs_counts_bytes(int n);

namespace {

constexpr int kBlk = 64;              // terms per block (include/mom4d.h)
constexpr int kPlaneA[6] = {0, 0, 0, 1, 1, 2}, kPlaneB[6] = {1, 2, 3, 2, 3, 3};     // kCombA / kCombB for the host

template <int C> __device__ __forceinline__ float group_sum(float v)
{
    // sum over the C lanes of this group (xor butterflies below C never leave it): the gathers' own reduction, a fixed tree
#pragma unroll
    for (int d = C / 2; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

// ---- gather: hexplane_bwd_kernel's arithmetic with stores where it has atomics --------------------------------------------------
// grid: one group of C lanes per (point, level).  gv [levels][6][P][C], part [levels][P][3].
template <int C>
__global__ void __launch_bounds__(256)
ordered_gather_kernel(HexArgs a, const float* __restrict__ xyz, const float* __restrict__ dfeat, float* __restrict__ gvbuf,
                      float* __restrict__ part)
{
    const int ch = threadIdx.x & (C - 1);
    const long long unit = (long long)blockIdx.x * (256 / C) + threadIdx.x / C;
    const int gi = (int)(unit / a.levels), lvl = (int)(unit % a.levels);
    if (gi >= a.P) return;
    const int g = a.order ? (int)a.order[gi] : gi;     // processing order (speed only): every store below is addressed by g
    if (g < 0 || g >= a.P) return;                     // not a permutation: nothing outside the buffers is touched
    float c[4];
    norm_coords(a, xyz, g, c);
    PlaneSample s[6];
    float v[6], t00[6], t01[6], t10[6], t11[6];
#pragma unroll
    for (int p = 0; p < 6; p++) {
        const int ca = kCombA[p], cb = kCombB[p];
        s[p] = make_sample(c[ca], c[cb], a.res[lvl][ca], a.res[lvl][cb]);
        const float* __restrict__ pl = a.planes[lvl][p];
        t00[p] = s[p].i00 >= 0 ? pl[(size_t)s[p].i00 * C + ch] : 0.f;
        t01[p] = s[p].i01 >= 0 ? pl[(size_t)s[p].i01 * C + ch] : 0.f;
        t10[p] = s[p].i10 >= 0 ? pl[(size_t)s[p].i10 * C + ch] : 0.f;
        t11[p] = s[p].i11 >= 0 ? pl[(size_t)s[p].i11 * C + ch] : 0.f;
        float acc = 0.f;
        acc += t00[p] * s[p].w00;
        acc += t01[p] * s[p].w01;
        acc += t10[p] * s[p].w10;
        acc += t11[p] * s[p].w11;
        v[p] = acc;
    }
    const float go = dfeat[(size_t)g * (a.levels * C) + lvl * C + ch];
    float pre[7], suf[7];
    pre[0] = 1.f;
#pragma unroll
    for (int p = 0; p < 6; p++) pre[p + 1] = pre[p] * v[p];
    suf[6] = 1.f;
#pragma unroll
    for (int p = 5; p >= 0; p--) suf[p] = suf[p + 1] * v[p];
    float gc[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int p = 0; p < 6; p++) {
        const float gv = go * pre[p] * suf[p + 1];
        gvbuf[(((size_t)lvl * 6 + p) * (size_t)a.P + (size_t)g) * C + ch] = gv;
        // grid gradient (ATen grid_sampler_2d backward): with x1 = x0+1, y1 = y0+1
        const float x0 = (float)s[p].ixn, y0 = (float)s[p].iyn, x1 = x0 + 1.f, y1 = y0 + 1.f;
        float gix = 0.f, giy = 0.f;
        gix -= t00[p] * (y1 - s[p].iy) * gv;
        giy -= t00[p] * (x1 - s[p].ix) * gv;
        gix += t01[p] * (y1 - s[p].iy) * gv;
        giy -= t01[p] * (s[p].ix - x0) * gv;
        gix -= t10[p] * (s[p].iy - y0) * gv;
        giy += t10[p] * (x1 - s[p].ix) * gv;
        gix += t11[p] * (s[p].iy - y0) * gv;
        giy += t11[p] * (s[p].ix - x0) * gv;
        const int ca = kCombA[p], cb = kCombB[p];
        if (ca < 3) gc[ca] += gix * s[p].gx_mul;
        if (cb < 3) gc[cb] += giy * s[p].gy_mul;
    }
    if (part) {
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const float tot = group_sum<C>(gc[k]) * (2.0f / (a.a1[k] - a.a0[k]));
            if (ch == 0) part[((size_t)lvl * (size_t)a.P + (size_t)g) * 3 + k] = tot;
        }
    }
}

// ---- orders ---------------------------------------------------------------------------------------------------------------------
// key = the texel cell of the point's CURRENT position (norm_coord / unnorm_clip / floorf as plane_key_kernel has them, through
// make_sample), y0 * Wd + x0; the second coordinate of a space-time plane is the shared timestamp, so its cells all lie in ONE row
// (the timestamp's) and the key is x0 alone: W cells, one sort pass.  The four corner weights are make_sample's (ATen's).  A
// coordinate that is not a number must not become an index: the cell is clamped into the plane.
__global__ void __launch_bounds__(256)
ordered_key_kernel(HexArgs a, int ca, int cb, int Wd, int Hd, const float* __restrict__ xyz, unsigned* __restrict__ keys,
                   unsigned* __restrict__ idx, float4* __restrict__ wts)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.P) return;
    const float cx = norm_coord(xyz[3 * (size_t)i + ca], a.a0[ca], 2.0f / (a.a1[ca] - a.a0[ca]));
    const float cy = cb < 3 ? norm_coord(xyz[3 * (size_t)i + cb], a.a0[cb], 2.0f / (a.a1[cb] - a.a0[cb])) : a.time;
    const PlaneSample s = make_sample(cx, cy, Wd, Hd);
    const int x0 = min(max(s.ixn, 0), Wd - 1), y0 = min(max(s.iyn, 0), Hd - 1);
    keys[i] = cb < 3 ? (unsigned)(y0 * Wd + x0) : (unsigned)x0;
    idx[i] = (unsigned)i;
    wts[i] = make_float4(s.w00, s.w01, s.w10, s.w11);
}

// seg[c] = the first sorted position whose key is >= c, c = 0 .. ncells (seg[ncells] = P)
__global__ void __launch_bounds__(256) ordered_segments_kernel(int P, int ncells, const unsigned* __restrict__ sorted_keys, unsigned* __restrict__ seg)
{
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c > ncells) return;
    int lo = 0, hi = P;
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (sorted_keys[mid] < (unsigned)c) lo = mid + 1;
        else hi = mid;
    }
    seg[c] = (unsigned)lo;
}

// bbase[c] = exclusive scan of the cells' block counts ceil(n_c / 64), c = 0 .. ncells (bbase[ncells] = all blocks).  One workgroup:
// integer sums, sixteen consecutive cells per thread, 16 384 cells a trip (the 128 x 128 planes of the shipped field: one trip).
constexpr int kScanPer = 16;
__global__ void __launch_bounds__(1024) ordered_blocks_kernel(int ncells, const unsigned* __restrict__ seg, unsigned* __restrict__ bbase)
{
    __shared__ unsigned s_v[1024];
    const int tid = threadIdx.x;
    unsigned carry = 0;
    for (int c0 = 0; c0 < ncells; c0 += 1024 * kScanPer) {
        const int c = c0 + tid * kScanPer;
        unsigned n[kScanPer], mine = 0;
#pragma unroll
        for (int i = 0; i < kScanPer; i++) {
            n[i] = c + i < ncells ? (seg[c + i + 1] - seg[c + i] + (kBlk - 1)) / kBlk : 0u;
            mine += n[i];
        }
        s_v[tid] = mine;
        __syncthreads();
        for (int d = 1; d < 1024; d <<= 1) {
            const unsigned t = tid >= d ? s_v[tid - d] : 0u;
            __syncthreads();
            s_v[tid] += t;
            __syncthreads();
        }
        unsigned at = carry + s_v[tid] - mine;
#pragma unroll
        for (int i = 0; i < kScanPer; i++) {
            if (c + i < ncells) bbase[c + i] = at;
            at += n[i];
        }
        carry += s_v[1023];
        __syncthreads();
    }
    if (tid == 0) bbase[ncells] = carry;
}

// ---- block sums: one group per block, terms left to right from +0.0, the four corner weights at once -----------------------------
// bsum [block][4][C].  Loads go out eight terms at a time; the additions stay in term order.
template <int C>
__global__ void __launch_bounds__(256)
ordered_block_sum_kernel(int ncells, unsigned maxblocks, const unsigned* __restrict__ seg, const unsigned* __restrict__ bbase,
                         const unsigned* __restrict__ sorted_g, const float4* __restrict__ wts, const float* __restrict__ gvp /* [P][C] */,
                         float* __restrict__ bsum)
{
    const int ch = threadIdx.x & (C - 1);
    const unsigned b = blockIdx.x * (256 / C) + threadIdx.x / C;
    const unsigned nblk = min(bbase[ncells], maxblocks);
    if (b >= nblk) return;
    // the cell of block b: the last c with bbase[c] <= b (an empty cell shares its base with its successor and is never the last)
    int lo = 0, hi = ncells;                 // first index in [0, ncells] with bbase[index] > b
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (bbase[mid] <= b) lo = mid + 1;
        else hi = mid;
    }
    const int cell = lo - 1;
    const unsigned pos0 = seg[cell] + (b - bbase[cell]) * kBlk;
    const int cnt = (int)min((unsigned)kBlk, seg[cell + 1] - pos0);
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    for (int t0 = 0; t0 < cnt; t0 += 8) {
        float r[8];
        float4 w[8];
#pragma unroll
        for (int u = 0; u < 8; u++) {
            const unsigned g = sorted_g[pos0 + min(t0 + u, cnt - 1)];
            r[u] = gvp[(size_t)g * C + ch];
            w[u] = wts[g];
        }
#pragma unroll
        for (int u = 0; u < 8; u++) {
            if (t0 + u < cnt) {
                s0 = s0 + r[u] * w[u].x;
                s1 = s1 + r[u] * w[u].y;
                s2 = s2 + r[u] * w[u].z;
                s3 = s3 + r[u] * w[u].w;
            }
        }
    }
    float* __restrict__ o = bsum + (size_t)b * 4 * C + ch;
    o[0] = s0;
    o[C] = s1;
    o[2 * C] = s2;
    o[3 * C] = s3;
}

// ---- texels: one group per texel (y, x): class k takes cell (y - (k >> 1), x - (k & 1)) with corner weight k -------------------
// The launch covers the texel rows [y_base, y_base + rows); the cell tables hold the cell rows [cell_row0, cell_row0 + cell_rows): all
// of them for a space plane, the timestamp's single row -- and the two texel rows it reaches -- for a space-time plane.
template <int C>
__global__ void __launch_bounds__(256)
ordered_texel_kernel(int Wd, int y_base, int rows, int cell_row0, int cell_rows, unsigned maxblocks, const unsigned* __restrict__ bbase,
                     const float* __restrict__ bsum, float* __restrict__ grad)
{
    const int ch = threadIdx.x & (C - 1);
    const int loc = blockIdx.x * (256 / C) + threadIdx.x / C;
    if (loc >= Wd * rows) return;
    const int y = y_base + loc / Wd, x = loc % Wd, tex = y * Wd + x;
    float s[4] = {0.f, 0.f, 0.f, 0.f};
    bool any = false;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int cx = x - (k & 1), cy = y - (k >> 1);
        if (cx < 0 || cy < cell_row0 || cy >= cell_row0 + cell_rows) continue;
        const int cell = (cy - cell_row0) * Wd + cx;
        const unsigned b0 = min(bbase[cell], maxblocks), b1 = min(bbase[cell + 1], maxblocks);
        if (b1 > b0) any = true;
        const float* __restrict__ src = bsum + (size_t)k * C + ch;
        float acc = 0.f;
        for (unsigned b = b0; b < b1; b++) acc = acc + src[(size_t)b * 4 * C];
        s[k] = acc;
    }
    if (!any) return;
    const float T = (s[0] + s[1]) + (s[2] + s[3]);
    float* __restrict__ d = grad + (size_t)tex * C + ch;
    *d = *d + T;
}

// dxyz[g][k] += ((part_0 + part_1) + part_2) + part_3 over the levels there are
__global__ void __launch_bounds__(256) ordered_dxyz_kernel(int P, int levels, const float* __restrict__ part, float* __restrict__ dxyz)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x, n = (size_t)P * 3;
    if (i >= n) return;
    float v = part[i];
    for (int l = 1; l < levels; l++) v = v + part[(size_t)l * n + i];
    dxyz[i] = dxyz[i] + v;
}

// ---- the host's coordinate arithmetic: norm_coord, unnorm_clip and make_sample's weights, restated (no contraction in this file) ----
inline float h_norm_coord(float x, float lo, float scale)
{
    const float m = (x - lo) * scale;
    return m - 1.0f;
}
inline float h_unnorm_clip(float c, int size)
{
    float v = ((c + 1.f) / 2.f) * (float)(size - 1);
    if (v <= 0.f) v = 0.f;
    else if (v >= (float)(size - 1)) v = (float)(size - 1);
    return v;
}

// the cell of the shared timestamp along a time axis of `size` texels, clamped into the plane like the key kernel's
inline int h_time_cell(float time, int size)
{
    const float f = floorf(h_unnorm_clip(time, size));
    const int t0 = f >= 0.f && f <= 65536.f ? (int)f : 0;
    return t0 > size - 1 ? size - 1 : t0;
}

// ---- what the call takes ---------------------------------------------------------------------------------------------------------
// Cells and texels are indexed with int and a texel row with (index * C) in size_t: a plane is taken when W * H * (4 C bytes) stays
// below 2^31, as planes_fit32 (hexplane.hip) asks of the chunked kernels -- which also keeps every key far inside 32 bits -- and every
// resolution within 1 .. 65536.  Everything indexed by the point (gv rows, weights, sorted positions) is addressed in size_t; the
// point index itself is formed as an int from the workgroup index (block * 256 + thread, the sort's tiles): P <= 2^30 keeps it one.
constexpr int kMaxPoints = 1 << 30;
bool ordered_takes(const MomHexPlane* hp, int P)
{
    if (!hp || (hp->channels != 32 && hp->channels != 16) || hp->levels < 1 || hp->levels > 4 || P < 0 || P > kMaxPoints) return false;
    for (int l = 0; l < hp->levels; l++) {
        for (int k = 0; k < 4; k++)
            if (hp->res[l][k] < 1 || hp->res[l][k] > 65536) return false;
        for (int p = 0; p < 6; p++)
            if ((unsigned long long)hp->res[l][kPlaneA[p]] * (unsigned long long)hp->res[l][kPlaneB[p]] * (4ull * hp->channels) >= (1ull << 31)) return false;
    }
    return true;
}

struct OrderedView {
    float* gv;            // [levels][6][P][C]
    float* part;          // [levels][P][3]
    unsigned* keys[2];
    unsigned* vals[2];
    unsigned* counts;
    float4* wts;          // [P]
    unsigned* seg;        // [maxcells + 1]
    unsigned* bbase;      // [maxcells + 1]
    float* bsum;          // [maxblocks][4][C]
    size_t maxblocks;
};

size_t ordered_view(const MomHexPlane* hp, int P, char* base, OrderedView* v)
{
    const size_t n = (size_t)(P > 0 ? P : 1), C = (size_t)hp->channels, L = (size_t)hp->levels;
    size_t maxcells = 1;
    for (int l = 0; l < hp->levels; l++)
        for (int p = 0; p < 6; p++) {
            const size_t cells = (size_t)hp->res[l][kPlaneA[p]] * (size_t)hp->res[l][kPlaneB[p]];
            if (cells > maxcells) maxcells = cells;
        }
    // sum over the cells of ceil(n_c / 64) <= P / 64 + (occupied cells)
    const size_t maxblocks = n / kBlk + (n < maxcells ? n : maxcells) + 1;
    size_t off = 0;
    const size_t o_gv = off; off = mom_align_up(off + L * 6 * n * C * 4);
    const size_t o_pt = off; off = mom_align_up(off + L * n * 3 * 4);
    size_t o_k[2], o_v[2];
    for (int i = 0; i < 2; i++) { o_k[i] = off; off = mom_align_up(off + n * 4); }
    for (int i = 0; i < 2; i++) { o_v[i] = off; off = mom_align_up(off + n * 4); }
    const size_t o_c = off; off = mom_align_up(off + mom_sort_pairs_counts_bytes(P));
    const size_t o_w = off; off = mom_align_up(off + n * 16);
    const size_t o_s = off; off = mom_align_up(off + (maxcells + 1) * 4);
    const size_t o_b = off; off = mom_align_up(off + (maxcells + 1) * 4);
    const size_t o_bs = off; off = mom_align_up(off + maxblocks * 4 * C * 4);
    if (v) {
        v->gv = (float*)(base + o_gv);
        v->part = (float*)(base + o_pt);
        for (int i = 0; i < 2; i++) { v->keys[i] = (unsigned*)(base + o_k[i]); v->vals[i] = (unsigned*)(base + o_v[i]); }
        v->counts = (unsigned*)(base + o_c);
        v->wts = (float4*)(base + o_w);
        v->seg = (unsigned*)(base + o_s);
        v->bbase = (unsigned*)(base + o_b);
        v->bsum = (float*)(base + o_bs);
        v->maxblocks = maxblocks;
    }
    return off + MOM_ALIGN;
}

template <int C>
int ordered_launch(const MomHexPlane* hp, const HexArgs& a, const float* xyz, const float* dfeat, float* dxyz, const OrderedView& v, hipStream_t s)
{
    const int P = a.P;
    constexpr int kUnits = 256 / C;
    const long long units = (long long)P * hp->levels;
    hipLaunchKernelGGL(ordered_gather_kernel<C>, dim3((unsigned)((units + kUnits - 1) / kUnits)), dim3(256), 0, s, a, xyz, dfeat, v.gv,
                       dxyz ? v.part : (float*)nullptr);
    if (hipGetLastError() != hipSuccess) return MOM_ELAUNCH;
    const unsigned pblocks = (unsigned)(((size_t)P + 255) / 256);
    for (int l = 0; l < hp->levels; l++)
        for (int p = 0; p < 6; p++) {
            const int ca = kPlaneA[p], cb = kPlaneB[p], Wd = hp->res[l][ca], Hd = hp->res[l][cb];
            // a space-time plane: the one cell row of the timestamp (the host forms it as the kernels do: no contraction in this file)
            const int t0 = cb < 3 ? 0 : h_time_cell(a.time, Hd);
            const int cell_rows = cb < 3 ? Hd : 1, y_base = t0, rows = cb < 3 ? Hd : (t0 + 1 < Hd ? 2 : 1);
            const int ncells = Wd * cell_rows;
            hipLaunchKernelGGL(ordered_key_kernel, dim3(pblocks), dim3(256), 0, s, a, ca, cb, Wd, Hd, xyz, v.keys[0], v.vals[0], v.wts);
            int bits = 1;
            while (bits < 32 && (1ull << bits) < (unsigned long long)ncells) bits++;
            unsigned* keys[2] = {v.keys[0], v.keys[1]};
            unsigned* vals[2] = {v.vals[0], v.vals[1]};
            const int cur = mom_sort_pairs_u32(P, bits, keys, vals, v.counts, s);
            if (cur < 0) return cur;
            hipLaunchKernelGGL(ordered_segments_kernel, dim3((unsigned)((ncells + 1 + 255) / 256)), dim3(256), 0, s, P, ncells, keys[cur], v.seg);
            hipLaunchKernelGGL(ordered_blocks_kernel, dim3(1), dim3(1024), 0, s, ncells, v.seg, v.bbase);
            // at most P / 64 + min(P, cells) blocks (ordered_view): the grid covers them all, a group without a block leaves
            size_t most = (size_t)P / kBlk + ((size_t)P < (size_t)ncells ? (size_t)P : (size_t)ncells) + 1;
            if (most > v.maxblocks) most = v.maxblocks;
            const float* gvp = v.gv + ((size_t)l * 6 + p) * (size_t)P * C;
            hipLaunchKernelGGL(ordered_block_sum_kernel<C>, dim3((unsigned)((most + kUnits - 1) / kUnits)), dim3(256), 0, s, ncells,
                               (unsigned)v.maxblocks, v.seg, v.bbase, vals[cur], v.wts, gvp, v.bsum);
            hipLaunchKernelGGL(ordered_texel_kernel<C>, dim3((unsigned)((Wd * rows + kUnits - 1) / kUnits)), dim3(256), 0, s, Wd, y_base, rows,
                               t0, cell_rows, (unsigned)v.maxblocks, v.bbase, v.bsum, a.grads[l][p]);
            if (hipGetLastError() != hipSuccess) return MOM_ELAUNCH;
        }
    if (dxyz) hipLaunchKernelGGL(ordered_dxyz_kernel, dim3((unsigned)(((size_t)P * 3 + 255) / 256)), dim3(256), 0, s, P, hp->levels, v.part, dxyz);
    return hipGetLastError() == hipSuccess ? MOM_OK : MOM_ELAUNCH;
}

}  // namespace

extern "C" size_t mom_hexplane_ordered_scratch_bytes(const MomHexPlane* hp, int P)
{
    if (!ordered_takes(hp, P)) return 0;
    return ordered_view(hp, P, nullptr, nullptr);
}

extern "C" int mom_hexplane_backward_ordered(const MomHexPlane* hp, int P, const float* xyz, float time, const uint32_t* order,
                                             const float* dfeat, float* dxyz, void* scratch, size_t scratch_bytes, mom_stream_t stream)
{
    if (!ordered_takes(hp, P)) return MOM_EINVAL;
    if (P == 0) return MOM_OK;
    if (!xyz || !dfeat || !scratch) return MOM_EINVAL;
    if (scratch_bytes < ordered_view(hp, P, nullptr, nullptr)) return MOM_EINVAL;
    HexArgs a;
    fill_args(hp, P, nullptr, time, order, true, &a);
    for (int l = 0; l < hp->levels; l++)
        for (int p = 0; p < 6; p++)
            if (!a.planes[l][p] || !a.grads[l][p]) return MOM_EINVAL;
    OrderedView v;
    ordered_view(hp, P, mom_align_ptr(scratch), &v);
    MomProfScope ps(MOM_P_HEX_BWD, (hipStream_t)stream);
    return hp->channels == 32 ? ordered_launch<32>(hp, a, xyz, dfeat, dxyz, v, (hipStream_t)stream)
                              : ordered_launch<16>(hp, a, xyz, dfeat, dxyz, v, (hipStream_t)stream);
}

// The reduction on the host, in the documented order.  hp: levels, channels, res, aabb and grads (HOST buffers in the planes'
// layout, added onto); planes are not read.  gv [levels][6][P][C] and dxyz_part [levels][P][3] as the call leaves them in its scratch.
extern "C" int mom_hexplane_ordered_sum_host(const MomHexPlane* hp, int P, const float* xyz, float time, const float* gv,
                                             const float* dxyz_part, float* dxyz)
{
    if (!ordered_takes(hp, P)) return MOM_EINVAL;
    if (P == 0) return MOM_OK;
    if (!xyz || !gv) return MOM_EINVAL;
    if (dxyz && !dxyz_part) return MOM_EINVAL;
    for (int l = 0; l < hp->levels; l++)
        for (int p = 0; p < 6; p++)
            if (!hp->grads[l][p]) return MOM_EINVAL;
    const int C = hp->channels;
    const size_t n = (size_t)P;
    std::vector<unsigned> key(n), ord(n);
    std::vector<float> w(4 * n);
    std::vector<size_t> seg;
    for (int l = 0; l < hp->levels; l++)
        for (int p = 0; p < 6; p++) {
            const int ca = kPlaneA[p], cb = kPlaneB[p], Wd = hp->res[l][ca], Hd = hp->res[l][cb];
            const size_t ncells = (size_t)Wd * (size_t)Hd;
            seg.assign(ncells + 1, 0);
            for (size_t g = 0; g < n; g++) {
                const float cx = h_norm_coord(xyz[3 * g + ca], hp->aabb[ca], 2.0f / (hp->aabb[3 + ca] - hp->aabb[ca]));
                const float cy = cb < 3 ? h_norm_coord(xyz[3 * g + cb], hp->aabb[cb], 2.0f / (hp->aabb[3 + cb] - hp->aabb[cb])) : time;
                const float ix = h_unnorm_clip(cx, Wd), iy = h_unnorm_clip(cy, Hd);
                const float fx = floorf(ix), fy = floorf(iy);
                int x0 = fx >= 0.f && fx <= 65536.f ? (int)fx : 0, y0 = fy >= 0.f && fy <= 65536.f ? (int)fy : 0;
                const int x1 = x0 + 1, y1 = y0 + 1;
                w[4 * g + 0] = ((float)x1 - ix) * ((float)y1 - iy);
                w[4 * g + 1] = (ix - (float)x0) * ((float)y1 - iy);
                w[4 * g + 2] = ((float)x1 - ix) * (iy - (float)y0);
                w[4 * g + 3] = (ix - (float)x0) * (iy - (float)y0);
                x0 = x0 > Wd - 1 ? Wd - 1 : x0;
                y0 = y0 > Hd - 1 ? Hd - 1 : y0;
                key[g] = (unsigned)(y0 * Wd + x0);
                seg[key[g] + 1]++;
            }
            for (size_t c = 0; c < ncells; c++) seg[c + 1] += seg[c];
            {
                std::vector<size_t> at(seg.begin(), seg.end() - 1);
                for (size_t g = 0; g < n; g++) ord[at[key[g]]++] = (unsigned)g;          // ascending g inside a cell
            }
            const float* gvp = gv + ((size_t)l * 6 + p) * n * C;
            float* grad = hp->grads[l][p];
            for (int y = 0; y < Hd; y++)
                for (int x = 0; x < Wd; x++) {
                    size_t s0[4], s1[4];
                    bool any = false;
                    for (int k = 0; k < 4; k++) {
                        const int cx = x - (k & 1), cy = y - (k >> 1);
                        s0[k] = s1[k] = 0;
                        if (cx < 0 || cy < 0) continue;
                        s0[k] = seg[(size_t)cy * Wd + cx];
                        s1[k] = seg[(size_t)cy * Wd + cx + 1];
                        if (s1[k] > s0[k]) any = true;
                    }
                    if (!any) continue;
                    for (int ch = 0; ch < C; ch++) {
                        float s[4];
                        for (int k = 0; k < 4; k++) {
                            float acc = 0.f;
                            for (size_t b = s0[k]; b < s1[k]; b += kBlk) {
                                float blk = 0.f;
                                const size_t e = b + kBlk < s1[k] ? b + kBlk : s1[k];
                                for (size_t t = b; t < e; t++) {
                                    const size_t g = ord[t];
                                    blk = blk + gvp[g * C + ch] * w[4 * g + k];
                                }
                                acc = acc + blk;
                            }
                            s[k] = acc;
                        }
                        float* d = grad + ((size_t)y * Wd + x) * C + ch;
                        *d = *d + ((s[0] + s[1]) + (s[2] + s[3]));
                    }
                }
        }
    if (dxyz) {
        for (size_t i = 0; i < 3 * n; i++) {
            float v = dxyz_part[i];
            for (int l = 1; l < hp->levels; l++) v = v + dxyz_part[(size_t)l * 3 * n + i];
            dxyz[i] = dxyz[i] + v;
        }
    }
    return MOM_OK;
}
