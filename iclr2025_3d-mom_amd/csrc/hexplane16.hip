// HexPlane feature field for 16-channel planes (kplanes_config output_coordinate_dim = 16), forward and backward, gfx950.
//
// The same arithmetic, in the same order, as the 32-channel kernels of hexplane.hip (ATen's grid_sampler_2d with align_corners and
// border padding; product over the six planes; level-major features), at half the row width: a channel-last texel row is
// 16 floats = 64 bytes, half a cache line.  Sixteen lanes -- a quarter of a wave64 -- own one (point, level): lane c of the group
// owns channel c, so a group's texel fetch is one 64-byte piece and a wave-wide load, store or float atomic is four such pieces
// (the memory side takes atomics in 64-byte requests anyway).  A wave therefore covers four units where the 32-channel forms
// cover two, and everything that was "per half-wave" there is "per group" here: the range of points a group walks, the
// reduction of the position gradient (four butterfly steps, never across a group), the pending rows of the scatter.
//
// LDS records are read as 16-byte broadcasts, one address per group.  ds_read_b128 serves a wave in four sets of sixteen lanes
// that mix two neighbouring groups, so two groups whose records lie a multiple of 256 bytes apart would hit the same banks;
// every record array here carries one 16-byte pad per group, which puts neighbouring groups four banks apart.
//
// Not here: the common-factor-row form and everything fused with the MLP (deform_field.hip) -- those stay 32 channels x 2 levels.
#include "hexplane_dev.h"

namespace {

constexpr int kC = 16;                       // channels = floats of one texel row
constexpr unsigned kRowB = kC * 4u;          // bytes of one texel row / one gv row

__device__ __forceinline__ float group_sum(float v)
{
    // sum over the 16 lanes of this group (xor butterflies never cross bit 4)
#pragma unroll
    for (int d = 8; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

// grid: one group per (point, level); blockDim 256 = 16 groups
__global__ void __launch_bounds__(256) hexplane16_fwd_kernel(HexArgs a, const float* __restrict__ xyz, float* __restrict__ feat)
{
    const int ch = threadIdx.x & 15;
    const long long unit = (long long)blockIdx.x * 16 + (threadIdx.x >> 4);
    const int gi = (int)(unit / a.levels), lvl = (int)(unit % a.levels);
    if (gi >= a.P) return;
    const int g = a.order ? (int)a.order[gi] : gi;
    float c[4];
    norm_coords(a, xyz, g, c);
    float prod = 1.f;
#pragma unroll
    for (int p = 0; p < 6; p++) {
        const int ca = kCombA[p], cb = kCombB[p];
        const int Wd = a.res[lvl][ca], Hd = a.res[lvl][cb];
        const PlaneSample s = make_sample(c[ca], c[cb], Wd, Hd);
        const float* __restrict__ pl = a.planes[lvl][p];
        float v = 0.f;
        if (s.i00 >= 0) v += pl[(size_t)s.i00 * kC + ch] * s.w00;
        if (s.i01 >= 0) v += pl[(size_t)s.i01 * kC + ch] * s.w01;
        if (s.i10 >= 0) v += pl[(size_t)s.i10 * kC + ch] * s.w10;
        if (s.i11 >= 0) v += pl[(size_t)s.i11 * kC + ch] * s.w11;
        prod = prod * v;
    }
    feat[(size_t)g * (a.levels * kC) + lvl * kC + ch] = prod;
}

// generic backward: one group per (point, level), 24 rows of 64 bytes of float atomics each
__global__ void __launch_bounds__(256)
hexplane16_bwd_kernel(HexArgs a, const float* __restrict__ xyz, const float* __restrict__ dfeat, float* __restrict__ dxyz)
{
    const int ch = threadIdx.x & 15;
    const long long unit = (long long)blockIdx.x * 16 + (threadIdx.x >> 4);
    const int g = (int)(unit / a.levels), lvl = (int)(unit % a.levels);
    if (g >= a.P) return;
    float c[4];
    norm_coords(a, xyz, g, c);
    PlaneSample s[6];
    float v[6], t00[6], t01[6], t10[6], t11[6];
#pragma unroll
    for (int p = 0; p < 6; p++) {
        const int ca = kCombA[p], cb = kCombB[p];
        s[p] = make_sample(c[ca], c[cb], a.res[lvl][ca], a.res[lvl][cb]);
        const float* __restrict__ pl = a.planes[lvl][p];
        t00[p] = s[p].i00 >= 0 ? pl[(size_t)s[p].i00 * kC + ch] : 0.f;
        t01[p] = s[p].i01 >= 0 ? pl[(size_t)s[p].i01 * kC + ch] : 0.f;
        t10[p] = s[p].i10 >= 0 ? pl[(size_t)s[p].i10 * kC + ch] : 0.f;
        t11[p] = s[p].i11 >= 0 ? pl[(size_t)s[p].i11 * kC + ch] : 0.f;
        float acc = 0.f;
        acc += t00[p] * s[p].w00;
        acc += t01[p] * s[p].w01;
        acc += t10[p] * s[p].w10;
        acc += t11[p] * s[p].w11;
        v[p] = acc;
    }
    const float go = dfeat[(size_t)g * (a.levels * kC) + lvl * kC + ch];
    float pre[7], suf[7];
    pre[0] = 1.f;
#pragma unroll
    for (int p = 0; p < 6; p++) pre[p + 1] = pre[p] * v[p];
    suf[6] = 1.f;
#pragma unroll
    for (int p = 5; p >= 0; p--) suf[p] = suf[p + 1] * v[p];
    float gc[3] = {0.f, 0.f, 0.f};  // dL/d(normalised x,y,z), this channel's share
#pragma unroll
    for (int p = 0; p < 6; p++) {
        const float gv = go * pre[p] * suf[p + 1];
        float* __restrict__ gp = a.grads[lvl][p];
        if (s[p].i00 >= 0) atomicAdd(&gp[(size_t)s[p].i00 * kC + ch], gv * s[p].w00);
        if (s[p].i01 >= 0) atomicAdd(&gp[(size_t)s[p].i01 * kC + ch], gv * s[p].w01);
        if (s[p].i10 >= 0) atomicAdd(&gp[(size_t)s[p].i10 * kC + ch], gv * s[p].w10);
        if (s[p].i11 >= 0) atomicAdd(&gp[(size_t)s[p].i11 * kC + ch], gv * s[p].w11);
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
    if (dxyz) {
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const float tot = group_sum(gc[k]) * (2.0f / (a.a1[k] - a.a0[k]));
            if (ch == 0) atomicAdd(&dxyz[3 * g + k], tot);  // the levels add into the same slot
        }
    }
}

// =================================================================================================================
// Chunked kernels (one shared timestamp): as in hexplane.hip, the sample parameters of a chunk of 32 points are computed once
// per (point, plane), by one lane, into LDS records (phase A); phase B walks the chunk with lane = channel, each of the wave's
// four groups its own eight points, and reads a point's records as LDS broadcasts.  Workgroups specialise by level.
// =================================================================================================================
constexpr int kChunk = 32;                   // points per wave and chunk: each group walks 8
constexpr int kPerGroup = kChunk / 4;
constexpr int kRecs = kChunk * 6 + 4;        // six records per point, one pad per group (see the head of the file)
__device__ __forceinline__ int rec_idx(int pt, int p) { return pt * 6 + p + (pt >> 3); }

// forward record of one (point, plane): the four corners' byte offsets and their four weights.  bx = ix - x0 and by = iy - y0 are
// exact; ax = 1 - bx, ay = 1 - by are bit-identical to ATen's (x0+1) - ix (Sterbenz), so the four weights are ATen's.  A corner
// that is outside gets weight exactly 0 and is redirected to the texel next to it.
__device__ __forceinline__ void make_rec_fwd(float cx, float cy, int Wd, int Hd, uint4& O, float4& Wt)
{
    float gxm, gym;
    const float ix = unnorm_clip(cx, Wd, gxm), iy = unnorm_clip(cy, Hd, gym);
    const int x0 = (int)floorf(ix), y0 = (int)floorf(iy);
    const unsigned o00 = (unsigned)(y0 * Wd + x0) * kRowB, sx = (x0 + 1 < Wd) ? kRowB : 0u, sy = (y0 + 1 < Hd) ? (unsigned)Wd * kRowB : 0u;
    const float bx = ix - (float)x0, by = iy - (float)y0, ax = 1.f - bx, ay = 1.f - by;
    O = make_uint4(o00, o00 + sx, o00 + sy, o00 + sy + sx);
    Wt = make_float4(ax * ay, bx * ay, ax * by, bx * by);
}

__global__ void __launch_bounds__(256)
hexplane16_fwd4_kernel(HexArgs a, int nchunks, const float* __restrict__ xyz, float* __restrict__ feat)
{
    __shared__ uint4 s_off[4][kRecs];
    __shared__ float4 s_wt[4][kRecs];
    const int lane = threadIdx.x & 63, ch = lane & 15, q = lane >> 4, wv = threadIdx.x >> 6;
    const int lvl = blockIdx.y;
    const int wave = (blockIdx.x * 256 + threadIdx.x) >> 6, nwaves = (gridDim.x * 256) >> 6;
    for (int chunk = wave; chunk < nchunks; chunk += nwaves) {
        const int gi = chunk * kChunk + lane;
        const int g_mine = (lane < kChunk && gi < a.P) ? (a.order ? (int)a.order[gi] : gi) : -1;
        __builtin_amdgcn_wave_barrier();
        if (g_mine >= 0) {
            float c[4];
            norm_coords(a, xyz, g_mine, c);
#pragma unroll
            for (int p = 0; p < 6; p++)
                make_rec_fwd(c[kCombA[p]], c[kCombB[p]], a.res[lvl][kCombA[p]], a.res[lvl][kCombB[p]], s_off[wv][rec_idx(lane, p)],
                             s_wt[wv][rec_idx(lane, p)]);
        }
        __builtin_amdgcn_wave_barrier();
        const int npts = min(kChunk, a.P - chunk * kChunk);
        const int n_grp = max(0, min(kPerGroup, npts - kPerGroup * q));     // this group walks points [8q, 8q + n_grp)
        // (n_grp never grows with q, and point 8q + i lives in a lane of group 0 or 1: the lane a shuffle reads is always active)
        for (int i = 0; i < n_grp; i++) {
            const int pt = kPerGroup * q + i;
            const int g = __shfl(g_mine, pt);
            float prod = 1.f;
#pragma unroll
            for (int p = 0; p < 6; p++) {
                const uint4 o = s_off[wv][rec_idx(pt, p)];
                const float4 w = s_wt[wv][rec_idx(pt, p)];
                const float* __restrict__ pl = a.planes[lvl][p] + ch;
                float v = 0.f;
                v += ld_f32(pl, o.x) * w.x;
                v += ld_f32(pl, o.y) * w.y;
                v += ld_f32(pl, o.z) * w.z;
                v += ld_f32(pl, o.w) * w.w;
                prod = prod * v;
            }
            feat[(size_t)g * (a.levels * kC) + lvl * kC + ch] = prod;
        }
    }
}

// =================================================================================================================
// Backward, one timestamp for all points, in two passes: the six-row form of hexplane.hip (hexplane_bwd5_gather_kernel +
// hexplane_bwd5_scatter_kernel<false>; the description of the scheme is there) with 64-byte rows.
//
//  pass 1 (GATHER, points in `order`, one group per point): per (point, level) the six samples, their product, and per plane
//    gv = dfeat * (product of the other five), STORED at the point's position in the order of the space plane it is scattered
//    with: gvbuf[slot][level][position][space row | time row][16], the two rows of a position one 128-byte line.  The position
//    gradient is reduced over the 16 channels and added to dxyz.
//  pass 2 (SCATTER, per space plane in its own order): every group streams its own contiguous range of positions and keeps four
//    pending texel rows (slot = parity of y, parity of x) and the carried space-time plane's two pending line rows in
//    registers; a row leaves as one 64-byte row of float atomics when its slot takes another row.
// =================================================================================================================

// pass-1 record of one (point, plane): R1 = {byte offset of texel (y0, x0), byte step to x0+1 (0 if outside), byte step to
// y0+1 (0 if outside), byte offset of the point's gv row}; R2 = {bx, by, gx, gy}: the fractions and d(ix)/d(world coordinate)
// (0 when the coordinate was clipped at the border, and for the time axis)
__device__ __forceinline__ void make_rec_gather(float cx, float cy, int Wd, int Hd, unsigned row_off, float gsx, float gsy, uint4& R1, float4& R2)
{
    float gxm, gym;
    const float ix = unnorm_clip(cx, Wd, gxm), iy = unnorm_clip(cy, Hd, gym);
    const int x0 = (int)floorf(ix), y0 = (int)floorf(iy);
    R1 = make_uint4((unsigned)(y0 * Wd + x0) * kRowB, (x0 + 1 < Wd) ? kRowB : 0u, (y0 + 1 < Hd) ? (unsigned)Wd * kRowB : 0u, row_off);
    R2 = make_float4(ix - (float)x0, iy - (float)y0, gxm != 0.f ? gsx : 0.f, gym != 0.f ? gsy : 0.f);
}

__global__ void __launch_bounds__(256, 4)
hexplane16_gather_kernel(HexArgs a, int nchunks, const float* __restrict__ xyz, const float* __restrict__ dfeat,
                         float* __restrict__ dxyz, const uint32_t* __restrict__ inv /* [3][levels][P] */,
                         float* __restrict__ gvbuf /* [3 slots][levels][P][2][16] */)
{
    __shared__ uint4 s_r1[4][kRecs];
    __shared__ float4 s_r2[4][kRecs];
    const int lane = threadIdx.x & 63, ch = lane & 15, q = lane >> 4, wv = threadIdx.x >> 6;
    const int pj = lane & 31, hh = lane >> 5;                           // phase A: point of the chunk, half of its planes
    const int lvl = blockIdx.y;
    const int wave = (blockIdx.x * 256 + threadIdx.x) >> 6, nwaves = (gridDim.x * 256) >> 6;
    const unsigned chb = (unsigned)ch * 4u;
    const size_t plane_floats = (size_t)a.P * kC;                     // one (plane, level) buffer of gv rows
    // d(ix)/d(world coordinate) per axis when the coordinate is not clipped: (size-1)/2 * 2/(aabb1 - aabb0)
    float gscale[4];
#pragma unroll
    for (int k = 0; k < 3; k++) gscale[k] = ((float)(a.res[lvl][k] - 1) / 2.f) * (2.0f / (a.a1[k] - a.a0[k]));
    gscale[3] = 0.f;

    for (int chunk = wave; chunk < nchunks; chunk += nwaves) {
        // phase A: lane j < 32 prepares planes 0..2 of point j, lane 32 + j planes 3..5 of the same point
        const int gi = chunk * kChunk + pj;
        const int g_mine = gi < a.P ? (a.order ? (int)a.order[gi] : gi) : -1;
        __builtin_amdgcn_wave_barrier();
        if (g_mine >= 0) {
            float c[4];
            norm_coords(a, xyz, g_mine, c);
            unsigned pos[3];
#pragma unroll
            for (int k = 0; k < 3; k++) pos[k] = inv[((size_t)k * a.levels + lvl) * a.P + g_mine] * (2u * kRowB);   // a slot's two rows are adjacent
#pragma unroll
            for (int r = 0; r < 3; r++) {
                const int p0 = r, p1 = 3 + r;            // hh == 0: (x,y) (x,z) (x,t); hh == 1: (y,z) (y,t) (z,t)
                const int ca = hh ? kCombA[p1] : kCombA[p0], cb = hh ? kCombB[p1] : kCombB[p0];
                const int slot = hh ? order_slot_of_plane(p1) : order_slot_of_plane(p0);
                uint4 R1; float4 R2;
                make_rec_gather(c[ca], c[cb], a.res[lvl][ca], a.res[lvl][cb], pos[slot], gscale[ca], gscale[cb], R1, R2);
                s_r1[wv][rec_idx(pj, 3 * hh + r)] = R1;
                s_r2[wv][rec_idx(pj, 3 * hh + r)] = R2;
            }
        }
        __builtin_amdgcn_wave_barrier();
        const int npts = min(kChunk, a.P - chunk * kChunk);
        const int n_grp = max(0, min(kPerGroup, npts - kPerGroup * q));     // this group walks points [8q, 8q + n_grp)
        const int pt0 = kPerGroup * q;
        float t00[6], t01[6], t10[6], t11[6];
        float go = 0.f;
        float dx_mine[3] = {0.f, 0.f, 0.f};
        // (n_grp never grows with q, and point 8q + i lives in a lane of group 0 or 1: the lane a shuffle reads is always active)
        auto fetch = [&](int i) {
            const int ng = __shfl(g_mine, pt0 + i);
#pragma unroll
            for (int p = 0; p < 6; p++) {
                const uint4 R1 = s_r1[wv][rec_idx(pt0 + i, p)];
                const float* __restrict__ pl = a.planes[lvl][p];
                const unsigned o = R1.x + chb;
                t00[p] = ld_f32(pl, o);
                t01[p] = ld_f32(pl, o + R1.y);
                t10[p] = ld_f32(pl, o + R1.z);
                t11[p] = ld_f32(pl, o + R1.y + R1.z);
            }
            go = dfeat[(size_t)ng * (a.levels * kC) + lvl * kC + ch];
        };
        if (n_grp > 0) fetch(0);
        for (int i = 0; i < n_grp; i++) {
            // first half of the iteration: consume the texels (bilinear sample and the two raw position derivatives per plane);
            // after it the 24 texel registers are dead and the next point's loads can land in them while the second half runs
            float v[6], dgx[6], dgy[6];
#pragma unroll
            for (int p = 0; p < 6; p++) {
                const float4 R2 = s_r2[wv][rec_idx(pt0 + i, p)];
                const float d0 = t01[p] - t00[p], d1 = t11[p] - t10[p];
                const float tx0 = __builtin_fmaf(R2.x, d0, t00[p]), tx1 = __builtin_fmaf(R2.x, d1, t10[p]);
                const float dy = tx1 - tx0;                          // = ax (t10 - t00) + bx (t11 - t01): d sample / d iy
                v[p] = __builtin_fmaf(R2.y, dy, tx0);
                dgx[p] = __builtin_fmaf(R2.y, d1 - d0, d0) * R2.z;   // (ay (t01 - t00) + by (t11 - t10)) * d ix / d coord
                dgy[p] = dy * R2.w;
            }
            const float gcur = go;
            const int icur = i;
            if (i + 1 < n_grp) fetch(i + 1);
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
                const float gv = gcur * (pre[p] * suf[p + 1]);
                const int ca = kCombA[p], cb = kCombB[p];
                float* __restrict__ dst = gvbuf + ((size_t)order_slot_of_plane(p) * a.levels + lvl) * 2 * plane_floats + ((p == 2 || p == 4 || p == 5) ? kC : 0);          // uniform
                *reinterpret_cast<float*>(reinterpret_cast<char*>(dst) + (s_r1[wv][rec_idx(pt0 + icur, p)].w + chb)) = gv;
                gc[ca] = __builtin_fmaf(gv, dgx[p], gc[ca]);
                if (cb < 3) gc[cb] = __builtin_fmaf(gv, dgy[p], gc[cb]);
            }
            if (dxyz) {
#pragma unroll
                for (int k = 0; k < 3; k++) {
                    const float tot = group_sum(gc[k]);
                    if (ch == icur) dx_mine[k] = tot;                    // lane i of the group keeps point 8q + i's total
                }
            }
        }
        if (dxyz) {
            const int gp = __shfl(g_mine, pt0 + (ch & (kPerGroup - 1)));  // lanes 0..7 of each group: point 8q + ch
            if (ch < n_grp && gp >= 0) {
#pragma unroll
                for (int k = 0; k < 3; k++) atomicAdd(&dxyz[3 * gp + k], dx_mine[k]);   // the other levels add their share too
            }
        }
    }
}

// pass 2: blockIdx.y = order slot (0: (x,y) + (x,t), 1: (x,z) + (z,t), 2: (y,z) + (y,t)); blockIdx.z = level.  Each GROUP walks
// its own contiguous range of sorted positions, one chunk = one batch of 16 positions at a time.
constexpr int kChunkS = 16;            // sorted positions per group and chunk = gv rows in flight per lane and plane
constexpr int kRecS = 4 + 4 + 4 + 2;   // dwords of one pass-2 record: int4 ids | float4 ws | float4 {lw0, lw1, flag, -} | int2 ride ids
constexpr int kSlotsS = 64 + 4;        // one record per lane, one pad per group

__global__ void __launch_bounds__(256)
hexplane16_scatter_kernel(HexArgs a, int per_group, const float* __restrict__ xyz,
                          const uint32_t* __restrict__ order /* [3][levels][P] */, const float* __restrict__ gvbuf)
{
    extern __shared__ float s_dyn16[];                 // [4 waves] x (int4 ids[68] | float4 ws[68] | float4 rd[68] | int2 rid[68]) | line [W][16]
    constexpr int kPer = kSlotsS * kRecS;              // dwords per wave
    float* s_line = s_dyn16 + 4 * kPer;
    const int lane = threadIdx.x & 63, ch = lane & 15, q = lane >> 4, wv = threadIdx.x >> 6;
    const int si = blockIdx.y, lvl = blockIdx.z;
    const int p = si == 0 ? 0 : (si == 1 ? 1 : 3), ca = si == 2 ? 1 : 0, cb = si == 0 ? 1 : 2;
    const int pt = si == 0 ? 2 : (si == 1 ? 5 : 4);    // the space-time plane carried along: shares axis `cs` with this plane
    const bool ride_on_b = si == 1;                     // (x,z) carries (z,t): the shared axis is this plane's second one
    const int cs = ride_on_b ? cb : ca;
    const int Wd = a.res[lvl][ca], Hd = a.res[lvl][cb], Ws = a.res[lvl][cs];
    float* __restrict__ gp = a.grads[lvl][p] + ch;
    const size_t plane_floats = (size_t)a.P * kC;
    const float* __restrict__ src_s = gvbuf + ((size_t)si * a.levels + lvl) * 2 * plane_floats + ch;    // [position][space row | time row][16]
    const float* __restrict__ src_t = src_s + kC;
    constexpr int kRowF = 2 * kC;                      // floats between consecutive positions
    const uint32_t* __restrict__ ord = order + ((size_t)si * a.levels + lvl) * a.P;
    const float lo_a = a.a0[ca], sc_a = 2.0f / (a.a1[ca] - a.a0[ca]), lo_b = a.a0[cb], sc_b = 2.0f / (a.a1[cb] - a.a0[cb]);
    float* __restrict__ my_line = s_line + ch;
    for (int i = threadIdx.x; i < Ws * kC; i += 256) s_line[i] = 0.f;
    __syncthreads();

    int pid[4] = {-1, -1, -1, -1};
    float pacc[4] = {0.f, 0.f, 0.f, 0.f};
    int lpid[2] = {-1, -1};
    float lacc[2] = {0.f, 0.f};
    int prev_cell = -1, prev_row = -1;                  // of the position before this chunk (uniform per group)
    // this group's contiguous range of sorted positions
    const long long grp = ((long long)blockIdx.x * 4 + wv) * 4 + q;
    const long long r_begin = grp * per_group;
    const int r_end = (int)(r_begin + per_group < (long long)a.P ? r_begin + per_group : (long long)a.P);
    float* rec = s_dyn16 + wv * kPer;
    int4* w_ids = reinterpret_cast<int4*>(rec);
    float4* w_ws = reinterpret_cast<float4*>(rec + 4 * kSlotsS);
    float4* w_rd = reinterpret_cast<float4*>(rec + 8 * kSlotsS);
    int2* w_rid = reinterpret_cast<int2*>(rec + 12 * kSlotsS);
    const int sl0 = (kChunkS + 1) * q;                  // this group's first record
    for (long long base_ll = r_begin; base_ll < r_end; base_ll += kChunkS) {
        const int base = (int)base_ll;
        const int npts = min(kChunkS, r_end - base);
        // phase A: lane (16 q + j) prepares position base + j of its group: corner ids and weights, already permuted into their
        // slots.  Slot k takes corner k ^ s, s = 2 (y0 & 1) + (x0 & 1): the four corners of a texel always take four different
        // slots and a row keeps its slot when the walk moves to a neighbouring texel.  The carried plane's two line rows take the
        // slot of their parity the same way.  A position whose cell (ride row) equals its predecessor's, both with every corner
        // inside, gets flag bit 0 (1) clear: phase B then only accumulates, without looking at the ids.
        __builtin_amdgcn_wave_barrier();
        {
            const bool on = ch < npts;
            const int g = (int)ord[base + (on ? ch : 0)];
            const float cx = norm_coord(xyz[3 * g + ca], lo_a, sc_a), cy = norm_coord(xyz[3 * g + cb], lo_b, sc_b);     // the gather's cells
            float gxm, gym;
            const float ix = unnorm_clip(cx, Wd, gxm), iy = unnorm_clip(cy, Hd, gym);
            const int x0 = (int)floorf(ix), y0 = (int)floorf(iy);
            const bool hx = x0 + 1 < Wd, hy = y0 + 1 < Hd;
            const int o00 = (y0 * Wd + x0) * kC;
            const float bx = ix - (float)x0, by = iy - (float)y0, ax = 1.f - bx, ay = 1.f - by;
            const int ids[4] = {o00, hx ? o00 + kC : -2, hy ? o00 + Wd * kC : -2, (hx && hy) ? o00 + Wd * kC + kC : -2};
            const float ws[4] = {ax * ay, bx * ay, ax * by, bx * by};
            const bool sx1 = x0 & 1, sy1 = y0 & 1;
            const int i0 = sx1 ? ids[1] : ids[0], i1 = sx1 ? ids[0] : ids[1], i2 = sx1 ? ids[3] : ids[2], i3 = sx1 ? ids[2] : ids[3];
            const float f0 = sx1 ? ws[1] : ws[0], f1 = sx1 ? ws[0] : ws[1], f2 = sx1 ? ws[3] : ws[2], f3 = sx1 ? ws[2] : ws[3];
            // carried plane: rows r0 (weight 1 - b) and r0 + 1 (weight b) along the shared axis
            const int r0 = ride_on_b ? y0 : x0;
            const bool hr = ride_on_b ? hy : hx;
            const float bw = ride_on_b ? by : bx, aw = 1.f - bw;
            const bool odd = r0 & 1;
            const int ra = r0 * kC, rb = hr ? (r0 + 1) * kC : -2;
            // run detection: a position with a corner outside gets a unique negative value, so neither it nor its successor
            // compares equal
            const int cell = (hx && hy) ? o00 : -2 - ch, row = hr ? r0 : -2 - ch;
            int pc = __shfl_up(cell, 1), pr = __shfl_up(row, 1);
            if (ch == 0) { pc = prev_cell; pr = prev_row; }
            const int flag = (cell != pc ? 1 : 0) | (row != pr ? 2 : 0);
            prev_cell = __shfl(cell, 16 * q + max(npts, 1) - 1);
            prev_row = __shfl(row, 16 * q + max(npts, 1) - 1);
            if (on) {
                w_ids[sl0 + ch] = make_int4(sy1 ? i2 : i0, sy1 ? i3 : i1, sy1 ? i0 : i2, sy1 ? i1 : i3);
                w_ws[sl0 + ch] = make_float4(sy1 ? f2 : f0, sy1 ? f3 : f1, sy1 ? f0 : f2, sy1 ? f1 : f3);
                w_rd[sl0 + ch] = make_float4(odd ? bw : aw, odd ? aw : bw, __int_as_float(flag), 0.f);
                w_rid[sl0 + ch] = make_int2(odd ? rb : ra, odd ? ra : rb);
            }
        }
        __builtin_amdgcn_wave_barrier();
        // phase B: the gv rows of this order are consecutive in memory: the chunk's rows are loaded, then consumed with no
        // vector-memory wait inside (the rare atomics never sit between a load and its use)
        float val[kChunkS], vat[kChunkS];
#pragma unroll
        for (int j = 0; j < kChunkS; j++) {
            const int r = min(j, npts - 1);
            val[j] = src_s[(size_t)(base + r) * kRowF];
            vat[j] = src_t[(size_t)(base + r) * kRowF];
        }
#pragma unroll
        for (int j = 0; j < kChunkS; j++) {
            if (j >= npts) continue;
            const float4 w4 = w_ws[sl0 + j];
            const float4 rd = w_rd[sl0 + j];
            const int flag = __float_as_int(rd.z);
            const float ws[4] = {w4.x, w4.y, w4.z, w4.w};
            const float lw[2] = {rd.x, rd.y};
            const float g_space = val[j], g_time = vat[j];      // the two planes' gv at this position
            if (flag & 1) {
                // the cell changed (or touches the border): a slot whose row differs flushes its pending row and restarts
                const int4 id4 = w_ids[sl0 + j];
                const int ids[4] = {id4.x, id4.y, id4.z, id4.w};
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    if (ids[k] == pid[k]) {
                        pacc[k] = __builtin_fmaf(g_space, ws[k], pacc[k]);
                    } else if (ids[k] >= 0) {
                        if (pid[k] >= 0) atomicAdd(&gp[pid[k]], pacc[k]);
                        pid[k] = ids[k];
                        pacc[k] = g_space * ws[k];
                    }
                }
            } else {
#pragma unroll
                for (int k = 0; k < 4; k++) pacc[k] = __builtin_fmaf(g_space, ws[k], pacc[k]);
            }
            if (flag & 2) {
                const int2 r2 = w_rid[sl0 + j];
                const int lid[2] = {r2.x, r2.y};
#pragma unroll
                for (int k = 0; k < 2; k++) {
                    if (lid[k] == lpid[k]) {
                        lacc[k] = __builtin_fmaf(g_time, lw[k], lacc[k]);
                    } else if (lid[k] >= 0) {
                        if (lpid[k] >= 0) atomicAdd(&my_line[lpid[k]], lacc[k]);
                        lpid[k] = lid[k];
                        lacc[k] = g_time * lw[k];
                    }
                }
            } else {
#pragma unroll
                for (int k = 0; k < 2; k++) lacc[k] = __builtin_fmaf(g_time, lw[k], lacc[k]);
            }
        }
    }
#pragma unroll
    for (int k = 0; k < 4; k++)
        if (pid[k] >= 0) atomicAdd(&gp[pid[k]], pacc[k]);
#pragma unroll
    for (int k = 0; k < 2; k++)
        if (lpid[k] >= 0) atomicAdd(&my_line[lpid[k]], lacc[k]);
    __syncthreads();
    // the carried plane's line -> its two global time rows t0 / t1 (the same for every point)
    int t0, t1;
    float wt0, wt1;
    time_sample(a.time, a.res[lvl][3], t0, t1, wt0, wt1);
    float* __restrict__ gt = a.grads[lvl][pt];
    for (int i = threadIdx.x; i < Ws * kC; i += 256) {
        const float sv = s_line[i];
        if (sv != 0.f) {
            if (t0 >= 0) atomicAdd(&gt[(size_t)t0 * Ws * kC + i], sv * wt0);
            if (t1 >= 0) atomicAdd(&gt[(size_t)t1 * Ws * kC + i], sv * wt1);
        }
    }
}

// the chunked kernels address texels with 32-bit byte offsets inside one plane
bool planes_fit32(const MomHexPlane* hp)
{
    for (int l = 0; l < hp->levels; l++)
        for (int p = 0; p < 6; p++) {
            static const int ca[6] = {0, 0, 0, 1, 1, 2}, cb[6] = {1, 2, 3, 2, 3, 3};
            if ((unsigned long long)hp->res[l][ca[p]] * (unsigned long long)hp->res[l][cb[p]] * kRowB >= (1ull << 31)) return false;
        }
    return true;
}

}  // namespace

// The launches behind mom_hexplane_forward / mom_hexplane_backward (hexplane.hip) for channels == 16; the caller has checked the
// descriptor and the pointers and opened the profile scope.
int mom_launch_hexplane16_forward(const MomHexPlane* hp, int P, const float* xyz, const float* times, float time, const uint32_t* order,
                                  float* feat, hipStream_t s)
{
    HexArgs a;
    fill_args(hp, P, times, time, order, false, &a);
    if (!times && planes_fit32(hp)) {
        const int nchunks = (P + kChunk - 1) / kChunk;
        int blocks = (nchunks + 3) / 4;
        if (blocks > 8192) blocks = 8192;              // one chunk per wave up to there, as the 32-channel forward
        hipLaunchKernelGGL(hexplane16_fwd4_kernel, dim3(blocks, hp->levels), dim3(256), 0, s, a, nchunks, xyz, feat);
        return hipGetLastError() == hipSuccess ? MOM_OK : MOM_ELAUNCH;
    }
    const long long units = (long long)P * hp->levels;
    hipLaunchKernelGGL(hexplane16_fwd_kernel, dim3((unsigned)((units + 15) / 16)), dim3(256), 0, s, a, xyz, feat);
    return hipGetLastError() == hipSuccess ? MOM_OK : MOM_ELAUNCH;
}

int mom_launch_hexplane16_backward(const MomHexPlane* hp, int P, const float* xyz, const float* times, float time, const uint32_t* order,
                                   const float* dfeat, float* dxyz, const uint32_t* plane_order, const uint32_t* plane_inverse,
                                   void* scratch, hipStream_t s)
{
    HexArgs a;
    fill_args(hp, P, times, time, order, true, &a);
    int wmax = 0;
    for (int l = 0; l < hp->levels; l++)
        for (int k = 0; k < 3; k++)
            if (hp->res[l][k] > wmax) wmax = hp->res[l][k];
    const size_t lds_s = sizeof(float) * ((size_t)4 * kSlotsS * kRecS + (size_t)wmax * kC);
    // gv rows are addressed with 32-bit byte offsets inside one (slot, level) buffer: two rows per position
    const bool fits32 = (unsigned long long)P * (2ull * kRowB) < (1ull << 32);
    if (!times && plane_order && plane_inverse && scratch && lds_s <= 160 * 1024 && fits32 && planes_fit32(hp)) {
        if (!mom_lds_limit<hexplane16_scatter_kernel>(160 * 1024)) return MOM_ELAUNCH;
        float* gvbuf = (float*)mom_align_ptr(scratch);
        constexpr int kGatherMaxBlocks = 1536, kScatterBlocks = 512;       // the 32-channel forms' caps
        const int nchunks = (P + kChunk - 1) / kChunk;
        int blocks = (nchunks + 3) / 4;
        if (blocks > kGatherMaxBlocks) blocks = kGatherMaxBlocks;
        hipLaunchKernelGGL(hexplane16_gather_kernel, dim3(blocks, hp->levels), dim3(256), 0, s, a, nchunks, xyz, dfeat, dxyz, plane_inverse,
                           gvbuf);
        if (hipGetLastError() != hipSuccess) return MOM_ELAUNCH;
        // every group walks one contiguous range of sorted positions (a multiple of the chunk size); 16 groups per workgroup
        const int groups = kScatterBlocks * 16;
        int per_group = (P + groups - 1) / groups;
        per_group = ((per_group + kChunkS - 1) / kChunkS) * kChunkS;
        const int sblocks = (int)(((long long)P + (long long)per_group * 16 - 1) / ((long long)per_group * 16));
        hipLaunchKernelGGL(hexplane16_scatter_kernel, dim3(sblocks, 3, hp->levels), dim3(256), lds_s, s, a, per_group, xyz, plane_order, gvbuf);
        return hipGetLastError() == hipSuccess ? MOM_OK : MOM_ELAUNCH;
    }
    // generic path (per-point timestamps, or no orders / scratch given): one group per (point, level), 24 atomic rows each
    const long long units = (long long)P * hp->levels;
    hipLaunchKernelGGL(hexplane16_bwd_kernel, dim3((unsigned)((units + 15) / 16)), dim3(256), 0, s, a, xyz, dfeat, dxyz);
    return hipGetLastError() == hipSuccess ? MOM_OK : MOM_ELAUNCH;
}
