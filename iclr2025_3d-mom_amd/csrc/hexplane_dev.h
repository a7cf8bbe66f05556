// Device helpers of the HexPlane kernels shared by hexplane.hip, deform_field.hip and deform_field16.hip: normalize_aabb and ATen's
// grid_sampler_2d coordinate arithmetic (align_corners=True, padding_mode='border'), the kernel argument block and its host-side fill.
#pragma once
#include "mom_common.h"

namespace {

__device__ __forceinline__ float unnorm_clip(float c, int size, float& gmul)
{
    // align_corners=True: ((c+1)/2)*(size-1); border: clip to [0, size-1] with zero gradient when clipped
    float v = ((c + 1.f) / 2.f) * (float)(size - 1);
    gmul = (float)(size - 1) / 2.f;
    if (v <= 0.f) {
        v = 0.f;
        gmul = 0.f;
    } else {
        const float mx = (float)(size - 1);
        if (v >= mx) {
            v = mx;
            gmul = 0.f;
        }
    }
    return v;
}

struct HexArgs {
    int P, levels;
    int res[4][4];
    const float* planes[4][6];
    float* grads[4][6];
    float a0[3], a1[3];  // aabb rows exactly as the reference stores them (row 0 = xyz_max, row 1 = xyz_min)
    float time;
    const float* times;  // optional per-point timestamps [P]; null -> `time` for every point
    const uint32_t* order;  // optional processing order (a permutation of 0..P-1, e.g. Morton order); null -> identity
};

// The per-frame table of time lines (deform_field.hip, hexplane_lines_kernel): for level l and axis k the rows
// lines[off[l][k] + r * 32 .. + 31] = the space-time plane (k, t) interpolated at the frame's timestamp, row r along axis k.
struct LineTab {
    unsigned off[4][3];                              // float offset of line (level, axis) inside the table
};

__constant__ int kCombA[6] = {0, 0, 0, 1, 1, 2};
__constant__ int kCombB[6] = {1, 2, 3, 2, 3, 3};

// normalize_aabb as torch evaluates it: the product and the difference rounded one after the other.  Left to the compiler the
// expression contracts into one fma; the result differs by an ulp at most, and that is visible in one place: a point that DEFINES
// the box -- set_aabb takes the cloud's extremes -- comes out at 1 - ulp in torch and at exactly 1 contracted, where the border
// clip takes its position gradient away.  Every backward kernel, the plane-order keys and the 16-channel forward normalise here.  (`scale` = 2.0f / (a1 - a0):
// torch forms reciprocal(a1 - a0) * 2, the same value, doubling being exact.)
__device__ __forceinline__ float norm_coord(float x, float lo, float scale)
{
#pragma clang fp contract(off)
    const float m = (x - lo) * scale;
    return m - 1.0f;
}

__device__ __forceinline__ void norm_coords(const HexArgs& a, const float* __restrict__ xyz, int g, float c[4])
{
#pragma unroll
    for (int k = 0; k < 3; k++) c[k] = norm_coord(xyz[3 * g + k], a.a0[k], 2.0f / (a.a1[k] - a.a0[k]));
    c[3] = a.times ? a.times[g] : a.time;
}

// The 32-channel FORWARD kernels (hexplane_fwd, hexplane_fwd4, the fused field forward's make_record) keep the expression as the
// compiler contracts it.  A feature is continuous in the coordinate -- across the border clip and across a cell boundary alike --
// so an ulp of the coordinate is an ulp of the feature, whichever rounding it has; what is NOT continuous is the position gradient
// (the clip's mask, the cell's slope), and every backward kernel takes both from norm_coord above.  Kept because the features, and
// with them every deformed position, stay bit for bit what they were: which (pixel, splat) pairs fall on the other side of a
// compositing threshold than in the CPU oracle follows those last bits.
__device__ __forceinline__ void norm_coords_fwd32(const HexArgs& a, const float* __restrict__ xyz, int g, float c[4])
{
#pragma unroll
    for (int k = 0; k < 3; k++) c[k] = (xyz[3 * g + k] - a.a0[k]) * (2.0f / (a.a1[k] - a.a0[k])) - 1.0f;
    c[3] = a.times ? a.times[g] : a.time;
}

// ---- the generic (one lane group per (point, level)) kernels' sample -------------------------------------------
struct PlaneSample {
    int i00, i01, i10, i11;      // texel indices (row-major over [H][W]), -1 when out of bounds
    float w00, w01, w10, w11;    // nw, ne, sw, se
    float gx_mul, gy_mul;        // d(ix)/d(coord) incl. border-clip mask
    float ix, iy;
    int ixn, iyn;
};

__device__ __forceinline__ PlaneSample make_sample(float cx, float cy, int Wd, int Hd)
{
    PlaneSample s;
    s.ix = unnorm_clip(cx, Wd, s.gx_mul);
    s.iy = unnorm_clip(cy, Hd, s.gy_mul);
    const float fx = floorf(s.ix), fy = floorf(s.iy);
    const int x0 = (int)fx, y0 = (int)fy, x1 = x0 + 1, y1 = y0 + 1;
    s.ixn = x0;
    s.iyn = y0;
    s.w00 = ((float)x1 - s.ix) * ((float)y1 - s.iy);
    s.w01 = (s.ix - (float)x0) * ((float)y1 - s.iy);
    s.w10 = ((float)x1 - s.ix) * (s.iy - (float)y0);
    s.w11 = (s.ix - (float)x0) * (s.iy - (float)y0);
    const bool x0in = x0 >= 0 && x0 < Wd, x1in = x1 >= 0 && x1 < Wd, y0in = y0 >= 0 && y0 < Hd, y1in = y1 >= 0 && y1 < Hd;
    s.i00 = (x0in && y0in) ? y0 * Wd + x0 : -1;
    s.i01 = (x1in && y0in) ? y0 * Wd + x1 : -1;
    s.i10 = (x0in && y1in) ? y1 * Wd + x0 : -1;
    s.i11 = (x1in && y1in) ? y1 * Wd + x1 : -1;
    return s;
}

// ---- helpers shared by the chunked kernels -------------------------------------------------------------------
__device__ __forceinline__ int time_sample(float c, int size, int& i0, int& i1, float& w0, float& w1)
{
    float gm;
    const float v = unnorm_clip(c, size, gm);
    const int x0 = (int)floorf(v), x1 = x0 + 1;
    w0 = (float)x1 - v;
    w1 = v - (float)x0;
    i0 = (x0 >= 0 && x0 < size) ? x0 : -1;
    i1 = (x1 >= 0 && x1 < size) ? x1 : -1;
    return 0;
}

__device__ __forceinline__ float ld_f32(const float* __restrict__ base, unsigned byte_off)
{
    return *reinterpret_cast<const float*>(reinterpret_cast<const char*>(base) + byte_off);     // uniform base + 32-bit lane offset
}

// order slot (0: (x,y), 1: (x,z), 2: (y,z)) whose sorted position a plane's gv row is stored at
__device__ __forceinline__ constexpr int order_slot_of_plane(int p) { return p == 0 ? 0 : (p == 1 ? 1 : (p == 2 ? 0 : (p == 3 ? 2 : (p == 4 ? 2 : 1)))); }

}  // namespace

static void fill_args(const MomHexPlane* hp, int P, const float* times, float time, const uint32_t* order, bool grads, HexArgs* a)
{
    a->P = P; a->levels = hp->levels; a->time = time; a->times = times; a->order = order;
    for (int l = 0; l < 4; l++)
        for (int k = 0; k < 4; k++) a->res[l][k] = hp->res[l][k];
    for (int l = 0; l < 4; l++)
        for (int p = 0; p < 6; p++) { a->planes[l][p] = hp->planes[l][p]; a->grads[l][p] = grads ? hp->grads[l][p] : nullptr; }
    for (int k = 0; k < 3; k++) { a->a0[k] = hp->aabb[k]; a->a1[k] = hp->aabb[3 + k]; }
}

static int line_table(const MomHexPlane* hp, LineTab* lt)
{
    unsigned off = 0;
    for (int l = 0; l < 4; l++)
        for (int k = 0; k < 3; k++) {
            lt->off[l][k] = off;
            if (l < hp->levels) off += (unsigned)hp->res[l][k] * 32u;
        }
    return (int)off;
}
