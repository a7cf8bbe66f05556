// What the atomic warp (eulerian_warp.hip) and its ordered form (eulerian_ordered.hip) share: the chain walk of euler_integration,
// ReflectionPad2d's index, the four targets of a splat and the geometry of blend_feature.  Every function is host and device code:
// the ordered form's host twins walk the same chains and form the same weights, operation by operation, without contraction.
#pragma once
#include "mom_common.h"

namespace {

constexpr float kMaxCoord = 1073741824.0f;   // 2^30: the splat converts only coordinates below this in magnitude

__host__ __device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// index of ReflectionPad2d: i in [-pad, n + pad) with pad < n -> [0, n)
__host__ __device__ __forceinline__ int reflect(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * (n - 1) - i : i); }

// One pixel's chain (cinemagraph_utils.py:42-57).  fetch(ix, iy, &mx, &my) reads the motion at an in-range integer position.
// Returns the displacement after `steps` steps; `all` (or null) receives every step's, `stride` floats apart, x then y at +plane.
template <typename Fetch>
__host__ __device__ __forceinline__ float2 walk_chain(int px, int py, int W, int H, int steps, Fetch fetch, float* all, size_t stride,
                                                      size_t plane)
{
#pragma clang fp contract(off)
    const float cx = (float)px, cy = (float)py, xmax = (float)(W - 1), ymax = (float)(H - 1);
    float x = cx, y = cy;
    bool invalid = false;
    float2 d = {0.0f, 0.0f};
    for (int s = 1; s <= steps; s++) {
        if (!invalid) {
            // x, y lie in [0, W-1] x [0, H-1] here; the clamp costs two instructions and makes that independent of the reasoning
            const int ix = clampi((int)rintf(x), 0, W - 1), iy = clampi((int)rintf(y), 0, H - 1);
            float mx, my;
            fetch(ix, iy, mx, my);
            x = x + mx;
            y = y + my;
            // the reference: x > W-1 || x < 0 (false for a NaN); here a NaN is out of bounds too
            invalid = !(x <= xmax && x >= 0.0f && y <= ymax && y >= 0.0f);
            d = invalid ? float2{0.0f, 0.0f} : float2{x - cx, y - cy};
        }
        if (all) {
            all[(size_t)s * stride] = d.x;
            all[(size_t)s * stride + plane] = d.y;
        }
    }
    return d;
}

// The four targets of one source position (softmax_splatting.py:20-35): texel offsets (y * W + x, or -1 when dropped) and weights.
struct Corners { int at[4]; float w[4]; };

__host__ __device__ __forceinline__ Corners corners(float ox, float oy, int W, int H)
{
#pragma clang fp contract(off)
    Corners c;
    if (!(fabsf(ox) < kMaxCoord && fabsf(oy) < kMaxCoord)) {     // huge or NaN: dropped, never converted
        for (int k = 0; k < 4; k++) { c.at[k] = -1; c.w[k] = 0.0f; }
        return c;
    }
    const int nwx = (int)floorf(ox), nwy = (int)floorf(oy);
    const int sex = nwx + 1, sey = nwy + 1;
    c.w[0] = ((float)sex - ox) * ((float)sey - oy);             // northwest
    c.w[1] = (ox - (float)nwx) * ((float)sey - oy);             // northeast
    c.w[2] = ((float)sex - ox) * (oy - (float)nwy);             // southwest
    c.w[3] = (ox - (float)nwx) * (oy - (float)nwy);             // southeast
    const int tx = nwx, ty = nwy;
    const bool x0 = tx >= 0 && tx < W, x1 = tx + 1 >= 0 && tx + 1 < W, y0 = ty >= 0 && ty < H, y1 = ty + 1 >= 0 && ty + 1 < H;
    c.at[0] = x0 && y0 ? ty * W + tx : -1;
    c.at[1] = x1 && y0 ? ty * W + tx + 1 : -1;
    c.at[2] = x0 && y1 ? (ty + 1) * W + tx : -1;
    c.at[3] = x1 && y1 ? (ty + 1) * W + tx + 1 : -1;
    return c;
}

// The same position as the ordered form sees it: its cell (floor oy, floor ox).  False: the atomic form drops the position whole
// (NaN, or a magnitude not below 2^30) or none of its four corners lies on the W x H canvas -- it has no terms.
__host__ __device__ __forceinline__ bool splat_cell(float ox, float oy, int W, int H, int* x0, int* y0)
{
    if (!(fabsf(ox) < kMaxCoord && fabsf(oy) < kMaxCoord)) return false;
    *x0 = (int)floorf(ox);
    *y0 = (int)floorf(oy);
    return *x0 >= -1 && *x0 <= W - 1 && *y0 >= -1 && *y0 <= H - 1;
}

// corners()' weight of corner k (0 nw, 1 ne, 2 sw, 3 se) of a position splat_cell takes, the same two subtractions and one product
__host__ __device__ __forceinline__ float splat_weight(float ox, float oy, int k)
{
#pragma clang fp contract(off)
    const int nwx = (int)floorf(ox), nwy = (int)floorf(oy);
    const float wx = (k & 1) ? ox - (float)nwx : (float)(nwx + 1) - ox;
    const float wy = (k & 2) ? oy - (float)nwy : (float)(nwy + 1) - oy;
    return wx * wy;
}

// Geometry of blend_feature for a square feature of size S: the cut, the padding of the cut size s, the padded size P, where
// crop_padded_tensor starts.
struct Geometry { int cut, s, pad, P, crop0; };

inline bool geometry(int S, Geometry* g)
{
    if (S < 1) return false;
    g->cut = S == 1024 ? 3 : S == 512 ? 2 : S == 256 ? 1 : 0;
    g->s = S - 2 * g->cut;
    g->pad = g->s / 4 + g->s / 8;
    if (g->s < 1 || g->pad >= g->s) return false;
    g->P = g->s + 2 * g->pad;
    g->crop0 = (g->P - S) / 2;
    if ((size_t)g->P * g->P >= ((size_t)1 << 31)) return false;
    return g->crop0 >= 0 && g->crop0 + S <= g->P;
}

// The blend's entry of source pixel (py, px) of the padded domain, half h (0 future, 1 past): its target on the canvas, as
// eulerian_blend_kernel forms it (joint_splatting.py:30-33: the past half's sources lie P columns to the right with P taken off
// their x flow; the two fp32 roundings are reproduced).  motion [2,S,S]; the chain walks the cut, reflection-padded field.
__host__ __device__ __forceinline__ float2 blend_target(int px, int py, int half, int S, const Geometry& g, int idx, int n_frames,
                                                        const float* __restrict__ motion)
{
#pragma clang fp contract(off)
    const int P = g.P;
    const size_t plane = (size_t)S * S;
    const float sign = half ? -1.0f : 1.0f;                   // the past half integrates pad(-flow) = -pad(flow)
    auto fetch = [&](int ix, int iy, float& mx, float& my) {
        const size_t at = (size_t)(reflect(iy - g.pad, g.s) + g.cut) * S + (reflect(ix - g.pad, g.s) + g.cut);
        mx = sign * motion[at];
        my = sign * motion[plane + at];
    };
    const float2 d = walk_chain(px, py, P, P, half ? n_frames - idx - 1 : idx, fetch, (float*)nullptr, 0, 0);
    const float ox = half ? (float)(px + P) + (d.x - (float)P) : (float)px + d.x;
    const float oy = (float)py + d.y;
    return float2{ox, oy};
}

// cinemagraph_utils.py:135,163,166: alpha is a Python float; the products with the fp32 ones round it to fp32
inline void blend_z(int idx, int n_frames, float* z_future, float* z_past)
{
    const double alpha = (double)idx / (double)(n_frames - 1);
    *z_future = (float)(1.0 - alpha);
    *z_past = (float)alpha;
}

}  // namespace
