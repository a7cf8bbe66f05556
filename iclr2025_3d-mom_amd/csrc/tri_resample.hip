// Scattered values -> every pixel centre, and the multi-view point-cloud renders' per-pixel remainder, gfx950.
//
// The reference calls scipy.interpolate.griddata(view's projected points, values, pixel grid, method="linear") three times per view
// in render_PCD (train_motion.py:304,307,319) and once more per view for our_flow (:198); each call triangulates the same scattered
// points again and then locates every pixel in the triangulation.  Here the host triangulates a view once (Qhull's choice stays
// Qhull's: view 0 sits on the integer lattice, where the Delaunay triangulation is not unique) and the device does the rest, for all
// V views at once -- the reverse direction of flow_sample.hip:
//
//   mom_tri_resample   init   owner[pixel] = INT_MAX
//                      cover  one lane per triangle: atomicMin of the triangle's index into the owner word of every pixel centre
//                             that passes LinearNDInterpolator's barycentric test.  A lane walks its own bounding box while that
//                             has at most kLaneBox pixels; a larger one (the triangles that bridge an occlusion gap: a few per
//                             thousand, up to thousands of pixels) is taken by the whole wave, 64 pixels per step
//                      resolve one lane per pixel: the owner's coordinates again, by the same expressions, and all C channels
//   mom_pcd_compose    clear, hit (plain stores of 1 at the rounded points), then three passes over 32 x 8 pixel tiles; each is a
//                      separable window maximum / minimum of a byte map in LDS followed by per-pixel arithmetic (:305-330,355,357)
//
// The owner word makes the result independent of the order the atomics land in: the same bits on every run.  All arithmetic is
// float64 without contraction, in the order include/mom4d.h writes out.  Nothing an input holds reaches an address: point indices are
// checked against the view's count, vertices for finiteness, boxes are clamped to the image as float64 before they become ints, the
// offsets are searched by a loop of at most 16 steps and every range read from them is checked against [0, N] / [0, T].
#include "mom_common.h"
#include <limits.h>

namespace {

constexpr int kThreads = 256;
constexpr int kLaneBox = MOM_TRI_LANE_BOX;      // a lane walks a bounding box of at most this many pixels itself
constexpr int kNoOwner = INT_MAX;
constexpr double kEps = 100.0 * 2.220446049250313e-16;         // LinearNDInterpolator's eps = 100 * DBL_EPSILON
constexpr double kGrow = 1.0 / 1048576.0;                      // MOM_TRI_BOX_GROW: the box is grown by 2^-20 before it is rounded inwards

// largest j in [0, V-1] with off[j] <= i: the view of element i when off is non-decreasing.  At most ceil(log2 V) steps whatever off holds.
__device__ __forceinline__ int view_of(const int* __restrict__ off, int V, int i)
{
    int lo = 0, hi = V - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (off[mid] <= i) lo = mid; else hi = mid - 1;
    }
    return lo;
}

struct Tri {
    double x2, y2, a, b, c, d, det;
    int i0, i1, i2;              // rows of pts / values, global
    int bx, by, bw, bh;          // the clamped bounding box: origin and size in pixels
    bool ok;
};

// Triangle t of view j, or ok = false: t outside the view's range, an index outside [0, n_j), a non-finite vertex, det == 0, or a box
// that misses the image.
__device__ __forceinline__ Tri load_tri(int t, int j, int N, int T, int H, int W, const double2* __restrict__ pts,
                                        const int* __restrict__ pt_off, const int* __restrict__ tris, const int* __restrict__ tri_off)
{
#pragma clang fp contract(off)
    Tri r;
    r.ok = false;
    if (t < 0 || t >= T || t < tri_off[j] || t >= tri_off[j + 1]) return r;
    const int pb = pt_off[j], pe = pt_off[j + 1];
    if (pb < 0 || pe < pb || pe > N) return r;
    const int n = pe - pb;
    const int l0 = tris[3 * (size_t)t], l1 = tris[3 * (size_t)t + 1], l2 = tris[3 * (size_t)t + 2];
    if (l0 < 0 || l0 >= n || l1 < 0 || l1 >= n || l2 < 0 || l2 >= n) return r;
    r.i0 = pb + l0; r.i1 = pb + l1; r.i2 = pb + l2;
    const double2 p0 = pts[r.i0], p1 = pts[r.i1], p2 = pts[r.i2];
    if (!(isfinite(p0.x) && isfinite(p0.y) && isfinite(p1.x) && isfinite(p1.y) && isfinite(p2.x) && isfinite(p2.y))) return r;
    r.x2 = p2.x; r.y2 = p2.y;
    r.a = p0.x - p2.x; r.b = p1.x - p2.x; r.c = p0.y - p2.y; r.d = p1.y - p2.y;
    r.det = r.a * r.d - r.b * r.c;
    if (!(r.det != 0.0) || !isfinite(r.det)) return r;
    // the box in float64, clamped to the image BEFORE it becomes an int
    const double xa = fmax(ceil(fmin(fmin(p0.x, p1.x), p2.x) - kGrow), 0.0), xb = fmin(floor(fmax(fmax(p0.x, p1.x), p2.x) + kGrow), (double)(W - 1));
    const double ya = fmax(ceil(fmin(fmin(p0.y, p1.y), p2.y) - kGrow), 0.0), yb = fmin(floor(fmax(fmax(p0.y, p1.y), p2.y) + kGrow), (double)(H - 1));
    if (!(xa <= xb && ya <= yb)) return r;
    r.bx = (int)xa; r.by = (int)ya; r.bw = (int)xb - r.bx + 1; r.bh = (int)yb - r.by + 1;
    r.ok = true;
    return r;
}

__device__ __forceinline__ void bary(const Tri& r, int X, int Y, double& c0, double& c1, double& c2)
{
#pragma clang fp contract(off)
    const double dx = (double)X - r.x2, dy = (double)Y - r.y2;
    c0 = (r.d * dx - r.b * dy) / r.det;
    c1 = (r.a * dy - r.c * dx) / r.det;
    c2 = (1.0 - c0) - c1;
}

__device__ __forceinline__ bool passes(double c0, double c1, double c2)
{
    return c0 >= -kEps && c0 <= 1.0 + kEps && c1 >= -kEps && c1 <= 1.0 + kEps && c2 >= -kEps && c2 <= 1.0 + kEps;
}

__device__ __forceinline__ void claim(const Tri& r, int t, int X, int Y, int* __restrict__ owner_view, int W)
{
    double c0, c1, c2;
    bary(r, X, Y, c0, c1, c2);
    if (passes(c0, c1, c2)) atomicMin(owner_view + (size_t)Y * W + X, t);
}

__global__ void __launch_bounds__(kThreads) tri_init_kernel(size_t n, int* __restrict__ owner)
{
    const size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (i < n) owner[i] = kNoOwner;
}

__global__ void __launch_bounds__(kThreads)
tri_cover_kernel(int V, int H, int W, int N, int T, const double2* __restrict__ pts, const int* __restrict__ pt_off,
                 const int* __restrict__ tris, const int* __restrict__ tri_off, int* __restrict__ owner)
{
    // no early return: every lane of a wave reaches the ballot
    const size_t g = (size_t)blockIdx.x * kThreads + threadIdx.x;
    const int t = g < (size_t)T ? (int)g : -1;
    const int j = t >= 0 ? view_of(tri_off, V, t) : 0;
    Tri r;
    r.ok = false;
    if (t >= 0) r = load_tri(t, j, N, T, H, W, pts, pt_off, tris, tri_off);
    const bool big = r.ok && (long long)r.bw * r.bh > kLaneBox;
    if (r.ok && !big) {
        int* __restrict__ ov = owner + (size_t)j * H * W;
        for (int y = 0; y < r.bh; ++y)
            for (int x = 0; x < r.bw; ++x) claim(r, t, r.bx + x, r.by + y, ov, W);
    }
    unsigned long long todo = __ballot(big);
    const int lane = mom_lane();
    while (todo) {
        const int src = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        const int tt = __shfl(t, src), jj = __shfl(j, src);
        // every lane forms the triangle again from the same words: the same bits as its owner's lane holds
        const Tri q = load_tri(tt, jj, N, T, H, W, pts, pt_off, tris, tri_off);
        if (!q.ok) continue;                                       // (cannot happen: lane src found it ok; uniform across the wave)
        int* __restrict__ ov = owner + (size_t)jj * H * W;
        const int npix = q.bw * q.bh;                              // <= H * W < 2^31
        for (int i = lane; i < npix; i += MOM_WAVE) claim(q, tt, q.bx + i % q.bw, q.by + i / q.bw, ov, W);
    }
}

template <int C>
__global__ void __launch_bounds__(kThreads)
tri_resolve_kernel(int V, int H, int W, int N, int T, const double2* __restrict__ pts, const int* __restrict__ pt_off,
                   const int* __restrict__ tris, const int* __restrict__ tri_off, const float* __restrict__ values, double fill,
                   const int* __restrict__ owner, double* __restrict__ out)
{
#pragma clang fp contract(off)
    const size_t hw = (size_t)H * W;
    const size_t p = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (p >= hw * V) return;
    const int j = (int)(p / hw);
    const int Y = (int)((p - (size_t)j * hw) / W), X = (int)(p - (size_t)j * hw - (size_t)Y * W);
    const int t = owner[p];
    double* __restrict__ o = out + p * C;
    Tri r;
    r.ok = false;
    if (t != kNoOwner) r = load_tri(t, j, N, T, H, W, pts, pt_off, tris, tri_off);
    if (!r.ok) {
#pragma unroll
        for (int k = 0; k < C; ++k) o[k] = fill;
        return;
    }
    double c0, c1, c2;
    bary(r, X, Y, c0, c1, c2);
    const float* __restrict__ v0 = values + (size_t)r.i0 * C;
    const float* __restrict__ v1 = values + (size_t)r.i1 * C;
    const float* __restrict__ v2 = values + (size_t)r.i2 * C;
#pragma unroll
    for (int k = 0; k < C; ++k) o[k] = ((c0 * (double)v0[k]) + (c1 * (double)v1[k])) + (c2 * (double)v2[k]);
}

// ---- the per-pixel remainder of render_PCD ------------------------------------------------------------------------------------
constexpr int kTileW = 32, kTileH = 8;         // 256 threads: one pixel each
constexpr int kMaxR = 5;

// The (2R+1) x (2R+1) maximum (kMax) or minimum of a byte map at this thread's pixel, the window clipped to the image (what scipy's
// default `reflect` border amounts to for a maximum or a minimum).  Separable, in LDS: the tile with its halo, then its row-wise
// reduction, then the column.  Every thread of the block calls it (two barriers); the value is meaningless outside the image.
template <int R, bool kMax>
__device__ __forceinline__ int window(const uint8_t* __restrict__ map, int H, int W, uint8_t* tile, uint8_t* rows)
{
    constexpr int TW = kTileW + 2 * R, TH = kTileH + 2 * R;
    constexpr int neutral = kMax ? 0 : 255;
    const int tid = threadIdx.y * kTileW + threadIdx.x;
    const int gx0 = (int)blockIdx.x * kTileW - R, gy0 = (int)blockIdx.y * kTileH - R;
    __syncthreads();                                               // the previous use of tile / rows is over
    for (int i = tid; i < TW * TH; i += kThreads) {
        const int ty = i / TW, tx = i - ty * TW, gy = gy0 + ty, gx = gx0 + tx;
        tile[i] = (gy >= 0 && gy < H && gx >= 0 && gx < W) ? map[(size_t)gy * W + gx] : (uint8_t)neutral;
    }
    __syncthreads();
    for (int i = tid; i < kTileW * TH; i += kThreads) {
        const int ty = i / kTileW, x = i - ty * kTileW;
        int v = neutral;
#pragma unroll
        for (int k = 0; k <= 2 * R; ++k) { const int w = tile[ty * TW + x + k]; v = kMax ? max(v, w) : min(v, w); }
        rows[i] = (uint8_t)v;
    }
    __syncthreads();
    int v = neutral;
#pragma unroll
    for (int k = 0; k <= 2 * R; ++k) { const int w = rows[(threadIdx.y + k) * kTileW + threadIdx.x]; v = kMax ? max(v, w) : min(v, w); }
    return v;
}

#define PCD_LDS                                                                     \
    __shared__ uint8_t tile[(kTileW + 2 * kMaxR) * (kTileH + 2 * kMaxR)];           \
    __shared__ uint8_t rows[kTileW * (kTileH + 2 * kMaxR)]

// step 1 (:305,320): the resampled pixel with its 2-pixel border replaced -- I[clamp(y,1,H-2)][clamp(x,1,W-2)], 4 doubles
__device__ __forceinline__ const double* bordered(const double* __restrict__ res_view, int H, int W, int x, int y)
{
    const int cy = min(max(y, 1), H - 2), cx = min(max(x, 1), W - 2);
    return res_view + ((size_t)cy * W + cx) * 4;
}

// step 4 (:313): maskj * image + (1 - maskj) * (-1), as written
__device__ __forceinline__ double holes(double dil, double v)
{
#pragma clang fp contract(off)
    return dil * v + (1.0 - dil) * (-1.0);
}

// step 10 (:355,357): np.round(x * 255.).astype(np.uint8) for x in [0, 1]; anything else (NaN included) is clamped, not wrapped
__device__ __forceinline__ uint8_t to_byte(double x)
{
#pragma clang fp contract(off)
    return (uint8_t)(int)fmin(fmax(rint(x * 255.0), 0.0), 255.0);
}

__global__ void __launch_bounds__(kThreads) pcd_clear_kernel(size_t n, uint8_t* __restrict__ hit)
{
    const size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (i < n) hit[i] = 0;
}

// step 2 (:298,310-311): hit[rint(v)][rint(u)] = 1, half-to-even in float64
__global__ void __launch_bounds__(kThreads)
pcd_hit_kernel(int V, int H, int W, int N, const double2* __restrict__ pts, const int* __restrict__ pt_off, uint8_t* __restrict__ hit)
{
    const size_t g = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (g >= (size_t)N) return;
    const int n = (int)g, j = view_of(pt_off, V, n);
    if (n < pt_off[j] || n >= pt_off[j + 1]) return;
    const double2 p = pts[n];
    const double ru = rint(p.x), rv = rint(p.y);
    if (!(ru >= 0.0 && ru <= (double)(W - 1) && rv >= 0.0 && rv <= (double)(H - 1))) return;      // a NaN fails every comparison
    hit[((size_t)j * H + (int)rv) * W + (int)ru] = 1;
}

// steps 3-5 (:312-315): dil = 9 x 9 maximum of hit; okA = ((r' + g') + b' != -3)
__global__ void __launch_bounds__(kThreads)
pcd_dilate_kernel(int H, int W, const double* __restrict__ res, const uint8_t* __restrict__ hit, uint8_t* __restrict__ dil,
                  uint8_t* __restrict__ okA)
{
#pragma clang fp contract(off)
    PCD_LDS;
    const size_t view = (size_t)blockIdx.z * H * W;
    const int x = (int)blockIdx.x * kTileW + threadIdx.x, y = (int)blockIdx.y * kTileH + threadIdx.y;
    const int dl = window<4, true>(hit + view, H, W, tile, rows);
    if (x >= W || y >= H) return;
    const double* __restrict__ I = bordered(res + view * 4, H, W, x, y);
    const double d = (double)dl;
    const double r = holes(d, I[0]), g = holes(d, I[1]), b = holes(d, I[2]);
    dil[view + (size_t)y * W + x] = (uint8_t)dl;
    okA[view + (size_t)y * W + x] = ((r + g) + b != -3.0) ? 1 : 0;
}

// steps 5-8 (:315-316,325,327): mj = 11 x 11 minimum of okA; the image's bytes; m' and okB = ((m' + m') + m' != -3)
__global__ void __launch_bounds__(kThreads)
pcd_image_kernel(int H, int W, const double* __restrict__ res, const uint8_t* __restrict__ dil, const uint8_t* __restrict__ okA,
                 uint8_t* __restrict__ mj_map, uint8_t* __restrict__ okB, uint8_t* __restrict__ image)
{
#pragma clang fp contract(off)
    PCD_LDS;
    const size_t view = (size_t)blockIdx.z * H * W;
    const int x = (int)blockIdx.x * kTileW + threadIdx.x, y = (int)blockIdx.y * kTileH + threadIdx.y;
    const int mji = window<5, false>(okA + view, H, W, tile, rows);
    if (x >= W || y >= H) return;
    const size_t p = view + (size_t)y * W + x;
    const double* __restrict__ I = bordered(res + view * 4, H, W, x, y);
    const double d = (double)dil[p], mj = (double)mji;
#pragma unroll
    for (int k = 0; k < 3; ++k) image[p * 3 + k] = to_byte(mj * holes(d, I[k]) + (1.0 - mj) * 0.0);
    const double m = d * I[3] + (1.0 - mj) * (-1.0);
    mj_map[p] = (uint8_t)mji;
    okB[p] = ((m + m) + m != -3.0) ? 1 : 0;
}

// steps 8-10 (:327-330,357): mj2 = 11 x 11 minimum of okB; mask = mj2 * m'
__global__ void __launch_bounds__(kThreads)
pcd_mask_kernel(int H, int W, const double* __restrict__ res, const uint8_t* __restrict__ dil, const uint8_t* __restrict__ mj_map,
                const uint8_t* __restrict__ okB, uint8_t* __restrict__ mask)
{
#pragma clang fp contract(off)
    PCD_LDS;
    const size_t view = (size_t)blockIdx.z * H * W;
    const int x = (int)blockIdx.x * kTileW + threadIdx.x, y = (int)blockIdx.y * kTileH + threadIdx.y;
    const int mj2i = window<5, false>(okB + view, H, W, tile, rows);
    if (x >= W || y >= H) return;
    const size_t p = view + (size_t)y * W + x;
    const double* __restrict__ I = bordered(res + view * 4, H, W, x, y);
    const double d = (double)dil[p], mj = (double)mj_map[p], mj2 = (double)mj2i;
    const double m = d * I[3] + (1.0 - mj) * (-1.0);
    mask[p] = to_byte(mj2 * m + (1.0 - mj2) * 0.0);
}

bool pixels_fit(int V, int H, int W, size_t* n)
{
    if (V <= 0 || V > 65535 || H < 1 || W < 1) return false;
    *n = (size_t)V * H * W;
    return *n <= (size_t)INT_MAX;
}

unsigned blocks_of(size_t n) { return (unsigned)((n + kThreads - 1) / kThreads); }

}  // namespace

extern "C" size_t mom_tri_resample_scratch_bytes(int V, int H, int W)
{
    size_t n;
    return pixels_fit(V, H, W, &n) ? n * sizeof(int) : 0;
}

extern "C" int mom_tri_resample(int V, int H, int W, int C, int N, int T, const double* pts, const int* pt_off, const int* tris,
                                const int* tri_off, const float* values, double fill, double* out, void* scratch, size_t scratch_bytes,
                                mom_stream_t stream)
{
    size_t n;
    if (!pixels_fit(V, H, W, &n) || C < 1 || C > 8 || N < 0 || T < 0) return MOM_EINVAL;
    if (!pt_off || !tri_off || !out || !scratch || (N > 0 && (!pts || !values)) || (T > 0 && !tris)) return MOM_EINVAL;
    if (scratch_bytes < n * sizeof(int) || ((uintptr_t)pts & 15) || ((uintptr_t)scratch & 3)) return MOM_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    int* owner = (int*)scratch;
    hipLaunchKernelGGL(tri_init_kernel, dim3(blocks_of(n)), dim3(kThreads), 0, s, n, owner);
    if (T > 0 && N > 0)
        hipLaunchKernelGGL(tri_cover_kernel, dim3(blocks_of((size_t)T)), dim3(kThreads), 0, s, V, H, W, N, T, (const double2*)pts, pt_off,
                           tris, tri_off, owner);
#define MOM_TRI_RESOLVE(c)                                                                                                          \
    case c:                                                                                                                         \
        hipLaunchKernelGGL(tri_resolve_kernel<c>, dim3(blocks_of(n)), dim3(kThreads), 0, s, V, H, W, N, T, (const double2*)pts, pt_off, \
                           tris, tri_off, values, fill, (const int*)owner, out);                                                    \
        break;
    switch (C) {
        MOM_TRI_RESOLVE(1) MOM_TRI_RESOLVE(2) MOM_TRI_RESOLVE(3) MOM_TRI_RESOLVE(4)
        MOM_TRI_RESOLVE(5) MOM_TRI_RESOLVE(6) MOM_TRI_RESOLVE(7) MOM_TRI_RESOLVE(8)
    }
#undef MOM_TRI_RESOLVE
    return hipGetLastError() == hipSuccess ? MOM_OK : MOM_ELAUNCH;
}

extern "C" size_t mom_pcd_compose_scratch_bytes(int V, int H, int W)
{
    size_t n;
    return pixels_fit(V, H, W, &n) && H >= 5 && W >= 5 ? 5 * n : 0;
}

extern "C" int mom_pcd_compose(int V, int H, int W, int N, const double* resampled, const double* pts, const int* pt_off,
                               uint8_t* image, uint8_t* mask, void* scratch, size_t scratch_bytes, mom_stream_t stream)
{
    size_t n;
    if (!pixels_fit(V, H, W, &n) || H < 5 || W < 5 || N < 0) return MOM_EINVAL;
    if (!resampled || !pt_off || !image || !mask || !scratch || (N > 0 && !pts)) return MOM_EINVAL;
    if (scratch_bytes < 5 * n || ((uintptr_t)pts & 15) || ((uintptr_t)resampled & 7)) return MOM_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    uint8_t* hit = (uint8_t*)scratch;
    uint8_t *dil = hit + n, *okA = dil + n, *mj = okA + n, *okB = mj + n;
    hipLaunchKernelGGL(pcd_clear_kernel, dim3(blocks_of(n)), dim3(kThreads), 0, s, n, hit);
    if (N > 0)
        hipLaunchKernelGGL(pcd_hit_kernel, dim3(blocks_of((size_t)N)), dim3(kThreads), 0, s, V, H, W, N, (const double2*)pts, pt_off, hit);
    const dim3 grid((unsigned)((W + kTileW - 1) / kTileW), (unsigned)((H + kTileH - 1) / kTileH), (unsigned)V), block(kTileW, kTileH);
    hipLaunchKernelGGL(pcd_dilate_kernel, grid, block, 0, s, H, W, resampled, (const uint8_t*)hit, dil, okA);
    hipLaunchKernelGGL(pcd_image_kernel, grid, block, 0, s, H, W, resampled, (const uint8_t*)dil, (const uint8_t*)okA, mj, okB, image);
    hipLaunchKernelGGL(pcd_mask_kernel, grid, block, 0, s, H, W, resampled, (const uint8_t*)dil, (const uint8_t*)mj, (const uint8_t*)okB, mask);
    return hipGetLastError() == hipSuccess ? MOM_OK : MOM_ELAUNCH;
}
