// Delaunay triangulation of every view's scattered points on the device, gfx950: pts / pt_off as mom_tri_resample reads them in,
// tris / tri_off as it reads them out, in the canonical form include/mom4d.h writes down.  No host round trip, no float atomics,
// the same integers on every run; mom_delaunay_host is the twin (csrc/delaunay_dev.h holds what both execute).
//
//   init, count, cell_scan, scatter, cell_sort   the view's points binned into the image's pixel cells, a cell's points by index
//                                                (integer atomics count and place; the sort takes their order out again)
//   star_lane       one lane per point: the star in LDS (MOM_DELAUNAY_LANE_STAR neighbours), candidates from the rings of cells
//                   around the point until the cell is closed and every vertex's circle lies inside what the rings covered.  A
//                   point that outgrows the star, sits on the hull or keeps a large circle after ring kLaneRings is deferred
//   star_deferred   one WAVE per deferred point: the star in LDS (MOM_DELAUNAY_MAX_STAR neighbours, 4 KB a wave), the rings again,
//                   then every vertex against the rows of cells its circle (the gap: its wedge) meets, until a pass inserts
//                   nothing.  A row's cells are one slice of the bucket array: the 64 lanes probe 64 candidates at a time and
//                   insertions are serial (delaunay_dev.h: offer_slice).  The finished star goes to a pool in scratch
//   view_scan, off_scan, emit   per point the count of triangles it owns (it is their smallest index), scanned per view and
//                   across views; T = 2 n - 2 - h is checked per view; one store per triangle
//
// A view's status is the largest code any of its points raised (atomicMax of an int): no order decides it.  Views are skipped by
// the snapshot cell_scan took of the status, never by a word another lane of the same launch may be writing.  Nothing an input
// holds reaches an address: ranges read from pt_off are checked against [0, N], points for range before they are binned, every
// cell slice is clamped to the view and every triangle slot to the capacity 2 N.
#include "mom_common.h"
#include "scan_dev.h"
#include "delaunay_dev.h"
#include <limits.h>
#include <vector>

namespace {

constexpr int kThreads = 256;
constexpr int kLane = MOM_DELAUNAY_LANE_STAR;
constexpr int kMax = MOM_DELAUNAY_MAX_STAR;
constexpr int kHdr = 64;                        // hdr[0] deferred points, hdr[1] the largest star, hdr[2] pool ints asked for
constexpr int kDeferredMark = 1 << 30;          // rec of a point whose star is still owed
constexpr int kWasDeferred = 1 << 29;           // rec of a point the lane path gave up
constexpr int kPoolPerSlot = 16;                // the pool of finished deferred stars: this many ints per entry of the deferred list
static_assert(kMax < 1024 && kLane < 16, "rec's fields");

// rec: triangles owned (10 bits) | (gap + 1) << 10 (11 bits) | the degree of a lane-path star << 21 (4 bits); a deferred star's
// degree is the first word of its pool entry
__host__ __device__ inline int rec_of(int count, int deg, int gap) { return count | ((gap + 1) << 10) | ((deg < 16 ? deg : 0) << 21); }
__host__ __device__ inline int rec_count(int r) { return r & 1023; }
__host__ __device__ inline int rec_deg(int r) { return (r >> 21) & 15; }
__host__ __device__ inline int rec_gap(int r) { return ((r >> 10) & 2047) - 1; }

struct Layout {
    size_t hdr, view_ok, view_T, cell_count, cell_start, cell_pts, rec, loc, toff, lane_star, deferred, def_star, ints;
    int dcap;
    size_t pool;         // ints of def_star
};

// False: a shape the entry points refuse.
bool layout(int V, int H, int W, int N, Layout* L)
{
    if (V <= 0 || V > 65535 || H < 1 || W < 1 || N < 0 || N > (1 << 30)) return false;
    const size_t hw = (size_t)H * W, cells = hw * V;
    if (cells > (size_t)INT_MAX) return false;
    const size_t n = (size_t)N;
    L->dcap = N / 8 + 4096;
    size_t o = 0;
    L->hdr = o; o += kHdr;
    L->view_ok = o; o += V;
    L->view_T = o; o += V;
    L->cell_count = o; o += cells;
    L->cell_start = o; o += cells + V;
    L->cell_pts = o; o += n;
    L->rec = o; o += n;
    L->loc = o; o += n;
    L->toff = o; o += n;
    L->lane_star = o; o += n * kLane;
    L->deferred = o; o += L->dcap;
    L->pool = (size_t)L->dcap * kPoolPerSlot;
    L->def_star = o; o += L->pool;
    L->ints = o;
    return true;
}

__host__ __device__ inline bool in_frame(dl::P2 p, int H, int W)
{
    return p.x >= 0.0 && p.x <= (double)(W - 1) && p.y >= 0.0 && p.y <= (double)(H - 1);        // a NaN fails every comparison
}

// view j's rows of pts: false (and n = 0) unless the range lies inside [0, N]
__host__ __device__ inline bool view_range(const int* pt_off, int j, int N, int& pb, int& n)
{
    const int b = pt_off[j], e = pt_off[j + 1];
    pb = 0;
    n = 0;
    if (b < 0 || e < b || e > N) return false;
    pb = b;
    n = e - b;
    return true;
}

// largest j in [0, V-1] with off[j] <= i (at most 16 steps whatever off holds)
__device__ __forceinline__ int view_of(const int* __restrict__ off, int V, int i)
{
    int lo = 0, hi = V - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (off[mid] <= i) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// point g -> its view and local index; false: g belongs to no well-formed view
__device__ __forceinline__ bool point_view(const int* __restrict__ pt_off, int V, int N, int g, int& j, int& pb, int& n)
{
    j = view_of(pt_off, V, g);
    return view_range(pt_off, j, N, pb, n) && g >= pb && g < pb + n;
}

__global__ void __launch_bounds__(kThreads)
dl_init_kernel(int V, int N, size_t cells, const int* __restrict__ pt_off, int* __restrict__ status, int* __restrict__ hdr,
               int* __restrict__ cell_count)
{
    const size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (i < cells) cell_count[i] = 0;
    if (i < (size_t)kHdr) hdr[i] = 0;
    if (i < (size_t)V) {
        int pb, n;
        status[i] = (view_range(pt_off, (int)i, N, pb, n) && n >= 3) ? MOM_DELAUNAY_OK : MOM_DELAUNAY_FEW;
    }
}

__global__ void __launch_bounds__(kThreads)
dl_count_kernel(int V, int H, int W, int N, const dl::P2* __restrict__ pts, const int* __restrict__ pt_off, int* __restrict__ status,
                int* __restrict__ cell_count)
{
    const size_t g = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (g >= (size_t)N) return;
    int j, pb, n;
    if (!point_view(pt_off, V, N, (int)g, j, pb, n)) return;
    const dl::P2 p = pts[g];
    if (!in_frame(p, H, W)) { atomicMax(status + j, MOM_DELAUNAY_RANGE); return; }
    atomicAdd(cell_count + (size_t)j * H * W + (size_t)(int)p.y * W + (int)p.x, 1);
}

// one workgroup per view: the exclusive scan of its cells' counts, and the snapshot of its status the later launches go by
__global__ void __launch_bounds__(kThreads)
dl_cell_scan_kernel(int H, int W, const int* __restrict__ status, const int* __restrict__ cell_count, int* __restrict__ cell_start,
                    int* __restrict__ view_ok)
{
    __shared__ int s_wave[4];
    const int j = blockIdx.x, hw = H * W;
    const int* __restrict__ cnt = cell_count + (size_t)j * hw;
    int* __restrict__ start = cell_start + (size_t)j * (hw + 1);
    int carry = 0;
    for (int base = 0; base < hw; base += kThreads) {
        const int c = base + (int)threadIdx.x;
        const int v = c < hw ? cnt[c] : 0;
        int total;
        const int ex = block_exclusive_scan_256(v, s_wave, total);
        if (c < hw) start[c] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) {
        start[hw] = carry;
        view_ok[j] = status[j] == MOM_DELAUNAY_OK;
    }
}

__global__ void __launch_bounds__(kThreads)
dl_scatter_kernel(int V, int H, int W, int N, const dl::P2* __restrict__ pts, const int* __restrict__ pt_off,
                  const int* __restrict__ view_ok, int* __restrict__ cell_count, const int* __restrict__ cell_start,
                  int* __restrict__ cell_pts)
{
    const size_t g = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (g >= (size_t)N) return;
    int j, pb, n;
    if (!point_view(pt_off, V, N, (int)g, j, pb, n) || !view_ok[j]) return;
    const dl::P2 p = pts[g];
    if (!in_frame(p, H, W)) return;                                // (an ok view has none)
    const size_t hw = (size_t)H * W, c = (size_t)(int)p.y * W + (int)p.x;
    const int slot = cell_start[(size_t)j * (hw + 1) + c] + atomicSub(cell_count + (size_t)j * hw + c, 1) - 1;
    if (slot >= 0 && slot < n) cell_pts[pb + slot] = (int)g - pb;
}

// one lane per cell: its points ascending by index, whatever order the scatter's atomics landed in
__global__ void __launch_bounds__(kThreads)
dl_cell_sort_kernel(int V, int H, int W, int N, const int* __restrict__ pt_off, const int* __restrict__ view_ok,
                    const int* __restrict__ cell_start, int* __restrict__ cell_pts)
{
    const size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x, hw = (size_t)H * W;
    if (i >= hw * V) return;
    const int j = (int)(i / hw);
    int pb, n;
    if (!view_ok[j] || !view_range(pt_off, j, N, pb, n)) return;
    const size_t c = i - (size_t)j * hw;
    int b = cell_start[(size_t)j * (hw + 1) + c], e = cell_start[(size_t)j * (hw + 1) + c + 1];
    if (b < 0) b = 0;
    if (e > n) e = n;
    int* __restrict__ a = cell_pts + pb;
    for (int k = b + 1; k < e; ++k) {
        const int x = a[k];
        int m = k;
        while (m > b && a[m - 1] > x) { a[m] = a[m - 1]; --m; }
        a[m] = x;
    }
}

__device__ __forceinline__ dl::View view_at(int j, int pb, int n, int H, int W, const dl::P2* __restrict__ pts,
                                            const int* __restrict__ cell_start, const int* __restrict__ cell_pts)
{
    dl::View v;
    v.pts = pts + pb;
    v.cell_start = cell_start + (size_t)j * ((size_t)H * W + 1);
    v.cell_pts = cell_pts + pb;
    v.n = n; v.H = H; v.W = W;
    return v;
}

__global__ void __launch_bounds__(kThreads)
dl_star_lane_kernel(int V, int H, int W, int N, int dcap, const dl::P2* __restrict__ pts, const int* __restrict__ pt_off,
                    const int* __restrict__ view_ok, const int* __restrict__ cell_start, const int* __restrict__ cell_pts,
                    int* __restrict__ status, int* __restrict__ hdr, int* __restrict__ rec, int* __restrict__ loc,
                    int* __restrict__ lane_star, int* __restrict__ deferred)
{
    __shared__ int s_star[kThreads * kLane];                       // element i of lane t at [i * kThreads + t]
    const size_t g = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (g >= (size_t)N) return;
    rec[g] = 0;
    loc[g] = -1;
    int j, pb, n;
    if (!point_view(pt_off, V, N, (int)g, j, pb, n) || !view_ok[j]) return;
    const dl::View v = view_at(j, pb, n, H, W, pts, cell_start, cell_pts);
    dl::Star S;
    S.s = s_star + threadIdx.x; S.stride = kThreads; S.cap = kLane; S.m = 0; S.gap = -1;
    const int p = (int)g - pb;
    int gap;
    const int rc = dl::build_star<0>(v, p, S, true, &gap);
    if (rc == dl::kDone) {
        for (int i = 0; i < S.m; ++i) lane_star[g * kLane + i] = S.get(i);
        rec[g] = rec_of(dl::upper_count(S, p, gap), S.m, gap);
        atomicMax(hdr + 1, S.m);
    } else if (rc == dl::kDefer) {
        const int slot = atomicAdd(hdr, 1);
        if (slot < dcap) deferred[slot] = (int)g;
        rec[g] = kDeferredMark | kWasDeferred;
    } else {
        atomicMax(status + j, MOM_DELAUNAY_UNCERTAIN);
    }
}

__global__ void __launch_bounds__(kThreads)
dl_star_deferred_kernel(int V, int H, int W, int N, int dcap, size_t pool, const dl::P2* __restrict__ pts, const int* __restrict__ pt_off,
                        const int* __restrict__ view_ok, const int* __restrict__ cell_start, const int* __restrict__ cell_pts,
                        int* __restrict__ status, int* __restrict__ hdr, int* __restrict__ rec, int* __restrict__ loc,
                        const int* __restrict__ deferred, int* __restrict__ def_star)
{
    __shared__ int s_star[(kThreads / MOM_WAVE) * kMax];            // one star per wave
    // everything below is uniform over the wave: its 64 lanes hold the same point and the same star
    const int wave = (int)threadIdx.x / MOM_WAVE, lane = (int)threadIdx.x % MOM_WAVE;
    const int t = (int)blockIdx.x * (kThreads / MOM_WAVE) + wave;
    const int D = hdr[0];
    if (D > dcap || t >= D || t >= dcap) return;                   // more than the list holds: every such point stays owed (status 3)
    const int g = deferred[t];
    if (g < 0 || g >= N) return;
    int j, pb, n;
    if (!point_view(pt_off, V, N, g, j, pb, n) || !view_ok[j]) return;
    const dl::View v = view_at(j, pb, n, H, W, pts, cell_start, cell_pts);
    dl::Star S;
    S.s = s_star + wave * kMax; S.stride = 1; S.cap = kMax; S.m = 0; S.gap = -1;
    const int p = g - pb;
    int gap;
    const int rc = dl::build_star<1>(v, p, S, false, &gap);
    if (rc == dl::kDone) {
        // the pool's words are asked for whether they are there or not: hdr[2] is a function of the input, and so is `too many`
        int at = 0;
        if (lane == 0) at = atomicAdd(hdr + 2, S.m + 1);
        at = __shfl(at, 0);
        if (at >= 0 && (size_t)at + (size_t)S.m + 1 <= pool) {
            for (int i = lane; i < S.m; i += MOM_WAVE) def_star[(size_t)at + 1 + i] = S.get(i);
            if (lane == 0) {
                def_star[at] = S.m;
                rec[g] = rec_of(dl::upper_count(S, p, gap), S.m, gap) | kWasDeferred;
                loc[g] = at;
                atomicMax(hdr + 1, S.m);
            }
        }
    } else if (lane == 0) {
        rec[g] = kWasDeferred;
        atomicMax(status + j, rc == dl::kOverflow ? MOM_DELAUNAY_OVERFLOW : MOM_DELAUNAY_UNCERTAIN);
    }
}

// one workgroup per view: where each point's triangles start within the view, T_j and h_j, and the count check
__global__ void __launch_bounds__(kThreads)
dl_view_scan_kernel(int N, size_t pool, const int* __restrict__ hdr, const int* __restrict__ pt_off, const int* __restrict__ view_ok,
                    const int* __restrict__ rec, int* __restrict__ toff, int* __restrict__ status, int* __restrict__ view_T)
{
    __shared__ int s_wave[4];
    __shared__ int s_hull[4];
    const int j = blockIdx.x;
    int pb, n;
    const bool live = view_range(pt_off, j, N, pb, n) && view_ok[j];          // uniform over the workgroup
    const bool short_pool = hdr[2] < 0 || (size_t)hdr[2] > pool;   // then every view with a deferred point is refused
    int carry = 0, hull = 0, owed = 0;
    for (int base = 0; live && base < n; base += kThreads) {
        const int i = base + (int)threadIdx.x;
        const int r = i < n ? rec[pb + i] : 0;
        const bool marked = (r & kDeferredMark) != 0;
        const int c = marked ? 0 : rec_count(r);
        int total;
        const int ex = block_exclusive_scan_256(c, s_wave, total);
        if (i < n) toff[pb + i] = carry + ex;
        carry += total;
        hull += (!marked && rec_gap(r) >= 0) ? 1 : 0;
        owed |= (marked || (short_pool && (r & kWasDeferred))) ? 1 : 0;
    }
    // h_j and `owed` over the workgroup (integers: the order of the sum decides nothing)
    for (int d = 32; d > 0; d >>= 1) { hull += __shfl_down(hull, d); owed |= __shfl_down(owed, d); }
    if ((threadIdx.x & 63) == 0) { s_hull[threadIdx.x >> 6] = hull; s_wave[threadIdx.x >> 6] = owed; }
    __syncthreads();
    if (threadIdx.x == 0) {
        const int h = s_hull[0] + s_hull[1] + s_hull[2] + s_hull[3];
        int st = status[j];
        if (live && (s_wave[0] | s_wave[1] | s_wave[2] | s_wave[3]) && st < MOM_DELAUNAY_OVERFLOW) st = MOM_DELAUNAY_OVERFLOW;
        if (live && st == MOM_DELAUNAY_OK && carry != 2 * n - 2 - h) st = MOM_DELAUNAY_INCONSISTENT;
        status[j] = st;
        view_T[j] = (live && st == MOM_DELAUNAY_OK) ? carry : 0;
    }
}

__global__ void __launch_bounds__(kThreads) dl_off_scan_kernel(int V, const int* __restrict__ view_T, int* __restrict__ tri_off)
{
    __shared__ int s_wave[4];
    int carry = 0;
    for (int base = 0; base < V; base += kThreads) {
        const int j = base + (int)threadIdx.x;
        const int v = j < V ? view_T[j] : 0;
        int total;
        const int ex = block_exclusive_scan_256(v, s_wave, total);
        if (j < V) tri_off[j] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) tri_off[V] = carry;
}

__global__ void __launch_bounds__(kThreads)
dl_emit_kernel(int V, int N, size_t pool, const int* __restrict__ pt_off, const int* __restrict__ status, const int* __restrict__ rec,
               const int* __restrict__ loc, const int* __restrict__ toff, const int* __restrict__ tri_off,
               int* __restrict__ lane_star, int* __restrict__ def_star, int* __restrict__ tris)
{
    const size_t g = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (g >= (size_t)N) return;
    int j, pb, n;
    if (!point_view(pt_off, V, N, (int)g, j, pb, n) || status[j] != MOM_DELAUNAY_OK) return;
    const int r = rec[g], at = loc[g];
    if ((r & kDeferredMark) || rec_count(r) == 0 || (at >= 0 && (size_t)at + 1 > pool)) return;
    dl::Star S;
    S.s = at < 0 ? lane_star + g * kLane : def_star + (size_t)at + 1;
    S.stride = 1; S.cap = at < 0 ? kLane : kMax; S.m = at < 0 ? rec_deg(r) : def_star[at]; S.gap = rec_gap(r);
    if (S.m < 0 || S.m > S.cap || (at >= 0 && (size_t)at + 1 + (size_t)S.m > pool)) return;
    dl::emit_star(S, (int)g - pb, rec_gap(r), tris, (size_t)tri_off[j] + (size_t)toff[g], 2 * (size_t)N);
}

unsigned blocks_of(size_t n) { return (unsigned)((n + kThreads - 1) / kThreads); }

}  // namespace

extern "C" size_t mom_delaunay_scratch_bytes(int V, int H, int W, int N)
{
    Layout L;
    return layout(V, H, W, N, &L) ? L.ints * sizeof(int) : 0;
}

extern "C" int mom_delaunay(int V, int H, int W, int N, const double* pts, const int* pt_off, int* tris, int* tri_off, int* status,
                            void* scratch, size_t scratch_bytes, mom_stream_t stream)
{
    Layout L;
    if (!layout(V, H, W, N, &L)) return MOM_EINVAL;
    if (!pt_off || !tri_off || !status || !scratch || (N > 0 && (!pts || !tris))) return MOM_EINVAL;
    if (scratch_bytes < L.ints * sizeof(int) || ((uintptr_t)pts & 15) || ((uintptr_t)scratch & 3)) return MOM_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    int* w = (int*)scratch;
    const dl::P2* p = (const dl::P2*)pts;
    const size_t cells = (size_t)V * H * W;
    const size_t first = cells > (size_t)kHdr ? cells : (size_t)kHdr;
    hipLaunchKernelGGL(dl_init_kernel, dim3(blocks_of(first)), dim3(kThreads), 0, s, V, N, cells, pt_off, status, w + L.hdr, w + L.cell_count);
    if (N > 0) {
        const dim3 per_point(blocks_of((size_t)N)), per_view((unsigned)V), block(kThreads);
        hipLaunchKernelGGL(dl_count_kernel, per_point, block, 0, s, V, H, W, N, p, pt_off, status, w + L.cell_count);
        hipLaunchKernelGGL(dl_cell_scan_kernel, per_view, block, 0, s, H, W, (const int*)status, (const int*)(w + L.cell_count),
                           w + L.cell_start, w + L.view_ok);
        hipLaunchKernelGGL(dl_scatter_kernel, per_point, block, 0, s, V, H, W, N, p, pt_off, (const int*)(w + L.view_ok), w + L.cell_count,
                           (const int*)(w + L.cell_start), w + L.cell_pts);
        hipLaunchKernelGGL(dl_cell_sort_kernel, dim3(blocks_of(cells)), block, 0, s, V, H, W, N, pt_off, (const int*)(w + L.view_ok),
                           (const int*)(w + L.cell_start), w + L.cell_pts);
        hipLaunchKernelGGL(dl_star_lane_kernel, per_point, block, 0, s, V, H, W, N, L.dcap, p, pt_off, (const int*)(w + L.view_ok),
                           (const int*)(w + L.cell_start), (const int*)(w + L.cell_pts), status, w + L.hdr, w + L.rec, w + L.loc,
                           w + L.lane_star, w + L.deferred);
        hipLaunchKernelGGL(dl_star_deferred_kernel, dim3(blocks_of((size_t)L.dcap * MOM_WAVE)), block, 0, s, V, H, W, N, L.dcap, L.pool, p, pt_off,
                           (const int*)(w + L.view_ok), (const int*)(w + L.cell_start), (const int*)(w + L.cell_pts), status, w + L.hdr,
                           w + L.rec, w + L.loc, (const int*)(w + L.deferred), w + L.def_star);
        hipLaunchKernelGGL(dl_view_scan_kernel, per_view, block, 0, s, N, L.pool, (const int*)(w + L.hdr), pt_off, (const int*)(w + L.view_ok), (const int*)(w + L.rec),
                           w + L.toff, status, w + L.view_T);
        hipLaunchKernelGGL(dl_off_scan_kernel, dim3(1), block, 0, s, V, (const int*)(w + L.view_T), tri_off);
        hipLaunchKernelGGL(dl_emit_kernel, per_point, block, 0, s, V, N, L.pool, pt_off, (const int*)status, (const int*)(w + L.rec),
                           (const int*)(w + L.loc), (const int*)(w + L.toff), (const int*)tri_off, w + L.lane_star, w + L.def_star, tris);
    } else {
        hipLaunchKernelGGL(dl_off_scan_kernel, dim3(1), dim3(kThreads), 0, s, V, (const int*)(w + L.cell_count), tri_off);     // zeros
    }
    return hipGetLastError() == hipSuccess ? MOM_OK : MOM_ELAUNCH;
}

// The twin: host pointers, the same expressions (delaunay_dev.h), one view after the other.
extern "C" int mom_delaunay_host(int V, int H, int W, int N, const double* pts, const int* pt_off, int* tris, int* tri_off, int* status)
{
    Layout L;
    if (!layout(V, H, W, N, &L)) return MOM_EINVAL;
    if (!pt_off || !tri_off || !status || (N > 0 && (!pts || !tris))) return MOM_EINVAL;
    const dl::P2* all = (const dl::P2*)pts;
    const size_t hw = (size_t)H * W;
    std::vector<int> start(hw + 1), cell_pts, star(kMax), recs, degs, at, stars;
    size_t T = 0;
    for (int j = 0; j < V; ++j) {
        tri_off[j] = (int)T;
        int pb, n;
        const bool ranged = view_range(pt_off, j, N, pb, n);
        int st = (ranged && n >= 3) ? MOM_DELAUNAY_OK : MOM_DELAUNAY_FEW;
        for (int i = 0; i < n; ++i)
            if (!in_frame(all[pb + i], H, W)) st = st > MOM_DELAUNAY_RANGE ? st : MOM_DELAUNAY_RANGE;
        status[j] = st;
        if (st != MOM_DELAUNAY_OK) continue;
        std::fill(start.begin(), start.end(), 0);
        for (int i = 0; i < n; ++i) ++start[(size_t)(int)all[pb + i].y * W + (int)all[pb + i].x + 1];
        for (size_t c = 0; c < hw; ++c) start[c + 1] += start[c];
        cell_pts.assign(n, 0);
        {
            std::vector<int> cursor(start.begin(), start.end() - 1);
            for (int i = 0; i < n; ++i) cell_pts[cursor[(size_t)(int)all[pb + i].y * W + (int)all[pb + i].x]++] = i;
        }
        dl::View v;
        v.pts = all + pb; v.cell_start = start.data(); v.cell_pts = cell_pts.data(); v.n = n; v.H = H; v.W = W;
        recs.assign(n, 0);
        degs.assign(n, 0);
        at.assign(n, 0);
        stars.clear();
        size_t count = 0;
        int hull = 0;
        for (int p = 0; p < n; ++p) {
            dl::Star S;
            S.s = star.data(); S.stride = 1; S.cap = kMax; S.m = 0; S.gap = -1;
            int gap;
            const int rc = dl::build_star<0>(v, p, S, false, &gap);
            if (rc == dl::kDone) {
                degs[p] = S.m;
                at[p] = (int)stars.size();
                stars.insert(stars.end(), star.begin(), star.begin() + S.m);
                recs[p] = rec_of(dl::upper_count(S, p, gap), S.m, gap);
                count += (size_t)rec_count(recs[p]);
                hull += gap >= 0;
            } else {
                const int code = rc == dl::kOverflow ? MOM_DELAUNAY_OVERFLOW : MOM_DELAUNAY_UNCERTAIN;
                st = st > code ? st : code;
            }
        }
        if (st == MOM_DELAUNAY_OK && count != (size_t)(2 * n - 2 - hull)) st = MOM_DELAUNAY_INCONSISTENT;
        status[j] = st;
        if (st != MOM_DELAUNAY_OK) continue;
        size_t first = T;
        for (int p = 0; p < n; ++p) {
            dl::Star S;
            S.s = stars.data() + at[p]; S.stride = 1; S.cap = kMax; S.m = degs[p]; S.gap = rec_gap(recs[p]);
            dl::emit_star(S, p, rec_gap(recs[p]), tris, first, 2 * (size_t)N);
            first += (size_t)rec_count(recs[p]);
        }
        T += count;
    }
    tri_off[V] = (int)T;
    return MOM_OK;
}
