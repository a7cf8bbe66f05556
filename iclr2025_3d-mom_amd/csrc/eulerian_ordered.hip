// The ordered form of the warp's splat (include/mom4d.h, "ordered splat of the video generator's warp"), gfx950: the accumulator of
// mom_eulerian_blend and the output of mom_softsplat_sum as a function of their inputs, bit for bit.  A PULL form, as the ordered
// HexPlane backward is one -- a texel's sum is formed by the texel's owner from the entries of the four cells around it -- with no
// float atomic anywhere:
//
//   entries    per (source pixel, half): the chain walk and the target of the atomic form (eulerian_dev.h), left as one 16-byte record
//              {ox, oy, Z, source index}, and the key (y0 + 1) (W + 1) + (x0 + 1) of its cell; an entry without terms gets the key
//              behind the last cell;
//   sort       the stable LSD sort of knn.hip on (key, entry) from the identity: a cell's entries are consecutive and ascending;
//   segments   the first sorted position of every cell, by binary search;
//   channels   for 16 channels and more, a channel-last copy of the feature, so that one term's C values are one contiguous run;
//   pull       one lane per (texel, channel), the channel on the fastest lanes: the four classes' sums in registers, blocks of 64
//              terms from each segment's start, one plain store -- a wave writes 256 contiguous bytes of the accumulator.
//
// A cell that many chains converge on is walked serially by every lane of its four texels; the blocks of 64 are in the order so that
// a later version can spread such a cell over lanes without changing a bit.
// THIS FILE IS COMPILED WITH -ffp-contract=off: the host twins at its end must multiply and add exactly as the kernels do.
#include "eulerian_dev.h"
#include <vector>

int mom_sort_pairs_u32(int n, int bits, unsigned* keys[2], unsigned* vals[2], unsigned* counts, hipStream_t s);   // knn.hip
size_t mom_sort_pairs_counts_bytes(int n);

namespace {

constexpr int kThreads = 256;
constexpr unsigned kBlk = 64;             // terms per block (include/mom4d.h)
constexpr int kChannelLast = 16;          // from this many channels on the blend reads a channel-last copy of the feature
constexpr size_t kMaxEntries = (size_t)1 << 30;     // the sort's positions are ints formed as workgroup * 4096 + item
constexpr size_t kMaxGrid = (size_t)1 << 24;        // workgroups of a grid-stride launch

struct Rec { float ox, oy, z; int src; };           // one entry: its target, its half's Z, where its values lie

// s_k of include/mom4d.h over the sorted positions [p0, p1): blocks of 64 from the first, every sum left to right from +0.0
template <typename Term>
__host__ __device__ __forceinline__ float class_sum(unsigned p0, unsigned p1, Term term)
{
    float s = 0.0f;
    for (unsigned b = p0; b < p1; b += kBlk) {
        const unsigned end = p1 - b < kBlk ? p1 : b + kBlk;
        float blk = 0.0f;
        for (unsigned t = b; t < end; t++) blk = blk + term(t);
        s = s + blk;
    }
    return s;
}

// the cell a texel's class k draws from, as an index into the (H + 1) x (W + 1) table of cells [-1, H-1] x [-1, W-1]
__host__ __device__ __forceinline__ unsigned class_cell(int y, int x, int k, int W) { return (unsigned)((y + 1 - (k >> 1)) * (W + 1) + (x + 1 - (k & 1))); }

__host__ __device__ __forceinline__ unsigned cell_key(float ox, float oy, int W, int H, unsigned ncells)
{
    int x0, y0;
    return splat_cell(ox, oy, W, H, &x0, &y0) ? (unsigned)((y0 + 1) * (W + 1) + (x0 + 1)) : ncells;
}

__host__ __device__ __forceinline__ Rec blend_entry(unsigned e, int S, const Geometry& g, int idx, int n_frames, float z_future,
                                                    float z_past, const float* __restrict__ motion)
{
    const unsigned npix = (unsigned)g.P * (unsigned)g.P;
    const int half = e >= npix;
    const unsigned pix = e - (half ? npix : 0u);
    const int px = (int)(pix % (unsigned)g.P), py = (int)(pix / (unsigned)g.P);
    const float2 o = blend_target(px, py, half, S, g, idx, n_frames, motion);
    return Rec{o.x, o.y, half ? z_past : z_future, (reflect(py - g.pad, g.s) + g.cut) * S + (reflect(px - g.pad, g.s) + g.cut)};
}

// ---- entries -------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kThreads)
blend_entries_kernel(unsigned n, unsigned ncells, int S, Geometry g, int idx, int n_frames, float z_future, float z_past,
                     const float* __restrict__ motion, Rec* __restrict__ rec, unsigned* __restrict__ keys, unsigned* __restrict__ vals)
{
    const unsigned e = blockIdx.x * kThreads + threadIdx.x;
    if (e >= n) return;
    const Rec r = blend_entry(e, S, g, idx, n_frames, z_future, z_past, motion);
    rec[e] = r;
    keys[e] = cell_key(r.ox, r.oy, g.P, g.P, ncells);
    vals[e] = e;
}

__global__ void __launch_bounds__(kThreads)
splat_entries_kernel(unsigned n, unsigned ncells, int H, int W, const float* __restrict__ flow, Rec* __restrict__ rec,
                     unsigned* __restrict__ keys, unsigned* __restrict__ vals)
{
#pragma clang fp contract(off)
    const unsigned e = blockIdx.x * kThreads + threadIdx.x;
    if (e >= n) return;
    const int x = (int)(e % (unsigned)W), y = (int)(e / (unsigned)W);
    const Rec r = {(float)x + flow[e], (float)y + flow[(size_t)n + e], 1.0f, (int)e};
    rec[e] = r;
    keys[e] = cell_key(r.ox, r.oy, W, H, ncells);
    vals[e] = e;
}

// seg[c] = the first sorted position whose key is >= c, c = 0 .. ncells (seg[ncells] = the entries that have terms)
__global__ void __launch_bounds__(kThreads)
segments_kernel(unsigned n, unsigned ncells, const unsigned* __restrict__ sorted_keys, unsigned* __restrict__ seg)
{
    const unsigned c = blockIdx.x * kThreads + threadIdx.x;
    if (c > ncells) return;
    unsigned lo = 0, hi = n;
    while (lo < hi) {
        const unsigned mid = lo + ((hi - lo) >> 1);
        if (sorted_keys[mid] < c) lo = mid + 1;
        else hi = mid;
    }
    seg[c] = lo;
}

// feature [C][plane] -> [plane][C].  Workgroup: 64 pixels, 32 channels a pass, through LDS (both sides coalesced).
__global__ void __launch_bounds__(kThreads)
channel_last_kernel(int C, size_t plane, const float* __restrict__ feature, float* __restrict__ out)
{
    __shared__ float tile[32][65];
    const size_t p0 = (size_t)blockIdx.x * 64;
    for (int c0 = 0; c0 < C; c0 += 32) {
        __syncthreads();
        for (int i = threadIdx.x; i < 32 * 64; i += kThreads) {
            const int c = i / 64, p = i % 64;
            if (c0 + c < C && p0 + p < plane) tile[c][p] = feature[(size_t)(c0 + c) * plane + p0 + p];
        }
        __syncthreads();
        for (int i = threadIdx.x; i < 32 * 64; i += kThreads) {
            const int p = i / 32, c = i % 32;
            if (c0 + c < C && p0 + p < plane) out[(p0 + p) * C + c0 + c] = tile[c][p];
        }
    }
}

// ---- pull ----------------------------------------------------------------------------------------------------------------------
// One lane per (texel, channel) of acc [P,P,C+1], the channel fastest: the lanes of a texel read the same records and, with the
// channel-last copy, consecutive floats of one feature row.
template <bool CHANNEL_LAST>
__global__ void __launch_bounds__(kThreads)
blend_pull_kernel(size_t total, int C, int P, size_t plane, const float* __restrict__ feat, const Rec* __restrict__ rec,
                  const unsigned* __restrict__ seg, const unsigned* __restrict__ sorted_e, float* __restrict__ acc)
{
    const unsigned C1 = (unsigned)C + 1;
    for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < total; i += (size_t)gridDim.x * kThreads) {
        const unsigned tex = (unsigned)(i / C1), c = (unsigned)(i % C1);
        const int y = (int)(tex / (unsigned)P), x = (int)(tex % (unsigned)P);
        float s[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const unsigned cell = class_cell(y, x, k, P);
            s[k] = class_sum(seg[cell], seg[cell + 1], [&](unsigned t) {
                const Rec r = rec[sorted_e[t]];
                const float f = c < (unsigned)C ? (CHANNEL_LAST ? feat[(size_t)r.src * C + c] : feat[(size_t)c * plane + r.src]) : 1.0f;
                return (f * r.z) * splat_weight(r.ox, r.oy, k);
            });
        }
        acc[i] = (s[0] + s[1]) + (s[2] + s[3]);
    }
}

// One lane per (channel, y, x) of one image's output [C,H,W], x fastest.  A texel without a term is not written.
__global__ void __launch_bounds__(kThreads)
splat_pull_kernel(size_t total, int H, int W, const float* __restrict__ input, const Rec* __restrict__ rec,
                  const unsigned* __restrict__ seg, const unsigned* __restrict__ sorted_e, float* __restrict__ output)
{
    const size_t plane = (size_t)H * W;
    for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < total; i += (size_t)gridDim.x * kThreads) {
        const size_t c = i / plane;
        const unsigned tex = (unsigned)(i % plane);
        const int y = (int)(tex / (unsigned)W), x = (int)(tex % (unsigned)W);
        float s[4];
        bool any = false;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const unsigned cell = class_cell(y, x, k, W);
            const unsigned p0 = seg[cell], p1 = seg[cell + 1];
            any = any || p1 > p0;
            s[k] = class_sum(p0, p1, [&](unsigned t) {
                const Rec r = rec[sorted_e[t]];
                return input[c * plane + (unsigned)r.src] * splat_weight(r.ox, r.oy, k);
            });
        }
        if (any) output[i] = output[i] + ((s[0] + s[1]) + (s[2] + s[3]));
    }
}

// ---- what the calls take, and their scratch ---------------------------------------------------------------------------------------
bool blend_takes(int C, int S, Geometry* g)
{
    if (C < 1 || !geometry(S, g)) return false;
    const size_t npix = (size_t)g->P * g->P;
    if (npix * (size_t)(C + 1) >= ((size_t)1 << 40)) return false;                       // as mom_eulerian_blend
    return 2 * npix <= kMaxEntries;                                                        // cells: (P + 1)^2 < 2^31 follows
}
bool splat_takes(int N, int C, int H, int W)
{
    if (N < 1 || C < 1 || H < 1 || W < 1) return false;
    if ((size_t)H * W >= ((size_t)1 << 31)) return false;                                 // as mom_softsplat_sum
    return (size_t)H * W <= kMaxEntries && ((size_t)H + 1) * ((size_t)W + 1) < ((size_t)1 << 31);
}

struct View {
    Rec* rec;             // [n]
    unsigned* keys[2];    // [n]
    unsigned* vals[2];    // [n]
    unsigned* counts;
    unsigned* seg;        // [ncells + 1]
    float* chlast;        // [feat_floats]
};

size_t view(size_t n, size_t ncells, size_t feat_floats, char* base, View* v)
{
    size_t off = 0;
    const size_t o_r = off; off = mom_align_up(off + n * sizeof(Rec));
    size_t o_k[2], o_v[2];
    for (int i = 0; i < 2; i++) { o_k[i] = off; off = mom_align_up(off + n * 4); }
    for (int i = 0; i < 2; i++) { o_v[i] = off; off = mom_align_up(off + n * 4); }
    const size_t o_c = off; off = mom_align_up(off + mom_sort_pairs_counts_bytes((int)n));
    const size_t o_s = off; off = mom_align_up(off + (ncells + 1) * 4);
    const size_t o_f = off; off = mom_align_up(off + feat_floats * 4);
    if (v) {
        v->rec = (Rec*)(base + o_r);
        for (int i = 0; i < 2; i++) { v->keys[i] = (unsigned*)(base + o_k[i]); v->vals[i] = (unsigned*)(base + o_v[i]); }
        v->counts = (unsigned*)(base + o_c);
        v->seg = (unsigned*)(base + o_s);
        v->chlast = (float*)(base + o_f);
    }
    return off;
}

size_t blend_view(int C, int S, const Geometry& g, char* base, View* v)
{
    const size_t P = (size_t)g.P;
    return view(2 * P * P, (P + 1) * (P + 1), C >= kChannelLast ? (size_t)S * S * C : 0, base, v);
}
size_t splat_view(int H, int W, char* base, View* v) { return view((size_t)H * W, ((size_t)H + 1) * ((size_t)W + 1), 0, base, v); }

bool scratch_ok(const void* scratch, size_t have, size_t need) { return scratch && ((uintptr_t)scratch & (MOM_ALIGN - 1)) == 0 && have >= need; }

unsigned grid_for(size_t total) { const size_t b = (total + kThreads - 1) / kThreads; return (unsigned)(b < kMaxGrid ? b : kMaxGrid); }

// sort the entries by cell and leave the segment table; the index (0 / 1) of the buffers that hold the sorted pairs, or an error
int sort_and_segment(unsigned n, unsigned ncells, View& v, hipStream_t s)
{
    int bits = 1;
    while (bits < 32 && (1ull << bits) <= (unsigned long long)ncells) bits++;            // keys run to ncells inclusive
    const int cur = mom_sort_pairs_u32((int)n, bits, v.keys, v.vals, v.counts, s);
    if (cur < 0) return cur;
    hipLaunchKernelGGL(segments_kernel, dim3((ncells + 1 + kThreads - 1) / kThreads), dim3(kThreads), 0, s, n, ncells, v.keys[cur], v.seg);
    return hipGetLastError() == hipSuccess ? cur : MOM_ELAUNCH;
}

// ---- the documented order on the host: a stable counting sort by cell, then every texel's classes ----------------------------------
void host_segments(const std::vector<unsigned>& key, size_t ncells, std::vector<unsigned>* seg, std::vector<unsigned>* ord)
{
    seg->assign(ncells + 2, 0);
    for (unsigned k : key) (*seg)[k + 1]++;
    for (size_t c = 0; c <= ncells; c++) (*seg)[c + 1] += (*seg)[c];
    std::vector<unsigned> at(seg->begin(), seg->end() - 1);
    ord->resize(key.size());
    for (size_t e = 0; e < key.size(); e++) (*ord)[at[key[e]]++] = (unsigned)e;           // ascending e inside a cell
}

}  // namespace

extern "C" size_t mom_eulerian_ordered_scratch_bytes(int C, int S)
{
    Geometry g;
    return blend_takes(C, S, &g) ? blend_view(C, S, g, nullptr, nullptr) : 0;
}

extern "C" int mom_eulerian_blend_ordered(int C, int H, int W, int idx, int n_frames, const float* feature, const float* motion,
                                          float* acc, void* scratch, size_t scratch_bytes, mom_stream_t stream)
{
    Geometry g;
    if (H != W || n_frames < 2 || idx < 0 || idx >= n_frames || !feature || !motion || !acc) return MOM_EINVAL;
    if (!blend_takes(C, H, &g) || !scratch_ok(scratch, scratch_bytes, blend_view(C, H, g, nullptr, nullptr))) return MOM_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    View v;
    blend_view(C, H, g, (char*)scratch, &v);
    const size_t npix = (size_t)g.P * g.P, plane = (size_t)H * H;
    const unsigned n = (unsigned)(2 * npix), ncells = (unsigned)((g.P + 1) * (g.P + 1));
    float z_future, z_past;
    blend_z(idx, n_frames, &z_future, &z_past);
    hipLaunchKernelGGL(blend_entries_kernel, dim3((n + kThreads - 1) / kThreads), dim3(kThreads), 0, s, n, ncells, H, g, idx, n_frames,
                       z_future, z_past, motion, v.rec, v.keys[0], v.vals[0]);
    const bool chlast = C >= kChannelLast;
    if (chlast)
        hipLaunchKernelGGL(channel_last_kernel, dim3((unsigned)((plane + 63) / 64)), dim3(kThreads), 0, s, C, plane, feature, v.chlast);
    const int cur = sort_and_segment(n, ncells, v, s);
    if (cur < 0) return cur;
    const size_t total = npix * (size_t)(C + 1);
    if (chlast)
        hipLaunchKernelGGL(blend_pull_kernel<true>, dim3(grid_for(total)), dim3(kThreads), 0, s, total, C, g.P, plane, v.chlast, v.rec,
                           v.seg, v.vals[cur], acc);
    else
        hipLaunchKernelGGL(blend_pull_kernel<false>, dim3(grid_for(total)), dim3(kThreads), 0, s, total, C, g.P, plane, feature, v.rec,
                           v.seg, v.vals[cur], acc);
    return hipGetLastError() == hipSuccess ? MOM_OK : MOM_ELAUNCH;
}

extern "C" size_t mom_softsplat_ordered_scratch_bytes(int N, int C, int H, int W)
{
    return splat_takes(N, C, H, W) ? splat_view(H, W, nullptr, nullptr) : 0;
}

extern "C" int mom_softsplat_sum_ordered(int N, int C, int H, int W, const float* input, const float* flow, float* output,
                                         void* scratch, size_t scratch_bytes, mom_stream_t stream)
{
    if (!splat_takes(N, C, H, W) || !input || !flow || !output) return MOM_EINVAL;
    if (!scratch_ok(scratch, scratch_bytes, splat_view(H, W, nullptr, nullptr))) return MOM_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    View v;
    splat_view(H, W, (char*)scratch, &v);
    const size_t plane = (size_t)H * W, total = plane * (size_t)C;
    const unsigned n = (unsigned)plane, ncells = (unsigned)((H + 1) * (W + 1));
    for (int img = 0; img < N; img++) {                           // one image after the other out of the same scratch
        hipLaunchKernelGGL(splat_entries_kernel, dim3((n + kThreads - 1) / kThreads), dim3(kThreads), 0, s, n, ncells, H, W,
                           flow + (size_t)img * 2 * plane, v.rec, v.keys[0], v.vals[0]);
        const int cur = sort_and_segment(n, ncells, v, s);
        if (cur < 0) return cur;
        hipLaunchKernelGGL(splat_pull_kernel, dim3(grid_for(total)), dim3(kThreads), 0, s, total, H, W, input + (size_t)img * total, v.rec,
                           v.seg, v.vals[cur], output + (size_t)img * total);
    }
    return hipGetLastError() == hipSuccess ? MOM_OK : MOM_ELAUNCH;
}

extern "C" int mom_eulerian_blend_ordered_host(int C, int H, int W, int idx, int n_frames, const float* feature, const float* motion,
                                               float* acc)
{
    Geometry g;
    if (H != W || n_frames < 2 || idx < 0 || idx >= n_frames || !feature || !motion || !acc) return MOM_EINVAL;
    if (!blend_takes(C, H, &g)) return MOM_EINVAL;
    const int P = g.P;
    const size_t npix = (size_t)P * P, plane = (size_t)H * H, n = 2 * npix, ncells = ((size_t)P + 1) * ((size_t)P + 1);
    float z_future, z_past;
    blend_z(idx, n_frames, &z_future, &z_past);
    std::vector<Rec> rec(n);
    std::vector<unsigned> key(n), seg, ord;
    for (size_t e = 0; e < n; e++) {
        rec[e] = blend_entry((unsigned)e, H, g, idx, n_frames, z_future, z_past, motion);
        key[e] = cell_key(rec[e].ox, rec[e].oy, P, P, (unsigned)ncells);
    }
    host_segments(key, ncells, &seg, &ord);
    for (int y = 0; y < P; y++)
        for (int x = 0; x < P; x++)
            for (int c = 0; c <= C; c++) {
                float s[4];
                for (int k = 0; k < 4; k++) {
                    const unsigned cell = class_cell(y, x, k, P);
                    s[k] = class_sum(seg[cell], seg[cell + 1], [&](unsigned t) {
                        const Rec& r = rec[ord[t]];
                        const float f = c < C ? feature[(size_t)c * plane + r.src] : 1.0f;
                        return (f * r.z) * splat_weight(r.ox, r.oy, k);
                    });
                }
                acc[((size_t)y * P + x) * (C + 1) + c] = (s[0] + s[1]) + (s[2] + s[3]);
            }
    return MOM_OK;
}

extern "C" int mom_softsplat_sum_ordered_host(int N, int C, int H, int W, const float* input, const float* flow, float* output)
{
    if (!splat_takes(N, C, H, W) || !input || !flow || !output) return MOM_EINVAL;
    const size_t plane = (size_t)H * W, ncells = ((size_t)H + 1) * ((size_t)W + 1);
    std::vector<Rec> rec(plane);
    std::vector<unsigned> key(plane), seg, ord;
    for (int img = 0; img < N; img++) {
        const float* fl = flow + (size_t)img * 2 * plane;
        for (size_t e = 0; e < plane; e++) {
            const int x = (int)(e % W), y = (int)(e / W);
            rec[e] = Rec{(float)x + fl[e], (float)y + fl[plane + e], 1.0f, (int)e};
            key[e] = cell_key(rec[e].ox, rec[e].oy, W, H, (unsigned)ncells);
        }
        host_segments(key, ncells, &seg, &ord);
        for (int c = 0; c < C; c++) {
            const float* in = input + ((size_t)img * C + c) * plane;
            float* out = output + ((size_t)img * C + c) * plane;
            for (int y = 0; y < H; y++)
                for (int x = 0; x < W; x++) {
                    float s[4];
                    bool any = false;
                    for (int k = 0; k < 4; k++) {
                        const unsigned cell = class_cell(y, x, k, W);
                        any = any || seg[cell + 1] > seg[cell];
                        s[k] = class_sum(seg[cell], seg[cell + 1], [&](unsigned t) {
                            const Rec& r = rec[ord[t]];
                            return in[r.src] * splat_weight(r.ox, r.oy, k);
                        });
                    }
                    if (any) out[(size_t)y * W + x] = out[(size_t)y * W + x] + ((s[0] + s[1]) + (s[2] + s[3]));
                }
        }
    }
    return MOM_OK;
}
