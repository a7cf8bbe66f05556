// Deformation field in one launch for 16-channel HexPlane fields (dnerf/eulerian_150_16: two levels of 16 channels, net_width 64,
// defor_depth 0), forward, one timestamp for all points, gfx950.
//
// The result of mom_hexplane_forward (channels 16, two levels; hexplane.hip at C = 16) followed by mom_deform_forward_activated_n
// (in_features 32; deform_mlp.hip), bit for bit, without feat[P,32] in between: a wave gathers the 32 features of its tile of 32
// Gaussians into LDS, reads them back as the trunk layer's B operand and runs deform_fwd_kernel<1>'s MLP on them.  fp32 throughout
// (v_mfma_f32_32x32x2_f32, the k-ascending chains of deform_mlp_dev.h): no bf16 split and no per-frame time
// lines here -- both reassociate sums, and a no-grad render() of such a model has to give the image of the op-by-op route.
//
// Gather (the lane mapping of hexplane.hip at C = 16): sixteen lanes own one (point, level), lane = channel; the wave's four groups take
// the points 4 i + q of the tile, i = 0..7, first at level 0, then at level 1.  What a (point, level) needs of its position is
// separable by axis -- cell index and fraction along x, y, z at that level's resolution -- and is computed ONCE, by lane
// (point, level) of the wave, into a 16-byte LDS record {x0 | y0 << 10 | z0 << 20, bx, by, bz}; the time axis is the same for every
// point.  The sixteen lanes of a group read the record as one broadcast and form the six planes' offsets and weights from it with
// the expressions of hexplane.hip's make_rec_fwd (ATen's weights from b = ix - x0 and 1 - b; a corner outside the plane gets
// weight exactly 0 and the address of its neighbour), so every sample, and the product over the planes in the reference's order,
// is that kernel's.  hexplane.hip keeps 32-byte records per (point, PLANE), 6 KB per wave and level: sixteen waves of those do
// not fit beside the weights.
//
// LDS, 1024 threads = sixteen waves around one copy of the weights (deform_mlp_dev.h's map, 70 720 B):
//   per wave  feature tile [32 Gaussians][36 floats]  4608 B   (32 features + 4 pad: the operand reads, 16 bytes per lane at a row
//                                                               stride of 36 banks, spread sixteen consecutive lanes over all 64 banks)
//             records      [2 levels][32 points] x 16 B  1024 B   (the four groups read four ADJACENT records: four banks apart)
//   70 720 + 16 x 5632 = 160 832 B of the CU's 163 840.
#include "deform_mlp_dev.h"
#include "hexplane_dev.h"

namespace {

constexpr int kC16 = 16;                             // channels = floats of one texel row
constexpr unsigned kRow16B = kC16 * 4u;              // bytes of one texel row
constexpr int kF16Waves = 16;                        // waves per workgroup
constexpr int kF16In = 32;                           // features of a Gaussian: two levels of kC16 channels
constexpr int kTileStride = kF16In + 4;              // floats of one Gaussian's row of the feature tile
constexpr int kTileFloats = 32 * kTileStride;
constexpr int kRecFloats = 2 * 32 * 4;               // uint4 [level][point]
constexpr int kLTile = kLFwdTotal;                   // [kF16Waves][kTileFloats]
constexpr int kLRec = kLTile + kF16Waves * kTileFloats;
constexpr int kLField16Total = kLRec + kF16Waves * kRecFloats;
constexpr int kMaxRes16 = 1024;                      // a cell index is 10 bits of the record's first word
static_assert(kLField16Total * 4 <= 160 * 1024, "LDS of deform_field16_fwd_kernel");
static_assert((kLTile * 4) % 16 == 0 && (kLRec * 4) % 16 == 0 && (kTileStride * 4) % 16 == 0, "16-byte LDS accesses");

// a.res[lvl][k] for a level that differs between the lanes of a wave, picked from the two scalar values (see res_of in
// deform_field.hip: indexed with a vector register the argument block is read from memory)
__device__ __forceinline__ int res16_of(const HexArgs& a, int lvl, int k)
{
    int r0 = a.res[0][k], r1 = a.res[1][k];
    asm volatile("" : "+s"(r0), "+s"(r1));
    return lvl == 1 ? r1 : r0;
}

// cell and fraction of a coordinate along one axis: make_rec_fwd's ix, x0 and bx
__device__ __forceinline__ void axis_cell(float c, int size, int& i0, float& b)
{
    float gm;
    const float ix = unnorm_clip(c, size, gm);
    i0 = (int)floorf(ix);
    b = ix - (float)i0;
}

// one plane's bilinear sample at this lane's channel (hexplane_fwd4_kernel<16>'s, term by term): `pl` already points at the channel,
// o00 is the byte offset of texel (y0, x0), sx / sy the byte steps to x0 + 1 / y0 + 1 (0 when that neighbour is outside)
__device__ __forceinline__ float sample16(const float* __restrict__ pl, unsigned o00, unsigned sx, unsigned sy, float ax, float bx,
                                          float ay, float by)
{
    const uint4 o = make_uint4(o00, o00 + sx, o00 + sy, o00 + sy + sx);
    const float4 w = make_float4(ax * ay, bx * ay, ax * by, bx * by);
    float v = 0.f;
    v += ld_f32(pl, o.x) * w.x;
    v += ld_f32(pl, o.y) * w.y;
    v += ld_f32(pl, o.z) * w.z;
    v += ld_f32(pl, o.w) * w.w;
    return v;
}

// The 32 features of the tile's Gaussians into `tile` (and into their rows of feat_save [P,32] if the caller keeps a copy).
// g_mine: the Gaussian of point (lane & 31) of the tile, -1 past the end; npts: points of the tile (1..32).
__device__ __forceinline__ void gather16_tile(const HexArgs& a, const float* __restrict__ xyz, int g_mine, int npts,
                                              uint4* __restrict__ rec, float* __restrict__ tile, float* __restrict__ feat_save, int lane)
{
    // phase A: lane = (point lane & 31, level lane >> 5)
    {
        const int lvl = lane >> 5;
        uint4 R = make_uint4(0u, 0u, 0u, 0u);            // past the end: cell 0 with weight 1, a fetch inside every plane
        if (g_mine >= 0) {
            float c[4];
            norm_coords(a, xyz, g_mine, c);
            int i0[3];
            float b[3];
#pragma unroll
            for (int k = 0; k < 3; k++) axis_cell(c[k], res16_of(a, lvl, k), i0[k], b[k]);
            R = make_uint4((unsigned)i0[0] | ((unsigned)i0[1] << 10) | ((unsigned)i0[2] << 20), __float_as_uint(b[0]),
                           __float_as_uint(b[1]), __float_as_uint(b[2]));
        }
        rec[lane] = R;
    }
    __builtin_amdgcn_wave_barrier();
    // phase B: group q takes the points 4 i + q
    const int ch = lane & 15, q = lane >> 4;
    const int iters = (npts + 3) >> 2;
#pragma unroll 1
    for (int lvl = 0; lvl < 2; lvl++) {
        const int Wx = a.res[lvl][0], Wy = a.res[lvl][1], Wz = a.res[lvl][2], Td = a.res[lvl][3];
        const float* __restrict__ pxy = a.planes[lvl][0] + ch;
        const float* __restrict__ pxz = a.planes[lvl][1] + ch;
        const float* __restrict__ pxt = a.planes[lvl][2] + ch;
        const float* __restrict__ pyz = a.planes[lvl][3] + ch;
        const float* __restrict__ pyt = a.planes[lvl][4] + ch;
        const float* __restrict__ pzt = a.planes[lvl][5] + ch;
        int t0;
        float bt;
        axis_cell(a.time, Td, t0, bt);
        const float at = 1.f - bt;
        const bool ht = t0 + 1 < Td;
        const unsigned rowx = (unsigned)Wx * kRow16B, rowy = (unsigned)Wy * kRow16B, rowz = (unsigned)Wz * kRow16B;
        const unsigned st_x = ht ? rowx : 0u, st_y = ht ? rowy : 0u, st_z = ht ? rowz : 0u;
#pragma unroll 1
        for (int i = 0; i < iters; i++) {
            const int pt = 4 * i + q;
            const uint4 R = rec[32 * lvl + pt];
            const int x0 = (int)(R.x & 1023u), y0 = (int)((R.x >> 10) & 1023u), z0 = (int)(R.x >> 20);
            const float bx = __uint_as_float(R.y), by = __uint_as_float(R.z), bz = __uint_as_float(R.w);
            const float ax = 1.f - bx, ay = 1.f - by, az = 1.f - bz;
            const unsigned sx = (x0 + 1 < Wx) ? kRow16B : 0u, sy = (y0 + 1 < Wy) ? kRow16B : 0u, sz = (z0 + 1 < Wz) ? kRow16B : 0u;
            const unsigned ry_x = (y0 + 1 < Wy) ? rowx : 0u, rz_x = (z0 + 1 < Wz) ? rowx : 0u, rz_y = (z0 + 1 < Wz) ? rowy : 0u;
            // the reference's order of the product: (x,y) (x,z) (x,t) (y,z) (y,t) (z,t)
            float prod = 1.f;
            prod = prod * sample16(pxy, (unsigned)(y0 * Wx + x0) * kRow16B, sx, ry_x, ax, bx, ay, by);
            prod = prod * sample16(pxz, (unsigned)(z0 * Wx + x0) * kRow16B, sx, rz_x, ax, bx, az, bz);
            prod = prod * sample16(pxt, (unsigned)(t0 * Wx + x0) * kRow16B, sx, st_x, ax, bx, at, bt);
            prod = prod * sample16(pyz, (unsigned)(z0 * Wy + y0) * kRow16B, sy, rz_y, ay, by, az, bz);
            prod = prod * sample16(pyt, (unsigned)(t0 * Wy + y0) * kRow16B, sy, st_y, ay, by, at, bt);
            prod = prod * sample16(pzt, (unsigned)(t0 * Wz + z0) * kRow16B, sz, st_z, az, bz, at, bt);
            tile[pt * kTileStride + kC16 * lvl + ch] = prod;
            if (feat_save) {
                const int g = __shfl(g_mine, pt);            // (lanes 0..31 hold the tile's 32 points; every lane is active)
                if (g >= 0) feat_save[(size_t)g * kF16In + kC16 * lvl + ch] = prod;
            }
        }
    }
    __builtin_amdgcn_wave_barrier();
}

// one workgroup of sixteen waves per CU around one copy of the weights; a contiguous, equal (+-1) share of the tiles per workgroup,
// dealt to its waves (deform_fwd_kernel<1>'s loop with the gather in front of each tile)
__global__ void __launch_bounds__(64 * kF16Waves)
deform_field16_fwd_kernel(HexArgs a, MlpDev m, int tiles, const float* __restrict__ xyz, const float* __restrict__ scaling,
                          const float* __restrict__ rotation, const float* __restrict__ flow, float flow_coef,
                          float* __restrict__ pts, float* __restrict__ scales, float* __restrict__ rots,
                          float* __restrict__ feat_save, float* __restrict__ a0_save, ActOut act)
{
    extern __shared__ float lds[];
    load_weights<1>(m, lds);
    __syncthreads();
    const int lane = threadIdx.x & 63, col = lane & 31, h = lane >> 5, wv = threadIdx.x >> 6;
    float* __restrict__ tile = lds + kLTile + wv * kTileFloats;
    uint4* __restrict__ rec = reinterpret_cast<uint4*>(lds + kLRec + wv * kRecFloats);
    const int P = a.P;
    const int t_begin = (int)((long long)tiles * blockIdx.x / gridDim.x), t_end = (int)((long long)tiles * (blockIdx.x + 1) / gridDim.x);
    const int t_step = (int)(blockDim.x >> 6);
    for (int t = t_begin + wv; t < t_end; t += t_step) {
        const int gi = t * 32 + col;
        const int g = gi < P ? (a.order ? (int)a.order[gi] : gi) : -1;
        const bool ok = g >= 0;
        gather16_tile(a, xyz, g, min(32, P - t * 32), rec, tile, feat_save, lane);
        f32x16 a0[2];
        {
            // the tile's rows in the trunk layer's operand layout: register 4q+j of lane half h is feature 8q+4h+j
            f32x16 x[1];
            const float* row = tile + col * kTileStride + 4 * h;
#pragma unroll
            for (int qq = 0; qq < 4; qq++) {
                float4 v = *reinterpret_cast<const float4*>(row + 8 * qq);
                if (!ok) v = make_float4(0.f, 0.f, 0.f, 0.f);
                x[0][4 * qq + 0] = v.x;
                x[0][4 * qq + 1] = v.y;
                x[0][4 * qq + 2] = v.z;
                x[0][4 * qq + 3] = v.w;
            }
            __builtin_amdgcn_wave_barrier();                // (the next tile's gather writes these rows)
            init_bias(lds + kLB, a0, h);
            layer64<false>(lds + kLW, x, a0, col, h);
        }
        relu_tile(a0);
        if (a0_save) store_feat(a0_save, g, ok, h, a0);     // relu(h0) [P,64], what the backward kernels reuse
#pragma nounroll
        for (int head = 0; head < 3; head++) {
            f32x16 h1[2];
            init_bias(lds + kLB + (1 + head) * kHid, h1, h);
            layer64<false>(lds + kLW + (1 + head) * kWFloats, a0, h1, col, h);
            relu_tile(h1);
            float o[4];
            out_layer(lds + kLW2 + head * 4 * kHid, lds + kLB2 + head * 4, h1, h, o);
            if (h == 0 && ok) {
                if (head == 0) {
#pragma unroll
                    for (int k = 0; k < 3; k++) pts[3 * g + k] = xyz[3 * g + k] + (o[k] + flow_coef * flow[3 * g + k]);
                } else if (head == 1) {
                    float s3[3];
#pragma unroll
                    for (int k = 0; k < 3; k++) {
                        s3[k] = scaling[3 * g + k] + o[k];
                        scales[3 * g + k] = s3[k];
                    }
                    if (act.scales) {
#pragma unroll
                        for (int k = 0; k < 3; k++) act.scales[3 * g + k] = expf(s3[k]);
                    }
                } else {
                    const float4 r4 = *reinterpret_cast<const float4*>(rotation + 4 * g);
                    const float4 q4 = make_float4(r4.x + o[0], r4.y + o[1], r4.z + o[2], r4.w + o[3]);
                    *reinterpret_cast<float4*>(rots + 4 * g) = q4;
                    if (act.rots) {
                        const float n = mom_quat_norm(q4.x, q4.y, q4.z, q4.w);
                        *reinterpret_cast<float4*>(act.rots + 4 * g) = make_float4(q4.x / n, q4.y / n, q4.z / n, q4.w / n);
                    }
                    if (act.opacity) act.opacity[g] = mom_sigmoid(act.opacity_raw[g]);
                }
            }
        }
    }
}

int field16_cus()
{
    static int cus = 0;
    if (!cus) {
        int dev = 0, n = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n < 1)
            return 256;
        cus = n;
    }
    return cus;
}

}  // namespace

extern "C" int mom_deform_field16_supported(const MomHexPlane* hp)
{
    if (!hp || hp->channels != kC16 || hp->levels != 2) return 0;
    // a cell index is 10 bits of a record; with that every plane's byte offsets fit 32 bits (1024 x 1024 x 64 B = 2^26)
    for (int l = 0; l < 2; l++)
        for (int k = 0; k < 4; k++)
            if (hp->res[l][k] < 1 || hp->res[l][k] > kMaxRes16) return 0;
    return 1;
}

extern "C" size_t mom_deform_field16_scratch_bytes(const MomHexPlane* hp, int P)
{
    // nothing is staged in memory: no time lines (the space-time planes are sampled in full) and no feature buffer (the features
    // of a tile live in LDS).  One aligned block, so that a caller always has a pointer to pass.
    (void)hp;
    (void)P;
    return MOM_ALIGN;
}

extern "C" int mom_deform_field16_forward(const MomHexPlane* hp, const MomDeformMLP* w, int P, const float* xyz, float time,
                                          const uint32_t* order, const float* scaling, const float* rotation, const float* scene_flow,
                                          float flow_coef, float* pts, float* scales, float* rots, float* feat_save, float* a0_save,
                                          const float* opacity_raw, float* scales_act, float* rots_act, float* opacity_act,
                                          void* scratch, mom_stream_t stream)
{
    if (P < 0 || !mom_deform_field16_supported(hp)) return MOM_EINVAL;
    if (P == 0) return MOM_OK;
    (void)scratch;                                        // nothing is staged (mom_deform_field16_scratch_bytes); may be null
    if (!xyz || !scaling || !rotation || !scene_flow || !pts || !scales || !rots) return MOM_EINVAL;
    if ((opacity_act != nullptr) != (opacity_raw != nullptr)) return MOM_EINVAL;
    for (int l = 0; l < 2; l++)
        for (int p = 0; p < 6; p++)
            if (!hp->planes[l][p]) return MOM_EINVAL;
    MlpDev d;
    int rc = fill_dev(w, &d);
    if (rc) return rc;
    HexArgs a;
    fill_args(hp, P, nullptr, time, order, false, &a);
    hipStream_t s = (hipStream_t)stream;
    const int tiles = (P + 31) / 32;
    const int cus = field16_cus();
    const int blocks = tiles < cus ? tiles : cus;         // never more workgroups than tiles: a small problem is spread over the CUs
    const size_t lds_bytes = sizeof(float) * kLField16Total;
    if (!mom_lds_limit<deform_field16_fwd_kernel>(lds_bytes)) return MOM_ELAUNCH;
    const ActOut act = {scales_act, rots_act, opacity_act, opacity_raw};
    MomProfScope ps(MOM_P_HEX_FWD, s);
    hipLaunchKernelGGL(deform_field16_fwd_kernel, dim3(blocks), dim3(64 * kF16Waves), lds_bytes, s, a, d, tiles, xyz, scaling, rotation,
                       scene_flow, flow_coef, pts, scales, rots, feat_save, a0_save, act);
    return hipGetLastError() == hipSuccess ? MOM_OK : MOM_ELAUNCH;
}
