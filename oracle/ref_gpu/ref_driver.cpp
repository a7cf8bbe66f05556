// extern "C" layer over the public entry points of the reference's rasterizer and k-NN, for the tests that hold the CPU
// oracle and the HIP kernels to the reference's own kernels (tests/test_reference_kernels_gpu.py).  TEST INFRASTRUCTURE ONLY.
//
// Built by oracle/ref_gpu.py beside the reference's translation units, which are copied from a reference checkout at build
// time and never committed.  Everything here takes HOST pointers: inputs are uploaded, the reference runs on the device with
// debug = false, outputs are copied back.  Every function returns the first failing hipError_t (0 = hipSuccess), or
// REF_EXCEPTION if the reference threw, and synchronises the device before it returns.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <functional>
#include <stdexcept>
#include <vector>

#include "rasterizer_impl.h"   // CudaRasterizer::{Rasterizer, GeometryState, BinningState, ImageState} -- the reference's header
#include "simple_knn.h"

#define REF_EXCEPTION (-1)

namespace {

struct HipFailure { hipError_t err; };

inline void ck(hipError_t e) { if (e != hipSuccess) throw HipFailure{e}; }

// Device allocations of one call or one handle, released together.
struct Pool {
    std::vector<void*> ptrs;
    ~Pool() { for (void* p : ptrs) (void)hipFree(p); }
    void* raw(size_t bytes) {
        void* p = nullptr;
        ck(hipMalloc(&p, bytes ? bytes : 1));
        ptrs.push_back(p);
        return p;
    }
    template <typename T> T* zeros(size_t n) {
        T* p = static_cast<T*>(raw(n * sizeof(T)));
        ck(hipMemset(p, 0, n ? n * sizeof(T) : 1));
        return p;
    }
    // null stays null: the reference tells "not given" from "given" by the pointer
    template <typename T> T* upload(const T* host, size_t n) {
        if (!host || !n) return nullptr;
        T* p = static_cast<T*>(raw(n * sizeof(T)));
        ck(hipMemcpy(p, host, n * sizeof(T), hipMemcpyHostToDevice));
        return p;
    }
};

template <typename T> void download(T* host, const void* dev, size_t n) {
    if (host && n) ck(hipMemcpy(host, dev, n * sizeof(T), hipMemcpyDeviceToHost));
}

struct Handle {
    Pool pool;
    int P = 0, D = 0, M = 0, W = 0, H = 0, R = 0;
    float scale_modifier = 1.f, tan_fovx = 0.f, tan_fovy = 0.f;
    float *bg = nullptr, *means3D = nullptr, *shs = nullptr, *colors = nullptr, *opacities = nullptr, *scales = nullptr,
          *rotations = nullptr, *cov3D_precomp = nullptr, *view = nullptr, *proj = nullptr, *campos = nullptr;
    char *geom = nullptr, *binning = nullptr, *img = nullptr;      // the three state chunks, as forward() was handed them
    float *out_color = nullptr, *out_depth = nullptr;
    int* radii = nullptr;
};

std::function<char*(size_t)> chunk_of(Handle* h, char** slot) {
    return [h, slot](size_t n) {
        *slot = h->pool.zeros<char>(n);
        return *slot;
    };
}

template <typename F> int guarded(F&& body) {
    int status = hipSuccess;
    try {
        body();
    } catch (const HipFailure& f) {
        status = f.err;
    } catch (const std::exception&) {
        status = REF_EXCEPTION;
    }
    hipError_t e = hipDeviceSynchronize();
    if (status == hipSuccess && e != hipSuccess) status = e;
    e = hipGetLastError();
    if (status == hipSuccess && e != hipSuccess) status = e;
    return status;
}

}  // namespace

extern "C" {

// CudaRasterizer::Rasterizer::forward as RasterizeGaussiansCUDA calls it (P > 0; the caller short-circuits P == 0 as
// rasterize_points.cu does).  Absent inputs are null.  *handle_out owns every device buffer until ref_free.
int ref_forward(void** handle_out, int P, int D, int M, const float* background, int W, int H, const float* means3D,
                const float* shs, const float* colors_precomp, const float* opacities, const float* scales, float scale_modifier,
                const float* rotations, const float* cov3D_precomp, const float* viewmatrix, const float* projmatrix,
                const float* campos, float tan_fovx, float tan_fovy, int* num_rendered) {
    *handle_out = nullptr;
    if (P <= 0 || W <= 0 || H <= 0) return hipErrorInvalidValue;
    Handle* h = new Handle;
    int status = guarded([&] {
        h->P = P; h->D = D; h->M = M; h->W = W; h->H = H;
        h->scale_modifier = scale_modifier; h->tan_fovx = tan_fovx; h->tan_fovy = tan_fovy;
        const size_t n = P;
        h->bg = h->pool.upload(background, 3);
        h->means3D = h->pool.upload(means3D, n * 3);
        h->shs = h->pool.upload(shs, n * M * 3);
        h->colors = h->pool.upload(colors_precomp, n * 3);
        h->opacities = h->pool.upload(opacities, n);
        h->scales = h->pool.upload(scales, n * 3);
        h->rotations = h->pool.upload(rotations, n * 4);
        h->cov3D_precomp = h->pool.upload(cov3D_precomp, n * 6);
        h->view = h->pool.upload(viewmatrix, 16);
        h->proj = h->pool.upload(projmatrix, 16);
        h->campos = h->pool.upload(campos, 3);
        h->out_color = h->pool.zeros<float>(size_t(3) * W * H);
        h->out_depth = h->pool.zeros<float>(size_t(W) * H);
        h->radii = h->pool.zeros<int>(n);
        h->R = CudaRasterizer::Rasterizer::forward(
            chunk_of(h, &h->geom), chunk_of(h, &h->binning), chunk_of(h, &h->img), P, D, M, h->bg, W, H, h->means3D, h->shs,
            h->colors, h->opacities, h->scales, scale_modifier, h->rotations, h->cov3D_precomp, h->view, h->proj, h->campos,
            tan_fovx, tan_fovy, /*prefiltered=*/false, h->out_color, h->out_depth, h->radii, /*debug=*/false);
    });
    if (status != hipSuccess) {
        delete h;
        return status;
    }
    *num_rendered = h->R;
    *handle_out = h;
    return hipSuccess;
}

// The state of a forward, re-parsed from its chunks with the reference's own fromChunk.  Null outputs are skipped.
int ref_state_copy(void* handle, float* depths, float* means2D, float* cov3D, float* conic_opacity, float* rgb,
                   uint8_t* clamped, uint32_t* tiles_touched, uint32_t* point_offsets, uint64_t* point_list_keys,
                   uint32_t* point_list, uint32_t* ranges, uint32_t* n_contrib, float* accum_alpha, int* radii,
                   float* out_color, float* out_depth) {
    Handle* h = static_cast<Handle*>(handle);
    if (!h) return hipErrorInvalidValue;
    return guarded([&] {
        static_assert(sizeof(bool) == 1, "clamped is copied out as bytes");
        const size_t P = h->P, R = h->R, N = size_t(h->W) * h->H;
        const size_t tiles = size_t((h->W + 15) / 16) * ((h->H + 15) / 16);
        char *g = h->geom, *b = h->binning, *i = h->img;
        auto geom = CudaRasterizer::GeometryState::fromChunk(g, P);
        auto bin = CudaRasterizer::BinningState::fromChunk(b, R);
        auto img = CudaRasterizer::ImageState::fromChunk(i, N);
        download(depths, geom.depths, P);
        download(means2D, geom.means2D, P * 2);
        download(cov3D, geom.cov3D, P * 6);
        download(conic_opacity, geom.conic_opacity, P * 4);
        download(rgb, geom.rgb, P * 3);
        download(clamped, geom.clamped, P * 3);
        download(tiles_touched, geom.tiles_touched, P);
        download(point_offsets, geom.point_offsets, P);
        download(point_list_keys, bin.point_list_keys, R);
        download(point_list, bin.point_list, R);
        download(ranges, img.ranges, tiles * 2);
        download(n_contrib, img.n_contrib, N);
        download(accum_alpha, img.accum_alpha, N);
        download(radii, h->radii, P);
        download(out_color, h->out_color, 3 * N);
        download(out_depth, h->out_depth, N);
    });
}

// CudaRasterizer::Rasterizer::backward on the handle's state, gradients zero-initialised as RasterizeGaussiansBackwardCUDA
// does.  All ten outputs: [P,3] [P,4] [P,1] [P,3] [P,1] [P,3] [P,6] [P,M,3] [P,3] [P,4].
int ref_backward(void* handle, const float* dL_dpix, const float* dL_dpix_depth, float* dL_dmean2D, float* dL_dconic,
                 float* dL_dopacity, float* dL_dcolor, float* dL_ddepth, float* dL_dmean3D, float* dL_dcov3D, float* dL_dsh,
                 float* dL_dscale, float* dL_drot) {
    Handle* h = static_cast<Handle*>(handle);
    if (!h || !dL_dpix || !dL_dpix_depth) return hipErrorInvalidValue;
    return guarded([&] {
        Pool tmp;
        const size_t P = h->P, N = size_t(h->W) * h->H, M = h->M;
        float* dpix = tmp.upload(dL_dpix, 3 * N);
        float* ddep = tmp.upload(dL_dpix_depth, N);
        float *d_mean2D = tmp.zeros<float>(P * 3), *d_conic = tmp.zeros<float>(P * 4), *d_opacity = tmp.zeros<float>(P),
              *d_color = tmp.zeros<float>(P * 3), *d_depth = tmp.zeros<float>(P), *d_mean3D = tmp.zeros<float>(P * 3),
              *d_cov3D = tmp.zeros<float>(P * 6), *d_sh = tmp.zeros<float>(P * M * 3), *d_scale = tmp.zeros<float>(P * 3),
              *d_rot = tmp.zeros<float>(P * 4);
        CudaRasterizer::Rasterizer::backward(
            h->P, h->D, h->M, h->R, h->bg, h->W, h->H, h->means3D, h->shs, h->colors, h->scales, h->scale_modifier,
            h->rotations, h->cov3D_precomp, h->view, h->proj, h->campos, h->tan_fovx, h->tan_fovy, h->radii, h->geom,
            h->binning, h->img, dpix, ddep, d_mean2D, d_conic, d_opacity, d_color, d_depth, d_mean3D, d_cov3D, d_sh, d_scale,
            d_rot, /*debug=*/false);
        ck(hipDeviceSynchronize());
        download(dL_dmean2D, d_mean2D, P * 3);
        download(dL_dconic, d_conic, P * 4);
        download(dL_dopacity, d_opacity, P);
        download(dL_dcolor, d_color, P * 3);
        download(dL_ddepth, d_depth, P);
        download(dL_dmean3D, d_mean3D, P * 3);
        download(dL_dcov3D, d_cov3D, P * 6);
        download(dL_dsh, d_sh, P * M * 3);
        download(dL_dscale, d_scale, P * 3);
        download(dL_drot, d_rot, P * 4);
    });
}

int ref_free(void* handle) {
    delete static_cast<Handle*>(handle);
    return hipSuccess;
}

// CudaRasterizer::Rasterizer::markVisible; present[P] as bytes.
int ref_mark_visible(int P, const float* means3D, const float* viewmatrix, const float* projmatrix, uint8_t* present) {
    if (P <= 0) return hipErrorInvalidValue;
    return guarded([&] {
        static_assert(sizeof(bool) == 1, "present is copied out as bytes");
        Pool tmp;
        float* m = tmp.upload(means3D, size_t(P) * 3);
        float* v = tmp.upload(viewmatrix, 16);
        float* p = tmp.upload(projmatrix, 16);
        bool* out = tmp.zeros<bool>(P);
        CudaRasterizer::Rasterizer::markVisible(P, m, v, p, out);
        ck(hipDeviceSynchronize());
        download(present, out, size_t(P));
    });
}

// SimpleKNN::knn as distCUDA2 calls it: mean squared distance to the three nearest neighbours, zero-initialised output.
int ref_knn(int P, const float* points, float* mean_dists) {
    if (P <= 0) return hipErrorInvalidValue;
    return guarded([&] {
        Pool tmp;
        float* pts = tmp.upload(points, size_t(P) * 3);
        float* out = tmp.zeros<float>(P);
        SimpleKNN::knn(P, reinterpret_cast<float3*>(pts), out);
        ck(hipDeviceSynchronize());
        download(mean_dists, out, size_t(P));
    });
}

}  // extern "C"
