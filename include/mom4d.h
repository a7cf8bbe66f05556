/*
 * mom4d.h -- C ABI of libmom4d.so, the MI355X (gfx950) hot path of the 4D Gaussian
 * Splatting train/render loop of cvsp-lab/ICLR2025_3D-MOM.
 *
 * Every entry point takes plain device pointers and sizes plus a hipStream_t
 * (passed as void*), is stream-ordered on that stream, never allocates, never
 * synchronises the host unless its comment says so, and returns 0 on success
 * or a negative MOM_E* code (it never throws across the ABI).
 *
 * Reference interfaces replaced (paths relative to the reference tree):
 *   CudaRasterizer::Rasterizer::forward / backward / markVisible
 *       submodules/depth-diff-gaussian-rasterization/cuda_rasterizer/rasterizer.h:19-87
 *       (implementation rasterizer_impl.cu:141-153,198-444)
 *   RasterizeGaussiansCUDA / RasterizeGaussiansBackwardCUDA / markVisible (torch glue)
 *       submodules/depth-diff-gaussian-rasterization/rasterize_points.h:18-68
 *   distCUDA2 / SimpleKNN::knn
 *       submodules/simple-knn/spatial.h, simple_knn.h  (simple_knn.cu:185-221)
 * and, one level up (torch ops the reference issues from Python):
 *   deform_network.forward           scene/deformation.py:190-223 + scene/hexplane.py:160-183
 *   torch.optim.Adam.step            scene/gaussian_model.py:209, train_4DGS.py:295-297
 *   l1_loss / ssim                   utils/loss_utils.py:23-24,52-92
 *   compute_regulation               scene/gaussian_model.py:730-769
 *   boolean-mask row compaction      scene/gaussian_model.py:424-459
 *   the scene-flow fit (SGD loop)    train_motion.py:125-207
 */
#ifndef MOM4D_H_INCLUDED
#define MOM4D_H_INCLUDED

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MOM_OK 0
#define MOM_EINVAL (-1)   /* bad argument (shape, null pointer, unsupported channel count) */
#define MOM_ELAUNCH (-2)  /* a HIP launch / runtime call failed (hipGetLastError) */
#define MOM_ECAPACITY (-3)/* scratch buffer too small */
#define MOM_EUNAVAILABLE (-4) /* an optional run-time dependency is missing (librccl for mom_comm_*): mom_comm_last_error() says which */

#define MOM_TILE 16       /* config.h:14-16 BLOCK_X == BLOCK_Y == 16 */

typedef void* mom_stream_t; /* hipStream_t */

/* ---- ABI versioning ------------------------------------------------------------------------
 * The argument structs below have grown between releases.  A binder built against an older header must not be able to
 * pass a short struct silently, so:
 *   - mom_abi_version() returns MOM_ABI_VERSION of the library that is loaded; a binder compares it with the value of
 *     the header (or Python mirror) it was written against and refuses to continue on a mismatch;
 *   - mom_abi_sizeof(which) returns sizeof of each argument struct as the library was compiled, so a foreign-language
 *     mirror (ctypes, cffi) can verify its own layout field for field at load time;
 *   - MomRasterArgs, the struct that changes most often, additionally starts with `struct_size`: every entry point that
 *     takes it returns MOM_EINVAL unless struct_size == sizeof(MomRasterArgs) of the library.
 * (The reference's counterpart is a C++ static-method signature, rasterizer.h:19-87: there the compiler checks it.) */
#define MOM_ABI_VERSION 8
/* floats per Gaussian of the compositing backward's accumulator record (mom_raster_layout().geom_gacc); ten are used.  (A build with
 * -DMOM_GACC_FLOATS=16 pads the record to one 64-byte line: a device-scope atomic costs the device by the LINES an instruction
 * touches and 48-byte records straddle 1.5 on average -- but the shipped kernel's atomics hide under its arithmetic, and the larger
 * record measured 3 us SLOWER in render_bwd and 5 us per step, three alternating pairs in one call: DESIGN.md section 3.1.) */
#ifndef MOM_GACC_FLOATS
#define MOM_GACC_FLOATS 12
#endif
int mom_abi_version(void);
enum {
    MOM_STRUCT_RASTER_ARGS = 0, MOM_STRUCT_RASTER_GRADS, MOM_STRUCT_RASTER_LAYOUT, MOM_STRUCT_HEXPLANE, MOM_STRUCT_ADAM_TENSOR,
    MOM_STRUCT_ROW_SELECT, MOM_STRUCT_REG_PLANE, MOM_STRUCT_DEFORM_MLP, MOM_STRUCT_RASTER_ACCUM, MOM_STRUCT_COUNT
};
size_t mom_abi_sizeof(int which);   /* 0 for an unknown id */

/* Arguments of one rasterizer call; the field meanings are those of
 * CudaRasterizer::Rasterizer::forward (rasterizer.h:29-55).  Null pointers stand
 * for "absent" exactly as empty tensors do in the reference (forward.cu:205,241).
 * Matrices are the transposed (column-major) 4x4s the reference passes. */
typedef struct MomRasterArgs {
    uint32_t struct_size;  /* = sizeof(MomRasterArgs) of the header the caller was built against; anything else: MOM_EINVAL */
    int P;                 /* number of Gaussians */
    int D;                 /* active SH degree (0..3) */
    int M;                 /* SH coefficients per Gaussian in `shs` (0 if absent) */
    int W, H;              /* image size in pixels */
    const float* background;     /* [3] */
    const float* means3D;        /* [P,3] */
    const float* shs;            /* [P,M,3] or null; if shs_rest != null: the DC coefficient only, [P,1,3] */
    const float* shs_rest;       /* null, or [P,M-1,3]: coefficients 1..M-1 stored apart (GaussianModel keeps
                                    _features_dc and _features_rest as two tensors; this avoids the torch.cat of
                                    get_features, scene/gaussian_model.py:137-140) */
    const float* colors_precomp; /* [P,3] or null */
    const float* opacities;      /* [P] (already activated) */
    const float* scales;         /* [P,3] or null */
    const float* rotations;      /* [P,4] (r,x,y,z), used as given, or null */
    const float* cov3D_precomp;  /* [P,6] or null */
    const float* viewmatrix;     /* [16] */
    const float* projmatrix;     /* [16] */
    const float* campos;         /* [3] */
    float scale_modifier;
    float tan_fovx, tan_fovy;
    int prefiltered;
    int debug;             /* !=0: hipStreamSynchronize + error check after every kernel (CHECK_CUDA, auxiliary.h:166-173) */
    /* Tile-row shard (one image split over several GPUs; the reference has no counterpart): bin, composite and
     * back-propagate only the 16-pixel tile rows [tile_row0, tile_row1).  0,0 = every row.  Projection is
     * unaffected (radii, depths, conics are those of the whole image); num_rendered counts the local instances;
     * pixels of other rows are neither read nor written. */
    int tile_row0, tile_row1;
    /* !=0: this forward will never be followed by a backward (no-grad render(), render_4DGS.py): the auxiliary state only the
     * backward reads -- cov3D[P][6], clamped[P], final_T[H*W], n_contrib[H*W] -- is not written (about 28 B per Gaussian and
     * 8 B per pixel).  mom_raster_backward on such a forward is an error the caller must not make. */
    int forward_only;
    /* What mom_raster_forward_render leaves in *status_dev when this call's binning overflows (0 = 1): a caller that runs
     * ahead of the GPU numbers its calls here and later reads WHICH call overflowed first. */
    uint32_t overflow_tag;
    /* 0 (default): a (splat, tile) instance is binned only if the splat can reach alpha >= 1/255 at some pixel of the tile --
     * a conservative bound on the compositing kernels' own per-pixel test (forward.cu:331-338 skips such pairs one pixel at a
     * time), so colour, depth and every gradient are bit-identical to binning the whole rectangle, while num_rendered, the
     * tile lists and n_contrib (positions in those lists) shrink: about 40 % of the instances at 960x540 / 200k.
     * !=0: every tile of the splat's rectangle is binned, as duplicateWithKeys does (rasterizer_impl.cu:70-111): num_rendered
     * and the lists are then the reference's, bit for bit.  The same value must be given to every stage of one frame. */
    int keep_all_tiles;
    /* Optional loss epilogue of the forward (train_4DGS.py:218 `Ll1 = l1_loss(image, gt_image)`): with l1_target [3,H,W] set,
     * mom_raster_forward_render also leaves l1_grad [3,H,W] = sign(image - target) / (3 H W) and ADDS sum |image - target| and
     * sum (image - target)^2 to l1_sums[0], [1] -- what mom_l1_loss_acc(3 H W, out_color, target, l1_grad, l1_sums) computes from
     * the stored image, without its launch and its re-read of the image.  All three null: no epilogue. */
    const float* l1_target;
    float* l1_grad;
    float* l1_sums;
    /* !=0: the caller has already cleared the backward's per-Gaussian accumulator record in the geometry scratch
     * (mom_raster_layout().geom_gacc, MOM_GACC_FLOATS floats = 48 bytes per Gaussian) since the last backward read it; mom_raster_backward /
     * _backward_render then skip their own fill command.  (The reference zeroes its ten gradient tensors in
     * RasterizeGaussiansBackwardCUDA, rasterize_points.cu:154-163; the fused training step does this fill on its second stream
     * during the forward.) */
    int accum_cleared;
    /* null, or [tiles of the whole image][2] floats (with l1_target set): every workgroup of the compositing forward then STORES its tile's
     * two sums at entry 2 * (ty * tiles_x + tx) instead of adding them to l1_sums (which may be null): 2040 workgroups adding into one
     * 64-byte line are serialised by the device (about 8 ns each; 6 us at the tail of the launch at 960x540), and nobody may ever read the
     * value.  Whoever wants it adds the entries up -- in a fixed order, so the loss value is reproducible to the bit, which the
     * atomic sums are not.  A tile-row shard writes the entries of its own rows only. */
    float* l1_partials;
    /* null, or one 64-bit word in PINNED HOST memory: the compositing forward then leaves (status_serial << 32) | status there with a
     * system-scope store -- status = this frame's status bits (bit 0: its binning overflowed `capacity`, the image is incomplete), as
     * of the end of the frame's binning.  A host that runs ahead of the device reads the frame's fate from the word once its upper half
     * equals the serial it gave, instead of copying the status back behind an event after every frame (a blit kernel and a marker: 12 us of
     * the stream per frame, 15 us of host time per call of the drop-in's async mode). */
    unsigned long long* status_post;
    uint32_t status_serial;
    /* 0 (= 1), or a factor on the L1 epilogue's gradient: l1_grad = sign(image - target) * ((1 / (3 H W)) * l1_grad_scale).  A camera-batch
     * shard's loss is the mean over the ranks' cameras (train_4DGS.py:189-229), so every rank's gradient image carries 1 / world: with
     * the factor here there is no scaling pass over the gradient image behind the forward.  The sums are not scaled. */
    float l1_grad_scale;
    /* !=0: scales, rotations and opacities hold the model's RAW parameters (_scaling, _rotation, _opacity) and the projection applies
     * render()'s activations itself, in registers -- exp, normalize, sigmoid (gaussian_renderer/__init__.py:130-132 of the coarse
     * stage, scene/gaussian_model.py:60-75): radii, rectangles, depth keys, conics, colours and the image are bit-identical to
     * mom_activations_forward followed by a call without the flag, and no activated copies exist in memory.  The backward (same args)
     * then writes dL_dscales / dL_drotations / dL_dopacity w.r.t. the raw values, as act_rotations_raw does.  Requires scales and
     * rotations; refused (MOM_EINVAL) with cov3D_precomp, and in the backward together with act_rotations_raw. */
    int params_raw;
} MomRasterArgs;

/* Scratch sizing (bytes).  The three buffers play the roles of the reference's
 * geomBuffer / binningBuffer / imgBuffer (rasterize_points.cu:72-78) and are
 * handed back to the backward pass unchanged.  Their internal layout is
 * private; mom_raster_layout exposes it for tests. */
size_t mom_raster_geom_bytes(int P);
size_t mom_raster_image_bytes(int W, int H);
size_t mom_raster_binning_bytes(int P, int W, int H, size_t capacity /* max instances */);

/* Forward, stage 1: per-Gaussian projection (preprocessCUDA, forward.cu:156-256),
 * per-tile instance histogram and its scan.  Writes radii[P] (int32), the tile
 * ranges and *num_rendered_dev (uint32, device).  If num_rendered_host is not
 * null it must be host memory (pinned recommended) and receives the same value by
 * an async copy on `stream` (the caller synchronises if it wants to read it; this
 * replaces the blocking cudaMemcpy at rasterizer_impl.cu:282). */
int mom_raster_forward_geometry(const MomRasterArgs* a, void* geom, void* image, int* radii,
                                uint32_t* num_rendered_dev, uint32_t* num_rendered_host, mom_stream_t stream);

/* Forward, stage 2: scatter instances into their tiles, per-tile depth sort
 * (with keep_all_tiles: result identical to the reference's global sort of (tile<<32|depth) keys,
 * rasterizer_impl.cu:70-111,301-318; by default: the same lists less the instances that cannot contribute) and alpha compositing (renderCUDA,
 * forward.cu:261-379).  `capacity` is the instance capacity the binning buffer
 * was sized for; if the true count exceeds it nothing beyond capacity is written, the image
 * is incomplete, and if *status_dev (may be null) is still 0 it receives a->overflow_tag (1
 * when that is 0).  The word is STICKY: the call never clears it, the caller zeroes it (before
 * the first call, and after it has dealt with an overflow), so a host that reads it late cannot
 * miss an overflow and learns which call overflowed first.
 * out_color [3,H,W], out_depth [1,H,W]. */
int mom_raster_forward_render(const MomRasterArgs* a, void* geom, void* binning, size_t capacity, void* image,
                              float* out_color, float* out_depth, uint32_t* status_dev, mom_stream_t stream);

/* Gradients of one backward call (RasterizeGaussiansBackwardCUDA,
 * rasterize_points.cu:154-163,202).  All are fully written by the call (zeros
 * for Gaussians with radius 0), so they need no prior memset. */
typedef struct MomRasterGrads {
    float* dL_dmeans2D;   /* [P,3] (x,y in NDC-scaled pixels; z = 0) */
    float* dL_dcolors;    /* [P,3] */
    float* dL_dopacity;   /* [P,1] */
    float* dL_dmeans3D;   /* [P,3] */
    float* dL_dcov3D;     /* [P,6] */
    float* dL_dsh;        /* [P,M,3] or null when M == 0; with dL_dsh_rest != null: the DC part only, [P,1,3] */
    float* dL_dsh_rest;   /* null, or [P,M-1,3] */
    float* dL_dscales;    /* [P,3] or null when scales absent */
    float* dL_drotations; /* [P,4] or null when rotations absent */
    /* Optional (null: off).  The RAW rotations [P,4] the caller normalised into MomRasterArgs.rotations, for callers whose scales /
     * rotations / opacities are exp / normalize / sigmoid of raw parameters (gaussian_renderer/__init__.py:134-137): dL_dscales,
     * dL_drotations and dL_dopacity are then written THROUGH those activations (w.r.t. the raw values), exactly as
     * mom_activations_backward would make them from the plain gradients, without its launch and its pass over the arrays. */
    const float* act_rotations_raw;
    /* Optional second destinations of dL_dscales / dL_drotations (same values): a caller that reduces those two over ranks in place
     * while another kernel still reads its own copy (the camera-batch shard's deformation backward) gets the copies from the kernel
     * that makes the values, not from two copy launches behind it. */
    float* dL_dscales_copy;
    float* dL_drotations_copy;
    /* Optional densification statistics epilogue (all three null: off; given in part: MOM_EINVAL).  The projection backward holds every
     * Gaussian's radius and dL/d mean2D in registers and performs the update of mom_densify_stats on these [P] accumulators in place
     * (train_4DGS.py:266, scene/gaussian_model.py:713-715 add_densification_stats): for radii[i] > 0, max_radii2D = max(., radius),
     * xyz_gradient_accum += |dL_dmeans2D[i, :2]|, denom += 1 -- the same bits as that function on the written dL_dmeans2D, without its
     * launch and its pass.  stats_skip_if_nonzero (device word, may be null; only with the accumulators) as in mom_adam_step. */
    float* stats_max_radii2D;
    float* stats_grad_accum;
    float* stats_denom;
    const uint32_t* stats_skip_if_nonzero;
} MomRasterGrads;

/* Backward (Rasterizer::backward, rasterizer_impl.cu:343-444): render backward
 * (backward.cu:415-590), cov2D backward (:144-274), preprocess backward (:346-412).
 * dL_dout_color [3,H,W]; dL_dout_depth [1,H,W] or null (treated as zeros).
 * `capacity` is the value given to mom_raster_forward_render, or any smaller value that is still >= the forward's num_rendered
 * (the tile lists sit at the start of the binning buffer whatever it was sized for).  dL_dscales /
 * dL_drotations are written only when scales/rotations are present. */
int mom_raster_backward(const MomRasterArgs* a, const int* radii, void* geom, void* binning, size_t capacity,
                        void* image, const float* dL_dout_color, const float* dL_dout_depth,
                        const MomRasterGrads* g, mom_stream_t stream);

/* The two halves of mom_raster_backward, for callers that must exchange between them (tile-row shard):
 * _render runs the compositing backward over this rank's tile rows and leaves, in the geometry scratch at
 * mom_raster_layout().geom_gacc, one record of MOM_GACC_FLOATS floats per Gaussian (ten used): the sums over the local pixels of the raw terms of
 * dL/d{mean2D.x, mean2D.y (before the Gaussian's conic matrix and the pixel-to-NDC factors are applied), conic.x, conic.y, conic.z
 * (before their -1/2), opacity, r, g, b, depth} and two zeros.  The
 * projection backward is linear in that record, so ranks sum it (an all-reduce of 48 bytes per Gaussian) and
 * then each runs _geometry, which yields identical parameter gradients everywhere. */
int mom_raster_backward_render(const MomRasterArgs* a, void* geom, void* binning, size_t capacity, void* image,
                               const float* dL_dout_color, const float* dL_dout_depth, mom_stream_t stream);
int mom_raster_backward_geometry(const MomRasterArgs* a, const int* radii, void* geom, const MomRasterGrads* grads,
                                 mom_stream_t stream);

/* A batch of cameras on one GPU (train_4DGS.py:172-229: every camera of opt.batch_size is rendered, ONE loss is taken over the
 * [B,3,H,W] stack, backward() runs once, so a parameter's gradient is the SUM over the cameras; :203-204,227-229 merge the radii with
 * max and the screen-space gradients with a sum).  The first camera's backward is mom_raster_backward: it stores.  Every later camera's
 * is the _acc form, which ADDS into the same MomRasterGrads: dL_dmeans2D, dL_dmeans3D, dL_dsh / dL_dsh_rest, dL_dscales, dL_drotations
 * and dL_dopacity become old + value -- one fp32 add of exactly the value the store form writes -- for the Gaussians with radius > 0
 * in THIS camera; a Gaussian with radius 0 here has none of them written.  dL_dcolors, dL_dcov3D, dL_dscales_copy and
 * dL_drotations_copy stay per-call outputs, fully written.  The statistics epilogue (stats_*) then performs mom_densify_stats' update
 * on the MERGED radius max(radii_max[i], radii[i]) and the accumulated dL_dmeans2D: given to the LAST camera's call it is the
 * once-per-step update of train_4DGS.py:266. */
typedef struct MomRasterAccum {
    uint32_t struct_size;    /* = sizeof(MomRasterAccum); anything else: MOM_EINVAL */
    /* null, or [P,3]: this call's own dL_dmeans3D (zeros for radius 0), plain stores -- what a deformation backward of THIS camera
     * reads while dL_dmeans3D holds the running sum (gaussian_renderer/__init__.py:96-99: pts = xyz + dx depends on the camera's time) */
    float* dL_dmeans3D_copy;
    /* null, or [P]: radii_max[i] = max(radii_max[i], radii[i]) (train_4DGS.py:203 `radii = torch.cat(radii_list, 0).max(dim=0).values`);
     * `radii`, the camera's own, stays what the backward reads.  Must not alias `radii`. */
    int* radii_max;
} MomRasterAccum;
/* mom_raster_backward / mom_raster_backward_geometry with the accumulating projection backward.  MOM_EINVAL, before anything is
 * launched: accum null or of another struct_size, a tile-row shard (a->tile_row0 / tile_row1 set: a shard of a batch is not
 * supported), and everything the store forms refuse (act_rotations_raw with params_raw, statistics pointers given in part, ...). */
int mom_raster_backward_acc(const MomRasterArgs* a, const int* radii, void* geom, void* binning, size_t capacity,
                            void* image, const float* dL_dout_color, const float* dL_dout_depth,
                            const MomRasterGrads* g, const MomRasterAccum* accum, mom_stream_t stream);
int mom_raster_backward_geometry_acc(const MomRasterArgs* a, const int* radii, void* geom, const MomRasterGrads* grads,
                                     const MomRasterAccum* accum, mom_stream_t stream);

/* ---- ordered backward reduction: gradients that are a function of their inputs, bit for bit ----------------------------------
 * mom_raster_backward_render adds every (wave, list entry) total into the per-Gaussian record with float atomics, in whatever
 * order the waves arrive: two runs differ by about 1e-6 relative.  The _ordered forms store those totals instead and add them up
 * in a defined order; everything else of the backward is per-Gaussian arithmetic already.
 *
 * SLOTS.  A Gaussian g with radius > 0 owns one slot per tile of its rectangle [x0,x1) x [y0,y1) (getRect, auxiliary.h:46-56, as the
 * projection computed it: tiles_touched of them), row-major, y outer: slot(g, tx, ty) = slot_base[g] + (ty - y0) (x1 - x0) + (tx - x0),
 * with slot_base the exclusive scan of tiles_touched over the Gaussians.  slot_base[P] is the reference's num_rendered whether or
 * not keep_all_tiles is set: binning and the tile lists are not involved.
 * PARTIALS.  partials[slot][wave 0..3][MOM_ORDERED_VALUES] floats (MOM_ORDERED_SLOT_BYTES = 160 bytes per slot), wave = the 8x8 pixel
 * block of the tile (0: left top, 1: right top, 2: left bottom, 3: right bottom), value k = float k of the accumulator record
 * (value 9, depth, stays +0.0 without a depth gradient).  The buffer is cleared to +0.0 by the call; a (slot, wave) nothing is
 * stored into stays +0.0: an instance the default binning culled, a wave the splat cannot reach, entries behind the last contributor.
 * ORDER.  For value k of a Gaussian with n slots:   t[s] = (p[s][0][k] + p[s][1][k]) + (p[s][2][k] + p[s][3][k]);
 *   a[r] = (...((+0.0 + t[r]) + t[r+4]) + t[r+8] ...) over s = r, r+4, ... < n, for r = 0..3 (a[r] = +0.0 when r >= n);
 *   record[k] = (a[0] + a[2]) + (a[1] + a[3]);   record[10], [11] = 0;   n = 0 (radius 0): zeros.
 * It depends on n alone -- not on the grid, the workgroup count or which lanes are active.  mom_raster_ordered_sum_host reproduces it
 * on the host (plain C++, compiled without FMA contraction) from a copy of slot_base and partials. */
#define MOM_ORDERED_VALUES 10
#define MOM_ORDERED_SLOT_BYTES 160
/* status bits of the ordered forms (OR-ed into *status_dev, which the caller zeroes): a computed slot lay outside the Gaussian's
 * rectangle or at/after `slots` and was skipped, never stored (a plan of another frame); the reduction cut a Gaussian's slots at `slots` */
#define MOM_ORDERED_BAD_SLOT 1
#define MOM_ORDERED_CUT 2
/* bytes of the plan buffer (slot_base[P+1] uint32 at its 256-byte aligned start, then the scan's block sums) and of the partials */
size_t mom_raster_ordered_plan_bytes(int P);
size_t mom_raster_ordered_bytes(int P, size_t slots);       /* 0: slots is not a count the ordered forms take (>= 2^32 - 1) */
/* Scans tiles_touched of the geometry scratch a forward of `a` left (two launches) into slot_base[P+1]; the total goes to *total_dev
 * (uint32, may be null) and, if total_host is not null (pinned host memory), there too by a system-scope store on `stream`.  A total of
 * 2^32 - 1 or more is reported as 2^32 - 1, which mom_raster_ordered_bytes and the backward refuse. */
int mom_raster_ordered_plan(const MomRasterArgs* a, void* geom, void* plan, uint32_t* total_dev, uint32_t* total_host,
                            mom_stream_t stream);
/* mom_raster_backward_render with the ordered reduction: clears partials, composites, reduces into the accumulator record; followed by
 * the unchanged mom_raster_backward_geometry.  `plan` as mom_raster_ordered_plan left it for THIS forward, `slots` its total,
 * partials / partials_bytes a buffer of at least mom_raster_ordered_bytes(P, slots).  MOM_EINVAL before anything is launched: plan,
 * partials or status_dev null, partials_bytes too small, slots >= 2^32 - 1, a forward_only frame, a tile-row shard (tile_row0 / tile_row1 set). */
int mom_raster_backward_render_ordered(const MomRasterArgs* a, void* geom, void* binning, size_t capacity, void* image,
                                       const float* dL_dout_color, const float* dL_dout_depth, const void* plan, void* partials,
                                       size_t partials_bytes, size_t slots, uint32_t* status_dev, mom_stream_t stream);
/* The two halves together, mirroring mom_raster_backward. */
int mom_raster_backward_ordered(const MomRasterArgs* a, const int* radii, void* geom, void* binning, size_t capacity, void* image,
                                const float* dL_dout_color, const float* dL_dout_depth, const MomRasterGrads* g, const void* plan,
                                void* partials, size_t partials_bytes, size_t slots, uint32_t* status_dev, mom_stream_t stream);
/* A camera batch's accumulating backward has no ordered form (its sum over cameras is a separate question): always MOM_EINVAL. */
int mom_raster_backward_ordered_acc(const MomRasterArgs* a, const int* radii, void* geom, void* binning, size_t capacity, void* image,
                                    const float* dL_dout_color, const float* dL_dout_depth, const MomRasterGrads* g,
                                    const MomRasterAccum* accum, const void* plan, void* partials, size_t partials_bytes, size_t slots,
                                    uint32_t* status_dev, mom_stream_t stream);
/* The reduction on the host (no GPU needed): slot_base [P+1], partials [slot_base[P]][4][MOM_ORDERED_VALUES] -> gacc [P][MOM_GACC_FLOATS]. */
int mom_raster_ordered_sum_host(int P, const uint32_t* slot_base, const float* partials, float* gacc);

/* checkFrustum (rasterizer_impl.cu:54-66): present[i] = p_view.z > 0.2 */
int mom_mark_visible(int P, const float* means3D, const float* viewmatrix, const float* projmatrix,
                     uint8_t* present, mom_stream_t stream);

/* Layout of the private scratch buffers, for tests: byte offsets of the named
 * arrays.  geom: rec[P][12] float = {x, y, depth, tiles_touched(bits) | conic.x,
 * conic.y, conic.z, opacity | r, g, b, radius(bits)}; cov3D[P][6]; clamped[P][4] u8.
 * image: ranges[tiles][2] u32, n_contrib[H*W] u32, final_T[H*W] f32, tile_counts[tiles] u32
 * (the per-tile histogram, bucket cursors and a small header also live here so that the
 * binning buffer can be sized AFTER the instance count is known).
 * binning: point_list[capacity] u32 at offset 0 (all the backward reads of this buffer: a backward may therefore be given
 * any capacity between the true instance count and the forward's), then keys[capacity] u64 (depth_bits<<32|idx, bucketed by tile). */
typedef struct MomRasterLayout {
    size_t geom_rec, geom_cov3D, geom_clamped, geom_gacc;
    size_t img_ranges, img_n_contrib, img_final_T, img_tile_counts;
    size_t bin_keys, bin_point_list;
    size_t img_tile_walked;   /* u32 per tile, valid after mom_raster_forward_render: list entries the tile's workgroup walked before
                               * every pixel was done, in rounds of 256 like forward.cu:305-327 (Q = 256 x their sum) */
} MomRasterLayout;
int mom_raster_layout(int P, int W, int H, size_t capacity, MomRasterLayout* out);

/* distCUDA2 (simple-knn/spatial.cu:15-25): mean squared distance to the 3 nearest
 * neighbours.  scratch must hold mom_knn_scratch_bytes(P).  Fully stream-ordered (the
 * reference does two blocking copies of the bounding box, simple_knn.cu:197,200). */
size_t mom_knn_scratch_bytes(int P);
int mom_knn_mean_dist2(int P, const float* points /* [P,3] */, float* mean_dist2 /* [P] */, void* scratch,
                       mom_stream_t stream);

/* ---- HexPlane feature field --------------------------------------------------------------
 * Replaces HexPlaneField.forward (scene/hexplane.py:160-183: normalize_aabb, 6 bilinear
 * grid_sample(align_corners=True, padding_mode='border') per level, product over planes,
 * concat over levels) and its autograd backward (plane scatter-adds + the gradient wrt the
 * sample positions).  Planes are CHANNEL-LAST: planes[l][p] points to [H][W][32] floats where,
 * for plane p = (a,b) in the order (0,1),(0,2),(0,3),(1,2),(1,3),(2,3) of (x,y,z,t),
 * W = res[l][a] and H = res[l][b].  aabb = the reference's 2x3 `aabb` parameter verbatim
 * (row 0 then row 1; the reference stores xyz_max in row 0, hexplane.py:152-157).  `time` is
 * the raw timestamp used as the 4th grid coordinate (gaussian_renderer/__init__.py:56). */
typedef struct MomHexPlane {
    int levels;            /* 1..4 */
    int channels;          /* 32 or 16 (every plane of the field) */
    int res[4][4];         /* per level: resolution along x, y, z, t */
    const float* planes[4][6];
    float* grads[4][6];    /* backward only: same layout as planes, ACCUMULATED into (+=, float atomics) */
    float aabb[6];
} MomHexPlane;
/* Planes are channel-last, [H][W][channels] floats.  feat [P, levels*channels] row-major, level-major within a row.  times:
 * optional per-point timestamps [P]; null -> `time` for all points (render() uses one timestamp per camera).  channels must be
 * 32 or 16 (MOM_EINVAL otherwise): 32 lanes own one (point, level) at 32 channels, 16 lanes at 16 (one template over the channel count, csrc/hexplane.hip). */
int mom_hexplane_forward(const MomHexPlane* hp, int P, const float* xyz, const float* times, float time,
                         const uint32_t* order, float* feat, mom_stream_t stream);
/* dfeat [P, levels*channels]; plane gradients accumulate into hp->grads; dxyz [P,3] (may be null) is ACCUMULATED into.
 * plane_order / plane_inverse ([3][levels][P] each, from mom_hexplane_orders) and scratch (mom_hexplane_backward_scratch_bytes)
 * select the two-pass path (times == null only): pass 1 gathers in `order` and stores each space plane's per-point gradient
 * row at the point's position in that plane's order, pass 2 walks each space plane in its order and turns runs of points of
 * one texel cell into one row of float atomics.  Any of the three null: the generic path (24 atomic rows per point and level).
 * Both paths exist for 32 and for 16 channels; the scratch size follows the channel count (six rows of `channels` floats per
 * point and level). */
size_t mom_hexplane_backward_scratch_bytes(const MomHexPlane* hp, int P);
int mom_hexplane_backward(const MomHexPlane* hp, int P, const float* xyz, const float* times, float time,
                          const uint32_t* order, const float* dfeat, float* dxyz, const uint32_t* plane_order,
                          const uint32_t* plane_inverse, void* scratch, mom_stream_t stream);
/* The same (two-pass path, one timestamp) for a caller that ran mom_deform_field_forward on this field at this `time` just
 * before: field_scratch is that call's scratch, whose head still holds the frame's time lines (the three space-time planes
 * interpolated at `time`), so they are not computed again.  The caller guarantees that neither the planes nor the scratch
 * changed in between (the fused training step: forward and backward of one camera).  Reference: as mom_hexplane_backward. */
int mom_hexplane_backward_lines(const MomHexPlane* hp, int P, const float* xyz, float time, const uint32_t* order,
                                const float* dfeat, float* dxyz, const uint32_t* plane_order, const uint32_t* plane_inverse,
                                void* scratch, const void* field_scratch, mom_stream_t stream);
/* Per-plane processing orders for the two-pass backward: for each space plane (x,y), (x,z), (y,z) and each level the
 * permutation of 0..P-1 that sorts the points by the texel cell of that level they fall into (2-D Morton order over the
 * cells), and its inverse.  Like `order`, they never change a result; they may be reused while the points drift (refresh
 * every few dozen iterations) and must be rebuilt when P changes. */
size_t mom_hexplane_orders_scratch_bytes(int P);
int mom_hexplane_orders(const MomHexPlane* hp, int P, const float* xyz, uint32_t* order /* [3][levels][P] */,
                        uint32_t* inverse /* [3][levels][P] */, void* scratch, mom_stream_t stream);
/* `order` (both calls, may be null = identity): a permutation of 0..P-1 giving the order in which points are
 * processed, e.g. mom_morton_order(xyz).  It never changes a result (float atomics aside); walking the points in a
 * spatially sorted order lets the backward sum consecutive points that hit the same texel in registers and issue one
 * atomic row for the run. */
size_t mom_morton_order_scratch_bytes(int P);
int mom_morton_order(int P, const float* points /* [P,3] */, uint32_t* order /* [P] */, void* scratch, mom_stream_t stream);

/* ---- ordered HexPlane backward: plane and position gradients that are a function of their inputs, bit for bit ------------------
 * mom_hexplane_backward adds into the plane gradients with float atomics, in whatever order the waves arrive, and the levels add
 * into one dxyz slot the same way.  The ordered form is a PULL: a texel's gradient is computed by the texel's owner from the points
 * of the four cells around it, with no float atomic anywhere (csrc/hexplane_ordered.hip).  One shared timestamp only (per-point
 * timestamps have no ordered form: the entry takes none); 32 or 16 channels, 1..4 levels.  The call is self-contained and
 * stream-ordered: it sorts the points of every (level, plane) by the cell of their CURRENT position itself and takes no plane
 * orders.  `order` (may be null) is the gather's processing order as in mom_hexplane_backward; no result depends on it.
 *
 * TERMS.  Per (point g, level l): the six samples and gv(g,l,p,c) = dfeat * (product of the other five), formed as
 * (dfeat * pre[p]) * suf[p+1] like the generic backward, in uncontracted fp32; the level's share of the position gradient is
 * reduced over the channels by the gathers' xor butterflies.  A point lies in cell (y0, x0) of plane p (W along its first axis):
 * x0 = floor of the clipped unnormalised coordinate exactly as the plane-order keys form it; for a space-time plane y0 is the cell
 * of the shared timestamp.  Its corner weights w00 (nw), w01 (ne), w10 (sw), w11 (se) are ATen's, (x1 - ix) (y1 - iy) etc.
 * ORDER.  Texel (y, x) of plane p, level l, channel c receives four classes:
 *   k = 0  nw: the points of cell (y, x),     weight w00        k = 1  ne: cell (y, x-1),   weight w01
 *   k = 2  sw: cell (y-1, x),                 weight w10        k = 3  se: cell (y-1, x-1), weight w11
 * (a cell outside the plane has no points; a corner outside the plane is no texel and receives nothing).  Within a class the cell's
 * n points are taken in ascending g; the term is e = gv * w, one fp32 multiply.  The terms are cut into blocks of 64 from the first:
 *   b_j = (...((+0.0 + e_64j) + e_64j+1) + ...)  left to right;      s_k = (...((+0.0 + b_0) + b_1) + ...)  left to right;
 *   T = (s_0 + s_1) + (s_2 + s_3)  (s_k = +0.0 for a class without terms);      grad = grad_in + T,
 * one add onto whatever the buffer held (the regulariser's gradient arrives there first).  A texel without a term in any class is not
 * written.  dxyz[g][k] = dxyz_in[g][k] + (((part_0 + part_1) + part_2) + part_3) over the levels there are, part_l the level's share.
 * The order is a function of the positions, the timestamp and the descriptor alone -- not of the grid, an environment switch, the
 * `order` argument or which wave arrives first.  mom_hexplane_ordered_sum_host reproduces it on the host (plain C++, no contraction).
 *
 * SCRATCH (mom_hexplane_ordered_scratch_bytes; 0 for a descriptor or P the call refuses).  From its 256-byte aligned start: the gv rows
 * [levels][6][P][channels] floats in POINT order, then at the next multiple of 256 bytes the position shares dxyz_part[levels][P][3]
 * (written when dxyz is given); behind them the sort buffers, per-point weights, per-cell segment and block tables and the block sums
 * of the plane being reduced.  Every byte the call reads it has written first.
 * LIMITS.  Cells and texels are indexed with int: W * H * (4 * channels) bytes must stay below 2^31 for each of the six planes of
 * each level (which keeps the cell key y0 W + x0 inside 32 bits), every resolution within 1 .. 65536; everything indexed by the
 * point is addressed with size_t, and P <= 2^30 keeps the point index (workgroup * 256 + thread) an int.  MOM_EINVAL before anything is
 * launched: hp null, channels other than 16 / 32, levels outside 1..4, P < 0 or above 2^30, a resolution or plane outside those limits; then P == 0 returns MOM_OK; then xyz, dfeat, scratch, a plane or a gradient
 * pointer null, scratch_bytes below mom_hexplane_ordered_scratch_bytes(hp, P).  dxyz may be null. */
size_t mom_hexplane_ordered_scratch_bytes(const MomHexPlane* hp, int P);
int mom_hexplane_backward_ordered(const MomHexPlane* hp, int P, const float* xyz, float time, const uint32_t* order,
                                  const float* dfeat, float* dxyz, void* scratch, size_t scratch_bytes, mom_stream_t stream);
/* The reduction on the host (no GPU needed).  hp: levels, channels, res, aabb as for the call and grads pointing at HOST buffers in
 * the planes' layout, added onto (planes are not read); xyz [P,3], gv and dxyz_part as the call leaves them in its scratch; dxyz
 * (may be null, with dxyz_part) is added onto. */
int mom_hexplane_ordered_sum_host(const MomHexPlane* hp, int P, const float* xyz, float time, const float* gv,
                                  const float* dxyz_part, float* dxyz);

/* ---- activations of render() (gaussian_renderer/__init__.py:130-132) and their backward, one launch each ----
 * scales = exp(scales_raw), rots = rots_raw / max(|rots_raw|, 1e-12) (F.normalize), opac = sigmoid(opac_raw) */
int mom_activations_forward(int P, const float* scales_raw, const float* rots_raw, const float* opac_raw, float* scales,
                            float* rots, float* opac, mom_stream_t stream);
/* in: activated values + raw rotations + gradients wrt the activated values; out: gradients wrt the raw values */
int mom_activations_backward(int P, const float* scales, const float* rots_raw, const float* opac, const float* dscales,
                             const float* drots, const float* dopac, float* dscales_raw, float* drots_raw, float* dopac_raw,
                             mom_stream_t stream);

/* ---- fused multi-tensor Adam (torch.optim.Adam, amsgrad=False, weight_decay=0) -----------
 * One launch updates every listed tensor: exp_avg.lerp_(g, 1-b1); exp_avg_sq = b2*v + (1-b2) g*g;
 * p -= lr/bc1 * exp_avg / (sqrt(exp_avg_sq)/sqrt(bc2) + eps), bc = 1 - beta^step computed by the
 * caller in double (as torch does).  Tensors are flat views of n floats in storage order; param,
 * grad and both moments of one tensor must share that order. */
#define MOM_ADAM_MAX_TENSORS 64
typedef struct MomAdamTensor {
    float* param;
    const float* grad;
    float* exp_avg;
    float* exp_avg_sq;
    size_t n;
    float lr;
    float bias_correction1;
    float bias_correction2_sqrt;
} MomAdamTensor;
/* skip_if_nonzero (device word, may be null): when it is nonzero at execution time the launch changes nothing.  The fused
 * training step points it at the rasterizer's sticky overflow word (mom_raster_forward_render), so that a step whose binning
 * buffer overflowed -- its image and gradients are truncated -- never reaches the parameters or the moments; the host, which
 * runs ahead of the GPU, finds the flag later and replays that iteration with a larger buffer. */
int mom_adam_step(const MomAdamTensor* tensors, int count, double beta1, double beta2, double eps,
                  const uint32_t* skip_if_nonzero, mom_stream_t stream);

/* ---- L1 loss + PSNR sums + gradient (utils/loss_utils.py:23-24, utils/image_utils.py:17-38) --
 * sums2[0] = sum |img-gt|, sums2[1] = sum (img-gt)^2 over n elements (zeroed by the call);
 * dimg (may be null) = sign(img-gt)/n = d mean|img-gt| / d img. */
int mom_l1_loss(size_t n, const float* img, const float* gt, float* dimg, float* sums2, mom_stream_t stream);
/* the same without zeroing sums2 first: for a caller that keeps them in memory it clears anyway */
int mom_l1_loss_acc(size_t n, const float* img, const float* gt, float* dimg, float* sums2, mom_stream_t stream);

/* ---- Row selection for densify / prune (scene/gaussian_model.py:409-482 _prune_optimizer, cat_tensors_to_optimizer,
 * prune_points; :511-581 densify_and_split, densify_and_clone, prune: `tensor[mask]` once per parameter, per Adam moment and
 * per auxiliary tensor, each with its own nonzero() and host synchronisation) ----
 * plan:  dst_index[i] (device, [n]) = position of row i among the rows with keep[i] != 0, or -1; *count_dev (device) and, if
 *        count_host != null (pinned host memory, copied on the stream), *count_host = the number of kept rows.
 * apply: for each of the `count` tensors, dst[dst_index[i]] = src[i] for the kept rows i; a row is row_bytes bytes (any size;
 *        4-byte words when size and alignment allow).  dst must hold *count rows. */
#define MOM_SELECT_MAX_TENSORS 32
typedef struct {
    const void* src;
    void* dst;
    unsigned row_bytes;
} MomRowSelect;
size_t mom_select_scratch_bytes(int n);
int mom_select_plan(int n, const uint8_t* keep, int* dst_index, int* count_dev, int* count_host, void* scratch,
                    mom_stream_t stream);
int mom_select_apply(int n, const int* dst_index, const MomRowSelect* tensors, int count, mom_stream_t stream);

/* ---- One-pass densify round (scene/gaussian_model.py:461-482 cat_tensors_to_optimizer, 484-509 densification_postfix,
 * 511-539 densify_and_split with its prune_points, 541-581 densify_and_clone / prune: clone, split and the removal of the split
 * parents, for every per-Gaussian tensor and both of its Adam moments) ----
 * With P rows, C rows to clone and S rows to split (the two masks are disjoint; K = P - S), the round leaves K + C + 2S rows:
 * the rows that are not split in order, then the clones in order, then child 0 of every split parent in order, then child 1.
 * plan:  kept_index[i] = position of row i among the rows that are not split, or -1; clone_rank[i] / split_rank[i] = rank of row
 *        i among the clones / the split parents, or -1 (device, [P] each); counts_dev (device) and, if non-null, counts_host
 *        (pinned host memory, copied on the stream) = {K, C, S}.  P == 0: MOM_OK, zero counts, counts_dev may be null.
 * apply: ONE launch for all `count` tensors.  `counts` is the plan's {K, C, S} ON THE HOST (the caller has waited for them: the
 *        outputs had to be allocated), dst holds K + C + 2S rows of row_bytes bytes, z is [2S,3] standard normals (null if S == 0).
 *        Per role:
 *          MOM_DENSIFY_COPY      every output row is its source row (16-byte or 4-byte words when size and alignment allow)
 *          MOM_DENSIFY_MOMENT    kept rows copy; clone and child rows are zero (an Adam moment: :461-482)
 *          MOM_DENSIFY_XYZ       [P,3] floats; kept and clone rows copy; child b of the j-th split parent i is
 *                                R(rotation_i) (z[b*S+j] * exp(scaling_i)) + xyz_i   (:517-524; R: utils/general_utils.py:84-105)
 *          MOM_DENSIFY_SCALING   [P,3] floats; kept and clone rows copy; child rows are log(exp(scaling_i) / (0.8*2))   (:525)
 *          MOM_DENSIFY_ROTATION  [P,4] floats; a copy, and the quaternions the xyz children read
 *          MOM_DENSIFY_ZERO      zero at the new length (the statistics, :505-508); src is not read
 *        The children are evaluated in torch's operation order, every element-wise operation rounded on its own.
 *        A tensor with row_bytes == 0 is skipped.  tensor_size = sizeof(MomDensifyTensor) of the caller's header.
 * MOM_EINVAL, before anything is launched: P < 0; a null index or counts pointer with P > 0; counts that are not a plan's
 * (K != P - S, C or S outside [0, P]); count outside [0, MOM_DENSIFY_MAX_TENSORS]; another tensor_size; an unknown role;
 * row_bytes > MOM_DENSIFY_MAX_ROW_BYTES; a tensor with rows and a null dst, or a null src unless its role is ZERO; an XYZ, SCALING
 * or ROTATION tensor of another row size, misaligned or given twice; S > 0 without all three of them, or without z. */
#define MOM_DENSIFY_MAX_TENSORS 32
#define MOM_DENSIFY_MAX_ROW_BYTES (1u << 20)
enum { MOM_DENSIFY_COPY = 0, MOM_DENSIFY_MOMENT, MOM_DENSIFY_XYZ, MOM_DENSIFY_SCALING, MOM_DENSIFY_ROTATION, MOM_DENSIFY_ZERO };
typedef struct MomDensifyTensor {
    const void* src;
    void* dst;
    unsigned row_bytes;
    int role;              /* MOM_DENSIFY_* */
} MomDensifyTensor;
size_t mom_densify_scratch_bytes(int P);
int mom_densify_plan(int P, const uint8_t* clone_mask, const uint8_t* split_mask, int* kept_index, int* clone_rank,
                     int* split_rank, int* counts_dev, int* counts_host, void* scratch, mom_stream_t stream);
int mom_densify_apply(int P, const int* kept_index, const int* clone_rank, const int* split_rank, const int* counts,
                      const float* z, const MomDensifyTensor* tensors, int count, size_t tensor_size, mom_stream_t stream);

/* ---- Densification statistics of one iteration (train_4DGS.py:266; scene/gaussian_model.py:713-715
 * add_densification_stats), in place, for the Gaussians with radii[i] > 0:
 *   max_radii2D[i] = max(max_radii2D[i], radii[i]);  xyz_gradient_accum[i] += |viewspace_grad[i, :2]|;  denom[i] += 1.
 * viewspace_grad is [P,3] (dL/d mean2D; the third column is unused), the three accumulators are [P] floats. */
int mom_densify_stats(int P, const int* radii, const float* viewspace_grad, float* max_radii2D, float* xyz_gradient_accum,
                      float* denom, const uint32_t* skip_if_nonzero /* as in mom_adam_step */, mom_stream_t stream);

/* ---- SSIM term of the loss (utils/loss_utils.py:29-92: ssim / _ssim / create_window / gaussian) ----
 * 11x11 Gaussian window = outer product of the 11 taps in window11 (host pointer; the reference's
 * gaussian(11, 1.5)), zero padding 5, C1 = 0.01^2, C2 = 0.03^2.  Images are [C][H][W] (any leading batch
 * dimension folded into C: the reference's conv2d is depthwise and its mean runs over every element).
 * forward:  sum points at MOM_SSIM_SUM_SLOTS doubles on the device (zeroed by the call): sum[0] receives the sum over
 *           all C*H*W elements of the SSIM map, so that ssim = sum[0] / (C*H*W); the other slots hold the partial
 *           sums the blocks spread their atomics over (one shared accumulator serialises in the L2).  dm (device, [3][C][H][W], or null when no gradient is wanted) receives the
 *           map's partial derivatives with respect to the blurred mu1, E[img1^2], E[img1*img2].
 * backward: dimg1 += scale * (scale_dev ? *scale_dev : 1) * d(*sum)/d img1, computed from dm.  For the loss
 *           term lambda * (1 - ssim) pass scale = -lambda / (C*H*W); scale_dev (device scalar, may be null)
 *           lets an autograd caller apply its upstream gradient without reading it back. */
#define MOM_SSIM_SUM_SLOTS 64
int mom_ssim_forward(int C, int H, int W, const float* window11, const float* img1, const float* img2, float* dm,
                     double* sum, mom_stream_t stream);
int mom_ssim_backward(int C, int H, int W, const float* window11, const float* img1, const float* img2, const float* dm,
                      float scale, const float* scale_dev, float* dimg1, mom_stream_t stream);
/* The same on a ROW SLAB of taller images (tile-row shard: a rank holds its own rows plus a halo): the pointers address the
 * slab's first row, H is the slab's height, channels (and the three derivative maps' channels) are chan_stride elements
 * apart (>= H*W; the full image's H*W).  The window is zero-padded at the slab's edges like at an image's, so only map rows
 * at least 5 pixels inside the slab are those of the full image: map rows in [sum_row0, sum_row1) (slab coordinates) are
 * summed, derivative maps are written for rows in [dm_row0, dm_row1) and zeroed elsewhere. */
int mom_ssim_forward_slab(int C, int H, int W, size_t chan_stride, int sum_row0, int sum_row1, int dm_row0, int dm_row1,
                          const float* window11, const float* img1, const float* img2, float* dm, double* sum,
                          mom_stream_t stream);
int mom_ssim_backward_slab(int C, int H, int W, size_t chan_stride, const float* window11, const float* img1, const float* img2,
                           const float* dm, float scale, const float* scale_dev, float* dimg1, mom_stream_t stream);

/* ---- HexPlane regularisers (scene/gaussian_model.py:730-769, scene/regulation.py:22-28) ----
 * value = sum over planes of w_smooth * mean((p[h+2]-2p[h+1]+p[h])^2) + w_l1 * mean|1-p|
 * (second difference along H, the reference's dim -2); if grad != null, grad_scale * d value / d plane is
 * ADDED into it.  Channel-last planes as above; a row is W * 32 floats, and the differences run along H per float: a [H][W][32]
 * plane passes its W, a [H][W][16] plane W / 2 (W even). */
#define MOM_REG_MAX_PLANES 24
typedef struct MomRegPlane {
    const float* plane;
    float* grad;
    int H, W;
    float w_smooth, w_l1, grad_scale;
} MomRegPlane;
int mom_plane_regulation(const MomRegPlane* planes, int count, float* value, mom_stream_t stream);
int mom_plane_regulation_acc(const MomRegPlane* planes, int count, float* value, mom_stream_t stream);   /* value is not zeroed first */
/* _acc with every gradient also multiplied by *upstream, a DEVICE scalar (null: 1): the weight autograd hands down to the
 * regulariser's backward, without reading it back to the host first. */
int mom_plane_regulation_grad(const MomRegPlane* planes, int count, float* value, const float* upstream, mom_stream_t stream);

/* ---- ordered loss values: the L1 sums, the SSIM sum and the regularisers' value as functions of their inputs, bit for bit ----------
 * mom_l1_loss, mom_ssim_forward and mom_plane_regulation end every workgroup with an atomicAdd into one or a few words, so the value
 * they return depends on the order the workgroups arrive in (the gradients behind them are formed per element and never did).  The
 * ordered forms STORE one partial per workgroup into caller-owned scratch and add the partials up in one more launch; there is no
 * float atomic anywhere in them (csrc/values_ordered.hip, the ordered instantiation of the SSIM kernel in csrc/ssim.hip).  Same
 * contract as the atomic entries: stream-ordered, no allocation, copy or synchronisation.  They store their results (nothing is
 * zeroed first and nothing is accumulated onto), and they compute VALUES only: the gradient image of the L1 pass and the SSIM
 * derivative maps are those of the atomic entries bit for bit, the regulariser's gradient stays with mom_plane_regulation_grad.
 *
 * FOLD.  fold(v_0 .. v_{m-1}) cuts the terms into blocks of 64 from the first, adds each block left to right from +0.0,
 *   b_j = (...((+0.0 + v_64j) + v_64j+1) + ...),  and then the block sums left to right,  fold = (...((+0.0 + b_0) + b_1) + ...);
 * fold of no term is +0.0.  Every order below is this one rule applied to a list that depends on the problem size alone -- not on a
 * grid chosen at launch, an environment switch, the pointers' alignment or which wave arrives first.
 * L1 (n elements, terms |d_i| and d_i * d_i with d_i = img[i] - gt[i], the product rounded on its own).  Workgroup g of
 *   ceil(n / 4096) owns elements [4096 g, 4096 g + 4096); its lane t of 256 owns the sixteen elements 4096 g + 1024 r + 4 t + j
 *   (r = 0..3 outer, j = 0..3 inner) and adds those below n in that -- ascending -- order from +0.0: lane_t.  The workgroup's partial
 *   is fold(lane_0 .. lane_255), and sums2[k] = fold(partial_0 .. partial_{G-1}), for k = 0 (|d|) and k = 1 (d * d) alike.
 *   dimg (may be null) = sign(d_i) * (1.0f / (float)n), mom_l1_loss's bits.  n == 0: both sums +0.0.
 * REGULARISERS (value of mom_plane_regulation; the planes' grad pointers are ignored).  The workgroups are mom_plane_regulation's:
 *   plane after plane in the order given, and within a [H][W * 32 floats] plane workgroup `local` covers the sixteen rows from
 *   16 (local / cb) and the 256 float columns from 256 (local % cb), cb = ceil(W * 32 / 256).  Lane t owns one column: for its rows h
 *   in ascending order it adds, from +0.0, first cs * s_h * s_h (s_h = p[h+2] - 2 p[h+1] + p[h], 0 where h + 2 >= H; the product formed
 *   as (cs * s_h) * s_h; cs = w_smooth / ((float)(H - 2) * (float)(W * 32)), 0 if H <= 2 or w_smooth == 0) and then, if w_l1 != 0,
 *   cl * |1 - p[h]| (cl = w_l1 / ((float)H * (float)(W * 32))); a lane whose column lies outside the plane holds +0.0.  The
 *   workgroup's partial is fold(lane_0 .. lane_255) and value = fold(all partials).  Every multiply and add is rounded on its own.
 * SSIM.  The map, the derivative maps dm and the workgroup totals are mom_ssim_forward's (one 16 x 16 tile of one channel per
 *   workgroup; its float total is the xor butterfly of each wave, offsets 32, 16, .. 1, then ((w_0 + w_1) + w_2) + w_3 over its
 *   four waves -- a fixed order).  The ordered form stores total_b at b = tile_x + tiles_x * (tile_y + tiles_y * channel) and
 *   sum[0] = fold(total_0 .. total_{B-1}) with every add in DOUBLE; only sum[0] is written (one double suffices).
 *   mom_ssim_sum_ordered is that fold alone, on `blocks` floats on the device.  The row slabs of a tile-row shard have no ordered form.
 * SCRATCH (the *_scratch_bytes queries; 0 for a size the call refuses or that needs none).  L1: the partials [2][G] floats.  SSIM:
 *   the totals [B] floats.  Regularisers: the partials, one float per workgroup.  Every byte a call reads it has written first.
 * MOM_EINVAL before anything is launched: a null image, target, result, window or plane pointer; n above 2^40; C above 65535 or more
 * than 65535 tile rows; a plane with H or W outside 1 .. 2^24, more than MOM_REG_MAX_PLANES planes or 2^30 workgroups; scratch
 * null or not 4-byte aligned where any is needed, scratch_bytes below the query's answer.
 * The *_host entries are the same sums in plain C++ (no contraction, no GPU; host pointers): what the device returns, bit for bit. */
size_t mom_l1_loss_ordered_scratch_bytes(size_t n);
int mom_l1_loss_ordered(size_t n, const float* img, const float* gt, float* dimg, float* sums2, void* scratch, size_t scratch_bytes,
                        mom_stream_t stream);
int mom_l1_loss_ordered_host(size_t n, const float* img, const float* gt, float* dimg, float* sums2);
size_t mom_ssim_ordered_scratch_bytes(int C, int H, int W);
int mom_ssim_forward_ordered(int C, int H, int W, const float* window11, const float* img1, const float* img2, float* dm,
                             double* sum, void* scratch, size_t scratch_bytes, mom_stream_t stream);
int mom_ssim_sum_ordered(size_t blocks, const float* totals, double* sum, mom_stream_t stream);
int mom_ssim_sum_ordered_host(size_t blocks, const float* totals, double* sum);
size_t mom_plane_regulation_ordered_scratch_bytes(const MomRegPlane* planes, int count);
int mom_plane_regulation_ordered(const MomRegPlane* planes, int count, float* value, void* scratch, size_t scratch_bytes,
                                 mom_stream_t stream);
int mom_plane_regulation_ordered_host(const MomRegPlane* planes, int count, float* value);

/* ---- fused deformation MLP (scene/deformation.py:53-65,97-135; W = 64, defor_depth = 0, heads pos/scales/rot) ----
 *   h0 = W0 feat + b0 ;  o_k = W2_k relu(W1_k relu(h0) + b1_k) + b2_k  for k in {pos, scales, rot}
 *   pts = xyz + o_pos + flow_coef * scene_flow ; scales = scaling + o_scales ; rots = rotation + o_rot
 * (flow_coef = delta_scale * frame_num, deformation.py:114).  Weights are nn.Linear tensors ([out,in] row-major);
 * both kernels are persistent and keep all four 64x64 matrices in LDS. */
typedef struct MomDeformMLP {
    const float *W0, *b0;            /* feature_out.0: [64,64], [64]  ([64,in_features] for the _n entry points below) */
    const float *W1[3], *b1[3];      /* {pos,scales,rotations}_deform.1: [64,64], [64] */
    const float *W2[3], *b2[3];      /* {pos,scales,rotations}_deform.3: [3|3|4,64], [3|3|4] */
    float *dW0, *db0, *dW1[3], *db1[3], *dW2[3], *db2[3];   /* backward only: ACCUMULATED into (+=) */
} MomDeformMLP;
/* a0_save (may be null for inference): [P,64], receives relu(h0) for the backward pass */
int mom_deform_forward(const MomDeformMLP* w, int P, const float* feat /* [P,64] */, const float* xyz, const float* scaling,
                       const float* rotation, const float* scene_flow, float flow_coef, float* pts, float* scales, float* rots,
                       float* a0_save, mom_stream_t stream);
/* The same, also leaving the activated values the rasterizer takes (gaussian_renderer/__init__.py:96-99: scaling_activation = exp,
 * rotation_activation = normalize, opacity_activation = sigmoid of the UNdeformed opacity) -- what mom_activations_forward would
 * compute from scales / rots / opacity_raw, without its launch.  Any of scales_act, rots_act, opacity_act may be null;
 * opacity_raw is required exactly when opacity_act is given. */
int mom_deform_forward_activated(const MomDeformMLP* w, int P, const float* feat, const float* xyz, const float* scaling,
                                 const float* rotation, const float* scene_flow, float flow_coef, float* pts, float* scales,
                                 float* rots, float* a0_save, const float* opacity_raw, float* scales_act, float* rots_act,
                                 float* opacity_act, mom_stream_t stream);
/* d{pts,scales,rots}: gradients of the three outputs; writes dfeat [P,64]; weight/bias gradients accumulate into w->d*.
 * (The identity paths d xyz += dpts etc. are the caller's.) */
size_t mom_deform_backward_scratch_bytes(int P);   /* the larger of 4 x [P,64] floats + 70 KB (the two-kernel form's pre-activation gradients and the
                                                       staging area its weight gradients meet in) and the one-kernel form's per-workgroup partial
                                                       sums (17.8 MB).  Either form adds to a weight-gradient buffer ONCE per element. */
int mom_deform_backward(const MomDeformMLP* w, int P, const float* feat, const float* a0, const float* dpts,
                        const float* dscales, const float* drots, float* dfeat, void* scratch, mom_stream_t stream);
/* The same with a second stream at the callee's disposal.  Default form (one kernel on the bf16 matrix pipe, csrc/deform_bwd_b3.hip:
 * the pre-activation gradients never leave the CU): dfeat is complete on `stream`; the weight / bias gradients are complete on
 * `dw_stream` (the sum over the workgroups' partial sums runs there, ordered behind the kernel on `stream`).
 * Two-kernel f32 form (MOM_MLP_BWD=split in the environment; the tests' reference): dfeat and the thin output layers' gradients are complete on `stream`,
 * the 64x64 layers' weight / bias gradients on `dw_stream`, which the call orders behind the part on `stream` that produces their
 * input.  Either way the caller joins `dw_stream` before reading the gradients or reusing `scratch`.  dw_stream == stream:
 * identical to mom_deform_backward.  These two are the forms there are: any other non-empty value of MOM_MLP_BWD than "b3" (the default)
 * or "split" is MOM_EINVAL. */
int mom_deform_backward_split(const MomDeformMLP* w, int P, const float* feat, const float* a0, const float* dpts,
                              const float* dscales, const float* drots, float* dfeat, void* scratch, mom_stream_t stream,
                              mom_stream_t dw_stream);
/* The four calls above for a trunk of `in_features` inputs (csrc/deform_mlp.hip: one set of kernel templates for both widths).  MomDeformMLP keeps its layout; W0 and dW0 point
 * at [64,in_features] tensors, feat and dfeat are [P,in_features], everything else (a0 [P,64], the heads, the scratch size) is as above.
 *   in_features == 64: exactly the call without _n (which forwards here).
 *   in_features == 32 (two HexPlane levels of 16 channels, dnerf/eulerian_150_16): the fp32 kernels at that width.  The backward is the
 *     two-kernel f32 form whatever MOM_MLP_BWD says -- unset, empty, "b3" or "split"; there is no bf16 one-kernel form for this
 *     shape -- with the stream contract of that form; any other value is MOM_EINVAL as above.
 *   anything else: MOM_EINVAL, before anything is launched. */
int mom_deform_forward_n(const MomDeformMLP* w, int P, int in_features, const float* feat /* [P,in_features] */, const float* xyz,
                         const float* scaling, const float* rotation, const float* scene_flow, float flow_coef, float* pts,
                         float* scales, float* rots, float* a0_save, mom_stream_t stream);
int mom_deform_forward_activated_n(const MomDeformMLP* w, int P, int in_features, const float* feat, const float* xyz,
                                   const float* scaling, const float* rotation, const float* scene_flow, float flow_coef, float* pts,
                                   float* scales, float* rots, float* a0_save, const float* opacity_raw, float* scales_act,
                                   float* rots_act, float* opacity_act, mom_stream_t stream);
int mom_deform_backward_n(const MomDeformMLP* w, int P, int in_features, const float* feat, const float* a0, const float* dpts,
                          const float* dscales, const float* drots, float* dfeat, void* scratch, mom_stream_t stream);
int mom_deform_backward_split_n(const MomDeformMLP* w, int P, int in_features, const float* feat, const float* a0, const float* dpts,
                                const float* dscales, const float* drots, float* dfeat, void* scratch, mom_stream_t stream,
                                mom_stream_t dw_stream);
/* ---- ordered MLP weight gradients: mom_deform_backward_n whose weight and bias gradients are a function of their inputs ----------
 * The two-kernel f32 form at either width (32 or 64 features, whatever MOM_MLP_BWD says), on ONE stream, with stores where that
 * form has float atomics (dfeat never had any).  Workgroup b of the first kernel -- min(ceil(P / 32), 256) of them, each a fixed
 * contiguous share of the 32-point tiles, dealt to its 8 waves by index -- adds its waves' output-layer sums in wave order,
 * ((+0.0 + wave_0) + wave_1) + ..., and stores record b; workgroup (layer L, range r) of the second -- 256 ranges of four consecutive
 * wave ranges of ceil(P / 1024) points rounded up to even -- adds its four waves' 64 x 64 tile the same way and stores record
 * (L, r).  Then every element takes its records in ascending index, total = (...((+0.0 + rec_0) + rec_1) + ...), and dst += total.
 * Both mappings are arithmetic on the workgroup and wave index: the order depends on P alone.
 * SCRATCH (mom_deform_backward_ordered_scratch_bytes(P); 0 for P < 0), in floats: dH [4][P][64], rounded up to a multiple of 64; then
 * the first kernel's records [256][784]: [3 heads][4][64] weights, [3][4] biases at 768, of which the first min(ceil(P / 32), 256)
 * are written; then the second kernel's records [4 layers][256][4160]: [64][in] weights ([64][32] for layer 0 at 32 features),
 * the 64 biases at 4096.  MOM_EINVAL as mom_deform_backward_n, and for scratch_bytes below that size. */
size_t mom_deform_backward_ordered_scratch_bytes(int P);
int mom_deform_backward_ordered_n(const MomDeformMLP* w, int P, int in_features, const float* feat, const float* a0, const float* dpts,
                                  const float* dscales, const float* drots, float* dfeat, void* scratch, size_t scratch_bytes,
                                  mom_stream_t stream);

/* ---- deformation field in one pass (the render() case: ONE timestamp for every point) ----
 * deform_network.forward = HexPlaneField lookup + trunk + heads (scene/deformation.py:97-153, scene/hexplane.py:160-183) as a
 * single persistent kernel: a wave gathers the 64 features of its tile of 32 Gaussians into their rows of feat[P,64] (feat_save,
 * kept for the backward's weight gradients, or a buffer in `scratch`), reads them back in the matrix-core operand layout and runs
 * the MLP on the bf16 pipe.  The three space-time planes are first collapsed to per-frame lines (one tiny launch into `scratch`,
 * mom_deform_field_scratch_bytes).  Same outputs and activated copies as mom_hexplane_forward + mom_deform_forward_activated;
 * `order` (optional) is the processing order as in mom_hexplane_forward.  Needs levels == 2, channels == 32 and resolutions
 * <= 1024 (mom_deform_field_supported); other shapes take the two separate calls. */
int mom_deform_field_supported(const MomHexPlane* hp);
size_t mom_deform_field_scratch_bytes(const MomHexPlane* hp, int P /* 0 if every call keeps a feature copy (feat_save) */);
int mom_deform_field_forward(const MomHexPlane* hp, const MomDeformMLP* w, int P, const float* xyz, float time,
                             const uint32_t* order, const float* scaling, const float* rotation, const float* scene_flow,
                             float flow_coef, float* pts, float* scales, float* rots, float* feat_save, float* a0_save,
                             const float* opacity_raw, float* scales_act, float* rots_act, float* opacity_act, void* scratch,
                             mom_stream_t stream);

/* The same for a field of two levels of 16-channel planes (dnerf/eulerian_150_16; csrc/deform_field16.hip): ONE persistent fp32
 * kernel computes what mom_hexplane_forward (channels 16) followed by mom_deform_forward_activated_n (in_features 32) computes, bit
 * for bit; a tile's 32 features go from the gather to the trunk layer through LDS and reach memory only if the caller asks for a
 * copy.  Argument list of mom_deform_field_forward with feat_save [P,32] and a0_save [P,64], both optional, as are the three
 * activated outputs (opacity_raw is required exactly when opacity_act is given).  Needs channels == 16, levels == 2 and resolutions
 * <= 1024 (mom_deform_field16_supported: 0 for everything else, 32 channels and 16 x 3 / 16 x 4 levels included); an unsupported
 * field or a missing argument is MOM_EINVAL before anything is launched, P == 0 does nothing.  Nothing is staged in memory:
 * mom_deform_field16_scratch_bytes is one aligned block and `scratch` is not read (it may be null). */
int mom_deform_field16_supported(const MomHexPlane* hp);
size_t mom_deform_field16_scratch_bytes(const MomHexPlane* hp, int P);
int mom_deform_field16_forward(const MomHexPlane* hp, const MomDeformMLP* w, int P, const float* xyz, float time,
                               const uint32_t* order, const float* scaling, const float* rotation, const float* scene_flow,
                               float flow_coef, float* pts, float* scales, float* rots, float* feat_save, float* a0_save,
                               const float* opacity_raw, float* scales_act, float* rots_act, float* opacity_act, void* scratch,
                               mom_stream_t stream);

/* ---- the scene-flow fit of the motion optimisation module (train_motion.py:125-207 MotionOptimization.optimize_motion) ----
 * SGD on the [3,P] Eulerian scene flow against V views' 2D flows, all E epochs in one launch: a thread owns a point and keeps its
 * flow in registers (csrc/sceneflow_fit.hip).  Per epoch e (train_motion.py:134-203), with q = p + f:
 *     c = R_j q + T_j, h = K c, (u, v) = (h_x, h_y) / h_z                      train_motion.py:169-172,181
 *     d = ((u, v) - pix0) - gt                                                 :184,187 (utils/loss_utils.py l1_loss)
 *     loss[e] = sum over j and the view's valid points of w_j (|d_x| + |d_y|)  :187-189; w_j = (1 / divisor) / (2 n_j)
 *     f -= lr[e] * d loss[e] / d f, sign(0) = 0                                :190-193, once per epoch; lr[e] = 0.5 * 0.97^e, :128-130,203
 *   points  [3,P]; K: HOST memory, the row-major 3x3 [[fx,0,cx],[0,fy,cy],[0,0,1]] of train_motion.py:58-62 (anything else: MOM_EINVAL)
 *   R [V,3,3], T [V,3] world to camera (:147-153 composes them); w [V]
 *   records [V,P,4] = {pix0.x, pix0.y, gt.x, gt.y} (16-byte aligned): the unflowed pixel of :180,183 and the estimated flow sampled
 *           there (:120); entries of invalid (view, point) pairs are read and ignored
 *   valid   [ceil(V/32),P] words: bit j % 32 of valid[j / 32][p] = point p is in view j's valid set (:173-177)
 *   lr [E]; flow [3,P] in and out (the reference starts from zeros, helpmotion.py:27)
 *   loss [E] or null; flow2d_last [V,P,2] or null: the last epoch's (u, v) - pix0, taken before the last update (:196-200), 0 where
 *           invalid; not written when E == 0
 *   scratch: mom_sceneflow_fit_scratch_bytes(P, V, E) bytes when loss is given (per-wave partial sums, added in a fixed order by a
 *           second launch on the same stream: no atomics, the same bits on every run); otherwise not read and may be null
 * Stream-ordered, no allocation, no copy, no synchronisation.  P == 0 does nothing.  V <= 0, E < 0, P < 0, a null required pointer,
 * a misaligned records / flow2d_last or a scratch_bytes below the sizing function's value: MOM_EINVAL before anything is launched.
 * Nothing guards h_z <= 0 once the flow has moved a valid point behind a camera: inf / nan there, as in the reference. */
size_t mom_sceneflow_fit_scratch_bytes(int P, int V, int E);
int mom_sceneflow_fit(int P, int V, int E, const float* points, const float* K, const float* R, const float* T, const float* w,
                      const float* records, const uint32_t* valid, const float* lr, float* flow, float* loss, float* flow2d_last,
                      void* scratch, size_t scratch_bytes, mom_stream_t stream);

/* ---- the fit's records: every view's 2D flow image sampled at the view's projected points (train_motion.py:117-121) ----
 * What scipy.interpolate.griddata(pixel grid, image, pixels, method="linear") computes there, for all V views in one launch
 * (csrc/flow_sample.hip): linear interpolation inside one of the two triangles of the pixel's cell.  Which diagonal splits a cell is
 * the triangulation's choice and depends on (H, W) alone; the caller passes it as one bit per cell.  Per valid (view, point),
 * everything in float64 without contraction, each channel f of the image:
 *     x0 = clamp((int)floor(u), 0, W-2); y0 = clamp((int)floor(v), 0, H-2); fx = u - x0; fy = v - y0
 *     f00 = f(x0,y0)  f10 = f(x0+1,y0)  f01 = f(x0,y0+1)  f11 = f(x0+1,y0+1)                  (float -> double)
 *     anti-diagonal cell: fx + fy <= 1 ? f00 + fx (f10 - f00) + fy (f01 - f00) : f11 + (1-fx) (f01 - f11) + (1-fy) (f10 - f11)
 *     main-diagonal cell: fx >= fy     ? f00 + fx (f10 - f00) + fy (f11 - f10) : f00 + fx (f11 - f01) + fy (f01 - f00)
 *     gt = (float)result
 *   flow    [V,H,W,2] float32, channel-last (8-byte aligned)
 *   pix     [V,P,2] float64 (16-byte aligned): the unflowed pixel (u, v) as the reference hands it to griddata (:115,120)
 *   valid   [ceil(V/32),P] words, the layout mom_sceneflow_fit reads
 *   diag    [ceil((H-1)(W-1)/32)] words: bit c % 32 of diag[c / 32], c = y (W-1) + x; set: the anti-diagonal (x+1,y)-(x,y+1) splits cell
 *           (x, y); clear: the main diagonal (x,y)-(x+1,y+1)
 *   records [V,P,4] float32 (16-byte aligned) = {(float)u, (float)v, gt.x, gt.y}, what mom_sceneflow_fit reads.  EVERY record is
 *           written: an invalid pair's is four zeros, chosen by selection on its bit; its cell indices are clamped like any other's
 *           (in float64, before the conversion), so whatever pix holds there -- NaN, 1e300 -- reaches no address.
 * Stream-ordered, no allocation, no copy, no synchronisation.  P == 0 does nothing.  P < 0, V <= 0, V > 65535 (the view is a grid
 * axis), H < 2, W < 2, a null pointer or a misaligned flow / pix / records: MOM_EINVAL before anything is launched. */
int mom_flow_sample(int P, int V, int H, int W, const float* flow, const double* pix, const uint32_t* valid, const uint32_t* diag,
                    float* records, mom_stream_t stream);

/* ---- values given at each view's projected points -> every pixel centre (train_motion.py:198,304,319) ----
 * What scipy.interpolate.griddata(view's pixels, values, pixel grid, method="linear", fill_value=fill) computes, for all V views in
 * one call (csrc/tri_resample.hip), given the views' triangulations (scipy.spatial.Delaunay's simplices: the host makes them once per
 * view, motion.triangulate_views).  Pixel (X, Y) of view j takes the LOWEST-INDEX triangle of that view whose test passes, and `fill`
 * if none does.  For a triangle with vertices p0, p1, p2 (rows tris[t][0..2] of the view's points), in float64 without contraction:
 *     a = x0 - x2; b = x1 - x2; c = y0 - y2; d = y1 - y2; det = a d - b c; dx = X - x2; dy = Y - y2
 *     c0 = (d dx - b dy) / det;  c1 = (a dy - c dx) / det;  c2 = (1 - c0) - c1
 *     test: -eps <= ci <= 1 + eps for all three, eps = 100 * 2^-52 (the bounds scipy's LinearNDInterpolator uses)
 *     out[k] = ((c0 v0[k]) + (c1 v1[k])) + (c2 v2[k])                                         (float -> double)
 *   The test is evaluated at the pixel centres of the triangle's bounding box, grown by MOM_TRI_BOX_GROW = 2^-20 on every side and
 *   clamped to the image: [ceil(min x - 2^-20), floor(max x + 2^-20)] x the same in y.  In exact arithmetic a centre outside the
 *   ungrown box by more than eps (|a| + |b|) cannot pass, so nothing is missed while the vertices lie within 2^24 of the image.
 *   A triangle with an index outside [0, n_j), a non-finite vertex, det == 0 or a non-finite det is skipped.
 *   pts     [N,2] float64 (16-byte aligned): the views' points (u, v) concatenated, view j's are rows pt_off[j] .. pt_off[j+1]
 *   pt_off  [V+1], tri_off [V+1] int32 DEVICE arrays.  Contract: non-decreasing, off[0] = 0, off[V] = N (T).  They are not read on the
 *           host; whatever they hold, a range read from them is used only if it lies within [0, N] ([0, T]), so a broken array loses
 *           triangles, never reaches an address outside the buffers and never makes a loop longer than 16 steps
 *   tris    [T,3] int32, indices LOCAL to the view;  values [N,C] float32, 1 <= C <= 8;  out [V,H,W,C] float64, written in full
 *   scratch mom_tri_resample_scratch_bytes(V, H, W) bytes, 4-byte aligned: owner [V,H,W] int32, the index of each pixel's triangle.
 *           The owner word, not the order the atomics land in, decides the result: the same bits on every run
 * Three launches on `stream` (init, cover, resolve); no allocation, no copy, no synchronisation.  A lane walks its triangle's box while
 * that has at most MOM_TRI_LANE_BOX pixels; a larger one is taken by the whole wave.  A view without points or triangles is all `fill`.
 * V <= 0, V > 65535, H < 1, W < 1, V H W >= 2^31, C outside 1..8, N < 0, T < 0, a null pointer that would be read or written, a
 * misaligned pts / scratch or a scratch_bytes below the sizing function's value (0 for an unsupported shape): MOM_EINVAL before
 * anything is launched. */
#define MOM_TRI_LANE_BOX 64
size_t mom_tri_resample_scratch_bytes(int V, int H, int W);
int mom_tri_resample(int V, int H, int W, int C, int N, int T, const double* pts, const int* pt_off, const int* tris,
                     const int* tri_off, const float* values, double fill, double* out, void* scratch, size_t scratch_bytes,
                     mom_stream_t stream);

/* ---- the per-pixel remainder of the multi-view point-cloud renders (MotionOptimization.render_PCD, train_motion.py:298-330,355,357)
 * resampled [V,H,W,4] float64 = (r, g, b, m): mom_tri_resample's output for the points' colours and ONE mask channel (the reference's
 * three are equal; where it sums three, (m + m) + m is formed).  Per view, everything in float64 without contraction, as written there:
 *    1 border (:305,320)  I = resampled[clamp(y,1,H-2)][clamp(x,1,W-2)], what edgemask I + (1-edgemask) pad(I[1:-1,1:-1], edge) is
 *    2 hit (:298,310-311) hit[rint(v)][rint(u)] = 1 for every point of the view (half to even; a point that rounds outside is skipped)
 *    3 dil (:312)         the 9 x 9 maximum of hit, the window clipped to the image (scipy's `reflect` border for a maximum / minimum)
 *    4 holes (:313)       rgb' = dil rgb + (1 - dil) (-1)
 *    5 (:315)             mj = the 11 x 11 minimum of ((r' + g') + b' != -3)
 *    6 (:316)             image = mj rgb' + (1 - mj) 0
 *    7 (:325)             m' = dil m + (1 - mj) (-1)          -- mj, the RGB pass's eroded mask, as the reference has it
 *    8 (:327)             mj2 = the 11 x 11 minimum of ((m' + m') + m' != -3)
 *    9 (:328-330)         mask = mj2 m' + (1 - mj2) 0
 *   10 (:355,357)         byte = rint(255 x), half to even; the reference's values lie in [0, 1], anything else is clamped to 0..255
 *   image [V,H,W,3], mask [V,H,W] uint8;  pts, pt_off as for mom_tri_resample;  scratch: mom_pcd_compose_scratch_bytes(V, H, W) bytes
 *   (five byte maps).
 * Five launches on `stream`; no allocation, no copy, no synchronisation.  The shapes mom_tri_resample refuses, H < 5, W < 5, a null
 * pointer, a misaligned pts / resampled or too small a scratch: MOM_EINVAL before anything is launched. */
size_t mom_pcd_compose_scratch_bytes(int V, int H, int W);
int mom_pcd_compose(int V, int H, int W, int N, const double* resampled, const double* pts, const int* pt_off, uint8_t* image,
                    uint8_t* mask, void* scratch, size_t scratch_bytes, mom_stream_t stream);

/* ---- the Delaunay triangulation of every view's points, on the device (csrc/delaunay.hip) ----
 * What mom_tri_resample needs between upload_views' points and its own call: pts / pt_off in, tris / tri_off out, no triangle
 * crosses the host.  Where a view's Delaunay triangulation is unique -- no predicate below falls inside its filter bound -- the result
 * is that triangulation, the set of triangles scipy.spatial.Delaunay gives; anything else is refused per view by a status code, never
 * guessed.
 *   pts [N,2] float64 (16-byte aligned), pt_off [V+1] int32 DEVICE: mom_tri_resample's layout and rules (not read on the host; a
 *           range read from pt_off is used only when it lies inside [0, N], any other makes the view MOM_DELAUNAY_FEW).  The device
 *           finds a point's view by a search of pt_off: with ranges that overlap (a pt_off that decreases somewhere) a point counts
 *           for one of them only, and the agreement with the twin below holds for a non-decreasing pt_off alone; memory stays safe
 *   tris    capacity [2N,3] int32, indices LOCAL to the view, packed view after view;  tri_off [V+1] int32, written on the device:
 *           both can be handed to mom_tri_resample unchanged
 *   status  [V] int32, per view the LARGEST code any of its points raised (no order decides it):
 *           MOM_DELAUNAY_OK            triangulated
 *           MOM_DELAUNAY_FEW           n_j < 3
 *           MOM_DELAUNAY_UNCERTAIN     a predicate fell inside its filter bound: duplicate, collinear or cocircular points, or
 *                                      anything too close to call (the exact pixel grid is all of these)
 *           MOM_DELAUNAY_OVERFLOW      a star outgrew MOM_DELAUNAY_MAX_STAR neighbours; or more points were deferred than the
 *                                      scratch's list holds (N / 8 + 4096), or their finished stars hold more than 16 words per
 *                                      entry of that list on average: then every view with a deferred point
 *           MOM_DELAUNAY_RANGE         a non-finite point, or one outside [0, W-1] x [0, H-1]
 *           MOM_DELAUNAY_INCONSISTENT  the count check below failed
 *           A view whose status is not 0 contributes no triangles and does not disturb any other view.
 * CANONICAL FORM: a function of the input, the same bits on every run.  Each triangle (i, j, k) has i as its smallest index and is
 *   counter-clockwise, orient(p_i, p_j, p_k) > 0 in the (u, v) coordinates as given; a view's triangles are sorted by (i, j); an OK
 *   view has T_j = 2 n_j - 2 - h_j triangles, h_j the number of points with an unbounded cell -- checked on the device.
 * PREDICATES, float64 without contraction, eps = 2^-53 (Shewchuk's first-stage bounds); the twin uses the same expressions:
 *   orient(a, b, c):      l = (ax-cx)(by-cy); r = (ay-cy)(bx-cx); det = l - r; certain iff |det| > (3 + 16 eps) eps (|l| + |r|)
 *   incircle(a, b, c, d): adx = ax-dx, ... cdy = cy-dy; alift = adx^2 + ady^2, likewise blift, clift;
 *                         det  = alift (bdx cdy - bdy cdx) + blift (cdx ady - cdy adx) + clift (adx bdy - ady bdx)
 *                         perm = alift (|bdx cdy| + |bdy cdx|) + blift (|cdx ady| + |cdy adx|) + clift (|adx bdy| + |ady bdx|)
 *                         certain iff |det| > (10 + 96 eps) eps perm
 *   An uncertain predicate makes the view MOM_DELAUNAY_UNCERTAIN; there is no exact-arithmetic stage.
 * THE STAR of p: its neighbours counter-clockwise around it; a consecutive pair (a, b) is a finite vertex if orient(p, a, b) > 0,
 *   otherwise the gap (p is on the hull).  A candidate q is a neighbour iff incircle(p, a, b, q) > 0 for a finite vertex or q lies in
 *   the gap's wedge, orient(p, a, q) > 0 or orient(p, q, b) > 0.  The vertices q cuts are a run of the cyclic list and q takes the place
 *   of the neighbours inside the run, so in a closed cell the in-circle tests alone place q: three points in a line that form no
 *   triangle make nothing uncertain there (while the cell is still open, such a triple with an end of the gap does).  A q that enters
 *   the gap removes the neighbours on either side while its pair with them is finite and the vertex beyond them holds q in its circle;
 *   a walk stops at a gap and does not start across one.  Candidates come from the image's pixel cells (cell (X, Y): floor(u) = X, floor(v) = Y,
 *   a cell's points by index): the rings around p's cell until the cell is closed and every circle lies within the rings, one lane
 *   per point with MOM_DELAUNAY_LANE_STAR neighbours in LDS; a point that outgrows that, lies on the hull or keeps a large circle
 *   after ring 3 is deferred to a second launch, one WAVE per point with MOM_DELAUNAY_MAX_STAR neighbours in LDS, which then visits
 *   for every vertex the rows of cells its circle -- grown by 2^-20, so that rounding can only add cells -- or the gap's wedge meets,
 *   until a pass inserts nothing; its lanes test 64 candidates of a row at a time, insertions are serial and in the candidates'
 *   order, and the finished star goes to a pool in scratch sized by the deferred list.  p writes the triangles (p, a, b) of its finite vertices with p < a and p < b.
 *   scratch mom_delaunay_scratch_bytes(V, H, W, N) bytes, 4-byte aligned; after the call its first two int32 words hold the number of
 *           deferred points and the largest star of the call.
 * Ten launches on `stream`; no allocation, no copy, no synchronisation, no float atomics.  V <= 0, V > 65535, H < 1, W < 1,
 * V H W >= 2^31, N < 0, N > 2^30, a null pointer that would be read or written, a misaligned pts / scratch or a scratch_bytes below the
 * sizing function's value (0 for an unsupported shape): MOM_EINVAL before anything is launched.  mom_delaunay_host is the twin: host
 * pointers, plain C++, the same decisions -- tris, tri_off and status equal the device's integer for integer; a test seam, not a
 * fallback. */
#define MOM_DELAUNAY_OK 0
#define MOM_DELAUNAY_FEW 1
#define MOM_DELAUNAY_UNCERTAIN 2
#define MOM_DELAUNAY_OVERFLOW 3
#define MOM_DELAUNAY_RANGE 4
#define MOM_DELAUNAY_INCONSISTENT 5
#define MOM_DELAUNAY_LANE_STAR 12
#define MOM_DELAUNAY_MAX_STAR 1020
size_t mom_delaunay_scratch_bytes(int V, int H, int W, int N);
int mom_delaunay(int V, int H, int W, int N, const double* pts, const int* pt_off, int* tris, int* tri_off, int* status,
                 void* scratch, size_t scratch_bytes, mom_stream_t stream);
int mom_delaunay_host(int V, int H, int W, int N, const double* pts, const int* pt_off, int* tris, int* tri_off, int* status);

/* ---- the warp of the reference's video generator (thirdparty/StyleCineGAN; csrc/eulerian_warp.hip) ----
 * The part of that generator that is neither a network nor a checkpoint.  All arithmetic is fp32 without contraction, operation by
 * operation what the reference's torch ops and its CUDA string compute.  Every call is stream-ordered on `stream`, allocates nothing,
 * copies nothing and does not synchronise; a shape it refuses is MOM_EINVAL before anything is launched.
 *
 * mom_euler_integrate (utils/cinemagraph_utils.py:9-59, euler_integration): one launch, each lane walks its own pixel's chain.
 *   motion [2,H,W] (x then y); disp [2,H,W], or [steps+1,2,H,W] when all_frames (return_all_frames; frame 0 is zero).  Per step, as
 *   :43-57: gather at (rintf(y), rintf(x)) -- half to even, torch.round's -- add; out of bounds if x > W-1, x < 0, y > H-1 or y < 0; the
 *   flag is sticky; an invalid pixel is reset to its own coordinate (displacement 0).  Integers and fp32 adds only: the reference's bits.
 *   NOT the reference: a coordinate that becomes NaN also sets the flag (the reference's comparisons are false for a NaN and its next
 *   step indexes with garbage), and every gather index is clamped, so non-finite motion reads nothing out of range and gives
 *   displacement 0.  H < 1, W < 1, H W >= 2^31, steps < 0 or a null pointer: MOM_EINVAL.
 *
 * mom_softsplat_sum (utils/softmax_splatting.py:8-53, kernel_Softsplat_updateOutput; the forward of _FunctionSoftsplat, :236-269):
 *   input [N,C,H,W], flow [N,2,H,W]; output [N,C,H,W] is ADDED to (the caller zeroes it).  Per element: o = (float)x + flow, the four
 *   corners of floor(o) with the weights as written there (:32-35), input * weight added atomically; a corner outside the canvas is
 *   dropped.  NOT the reference: a coordinate that is NaN or not below 2^30 in magnitude is dropped whole instead of being converted.
 *   N, C, H or W < 1, H W >= 2^31 or a null pointer: MOM_EINVAL.
 *
 * mom_eulerian_geometry: the sizes blend_feature / crop_padded_tensor derive from a square feature of size S (:139-147, 62-66, 77-83):
 *   cut = 3 / 2 / 1 at S = 1024 / 512 / 256, else 0; s = S - 2 cut; pad = s/4 + s/8; padded = s + 2 pad; crop0 = (padded - S) / 2.
 *   S < 1, pad >= s (ReflectionPad2d's own condition) or a crop that does not fit: MOM_EINVAL.  Any output pointer may be null.
 *
 * mom_eulerian_blend (cinemagraph_utils.py:131-178, blend_feature; utils/joint_splatting.py:23-42, joint_splatting mode "full"):
 *   feature [C,S,S], motion [2,S,S] (already at the feature's size; H and W are both passed so that a non-square call is refused,
 *   not misread), acc [padded,padded,C+1] channel-last, cleared by this call (a memset node) and then added to by one launch.  Per
 *   source pixel of the cut, reflection-padded domain (index arithmetic; nothing is padded or concatenated in memory): the future chain
 *   of idx steps on +motion and the past chain of n_frames-idx-1 steps on -motion (mom_euler_integrate's walk on the padded field);
 *   then (feature Z) w and Z w are added for the four corners of both halves, Z = (float)(1-alpha) for the future half and (float)alpha
 *   for the past half, alpha = idx / (n_frames-1) in double.  The reference puts the past half padded columns to the right
 *   with `padded` taken off its x flow and crops the result: the same canvas.  Its two fp32 roundings, (float)(x + padded) + (d -
 *   (float)padded), are reproduced, so only the order of the adds differs from the reference.
 *   form 0: the channel runs on the fastest lanes (a wave-instruction adds to contiguous bytes of a texel); form 1: a lane adds its
 *   own pixel's channels in a loop (measured for C = 1 and 3: DESIGN.md 3.18).
 *   C < 1, H != W, a size mom_eulerian_geometry refuses, n_frames < 2, idx outside [0, n_frames), form outside 0..1, a null pointer:
 *   MOM_EINVAL.
 *
 * mom_eulerian_finish (softmax_splatting.py:341-344; cinemagraph_utils.py:498-531 feature_inpaint_conv; :77-83 crop_padded_tensor):
 *   acc as mom_eulerian_blend leaves it.  out = acc[.. c] / metric with metric = acc[.. C], 0 -> 1.  full == 0: out [C,S,S] is the
 *   crop starting at crop0, and a pixel with metric == 0 -- the blank mask, which the reference gets from a second blend of a
 *   tensor of ones: a sum of non-negative terms is zero only if every term is -- takes the 7 x 7 box mean of the normalised map, 49
 *   products with (float)(1/49), zero padding at the padded map's border.  full != 0: out [C,padded,padded], the whole normalised
 *   map without the fill (blend_feature's own return).  blank (or null): [S,S] or [padded,padded] bytes, 1 where metric == 0.
 *   One launch.  C < 1, a size mom_eulerian_geometry refuses, padded > 65535 when full, a null acc or out: MOM_EINVAL. */
int mom_euler_integrate(int H, int W, int steps, int all_frames, const float* motion, float* disp, mom_stream_t stream);
int mom_softsplat_sum(int N, int C, int H, int W, const float* input, const float* flow, float* output, mom_stream_t stream);
int mom_eulerian_geometry(int S, int* cut, int* pad, int* padded, int* crop0);
int mom_eulerian_blend(int C, int H, int W, int idx, int n_frames, int form, const float* feature, const float* motion, float* acc,
                       mom_stream_t stream);
int mom_eulerian_finish(int C, int S, int full, const float* acc, float* out, uint8_t* blank, mom_stream_t stream);

/* ---- ordered splat of the video generator's warp: an accumulator that is a function of its inputs, bit for bit -------------------
 * mom_eulerian_blend and mom_softsplat_sum add with float atomics, in whatever order the waves arrive.  The ordered forms are a PULL:
 * a texel's sum is formed by the texel's owner from the entries of the four cells around it, with no float atomic anywhere
 * (csrc/eulerian_ordered.hip).  Same contract as the atomic entries: stream-ordered, no allocation, copy or synchronisation,
 * MOM_EINVAL before anything is launched; acc is [padded,padded,C+1] channel-last and mom_eulerian_finish takes it unchanged (the
 * ordered blend stores every element of it: no memset node); mom_softsplat_sum_ordered adds onto `output`.
 *
 * ENTRIES.  The blend: e = h padded^2 + (y padded + x), h = 0 the future half, h = 1 the past half, (y, x) the source pixel of the
 * cut, reflection-padded domain.  The splat: e = y W + x, per image.  An entry's target (ox, oy) is what the atomic form computes, bit
 * for bit (the same chain walk; for the past half the two roundings (float)(x + padded) + (d - (float)padded)).  It lies in cell
 * (y0, x0) = (floor oy, floor ox); its four weights are those of softmax_splatting.py:32-35 as formed there.  An entry the atomic form
 * drops whole (a NaN target, or a magnitude not below 2^30) has no terms.  A corner outside the canvas is no term; a corner inside
 * the canvas with weight 0 is one.
 * TERMS.  The products the atomic form adds, each one fp32 multiply: the blend's (feature[c] Z_h) w for the C channels and Z_h w
 * (formed as (1.0f Z_h) w) for the metric; the splat's input[c] w.
 * ORDER.  Texel (y, x), channel c receives four classes:
 *   k = 0  nw: the entries of cell (y, x)        k = 1  ne: cell (y, x-1)
 *   k = 2  sw: cell (y-1, x)                     k = 3  se: cell (y-1, x-1)
 * with cells running over [-1, H-1] x [-1, W-1] (H = W = padded for the blend).  Within a class the cell's entries are taken in
 * ascending e.  The terms are cut into blocks of 64 from the first:
 *   b_j = (...((+0.0 + e_64j) + e_64j+1) + ...)  left to right;      s_k = (...((+0.0 + b_0) + b_1) + ...)  left to right;
 *   T = (s_0 + s_1) + (s_2 + s_3)  (s_k = +0.0 for a class without terms).
 * The blend stores acc = T for every texel and channel: a texel nothing reaches holds +0.0, which mom_eulerian_finish reads as
 * blank.  The splat stores out = out_in + T, one add onto whatever the buffer held; a texel without a term in any class is not
 * written.  The result is a function of the feature (input), the motion (flow), idx and n_frames alone -- not of a grid size, a
 * `form`, an environment switch or which wave arrives first.  The _host entries reproduce it on the host (plain C++, no GPU, no
 * contraction) from HOST pointers.
 *
 * SCRATCH (mom_eulerian_ordered_scratch_bytes(C, S), mom_softsplat_ordered_scratch_bytes(N, C, H, W); 0 for a shape the call
 * refuses).  n entries and m cells (blend: n = 2 padded^2, m = (padded+1)^2; splat: n = H W, m = (H+1)(W+1), one image after the
 * other out of the same buffers), every part at the next multiple of 256 bytes: the entries' records {ox, oy, Z, source index}
 * (16 n bytes), the sort's two key and two value buffers (4 n bytes each) and its counters, the cells' segment table (4 (m + 1)
 * bytes) and, for the blend at C >= 16, a channel-last copy of the feature (4 S S C bytes).  Every byte a call reads it has written
 * first.
 * LIMITS.  The sort's keys and values are 32 bits and its positions ints: n <= 2^30 and m < 2^31.  MOM_EINVAL before anything is
 * launched: everything mom_eulerian_blend (without `form`) or mom_softsplat_sum refuses; n or m beyond those limits; scratch null or
 * not aligned to 256 bytes; scratch_bytes below the sizing function's value.  The _host entries refuse the same shapes and null
 * pointers. */
size_t mom_eulerian_ordered_scratch_bytes(int C, int S);
int mom_eulerian_blend_ordered(int C, int H, int W, int idx, int n_frames, const float* feature, const float* motion, float* acc,
                               void* scratch, size_t scratch_bytes, mom_stream_t stream);
size_t mom_softsplat_ordered_scratch_bytes(int N, int C, int H, int W);
int mom_softsplat_sum_ordered(int N, int C, int H, int W, const float* input, const float* flow, float* output, void* scratch,
                              size_t scratch_bytes, mom_stream_t stream);
int mom_eulerian_blend_ordered_host(int C, int H, int W, int idx, int n_frames, const float* feature, const float* motion, float* acc);
int mom_softsplat_sum_ordered_host(int N, int C, int H, int W, const float* input, const float* flow, float* output);

/* ---- the native ops of the StyleGAN2 under that generator (thirdparty/StyleCineGAN/models/stylegan2/op, and the encoder's copy under
 * external_modules/feature_style_encoder/pixel2style2pixel; csrc/stylegan_ops.hip) ----
 * The reference compiles both from CUDA sources when the package is imported and has no other path.  fp32, caller-allocated outputs,
 * stream-ordered on `stream`, no allocation, copy or synchronisation; MOM_EINVAL before anything is launched.  Forward and both
 * backward orders of the reference's autograd functions are these two calls with other arguments (stylegan_op.py).  The model files
 * and the checkpoints are not part of this library.
 *
 * mom_upfirdn2d (op/upfirdn2d.py:85-121; upfirdn2d_kernel.cu): x is M planes of [H,W], k is [kh,kw], out is M planes of [out_h,out_w],
 *   out_h = (H up_y + pad_y0 + pad_y1 - kh) / down_y + 1 and out_w likewise (op/upfirdn2d.py:100-101); pads of either sign.
 *     out[m,oy,ox] = sum over a < kh, b < kw of k[kh-1-a][kw-1-b] U[oy down_y + a - pad_y0][ox down_x + b - pad_x0]
 *     U[Y][X]      = x[m][Y/up_y][X/up_x] if Y, X >= 0, up_y | Y, up_x | X and the quotients lie in [0,H) x [0,W); 0 otherwise
 *   Each output is one fp32 sum in a fixed order (a ascending, then b; only the taps with up | coordinate are visited), without
 *   atomics: two calls give the same bits.  up_x == up_y, down_x == down_y and (up, down, kh x kw) one of (1,1,4x4) (1,1,3x3)
 *   (2,1,4x4) (2,1,2x2) (1,2,4x4) (1,2,2x2) -- the reference's six dispatch modes, upfirdn2d_kernel.cu:172-268 -- run compile-time
 *   instantiations that stage the input tile in LDS; everything else runs one general kernel.
 *   M, H, W < 1, a factor < 1, kh or kw outside 1..32, out_h or out_w < 1, H up, |pad| or down not below 2^29, H W or out_h out_w not
 *   below 2^31, 2^24 or more output tiles of 64 x 16, or a null pointer: MOM_EINVAL.
 *
 * mom_fused_bias_act (op/fused_act.py; fused_bias_act_kernel.cu:18-49 as its switch writes it): n elements; x' = x + b[(i / step_b)
 *   % size_b] when b is not null; with act * 10 + grad =
 *     10, 11: y = x'      12, 32: y = 0      30: y = x' > 0 ? x' : x' alpha      31: y = ref > 0 ? x' : x' alpha
 *   out = y scale.  Three fp32 roundings in that order (add, multiply, multiply), no contraction: bit-equal to the same statement in
 *   numpy float32.  ref is read for 31 alone.
 *   act outside {1,3}, grad outside 0..2, n < 1, n >= 2^31 (the reference's own int), step_b < 1, b with size_b < 1, 31 without ref,
 *   a null x or out: MOM_EINVAL. */
int mom_upfirdn2d(int M, int H, int W, int kh, int kw, int up_x, int up_y, int down_x, int down_y, int pad_x0, int pad_x1, int pad_y0,
                  int pad_y1, const float* x, const float* k, float* out, mom_stream_t stream);
int mom_fused_bias_act(size_t n, int step_b, int size_b, int act, int grad, float alpha, float scale, const float* x, const float* b,
                       const float* ref, float* out, mom_stream_t stream);

/* ---- the arithmetic around stage 1's 2D flow estimator (train_motion.py:368-374 estimate_flow; csrc/flow_frame.hip) ----
 * The reference runs it on the CPU once per view; both calls take all V views.  fp32 in the reference's order of operations, without
 * contraction except in the bilinear resize (below), caller-allocated outputs, stream-ordered on `stream`, no allocation, copy, synchronisation or atomic: two calls give the
 * same bits.  The estimator between the two calls (SPADEUnetMaskMotion.forward_flow) is not part of this library.
 *
 * mom_hint_field (thirdparty/cinemagraphy/demo.py:24-105, generate_mask_hints_from_user, from :73 on; the selection of the hints in
 *   front of it is host code, motion.hint_arguments):
 *   hint_pos [V,max_hints,2] int32 (x, y), hint_start / hint_end [V,max_hints,2] float64 (x, y): view v uses its first hint_count[v]
 *   rows (clamped to 0..max_hints); the hint's motion is (end - start) / 50 in float64 (:68-70).  sigma [V] float32; mask [V,H,W] bytes;
 *   hints [V,2,S,S], mask_s [V,1,S,S] float32.  Per pixel (x, y) of the H x W image, with fp32 coordinates (:77-81):
 *     dist = sqrt(dx dx + dy dy); w = expf(-(dist / sigma)^2); m_c = (float)((double)m_c + (double)w motion_c); norm += w    (:90-94)
 *     norm == 0 -> 1; field_c = m_c / norm * (mask != 0) * (float)(S / W or S / H)                                              (:95-101)
 *   then hints = the field resized bilinearly to S x S (:102) as torch's CPU kernels run F.interpolate(align_corners=False): the source
 *   coordinate fma(in / S, o + 0.5, -0.5), clamped at 0, its integer part and fraction in fp32, and fma(l0, a, l1 b) for each sum; and
 *   mask_s = F.interpolate(mode='area') of mask != 0 (:103): over the window [floor(o in / S), ceil((o + 1) in / S)) the count of
 *   ones, divided by the window's height and then by its width.  sqrt and the divisions are correctly rounded; expf is the device
 *   library's (1 ulp), the one operation that is not the reference's bits.  A hint's position is only ever a coordinate: nothing is
 *   indexed by it (the reference indexes its pixel grid with it and raises outside the image; the host mirrors that).
 *   Two launches: the field at H x W into scratch (V 2 H W floats, mom_hint_field_scratch_bytes), then the three S x S planes of
 *   every view.  One launch would evaluate every hint's exponential at the four source pixels of every output pixel: 9 times the
 *   exponentials at the reference's 512 -> 768.
 *
 * mom_flow_finish (thirdparty/cinemagraphy/lib/renderer.py:598-606, the tail of compute_flow_and_inpaint):
 *   pred [V,2,S,S], mask_s [V,1,S,S] -> flow [V,2,H,W]:  p = pred mask_s; b = the 15 x 15 box mean of p, zeros outside the image (the sum of
 *   15 row sums of 15 terms, divided by 225); flow = bilinear resize to H x W of b mask_s (float)(W / S or H / S).  The reference's
 *   `for _ in range(7)` blurs the SAME input seven times and keeps the last result (:600-601): one blur is what it computes.
 *   Two launches: blur, mask and scale into scratch (V 2 S S floats, mom_flow_finish_scratch_bytes), then the resize.
 *
 * V < 1, V > 21845, H, W or S < 1, V 2 H W or V 2 S S >= 2^31, max_hints outside 0..MOM_HINTS_MAX, a null pointer that would be read or
 * written, a misaligned scratch or a scratch_bytes below the sizing function's value (0 for an unsupported shape): MOM_EINVAL before
 * anything is launched. */
#define MOM_HINTS_MAX 1024
size_t mom_hint_field_scratch_bytes(int V, int H, int W);
int mom_hint_field(int V, int H, int W, int S, int max_hints, const int* hint_pos, const double* hint_start, const double* hint_end,
                   const int* hint_count, const float* sigma, const uint8_t* mask, float* hints, float* mask_s, void* scratch,
                   size_t scratch_bytes, mom_stream_t stream);
size_t mom_flow_finish_scratch_bytes(int V, int S);
int mom_flow_finish(int V, int S, int H, int W, const float* pred, const float* mask_s, float* flow, void* scratch,
                    size_t scratch_bytes, mom_stream_t stream);

/* ---- rendered image -> 8-bit interleaved RGB (render_4DGS.py:64 torchvision.utils.save_image: x * 255 + 0.5, clamp, truncate;
 * CHW -> HWC) in one pass, so that a frame can leave the device as the bytes a PNG encoder takes.  img [C,H,W] floats, out [H,W,C]
 * bytes; C <= 4. */
int mom_image_to_rgb8(int C, int H, int W, const float* img, uint8_t* out, mom_stream_t stream);

/* ---- those bytes -> the zlib stream of a PNG's IDAT, on the device (csrc/png_encode.hip, csrc/png_dev.h), so that the host only
 * frames it in chunks and writes it (render.AsyncPNGWriter(encoder="device"); the reference encodes on the host inside its timed
 * loop, render_4DGS.py:60-71).  Lossless: the stream inflates to the PNG scanlines -- a filter byte (1 Sub, 2 Up or 4 Paeth, the one
 * with the smallest sum of absolute signed residuals) and the filtered row -- of exactly the bytes given.
 *   Stream: 78 01; per segment of 4 rows one deflate block (BFINAL = 0), the smaller of a Huffman-coded block -- deflate's fixed
 *   code or one of a few constant dynamic-block tables (the cheapest for the segment), literals and run-length matches at distance 1
 *   and C, lengths 3..258 -- closed by an empty stored block so that it ends on a byte, and ceil(n / 65535) stored blocks; a final
 *   empty fixed block 03 00; the Adler-32 of the scanlines, big-endian.
 *   the bound        the capacity that always suffices: 2 + every segment as stored blocks + 2 + 4.  0 for an unsupported shape:
 *                    C not 1, 3 or 4, H < 1, W < 1, or a bound of 2^31 and above
 *   the scratch size bytes of device scratch for mom_png_encode (0 for an unsupported shape)
 *   the encoder      rgb8 [H,W,C], out [capacity], out_size [1], scratch: device pointers.  Four launches on `stream`; no allocation, no
 *                    copy, no synchronisation.  out[*out_size ..] is not written.
 *   the host form    the same stream, byte for byte, computed on the host from host pointers: a test seam (the device coder's
 *                    per-chunk code is host code too), not a fallback -- nothing in the package calls it in place of the kernels
 *   the tables       index -1: returns the number of tables.  Otherwise fills table `index`: litlen [288] and dist [32] code lengths
 *                    (0 = no code), header = the block header the encoder emits (BFINAL = 0, BTYPE, a dynamic block's code lengths),
 *                    least-significant bit first, *header_bits its length; returns the number of tables
 * An unsupported shape, a null pointer, a capacity below the bound, a table index out of range or a header_capacity too small:
 * MOM_EINVAL before anything is launched. */
size_t mom_png_bound(int C, int H, int W);
size_t mom_png_scratch_bytes(int C, int H, int W);
int mom_png_encode(int C, int H, int W, const uint8_t* rgb8, uint8_t* out, size_t capacity, uint32_t* out_size, void* scratch,
                   mom_stream_t stream);
int mom_png_encode_host(int C, int H, int W, const uint8_t* rgb8, uint8_t* out, size_t capacity, uint32_t* out_size);
int mom_png_tables(int index, uint8_t* litlen, uint8_t* dist, uint8_t* header, int header_capacity, int* header_bits);

/* ---- a rendered frame -> a baseline JPEG file, on the device (csrc/jpeg_encode.hip, csrc/jpeg_dev.h): the frames of the Motion-JPEG
 * video render.AsyncVideoWriter writes (the reference hands its frames to imageio on the host, render_4DGS.py:74-76).  The file is
 * what libjpeg writes for the same pixels with the quality Q, 4:2:0 sampling, the tables of ITU T.81 Annex K, the "islow" integer
 * transform and a restart interval of R MCUs (R: mom_jpeg_tables) -- every segment but APPn, and the scan bit for bit:
 *   SOI, APP0 (JFIF 1.01), DQT x 2, SOF0, DHT x 4, DRI, SOS, the intervals with RSTn between them, EOI.
 *   the bound        the capacity that always suffices: the header and every block of every interval at its longest code, every byte
 *                    stuffed.  0 for an unsupported shape: H or W outside 1..65535, or a bound of 2^31 and above
 *   the scratch size bytes of device scratch for mom_jpeg_encode / _chw (0 for an unsupported shape)
 *   the encoder      rgb8 [H][row_stride] bytes, R G B interleaved (row_stride >= 3 W), out [capacity], out_size [1], scratch: device
 *                    pointers.  Three launches on `stream`; no allocation, no copy, no synchronisation.  out[*out_size ..] is not written.
 *   _chw             the same encoder reading the window [y0, y0 + H) x [x0, x0 + W) of a [3, IH, IW] float image through the
 *                    reference's to8b: uint8(255 * clip(x, 0, 1)), truncated (not mom_image_to_rgb8's rounding)
 *   the host form    the same file, byte for byte, computed on the host from host pointers
 *   the tables       for the quality Q: quant [2][64] (luminance, chrominance; row-major 8x8), the four Huffman tables in the file's
 *                    order (DC luminance, AC luminance, DC chrominance, AC chrominance) as dht_counts [4][16], dht_symbols [4][162]
 *                    (zero-filled behind dht_nsymbols [4]), and *restart_interval = R
 * Q outside 1..100, an unsupported shape, a window outside the image, a row_stride below 3 W, a null pointer or a capacity below the
 * bound: MOM_EINVAL before anything is launched or written. */
size_t mom_jpeg_bound(int H, int W);
size_t mom_jpeg_scratch_bytes(int H, int W);
int mom_jpeg_encode(int H, int W, const uint8_t* rgb8, size_t row_stride, int Q, uint8_t* out, size_t capacity, uint32_t* out_size,
                    void* scratch, mom_stream_t stream);
int mom_jpeg_encode_chw(int IH, int IW, int y0, int x0, int H, int W, const float* image, int Q, uint8_t* out, size_t capacity,
                        uint32_t* out_size, void* scratch, mom_stream_t stream);
int mom_jpeg_encode_host(int H, int W, const uint8_t* rgb8, size_t row_stride, int Q, uint8_t* out, size_t capacity,
                         uint32_t* out_size);
int mom_jpeg_tables(int Q, uint8_t* quant, uint8_t* dht_counts, uint8_t* dht_symbols, int* dht_nsymbols, int* restart_interval);

/* ---- PIL's 8-bit bicubic resize on the device (csrc/pil_resize.hip): the bytes of Image.resize((OW, OH), Image.BICUBIC) of an "L"
 * (C = 1) or "RGB" (C = 3) image, what stage 1 resizes its video frames and the flow estimator's inputs with (train_motion.py:407,
 * demo.py:109-127).  PIL resamples an axis of `in` samples to `out` with integer arithmetic on coefficients computed in double:
 *   scale = in / out, fs = max(scale, 1), support = 2 fs, ksize = (int)ceil(support) * 2 + 1; for the output index xx:
 *   center = (xx + 0.5) scale, xmin = max((int)(center - support + 0.5), 0), n = min((int)(center + support + 0.5), in) - xmin,
 *   w[x] = f((x + xmin - center + 0.5) * (1 / fs)) for x < n, with f the cubic convolution kernel at a = -0.5; the weights are summed
 *   left to right and divided by a non-zero sum; k = (int)(w 2^22 + 0.5) for w >= 0 and (int)(w 2^22 - 0.5) below; a sample is
 *   clamp((2^21 + sum byte k) >> 22, 0, 255), the shift arithmetic on the signed 32-bit sum.
 * The horizontal axis goes first and is rounded to bytes, the vertical axis runs on those bytes; an axis with in == out is skipped,
 * and with both skipped the result is a copy.  "RGBA" is refused: PIL premultiplies alpha there, which is another arithmetic.
 *   _ksize           host, no GPU: ksize of (in_size, out_size)
 *   _coeffs          host, no GPU: bounds [out_size][2] = (xmin, n) and kk [out_size][ksize], zero behind n -- the tables a caller
 *                    uploads once per (in_size, out_size) and keeps
 *   _scratch_bytes   bytes of the intermediate mom_pil_resize needs: N H rows of OW C bytes at a pitch of 16; 0 when H == OH (the
 *                    vertical axis is skipped and nothing is staged) and for a shape that is refused
 *   mom_pil_resize   src [N,H,W,C] bytes -> out [N,OH,OW,C] bytes.  bounds_x / kk_x: the DEVICE tables of (W, OW), bounds_y / kk_y of
 *                    (H, OH); the pair of a skipped axis is not read and may be null.  scratch: device, 16-byte aligned.  One launch
 *                    per axis (a copy kernel when none changes) on `stream`: no allocation, no copy, no synchronisation, no atomics.
 *                    Windows read from the tables are clamped to the image, so wrong tables give wrong pixels, never a read outside src.
 *   _to8b            the same kernels reading src [N,H,W,C] float32: each sample first goes through (uint8)(x * 255.0f) -- the float32
 *                    product, truncated, clamped to 0..255 -- which is numpy's (frame * 255).astype(np.uint8) of train_motion.py:407
 *                    for x in (-1/255, 256/255); outside that interval numpy's cast is platform-defined and the clamp is this
 *                    library's choice (a NaN gives 0)
 *   _host            the bytes of mom_pil_resize computed on the host from host pointers, tables and all: a test seam like
 *                    mom_png_encode_host, not a fallback -- nothing in the package calls it
 * filter: MOM_RESIZE_BICUBIC, PIL's value.  Another filter, C other than 1 or 3, a size below 1, any of the three images at 2^31
 * bytes or more, a null or misaligned pointer, a scratch too small: MOM_EINVAL before anything is launched or written.  So is
 * H > 100 W with OH < H and OW != W: recent Pillow (Image.resize, its Python part) resamples such a strip vertically first, which
 * rounds differently, and that order is not built. */
#define MOM_RESIZE_BICUBIC 3
int mom_pil_resize_ksize(int in_size, int out_size, int filter);
int mom_pil_resize_coeffs(int in_size, int out_size, int filter, int* bounds, int* kk);
size_t mom_pil_resize_scratch_bytes(int N, int H, int W, int C, int OH, int OW);
int mom_pil_resize(int N, int H, int W, int C, const uint8_t* src, int OH, int OW, int filter, const int* bounds_x, const int* kk_x,
                   const int* bounds_y, const int* kk_y, uint8_t* out, void* scratch, size_t scratch_bytes, mom_stream_t stream);
int mom_pil_resize_to8b(int N, int H, int W, int C, const float* src, int OH, int OW, int filter, const int* bounds_x,
                        const int* kk_x, const int* bounds_y, const int* kk_y, uint8_t* out, void* scratch, size_t scratch_bytes,
                        mom_stream_t stream);
int mom_pil_resize_host(int N, int H, int W, int C, const uint8_t* src, int OH, int OW, int filter, uint8_t* out);

const char* mom_version(void);

/* Per-kernel HIP-event timing (bench.py's live roofline figure).  Slots: see mom_profile_name(0..15).
 * While a slot is enabled launches of that kernel are bracketed by two hipEventRecord on the launch stream: every launch with
 * on = 1, every on-th launch with on > 1 (an event pair costs the stream ~13 us of bubbles; a sampled mean costs 1/on of that).
 * mom_profile_read synchronises those events and returns the accumulated time and the number of launches TIMED. */
#define MOM_PROF_SLOTS 16
int mom_profile_enable(int slot, int on);
int mom_profile_read(int slot, double* total_ms, long long* count, int reset);
const char* mom_profile_name(int slot);

/* Stream ordering for a host mirror that runs parts of a step on a second stream (no counterpart in the reference, whose loop is
 * single-stream; torch's own Stream / Event objects do the same at 8-10 us of host time per call).
 * mom_stream_wait_stream: everything enqueued on `waiter` after this call runs after everything enqueued on `signaler` before it.
 * mom_stream_mark / mom_stream_wait_mark: a ring of MOM_STREAM_MARKS reusable marks per device -- record the current tail of a
 * stream under a slot number, make another stream wait for it later (a wait refers to the slot's most recent record at the time of
 * the call; waiting for a slot that was never recorded is MOM_EINVAL).
 * These calls order STREAMS OF ONE DEVICE and nothing else: their events carry no system-scope release (hipEventDisableSystemFence --
 * 3.4 instead of 6.2 us of the recording stream per record; MOM_EVENT_SYSTEM_FENCE=1 in the environment restores the default), so they
 * publish nothing to the host or to another device. */
#define MOM_STREAM_MARKS 64
int mom_stream_wait_stream(mom_stream_t waiter, mom_stream_t signaler);
int mom_stream_mark(int slot, mom_stream_t stream);
int mom_stream_wait_mark(mom_stream_t stream, int slot);
/* bytes of zeros at ptr, stream-ordered (the gradient buckets a step clears on its second stream) */
int mom_zero_async(void* ptr, size_t bytes, mom_stream_t stream);

/* ---- collectives of a multi-GPU step, over librccl (RCCL on xGMI), one process per GPU.
 * No counterpart in the reference, which is single-GPU: its batch axis (train_4DGS.py:172-229, `batch_size` cameras rendered one after
 * the other, loss averaged) is what the camera-batch shard spreads over ranks, and these are the exchanges of that shard and of the
 * tile-row shard.  They exist as C entry points because a torch.distributed call costs the rank's host 40-50 us
 * and the host paces a rank; here a collective is one ncclXxx call on a raw stream handle (~2 us), ordered against the compute
 * streams with mom_stream_mark / mom_stream_wait_mark.
 *   mom_comm_available     1 if librccl could be resolved (dlopen at first use; a process that has imported torch gets torch's copy)
 *   mom_comm_unique_id     rank 0 makes the 128-byte id and hands it to the other ranks through the launcher's own rendezvous
 *   mom_comm_create        ncclCommInitRank on the calling thread's CURRENT device; collective over all `world` ranks
 *   mom_comm_all_reduce    in place over `count` elements
 *   mom_comm_all_gather    in place: buf holds world x count_per_rank elements, this rank's slab at rank x count_per_rank going in
 *   mom_comm_reduce_scatter in place: buf holds world x count_per_rank elements; this rank's reduced block lands at rank x count_per_rank,
 *                          the rest of buf is left in an unspecified state
 *   mom_comm_group_start / _end   ncclGroupStart / ncclGroupEnd: the calls in between are submitted as one launch
 * dtype: MOM_COMM_F32 | MOM_COMM_I32 (4-byte elements); op: MOM_COMM_SUM | MOM_COMM_MAX.  Every rank must issue the same sequence. */
typedef struct MomComm MomComm;
#define MOM_COMM_F32 0
#define MOM_COMM_I32 1
#define MOM_COMM_SUM 0
#define MOM_COMM_MAX 1
int mom_comm_available(void);
const char* mom_comm_last_error(void);
int mom_comm_unique_id(void* id128);
int mom_comm_create(MomComm** out, const void* id128, int world, int rank);
int mom_comm_destroy(MomComm* comm);
int mom_comm_abort(MomComm* comm);
int mom_comm_world(const MomComm* comm);
int mom_comm_rank(const MomComm* comm);
int mom_comm_group_start(void);
int mom_comm_group_end(void);
int mom_comm_all_reduce(MomComm* comm, void* buf, size_t count, int dtype, int op, mom_stream_t stream);
int mom_comm_all_gather(MomComm* comm, void* buf, size_t count_per_rank, int dtype, mom_stream_t stream);
int mom_comm_reduce_scatter(MomComm* comm, void* buf, size_t count_per_rank, int dtype, int op, mom_stream_t stream);

/* Self test of the wave64 DPP reduction used by the render backward:
 * out[w] = sum(in[64w .. 64w+63]). */
int mom_selftest_wave_sum(const float* in, float* out, int waves, mom_stream_t stream);
/* Self test of the render backward's packed reduction (row-level DPP reduce-scatter of nvals = 9 or 10 values per lane, then the
 * 4 x 4 row transposition over four splats): in [waves][4][nvals][64] -> out [waves][4][nvals] = the sums over the 64 lanes. */
int mom_selftest_row_reduce(const float* in, float* out, int waves, int nvals, mom_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MOM4D_H_INCLUDED */
