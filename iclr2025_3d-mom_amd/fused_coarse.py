"""One coarse-stage training iteration as an explicit launch sequence -- no autograd graph, no activated copies of the parameters.

The coarse stage (train_4DGS.py:149-297 with stage "coarse", the first 3 000 iterations of every run) renders the Gaussians
WITHOUT the deformation field: the rasterizer's inputs are the model's own parameters through exp / normalize / sigmoid
(gaussian_renderer/__init__.py:113,130-132).  So the step is the rasterizer and the loss alone:

    projection on the raw parameters (MomRasterArgs.params_raw) -> binning -> compositing forward with the L1 epilogue
    (+ SSIM when lambda_dssim != 0) -> compositing backward -> projection backward, which writes the six parameter gradients
    through the activations and, below densify_until_iter, the densification statistics (MomRasterGrads.stats_*).

It leaves `.grad` on _xyz, _features_dc, _features_rest, _scaling, _rotation and _opacity only: the deformation network, the
HexPlane planes and _scene_flow keep None, so optimizer.step() skips them exactly as torch Adam does in the reference's coarse
stage.  What Trainer uses of fused_step.FusedStep -- the sticky overflow word and its ring, exact_next, next_tag -- is offered
with the same meaning, so the overflow / replay machinery of train.Trainer runs unchanged.  `tests/test_coarse_stage_gpu.py`
checks this step against the op-by-op autograd path.
"""
import ctypes as C
import math

import torch

from . import _native as N
from . import ops
from .fused_step import L1_PARTIALS, LazyLoss, _Lazy, _TileSums


class FusedCoarseStep:
    RING = 64
    HEADROOM, MARGIN = 1.5, 65536     # binning capacity = HEADROOM x an earlier frame's instance count + MARGIN (as FusedStep)
    keep_all_tiles = False            # True: bin whole rectangles like the reference (MomRasterArgs.keep_all_tiles)

    def __init__(self, gaussians, opt, hyper, background):
        self.g, self.opt, self.hyper, self.bg = gaussians, opt, hyper, background
        self.P = -1
        self.lib = N.lib()
        self.last = {}
        self.dist = None
        self.next_tag = 1
        self.stats_done = False       # whether the last step's projection backward updated the densification statistics
        self._frame = None
        self._resize_next = False
        self.cap = 0

    def _ensure(self, P, W, H, dev):
        f = dict(dtype=torch.float32, device=dev)
        e = lambda *s: torch.empty(*s, **f)
        if self._frame != (W, H, dev):
            self._frame = (W, H, dev)
            self.color, self.depth, self.dimg = e(3, H, W), e(1, H, W), e(3, H, W)
            self.img = torch.empty(self.lib.mom_raster_image_bytes(W, H), dtype=torch.uint8, device=dev)
            self.nr_dev = torch.zeros(1, dtype=torch.int32, device=dev)
            self.nr_host = torch.zeros(1, dtype=torch.int32).pin_memory()
            self.flag_ring = torch.zeros(self.RING, dtype=torch.int32).pin_memory()
            # L1 sums in spare words of the image scratch's header, which the projection clears every step (as FusedStep)
            hdr_f = self.img[(-self.img.data_ptr()) % 256:][:256].view(torch.float32)
            self.sums = hdr_f[8:10]
            self.l1_part = e(((W + 15) // 16) * ((H + 15) // 16), 2)
            self.ssim_dm = None
            self.binning = None
            self.P = -1
        if P == self.P:
            return
        self.P = P
        # [radii (P) | sticky overflow word]: the word keeps its value when P (and so its position) changes
        old = getattr(self, "flags", None)
        self._ibucket = torch.zeros(P + 1, dtype=torch.int32, device=dev)
        self.radii, self.flags = self._ibucket[:P], self._ibucket[P:]
        if old is not None and old.device == dev:
            self.flags.copy_(old)
        self.geom = torch.empty(self.lib.mom_raster_geom_bytes(P), dtype=torch.uint8, device=dev)
        # the six parameter gradients (persist across steps; .grad points at them) + the screen-space gradient and the internal ones
        self._grads = e(59 * P)
        cut = [0, 3 * P, 6 * P, 51 * P, 54 * P, 58 * P, 59 * P]
        seg = lambda i: self._grads[cut[i]:cut[i + 1]]
        self.gxyz, self.gdc, self.grest = seg(0).view(P, 3), seg(1).view(P, 1, 3), seg(2).view(P, 15, 3)
        self.gsc, self.grot, self.gop = seg(3).view(P, 3), seg(4).view(P, 4), seg(5).view(P, 1)
        self.g2d, self.gcol, self.gcov = e(P, 3), e(P, 3), e(P, 6)
        self.cap = 0                       # the first step at a new P sizes its binning buffer from its own count (one sync)

    def exact_next(self):
        """Size the binning buffer of the next step from that step's own instance count (one host sync): it cannot overflow."""
        self._resize_next = True

    def post_flag(self, slot):
        """Copy the overflow word to ring slot `slot` behind everything enqueued so far (FusedStep.post_flag)."""
        self.flag_ring[slot:slot + 1].copy_(self.flags, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        return ev

    def gather_moments(self):
        """(No sharded Adam in the coarse stage: the optimizer state is always whole.)"""

    def forward_backward(self, cam, delta_scale=1, early_adam=None, stats=False):
        """One coarse iteration up to (not including) the optimizer step.  stats: update the densification statistics in the
        projection backward (the caller's iteration is below densify_until_iter).  early_adam is ignored: there is no deformation
        backward to hide Adam under.  Returns (loss, radii, screen-space gradient) like FusedStep.forward_backward."""
        g, lib, s = self.g, self.lib, N.current_stream()
        dev = g._xyz.device
        P = g._xyz.shape[0]
        W, H = int(cam.image_width), int(cam.image_height)
        self._ensure(P, W, H, dev)
        if self._resize_next:
            self.cap, self._resize_next = 0, False
        view, proj, campos, gt = cam.device_tensors(dev)
        xyz, scal, rot, opac = g._xyz.detach(), g._scaling.detach(), g._rotation.detach(), g._opacity.detach()
        f_dc, f_rest = g._features_dc.detach(), g._features_rest.detach()
        for t in (xyz, scal, rot, opac, f_dc, f_rest):
            if not t.is_contiguous():
                raise N.MomError("FusedCoarseStep: the Gaussian parameters must be contiguous")
        a = N.MomRasterArgs()
        a.P, a.D, a.M, a.W, a.H = P, g.active_sh_degree, 16, W, H
        a.background, a.means3D = self.bg.data_ptr(), xyz.data_ptr()
        a.shs, a.shs_rest = f_dc.data_ptr(), f_rest.data_ptr()
        a.colors_precomp, a.cov3D_precomp = None, None
        # the raw parameters: the projection applies exp / normalize / sigmoid itself (gaussian_renderer/__init__.py:130-132)
        a.params_raw = 1
        a.opacities, a.scales, a.rotations = opac.data_ptr(), scal.data_ptr(), rot.data_ptr()
        a.viewmatrix, a.projmatrix, a.campos = view.data_ptr(), proj.data_ptr(), campos.data_ptr()
        a.scale_modifier = 1.0
        a.tan_fovx, a.tan_fovy = math.tan(cam.FoVx * 0.5), math.tan(cam.FoVy * 0.5)
        a.keep_all_tiles = int(self.keep_all_tiles)
        a.l1_target, a.l1_grad = gt.data_ptr(), self.dimg.data_ptr()
        if L1_PARTIALS:
            a.l1_partials = self.l1_part.data_ptr()
        else:
            a.l1_sums = self.sums.data_ptr()
        a.overflow_tag = self.next_tag
        prev_R = int(self.nr_host[0])
        N.check(lib.mom_raster_forward_geometry(C.byref(a), self.geom.data_ptr(), self.img.data_ptr(), self.radii.data_ptr(),
                                                self.nr_dev.data_ptr(), self.nr_host.data_ptr(), s), "raster_geometry")
        if self.cap == 0:                       # size exactly (one sync)
            torch.cuda.current_stream().synchronize()
            prev_R = int(self.nr_host[0])
        want = max(prev_R, int(prev_R * self.HEADROOM) + self.MARGIN)
        if self.binning is None or want > self._bin_cap or want < self._bin_cap // 4:
            self._bin_cap = want
            self.binning = torch.empty(lib.mom_raster_binning_bytes(P, W, H, want), dtype=torch.uint8, device=dev)
        self.cap = self._bin_cap
        N.check(lib.mom_raster_forward_render(C.byref(a), self.geom.data_ptr(), self.binning.data_ptr(), self.cap,
                                              self.img.data_ptr(), self.color.data_ptr(), self.depth.data_ptr(),
                                              self.flags.data_ptr(), s), "raster_render")
        n = self.color.numel()
        lam = float(self.opt.lambda_dssim)
        if lam != 0:
            # loss += lambda_dssim * (1 - ssim(image, gt))  (train_4DGS.py:222-223): its gradient is added into dimg
            win = ops._ssim_window()
            if self.ssim_dm is None:
                self.ssim_dm = torch.empty((3, 3, H, W), dtype=torch.float32, device=dev)
                self.ssim_sum = torch.empty(N.SSIM_SUM_SLOTS, dtype=torch.float64, device=dev)
            N.check(lib.mom_ssim_forward(3, H, W, win, self.color.data_ptr(), gt.data_ptr(), self.ssim_dm.data_ptr(),
                                         self.ssim_sum.data_ptr(), s), "ssim_fwd")
            N.check(lib.mom_ssim_backward(3, H, W, win, self.color.data_ptr(), gt.data_ptr(), self.ssim_dm.data_ptr(),
                                          -lam / n, None, self.dimg.data_ptr(), s), "ssim_bwd")
        gr = N.MomRasterGrads()
        gr.dL_dmeans2D, gr.dL_dcolors, gr.dL_dopacity = self.g2d.data_ptr(), self.gcol.data_ptr(), self.gop.data_ptr()
        gr.dL_dmeans3D, gr.dL_dcov3D = self.gxyz.data_ptr(), self.gcov.data_ptr()
        gr.dL_dsh, gr.dL_dsh_rest = self.gdc.data_ptr(), self.grest.data_ptr()
        gr.dL_dscales, gr.dL_drotations = self.gsc.data_ptr(), self.grot.data_ptr()
        if stats:
            # train_4DGS.py:266 in the projection backward's epilogue; a step whose binning overflowed leaves them alone (the replay
            # makes them), as mom_densify_stats does with the same word
            for t in (g.max_radii2D, g.xyz_gradient_accum, g.denom):
                if t.numel() != P or not t.is_contiguous() or t.dtype != torch.float32:
                    raise N.MomError("FusedCoarseStep: the densification accumulators must be contiguous float32, one per Gaussian")
            gr.stats_max_radii2D, gr.stats_grad_accum = g.max_radii2D.data_ptr(), g.xyz_gradient_accum.data_ptr()
            gr.stats_denom, gr.stats_skip_if_nonzero = g.denom.data_ptr(), self.flags.data_ptr()
        N.check(lib.mom_raster_backward(C.byref(a), self.radii.data_ptr(), self.geom.data_ptr(), self.binning.data_ptr(),
                                        self.cap, self.img.data_ptr(), self.dimg.data_ptr(), None, C.byref(gr), s), "raster_bwd")
        self.stats_done = bool(stats)
        for p, gbuf in ((g._xyz, self.gxyz), (g._features_dc, self.gdc), (g._features_rest, self.grest), (g._scaling, self.gsc),
                        (g._rotation, self.grot), (g._opacity, self.gop)):
            p.grad = gbuf
        sums = _TileSums(self.l1_part) if L1_PARTIALS else self.sums
        loss = LazyLoss(sums, None, None, self.ssim_sum if lam != 0 else None, lam, n)
        self.last = {"loss": loss, "mse_sum": _Lazy(sums, 1), "n": n}
        return loss, self.radii, self.g2d
