"""The training iteration as an explicit sequence of libmom4d launches -- no autograd graph, no per-op tensor allocation, no host
synchronisation.  FusedStep is the fine stage's, FusedCoarseStep the coarse stage's; _Step holds what they share.

FusedStep computes exactly what `train.Trainer.step` computes through `render()` + `loss.backward()` (the reference's
train_4DGS.py:149-297 with any batch_size on one GPU, stage "fine", L1 (+ lambda_dssim SSIM) loss, the shipped deformation config) and leaves the
same `.grad` tensors behind, so the optimizer step, the densification statistics and everything downstream are shared
with the autograd path.  `tests/test_fused_step_gpu.py` checks the two paths against each other.

Order of launches: hexplane_fwd -> deform_fwd -> activations_fwd -> preprocess / binning / sort / render_fwd -> l1 ->
render_bwd / preprocess_bwd -> activations_bwd -> deform_bwd (dx, dw) -> hexplane_bwd -> plane_reg -> adam.

A batch of B cameras (forward_backward takes one camera or a list; train_4DGS.py:172-229) runs them one after the other, forward
then backward of camera k, then k + 1, on the same scratch: memory does not grow with B.  The first camera's projection backward
stores the gradients exactly as a single camera's does, every later one ADDS (mom_raster_backward_acc) and merges its radii into
the first one's (max); every camera's gradient image carries 1 / B; the regulariser, the densification statistics and Adam run
once.  A list of one camera is the single-camera step, launch for launch.  Batches on the multi-GPU paths are out of scope.

Two model shapes have a fine step (step_features, fine_step): the shipped field, two HexPlane levels of 32 channels = 64 features, is
FusedStep's; two levels of 16 channels = 32 features (dnerf/eulerian_150_16) is FusedStep16's -- the same sequence on the 16-channel
kernels, one GPU only.
"""
import ctypes as C
import os

import torch

from . import _native as N
from . import ops
from .diff_gaussian_rasterization import _C as RC


class _Step:
    """What both steps share: the per-frame buffers, the sticky overflow word and what train.Trainer's overflow / replay protocol
    reads of it (flags, flag_ring, post_flag, next_tag, exact_next), the binning capacity, the full-image SSIM term and the loss
    value.  A subclass makes its per-Gaussian buffers in _per_gaussian and runs its iteration in forward_backward."""

    RING = 64
    keep_all_tiles = False            # True: bin whole rectangles like the reference (MomRasterArgs.keep_all_tiles; measurement only)
    HEADROOM, MARGIN = 1.5, 65536     # binning capacity = HEADROOM x an earlier frame's instance count + MARGIN

    def __init__(self, gaussians, opt, hyper, background):
        RC.refuse_if_deterministic(type(self).__name__)        # (and again in every step: _ensure)
        self.g, self.opt, self.hyper, self.bg = gaussians, opt, hyper, background
        self.P = -1
        self.lib = N.lib()
        self.last = {}
        self.dist = None      # parallel.DistContext (fine step: camera-batch or tile-row shard): set by parallel.attach()
        self.next_tag = 1     # what a step leaves in the overflow word if its binning overflows (Trainer numbers the steps)
        self.cap = 0
        self._resize_next = False
        self._bb = None            # what only the second and later cameras of a batch need (_batch_buffers)
        self._exact_step = False   # every camera of this step sizes its binning buffer from its own count (exact_next)
        self._key = self._frame = None

    def _rows(self, P):
        return P

    def _ensure(self, P, W, H, dev):
        """The step's buffers: the per-frame ones when the frame changes, the per-Gaussian ones (_per_gaussian) when P does."""
        RC.refuse_if_deterministic(type(self).__name__)
        pad = self._rows(P)
        key = (P, W, H, pad, dev)
        if key == self._key:
            return
        self._key = key
        self.P, self._wh = P, (W, H)
        new_frame = self._frame != (W, H, dev)
        if new_frame:
            self._frame = (W, H, dev)
            e = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)
            self.color, self.depth, self.dimg = e(3, H, W), e(1, H, W), e(3, H, W)
            self.img = torch.empty(self.lib.mom_raster_image_bytes(W, H), dtype=torch.uint8, device=dev)
            self.nr_dev = torch.zeros(1, dtype=torch.int32, device=dev)
            self.nr_host = torch.zeros(1, dtype=torch.int32).pin_memory()
            # Sticky overflow word (mom_raster_forward_render only ever sets bits in it).  The binning buffer is sized from
            # earlier frames without waiting for this frame's count; when a frame does not fit, its image and gradients are
            # truncated, the word becomes nonzero and stays so, and Adam / the densification statistics of that step and of every
            # later one are no-ops ON THE DEVICE (mom_adam_step / mom_densify_stats skip_if_nonzero) until the host -- which
            # runs several steps ahead and reads the word through flag_ring a few steps later -- clears it and replays the
            # skipped iterations with an exactly sized buffer (train.Trainer._recover).  Nothing truncated ever reaches the model.
            # (the word itself lives behind the radii: _set_bucket)
            self.flag_ring = torch.zeros(self.RING, dtype=torch.int32).pin_memory()
            # L1 sums in spare words of the image scratch's header, which the rasterizer forward clears at the start of every step
            # together with its tile counters: no memset of their own (mom_l1_loss_acc; the tile-row shard's logged loss)
            self.sums = self.img[(-self.img.data_ptr()) % 256:][:256].view(torch.float32)[8:10]
            # the compositing forward's L1 epilogue leaves one pair of sums per TILE here (MomRasterArgs.l1_partials): added up
            # only when somebody reads the loss (LazyLoss / _TileSums)
            # (a batch: one such array per camera, _l1_parts)
            self._l1_store = e(1, ((W + 15) // 16) * ((H + 15) // 16), 2)
            self.l1_part = self._l1_store[0]
            self.ssim_dm = None                  # SSIM term: made on first use (lambda_dssim may be switched on later)
            self.binning = None
        self._per_gaussian(P, pad, dev, new_frame)
        # the step after a change of P sizes its binning buffer from its own count (one sync); the buffer itself is kept if it fits
        self.cap = 0
        self._resize_next = False

    def _set_bucket(self, ibucket):
        """ibucket = [radii (P) | overflow word]: contiguous, so that a camera-batch shard agrees on both with ONE max-all-reduce.
        The word is sticky across steps: its value moves with it when P (and so its position) changes.  A new bucket comes zeroed."""
        old = getattr(self, "flags", None)
        P = ibucket.numel() - 1
        self.ibucket = ibucket
        self.radii, self.flags = ibucket[:P], ibucket[P:]
        if old is not None and old.device == ibucket.device and old.data_ptr() != self.flags.data_ptr():
            self.flags.copy_(old)

    def _begin(self, cam):
        """(P, W, H, device) of this iteration, with the buffers made for them."""
        g = self.g
        dev = g._xyz.device
        P = g._xyz.shape[0]
        W, H = int(cam.image_width), int(cam.image_height)
        self._ensure(P, W, H, dev)
        self._exact_step = self._resize_next
        if self._resize_next:                   # after a tile-row re-split, an overflow, or on request (exact_next)
            self.cap, self._resize_next = 0, False
        return P, W, H, dev

    @staticmethod
    def _cameras(cam):
        """forward_backward's camera argument as a list: one camera, or the cameras of a batch (all of one image size)."""
        cams = list(cam) if isinstance(cam, (list, tuple)) else [cam]
        if not cams:
            raise N.MomError("forward_backward needs at least one camera")
        wh = {(int(c.image_width), int(c.image_height)) for c in cams}
        if len(wh) != 1:
            raise N.MomError(f"the cameras of a batch must share one image size, got {sorted(wh)}")
        return cams

    def _l1_parts(self, B):
        """[B][tiles][2]: the compositing epilogue's per-tile L1 sums of every camera of the step (l1_part is camera 0's)."""
        if self._l1_store.shape[0] < B:
            self._l1_store = torch.empty((B,) + tuple(self._l1_store.shape[1:]), dtype=torch.float32, device=self._l1_store.device)
            self.l1_part = self._l1_store[0]
        return self._l1_store[:B]

    def _ssim_sums(self, B):
        """[B][slots]: the SSIM map sums of every camera of the step (ssim_sum is camera 0's)."""
        self._ssim_win()
        if self._ssim_store.shape[0] < B:
            self._ssim_store = torch.empty(B, N.SSIM_SUM_SLOTS, dtype=torch.float64, device=self._ssim_store.device)
            self.ssim_sum = self._ssim_store[0]
        return self._ssim_store[:B]

    def _batch_buffers(self, P, dev):
        """What only the second and later cameras of a batch need, made on first use: the camera's own radii (the merged ones live in
        ibucket) and a private d pts for its deformation backward (MomRasterAccum.dL_dmeans3D_copy)."""
        b = self._bb
        if b is None or b[0] != (P, dev):
            b = self._bb = ((P, dev), torch.zeros(P, dtype=torch.int32, device=dev), torch.empty(P, 3, dtype=torch.float32, device=dev))
        return b[1], b[2]

    def exact_next(self):
        """Size the binning buffer of the next step from that step's own instance count (one host sync): it cannot overflow."""
        self._resize_next = True

    def post_flag(self, slot):
        """Copy the overflow word to ring slot `slot` behind everything enqueued so far; the returned event tells when the
        slot is valid.  The word holds 0 or the tag of the FIRST step that overflowed since it was cleared."""
        self.flag_ring[slot:slot + 1].copy_(self.flags, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        return ev

    def gather_moments(self):
        """Before an iteration that reads or restructures the optimizer state (FusedStep: sharded Adam).  Here the state is whole."""

    def _raster_forward(self, a, P, W, H, dev, s, radii=None, first=True):
        """Projection + binning, then the compositing into color / depth, its overflow into the sticky word.  Async: the binning
        capacity comes from an earlier iteration's instance count (cap == 0: from this frame's own, one sync).  radii: where the
        projection leaves this camera's radii (default: the step's merged ones); first: the first camera of the step -- a later one
        may grow the binning buffer but not shrink it, and after exact_next() sizes it from its own count too."""
        lib = self.lib
        radii = self.radii if radii is None else radii
        # an earlier iteration's instance count (whichever copy landed last: a sizing hint, read without blocking)
        prev_R = int(self.nr_host[0])
        N.check(lib.mom_raster_forward_geometry(C.byref(a), self.geom.data_ptr(), self.img.data_ptr(), radii.data_ptr(),
                                                self.nr_dev.data_ptr(), self.nr_host.data_ptr(), s), "raster_geometry")
        if self.cap == 0 or self._exact_step:   # first call: size exactly (one sync)
            torch.cuda.current_stream().synchronize()
            prev_R = int(self.nr_host[0])
        want = max(prev_R, int(prev_R * self.HEADROOM) + self.MARGIN)
        if self.binning is None or want > self._bin_cap or (first and want < self._bin_cap // 4):
            self._bin_cap = want
            self.binning = torch.empty(lib.mom_raster_binning_bytes(P, W, H, want), dtype=torch.uint8, device=dev)
        self.cap = self._bin_cap          # the capacity every launch of this step is told (cap == 0 above: "size exactly")
        N.check(lib.mom_raster_forward_render(C.byref(a), self.geom.data_ptr(), self.binning.data_ptr(), self.cap,
                                              self.img.data_ptr(), self.color.data_ptr(), self.depth.data_ptr(),
                                              self.flags.data_ptr(), s), "raster_render")

    def _ssim_win(self):
        """The SSIM window; the derivative maps and the map sum (mom_ssim_forward) are made on first use."""
        if self.ssim_dm is None:
            (W, H), dev = self._wh, self.color.device
            self.ssim_dm = torch.empty((3, 3, H, W), dtype=torch.float32, device=dev)
            self._ssim_store = torch.empty(1, N.SSIM_SUM_SLOTS, dtype=torch.float64, device=dev)
            self.ssim_sum = self._ssim_store[0]                                                # [0] = the sum
        return ops._ssim_window()

    def _ssim_full(self, gt, lam, s, k=0, B=1):
        """loss += lambda_dssim * (1 - ssim(image, gt))  (train_4DGS.py:222-223) over the whole image: its gradient is added
        into dimg, the map's sum is left in ssim_sum.  Camera k of a batch of B: ssim() of the [B,3,H,W] stack is the mean over all
        of its elements, so the gradient carries 1 / B and the sum goes to the camera's own row of _ssim_sums."""
        win, (W, H), n = self._ssim_win(), self._wh, self.color.numel()
        sums = self.ssim_sum if B == 1 else self._ssim_sums(B)[k]
        N.check(self.lib.mom_ssim_forward(3, H, W, win, self.color.data_ptr(), gt.data_ptr(), self.ssim_dm.data_ptr(),
                                          sums.data_ptr(), s), "ssim_fwd")
        N.check(self.lib.mom_ssim_backward(3, H, W, win, self.color.data_ptr(), gt.data_ptr(), self.ssim_dm.data_ptr(),
                                           -lam / (n * B), None, self.dimg.data_ptr(), s), "ssim_bwd")

    def _set_grads(self):
        """.grad of the six Gaussian parameters = the step's own gradient buffers (they persist across steps)."""
        g = self.g
        for p, gbuf in ((g._xyz, self.gxyz), (g._features_dc, self.gdc), (g._features_rest, self.grest), (g._scaling, self.gsc),
                        (g._rotation, self.grot), (g._opacity, self.gop)):
            p.grad = gbuf

    def _loss(self, l1, reg, lam, n, B=1):
        """(loss, radii, screen-space gradient) of the step; the loss is formed when read (LazyLoss).  l1: a device scalar, or
        None for the per-tile sums the compositing epilogue left.  n: elements of one image; a batch of B cameras is the mean over
        all B n of them (train_4DGS.py:189-229), its sums added camera by camera, tile by tile, in a fixed order."""
        ssim_sum = self.ssim_sum if lam != 0 else None
        if B > 1:
            sums, n = _TileSums(self._l1_parts(B).view(-1, 2)), n * B
            ssim_sum = _BatchSum(self._ssim_sums(B)) if lam != 0 else None
        else:
            sums = _TileSums(self.l1_part) if l1 is None else self.sums
        loss = LazyLoss(sums if l1 is None else None, l1, reg, ssim_sum if lam != 0 else None, lam, n)
        self.last = {"loss": loss, "mse_sum": _Lazy(sums, 1), "n": n}       # float(last["mse_sum"]): formed when read
        return loss, self.radii, self.g2d


def step_features(dn):
    """Width of the HexPlane feature row the fused fine step runs a deformation net on, or 0 if it cannot take the model: 64 for the
    shipped field (two levels of 32 channels, Deformation._fusable), 32 for two levels of 16 channels inside the one-launch field
    kernel's resolution limit (dnerf/eulerian_150_16, Deformation._field16_fusable).  Pure: asks the module, needs no GPU and no
    library."""
    if dn._fusable():
        return 64
    if dn._field16_fusable():
        return 32
    return 0


class FusedStep(_Step):
    """One fine-stage iteration (module docstring) of the shipped model: two HexPlane levels of 32 channels, F = 64 features.  Every
    other model is refused, a 16 x 2 one too: that one is FusedStep16's, and fine_step() picks between the two."""

    WIDTHS = (64,)        # the feature widths (step_features) this class takes

    def __init__(self, gaussians, opt, hyper, background):
        dn = gaussians._deformation.deformation_net
        self.F = step_features(dn)
        if self.F not in self.WIDTHS:
            raise N.MomError("%s needs the shipped deformation configuration (W=64, D=0, no_do, no_dshs) on two HexPlane levels of %s "
                             "(fused_step.fine_step picks the step for a model: 32 channels FusedStep, 16 channels with every plane "
                             "resolution <= %d FusedStep16)" % (type(self).__name__, " or ".join("%d channels" % (w // 2) for w in self.WIDTHS),
                                                               dn.FIELD16_MAX_RES))
        if self.F != 64:      # feat / dfeat rows are F floats wide; the shipped model keeps the class's table as it is
            self._ROW_BUFFERS = tuple((name, self.F if name in ("feat", "dfeat") else cols, padded)
                                      for name, cols, padded in type(self)._ROW_BUFFERS)
        super().__init__(gaussians, opt, hyper, background)

    # ------------------------------------------------------------------ buffers (re-made when P changes)
    def _rows(self, P):
        """Rows of the per-Gaussian buffers a tile-row shard gathers: world x S (DistContext.slice_rows), else P."""
        dc = self.dist
        return dc.world * dc.slice_rows(P) if (dc is not None and dc.mode == "tile-row") else P

    def _per_gaussian(self, P, pad, dev, new_frame):
        """Per-Gaussian storage is CAPACITY based: a densify / prune round changes P by a few percent every
        hundred iterations (train_4DGS.py:264-290), and re-making fifty buffers each time sent the step after every round back to
        the driver for fresh memory (tools/probe/c5_leg.py: the first round of a process cost 148 ms instead of 13 and the steps
        behind it ran at 59 instead of 94 per second until the new pages had been touched).  Storage is re-made only when the
        model outgrows it (then with a quarter of headroom) or shrinks below half of it; otherwise the attributes below are
        re-sliced views of the same memory."""
        self._pad = pad
        e = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)
        cap = getattr(self, "_rows_cap", 0)
        if new_frame or pad > cap or 2 * pad < cap:
            grew = not new_frame and cap and pad > cap
            cap = self._rows_cap = pad + pad // 4 if grew else pad
            st = self._store = {name: e(cap, cols) for name, cols, _ in self._ROW_BUFFERS}
            st["radii"] = torch.zeros(cap + 1, dtype=torch.int32, device=dev)      # + the sticky overflow word behind the P radii
            st["early"] = e(59 * cap + 4 * self._world())                          # + the screen-space gradients behind the 56 P (sharded Adam: behind world x chunk)
            st["pflat"] = None                                                     # sharded Adam: the appearance parameters' flat home (_rehome)
            st["loc"] = (e(cap, 3), e(cap, 4))
            self.geom = torch.empty(self.lib.mom_raster_geom_bytes(cap), dtype=torch.uint8, device=dev)
            self.dh_scratch = torch.empty(self.lib.mom_deform_backward_scratch_bytes(cap), dtype=torch.uint8, device=dev)
        st = self._store
        # (the gathered buffers of a tile-row shard carry world x S >= P rows; every kernel reads the first P)
        for name, _, padded in self._ROW_BUFFERS:
            setattr(self, name, st[name][:pad if padded else P])
        self._set_bucket(st["radii"][:P + 1])
        # parameter gradients (persist across steps; .grad points at them).  They live in two flat buckets so that a
        # multi-GPU run all-reduces them in place, without packing: `early` (final once the activation backward has run:
        # SH, scaling, rotation, opacity = 56 floats per Gaussian) and `late` (xyz + the deformation field, final only
        # after the HexPlane backward; made in _deform_grads).
        # (behind the 56 P: the screen-space gradients, 3 P -- the densification statistics' input, summed over a camera-batch
        # shard's ranks in the same all-reduce)
        # sharded Adam (DistContext.shard_adam): the 56 P appearance gradients are cut into world chunks of `_chunk` elements for the
        # reduce-scatter, so the bucket's appearance part is padded to world x chunk and the screen-space gradients sit behind THAT
        dc = self.dist
        self._chunk = dc.chunk(56 * P) if (dc is not None and getattr(dc, "shard_adam", False)) else 0
        app = self._world() * self._chunk if self._chunk else 56 * P
        self.early_bucket = st["early"][:app + 3 * P]
        self.app_flat = self.early_bucket[:app]
        self.early = self.early_bucket[:56 * P]
        self.g2d_flat = self.early_bucket[app:]
        self.g2d = self.g2d_flat.view(P, 3)
        self._cut = cut = [0, 3 * P, 48 * P, 51 * P, 55 * P, 56 * P]
        seg = lambda i: self.early[cut[i]:cut[i + 1]]
        self.gdc, self.grest = seg(0).view(P, 1, 3), seg(1).view(P, 15, 3)
        self.gsc, self.grot, self.gop = seg(2).view(P, 3), seg(3).view(P, 4), seg(4).view(P, 1)
        self._loc = (st["loc"][0][:P], st["loc"][1][:P])

    # per-Gaussian float buffers: (attribute, floats per row, sized for a tile-row shard's padded row count)
    _ROW_BUFFERS = (("feat", 64, False), ("a0", 64, False), ("dfeat", 64, False), ("pts", 3, True), ("sc_d", 3, False),
                    ("rot_d", 4, True), ("sc", 3, True), ("rot", 4, True), ("op", 1, True), ("gcol", 3, False),
                    ("gcov", 6, False))

    def _world(self):
        return self.dist.world if self.dist is not None else 1

    _APP_SHAPES = ((1, 3), (15, 3), (3,), (4,), (1,))

    def _app_params(self):
        g = self.g
        return [g._features_dc, g._features_rest, g._scaling, g._rotation, g._opacity]

    def _rehome(self):
        """Sharded Adam: the five appearance parameters live in ONE flat buffer laid out like their gradient bucket
        ([f_dc 3P | f_rest 45P | scaling 3P | rotation 4P | opacity P], padded to world x chunk), so that the all-gather of the
        updated parameters is in place.  A parameter that is not there (first step, after a densify / prune round replaced it) is
        copied in and its .data pointed at its slice; the Parameter objects -- and with them the optimizer's state -- stay."""
        P, st = self.P, self._store
        need = self._world() * self._chunk
        flat = st.get("pflat")
        if flat is None or flat.numel() < need or flat.device != self.early.device:
            flat = st["pflat"] = torch.empty(56 * self._rows_cap + 4 * self._world(), dtype=torch.float32, device=self.early.device)
        self.pflat = flat[:need]
        for p, a, b, shp in zip(self._app_params(), self._cut[:-1], self._cut[1:], self._APP_SHAPES):
            v = self.pflat[a:b].view((P,) + shp)
            if p.data_ptr() != v.data_ptr():
                v.copy_(p.data)
                p.data = v

    def gather_moments(self):
        """Before an iteration that reads or restructures the optimizer state: every rank gets the moments of every slice (sharded
        Adam keeps only its own up to date)."""
        dc = self.dist
        if dc is None or not getattr(dc, "shard_adam", False) or self.P <= 0 or not self._chunk:
            return
        if self.g._xyz.shape[0] != self.P:
            return                       # the model was restructured since the last step: its state is whole (the round gathered first)
        dc.gather_moments(self.g.optimizer, self._app_params(), self._cut, self._chunk)

    OVERLAP_DW = os.environ.get("MOM_OVERLAP_DW", "1") != "0"     # the MLP weight-gradient kernel on a second stream, beside the HexPlane backward
    EARLY_ADAM = os.environ.get("MOM_EARLY_ADAM", "1") != "0"     # the appearance parameters' Adam on that stream, beside the MLP backward
    side = None

    def _hex_scratch_for(self, hp, rows, dev):
        """Scratch of the two-pass HexPlane backward for `rows` points (common-factor rows + the time lines): kept while it is
        large enough and not more than twice too large."""
        need = self.lib.mom_hexplane_backward_scratch_bytes(C.byref(hp), rows)
        t = getattr(self, "_hex_scratch", None)
        if t is None or t.device != dev or t.numel() < need or t.numel() > 2 * need + (1 << 20):
            grow = t is not None and t.device == dev and t.numel() < need
            self._hex_scratch = torch.empty(need + need // 4 if grow else need, dtype=torch.uint8, device=dev)

    def _gacc_view(self, P, W, H):
        """The per-Gaussian record of the compositing backward inside the geometry scratch, as a flat fp32 tensor."""
        lay = N.MomRasterLayout()
        self.lib.mom_raster_layout(P, W, H, 0, C.byref(lay))
        base = self.geom[(-self.geom.data_ptr()) % 256:]
        return base[lay.geom_gacc:lay.geom_gacc + P * 4 * N.GACC_FLOATS].view(torch.float32)

    def _deform_grads(self):
        """Flat zero-able gradient storage for the deformation field (planes channel-last + live MLP tensors)."""
        dn = self.g._deformation.deformation_net
        planes = [p for lv in dn.grid.grids for p in lv]
        mlp = dn._fused_params()
        key = tuple(p.data_ptr() for p in planes + mlp) + (self.P, self._pad, self._rows_cap)
        if getattr(self, "_dg_key", None) != key:
            n = self._dg_n = sum(p.numel() for p in planes + mlp)
            store = getattr(self, "_dg_store", None)
            if store is None or store.numel() != 4 + n + 3 * self._rows_cap or store.device != planes[0].device:
                store = self._dg_store = torch.zeros(4 + n + 3 * self._rows_cap, dtype=torch.float32, device=planes[0].device)
            # [loss sums (4) | field gradients (n) | xyz gradients (3 pad)]: the four floats in front carry a tile-row shard's loss
            # sums (sum |d|, sum d^2, sum of the SSIM map over the rank's own rows) into the SAME all-reduce as the field
            # gradients -- a collective of their own cost the step ~20 us of stream hand-over and four small launches
            self._dg_all = store[:4 + n + 3 * self._pad]
            self._tr_sums = self._dg_all[:4]
            self._dg_flat = self._dg_all[4:]                                                                # the `late` bucket
            self.gxyz_rows = self._dg_flat[n:].view(self._pad, 3)
            self.gxyz = self.gxyz_rows[:self.P]
            off, self._dg_planes, self._dg_mlp = 0, [], []
            for p in planes:       # same channel-last strides as the parameter
                st = ops.plane_storage(p)
                v = self._dg_flat[off:off + p.numel()].view(st.shape).permute(2, 0, 1).unsqueeze(0)
                self._dg_planes.append(v)
                off += p.numel()
            for p in mlp:
                self._dg_mlp.append(self._dg_flat[off:off + p.numel()].view(p.shape))
                off += p.numel()
            self._dg_key = key
        return planes, mlp

    # ------------------------------------------------------------------ one iteration (forward + backward)
    def forward_backward(self, cam, delta_scale=1, early_adam=None):
        """cam: one camera, or the list of a batch's cameras (module docstring).  early_adam: callable(list of parameters) or None
        -- see EARLY_ADAM below; the caller promises that its optimizer step for this iteration follows with nothing in between
        that reads or replaces those parameters."""
        g, lib, s = self.g, self.lib, N.current_stream()
        cams = self._cameras(cam)
        B, cam = len(cams), cams[0]
        if B > 1 and self.dist is not None:
            raise N.MomError("FusedStep: a batch of cameras on the multi-GPU paths is not supported (one camera per rank)")
        if self.F == 32 and self.dist is not None:
            raise N.MomError("FusedStep16 on 16-channel fields: single GPU only")
        P, W, H, dev = self._begin(cam)
        sharded = bool(self._chunk) and early_adam is not None and self.EARLY_ADAM     # this iteration takes the sharded-Adam path
        if self._chunk:
            self._rehome()
        dn = g._deformation.deformation_net
        field = dn.grid
        planes, mlp = self._deform_grads()
        xyz, f_dc, f_rest, scal, rot, opac = ops.gaussian_params(g, "FusedStep")
        flow = g._scene_flow if g._scene_flow.is_contiguous() else g._scene_flow.contiguous()
        lam = float(self.opt.lambda_dssim)
        order = field._processing_order(xyz)
        optr = None if order is None else order.data_ptr()
        porders = field._plane_orders(xyz)           # per-space-plane orders of the two-pass HexPlane backward

        # ---- deformation field
        # the descriptors only hold pointers and shapes: rebuilt when a parameter or the aabb moves, not every iteration
        dkey = (self._dg_key, tuple(field.aabb_host()))
        if getattr(self, "_desc_key", None) != dkey:
            levels = [list(lv) for lv in field.grids]
            gl, k = [], 0
            for lv in levels:
                gl.append(self._dg_planes[k:k + 6])
                k += 6
            hp, keep = ops._hexplane_desc([[p.detach() for p in lv] for lv in levels], field.aabb, gl, aabb_host=field.aabb_host())
            md = ops.DeformMLPFunction._desc([p.detach() for p in mlp], self._dg_mlp)
            self._desc = (hp, keep, md)
            self._desc_key, self._reg_arr = dkey, None
        hp, keep, md = self._desc
        # ---- second stream, first job: clear the deformation field's gradient bucket and run the plane regularisers (value +
        # gradient; they depend on the planes only, so they need not wait for the backward) while this stream renders.  The
        # backward's kernels then ADD into what the regulariser left; this stream waits for the event before its first write
        # to the bucket (the projection backward's d xyz).
        dc = self.dist
        reg_scale = 1.0 / dc.world if dc is not None else 1.0
        # each on its own check: `side` is a public attribute a caller may have set
        if self.side is None:
            self.side = torch.cuda.Stream(device=dev)
        if getattr(self, "regacc", None) is None:
            self.regacc = torch.zeros(1, dtype=torch.float32, device=dev)
        hy = self.hyper
        reg = None
        # (everything on the second stream goes there through its raw handle -- libmom4d's launches, mom_zero_async, the ordering
        # calls of csrc/stream_order.hip: entering a torch stream context, a wait_stream and an event cost ~10 us of host time each,
        # and at config 1 the host paces the step)
        side = self.side.cuda_stream
        ops.stream_wait_stream(side, s)
        ops.zero_async(self._dg_all, side)
        # the compositing backward's accumulator record too (MomRasterArgs.accum_cleared): its last reader, the previous
        # step's projection backward, is behind this stream's wait above
        gk = (P, W, H, self.geom.data_ptr())
        if getattr(self, "_gacc_cache", (None,))[0] != gk:
            self._gacc_cache = (gk, self._gacc_view(P, W, H))
        ops.zero_async(self._gacc_cache[1], side)
        if hy.time_smoothness_weight != 0:
            rkey = (hy.time_smoothness_weight, hy.plane_tv_weight, hy.l1_time_planes, reg_scale)
            if self._reg_arr is None or self._reg_arr[0] != rkey:
                arr = (N.MomRegPlane * len(planes))()
                for i, p in enumerate(planes):
                    st, gs = ops.plane_storage(p.detach()), ops.plane_storage(self._dg_planes[i])
                    arr[i].plane, arr[i].grad = st.data_ptr(), gs.data_ptr()
                    arr[i].H, arr[i].W = st.shape[0], ops._reg_row_units(st)      # rows in units of 32 floats: W, or W / 2 at 16 channels
                    tplane = (i % 6) in (2, 4, 5)
                    arr[i].w_smooth = hy.time_smoothness_weight if tplane else hy.plane_tv_weight
                    arr[i].w_l1 = hy.l1_time_planes if tplane else 0.0
                    arr[i].grad_scale = reg_scale      # identical on every rank: the sum over ranks restores it
                self._reg_arr = (rkey, arr)
            arr = self._reg_arr[1]
            ops.zero_async(self.regacc, side)
            N.check(lib.mom_plane_regulation_acc(arr, len(planes), self.regacc.data_ptr(), side), "plane_reg")
            reg = self.regacc
        ops.stream_mark(ops.MARK_BUCKET, side)
        # the field's processing orders, if their refresh is due within a few steps: sorted on the second stream from here on, beside
        # this step's forward and backward (scene/hexplane.py: prefetch_if_due)
        if dc is None or dc.mode == "camera":
            field.prefetch_if_due(xyz, side)
        # ---- the cameras, one after the other: forward and backward of camera k, then k + 1, on the same scratch
        for k, cam in enumerate(cams):
            view, proj, campos, gt = cam.device_tensors(dev)
            time = float(cam.time)
            coef = float(delta_scale * cam.frame_num)
            radii_k, d_pts, gmark = self.radii, self.gxyz, None
            if k > 0:
                # the camera's own radii and d pts (the merged radii / the running sum of d xyz stay in the buckets), and the
                # compositing accumulator cleared again -- on the second stream, behind camera k - 1's projection backward, its
                # last reader (this stream has joined the second one at the end of that camera)
                radii_k, d_pts = self._batch_buffers(P, dev)
                ops.stream_wait_stream(self.side.cuda_stream, s)
                ops.zero_async(self._gacc_cache[1], self.side.cuda_stream)
                gmark = ops.next_ring_mark(self.side.cuda_stream)
            # HexPlane lookup + MLP + the activations (exp / normalize / sigmoid) in one kernel (csrc/deform_field.hip)
            dc = self.dist
            sl = None
            if dc is not None and dc.mode == "tile-row":
                # the deformation field is half of a step and does not care which rank computes which Gaussian: every rank takes a
                # contiguous slice [g0, g1) of them, forward and backward, and the ranks all-gather the deformed state (what the
                # replicated projection needs of ALL Gaussians: 15 floats each) while nothing else is in flight
                S = dc.slice_rows(P)
                g0 = min(P, dc.rank * S)
                g1 = min(P, g0 + S)
                sl = (S, g0, g1)
                # The five tensors of the deformed state are gathered IN PLACE, each in its own [world * S, k] array (the slice's
                # field kernel writes this rank's rows directly), as ONE grouped submission on the direct RCCL transport
                # (ncclGroupStart / End: one launch).  Round 5 packed them into one slab per rank for a single torch.distributed call
                # (40-50 us of host each) and paid five strided copies behind the gather at every world size; with the collectives
                # behind the C ABI a call costs 0.6 us and the copies are gone.  (torch.distributed, the fallback and the CPU tests'
                # transport, issues the five gathers one after the other.)
                if g1 > g0:
                    v = lambda t: t[g0:g1]
                    so = field._slice_order(xyz, g0, g1)
                    lines_kept = ops.field_forward(hp, md, g1 - g0, v(xyz), time, so, v(scal), v(rot), v(flow), coef, v(self.pts), v(self.sc_d),
                                      v(self.rot_d), v(self.feat), v(self.a0), v(opac), v(self.sc), v(self.rot), v(self.op), s)
                grp = None
                if hasattr(dc, "group"):
                    with dc.group() as grp:
                        dc.start_gather([self.pts, self.sc, self.rot, self.op, self.rot_d], S)
                else:
                    dc.start_gather([self.pts, self.sc, self.rot, self.op, self.rot_d], S)
                if grp is not None and getattr(grp, "work", None) is not None:
                    dc._pending.append(grp.work)
                dc.finish()
            elif self.F == 32:
                # two levels of 16 channels: the one-launch field of csrc/deform_field16.hip; it stages no time lines.  Its raw outputs
                # only: the activated copies are torch's exp / normalize / sigmoid, as in FusedRender and for the same reason -- the
                # autograd path of such a model is op by op, and the kernel's expf / quaternion norm differ from torch's in last bits,
                # which moves (pixel, splat) pairs across the compositing thresholds (measured on the tiny scene: 43 of 6000 Gaussians'
                # d xyz up to 1.1e-3 of the tensor's scale away from the autograd path's; with torch's activations the image is that
                # path's bit for bit and every gradient within 5e-6: DESIGN 3.10)
                ops.field16_forward(hp, md, P, xyz, time, order, scal, rot, flow, coef, self.pts, self.sc_d, self.rot_d, self.feat, self.a0,
                                    None, None, None, None, s)
                torch.exp(self.sc_d, out=self.sc)
                torch.nn.functional.normalize(self.rot_d, out=self.rot)
                torch.sigmoid(opac, out=self.op)
                lines_kept = False
            else:
                lines_kept = ops.field_forward(hp, md, P, xyz, time, order, scal, rot, flow, coef, self.pts, self.sc_d, self.rot_d, self.feat, self.a0,
                                  opac, self.sc, self.rot, self.op, s)
            # ---- rasterizer forward (async: capacity from the previous iterations, checked below)
            a = ops.raster_args(cam, view, proj, campos, self.bg, P, g.active_sh_degree, self.pts, f_dc, f_rest, self.op, self.sc, self.rot,
                                False, 1.0, False, self.keep_all_tiles)
            a.accum_cleared = 1                     # on the second stream, above
            # L1 (its gradient image and its sums) in the compositing kernel's epilogue, one pair of sums per tile.  A tile-row shard too,
            # unless its forward renders a halo (SSIM term): the kernel runs this rank's tiles only, and the rank adds up ITS rows
            tr_rows = dc is not None and dc.mode == "tile-row"
            l1_scaled = False
            fuse_l1 = not tr_rows or lam == 0
            if fuse_l1:
                a.l1_target, a.l1_grad, a.l1_partials = gt.data_ptr(), self.dimg.data_ptr(), self._l1_parts(B)[k].data_ptr()
                # camera-batch shard: the batch loss is the mean over the ranks' cameras, every gradient carries 1 / world (below)
                # -- in the epilogue itself when the loss is L1 alone (with the SSIM term the whole gradient image is scaled once, below)
                l1_scaled = dc is not None and dc.mode == "camera" and lam == 0
                a.l1_grad_scale = 1.0 / dc.world if l1_scaled else 0.0
                if B > 1:
                    a.l1_grad_scale = 1.0 / B           # the batch loss is the mean over its cameras (the SSIM term: _ssim_full)
            a.overflow_tag = self.next_tag          # what this step leaves in the sticky word if its binning overflows (Trainer numbers the steps)
            rows = fwd_rows = None
            if dc is not None and dc.mode == "tile-row":
                # every rank renders this same camera, restricted to its rows of 16-pixel tiles.  With the SSIM term the forward
                # also renders one tile row of halo on each side: the 11x11 window makes an owned pixel depend on map pixels up to
                # 5 rows outside, and those on image pixels up to 10 rows outside -- all inside the 16-row halo, so nothing is
                # exchanged (the neighbour composites the same rows to the same bits).  The backward covers the own rows only.
                gy = (H + 15) // 16
                rows = dc.rows(gy)
                halo = 1 if (lam != 0 and rows[1] > rows[0]) else 0
                fwd_rows = (max(rows[0] - halo, 0), min(rows[1] + halo, gy))
                a.tile_row0, a.tile_row1 = fwd_rows
            self._raster_forward(a, P, W, H, dev, s, radii_k, k == 0)
            early_works = []                        # camera-batch shard: what the early Adam launch must see reduced (below)
            if dc is not None and dc.mode != "camera":
                early_works.append(dc.start(self.flags, "max"))         # every rank skips (and later replays) the same steps
                # (a camera-batch shard agrees on the word together with the radii, behind its own backward: below)
            # ---- loss: L1 (+ its gradient image) ; regulariser value and gradient
            n = self.color.numel()
            if not fuse_l1:
                N.check(lib.mom_l1_loss_acc(n, self.color.data_ptr(), gt.data_ptr(), self.dimg.data_ptr(), self.sums.data_ptr(), s), "l1")
            # camera-batch shard: the batch loss is the mean over the ranks' cameras (train_4DGS.py:189-229), so every
            # gradient carries 1/world and the all-reduces below are plain sums (1/2, 1/4, 1/8 are exact in fp32)
            inv_world = 1.0 / dc.world if (dc is not None and dc.mode == "camera") else 1.0
            # tile-row shard: the ranks' deformation gradients are SUMMED (each holds its slice's share); the regulariser's gradient,
            # which every rank computes in full, must enter that sum once
            reg_scale = 1.0 / dc.world if dc is not None else 1.0
            if lam != 0:
                # loss += lambda_dssim * (1 - ssim(image, gt))  (train_4DGS.py:222-223): its gradient is added into dimg
                if rows is None:
                    self._ssim_full(gt, lam, s, k, B)
                elif rows[1] > rows[0]:
                    # the slab this rank rendered (own rows + halo), as a pitched view of the full buffers: map rows of the own
                    # tile rows count toward the sum; derivative maps are kept 5 rows beyond them (up to the image's own edges,
                    # where zero padding is the reference's behaviour) and are zero elsewhere
                    win = self._ssim_win()
                    ys0, ys1 = fwd_rows[0] * 16, min(H, fwd_rows[1] * 16)
                    y0, y1 = rows[0] * 16, min(H, rows[1] * 16)
                    off = ys0 * W * 4
                    N.check(lib.mom_ssim_forward_slab(3, ys1 - ys0, W, H * W, y0 - ys0, y1 - ys0, max(0, y0 - 5) - ys0,
                                                      min(H, y1 + 5) - ys0, win, self.color.data_ptr() + off, gt.data_ptr() + off,
                                                      self.ssim_dm.data_ptr() + off, self.ssim_sum.data_ptr(), s), "ssim_fwd_slab")
                    N.check(lib.mom_ssim_backward_slab(3, ys1 - ys0, W, H * W, win, self.color.data_ptr() + off, gt.data_ptr() + off,
                                                       self.ssim_dm.data_ptr() + off, -lam / n, None, self.dimg.data_ptr() + off, s),
                            "ssim_bwd_slab")
                else:
                    self._ssim_win()
                    self.ssim_sum.zero_()
            if dc is not None and dc.mode == "camera" and not (fuse_l1 and l1_scaled):
                self.dimg.mul_(inv_world)            # (L1 alone: the forward's epilogue wrote the gradient image with the factor in it)
            # ---- rasterizer backward
            # the gradient bucket is cleared and holds the regulariser's share (a later camera: its accumulator record is cleared)
            ops.stream_wait_mark(s, ops.MARK_BUCKET if k == 0 else gmark)
            gr = ops.raster_grads(self.g2d, self.gcol, self.gop, self.gxyz, self.gcov, self.gdc, self.grest, self.gsc, self.grot)
            # scale / rotation / opacity gradients leave the projection backward already through exp / normalize / sigmoid
            # (MomRasterGrads.act_rotations_raw): no activation-backward launch behind it
            gr.act_rotations_raw = self.rot_d.data_ptr()
            if dc is not None and dc.mode == "camera":
                # the deformation backward still reads this rank's own d_sc / d_rot while the bucket that holds them is being reduced in
                # place: its private copies (7 floats per Gaussian) come out of the same kernel
                gr.dL_dscales_copy, gr.dL_drotations_copy = self._loc[0].data_ptr(), self._loc[1].data_ptr()
            if k > 0:
                # cameras 2..B ADD their gradients to the first one's and merge their radii into its (train_4DGS.py:203-204,217-229);
                # the deformation backward of THIS camera reads its own d pts / d scales / d rotations, private plain stores
                gr.dL_dscales_copy, gr.dL_drotations_copy = self._loc[0].data_ptr(), self._loc[1].data_ptr()
                acc = N.MomRasterAccum()
                acc.dL_dmeans3D_copy, acc.radii_max = d_pts.data_ptr(), self.radii.data_ptr()
                N.check(lib.mom_raster_backward_acc(C.byref(a), radii_k.data_ptr(), self.geom.data_ptr(), self.binning.data_ptr(),
                                                    self.cap, self.img.data_ptr(), self.dimg.data_ptr(), None, C.byref(gr),
                                                    C.byref(acc), s), "raster_bwd_acc")
            elif rows is None:
                N.check(lib.mom_raster_backward(C.byref(a), self.radii.data_ptr(), self.geom.data_ptr(), self.binning.data_ptr(),
                                                self.cap, self.img.data_ptr(), self.dimg.data_ptr(), None, C.byref(gr), s), "raster_bwd")
            else:
                # tile-row shard: the compositing backward covers this rank's rows only (dimg outside them is never read); the
                # per-Gaussian record it leaves is summed over the ranks, after which the projection backward -- linear in that
                # record -- and everything downstream give the same gradients on every rank, with nothing left to exchange
                if hasattr(dc, "rebalance_due") and dc.rebalance_due():
                    # instance counts per tile row of the rows this rank owns -> agreed weights for the next splits; after a
                    # re-split the local instance count can jump, so the next step sizes its binning buffer exactly again
                    gx_ = (W + 15) // 16
                    lay = N.MomRasterLayout()
                    lib.mom_raster_layout(P, W, H, 0, C.byref(lay))
                    base = self.img[(-self.img.data_ptr()) % 256:]
                    per_row = base[lay.img_tile_counts:lay.img_tile_counts + gx_ * gy * 4].view(torch.int32).view(gy, gx_).sum(1).float()
                    own = torch.zeros_like(per_row)
                    own[rows[0]:rows[1]] = per_row[rows[0]:rows[1]]
                    if dc.rebalance_rows(own):
                        # the local instance count can jump with the new rows: size the NEXT step's buffer exactly.  This step's
                        # backward below still runs on the buffer (and capacity) its forward filled.
                        self._resize_next = True
                a.tile_row0, a.tile_row1 = rows          # own rows only (the forward may have covered a halo)
                N.check(lib.mom_raster_backward_render(C.byref(a), self.geom.data_ptr(), self.binning.data_ptr(), self.cap,
                                                       self.img.data_ptr(), self.dimg.data_ptr(), None, s), "raster_bwd_render")
                dc.start(self._gacc_view(P, W, H), "sum")
                dc.finish()
                N.check(lib.mom_raster_backward_geometry(C.byref(a), self.radii.data_ptr(), self.geom.data_ptr(), C.byref(gr), s),
                        "raster_bwd_geometry")
            if dc is not None and dc.mode == "camera":
                # densification statistics (train_4DGS.py:203-204,227-229): largest radius, mean 2-D gradient
                # (this rank's backward has read its OWN radii by now; the overflow word rides in the same integer bucket.  Every
                # torch.distributed call costs the host 40-50 us and the host paces a rank: three collectives per step, not five)
                early_works.append(dc.start(self.ibucket, "max"))
            d_sc, d_rot = self.gsc, self.grot       # also the gradients w.r.t. the MLP's scale / rotation outputs
            if k > 0:
                d_sc, d_rot = self._loc
            if dc is not None and dc.mode == "camera":      # 56 of the 59 floats per Gaussian travel underneath the deformation backward
                d_sc, d_rot = self._loc            # private copies, written by the projection backward (above)
                if sharded:
                    # reduce-scatter of the appearance gradients (this rank keeps the sum of ITS chunk) + the small all-reduce of the
                    # screen-space gradients every rank's statistics need in full: one launch on the direct path
                    with dc.group() as grp:
                        w_rs = dc.start_reduce_scatter(self.app_flat, self._chunk, "sum")
                        w_g2 = dc.start(self.g2d_flat, "sum")
                    if grp.work is not None:
                        dc._pending.append(grp.work)
                        early_works.append(grp.work)
                    else:
                        early_works += [w_rs, w_g2]
                else:
                    early_works.append(dc.start(self.early_bucket, "sum"))     # appearance gradients + mean 2-D gradients
            # ---- deformation backward: pts = xyz + dx(...) so d xyz starts as d pts (already in gxyz); the HexPlane adds its share
            # the MLP's weight-gradient kernel (matrix pipe) runs on a second stream beside the HexPlane backward (vector issue,
            # memory latency); joined below, before anything reads the weight gradients
            side = self.side.cuda_stream if self.OVERLAP_DW else s
            early_cam = None
            if early_adam is not None and self.EARLY_ADAM and k == B - 1:       # (a batch: behind the LAST camera's projection backward)
                # The appearance parameters' gradients (SH, scaling, rotation, opacity: 56 of a Gaussian's 59 floats) are final here.
                # Their Adam update -- a pure HBM stream, 335 of Adam's 412 MB -- goes to the second stream now and runs underneath the
                # MLP backward (matrix pipe, 2 TB/s); nothing on this stream reads those parameters again before the join below.
                for p, gbuf in ((g._features_dc, self.gdc), (g._features_rest, self.grest), (g._scaling, self.gsc),
                                (g._rotation, self.grot), (g._opacity, self.gop)):
                    p.grad = gbuf
                if dc is None or dc.mode == "tile-row":
                    # (a tile-row shard's gradients are already the full sums here: the ranks summed the compositing backward's record,
                    # and projection / activation backward ran replicated on it)
                    ops.stream_wait_stream(self.side.cuda_stream, s)
                    early_adam([g._features_dc, g._features_rest, g._scaling, g._rotation, g._opacity], stream=self.side.cuda_stream)
                else:
                    # camera-batch shard: the launch needs the REDUCED bucket (and, for the densification statistics it carries, the
                    # reduced radii / screen-space gradients and the agreed overflow word).  The second stream waits for exactly those
                    # collectives -- each was begun behind the kernels that produced its buffer, so it orders the stream behind them
                    # too -- and not for this stream, which goes on with the deformation backward.  Enqueued BELOW, after that
                    # backward: on RCCL wait() only makes the waiting stream wait, but gloo (the tests) blocks the host in it, and the
                    # host should block with the GPU's work already queued.
                    early_cam = list(early_works)

            def launch_early_cam():
                """Camera-batch shard: the second stream waits for the early collectives, then takes the appearance parameters' Adam
                launch (sharded: this rank's 1/world of it, then the in-place all-gather of the UPDATED parameters behind it -- begun from
                inside the second stream's context, so it is ordered behind that stream's Adam launch; the caller's DistContext.finish()
                makes the main stream wait for it before anything reads a parameter)."""
                app = [g._features_dc, g._features_rest, g._scaling, g._rotation, g._opacity]
                if getattr(dc, "direct", None) is not None and not sharded:
                    # direct RCCL path: a wait is one hipStreamWaitEvent on the second stream's raw handle (no torch stream context: ~10 us)
                    dc.wait_for(early_cam, stream=self.side.cuda_stream)
                    early_adam(app, stream=self.side.cuda_stream)
                    return
                with torch.cuda.stream(self.side):          # (torch.distributed's wait() orders the CURRENT torch stream)
                    dc.wait_for(early_cam)
                    if sharded:
                        ranges = {id(p_): r for p_, r in zip(app, dc.shard_ranges(self._cut, self._chunk))}
                        early_adam(app, stream=self.side.cuda_stream, ranges=ranges)
                        dc.start_gather_flat(self.pflat, self._chunk)
                if not sharded:
                    early_adam(app, stream=self.side.cuda_stream)

            if early_cam is not None and not getattr(dc, "host_blocking", False):
                # On RCCL (either transport) a wait only orders streams: the launch goes to the second stream NOW, ahead of the MLP
                # backward's reduction kernel that is about to be queued there, and runs underneath that backward as in the unsharded
                # step.  (Queued behind the reduction it ran beside the HexPlane gather instead, which it slows from 83 to 116 us.)
                launch_early_cam()
                early_cam = None
            if sl is None:
                N.check(lib.mom_deform_backward_split_n(C.byref(md), P, self.F, self.feat.data_ptr(), self.a0.data_ptr(), d_pts.data_ptr(),
                                                        d_sc.data_ptr(), d_rot.data_ptr(), self.dfeat.data_ptr(),
                                                        self.dh_scratch.data_ptr(), s, side), "deform_bwd")
                if porders is not None:
                    self._hex_scratch_for(hp, P, dev)
                if porders is not None and lines_kept:      # the forward's time lines are still in the field scratch
                    N.check(lib.mom_hexplane_backward_lines(C.byref(hp), P, xyz.data_ptr(), time, optr, self.dfeat.data_ptr(),
                                                            self.gxyz.data_ptr(), porders[0].data_ptr(), porders[1].data_ptr(),
                                                            self._hex_scratch.data_ptr(), ops.field_scratch(hp, dev).data_ptr(), s),
                            "hexplane_bwd")
                else:
                    N.check(lib.mom_hexplane_backward(C.byref(hp), P, xyz.data_ptr(), None, time, optr, self.dfeat.data_ptr(),
                                                      self.gxyz.data_ptr(), None if porders is None else porders[0].data_ptr(),
                                                      None if porders is None else porders[1].data_ptr(),
                                                      None if porders is None else self._hex_scratch.data_ptr(), s), "hexplane_bwd")
            else:
                # tile-row shard: the deformation backward of this rank's slice only.  Its weight / plane gradients are partial sums
                # (summed over the ranks below); its position gradients complete gxyz for the slice's rows, which the ranks then
                # all-gather -- the other rows hold d pts only, replicated by the projection backward.
                S, g0, g1 = sl
                ns = g1 - g0
                if ns > 0:
                    v = lambda t: t[g0:g1]
                    N.check(lib.mom_deform_backward_split(C.byref(md), ns, v(self.feat).data_ptr(), v(self.a0).data_ptr(),
                                                          v(self.gxyz).data_ptr(), v(d_sc).data_ptr(), v(d_rot).data_ptr(),
                                                          v(self.dfeat).data_ptr(), self.dh_scratch.data_ptr(), s, side), "deform_bwd")
                    so = field._slice_order(xyz, g0, g1, bump=False)      # the forward's order of this step
                    spo = field._slice_plane_orders(xyz, g0, g1)
                    if spo is not None:
                        self._hex_scratch_for(hp, ns, dev)
                    N.check(lib.mom_hexplane_backward(C.byref(hp), ns, v(xyz).data_ptr(), None, time, None if so is None else so.data_ptr(),
                                                      v(self.dfeat).data_ptr(), v(self.gxyz).data_ptr(),
                                                      None if spo is None else spo[0].data_ptr(), None if spo is None else spo[1].data_ptr(),
                                                      None if spo is None else self._hex_scratch.data_ptr(), s), "hexplane_bwd")
                dc.start_gather([self.gxyz_rows], S)
            if early_cam is not None:
                launch_early_cam()          # (gloo: its wait() blocks the host, so only now, with the deformation backward queued)
            if self.side is not None:
                ops.stream_wait_stream(s, self.side.cuda_stream)
        if dc is not None and dc.mode == "camera":
            dc.start(self._dg_flat, "sum")     # xyz + deformation field; the caller waits (DistContext.finish) before Adam
        elif sl is not None:
            # this rank's share of the logged loss value -- [sum |d|, sum d^2, sum of the SSIM map] over its OWN rows (the gradient
            # image is already normalised by the whole image's element count) -- rides in front of the field gradients
            if rows[1] > rows[0]:
                if fuse_l1:     # the compositing epilogue left one pair of sums per tile of this rank's rows
                    gx_ = (W + 15) // 16
                    torch.sum(self.l1_part[rows[0] * gx_:rows[1] * gx_], dim=0, out=self._tr_sums[:2])
                else:
                    y0, y1 = rows[0] * 16, min(H, rows[1] * 16)
                    for c in range(3):
                        N.check(lib.mom_l1_loss_acc((y1 - y0) * W, self.color[c, y0:y1].data_ptr(), gt[c, y0:y1].data_ptr(), None,
                                                    self._tr_sums.data_ptr(), s), "l1_slab")
                if lam != 0:
                    self._tr_sums[2:3].copy_(self.ssim_sum[:1])
            # the deformation field's gradients: the slices' shares (and the regulariser's, once) + the loss sums, one collective
            dc.start(self._dg_all[:4 + self._dg_n], "sum")
            dc.finish()
        # ---- hand the gradients to the parameters
        self._set_grads()
        for p, gbuf in zip(planes, self._dg_planes):
            p.grad = gbuf
        for p, gbuf in zip(mlp, self._dg_mlp):
            p.grad = gbuf
        if rows is None:
            l1 = None                        # formed lazily from the per-tile sums (LazyLoss): no kernels for a value nobody may read
        else:
            # the image holds this rank's rows only: the logged values are the sums over the ranks, reduced above
            self.sums.copy_(self._tr_sums[:2])
            if lam != 0:
                self.ssim_sum[:1].copy_(self._tr_sums[2:3])
            l1 = self._tr_sums[0] / n
        return self._loss(l1, reg, lam, n, B)


class FusedStep16(FusedStep):
    """The fine-stage iteration of a model with two HexPlane levels of 16-channel planes, F = 32 features into the shipped network
    (dnerf/eulerian_150_16): FusedStep's launch sequence on the one-launch field of csrc/deform_field16.hip, the MLP backward on 32
    features and the 16-channel HexPlane backward (the F == 32 branches of forward_backward).  One GPU only.  A class of its own
    because FusedStep(...) on such a model is a MomError and stays one."""

    WIDTHS = (32,)


def fine_step(gaussians, opt, hyper, background):
    """The fused fine-stage step of a model -- FusedStep for 64 features, FusedStep16 for 32 (step_features) -- or MomError."""
    F = step_features(gaussians._deformation.deformation_net)
    return (FusedStep16 if F == 32 else FusedStep)(gaussians, opt, hyper, background)


class FusedCoarseStep(_Step):
    """One coarse-stage training iteration as an explicit launch sequence -- no autograd graph, no activated copies of the parameters.

    The coarse stage (train_4DGS.py:149-297 with stage "coarse", the first 3 000 iterations of every run) renders the Gaussians
    WITHOUT the deformation field: the rasterizer's inputs are the model's own parameters through exp / normalize / sigmoid
    (gaussian_renderer/__init__.py:113,130-132).  So the step is the rasterizer and the loss alone:

        projection on the raw parameters (MomRasterArgs.params_raw) -> binning -> compositing forward with the L1 epilogue
        (+ SSIM when lambda_dssim != 0) -> compositing backward -> projection backward, which writes the six parameter gradients
        through the activations and, below densify_until_iter, the densification statistics (MomRasterGrads.stats_*).

    It leaves `.grad` on _xyz, _features_dc, _features_rest, _scaling, _rotation and _opacity only: the deformation network, the
    HexPlane planes and _scene_flow keep None, so optimizer.step() skips them exactly as torch Adam does in the reference's coarse
    stage.  The overflow word and the rest of _Step behave as in FusedStep, so the overflow / replay machinery of train.Trainer
    runs unchanged.  `tests/test_coarse_stage_gpu.py` checks this step against the op-by-op autograd path."""

    def __init__(self, gaussians, opt, hyper, background):
        super().__init__(gaussians, opt, hyper, background)
        self.stats_done = False       # whether the last step's projection backward updated the densification statistics

    def _per_gaussian(self, P, pad, dev, new_frame):
        """Made anew for every P."""
        e = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)
        self._set_bucket(torch.zeros(P + 1, dtype=torch.int32, device=dev))
        self.geom = torch.empty(self.lib.mom_raster_geom_bytes(P), dtype=torch.uint8, device=dev)
        # the six parameter gradients (persist across steps; .grad points at them) + the screen-space gradient and the internal ones
        self._grads = e(59 * P)
        cut = [0, 3 * P, 6 * P, 51 * P, 54 * P, 58 * P, 59 * P]
        seg = lambda i: self._grads[cut[i]:cut[i + 1]]
        self.gxyz, self.gdc, self.grest = seg(0).view(P, 3), seg(1).view(P, 1, 3), seg(2).view(P, 15, 3)
        self.gsc, self.grot, self.gop = seg(3).view(P, 3), seg(4).view(P, 4), seg(5).view(P, 1)
        self.g2d, self.gcol, self.gcov = e(P, 3), e(P, 3), e(P, 6)

    def forward_backward(self, cam, delta_scale=1, early_adam=None, stats=False):
        """One coarse iteration up to (not including) the optimizer step.  cam: one camera, or the list of a batch's cameras (the
        first one's projection backward stores, the others add: module docstring).  stats: update the densification statistics in
        the projection backward (the caller's iteration is below densify_until_iter) -- of a batch: in the LAST camera's, from the
        merged radii and the summed screen-space gradient.  early_adam is ignored: there is no deformation backward to hide Adam
        under.  Returns (loss, radii, screen-space gradient) like FusedStep.forward_backward."""
        g, lib, s = self.g, self.lib, N.current_stream()
        cams = self._cameras(cam)
        B = len(cams)
        if B > 1 and self.dist is not None:
            raise N.MomError("FusedCoarseStep: a batch of cameras on the multi-GPU paths is not supported")
        P, W, H, dev = self._begin(cams[0])
        xyz, f_dc, f_rest, scal, rot, opac = ops.gaussian_params(g, "FusedCoarseStep")
        lam = float(self.opt.lambda_dssim)
        if stats:
            # train_4DGS.py:266 in the projection backward's epilogue; a step whose binning overflowed leaves them alone (the replay
            # makes them), as mom_densify_stats does with the same word
            for t in (g.max_radii2D, g.xyz_gradient_accum, g.denom):
                if t.numel() != P or not t.is_contiguous() or t.dtype != torch.float32:
                    raise N.MomError("FusedCoarseStep: the densification accumulators must be contiguous float32, one per Gaussian")
        for k, cam in enumerate(cams):
            view, proj, campos, gt = cam.device_tensors(dev)
            # the raw parameters: the projection applies exp / normalize / sigmoid itself (gaussian_renderer/__init__.py:130-132)
            a = ops.raster_args(cam, view, proj, campos, self.bg, P, g.active_sh_degree, xyz, f_dc, f_rest, opac, scal, rot, True, 1.0,
                                False, self.keep_all_tiles)
            a.l1_target, a.l1_grad, a.l1_partials = gt.data_ptr(), self.dimg.data_ptr(), self._l1_parts(B)[k].data_ptr()
            if B > 1:
                a.l1_grad_scale = 1.0 / B           # the batch loss is the mean over its cameras (the SSIM term: _ssim_full)
            a.overflow_tag = self.next_tag          # one tag per STEP: any camera's overflow makes the whole step a no-op
            radii_k = self.radii if k == 0 else self._batch_buffers(P, dev)[0]
            self._raster_forward(a, P, W, H, dev, s, radii_k, k == 0)
            if lam != 0:
                self._ssim_full(gt, lam, s, k, B)
            gr = ops.raster_grads(self.g2d, self.gcol, self.gop, self.gxyz, self.gcov, self.gdc, self.grest, self.gsc, self.grot)
            if stats and k == B - 1:
                gr.stats_max_radii2D, gr.stats_grad_accum = g.max_radii2D.data_ptr(), g.xyz_gradient_accum.data_ptr()
                gr.stats_denom, gr.stats_skip_if_nonzero = g.denom.data_ptr(), self.flags.data_ptr()
            if k == 0:
                N.check(lib.mom_raster_backward(C.byref(a), self.radii.data_ptr(), self.geom.data_ptr(), self.binning.data_ptr(),
                                                self.cap, self.img.data_ptr(), self.dimg.data_ptr(), None, C.byref(gr), s), "raster_bwd")
            else:
                # cameras 2..B add their gradients to the first one's and merge their radii into its (train_4DGS.py:203-204,217-229)
                acc = N.MomRasterAccum()
                acc.radii_max = self.radii.data_ptr()
                N.check(lib.mom_raster_backward_acc(C.byref(a), radii_k.data_ptr(), self.geom.data_ptr(), self.binning.data_ptr(),
                                                    self.cap, self.img.data_ptr(), self.dimg.data_ptr(), None, C.byref(gr),
                                                    C.byref(acc), s), "raster_bwd_acc")
        self.stats_done = bool(stats)
        self._set_grads()
        return self._loss(None, None, lam, self.color.numel(), B)


class _TileSums:
    """[sum |image - target|, sum (image - target)^2] of the last step from the per-tile pairs the compositing forward left: sums[k] is a
    device scalar formed on demand (one torch reduction, in a fixed order: the same bits for the same image).  Like LazyLoss it must be
    read before the next step overwrites the pairs."""

    def __init__(self, part):
        self._part, self._t = part, None

    def __getitem__(self, k):
        if self._t is None:
            self._t = self._part.sum(0)
        return self._t[k]


class _BatchSum:
    """sums[0] = the cameras' SSIM map sums added up (rows of _Step._ssim_sums), formed when asked for."""

    def __init__(self, rows):
        self._rows = rows

    def __getitem__(self, k):
        return self._rows[:, k].sum()


class _Lazy:
    """float(x) / x.tensor() = sums[k], looked up when asked for."""

    def __init__(self, sums, k):
        self._sums, self._k = sums, k

    def tensor(self):
        return self._sums[self._k]

    def __float__(self):
        return float(self.tensor())


class LazyLoss:
    """The step's loss value, formed on demand from the accumulators the kernels left on the device (the training loop only
    needs it for logging): float(loss), loss.item(), loss.tensor().  The accumulators are overwritten by the next step, so a
    value wanted later must be taken (tensor()) before that step is enqueued; tensor() is stream-ordered like any torch op."""

    def __init__(self, sums, l1, reg, ssim_sum, lam, n):
        self._sums, self._l1, self._reg, self._ssim, self._lam, self._n, self._t = sums, l1, reg, ssim_sum, lam, n, None

    @property
    def l1(self):
        return self._l1 if self._l1 is not None else self._sums[0] / self._n

    def tensor(self):
        if self._t is None:
            v = self.l1
            if self._reg is not None:
                v = v + self._reg[0]
            if self._ssim is not None:
                v = v + self._lam * (1.0 - (self._ssim[0] / self._n).float())
            self._t = v
        return self._t

    def detach(self):
        return self.tensor().detach()

    def item(self):
        return self.tensor().item()

    def __float__(self):
        return float(self.tensor())
