"""torch-facing wrappers (autograd Functions, optimizer) around the libmom4d C ABI.

Every op here runs on the GPU through hand-written HIP; given CPU tensors they raise (no fallback).
CPU-only tests of the host logic swap `BACKEND` for the oracle's torch restatement explicitly."""
from __future__ import annotations

import ctypes as C
import math
import os as _os

import numpy as np
import torch

from . import _native as N
from .diff_gaussian_rasterization import _C as _RC          # the process-wide switches (set_deterministic) and their scratch


def _need_cuda(t, what):
    if not t.is_cuda:
        raise N.MomError(f"{what}: libmom4d has no CPU path (got a {t.device} tensor)")


# --------------------------------------------------------------------------- HexPlane
def plane_storage(p):
    """Channel-last [H,W,C] storage view of a logical [1,C,H,W] plane parameter (or None if it is not
    laid out that way)."""
    if p.dim() == 4 and p.shape[0] == 1:
        v = p[0].permute(1, 2, 0)
        if v.is_contiguous():
            return v
    return None


def make_plane(C_, H, W, device=None):
    """A [1,C,H,W] tensor whose memory is channel-last ([H][W][C]) -- the layout libmom4d's kernels read: one texel is one
    row of C floats (C = 32: a 128-byte line; C = 16: half of one)."""
    return torch.empty(1, H, W, C_, device=device).permute(0, 3, 1, 2)


def _hexplane_desc(planes_by_level, aabb, grads_by_level=None, aabb_host=None):
    """MomHexPlane descriptor.  `aabb_host`: the six aabb floats already on the host (HexPlaneField.aabb_host());
    without it they are read back from the `aabb` tensor, which blocks the host until the GPU has drained."""
    d = N.MomHexPlane()
    d.levels = len(planes_by_level)
    d.channels = planes_by_level[0][0].shape[1]
    keep = []
    for l, planes in enumerate(planes_by_level):
        # resolutions: plane (a,b) has W = res[a], H = res[b]
        res = [0, 0, 0, 0]
        for p, (a, b) in enumerate(((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))):
            st = plane_storage(planes[p])
            if st is None:
                raise N.MomError("HexPlane planes must be channel-last (use ops.make_plane)")
            if st.shape[2] != d.channels:
                raise N.MomError(f"HexPlane planes disagree in channel count: {st.shape[2]} at level {l}, {d.channels} at level 0 "
                                 "(one count, 16 or 32, for every plane of a field)")
            res[a], res[b] = st.shape[1], st.shape[0]
            d.planes[l][p] = st.data_ptr()
            keep.append(st)
            if grads_by_level is not None:
                gs = plane_storage(grads_by_level[l][p])
                d.grads[l][p] = gs.data_ptr()
                keep.append(gs)
        for k in range(4):
            d.res[l][k] = res[k]
    a = aabb_host if aabb_host is not None else aabb.detach().float().cpu().reshape(-1).tolist()
    for k in range(6):
        d.aabb[k] = a[k]
    return d, keep


def hexplane_backward_ordered(lib, hp, P, xyz, time, order, dfeat, dxyz, s):
    """mom_hexplane_backward under set_deterministic(True): the pull form out of the cached scratch (one shared timestamp)."""
    need = lib.mom_hexplane_ordered_scratch_bytes(C.byref(hp), P)
    if need == 0:
        raise N.MomError("the ordered HexPlane backward (set_deterministic) does not take this field: "
                         f"{hp.levels} levels of {hp.channels} channels, P = {P} (include/mom4d.h, LIMITS)")
    scratch = _RC.field_ordered_scratch("hex", need, xyz.device)
    N.check(lib.mom_hexplane_backward_ordered(C.byref(hp), P, xyz.data_ptr(), float(time), None if order is None else order.data_ptr(),
                                              dfeat.data_ptr(), None if dxyz is None else dxyz.data_ptr(), scratch.data_ptr(),
                                              scratch.numel(), s), "mom_hexplane_backward_ordered")


def mlp_backward_is_ordered(n_in):
    """Which MLP backward set_deterministic(True) selects: the ordered f32 form for a 32-feature trunk and, at 64 features, under
    MOM_MLP_BWD=split; the default 64-feature form (csrc/deform_bwd_b3.hip) already adds its partials in a fixed order and stays
    (tests/test_field_ordered_gpu.py pins that it repeats)."""
    return n_in == 32 or _os.environ.get("MOM_MLP_BWD") == "split"


def deform_backward_ordered(lib, md, P, n_in, feat, a0, dpts, dsc, dro, dfeat, s):
    """mom_deform_backward_n under set_deterministic(True): one stream; ordered weight gradients where the form has atomics."""
    if not mlp_backward_is_ordered(n_in):
        scratch = _RC.field_ordered_scratch("mlp", lib.mom_deform_backward_scratch_bytes(P), feat.device)
        N.check(lib.mom_deform_backward_n(C.byref(md), P, n_in, feat.data_ptr(), a0.data_ptr(), dpts.data_ptr(), dsc.data_ptr(),
                                          dro.data_ptr(), dfeat.data_ptr(), scratch.data_ptr(), s), "mom_deform_backward_n")
        return
    scratch = _RC.field_ordered_scratch("mlp", lib.mom_deform_backward_ordered_scratch_bytes(P), feat.device)
    N.check(lib.mom_deform_backward_ordered_n(C.byref(md), P, n_in, feat.data_ptr(), a0.data_ptr(), dpts.data_ptr(), dsc.data_ptr(),
                                              dro.data_ptr(), dfeat.data_ptr(), scratch.data_ptr(), scratch.numel(), s),
            "mom_deform_backward_ordered_n")


class HexPlaneFunction(torch.autograd.Function):
    """features[P, L*C] = HexPlaneField(xyz, t) (reference scene/hexplane.py:160-183), level-major; C = the planes' channel
    count, 32 or 16 (csrc/hexplane.hip, one template instantiated for both; any other count is a MomError from the library)."""

    @staticmethod
    def forward(ctx, xyz, time, aabb, n_levels, order, aabb_host, plane_orders, *planes):
        _need_cuda(xyz, "hexplane")
        ctx.plane_orders = plane_orders
        lv = [list(planes[6 * l:6 * l + 6]) for l in range(n_levels)]
        d, keep = _hexplane_desc(lv, aabb, aabb_host=aabb_host)
        ctx.aabb_host = aabb_host
        xyz_c = xyz.detach().contiguous().float()
        P = xyz_c.shape[0]
        feat = torch.empty((P, n_levels * d.channels), dtype=torch.float32, device=xyz.device)
        # one timestamp per camera (a python float) or per-point timestamps (a tensor, as the reference passes)
        times = time.detach().reshape(-1).contiguous().float() if torch.is_tensor(time) else None
        tval = 0.0 if times is not None else float(time)
        optr = None if order is None else order.data_ptr()
        N.check(N.lib().mom_hexplane_forward(C.byref(d), P, xyz_c.data_ptr(), None if times is None else times.data_ptr(),
                                             tval, optr, feat.data_ptr(), N.current_stream()), "mom_hexplane_forward")
        ctx.save_for_backward(xyz_c, aabb, *planes)
        ctx.times, ctx.time, ctx.n_levels, ctx.order = times, tval, n_levels, order
        return feat

    @staticmethod
    def backward(ctx, dfeat):
        ordered = _RC.deterministic()
        if ordered and ctx.times is not None:
            raise N.MomError("hexplane backward with per-point timestamps has no ordered form: it cannot run under "
                             "diff_gaussian_rasterization._C.set_deterministic(True)")
        xyz_c, aabb, *planes = ctx.saved_tensors
        n_levels = ctx.n_levels
        wait_reg_pending_all()         # (AccumulateGrad adds what this returns to plane gradients the second stream may be writing)
        lv = [list(planes[6 * l:6 * l + 6]) for l in range(n_levels)]
        grads = [[torch.zeros_like(p) for p in level] for level in lv]   # preserves the channel-last strides
        d, keep = _hexplane_desc(lv, aabb, grads, aabb_host=ctx.aabb_host)
        P = xyz_c.shape[0]
        dxyz = torch.zeros_like(xyz_c) if ctx.needs_input_grad[0] else None
        dfeat = dfeat.contiguous()
        lib = N.lib()
        if ordered:
            hexplane_backward_ordered(lib, d, P, xyz_c, ctx.time, ctx.order, dfeat, dxyz, N.current_stream())
            return (dxyz, None, None, None, None, None, None, *[g for level in grads for g in level])
        po, scratch = ctx.plane_orders, None
        if po is not None and ctx.times is None:        # two-pass backward: per-plane orders + the gradient-row scratch
            scratch = torch.empty(lib.mom_hexplane_backward_scratch_bytes(C.byref(d), P), dtype=torch.uint8, device=xyz_c.device)
        N.check(lib.mom_hexplane_backward(C.byref(d), P, xyz_c.data_ptr(),
                                          None if ctx.times is None else ctx.times.data_ptr(), ctx.time,
                                          None if ctx.order is None else ctx.order.data_ptr(), dfeat.data_ptr(),
                                          None if dxyz is None else dxyz.data_ptr(),
                                          None if scratch is None else po[0].data_ptr(), None if scratch is None else po[1].data_ptr(),
                                          None if scratch is None else scratch.data_ptr(), N.current_stream()),
                "mom_hexplane_backward")
        flat = [g for level in grads for g in level]
        return (dxyz, None, None, None, None, None, None, *flat)


def hexplane_features(xyz, time, aabb, planes_by_level, order=None, aabb_host=None, plane_orders=None):
    flat = [p for level in planes_by_level for p in level]
    return HexPlaneFunction.apply(xyz, time, aabb, len(planes_by_level), order, aabb_host, plane_orders, *flat)


def hexplane_orders(xyz, planes_by_level, aabb, aabb_host=None, stream=None, keepalive=None):
    """(order, inverse), int32 [3, levels, P] each: per space plane and level the permutation that sorts the points by that
    level's texel cell, and its inverse (mom_hexplane_orders) -- what the two-pass HexPlane backward walks.  Speed only.
    stream: a raw stream handle to launch on (default: the current stream); `keepalive`: a list that receives everything the launch
    refers to (scratch, the point tensor, the descriptor's tensors), for a caller that launches on another stream and must keep it
    alive until that work is done."""
    _need_cuda(xyz, "hexplane_orders")
    lib = N.lib()
    pts = xyz.detach().contiguous().float()
    P = pts.shape[0]
    d, keep = _hexplane_desc([[p.detach() for p in lv] for lv in planes_by_level], aabb, aabb_host=aabb_host)
    order = torch.empty((3, d.levels, max(P, 1)), dtype=torch.int32, device=pts.device)
    inverse = torch.empty((3, d.levels, max(P, 1)), dtype=torch.int32, device=pts.device)
    if P:
        scratch = torch.empty(lib.mom_hexplane_orders_scratch_bytes(P), dtype=torch.uint8, device=pts.device)
        N.check(lib.mom_hexplane_orders(C.byref(d), P, pts.data_ptr(), order.data_ptr(), inverse.data_ptr(), scratch.data_ptr(),
                                        N.current_stream() if stream is None else stream), "mom_hexplane_orders")
        if keepalive is not None:
            keepalive += [scratch, pts, keep]
    return order, inverse


def morton_order(xyz, stream=None, keepalive=None):
    """uint32 permutation that walks the points along a Morton curve (int32 tensor of the same bits).  stream / keepalive: as in
    hexplane_orders."""
    _need_cuda(xyz, "morton_order")
    lib = N.lib()
    pts = xyz.detach().contiguous().float()
    P = pts.shape[0]
    order = torch.empty(P, dtype=torch.int32, device=pts.device)
    if P:
        scratch = torch.empty(lib.mom_morton_order_scratch_bytes(P), dtype=torch.uint8, device=pts.device)
        N.check(lib.mom_morton_order(P, pts.data_ptr(), order.data_ptr(), scratch.data_ptr(),
                                     N.current_stream() if stream is None else stream), "mom_morton_order")
        if keepalive is not None:
            keepalive += [scratch, pts]
    return order


# --------------------------------------------------------------------------- deformation field in one pass
FUSE_FIELD = True        # what field_forward does when its caller does not say (fused=None); no environment switch behind it
_field_scratch = {}


def field_scratch(hp, device, P=0):
    """Scratch of the fused deformation kernels, one per device: the per-frame table of time lines (73 KB at the shipped
    resolutions) and, for calls that keep no copy of the features (P > 0: no-grad render()), a [P,64] feature buffer."""
    n = N.lib().mom_deform_field_scratch_bytes(C.byref(hp), int(P))
    t = _field_scratch.get(device)
    if t is None or t.numel() < n:
        t = _field_scratch[device] = torch.empty(n, dtype=torch.uint8, device=device)
    return t


def field_forward(hp, md, P, xyz, time, order, scal, rot, flow, coef, pts, sc_d, rot_d, feat, a0, opac, sc, rot_act, op, s,
                  scratch_feat=None, scratch=None, fused=None):
    """deform_network.forward for one timestamp: the fused kernel (csrc/deform_field.hip) when the field's shape allows it, else
    HexPlane + MLP; fused=False: the two kernels in any case (the tests' comparison); None: the module's FUSE_FIELD.
    feat / a0: [P,64] tensors that receive the features and relu(h0) for the backward, or None (no backward follows; the
    two-kernel path then needs `scratch_feat` for the features).
    scratch: the caller's own field scratch (mom_deform_field_scratch_bytes) -- callers that keep several frames in flight on
    different streams must not share the per-device one (the time-line table and the feature buffer live for the whole launch)."""
    lib = N.lib()
    q = lambda t: None if t is None else t.data_ptr()
    if (FUSE_FIELD if fused is None else fused) and lib.mom_deform_field_supported(C.byref(hp)):
        N.check(lib.mom_deform_field_forward(C.byref(hp), C.byref(md), P, xyz.data_ptr(), float(time),
                                             q(order), scal.data_ptr(),
                                             rot.data_ptr(), flow.data_ptr(), float(coef), pts.data_ptr(), sc_d.data_ptr(),
                                             rot_d.data_ptr(), q(feat), q(a0), q(opac), q(sc), q(rot_act), q(op),
                                             (scratch if scratch is not None else
                                              field_scratch(hp, xyz.device, 0 if feat is not None else P)).data_ptr(), s), "deform_field_fwd")
        return True          # the device's field scratch now holds this frame's time lines (mom_hexplane_backward_lines)
    f = feat if feat is not None else scratch_feat
    N.check(lib.mom_hexplane_forward(C.byref(hp), P, xyz.data_ptr(), None, float(time), q(order), f.data_ptr(), s), "hexplane_fwd")
    N.check(lib.mom_deform_forward_activated(C.byref(md), P, f.data_ptr(), xyz.data_ptr(), scal.data_ptr(), rot.data_ptr(),
                                             flow.data_ptr(), float(coef), pts.data_ptr(), sc_d.data_ptr(), rot_d.data_ptr(), q(a0),
                                             q(opac), q(sc), q(rot_act), q(op), s), "deform_fwd")
    return False


def field16_forward(hp, md, P, xyz, time, order, scal, rot, flow, coef, pts, sc_d, rot_d, feat, a0, opac, sc, rot_act, op, s,
                    scratch=None):
    """field_forward for two levels of 16-channel planes (csrc/deform_field16.hip): HexPlane gather, trunk, heads, residuals and
    activations in one launch, the bits of mom_hexplane_forward + mom_deform_forward_activated_n.  feat [P,32] / a0 [P,64] and the
    activated outputs sc / rot_act / op (with opac) are optional.  A field mom_deform_field16_supported refuses is a MomError: the
    caller routes (Deformation._field16_fusable), nothing falls back here."""
    lib = N.lib()
    q = lambda t: None if t is None else t.data_ptr()
    if not lib.mom_deform_field16_supported(C.byref(hp)):
        raise N.MomError(f"field16_forward: {hp.levels} levels of {hp.channels} channels (needs 2 of 16, resolutions <= 1024)")
    N.check(lib.mom_deform_field16_forward(C.byref(hp), C.byref(md), P, xyz.data_ptr(), float(time), q(order), scal.data_ptr(),
                                           rot.data_ptr(), flow.data_ptr(), float(coef), pts.data_ptr(), sc_d.data_ptr(),
                                           rot_d.data_ptr(), q(feat), q(a0), q(opac), q(sc), q(rot_act), q(op), q(scratch), s),
            "deform_field16_fwd")


# --------------------------------------------------------------------------- rasterizer arguments (the fused paths)
def gaussian_params(g, who):
    """(xyz, f_dc, f_rest, scaling, rotation, opacity) of model g, detached; MomError unless every one is contiguous (the kernels
    read them through raw pointers).  (.data: a detached alias like .detach(), at half the host time -- the fused steps are paced
    by the host at small sizes.)"""
    ps = g._xyz.data, g._features_dc.data, g._features_rest.data, g._scaling.data, g._rotation.data, g._opacity.data
    for t in ps:
        if not t.is_contiguous():
            raise N.MomError(f"{who}: the Gaussian parameters must be contiguous")
    return ps


def raster_args(cam, view, proj, campos, bg, P, D, means, f_dc, f_rest, opac, scales, rots, params_raw, scale_modifier, debug,
                keep_all_tiles):
    """MomRasterArgs of one camera with 16 SH coefficients read through two pointers (DC, rest).  params_raw: scales / rots / opac
    are the raw parameters and the projection applies exp / normalize / sigmoid itself.  The struct holds raw pointers only: the
    caller keeps every tensor behind them alive until the last launch that reads it."""
    a = N.MomRasterArgs()
    a.P, a.D, a.M, a.W, a.H = P, D, 16, int(cam.image_width), int(cam.image_height)
    a.background, a.means3D = bg.data_ptr(), means.data_ptr()
    a.shs, a.shs_rest = f_dc.data_ptr(), f_rest.data_ptr()
    a.opacities, a.scales, a.rotations = opac.data_ptr(), scales.data_ptr(), rots.data_ptr()
    a.params_raw = int(params_raw)
    a.viewmatrix, a.projmatrix, a.campos = view.data_ptr(), proj.data_ptr(), campos.data_ptr()
    a.scale_modifier = float(scale_modifier)
    a.tan_fovx, a.tan_fovy = math.tan(cam.FoVx * 0.5), math.tan(cam.FoVy * 0.5)
    a.debug = int(bool(debug))
    a.keep_all_tiles = int(keep_all_tiles)
    return a


def raster_grads(g2d, gcol, gop, gxyz, gcov, gdc, grest, gsc, grot):
    """MomRasterGrads with the nine gradient outputs every backward of the fused paths writes."""
    gr = N.MomRasterGrads()
    gr.dL_dmeans2D, gr.dL_dcolors, gr.dL_dopacity = g2d.data_ptr(), gcol.data_ptr(), gop.data_ptr()
    gr.dL_dmeans3D, gr.dL_dcov3D = gxyz.data_ptr(), gcov.data_ptr()
    gr.dL_dsh, gr.dL_dsh_rest = gdc.data_ptr(), grest.data_ptr()
    gr.dL_dscales, gr.dL_drotations = gsc.data_ptr(), grot.data_ptr()
    return gr


# --------------------------------------------------------------------------- fused deformation MLP
class DeformMLPFunction(torch.autograd.Function):
    """(pts, scales, rots) = fused trunk + pos/scales/rotations heads + residual adds
    (reference scene/deformation.py:97-135 with the shipped config).  Parameter order:
    W0,b0, W1p,b1p,W2p,b2p, W1s,b1s,W2s,b2s, W1r,b1r,W2r,b2r."""

    @staticmethod
    def _desc(params, grads=None):
        d = N.MomDeformMLP()
        W0, b0, *rest = params
        d.W0, d.b0 = W0.data_ptr(), b0.data_ptr()
        for k in range(3):
            W1, b1, W2, b2 = rest[4 * k:4 * k + 4]
            d.W1[k], d.b1[k], d.W2[k], d.b2[k] = W1.data_ptr(), b1.data_ptr(), W2.data_ptr(), b2.data_ptr()
        if grads is not None:
            gW0, gb0, *grest = grads
            d.dW0, d.db0 = gW0.data_ptr(), gb0.data_ptr()
            for k in range(3):
                g = grest[4 * k:4 * k + 4]
                d.dW1[k], d.db1[k], d.dW2[k], d.db2[k] = (t.data_ptr() for t in g)
        return d

    @staticmethod
    def check_shapes(feat, params):
        """The trunk width (32 or 64) of a call, from feat [P,width]; MomError unless W0 is [64,width] and the other 13 tensors
        have the shapes _desc hands to the kernels as raw pointers (a narrower tensor would be read past its end)."""
        if feat.dim() != 2 or feat.shape[1] not in (32, 64):
            raise N.MomError(f"deform_mlp: feat must be [P,32] or [P,64], got {tuple(feat.shape)}")
        n_in = int(feat.shape[1])
        want = [(64, n_in), (64,)]
        for nout in (3, 3, 4):
            want += [(64, 64), (64,), (nout, 64), (nout,)]
        if len(params) != len(want):
            raise N.MomError(f"deform_mlp: {len(want)} parameter tensors expected, got {len(params)}")
        for i, (p, w) in enumerate(zip(params, want)):
            if tuple(p.shape) != w or p.dtype != torch.float32:
                raise N.MomError(f"deform_mlp: parameter {i} must be float32 {w} for {n_in} features, "
                                 f"got {p.dtype} {tuple(p.shape)}")
        return n_in

    @staticmethod
    def forward(ctx, feat, xyz, scaling, rotation, scene_flow, flow_coef, *params):
        _need_cuda(feat, "deform_mlp")
        n_in = DeformMLPFunction.check_shapes(feat, params)
        lib = N.lib()
        P = feat.shape[0]
        ps = [p.detach().contiguous() for p in params]
        feat_c = feat.detach().contiguous()
        d = DeformMLPFunction._desc(ps)
        s = N.current_stream()
        pts = torch.empty_like(xyz)
        sc = torch.empty_like(scaling)
        ro = torch.empty_like(rotation)
        xyz_c, scal_c, rot_c, flow_c = (t.detach().contiguous() for t in (xyz, scaling, rotation, scene_flow))
        need_bwd = any(ctx.needs_input_grad)
        a0 = torch.empty((P, 64), dtype=torch.float32, device=feat_c.device) if need_bwd else None      # relu(h0), whatever the trunk reads
        N.check(lib.mom_deform_forward_n(C.byref(d), P, n_in, feat_c.data_ptr(), xyz_c.data_ptr(), scal_c.data_ptr(), rot_c.data_ptr(),
                                         flow_c.data_ptr(), float(flow_coef), pts.data_ptr(), sc.data_ptr(), ro.data_ptr(),
                                         None if a0 is None else a0.data_ptr(), s), "mom_deform_forward_n")
        ctx.save_for_backward(feat_c, a0 if a0 is not None else feat_c, *ps)
        return pts, sc, ro

    @staticmethod
    def backward(ctx, dpts, dsc, dro):
        feat_c, a0, *ps = ctx.saved_tensors
        lib = N.lib()
        P = feat_c.shape[0]
        grads = [torch.zeros_like(p) for p in ps]
        d = DeformMLPFunction._desc(ps, grads)
        dpts, dsc, dro = dpts.contiguous(), dsc.contiguous(), dro.contiguous()
        dfeat = torch.empty_like(feat_c)                # [P,32] or [P,64]: the trunk's width
        if _RC.deterministic():
            deform_backward_ordered(lib, d, P, feat_c.shape[1], feat_c, a0, dpts, dsc, dro, dfeat, N.current_stream())
            return (dfeat, dpts, dsc, dro, None, None, *grads)
        scratch = torch.empty(lib.mom_deform_backward_scratch_bytes(P), dtype=torch.uint8, device=feat_c.device)
        N.check(lib.mom_deform_backward_n(C.byref(d), P, feat_c.shape[1], feat_c.data_ptr(), a0.data_ptr(), dpts.data_ptr(),
                                          dsc.data_ptr(), dro.data_ptr(), dfeat.data_ptr(), scratch.data_ptr(), N.current_stream()),
                "mom_deform_backward_n")
        # identity paths: pts = xyz + ..., scales = scaling + ..., rots = rotation + ...; scene_flow has no grad
        return (dfeat, dpts, dsc, dro, None, None, *grads)


def deform_mlp(feat, xyz, scaling, rotation, scene_flow, flow_coef, params):
    return DeformMLPFunction.apply(feat, xyz, scaling, rotation, scene_flow, flow_coef, *params)


# --------------------------------------------------------------------------- L1 + PSNR
class L1LossFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, img, gt):
        if img.numel() != gt.numel():      # (the kernel walks both with one index: a shorter gt would be read past its end)
            raise N.MomError(f"l1_loss: image {tuple(img.shape)} and target {tuple(gt.shape)} differ in their number of elements")
        _need_cuda(img, "l1_loss")
        _need_cuda(gt, "l1_loss")
        a = img.detach().contiguous().float()
        b = gt.detach().contiguous().float()
        dimg = torch.empty_like(a)
        sums = torch.empty(2, dtype=torch.float32, device=a.device)
        if _RC.deterministic():        # the two sums in the documented order (include/mom4d.h, "ordered loss values"); dimg is the same bits
            lib = N.lib()
            scratch = _RC.value_ordered_scratch("l1", lib.mom_l1_loss_ordered_scratch_bytes(a.numel()), a.device)
            N.check(lib.mom_l1_loss_ordered(a.numel(), a.data_ptr(), b.data_ptr(), dimg.data_ptr(), sums.data_ptr(), scratch.data_ptr(),
                                            scratch.numel(), N.current_stream()), "mom_l1_loss_ordered")
        else:
            N.check(N.lib().mom_l1_loss(a.numel(), a.data_ptr(), b.data_ptr(), dimg.data_ptr(), sums.data_ptr(),
                                        N.current_stream()), "mom_l1_loss")
        ctx.save_for_backward(dimg)
        ctx.mark_non_differentiable(sums)
        return sums[0] / a.numel(), sums

    @staticmethod
    def backward(ctx, g, _):
        (dimg,) = ctx.saved_tensors
        return dimg * g, None


def l1_loss_with_sums(img, gt):
    """(mean |img-gt|, [sum|d|, sum d^2]) in one pass; the second output feeds psnr without re-reading the images."""
    return L1LossFunction.apply(img, gt)


# --------------------------------------------------------------------------- row selection (densify / prune)
def select_rows(mask, tensors):
    """[t[mask] for t in tensors] -- the selection the reference's optimizer surgery does per tensor (scene/gaussian_model.py:
    409-482, 511-581) -- through ONE compaction plan: the mask is scanned once, one host synchronisation reads the number of
    kept rows (the outputs have to be allocated), and one kernel gathers the rows of every tensor."""
    _need_cuda(mask, "select_rows")
    n = mask.shape[0]
    if mask.dim() != 1 or mask.dtype != torch.bool:
        raise N.MomError("select_rows: the mask must be a 1-D bool tensor")
    srcs = []
    for t_ in tensors:
        if t_.shape[0] != n or not t_.is_cuda:
            raise N.MomError("select_rows: every tensor needs one row per mask element, on the GPU")
        srcs.append(t_.detach().contiguous())
    lib, s = N.lib(), N.current_stream()
    dev = mask.device
    keep = mask.contiguous().view(torch.uint8)
    dst_index = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    count_dev = torch.empty(1, dtype=torch.int32, device=dev)
    count_host = torch.empty(1, dtype=torch.int32).pin_memory()
    scratch = torch.empty(lib.mom_select_scratch_bytes(n), dtype=torch.uint8, device=dev)
    N.check(lib.mom_select_plan(n, keep.data_ptr(), dst_index.data_ptr(), count_dev.data_ptr(), count_host.data_ptr(),
                                scratch.data_ptr(), s), "mom_select_plan")
    torch.cuda.current_stream().synchronize()          # the one sync of the round: sizes of the outputs
    m = int(count_host[0])
    outs = [torch.empty((m,) + tuple(t_.shape[1:]), dtype=t_.dtype, device=dev) for t_ in srcs]
    if m == 0:                                           # nothing kept: empty outputs (their data pointers are null)
        return outs
    for lo in range(0, len(srcs), N.SELECT_MAX_TENSORS):
        part = list(zip(srcs, outs))[lo:lo + N.SELECT_MAX_TENSORS]
        arr = (N.MomRowSelect * len(part))()
        for i, (a, b) in enumerate(part):
            rb = (a.numel() // max(n, 1)) * a.element_size() if n else 0
            arr[i].src, arr[i].dst, arr[i].row_bytes = a.data_ptr(), b.data_ptr(), rb
        N.check(lib.mom_select_apply(n, dst_index.data_ptr(), arr, len(part), s), "mom_select_apply")
    return outs


# --------------------------------------------------------------------------- one-pass densify round
_DENSIFY_SINGLE = (("xyz", N.DENSIFY_XYZ, 3), ("scaling", N.DENSIFY_SCALING, 3), ("rotation", N.DENSIFY_ROTATION, 4))
_DENSIFY_LISTS = (("copy", N.DENSIFY_COPY), ("moment", N.DENSIFY_MOMENT), ("zero", N.DENSIFY_ZERO))
_densify_counts_host = None        # three pinned ints, reused: the plan's counts land here


def densify_round(clone_mask, split_mask, tensors_by_role, z=None):
    """Clone, split and the removal of the split parents (scene/gaussian_model.py:461-581: densify_and_clone, densify_and_split,
    cat_tensors_to_optimizer, densification_postfix, prune_points) for every tensor of a model in one pass: the two masks are
    scanned once, ONE host synchronisation reads the three counts (the outputs have to be allocated), and one kernel reads every
    source row once and writes the round's final layout -- the rows that are not split in order, the clones in order, child 0 of
    every split parent, child 1 of every split parent.

    tensors_by_role: {"xyz": [P,3], "scaling": [P,3], "rotation": [P,4]} (float32; needed when anything is split: the children
    are made of them) and the lists "copy" (every output row is its source row), "moment" (Adam moments: clone and child rows
    are zero) and "zero" (statistics: zero at the new length).  The masks are disjoint 1-D bool tensors.  `z`: the [2S,3]
    standard normals of the children; None draws them from torch's generator of the device, after the counts are known and only
    if S > 0 -- the draw of the reference's torch.normal(zeros(2S,3), std).
    Returns a dict with the same keys holding the new tensors, plus "counts" = (K, C, S) and "z" (None if S == 0)."""
    global _densify_counts_host
    _need_cuda(clone_mask, "densify_round")
    _need_cuda(split_mask, "densify_round")
    P = clone_mask.shape[0]
    for m in (clone_mask, split_mask):
        if m.dim() != 1 or m.dtype != torch.bool or m.shape[0] != P or m.device != clone_mask.device:
            raise N.MomError("densify_round: the masks must be 1-D bool tensors of one length on one device")
    dev = clone_mask.device
    unknown = set(tensors_by_role) - {k for k, _, _ in _DENSIFY_SINGLE} - {k for k, _ in _DENSIFY_LISTS}
    if unknown:
        raise N.MomError(f"densify_round: unknown roles {sorted(unknown)}")
    items = []                                                       # (key, position or None, role, source)
    for key, role, width in _DENSIFY_SINGLE:
        t_ = tensors_by_role.get(key)
        if t_ is not None:
            if t_.dtype != torch.float32 or tuple(t_.shape) != (P, width):
                raise N.MomError(f"densify_round: {key} must be a float32 [{P},{width}] tensor, got {t_.dtype} {tuple(t_.shape)}")
            items.append((key, None, role, t_))
    for key, role in _DENSIFY_LISTS:
        items += [(key, j, role, t_) for j, t_ in enumerate(tensors_by_role.get(key, ()))]
    if len(items) > N.DENSIFY_MAX_TENSORS:
        raise N.MomError(f"densify_round: {len(items)} tensors, one launch takes {N.DENSIFY_MAX_TENSORS}")
    srcs = []
    for key, j, role, t_ in items:
        _need_cuda(t_, "densify_round")
        t_ = t_.detach()
        if t_.dim() < 1 or t_.shape[0] != P or t_.device != dev:
            raise N.MomError(f"densify_round: every tensor needs one row per mask element on the masks' device ({key})")
        if not t_.is_contiguous():
            raise N.MomError(f"densify_round: {key} is not contiguous")
        rb = (t_.numel() // P) * t_.element_size() if P else 0
        if rb > N.DENSIFY_MAX_ROW_BYTES:
            raise N.MomError(f"densify_round: rows of {rb} bytes ({key}); the limit is {N.DENSIFY_MAX_ROW_BYTES}")
        srcs.append((t_, rb))
    if z is not None:
        _need_cuda(z, "densify_round")
        if z.dtype != torch.float32 or z.dim() != 2 or z.shape[1] != 3 or not z.is_contiguous() or z.device != dev:
            raise N.MomError("densify_round: z must be a contiguous float32 [2S,3] tensor on the masks' device")

    lib, s = N.lib(), N.current_stream()
    K = C_ = S = 0
    if P:
        if _densify_counts_host is None:
            _densify_counts_host = torch.empty(3, dtype=torch.int32).pin_memory()
        counts_host = _densify_counts_host
        index = torch.empty((3, P), dtype=torch.int32, device=dev)
        counts_dev = torch.empty(3, dtype=torch.int32, device=dev)
        scratch = torch.empty(lib.mom_densify_scratch_bytes(P), dtype=torch.uint8, device=dev)
        cm, sm = clone_mask.contiguous().view(torch.uint8), split_mask.contiguous().view(torch.uint8)
        N.check(lib.mom_densify_plan(P, cm.data_ptr(), sm.data_ptr(), index[0].data_ptr(), index[1].data_ptr(),
                                     index[2].data_ptr(), counts_dev.data_ptr(), counts_host.data_ptr(), scratch.data_ptr(), s),
                "mom_densify_plan")
        torch.cuda.current_stream().synchronize()      # the one sync of the round: sizes of the outputs
        K, C_, S = (int(v) for v in counts_host)
    if S:
        if not all(k in tensors_by_role and tensors_by_role[k] is not None for k, _, _ in _DENSIFY_SINGLE):
            raise N.MomError("densify_round: rows are split, and the children need xyz, scaling and rotation")
        if z is None:
            z = torch.randn((2 * S, 3), dtype=torch.float32, device=dev)
        elif z.shape[0] != 2 * S:
            raise N.MomError(f"densify_round: {S} rows are split, z has {z.shape[0]} rows instead of {2 * S}")
    else:
        z = None
    nout = K + C_ + 2 * S
    outs = [torch.empty((nout,) + tuple(t_.shape[1:]), dtype=t_.dtype, device=dev) for t_, _ in srcs]
    if P:
        arr = (N.MomDensifyTensor * max(len(items), 1))()
        for i, ((_, _, role, _), (t_, rb), o) in enumerate(zip(items, srcs, outs)):
            arr[i].src, arr[i].dst, arr[i].row_bytes, arr[i].role = t_.data_ptr(), o.data_ptr(), rb, role
        counts = (C.c_int * 3)(K, C_, S)
        N.check(lib.mom_densify_apply(P, index[0].data_ptr(), index[1].data_ptr(), index[2].data_ptr(), counts,
                                      None if z is None else z.data_ptr(), arr, len(items), C.sizeof(N.MomDensifyTensor), s),
                "mom_densify_apply")
    result = {"counts": (K, C_, S), "z": z}
    for key, _ in _DENSIFY_LISTS:
        if key in tensors_by_role:
            result[key] = []
    for (key, j, _, _), o in zip(items, outs):
        if j is None:
            result[key] = o
        else:
            result[key].append(o)
    return result


# --------------------------------------------------------------------------- scene-flow fit
def sceneflow_fit(points, K, R, T, w, records, valid, lr, flow, loss=None, flow2d_last=None):
    """The motion optimisation module's SGD loop (train_motion.py:125-207), every epoch and every view in one launch
    (csrc/sceneflow_fit.hip; include/mom4d.h has the arithmetic).  Enqueued on the current stream; nothing is read back.

    points [3,P], R [V,3,3], T [V,3], w [V], records [V,P,4] = {pix0, gt}, lr [E]: contiguous float32 on one device;
    valid [ceil(V/32),P] int32 bit words; K: the 3x3 intrinsics as HOST numbers (a CPU tensor, an array or nested lists);
    flow [3,P] is updated in place; loss [E] and flow2d_last [V,P,2] are optional outputs.  Returns flow."""
    _need_cuda(points, "sceneflow_fit")
    dev = points.device
    if points.dim() != 2 or points.shape[0] != 3:
        raise N.MomError(f"sceneflow_fit: points must be [3,P], got {tuple(points.shape)}")
    P = points.shape[1]
    if R.dim() != 3 or tuple(R.shape[1:]) != (3, 3) or R.shape[0] < 1:
        raise N.MomError(f"sceneflow_fit: R must be [V,3,3] with V >= 1, got {tuple(R.shape)}")
    V = R.shape[0]
    if lr.dim() != 1:
        raise N.MomError(f"sceneflow_fit: lr must be [E], got {tuple(lr.shape)}")
    E = lr.shape[0]
    words = (V + 31) // 32
    want = [("points", points, (3, P), torch.float32), ("R", R, (V, 3, 3), torch.float32), ("T", T, (V, 3), torch.float32),
            ("w", w, (V,), torch.float32), ("records", records, (V, P, 4), torch.float32), ("valid", valid, (words, P), torch.int32),
            ("lr", lr, (E,), torch.float32), ("flow", flow, (3, P), torch.float32)]
    if loss is not None:
        want.append(("loss", loss, (E,), torch.float32))
    if flow2d_last is not None:
        want.append(("flow2d_last", flow2d_last, (V, P, 2), torch.float32))
    for name, t_, shape, dtype in want:
        _need_cuda(t_, "sceneflow_fit")
        if tuple(t_.shape) != shape or t_.dtype != dtype or t_.device != dev or not t_.is_contiguous():
            raise N.MomError(f"sceneflow_fit: {name} must be a contiguous {dtype} {list(shape)} tensor on {dev}, "
                             f"got {t_.dtype} {list(t_.shape)} on {t_.device}")
    if flow.requires_grad or (loss is not None and loss.requires_grad):
        raise N.MomError("sceneflow_fit: flow is updated in place and takes no gradient (the kernel is the optimiser)")
    if torch.is_tensor(K):
        if K.is_cuda:
            raise N.MomError("sceneflow_fit: K is read on the host; pass a CPU tensor or an array (a device tensor would be a synchronisation)")
        K = K.detach().numpy()
    K = np.asarray(K, dtype=np.float32)
    if K.shape != (3, 3):
        raise N.MomError(f"sceneflow_fit: K must be 3x3, got {K.shape}")
    if K[0, 1] != 0 or K[1, 0] != 0 or K[2, 0] != 0 or K[2, 1] != 0 or K[2, 2] != 1:
        raise N.MomError("sceneflow_fit: K must be [[fx,0,cx],[0,fy,cy],[0,0,1]]")
    lib = N.lib()
    k9 = (C.c_float * 9)(*[float(x) for x in K.reshape(-1)])
    scratch, nbytes = None, 0
    if loss is not None and P:
        nbytes = lib.mom_sceneflow_fit_scratch_bytes(P, V, E)
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    N.check(lib.mom_sceneflow_fit(P, V, E, N.ptr(points), k9, N.ptr(R), N.ptr(T), N.ptr(w), N.ptr(records), N.ptr(valid), N.ptr(lr),
                                  N.ptr(flow), N.ptr(loss), N.ptr(flow2d_last), N.ptr(scratch), nbytes, N.current_stream()),
            "mom_sceneflow_fit")
    return flow


def flow_sample(flow_images, pix, valid, diagonals, records=None):
    """The fit's records from the views' 2D flow images: what scipy.interpolate.griddata(pixel grid, image, pixels, "linear") gives
    at every view's valid points (train_motion.py:117-121), all V views in one launch (csrc/flow_sample.hip; include/mom4d.h has the
    arithmetic).  Enqueued on the current stream; nothing is read back.

    flow_images [V,2,H,W] (the frames' layout, repacked on the device) or [V,H,W,2] (taken as it is); a shape that could be either,
    [V,2,n,2], is read as [V,2,H,W]: float32; pix [V,P,2] float64, the unflowed pixels; valid [ceil(V/32),P] int32 bit words;
    diagonals [ceil((H-1)(W-1)/32)] int32 bit words (motion.pack_diagonals): all contiguous on one device.
    records [V,P,4] float32 is written in full -- zeros for invalid pairs -- and returned (allocated when not given)."""
    if flow_images.dim() != 4 or 2 not in (flow_images.shape[1], flow_images.shape[3]) or flow_images.shape[0] < 1:
        raise N.MomError(f"flow_sample: flow_images must be [V,2,H,W] or [V,H,W,2] with V >= 1, got {tuple(flow_images.shape)}")
    if flow_images.dtype != torch.float32 or not flow_images.is_contiguous():
        raise N.MomError(f"flow_sample: flow_images must be a contiguous torch.float32 tensor, got {flow_images.dtype}, "
                         f"strides {tuple(flow_images.stride())}")
    channel_first = flow_images.shape[1] == 2
    V, H, W = (flow_images.shape[0], *flow_images.shape[2:]) if channel_first else flow_images.shape[:3]
    if H < 2 or W < 2:
        raise N.MomError(f"flow_sample: an image needs at least one cell (H, W >= 2), got H {H}, W {W}")
    if pix.dim() != 3:
        raise N.MomError(f"flow_sample: pix must be [V,P,2], got {tuple(pix.shape)}")
    P, dev = pix.shape[1], flow_images.device
    want = [("pix", pix, (V, P, 2), torch.float64), ("valid", valid, ((V + 31) // 32, P), torch.int32),
            ("diagonals", diagonals, (((H - 1) * (W - 1) + 31) // 32,), torch.int32)]
    if records is not None:
        want.append(("records", records, (V, P, 4), torch.float32))
    for name, t_, shape, dtype in want:
        if tuple(t_.shape) != shape or t_.dtype != dtype or t_.device != dev or not t_.is_contiguous():
            raise N.MomError(f"flow_sample: {name} must be a contiguous {dtype} {list(shape)} tensor on {dev}, "
                             f"got {t_.dtype} {list(t_.shape)} on {t_.device}")
    _need_cuda(flow_images, "flow_sample")
    if records is None:
        records = torch.empty((V, P, 4), dtype=torch.float32, device=dev)
    elif records.requires_grad:
        raise N.MomError("flow_sample: records is written in place and takes no gradient")
    if channel_first:
        flow_images = flow_images.permute(0, 2, 3, 1).contiguous()
    N.check(N.lib().mom_flow_sample(P, V, H, W, N.ptr(flow_images), N.ptr(pix), N.ptr(valid), N.ptr(diagonals), N.ptr(records),
                                    N.current_stream()), "mom_flow_sample")
    return records


# --------------------------------------------------------------------------- the video generator's warp (csrc/eulerian_warp.hip)
def _f32_device(what, **tensors):
    first = next(iter(tensors.values()))
    for name, t_ in tensors.items():
        if t_.dtype != torch.float32 or not t_.is_contiguous() or t_.device != first.device:
            raise N.MomError(f"{what}: {name} must be a contiguous torch.float32 tensor on {first.device}, got {t_.dtype}, "
                             f"strides {tuple(t_.stride())} on {t_.device}")
        if t_.requires_grad and torch.is_grad_enabled():
            raise N.MomError(f"{what}: forward only (the reference's generator runs under no_grad); {name} requires grad")
    _need_cuda(first, what)


def eulerian_geometry(S):
    """(cut, pad, padded, crop0) of blend_feature / crop_padded_tensor for a square feature of size S (mom_eulerian_geometry)."""
    out = [C.c_int() for _ in range(4)]
    if N.lib().mom_eulerian_geometry(int(S), *[C.byref(o) for o in out]) != N.MOM_OK:
        raise N.MomError(f"eulerian_geometry: no cut / reflection padding / crop exists for a feature of size {S}")
    return tuple(o.value for o in out)


def euler_integrate(motion, steps, all_frames=False):
    """euler_integration of the reference's video generator (cinemagraph_utils.py:9-59) in one launch: motion [2,H,W] ->
    the displacement after `steps` steps [2,H,W], or every step's [steps+1,2,H,W].  The reference's bits; non-finite motion gives
    displacement 0 where the reference would index out of range (include/mom4d.h)."""
    if motion.dim() != 3 or motion.shape[0] != 2 or motion.shape[1] < 1 or motion.shape[2] < 1:
        raise N.MomError(f"euler_integrate: motion must be [2,H,W], got {tuple(motion.shape)}")
    steps = int(steps)
    if steps < 0:
        raise N.MomError(f"euler_integrate: steps must be >= 0, got {steps}")
    _f32_device("euler_integrate", motion=motion)
    H, W = motion.shape[1:]
    disp = torch.empty(((steps + 1, 2, H, W) if all_frames else (2, H, W)), dtype=torch.float32, device=motion.device)
    N.check(N.lib().mom_euler_integrate(H, W, steps, int(bool(all_frames)), N.ptr(motion), N.ptr(disp), N.current_stream()),
            "mom_euler_integrate")
    return disp


def _warp_ordered(ordered):
    """The `ordered` argument of the warp's ops: None follows the process-wide switch (_RC.set_deterministic)."""
    return _RC.deterministic() if ordered is None else bool(ordered)


def softsplat_sum(input, flow, ordered=None):
    """The forward of the reference's _FunctionSoftsplat (softmax_splatting.py:8-53, 236-269): input [N,C,H,W] splatted along
    flow [N,2,H,W] with bilinear weights into a new [N,C,H,W]; targets outside the canvas are dropped.
    ordered (None: as diff_gaussian_rasterization._C.deterministic() says): mom_softsplat_sum_ordered, the sums in the order
    include/mom4d.h defines, out of the grow-only scratch _RC.warp_ordered_scratch; False: float atomics, no scratch."""
    if input.dim() != 4 or flow.dim() != 4 or flow.shape[1] != 2 or flow.shape[0] != input.shape[0] \
            or flow.shape[2:] != input.shape[2:] or 0 in input.shape:
        raise N.MomError(f"softsplat_sum: input [N,C,H,W] and flow [N,2,H,W] are needed, got {tuple(input.shape)} and "
                         f"{tuple(flow.shape)}")
    _f32_device("softsplat_sum", input=input, flow=flow)
    n, c, H, W = input.shape
    out = torch.zeros_like(input)
    if _warp_ordered(ordered):
        need = N.lib().mom_softsplat_ordered_scratch_bytes(n, c, H, W)
        if need == 0:
            raise N.MomError(f"softsplat_sum: the ordered splat does not take {tuple(input.shape)} (include/mom4d.h has its limits)")
        scratch = _RC.warp_ordered_scratch(need, input.device)
        N.check(N.lib().mom_softsplat_sum_ordered(n, c, H, W, N.ptr(input), N.ptr(flow), N.ptr(out), N.ptr(scratch), scratch.numel(),
                                                  N.current_stream()), "mom_softsplat_sum_ordered")
        return out
    N.check(N.lib().mom_softsplat_sum(n, c, H, W, N.ptr(input), N.ptr(flow), N.ptr(out), N.current_stream()), "mom_softsplat_sum")
    return out


EULERIAN_FORM = {"channels": 0, "pixels": 1}     # mom_eulerian_blend's `form`: which index runs on the fastest lanes


def eulerian_blend(feature, motion, idx, n_frames, acc=None, form="channels", ordered=None):
    """blend_feature's cut, reflection padding, two Euler chains and joint splat (cinemagraph_utils.py:131-178) as one launch
    into the channel-last accumulator acc [padded,padded,C+1] (feature Z in the first C channels, Z in the last), which is
    cleared first and returned.  feature [C,S,S], motion [2,S,S].
    ordered (None: as diff_gaussian_rasterization._C.deterministic() says): mom_eulerian_blend_ordered -- entries sorted by cell and
    every texel's sum pulled in the order include/mom4d.h defines, the same bits run after run, whatever `form` says -- out of the
    grow-only scratch _RC.warp_ordered_scratch; False: float atomics, no scratch."""
    if feature.dim() != 3 or motion.dim() != 3 or motion.shape[0] != 2 or feature.shape[0] < 1:
        raise N.MomError(f"eulerian_blend: feature [C,S,S] and motion [2,S,S] are needed, got {tuple(feature.shape)} and "
                         f"{tuple(motion.shape)}")
    c, H, W = feature.shape
    if H != W or tuple(motion.shape[1:]) != (H, W):
        raise N.MomError(f"eulerian_blend: the feature must be square and the motion at its size, got {tuple(feature.shape)} and "
                         f"{tuple(motion.shape)}")
    idx, n_frames = int(idx), int(n_frames)
    if n_frames < 2 or not 0 <= idx < n_frames:
        raise N.MomError(f"eulerian_blend: n_frames >= 2 and 0 <= idx < n_frames are needed, got idx {idx}, n_frames {n_frames}")
    if form not in EULERIAN_FORM:
        raise N.MomError(f"eulerian_blend: form must be one of {sorted(EULERIAN_FORM)}, got {form!r}")
    padded = eulerian_geometry(H)[2]
    tensors = dict(feature=feature, motion=motion)
    if acc is not None:
        if tuple(acc.shape) != (padded, padded, c + 1):
            raise N.MomError(f"eulerian_blend: acc must be [{padded},{padded},{c + 1}], got {tuple(acc.shape)}")
        tensors["acc"] = acc
    _f32_device("eulerian_blend", **tensors)
    if acc is None:
        acc = torch.empty((padded, padded, c + 1), dtype=torch.float32, device=feature.device)
    if _warp_ordered(ordered):
        need = N.lib().mom_eulerian_ordered_scratch_bytes(c, H)
        if need == 0:
            raise N.MomError(f"eulerian_blend: the ordered blend does not take {tuple(feature.shape)} (include/mom4d.h has its limits)")
        scratch = _RC.warp_ordered_scratch(need, feature.device)
        N.check(N.lib().mom_eulerian_blend_ordered(c, H, W, idx, n_frames, N.ptr(feature), N.ptr(motion), N.ptr(acc), N.ptr(scratch),
                                                   scratch.numel(), N.current_stream()), "mom_eulerian_blend_ordered")
        return acc
    N.check(N.lib().mom_eulerian_blend(c, H, W, idx, n_frames, EULERIAN_FORM[form], N.ptr(feature), N.ptr(motion), N.ptr(acc),
                                       N.current_stream()), "mom_eulerian_blend")
    return acc


def eulerian_finish(acc, S, full=False, return_blank=False, out=None):
    """The rest of warp_one_level in one launch (softmax_splatting.py:341-344, cinemagraph_utils.py:498-531, 77-83): acc
    [padded,padded,C+1] as eulerian_blend leaves it -> [C,S,S], normalised, the blank pixels (weight 0) filled with the 7 x 7 box
    mean, cropped.  full=True: the whole normalised map [C,padded,padded] without the fill (blend_feature's return).
    return_blank: also the blank mask of what is returned, torch.uint8."""
    cut, pad, padded, crop0 = eulerian_geometry(S)
    if acc.dim() != 3 or tuple(acc.shape[:2]) != (padded, padded) or acc.shape[2] < 2:
        raise N.MomError(f"eulerian_finish: acc must be [{padded},{padded},C+1] for S = {S}, got {tuple(acc.shape)}")
    _f32_device("eulerian_finish", acc=acc)
    c, size = acc.shape[2] - 1, padded if full else S
    if out is None:
        out = torch.empty((c, size, size), dtype=torch.float32, device=acc.device)
    elif tuple(out.shape) != (c, size, size) or out.dtype != torch.float32 or not out.is_contiguous() or out.device != acc.device:
        raise N.MomError(f"eulerian_finish: out must be a contiguous torch.float32 [{c},{size},{size}] tensor on {acc.device}")
    blank = torch.empty((size, size), dtype=torch.uint8, device=acc.device) if return_blank else None
    N.check(N.lib().mom_eulerian_finish(c, S, int(bool(full)), N.ptr(acc), N.ptr(out), N.ptr(blank), N.current_stream()),
            "mom_eulerian_finish")
    return (out, blank) if return_blank else out


# --------------------------------------------------------------------------- StyleGAN2's native ops (csrc/stylegan_ops.hip)
def upfirdn2d_out_size(H, W, kh, kw, up, down, pad):
    """(out_h, out_w) of op/upfirdn2d.py:100-101; Python's floor division, so a negative numerator gives a size below 1."""
    (ux, uy), (dx, dy), (px0, px1, py0, py1) = up, down, pad
    return (H * uy + py0 + py1 - kh) // dy + 1, (W * ux + px0 + px1 - kw) // dx + 1


def upfirdn2d(input, kernel, up=(1, 1), down=(1, 1), pad=(0, 0, 0, 0)):
    """upfirdn2d of the reference's StyleGAN2 (op/upfirdn2d.py:85-121): input [N,C,H,W], kernel [kh,kw], up (ux,uy), down (dx,dy),
    pad (px0,px1,py0,py1) of either sign -> [N,C,out_h,out_w].  One launch; the definition is include/mom4d.h's."""
    if input.dim() != 4 or kernel.dim() != 2 or 0 in input.shape or 0 in kernel.shape:
        raise N.MomError(f"upfirdn2d: input [N,C,H,W] and kernel [kh,kw] are needed, got {tuple(input.shape)} and "
                         f"{tuple(kernel.shape)}")
    try:
        (ux, uy), (dx, dy), (px0, px1, py0, py1) = ([int(v) for v in t] for t in (up, down, pad))
    except (TypeError, ValueError):
        raise N.MomError(f"upfirdn2d: up (ux,uy), down (dx,dy) and pad (px0,px1,py0,py1) are needed, got {up!r}, {down!r}, "
                         f"{pad!r}") from None
    n, c, H, W = input.shape
    kh, kw = kernel.shape
    if min(ux, uy, dx, dy) < 1 or max(kh, kw) > 32:
        raise N.MomError(f"upfirdn2d: factors >= 1 and a kernel of at most 32 x 32 are needed, got up {(ux, uy)}, down {(dx, dy)}, "
                         f"kernel {(kh, kw)}")
    out_h, out_w = upfirdn2d_out_size(H, W, kh, kw, (ux, uy), (dx, dy), (px0, px1, py0, py1))
    if out_h < 1 or out_w < 1:
        raise N.MomError(f"upfirdn2d: the output would be [{out_h},{out_w}] for input {tuple(input.shape)}, kernel {(kh, kw)}, "
                         f"up {(ux, uy)}, down {(dx, dy)}, pad {(px0, px1, py0, py1)}")
    _f32_device("upfirdn2d", input=input, kernel=kernel)
    out = torch.empty((n, c, out_h, out_w), dtype=torch.float32, device=input.device)
    N.check(N.lib().mom_upfirdn2d(n * c, H, W, kh, kw, ux, uy, dx, dy, px0, px1, py0, py1, N.ptr(input), N.ptr(kernel), N.ptr(out),
                                  N.current_stream()), "mom_upfirdn2d")
    return out


def fused_bias_act(input, bias, ref, act, grad, alpha, scale):
    """fused_bias_act of the reference's StyleGAN2 (fused_bias_act_kernel.cu): input of 1 to 5 dimensions, bias (or None) 1-D with
    size(1) elements (size(0) for a 1-D input), ref (or None) like input; act 1 (linear) or 3 (leaky ReLU), grad 0..2 -> like input.
    One launch; the table of cases is include/mom4d.h's."""
    if not 1 <= input.dim() <= 5 or input.numel() < 1:
        raise N.MomError(f"fused_bias_act: an input of 1 to 5 dimensions is needed, got {tuple(input.shape)}")
    act, grad = int(act), int(grad)
    if act not in (1, 3) or not 0 <= grad <= 2:
        raise N.MomError(f"fused_bias_act: act must be 1 or 3 and grad 0, 1 or 2, got act {act}, grad {grad}")
    channels = input.shape[1] if input.dim() > 1 else input.shape[0]
    tensors = dict(input=input)
    if bias is not None:
        if bias.dim() != 1 or bias.shape[0] != channels:
            raise N.MomError(f"fused_bias_act: bias must be [{channels}] for input {tuple(input.shape)}, got {tuple(bias.shape)}")
        tensors["bias"] = bias
    if ref is not None:
        if ref.shape != input.shape:
            raise N.MomError(f"fused_bias_act: ref must be {tuple(input.shape)} like input, got {tuple(ref.shape)}")
        tensors["ref"] = ref
    elif act == 3 and grad == 1:
        raise N.MomError("fused_bias_act: act 3, grad 1 selects by the sign of ref; ref is None")
    _f32_device("fused_bias_act", **tensors)
    step_b = math.prod(input.shape[2:])
    out = torch.empty_like(input)
    N.check(N.lib().mom_fused_bias_act(input.numel(), step_b, channels, act, grad, float(alpha), float(scale), N.ptr(input),
                                       N.ptr(bias), N.ptr(ref), N.ptr(out), N.current_stream()), "mom_fused_bias_act")
    return out


# --------------------------------------------------------------------------- around stage 1's flow estimator (csrc/flow_frame.hip)
def _typed(what, dev, *want):
    for name, t_, shape, dtype in want:
        if tuple(t_.shape) != tuple(shape) or t_.dtype != dtype or t_.device != dev or not t_.is_contiguous():
            raise N.MomError(f"{what}: {name} must be a contiguous {dtype} {list(shape)} tensor on {dev}, "
                             f"got {t_.dtype} {list(t_.shape)} on {t_.device}")


def hint_field(hint_pos, hint_start, hint_end, hint_count, sigma, mask, size):
    """The dense hint field and the resized mask in front of the reference's flow estimator (demo.py:73-105,
    generate_mask_hints_from_user) for all V views in one call: hint_pos [V,n,2] int32 (x, y), hint_start / hint_end [V,n,2] float64
    (the motion is (end - start) / 50), hint_count [V] int32 (rows used per view), sigma [V] float32, mask [V,H,W] uint8, size = S
    -> (hints [V,2,S,S], mask_s [V,1,S,S]) float32.  Two launches; the arithmetic is include/mom4d.h's."""
    if mask.dim() != 3 or hint_pos.dim() != 3 or 0 in mask.shape:
        raise N.MomError(f"hint_field: mask [V,H,W] and hint_pos [V,n,2] are needed, got {tuple(mask.shape)} and {tuple(hint_pos.shape)}")
    (V, H, W), n, S, dev = mask.shape, hint_pos.shape[1], int(size), mask.device
    if S < 1 or n > N.HINTS_MAX:
        raise N.MomError(f"hint_field: size >= 1 and at most {N.HINTS_MAX} hints a view are needed, got size {S}, {n} hints")
    _typed("hint_field", dev, ("mask", mask, (V, H, W), torch.uint8), ("hint_pos", hint_pos, (V, n, 2), torch.int32),
           ("hint_start", hint_start, (V, n, 2), torch.float64), ("hint_end", hint_end, (V, n, 2), torch.float64),
           ("hint_count", hint_count, (V,), torch.int32), ("sigma", sigma, (V,), torch.float32))
    _need_cuda(mask, "hint_field")
    nbytes = int(N.lib().mom_hint_field_scratch_bytes(V, H, W))
    if nbytes == 0:
        raise N.MomError(f"hint_field: {V} views of {H} x {W} pixels are more than the kernels index")
    scratch = torch.empty(nbytes // 4, dtype=torch.float32, device=dev)
    hints = torch.empty((V, 2, S, S), dtype=torch.float32, device=dev)
    mask_s = torch.empty((V, 1, S, S), dtype=torch.float32, device=dev)
    N.check(N.lib().mom_hint_field(V, H, W, S, n, N.ptr(hint_pos), N.ptr(hint_start), N.ptr(hint_end), N.ptr(hint_count), N.ptr(sigma),
                                   N.ptr(mask), N.ptr(hints), N.ptr(mask_s), scratch.data_ptr(), nbytes, N.current_stream()),
            "mom_hint_field")
    return hints, mask_s


def flow_finish(pred, mask_s, H, W):
    """What the reference does to its estimator's output (renderer.py:598-606) for all V views in one call: pred [V,2,S,S],
    mask_s [V,1,S,S] -> flow [V,2,H,W]: pred * mask, the 15 x 15 box mean with a zero border (the reference's loop of seven blurs
    keeps one), * mask, scale by (W / S, H / S), bilinear resize.  Two launches."""
    if pred.dim() != 4 or pred.shape[1] != 2 or pred.shape[2] != pred.shape[3] or 0 in pred.shape:
        raise N.MomError(f"flow_finish: pred must be [V,2,S,S], got {tuple(pred.shape)}")
    V, _, S, _ = pred.shape
    H, W = int(H), int(W)
    if H < 1 or W < 1:
        raise N.MomError(f"flow_finish: H and W >= 1 are needed, got {H} x {W}")
    if tuple(mask_s.shape) != (V, 1, S, S):
        raise N.MomError(f"flow_finish: mask_s must be [{V},1,{S},{S}] like pred, got {tuple(mask_s.shape)}")
    _f32_device("flow_finish", pred=pred, mask_s=mask_s)
    nbytes = int(N.lib().mom_flow_finish_scratch_bytes(V, S))
    if nbytes == 0 or V * 2 * H * W >= 2 ** 31:
        raise N.MomError(f"flow_finish: {V} views of {S} x {S} -> {H} x {W} pixels are more than the kernels index")
    scratch = torch.empty(nbytes // 4, dtype=torch.float32, device=pred.device)
    flow = torch.empty((V, 2, H, W), dtype=torch.float32, device=pred.device)
    N.check(N.lib().mom_flow_finish(V, S, H, W, N.ptr(pred), N.ptr(mask_s), N.ptr(flow), scratch.data_ptr(), nbytes,
                                    N.current_stream()), "mom_flow_finish")
    return flow


# --------------------------------------------------------------------------- PNG: the IDAT's zlib stream on the device
def png_bound(C_, H, W):
    """Bytes that always hold the stream of an [H,W,C_] image (mom_png_bound; 0: unsupported shape)."""
    return int(N.lib().mom_png_bound(C_, H, W))


def png_scratch(C_, H, W, device):
    """The uint8 device scratch png_encode needs for an [H,W,C_] image; reusable by later calls on the same stream."""
    if torch.device(device).type != "cuda":
        raise N.MomError(f"png_scratch: libmom4d has no CPU path (got device {device})")
    n = int(N.lib().mom_png_scratch_bytes(C_, H, W))
    if n == 0:
        raise N.MomError(f"png_scratch: unsupported image shape C {C_}, H {H}, W {W}")
    return torch.empty(n, dtype=torch.uint8, device=device)


def png_encode(rgb8, out, out_size, scratch):
    """rgb8 [H,W,C] uint8 (what mom_image_to_rgb8 writes; C 1, 3 or 4) -> out [>= png_bound] uint8: the complete zlib stream of the
    image's PNG scanlines, its length in out_size [1] int32 (csrc/png_encode.hip).  utils.image_io.png_from_zlib_stream frames
    out[:out_size] as a file.  Enqueued on the current stream; nothing is read back, bytes of out behind the stream are untouched."""
    _need_cuda(rgb8, "png_encode")
    if rgb8.dim() != 3 or rgb8.dtype != torch.uint8 or not rgb8.is_contiguous():
        raise N.MomError(f"png_encode: rgb8 must be a contiguous uint8 [H,W,C] tensor, got {rgb8.dtype} {list(rgb8.shape)}")
    H, W, C_ = rgb8.shape
    bound = png_bound(C_, H, W)
    if bound == 0:
        raise N.MomError(f"png_encode: unsupported image shape C {C_}, H {H}, W {W}")
    for name, t_, dtype, n in (("out", out, torch.uint8, bound), ("out_size", out_size, torch.int32, 1),
                               ("scratch", scratch, torch.uint8, N.lib().mom_png_scratch_bytes(C_, H, W))):
        if t_.dtype != dtype or t_.device != rgb8.device or not t_.is_contiguous() or t_.numel() < n:
            raise N.MomError(f"png_encode: {name} must be a contiguous {dtype} tensor of at least {n} elements on {rgb8.device}, "
                             f"got {t_.dtype} {list(t_.shape)} on {t_.device}")
    N.check(N.lib().mom_png_encode(C_, H, W, rgb8.data_ptr(), out.data_ptr(), out.numel(), out_size.data_ptr(), scratch.data_ptr(),
                                   N.current_stream()), "mom_png_encode")
    return out


# --------------------------------------------------------------------------- PIL's bicubic resize (csrc/pil_resize.hip)
_PIL_TABLES = {}          # (device, in, out) -> (bounds [out,2], kk [out,ksize]) int32 on the device, uploaded once


def pil_resize_coeffs(in_size, out_size):
    """PIL's bicubic resampling tables of one axis on the host (mom_pil_resize_coeffs; no GPU): bounds [out,2] = (xmin, n) and
    kk [out,ksize] int32, the weights in 22 fractional bits."""
    ksize = int(N.lib().mom_pil_resize_ksize(in_size, out_size, N.RESIZE_BICUBIC))
    if ksize < 1:
        raise N.MomError(f"pil_resize: no bicubic tables for {in_size} -> {out_size} samples")
    bounds, kk = np.empty((out_size, 2), np.int32), np.empty((out_size, ksize), np.int32)
    N.check(N.lib().mom_pil_resize_coeffs(in_size, out_size, N.RESIZE_BICUBIC, bounds.ctypes.data, kk.ctypes.data), "mom_pil_resize_coeffs")
    return bounds, kk


def _pil_tables(in_size, out_size, dev):
    if in_size == out_size:
        return None, None                # the axis is skipped, its tables are not read
    key = (dev, in_size, out_size)
    if key not in _PIL_TABLES:
        _PIL_TABLES[key] = tuple(torch.from_numpy(a).to(dev) for a in pil_resize_coeffs(in_size, out_size))
    return _PIL_TABLES[key]


def pil_resize_scratch(shape, size, device):
    """The uint8 intermediate pil_resize needs for images of `shape` ([N,H,W,C], [H,W,C] or [H,W]) resized to size = (OW, OH), or
    None when it needs none (the height does not change); reusable by later calls on the same stream."""
    N_, H, W, C_ = _pil_shape(shape)
    n = int(N.lib().mom_pil_resize_scratch_bytes(N_, H, W, C_, int(size[1]), int(size[0])))
    return torch.empty(n, dtype=torch.uint8, device=device) if n else None


def _pil_shape(shape):
    shape = tuple(int(s) for s in shape)
    if len(shape) == 2:
        return (1,) + shape + (1,)
    if len(shape) == 3:
        return (1,) + shape
    if len(shape) == 4:
        return shape
    raise N.MomError(f"pil_resize: images are [N,H,W,C], [H,W,C] or [H,W], got {list(shape)}")


def pil_resize(src, size, to8b=False, out=None, scratch=None):
    """PIL's Image.resize(size, Image.BICUBIC) of 8-bit "L" or "RGB" images, byte for byte, on the device (csrc/pil_resize.hip; the
    arithmetic is include/mom4d.h's).  src: uint8 [N,H,W,C], [H,W,C] or [H,W] with C 1 or 3 (RGBA is refused: PIL premultiplies
    alpha there); size = (OW, OH) as PIL takes it; returns uint8 of src's rank at [OH,OW].  to8b=True: src is float32 and every
    sample first goes through (x * 255).astype(uint8) -- truncated, and clamped to 0..255 where numpy's cast is platform-defined.
    out: where the result goes (uint8, contiguous, the result's shape) -- an AsyncPNGWriter's slot, say; scratch: the intermediate
    of pil_resize_scratch, for a caller that resizes many frames of one shape.  The coefficient tables are computed on the host once
    per (device, in, out) and stay on the device.  One launch per axis on the current stream, nothing is read back."""
    _need_cuda(src, "pil_resize")
    want = torch.float32 if to8b else torch.uint8
    if src.dtype != want or not src.is_contiguous():
        raise N.MomError(f"pil_resize: src must be a contiguous {want} tensor (to8b={bool(to8b)}), got {src.dtype} {list(src.shape)}"
                         f"{'' if src.is_contiguous() else ', not contiguous'}")
    N_, H, W, C_ = _pil_shape(src.shape)
    OW, OH = int(size[0]), int(size[1])
    if C_ not in (1, 3) or min(N_, H, W, OW, OH) < 1:
        raise N.MomError(f"pil_resize: {N_} images of {H} x {W} x {C_} -> {OH} x {OW}: one or three channels and sizes >= 1 are needed")
    dev = src.device
    shape = {2: (OH, OW), 3: (OH, OW, C_), 4: (N_, OH, OW, C_)}[src.dim()]
    if out is None:
        out = torch.empty(shape, dtype=torch.uint8, device=dev)
    else:
        _typed("pil_resize", dev, ("out", out, shape, torch.uint8))
    need = int(N.lib().mom_pil_resize_scratch_bytes(N_, H, W, C_, OH, OW))
    if need and scratch is None:
        scratch = torch.empty(need, dtype=torch.uint8, device=dev)
    elif need and (scratch.dtype != torch.uint8 or scratch.device != dev or not scratch.is_contiguous() or scratch.numel() < need):
        raise N.MomError(f"pil_resize: scratch must be a contiguous uint8 tensor of at least {need} elements on {dev}, "
                         f"got {scratch.dtype} {list(scratch.shape)} on {scratch.device}")
    bx, kx = _pil_tables(W, OW, dev)
    by, ky = _pil_tables(H, OH, dev)
    fn = N.lib().mom_pil_resize_to8b if to8b else N.lib().mom_pil_resize
    N.check(fn(N_, H, W, C_, src.data_ptr(), OH, OW, N.RESIZE_BICUBIC, N.ptr(bx), N.ptr(kx), N.ptr(by), N.ptr(ky), out.data_ptr(),
               N.ptr(scratch) if need else None, need, N.current_stream()),
            "mom_pil_resize_to8b" if to8b else "mom_pil_resize")
    return out


# --------------------------------------------------------------------------- scattered values -> the pixel grid (stage 1)
def _tri_views(name, pts, pt_off, H, W):
    """Checks shared by tri_resample and pcd_compose; returns (V, N, device)."""
    _need_cuda(pts, name)
    dev = pts.device
    if pts.dim() != 2 or pts.shape[1] != 2 or pts.dtype != torch.float64 or not pts.is_contiguous():
        raise N.MomError(f"{name}: pts must be a contiguous torch.float64 [N,2] tensor, got {pts.dtype} {list(pts.shape)}")
    if pt_off.dim() != 1 or pt_off.numel() < 2 or pt_off.dtype != torch.int32 or pt_off.device != dev or not pt_off.is_contiguous():
        raise N.MomError(f"{name}: pt_off must be a contiguous torch.int32 [V+1] tensor on {dev} with V >= 1, "
                         f"got {pt_off.dtype} {list(pt_off.shape)} on {pt_off.device}")
    V = pt_off.numel() - 1
    if N.lib().mom_tri_resample_scratch_bytes(V, H, W) == 0:
        raise N.MomError(f"{name}: unsupported shape V {V}, H {H}, W {W}")
    return V, pts.shape[0], dev


def delaunay_scratch_elements(V, H, W, n):
    """int32 elements of scratch ops.delaunay needs for V views of H x W with n points in all (0: a shape it refuses)."""
    return (N.lib().mom_delaunay_scratch_bytes(int(V), int(H), int(W), int(n)) + 3) // 4


def delaunay(pts, pt_off, H, W, tris=None, tri_off=None, status=None, scratch=None):
    """The Delaunay triangulation of every view's points, on the device (csrc/delaunay.hip; include/mom4d.h has the canonical
    form, the predicates and the status codes).  Enqueued on the current stream; nothing is read back.

    pts [N,2] float64, the views' points concatenated; pt_off [V+1] int32 (not read on the host): as for tri_resample.  Returns
    (tris [2N,3] int32, indices local to the view, of which the first tri_off[V] rows are written; tri_off [V+1] int32;
    status [V] int32, N.DELAUNAY_OK or why the view has no triangles).  tris[:tri_off[V]] and tri_off go to tri_resample as they
    are.  tris, tri_off, status: tensors to write into, or None; scratch: an int32 tensor of at least
    delaunay_scratch_elements(V, H, W, N) elements to reuse, or None.  Afterwards scratch[0] is the number of deferred points and
    scratch[1] the largest star of the call."""
    V, n, dev = _tri_views("delaunay", pts, pt_off, H, W)
    need = delaunay_scratch_elements(V, H, W, n)
    if need == 0:
        raise N.MomError(f"delaunay: unsupported shape V {V}, H {H}, W {W}, N {n}")
    given = [("tris", tris, (2 * n, 3)), ("tri_off", tri_off, (V + 1,)), ("status", status, (V,))]
    for name, t_, shape in given:
        if t_ is not None and (tuple(t_.shape) != shape or t_.dtype != torch.int32 or t_.device != dev or not t_.is_contiguous()):
            raise N.MomError(f"delaunay: {name} must be a contiguous torch.int32 {list(shape)} tensor on {dev}, "
                             f"got {t_.dtype} {list(t_.shape)} on {t_.device}")
    tris, tri_off, status = (torch.empty(shape, dtype=torch.int32, device=dev) if t_ is None else t_ for _, t_, shape in given)
    if scratch is None:
        scratch = torch.empty(need, dtype=torch.int32, device=dev)
    elif scratch.dtype != torch.int32 or scratch.device != dev or not scratch.is_contiguous() or scratch.numel() < need:
        raise N.MomError(f"delaunay: scratch must be a contiguous torch.int32 tensor of at least {need} elements on {dev}")
    N.check(N.lib().mom_delaunay(V, H, W, n, N.ptr(pts), pt_off.data_ptr(), N.ptr(tris), tri_off.data_ptr(), status.data_ptr(),
                                 scratch.data_ptr(), scratch.numel() * 4, N.current_stream()), "mom_delaunay")
    return tris, tri_off, status


def tri_resample(pts, pt_off, tris, tri_off, values, H, W, fill=0.0, out=None, scratch=None):
    """Linear interpolation of values given at each view's projected points, at every pixel centre: what
    scipy.interpolate.griddata(points, values, pixel grid, "linear", fill_value=fill) gives (train_motion.py:198,304,319), for all
    V views in one call, from the views' triangulations (csrc/tri_resample.hip; include/mom4d.h has the arithmetic and the
    lowest-index rule).  Enqueued on the current stream; nothing is read back.

    pts [N,2] float64, the views' points concatenated; pt_off [V+1] int32; tris [T,3] int32, indices local to the view;
    tri_off [V+1] int32 (both offset arrays non-decreasing from 0 to N / T: they are not read on the host); values [N,C] float32,
    1 <= C <= 8: contiguous on one device.  Returns out [V,H,W,C] float64 (allocated when not given).  scratch: an int32 tensor
    of at least V*H*W elements to reuse, or None."""
    V, n, dev = _tri_views("tri_resample", pts, pt_off, H, W)
    if values.dim() != 2 or not 1 <= values.shape[1] <= 8:
        raise N.MomError(f"tri_resample: values must be [N,C] with 1 <= C <= 8, got {tuple(values.shape)}")
    C_ = values.shape[1]
    if tris.dim() != 2:
        raise N.MomError(f"tri_resample: tris must be [T,3], got {tuple(tris.shape)}")
    T = tris.shape[0]
    want = [("tris", tris, (T, 3), torch.int32), ("tri_off", tri_off, (V + 1,), torch.int32),
            ("values", values, (n, C_), torch.float32)]
    if out is not None:
        want.append(("out", out, (V, H, W, C_), torch.float64))
    for name, t_, shape, dtype in want:
        if tuple(t_.shape) != shape or t_.dtype != dtype or t_.device != dev or not t_.is_contiguous():
            raise N.MomError(f"tri_resample: {name} must be a contiguous {dtype} {list(shape)} tensor on {dev}, "
                             f"got {t_.dtype} {list(t_.shape)} on {t_.device}")
    if out is None:
        out = torch.empty((V, H, W, C_), dtype=torch.float64, device=dev)
    if scratch is None:
        scratch = torch.empty(V * H * W, dtype=torch.int32, device=dev)
    elif scratch.dtype != torch.int32 or scratch.device != dev or not scratch.is_contiguous() or scratch.numel() < V * H * W:
        raise N.MomError(f"tri_resample: scratch must be a contiguous torch.int32 tensor of at least {V * H * W} elements on {dev}")
    N.check(N.lib().mom_tri_resample(V, H, W, C_, n, T, N.ptr(pts), pt_off.data_ptr(), N.ptr(tris), tri_off.data_ptr(),
                                     N.ptr(values), float(fill), out.data_ptr(), scratch.data_ptr(), scratch.numel() * 4,
                                     N.current_stream()), "mom_tri_resample")
    return out


def pcd_compose(resampled, pts, pt_off):
    """The per-pixel remainder of the reference's render_PCD (train_motion.py:298-330,355,357) for V views: border, hit map, 9 x 9
    dilation, 11 x 11 erosions, the 8-bit cast (csrc/tri_resample.hip; include/mom4d.h lists the steps).  resampled [V,H,W,4]
    float64 = tri_resample of (r, g, b, mask) with fill 0; pts, pt_off as for tri_resample.  Returns (image [V,H,W,3],
    mask [V,H,W]) uint8 on the device.  Enqueued on the current stream; nothing is read back."""
    if resampled.dim() != 4 or resampled.shape[3] != 4 or resampled.dtype != torch.float64 or not resampled.is_contiguous():
        raise N.MomError(f"pcd_compose: resampled must be a contiguous torch.float64 [V,H,W,4] tensor, got {resampled.dtype} "
                         f"{list(resampled.shape)}")
    _, H, W, _ = resampled.shape
    V, n, dev = _tri_views("pcd_compose", pts, pt_off, H, W)
    if resampled.shape[0] != V or resampled.device != dev:
        raise N.MomError(f"pcd_compose: resampled has {resampled.shape[0]} views on {resampled.device}, pt_off {V} on {dev}")
    nbytes = int(N.lib().mom_pcd_compose_scratch_bytes(V, H, W))
    if nbytes == 0:
        raise N.MomError(f"pcd_compose: unsupported shape V {V}, H {H}, W {W} (H, W >= 5)")
    image = torch.empty((V, H, W, 3), dtype=torch.uint8, device=dev)
    mask = torch.empty((V, H, W), dtype=torch.uint8, device=dev)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    N.check(N.lib().mom_pcd_compose(V, H, W, n, resampled.data_ptr(), N.ptr(pts), pt_off.data_ptr(), image.data_ptr(),
                                    mask.data_ptr(), scratch.data_ptr(), nbytes, N.current_stream()), "mom_pcd_compose")
    return image, mask


# --------------------------------------------------------------------------- densification statistics
def densify_stats(radii, viewspace_grad, max_radii2D, xyz_gradient_accum, denom, skip_flag=None, stream=None):
    """In place, for the Gaussians with radii > 0: running maximum radius, accumulated |dL/d mean2D| and its count
    (train_4DGS.py:266, scene/gaussian_model.py:713-715).  `skip_flag`: optional int32 device word; nonzero makes the
    launch a no-op (FusedAdam.skip_flag has the story)."""
    _need_cuda(radii, "densify_stats")
    P = radii.shape[0]
    for t_, n_ in ((max_radii2D, P), (xyz_gradient_accum, P), (denom, P)):
        if t_.numel() != n_ or not t_.is_contiguous() or t_.dtype != torch.float32:
            raise N.MomError("densify_stats: accumulators must be contiguous float32 tensors with one element per Gaussian")
    if radii.dtype != torch.int32 or not radii.is_contiguous():
        raise N.MomError("densify_stats: radii must be a contiguous int32 tensor")
    g = viewspace_grad
    if g.shape != (P, 3) or g.dtype != torch.float32 or not g.is_contiguous():
        raise N.MomError("densify_stats: viewspace gradient must be a contiguous float32 [P,3] tensor")
    N.check(N.lib().mom_densify_stats(P, radii.data_ptr(), g.data_ptr(), max_radii2D.data_ptr(), xyz_gradient_accum.data_ptr(),
                                      denom.data_ptr(), None if skip_flag is None else skip_flag.data_ptr(),
                                      N.current_stream() if stream is None else stream), "mom_densify_stats")


# --------------------------------------------------------------------------- SSIM
def ssim_window():
    """The 11 taps of the reference's gaussian(11, 1.5) (utils/loss_utils.py:29-31), computed the way it computes them
    (python doubles rounded to float32, then normalised in float32), as a ctypes array for the C ABI."""
    from math import exp
    g = torch.tensor([exp(-(x - 5) ** 2 / float(2 * 1.5 ** 2)) for x in range(11)], dtype=torch.float32)
    g = g / g.sum()
    return (C.c_float * 11)(*g.tolist())


_SSIM_WINDOW = None


def _ssim_window():
    global _SSIM_WINDOW
    if _SSIM_WINDOW is None:
        _SSIM_WINDOW = ssim_window()
    return _SSIM_WINDOW


class SSIMFunction(torch.autograd.Function):
    """mean SSIM of two images (reference utils/loss_utils.py:52-92 with its default window), gradient w.r.t. img1."""

    @staticmethod
    def forward(ctx, img1, img2):
        _need_cuda(img1, "ssim")
        a = img1.detach().contiguous().float()
        b = img2.detach().contiguous().float()
        if a.shape != b.shape or a.dim() < 3:
            raise N.MomError(f"ssim: expected two [...,C,H,W] images of one shape, got {tuple(a.shape)} and {tuple(b.shape)}")
        H, W = a.shape[-2], a.shape[-1]
        Cn = a.numel() // max(1, H * W)
        need_grad = ctx.needs_input_grad[0]
        dm = torch.empty((3,) + tuple(a.shape), dtype=torch.float32, device=a.device) if need_grad else None
        total = torch.empty(N.SSIM_SUM_SLOTS, dtype=torch.float64, device=a.device)      # [0] = the sum, the rest scratch
        if _RC.deterministic() and a.numel():      # the workgroup totals stored and folded in the documented order; dm is the same bits
            lib = N.lib()
            scratch = _RC.value_ordered_scratch("ssim", lib.mom_ssim_ordered_scratch_bytes(Cn, H, W), a.device)
            N.check(lib.mom_ssim_forward_ordered(Cn, H, W, _ssim_window(), a.data_ptr(), b.data_ptr(),
                                                 None if dm is None else dm.data_ptr(), total.data_ptr(), scratch.data_ptr(),
                                                 scratch.numel(), N.current_stream()), "mom_ssim_forward_ordered")
        else:
            N.check(N.lib().mom_ssim_forward(Cn, H, W, _ssim_window(), a.data_ptr(), b.data_ptr(),
                                             None if dm is None else dm.data_ptr(), total.data_ptr(), N.current_stream()),
                    "mom_ssim_forward")
        if need_grad:
            ctx.save_for_backward(a, b, dm)
        ctx.dims = (Cn, H, W)
        return (total[0] / max(1, a.numel())).float().reshape(())

    @staticmethod
    def backward(ctx, g):
        a, b, dm = ctx.saved_tensors
        Cn, H, W = ctx.dims
        dimg = torch.zeros_like(a)
        g = g.detach().contiguous().float()
        N.check(N.lib().mom_ssim_backward(Cn, H, W, _ssim_window(), a.data_ptr(), b.data_ptr(), dm.data_ptr(),
                                          1.0 / max(1, a.numel()), g.data_ptr(), dimg.data_ptr(), N.current_stream()),
                "mom_ssim_backward")
        return dimg, None


def ssim(img1, img2):
    return SSIMFunction.apply(img1, img2)


# --------------------------------------------------------------------------- second stream of the autograd path
# OFF by default: measured in one process, alternating (tools/probe/api_leg.py, config 2): with it the path enqueues a step in 1.08
# instead of 0.95 ms of host time (a second Adam launch, a dozen ordering calls) and the HOST is what paces this path -- 925 against
# 1015 steps/s in async mode, 745 against 780-920 in exact mode.  It pays only where the GPU is the bottleneck (larger models, a
# faster host); MOM_API_OVERLAP=1 or ops.API_OVERLAP = True switches it on.
API_OVERLAP = _os.environ.get("MOM_API_OVERLAP", "0") == "1"
_side_streams = {}
_reg_pending = {}      # device -> True while the regulariser's gradient kernel may still run on the second stream (mark MARK_REG): the next writer of plane gradients waits
_params_ready = {}     # device -> (stream the last FusedAdam.step() ended on -- mark MARK_PARAMS --, {(id, version)} of every plane it updated)


def side_stream(device):
    """One second stream per device for the render() + loss.backward() path: it carries what does not depend on the compositing
    (the plane regularisers' two kernels), the MLP backward's partial-sum reduction and -- the largest piece -- the appearance
    parameters' Adam launch, which FusedAdam.step() starts there behind the event the backward recorded when those gradients
    became final (fused_autograd.py).  Opt-in (API_OVERLAP above): by default everything stays on the caller's stream."""
    st = _side_streams.get(device)
    if st is None:
        st = _side_streams[device] = torch.cuda.Stream(device=device)
    return st


# Ordering goes through libmom4d's stream helpers (csrc/stream_order.hip), not torch's Stream / Event objects: a dozen of these per
# iteration at 8-10 us each were a tenth of the path's host time.  Mark slots (per device): 0 = the parameters as the last
# FusedAdam.step() left them, 1 = the regulariser's gradient kernel on the second stream, 2 = the fused step's gradient bucket is cleared,
# 3 = a field's prefetched processing orders, 4.. = a ring of 60 for the backward's "appearance gradients final".
MARK_PARAMS, MARK_REG, MARK_BUCKET, MARK_ORDERS, MARK_RING0, MARK_RING_N = 0, 1, 2, 3, 4, 60
_ring = [0]


def stream_wait_stream(waiter, signaler):
    N.check(N.lib().mom_stream_wait_stream(waiter, signaler), "mom_stream_wait_stream")


def stream_mark(slot, stream):
    N.check(N.lib().mom_stream_mark(slot, stream), "mom_stream_mark")


def stream_wait_mark(stream, slot):
    N.check(N.lib().mom_stream_wait_mark(stream, slot), "mom_stream_wait_mark")


def zero_async(t, stream):
    """t.zero_() on a raw stream handle (no torch stream context: entering and leaving one costs ~10 us of host time)."""
    N.check(N.lib().mom_zero_async(t.data_ptr(), t.numel() * t.element_size(), stream), "mom_zero_async")


def next_ring_mark(stream):
    """Record the tail of `stream` under the next slot of the ring; returns the slot (valid until MARK_RING_N more have been taken)."""
    _ring[0] = (_ring[0] + 1) % MARK_RING_N
    slot = MARK_RING0 + _ring[0]
    stream_mark(slot, stream)
    return slot


def wait_reg_pending(device):
    """The current stream waits for a regulariser gradient kernel still running on the second stream (it ADDS into plane gradient
    buffers the caller is about to add into as well)."""
    if _reg_pending.pop(device, None) is not None:
        stream_wait_mark(N.current_stream(), MARK_REG)


def wait_reg_pending_all():
    """The same for every device that has such a kernel in flight: what FusedAdam.step() / zero_grad() and the per-op HexPlane
    backward call before they read or write plane gradients.  The autograd engine knows nothing of the raw second stream, so every
    consumer of the plane gradients that is not render()'s own backward joins here (the dict is empty unless API_OVERLAP is on)."""
    if _reg_pending:
        for dev in list(_reg_pending):
            with torch.cuda.device(dev):
                wait_reg_pending(dev)


# device -> number of fused render() nodes whose backward has not run yet.  The regulariser's gradient kernel may stay un-joined on
# the second stream only while such a node is still to come (its backward joins before it touches the plane gradients); with none
# pending -- the regulariser node runs last, the loss is regulariser-only, render() took the per-op path -- it joins at once.
_render_pending = {}


# --------------------------------------------------------------------------- plane regularisers
def direct_grads_ok(params, needs):
    """May a backward hand these parameters their gradients itself (p.grad = ...) instead of returning them to the engine?  Only
    if the engine would do exactly that with a returned gradient: every one of them is asked for (needs_input_grad), is a leaf
    that requires grad, and carries no tensor hook or post-accumulate hook -- those only fire on the engine's own path.
    (torch.autograd.grad() cannot be told apart from backward() inside a node: callers that use it switch the direct path off,
    fused_autograd.grads_through_graph().)"""
    for p, n in zip(params, needs):
        if not n or not p.requires_grad or not p.is_leaf:
            return False
        if getattr(p, "_backward_hooks", None) or getattr(p, "_post_accumulate_grad_hooks", None):
            return False
    return True


def _buffers_free(views, held_by_cache=1):
    """True if nobody but the cache (held_by_cache references per view) and this call still refers to the cached gradient views: a
    caller that kept a parameter's .grad tensor from the last iteration must not see it zeroed and rewritten."""
    import sys
    return all(sys.getrefcount(v) <= held_by_cache + 2 for v in views)      # + the loop variable and getrefcount's argument


def _reg_row_units(st):
    """MomRegPlane.W of a channel-last [H, W, C] plane.  The regulariser differences along H for every float of a row and never
    looks at where a texel ends, and it counts a row in units of 32 floats: W for 32-channel planes, W / 2 for 16-channel ones."""
    n = st.shape[1] * st.shape[2]
    if n % 32:
        raise N.MomError(f"plane_regulation: a plane row of {st.shape[1]} texels x {st.shape[2]} channels is no multiple of 32 floats")
    return n // 32


class PlaneRegFunction(torch.autograd.Function):
    """value = sum_p  w_smooth[p] * smooth2(plane_p) + w_l1[p] * mean|1 - plane_p|."""

    @staticmethod
    def forward(ctx, w_smooth, w_l1, *planes):
        # the descriptor array holds pointers, shapes and weights only: rebuilt when one of them moves (the loop hands in the same
        # twelve planes every iteration; twelve plane_storage() views and sixty field stores were 40 us of host time per call).
        # The planes' layout and device are checked where it is built: a key that matches names planes that passed
        key = (tuple((p.data_ptr(), p.shape, p.stride()) for p in planes), tuple(w_smooth), tuple(w_l1))
        c = PlaneRegFunction._fwd_cache
        if c is None or c[0] != key:
            arr = (N.MomRegPlane * len(planes))()
            for i, p in enumerate(planes):
                st = plane_storage(p)
                if st is None or p.dtype != torch.float32:
                    raise N.MomError(f"plane_regulation: plane {i} (shape {tuple(p.shape)}, strides {p.stride()}, {p.dtype}) is not a "
                                     "channel-last float32 [1,C,H,W] tensor (ops.make_plane)")
                arr[i].plane, arr[i].grad = st.data_ptr(), None
                arr[i].H, arr[i].W = st.shape[0], _reg_row_units(st)
                arr[i].w_smooth, arr[i].w_l1, arr[i].grad_scale = float(w_smooth[i]), float(w_l1[i]), 0.0
            for p in planes:
                _need_cuda(p, "plane_regulation")
            c = PlaneRegFunction._fwd_cache = (key, arr)
        arr = c[1]
        dev = planes[0].device
        val = torch.empty(1, dtype=torch.float32, device=dev)

        def value(stream):
            lib = N.lib()
            if _RC.deterministic():    # one partial per workgroup, folded in the documented order (include/mom4d.h, "ordered loss values")
                scratch = _RC.value_ordered_scratch("reg", lib.mom_plane_regulation_ordered_scratch_bytes(arr, len(planes)), dev)
                N.check(lib.mom_plane_regulation_ordered(arr, len(planes), val.data_ptr(), scratch.data_ptr(), scratch.numel(), stream),
                        "mom_plane_regulation_ordered")
            else:
                N.check(lib.mom_plane_regulation(arr, len(planes), val.data_ptr(), stream), "mom_plane_regulation")

        if API_OVERLAP:
            # the value depends on the planes only: on the second stream it runs beside the compositing the caller's stream is
            # still busy with (the loop calls this right after render()); the caller's stream waits for it before it reads `val`.
            # The second stream need not wait for the whole of the caller's queue if the planes are exactly as the last
            # FusedAdam.step() left them (same tensors, same versions -- any torch write since would have bumped one): then the
            # event that step recorded is the only dependency
            cur, side = N.current_stream(), side_stream(dev).cuda_stream
            mark = _params_ready.get(dev)
            if mark is not None and mark[0] == cur and mark[1] >= frozenset((id(p), p._version) for p in planes):
                stream_wait_mark(side, MARK_PARAMS)
            else:
                stream_wait_stream(side, cur)
            value(side)
            stream_wait_stream(cur, side)
        else:
            value(N.current_stream())
        ctx.save_for_backward(*planes)
        ctx.w = (list(w_smooth), list(w_l1))
        return val[0]

    @staticmethod
    def backward(ctx, g):
        planes = ctx.saved_tensors
        w_smooth, w_l1 = ctx.w
        # The kernel ADDS the regulariser's share into a plane's gradient.  Planes that already hold one of the right layout (the
        # render node ran first) are accumulated into in place; the others get a view of one flat zeroed buffer, which becomes
        # their gradient.  Handing the gradients to the planes here, instead of returning them, also spares the engine twelve
        # AccumulateGrad nodes and -- a plane has two consumers, this op and render() -- twelve elementwise additions
        # (DIRECT_GRADS = False returns them through the graph).  The buffer and the descriptor are cached between iterations
        # while the planes have let go of last iteration's gradients (zero_grad(set_to_none=True)); the upstream weight stays on
        # the device (float(g) was a host synchronisation in every iteration).
        direct = PlaneRegFunction.DIRECT_GRADS and direct_grads_ok(planes, ctx.needs_input_grad[2:])
        held = [p.grad if direct else None for p in planes]
        in_place = in_place_flags(held, planes)
        # (the shapes belong to the key: the descriptor holds H and W, and two planes of one size may follow each other at one address)
        key = (tuple((p.data_ptr(), p.shape) for p in planes), tuple(w_smooth), tuple(w_l1),
               tuple(h.data_ptr() if ip else 0 for h, ip in zip(held, in_place)))
        c = PlaneRegFunction._cache
        busy = c is not None and (any(h is not None and h.data_ptr() == v.data_ptr() for h, v in zip(held, c[2]))
                                  or not _buffers_free(c[2]))
        if c is None or c[0] != key or busy:
            flat = torch.zeros(sum(p.numel() for p in planes), dtype=torch.float32, device=planes[0].device)
            off, grads = 0, []
            arr = (N.MomRegPlane * len(planes))()
            for i, p in enumerate(planes):
                st = plane_storage(p)
                gv = flat[off:off + p.numel()].view(st.shape)
                off += p.numel()
                grads.append(gv.permute(2, 0, 1).unsqueeze(0))
                target = plane_storage(held[i]) if in_place[i] else gv
                arr[i].plane, arr[i].grad = st.data_ptr(), target.data_ptr()
                arr[i].H, arr[i].W = st.shape[0], _reg_row_units(st)
                arr[i].w_smooth, arr[i].w_l1, arr[i].grad_scale = float(w_smooth[i]), float(w_l1[i]), 1.0
            val = torch.empty(1, dtype=torch.float32, device=planes[0].device)
            c = (key, flat, grads, arr, val)
            if not busy:
                PlaneRegFunction._cache = c
        else:
            c[1].zero_()
        _, flat, grads, arr, val = c
        up = g.detach().reshape(1).float()
        dev = planes[0].device
        if API_OVERLAP and direct:
            # the engine runs this node BEFORE render()'s (it was created later): on the second stream the kernel runs beside the
            # compositing backward; whoever adds into the plane gradients next (the HexPlane backward, a second regulariser call)
            # waits for the event first (wait_reg_pending)
            wait_reg_pending(dev)
            side_t = side_stream(dev)
            cur, side = N.current_stream(), side_t.cuda_stream
            stream_wait_stream(side, cur)              # the upstream weight, and the clearing of the buffer above
            N.check(N.lib().mom_plane_regulation_grad(arr, len(planes), val.data_ptr(), up.data_ptr(), side), "mom_plane_regulation")
            up.record_stream(side_t)                   # (the engine frees it when this node returns; the second stream still reads it)
            if _render_pending.get(dev, 0) > 0:
                stream_mark(MARK_REG, side)
                _reg_pending[dev] = True
            else:
                stream_wait_stream(cur, side)          # nobody downstream is known to join: the caller's stream does, now
        else:
            N.check(N.lib().mom_plane_regulation_grad(arr, len(planes), val.data_ptr(), up.data_ptr(), N.current_stream()),
                    "mom_plane_regulation")
        if direct:
            for p, gp, ip in zip(planes, grads, in_place):
                if not ip:
                    if p.grad is None:
                        p.grad = gp
                    else:
                        wait_reg_pending(dev)          # (a torch op on the caller's stream reads what the second stream writes)
                        p.grad.add_(gp)
            return (None, None) + (None,) * len(planes)
        return (None, None, *[gp if n else None for gp, n in zip(grads, ctx.needs_input_grad[2:])])

    _cache = None
    _fwd_cache = None
    DIRECT_GRADS = True


def plane_regulation(planes, w_smooth, w_l1):
    return PlaneRegFunction.apply(w_smooth, w_l1, *planes)


# --------------------------------------------------------------------------- Adam
# numpy mirror of N.MomAdamTensor (same offsets and size): FusedAdam writes whole columns of its descriptor arrays through it
_ADAM_DT = np.dtype({"names": [n for n, _ in N.MomAdamTensor._fields_],
                     "formats": [{C.c_void_p: np.uint64, C.c_size_t: np.uint64, C.c_float: np.float32}[t] for _, t in N.MomAdamTensor._fields_],
                     "offsets": [getattr(N.MomAdamTensor, n).offset for n, _ in N.MomAdamTensor._fields_],
                     "itemsize": C.sizeof(N.MomAdamTensor)})


def _dense(t):
    """True if t's elements tile its storage span without gaps or overlap (any dim order)."""
    dims = sorted(((st, sz) for st, sz in zip(t.stride(), t.shape) if sz > 1), reverse=True)
    expect = 1
    for st, sz in reversed(dims):
        if st != expect:
            return False
        expect *= sz
    return True


def _same_layout(a, b):
    """Same shape and same strides on every dimension that has more than one element."""
    if a.shape != b.shape:
        return False
    if a.stride() == b.stride():          # the common case, one tuple comparison (this runs 24 times per iteration of the API path)
        return True
    return all(sa == sb for sa, sb, n in zip(a.stride(), b.stride(), a.shape) if n > 1)


_IN_PLACE_MEMO = {}


def in_place_flags(held, planes):
    """[h is a gradient tensor the kernels can add into in place: same layout as its plane, dense] for every plane.  The answer
    depends on the two tensors' storage, shape and strides only, and the loop hands in the SAME buffers iteration after iteration
    (the gradient buffers are cached), so it is remembered: twelve dictionary reads instead of twelve shape-and-stride walks, twice
    per iteration of the API path.  The key holds BOTH tensors' shape and strides beside the pointers: two views of one buffer
    share a pointer and differ in layout."""
    out = []
    for h, p in zip(held, planes):
        if h is None:
            out.append(False)
            continue
        k = (h.data_ptr(), p.data_ptr(), h.shape, h.stride(), p.shape, p.stride())
        v = _IN_PLACE_MEMO.get(k)
        if v is None:
            if len(_IN_PLACE_MEMO) > 4096:
                _IN_PLACE_MEMO.clear()
            v = _IN_PLACE_MEMO[k] = bool(_same_layout(h, p) and _dense(h))
        out.append(v)
    return out


class FusedAdam(torch.optim.Optimizer):
    """torch.optim.Adam (amsgrad=False, weight_decay=0, maximize=False) whose step() is ONE HIP launch over all
    parameters with a gradient.  State layout ('step', 'exp_avg', 'exp_avg_sq') and param_groups are those of
    torch.optim.Adam, so the reference's optimizer-state surgery (scene/gaussian_model.py:409-482) and
    state_dict()/load_state_dict() work unchanged."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8):
        # the other keys are torch.optim.Adam's (all at their defaults: this optimizer implements exactly that configuration), so
        # that a state_dict() written here loads into the reference's torch.optim.Adam and the other way round
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=0, amsgrad=False, maximize=False, foreach=None,
                                      capturable=False, differentiable=False, fused=None, decoupled_weight_decay=False))
        self._plan = None
        self._plans = {}            # "early" / "late": the plans of a step taken in two parts (step_partial)
        self._early = None          # ids of the parameters step_partial() has already advanced in this iteration
        # int32 device word or None.  While it is nonzero on the device a step() changes neither parameters nor moments:
        # the asynchronous training step points it at the rasterizer's sticky overflow word, so that a step whose image was
        # truncated never reaches the model; the host notices later and replays (train.Trainer._recover, rewind()).
        self.skip_flag = None
        # (mark slot, second stream's handle, [(param, its gradient tensor, the gradient's version)]) left by render()'s backward when the
        # appearance parameters' gradients became final, or None: see step()
        self.early_hint = None

    def zero_grad(self, set_to_none=True):
        """torch.optim.Optimizer.zero_grad without its dynamo guard, foreach grouping and profiler range (30 us per call on the
        API path's host, which sets the pace there): the same effect for dense gradients."""
        wait_reg_pending_all()         # a regulariser gradient kernel on the second stream may still be adding into what is dropped here
        for group in self.param_groups:
            for p in group["params"]:
                g = p.grad
                if g is None:
                    continue
                if set_to_none:
                    p.grad = None
                else:
                    if g.grad_fn is not None:
                        g.detach_()
                    else:
                        g.requires_grad_(False)
                    g.zero_()

    def rewind(self, n):
        """Take back the host-side step counters of the last n step() calls (they were no-ops on the device)."""
        for st in self.state.values():
            if "step" in st:
                st["step"] -= float(n)

    def _build_plan(self, live, key, ranges=None):
        """Validate every (param, state) once and lay the MomAdamTensor arrays out; reused until a parameter or a moment moves
        (densify / prune / reset_opacity replace parameters and state, load_state_dict replaces state).  The gradient pointers
        are NOT part of the plan's identity: under autograd the gradients are fresh tensors every iteration, and a plan keyed on
        them was rebuilt in four iterations out of ten (0.5 ms of host time each); they are refreshed per step instead."""
        by_cfg, entries, steps, params = {}, [], [], []
        for group, p in live:
            _need_cuda(p, "FusedAdam")
            st = self.state[p]
            if not _dense(p):
                raise N.MomError("FusedAdam: parameters must be dense")
            b1, b2 = group["betas"]
            cfg = (b1, b2, group["eps"])
            slot = by_cfg.setdefault(cfg, [])
            t = N.MomAdamTensor()
            # ranges (a rank's share of a sharded step, FusedAdam.step_partial): elements [off, off + n) of the tensor in storage
            # order -- Adam is element-wise, so a slice of the parameter, its gradient and its moments is a step of its own; an empty
            # slice stays in the plan with n = 0 (no work) so that the parameter's step counter advances on every rank alike
            off, cnt = (0, p.numel()) if ranges is None else ranges[id(p)]
            if ranges is not None and (not p.is_contiguous() or not st["exp_avg"].is_contiguous() or not st["exp_avg_sq"].is_contiguous()):
                raise N.MomError("FusedAdam: a sharded step needs contiguous parameters and moments")
            t.param = p.data_ptr() + 4 * off
            t.exp_avg, t.exp_avg_sq = st["exp_avg"].data_ptr() + 4 * off, st["exp_avg_sq"].data_ptr() + 4 * off
            t.n = cnt
            entries.append((group, b1, b2, cfg, len(slot)))
            slot.append(t)
            steps.append(st["step"])
            params.append(p)
        arrs = {cfg: (N.MomAdamTensor * len(ts))(*ts) for cfg, ts in by_cfg.items()}
        # numpy views of the descriptor arrays (same memory): a step refreshes three float columns and one pointer column of ~32 rows
        # with four vector assignments instead of ~130 ctypes field stores (0.3 us each: a tenth of the render() path's host time)
        views = {cfg: np.frombuffer(arr, dtype=_ADAM_DT) for cfg, arr in arrs.items()}
        cfg_list = list(arrs)
        rows = {cfg: [] for cfg in cfg_list}            # per configuration: the plan-entry index of every row of its array
        for j, (_, _, _, cfg, i) in enumerate(entries):
            rows[cfg].append(j)
        groups = []
        gidx = []
        for group, _ in live:
            for k, gq in enumerate(groups):
                if gq is group:
                    gidx.append(k)
                    break
            else:
                groups.append(group)
                gidx.append(len(groups) - 1)
        # The step counters of the plan's parameters live in ONE host buffer and every state["step"] is a 0-d view into it (same
        # dtype, same values, still torch.optim.Adam's state layout): advancing and reading thirty-odd separate host tensors cost
        # 65 us per step() (torch._foreach_add_ + torch.stack), a tenth of the API path's host time; one add and one tolist() on the
        # buffer cost 3.  A counter that is replaced (load_state_dict) changes its pointer and with it the plan's key.
        buf = torch.tensor([float(t) for t in steps], dtype=torch.float32)
        for j, (_, p) in enumerate(live):
            self.state[p]["step"] = buf[j]
        return {"key": self._plan_key(live) + (() if ranges is None else (tuple(ranges[id(p)] for _, p in live),)), "entries": entries,
                "step_buf": buf, "arrs": arrs, "params": params, "offs": [0 if ranges is None else ranges[id(p)][0] for _, p in live],
                "views": views, "rows": {cfg: np.asarray(r, dtype=np.int64) for cfg, r in rows.items()}, "groups": groups,
                "gidx": np.asarray(gidx, dtype=np.int64), "offs4": np.asarray([0 if ranges is None else 4 * ranges[id(p)][0] for _, p in live], dtype=np.uint64),
                "last_grad": [(0, None)] * len(params), "betas": [(b1, b2) for _, b1, b2, _, _ in entries]}

    def _plan_key(self, live):
        return tuple((p.data_ptr(), self.state[p]["exp_avg"].data_ptr(), self.state[p]["exp_avg_sq"].data_ptr(),
                      self.state[p]["step"].data_ptr(), p.numel()) for _, p in live)

    def _launch(self, live, which, stream=None, ranges=None):
        state, key = self.state, []
        for _, p in live:               # one pass: create missing state, and read the pointers the plan is keyed on
            st = state[p]
            if len(st) == 0:
                st["step"] = torch.tensor(0.0, dtype=torch.float32)
                st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            key.append((p.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(), st["step"].data_ptr(), p.numel()))
        key = tuple(key)
        if ranges is not None:
            key = key + (tuple(ranges[id(p)] for _, p in live),)
        plan = self._plans.get(which)
        if plan is None or plan["key"] != key:
            plan = self._plans[which] = self._build_plan(live, key, ranges)
        if which is None:
            self._plan = plan
        # this step's gradients: pointers refreshed and strides checked every step.  (Shape, device and dtype need no check here:
        # torch refuses a .grad assignment whose size, device or dtype differs from the parameter's -- THPVariable_set_grad --
        # but it accepts any strides.)
        arrs = plan["arrs"]
        last, ptrs = plan["last_grad"], []
        for j, p in enumerate(plan["params"]):
            g = p.grad
            gp, gs = g.data_ptr(), g.stride()
            seen = last[j]
            # (the same buffer WITH the same strides as last step -- the gradient buffers are cached -- was checked then; the pointer
            # alone says nothing: a contiguous view of the buffer a channel-last gradient lived in has its address)
            if gp != seen[0] or gs != seen[1]:
                if gs != p.stride() and not _same_layout(g, p):
                    raise N.MomError("FusedAdam: param/grad must be dense with identical strides")
                last[j] = (gp, gs)
            ptrs.append(gp)
        plan["step_buf"] += 1
        # the step counters are host tensors the state surgery and rewind() may have touched: read them all in one go, and form
        # the two bias corrections once per distinct (betas, step) -- one or two values, not one per tensor.  Python float
        # arithmetic, exactly as torch.optim.Adam forms them (numpy's pow may round differently in the last place)
        step_vals = plan["step_buf"].tolist()
        bias = {}
        bc1, bc2 = [], []
        for (b1, b2), step in zip(plan["betas"], step_vals):
            bc = bias.get((b1, b2, step))
            if bc is None:
                bc = bias[(b1, b2, step)] = (1.0 - b1 ** step, math.sqrt(1.0 - b2 ** step))
            bc1.append(bc[0])
            bc2.append(bc[1])
        grad_col = np.asarray(ptrs, dtype=np.uint64) + plan["offs4"]
        lr_col = np.asarray([float(gq["lr"]) for gq in plan["groups"]], dtype=np.float64)[plan["gidx"]]
        bc1_col, bc2_col = np.asarray(bc1, dtype=np.float64), np.asarray(bc2, dtype=np.float64)
        for cfg, view in plan["views"].items():
            r = plan["rows"][cfg]
            view["grad"] = grad_col[r]
            view["lr"] = lr_col[r]                      # (float64 -> float32 on assignment: the rounding a ctypes c_float store makes)
            view["bias_correction1"] = bc1_col[r]
            view["bias_correction2_sqrt"] = bc2_col[r]
        for (b1, b2, eps), arr in arrs.items():
            N.check(N.lib().mom_adam_step(arr, len(arr), b1, b2, eps,
                                          None if self.skip_flag is None else self.skip_flag.data_ptr(),
                                          N.current_stream() if stream is None else stream), "mom_adam_step")

    @torch.no_grad()
    def ensure_state(self, params):
        """Create the Adam state of `params` now, on the current stream (torch.optim.Adam creates it in the first step() that sees
        a gradient; a step_partial() on a second stream would otherwise allocate the moments from that stream's pool).
        Returns True if any state was created: its zero fill is queued on the current stream, and a second stream that is to
        read the moments must first wait for THAT stream, not only for an earlier mark."""
        created = False
        for p in params:
            st = self.state[p]
            if len(st) == 0:
                st["step"] = torch.tensor(0.0, dtype=torch.float32)
                st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                created = True
        return created

    @torch.no_grad()
    def step_partial(self, params, stream=None, ranges=None):
        """Advance only `params` (their gradients are final) on the CURRENT stream; the step() that follows in the same iteration
        advances the rest.  The fused training step uses it to put the Gaussians' appearance parameters -- 56 of their 59 floats,
        four fifths of Adam's bytes -- on its second stream underneath the deformation backward (fused_step.py).  Element for
        element the same update as one step(): Adam is element-wise.
        ranges: {id(p): (first element, count)} -- only that slice of each parameter (storage order) is advanced: this rank's share
        of a camera-batch shard whose ranks reduce-scatter the gradients and all-gather the updated parameters (parallel.py)."""
        ids = {id(p) for p in params}
        live = [(group, p) for group in self.param_groups for p in group["params"] if id(p) in ids and p.grad is not None]
        if not live:
            return
        self._launch(live, "early" if ranges is None else "early-sharded", stream=stream, ranges=ranges)
        self._early = {id(p) for _, p in live}

    @torch.no_grad()
    def step(self, closure=None):
        # (torch.optim.Optimizer wraps every subclass's step() in profile_hook_step -- a record_function range, two hook walks and
        # a functools wrapper: 40 us per call, 4 % of the render() path's host time.  The class is marked `hooked` below so that the
        # wrapper is not installed; registered step hooks are still honoured, here.)
        pre = self._optimizer_step_pre_hooks
        post = self._optimizer_step_post_hooks
        if pre or post or _TORCH_OPT._global_optimizer_pre_hooks or _TORCH_OPT._global_optimizer_post_hooks:
            return self._step_with_hooks(closure)
        return self._step(closure)

    def _step_with_hooks(self, closure):
        import itertools
        O = _TORCH_OPT
        for hook in itertools.chain(O._global_optimizer_pre_hooks.values(), self._optimizer_step_pre_hooks.values()):
            r = hook(self, (closure,), {})
            if r is not None:
                (closure,), _ = r if isinstance(r, tuple) and len(r) == 2 else ((closure,), {})
        out = self._step(closure)
        for hook in itertools.chain(self._optimizer_step_post_hooks.values(), O._global_optimizer_post_hooks.values()):
            hook(self, (closure,), {})
        return out

    def _step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        hint, self.early_hint = self.early_hint, None
        wait_reg_pending_all()         # the plane gradients this step reads are complete (a regulariser kernel on the second stream)
        joined = None
        if hint is not None and self._early is None:
            # render()'s backward (fused_autograd.py) recorded an event when the appearance parameters' gradients -- SH, scaling,
            # rotation, opacity: four fifths of Adam's bytes -- were final, half-way through the backward.  If nothing has touched
            # them since (same gradient tensors, same versions: any torch in-place op bumps the version; densify / prune replace the
            # parameters and with them the optimizer's entries), their update goes to the second stream behind that event and runs
            # underneath the deformation backward the GPU is still working on, as in the fused step (fused_step.py: early_adam).
            # Element for element the same update as one step().
            slot, side, entries = hint
            mine = {id(p) for group in self.param_groups for p in group["params"]}
            if all(id(p) in mine and p.grad is g and g._version == v for p, g, v in entries):
                ps = [p for p, _, _ in entries]
                if self.ensure_state(ps):
                    # first step (or state made lazily after densify): the moments' zero fill sits on the caller's stream BEHIND the
                    # whole backward, the mark half-way through it -- the second stream waits for the fill itself this once
                    stream_wait_stream(side, N.current_stream())
                stream_wait_mark(side, slot)
                self.step_partial(ps, stream=side)
                joined = side
        early, self._early = self._early, None
        live = [(group, p) for group in self.param_groups for p in group["params"]
                if p.grad is not None and (early is None or id(p) not in early)]
        if live:
            self._launch(live, None if early is None else "late")
        if joined is not None:
            stream_wait_stream(N.current_stream(), joined)      # the step is complete for whatever the caller enqueues next
        if API_OVERLAP and live:
            # what a consumer of the parameters alone (the plane regularisers' forward) may wait for instead of the whole stream
            planes = [p for _, p in live if p.dim() == 4]
            if planes and planes[0].is_cuda:
                cur = N.current_stream()
                stream_mark(MARK_PARAMS, cur)
                _params_ready[planes[0].device] = (cur, frozenset((id(p), p._version) for p in planes))
        return loss


_TORCH_OPT = __import__("sys").modules["torch.optim.optimizer"]     # (torch.optim deletes the submodule's name from its namespace)
FusedAdam.step.hooked = True      # see FusedAdam.step: keeps torch.optim.Optimizer._patch_step_function from wrapping it


# --------------------------------------------------------------------------- backend switch
class _HipBackend:
    """The product path.  Tests of pure host logic on a GPU-less machine may install the oracle's torch
    restatement here EXPLICITLY (oracle.torch_ref.TorchBackend); nothing falls back to it by itself."""
    name = "hip"
    hexplane_features = staticmethod(hexplane_features)
    hexplane_orders = staticmethod(hexplane_orders)
    morton_order = staticmethod(morton_order)
    deform_mlp = staticmethod(deform_mlp)
    l1_loss_with_sums = staticmethod(l1_loss_with_sums)
    ssim = staticmethod(ssim)
    densify_stats = staticmethod(densify_stats)
    select_rows = staticmethod(select_rows)
    densify_round = staticmethod(densify_round)
    plane_regulation = staticmethod(plane_regulation)
    Adam = FusedAdam


BACKEND = _HipBackend


def set_backend(b):
    global BACKEND
    BACKEND = b
