"""gaussian_renderer.render() under autograd as ONE autograd node.

The reference's own training loop (train_4DGS.py:189-297) calls render(), forms the loss in torch, calls loss.backward() and
optimizer.step().  Through the per-op mirror (HexPlane op, MLP op, activations, rasterizer op ...) that is ~40 small torch
launches and as many autograd nodes per iteration and the host becomes the bottleneck (3.8 ms per iteration at 200 k Gaussians
where the kernels need 1.3 ms).  Here the whole fine-stage forward of one camera is one Function whose forward is the launch
sequence of fused_render.py (with the state a backward needs kept) and whose backward is the second half of fused_step.py:
rasterizer backward -> activations -> MLP -> HexPlane, every parameter gradient returned at once.  The loss, the
regularisers, the statistics and Adam stay where the reference has them.

Every call owns its buffers (they come from torch's caching allocator), so several cameras can be rendered before the
backward -- the reference's batch loop -- and images may be kept.  Binning capacity follows the rasterizer module's sync mode
(diff_gaussian_rasterization._C.set_sync_mode): "exact" waits for the frame's instance count like the reference's cudaMemcpy;
"async" sizes from earlier frames and reports an overflow through the module's sticky flag.

Two model shapes run as the node (node_width, NODE_WIDTHS): the shipped field, two HexPlane levels of 32 channels = 64 features, and
two levels of 16 channels = 32 features (dnerf/eulerian_150_16).  The 16 x 2 node is the F == 32 branch of
fused_step.FusedStep.forward_backward cut in two, with that branch's one-launch field written as the two launches whose bits it
gives (16-channel HexPlane forward, MLP forward on 32 features: DESIGN 3.12) for their RAW outputs, torch's own
exp / normalize / sigmoid on them (the image is then the op-by-op path's bit for bit), the shared rasterizer;
backward: rasterizer, the MLP backward on 32 features, the 16-channel HexPlane backward.  feat / dfeat rows are as wide as the
model's feature row, and so the buffer sets of the two shapes never mix (the width is part of the free list's key).
"""
import ctypes as C

import torch

from . import _native as N
from . import ops
from .diff_gaussian_rasterization import _C as RC
from .fused_step import step_features


DIRECT_GRADS = True      # False: always return the parameter gradients through the autograd graph

# The feature widths (fused_step.step_features) gradient-mode render() runs as one node; every other model goes op by op.  32 is here
# by the routing rule of DESIGN 3.6, measured in DESIGN 3.12 (tools/autograd16_rate.py); (64,) keeps 16 x 2 models op by op.
NODE_WIDTHS = (64, 32)


class grads_through_graph:
    """Context manager: render() and the regulariser return their parameter gradients to the autograd engine instead of writing
    p.grad themselves.  Needed around torch.autograd.grad() (which must not touch .grad and expects the gradients back); hooks,
    frozen parameters and backward(inputs=...) are detected and need nothing (ops.direct_grads_ok)."""

    def __enter__(self):
        global DIRECT_GRADS
        self._old = (DIRECT_GRADS, ops.PlaneRegFunction.DIRECT_GRADS)
        DIRECT_GRADS = ops.PlaneRegFunction.DIRECT_GRADS = False

    def __exit__(self, *a):
        global DIRECT_GRADS
        DIRECT_GRADS, ops.PlaneRegFunction.DIRECT_GRADS = self._old


# Internal buffers of a render() call (what no caller ever sees: the field's outputs, the rasterizer's geometry and image state, the
# backward's intermediate gradients and scratch) are handed from one call to the next through a free list per (P, W, H, stream)
# instead of going back to torch's allocator and being asked for again: twenty torch.empty calls and as many frees per iteration,
# 40 us of the host time that paces this path.  (The key also holds the stage and the feature width F: a 32 x 2 and a 16 x 2 model of
# one size in one process must not hand each other sets -- a [P,32] feat given to the 64-feature field kernel is a write past its
# end.)  A call takes a set in its forward and gives it back at the end of its backward; a
# call that is never back-propagated simply keeps its set (the garbage collector frees it), and several cameras rendered before one
# backward each hold a set of their own.  The tensors a caller CAN hold -- image, depth, radii, every gradient -- are never pooled.
_POOL = {}
_POOL_MAX = 4


def _pool_take(key):
    free = _POOL.get(key)
    return free.pop() if free else None


def _pool_give(key, bufs):
    free = _POOL.setdefault(key, [])
    if len(free) < _POOL_MAX:
        free.append(bufs)
    if len(_POOL) > 8:                    # the model changed size a few times (densify / prune): forget the old sizes
        for k in list(_POOL)[:-4]:
            del _POOL[k]


class _State:
    __slots__ = ("pool_key", "bufs", "a", "keep", "P", "W", "H", "F", "cam_time", "order", "porders", "feat", "a0", "pts", "sc_d", "rot_d", "sc", "rot", "op",
                 "color", "depth", "radii", "geom", "img", "binning", "cap", "xyz", "scal", "rotq", "opac", "flow", "coef", "planes",
                 "mlp", "field", "f_dc", "f_rest", "ready", "side")


def _field_cache(dn):
    """(first plane, first MLP tensor, planes, MLP tensors, step_features) of a deformation net, cached on it until a parameter
    object is replaced (walking the nn.Module tree costs 70 us per call, and _field16_fusable() behind step_features walks every
    plane: neither is paid per frame on a path the host paces)."""
    c = getattr(dn, "_fa_params", None)
    if c is None or c[0] is not dn.grid.grids[0][0] or c[1] is not dn.feature_out[0].weight:
        planes, mlp = [p for lv in dn.grid.grids for p in lv], dn._fused_params()
        c = dn._fa_params = (planes[0], mlp[0], planes, mlp, step_features(dn))
    return c


def field_params(pc):
    """(planes, MLP tensors) of the deformation field (_field_cache)."""
    c = _field_cache(pc._deformation.deformation_net)
    return c[2], c[3]


def node_width(dn):
    """Width of the HexPlane feature row at which gradient-mode render() runs deformation net dn as ONE node, or 0 if it goes op by
    op: fused_step.step_features(dn) -- 64 for the shipped field (Deformation._fusable), 32 for two levels of 16 channels
    (Deformation._field16_fusable) where 32 is in NODE_WIDTHS.  The module's answer is cached with its parameter lists; NODE_WIDTHS
    is read at every call."""
    F = _field_cache(dn)[4]
    return F if F == 64 or F in NODE_WIDTHS else 0


def _forward_desc(pc, field, planes, mlp):
    """HexPlane / MLP descriptors of the forward (pointers and shapes only): rebuilt when a parameter or the aabb moves."""
    key = (tuple(p.data_ptr() for p in planes), tuple(p.data_ptr() for p in mlp), tuple(field.aabb_host()))
    c = getattr(pc, "_fa_desc", None)
    if c is None or c[0] != key:
        hp, keep = ops._hexplane_desc([[p.detach() for p in lv] for lv in field.grids], field.aabb, None, aabb_host=field.aabb_host())
        md = ops.DeformMLPFunction._desc([p.detach() for p in mlp], None)
        c = pc._fa_desc = (key, hp, keep, md)
    return c[1], c[2], c[3]


def _forward(pc, cam, bg, delta_scale, scaling_modifier, debug, coarse):
    """coarse: no deformation field -- the projection reads the raw parameters and applies the activations itself."""
    lib, s = N.lib(), N.current_stream()
    st = _State()
    dev = pc._xyz.device
    P = st.P = pc._xyz.shape[0]
    W, H = st.W, st.H = int(cam.image_width), int(cam.image_height)
    view, proj, campos, _ = cam.device_tensors(dev)
    st.xyz, st.f_dc, st.f_rest, st.scal, st.rotq, st.opac = ops.gaussian_params(pc, "fused render()")
    st.planes, st.mlp, st.field, st.ready, st.side = (), (), None, None, None
    e = lambda *sh: torch.empty(*sh, dtype=torch.float32, device=dev)
    F = 0
    if not coarse:
        fc = _field_cache(pc._deformation.deformation_net)
        F = fc[4]
        if F not in (64, 32):
            raise N.MomError("fused render(): the deformation field is neither the shipped one (two HexPlane levels of 32 channels) nor two "
                             "levels of 16 channels inside the field kernel's limits (fused_autograd.node_width)")
    st.F = F
    st.pool_key = (P, W, H, dev, s, coarse, F)
    b = st.bufs = _pool_take(st.pool_key)
    if b is None:
        b = st.bufs = {"geom": torch.empty(lib.mom_raster_geom_bytes(P), dtype=torch.uint8, device=dev),
                       "img": torch.empty(lib.mom_raster_image_bytes(W, H), dtype=torch.uint8, device=dev),
                       "nr_dev": torch.empty(1, dtype=torch.int32, device=dev)}
        if not coarse:
            # (feat rows are F floats; a0 = relu(h0) is the network's width whatever feeds it)
            b.update(feat=e(P, F), a0=e(P, 64), pts=e(P, 3), sc_d=e(P, 3), rot_d=e(P, 4), sc=e(P, 3), rot=e(P, 4), op=e(P, 1))
    st.color, st.depth = e(3, H, W), e(1, H, W)
    st.radii = torch.empty(P, dtype=torch.int32, device=dev)
    st.geom, st.img = b["geom"], b["img"]
    st.keep = (bg, view, proj, campos)      # (with st's own tensors: what the pointers in st.a point at)
    if coarse:
        means, sc, rot, op = st.xyz, st.scal, st.rotq, st.opac
    else:
        field = st.field = pc._deformation.deformation_net.grid
        st.planes, st.mlp = fc[2], fc[3]
        flow = st.flow = pc._scene_flow if pc._scene_flow.is_contiguous() else pc._scene_flow.contiguous()
        st.cam_time = float(cam.time)
        st.coef = float(delta_scale * cam.frame_num)
        st.order = field._processing_order(st.xyz)
        st.porders = field._plane_orders(st.xyz)
        st.feat, st.a0 = b["feat"], b["a0"]
        st.pts, st.sc_d, st.rot_d = b["pts"], b["sc_d"], b["rot_d"]
        st.sc, st.rot, st.op = b["sc"], b["rot"], b["op"]
        means, sc, rot, op = st.pts, st.sc, st.rot, st.op
        hp, keep, md = _forward_desc(pc, field, st.planes, st.mlp)
        st.keep += (keep,)
        if F == 32:
            # two levels of 16 channels: the 16-channel HexPlane forward and the MLP forward on 32 features, raw outputs only; the
            # activated copies are torch's exp / normalize / sigmoid, as in FusedStep16 and FusedRender and for the same reason --
            # the kernels' expf / quaternion norm differ from torch's in last bits, and the image would no longer be the op-by-op
            # path's.  The two launches and not the one-launch field of csrc/deform_field16.hip, whose bits and
            # time they are (96 against 97 us at 200 k points): that kernel reports under the hexplane_fwd profile slot
            # alone, and gradient-mode render() of such a model is held to launching the MLP forward under its own slot
            # (tests/test_mlp32_gpu.py); DESIGN 3.12
            N.check(lib.mom_hexplane_forward(C.byref(hp), P, st.xyz.data_ptr(), None, st.cam_time,
                                             None if st.order is None else st.order.data_ptr(), st.feat.data_ptr(), s), "hexplane_fwd")
            N.check(lib.mom_deform_forward_n(C.byref(md), P, 32, st.feat.data_ptr(), st.xyz.data_ptr(), st.scal.data_ptr(),
                                             st.rotq.data_ptr(), flow.data_ptr(), st.coef, st.pts.data_ptr(), st.sc_d.data_ptr(),
                                             st.rot_d.data_ptr(), st.a0.data_ptr(), s), "deform_fwd")
            torch.exp(st.sc_d, out=st.sc)
            torch.nn.functional.normalize(st.rot_d, out=st.rot)
            torch.sigmoid(st.opac, out=st.op)
        else:
            ops.field_forward(hp, md, P, st.xyz, st.cam_time, st.order, st.scal, st.rotq, flow, st.coef, st.pts, st.sc_d, st.rot_d,
                              st.feat, st.a0, st.opac, st.sc, st.rot, st.op, s)
    st.a = ops.raster_args(cam, view, proj, campos, bg, P, pc.active_sh_degree, means, st.f_dc, st.f_rest, op, sc, rot, coarse,
                           scaling_modifier, debug, False)
    # projection, binning and compositing under the rasterizer module's settings (set_sync_mode: the binning capacity;
    # set_keep_all_tiles: the reference's lists, written into st.a for the backward too): the drop-in's own driver
    st.cap, st.binning = RC.raster_forward(lib, st.a, st.geom, st.img, st.radii, st.color, st.depth, b["nr_dev"], P, W, H, dev, s)
    return st


def _field_grads(st, f, direct=True):
    """Gradient storage of the deformation field -- the planes in their channel-last storage order, then the MLP tensors, one
    flat zeroed buffer -- with the backward descriptors that point into it.  One set is cached on the field and reused from
    iteration to iteration (the reference's loop drops the gradients with zero_grad(set_to_none=True), so the parameters let go
    of it); while the parameters still hold it -- a second camera of a batch -- a temporary set is made.

    Planes that already HAVE a gradient of the right layout (the regulariser's backward ran first) are accumulated into in
    place: the kernels add with atomics anyway, and twelve elementwise additions and their launches are saved.
    Returns (plane targets, MLP targets, hp, md, in_place) -- in_place[i]: plane i's target is its own .grad."""
    field = st.field
    # through-the-graph mode (direct False): never touch a .grad, never hand out the cached buffer
    held = [p.grad if direct else None for p in st.planes]
    in_place = ops.in_place_flags(held, st.planes)
    key = (tuple(p.data_ptr() for p in st.planes), tuple(p.data_ptr() for p in st.mlp), tuple(field.aabb_host()),
           tuple(g.data_ptr() if ip else 0 for g, ip in zip(held, in_place)))
    c = getattr(field, "_fa_grads", None)
    own_busy = c is not None and (not direct or (st.mlp[0].grad is not None and st.mlp[0].grad.data_ptr() == c[3][0].data_ptr())
                                  or any(g is not None and g.data_ptr() == v.data_ptr() for g, v in zip(held, c[2]))
                                  or not ops._buffers_free(c[3]) or not ops._buffers_free(c[2], 2))   # a caller kept last iteration's gradient tensors (planes: also in `targets`)
    if c is not None and c[0] == key and not own_busy:
        c[1].zero_()
        return [held[i] if in_place[i] else c[2][i] for i in range(len(c[2]))], c[3], c[5], c[7], in_place
    n = sum(p.numel() for p in st.planes + st.mlp)
    flat = torch.zeros(n, **f)
    off, gplanes, gmlp = 0, [], []
    for p in st.planes:
        shape = ops.plane_storage(p).shape
        gplanes.append(flat[off:off + p.numel()].view(shape).permute(2, 0, 1).unsqueeze(0))
        off += p.numel()
    for p in st.mlp:
        gmlp.append(flat[off:off + p.numel()].view(p.shape))
        off += p.numel()
    targets = [held[i] if in_place[i] else gplanes[i] for i in range(len(gplanes))]
    levels, k = [], 0
    for lv in field.grids:
        levels.append(targets[k:k + len(lv)])
        k += len(lv)
    hp, keep = ops._hexplane_desc([[p.detach() for p in lv] for lv in field.grids], field.aabb, levels, aabb_host=field.aabb_host())
    md = ops.DeformMLPFunction._desc([p.detach() for p in st.mlp], gmlp)
    if not own_busy:
        # (no reference to `held`: those are the regulariser's cached gradient views, and a reference kept here made ITS cache
        # look busy in the next iteration -- it then made new buffers, this key changed, and both caches missed every iteration:
        # 1 ms of host time per step, found with tools/host_profile.py --autograd)
        field._fa_grads = (key, flat, gplanes, gmlp, None, hp, keep, md)
    return targets, gmlp, hp, md, in_place


def _backward(st, dcolor, ddepth, direct=True):
    """(screen-space gradient, the parameter gradients in the order of st's parameters: the six Gaussian ones, planes, MLP)."""
    lib, s = N.lib(), N.current_stream()
    P, dev = st.P, st.color.device
    f = dict(dtype=torch.float32, device=dev)
    e = lambda *sh: torch.empty(*sh, **f)
    dcol = dcolor.contiguous().float()
    ddep = None if ddepth is None else ddepth.contiguous().float()
    b = st.bufs
    if "gcol" not in b:               # the backward's internal gradients: made once per pooled set
        b.update(gcol=e(P, 3), gcov=e(P, 6))
    g2d, gxyz, gdc, grest, gsc, grot, gop = e(P, 3), e(P, 3), e(P, 1, 3), e(P, 15, 3), e(P, 3), e(P, 4), e(P, 1)
    gr = ops.raster_grads(g2d, b["gcol"], gop, gxyz, b["gcov"], gdc, grest, gsc, grot)
    if st.field is not None:
        # (scale / rotation / opacity gradients: through their activations inside the projection backward -- act_rotations_raw)
        gr.act_rotations_raw = st.rot_d.data_ptr()
    if RC.deterministic():            # the ordered reduction (RC.set_deterministic): one synchronisation, the same bits every run
        RC.ordered_backward(lib, st.a, st.radii, st.geom, st.binning, st.cap, st.img, dcol, ddep, gr, P, dev, s)
    else:
        N.check(lib.mom_raster_backward(C.byref(st.a), st.radii.data_ptr(), st.geom.data_ptr(), st.binning.data_ptr(), st.cap,
                                        st.img.data_ptr(), dcol.data_ptr(), None if ddep is None else ddep.data_ptr(), C.byref(gr), s),
                "raster_bwd")
    if st.field is None:              # coarse stage: the raw parameters' gradients are complete
        _pool_give(st.pool_key, b)
        st.bufs = None
        return g2d, (gxyz, gdc, grest, gsc, grot, gop)
    if "dfeat" not in b:              # the deformation backward's intermediate gradient and scratch
        b.update(dfeat=e(P, st.F), scratch=torch.empty(lib.mom_deform_backward_scratch_bytes(P), dtype=torch.uint8, device=dev))
    det = RC.deterministic()
    overlap = ops.API_OVERLAP and direct and not det          # (the ordered field backward is one stream)
    ready = side = None
    if overlap:
        # the appearance parameters' gradients (SH, scaling, rotation, opacity) are final here: FusedAdam.step() may start their
        # update on the second stream behind this event while the deformation backward below still runs (ops.FusedAdam.step)
        side = ops.side_stream(dev).cuda_stream
        ready = ops.next_ring_mark(s)
    gplanes, gmlp, hp, md, in_place = _field_grads(st, f, direct)
    dfeat, scratch = b["dfeat"], b["scratch"]
    # pts = xyz + dx(...): d xyz starts as d pts (already in gxyz); scale / rotation residuals likewise
    if det:
        ops.deform_backward_ordered(lib, md, P, st.F, st.feat, st.a0, gxyz, gsc, grot, dfeat, s)
    elif overlap:
        # with a second stream the MLP backward leaves an eighth of the chip free (for that Adam launch) and its partial-sum
        # reduction goes there too (csrc/deform_bwd_b3.hip; on 32 features: the weight-gradient kernel of csrc/deform_mlp.hip);
        # joined below
        N.check(lib.mom_deform_backward_split_n(C.byref(md), P, st.F, st.feat.data_ptr(), st.a0.data_ptr(), gxyz.data_ptr(),
                                                gsc.data_ptr(), grot.data_ptr(), dfeat.data_ptr(), scratch.data_ptr(), s, side),
                "deform_bwd")
    else:
        N.check(lib.mom_deform_backward_n(C.byref(md), P, st.F, st.feat.data_ptr(), st.a0.data_ptr(), gxyz.data_ptr(), gsc.data_ptr(),
                                          grot.data_ptr(), dfeat.data_ptr(), scratch.data_ptr(), s), "deform_bwd")
    ops.wait_reg_pending(dev)          # the regulariser's gradient kernel (second stream) adds into the plane gradients too
    porders = None if det else st.porders
    hscratch = None
    if porders is not None:
        need = lib.mom_hexplane_backward_scratch_bytes(C.byref(hp), P)
        hscratch = b.get("hscratch")
        if hscratch is None or hscratch.numel() < need:
            hscratch = b["hscratch"] = torch.empty(need, dtype=torch.uint8, device=dev)
    if det:
        ops.hexplane_backward_ordered(lib, hp, P, st.xyz, st.cam_time, st.order, dfeat, gxyz, s)
    else:
        N.check(lib.mom_hexplane_backward(C.byref(hp), P, st.xyz.data_ptr(), None, st.cam_time,
                                          None if st.order is None else st.order.data_ptr(), dfeat.data_ptr(), gxyz.data_ptr(),
                                          None if porders is None else porders[0].data_ptr(),
                                          None if porders is None else porders[1].data_ptr(),
                                          None if hscratch is None else hscratch.data_ptr(), s), "hexplane_bwd")
    if overlap:
        ops.stream_wait_stream(s, side)                    # the MLP weight gradients are complete for whoever reads them next
    st.ready, st.side = ready, side
    # the set goes back to the free list: everything that reads it is enqueued on this stream, and so is whoever takes it next
    # (the key holds the stream).  With the second-stream overlap a kernel on the OTHER stream may still read it: that call keeps it.
    if not overlap:
        _pool_give(st.pool_key, b)
    st.bufs = None
    return g2d, (gxyz, gdc, grest, gsc, grot, gop, *gplanes, *gmlp)


def _take(ctx):
    st = ctx.st
    if st is None:
        raise RuntimeError("render(): a second backward through the same call -- its buffers were released after the first "
                           "(render again, or set pipe.per_op_autograd = True for retain_graph use)")
    ctx.st = None                                  # the call's buffers go back to the allocator after this backward
    return st


def _node_backward(ctx, st, lead, dcolor, ddepth):
    """Function.backward of one render() node with `lead` plain inputs in front of the 2-D gradient holder."""
    pc = ctx.pc
    params = (pc._xyz, pc._features_dc, pc._features_rest, pc._scaling, pc._rotation, pc._opacity, *st.planes, *st.mlp)
    needs = ctx.needs_input_grad[lead + 1:]
    direct = DIRECT_GRADS and ops.direct_grads_ok(params, needs)
    g2d, grads = _backward(st, dcolor, ddepth, direct)
    if not direct:
        # through the graph (fresh buffers: nothing is accumulated in place on this path); inputs that were not asked for get None
        return (None,) * lead + (g2d, *[g if n else None for g, n in zip(grads, needs)])
    # The parameter gradients are handed to the parameters here (set, or added to what an earlier camera of the batch left)
    # instead of being returned: 32 AccumulateGrad nodes cost the autograd engine more host time than the whole fine forward.
    # Only the 2-D gradient holder, a non-leaf, goes back through the graph.
    fresh = True
    for p, g in zip(params, grads):
        if p.grad is None:
            p.grad = g
        elif p.grad is not g:                   # (a plane accumulated into in place IS its own gradient)
            p.grad.add_(g)
            fresh = False
    # one camera per optimizer step (the reference's batch_size 1): tell the optimizer when the appearance gradients were final,
    # so that its step() can start their update underneath the rest of this backward (ops.FusedAdam.step checks that nothing
    # touched them in between).  A second camera accumulating into them, or a backward without that overlap (the coarse stage
    # has no deformation backward to hide it under), withdraws the hint.
    opt = getattr(pc, "optimizer", None)
    if opt is not None and hasattr(opt, "early_hint"):
        app = params[1:6]
        if st.ready is not None and fresh and all(p.grad is g for p, g in zip(app, grads[1:6])):
            opt.early_hint = (st.ready, st.side, [(p, p.grad, p.grad._version) for p in app])
        else:
            opt.early_hint = None
    return (None,) * lead + (g2d,) + (None,) * len(params)


class FusedRenderFunction(torch.autograd.Function):
    """(image, depth, radii) = render of one camera; inputs after the six plain arguments: the 2-D gradient holder, the six
    Gaussian parameter tensors, the 12 HexPlane planes, the 14 MLP tensors."""

    @staticmethod
    def forward(ctx, pc, cam, bg, delta_scale, scaling_modifier, debug, screenspace, xyz, f_dc, f_rest, scaling, rotation, opacity,
                *field):
        st = _forward(pc, cam, bg, delta_scale, scaling_modifier, debug, False)
        ctx.st, ctx.pc = st, pc
        dev = st.color.device
        ops._render_pending[dev] = ops._render_pending.get(dev, 0) + 1       # (ops.PlaneRegFunction.backward: who joins its kernel)
        ctx.mark_non_differentiable(st.radii)
        return st.color, st.depth, st.radii

    @staticmethod
    def backward(ctx, dcolor, ddepth, _dradii):
        st = _take(ctx)
        dev = st.color.device
        ops._render_pending[dev] = max(0, ops._render_pending.get(dev, 0) - 1)
        return _node_backward(ctx, st, 6, dcolor, ddepth)


# The coarse stage (train_4DGS.py with stage "coarse": the first 3 000 iterations of every run) renders the Gaussians without the
# deformation field, so its render() is the rasterizer alone on exp / normalize / sigmoid of the parameters
# (gaussian_renderer/__init__.py:113,130-132).  As one node: the projection reads the RAW parameters and applies the activations in
# registers (MomRasterArgs.params_raw), the backward writes the six parameter gradients through them -- no activated copies, no
# activation nodes, no separate rasterizer node.
class FusedCoarseRenderFunction(torch.autograd.Function):
    """(image, depth, radii) = coarse-stage render of one camera; inputs after the five plain arguments: the 2-D gradient holder
    and the six Gaussian parameter tensors."""

    @staticmethod
    def forward(ctx, pc, cam, bg, scaling_modifier, debug, screenspace, xyz, f_dc, f_rest, scaling, rotation, opacity):
        st = _forward(pc, cam, bg, None, scaling_modifier, debug, True)
        ctx.st, ctx.pc = st, pc
        ctx.mark_non_differentiable(st.radii)
        return st.color, st.depth, st.radii

    @staticmethod
    def backward(ctx, dcolor, ddepth, _dradii):
        return _node_backward(ctx, _take(ctx), 5, dcolor, ddepth)


def render_coarse(cam, pc, pipe, bg, scaling_modifier, screenspace_points):
    return FusedCoarseRenderFunction.apply(pc, cam, bg, scaling_modifier, pipe.debug, screenspace_points, pc._xyz,
                                           pc._features_dc, pc._features_rest, pc._scaling, pc._rotation, pc._opacity)


def render(cam, pc, pipe, bg, delta_scale, scaling_modifier, screenspace_points):
    planes, mlp = field_params(pc)
    return FusedRenderFunction.apply(pc, cam, bg, delta_scale, scaling_modifier, pipe.debug,
                                     screenspace_points, pc._xyz, pc._features_dc, pc._features_rest, pc._scaling, pc._rotation,
                                     pc._opacity, *planes, *mlp)
