"""Gradient-mode gaussian_renderer.render() of a 16 x 2 HexPlane model (dnerf/eulerian_150_16: two levels of 16-channel planes, 32
features into the shipped network) as ONE autograd node (fused_autograd.FusedRenderFunction at F == 32) against the real
operator-by-operator path of the same model (pipe.per_op_autograd = True).

The node's forward is the 16-channel HexPlane forward and the MLP forward on 32 features for their raw outputs with torch's exp /
normalize / sigmoid on them, the launches of the two ops the per-op path runs, so images, depths and radii are compared with torch.equal; its backward is the
rasterizer backward, the MLP backward on 32 features and the 16-channel HexPlane backward, the per-op path's kernels in another
order of float atomics, so every gradient is held to 5e-5 of the per-op tensor's largest magnitude -- the bound
tests/test_fused_step16_gpu.py holds this pair of kernel sequences to (it measured 4.4e-6).

Every test sets fused_autograd.NODE_WIDTHS itself: the tests hold whichever default ships.  Shapes: the tiny scene of
tests/test_whole_step_gpu.py (P = 6000, 160 x 96, 4 frames)."""
import functools
import importlib
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import test_fused_step16_gpu as S16                     # _model / _cams / _tensors and the trainer helpers of the 16 x 2 model
from test_fused_autograd_gpu import _params             # name -> parameter: the six Gaussian ones, 12 planes, 14 MLP tensors

pkg = "iclr2025_3d-mom_amd"
FA = importlib.import_module(pkg + ".fused_autograd")
CFG = S16.CFG
TOL = 5e-5
BOTH, OFF = (64, 32), (64,)
NODE = "FusedRenderFunctionBackward"
CAM = 1                                  # the camera of tests/test_fused_step16_gpu.py's first step: it sees the box model's min-face Gaussian


def _setup(per_op=False, **kw):
    T = importlib.import_module(pkg + ".train")
    scene, g, op, pp, hp = S16._model(**kw)
    trainer = T.Trainer(scene, g, op, hp, pp, stage="fine", delta_scale=1, sync_every_step=False, fused=False)
    trainer.pipe.per_op_autograd = per_op
    return scene, g, trainer


def _render(scene, g, trainer, cam):
    render = importlib.import_module(pkg + ".gaussian_renderer").render
    return render(cam, g, trainer.pipe, trainer.background, stage="fine", cam_type=scene.dataset_type, delta_scale=trainer.delta_scale)


def _weights():
    gen = torch.Generator("cpu").manual_seed(5)
    return torch.rand(3, CFG["H"], CFG["W"], generator=gen).cuda()


def _loss(pkgs, wgt):
    return sum(((pk["render"] * wgt).sum() + 0.3 * pk["depth"].sum()) for pk in pkgs)


def _nodes(t):
    """Names of every autograd node behind tensor t."""
    seen, todo, names = set(), [t.grad_fn], []
    while todo:
        fn = todo.pop()
        if fn is None or fn in seen:
            continue
        seen.add(fn)
        names.append(type(fn).__name__)
        todo += [nf for nf, _ in fn.next_functions]
    return names


def _run(per_op, cam_ids, P=CFG["P"], box=False):
    """One loss over the cameras cam_ids, back-propagated: (images, depths, radii, gradients by name, screen-space gradients).
    Computed once per argument list and shared: callers do not write into what it returns."""
    return _run_once(bool(per_op), tuple(cam_ids), int(P), bool(box))


@functools.lru_cache(maxsize=None)
def _run_once(per_op, cam_ids, P, box):
    assert FA.NODE_WIDTHS == BOTH
    scene, g, trainer = _setup(per_op, P=P, box=box)
    cams = S16._cams(trainer, box)
    ps = _params(g)
    assert len(ps) == 32
    pkgs = [_render(scene, g, trainer, cams[c % len(cams)]) for c in cam_ids]
    for pk in pkgs:
        assert (type(pk["render"].grad_fn).__name__ == NODE) == (not per_op)
        assert (NODE in _nodes(pk["render"])) == (not per_op)
    images = [pk["render"].detach().clone() for pk in pkgs]
    depths = [pk["depth"].detach().clone() for pk in pkgs]
    _loss(pkgs, _weights()).backward()
    torch.cuda.synchronize()
    grads = {k: p.grad.detach().clone() for k, p in ps.items()}
    vsp = [pk["viewspace_points"].grad.detach().clone() for pk in pkgs]
    radii = [pk["radii"].clone() for pk in pkgs]
    return images, depths, radii, grads, vsp


def _rel(a, b):
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-30)


def _layout(t):
    return tuple(t.shape), [s for s, n in zip(t.stride(), t.shape) if n > 1]


# ---------------------------------------------------------------------------------------------------------------- 1
def test_routing(monkeypatch):
    """Gradient mode, 16 x 2: the image's grad_fn is the node; not with per_op_autograd, not without 32 in NODE_WIDTHS.  (Before the
    node took 32 features the first assertion failed: the image came out of the rasterizer op's node.)"""
    monkeypatch.setattr(FA, "NODE_WIDTHS", BOTH)
    scene, g, trainer = _setup()
    dn = g._deformation.deformation_net
    assert dn._field16_fusable() and not dn._fusable() and FA.node_width(dn) == 32
    cam = trainer.cams[2]
    pk = _render(scene, g, trainer, cam)
    assert type(pk["render"].grad_fn).__name__ == NODE and pk["render"].grad_fn is pk["depth"].grad_fn
    assert isinstance(pk["render"].grad_fn, FA.FusedRenderFunction._backward_cls)
    assert pk["render"].grad_fn.st.F == 32
    assert not pk["radii"].requires_grad and pk["radii"].grad_fn is None and pk["radii"].dtype == torch.int32
    assert pk["viewspace_points"].requires_grad
    assert getattr(g, "_fused_render", None) is None              # no forward-only renderer was made in gradient mode
    with torch.no_grad():
        ng = _render(scene, g, trainer, cam)
    assert getattr(g, "_fused_render", None) is not None and ng["render"].grad_fn is None
    torch.cuda.synchronize()
    assert torch.equal(ng["render"], pk["render"]) and torch.equal(ng["depth"], pk["depth"]) and torch.equal(ng["radii"], pk["radii"])
    assert float(pk["render"].detach().abs().max()) > 0 and int((pk["radii"] > 0).sum()) > 0

    trainer.pipe.per_op_autograd = True
    po = _render(scene, g, trainer, cam)
    assert NODE not in _nodes(po["render"]) and po["render"].grad_fn is not None
    trainer.pipe.per_op_autograd = False
    monkeypatch.setattr(FA, "NODE_WIDTHS", OFF)
    assert FA.node_width(dn) == 0
    off = _render(scene, g, trainer, cam)
    assert NODE not in _nodes(off["render"]) and off["render"].grad_fn is not None
    torch.cuda.synchronize()
    assert torch.equal(po["render"], pk["render"]) and torch.equal(off["render"], pk["render"])
    pk["render"].sum().backward()                                 # the call gives its buffer set back
    torch.cuda.synchronize()
    assert pk["render"].grad_fn.st is None and torch.isfinite(g._xyz.grad).all()


# ---------------------------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("P,box", [(6000, False), (6001, False), (97, True)])
def test_node_against_op_by_op(monkeypatch, P, box):
    """Image, depth and radii equal to the bit; all 32 parameter gradients and the screen-space gradient within 5e-5 of the per-op
    tensor's largest magnitude, in the per-op path's layout.  6001 and 97 are no multiple of the field kernel's 32-Gaussian tile or
    of the backward's four-unit group, 97 leaves a last tile of one and sits in the asymmetric box of tests/hexplane_box_cases.py
    with one Gaussian exactly on the z min face.  (On the parent the `not per_op` run is op by op too and _run's assertion on the
    node fails.)

    Measured on an MI355X (the printed maxima, the larger of two runs): 3.9e-6 (scaling) at P = 6000, 1.2e-6 (an MLP head weight) at 6001,
    2.4e-6 (rotation) at 97."""
    monkeypatch.setattr(FA, "NODE_WIDTHS", BOTH)
    im0, d0, r0, g0, v0 = _run(True, (CAM,), P, box)
    im1, d1, r1, g1, v1 = _run(False, (CAM,), P, box)
    assert g0["xyz"].shape[0] == P and g0["mlp_0"].shape == (64, 32) and g0["plane_0_0"].shape[1] == 16
    worst = {k: _rel(g1[k], g0[k]) for k in g0}
    worst["viewspace_points"] = _rel(v1[0], v0[0])
    print("P", P, "box", box, "gradient errors relative to the per-op tensor's max:", {k: "%.2e" % v for k, v in worst.items()})
    print("P", P, "largest: %.2e (%s)" % max((v, k) for k, v in worst.items()))
    assert torch.equal(im1[0], im0[0]) and torch.equal(d1[0], d0[0]) and torch.equal(r1[0], r0[0])
    assert float(im0[0].abs().max()) > 0 and float(d0[0].abs().max()) > 0 and int((r0[0] > 0).sum()) > 0
    if box:
        assert int(r0[0][P // 2]) > 0                              # the Gaussian on the min face is on screen
    for k in g0:
        assert _layout(g1[k]) == _layout(g0[k]), k
        assert torch.isfinite(g1[k]).all() and float(g0[k].abs().max()) > 0, k
        assert worst[k] <= TOL, (k, worst[k])
    assert _layout(v1[0]) == _layout(v0[0]) and worst["viewspace_points"] <= TOL, worst["viewspace_points"]


# ---------------------------------------------------------------------------------------------------------------- 3
def test_two_cameras_before_one_backward(monkeypatch):
    """tests/test_fused_autograd_gpu.py::test_a_batch_of_cameras_before_one_backward_accumulates on the 16 x 2 node, its tolerance
    unchanged: both images survive the second render, each gradient is the sum of the single-camera gradients within 5e-5."""
    monkeypatch.setattr(FA, "NODE_WIDTHS", BOTH)
    scene, g, trainer = _setup()
    assert float(trainer.cams[1].time) != float(trainer.cams[3].time)
    im_a, d_a, _, g_a, v_a = _run(False, (1,))
    im_b, d_b, _, g_b, v_b = _run(False, (3,))
    im_ab, d_ab, _, g_ab, v_ab = _run(False, (1, 3))
    assert torch.equal(im_ab[0], im_a[0]) and torch.equal(im_ab[1], im_b[0]) and not torch.equal(im_a[0], im_b[0])
    assert torch.equal(d_ab[0], d_a[0]) and torch.equal(d_ab[1], d_b[0])
    assert _rel(v_ab[0], v_a[0]) <= TOL and _rel(v_ab[1], v_b[0]) <= TOL
    worst = {k: _rel(g_ab[k], g_a[k] + g_b[k]) for k in g_ab}
    print("two cameras, error of the accumulated gradient relative to the sum's max: largest %.2e (%s)" % max((v, k) for k, v in worst.items()))
    for k, e in worst.items():
        assert e <= TOL, (k, e)


# ---------------------------------------------------------------------------------------------------------------- 4
def test_gradients_through_the_graph(monkeypatch):
    """Under grads_through_graph() torch.autograd.grad() gets all 32 gradients back and no .grad is touched."""
    monkeypatch.setattr(FA, "NODE_WIDTHS", BOTH)
    _, _, _, ref, _ = _run(False, (CAM,))
    scene, g, trainer = _setup()
    ps = _params(g)
    pk = _render(scene, g, trainer, trainer.cams[CAM])
    assert type(pk["render"].grad_fn).__name__ == NODE
    with FA.grads_through_graph():
        got = torch.autograd.grad(_loss([pk], _weights()), list(ps.values()))
    torch.cuda.synchronize()
    assert len(got) == 32 and all(p.grad is None for p in ps.values())
    worst = {k: _rel(a, ref[k]) for k, a in zip(ps, got)}
    print("through the graph, error relative to the direct gradient's max: largest %.2e (%s)" % max((v, k) for k, v in worst.items()))
    for k, a in zip(ps, got):
        assert a.shape == ref[k].shape and worst[k] <= TOL, (k, worst[k])


# ---------------------------------------------------------------------------------------------------------------- 5
def test_a_second_backward_raises(monkeypatch):
    monkeypatch.setattr(FA, "NODE_WIDTHS", BOTH)
    scene, g, trainer = _setup()
    pk = _render(scene, g, trainer, trainer.cams[2])
    loss = pk["render"].sum()
    loss.backward(retain_graph=True)
    with pytest.raises(RuntimeError, match="a second backward through the same call"):
        loss.backward()
    torch.cuda.synchronize()
    assert torch.isfinite(g._xyz.grad).all()


# ---------------------------------------------------------------------------------------------------------------- 6
def test_two_widths_in_one_process_keep_their_buffer_sets_apart(monkeypatch):
    """A 32 x 2 and a 16 x 2 model of the same P, W and H, rendered and back-propagated alternately on one stream: the free list's
    key carries the feature width, so a 16 x 2 call holds [P,32] feat / dfeat and a 32 x 2 call [P,64] -- checked by buffer shape;
    a [P,32] feat handed to the 64-feature field kernel would be a write past its end."""
    monkeypatch.setattr(FA, "NODE_WIDTHS", BOTH)
    monkeypatch.setattr(FA, "_POOL", {})
    monkeypatch.setattr(importlib.import_module(pkg + ".ops"), "API_OVERLAP", False)      # (with it a call keeps its set)
    wgt = _weights()
    P = CFG["P"]
    models = {64: _setup(channels=32), 32: _setup(channels=16)}
    first, sets = {}, {}
    for rnd in range(2):
        for F in (64, 32):
            scene, g, trainer = models[F]
            ps = _params(g)
            for p in ps.values():
                p.grad = None
            pk = _render(scene, g, trainer, trainer.cams[2])
            st = pk["render"].grad_fn.st
            b = st.bufs
            assert st.F == F and st.pool_key[-1] == F and tuple(b["feat"].shape) == (P, F) and tuple(b["a0"].shape) == (P, 64)
            assert st.feat is b["feat"]
            if rnd == 1:
                assert b is sets[F]                                # the set this model's first call gave back, not the other model's
                assert tuple(b["dfeat"].shape) == (P, F)
            image = pk["render"].detach().clone()
            _loss([pk], wgt).backward()
            assert tuple(b["dfeat"].shape) == (P, F)               # made by the first backward of the set
            assert len(FA._POOL[st.pool_key]) == 1 and FA._POOL[st.pool_key][0] is b and pk["render"].grad_fn.st is None
            sets[F] = b
            torch.cuda.synchronize()
            grads = {k: p.grad.detach().clone() for k, p in ps.items()}
            if rnd == 0:
                first[F] = (image, grads)
                continue
            assert torch.equal(image, first[F][0]), F
            for k in grads:
                assert _rel(grads[k], first[F][1][k]) <= TOL, (F, k)
    assert sets[64] is not sets[32] and len(FA._POOL) == 2
    for key, free in FA._POOL.items():
        for b in free:
            assert b["feat"].shape[1] == b["dfeat"].shape[1] == key[-1]


# ---------------------------------------------------------------------------------------------------------------- 7
@functools.lru_cache(maxsize=None)
def _train(per_op, steps, lambda_dssim):
    """tests/test_fused_step16_gpu.py::_run_once on Trainer(fused=False), the node or the op-by-op path."""
    assert FA.NODE_WIDTHS == BOTH
    scene, g, trainer = S16._trainer(False, lambda_dssim=lambda_dssim)
    trainer.pipe.per_op_autograd = per_op
    calls, node_render = [0], FA.render

    def counted(*a, **k):
        calls[0] += 1
        return node_render(*a, **k)
    FA.render = counted
    try:
        losses = [float(trainer.step(5001 + it, cams=S16._cam_lists(trainer, it, 1, False))) for it in range(steps)]
    finally:
        FA.render = node_render
    assert calls[0] == (0 if per_op else steps)                   # the path this trainer's render() took
    trainer.drain()
    torch.cuda.synchronize()
    params, moments = S16._collect(g, steps == 1)
    lr_max = max(grp["lr"] for grp in g.optimizer.param_groups)
    return tuple(losses), params, moments, lr_max


@pytest.mark.parametrize("lambda_dssim", [0.0, 0.2])
def test_trainer_on_the_node_against_the_op_by_op_trainer(monkeypatch, lambda_dssim):
    """Trainer(fused=False) -- render() + loss.backward() + optimizer.step(), what an unchanged train_4DGS.py drives -- on the node
    against the same trainer with pipe.per_op_autograd = True, under the rules of tests/test_fused_step16_gpu.py: after one step the
    loss at rtol 2e-5, Adam's first moments ((1 - beta1) x gradient) within 5e-5 of the tensor's largest magnitude, denom and
    max_radii2D equal; after three steps at most 1e-4 of a tensor's elements outside 2e-4 scale + 1e-6 and none beyond
    2 steps lr_max 1.01."""
    monkeypatch.setattr(FA, "NODE_WIDTHS", BOTH)
    la, pa, ma, _ = _train(True, 1, lambda_dssim)
    lf, pf, mf, _ = _train(False, 1, lambda_dssim)
    worst = {}
    for k in S16.LIVE:
        assert ma[k].shape == mf[k].shape and float(np.abs(ma[k]).max()) > 0, k
        worst[k] = float(np.abs(mf[k] - ma[k]).max()) / max(1e-30, float(np.abs(ma[k]).max()))
    print("lambda", lambda_dssim, "loss node", lf, "per-op", la, "first moments, error relative to the tensor's max:",
          {k: "%.2e" % v for k, v in worst.items()})
    np.testing.assert_allclose(lf, la, rtol=2e-5)
    for k, e in worst.items():
        assert e <= TOL, (k, e)
    np.testing.assert_array_equal(pf["denom"], pa["denom"])
    np.testing.assert_array_equal(pf["maxr"], pa["maxr"])
    assert float(pa["denom"].sum()) > 0

    steps = 3
    la, pa, _, lr_max = _train(True, steps, lambda_dssim)
    lf, pf, _, _ = _train(False, steps, lambda_dssim)
    figures = {}
    for k in S16.LIVE:
        scale = max(1e-12, float(np.abs(pa[k]).max()))
        diff = np.abs(pf[k] - pa[k])
        tight = 2e-4 * scale + 1e-6
        figures[k] = (float((diff > tight).mean()), float(diff.max()), tight)
    print("after", steps, "steps: (fraction outside the tight tolerance, largest difference, tight tolerance)",
          {k: "%.1e %.2e %.2e" % v for k, v in figures.items()})
    np.testing.assert_allclose(lf, la, rtol=2e-5)
    for k, (outliers, far, tight) in figures.items():
        assert outliers <= 1e-4, (k, "fraction of elements outside the tight tolerance", outliers)
        assert far <= 2.0 * steps * lr_max * 1.01, (k, far, lr_max)
    np.testing.assert_array_equal(pf["denom"], pa["denom"])
    np.testing.assert_array_equal(pf["maxr"], pa["maxr"])


# ---------------------------------------------------------------------------------------------------------------- 8
def test_a_refused_field_stays_op_by_op(monkeypatch):
    """One space axis of 520 texels: the second level's 1040 is beyond the field kernel's 1024 (Deformation.FIELD16_MAX_RES), the
    planes stay in the kilobytes.  Gradient mode renders it op by op, and every gradient arrives finite."""
    monkeypatch.setattr(FA, "NODE_WIDTHS", BOTH)
    scene, g, trainer = _setup(res=(520, 8, 8, 10))
    dn = g._deformation.deformation_net
    assert dn.grid.grids[1][0].shape[3] == 1040 or dn.grid.grids[1][0].shape[2] == 1040
    assert dn._mlp_fusable() and not dn._field16_fusable() and FA.node_width(dn) == 0
    ps = _params(g)
    pk = _render(scene, g, trainer, trainer.cams[2])
    names = _nodes(pk["render"])
    assert NODE not in names and len(names) > 5, names
    _loss([pk], _weights()).backward()
    torch.cuda.synchronize()
    assert float(pk["render"].detach().abs().max()) > 0
    for k, p in ps.items():
        assert p.grad is not None and p.grad.shape == p.shape and torch.isfinite(p.grad).all(), k
    assert float(ps["plane_1_0"].grad.abs().max()) > 0 and float(ps["xyz"].grad.abs().max()) > 0


# ---------------------------------------------------------------------------------------------------------------- 9
def _overlap_steps(overlap, steps=3):
    """tests/test_fused_autograd_gpu.py::_api_steps on the 16 x 2 trainer: (parameters, early optimizer launches on the second stream)."""
    ops = importlib.import_module(pkg + ".ops")
    old, calls = ops.API_OVERLAP, [0]
    ops.API_OVERLAP = overlap
    try:
        scene, g, trainer = S16._trainer(False, lambda_dssim=0.2)
        orig = g.optimizer.step_partial

        def counted(params, stream=None):
            calls[0] += 1
            assert stream is not None and stream != torch.cuda.current_stream().cuda_stream        # on the second stream
            return orig(params, stream=stream)
        g.optimizer.step_partial = counted
        for it in range(steps):
            trainer.step(5001 + it, cams=S16._cam_lists(trainer, it, 1, False))
        torch.cuda.synchronize()
        return {k: v.detach().clone() for k, v in S16._tensors(g).items()}, calls[0]
    finally:
        ops.API_OVERLAP = old


def test_second_stream_overlap_of_the_node_changes_no_result(monkeypatch):
    """ops.API_OVERLAP on the 16 x 2 node: the backward takes mom_deform_backward_split_n with the second stream and hands the
    optimizer its early hint (one early launch per step); the model after three steps is the one without the overlap under the
    rule of tests/test_fused_autograd_gpu.py::test_api_path_overlap_changes_no_result_and_withdraws_itself_when_gradients_are_touched."""
    monkeypatch.setattr(FA, "NODE_WIDTHS", BOTH)
    a, n_a = _overlap_steps(True)
    b, n_b = _overlap_steps(False)
    assert n_a == 3 and n_b == 0
    for k in a:
        scale = max(1e-12, float(b[k].abs().max()))
        frac = float(((a[k] - b[k]).abs() > 1e-3 * scale + 1e-6).float().mean())
        assert frac <= 2e-3, (k, frac)
