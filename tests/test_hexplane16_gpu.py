"""HexPlane fields with 16-channel planes (kplanes_config output_coordinate_dim = 16: the reference's dnerf eulerian_150_16,
dynerf and hypernerf configurations; resolution [64, 64, 64, 150], multires [1, 2] or [1, 2, 4]) on the GPU: the 16-channel
instantiations of csrc/hexplane.hip against oracle.torch_ref.hexplane_features (the reference's grid_sample sequence, channel-agnostic), and a
model of that shape through the op-by-op module, render() and one training iteration against the CPU oracle.

Tolerances are those of tests/test_ops_gpu.py::test_hexplane_forward_backward_parity (forward rtol 2e-5 / atol 5e-6; gradients
rtol 2e-4 / atol 2e-5 max(1, |ref|max)): the same arithmetic with 16 instead of 32 terms in the position-gradient sum."""
import contextlib
import ctypes as C
import importlib

import numpy as np
import pytest
import torch

from oracle import torch_ref as tr

pytestmark = pytest.mark.gpu

pkg = "iclr2025_3d-mom_amd"
ops = importlib.import_module(pkg + ".ops")
N = importlib.import_module(pkg + "._native")
HexPlaneField = importlib.import_module(pkg + ".scene.hexplane").HexPlaneField


def _field(res=(8, 8, 8, 5), multires=(1, 2), seed=0, channels=16):
    torch.manual_seed(seed)
    cfg = {'grid_dimensions': 2, 'input_coordinate_dim': 4, 'output_coordinate_dim': channels, 'resolution': list(res)}
    f = HexPlaneField(1.6, cfg, list(multires))
    f.set_aabb([1.0, 1.2, 1.4], [-1.0, -1.2, -1.4])
    with torch.no_grad():
        for g in f.grids:
            for p in g:
                p.add_(torch.randn_like(p) * 0.2)
    return f


def _points(n, seed=1):
    g = torch.Generator().manual_seed(seed)
    pts = (torch.rand(n, 3, generator=g) * 2 - 1) * torch.tensor([1.1, 1.3, 1.5])   # some outside the box
    pts[0] = torch.tensor([1.0, 1.2, 1.4])      # exact corners
    if n > 1:
        pts[1] = torch.tensor([-1.0, -1.2, -1.4])
    return pts


def _close(a, b, what=""):   # sums of signed terms: tolerance relative to the tensor's scale
    np.testing.assert_allclose(a, b, rtol=2e-4, atol=2e-5 * max(1.0, float(np.abs(b).max())), err_msg=what)


def _oracle(f, pts, t, w):
    """(features, d/d points, [[d/d plane]]) of the reference's op sequence on the CPU."""
    p_cpu = pts.clone().requires_grad_(True)
    planes_cpu = [[p.detach().clone().contiguous().requires_grad_(True) for p in g] for g in f.grids]
    feat = tr.hexplane_features(p_cpu, t, f.aabb.detach(), planes_cpu)
    (feat * w).sum().backward()
    return feat.detach().numpy(), p_cpu.grad.numpy(), [[p.grad.numpy() for p in g] for g in planes_cpu]


def _grads_close(fg, p_gpu, ref, what):
    _close(p_gpu.grad.cpu().numpy(), ref[1], what + " dxyz")
    for l, (gl, gc) in enumerate(zip(fg.grids, ref[2])):
        for i, (a, b) in enumerate(zip(gl, gc)):
            assert a.grad.shape == b.shape
            _close(a.grad.cpu().numpy(), b, f"{what} plane {l} {i}")


@pytest.mark.parametrize("res,multires,t", [((8, 8, 8, 5), (1, 2), 0.3), ((16, 12, 10, 7), (1, 2, 4), 0.0),
                                             ((8, 8, 8, 5), (1,), 1.0), ((64, 64, 64, 150), (1, 2), 0.77)])
def test_forward_backward_parity_16_channels(res, multires, t):
    f = _field(res, multires)
    assert f.feat_dim == 16 * len(multires)
    pts = _points(257)
    w = torch.randn(257, f.feat_dim, generator=torch.Generator().manual_seed(3))
    ref = _oracle(f, pts, t, w)
    fg = f.cuda()
    # Morton order, two-pass backward
    p_gpu = pts.cuda().requires_grad_(True)
    feat = fg(p_gpu, t)
    assert feat.shape == (257, f.feat_dim)
    (feat * w.cuda()).sum().backward()
    torch.cuda.synchronize()
    np.testing.assert_allclose(feat.detach().cpu().numpy(), ref[0], rtol=2e-5, atol=5e-6)
    _grads_close(fg, p_gpu, ref, "morton")
    # identity order
    fg.zero_grad()
    fg._order, fg._order_age = torch.arange(257, dtype=torch.int32, device="cuda"), -10**9
    p2 = pts.cuda().requires_grad_(True)
    feat_id = fg(p2, t)
    np.testing.assert_array_equal(feat_id.detach().cpu().numpy(), feat.detach().cpu().numpy())
    (feat_id * w.cuda()).sum().backward()
    _grads_close(fg, p2, ref, "identity")
    # per-point timestamps (the form the reference passes): the same features bit for bit, the generic backward
    fg.zero_grad()
    p3 = pts.cuda().requires_grad_(True)
    feat2 = fg(p3, torch.full((257, 1), t, device="cuda"))
    np.testing.assert_array_equal(feat2.detach().cpu().numpy(), feat.detach().cpu().numpy())
    (feat2 * w.cuda()).sum().backward()
    _grads_close(fg, p3, ref, "per-point t")


# (the two-pass backward against the generic one, both channel counts: tests/test_hexplane_widths_gpu.py)


class HP:
    net_width = 64; timebase_pe = 4; defor_depth = 0; posebase_pe = 10; scale_rotation_pe = 2; opacity_pe = 2
    timenet_width = 64; timenet_output = 32; bounds = 1.6; plane_tv_weight = 0.0001; time_smoothness_weight = 0.01
    l1_time_planes = 0.0001
    kplanes_config = {'grid_dimensions': 2, 'input_coordinate_dim': 4, 'output_coordinate_dim': 16, 'resolution': [8, 8, 8, 5]}
    multires = [1, 2, 4, 8]; no_dx = False; no_grid = False; no_ds = False; no_dr = False; no_do = True; no_dshs = True
    empty_voxel = False; grid_pe = 0; static_mlp = False; apply_rotation = False


def _rel_close(got, want, rel, what=""):      # tests/test_golden_gpu.py::close
    got = got.detach().float().cpu().numpy()
    want = want.detach().float().cpu().numpy()
    scale = max(float(np.abs(want).max()), 1e-30)
    err = float(np.abs(got - want).max())
    assert got.shape == want.shape and err <= rel * scale, (what, err, scale)


def test_four_levels_of_16_channels_run_op_by_op_and_match_the_cpu_oracle():
    """16 channels x multires (1, 2, 4, 8) = 64 features, the fused MLP's width -- but not the fused kernels' 32 x 2 layout."""
    from oracle import cpu_backend
    deform_network = importlib.import_module(pkg + ".scene.deformation").deform_network
    torch.manual_seed(11)
    net_c = deform_network(HP)
    net_c.deformation_net.set_aabb([1.0, 1.2, 1.4], [-1.0, -1.2, -1.4])
    with torch.no_grad():
        for g in net_c.deformation_net.grid.grids:
            for p in g:
                p.add_(torch.randn_like(p) * 0.2)
    assert net_c.deformation_net.grid.feat_dim == 64 and not net_c.deformation_net._fusable()
    net_g = deform_network(HP)
    net_g.deformation_net.set_aabb([1.0, 1.2, 1.4], [-1.0, -1.2, -1.4])
    net_g.load_state_dict(net_c.state_dict())
    net_g = net_g.cuda()
    assert not net_g.deformation_net._fusable()
    P = 257
    gen = torch.Generator().manual_seed(5)
    xyz, scal, rot = _points(P), torch.randn(P, 3, generator=gen), torch.randn(P, 4, generator=gen)
    op, sh, flow = torch.randn(P, 1, generator=gen), torch.randn(P, 16, 3, generator=gen), torch.randn(P, 3, generator=gen) * 0.01
    ws = [torch.randn(P, k, generator=gen) for k in (3, 3, 4)]
    for frame_num, delta_scale, t in ((0, 0, 0.0), (7, 1, 0.4)):
        outs = {}
        for dev, net in (("cpu", net_c), ("cuda", net_g)):
            x, s, r = (v.clone().to(dev).requires_grad_(True) for v in (xyz, scal, rot))
            net.zero_grad(set_to_none=True)
            with (cpu_backend.installed() if dev == "cpu" else contextlib.nullcontext()):
                pts, sc, ro_, op_o, sh_o = net(x, s, r, op.to(dev), sh.to(dev), t, flow.to(dev), frame_num, delta_scale)
                ((pts * ws[0].to(dev)).sum() + (sc * ws[1].to(dev)).sum() + (ro_ * ws[2].to(dev)).sum()).backward()
            assert torch.equal(op_o.cpu(), op) and torch.equal(sh_o.cpu(), sh)            # pass-through (no_do, no_dshs)
            outs[dev] = (pts, sc, ro_, x.grad, s.grad, r.grad, {k: p.grad for k, p in net.named_parameters()})
        a, b = outs["cuda"], outs["cpu"]
        tag = f"f{frame_num}_d{delta_scale}"
        for i, (name, rel) in enumerate((("pts", 2e-6), ("scales", 2e-6), ("rots", 2e-6), ("dxyz", 2e-5), ("dscal", 2e-6), ("drot", 2e-6))):
            _rel_close(a[i], b[i], rel, f"{name} {tag}")
        live = 0
        for k, gref in b[6].items():
            if gref is None:
                assert a[6][k] is None, k
            else:
                live += 1
                _rel_close(a[6][k], gref, 3e-5, f"grad {tag} {k}")
        assert live >= 24 + 14          # every plane and the trunk + three heads


def test_refusals():
    pts = _points(33).cuda()
    for ch in (8, 24):
        f = _field(channels=ch).cuda()
        with pytest.raises(N.MomError):
            f(pts, 0.3)
    f16, f32 = _field().cuda(), _field(channels=32).cuda()
    with pytest.raises(N.MomError, match="channel count"):
        ops.hexplane_features(pts, 0.3, f16.aabb, [list(f16.grids[0]), list(f32.grids[1])], aabb_host=f16.aabb_host())
    d, keep = ops._hexplane_desc([list(g) for g in f16.grids], f16.aabb, aabb_host=f16.aabb_host())
    assert d.channels == 16 and d.levels == 2
    assert N.lib().mom_deform_field_supported(C.byref(d)) == 0
    d32, keep32 = ops._hexplane_desc([list(g) for g in f32.grids], f32.aabb, aabb_host=f32.aabb_host())
    assert N.lib().mom_deform_field_supported(C.byref(d32)) == 1
    scene, g, op, pp, hp = _model16("cuda")
    FusedStep = importlib.import_module(pkg + ".fused_step").FusedStep
    with pytest.raises(N.MomError):
        FusedStep(g, op, hp, torch.zeros(3, device="cuda"))


def test_plane_regulariser_on_16_channel_planes():
    """The regulariser kernel counts a plane row in units of 32 floats; a 16-channel row of W texels is W / 2 of them."""
    f = _field((8, 6, 10, 5), (1, 2))
    planes_cpu = [p.detach().clone().contiguous().requires_grad_(True) for g in f.grids for p in g]
    ws = [0.01 if i % 6 in (2, 4, 5) else 1e-4 for i in range(12)]
    wl = [1e-4 if i % 6 in (2, 4, 5) else 0.0 for i in range(12)]
    val_ref = tr.plane_regulation(planes_cpu, ws, wl)
    (val_ref * 3.0).backward()
    fg = f.cuda()
    planes = [p for g in fg.grids for p in g]
    val = ops.plane_regulation(planes, ws, wl)
    (val * 3.0).backward()
    torch.cuda.synchronize()
    np.testing.assert_allclose(float(val), float(val_ref), rtol=2e-5)
    for a, b in zip(planes, planes_cpu):
        np.testing.assert_allclose(a.grad.cpu().numpy(), b.grad.numpy(), rtol=2e-4, atol=1e-9)
    odd = ops.make_plane(16, 4, 5, device="cuda").requires_grad_(True)       # 5 x 16 floats: no whole number of units
    with pytest.raises(N.MomError):
        ops.plane_regulation([odd], [1.0], [0.0])


# ---------------------------------------------------------------------------------------------------------------------
# a model of the eulerian_150_16 shape (W = 64, D = 0, no_do, no_dshs, 16 channels, multires [1, 2]) on the tiny scene of
# tests/test_whole_step_gpu.py
def _model16(device):
    from op_by_op_step import tiny_scene_model
    kc = {'grid_dimensions': 2, 'input_coordinate_dim': 4, 'output_coordinate_dim': 16, 'resolution': [64, 64, 64, 150]}
    scene, g, op, pp, hp = tiny_scene_model(device, kplanes_config=kc, multires=[1, 2])
    assert hp.kplanes_config["output_coordinate_dim"] == 16 and hp.net_width == 64 and hp.defor_depth == 0 and hp.no_do and hp.no_dshs
    assert g._deformation.deformation_net.grid.feat_dim == 32 and not g._deformation.deformation_net._fusable()
    return scene, g, op, pp, hp


def _one_step16(device):
    """tests/test_whole_step_gpu.py::_one_step on the autograd path (render() + loss.backward() + optimizer.step()):
    tests/op_by_op_step.py::one_step on camera 1."""
    from op_by_op_step import one_step
    loss, grads, stats, images, received = one_step(device, _model16)
    assert not any(received.values()), ("dead heads received a gradient", received)
    return loss, grads, stats, None if images is None else images[0]


def test_one_iteration_and_a_no_grad_render_of_a_16_channel_model():
    """Tolerances: tests/test_whole_step_gpu.py::_against_the_oracle at its "tiny" size (tests/op_by_op_step.py::assert_tiny_gates)."""
    from op_by_op_step import assert_tiny_gates
    from test_whole_step_gpu import LIVE
    ref = _one_step16("cpu")
    got = _one_step16("cuda")
    img_ng, img_g = got[3]
    assert float(img_g.abs().max()) > 0 and torch.equal(img_ng, img_g)       # no-grad render() = grad-mode render(), bit for bit
    assert sorted(got[1]) == sorted(LIVE)
    for k in LIVE:
        if k.startswith("plane_"):
            assert got[1][k].shape[1] == 16
    assert_tiny_gates(ref, got)


def test_forward_is_deterministic():
    """Fifty launches of the shared-timestamp forward, bit for bit (the short form of the 32-channel forward's soak)."""
    f = _field((64, 64, 64, 150), (1, 2)).cuda()
    pts = _points(5000).cuda()
    levels = [list(g) for g in f.grids]
    order = ops.morton_order(pts)
    with torch.no_grad():
        first = ops.hexplane_features(pts, 0.77, f.aabb, levels, order=order, aabb_host=f.aabb_host())
        for _ in range(49):
            again = ops.hexplane_features(pts, 0.77, f.aabb, levels, order=order, aabb_host=f.aabb_host())
            assert torch.equal(again, first)
    assert float(first.abs().max()) > 0 and bool(torch.isfinite(first).all())
