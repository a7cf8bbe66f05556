"""The deformation field of a 16-channel HexPlane model in one launch (csrc/deform_field16.hip: gather of two levels of 16
channels, 32-feature trunk, three heads, residuals and activations) against the two calls it stands for (mom_hexplane_forward
with channels 16 + mom_deform_forward_activated_n with in_features 32), against the CPU oracle, with its optional outputs, its
refusals, and as the field kernel of a no-grad render().

Bounds.  Outputs: the relative-to-tensor-scale measure of tests/test_hexplane16_gpu.py::_rel_close at 2e-6, its bound for this
model's forward.  Features and relu(h0): the bounds tests/test_deform_field_gpu.py has for the same comparison on the 32-channel
kernel (2e-6 and 5e-5 of max(1, scale)).  The kernel keeps the two calls' arithmetic term by term, so what is measured is 0
everywhere (every comparison prints its figure); render() is held to the whole-iteration test's torch.equal."""
import contextlib
import ctypes as C
import functools
import importlib

import numpy as np
import pytest
import torch

import hexplane_box_cases as hb

pytestmark = pytest.mark.gpu

pkg = "iclr2025_3d-mom_amd"
ops = importlib.import_module(pkg + ".ops")
N = importlib.import_module(pkg + "._native")
HexPlaneField = importlib.import_module(pkg + ".scene.hexplane").HexPlaneField

OUT = ("pts", "sc_d", "rot_d", "sc", "rot", "op")
WIDTH = dict(pts=3, sc_d=3, rot_d=4, feat=32, a0=64, sc=3, rot=4, op=1)
GRIDS = {"tiny": (8, 6, 10, 5), "shipped": (64, 64, 64, 150)}


def _field(res, multires=(1, 2), channels=16, seed=0):
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
    pts = (torch.rand(n, 3, generator=g) * 2 - 1) * torch.tensor([1.1, 1.3, 1.5])   # some outside the box (border clipping)
    pts[0] = torch.tensor([1.0, 1.2, 1.4])      # exact corners
    if n > 1:
        pts[1] = torch.tensor([-1.0, -1.2, -1.4])
    return pts


def _mlp(seed, n_in=32):
    g = torch.Generator().manual_seed(seed)
    mk = lambda *s: (torch.randn(*s, generator=g) * 0.3)
    params = [mk(64, n_in), mk(64)]
    for nout in (3, 3, 4):
        params += [mk(64, 64), mk(64), mk(nout, 64), mk(nout)]
    return params, mk


def _desc(f):
    return ops._hexplane_desc([[p.detach() for p in lv] for lv in f.grids], f.aabb, None, aabb_host=f.aabb_host())


def _rel(got, want):
    """(max |difference|, scale of `want`): tests/test_hexplane16_gpu.py::_rel_close's measure."""
    got, want = got.detach().float().cpu().numpy(), want.detach().float().cpu().numpy()
    assert got.shape == want.shape
    return float(np.abs(got - want).max()), max(float(np.abs(want).max()), 1e-30)


def _empty(P, names, fill=float("nan")):
    return {k: torch.full((P, WIDTH[k]), fill, device="cuda") for k in names}


def _two_calls(hp, md, P, xyz, scal, rot, flow, opac, t, order, coef):
    lib, s = N.lib(), N.current_stream()
    o = _empty(P, OUT + ("feat", "a0"))
    N.check(lib.mom_hexplane_forward(C.byref(hp), P, xyz.data_ptr(), None, t, N.ptr(order), o["feat"].data_ptr(), s), "hexplane_fwd")
    N.check(lib.mom_deform_forward_activated_n(C.byref(md), P, 32, o["feat"].data_ptr(), xyz.data_ptr(), scal.data_ptr(),
                                               rot.data_ptr(), flow.data_ptr(), coef, o["pts"].data_ptr(), o["sc_d"].data_ptr(),
                                               o["rot_d"].data_ptr(), o["a0"].data_ptr(), opac.data_ptr(), o["sc"].data_ptr(),
                                               o["rot"].data_ptr(), o["op"].data_ptr(), s), "deform_fwd")
    torch.cuda.synchronize()
    return o


def _one_launch(hp, md, P, xyz, scal, rot, flow, opac, t, order, coef, names=OUT + ("feat", "a0"), fill=float("nan")):
    o = _empty(P, names, fill)
    g = o.get
    ops.field16_forward(hp, md, P, xyz, t, order, scal, rot, flow, coef, o["pts"], o["sc_d"], o["rot_d"], g("feat"), g("a0"),
                        opac if "op" in o else None, g("sc"), g("rot"), g("op"), N.current_stream())
    torch.cuda.synchronize()
    return o


def _compare(a, b, what):
    for k in OUT:
        assert torch.isfinite(a[k]).all(), (what, k)
        err, scale = _rel(a[k], b[k])
        print(what, k, "max |diff| %.3e of scale %.3e" % (err, scale))
        assert err <= 2e-6 * scale, (what, k, err, scale)
    err, scale = _rel(a["feat"], b["feat"])
    print(what, "feat max |diff| %.3e of scale %.3e" % (err, scale))
    assert err <= 2e-6 * max(1.0, scale), (what, "feat", err, scale)
    err, scale = _rel(a["a0"], b["a0"])
    print(what, "a0 max |diff| %.3e of scale %.3e" % (err, scale))
    assert err <= 5e-5 * max(1.0, scale), (what, "a0", err, scale)


def _second_round_P():
    """Just above one pass of every workgroup (one per CU, sixteen waves of 32 Gaussians) + 33: two workgroups take a tile in a
    second round, and the last tile has one Gaussian."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    return cus * 16 * 32 + 33


@functools.lru_cache(maxsize=None)
def _field_on_gpu(grid):
    return _field(GRIDS[grid]).cuda()


@pytest.mark.parametrize("grid", ["tiny", "shipped"])
@pytest.mark.parametrize("P", [1, 31, 32, 33, 257, "second round"])
def test_one_launch_equals_the_two_calls(P, grid):
    P = _second_round_P() if P == "second round" else P
    f = _field_on_gpu(grid)
    hp, keep = _desc(f)
    assert N.lib().mom_deform_field16_supported(C.byref(hp)) == 1
    params_cpu, mk = _mlp(P)
    params = [p.cuda() for p in params_cpu]
    md = ops.DeformMLPFunction._desc(params)
    xyz, scal, rot, flow, opac = (t_.cuda() for t_ in (_points(P), mk(P, 3), mk(P, 4), mk(P, 3), mk(P, 1)))
    morton = ops.morton_order(xyz)
    for t in (0.0, 0.37, 1.0):
        for order in (None, morton):
            for coef in (0.0, 7.0):
                what = f"P={P} {grid} t={t} order={order is not None} coef={coef}"
                b = _two_calls(hp, md, P, xyz, scal, rot, flow, opac, t, order, coef)
                a = _one_launch(hp, md, P, xyz, scal, rot, flow, opac, t, order, coef)
                _compare(a, b, what)


@pytest.mark.parametrize("box", sorted(hb.BOXES))
def test_one_launch_equals_the_two_calls_on_the_points_that_define_a_box(box):
    """tests/hexplane_box_cases.py: asymmetric boxes, points on their faces and corners, an ulp inside and outside, far outside."""
    shape = "small"
    f = hb.field(16, box, shape).cuda()
    hp, keep = _desc(f)
    P = hb.P
    params_cpu, mk = _mlp(17)
    params = [p.cuda() for p in params_cpu]          # (kept: the descriptor holds their addresses only)
    md = ops.DeformMLPFunction._desc(params)
    xyz, scal, rot, flow, opac = (t_.cuda() for t_ in (hb.points(box), mk(P, 3), mk(P, 4), mk(P, 3), mk(P, 1)))
    morton = ops.morton_order(xyz)
    for t in (hb.SHAPES[shape][2], 0.0, 1.0):
        for order in (None, morton):
            b = _two_calls(hp, md, P, xyz, scal, rot, flow, opac, t, order, 7.0)
            a = _one_launch(hp, md, P, xyz, scal, rot, flow, opac, t, order, 7.0)
            _compare(a, b, f"{box} t={t} order={order is not None}")


class HP:          # the network of eulerian_150_16 on a small field
    net_width = 64; timebase_pe = 4; defor_depth = 0; posebase_pe = 10; scale_rotation_pe = 2; opacity_pe = 2
    timenet_width = 64; timenet_output = 32; bounds = 1.6; plane_tv_weight = 0.0001; time_smoothness_weight = 0.01
    l1_time_planes = 0.0001
    kplanes_config = {'grid_dimensions': 2, 'input_coordinate_dim': 4, 'output_coordinate_dim': 16, 'resolution': [8, 8, 8, 5]}
    multires = [1, 2]; no_dx = False; no_grid = False; no_ds = False; no_dr = False; no_do = True; no_dshs = True
    empty_voxel = False; grid_pe = 0; static_mlp = False; apply_rotation = False


def test_one_launch_matches_the_cpu_oracle():
    """deform_network on the CPU backend, as tests/test_hexplane16_gpu.py runs it for four levels, here for the 16 x 2 model."""
    from oracle import cpu_backend
    deform_network = importlib.import_module(pkg + ".scene.deformation").deform_network
    torch.manual_seed(11)
    net_c = deform_network(HP)
    net_c.deformation_net.set_aabb([1.0, 1.2, 1.4], [-1.0, -1.2, -1.4])
    with torch.no_grad():
        for g in net_c.deformation_net.grid.grids:
            for p in g:
                p.add_(torch.randn_like(p) * 0.2)
    net_g = deform_network(HP)
    net_g.deformation_net.set_aabb([1.0, 1.2, 1.4], [-1.0, -1.2, -1.4])
    net_g.load_state_dict(net_c.state_dict())
    net_g = net_g.cuda()
    dn = net_g.deformation_net
    assert dn._field16_fusable() and not dn._fusable()
    hp, keep = _desc(dn.grid)
    params = [p.detach() for p in dn._fused_params()]
    md = ops.DeformMLPFunction._desc(params)
    P = 257
    gen = torch.Generator().manual_seed(5)
    xyz, scal, rot = _points(P), torch.randn(P, 3, generator=gen), torch.randn(P, 4, generator=gen)
    op, sh, flow = torch.randn(P, 1, generator=gen), torch.randn(P, 16, 3, generator=gen), torch.randn(P, 3, generator=gen) * 0.01
    cu = [v.cuda() for v in (xyz, scal, rot, flow, op)]
    order = ops.morton_order(cu[0])
    for frame_num, delta_scale, t in ((0, 0, 0.0), (7, 1, 0.4)):
        with cpu_backend.installed(), torch.no_grad():
            pts, sc, ro_, op_o, sh_o = net_c(xyz, scal, rot, op, sh, t, flow, frame_num, delta_scale)
        a = _one_launch(hp, md, P, *cu, t, order, float(delta_scale * frame_num))
        for name, got, want in (("pts", a["pts"], pts), ("scales", a["sc_d"], sc), ("rots", a["rot_d"], ro_),
                                ("exp(scales)", a["sc"], torch.exp(sc)), ("normalize(rots)", a["rot"], torch.nn.functional.normalize(ro_)),
                                ("sigmoid(opacity)", a["op"], torch.sigmoid(op_o))):
            err, scale = _rel(got, want)
            print(f"f{frame_num}_d{delta_scale}", name, "max |diff| %.3e of scale %.3e" % (err, scale))
            assert err <= 2e-6 * scale, (name, frame_num, err, scale)


def test_optional_outputs():
    f = _field_on_gpu("shipped")
    hp, keep = _desc(f)
    P = 777
    params_cpu, mk = _mlp(3)
    params = [p.cuda() for p in params_cpu]          # (kept: the descriptor holds their addresses only)
    md = ops.DeformMLPFunction._desc(params)
    ins = [t_.cuda() for t_ in (_points(P), mk(P, 3), mk(P, 4), mk(P, 3), mk(P, 1))]
    order = ops.morton_order(ins[0])
    full = _one_launch(hp, md, P, *ins, 0.5, order, 0.7)
    for names in (("pts", "sc_d", "rot_d"), ("pts", "sc_d", "rot_d", "feat"), ("pts", "sc_d", "rot_d", "sc", "rot", "op"),
                  ("pts", "sc_d", "rot_d", "a0"), ("pts", "sc_d", "rot_d", "sc"), ("pts", "sc_d", "rot_d", "rot")):
        part = _one_launch(hp, md, P, *ins, 0.5, order, 0.7, names=names)
        for k in names:
            assert torch.isfinite(part[k]).all() and torch.equal(part[k], full[k]), (names, k)
    # P == 0 does nothing, and needs nothing
    assert N.lib().mom_deform_field16_forward(C.byref(hp), C.byref(md), 0, *([None] * 1), 0.5, *([None] * 4), 0.7, *([None] * 11)) == N.MOM_OK


def test_refusals_leave_the_outputs_untouched():
    lib, s = N.lib(), N.current_stream()
    P = 33
    params_cpu, mk = _mlp(3)
    params = [p.cuda() for p in params_cpu]          # (kept: the descriptor holds their addresses only)
    md = ops.DeformMLPFunction._desc(params)
    xyz, scal, rot, flow, opac = (t_.cuda() for t_ in (_points(P), mk(P, 3), mk(P, 4), mk(P, 3), mk(P, 1)))
    names = OUT + ("feat", "a0")

    def call(hp, o, opac_raw):
        q = lambda k: o[k].data_ptr()
        return lib.mom_deform_field16_forward(C.byref(hp), C.byref(md), P, xyz.data_ptr(), 0.3, None, scal.data_ptr(), rot.data_ptr(),
                                              flow.data_ptr(), 0.7, q("pts"), q("sc_d"), q("rot_d"), q("feat"), q("a0"), opac_raw,
                                              q("sc"), q("rot"), q("op"), None, s)

    fields = {"32 x 2": _field((8, 8, 8, 5), channels=32), "16 x 3": _field((8, 8, 8, 5), (1, 2, 4)),
              "16 x 4": _field((8, 8, 8, 5), (1, 2, 4, 8))}
    for what, f in fields.items():
        f = f.cuda()
        hp, keep = _desc(f)
        assert lib.mom_deform_field16_supported(C.byref(hp)) == 0, what
        assert lib.mom_deform_field_supported(C.byref(hp)) == (1 if what == "32 x 2" else 0), what     # as before
        o = _empty(P, names, fill=-77.0)
        assert call(hp, o, opac.data_ptr()) == N.MOM_EINVAL, what
        torch.cuda.synchronize()
        for k in names:
            assert bool((o[k] == -77.0).all()), (what, k)
        with pytest.raises(N.MomError):
            ops.field16_forward(hp, md, P, xyz, 0.3, None, scal, rot, flow, 0.7, o["pts"], o["sc_d"], o["rot_d"], None, None, None,
                                None, None, None, s)
    # 8 channels: no descriptor of the package has them (ops._hexplane_desc takes any count, the kernels 16 or 32)
    f8 = _field((8, 8, 8, 5), channels=8).cuda()
    hp8, keep8 = _desc(f8)
    assert hp8.channels == 8 and lib.mom_deform_field16_supported(C.byref(hp8)) == 0 and lib.mom_deform_field_supported(C.byref(hp8)) == 0
    o = _empty(P, names, fill=-77.0)
    assert call(hp8, o, opac.data_ptr()) == N.MOM_EINVAL
    torch.cuda.synchronize()
    for k in names:
        assert bool((o[k] == -77.0).all()), ("8 channels", k)
    # a supported field: opacity_act without opacity_raw
    f16 = _field((8, 8, 8, 5)).cuda()
    hp16, keep16 = _desc(f16)
    assert lib.mom_deform_field16_supported(C.byref(hp16)) == 1 and lib.mom_deform_field_supported(C.byref(hp16)) == 0
    assert call(hp16, o, None) == N.MOM_EINVAL
    torch.cuda.synchronize()
    for k in names:
        assert bool((o[k] == -77.0).all()), k
    assert call(hp16, o, opac.data_ptr()) == N.MOM_OK
    torch.cuda.synchronize()
    for k in names:
        assert torch.isfinite(o[k]).all() and not bool((o[k] == -77.0).any()), k


# ---------------------------------------------------------------------------------------------------------------------
# a model of the eulerian_150_16 shape on the tiny scene of tests/test_whole_step_gpu.py (as tests/test_hexplane16_gpu.py::_model16)
def _model16():
    from test_whole_step_gpu import CFG
    A = importlib.import_module(pkg + ".arguments")
    S = importlib.import_module(pkg + ".scene")
    T = importlib.import_module(pkg + ".train")
    kc = {'grid_dimensions': 2, 'input_coordinate_dim': 4, 'output_coordinate_dim': 16, 'resolution': [64, 64, 64, 150]}
    args, lp, op, pp, hp = A.default_args(kplanes_config=kc, multires=[1, 2])
    op.lambda_dssim = 0.0
    torch.manual_seed(6666)
    scene = S.SyntheticScene(CFG["P"], CFG["F"], CFG["W"], CFG["H"], seed=6666)
    g = S.GaussianModel(lp.sh_degree, hp, device=torch.device("cuda"))
    scene.init_gaussians(g)
    scene.make_trained_like(g)
    dn = g._deformation.deformation_net
    assert dn.grid.feat_dim == 32 and not dn._fusable() and dn._field16_fusable()
    trainer = T.Trainer(scene, g, op, hp, pp, stage="fine", delta_scale=1, sync_every_step=False, fused=False)
    assert trainer.fused is None
    return g, op, pp, hp, trainer


def test_no_grad_render_takes_the_one_launch_field_and_shows_the_op_by_op_image():
    R = importlib.import_module(pkg + ".gaussian_renderer")
    g, op, pp, hp, trainer = _model16()
    cam, bg = trainer.cams[1], trainer.background
    # gradient mode first, on the fresh model: op by op, and no forward-only renderer is made
    out_g = R.render(cam, g, pp, bg, stage="fine", delta_scale=1)
    assert getattr(g, "_fused_render", None) is None and getattr(g, "_fused_render_pool", None) is None
    assert out_g["render"].requires_grad
    img_g, depth_g, radii_g = out_g["render"].detach().clone(), out_g["depth"].detach().clone(), out_g["radii"].clone()
    with torch.no_grad():
        out = R.render(cam, g, pp, bg, stage="fine", delta_scale=1)
    torch.cuda.synchronize()
    fr = getattr(g, "_fused_render", None)
    assert fr is not None and fr.feat is None               # the fast path ran, without a [P,64] feature buffer
    assert float(img_g.abs().max()) > 0 and int((radii_g > 0).sum()) > 0
    assert torch.equal(out["render"], img_g)                # tests/test_hexplane16_gpu.py: img_ng against img_g, bit for bit
    assert torch.equal(out["depth"], depth_g) and torch.equal(out["radii"], radii_g)
    assert torch.equal(out["visibility_filter"], radii_g > 0)
    # two alternating streams
    R.set_render_streams(2)
    try:
        with torch.no_grad():
            outs = [R.render(cam, g, pp, bg, stage="fine", delta_scale=1) for _ in range(3)]
        for o in outs:
            assert "stream" in o and "ready" in o
            o["stream"].synchronize()
            assert torch.equal(o["render"], img_g) and torch.equal(o["depth"], depth_g) and torch.equal(o["radii"], radii_g)
        assert g._fused_render_pool.n == 2 and all(sl.feat is None for sl in g._fused_render_pool.slots[:2])
    finally:
        R.set_render_streams(1)
    # the training step keeps refusing the model
    FusedStep = importlib.import_module(pkg + ".fused_step").FusedStep
    with pytest.raises(N.MomError):
        FusedStep(g, op, hp, torch.zeros(3, device="cuda"))
