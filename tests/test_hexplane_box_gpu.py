"""HexPlane kernels (32 and 16 channels) at the points that define an asymmetric bounding box.

`set_aabb` takes the cloud's extremes, so up to six Gaussians of every trained model sit exactly on a face of the box.  On a MIN
face the reference's fp32 normalize_aabb (product rounded, then the difference) gives c = 1 - 2^-23 for most boxes, grid_sample's
border clip leaves the point inside, and the point keeps its position gradient; a kernel that contracts the expression into one
fma gets the border itself, clips, and returns zero for d xyz along that axis -- wrong at full scale, while the features differ
by rounding only.  The kernel tests elsewhere use the symmetric box +-(1.0, 1.2, 1.4), for which both forms give 1.0, and the
whole-iteration tests compare with a quantile; neither can see it.  tests/test_hexplane_box_cpu.py pins, without a GPU, that the
boxes used here do separate the two forms and that the gradients in question are far above the tolerances.

THE REFERENCE IS oracle.torch_ref.hexplane_features IN FP32 ON THE CPU, not an fp64 evaluation: the clip decision is defined by
the reference's fp32 roundings.  In exact arithmetic the point sits on the border and IS clipped, so an fp64 statement would agree
with the defect.

Tolerances: those of tests/test_ops_gpu.py::test_hexplane_forward_backward_parity and tests/test_hexplane16_gpu.py (features rtol
2e-5 / atol 5e-6; gradients rtol 2e-4, atol 2e-5 x the tensor's scale), per element, nothing left out.  And one assertion without a
tolerance: at every special point the zero pattern of d xyz equals the oracle's."""
import ctypes as C
import importlib

import numpy as np
import pytest
import torch

import hexplane_box_cases as hb

pytestmark = pytest.mark.gpu

pkg = "iclr2025_3d-mom_amd"
ops = importlib.import_module(pkg + ".ops")
N = importlib.import_module(pkg + "._native")

BOXES = list(hb.BOXES)
SPECIAL = hb.special_indices()


def _check_features(feat, ref, what):
    np.testing.assert_allclose(feat.detach().cpu().numpy(), ref[0], rtol=hb.FEAT_RTOL, atol=hb.FEAT_ATOL, err_msg=what + " features")


def _check_dxyz(dxyz, ref_dxyz, rows, what):
    """The zero pattern at `rows` (no tolerance), then every element of the tensor."""
    g = dxyz.detach().cpu().numpy()
    got0, want0 = g[rows] == 0, ref_dxyz[rows] == 0
    wrong = [(int(rows[i]), int(k), float(g[rows[i], k]), float(ref_dxyz[rows[i], k])) for i, k in zip(*np.nonzero(got0 != want0))]
    print(f"{what}: d xyz max |err| {float(np.abs(g - ref_dxyz).max()):.3e} of scale {float(np.abs(ref_dxyz).max()):.3e}; "
          f"zero-pattern mismatches (point, axis, got, oracle): {wrong}")
    assert not wrong, (what, "clip decision differs from the oracle's at (point, axis, got, oracle)", wrong)
    np.testing.assert_allclose(g, ref_dxyz, rtol=hb.GRAD_RTOL, atol=hb.grad_atol(ref_dxyz), err_msg=what + " dxyz")


def _check_planes(grads, ref_planes, what):
    for l, (gl, rl) in enumerate(zip(grads, ref_planes)):
        for i, (a, b) in enumerate(zip(gl, rl)):
            a = a.detach().cpu().numpy()
            assert a.shape == b.shape
            np.testing.assert_allclose(a, b, rtol=hb.GRAD_RTOL, atol=hb.grad_atol(b), err_msg=f"{what} plane {l} {i}")


def _module_backward(fg, pts, t, w, form):
    """features, d xyz, [[d plane]] of the field module on the GPU in one of its forms."""
    n = pts.shape[0]
    fg.zero_grad()
    fg._order, fg._order_age, fg._porders = None, 0, None
    if form == "identity":
        fg._order, fg._order_age = torch.arange(n, dtype=torch.int32, device="cuda"), -10**9
    p = pts.cuda().requires_grad_(True)
    feat = fg(p, torch.full((n, 1), t, device="cuda") if form == "per_point_t" else t)
    (feat * w.cuda()).sum().backward()
    torch.cuda.synchronize()
    return feat, p.grad, [[q.grad for q in g] for g in fg.grids]


# scalar time in Morton order with the two-pass backward (the default); the same with an identity order; per-point timestamps
# (generic forward and generic backward); the two gathers of the 32-channel two-pass backward by name
FORMS = [(32, "morton"), (32, "identity"), (32, "per_point_t"), (32, "gather5"), (32, "gather6"),
         (16, "morton"), (16, "identity"), (16, "per_point_t")]


@pytest.mark.parametrize("box", BOXES)
@pytest.mark.parametrize("channels,form", FORMS)
def test_field_at_the_box_faces(channels, form, box, monkeypatch):
    ref = hb.oracle(channels, box, "small")
    fg = hb.field(channels, box, "small").cuda()
    if form.startswith("gather"):
        monkeypatch.setenv("MOM_HEX_GATHER", form[-1])
    else:
        monkeypatch.delenv("MOM_HEX_GATHER", raising=False)
    what = f"{channels} channels, {box}, {form}"
    feat, dxyz, planes = _module_backward(fg, hb.points(box), hb.SHAPES["small"][2], hb.weights(fg.feat_dim), form)
    assert feat.shape == (hb.P, 2 * channels)
    _check_features(feat, ref, what)
    _check_dxyz(dxyz, ref[1], SPECIAL, what)
    _check_planes(planes, ref[2], what)


@pytest.mark.parametrize("box", BOXES)
@pytest.mark.parametrize("channels", [32, 16])
def test_three_level_field_at_the_box_faces(channels, box):
    """(16, 12, 10, 7) x (1, 2, 4): three levels, which no fused kernel takes -- the per-op kernels in their six-row form."""
    ref = hb.oracle(channels, box, "three_levels")
    fg = hb.field(channels, box, "three_levels").cuda()
    what = f"{channels} channels, {box}, three levels"
    feat, dxyz, planes = _module_backward(fg, hb.points(box), hb.SHAPES["three_levels"][2], hb.weights(fg.feat_dim), "morton")
    _check_features(feat, ref, what)
    _check_dxyz(dxyz, ref[1], SPECIAL, what)
    _check_planes(planes, ref[2], what)


@pytest.mark.parametrize("box", BOXES)
def test_fused_field_forward_and_the_step_backward_at_the_box_faces(box):
    """32 channels x 2 levels as the fused training step runs them: ops.field_forward fused (csrc/deform_field.hip, make_record)
    against the two-kernel path and the oracle, then mom_hexplane_backward_lines on the time lines that forward left in the field
    scratch, with the orders of mom_hexplane_orders and a Morton processing order."""
    from test_deform_field_gpu import _mlp, _run_forward
    ref = hb.oracle(32, box, "small")
    t = hb.SHAPES["small"][2]
    fg = hb.field(32, box, "small").cuda()
    params_cpu, mk = _mlp(7)
    params = [p.cuda() for p in params_cpu]
    xyz = hb.points(box).cuda()
    scal, rot, flow, opac = (mk(hb.P, k).cuda() for k in (3, 4, 3, 1))
    order = ops.morton_order(xyz)
    what = f"32 channels, {box}, fused"
    b = _run_forward(fg, params, hb.P, xyz, scal, rot, flow, opac, t, order, fused=False)
    a = _run_forward(fg, params, hb.P, xyz, scal, rot, flow, opac, t, order, fused=True)       # last: its lines stay in the scratch
    _check_features(a["feat"], ref, what)
    _check_features(b["feat"], ref, what + " (two kernels)")
    assert float((a["feat"] - b["feat"]).abs().max()) <= 2e-6 * max(1.0, float(b["feat"].abs().max()))     # tests/test_deform_field_gpu.py
    # the backward the fused step takes
    lib, s = N.lib(), N.current_stream()
    levels = [[p.detach() for p in lv] for lv in fg.grids]
    grads = [[torch.zeros_like(p) for p in lv] for lv in levels]
    hp, keep = ops._hexplane_desc(levels, fg.aabb, grads, aabb_host=fg.aabb_host())
    assert lib.mom_deform_field_supported(C.byref(hp)) == 1
    po = ops.hexplane_orders(xyz, levels, fg.aabb, aabb_host=fg.aabb_host())
    dfeat = hb.weights(fg.feat_dim).cuda().contiguous()
    dxyz = torch.zeros(hb.P, 3, device="cuda")
    scratch = torch.empty(lib.mom_hexplane_backward_scratch_bytes(C.byref(hp), hb.P), dtype=torch.uint8, device="cuda")
    N.check(lib.mom_hexplane_backward_lines(C.byref(hp), hb.P, xyz.data_ptr(), t, order.data_ptr(), dfeat.data_ptr(), dxyz.data_ptr(),
                                            po[0].data_ptr(), po[1].data_ptr(), scratch.data_ptr(),
                                            ops.field_scratch(hp, xyz.device).data_ptr(), s), "mom_hexplane_backward_lines")
    torch.cuda.synchronize()
    _check_dxyz(dxyz, ref[1], SPECIAL, what + " backward_lines")
    _check_planes(grads, ref[2], what + " backward_lines")


@pytest.mark.parametrize("channels", [32, 16])
def test_clouds_that_set_their_own_box(channels):
    """Two dozen seeded clouds of 300 points, the box from each cloud's own extremes as training sets it: at the (up to six) points
    that define the box the zero pattern of d xyz is the oracle's, and the whole tensor agrees.  The emulation of
    tests/hexplane_box_cases.py must predict, for several of the clouds, an axis on which a contracted normalisation clips the
    min-face point and torch does not: asserted here from the emulation, not read off the kernel."""
    fg = hb.field(channels, "symmetric", "small").cuda()
    t = hb.SHAPES["small"][2]
    w = hb.weights(fg.feat_dim)
    predicted, failures = 0, []
    for seed in hb.CLOUD_SEEDS:
        pts, hi, lo = hb.cloud(seed)
        fg.set_aabb(hi, lo)
        ref = hb.oracle_of(fg, pts, t, w)
        defining = hb.defining_points(pts, hi, lo)
        axes = hb.predicted_divergent_axes(hi, lo, "small")
        predicted += bool(axes)
        for i, k, side in defining:
            if side == "max" or (side == "min" and k in axes):
                assert (ref[1][i, k] != 0) == (side == "min"), (seed, i, k, side)       # the emulation agrees with the oracle
        feat, dxyz, planes = _module_backward(fg, pts, t, w, "morton")
        rows = np.asarray(sorted({i for i, _, _ in defining}))
        try:
            _check_features(feat, ref, f"cloud {seed}")
            _check_dxyz(dxyz, ref[1], rows, f"cloud {seed}, {channels} channels, predicted axes {axes}")
        except AssertionError as e:
            failures.append((seed, axes, str(e)[:300]))
    assert predicted >= 3, predicted
    assert not failures, failures
