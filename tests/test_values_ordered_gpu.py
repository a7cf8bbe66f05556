"""The ordered loss values on the GPU (include/mom4d.h, "ordered loss values"): the device returns the host twin's bits, twice, at every
size of values_ordered_cases.py; the gradients beside them are the atomic entries' bit for bit; the switch carries the ordered
entries through the three autograd functions; and under it a training run logs the same numbers run after run.  Nothing here asserts
that the atomic path differs."""
import ctypes as C
import importlib
import random

import numpy as np
import pytest
import torch

import values_ordered_cases as vc

pytestmark = pytest.mark.gpu

pkg = vc.pkg
ops = importlib.import_module(pkg + ".ops")
N = vc.N


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def stream():
    return N.current_stream()


def l1_device(img, gt, ordered=True, offset=0):
    """(sums2, dimg) of the device entry; offset: the three arrays start that many floats off a 16-byte boundary."""
    n = img.size
    a, b = (torch.zeros(n + offset, device="cuda")[offset:].copy_(dev(x)) for x in (img, gt))
    dimg = torch.full((n + offset,), float("nan"), device="cuda")[offset:]
    sums = torch.full((2,), float("nan"), device="cuda")
    lib = N.lib()
    if ordered:
        need = lib.mom_l1_loss_ordered_scratch_bytes(n)
        scratch = torch.full((need + 64,), 0xFF, dtype=torch.uint8, device="cuda")          # NaN patterns: nothing is read unwritten
        rc = lib.mom_l1_loss_ordered(n, a.data_ptr(), b.data_ptr(), dimg.data_ptr(), sums.data_ptr(), scratch.data_ptr(), need, stream())
    else:
        rc = lib.mom_l1_loss(n, a.data_ptr(), b.data_ptr(), dimg.data_ptr(), sums.data_ptr(), stream())
    assert rc == N.MOM_OK
    return sums.cpu().numpy(), dimg.cpu().numpy()


@pytest.mark.parametrize("n", vc.L1_SIZES)
def test_l1_device_equals_the_host_twin_twice_and_keeps_the_gradient(n):
    img, gt = vc.l1_inputs(n)
    want, want_dimg = vc.l1_host(img, gt)
    one, two = l1_device(img, gt), l1_device(img, gt)
    for got in (one, two):
        np.testing.assert_array_equal(vc.bits(got[0]), vc.bits(want))
        np.testing.assert_array_equal(vc.bits(got[1]), vc.bits(want_dimg))
    atomic = l1_device(img, gt, ordered=False)
    np.testing.assert_array_equal(vc.bits(one[1]), vc.bits(atomic[1]))                     # the gradient image is mom_l1_loss's
    np.testing.assert_allclose(one[0], atomic[0], rtol=1e-4)
    if n >= vc.L1_SHARE:                                                                     # off a 16-byte boundary: one by one, same order
        off = l1_device(img, gt, offset=1)
        np.testing.assert_array_equal(vc.bits(off[0]), vc.bits(want))
        np.testing.assert_array_equal(vc.bits(off[1]), vc.bits(want_dimg))


def ssim_device(a, b, ordered=True):
    """(sum[0] as float64, dm, the workgroup totals or None)."""
    Cn, H, W = a.shape
    x, y = dev(a), dev(b)
    dm = torch.full((3, Cn, H, W), float("nan"), device="cuda")
    total = torch.full((N.SSIM_SUM_SLOTS,), float("nan"), dtype=torch.float64, device="cuda")
    lib, totals = N.lib(), None
    if ordered:
        need = lib.mom_ssim_ordered_scratch_bytes(Cn, H, W)
        scratch = torch.full((need + 64,), 0xFF, dtype=torch.uint8, device="cuda")
        rc = lib.mom_ssim_forward_ordered(Cn, H, W, ops.ssim_window(), x.data_ptr(), y.data_ptr(), dm.data_ptr(), total.data_ptr(),
                                          scratch.data_ptr(), need, stream())
        totals = scratch[:need].cpu().numpy().view(np.float32).copy()
        assert np.isnan(total[1:].cpu().numpy()).all()                                       # only sum[0] is written
    else:
        rc = lib.mom_ssim_forward(Cn, H, W, ops.ssim_window(), x.data_ptr(), y.data_ptr(), dm.data_ptr(), total.data_ptr(), stream())
    assert rc == N.MOM_OK
    return total[:1].cpu().numpy()[0], dm.cpu().numpy(), totals


@pytest.mark.parametrize("which", ["g3", "tile", "flat"])
def test_ssim_device_equals_the_host_twin_twice_and_keeps_the_derivative_maps(which):
    a, b = vc.ssim_images(which)
    one, two = ssim_device(a, b), ssim_device(a, b)
    assert one[2].size == 3 * ((a.shape[1] + 15) // 16) * ((a.shape[2] + 15) // 16) and np.isfinite(one[2]).all()
    want = vc.ssim_sum_host(one[2])
    for got in (one, two):
        assert vc.bits(np.float64(got[0])) == vc.bits(np.float64(want))
        np.testing.assert_array_equal(vc.bits(got[1]), vc.bits(one[1]))
        np.testing.assert_array_equal(vc.bits(got[2]), vc.bits(one[2]))
    atomic = ssim_device(a, b, ordered=False)
    np.testing.assert_array_equal(vc.bits(one[1]), vc.bits(atomic[1]))                     # dm is mom_ssim_forward's
    assert abs(one[0] - atomic[0]) <= 1e-12 * a.size                                         # doubles of at most 256 each: the same sum
    if which == "flat":
        assert abs(one[0] / a.size - 1.0) < 1e-5


@pytest.mark.parametrize("shape", vc.SSIM_SHAPES)
def test_ssim_sum_device_equals_the_host_twin_on_totals_that_show_an_order(shape):
    totals = vc.ssim_totals(shape)
    want = vc.ssim_sum_host(totals)
    t = dev(totals)
    for _ in range(2):
        out = torch.full((1,), float("nan"), dtype=torch.float64, device="cuda")
        assert N.lib().mom_ssim_sum_ordered(totals.size, t.data_ptr(), out.data_ptr(), stream()) == N.MOM_OK
        assert vc.bits(out.cpu().numpy())[0] == vc.bits(np.float64(want))[0]


def reg_device(planes):
    held = [dev(p) for p, _, _ in planes]
    arr = vc.reg_desc(planes, [h.data_ptr() for h in held])
    lib = N.lib()
    need = lib.mom_plane_regulation_ordered_scratch_bytes(arr, len(planes))
    scratch = torch.full((need + 64,), 0xFF, dtype=torch.uint8, device="cuda")
    out = torch.full((1,), float("nan"), device="cuda")
    assert lib.mom_plane_regulation_ordered(arr, len(planes), out.data_ptr(), scratch.data_ptr(), need, stream()) == N.MOM_OK
    atomic = torch.full((1,), float("nan"), device="cuda")
    assert lib.mom_plane_regulation(arr, len(planes), atomic.data_ptr(), stream()) == N.MOM_OK
    return out.cpu().numpy()[0], atomic.cpu().numpy()[0]


@pytest.mark.parametrize("name", vc.REG_CASES)
def test_regulariser_device_equals_the_host_twin_twice(name):
    planes = vc.reg_case(name)
    want = vc.reg_host(planes)
    for _ in range(2):
        got, atomic = reg_device(planes)
        assert vc.bits(np.float32(got)) == vc.bits(np.float32(want))
        assert abs(float(got) - float(atomic)) <= 1e-4 * abs(float(atomic))


def _plane_leaf(p, channels):
    H, row = p.shape
    t = ops.make_plane(channels, H, row // channels, device="cuda")
    t.copy_(dev(p).view(H, row // channels, channels).permute(2, 0, 1)[None])
    return t.requires_grad_(True)


def _through_autograd(name, channels):
    """(l1 value, l1 sums, l1 gradient, ssim value, ssim gradient, regulariser value, plane gradients) of the three functions."""
    img, gt = vc.ssim_images("g3")
    x = dev(img).requires_grad_(True)
    l1, sums = ops.l1_loss_with_sums(x, dev(gt))
    l1.backward()
    g_l1 = x.grad.clone()
    x.grad = None
    s = ops.ssim(x, dev(gt))
    (s * 0.2).backward()
    planes = vc.reg_case(name)
    leaves = [_plane_leaf(p, channels) for p, _, _ in planes]
    v = ops.plane_regulation(leaves, [w for _, w, _ in planes], [w for _, _, w in planes])
    (v * 3.0).backward()
    torch.cuda.synchronize()
    return [t.detach().clone() for t in (l1, sums, g_l1, s, x.grad, v)] + [p.grad.detach().clone() for p in leaves]


@pytest.mark.parametrize("name,channels", [("field32+wide", 32), ("field16", 16)])
def test_the_switch_routes_the_values_and_leaves_the_gradients(name, channels, monkeypatch):
    from hip_helpers import RC
    monkeypatch.setattr(ops.PlaneRegFunction, "_cache", None)
    monkeypatch.setattr(ops.PlaneRegFunction, "_fwd_cache", None)
    assert RC.deterministic() is False
    off = _through_autograd(name, channels)
    RC.set_deterministic(True)
    try:
        one, two = _through_autograd(name, channels), _through_autograd(name, channels)
    finally:
        RC.set_deterministic(False)
    vo = RC._state["value_ordered"]
    assert vo is not None and all(vo[k] is not None for k in ("l1", "ssim", "reg"))
    for k, (a, b) in enumerate(zip(one, two)):
        assert torch.equal(a, b), k
    for k in (2, 4) + tuple(range(6, len(off))):                                             # the gradients never read the sums
        assert torch.equal(one[k], off[k]), k
    # the values are the twins': the L1 sums of the image pair, the regulariser of the planes
    img, gt = vc.ssim_images("g3")
    np.testing.assert_array_equal(vc.bits(one[1].cpu().numpy()), vc.bits(vc.l1_host(img.ravel(), gt.ravel())[0]))
    assert vc.bits(np.float32(one[5].item())) == vc.bits(np.float32(vc.reg_host(vc.reg_case(name))))
    for k in (0, 3, 5):
        assert abs(float(one[k]) - float(off[k])) <= 1e-4 * abs(float(off[k])), k


def _run(stage, model, iterations=6):
    """tests/test_field_ordered_gpu.py::_fine_run's recipe with the SSIM term on, keeping what a log shows of every iteration."""
    from hip_helpers import RC
    A, S, T, L = (importlib.import_module(f"{pkg}.{m}") for m in ("arguments", "scene", "train", "utils.loss_utils"))
    if model == 16:
        kc = {'grid_dimensions': 2, 'input_coordinate_dim': 4, 'output_coordinate_dim': 16, 'resolution': [64, 64, 64, 10]}
        args, lp, op, pp, hp = A.default_args(kplanes_config=kc, multires=[1, 2])
    else:
        args, lp, op, pp, hp = A.default_args(time_resolution=10)
    op.lambda_dssim = 0.2
    torch.manual_seed(6666)
    random.seed(6666)
    np.random.seed(6666)
    scene = S.SyntheticScene(1500, 3, 96, 64, seed=6666)
    g = S.GaussianModel(lp.sh_degree, hp, device=torch.device("cuda"))
    scene.init_gaussians(g)
    scene.make_trained_like(g)
    trainer = T.Trainer(scene, g, op, hp, pp, stage=stage, delta_scale=1, sync_every_step=True, fused=False, deterministic=True)
    log = []
    for it in range(1, iterations + 1):
        loss = trainer.step(it)
        last = trainer.last
        log.append([loss.reshape(1).float(), last["l1"].reshape(1), last["ssim"].reshape(1),
                    torch.zeros(1, device="cuda") if last["reg"] is None else last["reg"].reshape(1),
                    L.psnr_from_last_l1().reshape(1)])
        assert (last["reg"] is not None) == (stage == "fine")
    torch.cuda.synchronize()
    log = torch.cat([torch.cat(row) for row in log]).cpu().numpy().reshape(iterations, 5)
    state = []
    for group in g.optimizer.param_groups:
        for p in group["params"]:
            st = g.optimizer.state.get(p, {})
            state.append(p.detach().clone())
            state += [st[k].detach().clone() for k in ("exp_avg", "exp_avg_sq") if k in st]
    return log, state, (trainer.ema_loss, trainer.ema_psnr), RC.ordered_status()


@pytest.mark.parametrize("stage,model", [("coarse", 32), ("fine", 32), ("fine", 16)])
def test_a_training_run_logs_the_same_numbers_twice(stage, model):
    from hip_helpers import RC
    try:
        a, b = _run(stage, model), _run(stage, model)
    finally:
        RC.set_deterministic(False)
    assert a[3] == 0 and b[3] == 0
    assert np.isfinite(a[0]).all() and (a[0][:, 0] > 0).all() and (a[0][:, 4] > 0).all()
    np.testing.assert_array_equal(vc.bits(a[0].astype(np.float32)), vc.bits(b[0].astype(np.float32)))      # loss, L1, SSIM, regulariser, PSNR
    assert a[2] == b[2]                                                                       # both EMAs, as Python floats
    assert len(a[1]) == len(b[1]) >= 3 * 8
    for k, (x, y) in enumerate(zip(a[1], b[1])):
        assert torch.equal(x, y), k
