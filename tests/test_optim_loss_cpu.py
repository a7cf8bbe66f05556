"""Adam, L1 and the plane regulariser without a GPU: the float64 references of optim_loss_cases.py agree with oracle/torch_ref.py
evaluated in float64 on the case inputs; the wrappers and the C entry points refuse bad shapes, layouts and pointers before
anything touches a device; and the two stride memories (in_place_flags' memo, FusedAdam's per-gradient check) tell two views of
one buffer apart."""
import importlib

import numpy as np
import pytest
import torch

import optim_loss_cases as oc
from oracle import torch_ref as tr

pkg = "iclr2025_3d-mom_amd"
N = importlib.import_module(pkg + "._native")
ops = importlib.import_module(pkg + ".ops")
FAKE = 1 << 20          # a non-null pointer value; every call below is refused before it could be followed


# ------------------------------------------------------------------------------------------------ the references
def test_adam_f64_is_the_oracle_update_with_per_parameter_steps():
    c = oc.adam_case()
    want = oc.adam_case_f64()
    p = [t.double().clone() for t in c.params]
    m = [torch.zeros_like(t) for t in p]
    v = [torch.zeros_like(t) for t in p]
    step = [0] * len(p)
    for r, (grads, lrs) in enumerate(c.f64_rounds()):
        for i, g in enumerate(grads):
            if g is None:
                continue
            step[i] += 1
            tr.adam_reference([p[i]], [g.double()], [m[i]], [v[i]], step[i], lrs[i], c.betas[i][0], c.betas[i][1], c.eps[i])
        assert want[r]["step"] == step
        for i in range(len(p)):
            for got, ref in ((want[r]["p"][i], p[i]), (want[r]["m"][i], m[i]), (want[r]["v"][i], v[i])):
                # two float64 evaluations, differently ordered: a few 2^-53 of the tensor's scale (an element may cancel to near 0)
                scale = float(ref.abs().max()) if ref.numel() else 0.0
                np.testing.assert_allclose(got.numpy(), ref.numpy(), rtol=1e-12, atol=1e-14 * scale, err_msg=f"round {r} tensor {i}")
    # the case is what the GPU test says it is
    assert want[3]["step"] == [3 if i in oc.ADAM_NO_GRAD_ROUND4 else 4 for i in range(73)] and want[5]["step"][1] == 6
    for i in oc.ADAM_NO_GRAD_ROUND4:
        assert torch.equal(want[3]["p"][i], want[2]["p"][i]) and torch.equal(want[3]["m"][i], want[2]["m"][i])
    sizes = [t.numel() for t in c.params]
    assert {0, 1, 7, 2047, 2048, 2049, 4096, 6149} <= set(sizes) and sizes[2] and not sizes[3] and sizes[4]
    assert sum(1 for b in c.betas if b == oc.ADAM_CFG_A[0]) == 70 > 64 and c.params[8].stride() == ops.make_plane(*oc.ADAM_PLANE).stride()
    # ... and float32 torch.optim.Adam counts the same steps and is float32-close to it
    f32 = oc.adam_case_torch_f32()
    for r in range(6):
        assert f32[r]["step"] == want[r]["step"]
        for i in range(73):
            np.testing.assert_allclose(f32[r]["p"][i].numpy(), want[r]["p"][i].numpy(), rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("weights", ["ws", "wl", "both", "none", "mixed"])
def test_reg_f64_is_the_oracle_regulariser_in_float64(weights):
    for shapes in (tuple(oc.REG_SINGLE), tuple(oc.REG_MIXED)):
        case = oc.reg_case(shapes, weights)
        # float32-rounded weights on both sides (reg_f64 rounds them itself)
        ws, wl = [float(np.float32(a)) for a in case["ws"]], [float(np.float32(b)) for b in case["wl"]]
        val, grads = oc.reg_torch(case["planes"], ws, wl, torch.float64)
        np.testing.assert_allclose(case["value"], val, rtol=1e-12, atol=0)
        for i, (g, r) in enumerate(zip(case["grads"], grads)):
            np.testing.assert_allclose(g, r, rtol=1e-10, atol=1e-18, err_msg=str(shapes[i]))
        for t, g, b in zip(case["planes"], case["grads"], wl):
            if weights == "wl":
                assert (g[t == 1.0] == 0.0).all() and (g[t != 1.0] != 0.0).all()      # the L1 part is exactly 0 at a texel of 1
        if weights == "none":
            assert case["value"] == 0.0 and all(not g.any() for g in case["grads"])


def test_reg_f64_gradient_is_the_finite_difference_of_its_value():
    t = oc.reg_plane(32, 19, 2, seed=5)
    _, (g,) = oc.reg_f64([t], [0.3], [0.0])
    rng = np.random.default_rng(0)
    for _ in range(20):
        h, w, c = rng.integers(19), rng.integers(2), rng.integers(32)
        a, b = t.astype(np.float64), t.astype(np.float64)
        a[h, w, c] += 1e-4
        b[h, w, c] -= 1e-4
        fd = (oc.reg_f64([a], [0.3], [0.0])[0] - oc.reg_f64([b], [0.3], [0.0])[0]) / 2e-4      # the value is quadratic: exact
        assert abs(fd - g[h, w, c]) <= 1e-9 * max(1.0, abs(g[h, w, c]))


@pytest.mark.parametrize("n", sorted(oc.L1_SHAPES))
def test_l1_f64_is_the_oracle_loss_in_float64(n):
    case = oc.l1_case(n)
    assert case["img"].size == n
    a = torch.from_numpy(case["img"]).double().requires_grad_(True)
    loss, sums = tr.l1_loss_with_sums(a, torch.from_numpy(case["gt"]).double())
    loss.backward()
    np.testing.assert_allclose([case["s1"], case["s2"]], sums.numpy(), rtol=1e-12)
    g = a.grad.numpy()
    assert np.array_equal(np.sign(g), np.sign(case["grad"])) and int((case["grad"] == 0).sum()) >= case["zeros"]
    np.testing.assert_allclose(case["grad"], g, rtol=2.0 ** -23)             # float32(1/n) against 1/n
    assert case["grad"].dtype == np.float32 and oc.l1_chain(n) >= 12


def test_l1_chain_counts_what_the_kernel_does():
    assert oc.l1_chain(1) == 4 + 1 + 6 + 4 + 1
    assert oc.l1_chain(262144) == 4 + 1 + 6 + 4 + 256                          # the cap, one float4 per thread
    assert oc.l1_chain(270001) == 8 + 1 + 6 + 4 + 256                          # a second trip of the grid-stride loop


# ------------------------------------------------------------------------------------------------ refusals that need no device
def test_l1_refuses_images_of_different_sizes():
    for a, b in (((3, 8, 8), (3, 8, 7)), ((3, 8, 8), (1, 8, 8)), ((5,), (4,))):
        with pytest.raises(N.MomError, match="number of elements"):
            ops.l1_loss_with_sums(torch.zeros(a), torch.zeros(b))
        with pytest.raises(N.MomError, match="number of elements"):
            ops.l1_loss_with_sums(torch.zeros(b), torch.zeros(a))


def test_plane_regulation_refuses_a_plane_that_is_not_channel_last(monkeypatch):
    monkeypatch.setattr(ops.PlaneRegFunction, "_fwd_cache", None)
    good = ops.make_plane(32, 5, 4).zero_()
    for bad in (torch.zeros(1, 32, 5, 4), torch.zeros(32, 5, 4), torch.zeros(2, 32, 5, 4), good.double()):
        with pytest.raises(N.MomError, match="channel-last"):
            ops.plane_regulation([bad], [0.1], [0.1])
        with pytest.raises(N.MomError, match="channel-last"):
            ops.plane_regulation([good, bad], [0.1, 0.1], [0.1, 0.1])
    with pytest.raises(N.MomError, match="no CPU path"):                     # the layout is right: what is refused is the device
        ops.plane_regulation([good], [0.1], [0.1])
    assert ops.PlaneRegFunction._fwd_cache is None                           # a refused call leaves no descriptor behind


def _planes(*specs):
    arr = (N.MomRegPlane * max(len(specs), 1))()
    for i, (plane, grad, H, W) in enumerate(specs):
        arr[i].plane, arr[i].grad, arr[i].H, arr[i].W = plane, grad, H, W
        arr[i].w_smooth, arr[i].w_l1, arr[i].grad_scale = 0.1, 0.1, 1.0
    return arr


def test_every_invalid_regulariser_call_is_refused_before_anything_is_launched():
    lib = N.lib()
    good = (FAKE, FAKE, 19, 3)
    too_many = _planes(*([good] * (_max_planes() + 1)))
    assert lib.mom_plane_regulation_grad(too_many, _max_planes() + 1, FAKE, None, None) == N.MOM_EINVAL
    assert lib.mom_plane_regulation_grad(_planes(good), -1, FAKE, None, None) == N.MOM_EINVAL
    assert lib.mom_plane_regulation_grad(_planes(good), 1, None, None, None) == N.MOM_EINVAL            # nowhere to put the value
    assert lib.mom_plane_regulation_grad(None, 1, FAKE, None, None) == N.MOM_EINVAL
    for bad in ((FAKE, FAKE, 0, 3), (FAKE, FAKE, -1, 3), (FAKE, FAKE, 19, 0), (None, FAKE, 19, 3)):
        assert lib.mom_plane_regulation_grad(_planes(bad), 1, FAKE, None, None) == N.MOM_EINVAL, bad
        assert lib.mom_plane_regulation_grad(_planes(good, bad, good), 3, FAKE, None, None) == N.MOM_EINVAL, bad


def _max_planes():
    import os
    import re
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mom4d.h")).read()
    n = int(re.search(r"#define MOM_REG_MAX_PLANES (\d+)", header).group(1))
    assert n == len(oc.REG_MIXED)
    return n


def _adam(*specs):
    arr = (N.MomAdamTensor * max(len(specs), 1))()
    for i, (p, g, m, v, n) in enumerate(specs):
        arr[i].param, arr[i].grad, arr[i].exp_avg, arr[i].exp_avg_sq, arr[i].n = p, g, m, v, n
        arr[i].lr, arr[i].bias_correction1, arr[i].bias_correction2_sqrt = 1e-3, 0.1, 0.03
    return arr


def test_every_invalid_adam_call_is_refused_before_anything_is_launched():
    lib = N.lib()
    step = lambda arr, count: lib.mom_adam_step(arr, count, 0.9, 0.999, 1e-15, None, None)
    assert step(_adam(), -1) == N.MOM_EINVAL
    assert step(None, 1) == N.MOM_EINVAL
    for hole in range(4):                                          # param, grad, exp_avg, exp_avg_sq
        t = [FAKE] * 4
        t[hole] = None
        assert step(_adam((*t, 5)), 1) == N.MOM_EINVAL, hole
        assert step(_adam((None, None, None, None, 0), (*t, 2048)), 2) == N.MOM_EINVAL, hole
    # nothing to do is not an error: no tensors, or only empty ones (null pointers are what an empty tensor has)
    assert step(None, 0) == N.MOM_OK
    assert step(_adam((None, None, None, None, 0), (None, None, None, None, 0)), 2) == N.MOM_OK


# ------------------------------------------------------------------------------------------------ stride memories, host only
def test_in_place_flags_tells_two_layouts_at_one_address_apart(monkeypatch):
    monkeypatch.setattr(ops, "_IN_PLACE_MEMO", {})
    Cn, H, W = 32, 5, 4
    buf = torch.zeros(Cn * H * W)
    channel_last = buf.view(1, H, W, Cn).permute(0, 3, 1, 2)       # [1,C,H,W], texel rows of C floats
    contiguous = buf.view(1, Cn, H, W)
    grad = ops.make_plane(Cn, H, W).zero_()
    assert channel_last.data_ptr() == contiguous.data_ptr() and channel_last.shape == contiguous.shape
    assert ops.in_place_flags([grad], [channel_last]) == [True]
    assert ops.in_place_flags([grad], [contiguous]) == [False]     # same two pointers, same gradient: the plane's strides differ
    assert ops.in_place_flags([grad], [channel_last]) == [True]
    # ... and the gradient's own
    gbuf = torch.zeros(Cn * H * W)
    assert ops.in_place_flags([gbuf.view(1, H, W, Cn).permute(0, 3, 1, 2)], [channel_last]) == [True]
    assert ops.in_place_flags([gbuf.view(1, Cn, H, W)], [channel_last]) == [False]
    assert ops.in_place_flags([None, grad], [channel_last, channel_last]) == [False, True]
    # same strides, another shape at the same address
    other = buf.view(1, W, H, Cn).permute(0, 3, 1, 2)              # [1,C,W,H]
    assert ops.in_place_flags([grad], [other]) == [False]


def test_fused_adam_checks_a_gradient_whose_address_is_known_and_whose_strides_are_new(monkeypatch):
    """FusedAdam's host side with the launch stubbed out: a contiguous gradient at the address last step's channel-last gradient
    had is refused like any other gradient of the wrong layout, and the refused step counts nothing."""
    launches = []

    class Lib:
        @staticmethod
        def mom_adam_step(arr, count, b1, b2, eps, skip, stream):
            launches.append([(arr[i].param, arr[i].grad, arr[i].n) for i in range(count)])
            return N.MOM_OK
    monkeypatch.setattr(N, "lib", lambda: Lib)
    monkeypatch.setattr(N, "current_stream", lambda: None)
    monkeypatch.setattr(ops, "_need_cuda", lambda t, what: None)
    Cn, H, W = 32, 5, 4
    plane = torch.nn.Parameter(ops.make_plane(Cn, H, W).zero_())
    other = torch.nn.Parameter(torch.zeros(7))
    opt = ops.FusedAdam([plane, other], lr=1e-3)
    buf = torch.ones(Cn * H * W)
    plane.grad, other.grad = buf.view(1, H, W, Cn).permute(0, 3, 1, 2), torch.ones(7)
    opt.step()
    assert launches == [[(plane.data_ptr(), buf.data_ptr(), plane.numel()), (other.data_ptr(), other.grad.data_ptr(), 7)]]
    plane.grad = buf.view(1, Cn, H, W)                               # torch takes any strides
    assert plane.grad.data_ptr() == buf.data_ptr() and plane.grad.stride() != plane.stride()
    with pytest.raises(N.MomError, match="identical strides"):
        opt.step()
    assert len(launches) == 1 and float(opt.state[plane]["step"]) == 1.0 == float(opt.state[other]["step"])
    plane.grad = buf.view(1, H, W, Cn).permute(0, 3, 1, 2)           # the right layout again, same address: accepted
    opt.step()
    assert len(launches) == 2 and float(opt.state[plane]["step"]) == 2.0
    fresh = ops.FusedAdam([plane], lr=1e-3)                          # the plain refusal: wrong strides on the first step
    plane.grad = buf.view(1, Cn, H, W)
    with pytest.raises(N.MomError, match="identical strides"):
        fresh.step()
    assert len(launches) == 2
