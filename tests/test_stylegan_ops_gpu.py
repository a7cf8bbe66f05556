"""StyleGAN2's native ops on the GPU (csrc/stylegan_ops.hip through ops and stylegan_op) against the restatements of
stylegan_ops_cases.py, which test_stylegan_ops_cpu.py holds to the reference's own code.  Reads nothing outside the repository.

Bounds (derived, not tuned; eps = 2^-24, the unit roundoff of fp32):
  * upfirdn2d, per element: |got - want| <= (kh kw + 1) eps S, S the sum of the absolute values of the element's terms: recursive
    fp32 summation of kh kw rounded products, plus one rounding for the fp32 cast of the comparison side.  Values are compared,
    not bits; two calls must give the same bits.  Its gradients are upfirdn2d calls themselves and carry the same formula on the
    gradient's terms.
  * fused_bias_act: three fp32 roundings in the reference's order, so bit-equal to the numpy float32 restatement, NaNs at the same
    places.  grad_bias is torch's sum of n fp32 terms: within n eps sum|g| of the float64 sum.  Against float64 autograd (double
    backward) the three roundings and the cast give 4 eps |want|.
  * the composed block: both routes are within K eps A of the exact result to first order, so they differ by at most 2 K eps A; A is
    the block evaluated on the absolute values of every input, parameter and tap (the activation replaced by its Lipschitz bound,
    the gain), K the summed (terms + 1) of the ops on the path; a gradient passes through the chain twice: 2 K.

Achieved maxima as a share of the bound, MI355X (pytest -s prints them): upfirdn2d recorded calls 0.147, the six modes
across tiles 0.414, the general kernel 0.454, 70 000 planes 0.356; input gradients 0.213; grad_bias 0.116; the activation's second
order 0.382; the composed block 0.005."""
import importlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import stylegan_ops_cases as sc

pytestmark = pytest.mark.gpu
pkg = "iclr2025_3d-mom_amd"
N = importlib.import_module(pkg + "._native")
ops = importlib.import_module(pkg + ".ops")
so = importlib.import_module(pkg + ".stylegan_op")
up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
bits = lambda a: np.ascontiguousarray(a).view(np.uint32)
ALPHA, SCALE = 0.2, 2 ** 0.5


def check_upfirdn2d(x, k, u, d, pad, what):
    """x [M,H,W], k [kh,kw] numpy -> asserts the kernel's result within the bound, and that a second call gives the same bits."""
    want, S = sc.upfirdn2d(x, k, u, d, pad)
    M, H, W = x.shape
    n = 2 if M % 2 == 0 else 1                              # [N,C,H,W] with N C = M
    got = ops.upfirdn2d(up(x).reshape(n, M // n, H, W), up(k), u, d, pad)
    assert got.shape == (n, M // n, *want.shape[1:]) and got.dtype == torch.float32
    again = ops.upfirdn2d(up(x).reshape(n, M // n, H, W), up(k), u, d, pad)
    assert torch.equal(got, again)
    got = got.cpu().numpy().reshape(want.shape)
    bound = sc.bound(S, *k.shape)
    s = sc.share(got - want, bound)
    print(f"{what}: {x.shape} -> {want.shape}, |d| max {np.abs(got - want).max():.3g}, largest share of the bound {s:.3g}")
    assert np.isfinite(got).all() and (np.abs(got - want) <= bound).all()
    return s


# ------------------------------------------------------------------------------------------------------------------- upfirdn2d
RECORDED = sorted({tuple(r[1:11]) for r in sc.g21()["calls_upfirdn2d"].tolist()})


@pytest.mark.parametrize("shape", [(3, 9, 7), (4, 8, 8), (2, 17, 17)])
@pytest.mark.parametrize("call", RECORDED)
def test_upfirdn2d_recorded_generator_and_discriminator_calls(call, shape):
    kh, kw, ux, uy, dx, dy, px0, px1, py0, py1 = call
    check_upfirdn2d(sc.planes(shape, 1), sc.taps(kh, kw, 0) * (ux * uy), (ux, uy), (dx, dy), (px0, px1, py0, py1), f"recorded {call}")


def test_recorded_calls_are_instantiated_modes():
    assert len(RECORDED) >= 3
    for kh, kw, ux, uy, dx, dy, *_ in RECORDED:
        assert ux == uy and dx == dy and (ux, dx, kh, kw) in sc.MODES


# per mode: an input whose output spans more than one 64 x 16 tile in each axis and ends inside a tile, with the module's pads and
# with pads of mixed sign and parity (the other phase of an up-2 output, a cropped border)
MODE_CASES = {(1, 1, 4, 4): ((5, 33, 65), (2, 1, 2, 1)), (1, 1, 3, 3): ((5, 33, 65), (1, 1, 1, 1)),
              (2, 1, 4, 4): ((5, 17, 35), (2, 1, 2, 1)), (2, 1, 2, 2): ((5, 17, 35), (1, 0, 1, 0)),
              (1, 2, 4, 4): ((5, 67, 133), (1, 1, 1, 1)), (1, 2, 2, 2): ((5, 67, 133), (0, 0, 0, 0))}


@pytest.mark.parametrize("odd_pads", [False, True])
@pytest.mark.parametrize("mode", sc.MODES)
def test_upfirdn2d_every_mode_across_tiles(mode, odd_pads):
    u, d, kh, kw = mode
    shape, pad = MODE_CASES[mode]
    if odd_pads:
        pad = (pad[0] - 3, pad[1] + 4, pad[2] + 3, pad[3] - 2)
    oh, ow = sc.out_size(*shape[1:], kh, kw, (u, u), (d, d), pad)
    assert ow > sc.TILE_W and ow % sc.TILE_W and oh > sc.TILE_H and oh % sc.TILE_H
    check_upfirdn2d(sc.planes(shape, 2), sc.taps(kh, kw, 1), (u, u), (d, d), pad, f"mode {mode} pad {pad}")


GENERAL = [((1, 7, 9), (3, 2), (2, 1), (1, 3), (-1, 2, 3, -2)),         # unequal factors per axis, negative pads
           ((3, 5, 6), (1, 1), (2, 3), (1, 2), (1, 0, 0, 2)),           # a 1 x 1 kernel
           ((2, 3, 3), (7, 5), (1, 1), (1, 1), (4, 4, 5, 5)),           # a kernel larger than the input
           ((2, 20, 24), (32, 32), (1, 1), (1, 1), (16, 15, 16, 15)),   # 32 x 32; more than one workgroup per plane, a partial one
           ((2, 9, 9), (4, 4), (2, 2), (2, 2), (2, 1, 2, 1)),           # the modes' taps with factors no mode has
           ((2, 9, 9), (4, 4), (2, 1), (1, 1), (2, 1, 2, 1)),
           ((1, 6, 5), (5, 3), (3, 4), (1, 1), (0, 0, 0, 0))]           # up beyond a kernel side: phases without a tap


@pytest.mark.parametrize("case", GENERAL)
def test_upfirdn2d_general_path(case):
    shape, (kh, kw), u, d, pad = case
    check_upfirdn2d(sc.planes(shape, 3), sc.taps(kh, kw, 2), u, d, pad, f"general {case}")


@pytest.mark.parametrize("kernel,u,pad", [((4, 4), (1, 1), (2, 1, 2, 1)), ((3, 2), (2, 1), (1, 1, 1, 0))])
def test_upfirdn2d_more_planes_than_a_grid_axis(kernel, u, pad):
    check_upfirdn2d(sc.planes((70000, 4, 4), 4), sc.taps(*kernel, 3), u, (1, 1), pad, f"70 000 planes, kernel {kernel}")


# ------------------------------------------------------------------------------------------------------------------- bias + act
def same(got, want):
    got, want = np.asarray(got), np.asarray(want)
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and np.array_equal(bits(got)[~nan], bits(want)[~nan])


def check_bias_act(x, b, what):
    """Every case of the switch on x (numpy, any shape) with bias b (or None), bit-equal to the restatement."""
    ref = sc.special_values(x.size, 7).reshape(x.shape)
    xd, bd, rd = up(x), None if b is None else up(b), up(ref)
    for act, grad, r in ((3, 0, None), (3, 1, ref), (1, 0, None), (1, 1, None), (1, 1, ref), (1, 2, None), (3, 2, None), (3, 0, ref)):
        got = ops.fused_bias_act(xd, bd, None if r is None else rd, act, grad, ALPHA, SCALE)
        assert got.shape == xd.shape and got.dtype == torch.float32
        assert same(got.cpu().numpy(), sc.bias_act(x, b, r, act, grad, ALPHA, SCALE)), (what, act, grad)


@pytest.mark.parametrize("aligned", [True, False])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 513, sc.ACT_BLOCK + 1, 2 * sc.ACT_BLOCK + 3])
def test_bias_act_element_counts(n, aligned):
    """1-D inputs (the bias then has n elements); `aligned` False: the same values one float into a buffer, the scalar path."""
    x, b = sc.special_values(n + 1, n)[1:], sc.planes((n,), 5)
    if not aligned:
        xd = up(np.concatenate([[0.0], x]).astype(np.float32))[1:]
        assert xd.data_ptr() % 16 == 4 and xd.is_contiguous()
        got = ops.fused_bias_act(xd, up(b), None, 3, 0, ALPHA, SCALE)
        assert same(got.cpu().numpy(), sc.bias_act(x, b, None, 3, 0, ALPHA, SCALE))
        got = ops.fused_bias_act(xd, None, xd, 3, 1, ALPHA, SCALE)
        assert same(got.cpu().numpy(), sc.bias_act(x, None, x, 3, 1, ALPHA, SCALE))
        return
    check_bias_act(x, b, f"n {n}")
    check_bias_act(x, None, f"n {n}, no bias")


@pytest.mark.parametrize("shape", [(3, 5), (2, 3, 4), (2, 3, 5, 7), (2, 3, 2, 2, 3)])
def test_bias_act_input_shapes(shape):
    x = sc.special_values(int(np.prod(shape)), len(shape)).reshape(shape)
    assert np.isnan(x).any() and np.isinf(x).any() and (x == 0).any() and ((x != 0) & (np.abs(x) < 1e-38)).any()
    check_bias_act(x, sc.planes((shape[1],), 6), f"shape {shape}")
    check_bias_act(x, None, f"shape {shape}, no bias")


def test_bias_act_keeps_denormals():
    x = np.array([1e-45, -1e-45, 1.1754942e-38, -5e-42, 3e-39], np.float32)
    got = ops.fused_bias_act(up(x), None, None, 3, 0, ALPHA, 1.0).cpu().numpy()
    assert same(got, sc.bias_act(x, None, None, 3, 0, ALPHA, 1.0)) and (got != 0).sum() >= 4


# ------------------------------------------------------------------------------------------------------------------- autograd
AUTOGRAD = [((2, 2, 8, 8), (4, 4), (1, 1), (1, 1), (2, 1, 2, 1)), ((2, 2, 8, 8), (4, 4), (2, 2), (1, 1), (2, 1, 2, 1)),
            ((1, 3, 9, 7), (4, 4), (1, 1), (2, 2), (1, 1, 1, 1)), ((1, 3, 9, 7), (4, 4), (1, 1), (1, 1), (2, 2, 2, 2)),
            ((1, 1, 7, 9), (3, 2), (2, 1), (1, 3), (-1, 2, 3, -2)), ((1, 2, 5, 6), (2, 2), (3, 2), (2, 1), (0, 3, -2, 4))]


@pytest.mark.parametrize("case", AUTOGRAD)
def test_upfirdn2d_input_gradient(case):
    shape, (kh, kw), u, d, pad = case
    x, k = sc.planes(shape, 8), sc.taps(kh, kw, 4)
    oh, ow = sc.out_size(*shape[2:], kh, kw, u, d, pad)
    g = sc.planes((*shape[:2], oh, ow), 9)
    # float64 autograd through the torch restatement on the CPU
    x64 = torch.from_numpy(x).double().requires_grad_()
    sc.upfirdn2d_torch(x64, torch.from_numpy(k).double(), u, d, pad).backward(torch.from_numpy(g).double())
    want = x64.grad.numpy()
    # the gradient's own terms: upfirdn2d of g with the flipped kernel, up and down exchanged, the reference's pads
    gp = sc.grad_pad((kh, kw), shape[2:], (oh, ow), u, d, pad)
    again, S = sc.upfirdn2d(g.reshape(-1, oh, ow), k[::-1, ::-1], d, u, gp)
    assert again.shape[1:] == shape[2:] and np.abs(again.reshape(shape) - want).max() <= 2.0 ** -50 * (kh * kw + 1) * S.max()
    xd = up(x).requires_grad_()
    out = so.UpFirDn2d.apply(xd, up(k), u, d, pad)
    assert out.shape == (*shape[:2], oh, ow)
    out.backward(up(g))
    bound = sc.bound(S, kh, kw).reshape(shape)
    d_ = xd.grad.cpu().numpy() - want
    print(f"gradient {case}: |d| max {np.abs(d_).max():.3g}, largest share of the bound {sc.share(d_, bound):.3g}")
    assert (np.abs(d_) <= bound).all()
    if u[0] == u[1] and d[0] == d[1] and pad[:2] == pad[2:]:                # the reference's public signature
        x2 = up(x).requires_grad_()
        so.upfirdn2d(x2, up(k), up=u[0], down=d[0], pad=pad[:2]).backward(up(g))
        assert torch.equal(x2.grad, xd.grad)


@pytest.mark.parametrize("shape", [(3, 5), (2, 3, 4), (2, 3, 5, 7)])
def test_fused_leaky_relu_gradients(shape):
    x, b = sc.planes(shape, 10), sc.planes((shape[1],), 11)
    g = sc.planes(shape, 12)
    xd, bd = up(x).requires_grad_(), up(b).requires_grad_()
    out = so.fused_leaky_relu(xd, bd, ALPHA, SCALE)
    fwd = sc.bias_act(x, b, None, 3, 0, ALPHA, SCALE)
    assert same(out.detach().cpu().numpy(), fwd)
    out.backward(up(g))
    gin = sc.bias_act(g, None, fwd, 3, 1, ALPHA, SCALE)                     # the reference's formula: case 31 on the saved output
    assert same(xd.grad.cpu().numpy(), gin)
    axes = (0, *range(2, len(shape)))
    want = gin.astype(np.float64).sum(axes)
    n = gin.size // shape[1]
    bound = n * sc.EPS * np.abs(gin.astype(np.float64)).sum(axes)
    d_ = bd.grad.cpu().numpy() - want
    print(f"grad_bias {shape}: |d| max {np.abs(d_).max():.3g}, largest share of the bound {sc.share(d_, bound):.3g}")
    assert bd.grad.shape == (shape[1],) and (np.abs(d_) <= bound).all()
    # the module: the same call with its own parameter
    m = so.FusedLeakyReLU(shape[1]).cuda()
    with torch.no_grad():
        m.bias.copy_(up(b))
    assert torch.equal(m(up(x)), out.detach())


def test_upfirdn2d_double_backward():
    shape, kh, kw, u, d, pad = (1, 2, 5, 5), 4, 4, 2, 1, (2, 1)
    x, k = sc.planes(shape, 13), sc.taps(kh, kw, 0) * 4
    oh, ow = sc.out_size(5, 5, kh, kw, (u, u), (d, d), (*pad, *pad))
    v, w = sc.planes((1, 2, oh, ow), 14), sc.planes(shape, 15)

    def second(f, t):
        xx, vv = t(x).requires_grad_(), t(v).requires_grad_()
        gx, = torch.autograd.grad(f(xx, t(k)), xx, vv, create_graph=True)
        gv, = torch.autograd.grad(gx, vv, t(w))
        return gx.detach().cpu().numpy(), gv.cpu().numpy()
    gx64, gv64 = second(lambda a, kk: sc.upfirdn2d_torch(a, kk, (u, u), (d, d), (*pad, *pad)), lambda a: torch.from_numpy(a).double())
    gx, gv = second(lambda a, kk: so.upfirdn2d(a, kk, up=u, down=d, pad=pad), up)
    # the second order is the op itself applied to w; the first its adjoint applied to v
    fwd, S = sc.upfirdn2d(w.reshape(-1, 5, 5), k, (u, u), (d, d), (*pad, *pad))
    assert np.abs(fwd.reshape(gv64.shape) - gv64).max() <= 2.0 ** -50 * 17 * S.max()
    assert (np.abs(gv - gv64) <= sc.bound(S, kh, kw).reshape(gv.shape)).all()
    _, Sg = sc.upfirdn2d(v.reshape(-1, oh, ow), k[::-1, ::-1], (d, d), (u, u), sc.grad_pad((kh, kw), (5, 5), (oh, ow), (u, u), (d, d), (*pad, *pad)))
    assert (np.abs(gx - gx64) <= sc.bound(Sg, kh, kw).reshape(gx.shape)).all()


def test_fused_leaky_relu_double_backward():
    shape = (1, 2, 5, 5)
    x, b, v, w1, w2 = sc.planes(shape, 16), sc.planes((2,), 17), sc.planes(shape, 18), sc.planes(shape, 19), sc.planes((2,), 20)
    a32, s32 = float(np.float32(ALPHA)), float(np.float32(SCALE))          # the constants as the kernel receives them

    def second(f, t):
        xx, bb, vv = t(x).requires_grad_(), t(b).requires_grad_(), t(v).requires_grad_()
        gx, gb = torch.autograd.grad(f(xx, bb), (xx, bb), vv, create_graph=True)
        gv, = torch.autograd.grad((gx, gb), vv, (t(w1), t(w2)))
        return gv.cpu().numpy()
    want = second(lambda a, bb: F.leaky_relu(a + bb.view(1, -1, 1, 1), a32) * s32, lambda a: torch.from_numpy(a).double())
    got = second(lambda a, bb: so.fused_leaky_relu(a, bb, ALPHA, SCALE), up)
    d_ = got - want
    print(f"activation, second order: |d| max {np.abs(d_).max():.3g}, largest share of the bound {sc.share(d_, 4 * sc.EPS * np.abs(want)):.3g}")
    assert (np.abs(d_) <= 4 * sc.EPS * np.abs(want)).all()


# ------------------------------------------------------------------------------------------------------------------- composition
NAMES = ("x", "w", "nw", "b", "wrgb", "brgb", "skip")


def block(p, upfirdn, lrelu):
    """One up-sampling block of the generator, 8 -> 4 channels, 8 x 8 -> 16 x 16, with torch's own convolutions: transposed
    convolution, blur, noise, activation, a 1 x 1 to-RGB, plus the up-sampled skip image."""
    y = F.conv_transpose2d(p["x"], p["w"], stride=2)                       # [1,4,17,17]
    y = upfirdn(y, p["k"], 1, 1, (1, 1))                                   # [1,4,16,16]
    y = y + p["nw"] * p["noise"]
    y = lrelu(y, p["b"])
    rgb = F.conv2d(y, p["wrgb"]) + p["brgb"].view(1, 3, 1, 1)
    return rgb + upfirdn(p["skip"], p["k"], 2, 1, (2, 1))


def test_composed_upsampling_block_forward_and_backward():
    rng = np.random.default_rng(2199)
    val = {"x": (1, 8, 8, 8), "w": (8, 4, 3, 3), "nw": (1,), "b": (4,), "wrgb": (3, 4, 1, 1), "brgb": (3,), "skip": (1, 3, 8, 8),
           "noise": (1, 1, 16, 16), "G": (1, 3, 16, 16)}
    val = {n: rng.standard_normal(s).astype(np.float32) for n, s in val.items()}
    val["k"] = sc.taps(4, 4, 0) * 4
    ref_up = lambda a, k, u, d, pad: sc.upfirdn2d_torch(a, k, (u, u), (d, d), (*pad, *pad))

    def run(t, upfirdn, lrelu, absolute=False):
        p = {n: t(np.abs(a) if absolute else a) for n, a in val.items()}
        for n in NAMES:
            p[n].requires_grad_()
        image = block(p, upfirdn, lrelu)
        image.backward(p["G"])
        return [image.detach().cpu().numpy()] + [p[n].grad.cpu().numpy() for n in NAMES]
    ours = run(up, lambda a, k, u, d, pad: so.upfirdn2d(a, k, up=u, down=d, pad=pad), lambda a, b: so.fused_leaky_relu(a, b, ALPHA, SCALE))
    theirs = run(up, ref_up, lambda a, b: F.leaky_relu(a + b.view(1, -1, 1, 1), ALPHA) * SCALE)
    A = run(lambda a: torch.from_numpy(a).double(), ref_up, lambda a, b: (a + b.view(1, -1, 1, 1)) * SCALE, absolute=True)
    # (terms + 1) per op: transposed convolution 8 x 9, blur 16, noise 2, activation 3, to-RGB 4 + bias, up-sampling 16, the sum
    K = (72 + 1) + (16 + 1) + (2 + 1) + 3 + (5 + 1) + (16 + 1) + 1
    for name, o, t_, a, k_ in zip(("image",) + NAMES, ours, theirs, A, (K,) + (2 * K,) * len(NAMES)):
        bound = 2 * k_ * sc.EPS * a
        print(f"block {name}: |d| max {np.abs(o - t_).max():.3g}, largest share of the bound {sc.share(o - t_, bound):.3g}")
        assert o.shape == t_.shape == a.shape and np.isfinite(o).all() and (np.abs(o - t_) <= bound).all(), name
