"""Restatements and case tables of the two ops of csrc/stylegan_ops.hip (include/mom4d.h has the definitions).

  * `upfirdn2d` is the definition of include/mom4d.h in float64 numpy: the zero-inserted, padded / cropped map U is built in memory
    and the kh x kw taps are summed over strided views of it.  It also returns S, the same sum over the absolute values of the
    terms: what the bound on an fp32 sum of kh kw rounded products is made of (`bound`).
  * `upfirdn2d_torch` is the same definition in torch ops of any dtype and device (zero insertion, F.pad of either sign, conv2d with
    the flipped kernel, stride slice), differentiable: what autograd through the restatement means in the GPU tests, and the op
    sequence a user without the kernel would write.
  * `bias_act` is fused_bias_act_kernel.cu's switch in numpy float32, three roundings in its order, on the flat index: the bias of
    element i is b[(i // step_b) % size_b].
tests/golden/g21_stylegan_ops.npz (tools/gen_stylegan_ops_golden.py) holds the outputs of the REFERENCE's upfirdn2d_native for
NATIVE_CASES and the argument tuples its Generator and Discriminator call the two ops with.
"""
import functools
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
G21 = os.path.join(HERE, "golden", "g21_stylegan_ops.npz")
EPS = 2.0 ** -24

# the six instantiated modes of the tile kernel: (up, down, kh, kw)
MODES = [(1, 1, 4, 4), (1, 1, 3, 3), (2, 1, 4, 4), (2, 1, 2, 2), (1, 2, 4, 4), (1, 2, 2, 2)]
TILE_W, TILE_H = 64, 16                 # the tile kernel's outputs per workgroup
ACT_BLOCK = 256 * 4 * 4                 # elements one workgroup of the activation kernel covers in its whole loop

# what the reference's upfirdn2d_native was run on for g21: ((M, H, W), (kh, kw), (ux, uy), (dx, dy), (px0, px1, py0, py1))
NATIVE_CASES = [
    ((3, 9, 7), (4, 4), (1, 1), (1, 1), (2, 1, 2, 1)),            # Blur
    ((2, 8, 8), (4, 4), (2, 2), (1, 1), (2, 1, 2, 1)),            # Upsample
    ((2, 17, 17), (4, 4), (1, 1), (2, 2), (1, 1, 1, 1)),          # Downsample
    ((1, 7, 9), (3, 2), (2, 1), (1, 3), (-1, 2, 3, -2)),          # unequal factors per axis, negative pads
    ((2, 6, 5), (3, 3), (1, 1), (1, 1), (-1, -1, 0, 2)),          # cropping on both sides of x
    ((1, 5, 6), (2, 2), (3, 2), (2, 1), (0, 3, -2, 4)),           # up 3 x 2, down 2 x 1
]


def g21():
    return _g21()


@functools.lru_cache(maxsize=None)
def _g21():
    with np.load(G21) as z:
        return {k: z[k] for k in z.files}


def planes(shape, seed):
    return np.random.default_rng(2100 + seed).standard_normal(shape).astype(np.float32)


def taps(kh, kw, seed):
    """A random fp32 kernel; 4 x 4 with seed 0 is the generator's blur, make_kernel([1, 3, 3, 1])."""
    if (kh, kw, seed) == (4, 4, 0):
        k = np.outer([1, 3, 3, 1], [1, 3, 3, 1]).astype(np.float32)
        return k / k.sum()
    return np.random.default_rng(2150 + 100 * kh + kw + 7 * seed).standard_normal((kh, kw)).astype(np.float32)


def out_size(H, W, kh, kw, up, down, pad):
    (ux, uy), (dx, dy), (px0, px1, py0, py1) = up, down, pad
    return (H * uy + py0 + py1 - kh) // dy + 1, (W * ux + px0 + px1 - kw) // dx + 1


def grad_pad(kernel_shape, in_hw, out_hw, up, down, pad):
    """op/upfirdn2d.py:108-111, restated."""
    (kh, kw), (H, W), (oh, ow), (ux, uy), (dx, dy), (px0, px1, py0, py1) = kernel_shape, in_hw, out_hw, up, down, pad
    return kw - px0 - 1, W * ux - ow * dx + px0 - ux + 1, kh - py0 - 1, H * uy - oh * dy + py0 - uy + 1


def upfirdn2d(x, k, up=(1, 1), down=(1, 1), pad=(0, 0, 0, 0)):
    """x [M,H,W], k [kh,kw] -> (out [M,out_h,out_w], S) in float64; S is the sum of the absolute values of out's terms."""
    x, k = np.asarray(x, np.float64), np.asarray(k, np.float64)
    (ux, uy), (dx, dy), (px0, px1, py0, py1) = up, down, pad
    M, H, W = x.shape
    kh, kw = k.shape
    oh, ow = out_size(H, W, kh, kw, up, down, pad)
    assert oh >= 1 and ow >= 1
    TH, TW = H * uy + py0 + py1, W * ux + px0 + px1
    U = np.zeros((M, TH, TW))
    ys, xs = np.arange(H) * uy + py0, np.arange(W) * ux + px0          # where x[iy][ix] lands in the padded map
    yk, xk = (ys >= 0) & (ys < TH), (xs >= 0) & (xs < TW)
    U[:, ys[yk][:, None], xs[xk][None, :]] = x[:, yk][:, :, xk]
    out, S = np.zeros((M, oh, ow)), np.zeros((M, oh, ow))
    for a in range(kh):
        for b in range(kw):
            term = k[kh - 1 - a, kw - 1 - b] * U[:, a:a + (oh - 1) * dy + 1:dy, b:b + (ow - 1) * dx + 1:dx]
            out += term
            S += np.abs(term)
    return out, S


def bound(S, kh, kw):
    """|fp32 result - float64 result| <= (kh kw + 1) eps S: recursive fp32 summation of kh kw rounded products, plus one rounding
    for the fp32 cast of the comparison side."""
    return (kh * kw + 1) * EPS * S


def share(d, bnd):
    """Largest |d| / bound; a nonzero difference where the bound is zero is infinite."""
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(d == 0, 0.0, np.abs(d) / bnd)
    return float(q.max())


def upfirdn2d_torch(x, k, up=(1, 1), down=(1, 1), pad=(0, 0, 0, 0)):
    """x [N,C,H,W], k [kh,kw] torch tensors of one dtype and device -> [N,C,out_h,out_w]; differentiable."""
    import torch
    import torch.nn.functional as F
    (ux, uy), (dx, dy), (px0, px1, py0, py1) = up, down, pad
    n, c, H, W = x.shape
    kh, kw = k.shape
    u = x.new_zeros(n * c, 1, H * uy, W * ux)
    u[:, :, ::uy, ::ux] = x.reshape(n * c, 1, H, W)
    u = F.pad(u, [px0, px1, py0, py1])                                  # a negative pad crops
    out = F.conv2d(u, torch.flip(k, [0, 1]).reshape(1, 1, kh, kw))[:, :, ::dy, ::dx]
    return out.reshape(n, c, out.shape[2], out.shape[3])


def bias_act(x, b, ref, act, grad, alpha, scale, step_b=None):
    """The reference's switch in float32.  x of any shape; b [size_b] or None; ref like x or None.  step_b defaults to the product
    of the sizes from dimension 2 on."""
    x = np.asarray(x, np.float32)
    flat = x.reshape(-1).copy()
    alpha, scale = np.float32(alpha), np.float32(scale)
    with np.errstate(all="ignore"):
        if b is not None:
            b = np.asarray(b, np.float32)
            step_b = int(np.prod(x.shape[2:], dtype=np.int64)) if step_b is None else step_b
            flat = flat + b[(np.arange(flat.size) // step_b) % b.size]
        r = np.zeros_like(flat) if ref is None else np.asarray(ref, np.float32).reshape(-1)
        mode = act * 10 + grad
        if mode in (10, 11):
            y = flat
        elif mode in (12, 32):
            y = np.zeros_like(flat)
        elif mode == 30:
            y = np.where(flat > 0, flat, flat * alpha)
        elif mode == 31:
            y = np.where(r > 0, flat, flat * alpha)
        else:
            raise ValueError(mode)
        return (y * scale).astype(np.float32).reshape(x.shape)


def special_values(n, seed):
    """n fp32 values: normals, with +-0, +-inf, NaN and denormals (the smallest, the largest, a middle one) at seeded places."""
    rng = np.random.default_rng(2190 + seed)
    v = rng.standard_normal(n).astype(np.float32)
    special = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1e-45, -1e-45, 1.1754942e-38, -5e-42], np.float32)
    at = rng.permutation(n)[:min(n, len(special))]
    v[at] = special[:len(at)]
    return v
