"""Closed-form inputs and a numpy restatement of the four ops of csrc/eulerian_warp.hip (include/mom4d.h has the arithmetic).

The restatement follows the reference's video generator operation by operation (thirdparty/StyleCineGAN/utils/cinemagraph_utils.py,
joint_splatting.py, softmax_splatting.py):
  * `euler` is euler_integration in fp32: integers and fp32 adds only, so it has the reference's bits;
  * `splat` is the summation splat: the coordinates, the four weights and the products input * weight are formed in fp32 as the
    kernel (and the reference's CUDA string) forms them, and ACCUMULATED in float64, so it carries no summation error of its own.
    It also returns, per target pixel, the number of contributions k and the splat of |input|: what the bound on an fp32 sum in
    any order is made of.
tools/gen_eulerian_warp_golden.py hands `splat_for_reference` to the reference's own code in place of its cupy kernel.
"""
import functools
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
G20 = os.path.join(HERE, "golden", "g20_eulerian_warp.npz")
EPS = 2.0 ** -24

# (S, C, n_frames) of the two families the fixture holds, and the frames checked in each: first, second, middle, last
GOLDEN = {32: (32, 3, 6, (0, 1, 3, 5)), 256: (256, 2, 8, (0, 1, 4, 7))}
STRIDE = {32: 1, 256: 8}              # g20 keeps every STRIDE-th row and column of the S = 256 float maps (1 MiB per committed file)


def features(C, S, seed=20):
    return np.random.default_rng(seed + 1000 * C + S).standard_normal((C, S, S)).astype(np.float32)


def flow(H, W=None, amp=1.0):
    """[2,H,W] float32: two sinusoids per component whose chains fold, diverge and leave the image; zero in a block on the left."""
    W = H if W is None else W
    y, x = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    L = max(min(H, W) / 4.0, 6.0)
    u = 2.6 * np.sin(2 * np.pi * y / L + 0.3) + 1.7 * np.sin(2 * np.pi * x / (0.7 * L) + 1.1) + 0.9 * (x - W / 2) / (W / 8)
    v = 2.2 * np.cos(2 * np.pi * x / L + 0.7) + 1.3 * np.sin(2 * np.pi * (x + y) / (0.9 * L)) + 0.9 * (y - H / 2) / (H / 8)
    f = amp * np.stack([u, v])
    f[:, H // 3:H // 3 + max(H // 5, 2), W // 8:W // 8 + max(W // 4, 2)] = 0.0        # the region of zero flow
    return f.astype(np.float32)


def geometry(S):
    """(cut, pad, padded, crop0) of blend_feature / crop_padded_tensor."""
    cut = {1024: 3, 512: 2, 256: 1}.get(S, 0)
    s = S - 2 * cut
    pad = int(s / 4) + int(s / 8)
    P = s + 2 * pad
    return cut, pad, P, int((P - S) / 2)


def euler(motion, steps, all_frames=False):
    """euler_integration (cinemagraph_utils.py:9-59) in fp32.  motion [2,H,W] -> [2,H,W] or [steps+1,2,H,W]."""
    motion = np.asarray(motion, np.float32)
    _, H, W = motion.shape
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    coord = np.stack([xx, yy]).astype(np.float32)
    dest = coord.copy()
    invalid = np.zeros((H, W), bool)
    out = np.zeros((steps + 1, 2, H, W), np.float32)
    for s in range(1, steps + 1):
        iy, ix = np.rint(dest[1]).astype(np.int64), np.rint(dest[0]).astype(np.int64)       # np.rint: half to even, torch.round's
        dest = (dest + motion[:, iy, ix]).astype(np.float32)
        invalid |= (dest[0] > W - 1) | (dest[0] < 0) | (dest[1] > H - 1) | (dest[1] < 0)
        dest[:, invalid] = coord[:, invalid]
        out[s] = dest - coord
    return out if all_frames else out[steps]


def splat(inp, flw):
    """The summation splat (softmax_splatting.py:8-53).  inp [N,C,H,W], flw [N,2,H,W], float32.
    Returns (out float64 [N,C,H,W], k int [N,H,W], out_abs float64 [N,C,H,W])."""
    inp, flw = np.asarray(inp, np.float32), np.asarray(flw, np.float32)
    N, C, H, W = inp.shape
    out = np.zeros((N, C, H * W))
    out_abs = np.zeros((N, C, H * W))
    k = np.zeros((N, H * W), np.int64)
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    for n in range(N):
        ox = (xx.astype(np.float32) + flw[n, 0]).astype(np.float32)
        oy = (yy.astype(np.float32) + flw[n, 1]).astype(np.float32)
        nwx, nwy = np.floor(ox).astype(np.int64), np.floor(oy).astype(np.int64)
        f = lambda a: a.astype(np.float32)
        wx1, wx0 = f(f(nwx + 1) - ox), f(ox - f(nwx))              # (float)(southeast x) - x,  x - (float)(northwest x)
        wy1, wy0 = f(f(nwy + 1) - oy), f(oy - f(nwy))
        for dx, dy, w in ((0, 0, f(wx1 * wy1)), (1, 0, f(wx0 * wy1)), (0, 1, f(wx1 * wy0)), (1, 1, f(wx0 * wy0))):
            tx, ty = nwx + dx, nwy + dy
            ok = (tx >= 0) & (tx < W) & (ty >= 0) & (ty < H)
            at = (ty * W + tx)[ok]
            k[n] += np.bincount(at, minlength=H * W)
            for c in range(C):
                prod = f(inp[n, c] * w)[ok].astype(np.float64)     # the fp32 product the kernel adds; bincount sums in float64
                out[n, c] += np.bincount(at, weights=prod, minlength=H * W)
                out_abs[n, c] += np.bincount(at, weights=np.abs(prod), minlength=H * W)
    return out.reshape(N, C, H, W), k.reshape(N, H, W), out_abs.reshape(N, C, H, W)


def splat_for_reference(inp, flw):
    """What tools/gen_eulerian_warp_golden.py puts in place of _FunctionSoftsplat.apply: the float64 sums alone."""
    return splat(inp, flw)[0]


def blend(feature, motion, idx, n_frames):
    """blend_feature (cinemagraph_utils.py:131-178) with joint_splatting's double canvas (joint_splatting.py:23-42).
    feature [C,S,S], motion [2,S,S] float32.  Returns a dict: future, past (the two displacement maps [2,P,P], fp32), num [C,P,P]
    and den [P,P] (float64 sums), k [P,P], num_abs [C,P,P], blended [C,P,P] (num / den, den 0 -> 1), blank [P,P]."""
    feature, motion = np.asarray(feature, np.float32), np.asarray(motion, np.float32)
    C, S, _ = feature.shape
    cut, pad, P, _ = geometry(S)
    if cut:
        feature, motion = feature[:, cut:-cut, cut:-cut], motion[:, cut:-cut, cut:-cut]
    padw = ((0, 0), (pad, pad), (pad, pad))
    fpad, mpad = np.pad(feature, padw, mode="reflect"), np.pad(motion, padw, mode="reflect")
    future, past = euler(mpad, idx), euler(-mpad, n_frames - idx - 1)
    alpha = idx / (n_frames - 1)
    z1, z2 = np.float32(1 - alpha), np.float32(alpha)
    past_off = past.copy()
    past_off[0] = (past_off[0] - np.float32(P)).astype(np.float32)                    # flow2_offset[:, 0] -= W
    inp = np.concatenate([np.concatenate([fpad * z1, np.full((1, P, P), z1, np.float32)]),
                          np.concatenate([fpad * z2, np.full((1, P, P), z2, np.float32)])], axis=-1)
    out, k, out_abs = splat(inp[None], np.concatenate([future, past_off], axis=-1)[None])
    out, k, out_abs = out[0, :, :, :P], k[0, :, :P], out_abs[0, :, :, :P]              # output_size
    num, den = out[:C], out[C]
    blank = den == 0
    div = np.where(blank, 1.0, den)
    return dict(future=future, past=past, num=num, den=den, k=k, num_abs=out_abs[:C], blended=num / div,
                blended_abs=out_abs[:C] / div, blank=blank, P=P)


def box_mean(a):
    """The 7 x 7 box mean with zero padding, 49 products with (float)(1/49), summed in float64.  a [C,P,P]."""
    w = np.float64(np.float32(1.0) / np.float32(49.0))
    C, P, _ = a.shape
    ap = np.pad(a, ((0, 0), (3, 3), (3, 3)))
    out = np.zeros_like(a)
    for dy in range(7):
        for dx in range(7):
            out += ap[:, dy:dy + P, dx:dx + P] * w
    return out


def finish(b, S):
    """feature_inpaint_conv and crop_padded_tensor on blend()'s result.  Returns (final [C,S,S] float64, blank [S,S], bound_abs
    [C,S,S]): bound_abs is blend(|feature|) outside the blank pixels and its box mean at them."""
    _, _, P, c0 = geometry(S)
    filled = np.where(b["blank"][None], box_mean(b["blended"]), b["blended"])
    mag = np.where(b["blank"][None], box_mean(b["blended_abs"]), b["blended_abs"])
    crop = (slice(None), slice(c0, c0 + S), slice(c0, c0 + S))
    return filled[crop], b["blank"][crop[1:]], mag[crop]


@functools.lru_cache(maxsize=None)
def case(S, C, n_frames, idx):
    """One blend case, computed once per process and shared (the arrays are not to be written to)."""
    f, m = features(C, S), flow(S)
    b = blend(f, m, idx, n_frames)
    final, blank_crop, mag = finish(b, S)
    b.update(feature=f, motion=m, final=final, blank_crop=blank_crop, final_abs=mag)
    for v in b.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return b


def bound_blend(b):
    """|got - want| allowed on the blended map outside the blank pixels: numerator and denominator each carry the recursive-summation
    bound of k fp32 terms in any order plus the roundings of the two products ((k + 4) eps each), then the division."""
    return (2 * int(b["k"].max()) + 8) * EPS * b["blended_abs"]


def bound_final(b):
    """The same on the cropped result; at the blank pixels 50 more terms (49 products and their sum), on the box mean of |.|."""
    kmax = int(b["k"].max())
    return np.where(b["blank_crop"][None], (2 * kmax + 8 + 50), (2 * kmax + 8)) * EPS * b["final_abs"]


@functools.lru_cache(maxsize=None)
def g20():
    z = np.load(G20)
    return {k: z[k] for k in z.files}
