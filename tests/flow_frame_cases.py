"""Inputs, float64 evaluations and derived bounds for the flow step around stage 1's estimator (csrc/flow_frame.hip, motion.py):
shared by tools/gen_stage1_golden.py, which runs the REFERENCE on these inputs and writes tests/golden/g22_*.npz, and by the tests.

The bounds (eps = 2^-24, the unit roundoff of fp32).  The kernels repeat the reference's fp32 operations in its order except in two
places: expf is another implementation, and the 15 x 15 box sum is formed in another order.

hint field.  Two expf of at most 1 ulp each differ by at most 2 ulp on the same fp32 argument: |dw_i| <= a_i = 2 max(2^-23 w_i, 2^-149).
With N_c = sum w_i m_ic and D = sum w_i (n hints), each of the n fp32 roundings of N and of D can fall differently on the two sides
(2 (eps |partial| + 2^-150) each), so |dN| <= sum a_i |m_ic| + 2 n (eps sum w_i |m_ic| + 2^-150), |dD| <= sum a_i + 2 n (eps D + 2^-150),
and for f = N / D:  |df| <= (|dN| + |f| |dD|) / (D - |dD|) + 2 eps |f| + 2^-149.
  * Where the largest weight is below 2^-152 every weight is 0 on both sides, the sum is replaced by 1 and f is exactly 0: bound 0.
  * Where D < 2^-110 the weights are subnormal or nearly so: the format itself quantises N and D to a few units of 2^-149, the
    reference's own value there is noise of the size of the motion (a rounded numerator over a rounded denominator is at most twice
    the largest |m_ic|), and the bound is 4 max_i |m_ic|, both values' largest magnitude added.
Behind f: the mask (exact), the scale (one rounding, 2 eps |v| between the sides) and the bilinear resize -- a convex combination,
so the bound is interpolated with the same weights, plus 12 eps of the interpolated magnitude for its four products and three sums
on either side, with or without contraction in the reference's build.

flow tail.  p = pred mask carries one rounding and the box mean 224 additions and one division: against exact arithmetic
227 eps boxmean(|p|) to first order, whatever the order of the sum.  Then the mask and the scale (3 eps |v|) and the resize as above.
That is one side's distance from exact arithmetic; two fp32 evaluations lie within twice it of each other.

Against the float64 evaluation the gate is the reference's own largest distance from it plus the bound.  The float64 evaluation
resizes with the fp32 source coordinates and weights torch's CPU kernels form (taps): they select pixels, so they are part of what
is evaluated."""
import os

import numpy as np

EPS = 2.0 ** -24
G22 = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g22_%s.npz")
H, W = 40, 56
SIZES = (24, 72)


def g22(name):
    return np.load(G22 % name)


def frame(mask, starts, ends):
    """A frame as render_pcd leaves it, as far as the flow step reads it: every hint coordinate is an array of shape (1,)."""
    from PIL import Image
    col = lambda pts, k: [np.array([float(p[k])]) for p in pts]
    return {"mask": Image.fromarray(mask), "final_hint_start_x": col(starts, 0), "final_hint_start_y": col(starts, 1),
            "final_hint_end_x": col(ends, 0), "final_hint_end_y": col(ends, 1)}


def disc(h, w, cx, cy, r, value=255):
    y, x = np.mgrid[0:h, 0:w]
    return (((x - cx) ** 2 + (y - cy) ** 2 <= r * r) * value).astype(np.uint8)


def hint_views():
    """(frames, sigmas) of the three 40 x 56 views of the hint-field test:
    0: one hint, on the border column x = 55, sigma = 1: beyond ten pixels every weight underflows and the weight sum is replaced;
    1: four hints listed, the second filtered (x < 0) so that the two behind it move with their predecessors' motion; of the three
       kept one lies outside the mask and one on the border pixel (0, 39);
    2: no hint in range (x < 0, y >= 512): the (0, 0) fallback with hint 0's motion."""
    m0 = disc(H, W, 44, 14, 13)
    m1 = disc(H, W, 20, 22, 15)
    m1[30:, :12] = 7                                  # any non-zero byte counts
    m2 = disc(H, W, 8, 8, 12)
    f0 = frame(m0, [(55.3, 12.8)], [(61.0, 30.1)])
    f1 = frame(m1, [(18.2, 20.9), (-3.0, 5.0), (50.7, 3.1), (0.4, 39.6)], [(40.2, 25.0), (-30.0, 60.0), (45.0, -20.5), (9.9, 20.0)])
    f2 = frame(m2, [(-2.0, 3.0), (5.0, 600.0)], [(14.0, -9.0), (0.0, 0.0)])
    return [f0, f1, f2], [1, 9, 14]


def selection_frames():
    """Frames of a 16 x 600 image for the host selection: a hint at x = 511 (kept) and one at x = 512 (dropped by the literal
    bound although the image is 600 wide); no hint in range; a filtered hint in the middle (the index quirk)."""
    m = np.zeros((16, 600), np.uint8)
    m[2:14, 5:590] = 255
    return [frame(m, [(511.2, 5.0), (512.0, 7.0)], [(530.0, 9.5), (400.0, 1.0)]),
            frame(m, [(520.0, 3.0), (-1.0, 2.0)], [(500.0, 8.0), (7.0, 7.0)]),
            frame(m, [(10.5, 3.2), (700.0, 4.0), (300.9, 12.4)], [(25.0, 9.0), (650.0, 14.0), (280.0, 2.0)])]


SELECTION_SIZE, SELECTION_SEED = 32, 22


# ---------------------------------------------------------------------------------------------------------------- resizes, in float64
def taps(n_in, n_out):
    """F.interpolate(bilinear, align_corners=False): (i0, i1, l0, l1) per output coordinate, as torch's CPU kernels form them in
    fp32 -- they are part of the operation's definition, not of its rounding error: the source coordinate is one fused
    multiply-add (the product of two fp32 numbers is exact in float64, so is its sum with -0.5, and one rounding follows), and where
    it is an integer in exact arithmetic the fp32 value can lie just below it and take the previous pixel with a weight of 1 - 2^-24."""
    scale = np.float32(n_in) / np.float32(n_out)
    src = (np.float64(scale) * (np.arange(n_out, dtype=np.float32) + np.float32(0.5)).astype(np.float64) - 0.5).astype(np.float32)
    src = np.maximum(src, np.float32(0))
    i0 = np.minimum(src.astype(np.int64), n_in - 1)
    i1 = i0 + (i0 < n_in - 1)
    l1 = src - i0.astype(np.float32)
    return i0, i1, (np.float32(1) - l1).astype(np.float64), l1.astype(np.float64)


def bilinear(x, oh, ow):
    """x [..., h, w] float64 -> [..., oh, ow]."""
    y0, y1, ly0, ly1 = taps(x.shape[-2], oh)
    x0, x1, lx0, lx1 = taps(x.shape[-1], ow)
    top = lx0 * x[..., y0, :][..., x0] + lx1 * x[..., y0, :][..., x1]
    bot = lx0 * x[..., y1, :][..., x0] + lx1 * x[..., y1, :][..., x1]
    return ly0[:, None] * top + ly1[:, None] * bot


def area(mask, S):
    """F.interpolate(mode='area') of mask != 0 as fp32 forms it: the count over the window, divided by its height, then its width."""
    h, w = mask.shape
    out = np.zeros((S, S), np.float32)
    for oy in range(S):
        y0, y1 = (oy * h) // S, -((-(oy + 1) * h) // S)
        for ox in range(S):
            x0, x1 = (ox * w) // S, -((-(ox + 1) * w) // S)
            out[oy, ox] = np.float32((mask[y0:y1, x0:x1] != 0).sum()) / np.float32(y1 - y0) / np.float32(x1 - x0)
    return out


# ---------------------------------------------------------------------------------------------------------------- the hint field
def hint_eval(pos, start, end, sigma, mask, S):
    """(hints [2,S,S] float64, bound [2,S,S]) of one view: the reference's formula (demo.py:77-102) in float64, and the derived bound
    on the distance between two fp32 evaluations that differ in expf alone (the module's docstring)."""
    h, w = mask.shape
    m = (np.asarray(end, np.float64) - np.asarray(start, np.float64)) / 50.0                      # [n,2]
    n = len(m)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    a = -np.stack([((x - px) ** 2 + (y - py) ** 2) for px, py in np.asarray(pos, np.float64)]) / float(sigma) ** 2
    wgt = np.exp(a)                                                                               # [n,h,w]
    D = wgt.sum(0)
    absm = np.abs(m)
    N = np.einsum("nhw,nc->chw", wgt, m)
    Nabs = np.einsum("nhw,nc->chw", wgt, absm)
    with np.errstate(divide="ignore", invalid="ignore"):
        f = np.where(D > 0, N / np.where(D > 0, D, 1.0), 0.0)
    ai = 2.0 * 1.001 * np.maximum(2.0 ** -23 * wgt, 2.0 ** -149)
    dN = np.einsum("nhw,nc->chw", ai, absm) + 2 * n * (EPS * Nabs + 2.0 ** -150)
    dD = ai.sum(0) + 2 * n * (EPS * D + 2.0 ** -150)
    ok = D >= 2.0 ** -110
    with np.errstate(divide="ignore", invalid="ignore"):
        normal = (dN + np.abs(f) * dD) / np.where(ok, D - dD, 1.0) + 2 * EPS * np.abs(f) + 2.0 ** -149
    B = np.where(ok, normal, 4.0 * absm.max(0)[:, None, None])
    B = np.where(a.max(0) < np.log(2.0 ** -152), 0.0, B)
    keep = (mask != 0).astype(np.float64)
    sc = np.array([np.float32(S / w), np.float32(S / h)], np.float64)[:, None, None]
    field = f * keep * sc
    Bs = (B * sc * (1 + EPS) + 2 * EPS * np.abs(field)) * keep
    return bilinear(field, S, S), bilinear(Bs, S, S) + 12 * EPS * bilinear(np.abs(field), S, S)


def hint_restated(pos, start, end, sigma, mask, S):
    """The reference's statements (demo.py:73-103) on torch's CPU, from the selected hints on: (hints [1,2,S,S], mask_s [1,1,S,S])."""
    import torch
    import torch.nn.functional as F
    h, w = mask.shape
    hint_x, hint_y = torch.tensor([int(p[0]) for p in pos]).long(), torch.tensor([int(p[1]) for p in pos]).long()
    hint_motion = torch.tensor((np.asarray(end, np.float64) - np.asarray(start, np.float64)) / 50.).permute(1, 0)[None]
    xs = torch.linspace(0, w - 1, w).view(1, 1, w).repeat(1, h, 1)
    ys = torch.linspace(0, h - 1, h).view(1, h, 1).repeat(1, 1, w)
    xys = torch.cat((xs, ys), 1).view(2, -1)
    dense, norm = torch.zeros(1, 2, h * w), torch.zeros(1, 2, h * w)
    for i in range(hint_motion.shape[-1]):
        dist = ((xys - xys.view(2, h, w)[:, hint_y[i], hint_x[i]].unsqueeze(1)) ** 2).sum(0, True).sqrt()
        weight = (-(dist / sigma) ** 2).exp().unsqueeze(0)
        dense += weight * hint_motion[:, :, i].unsqueeze(2)
        norm += weight
    norm[norm == 0.0] = 1.0
    dense = (dense / norm).view(1, 2, h, w) * torch.tensor(mask).bool()
    dense = dense * torch.FloatTensor([S / w, S / h]).view(1, 2, 1, 1)
    return (F.interpolate(dense, (S, S), mode="bilinear", align_corners=False),
            F.interpolate(torch.tensor(mask[None, None]).bool().float(), (S, S), mode="area"))


# ---------------------------------------------------------------------------------------------------------------- the flow tail
FINISH_SIZES = (24, 72, 9)


def finish_inputs(S):
    """(pred [2,2,S,S], mask_s [2,1,S,S]) float32: two views with fractional masks (the area resize of two discs).  At S = 9, where
    the 15-wide window is wider than the image, view 0 is all ones under a pred that is zero except at (0, 0): row 8 and column 8,
    whose windows start at 1, do not see it and must be exactly zero."""
    rng = np.random.default_rng(2200 + S)
    pred = rng.standard_normal((2, 2, S, S)).astype(np.float32)
    mask_s = np.stack([area(disc(H, W, 30, 18, 16), S), area(disc(H, W, 12, 25, 11), S)])[:, None]
    if S == 9:
        mask_s[0] = 1.0
        keep = np.zeros((S, S), np.float32)
        keep[0, 0] = 1.0
        pred[0] *= keep
    return pred, mask_s


def box_mean_direct(x):
    """The 15 x 15 box mean with a zero border of x [..., S, S] in float64, by 225 shifted additions: no cancellation, so zeros stay
    zeros."""
    S = x.shape[-1]
    p = np.zeros(x.shape[:-2] + (S + 14, S + 14))
    p[..., 7:7 + S, 7:7 + S] = x
    out = np.zeros_like(x, dtype=np.float64)
    for dy in range(15):
        for dx in range(15):
            out += p[..., dy:dy + S, dx:dx + S]
    return out / 225.0


def finish_eval(pred, mask_s, h, w):
    """(flow [V,2,h,w] float64, bound) of renderer.py:598-606 in float64; the bound is one fp32 evaluation's distance from it (the
    module's docstring)."""
    S = pred.shape[-1]
    pm = pred.astype(np.float64) * mask_s.astype(np.float64)
    sc = np.array([np.float32(w / S), np.float32(h / S)], np.float64)[None, :, None, None]
    v = box_mean_direct(pm) * mask_s * sc
    Bv = 227 * EPS * box_mean_direct(np.abs(pm)) * mask_s * sc + 3 * EPS * np.abs(v)
    return bilinear(v, h, w), bilinear(Bv, h, w) + 12 * EPS * bilinear(np.abs(v), h, w)


def finish_restated(pred, mask_s, h, w):
    """renderer.py:598-606 with kornia's box_blur(flow, (15, 15), border_type='constant') restated as zero padding of 7 and
    avg_pool2d(15, stride=1); one blur, as the reference's loop keeps one.  torch tensors in, on any device."""
    import torch
    import torch.nn.functional as F
    flow = pred * mask_s
    flow_ = F.avg_pool2d(F.pad(flow, (7, 7, 7, 7)), 15, stride=1)
    flow = flow_ * mask_s
    scale = [w / flow.shape[3], h / flow.shape[2]]
    flow = flow * torch.FloatTensor(scale).to(flow.device).view(1, 2, 1, 1)
    return F.interpolate(flow, (h, w), mode="bilinear", align_corners=False)
