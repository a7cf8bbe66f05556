"""Yardstick and inputs of the flow-sampling tests (test_flow_sample_cpu.py, test_flow_sample_gpu.py).

`restate` is the arithmetic include/mom4d.h writes out for mom_flow_sample, in float64 numpy, operation by operation in the same
order: linear interpolation inside one of the two triangles of the pixel's cell, the cell's diagonal read from a mask.  With the mask
of scipy's own triangulation (fixture g17, written by tools/gen_grid_diagonals.py) it IS scipy.interpolate.griddata(method="linear")
over the pixel grid to float64 rounding -- test_flow_sample_cpu.py holds it to that -- so the GPU tests need no scipy.

Cases are built on sceneflow_cases (cloud, poses, intrinsics, g15) and computed once (functools.lru_cache); callers do not modify them."""
import functools
import importlib
import os

import numpy as np

import sceneflow_cases as sc

G17 = os.path.join(sc.ROOT, "tests", "golden", "g17_grid_diagonals.npz")
SIZES = [(2, 2), (5, 7), (24, 24), (37, 53)]                      # (H, W)
SHAPES = [(1, 6), (63, 6), (65, 6), (257, 6), (300, 6), (65, 1), (65, 33), (65, 70)]      # (P, V): the fit's


def restate(image, pix, mask, corners=False):
    """image [2,H,W] (a frame's flow image without its leading 1), pix [n,2] float64 pixels (u, v), mask bool [H-1,W-1], True where
    the anti-diagonal splits the cell.  Returns gt [n,2] float64; with corners=True also [n,2], the largest magnitude among the
    four corner values each result interpolates."""
    f = np.asarray(image, dtype=np.float64)
    _, H, W = f.shape
    pix = np.asarray(pix, dtype=np.float64)
    u, v = pix[:, 0], pix[:, 1]
    x0 = np.clip(np.floor(u).astype(np.int64), 0, W - 2)
    y0 = np.clip(np.floor(v).astype(np.int64), 0, H - 2)
    fx, fy = u - x0, v - y0
    f00, f10, f01, f11 = f[:, y0, x0], f[:, y0, x0 + 1], f[:, y0 + 1, x0], f[:, y0 + 1, x0 + 1]
    anti = np.where(fx + fy <= 1, f00 + fx * (f10 - f00) + fy * (f01 - f00), f11 + (1 - fx) * (f01 - f11) + (1 - fy) * (f10 - f11))
    main = np.where(fx >= fy, f00 + fx * (f10 - f00) + fy * (f11 - f10), f00 + fx * (f11 - f01) + fy * (f01 - f00))
    out = np.where(np.asarray(mask, dtype=bool)[y0, x0], anti, main).T
    if corners:
        return out, np.max(np.abs(np.stack([f00, f10, f01, f11])), axis=0).T
    return out


@functools.lru_cache(maxsize=None)
def g17():
    """{(H, W): bool [H-1, W-1]} of the fixture, and the scipy version that produced it."""
    d = np.load(G17)
    masks = {}
    for H, W in d["sizes"].tolist():
        cells = (H - 1) * (W - 1)
        masks[(H, W)] = np.unpackbits(d[f"mask_{H}x{W}"])[:cells].astype(bool).reshape(H - 1, W - 1)
    return masks, str(d["scipy"])


def mask_variants(H, W):
    """The three masks every kernel case runs under: scipy's, scipy's with every bit flipped, and main diagonals only."""
    m = g17()[0][(H, W)]
    return {"g17": m, "flipped": ~m, "all-main": np.zeros_like(m)}


def hand_pixels(H, W):
    """[n,2] float64 pixels (u, v) inside the H x W image where an implementation is most easily wrong: the four corners; u = W-1 and
    v = H-1 with a fractional other coordinate; integer pixels; points on each diagonal (fx == fy, fx + fy == 1) of the first, a
    middle and the last cell; points within 1e-9 of a cell border."""
    X, Y = float(W - 1), float(H - 1)
    p = [(0, 0), (X, 0), (0, Y), (X, Y), (X, 0.37 * Y), (0.61 * X, Y), (min(1, X), min(1, Y)), (W // 2, H // 2), (X, H // 2), (W // 2, 0)]
    for cx, cy in {(0, 0), ((W - 2) // 2, (H - 2) // 2), (W - 2, H - 2)}:
        p += [(cx + 0.25, cy + 0.25), (cx + 0.5, cy + 0.5), (cx + 0.25, cy + 0.75), (cx + 0.75, cy + 0.25), (cx + 0.6875, cy + 0.6875)]
    cx, cy = (W - 2) // 2, (H - 2) // 2
    p += [(cx + 1 - 1e-9, cy + 0.3), (cx + 1 + 1e-9, cy + 0.3), (cx + 0.3, cy + 1e-9), (cx + 0.7, cy + 1 - 1e-9), (cx + 1e-9, cy + 1 - 1e-9)]
    return np.clip(np.asarray(p, dtype=np.float64), 0.0, [X, Y])


def noise_images(V, H, W, seed, px=3.0):
    """[V,2,H,W] float32 noise of `px` pixels: neighbouring texels unrelated, so a wrong corner, triangle or diagonal shows."""
    return (np.random.default_rng(seed).standard_normal((V, 2, H, W)) * px).astype(np.float32)


def cloud(P, H, W, seed):
    """sceneflow_cases.cloud where its margins fit the image; in a smaller image points spread over and a little beyond it, point 0
    near the centre so that every view sees one."""
    if min(H, W) >= 8:
        return sc.cloud(P, H, W, seed)
    rng = np.random.default_rng(seed)
    K = sc.intrinsics(H, W)
    z = rng.uniform(2.5, 4.0, P)
    u, v = rng.uniform(-0.4, W - 0.6, P), rng.uniform(-0.4, H - 0.6, P)
    u[0], v[0] = (W - 1) / 2 + 0.1, (H - 1) / 2 - 0.15
    return np.stack([(u - K[0, 2]) / K[0, 0] * z, (v - K[1, 2]) / K[1, 1] * z, z]).astype(np.float32)


class KernelCase:
    """mom_flow_sample's inputs for V views of P points in H x W images: the views of a projected cloud (motion.prepare_views), the
    first valid slots of every view then overwritten with the hand-placed pixels (each view starts at another of them)."""
    def __init__(self, H, W, P, V):
        motion = importlib.import_module("iclr2025_3d-mom_amd.motion")
        self.H, self.W, self.P, self.V = H, W, P, V
        self.points = cloud(P, H, W, seed=P + H)
        self.views = motion.prepare_views(self.points, sc.intrinsics(H, W), sc.poses(V, seed=V + W), H, W)
        self.images = noise_images(V, H, W, seed=1000 * H + W + P + V)
        self.bits = motion.valid_words(self.views)
        hand = hand_pixels(H, W)
        self.pix = np.zeros((V, P, 2), np.float64)
        for j, idx in enumerate(self.views.valid):
            self.pix[j, idx] = self.views.pix64[j].T
            n = min(len(hand), len(idx))
            self.pix[j, idx[:n]] = np.roll(hand, -7 * j, axis=0)[:n]

    @functools.lru_cache(maxsize=None)
    def expected(self, which):
        """Under mask_variants(H, W)[which]: per view (gt [n_j,2] float64, corner magnitudes [n_j,2]) at the view's valid points."""
        mask = mask_variants(self.H, self.W)[which]
        return [restate(self.images[j], self.pix[j, idx], mask, corners=True) for j, idx in enumerate(self.views.valid)]


@functools.lru_cache(maxsize=None)
def kernel_case(H, W, P, V):
    return KernelCase(H, W, P, V)


def check_records(rec, case, expected, valid=None, name=""):
    """rec [V,P,4] (numpy, from the device) against `expected` (KernelCase.expected's form) at `valid` (default: the case's valid
    sets): pix0 bit-equal to float32(pix); gt within one float32 ulp of the cell's largest corner magnitude, 2^-23 max|f| -- the
    result is a convex combination of the corners, two float64 evaluations of it differ by a few 2^-53 max|f|, so their float32
    roundings are equal or adjacent; every other record exactly zero.  Prints the share of bit-equal gt elements."""
    valid = case.views.valid if valid is None else valid
    equal = total = 0
    worst = 0.0
    for j, idx in enumerate(valid):
        gt, cmax = expected[j]
        assert np.array_equal(rec[j, idx, :2].view(np.uint32), case.pix[j, idx].astype(np.float32).view(np.uint32)), (name, j)
        want = gt.astype(np.float32)
        d = np.abs(rec[j, idx, 2:].astype(np.float64) - want.astype(np.float64))
        assert np.isfinite(rec[j, idx]).all() and (d <= 2.0 ** -23 * cmax).all(), (name, j, float((d / np.maximum(cmax, 1e-300)).max()) * 2 ** 23)
        worst = max(worst, float((d / np.maximum(cmax, 1e-300)).max()) * 2 ** 23) if d.size else worst
        equal += int((rec[j, idx, 2:].view(np.uint32) == want.view(np.uint32)).sum())
        total += want.size
        out = np.ones(rec.shape[1], bool)
        out[idx] = False
        assert not rec[j, out].view(np.uint32).any(), (name, j)               # four zeros, +0.0 each
    print(f"{name}: gt bit-equal in {equal} of {total} elements ({100.0 * equal / max(total, 1):.2f} %), "
          f"largest distance {worst:.3f} of the bound (one float32 ulp of the cell's largest corner)")
    return equal, total
