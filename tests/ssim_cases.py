"""Inputs, a float64 reference, a float32 restatement and a derived error bound for the SSIM kernels (csrc/ssim.hip): shared by
tests/test_ssim_cpu.py and tests/test_ssim_gpu.py.  numpy and torch on the CPU only.

What is computed (include/mom4d.h, "SSIM term of the loss"), x the rendered image, y the ground truth, blur the 11 x 11 window
w (x) w of the eleven taps w with zero padding 5, C1 = 0.01^2, C2 = 0.03^2:
    mu1 = blur x, mu2 = blur y, E11 = blur x^2, E22 = blur y^2, E12 = blur xy
    s1 = E11 - mu1^2, s2 = E22 - mu2^2, s12 = E12 - mu1 mu2
    A = mu1^2 + mu2^2 + C1, B = s1 + s2 + C2, Cn = 2 mu1 mu2 + C1, D = 2 s12 + C2, map = Cn D / (A B)
    dm0 = d map / d mu1 = 2 mu2 (D - Cn) / (A B) - 2 mu1 map (B - A) / (A B)
    dm1 = d map / d E11 = -map / B,        dm2 = d map / d E12 = 2 Cn / (A B)
    d sum(map) / d x = blur dm0 + 2 x blur dm1 + y blur dm2        (the zero-padded symmetric blur is its own transpose)

reference64   the above in float64, the taps widened exactly.  The window it blurs with is then the exact product w_i w_j, which
              is what a separable float32 kernel approximates.  oracle/torch_ref.ssim blurs with ONE 11 x 11 window whose entries
              are the float32 ROUNDINGS of those products (relative difference up to 2^-24 per entry): `window2d` hands reference64
              that window instead, and only in that form can the two agree to 1e-12 (tests/test_ssim_cpu.py checks that, and the
              distance between the two forms against the bound below).
restatement32 the kernel's arithmetic in float32 numpy, in its order: rows then columns, eleven taps each accumulated from k = 0
              onto 0, zero outside the image, s = E - mu^2 as one subtraction, inv_AB = 1 / (A B), block sums of 256 threads as a
              butterfly within each 64 lanes and ((p0 + p1) + p2) + p3, doubles behind slot 1 + block % 63.  numpy multiplies and
              adds separately where the compiled kernel fuses; both are inside the bound.  `fault` plants one defect (FAULTS).

bound         a first-order running error bound of a float32 evaluation, in float64, per pixel.  u = 2^-24,
              gamma(n) = n u / (1 - n u).  Nothing below was chosen by looking at what an evaluation returns.
 (1) One pass of the blur is a sum of eleven products accumulated onto 0: a term passes through its product and at most ten
     additions (fused or not), eleven roundings; x^2, y^2 and xy carry one more for the product formed first.  The second pass
     acts on the computed first pass.  gamma(a) + gamma(b) + gamma(a) gamma(b) <= gamma(a + b), so
         e(mu) = gamma(22) blur|t|,  e(E) = gamma(23) blur|t|                      (K_BLUR; t the blurred image)
     (oracle/torch_ref.ssim in float32 is a direct 121-tap convolution, whose worst case would be gamma(123): it is not what
     this bound was derived for.  tests/test_ssim_cpu.py holds it to the same bound all the same, and it stays inside.)
 (2) FIRST ORDER from here on (products of two errors are dropped; `ab_rel` below keeps that honest).
     e(mu^2) = 2 |mu| e(mu) + u mu^2,  e(mu1 mu2) = |mu2| e(mu1) + |mu1| e(mu2) + u |mu1 mu2|
     e(s) = e(E) + e(mu^2) + u (|E| + mu^2)            (the subtraction, fused with the product or not)
     e(A) = e(mu1^2) + e(mu2^2) + u (mu1^2 + mu2^2) + u A + 3 u C1      (two additions; C1 = fl(fl(.01) fl(.01)): three roundings)
     e(B) = e(s1) + e(s2) + u (|s1| + |s2|) + u (|s1| + |s2| + C2) + 3 u C2
     e(Cn) = 2 e(mu1 mu2) + u (2 |mu1 mu2| + C1) + 3 u C1,   e(D) = 2 e(s12) + u (2 |s12| + C2) + 3 u C2
 (3) map, dm0, dm1, dm2 are functions F of (mu1, mu2, A, B, Cn, D).  Their exact partial derivatives come from float64 autograd of
     sum(F) (everything after the blur is elementwise).  e(F) = sum_v |dF/dv| e(v) + the roundings of F's own operations:
     1 / (A B) counts 1 + 3 (a division is allowed 3 u, which covers a reciprocal that is not correctly rounded),
         map 6 u |map|;   dm1 9 u |dm1|;   dm2 5 u |dm2|;   dm0 8 u |T1| + 15 u |T2|,  T1, T2 its two terms.
     FIRST ORDER: the partials are taken at the exact point.  `ab_rel` = e(A)/A + e(B)/B is the relative perturbation of the
     denominator; every case asserts it below 1/8 (it is below 1e-2 on all of them).
 (4) gradient: blur e(dm0) + 2 |x| blur e(dm1) + |y| blur e(dm2)  +  (gamma(22) + 3 u) T,
     T = blur|dm0| + 2 |x| blur|dm1| + |y| blur|dm2|: the blur of the computed maps as in (1) and two products and two additions.
     Scaled by s: |s| times that + 2 u |s g| (the product scale * scale_dev, and the multiplication).
 (5) sum over a set of pixels: sum e(map) + gamma(9) sum|map| (a block's float32 tree is 9 additions deep; the doubles behind it
     add floats exactly to 2^-50).  The value a caller forms, float(sum / n): that over n, + u |value|.

Membership.  The bound is proportional to the magnitudes AROUND a pixel, so it is tight where the image is dark or flat in value
and a wrong pixel cannot hide behind a large one elsewhere.  Where every term is exactly zero the bound is zero and `share`
demands the exact value: that is how the impulse cases pin which pixels a window reaches."""
import functools
import importlib

import numpy as np
import torch

pkg = "iclr2025_3d-mom_amd"
EPS = 2.0 ** -24
C1, C2 = 0.01 ** 2, 0.03 ** 2
TILE, RADIUS, SLOTS = 16, 5, 64
K_BLUR = (22, 23)
FAULTS = ("tap", "c2", "replicate", "radius4", "seam", "no_2x", "last_row", "slot")    # ("dm4": slab_args(keep=4))


def gamma(n, u=EPS):
    return n * u / (1.0 - n * u)


def window():
    """ops.ssim_window()'s eleven float32 taps."""
    ops = importlib.import_module(pkg + ".ops")
    return np.array(list(ops.ssim_window()), np.float32)


def fold(a):
    """[..., H, W] -> [C, H, W] (the kernels fold every leading dimension into the channels)."""
    a = np.asarray(a)
    return a.reshape((-1,) + a.shape[-2:])


# ------------------------------------------------------------------------------------------------------------ float64
def blur64(a, w, window2d=None):
    """Zero-padded blur of [C,H,W] float64 with w (x) w, or with the 11 x 11 `window2d`."""
    w = np.asarray(w, np.float64)
    C, H, W = a.shape
    p = np.pad(a, ((0, 0), (RADIUS, RADIUS), (RADIUS, RADIUS)))
    if window2d is not None:
        out = np.zeros_like(a)
        for i in range(11):
            for j in range(11):
                out += window2d[i, j] * p[:, i:i + H, j:j + W]
        return out
    h = sum(w[k] * p[:, :, k:k + W] for k in range(11))
    return sum(w[k] * h[:, k:k + H, :] for k in range(11))


def _outputs(mu1, mu2, A, B, Cn, D):
    iab = 1.0 / (A * B)
    m = Cn * D * iab
    t1 = 2.0 * mu2 * (D - Cn) * iab
    t2 = 2.0 * mu1 * m * (B - A) * iab
    return dict(map=m, dm0=t1 - t2, dm1=-m / B, dm2=2.0 * Cn * iab, t1=t1, t2=t2)


def _nodes(mo):
    mu1, mu2, e11, e22, e12 = mo
    s1, s2, s12 = e11 - mu1 * mu1, e22 - mu2 * mu2, e12 - mu1 * mu2
    return dict(s1=s1, s2=s2, s12=s12, A=mu1 * mu1 + mu2 * mu2 + C1, B=s1 + s2 + C2, Cn=2.0 * mu1 * mu2 + C1, D=2.0 * s12 + C2)


def reference64(img, gt, window11, window2d=None):
    """Per pixel, float64, [C,H,W] each: the five blurred moments "mu1 mu2 e11 e22 e12", "map", the derivative maps "dm" [3,C,H,W]
    and "grad" = d sum(map) / d img (no scale); "sum" = sum(map)."""
    x, y = np.asarray(fold(img), np.float64), np.asarray(fold(gt), np.float64)
    b = lambda a: blur64(a, window11, window2d)
    mo = [b(x), b(y), b(x * x), b(y * y), b(x * y)]
    n = _nodes(mo)
    o = _outputs(mo[0], mo[1], n["A"], n["B"], n["Cn"], n["D"])
    dm = np.stack([o["dm0"], o["dm1"], o["dm2"]])
    grad = b(dm[0]) + 2.0 * x * b(dm[1]) + y * b(dm[2])
    return dict(mu1=mo[0], mu2=mo[1], e11=mo[2], e22=mo[3], e12=mo[4], map=o["map"], dm=dm, grad=grad, sum=float(o["map"].sum()),
                nodes=n, t1=o["t1"], t2=o["t2"], x=x, y=y)


def bound(img, gt, window11, ref=None):
    """The module docstring's bound around reference64 (`ref`, computed if not given): "map", "dm" [3,C,H,W], "grad" (scale 1),
    and "ab_rel", the largest relative perturbation of A B (to be asserted below 1/8)."""
    r = reference64(img, gt, window11) if ref is None else ref
    x, y = r["x"], r["y"]
    b = lambda a: blur64(a, window11)
    u = EPS
    g_mu, g_e = gamma(K_BLUR[0]), gamma(K_BLUR[1])
    mu1, mu2, e11, e22, e12 = (r[n] for n in ("mu1", "mu2", "e11", "e22", "e12"))
    n = r["nodes"]
    e_mu1, e_mu2 = g_mu * b(np.abs(x)), g_mu * b(np.abs(y))
    e_e11, e_e22, e_e12 = g_e * b(x * x), g_e * b(y * y), g_e * b(np.abs(x * y))
    e_m1sq = 2 * np.abs(mu1) * e_mu1 + u * mu1 ** 2
    e_m2sq = 2 * np.abs(mu2) * e_mu2 + u * mu2 ** 2
    e_m12 = np.abs(mu2) * e_mu1 + np.abs(mu1) * e_mu2 + u * np.abs(mu1 * mu2)
    e_s1 = e_e11 + e_m1sq + u * (np.abs(e11) + mu1 ** 2)
    e_s2 = e_e22 + e_m2sq + u * (np.abs(e22) + mu2 ** 2)
    e_s12 = e_e12 + e_m12 + u * (np.abs(e12) + np.abs(mu1 * mu2))
    a12 = np.abs(n["s1"]) + np.abs(n["s2"])
    err = dict(mu1=e_mu1, mu2=e_mu2,
               A=e_m1sq + e_m2sq + u * (mu1 ** 2 + mu2 ** 2) + u * n["A"] + 3 * u * C1,
               B=e_s1 + e_s2 + u * a12 + u * (a12 + C2) + 3 * u * C2,
               Cn=2 * e_m12 + u * (2 * np.abs(mu1 * mu2) + C1) + 3 * u * C1,
               D=2 * e_s12 + u * (2 * np.abs(n["s12"]) + C2) + 3 * u * C2)
    names = ("mu1", "mu2", "A", "B", "Cn", "D")
    leaves = [torch.from_numpy(np.ascontiguousarray(v)).requires_grad_(True) for v in (mu1, mu2, n["A"], n["B"], n["Cn"], n["D"])]
    o = _outputs(*leaves)
    own = dict(map=6 * u * np.abs(r["map"]), dm0=8 * u * np.abs(r["t1"]) + 15 * u * np.abs(r["t2"]), dm1=9 * u * np.abs(r["dm"][1]),
               dm2=5 * u * np.abs(r["dm"][2]))
    e = {}
    for name in ("map", "dm0", "dm1", "dm2"):
        parts = torch.autograd.grad(o[name].sum(), leaves, retain_graph=True, allow_unused=True)
        e[name] = own[name] + sum(np.abs(p.numpy()) * err[v] for v, p in zip(names, parts) if p is not None)
    e_dm = np.stack([e["dm0"], e["dm1"], e["dm2"]])
    adm = np.abs(r["dm"])
    T = b(adm[0]) + 2 * np.abs(x) * b(adm[1]) + np.abs(y) * b(adm[2])
    e_grad = b(e_dm[0]) + 2 * np.abs(x) * b(e_dm[1]) + np.abs(y) * b(e_dm[2]) + (gamma(K_BLUR[0]) + 3 * u) * T
    return dict(map=e["map"], dm=e_dm, grad=e_grad, ab_rel=float((err["A"] / n["A"] + err["B"] / n["B"]).max()))


def grad_bound(ref, bnd, scale):
    """(4): the bound of scale * grad."""
    return abs(scale) * bnd["grad"] + 2 * EPS * np.abs(scale * ref["grad"])


def sum_ref_bound(ref, bnd, rows=None):
    """(5): (float64 sum of the map over image rows [rows[0], rows[1]), its bound)."""
    sl = slice(None) if rows is None else slice(rows[0], rows[1])
    m = ref["map"][:, sl]
    return float(m.sum()), float(bnd["map"][:, sl].sum() + (gamma(9) + 2.0 ** -50) * np.abs(m).sum())


def value_bound(ref, bnd):
    """(5): the bound of float(sum / n)."""
    s, e = sum_ref_bound(ref, bnd)
    n = ref["map"].size
    return e / n + EPS * abs(s / n)


def block_ref_bound(ref, bnd):
    """(5) per 16 x 16 block, in the kernel's block order b = bx + gx (by + gy c): (float64 sums of the map, bounds)."""
    C, H, W = ref["map"].shape
    gy, gx = -(-H // TILE), -(-W // TILE)

    def per_block(a):
        p = np.zeros((C, gy * TILE, gx * TILE))
        p[:, :H, :W] = a
        return p.reshape(C, gy, TILE, gx, TILE).sum(axis=(2, 4)).reshape(-1)
    return per_block(ref["map"]), per_block(bnd["map"]) + (gamma(9) + 2.0 ** -50) * per_block(np.abs(ref["map"]))


def slot_ref_bound(ref, bnd):
    """(5) per partial-sum slot: block b adds into slot 1 + b % 63.  ([64] float64 sums, [64] bounds); slot 0 is the total."""
    s, e = block_ref_bound(ref, bnd)
    slot = 1 + np.arange(s.size) % (SLOTS - 1)
    sums, bounds = np.zeros(SLOTS), np.zeros(SLOTS)
    np.add.at(sums, slot, s)
    np.add.at(bounds, slot, e)
    sums[0], bounds[0] = sums[1:].sum(), bounds[1:].sum()
    return sums, bounds


def share(got, want, bnd):
    """Largest |got - want| / bound over the elements; an element whose bound is 0 must be met exactly (share inf if not)."""
    d = np.abs(np.asarray(got, np.float64) - want)
    bnd = np.broadcast_to(np.asarray(bnd, np.float64), d.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        s = np.where(bnd > 0, d / bnd, np.where(d == 0, 0.0, np.inf))
    return float(s.max()) if s.size else 0.0


# ------------------------------------------------------------------------------------------------------------ float32
def _blur32_axis(a, w, axis, replicate):
    pad = [(0, 0)] * 3
    pad[axis] = (RADIUS, RADIUS)
    p = np.pad(a, pad, mode="edge" if replicate else "constant")
    n = a.shape[axis]
    acc = np.zeros_like(a)
    for k in range(11):
        acc = acc + w[k] * np.take(p, np.arange(k, k + n), axis=axis)
    return acc


def _block_sums32(m):
    """[C,H,W] float32 (zero where a pixel does not count) -> [C,gy,gx] float32 block sums in the kernel's order."""
    C, H, W = m.shape
    gy, gx = -(-H // TILE), -(-W // TILE)
    p = np.zeros((C, gy * TILE, gx * TILE), np.float32)
    p[:, :H, :W] = m
    v = p.reshape(C, gy, TILE, gx, TILE).transpose(0, 1, 3, 2, 4).reshape(C, gy, gx, TILE * TILE)     # thread = ty * 16 + tx
    lane = np.arange(TILE * TILE)
    for d in (32, 16, 8, 4, 2, 1):
        v = v + v[..., lane ^ d]
    return ((v[..., 0] + v[..., 64]) + v[..., 128]) + v[..., 192]


def restatement32(img, gt, window11, sum_rows=None, dm_rows=None, fault=None):
    """The kernel's float32 arithmetic on a [C,H,W] image or row slab (module docstring): "map", "dm" [3,C,H,W] (zero outside
    dm_rows), "grad" (scale 1, from that dm), float32; "slots" the 64 doubles behind `sum`, "sum" = slots[0].
    fault: one of FAULTS, planted."""
    assert fault is None or fault in FAULTS, fault
    f32 = np.float32
    x, y = np.asarray(fold(img), f32), np.asarray(fold(gt), f32)
    C, H, W = x.shape
    w = np.asarray(window11, f32).copy()
    if fault == "tap":
        w[3] = f32(w[3] * (1.0 + 1e-4))
    if fault == "radius4":
        w[0] = w[10] = 0
    c1, c2 = f32(0.01) * f32(0.01), f32(0.03) * f32(0.03)
    if fault == "c2":
        c2 = f32(c2 * (1.0 + 1e-3))
    rep = fault == "replicate"

    def blur(a, seam=False):
        h = _blur32_axis(a, w, 2, rep)                       # rows: along x
        if seam and W > TILE:
            h[:, :, TILE] = h[:, :, TILE - 1]                # the second tile's first column reads its neighbour's row blur
        return _blur32_axis(h, w, 1, rep)                    # columns
    seam = fault == "seam"
    mu1, mu2 = blur(x, seam), blur(y, seam)
    e11, e22, e12 = blur(x * x, seam), blur(y * y, seam), blur(x * y, seam)
    mu1_sq, mu2_sq, mu12 = mu1 * mu1, mu2 * mu2, mu1 * mu2
    s1, s2, s12 = e11 - mu1_sq, e22 - mu2_sq, e12 - mu12
    A, B = mu1_sq + mu2_sq + c1, s1 + s2 + c2
    Cn, D = f32(2) * mu12 + c1, f32(2) * s12 + c2
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        inv_ab = f32(1) / (A * B)
        m = Cn * D * inv_ab
        dm = np.stack([f32(2) * mu2 * (D - Cn) * inv_ab - f32(2) * mu1 * m * (B - A) * inv_ab, -m / B, f32(2) * Cn * inv_ab])
    r0, r1 = (0, H) if dm_rows is None else dm_rows
    keep = np.zeros(H, bool)
    keep[max(r0, 0):max(r1, 0)] = True
    dm = np.where(keep[None, None, :, None], dm, f32(0))
    b = [blur(dm[i]) for i in range(3)]
    two_x = x if fault == "no_2x" else f32(2) * x
    grad = (b[0] + two_x * b[1]) + y * b[2]
    q0, q1 = (0, H) if sum_rows is None else sum_rows
    if fault == "last_row":
        q1 -= 1
    cnt = np.zeros(H, bool)
    cnt[max(q0, 0):max(q1, 0)] = True
    tot = _block_sums32(np.where(cnt[None, :, None], m, f32(0))).astype(np.float64).reshape(-1)      # block = bx + gx (by + gy c)
    slots = np.zeros(SLOTS)
    for blk, t in enumerate(tot):
        if fault == "slot" and blk == SLOTS - 1:
            continue                                          # the first block that wraps onto slot 1 is lost
        slots[1 + blk % (SLOTS - 1)] += t
    slots[0] = slots[1:].sum()
    return dict(map=m, dm=dm, grad=grad, slots=slots, sum=float(slots[0]), blocks=len(tot))


def fma32(a, b, c):
    """fl32(a * b + c) with ONE rounding, elementwise on float32 arrays (what `c += a * b` compiles to in the kernels)."""
    a, b, c = (np.asarray(v, np.float32).astype(np.float64) for v in np.broadcast_arrays(a, b, c))
    p = a * b                                                 # exact: 24 x 24 bits
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)                           # TwoSum: p + c = s + err exactly
    r = s.astype(np.float32)
    d = s - r.astype(np.float64)
    other = np.nextafter(r, np.where(d > 0, np.inf, -np.inf).astype(np.float32))
    # s can only mislead where it is exactly half way between two floats: the part the double dropped then decides
    tie = (d != 0) & (2.0 * np.abs(d) == np.abs(other.astype(np.float64) - r.astype(np.float64))) & (err != 0)
    return np.where(tie & (np.sign(err) == np.sign(d)), other, r).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------ inputs
FAMILIES = ("noise", "flat_white", "flat_grey", "equal", "black_render", "both_black", "blocks", "overshoot")


def family(name, shape):
    """(img, gt): float32 arrays of `shape`, a function of the family's name and the shape alone."""
    g = torch.Generator().manual_seed(1000 * (FAMILIES + ("impulse",)).index(name) + sum((i + 1) * s for i, s in enumerate(shape)))
    rand = lambda: torch.rand(shape, generator=g)
    randn = lambda: torch.randn(shape, generator=g)
    if name == "noise":                 # tests/test_ops_gpu.py's pair
        gt = rand()
        img = (gt + 0.15 * randn()).clamp(0, 1)
    elif name == "flat_white":          # a saturated background against a render that is almost there
        gt = torch.ones(shape)
        img = 1.0 - 0.01 * rand()
    elif name == "flat_grey":
        gt = 0.7 + 1e-3 * randn()
        img = 0.7 + 1e-3 * randn()
    elif name == "equal":
        gt = rand()
        img = gt.clone()
    elif name == "black_render":        # the first iterations
        gt = rand()
        img = torch.zeros(shape)
    elif name == "both_black":
        gt, img = torch.zeros(shape), torch.zeros(shape)
    elif name == "blocks":              # 8 x 8 binary blocks: edges at every multiple of 8, so on and beside every tile seam
        H, W = shape[-2:]
        cells = (torch.rand(tuple(shape[:-2]) + (-(-H // 8), -(-W // 8)), generator=g) < 0.5).float()
        gt = cells.repeat_interleave(8, -2).repeat_interleave(8, -1)[..., :H, :W].contiguous()
        img = gt + 0.05 * randn()
    elif name == "overshoot":           # an unclamped render: values below 0 and above 1
        gt = rand()
        img = 1.6 * gt - 0.2
    else:
        raise KeyError(name)
    return img.float().numpy(), gt.float().numpy()


def impulse(shape, r, c):
    """img one 1.0 at (r, c) of every channel on zeros, gt zero: mu1 is the window itself.  Negative r, c count from the end."""
    img = np.zeros(shape, np.float32)
    img[..., r, c] = 1.0
    return img, np.zeros(shape, np.float32)


# (family, shape, why this pair is here)
CASES = (
    ("noise", (1, 1, 1), "one pixel: every tap but the centre falls on padding"),
    ("flat_white", (1, 1, 1), "... and B is all but C2"),
    ("noise", (1, 1, 40), "H = 1: the column pass sees ten rows of padding; three tiles across"),
    ("blocks", (1, 40, 1), "W = 1: the same for the row pass; three tiles down"),
    ("noise", (3, 5, 7), "smaller than the window's radius both ways, three channels"),
    ("flat_grey", (3, 5, 7), "the same shape where s = E - mu^2 cancels"),
    ("noise", (1, 11, 11), "one window exactly"),
    ("blocks", (1, 15, 17), "one short of a tile down, one past it across"),
    ("noise", (1, 16, 16), "one tile exactly: no partial block"),
    ("flat_grey", (1, 16, 16), "one tile, flat"),
    ("blocks", (1, 17, 15), "one past a tile down, one short across"),
    ("overshoot", (1, 17, 15), "negative and > 1 values next to the ragged edge"),
    ("noise", (2, 32, 48), "whole tiles only: every seam is interior"),
    ("equal", (2, 32, 48), "img == gt: map 1, gradient a sum of cancelling terms"),
    ("noise", (3, 37, 53), "ragged both ways, several blocks (tests/test_ops_gpu.py's shape)"),
    ("flat_white", (3, 37, 53), "the pair on which the float32 oracle itself is 4e-5 off"),
    ("flat_grey", (3, 37, 53), "flat away from 1"),
    ("black_render", (3, 37, 53), "img = 0: mu1, E11, E12 exactly 0"),
    ("both_black", (1, 17, 33), "everything 0: map exactly C1 C2 / (C1 C2), dm1 = -1 / C2 carries C2 alone"),
    ("blocks", (3, 37, 53), "edges on and beside the seams at 16 and 32"),
    ("overshoot", (3, 37, 53), "an unclamped render"),
    ("equal", (3, 37, 53), "img == gt, ragged"),
    ("noise", (2, 3, 21, 33), "a leading batch dimension folded into the channels"),
    ("black_render", (2, 3, 21, 33), "... with a black render"),
    ("noise", (1, 112, 144), "63 blocks: every slot once, none twice"),
    ("flat_white", (1, 112, 144), "63 blocks, flat"),
    ("noise", (1, 128, 128), "64 blocks: the first wrap onto slot 1"),
    ("flat_grey", (1, 128, 128), "64 blocks, flat"),
    ("noise", (4, 65, 81), "120 blocks: every slot but the last twice, ragged"),
    ("blocks", (4, 65, 81), "120 blocks, edges on the seams"),
)
WRAP_SHAPES = ((1, 112, 144), (1, 128, 128), (4, 65, 81))
IMPULSE_SHAPES = ((1, 32, 32), (1, 17, 33))


def impulse_positions(shape):
    """Corners, both sides of the seam at 16 in both directions, the last row and column, the centre."""
    H, W = shape[-2:]
    pos = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (15, 15), (15, 16), (16, 15), (16, 16), (H - 1, W // 2), (H // 2, W - 1),
           (H // 2, W // 2)]
    return tuple(dict.fromkeys(pos))


def blocks_of(shape):
    H, W = shape[-2:]
    return int(np.prod(shape[:-2])) * (-(-H // TILE)) * (-(-W // TILE))


def _pack(img, gt):
    w = window()
    ref = reference64(img, gt, w)
    bnd = bound(img, gt, w, ref)
    assert bnd["ab_rel"] < 0.125, bnd["ab_rel"]               # first order is valid
    for a in (img, gt):
        a.setflags(write=False)
    return dict(img=img, gt=gt, w=w, ref=ref, bnd=bnd)


@functools.lru_cache(maxsize=None)
def case(name, shape):
    """One (family, shape) pair with its reference and bound (shared, read-only)."""
    return _pack(*family(name, shape))


@functools.lru_cache(maxsize=None)
def impulse_case(shape, r, c):
    return _pack(*impulse(shape, r, c))


# ------------------------------------------------------------------------------------------------------------ row slabs
SLAB_IMAGES = ((3, 96, 40), (3, 90, 40))                      # six tile rows each; the second one's last tile row is ragged
SLAB_SPLITS = (((0, 2), (2, 4), (4, 6)), ((0, 1), (1, 5), (5, 6)), tuple((i, i + 1) for i in range(6)))


def slab_args(H, W, rows, keep=RADIUS):
    """The arguments of mom_ssim_forward_slab / _backward_slab for a rank that owns the tile rows [rows[0], rows[1]) of an H x W
    image, formed as FusedStep forms them: one tile row of halo, dm rows `keep` = 5 beyond the own rows, clipped to the image.
    Image coordinates: slab = (ys0, ys1), own = (y0, y1); slab coordinates: sum, dm.  off: elements from a channel's first row to
    the slab's."""
    gy = (H + 15) // 16
    fwd = (max(rows[0] - 1, 0), min(rows[1] + 1, gy))
    ys0, ys1 = fwd[0] * 16, min(H, fwd[1] * 16)
    y0, y1 = rows[0] * 16, min(H, rows[1] * 16)
    return dict(slab=(ys0, ys1), own=(y0, y1), sum=(y0 - ys0, y1 - ys0), dm=(max(0, y0 - keep) - ys0, min(H, y1 + keep) - ys0),
                off=ys0 * W, H=ys1 - ys0, grad=(y0, y1))


def unaligned_slab(W):
    """A slab the ABI allows and no caller forms: rows 23..71 of a 96-row image, sum and dm rows 28..66; its gradient is the
    whole image's where all of the window's dm rows were kept: rows 33..61."""
    return dict(slab=(23, 71), own=(28, 66), sum=(5, 43), dm=(5, 43), off=23 * W, H=48, grad=(33, 61))


def dm_rows_that_match(a, H):
    """Image rows of a slab's dm interval whose window lies inside the slab or is cut by a true image edge."""
    ys0, ys1 = a["slab"]
    rows = np.arange(a["dm"][0] + ys0, a["dm"][1] + ys0)
    ok = ((rows - RADIUS >= ys0) | (ys0 == 0)) & ((rows + RADIUS < ys1) | (ys1 == H))
    return rows[ok]


def slab_reference64(c, a):
    """reference64 of a slab ALONE (zero padding at its edges, as the slab entries see it): "map", "dm" kept on the slab's dm rows and
    zero elsewhere, "grad" from that dm.  Slab coordinates."""
    ys0, ys1 = a["slab"]
    r = reference64(fold(c["img"])[:, ys0:ys1], fold(c["gt"])[:, ys0:ys1], c["w"])
    keep = np.zeros(ys1 - ys0, bool)
    keep[a["dm"][0]:a["dm"][1]] = True
    dm = np.where(keep[None, None, :, None], r["dm"], 0.0)
    b = lambda v: blur64(v, c["w"])
    return dict(map=r["map"], dm=dm, grad=b(dm[0]) + 2.0 * r["x"] * b(dm[1]) + r["y"] * b(dm[2]))


def slab_list():
    """(image shape, name, arguments, tile rows) of every slab the tests run: each rank of each split of each image, and the
    unaligned one (tile rows None)."""
    out = []
    for shape in SLAB_IMAGES:
        for si, split in enumerate(SLAB_SPLITS):
            for rank, rows in enumerate(split):
                out.append((shape, "%dx%dx%d-split%d-rank%d" % (shape + (si, rank)), slab_args(shape[1], shape[2], rows), rows))
    out.append((SLAB_IMAGES[0], "unaligned", unaligned_slab(SLAB_IMAGES[0][2]), None))
    return out
