"""What tests/test_values_ordered_cpu.py and tests/test_values_ordered_gpu.py share: the sizes the ordered loss values are tried at, inputs
that mix magnitudes (so that an order shows in the bits), the documented order (include/mom4d.h, "ordered loss values") restated
in numpy with every float32 add and multiply done on its own, and the host twins through ctypes.  numpy and ctypes only; nothing here
touches a GPU.

The restatements are vectorised ACROSS independent sums (lanes, workgroups, blocks) and sequential ALONG every sum, so each add is
the one the order text names.  Where a list is padded, it is padded with +0.0 terms behind its last term: x + (+0.0) == x bit for bit
for every x a sum that started at +0.0 can hold."""
import ctypes as C
import functools
import importlib

import numpy as np

pkg = "iclr2025_3d-mom_amd"
N = importlib.import_module(pkg + "._native")
F32 = np.float32
BLOCK = 64
L1_SHARE = 4096                     # elements per workgroup of the L1 pass
REG_ROWS = 16                       # rows per workgroup of the regulariser

# n: 1, around a block of 64, one below / at / above a workgroup's share, fixture g3's 3 x 37 x 53, and 65 workgroups and a bit (the
# partials themselves then fill more than one block)
L1_SIZES = (1, 63, 64, 65, L1_SHARE - 1, L1_SHARE, L1_SHARE + 1, 3 * 37 * 53, 65 * L1_SHARE + 5)
SSIM_SHAPES = ((3, 37, 53), (3, 16, 16), (3, 150, 130))        # 36, 3 and 270 workgroups (270: more than four blocks of totals)
PLANES = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))      # (ca, cb) of plane p over (x, y, z, t): W = res[ca], H = res[cb]
REG_CASES = ("field32", "field16", "wide", "field32+wide")


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


# ------------------------------------------------------------------------------------------------ the documented order, in numpy
def fold_rows(v, dtype=F32):
    """fold() of every row of v [m, n]: blocks of 64 from the first, each left to right from +0.0, then the block sums left to right."""
    v = np.asarray(v)
    m, n = v.shape
    nb = (n + BLOCK - 1) // BLOCK
    pad = np.zeros((m, nb * BLOCK), dtype)
    pad[:, :n] = v.astype(dtype)
    pad = pad.reshape(m, nb, BLOCK)
    b = np.zeros((m, nb), dtype)
    for i in range(BLOCK):
        b = (b + pad[:, :, i]).astype(dtype)
    total = np.zeros(m, dtype)
    for j in range(nb):
        total = (total + b[:, j]).astype(dtype)
    return total


def fold(v, dtype=F32):
    return fold_rows(np.asarray(v).reshape(1, -1), dtype)[0]


def reversed_sum(terms, dtype=F32):
    """The same terms added one by one from the last to the first: another order, which a case must be able to tell from fold()."""
    t = dtype(0)
    for x in np.asarray(terms)[::-1]:
        t = dtype(t + dtype(x))
    return t


def l1_terms(img, gt):
    d = (img - gt).astype(F32)
    return np.abs(d), (d * d).astype(F32), d


def l1_numpy(img, gt):
    """(sums2 [2] float32, dimg [n] float32) in the documented order."""
    n = img.size
    G = (n + L1_SHARE - 1) // L1_SHARE
    a, q, d = l1_terms(img, gt)
    sums = []
    for terms in (a, q):
        pad = np.zeros(G * L1_SHARE, F32)
        pad[:n] = terms
        pad = pad.reshape(G, 4, 256, 4)                    # [g][r][t][j]: element 4096 g + 1024 r + 4 t + j
        lane = np.zeros((G, 256), F32)
        for r in range(4):
            for j in range(4):
                lane = (lane + pad[:, r, :, j]).astype(F32)
        sums.append(fold(fold_rows(lane)) if G else F32(0))
    inv_n = F32(1.0) / F32(n)
    dimg = np.where(d > 0, inv_n, np.where(d < 0, -inv_n, F32(0))).astype(F32)
    return np.array(sums, F32), dimg


def reg_plane_terms(p, w_smooth, w_l1):
    """Per (h, column) the two terms of a [H, row] plane: the smoothness term (0 where h + 2 >= H) and the |1 - p| term (None if w_l1 == 0)."""
    H, row = p.shape
    cs = F32(w_smooth) / (F32(H - 2) * F32(row)) if (H > 2 and w_smooth != 0) else F32(0)
    smooth = np.zeros((H, row), F32)
    if H > 2:
        two = (F32(2) * p[1:-1]).astype(F32)
        s = ((p[2:] - two).astype(F32) + p[:-2]).astype(F32)
        smooth[:H - 2] = ((cs * s).astype(F32) * s).astype(F32)
    l1 = None
    if w_l1 != 0:
        cl = F32(w_l1) / (F32(H) * F32(row))
        l1 = (cl * np.abs((F32(1) - p).astype(F32))).astype(F32)
    return smooth, l1


def reg_numpy(planes):
    """value (float32) of [(plane [H, row] float32, w_smooth, w_l1), ...] in the documented order; also the number of workgroups."""
    partials = []
    for p, w_smooth, w_l1 in planes:
        H, row = p.shape
        cb, rb = (row + 255) // 256, (H + REG_ROWS - 1) // REG_ROWS
        smooth, l1 = reg_plane_terms(p, w_smooth, w_l1)
        sp = np.zeros((rb * REG_ROWS, cb * 256), F32)
        sp[:H, :row] = smooth
        lp = np.zeros_like(sp)
        if l1 is not None:
            lp[:H, :row] = l1
        sp, lp = sp.reshape(rb, REG_ROWS, cb * 256), lp.reshape(rb, REG_ROWS, cb * 256)
        lane = np.zeros((rb, cb * 256), F32)
        for k in range(REG_ROWS):
            lane = (lane + sp[:, k]).astype(F32)
            if l1 is not None:
                lane = (lane + lp[:, k]).astype(F32)
        partials.append(fold_rows(lane.reshape(rb * cb, 256)))       # workgroup local = row block * cb + column block
    partials = np.concatenate(partials) if partials else np.zeros(0, F32)
    return fold(partials), partials.size


# ------------------------------------------------------------------------------------------------ inputs
def mixed(rng, n, small=1e-3, large=1e4, every=7):
    """n float32 values near `small`, every `every`-th one near `large`: sums of them round at every add."""
    v = rng.uniform(0.2, 1.0, n) * small * rng.choice([-1.0, 1.0], n)
    idx = np.arange(rng.integers(0, every), n, every)
    v[idx] = rng.uniform(0.2, 1.0, idx.size) * large * rng.choice([-1.0, 1.0], idx.size)
    return v.astype(F32)


@functools.lru_cache(maxsize=None)
def l1_inputs(n):
    """(img, gt) whose two lists of terms tell the documented order from the reversed one (the first seed from 1000 + n on that does:
    with 63 terms the two orders meet in the same float once in a while); n == 1 has one order."""
    for seed in range(1000 + n, 1100 + n):
        rng = np.random.default_rng(seed)
        gt = rng.uniform(0.0, 1.0, n).astype(F32)
        img = (gt + mixed(rng, n)).astype(F32)
        if n > 70:
            img[5], img[66] = gt[5], np.nextafter(gt[66], F32(-1))      # d == 0 (gradient 0) and the smallest negative d
        a, q, _ = l1_terms(img, gt)
        want = l1_numpy(img, gt)[0]
        if n == 1 or (bits(F32(reversed_sum(a))) != bits(want[0]) and bits(F32(reversed_sum(q))) != bits(want[1])):
            return img, gt
    raise AssertionError(f"no seed makes n = {n} order-sensitive")


@functools.lru_cache(maxsize=None)
def ssim_totals(shape):
    """Synthetic workgroup totals for an image of `shape`: floats near 1e16 among floats near 1, so that their DOUBLE sum rounds
    (the totals of real images, at most 256 each, add exactly in double in any order: an order cannot show in them); the first seed
    whose fold differs from the reversed sum."""
    Cn, H, W = shape
    blocks = Cn * ((H + 15) // 16) * ((W + 15) // 16)
    for seed in range(2000 + blocks, 2100 + blocks):
        t = mixed(np.random.default_rng(seed), blocks, small=1.0, large=1e16, every=3)
        if bits(np.float64(reversed_sum(t, np.float64))) != bits(np.float64(fold(t, np.float64))):
            return t
    raise AssertionError(f"no seed makes {blocks} totals order-sensitive")


def ssim_images(which):
    """(img1, img2) [3, H, W] float32 in [0, 1]: fixture g3's size, one tile per channel, and a flat pair."""
    rng = np.random.default_rng(77)
    if which == "flat":
        return np.full((3, 37, 53), 0.25, F32), np.full((3, 37, 53), 0.25, F32)
    H, W = (37, 53) if which == "g3" else (16, 16)
    a = rng.uniform(0, 1, (3, H, W)).astype(F32)
    return a, np.clip(a + rng.normal(0, 0.1, a.shape), 0, 1).astype(F32)


def field_planes(channels, res=(8, 8, 8, 5), multires=(1, 2), seed=5):
    """The twelve planes of a two-level field as [(plane [H, W * channels] float32, w_smooth, w_l1)]: space planes carry the
    total-variation weight, space-time planes the time-smoothness and the |1 - p| weights (scene/gaussian_model.py:730-769)."""
    rng = np.random.default_rng(seed + channels)
    out = []
    for m in multires:
        r = [res[0] * m, res[1] * m, res[2] * m, res[3]]
        for ca, cb in PLANES:
            W, H = r[ca], r[cb]
            p = mixed(rng, H * W * channels, small=1e-2, large=1e2, every=5).reshape(H, W * channels)
            if cb == 3:
                p = (p + F32(1)).astype(F32)
            out.append((p, 1e-4, 0.0) if cb != 3 else (p, 1e-2, 1e-4))
    return out


def wide_plane():
    """One plane over several workgroups in both directions: 330 rows (21 row blocks, the last of 10 rows) of 20 x 32 = 640 floats
    (3 column blocks, the last half empty): 63 workgroups."""
    p = mixed(np.random.default_rng(9), 330 * 640, small=1e-2, large=1e2, every=5).reshape(330, 640)
    return [((p + F32(1)).astype(F32), 1e-2, 1e-4)]


def reg_case(name):
    parts = {"field32": lambda: field_planes(32), "field16": lambda: field_planes(16), "wide": wide_plane}
    out = []
    for k in name.split("+"):
        out += parts[k]()
    return out


def reg_desc(planes, pointers=None):
    """The MomRegPlane array of `planes` (pointers: one address per plane, e.g. device pointers; default the host arrays')."""
    arr = (N.MomRegPlane * len(planes))()
    for i, (p, w_smooth, w_l1) in enumerate(planes):
        assert p.shape[1] % 32 == 0 and p.flags.c_contiguous
        arr[i].plane = p.ctypes.data if pointers is None else pointers[i]
        arr[i].grad = None
        arr[i].H, arr[i].W = p.shape[0], p.shape[1] // 32
        arr[i].w_smooth, arr[i].w_l1, arr[i].grad_scale = w_smooth, w_l1, 0.0
    return arr


# ------------------------------------------------------------------------------------------------ the host twins
def l1_host(img, gt):
    sums, dimg = np.full(2, np.nan, F32), np.full(img.size, np.nan, F32)
    assert N.lib().mom_l1_loss_ordered_host(img.size, ptr(img), ptr(gt), ptr(dimg), ptr(sums)) == N.MOM_OK
    return sums, dimg


def ssim_sum_host(totals):
    out = np.full(1, np.nan, np.float64)
    assert N.lib().mom_ssim_sum_ordered_host(totals.size, ptr(totals), ptr(out)) == N.MOM_OK
    return out[0]


def reg_host(planes):
    out = np.full(1, np.nan, F32)
    assert N.lib().mom_plane_regulation_ordered_host(reg_desc(planes), len(planes), ptr(out)) == N.MOM_OK
    return out[0]
