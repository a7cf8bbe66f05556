"""Shared by test_raster_ordered_cpu.py and test_raster_ordered_gpu.py: the documented order of the ordered backward reduction
(include/mom4d.h) restated in numpy float32, the scenes at which each of its mechanisms can go wrong, and a driver that runs the
ordered backward through the C ABI and brings back everything it defines (slot_base, partials, the accumulator record, status)."""
import ctypes as C

import numpy as np

from scenes import random_gaussians

VALUES, WAVES = 10, 4           # MOM_ORDERED_VALUES, the four 8x8 pixel blocks of a tile
SLOT_COUNTS = (1, 3, 4, 5, 63, 64, 65, 8160)      # 8160 = 60 x 34 x 4: a full-screen splat at 960x540, four waves a tile


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def ordered_sum_numpy(partials):
    """[n, 4, 10] float32 -> [10]: t[s] = (p0 + p1) + (p2 + p3); a[r] = +0.0 + t[r] + t[r+4] + ... left to right; (a0 + a2) + (a1 + a3)."""
    p = np.ascontiguousarray(partials, np.float32).reshape(-1, WAVES, VALUES)
    t = (p[:, 0] + p[:, 1]) + (p[:, 2] + p[:, 3])
    a = np.zeros((4, VALUES), np.float32)
    for r in range(4):
        for row in t[r::4]:
            a[r] = a[r] + row
    return (a[0] + a[2]) + (a[1] + a[3])


def record_numpy(slot_base, partials, gacc_floats):
    """The whole accumulator record [P, gacc_floats] from slot_base [P+1] and partials [slots, 4, 10]."""
    P = len(slot_base) - 1
    out = np.zeros((P, gacc_floats), np.float32)
    for g in range(P):
        out[g, :VALUES] = ordered_sum_numpy(partials[slot_base[g]:slot_base[g + 1]])
    return out


def random_partials(n, seed):
    """n slots of random partials over nine decades, with slots of exact zeros, -0.0 entries and a slot of -0.0 only."""
    rng = np.random.default_rng(seed)
    p = (rng.standard_normal((n, WAVES, VALUES)) * 10.0 ** rng.uniform(-6, 3, (n, WAVES, VALUES))).astype(np.float32)
    p[rng.random(n) < 0.2] = 0.0
    p[rng.random((n, WAVES, VALUES)) < 0.1] = -0.0
    if n >= 3:
        p[n // 2] = -0.0
    return p


# ---- scenes ----------------------------------------------------------------------------------------------------------------------
def _place(s, idx, px, py, z):
    """Move Gaussians `idx` so that they project to pixel centres (px, py) at depth z under the identity camera."""
    W, H = s["W"], s["H"]
    fx, fy = W / (2.0 * s["tanfovx"]), H / (2.0 * s["tanfovy"])
    s["means3D"][idx, 0] = ((px + 0.5 - W / 2.0) * z / fx).astype(np.float32)
    s["means3D"][idx, 1] = ((py + 0.5 - H / 2.0) * z / fy).astype(np.float32)
    s["means3D"][idx, 2] = z.astype(np.float32)


def case_a():
    """40x24: a 3x2 tile grid with partial tiles on both edges, P = 300.  One splat covers the whole grid; the generator's own
    Gaussians behind the camera and five small ones far off screen have radius 0; a hundred small faint splats (opacity 0.005 .. 0.02: alpha reaches
    1/255 within ~1.4 sigma, the rectangle spans 3 sigma) own tiles they cannot reach, which the default binning culls."""
    s = random_gaussians(300, seed=301, W=40, H=24)
    rng = np.random.default_rng(302)
    _place(s, np.array([20]), np.array([19.0]), np.array([11.0]), np.array([2.0]))
    s["scales"][20] = 0.5
    s["opacities"][20] = 0.3
    off = np.arange(30, 35)
    _place(s, off, np.full(5, -200.0), rng.uniform(1, 23, 5), np.full(5, 5.0))
    s["scales"][off] = 1e-3
    faint = np.arange(100, 200)
    _place(s, faint, rng.uniform(1, 39, 100), rng.uniform(1, 23, 100), rng.uniform(2.0, 5.0, 100))
    s["scales"][faint] = (np.exp(rng.uniform(-4.2, -3.6, (100, 3)))).astype(np.float32)
    s["opacities"][faint, 0] = rng.uniform(0.005, 0.02, 100).astype(np.float32)
    return s


def case_b():
    """32x32 with 601 small splats in tile (0, 0): the tile's list takes two staging rounds of 512, and the waves' last groups hold
    fewer than four splats (the padding of the kernel's drain)."""
    s = random_gaussians(601, seed=311, W=32, H=32)
    rng = np.random.default_rng(312)
    _place(s, np.arange(601), rng.uniform(4, 11, 601), rng.uniform(4, 11, 601), rng.uniform(1.0, 6.0, 601))
    s["scales"][:] = 1e-4
    s["opacities"][:, 0] = rng.uniform(0.01, 0.08, 601).astype(np.float32)
    return s


def case_c():
    """tests/test_raster_gpu.py's (11, 400, 70, 45, scale=(-3, -1)): large splats over every tile."""
    return random_gaussians(400, seed=11, W=70, H=45, scale=(-3.0, -1.0))


def case_config1():
    return random_gaussians(5000, seed=12, W=256, H=256, scale=(-5.0, -3.0))


CASES = {"A": case_a, "B": case_b, "C": case_c}


def image_grads(s, seed, depth=True):
    rng = np.random.default_rng(seed)
    dcol = rng.normal(size=(3, s["H"], s["W"])).astype(np.float32)
    ddep = (rng.normal(size=(1, s["H"], s["W"])) * 0.2).astype(np.float32) if depth else None
    return dcol, ddep


def rects(means2D, radii, W, H):
    """getRect (auxiliary.h:46-56) in float32, as the projection evaluates it: (x0, y0, x1, y1) per Gaussian, empty for radius 0."""
    gx, gy = (W + 15) // 16, (H + 15) // 16
    r = radii.astype(np.float32)
    px, py = means2D[:, 0].astype(np.float32), means2D[:, 1].astype(np.float32)
    f = lambda v, hi: np.clip(np.trunc(v / np.float32(16)).astype(np.int64), 0, hi)
    x0, y0 = f(px - r, gx), f(py - r, gy)
    up = lambda v: (v + r + np.float32(16)) - np.float32(1)          # px + max_radius + BLOCK - 1, left to right in float32
    x1, y1 = f(up(px), gx), f(up(py), gy)
    dead = radii <= 0
    for v in (x0, y0, x1, y1):
        v[dead] = 0
    return x0, y0, x1, y1


def instances(fw, W):
    """{(Gaussian, tile)} of a decoded forward's tile lists."""
    out = set()
    for tile, (b, e) in enumerate(fw["ranges"]):
        out.update((int(g), tile) for g in fw["point_list"][b:e])
    return out


# ---- the ordered backward through the C ABI --------------------------------------------------------------------------------------
def ordered_backward(fw, dL_dcolor, dL_ddepth=None, fresh_fill=None, claim=None):
    """Plan + mom_raster_backward_render_ordered + mom_raster_backward_geometry on hip_helpers.hip_forward's state, every output in
    fresh buffers (the partials pre-filled with the byte `fresh_fill` if given: the call must clear them itself).  Returns the eight
    gradient tensors (hip_backward's names) and "slot_base", "partials", "gacc", "status", "slots".  claim: the slot count handed to
    the backward instead of the plan's own (a smaller one: the bounds guard's case); "tail" is then what lies behind the claimed slots
    in a buffer that was filled with the byte 0x5A."""
    import torch
    from hip_helpers import N, RC, t, _aligned
    lib, stream = N.lib(), N.current_stream()
    (bg, means3D, colors, opacity, scales, rotations, scale_modifier, cov3D_precomp, viewmatrix, projmatrix, tanx, tany, H, W,
     sh, degree, campos, _, debug) = fw["args"]
    geom, binning, img = fw["bufs"]
    P = means3D.shape[0]
    M = int(sh.shape[1]) if sh.numel() else 0
    RC.set_keep_all_tiles(fw["keep_all_tiles"])
    try:
        a, keep = RC._args(bg, means3D, colors, means3D.new_ones((1,)), scales, rotations, scale_modifier, cov3D_precomp, viewmatrix,
                           projmatrix, tanx, tany, H, W, sh, degree, campos, False, debug)
    finally:
        RC.set_keep_all_tiles(False)
    u8 = lambda n: torch.empty(n, dtype=torch.uint8, device="cuda")
    plan = u8(lib.mom_raster_ordered_plan_bytes(P))
    total = torch.full((1,), -1, dtype=torch.int32).pin_memory()
    total_dev = torch.zeros(1, dtype=torch.int32, device="cuda")
    N.check(lib.mom_raster_ordered_plan(C.byref(a), geom.data_ptr(), plan.data_ptr(), total_dev.data_ptr(), total.data_ptr(), stream), "plan")
    torch.cuda.synchronize()
    slots = int(total[0]) & 0xFFFFFFFF
    assert slots == int(total_dev.item()) & 0xFFFFFFFF
    if claim is not None:
        assert claim <= slots
        slots, fresh_fill = claim, 0x5A
    need = lib.mom_raster_ordered_bytes(P, slots)
    assert need >= slots * 160
    part = u8(need + 4096)
    if fresh_fill is not None:
        part.fill_(fresh_fill)
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    dcol = t(dL_dcolor)
    ddep = None if dL_ddepth is None else t(dL_ddepth)
    radii = t(fw["radii"])
    N.check(lib.mom_raster_backward_render_ordered(C.byref(a), geom.data_ptr(), binning.data_ptr(), int(fw["R"]), img.data_ptr(),
                                                   dcol.data_ptr(), None if ddep is None else ddep.data_ptr(), plan.data_ptr(),
                                                   part.data_ptr(), part.numel(), slots, status.data_ptr(), stream), "render_ordered")
    torch.cuda.synchronize()
    lay = N.MomRasterLayout()
    lib.mom_raster_layout(P, W, H, int(fw["R"]), C.byref(lay))
    gf = N.GACC_FLOATS
    out = {"slots": slots, "status": int(status.item())}
    out["gacc"] = _aligned(geom)[lay.geom_gacc:lay.geom_gacc + P * gf * 4].cpu().numpy().view(np.float32).reshape(P, gf).copy()
    out["slot_base"] = _aligned(plan)[:(P + 1) * 4].cpu().numpy().view(np.uint32).copy()
    out["partials"] = _aligned(part)[:slots * 160].cpu().numpy().view(np.float32).reshape(slots, WAVES, VALUES).copy()
    out["tail"] = _aligned(part)[slots * 160:].cpu().numpy().copy()
    f = dict(dtype=torch.float32, device="cuda")
    res = dict(dL_dmeans2D=torch.empty(P, 3, **f), dL_dcolors=torch.empty(P, 3, **f), dL_dopacity=torch.empty(P, 1, **f),
               dL_dmeans3D=torch.empty(P, 3, **f), dL_dcov3D=torch.empty(P, 6, **f), dL_dsh=torch.empty(P, M, 3, **f),
               dL_dscales=torch.empty(P, 3, **f), dL_drotations=torch.empty(P, 4, **f))
    g = N.MomRasterGrads()
    for k, v in res.items():
        setattr(g, k, v.data_ptr())
    N.check(lib.mom_raster_backward_geometry(C.byref(a), radii.data_ptr(), geom.data_ptr(), C.byref(g), stream), "geometry")
    torch.cuda.synchronize()
    del keep
    out.update({k: v.cpu().numpy() for k, v in res.items()})
    return out
