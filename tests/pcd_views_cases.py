"""What the multi-view point-cloud render tests share: fixture g18 (the reference's own render_PCD run on two small scenes,
tools/gen_pcd_views_golden.py) and the float64 numpy restatement of include/mom4d.h's mom_tri_resample and mom_pcd_compose,
operation for operation.  numpy evaluates every ufunc as one IEEE operation (no contraction), so the kernels, which are float64 with
contraction off and the same order of operations, are held to these BIT FOR BIT.  Needs neither scipy nor the GPU."""
import functools
import importlib
import os
from types import SimpleNamespace

import numpy as np

pkg = "iclr2025_3d-mom_amd"
N = importlib.import_module(pkg + "._native")
motion = importlib.import_module(pkg + ".motion")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g18_pcd_views.npz")
CASES = ("s", "l")                       # 40 x 48 and 80 x 96
EPS = 100.0 * 2.0 ** -52                 # LinearNDInterpolator's eps
GROW = N.TRI_BOX_GROW
LANE_BOX = N.TRI_LANE_BOX
NO_OWNER = np.iinfo(np.int32).max


# ------------------------------------------------------------------------------------------------ mom_tri_resample, restated
def tri_setup(pts, tris, H, W):
    """Per triangle: ok, (a, b, c, d, det, x2, y2) and the grown, clamped box (bx, by, bw, bh) -- load_tri of the kernel."""
    pts, tris = np.asarray(pts, np.float64).reshape(-1, 2), np.asarray(tris, np.int64).reshape(-1, 3)
    n = len(pts)
    ok = ((tris >= 0) & (tris < n)).all(1)
    t = np.where(ok[:, None], tris, 0) if n else np.zeros_like(tris)
    P = pts[t] if n else np.zeros((len(tris), 3, 2))
    with np.errstate(all="ignore"):
        ok &= np.isfinite(P).all((1, 2))
        x0, y0, x1, y1, x2, y2 = P[:, 0, 0], P[:, 0, 1], P[:, 1, 0], P[:, 1, 1], P[:, 2, 0], P[:, 2, 1]
        a, b, c, d = x0 - x2, x1 - x2, y0 - y2, y1 - y2
        det = a * d - b * c
        ok &= (det != 0) & np.isfinite(det)
        xa = np.maximum(np.ceil(np.minimum(np.minimum(x0, x1), x2) - GROW), 0.0)
        xb = np.minimum(np.floor(np.maximum(np.maximum(x0, x1), x2) + GROW), float(W - 1))
        ya = np.maximum(np.ceil(np.minimum(np.minimum(y0, y1), y2) - GROW), 0.0)
        yb = np.minimum(np.floor(np.maximum(np.maximum(y0, y1), y2) + GROW), float(H - 1))
        ok &= (xa <= xb) & (ya <= yb)
    z = lambda v: np.where(ok, v, 0.0)
    bx, by = z(xa).astype(np.int64), z(ya).astype(np.int64)
    bw, bh = np.where(ok, z(xb).astype(np.int64) - bx + 1, 0), np.where(ok, z(yb).astype(np.int64) - by + 1, 0)
    return SimpleNamespace(ok=ok, tris=tris, a=a, b=b, c=c, d=d, det=det, x2=x2, y2=y2, bx=bx, by=by, bw=bw, bh=bh)


def bary(s, t, X, Y):
    """c0, c1, c2 of pixel centres (X, Y) in triangles t, by the header's expressions."""
    with np.errstate(all="ignore"):
        dx, dy = X.astype(np.float64) - s.x2[t], Y.astype(np.float64) - s.y2[t]
        c0 = (s.d[t] * dx - s.b[t] * dy) / s.det[t]
        c1 = (s.a[t] * dy - s.c[t] * dx) / s.det[t]
        c2 = (1.0 - c0) - c1
    return c0, c1, c2


def passes(c0, c1, c2):
    return (c0 >= -EPS) & (c0 <= 1.0 + EPS) & (c1 >= -EPS) & (c1 <= 1.0 + EPS) & (c2 >= -EPS) & (c2 <= 1.0 + EPS)


def candidates(s, whole_image=None):
    """(triangle, X, Y) of every pixel centre in every valid triangle's box; whole_image=(H, W): every pixel for every valid triangle."""
    tri = np.nonzero(s.ok)[0]
    if whole_image is not None:
        H, W = whole_image
        t = np.repeat(tri, H * W)
        k = np.tile(np.arange(H * W), len(tri))
        return t, k % W, k // W
    npix = s.bw[tri] * s.bh[tri]
    t = np.repeat(tri, npix)
    k = np.arange(npix.sum()) - np.repeat(np.cumsum(npix) - npix, npix)
    return t, s.bx[t] + k % s.bw[t], s.by[t] + k // s.bw[t]


def tri_owner(pts, tris, H, W, whole_image=False):
    """owner [H,W]: the lowest-index passing triangle per pixel (NO_OWNER: none), and how many triangles pass per pixel."""
    s = tri_setup(pts, tris, H, W)
    t, X, Y = candidates(s, (H, W) if whole_image else None)
    hit = passes(*bary(s, t, X, Y))
    owner = np.full(H * W, NO_OWNER, np.int64)
    count = np.zeros(H * W, np.int64)
    np.minimum.at(owner, (Y * W + X)[hit], t[hit])
    np.add.at(count, (Y * W + X)[hit], 1)
    return s, owner.reshape(H, W), count.reshape(H, W)


def tri_resample_ref(pts, tris, values, H, W, fill=0.0):
    """One view of mom_tri_resample: [H,W,C] float64."""
    values = np.asarray(values, np.float32)
    s, owner, _ = tri_owner(pts, tris, H, W)
    out = np.full((H, W, values.shape[1]), float(fill), np.float64)
    Y, X = np.nonzero(owner != NO_OWNER)
    t = owner[Y, X]
    c0, c1, c2 = bary(s, t, X, Y)
    v = values.astype(np.float64)[s.tris[t]]                               # [n, 3, C]
    out[Y, X] = ((c0[:, None] * v[:, 0]) + (c1[:, None] * v[:, 1])) + (c2[:, None] * v[:, 2])
    return out


def box_pixels(pts, tris, H, W):
    s = tri_setup(pts, tris, H, W)
    return s.bw * s.bh


# ------------------------------------------------------------------------------------------------ mom_pcd_compose, restated
def window(m, r, maximum):
    """(2r+1)^2 maximum / minimum of an integer map, the window clipped to the image."""
    H, W = m.shape
    pad = np.full((H + 2 * r, W + 2 * r), 0 if maximum else 255, np.int64)
    pad[r:r + H, r:r + W] = m
    out = pad[r:r + H, r:r + W].copy()
    for dy in range(2 * r + 1):
        for dx in range(2 * r + 1):
            w = pad[dy:dy + H, dx:dx + W]
            out = np.maximum(out, w) if maximum else np.minimum(out, w)
    return out


def border_clamp(I):
    """Step 1 in the form the kernel uses: I[clamp(y,1,H-2)][clamp(x,1,W-2)]."""
    H, W = I.shape[:2]
    return I[np.clip(np.arange(H), 1, H - 2)][:, np.clip(np.arange(W), 1, W - 2)]


def border_as_written(I):
    """Step 1 as train_motion.py:215-217,305 writes it."""
    H, W = I.shape[:2]
    edge = np.pad(np.ones((H - 4, W - 4)), ((2, 2), (2, 2)))[..., None]
    return edge * I + (1 - edge) * np.pad(I[1:-1, 1:-1], ((1, 1), (1, 1), (0, 0)), mode="edge")


def to_bytes(x):
    return np.clip(np.rint(x * 255.0), 0.0, 255.0).astype(np.uint8)


def compose_ref(resampled, pts, border=border_clamp):
    """One view of mom_pcd_compose: (image [H,W,3] uint8, mask [H,W] uint8, the float images before the cast)."""
    H, W = resampled.shape[:2]
    I = border(np.asarray(resampled, np.float64))
    hit = np.zeros((H, W), np.int64)
    r = np.rint(np.asarray(pts, np.float64).reshape(-1, 2))
    inside = (r[:, 0] >= 0) & (r[:, 0] <= W - 1) & (r[:, 1] >= 0) & (r[:, 1] <= H - 1)
    hit[r[inside, 1].astype(np.int64), r[inside, 0].astype(np.int64)] = 1
    dil = window(hit, 4, True).astype(np.float64)
    rgb = dil[..., None] * I[..., :3] + (1.0 - dil[..., None]) * (-1.0)
    mj = window((((rgb[..., 0] + rgb[..., 1]) + rgb[..., 2]) != -3.0) * 1, 5, False).astype(np.float64)
    image = mj[..., None] * rgb + (1.0 - mj[..., None]) * 0.0
    m = dil * I[..., 3] + (1.0 - mj) * (-1.0)
    mj2 = window((((m + m) + m) != -3.0) * 1, 5, False).astype(np.float64)
    mask = mj2 * m + (1.0 - mj2) * 0.0
    return to_bytes(image), to_bytes(mask), (image, mask)


# ------------------------------------------------------------------------------------------------ the fixture
@functools.lru_cache(maxsize=None)
def g18():
    return dict(np.load(GOLDEN))


@functools.lru_cache(maxsize=None)
def case(name):
    """One scene of g18 with what the package's host code makes of its inputs: the point cloud and the ViewSet, the fixture's
    triangulation injected."""
    d = g18()
    g = lambda k: d[f"{name}_{k}"]
    depth, K, render, internal = g("depth"), g("K"), g("render_poses"), g("internal_poses")
    H, W = depth.shape
    world, colors, masks = motion.pcd_points(g("image"), g("mask"), depth, K, render[0, :3, :3], render[0, :3, 3:4])
    views, present, none_idx = motion.pcd_views(world, K, motion.compose_slots(render, internal), H, W)
    V = views.V
    assert V == int(g("views")) and present == list(range(V)) and none_idx == list(g("none_idx"))
    for k in range(V):
        assert np.array_equal(views.valid[k], g(f"valid_{k}").astype(np.int64)), k
    views.simplices = [np.ascontiguousarray(g(f"tris_{k}"), dtype=np.int32) for k in range(V)]
    return SimpleNamespace(name=name, H=H, W=W, V=V, K=K, depth=depth, render=render, internal=internal, image=g("image"), mask=g("mask"),
                           hints=[list(map(int, h)) for h in g("hints")], world=world, colors=colors, masks=masks, views=views,
                           values=motion.pcd_values(views, colors, masks), get=g)


@functools.lru_cache(maxsize=None)
def resampled_ref(name):
    """The restatement's [V,H,W,4] of a scene's (r, g, b, m): computed once, shared read-only."""
    c = case(name)
    out = np.stack([tri_resample_ref(c.views.pix64[k].T, c.views.simplices[k], c.values[k], c.H, c.W) for k in range(c.V)])
    out.setflags(write=False)
    return out


def fresh_views(name):
    """A copy of the scene's ViewSet that shares nothing mutable with the cached one (no simplices, nothing uploaded)."""
    v = case(name).views
    return motion.ViewSet(P=v.P, H=v.H, W=v.W, R=v.R, T=v.T, valid=v.valid, pix0=v.pix0, pix64=v.pix64)


def recorded(name):
    """(view, channels, griddata's recorded output [H,W,len(channels)]) for every record the fixture keeps of a scene."""
    c = case(name)
    for k in range(c.V):
        for key, ch in (("rgb", [0, 1, 2]), ("r", [0]), ("m", [3])):
            full = f"{name}_gd_{k}_{key}"
            if full in g18():
                yield k, ch, g18()[full].reshape(c.H, c.W, len(ch))
