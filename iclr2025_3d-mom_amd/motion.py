"""The 3D motion optimisation module's fit: the [3,P] Eulerian scene flow from multi-view 2D flows.

The reference's MotionOptimization.optimize_motion (train_motion.py:65-207) projects a point cloud into 14 x 5 views, samples each
view's estimated 2D flow at the projected points and runs SGD on one [3,P] tensor so that the flowed points' projections move by
those 2D flows.  Its output, MOM/scene_flow.pth, is the prior every deformation field of this package adds to its positions.  Here
the preparation (valid sets, unflowed pixels: float64 numpy, cast as the reference casts) stays on the host and the whole SGD
loop -- every epoch, every view -- is one HIP launch (ops.sceneflow_fit, csrc/sceneflow_fit.hip).  The sampling is the
reference's scipy.interpolate.griddata, one call per view on the host (sampler="griddata", the default), or one HIP launch for all
views (sampler="device": ops.flow_sample, csrc/flow_sample.hip) that needs the pixel grid's triangulation once per image size.

The opposite direction -- values given at a view's projected points, wanted at every pixel centre -- is what the reference's
render_PCD (train_motion.py:211-366: the multi-view renders of the point cloud stage 2 trains on) and the our_flow resampling at
the end of optimize_motion (:196-200) do, again with one griddata per use, each triangulating the same scattered points anew.
Here a view is triangulated once, on host threads (triangulate_views: scipy.spatial.Delaunay, Qhull's own choice where the
triangulation is not unique), the triangulation is kept on the ViewSet for every use, and point location, interpolation, the
border and mask morphology and the 8-bit cast run on the device (ops.tri_resample, ops.pcd_compose, csrc/tri_resample.hip).

    prepare_views      valid sets and unflowed pixels of a list of world-to-camera poses  -> ViewSet
    grid_diagonals     which diagonal griddata's triangulation of an H x W pixel grid puts into every cell (cached)
    sample_flow_images the fit's records from the views' flow images, on the device
    fit_scene_flow     the fit itself, targets given per view at that view's valid points or as device records
    optimize_motion    the reference's function: pose composition, griddata sampling, fit, our_flow
    triangulate_views  one Delaunay triangulation per view of a ViewSet, in a thread pool, cached on the ViewSet
    resample_to_grid   per-view values at the views' points -> [V,H,W,C] on the device
    render_pcd         the reference's render_PCD: the multi-view images and masks of the point cloud
    refit_scene_flow   a stage-1 directory's MOM/train_data.pth -> MOM/scene_flow.pth
    write_pixel_video  MOM/video/%06d.png from the centre frame's image, our_flow and mask by warping pixels (cinemagraph.pixel_video)
    pcd_gen_poses      the reference's 'lookaround' and 'hemisphere' poses (utils/trajectory.py)
    read_json          the hints of a labelme image.json
    hint_arguments     the hints of one frame as the reference's flow step selects them, quirks included
    estimate_flows     the reference's estimate_flow: every frame's T2C_flow, the arithmetic around the estimator on the device
    flow_image         helpmotion.flow2img, the colour-wheel image of a flow
    build_stage1       the reference's train_motion.py main: an input folder -> MOM/train_data.pth, scene_flow.pth, Flow_viz

The networks of stage 1 (the depth network, the 2D flow estimator, the video generator's GAN) are not part of this package: the depth
is an argument, the estimator is a callable of the user's, and each of the other two has a checkpoint-free SUBSTITUTE that is not
the reference's output -- `--flow hints` takes the dense hint field itself as the estimated motion, and `--video pixels` makes the
looping video with the video generator's warp (cinemagraph.py) from the image's pixels instead of StyleGAN features.

    python -m iclr2025_3d-mom_amd.motion --input_dir DIR [--train_iteration N] [--sampler device] [--resampler device]
                                          [--triangulator device]
    python -m iclr2025_3d-mom_amd.motion --input_dir DIR --video pixels [--n_frames 120] [--video_size 1024] [--video-writer device]
    python -m iclr2025_3d-mom_amd.motion --input_dir DIR --build --depth FILE [--flow hints] [--video pixels]
"""
import functools
import os
from concurrent.futures import ThreadPoolExecutor
from dataclasses import dataclass
from typing import List, Optional

import numpy as np
import torch

from . import ops

YZ_REVERSE = np.array([[1, 0, 0], [0, -1, 0], [0, 0, -1]], dtype=np.float64)     # train_motion.py:71


@dataclass
class ViewSet:
    """What the fit needs of V views of P points.  R, T: float32 world-to-camera (train_motion.py:164-165 casts them);
    valid[j]: the indices of view j's valid set, ascending (:173-177); pix0[j]: [2, n_j] float32, the unflowed pixels (:180,183);
    pix64[j]: the same pixels before that cast, as the reference hands them to griddata (:115,120) -- prepare_views fills it.
    simplices[j]: int32 [T_j, 3], view j's Delaunay triangulation (triangulate_views fills and keeps it); packed: what
    upload_views put on a device, kept for the next use on that device; fallbacks: after an upload with the device triangulator
    the (view, status) pairs the device refused and scipy triangulated instead."""
    P: int
    H: int
    W: int
    R: np.ndarray
    T: np.ndarray
    valid: List[np.ndarray]
    pix0: List[np.ndarray]
    pix64: Optional[List[np.ndarray]] = None
    simplices: Optional[List[np.ndarray]] = None
    packed: Optional[dict] = None
    fallbacks: Optional[list] = None

    @property
    def V(self):
        return len(self.valid)


def _pose(p):
    """(R [3,3], T [3,1]) of a pose given as an (R, T) pair or as a 3x4 / 4x4 matrix, dtypes kept."""
    if isinstance(p, (tuple, list)) and len(p) == 2:
        R, T = np.asarray(p[0]), np.asarray(p[1])
    else:
        p = np.asarray(p)
        R, T = p[:3, :3], p[:3, 3:4]
    if R.shape != (3, 3) or T.size != 3:
        raise ValueError(f"a world-to-camera pose is (R [3,3], T [3]) or a 3x4 / 4x4 matrix, got {R.shape} and {T.shape}")
    return R, T.reshape(3, 1)


def _valid_pixels(points, K, R, T, H, W):
    """(valid indices, float64 pixels [2, n]) of one view, by the reference's expressions (train_motion.py:105-115,285-297)."""
    pix = np.matmul(K, R.dot(points) + T)
    with np.errstate(divide="ignore", invalid="ignore"):
        idx = np.where(np.logical_and.reduce((pix[2] > 0, pix[0] / pix[2] >= 0, pix[0] / pix[2] <= W - 1,
                                              pix[1] / pix[2] >= 0, pix[1] / pix[2] <= H - 1)))[0]
    return idx, pix[:2, idx] / pix[-1:, idx]


def _view_set(P, H, W, poses, valid, pix64):
    return ViewSet(P=P, H=int(H), W=int(W), R=np.stack([np.asarray(R, np.float32) for R, _ in poses]),
                   T=np.stack([np.asarray(T, np.float32).reshape(3) for _, T in poses]), valid=valid,
                   pix0=[p.astype(np.float32) for p in pix64], pix64=pix64)


def prepare_views(points, K, w2c_list, H, W):
    """Valid sets and unflowed pixels exactly as train_motion.py:161-183 forms them: numpy in the dtypes given (the reference has
    float32 points and K and float64 poses, so float64 throughout), `z > 0, 0 <= u <= W-1, 0 <= v <= H-1`, pixels cast to
    float32 at the end.  A view without a single valid point raises ValueError: the reference skips such a view in one of its two
    loops only, its lists go out of step and it cannot run either."""
    points = np.asarray(points)
    if points.ndim != 2 or points.shape[0] != 3:
        raise ValueError(f"points must be [3, P], got {points.shape}")
    K = np.asarray(K)
    poses, valid, pix64 = [], [], []
    for j, pose in enumerate(w2c_list):
        R, T = _pose(pose)
        idx, pix = _valid_pixels(points, K, R, T, H, W)
        if len(idx) == 0:
            raise ValueError(f"view {j} sees none of the {points.shape[1]} points")
        poses.append((R, T))
        valid.append(idx)
        pix64.append(pix)
    if not valid:
        raise ValueError("no views")
    return _view_set(points.shape[1], H, W, poses, valid, pix64)


def learning_rates(epochs, lr=0.5, gamma=0.97):
    """lr of every epoch as SGD + ExponentialLR hold it (train_motion.py:128-130,203): one multiplication per epoch, in Python
    floats; the optimiser rounds it to float32 when it is used."""
    out, cur = [], float(lr)
    for _ in range(epochs):
        out.append(cur)
        cur = cur * gamma
    return np.asarray(out, dtype=np.float32)


def view_weights(views, divisor):
    """w_j = (1 / divisor) / (2 n_j) in float32, in the order autograd forms it: the division of the summed loss by idx + 1,
    then the mean over the view's 2 n_j entries."""
    inv = np.float32(1.0) / np.float32(divisor)
    return np.asarray([inv / np.float32(2 * len(v)) for v in views.valid], dtype=np.float32)


def valid_words(views):
    """valid [ceil(V/32),P] int32 bit words: bit j % 32 of word [j // 32, p] = point p is in view j's valid set."""
    bits = np.zeros(((views.V + 31) // 32, views.P), np.uint32)
    for j, idx in enumerate(views.valid):
        bits[j // 32, idx] |= np.uint32(1 << (j % 32))
    return bits.view(np.int32)


def _upload(a, dev):
    """An array or CPU tensor on `dev`.  To a GPU it goes through pinned memory and an asynchronous copy on the current stream, so
    that preparing a fit only enqueues (a copy from pageable memory makes the host wait for the stream)."""
    t = a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))
    return t.pin_memory().to(dev, non_blocking=True) if dev.type == "cuda" and not t.is_cuda else t.to(dev)


def pack_views(views, gt):
    """records [V,P,4] float32 = {pix0, gt} and valid [ceil(V/32),P] int32 bit words, on the host."""
    V, P = views.V, views.P
    if len(gt) != V:
        raise ValueError(f"{len(gt)} targets for {V} views")
    rec = np.zeros((V, P, 4), np.float32)
    for j in range(V):
        g = gt[j].detach().cpu().numpy() if torch.is_tensor(gt[j]) else np.asarray(gt[j])
        idx = views.valid[j]
        if g.shape != (2, len(idx)):
            raise ValueError(f"the target of view {j} must be [2, {len(idx)}] (one column per valid point), got {g.shape}")
        rec[j, idx, 0:2] = views.pix0[j].T
        rec[j, idx, 2:4] = g.T.astype(np.float32)
    return rec, valid_words(views)


def fit_scene_flow(points, K, views, gt, epochs=200, lr=0.5, gamma=0.97, divisor=None, device=None, records=None):
    """The fit (train_motion.py:125-207).  points [3,P]; K 3x3; views: a ViewSet of the same points; gt: per view a [2, n_j]
    array or tensor, the 2D flow at that view's valid points (the reference's GT_list); divisor: the reference's idx + 1 (:189),
    one more than the slot index of the last view that has a flow -- the number of views when none was skipped, the default.
    records: in place of gt (then None), what sample_flow_images returned -- (records [V,P,4], valid words) already on the device:
    nothing is packed or uploaded for them; the view weights still come from the host's valid counts.
    Returns (flow [3,P], loss [E], flow2d_last [V,P,2]) on the device: the scene flow, every epoch's loss, and the last epoch's
    2D flow of every point in every view (0 where the point is not in the view's valid set).  Everything is enqueued on the current
    stream; nothing is read back."""
    dev = torch.device("cuda" if device is None else device)
    pts = np.ascontiguousarray(np.asarray(points.detach().cpu() if torch.is_tensor(points) else points), dtype=np.float32)
    if pts.shape != (3, views.P):
        raise ValueError(f"points must be [3, {views.P}] like the views', got {pts.shape}")
    if epochs < 0:
        raise ValueError("epochs must not be negative")
    up = lambda a: _upload(a, dev)
    if records is not None:
        if gt is not None:
            raise ValueError("give the targets as gt (per view, on the host) or as records (on the device), not both")
        rec, bits = records
    else:
        rec, bits = (up(a) for a in pack_views(views, gt))
    w = view_weights(views, views.V if divisor is None else divisor)
    K_host = np.asarray(K.detach().cpu() if torch.is_tensor(K) else K, dtype=np.float32)
    V, P = views.V, views.P
    flow = torch.zeros((3, P), dtype=torch.float32, device=dev)
    loss = torch.zeros(epochs, dtype=torch.float32, device=dev)
    flow2d = torch.zeros((V, P, 2), dtype=torch.float32, device=dev)
    ops.sceneflow_fit(up(pts), K_host, up(views.R), up(views.T), up(w), rec, bits, up(learning_rates(epochs, lr, gamma)),
                      flow, loss, flow2d)
    return flow, loss, flow2d


def _griddata():
    try:
        from scipy.interpolate import griddata
    except ImportError as e:
        raise ImportError("optimize_motion samples the 2D flow images with scipy.interpolate.griddata (train_motion.py:22,120,198): "
                          "scipy is needed for it and for refit_scene_flow; fit_scene_flow takes already sampled targets") from e
    return griddata


def _pixel_grid(H, W):
    x, y = np.meshgrid(np.arange(W, dtype=np.float32), np.arange(H, dtype=np.float32), indexing="xy")    # train_motion.py:87-88
    return np.stack((x, y), axis=-1).reshape(-1, 2)


def sample_flow_image(flow_image, pix0, H, W):
    """A [1,2,H,W] flow image at the pixels pix0 [2,n] (train_motion.py:117-121): linear griddata over the pixel grid, 0 outside."""
    g = torch.as_tensor(flow_image).permute(2, 3, 1, 0).squeeze().reshape(H * W, 2).cpu().clone().numpy()
    return _griddata()(_pixel_grid(H, W), g, np.asarray(pix0).transpose(1, 0), method="linear", fill_value=0).T


@functools.lru_cache(maxsize=None)
def grid_diagonals(H, W):
    """bool [H-1, W-1], True where the anti-diagonal (x+1, y)-(x, y+1) splits cell (x, y) of griddata's triangulation of the H x W
    pixel grid and False where the main diagonal (x, y)-(x+1, y+1) does: scipy.spatial.Delaunay over exactly the points griddata is
    given, read simplex by simplex.  The choice is Qhull's and irregular, but it depends on (H, W) alone, so the result is kept per
    (H, W) for the life of the process (read-only).  Raises RuntimeError unless the triangulation is two triangles per cell with
    one diagonal in every cell -- a Qhull that answers differently must not pass silently."""
    H, W = int(H), int(W)
    if H < 2 or W < 2:
        raise ValueError(f"a pixel grid needs at least one cell (H, W >= 2), got H {H}, W {W}")
    try:
        from scipy.spatial import Delaunay
    except ImportError as e:
        raise ImportError("grid_diagonals reads the cell diagonals out of scipy.spatial.Delaunay: scipy is needed for it; "
                          "sample_flow_images also takes an explicit mask") from e
    s = np.asarray(Delaunay(_pixel_grid(H, W)).simplices, dtype=np.int64)
    cells = (H - 1) * (W - 1)
    if s.shape != (2 * cells, 3):
        raise RuntimeError(f"the triangulation of the {H} x {W} pixel grid has {s.shape[0]} triangles, not two per cell ({2 * cells})")
    xs, ys = s % W, s // W
    x0, y0 = xs.min(1), ys.min(1)
    if (xs.max(1) - x0 != 1).any() or (ys.max(1) - y0 != 1).any():
        raise RuntimeError(f"the triangulation of the {H} x {W} pixel grid has a triangle that is not half of one cell")
    # corner k = dx + 2 dy of the cell; a triangle is the cell without one corner: without 0 or 3 it lies on the anti-diagonal
    missing = 15 - (1 << ((xs - x0[:, None]) + 2 * (ys - y0[:, None]))).sum(1)
    cell = y0 * (W - 1) + x0
    count = np.bincount(cell, minlength=cells)
    halves = np.bincount(cell, weights=missing, minlength=cells).astype(np.int64)
    if not np.isin(missing, (1, 2, 4, 8)).all() or (count != 2).any() or not np.isin(halves, (1 + 8, 2 + 4)).all():
        raise RuntimeError(f"the triangulation of the {H} x {W} pixel grid does not split every cell by exactly one diagonal")
    mask = (halves == 1 + 8).reshape(H - 1, W - 1)
    mask.setflags(write=False)
    return mask


def pack_diagonals(mask):
    """The mask of grid_diagonals as ops.flow_sample's bit words: int32 [ceil(cells / 32)], bit c % 32 of word c // 32 for the
    cell c = y (W-1) + x."""
    b = np.packbits(np.asarray(mask, dtype=bool).reshape(-1), bitorder="little")
    words = np.zeros((b.size + 3) // 4 * 4, np.uint8)
    words[:b.size] = b
    return words.view("<u4").astype(np.uint32).view(np.int32)


def sample_flow_images(views, flow_images, diagonals=None, device=None):
    """The fit's records on the device: (records [V,P,4] float32 = {pix0, gt}, valid [ceil(V/32),P] int32 bit words), gt being
    view j's flow image sampled at its valid points as sample_flow_image does, to float64 rounding, for all views in one launch
    (ops.flow_sample).  views: a ViewSet of prepare_views (it carries the float64 pixels); flow_images: per view a [1,2,H,W]
    tensor or array, or one [V,2,H,W] tensor; they are read as float32, which the stage-1 flow images are.
    diagonals: the bool [H-1, W-1] mask of the cells the anti-diagonal splits; None means grid_diagonals(H, W), which needs scipy.
    A caller without scipy can pass a mask of its own (all False, say) and still run, knowing that in every cell whose diagonal is
    not griddata's the result then leaves the reference by up to the cell's mixed second difference f00 - f10 - f01 + f11 (times
    min(fx, fy, 1-fx, 1-fy) <= 1/2) -- on a noisy flow image that is the scale of the image itself.
    Uploads the dense float64 pixels ([V,P,2], 16 bytes per pair) and the bit words; nothing is read back."""
    dev = torch.device("cuda" if device is None else device)
    V, P, H, W = views.V, views.P, views.H, views.W
    if views.pix64 is None:
        raise ValueError("the ViewSet carries no float64 pixels (pix64): build it with prepare_views")
    if torch.is_tensor(flow_images) and flow_images.dim() == 4:
        images = flow_images
    else:
        images = torch.cat([torch.as_tensor(f).reshape(1, 2, H, W) for f in flow_images])
    if tuple(images.shape) != (V, 2, H, W):
        raise ValueError(f"{V} views of {H} x {W} pixels need flow images [{V}, 2, {H}, {W}], got {tuple(images.shape)}")
    mask = grid_diagonals(H, W) if diagonals is None else np.asarray(diagonals)
    if mask.shape != (H - 1, W - 1):
        raise ValueError(f"diagonals must be [{H - 1}, {W - 1}], one entry per cell, got {mask.shape}")
    pix = np.zeros((V, P, 2), np.float64)
    for j, idx in enumerate(views.valid):
        pix[j, idx] = views.pix64[j].T
    up = lambda a: _upload(a, dev)
    bits = up(valid_words(views))
    return ops.flow_sample(up(images.detach().to(torch.float32).contiguous()), up(pix), bits, up(pack_diagonals(mask))), bits


SAMPLERS = ("griddata", "device")
RESAMPLERS = ("griddata", "device")
TRIANGULATORS = ("host", "device")
MAX_WORKERS = 16
DELAUNAY_SCRATCH_BYTES = 1 << 30          # the device triangulator takes the views in chunks whose scratch stays below this


def _triangulator(triangulator):
    """The switch, checked: None means "host"."""
    triangulator = "host" if triangulator is None else triangulator
    if triangulator not in TRIANGULATORS:
        raise ValueError(f"triangulator must be one of {TRIANGULATORS}, got {triangulator!r}")
    return triangulator


def triangulate_views(views, workers=8, triangulator="host"):
    """Per view of a ViewSet the simplices of scipy.spatial.Delaunay over pix64[j].T -- exactly the points, and the Qhull options,
    griddata triangulates (train_motion.py:198,304,319) -- as int32 [T_j, 3], in a pool of `workers` threads (Qhull releases the
    GIL; at most 16, never sized by the machine).  The list is kept on the ViewSet: every later consumer of the same views
    (render_pcd, optimize_motion's our_flow, resample_to_grid) finds it there.  A view with fewer than 3 valid points, or one
    Qhull rejects (collinear points, say), raises ValueError naming the view.
    triangulator="device": the views are uploaded and triangulated there (upload_views; ops.delaunay, csrc/delaunay.hip) and the
    list is what comes back: the same triangles in the canonical order of include/mom4d.h, scipy's own for a view the device refused."""
    triangulator = _triangulator(triangulator)
    if views.simplices is not None:
        return views.simplices
    if views.pix64 is None:
        raise ValueError("the ViewSet carries no float64 pixels (pix64): build it with prepare_views")
    if triangulator == "device":
        pk = upload_views(views, workers=workers, triangulator="device")
        tris, off = pk["tris"].cpu().numpy(), pk["tri_off"].cpu().numpy()
        views.simplices = [np.ascontiguousarray(tris[off[j]:off[j + 1]]) for j in range(views.V)]
        return views.simplices
    views.simplices = _qhull_views(views, range(views.V), workers)
    return views.simplices


def _qhull_views(views, which, workers):
    """scipy.spatial.Delaunay's simplices of the views `which`, in the thread pool."""
    which = list(which)
    try:
        from scipy.spatial import Delaunay, QhullError
    except ImportError as e:
        raise ImportError("triangulate_views triangulates each view's pixels with scipy.spatial.Delaunay: scipy is needed for it; "
                          "a ViewSet whose `simplices` are already filled in needs none") from e

    def one(j):
        pts = np.ascontiguousarray(views.pix64[j].T, dtype=np.float64)
        if pts.shape[0] < 3:
            raise ValueError(f"view {j} has {pts.shape[0]} valid points: a triangulation needs at least 3")
        try:
            return np.ascontiguousarray(Delaunay(pts).simplices, dtype=np.int32)
        except QhullError as e:
            raise ValueError(f"view {j}: Qhull cannot triangulate its {pts.shape[0]} points ({str(e).strip().splitlines()[0]})") from e

    workers = max(1, min(int(workers), MAX_WORKERS, len(which)))
    if workers == 1:
        return [one(j) for j in which]
    with ThreadPoolExecutor(max_workers=workers) as pool:
        return list(pool.map(one, which))


def _delaunay_chunks(counts, H, W):
    """Runs of views [j0, j1) whose ops.delaunay scratch stays below DELAUNAY_SCRATCH_BYTES (a run has at least one view)."""
    runs, j0, n = [], 0, 0
    for j, c in enumerate(counts):
        if j > j0 and 4 * ops.delaunay_scratch_elements(j + 1 - j0, H, W, n + c) > DELAUNAY_SCRATCH_BYTES:
            runs.append((j0, j))
            j0, n = j, 0
        n += c
    return runs + [(j0, len(counts))]


def _device_triangulation(views, pts, counts, dev, workers):
    """(tris [T,3] int32, tri_off [V+1] int32) on the device for points already there: ops.delaunay per chunk of views, only status
    and tri_off read back; a view the device refuses is triangulated by scipy and spliced in (views.fallbacks names it)."""
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    parts, fallbacks = [None] * views.V, []
    for j0, j1 in _delaunay_chunks(counts, views.H, views.W):
        local = _upload((off[j0:j1 + 1] - off[j0]).astype(np.int32), dev)
        tris, tri_off_dev, status = ops.delaunay(pts[off[j0]:off[j1]], local, views.H, views.W)
        tri_off, status = tri_off_dev.cpu().numpy(), status.cpu().numpy()
        for j in range(j0, j1):
            st = int(status[j - j0])
            if st == ops.N.DELAUNAY_FEW:
                raise ValueError(f"view {j} has {counts[j]} valid points: a triangulation needs at least 3")
            if st != ops.N.DELAUNAY_OK:
                fallbacks.append((j, st))
            else:
                parts[j] = tris[tri_off[j - j0]:tri_off[j - j0 + 1]]
        if j0 == 0 and j1 == views.V and not fallbacks:
            views.fallbacks = []
            return tris[:tri_off[-1]], tri_off_dev
    for (j, _), t in zip(fallbacks, _qhull_views(views, [j for j, _ in fallbacks], workers)):
        parts[j] = _upload(t.astype(np.int32).reshape(-1, 3), dev)
    views.fallbacks = fallbacks
    return torch.cat(parts).contiguous(), _upload(_offsets([len(t) for t in parts]), dev)


def _offsets(counts):
    off = np.zeros(len(counts) + 1, np.int64)
    np.cumsum(counts, out=off[1:])
    if off[-1] > np.iinfo(np.int32).max:
        raise ValueError(f"{off[-1]} rows in all: more than an int32 offset holds")
    return off.astype(np.int32)


def upload_views(views, device=None, workers=8, triangulator="host"):
    """What ops.tri_resample and ops.pcd_compose read of a ViewSet, on the device: pts [N,2] float64 (the views' pixels
    concatenated), pt_off, tris [T,3] int32, tri_off, and `gather` [N] int64 = j P + valid[j], the rows of a dense [V,P,C] tensor in
    that order.  Triangulates first when the ViewSet has no simplices yet; kept on the ViewSet per device.
    triangulator="device" (and no simplices yet): the points are uploaded, ops.delaunay triangulates them there and only its status
    and tri_off are read back; a view with fewer than 3 points raises as on the host route, a view the device refuses for any other
    reason (an exact grid, say) is triangulated by scipy in the thread pool and listed in views.fallbacks with its status.  Without
    such a view scipy is not needed.  views.simplices stays empty until triangulate_views is asked for it."""
    triangulator = _triangulator(triangulator)
    dev = torch.device("cuda" if device is None else device)
    if views.packed is not None and views.packed["device"] == dev:
        return views.packed
    up = lambda a: _upload(a, dev)
    if triangulator == "device" and views.simplices is None:
        if views.pix64 is None:
            raise ValueError("the ViewSet carries no float64 pixels (pix64): build it with prepare_views")
        counts = [len(v) for v in views.valid]
        pts = up(np.concatenate([p.T for p in views.pix64]).astype(np.float64))
        tris, tri_off = _device_triangulation(views, pts, counts, dev, workers)
        views.packed = dict(device=dev, pts=pts, pt_off=up(_offsets(counts)), tris=tris, tri_off=tri_off,
                            gather=up(np.concatenate([j * views.P + np.asarray(v, np.int64) for j, v in enumerate(views.valid)])))
        return views.packed
    tris = triangulate_views(views, workers)
    views.packed = dict(device=dev,
                        pts=up(np.concatenate([p.T for p in views.pix64]).astype(np.float64)),
                        pt_off=up(_offsets([len(v) for v in views.valid])),
                        tris=up(np.concatenate(tris).astype(np.int32).reshape(-1, 3)),
                        tri_off=up(_offsets([len(t) for t in tris])),
                        gather=up(np.concatenate([j * views.P + np.asarray(v, np.int64) for j, v in enumerate(views.valid)])))
    return views.packed


def upload_values(views, values, device=None):
    """Per-view [n_j, C] arrays or tensors, one row per valid point -> one [N, C] float32 tensor on the device, in the views' order."""
    dev = torch.device("cuda" if device is None else device)
    if len(values) != views.V:
        raise ValueError(f"{len(values)} value arrays for {views.V} views")
    rows = [np.asarray(v.detach().cpu() if torch.is_tensor(v) else v, dtype=np.float32) for v in values]
    for j, r in enumerate(rows):
        if r.ndim != 2 or r.shape[0] != len(views.valid[j]) or r.shape[1] != rows[0].shape[1]:
            raise ValueError(f"the values of view {j} must be [{len(views.valid[j])}, C] (one row per valid point), got {r.shape}")
    return _upload(np.concatenate(rows), dev)


def resample_to_grid(views, values, fill=0.0, device=None, workers=8, triangulator="host"):
    """Values given at every view's valid points, linearly interpolated at every pixel centre: what
    griddata(pix64[j].T, values[j], pixel grid, method="linear", fill_value=fill) gives per view, for all views in one call of
    ops.tri_resample.  values: per view an [n_j, C] array or tensor (read as float32), what upload_values made of such a list, or
    one dense [V,P,C] device tensor such as fit_scene_flow's flow2d, whose valid rows are gathered on the device.  Returns
    [V,H,W,C] float64 on the device; with the views uploaded (upload_views) and the values on the device it only enqueues.
    triangulator: where views that are not uploaded yet are triangulated (upload_views)."""
    dev = torch.device("cuda" if device is None else device)
    pk = upload_views(views, dev, workers, triangulator)
    if torch.is_tensor(values) and values.dim() == 3:
        if values.shape[:2] != (views.V, views.P):
            raise ValueError(f"dense values must be [{views.V}, {views.P}, C], got {tuple(values.shape)}")
        vals = values.to(dev).reshape(views.V * views.P, -1).index_select(0, pk["gather"]).to(torch.float32).contiguous()
    elif torch.is_tensor(values) and values.is_cuda:
        vals = values                                   # [N, C] on the device already, in the views' order (upload_values)
    else:
        vals = upload_values(views, values, dev)
    return ops.tri_resample(pk["pts"], pk["pt_off"], pk["tris"], pk["tri_off"], vals, views.H, views.W, fill=fill)


def compose_slots(render_poses, internal_poses):
    """View slot i * len(internal) + j -> (Rw2j, Tw2j) = internal[j] o render[i] (train_motion.py:91-97,271-277)."""
    render_poses, internal_poses = np.asarray(render_poses), np.asarray(internal_poses)
    slots = []
    for i in range(len(render_poses)):
        for j in range(len(internal_poses)):
            Rw2i, Tw2i = render_poses[i, :3, :3], render_poses[i, :3, 3:4]
            Ri2j, Ti2j = internal_poses[j, :3, :3], internal_poses[j, :3, 3:4]
            slots.append((np.matmul(Ri2j, Rw2i), np.matmul(Ri2j, Tw2i) + Ti2j))
    return slots


def pcd_points(src_img, src_mask, depth, K, R0, T0):
    """The point cloud render_PCD makes of the source image (train_motion.py:213-226): every pixel unprojected with inv(K) and its
    depth and moved by the inverse of the first render pose, cast to float32; colours and (three equal) mask colours in [0, 1]."""
    mask3 = np.repeat(np.array(src_mask)[..., np.newaxis], 3, axis=-1).astype(np.uint8)
    H, W = depth.shape
    x, y = np.meshgrid(np.arange(W, dtype=np.float32), np.arange(H, dtype=np.float32), indexing="xy")
    cam = np.matmul(np.linalg.inv(K), np.stack((x * depth, y * depth, 1 * depth), axis=0).reshape(3, -1))
    world = (np.linalg.inv(R0).dot(cam) - np.linalg.inv(R0).dot(T0)).astype(np.float32)
    return world, np.array(src_img).reshape(-1, 3).astype(np.float32) / 255., mask3.reshape(-1, 3).astype(np.float32) / 255.


def _hint_points(xs, ys, depth, K, R0, T0):
    """A list of hint pixels in world space (train_motion.py:228-247), with the reference's swapped [h_y, h_x, 1] as written."""
    out = []
    for h_x, h_y in zip(xs, ys):
        cam = np.linalg.inv(K).dot(np.array([[h_y], [h_x], [1]]) * depth[h_y, h_x])
        out.append((np.linalg.inv(R0).dot(cam) - np.linalg.inv(R0).dot(T0)).astype(np.float32))
    return out


def _project_hints(hints, K, R, T):
    """(:338-352): the first pixel coordinate goes to the `y` list and the second to the `x` list, as the reference has it."""
    first, second = [], []
    for h in hints:
        pix = np.matmul(K, R.dot(h) + T)
        pix /= pix[2]
        first.append(pix[0])
        second.append(pix[1])
    return second, first


def pcd_views(points, K, slots, H, W):
    """(ViewSet of the slots that see a point, their slot indices, none_idx) (train_motion.py:285-297)."""
    poses, valid, pix64, present, none_idx = [], [], [], [], []
    for idx, (R, T) in enumerate(slots):
        v, pix = _valid_pixels(points, K, R, T, H, W)
        if len(v) == 0:
            none_idx.append(idx)
            continue
        poses.append((R, T))
        valid.append(v)
        pix64.append(pix)
        present.append(idx)
    if not present:
        raise ValueError("no view sees a point of the cloud")
    return _view_set(points.shape[1], H, W, poses, valid, pix64), present, none_idx


def pcd_values(views, colors, mask_colors):
    """Per view the [n_j, 4] float32 rows (r, g, b, m) of its valid points; mask_colors [P] or [P,3] (three equal channels: one is kept)."""
    colors, mask_colors = np.asarray(colors, np.float32), np.asarray(mask_colors, np.float32)
    rgbm = np.concatenate([colors, (mask_colors if mask_colors.ndim == 1 else mask_colors[:, 0])[:, None]], axis=1)
    return [rgbm[v] for v in views.valid]


def render_pcd_device(views, values, device=None, workers=8, triangulator="host"):
    """The device part of render_pcd: (image [V,H,W,3], mask [V,H,W]) uint8 on the device for a ViewSet of the point cloud and its
    (r, g, b, m) values (pcd_values, or what upload_values made of them).  One tri_resample and one pcd_compose: eight launches for
    all views; with the views and the values uploaded it only enqueues."""
    dev = torch.device("cuda" if device is None else device)
    pk = upload_views(views, dev, workers, triangulator)
    return ops.pcd_compose(resample_to_grid(views, values, fill=0.0, device=dev), pk["pts"], pk["pt_off"])


def render_pcd(src_img, src_mask, depth, hints, render_poses, internal_poses, device=None, workers=8, K=None, triangulator="host"):
    """MotionOptimization.render_PCD (train_motion.py:211-366): the renders of the source image's point cloud from
    len(render_poses) x len(internal_poses) views, which stage 2 trains on.  src_img, src_mask: PIL images (or arrays) of one size;
    depth [H,W]: the source depth (the reference's self.src_depth; the depth network is not part of this package); hints: four lists
    (start x, start y, end x, end y); the poses are arguments as in optimize_motion; K: the intrinsics, by default the
    reference's (stage1_intrinsics).  Everything that is not per-pixel work follows the reference on the host in its dtypes; each
    view is triangulated once (triangulate_views, `workers` threads) and the resampling, the border, the mask morphology and the
    8-bit cast run on the device for all views at once (render_pcd_device).  The reference's depth image (:307-308) is never used
    and is not computed.  Returns (train_data, none_idx) in the reference's layout (:251-260,354-364): `image` and `mask` are PIL
    images, T2C_flow and our_flow empty lists; a slot that sees no point is in none_idx and has no frame.
    triangulator: "host" (scipy, `workers` threads) or "device" (upload_views: ops.delaunay, scipy only for a view it refuses)."""
    from PIL import Image
    triangulator = _triangulator(triangulator)
    depth = np.asarray(depth)
    H, W = depth.shape
    if K is None:
        from .scene.dataset_readers import FOCAL
        K, focal = stage1_intrinsics(H, W), (FOCAL * (W / H), FOCAL)
    else:
        K = np.asarray(K)
        focal = (float(K[0, 0]), float(K[1, 1]))
    render_poses = np.asarray(render_poses)
    R0, T0 = render_poses[0, :3, :3], render_poses[0, :3, 3:4]
    world, colors, mask_colors = pcd_points(src_img, src_mask, depth, K, R0, T0)
    starts = _hint_points(hints[0], hints[1], depth, K, R0, T0)
    ends = _hint_points(hints[2], hints[3], depth, K, R0, T0)
    train_data = {"camera_angle_x": 2 * np.arctan(W / (2 * focal[0])), "camera_angle_y": 2 * np.arctan(H / (2 * focal[1])),
                  "W": W, "H": H, "pcd_points": world.copy(), "pcd_colors": colors.copy(), "pcd_masks": mask_colors.copy(), "frames": []}
    slots = compose_slots(render_poses, internal_poses)
    views, present, none_idx = pcd_views(world, K, slots, H, W)
    image, mask = (t.cpu().numpy() for t in render_pcd_device(views, pcd_values(views, colors, mask_colors), device, workers, triangulator))
    for k, idx in enumerate(present):
        R, T = slots[idx]
        sx, sy = _project_hints(starts, K, R, T)
        ex, ey = _project_hints(ends, K, R, T)
        train_data["frames"].append({"image": Image.fromarray(image[k]), "transform_matrix": transform_matrix_from_pose(R, T).tolist(),
                                     "mask": Image.fromarray(mask[k]), "final_hint_start_x": sx, "final_hint_start_y": sy,
                                     "final_hint_end_x": ex, "final_hint_end_y": ey, "T2C_flow": [], "our_flow": []})
    return train_data, none_idx


def _fit_slots(train_data, slots, K, H, W, train_iteration, device=None, sampler="griddata"):
    """slots: per view slot its (R, T) world-to-camera pose, or None for a slot without a flow (the reference's non_frame_idx).
    Frame k of train_data carries the k-th present slot's T2C_flow (train_motion.py:81-85).  sampler: "griddata" samples every
    view's image on the host as the reference does, "device" samples all of them in one launch (sample_flow_images; the returned
    gt is then None)."""
    if sampler not in SAMPLERS:
        raise ValueError(f"sampler must be one of {SAMPLERS}, got {sampler!r}")
    present = [i for i, s in enumerate(slots) if s is not None]
    if not present:
        raise ValueError("no view has a 2D flow to fit")
    points = train_data["pcd_points"]
    views = prepare_views(points, K, [slots[i] for i in present], H, W)
    if sampler == "device":
        images = [train_data["frames"][k]["T2C_flow"][0] for k in range(len(present))]
        flow, loss, flow2d = fit_scene_flow(points, K, views, None, epochs=train_iteration, divisor=present[-1] + 1, device=device,
                                            records=sample_flow_images(views, images, device=device))
        return views, present, None, flow, loss, flow2d
    gt = []
    for k, _ in enumerate(present):
        # float64 pixels, as the reference hands them to griddata (:115,120)
        R, T = _pose(slots[present[k]])
        pix = np.matmul(np.asarray(K), R.dot(np.asarray(points)) + T)
        idx = views.valid[k]
        gt.append(sample_flow_image(train_data["frames"][k]["T2C_flow"][0], pix[:2, idx] / pix[-1:, idx], H, W))
    flow, loss, flow2d = fit_scene_flow(points, K, views, gt, epochs=train_iteration, divisor=present[-1] + 1, device=device)
    return views, present, gt, flow, loss, flow2d


def optimize_motion(train_data, render_poses, internal_poses, K, H, W, non_frame_idx=(), train_iteration=200, device=None,
                    sampler="griddata", resampler="griddata", workers=8, triangulator="host"):
    """MotionOptimization.optimize_motion (train_motion.py:65-207) without its unused arguments: view slot idx = i * len(internal)
    + j has the pose internal[j] o render[i] (:91-97); slots in non_frame_idx have no flow; the k-th remaining slot takes
    train_data['frames'][k]['T2C_flow'][0].  After the fit each fitted slot's last-epoch 2D flow is resampled onto the pixel
    grid and appended to train_data['frames'][idx]['our_flow'] -- indexed by the SLOT, as the reference does (:200) -- as a
    [1,2,H,W] float64 CPU tensor.  resampler: "griddata" does that with one scipy griddata per view on the host, as the reference
    does; "device" triangulates each view once on `workers` host threads (triangulate_views) and resamples all views in one call
    (resample_to_grid) from the flow the fit left on the device; triangulator="device" triangulates them there as well
    (upload_views).  Returns (train_data, scene_flow [3,P] on the device)."""
    if resampler not in RESAMPLERS:
        raise ValueError(f"resampler must be one of {RESAMPLERS}, got {resampler!r}")
    triangulator = _triangulator(triangulator)
    slots = [None if idx in non_frame_idx else s for idx, s in enumerate(compose_slots(render_poses, internal_poses))]
    views, present, _, flow, _, flow2d = _fit_slots(train_data, slots, K, H, W, train_iteration, device, sampler)
    if train_iteration > 0 and resampler == "device":
        final = resample_to_grid(views, flow2d, fill=0.0, device=flow2d.device, workers=workers, triangulator=triangulator).permute(0, 3, 1, 2).cpu()
        for k, idx in enumerate(present):
            train_data["frames"][idx]["our_flow"].append(final[k].contiguous().unsqueeze(0))
    elif train_iteration > 0:
        griddata, grid = _griddata(), _pixel_grid(H, W)
        flow2d = flow2d.cpu().numpy()
        points = np.asarray(train_data["pcd_points"])
        for k, idx in enumerate(present):
            R, T = _pose(slots[idx])
            pix = np.matmul(np.asarray(K), R.dot(points) + T)
            v = views.valid[k]
            final = griddata((pix[:2, v] / pix[-1:, v]).transpose(1, 0), flow2d[k, v], grid, method="linear",
                             fill_value=0).reshape(H, W, 2)
            train_data["frames"][idx]["our_flow"].append(torch.tensor(np.transpose(final, (2, 0, 1))).unsqueeze(0))
    return train_data, flow


def pose_from_transform_matrix(transform_matrix):
    """The world-to-camera (R, T) a frame's transform_matrix was made of: the inverse of train_motion.py:156-159, where
    Rj2w = (yz_reverse R)^T and Tj2w = -Rj2w (yz_reverse T)."""
    m = np.asarray(transform_matrix, dtype=np.float64)
    Rj2w, Tj2w = m[:3, :3], m[:3, 3:4]
    return np.matmul(YZ_REVERSE, Rj2w.T), -np.matmul(YZ_REVERSE, np.matmul(Rj2w.T, Tj2w))


def transform_matrix_from_pose(R, T):
    """train_motion.py:156-159."""
    R, T = np.asarray(R, np.float64), np.asarray(T, np.float64).reshape(3, 1)
    Rj2w = np.matmul(YZ_REVERSE, R).T
    Tj2w = -np.matmul(Rj2w, np.matmul(YZ_REVERSE, T))
    return np.concatenate((np.concatenate((Rj2w, Tj2w), axis=1), np.array([[0, 0, 0, 1.0]])), axis=0)


def stage1_intrinsics(H, W):
    """K of a stage-1 output (train_motion.py:47-62): the fixed focal length, the principal point at the image centre."""
    from .scene.dataset_readers import FOCAL
    return np.array([[FOCAL * (W / H), 0., W / 2], [0., FOCAL, H / 2], [0., 0., 1.]]).astype(np.float32)


def refit_scene_flow(input_dir, train_iteration=200, device=None, sampler="griddata", resampler="griddata", triangulator="host"):
    """Fits the scene flow of a stage-1 directory again from what MOM/train_data.pth holds -- the point cloud, every frame's pose
    (its transform_matrix) and 2D flow (T2C_flow) -- and writes MOM/scene_flow.pth.  A frame with an empty T2C_flow list is a view
    without a flow.  sampler: "griddata" (one scipy call per view on the host) or "device" (_fit_slots).  resampler: checked like
    optimize_motion's and otherwise without effect here -- the refit writes the scene flow alone, and our_flow, the one thing the
    resampler makes, is not part of it; triangulator likewise.  Returns the [3,P] flow (a CPU tensor, what is written)."""
    from .scene.dataset_readers import load_train_data
    _triangulator(triangulator)
    if sampler not in SAMPLERS:
        raise ValueError(f"sampler must be one of {SAMPLERS}, got {sampler!r}")
    if resampler not in RESAMPLERS:
        raise ValueError(f"resampler must be one of {RESAMPLERS}, got {resampler!r}")
    mom = os.path.join(input_dir, "MOM")
    data = load_train_data(os.path.join(mom, "train_data.pth"))
    H, W = int(data["H"]), int(data["W"])
    frames = data["frames"]
    slots = [pose_from_transform_matrix(fr["transform_matrix"]) if len(fr.get("T2C_flow", ())) else None for fr in frames]
    if all(s is None for s in slots):
        raise ValueError(f"{mom}/train_data.pth: no frame carries a T2C_flow image (every list is empty), so there is nothing to "
                         "fit the scene flow to")
    # _fit_slots reads the k-th present slot's flow from frame k: hand it the frames that have one, in order
    with_flow = dict(data, frames=[fr for fr, s in zip(frames, slots) if s is not None])
    _, _, _, flow, _, _ = _fit_slots(with_flow, slots, stage1_intrinsics(H, W), H, W, train_iteration, device, sampler)
    flow = flow.cpu()
    torch.save(flow, os.path.join(mom, "scene_flow.pth"))
    return flow


def write_pixel_video(input_dir, n_frames=120, size=1024, center_idx=2, writer=None, ordered=None):
    """MOM/video/%06d.png of a stage-1 directory from the centre frame of its MOM/train_data.pth -- image, our_flow[0] and mask, what
    the reference hands its VideoGenerator (main_jih.py:27-39) -- by cinemagraph.pixel_video, saved at the data's W x H as
    train_motion.save_video names the frames (train_motion.py:402-412).  A pixel warp, not the reference's StyleGAN output.
    writer: cinemagraph.save_video's -- "host" (the default) copies every frame to the host and resizes and deflates it there; "device"
    resizes and deflates each frame on the GPU as it is made; the files decode to the same pixels.
    ordered: cinemagraph.warp_one_level's -- None follows diff_gaussian_rasterization._C.set_deterministic; True: the warp adds in a
    defined order and the frames are the same bits run after run."""
    from . import cinemagraph
    from .scene.dataset_readers import load_train_data
    mom = os.path.join(input_dir, "MOM")
    data = load_train_data(os.path.join(mom, "train_data.pth"))
    frame = data["frames"][center_idx]
    missing = [k for k in ("image", "our_flow", "mask") if k not in frame or (k == "our_flow" and not len(frame[k]))]
    if missing:
        raise ValueError(f"{mom}/train_data.pth: frame {center_idx} lacks {missing}, which the video is made from")
    if writer not in (None,) + cinemagraph.VIDEO_WRITERS:
        raise ValueError(f"writer must be one of {cinemagraph.VIDEO_WRITERS}, got {writer!r}")
    make = cinemagraph.pixel_video_frames if writer == "device" else cinemagraph.pixel_video
    frames = make(frame["image"], frame["our_flow"][0], frame["mask"], n_frames=n_frames, size=size, ordered=ordered)
    return cinemagraph.save_video(frames, mom, int(data["W"]), int(data["H"]), writer=writer)


def _rotation(th_deg, phi_deg):
    """Ry(th) Rx(phi) with the reference's signs and its degree -> radian expression (utils/trajectory.py:224,296).  Every entry of the
    product has one non-zero term, so the result does not depend on how a BLAS orders a 3 x 3 matmul."""
    th, phi = th_deg / 180 * np.pi, phi_deg / 180 * np.pi
    return np.matmul(np.array([[np.cos(th), 0, -np.sin(th)], [0, 1, 0], [np.sin(th), 0, np.cos(th)]]),
                     np.array([[1, 0, 0], [0, np.cos(phi), -np.sin(phi)], [0, np.sin(phi), np.cos(phi)]]))


# utils/trajectory.py:210-226 generate_seed_preset: entries 0, 1, 4, 7, 14 of its 21-pose table, (theta, phi) in degrees
LOOKAROUND_DEG = ((0.0, 0.0), (20.0, 0.0), (-20.0, 0.0), (0.0, -22.5), (0.0, 22.5))
# utils/trajectory.py:282-300 generate_seed_hemisphere: its `degree` argument is overwritten by 5, and d is the literal 4.3 -- the
# centre depth train_motion.py:41 passes is ignored (:293-294)
HEMISPHERE_DEG = ((5, 0), (0, -5), (0, 0), (0, 5), (-5, 0))
HEMISPHERE_D = 4.3


def pcd_gen_poses(name):
    """utils/trajectory.py get_pcdGenPoses(name) for the two names stage 1 uses (train_motion.py:38,41), [5,3,4] float64
    world-to-camera: 'lookaround' is generate_seed_preset -- five pure rotations, not the fourteen train_motion.py's comment speaks
    of -- and 'hemisphere' five poses on a sphere of radius 4.3 about the scene, 5 degrees apart.  Another name raises ValueError
    (the reference raises a TypeError from `raise("...")`, or serves trajectories stage 1 never asks for)."""
    if name == "lookaround":
        poses = np.zeros((len(LOOKAROUND_DEG), 3, 4))
        for i, (th, phi) in enumerate(LOOKAROUND_DEG):
            poses[i, :3, :3] = _rotation(th, phi)
        return poses
    if name == "hemisphere":
        d, poses = HEMISPHERE_D, np.zeros((len(HEMISPHERE_DEG), 3, 4))
        for i, (th, phi) in enumerate(HEMISPHERE_DEG):
            poses[i, :3, :3] = _rotation(th, phi)
            poses[i, :3, 3:4] = (np.array([d * np.sin(th / 180 * np.pi), 0, d - d * np.cos(th / 180 * np.pi)]).reshape(3, 1)
                                 + np.array([0, d * np.sin(phi / 180 * np.pi), d - d * np.cos(phi / 180 * np.pi)]).reshape(3, 1))
        return poses
    raise ValueError(f"pcd_gen_poses knows 'lookaround' and 'hemisphere' (what stage 1 uses), got {name!r}")


def read_json(source):
    """train_motion.py:376-392: the hints of a labelme file (a path, or the parsed dict) as four lists of ints -- start x, start y,
    end x, end y -- of every shape whose label starts with 'hint', truncated towards zero as int() does."""
    import json
    if isinstance(source, dict):
        data = source
    else:
        with open(source) as f:
            data = json.load(f)
    out = [[], [], [], []]
    for shape in data["shapes"]:
        if shape["label"].startswith("hint"):
            start, end = np.array(shape["points"])
            for lst, val in zip(out, (start[0], start[1], end[0], end[1])):
                lst.append(int(val))
    return out


HINT_BOUND = 512          # demo.py:57: a literal, whatever the image's size


def hint_arguments(frame, sigma=None):
    """The hints generate_mask_hints_from_user hands its arithmetic (thirdparty/cinemagraphy/demo.py:47-86) for one frame of
    render_pcd: (pos int64 [n,2], start float64 [n,2], end float64 [n,2], sigma), columns (x, y); hint k sits at pos[k] and moves by
    (end[k] - start[k]) / 50.  The reference's quirks, as written:
      * a hint is kept if 0 <= x < 512 and 0 <= y < 512 -- the literal 512, not the image's size (:57).  In an image smaller than
        512 a kept hint can lie outside it; the reference then indexes its pixel grid out of range and raises IndexError, and so
        does this function;
      * when no hint is kept, one hint at (0, 0) is used (:61-63);
      * the motion of kept hint number k is read from the UNFILTERED lists at index k (:67-70): after a dropped hint every later
        hint moves with an earlier hint's motion, and the (0, 0) fallback moves with hint 0's;
      * sigma=None draws np.random.randint(height // (n * 2), height // (n / 2)) from numpy's global generator, the reference's
        expression (:86), so a seeded run draws what the seeded reference draws; an int is taken as it is."""
    sx, sy, ex, ey = (frame[k] for k in ("final_hint_start_x", "final_hint_start_y", "final_hint_end_x", "final_hint_end_y"))
    height, width = np.array(frame["mask"]).shape[:2]
    pos = [(int(x[0]), int(y[0])) for x, y in zip(sx, sy) if 0 <= x[0] < HINT_BOUND and 0 <= y[0] < HINT_BOUND]
    if not pos:
        pos = [(0, 0)]
    for x, y in pos:
        if x >= width or y >= height:
            raise IndexError(f"a hint at ({x}, {y}) passes the reference's literal bound of {HINT_BOUND} but lies outside the "
                             f"{width} x {height} image")
    n = len(pos)
    first = lambda lst: np.array([np.asarray(lst[k], np.float64).reshape(-1)[0] for k in range(n)])
    start, end = np.stack([first(sx), first(sy)], axis=1), np.stack([first(ex), first(ey)], axis=1)
    if sigma is None:
        sigma = np.random.randint(height // (n * 2), height // (n / 2))
    return np.asarray(pos, np.int64).reshape(n, 2), start, end, int(sigma)


RESIZERS = ("pil", "device")


def motion_rgbs(frames, size, resizer="pil", device=None):
    """[V,3,S,S] float32 in [-1, 1]: every frame's image resized bicubically to S x S, ToTensor, Normalize(0.5, 0.5) (demo.py:109-127).
    PIL's Image.resize(BICUBIC) is what torchvision's Resize calls for a PIL image.
    resizer "pil": one Image.resize per view on the host; a CPU tensor.  "device": the images -- all RGB and of one size, anything
    else raises -- are uploaded once as [V,H,W,3] bytes and resized in one ops.pil_resize call, PIL's bytes; the normalisation is a
    256-entry table made on the host by the host route's own statements, so the floats are the host route's bit for bit (a division
    on the device is a product with a reciprocal, which is not).  A tensor on `device` (default: the current GPU)."""
    from PIL import Image
    if resizer not in RESIZERS:
        raise ValueError(f"resizer must be one of {RESIZERS}, got {resizer!r}")
    if resizer == "device":
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        images = [fr["image"] for fr in frames]
        odd = [(k, getattr(im, "mode", type(im).__name__), getattr(im, "size", None)) for k, im in enumerate(images)
               if not isinstance(im, Image.Image) or im.mode != "RGB" or im.size != images[0].size]
        if not images or odd:
            raise ValueError(f"motion_rgbs(resizer='device') takes RGB PIL images of one size; (frame, mode, size) of the others: {odd}")
        rgb8 = ops.pil_resize(_upload(np.stack([np.asarray(im, np.uint8) for im in images]), dev), (size, size))
        table = (torch.arange(256).float().div(255) - 0.5) / 0.5
        floats = torch.index_select(table.to(dev), 0, rgb8.reshape(-1).int())          # (a uint8 index would be read as a mask)
        return floats.view(rgb8.shape).permute(0, 3, 1, 2).contiguous()
    out = np.empty((len(frames), 3, size, size), np.float32)
    for k, fr in enumerate(frames):
        im = np.asarray(fr["image"].convert("RGB").resize((size, size), Image.BICUBIC), np.uint8)
        out[k] = ((torch.from_numpy(im.transpose(2, 0, 1).copy()).float().div(255) - 0.5) / 0.5).numpy()
    return torch.from_numpy(out)


def estimate_flows(train_data, estimator=None, size=768, device=None, resizer="pil"):
    """MotionOptimization.estimate_flow (train_motion.py:368-374): appends a [1,2,H,W] float32 CPU tensor to every frame's T2C_flow.
    The reference builds its estimator, loads its weights and runs the arithmetic around it on the CPU once per view; here the
    hints of all views are selected on the host (hint_arguments, in frame order, so sigma is drawn as the reference draws it) and
    the arithmetic runs on the device for all views at once: ops.hint_field in front of the estimator, ops.flow_finish behind it.
    estimator: a callable (motion_rgbs [V,3,S,S], mask_s [V,1,S,S], hints [V,2,S,S]) -> pred [V,2,S,S] on the device -- the user's
    own network (the reference's SPADEUnetMaskMotion.forward_flow(...)["PredMotion"]), loaded once; resizer: who resizes the images
    it is given, motion_rgbs' argument ("pil" on the host, "device": the same floats).  estimator=None takes pred = hints:
    the dense hint field itself as the motion -- a SUBSTITUTE for the reference's estimator that needs no checkpoint, not its output
    (as cinemagraph.pixel_video is for the video generator).  size: the estimator's working size (config.yaml's data.W)."""
    dev = torch.device("cuda" if device is None else device)
    if resizer not in RESIZERS:
        raise ValueError(f"resizer must be one of {RESIZERS}, got {resizer!r}")
    frames = train_data["frames"]
    if not frames:
        raise ValueError("train_data has no frames")
    args = [hint_arguments(fr) for fr in frames]
    masks = np.stack([np.array(fr["mask"]) for fr in frames])
    if masks.ndim != 3:
        raise ValueError(f"every frame's mask must be one channel of one size, got {masks.shape}")
    V, n = len(frames), max(len(a[0]) for a in args)
    pos, start, end = np.zeros((V, n, 2), np.int32), np.zeros((V, n, 2), np.float64), np.zeros((V, n, 2), np.float64)
    for k, (p, s, e, _) in enumerate(args):
        pos[k, :len(p)], start[k, :len(p)], end[k, :len(p)] = p, s, e
    up = lambda a: _upload(a, dev)
    hints, mask_s = ops.hint_field(up(pos), up(start), up(end), up(np.asarray([len(a[0]) for a in args], np.int32)),
                                   up(np.asarray([a[3] for a in args], np.float32)), up((masks != 0).astype(np.uint8)), size)
    if estimator is None:
        pred = hints
    else:
        with torch.no_grad():
            pred = estimator(up(motion_rgbs(frames, size, resizer=resizer, device=dev)), mask_s, hints)
        if tuple(pred.shape) != tuple(hints.shape):
            raise ValueError(f"the estimator must return [{V}, 2, {size}, {size}], got {tuple(pred.shape)}")
        pred = pred.detach().to(torch.float32).contiguous()
    flow = ops.flow_finish(pred, mask_s, masks.shape[1], masks.shape[2]).cpu()
    for k, fr in enumerate(frames):
        fr["T2C_flow"].append(flow[k:k + 1].clone())
    return train_data


def _color_wheel():
    """The 55-entry Middlebury colour wheel (Baker et al., ICCV 2007) as helpmotion.make_colorwheel fills it: six segments, in each
    one channel at 255 and one ramping by floor(255 i / n), up or down."""
    wheel, row = np.zeros((55, 3)), 0
    for n, full, ramp, down in ((15, 0, 1, False), (6, 1, 0, True), (4, 1, 2, False), (11, 2, 1, True), (13, 2, 0, False), (6, 0, 2, True)):
        steps = np.floor(255 * np.arange(0, n) / n)
        wheel[row:row + n, full] = 255
        wheel[row:row + n, ramp] = 255 - steps if down else steps
        row += n
    return wheel


def flow_image(flow):
    """helpmotion.flow2img: a [2,H,W] flow (tensor or array) as the [H,W,3] uint8 colour-wheel image train_motion.viz_flow saves,
    in the flow's own dtype as the reference computes it.  As written there: the flow is normalised by its largest magnitude + 1e-5;
    the hue index next to the last wheel entry wraps to entry 1, not 0 (helpmotion.py:113); magnitudes above 1 are dimmed by 0.75."""
    f = flow.detach().cpu().numpy() if torch.is_tensor(flow) else np.asarray(flow)
    if f.ndim != 3 or f.shape[0] != 2:
        raise ValueError(f"flow must be [2,H,W], got {f.shape}")
    H, W = f.shape[1:]
    u, v = f[0].reshape(-1), f[1].reshape(-1)
    rad_max = np.max(np.sqrt(np.square(u) + np.square(v)))
    u, v = u / (rad_max + 1e-5), v / (rad_max + 1e-5)
    wheel = _color_wheel()
    ncols = wheel.shape[0]
    rad = np.sqrt(np.square(u) + np.square(v))
    fk = (np.arctan2(-v, -u) / np.pi + 1) / 2 * (ncols - 1)
    k0 = np.floor(fk).astype(np.int32)
    k1 = k0 + 1
    k1[k1 == ncols] = 1
    frac = fk - k0
    image, inside = np.zeros((H * W, 3), np.uint8), rad <= 1
    for c in range(3):
        col = (1 - frac) * (wheel[k0, c] / 255.0) + frac * (wheel[k1, c] / 255.0)
        col[inside] = 1 - rad[inside] * (1 - col[inside])
        col[~inside] = col[~inside] * 0.75
        image[:, c] = np.floor(255 * col)
    return image.reshape(H, W, 3)


def build_stage1(input_dir, depth, flow="hints", train_iteration=200, video="none", render_poses=None, internal_poses=None, size=768,
                 n_frames=120, video_size=1024, device=None, video_writer=None, triangulator="host", ordered=None):
    """Stage 1 from an input folder, as train_motion.py:442-464 runs it: image.png, image_json/mask.png and the hints of image.json ->
    MOM/train_data.pth, MOM/scene_flow.pth and MOM/Flow_viz/%03d.png, what stage 2 (Trainer) reads.
    depth: float32 [H,W] or the path of a .npy holding it -- what the reference's depth network returns for the image
    (d_model.infer_pil; the network is not part of this package).  flow: "hints" (estimate_flows without an estimator: the hint
    field as the motion, a SUBSTITUTE for the reference's flow estimator) or the estimator callable of estimate_flows.
    render_poses / internal_poses: [n,3,4] world-to-camera, by default pcd_gen_poses('lookaround') / ('hemisphere').
    video="pixels" also writes MOM/video/%06d.png with write_pixel_video (again a substitute, for the reference's GAN), through its
    writer `video_writer` ("host", the default, or "device"); ordered: write_pixel_video's (the video's warp is the one stage-1 kernel
    with float atomics: with ordered=True, or under _C.set_deterministic(True), the whole folder is a function of the input).
    The renders, the flow arithmetic, the sampling, the fit and our_flow all run on the device (render_pcd, estimate_flows,
    optimize_motion with the device sampler and resampler); triangulator: where their views are triangulated, "host" (scipy's
    thread pool, the default) or "device" (upload_views).  Returns (train_data, scene_flow [3,P] CPU)."""
    from PIL import Image
    triangulator = _triangulator(triangulator)
    if video not in ("none", "pixels"):
        raise ValueError(f"video must be 'none' or 'pixels', got {video!r}")
    if not (flow == "hints" or callable(flow)):
        raise ValueError(f"flow must be 'hints' or an estimator callable, got {flow!r}")
    src_img = Image.open(os.path.join(input_dir, "image.png"))
    if src_img.mode != "RGB":
        src_img = src_img.convert("RGB")
    src_mask = Image.open(os.path.join(input_dir, "image_json", "mask.png"))
    hints = read_json(os.path.join(input_dir, "image.json"))
    W, H = src_img.size
    depth = np.load(depth) if isinstance(depth, (str, os.PathLike)) else np.asarray(depth)
    if depth.shape != (H, W):
        raise ValueError(f"the depth must be [{H}, {W}] like image.png, got {depth.shape}")
    if np.array(src_mask).shape != (H, W):
        raise ValueError(f"image_json/mask.png must be one channel of {W} x {H} like image.png, got {np.array(src_mask).shape}")
    K = stage1_intrinsics(H, W)
    render_poses = pcd_gen_poses("lookaround") if render_poses is None else np.asarray(render_poses)
    internal_poses = pcd_gen_poses("hemisphere") if internal_poses is None else np.asarray(internal_poses)
    mom = os.path.join(input_dir, "MOM")
    os.makedirs(mom, exist_ok=True)
    train_data, none_idx = render_pcd(src_img, src_mask, depth.astype(np.float32), hints, render_poses, internal_poses, device=device,
                                      triangulator=triangulator)
    train_data = estimate_flows(train_data, None if flow == "hints" else flow, size=size, device=device)
    train_data, scene_flow = optimize_motion(train_data, render_poses, internal_poses, K, H, W, non_frame_idx=none_idx,
                                             train_iteration=train_iteration, device=device, sampler="device", resampler="device",
                                             triangulator=triangulator)
    scene_flow = scene_flow.cpu()
    viz = os.path.join(mom, "Flow_viz")
    os.makedirs(viz, exist_ok=True)
    for idx, fr in enumerate(train_data["frames"]):                       # train_motion.py:394-399 viz_flow
        if len(fr["our_flow"]):
            Image.fromarray(flow_image(fr["our_flow"][0][0])).save(os.path.join(viz, f"{idx:03d}.png"))
    torch.save(train_data, os.path.join(mom, "train_data.pth"))
    torch.save(scene_flow, os.path.join(mom, "scene_flow.pth"))
    if video == "pixels":
        write_pixel_video(input_dir, n_frames, video_size, writer=video_writer, ordered=ordered)
    return train_data, scene_flow


def main(argv=None):
    from argparse import ArgumentParser
    ap = ArgumentParser(description="Fit MOM/scene_flow.pth of a stage-1 directory to the 2D flows in its MOM/train_data.pth")
    ap.add_argument("--input_dir", required=True)
    ap.add_argument("--train_iteration", type=int, default=200)
    ap.add_argument("--sampler", choices=SAMPLERS, default="griddata", help="where the 2D flow images are sampled: scipy's griddata "
                    "per view on the host, or one HIP launch for all views")
    ap.add_argument("--resampler", choices=RESAMPLERS, default="griddata", help="where optimize_motion resamples our_flow onto the "
                    "pixel grid: scipy's griddata per view on the host, or one triangulation per view and the device for the rest; "
                    "scene_flow.pth does not depend on it")
    ap.add_argument("--triangulator", choices=TRIANGULATORS, default="host", help="where each view's scattered points are triangulated: "
                    "scipy's Delaunay on host threads, or the device (scipy then only for a view the device refuses)")
    ap.add_argument("--video", choices=("none", "pixels"), default="none", help="pixels: instead of the fit, write MOM/video/%%06d.png "
                    "from frame 2's image, our_flow and mask by warping the image's PIXELS (cinemagraph.pixel_video) -- a substitute "
                    "for the reference's StyleGAN video, which needs checkpoints; no mp4 is written")
    ap.add_argument("--n_frames", type=int, default=120, help="frames of the --video loop (the reference's option.py:35)")
    ap.add_argument("--video_size", type=int, default=1024, help="side of the square the --video warp runs at (main_jih.py:33-39)")
    ap.add_argument("--video-writer", dest="video_writer", choices=("host", "device"), default="host", help="--video pixels: who resizes "
                    "and encodes the frames -- the host (PIL and zlib on the calling thread), or the device as each frame is made; the "
                    "files decode to the same pixels")
    ap.add_argument("--build", action="store_true", help="build stage 1 from the folder's image.png, image.json and image_json/mask.png "
                    "(build_stage1): writes MOM/train_data.pth, MOM/scene_flow.pth and MOM/Flow_viz; with --video pixels the frames too")
    ap.add_argument("--depth", help="--build: a .npy with the image's float32 [H,W] depth (the depth network is the user's own)")
    ap.add_argument("--flow", choices=("hints",), default="hints", help="--build: where the 2D flows come from.  hints: the dense hint "
                    "field itself -- a substitute for the reference's flow estimator, which needs a checkpoint (an estimator of "
                    "one's own is passed to build_stage1 in Python)")
    ap.add_argument("--size", type=int, default=768, help="--build: the flow estimator's working size (config.yaml's data.W)")
    ap.add_argument("--render_poses", type=int, default=None, help="--build: use only the first N of the five 'lookaround' poses")
    ap.add_argument("--seed", type=int, default=None, help="--build: seed numpy's global generator, which draws every view's sigma")
    ap.add_argument("--deterministic", action="store_true", help="diff_gaussian_rasterization._C.set_deterministic(True) before any work: "
                    "the --video warp adds in a defined order, so the frames are the same bits run after run")
    a = ap.parse_args(argv)
    if a.deterministic:
        from .diff_gaussian_rasterization import _C
        _C.set_deterministic(True)
    if a.build:
        if not a.depth:
            ap.error("--build needs --depth FILE")
        if a.seed is not None:
            np.random.seed(a.seed)
        poses = None if a.render_poses is None else pcd_gen_poses("lookaround")[:a.render_poses]
        data, flow = build_stage1(a.input_dir, a.depth, flow=a.flow, train_iteration=a.train_iteration, video=a.video,
                                  render_poses=poses, size=a.size, n_frames=a.n_frames, video_size=a.video_size,
                                  video_writer=a.video_writer, triangulator=a.triangulator)
        print(f"{os.path.join(a.input_dir, 'MOM')}: {len(data['frames'])} frames; scene_flow.pth: {tuple(flow.shape)}, largest "
              f"magnitude {float(flow.abs().max()):.6g}")
        return
    if a.video == "pixels":
        paths = write_pixel_video(a.input_dir, a.n_frames, a.video_size, writer=a.video_writer)
        print(f"{os.path.dirname(paths[0])}: {len(paths)} frames")
        return
    flow = refit_scene_flow(a.input_dir, a.train_iteration, sampler=a.sampler, resampler=a.resampler, triangulator=a.triangulator)
    print(f"scene_flow.pth: {tuple(flow.shape)}, largest magnitude {float(flow.abs().max()):.6g}")


if __name__ == "__main__":
    main()
