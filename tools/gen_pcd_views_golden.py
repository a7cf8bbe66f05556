"""Writes tests/golden/g18_pcd_views.npz: two small multi-view point-cloud renders by the REFERENCE's own render_PCD
(train_motion.py:211-366).

Run by hand on a machine that has a checkout of the reference and scipy; the tests read only the file it writes.

    python tools/gen_pcd_views_golden.py --reference /path/to/ICLR2025_3D-MOM [--out tests/golden/g18_pcd_views.npz]

The import harness is tools/gen_sceneflow_golden.py's (every module of stage 1 that is not installed is replaced by an empty
stand-in).  render_PCD is called unbound on a namespace that carries the attributes it reads (H, W, K, src_depth, render_poses,
internel_render_poses, fov).  Two names of the module are wrapped while it runs, without changing what they return: `interp_grid`,
to record each call's points, values and result, and `np.round`, to record the float images in front of the 8-bit cast.  Only data
is stored: the inputs, each view's valid indices, scipy's own simplices of each view's points (what griddata triangulates), a part
of the recorded griddata outputs (all of them do not fit the size a fixture may have; the final bytes cover every view and channel),
the final images and masks, the hints and transform matrices.

The scenes: 40 x 48 ("s") and 80 x 96 ("l") pixels, 2 render poses x 2 internal poses each.  View 0 is the identity: its points sit
on the pixel lattice, every pixel centre lies on a vertex or an edge, and the lowest-index rule decides.  The other poses rotate by
0.03-0.1 rad and translate by 0.1-0.3.  The depth is smooth plus a step of 1.2 over one quadrant, so the warped sheet folds and
opens gaps that large triangles bridge.  The image is random bytes, the mask has the levels 0 / 128 / 200 / 255, there is one hint.
"""
import argparse
import importlib
import os
import sys
import types

import numpy as np
from PIL import Image

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path[:0] = [os.path.dirname(os.path.abspath(__file__)), ROOT, os.path.join(ROOT, "tests")]
from gen_sceneflow_golden import import_reference, rot  # noqa: E402

SIZES = {"s": (40, 48), "l": (80, 96)}
# which recorded griddata outputs are kept: per scene, view -> keys ("rgb": the colour call, "r": its first channel, "m": the mask
# call's first channel; the reference's three mask channels are asserted equal)
KEPT = {"s": {0: ("rgb", "m"), 1: ("rgb", "m"), 2: ("r", "m"), 3: ("rgb", "m")}, "l": {0: ("m",), 1: ("r", "m"), 2: ("m",), 3: ("r", "m")}}


def pose(ax, ay, t):
    return np.concatenate([rot(ax, ay), np.asarray(t, np.float64).reshape(3, 1)], axis=1)


def make_scene(name, seed=18):
    H, W = SIZES[name]
    rng = np.random.default_rng(seed + H)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    depth = 3.0 + 0.3 * np.sin(x * (7.0 / W)) + 0.2 * np.cos(y * (5.0 / H))
    depth[: H // 2, : W // 2] += 1.2
    image = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    mask = np.zeros((H, W), np.uint8)
    mask[H // 8: H // 2, W // 6: W // 2] = 128
    mask[H // 3: 3 * H // 4, W // 3: 5 * W // 6] = 200
    mask[H // 2: 7 * H // 8, W // 2: 7 * W // 8] = 255
    f = 0.95 * W
    K = np.array([[f, 0, W / 2], [0, f, H / 2], [0, 0, 1]], np.float32)
    render = np.stack([pose(0.0, 0.0, (0, 0, 0)), pose(0.05, -0.08, (0.2, -0.1, 0.1))])
    internal = np.stack([pose(0.0, 0.0, (0, 0, 0)), pose(-0.03, 0.1, (-0.3, 0.1, 0.15))])
    hints = [[W // 3], [H // 3], [2 * W // 3], [H // 2]]
    return dict(H=H, W=W, depth=depth.astype(np.float32), image=image, mask=mask, K=K, render=render, internal=internal, hints=hints)


def run_reference(tm, sc):
    H, W = sc["H"], sc["W"]
    calls, rounds = [], []
    real_interp = tm.interp_grid

    def interp(points, values, xi, **kw):
        out = real_interp(points, values, xi, **kw)
        calls.append((np.array(points), np.array(values), np.array(out)))
        return out

    class NumpyProxy:
        def __getattr__(self, name):
            return getattr(np, name)

        @staticmethod
        def round(a, *args, **kw):
            if np.shape(a) in ((H, W, 3), (H, W)):
                rounds.append(np.array(a))
            return np.round(a, *args, **kw)

    K = sc["K"]
    fov = (2 * np.arctan(W / (2 * float(K[0, 0]))), 2 * np.arctan(H / (2 * float(K[1, 1]))))
    ns = types.SimpleNamespace(H=H, W=W, K=K, src_depth=sc["depth"], render_poses=sc["render"], internel_render_poses=sc["internal"], fov=fov)
    tm.interp_grid, tm.np = interp, NumpyProxy()
    try:
        data, none_idx = tm.MotionOptimization.render_PCD(ns, Image.fromarray(sc["image"]), Image.fromarray(sc["mask"]), sc["hints"])
    finally:
        tm.interp_grid, tm.np = real_interp, np
    return data, none_idx, calls, rounds


def main():
    import scipy
    from scipy.spatial import Delaunay
    import pcd_views_cases as pc
    motion = importlib.import_module("iclr2025_3d-mom_amd.motion")

    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="a checkout of cvsp-lab/ICLR2025_3D-MOM")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "g18_pcd_views.npz"))
    ap.add_argument("--stub", nargs="*", default=[], help="further top-level modules to stand in for")
    a = ap.parse_args()
    tm, used = import_reference(os.path.abspath(a.reference), a.stub)
    print("stand-ins used for:", used)
    out = {"scipy_version": np.array(scipy.__version__)}
    for name in SIZES:
        sc = make_scene(name)
        H, W = sc["H"], sc["W"]
        data, none_idx, calls, rounds = run_reference(tm, sc)
        V = len(data["frames"])
        assert V == 4 and none_idx == [] and len(calls) == 3 * V and len(rounds) == 2 * V
        put = lambda k, v: out.__setitem__(f"{name}_{k}", v)
        for k in ("depth", "image", "mask", "K"):
            put(k, sc[k])
        put("render_poses", sc["render"])
        put("internal_poses", sc["internal"])
        put("hints", np.asarray(sc["hints"], np.int64))
        put("fov", np.asarray([data["camera_angle_x"], data["camera_angle_y"]], np.float64))
        put("views", np.int64(V))
        put("none_idx", np.asarray(none_idx, np.int64))
        nearest, big, multi = np.inf, 0, 0
        for k in range(V):
            pts, _, rgb_out = calls[3 * k]
            _, _, mask_out = calls[3 * k + 2]
            assert np.array_equal(pts, calls[3 * k + 2][0]) and np.array_equal(mask_out[:, 0], mask_out[:, 1]) and \
                np.array_equal(mask_out[:, 0], mask_out[:, 2])
            tris = Delaunay(pts).simplices
            assert tris.max() < 2 ** 15 and len(pts) < 2 ** 16
            put(f"tris_{k}", tris.astype(np.int16))
            kept = KEPT[name][k]
            if "rgb" in kept:
                put(f"gd_{k}_rgb", rgb_out.reshape(H, W, 3))
            if "r" in kept:
                put(f"gd_{k}_r", rgb_out.reshape(H, W, 3)[..., 0])
            if "m" in kept:
                put(f"gd_{k}_m", mask_out.reshape(H, W, 3)[..., 0])
            fr = data["frames"][k]
            put(f"out_image_{k}", np.array(fr["image"]))
            put(f"out_mask_{k}", np.array(fr["mask"]))
            put(f"tm_{k}", np.asarray(fr["transform_matrix"], np.float64))
            put(f"hints_{k}", np.asarray([np.ravel(fr[n]) for n in ("final_hint_start_x", "final_hint_start_y", "final_hint_end_x",
                                                                     "final_hint_end_y")], np.float64))
            for f in rounds[2 * k: 2 * k + 2]:
                assert f.min() >= 0.0 and f.max() <= 255.0, (name, k, f.min(), f.max())
                nearest = min(nearest, float(np.abs(f - np.floor(f) - 0.5).min()))
            big += int((pc.box_pixels(pts, tris, H, W) > pc.LANE_BOX).sum())
            multi += int((pc.tri_owner(pts, tris, H, W)[2] > 1).sum())
        # valid sets: by the package's own projection (the expressions of :285-297), checked against the points griddata was given
        views, present, none2 = motion.pcd_views(data["pcd_points"], sc["K"], motion.compose_slots(sc["render"], sc["internal"]), H, W)
        assert present == list(range(V)) and none2 == []
        world, colors, masks = motion.pcd_points(sc["image"], sc["mask"], sc["depth"], sc["K"], sc["render"][0, :3, :3], sc["render"][0, :3, 3:4])
        assert np.array_equal(world, data["pcd_points"]) and np.array_equal(colors, data["pcd_colors"]) and np.array_equal(masks, data["pcd_masks"])
        for k in range(V):
            assert np.array_equal(views.pix64[k].T, calls[3 * k][0]), (name, k)
            assert np.array_equal(data["pcd_colors"][views.valid[k]], calls[3 * k][1])
            put(f"valid_{k}", views.valid[k].astype(np.uint16))
        print(f"{name}: {H} x {W}, valid per view {[len(v) for v in views.valid]}, triangles {[len(out[f'{name}_tris_{k}']) for k in range(V)]}; "
              f"{big} boxes above {pc.LANE_BOX} pixels, {multi} pixels with two or more passing triangles, nearest 255 v to a half-integer {nearest:.3g}")
        assert big >= 1 and multi >= 1 and nearest >= 1e-7
    np.savez_compressed(a.out, **out)
    print(a.out, os.path.getsize(a.out), "bytes")


if __name__ == "__main__":
    main()
