"""Time of the multi-view point-cloud renders (motion.render_pcd_device) and of the our_flow resampling (motion.resample_to_grid) at the
reference's size -- a 512 x 512 source image, 14 x 5 views -- against the reference's scipy.interpolate.griddata path, in one process:

  griddata   the reference's path (train_motion.py:304,307,319 and :198): three griddata calls per view for render_PCD (colours, the
             unused depth, the mask colours) and one more for our_flow.  Two views are timed, once each; "x 70" is an extrapolation
             and labelled so
  new path   triangulate_views (scipy.spatial.Delaunay per view on host threads) + upload + ops.tri_resample + ops.pcd_compose for all
             views, by wall clock, triangulation included, at 1, 8 and 16 workers
  kernels    the device part alone (tri_resample of 4 channels + pcd_compose; tri_resample of 2 channels for our_flow) between a
             torch.cuda.Event pair, per view; median and range of five windows after a warm-up

The scene: a smooth depth with a step of 1.2 over one quadrant, back-projected with the stage-1 intrinsics; random colours, a blocky
mask.  Parity is checked on the two timed views: the device's resampled colours against griddata's own output.

One process.  Every GPU step runs under an alarm of --step-limit seconds that ends the process; run it under a time limit as well.

    python tools/pcd_views_time.py [--side 512] [--windows 5] [--out profiles/pcd_views_time.json]
"""
import argparse
import importlib
import json
import math
import os
import signal
import statistics
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
pkg = "iclr2025_3d-mom_amd"

from sceneflow_fit_time import rot          # noqa: E402  (tools/ is this script's directory)


def make_scene(side, n_render, n_internal, seed=18):
    motion = importlib.import_module(pkg + ".motion")
    rng = np.random.default_rng(seed)
    H = W = side
    K = motion.stage1_intrinsics(H, W)
    v, u = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    depth = 3.0 + 0.3 * np.sin(u * (7 * math.pi / W) + 0.4) + 0.2 * np.sin(v * (5 * math.pi / H) + 1.1)
    depth[: H // 2, : W // 2] += 1.2
    image = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    mask = np.zeros((H, W), np.uint8)
    mask[H // 8: H // 2, W // 6: W // 2] = 128
    mask[H // 3: 3 * H // 4, W // 3: 5 * W // 6] = 255
    pose = lambda R, T: np.concatenate([R, T], axis=1)
    render = [pose(np.eye(3), np.zeros((3, 1)))]
    for _ in range(n_render - 1):
        a = rng.uniform(-0.06, 0.06, 2)
        render.append(pose(rot(a[0], a[1]), rng.uniform(-0.15, 0.15, (3, 1))))
    internal = [pose(np.eye(3), np.zeros((3, 1)))]
    for _ in range(n_internal - 1):
        b = rng.uniform(-0.03, 0.03, 2)
        internal.append(pose(rot(b[0], b[1]), rng.uniform(-0.05, 0.05, (3, 1))))
    return depth.astype(np.float32), image, mask, K, np.stack(render), np.stack(internal)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=512)
    ap.add_argument("--render", type=int, default=14)
    ap.add_argument("--internal", type=int, default=5)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--launches", type=int, default=3, help="device passes over all views per window")
    ap.add_argument("--workers", type=int, nargs="*", default=[1, 8, 16])
    ap.add_argument("--step-limit", type=int, default=300, help="seconds any one GPU step may take before the process is ended")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from scipy.interpolate import griddata
    N = importlib.import_module(pkg + "._native")
    ops = importlib.import_module(pkg + ".ops")
    motion = importlib.import_module(pkg + ".motion")
    assert torch.cuda.is_available(), "this tool measures on the GPU; there is nothing to fall back to"
    dev = torch.device("cuda", 0)
    say = lambda *s: print(*s, file=sys.stderr, flush=True)

    class gpu_step:
        """SIGALRM's default action ends the process, inside a blocked runtime call as well."""
        def __enter__(self):
            signal.alarm(a.step_limit)

        def __exit__(self, *exc):
            signal.alarm(0)

    def wall(fn, sync=False):
        t0 = time.perf_counter()
        r = fn()
        if sync:
            torch.cuda.synchronize()
        return r, time.perf_counter() - t0

    H = W = a.side
    depth, image, mask, K, render, internal = make_scene(a.side, a.render, a.internal)
    (world, colors, masks), t_points = wall(lambda: motion.pcd_points(image, mask, depth, K, render[0, :3, :3], render[0, :3, 3:4]))
    slots = motion.compose_slots(render, internal)
    (views, present, none_idx), t_views = wall(lambda: motion.pcd_views(world, K, slots, H, W))
    V = views.V
    say(f"{H} x {W}, {V} views ({len(none_idx)} see nothing), valid per view {min(map(len, views.valid))}..{max(map(len, views.valid))}")
    values = motion.pcd_values(views, colors, masks)

    def fresh():
        return motion.ViewSet(P=views.P, H=H, W=W, R=views.R, T=views.T, valid=views.valid, pix0=views.pix0, pix64=views.pix64)

    # ---- the new path by wall clock, triangulation included
    with gpu_step():
        torch.zeros(1, device=dev)
        torch.cuda.synchronize()
    new_path = []
    for w in a.workers:
        v = fresh()
        with gpu_step():
            _, t_tri = wall(lambda: motion.triangulate_views(v, workers=w))
            (im, ma), t_rest = wall(lambda: tuple(t.cpu() for t in motion.render_pcd_device(v, values, dev)), sync=True)
        new_path.append({"workers": w, "triangulate_views_s": round(t_tri, 2), "upload_kernels_download_s": round(t_rest, 3),
                         "whole_s": round(t_tri + t_rest, 2), "per_view_s": round((t_tri + t_rest) / V, 3)})
        say(f"new path, {w} workers: {new_path[-1]}")
        keep = v
    views = keep                                            # triangulated and uploaded
    tri_counts = [len(t) for t in views.simplices]

    # ---- the device part alone, per view, by events
    pk = motion.upload_views(views, dev)
    d_vals = motion.upload_values(views, values, dev)
    flow2d = torch.randn(V, views.P, 2, device=dev)
    with gpu_step():
        d_flow_vals = flow2d.reshape(V * views.P, 2).index_select(0, pk["gather"]).contiguous()
        res = ops.tri_resample(pk["pts"], pk["pt_off"], pk["tris"], pk["tri_off"], d_vals, H, W)
        ops.pcd_compose(res, pk["pts"], pk["pt_off"])
        torch.cuda.synchronize()

    def window(fn):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0.record()
        for _ in range(a.launches):
            fn()
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1) / a.launches / V

    out4 = torch.empty((V, H, W, 4), dtype=torch.float64, device=dev)
    out2 = torch.empty((V, H, W, 2), dtype=torch.float64, device=dev)
    scratch = torch.empty(V * H * W, dtype=torch.int32, device=dev)
    forms = {"resample_rgbm": lambda: ops.tri_resample(pk["pts"], pk["pt_off"], pk["tris"], pk["tri_off"], d_vals, H, W, out=out4, scratch=scratch),
             "compose": lambda: ops.pcd_compose(out4, pk["pts"], pk["pt_off"]),
             "resample_our_flow": lambda: ops.tri_resample(pk["pts"], pk["pt_off"], pk["tris"], pk["tri_off"], d_flow_vals, H, W, out=out2,
                                                           scratch=scratch)}
    kernels = {}
    for name, fn in forms.items():
        ms = []
        for _ in range(a.windows):
            with gpu_step():
                ms.append(window(fn))
        kernels[name] = {"median_ms_per_view": round(statistics.median(ms), 4), "min": round(min(ms), 4), "max": round(max(ms), 4),
                         "windows": [round(x, 4) for x in ms]}
        say(f"{name}: {kernels[name]}")
    with gpu_step():
        (_, t_flow) = wall(lambda: motion.resample_to_grid(views, flow2d, device=dev).permute(0, 3, 1, 2).cpu(), sync=True)
        res_host = out4.cpu().numpy()
        flow_host = out2.cpu().numpy()
        flow_vals_host = d_flow_vals.cpu().numpy()

    # ---- the host yardstick, and parity with griddata's own output on the same views
    x, y = np.meshgrid(np.arange(W, dtype=np.float32), np.arange(H, dtype=np.float32), indexing="xy")
    grid = np.stack((x, y), axis=-1).reshape(-1, 2)
    off = np.concatenate([[0], np.cumsum([len(v) for v in views.valid])])
    sample, host, parity = sorted({0, V // 2}), [], []
    for j in sample:
        pts = views.pix64[j].T
        rgb, t_rgb = wall(lambda: griddata(pts, colors[views.valid[j]], grid, method="linear", fill_value=0))
        _, t_depth = wall(lambda: griddata(pts, world[2, views.valid[j]][:, None], grid, method="linear", fill_value=0))
        _, t_mask = wall(lambda: griddata(pts, masks[views.valid[j]], grid, method="linear", fill_value=0))
        fl, t_fl = wall(lambda: griddata(pts, flow_vals_host[off[j]:off[j + 1]], grid, method="linear", fill_value=0))
        host.append({"view": j, "valid_points": int(len(pts)), "triangles": tri_counts[j], "render_pcd_three_calls_s": round(t_rgb + t_depth + t_mask, 2),
                     "one_three_channel_call_s": round(t_rgb, 2), "our_flow_call_s": round(t_fl, 2)})
        parity.append({"view": j,
                       "colours_largest_difference": float(np.abs(res_host[j, ..., :3].reshape(-1, 3) - rgb).max()),
                       "colours_same_fill_pixels": bool(np.array_equal((res_host[j, ..., :3].reshape(-1, 3) == 0).all(1), (rgb == 0).all(1))),
                       "our_flow_largest_difference_over_scale": float(np.abs(flow_host[j].reshape(-1, 2) - fl).max() / np.abs(fl).max())})
        say(f"griddata, view {j}: {host[-1]}; {parity[-1]}")

    per_view_new = {p["workers"]: p["per_view_s"] for p in new_path}
    one_call = min(h["one_three_channel_call_s"] for h in host)
    three = statistics.mean(h["render_pcd_three_calls_s"] for h in host)
    out = {"library": N.lib().mom_version().decode(), "device": torch.cuda.get_device_name(0), "H": H, "W": W, "V": V,
           "valid_per_view_min_max": [min(map(len, views.valid)), max(map(len, views.valid))],
           "triangles_per_view_min_max": [min(tri_counts), max(tri_counts)],
           "what": "new_path: host wall clock for all views, one call each; kernels: GPU time per view in ms between two torch.cuda.Event "
                   "records around --launches passes over all views, synchronised before and after each window; griddata: host wall clock",
           "host_cpus_used": "the thread pool's workers only; the box's CPU count is not read",
           "new_path": new_path, "kernels": kernels, "our_flow_resample_to_grid_wall_s_all_views": round(t_flow, 3),
           "griddata": {"views": host,
                        "render_pcd_extrapolated_x_V_s": round(three * V, 1),
                        "our_flow_extrapolated_x_V_s": round(statistics.mean(h["our_flow_call_s"] for h in host) * V, 1),
                        "note": f"two views timed once each; the figures for {V} views are their mean times {V}, an extrapolation"},
           "criterion": {"what": "a view's wall-clock cost on the new path (whole_s / V) against ONE three-channel griddata call of a view, same box",
                         "new_path_per_view_s_by_workers": per_view_new, "fastest_griddata_call_s": one_call,
                         "met_by_workers": {str(w): s < one_call for w, s in per_view_new.items()}},
           "host_bound": "the triangulation: scipy.spatial.Delaunay per view (triangulate_views_s); everything behind it is "
                         "upload_kernels_download_s",
           "parity_on_the_timed_views": parity,
           "not_measured": "no hardware counters (no rocprofv3 run); the rate of the integer atomics in the cover pass is not isolated; "
                           "real stage-1 depth maps"}
    txt = json.dumps(out, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(txt + "\n")
    print(txt)


if __name__ == "__main__":
    main()
