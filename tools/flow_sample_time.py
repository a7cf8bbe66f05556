"""Time of sampling the 2D flow images for one scene-flow fit at the reference's size (P = 512 x 512 points, 14 x 5 views, 512 x 512
flow images), two forms in one process:

  griddata  the reference's path (train_motion.py:117-121, motion.sample_flow_image): scipy.interpolate.griddata once per view on the
            host.  Three views are timed, once each (first, middle, last); "x 70" is an extrapolation and labelled so
  kernel    motion's sampler="device" path: ops.flow_sample, one launch for all views (csrc/flow_sample.hip)

The scene is tools/sceneflow_fit_time.py's (a 512 x 512 depth map back-projected with the stage-1 intrinsics, its 70 poses); the flow
images are smooth, a few pixels in size.  A kernel window is --launches launches of all views (the figure is per launch) between a
torch.cuda.Event pair, ending in one synchronisation; five windows after a warm-up.  The record keeps every window, the criterion --
the slowest kernel window against the fastest single-view griddata call --, the rate over the algorithmic bytes, the time of
motion.grid_diagonals cold and from its cache, the whole sampler="device" fit by wall clock with its parts, and the parity of the
kernel's records with the float64 restatement (tests/flow_sample_cases.py) and with griddata's own results on the three timed views.

One process.  Every GPU step runs under an alarm of --step-limit seconds that ends the process (nothing is started behind a step
that hangs); run it under a time limit as well (timeout -k 10 600 python tools/flow_sample_time.py ...).

    python tools/flow_sample_time.py [--windows 5] [--launches 20] [--epochs 200] [--out profiles/flow_sample_time.json]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
pkg = "iclr2025_3d-mom_amd"

from sceneflow_fit_time import STREAM_TBPS, make_scene          # noqa: E402  (tools/ is this script's directory)


def smooth_images(V, H, W):
    """[V,2,H,W] float32: sinusoids of 3 px, another phase per view and channel."""
    y, x = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    out = np.empty((V, 2, H, W), np.float32)
    for j in range(V):
        out[j, 0] = 3.0 * np.sin(x * (5 * math.pi / W) + 0.3 * j) * np.cos(y * (3 * math.pi / H) + 0.1 * j)
        out[j, 1] = 2.0 * np.cos(x * (4 * math.pi / W) - 0.2 * j) + 1.5 * np.sin(y * (6 * math.pi / H) + 0.05 * j)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=512, help="the point cloud and the flow images are side x side")
    ap.add_argument("--render", type=int, default=14)
    ap.add_argument("--internal", type=int, default=5)
    ap.add_argument("--epochs", type=int, default=200)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--launches", type=int, default=20, help="kernel launches per window")
    ap.add_argument("--step-limit", type=int, default=120, help="seconds any one GPU step may take before the process is ended")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import flow_sample_cases as fc
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
    (pts, K, views, _), t_scene = wall(lambda: make_scene(a.side, a.render, a.internal))
    V, P = views.V, views.P
    images = smooth_images(V, H, W)
    say(f"P {P}  V {V}  valid per view {min(map(len, views.valid))}..{max(map(len, views.valid))}  scene {t_scene:.1f} s")

    # ---- the triangulation, cold and from the cache
    mask, t_tri = wall(lambda: motion.grid_diagonals(H, W))
    _, t_tri_cached = wall(lambda: motion.grid_diagonals(H, W))
    say(f"grid_diagonals({H}, {W}): {t_tri:.2f} s, again {t_tri_cached * 1e6:.1f} us; {mask.mean():.3f} anti-diagonal")

    # ---- the parts of sample_flow_images, one by one
    _, t_prepare = wall(lambda: motion.prepare_views(pts, K, [(views.R[j].astype(np.float64), views.T[j].astype(np.float64))
                                                              for j in range(V)], H, W))

    def dense():
        pix = np.zeros((V, P, 2), np.float64)
        for j, idx in enumerate(views.valid):
            pix[j, idx] = views.pix64[j].T
        return pix, motion.valid_words(views), motion.pack_diagonals(mask)
    (pix, bits, words), t_dense = wall(dense)
    with gpu_step():
        (d_img, d_pix, d_bits, d_words), t_upload = wall(lambda: [motion._upload(x, dev) for x in (images, pix, bits, words)], sync=True)
    rec = torch.empty((V, P, 4), dtype=torch.float32, device=dev)
    with gpu_step():
        d_img = d_img.permute(0, 2, 3, 1).contiguous()
        ops.flow_sample(d_img, d_pix, d_bits, d_words, rec)                  # warm-up
        torch.cuda.synchronize()

    def window():
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0.record()
        for _ in range(a.launches):
            ops.flow_sample(d_img, d_pix, d_bits, d_words, rec)
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1) / a.launches
    kernel_ms = []
    for w in range(a.windows):
        with gpu_step():
            kernel_ms.append(window())
        say(f"window {w}: {kernel_ms[-1] * 1e3:.1f} us per launch of {V} views")
    with gpu_step():
        _, t_one = wall(lambda: ops.flow_sample(d_img, d_pix, d_bits, d_words, rec), sync=True)
        rec_host = rec.cpu().numpy()

    # ---- the host yardstick and the parity on the same three views
    sample, griddata_s, parity = sorted({0, V // 2, V - 1}), [], []
    for j in sample:
        idx = views.valid[j]
        got, t = wall(lambda: motion.sample_flow_image(torch.from_numpy(images[j:j + 1]), views.pix64[j], H, W))
        griddata_s.append(t)
        want, cmax = fc.restate(images[j], views.pix64[j].T, mask, corners=True)
        k = rec_host[j, idx, 2:].astype(np.float64)
        d = np.abs(k - want.astype(np.float32))
        out = np.ones(P, bool)
        out[idx] = False
        parity.append({"view": j, "valid_points": int(len(idx)),
                       "within_one_float32_ulp_of_the_largest_corner": bool((d <= 2.0 ** -23 * cmax).all()),
                       "gt_bit_equal_share": float((rec_host[j, idx, 2:].view(np.uint32) == want.astype(np.float32).view(np.uint32)).mean()),
                       "pix0_bit_equal": bool(np.array_equal(rec_host[j, idx, :2], views.pix0[j].T)),
                       "invalid_records_all_zero": bool(not rec_host[j, out].any()),
                       "restatement_against_griddata_over_scale": float(np.abs(want - got.T).max() / np.abs(images[j]).max()),
                       "kernel_against_float32_of_griddata_largest": float(np.abs(k - got.T.astype(np.float32)).max()),
                       "image_scale": float(np.abs(images[j]).max())})
        say(f"view {j}: griddata {t:.2f} s; {parity[-1]}")

    # ---- the whole sampler="device" fit by wall clock (triangulation from the cache), and the fit alone
    def whole():
        v = motion.prepare_views(pts, K, [(views.R[j].astype(np.float64), views.T[j].astype(np.float64)) for j in range(V)], H, W)
        return motion.fit_scene_flow(pts, K, v, None, epochs=a.epochs, records=motion.sample_flow_images(v, torch.from_numpy(images)))
    with gpu_step():
        _, t_fit = wall(lambda: motion.fit_scene_flow(pts, K, views, None, epochs=a.epochs, records=(rec, d_bits)), sync=True)
    with gpu_step():
        _, t_whole = wall(whole, sync=True)
    say(f"whole device-sampled fit {t_whole:.2f} s (fit_scene_flow alone {t_fit * 1e3:.1f} ms)")

    nbytes = V * P * (16 + 16) + V * H * W * 8 + words.nbytes + bits.nbytes
    med = statistics.median(kernel_ms)
    tbps = nbytes / (med * 1e-3) / 1e12
    out = {"library": N.lib().mom_version().decode(), "device": torch.cuda.get_device_name(0), "P": P, "V": V, "H": H, "W": W,
           "valid_per_view_min_max": [min(map(len, views.valid)), max(map(len, views.valid))],
           "what": "kernel: GPU time of one launch for all V views in ms, between two torch.cuda.Event records around --launches "
                   "launches, device synchronised before and after each window; griddata: host wall clock of one call, one view",
           "windows": a.windows, "launches_per_window": a.launches,
           "kernel": {"median_ms": round(med, 4), "min_ms": round(min(kernel_ms), 4), "max_ms": round(max(kernel_ms), 4),
                      "windows_ms": [round(x, 4) for x in kernel_ms], "one_launch_wall_ms_with_synchronise": round(t_one * 1e3, 3)},
           "griddata": {"views": sample, "seconds_per_view": [round(t, 2) for t in griddata_s],
                        "extrapolated_x_V_seconds": round(statistics.mean(griddata_s) * V, 1),
                        "note": f"three calls timed once each; the figure for {V} views is their mean times {V}, an extrapolation"},
           "criterion": {"slowest_kernel_window_ms_all_views": round(max(kernel_ms), 4),
                         "fastest_griddata_call_ms_one_view": round(min(griddata_s) * 1e3, 1),
                         "met": max(kernel_ms) < min(griddata_s) * 1e3},
           "algorithmic_bytes": nbytes,
           "algorithmic_bytes_are": "V x P x (16 pix + 16 record) + V x H x W x 8 + the diagonal bitmap + the validity words",
           "kernel_TB_per_s": round(tbps, 3), "streaming_read_TB_per_s_of_the_device": list(STREAM_TBPS),
           "share_of_streaming_rate": round(tbps / STREAM_TBPS[0], 3),
           "bound": "memory: about 0.4 float64 operations per byte, far below the device's balance; the least time is the algorithmic bytes "
                    "over the streaming rate (two fifths of them are writes, so the read rate is an upper bound on what a copy reaches)",
           "grid_diagonals_s": {"first_call": round(t_tri, 2), "from_the_cache": round(t_tri_cached, 7),
                                "anti_diagonal_share": round(float(mask.mean()), 4)},
           "device_sampled_fit_wall_s": {"whole_with_cached_triangulation": round(t_whole, 3), "epochs": a.epochs,
                                         "parts": {"triangulation_first_call": round(t_tri, 2), "prepare_views": round(t_prepare, 3),
                                                   "dense_pixels_and_bit_words_on_the_host": round(t_dense, 3),
                                                   "upload_pinned": round(t_upload, 3), "kernel_one_launch": round(t_one, 5),
                                                   "fit_scene_flow_with_device_records": round(t_fit, 4)}},
           "parity_on_the_timed_views": parity,
           "not_measured": "no hardware counters (no rocprofv3 run): the rate is algorithmic bytes over event time"}
    txt = json.dumps(out, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(txt + "\n")
    print(txt)
    if not out["criterion"]["met"] or not all(p["within_one_float32_ulp_of_the_largest_corner"] for p in parity):
        sys.exit(2)


if __name__ == "__main__":
    main()
