"""Time of the triangulation of stage 1's views at the reference's size -- a 512 x 512 source image, 14 x 5 views, the scene of
tools/pcd_views_time.py -- on the two routes of motion.triangulate_views, in alternating windows of one process:

  host      triangulate_views(triangulator="host"): scipy.spatial.Delaunay per view, 8 threads and 1 thread, by wall clock
  device    ops.delaunay (mom_delaunay alone) over the uploaded points, in the chunks of views upload_views uses, a chunk at a
            time between a torch.cuda.Event pair (the chunks' times added); then its deferred points, largest star and the views it refused
  render    motion.render_pcd_device end to end on a fresh ViewSet (triangulation, upload, resampling, compose, download) on both
            routes, by wall clock; the device route's frames are compared with the host route's

The comparison partner of the device route is the 8-thread pool of the same process.  The 1-thread pool is slow (about a minute a
window): --windows-one sets how often it is timed.

One process.  Every GPU step runs under an alarm of --step-limit seconds that ends the process; run it under a time limit as well.

    python tools/delaunay_time.py [--side 512] [--windows 3] [--out profiles/delaunay_time.json]
"""
import argparse
import importlib
import json
import os
import signal
import statistics
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
pkg = "iclr2025_3d-mom_amd"

from pcd_views_time import make_scene          # noqa: E402  (tools/ is this script's directory)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=512)
    ap.add_argument("--render", type=int, default=14)
    ap.add_argument("--internal", type=int, default=5)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--windows-one", type=int, default=1, help="windows of the 1-thread pool")
    ap.add_argument("--step-limit", type=int, default=300, help="seconds any one GPU step may take before the process is ended")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
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

    def wall(fn):
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return r, time.perf_counter() - t0

    H = W = a.side
    depth, image, mask, K, render, internal = make_scene(a.side, a.render, a.internal)
    world, colors, masks = motion.pcd_points(image, mask, depth, K, render[0, :3, :3], render[0, :3, 3:4])
    views, _, none_idx = motion.pcd_views(world, K, motion.compose_slots(render, internal), H, W)
    V, counts = views.V, [len(v) for v in views.valid]
    values = motion.pcd_values(views, colors, masks)
    say(f"{H} x {W}, {V} views, valid per view {min(counts)}..{max(counts)}")
    fresh = lambda: motion.ViewSet(P=views.P, H=H, W=W, R=views.R, T=views.T, valid=views.valid, pix0=views.pix0, pix64=views.pix64)

    # ---- the device route's pieces: the points on the device, the chunks, one scratch
    with gpu_step():
        pts = torch.from_numpy(np.concatenate([p.T for p in views.pix64]).astype(np.float64)).to(dev)
        off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        chunks = motion._delaunay_chunks(counts, H, W)
        local = [torch.from_numpy((off[j0:j1 + 1] - off[j0]).astype(np.int32)).to(dev) for j0, j1 in chunks]
        scratch = torch.empty(max(ops.delaunay_scratch_elements(j1 - j0, H, W, int(off[j1] - off[j0])) for j0, j1 in chunks),
                              dtype=torch.int32, device=dev)
        torch.cuda.synchronize()

    def device_window():
        """All views, chunk by chunk: each chunk's launches between its own event pair and under its own alarm."""
        out, total = [], 0.0
        for (j0, j1), lo in zip(chunks, local):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with gpu_step():
                torch.cuda.synchronize()
                t0.record()
                tris, tri_off, status = ops.delaunay(pts[off[j0]:off[j1]], lo, H, W, scratch=scratch)
                t1.record()
                torch.cuda.synchronize()
                out.append((status, tri_off, scratch[:2].clone()))
            total += t0.elapsed_time(t1) / 1e3
        return out, total

    first, t_first = device_window()                           # the warm-up window, reported apart
    status = np.concatenate([s.cpu().numpy() for s, _, _ in first])
    stats = {"deferred_points": int(sum(int(h[0]) for _, _, h in first)), "largest_star": int(max(int(h[1]) for _, _, h in first)),
             "points": int(off[-1]), "triangles": int(sum(int(t[-1]) for _, t, _ in first)),
             "views_refused": [[int(j), int(s)] for j, s in enumerate(status) if s != 0], "chunks": [list(c) for c in chunks]}
    say(f"device, first window {t_first:.3f} s: {stats}")

    host8, host1, device_s = [], [], []
    for w in range(a.windows):
        host8.append(wall(lambda: motion.triangulate_views(fresh(), workers=8))[1])
        device_s.append(device_window()[1])
        if w < a.windows_one:
            host1.append(wall(lambda: motion.triangulate_views(fresh(), workers=1))[1])
        say(f"window {w}: host 8 threads {host8[-1]:.2f} s, device {device_s[-1]:.3f} s" + (f", host 1 thread {host1[-1]:.2f} s" if w < a.windows_one else ""))

    # ---- render_pcd_device end to end, both routes, alternating
    end = {"host": [], "device": []}
    frames, fallbacks = {}, None
    for w in range(a.windows):
        for route in ("host", "device"):
            v = fresh()
            with gpu_step():
                out, t = wall(lambda: tuple(t_.cpu() for t_ in motion.render_pcd_device(v, values, dev, workers=8, triangulator=route)))
            end[route].append(t)
            frames[route] = out
            if route == "device":
                fallbacks = [[int(j), int(s)] for j, s in v.fallbacks]
        say(f"window {w}: render_pcd_device host route {end['host'][-1]:.2f} s, device route {end['device'][-1]:.2f} s")
    same = all(bool(torch.equal(x, y)) for x, y in zip(frames["host"], frames["device"]))

    box = lambda xs: {"median_s": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4),
                      "windows": [round(x, 4) for x in xs]} if xs else None
    out = {"library": N.lib().mom_version().decode(), "device": torch.cuda.get_device_name(0), "H": H, "W": W, "V": V,
           "valid_per_view_min_max": [min(counts), max(counts)],
           "what": "triangulate_views: host wall clock for all views; mom_delaunay: GPU time for all views between two torch.cuda.Event "
                   "records, synchronised before and after each window, the windows alternating with the host pool's in one process; "
                   "render_pcd_device: wall clock from a fresh ViewSet to the frames on the host",
           "host_cpus_used": "the thread pool's workers only; the box's CPU count is not read",
           "triangulate_views_8_threads": box(host8), "triangulate_views_1_thread": box(host1),
           "mom_delaunay_all_views": box(device_s), "mom_delaunay_first_window_s": round(t_first, 4), "mom_delaunay": stats,
           "render_pcd_device_host_route": box(end["host"]), "render_pcd_device_device_route": box(end["device"]),
           "device_route_fallbacks": fallbacks, "device_route_frames_equal_host_route": same,
           "not_measured": "no hardware counters (no rocprofv3 run); the lane and the deferred launch are not timed apart; real stage-1 "
                           "depth maps"}
    txt = json.dumps(out, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(txt + "\n")
    print(txt)


if __name__ == "__main__":
    main()
