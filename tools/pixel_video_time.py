"""Seconds of motion.write_pixel_video with the host writer against the device writer, in one process, and of motion_rgbs on the host
against the device.

  host    the frames cross to the host as float32; each is quantised by numpy, resized by PIL and deflated by zlib on the calling thread
  device  each frame is quantised and resized by ops.pil_resize(to8b=True) (csrc/pil_resize.hip) and deflated by mom_png_encode as it is
          made; the host frames the finished zlib stream and writes it

Leg 1: a stage-1 directory with a --data x --data centre frame; after one warm-up pass of each writer, --windows windows of each
alternate (host, device, host, ...).  A window is one write_pixel_video(n_frames, size) and its figure is the wall clock from the call
to its return, which is behind the PNG writer's close(): every file is on disk.  The record keeps every window and the median, lowest
and highest per writer.
Separately: the resize kernels' time per frame (one float32 frame size x size -> data x data) between two event records around
--launches calls, its algorithmic bytes (the float frame in, the byte frame out) over that time, and whether the kernels' bytes of
one frame of the video are PIL's of the quantised frame.
Leg 2: motion_rgbs of --views views, --rgb-in -> --rgb-out, resizer "pil" against "device", each ending with the images on the device
and a device synchronise, alternating in the same way.

One process.  Every GPU step runs under an alarm of --step-limit seconds that ends the process; run it under a time limit as well
(timeout -k 10 600 python tools/pixel_video_time.py ...).

    python tools/pixel_video_time.py [--windows 5] [--out profiles/pixel_video_time.json]
"""
import argparse
import importlib
import json
import os
import shutil
import signal
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
pkg = "iclr2025_3d-mom_amd"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--n-frames", type=int, default=120)
    ap.add_argument("--size", type=int, default=1024, help="side of the square the warp runs at")
    ap.add_argument("--data", type=int, default=512, help="W = H of the data, the size the frames are written at")
    ap.add_argument("--views", type=int, default=70)
    ap.add_argument("--rgb-in", type=int, default=512)
    ap.add_argument("--rgb-out", type=int, default=768)
    ap.add_argument("--launches", type=int, default=20, help="ops.pil_resize calls per event pair")
    ap.add_argument("--step-limit", type=int, default=120, help="seconds any one GPU step may take before the process is ended")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.windows >= 5, "at least five windows of each route"
    import torch
    from PIL import Image
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

    # ---- leg 1: the video
    rng = np.random.default_rng(1)
    D = a.data
    yy, xx = np.meshgrid(np.arange(D, dtype=np.float32), np.arange(D, dtype=np.float32), indexing="ij")
    # a smooth image with noise on it: neither the best nor the worst case of either deflate
    image = (127 + 90 * np.sin(xx / 37)[..., None] * np.cos(yy / 23)[..., None] + rng.normal(0, 12, (D, D, 3))).clip(0, 255).astype(np.uint8)
    mask = np.zeros((D, D), np.uint8)
    mask[D // 4:3 * D // 4, D // 4:] = 255
    flow = torch.from_numpy(np.stack([0.5 * np.sin(yy / 40), 0.5 * np.cos(xx / 55)]).astype(np.float32))[None]
    tmp = tempfile.mkdtemp(prefix="mom_pixel_video_time_")
    try:
        mom = os.path.join(tmp, "MOM")
        os.makedirs(mom)
        frame = lambda: {"image": Image.fromarray(image), "mask": Image.fromarray(mask), "our_flow": [flow.clone()],
                         "transform_matrix": np.eye(4).tolist()}
        torch.save({"camera_angle_x": 0.6, "camera_angle_y": 0.6, "W": D, "H": D, "pcd_points": np.zeros((3, 4), np.float32),
                    "pcd_colors": np.zeros((4, 3), np.float32), "frames": [frame() for _ in range(3)]}, os.path.join(mom, "train_data.pth"))

        def window(kind):
            with gpu_step():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                paths = motion.write_pixel_video(tmp, n_frames=a.n_frames, size=a.size, writer=kind)
                return time.perf_counter() - t0, paths
        for kind in ("host", "device"):
            say(f"warm-up {kind}: {window(kind)[0]:.3f} s")
        secs = {"host": [], "device": []}
        for w in range(a.windows):
            for kind in ("host", "device"):
                s, paths = window(kind)
                secs[kind].append(s)
                say(f"window {w} {kind}: {s:.3f} s")
        nbytes = sum(os.path.getsize(p) for p in paths)

        # ---- the resize kernels alone, and the last window's files against them
        cg = importlib.import_module(pkg + ".cinemagraph")
        with gpu_step():
            frames = list(cg.pixel_video_frames(image, flow, mask, n_frames=3, size=a.size))
            x = frames[1]
            rgb8 = torch.empty((D, D, 3), dtype=torch.uint8, device=dev)
            scratch = ops.pil_resize_scratch(x.shape, (D, D), dev)
            ops.pil_resize(x, (D, D), to8b=True, out=rgb8, scratch=scratch)
            torch.cuda.synchronize()
            ms = []
            for _ in range(a.windows):
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                for _ in range(a.launches):
                    ops.pil_resize(x, (D, D), to8b=True, out=rgb8, scratch=scratch)
                t1.record()
                torch.cuda.synchronize()
                ms.append(t0.elapsed_time(t1) / a.launches)
            q = (frames[0].cpu().numpy() * 255).astype(np.uint8)
            want = np.array(Image.fromarray(q).resize((D, D)))
            got_dev = ops.pil_resize(frames[0], (D, D), to8b=True).cpu().numpy()
            kernel_is_pil = bool(np.array_equal(got_dev, want))
        algo_bytes = a.size * a.size * 3 * 4 + D * D * 3
        kern = {"ms_per_frame_median": round(statistics.median(ms), 4), "ms_per_frame_windows": [round(v, 4) for v in ms],
                "algorithmic_bytes": algo_bytes, "intermediate_bytes_written_and_read": 2 * int(scratch.numel()) if scratch is not None else 0,
                "algorithmic_GB_per_s": round(algo_bytes / (statistics.median(ms) * 1e-3) / 1e9, 1),
                "frame_0_equals_pil_of_the_quantised_frame": kernel_is_pil}
        say(f"resize kernels: {kern}")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)

    # ---- leg 2: motion_rgbs
    views = [{"image": Image.fromarray(rng.integers(0, 256, (a.rgb_in, a.rgb_in, 3), dtype=np.uint8))} for _ in range(a.views)]

    def rgbs(kind):
        with gpu_step():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            t = motion._upload(motion.motion_rgbs(views, a.rgb_out, resizer=kind, device=dev), dev)
            torch.cuda.synchronize()
            return time.perf_counter() - t0, t
    same = None
    rsecs = {"pil": [], "device": []}
    for w in range(a.windows + 1):                      # window 0 of each is the warm-up
        got = {}
        for kind in ("pil", "device"):
            s, got[kind] = rgbs(kind)
            if w:
                rsecs[kind].append(s)
            say(f"motion_rgbs window {w} {kind}: {s:.3f} s")
        if same is None:
            same = bool(torch.equal(got["pil"], got["device"]))
        del got

    summary = lambda v: {"median": round(statistics.median(v), 4), "lowest": round(min(v), 4), "highest": round(max(v), 4),
                         "windows": [round(x, 4) for x in v]}
    res = {"library": N.lib().mom_version().decode(), "device": torch.cuda.get_device_name(0),
           "cpus_in_affinity_mask": len(os.sched_getaffinity(0)),
           "video": {"what": f"seconds of motion.write_pixel_video(n_frames={a.n_frames}, size={a.size}) writing {D} x {D} PNGs, call to "
                             "return (every file on disk); windows of the two writers alternate in one process after one warm-up pass of each",
                     "seconds": {k: summary(v) for k, v in secs.items()},
                     "device_faster_than_host": statistics.median(secs["device"]) < statistics.median(secs["host"]),
                     "device_files_bytes": nbytes, "resize_kernels": kern},
           "motion_rgbs": {"what": f"seconds of motion_rgbs of {a.views} views {a.rgb_in} -> {a.rgb_out}, the result on the device, "
                                   "ending in a device synchronise; alternating windows after one warm-up of each",
                           "seconds": {k: summary(v) for k, v in rsecs.items()},
                           "device_faster_than_pil": statistics.median(rsecs["device"]) < statistics.median(rsecs["pil"]),
                           "device_equals_pil_bit_for_bit": same},
           "not_measured": "no hardware counters (no rocprofv3 run); only this synthetic frame; only this machine's file system (a "
                           "temporary directory); the host writer's share depends on the host's cores, which this tool does not vary"}
    txt = json.dumps(res, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(txt + "\n")
    print(txt)
    if not (kernel_is_pil and same):
        sys.exit(2)


if __name__ == "__main__":
    main()
