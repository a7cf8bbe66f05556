"""Frames/s of render_set with every frame written as a PNG, the host encoder against the device encoder, in one process on one model:
bench.py's config 2 scene, the `side` trajectory, one AsyncPNGWriter of each kind.

  host    AsyncPNGWriter(encoder="host"): raw RGB crosses to pinned memory, a pool of threads deflates it (zlib level 1, filter 0)
  device  AsyncPNGWriter(encoder="device"): mom_png_encode deflates on the GPU (csrc/png_encode.hip), the threads frame and write

After one warm-up pass of each, --windows windows of each alternate (host, device, host, ...); a window is one render_set over the
trajectory with video=False and its figure is render_set's own fps: (frames - 1) / seconds from the first render to the last file on
disk.  The record keeps every window, the median, lowest and highest of both writers, the criterion -- the slowest device window
against the fastest host window --, the bytes of the trajectory's files under both writers (the device writer's must not be larger),
the four encode kernels' time per frame between event pairs on three frames of the trajectory, and whether every file of the device
writer decodes (PIL) to the host writer's frame.

One process.  Every GPU step runs under an alarm of --step-limit seconds that ends the process; run it under a time limit as well
(timeout -k 10 600 python tools/png_rate.py ...).

    python tools/png_rate.py [--windows 5] [--launches 20] [--out profiles/png_rate.json]
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

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
pkg = "iclr2025_3d-mom_amd"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c2")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--launches", type=int, default=20, help="mom_png_encode calls per event pair")
    ap.add_argument("--step-limit", type=int, default=120, help="seconds any one GPU step may take before the process is ended")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.windows >= 5, "at least five windows of each writer"
    import torch
    from PIL import Image
    import bench
    N = importlib.import_module(pkg + "._native")
    ops = importlib.import_module(pkg + ".ops")
    own = importlib.import_module(pkg + ".render")
    R = importlib.import_module(pkg + ".gaussian_renderer")
    DGR = importlib.import_module(pkg + ".diff_gaussian_rasterization")
    assert torch.cuda.is_available(), "this tool measures on the GPU; there is nothing to fall back to"
    dev = torch.device("cuda", 0)
    say = lambda *s: print(*s, file=sys.stderr, flush=True)

    class gpu_step:
        """SIGALRM's default action ends the process, inside a blocked runtime call as well."""
        def __enter__(self):
            signal.alarm(a.step_limit)

        def __exit__(self, *exc):
            signal.alarm(0)

    with gpu_step():
        scene, g, trainer, op = bench.build_state(bench.CONFIGS[a.config], dev, fused=True)
    cams = scene.getVideoCameras_side()
    for c in cams:
        c.device_tensors(dev)
    H, W = int(cams[0].image_height), int(cams[0].image_width)
    pp, bg, ds = trainer.pipe, trainer.background, trainer.delta_scale
    tmp = tempfile.mkdtemp(prefix="mom_png_rate_")
    DGR.set_sync_mode("async")
    writers = {}
    try:
        with gpu_step():
            writers = {k: own.AsyncPNGWriter(H, W, encoder=k) for k in ("host", "device")}
        assert writers["device"].zcap > 0

        def window(kind):
            with gpu_step():
                return own.render_set(tmp, kind, 0, cams, g, pp, bg, scene.dataset_type, delta_scale=ds, video=False,
                                      writer=writers[kind])["fps"]
        for kind in ("host", "device"):
            say(f"warm-up {kind}: {window(kind):.0f} frames/s")
        fps = {"host": [], "device": []}
        for w in range(a.windows):
            for kind in ("host", "device"):
                fps[kind].append(window(kind))
                say(f"window {w} {kind}: {fps[kind][-1]:.0f} frames/s")

        def files(kind):
            d = os.path.join(tmp, "frame_result", kind)
            return [os.path.join(d, n) for n in sorted(os.listdir(d))]
        nbytes = {k: sum(os.path.getsize(p) for p in files(k)) for k in fps}
        assert len(files("host")) == len(files("device")) == len(cams)
        same = [bool(np.array_equal(np.asarray(Image.open(p)), np.asarray(Image.open(q)))) for p, q in zip(files("host"), files("device"))]
        say(f"bytes: host {nbytes['host']}, device {nbytes['device']}; {sum(same)} of {len(same)} frames decode alike")

        # ---- the encode kernels alone, on three frames of the trajectory
        DGR.set_sync_mode("exact")
        kernels = []
        rgb8 = torch.empty((H, W, 3), dtype=torch.uint8, device=dev)
        out = torch.empty(ops.png_bound(3, H, W), dtype=torch.uint8, device=dev)
        size = torch.zeros(1, dtype=torch.int32, device=dev)
        scratch = ops.png_scratch(3, H, W, dev)
        for i in sorted({0, len(cams) // 2, len(cams) - 1}):
            with gpu_step(), torch.no_grad():
                img = R.render(cams[i], g, pp, bg, stage="fine", cam_type=scene.dataset_type, delta_scale=ds)["render"].contiguous()
                N.check(N.lib().mom_image_to_rgb8(3, H, W, img.data_ptr(), rgb8.data_ptr(), N.current_stream()), "mom_image_to_rgb8")
                ops.png_encode(rgb8, out, size, scratch)
                torch.cuda.synchronize()
                ms = []
                for _ in range(a.windows):
                    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    t0.record()
                    for _ in range(a.launches):
                        ops.png_encode(rgb8, out, size, scratch)
                    t1.record()
                    torch.cuda.synchronize()
                    ms.append(t0.elapsed_time(t1) / a.launches)
            kernels.append({"frame": i, "stream_bytes": int(size.item()), "raw_bytes": H * W * 3,
                            "ms_per_frame_median": round(statistics.median(ms), 4), "ms_per_frame_windows": [round(x, 4) for x in ms]})
            say(f"frame {i}: {kernels[-1]}")
    finally:
        DGR.set_sync_mode("exact")
        for w in writers.values():
            w.close()
        shutil.rmtree(tmp, ignore_errors=True)

    summary = lambda v: {"median": round(statistics.median(v), 1), "lowest": round(min(v), 1), "highest": round(max(v), 1),
                         "windows": [round(x, 1) for x in v]}
    res = {"library": N.lib().mom_version().decode(), "device": torch.cuda.get_device_name(0), "config": a.config,
           "scene": bench.CONFIGS[a.config]["name"], "trajectory": f"side, {len(cams)} poses", "image": [H, W, 3],
           "what": "frames/s = (frames - 1) / seconds of render_set(video=False, writer=...), first render to last file on disk; windows "
                   "of the two writers alternate in one process after one warm-up pass of each",
           "cpus_in_affinity_mask": len(os.sched_getaffinity(0)), "writer_threads": writers["host"].pool._max_workers,
           "host_zlib_level": writers["host"].level,
           "frames_per_s": {k: summary(v) for k, v in fps.items()},
           "criterion_rate": {"slowest_device_window": round(min(fps["device"]), 1), "fastest_host_window": round(max(fps["host"]), 1),
                              "met": min(fps["device"]) >= max(fps["host"])},
           "file_bytes": {"host": nbytes["host"], "device": nbytes["device"], "frames": len(cams),
                          "device_over_host": round(nbytes["device"] / nbytes["host"], 4), "met": nbytes["device"] <= nbytes["host"]},
           "parity": {"frames": len(same), "device_files_decode_to_the_host_writers_frames": all(same)},
           "encode_kernels": {"what": "GPU time of one mom_png_encode (plan, scan, encode, compact) in ms, between two torch.cuda.Event "
                                      "records around --launches calls on an otherwise idle device", "launches": a.launches,
                              "frames": kernels},
           "not_measured": "no hardware counters of the encode kernels (no rocprofv3 run); only the synthetic scene's frames; only this "
                           "machine's file system (a temporary directory)"}
    txt = json.dumps(res, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(txt + "\n")
    print(txt)
    if not (res["parity"]["device_files_decode_to_the_host_writers_frames"] and res["criterion_rate"]["met"] and res["file_bytes"]["met"]):
        sys.exit(2)


if __name__ == "__main__":
    main()
