"""Frames/s of render_set with the video written as Motion-JPEG, the host route against the device route, in one process on one
model: bench.py's config 2 scene, the `side` trajectory, the PNG frames written as always (one AsyncPNGWriter, the default encoder).

  host    MOM_VIDEO_ENCODER=host: every frame's crop crosses to the host through to8b and a pool of threads encodes it with PIL
  device  MOM_VIDEO_ENCODER=device: mom_jpeg_encode_chw encodes on the GPU behind the frame's kernels (csrc/jpeg_encode.hip), the
          threads only collect the finished files

After one warm-up pass of each, --windows windows of each alternate (host, device, host, ...); a window is one render_set over the
trajectory.  Two figures per window: render_set's own fps ((frames - 1) / seconds from the first render to the last PNG on disk,
the video's frames still being collected) and frames / seconds of the whole call, the AVI on disk.  The record keeps every window,
the bytes of the two AVI files and whether they are the same frames byte for byte, and the three encode kernels' time per frame
between event pairs on three frames of the trajectory.  Nothing here is a pass condition.

One process.  Every GPU step runs under an alarm of --step-limit seconds that ends the process; run it under a time limit as well
(timeout -k 10 600 python tools/video_rate.py ...).

    python tools/video_rate.py [--windows 5] [--launches 20] [--out profiles/video_rate.json]
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

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
pkg = "iclr2025_3d-mom_amd"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c2")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--launches", type=int, default=20, help="mom_jpeg_encode_chw calls per event pair")
    ap.add_argument("--step-limit", type=int, default=120, help="seconds any one GPU step may take before the process is ended")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import bench
    import jpeg_cases as J
    N = importlib.import_module(pkg + "._native")
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
    vh, vw = H - 64, W - 64
    pp, bg, ds = trainer.pipe, trainer.background, trainer.delta_scale
    tmp = tempfile.mkdtemp(prefix="mom_video_rate_")
    DGR.set_sync_mode("async")
    quality = int(os.environ.get("MOM_VIDEO_QUALITY") or 90)
    writer = None
    try:
        with gpu_step():
            writer = own.AsyncPNGWriter(H, W)

        def window(kind):
            os.environ["MOM_VIDEO_ENCODER"] = kind
            with gpu_step():
                t0 = time.time()
                r = own.render_set(os.path.join(tmp, kind), "side", 0, cams, g, pp, bg, scene.dataset_type, delta_scale=ds, writer=writer)
                return r["fps"], len(cams) / (time.time() - t0)
        for kind in ("host", "device"):
            say(f"warm-up {kind}: {window(kind)}")
        fps = {"host": [], "device": []}
        whole = {"host": [], "device": []}
        for w in range(a.windows):
            for kind in ("host", "device"):
                f, t = window(kind)
                fps[kind].append(f)
                whole[kind].append(t)
                say(f"window {w} {kind}: {f:.0f} frames/s to the last PNG, {t:.0f} frames/s with the AVI on disk")
        avi = {k: open(os.path.join(tmp, k, "vid_result", "side.avi"), "rb").read() for k in fps}
        parsed = {k: J.parse_avi(v) for k, v in avi.items()}
        same = [p == q for p, q in zip(parsed["host"]["frames"], parsed["device"]["frames"])]
        assert len(parsed["host"]["frames"]) == len(parsed["device"]["frames"]) == len(cams)
        say(f"bytes: host {len(avi['host'])}, device {len(avi['device'])}; {sum(same)} of {len(same)} frames are the same bytes")

        # ---- the encode kernels alone, on three frames of the trajectory
        DGR.set_sync_mode("exact")
        kernels = []
        lib = N.lib()
        bound = int(lib.mom_jpeg_bound(vh, vw))
        out = torch.empty(bound, dtype=torch.uint8, device=dev)
        size = torch.zeros(1, dtype=torch.int32, device=dev)
        scratch = torch.empty(int(lib.mom_jpeg_scratch_bytes(vh, vw)), dtype=torch.uint8, device=dev)
        for i in sorted({0, len(cams) // 2, len(cams) - 1}):
            with gpu_step(), torch.no_grad():
                img = R.render(cams[i], g, pp, bg, stage="fine", cam_type=scene.dataset_type, delta_scale=ds)["render"].contiguous()

                def encode():
                    N.check(lib.mom_jpeg_encode_chw(H, W, 32, 32, vh, vw, img.data_ptr(), quality, out.data_ptr(), bound, size.data_ptr(),
                                                    scratch.data_ptr(), N.current_stream()), "mom_jpeg_encode_chw")
                encode()
                torch.cuda.synchronize()
                ms = []
                for _ in range(a.windows):
                    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    t0.record()
                    for _ in range(a.launches):
                        encode()
                    t1.record()
                    torch.cuda.synchronize()
                    ms.append(t0.elapsed_time(t1) / a.launches)
            kernels.append({"frame": i, "file_bytes": int(size.item()), "raw_bytes": vh * vw * 3,
                            "ms_per_frame_median": round(statistics.median(ms), 4), "ms_per_frame_windows": [round(x, 4) for x in ms]})
            say(f"frame {i}: {kernels[-1]}")
    finally:
        DGR.set_sync_mode("exact")
        os.environ.pop("MOM_VIDEO_ENCODER", None)
        if writer is not None:
            writer.close()
        shutil.rmtree(tmp, ignore_errors=True)

    summary = lambda v: {"median": round(statistics.median(v), 1), "lowest": round(min(v), 1), "highest": round(max(v), 1),
                         "windows": [round(x, 1) for x in v]}
    res = {"library": N.lib().mom_version().decode(), "device": torch.cuda.get_device_name(0), "config": a.config,
           "scene": bench.CONFIGS[a.config]["name"], "trajectory": f"side, {len(cams)} poses", "image": [H, W, 3], "video_frame": [vh, vw, 3],
           "quality": quality,
           "what": "render_set(video=True, writer=one AsyncPNGWriter) under MOM_VIDEO_ENCODER=host / device; windows of the two routes "
                   "alternate in one process after one warm-up pass of each",
           "cpus_in_affinity_mask": len(os.sched_getaffinity(0)),
           "frames_per_s_to_the_last_png": {k: summary(v) for k, v in fps.items()},
           "frames_per_s_with_the_avi_on_disk": {k: summary(v) for k, v in whole.items()},
           "file_bytes": {"host": len(avi["host"]), "device": len(avi["device"]), "frames": len(cams)},
           "parity": {"frames": len(same), "device_frames_are_the_host_routes_bytes": all(same)},
           "encode_kernels": {"what": "GPU time of one mom_jpeg_encode_chw (transform, entropy, compact) in ms, between two torch.cuda.Event "
                                      "records around --launches calls on an otherwise idle device", "launches": a.launches,
                              "frames": kernels},
           "not_measured": "no hardware counters of the encode kernels (no rocprofv3 run); only the synthetic scene's frames; only this "
                           "machine's file system (a temporary directory); no player was run on the files"}
    txt = json.dumps(res, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(txt + "\n")
    print(txt)
    if not res["parity"]["device_frames_are_the_host_routes_bytes"]:
        sys.exit(2)


if __name__ == "__main__":
    main()
