"""Time of the video generator's warp with the ordered splat against the atomic one: cinemagraph.warp_one_level (blend + finish, the
fused route) with ordered=False and ordered=True in one process, alternating windows, at

  S 1024, C 32   frames 0, 60 and 119 of 120 (the widest level the reference warps)
  S 128, C 256   frame 60
  S 1024, C 3    frame 60 (the pixel route)

and cinemagraph.pixel_video's frames per second for 120 frames at 1024 by wall clock, both ways.  The comparison partner of the
ordered form is the atomic form of the same process, never an earlier run.  Also: the ordered call's scratch bytes
(mom_eulerian_ordered_scratch_bytes), the longest cell of every measured frame (the entries one lane walks serially; counted from the
displacements themselves), and the ordered blend's time by kernel from ONE `rocprofv3 --kernel-trace --stats` run of a fresh child
process of this script (S 1024, C 32, frame 60), started before this process touches the GPU.  If that child ends with any
status but 0 -- a fault, an abort, its alarm -- this process ends there with a non-zero status and starts nothing on the GPU;
--no-trace measures without the child.

The flow is tools/eulerian_warp_time.py's: smooth, about --px pixels per frame at 1024 with a still region.  A window is --calls calls
between a torch.cuda.Event pair, the device synchronised before and after; --windows windows per form after a warm-up call of each;
the median is reported with the lowest and the highest window.  Every GPU step runs under an alarm of --step-limit seconds that ends
the process; run it under a time limit as well (timeout -k 10 600 python tools/eulerian_ordered_time.py ...).

    python tools/eulerian_ordered_time.py [--windows 5] [--calls 3] [--no-trace] [--out profiles/eulerian_ordered_time.json]
"""
import argparse
import csv
import glob
import importlib
import json
import os
import shutil
import signal
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
pkg = "iclr2025_3d-mom_amd"
SHAPES = [(1024, 32, (0, 60, 119)), (128, 256, (60,)), (1024, 3, (60,))]
N_FRAMES = 120
TRACE_SHAPE = (1024, 32, 60)


def kernel_trace(px, limit):
    """One rocprofv3 kernel trace of a child that runs the ordered blend alone: [{kernel, calls, average_us}] of its kernels."""
    if shutil.which("rocprofv3") is None:               # nothing has touched the GPU yet: the windows may still be measured
        return {"skipped": "no rocprofv3 on PATH"}
    out = tempfile.mkdtemp(prefix="eulerian_ordered_trace_")
    try:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "-o", "run", "--",
               sys.executable, os.path.abspath(__file__), "--trace-child", "--px", str(px), "--step-limit", str(limit)]
        try:
            r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=limit + 30)      # (the child's own alarm comes first)
        except subprocess.TimeoutExpired as e:
            sys.exit(f"the traced child did not end within {limit + 30} s: nothing more is started on the GPU\n{(e.stdout or '')[-800:]}")
        if r.returncode != 0:
            # a fault, an abort, a segmentation fault or the child's own alarm: after that nothing more is started on the GPU in
            # this call (--no-trace measures without the child)
            sys.exit(f"the traced child ended with status {r.returncode}: nothing more is started on the GPU\n{r.stdout[-800:]}")
        found = sorted(glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True))
        if not found:
            return {"failed": "the child ended with status 0 and rocprofv3 left no kernel_stats.csv", "tail": r.stdout[-800:]}
        rows = []
        for row in csv.DictReader(open(found[0])):
            name = row["Name"].replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]
            rows.append({"kernel": name, "calls": int(row.get("Calls", 0) or 0), "average_us": round(float(row["AverageNs"]) / 1e3, 2)})
        return {"shape": dict(zip(("S", "C", "idx"), TRACE_SHAPE)), "calls_traced": TRACE_CALLS, "kernels": rows}
    finally:
        shutil.rmtree(out, ignore_errors=True)


TRACE_CALLS = 4


def trace_child(px):
    import torch
    from eulerian_warp_time import smooth_flow
    ops = importlib.import_module(pkg + ".ops")
    S, C, idx = TRACE_SHAPE
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    feature, m = torch.randn(C, S, S, device=dev), torch.from_numpy(smooth_flow(S, px)).to(dev)
    acc = None
    for _ in range(TRACE_CALLS):
        acc = ops.eulerian_blend(feature, m, idx, N_FRAMES, acc=acc, ordered=True)
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--calls", type=int, default=3, help="calls of warp_one_level per window")
    ap.add_argument("--px", type=float, default=1.0, help="flow magnitude in pixels per frame at 1024")
    ap.add_argument("--video-frames", type=int, default=120)
    ap.add_argument("--step-limit", type=int, default=120, help="seconds any one GPU step may take before the process is ended")
    ap.add_argument("--no-trace", action="store_true", help="skip the rocprofv3 child")
    ap.add_argument("--trace-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.trace_child:
        signal.alarm(a.step_limit)
        return trace_child(a.px)
    say = lambda *s: print(*s, file=sys.stderr, flush=True)
    by_kernel = {"skipped": "--no-trace"} if a.no_trace else kernel_trace(a.px, a.step_limit)      # before this process opens the GPU
    say("ordered blend by kernel:", json.dumps(by_kernel))

    import torch
    import torch.nn.functional as F
    from eulerian_warp_time import smooth_flow
    N = importlib.import_module(pkg + "._native")
    ops = importlib.import_module(pkg + ".ops")
    cg = importlib.import_module(pkg + ".cinemagraph")
    assert torch.cuda.is_available(), "this tool measures on the GPU; there is nothing to fall back to"
    dev = torch.device("cuda", 0)

    class gpu_step:
        """SIGALRM's default action ends the process, inside a blocked runtime call as well."""
        def __enter__(self):
            signal.alarm(a.step_limit)

        def __exit__(self, *exc):
            signal.alarm(0)

    def window(fn, calls):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0.record()
        for _ in range(calls):
            fn()
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1) / calls

    def stats(ms):
        return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
                "windows_ms": [round(x, 4) for x in ms]}

    def longest_cell(flow_s, idx):
        """The most entries in one cell (floor oy, floor ox) of the blend, both halves, from the displacements themselves."""
        S = flow_s.shape[-1]
        cut, pad, P, _ = ops.eulerian_geometry(S)
        inner = flow_s[:, :, cut:S - cut, cut:S - cut]
        yy, xx = torch.meshgrid(torch.arange(P, device=dev), torch.arange(P, device=dev), indexing="ij")
        keys = []
        for sign, steps in ((1.0, idx), (-1.0, N_FRAMES - idx - 1)):
            d = ops.euler_integrate(F.pad(sign * inner, (pad,) * 4, mode="reflect")[0].contiguous(), steps)
            nx, ny = torch.floor(xx + d[0]).long(), torch.floor(yy + d[1]).long()
            keys.append(((ny + 1) * (P + 1) + nx + 1).flatten())
        return int(torch.bincount(torch.cat(keys)).max())

    torch.manual_seed(0)
    flow1024 = torch.from_numpy(smooth_flow(1024, a.px))[None].to(dev)
    rows = []
    with torch.no_grad():
        for S, C, idxs in SHAPES:
            feature = torch.randn(1, C, S, S, device=dev)
            flow_s = cg.resize_flow(flow1024, S)
            for idx in idxs:
                forms = {"atomic": lambda: cg.warp_one_level(feature, flow1024, idx, N_FRAMES, fused=True, ordered=False),
                         "ordered": lambda: cg.warp_one_level(feature, flow1024, idx, N_FRAMES, fused=True, ordered=True)}
                ms = {k: [] for k in forms}
                with gpu_step():
                    for fn in forms.values():
                        fn()
                    torch.cuda.synchronize()
                for _ in range(a.windows):
                    for k, fn in forms.items():                   # alternating windows
                        with gpu_step():
                            ms[k].append(window(fn, a.calls))
                with gpu_step():
                    cell = longest_cell(flow_s, idx)
                row = {"S": S, "C": C, "idx": idx, "atomic": stats(ms["atomic"]), "ordered": stats(ms["ordered"]),
                       "ordered_over_atomic_of_medians": round(statistics.median(ms["ordered"]) / statistics.median(ms["atomic"]), 2),
                       "scratch_bytes": int(N.lib().mom_eulerian_ordered_scratch_bytes(C, S)), "longest_cell": cell}
                rows.append(row)
                say(f"S {S} C {C} idx {idx}: atomic {row['atomic']['median_ms']} ms ({row['atomic']['min_ms']}-{row['atomic']['max_ms']}), "
                    f"ordered {row['ordered']['median_ms']} ms ({row['ordered']['min_ms']}-{row['ordered']['max_ms']}), scratch "
                    f"{row['scratch_bytes'] / 2 ** 20:.1f} MiB, longest cell {cell}")
            del feature
            torch.cuda.empty_cache()

        # ---- the pixel video by wall clock, both ways, taking turns
        image = np.random.default_rng(0).integers(0, 256, (1024, 1024, 3), dtype=np.uint8)
        mask = np.full((1024, 1024), 255, np.uint8)
        video = {"atomic": [], "ordered": []}
        with gpu_step():
            for ordered in (False, True):
                cg.pixel_video(image, flow1024.cpu(), mask, n_frames=2, size=1024, ordered=ordered)          # warm-up
        for _ in range(3):
            for k, ordered in (("atomic", False), ("ordered", True)):
                with gpu_step():
                    t0 = time.perf_counter()
                    frames = cg.pixel_video(image, flow1024.cpu(), mask, n_frames=a.video_frames, size=1024, ordered=ordered)
                    video[k].append(len(frames) / (time.perf_counter() - t0))
        say("pixel_video frames/s: " + ", ".join(f"{k} {statistics.median(v):.1f}" for k, v in video.items()))

    out = {"library": N.lib().mom_version().decode(), "device": torch.cuda.get_device_name(0), "n_frames": N_FRAMES,
           "flow": f"smooth, about {a.px} px per frame at 1024, a still region; resized per level by resize_flow",
           "what": "GPU time of one warp_one_level call (fused route: blend + finish) in ms between two torch.cuda.Event records around "
                   "--calls calls, the device synchronised before and after each window; the two forms' windows alternate in one process",
           "windows": a.windows, "calls_per_window": a.calls, "shapes": rows,
           "pixel_video": {"frames": a.video_frames, "size": 1024, "runs_each": 3,
                           **{k: {"frames_per_s_median": round(statistics.median(v), 2), "min": round(min(v), 2), "max": round(max(v), 2)}
                              for k, v in video.items()},
                           "includes": "the resize of the inputs, every frame's warp, composite and copy to the host"},
           "ordered_blend_by_kernel": by_kernel,
           "not_measured": "no hardware counters; the trace is one run of four calls at one shape"}
    txt = json.dumps(out, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(txt + "\n")
    print(txt)


if __name__ == "__main__":
    main()
