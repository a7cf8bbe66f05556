"""Time of the video generator's warp, cinemagraph.warp_one_level, on its two routes in one process, alternating windows:

  op_by_op  fused=False: the reference's sequence of ops (cinemagraph_utils.py:181-190) -- cut, two reflection paddings, two
            euler_integration calls, Z, the double-width concatenation, the summation splat (ops.softsplat_sum), the division, the
            whole thing again on a tensor of ones for the blank mask, 7 x 7 conv2d per channel, crop
  fused     fused=True: ops.eulerian_blend (a clear and one launch) and ops.eulerian_finish (one launch)

at the levels the reference warps (models/stylegan2/model.py:670-691: S = 128 C = 256, S = 256 C = 128, S = 512 C = 64, S = 1024
C = 32) and the pixel route's (S = 1024, C = 3), n_frames = 120, idx 0, 60, 119.  The comparison partner of the fused route is the
op-by-op route of the same process, never an earlier run.  Both routes call the one-launch Euler kernel; the reference's own ~119
rounds of torch launches per chain are not part of either.

Also, for the fused route: its two calls' own times; the bytes its atomics add per second (kept corner adds x (C + 1) x 4 bytes, the
corner count taken from the displacements) against the ~1.3 TB/s at which the chip adds; both accumulation forms for C = 1 and 3; and
cinemagraph.pixel_video's frames per second for 120 frames at 1024 by wall clock.

The flow is smooth, about --px pixels per frame at 1024 with a still region, resized to each level as warp_one_level does.  A window
is --calls calls between a torch.cuda.Event pair, the device synchronised before and after; --windows windows per route after a
warm-up call of each.  Every GPU step runs under an alarm of --step-limit seconds that ends the process; run it under a time limit
as well (timeout -k 10 600 python tools/eulerian_warp_time.py ...).

    python tools/eulerian_warp_time.py [--windows 5] [--calls 3] [--out profiles/eulerian_warp_time.json]
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
LEVELS = [(128, 256), (256, 128), (512, 64), (1024, 32), (1024, 3)]
ATOMIC_TBPS = 1.3         # added bytes per second chip-wide, 256 contiguous bytes per wave-instruction


def smooth_flow(size, px):
    y, x = np.meshgrid(np.arange(size, dtype=np.float64), np.arange(size, dtype=np.float64), indexing="ij")
    u = px * (0.8 * np.sin(y * (3 * math.pi / size) + 0.3) + 0.4 * np.cos(x * (5 * math.pi / size)))
    v = px * (0.6 * np.cos(x * (4 * math.pi / size) - 0.2) + 0.5 * np.sin((x + y) * (2 * math.pi / size)))
    f = np.stack([u, v])
    f[:, : size // 3, : size // 3] = 0.0
    return f.astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--calls", type=int, default=3, help="calls of warp_one_level per window")
    ap.add_argument("--n-frames", type=int, default=120)
    ap.add_argument("--px", type=float, default=1.0, help="flow magnitude in pixels per frame at 1024")
    ap.add_argument("--video-frames", type=int, default=120)
    ap.add_argument("--step-limit", type=int, default=120, help="seconds any one GPU step may take before the process is ended")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import torch.nn.functional as F
    N = importlib.import_module(pkg + "._native")
    ops = importlib.import_module(pkg + ".ops")
    cg = importlib.import_module(pkg + ".cinemagraph")
    assert torch.cuda.is_available(), "this tool measures on the GPU; there is nothing to fall back to"
    dev = torch.device("cuda", 0)
    say = lambda *s: print(*s, file=sys.stderr, flush=True)
    n_frames, idxs = a.n_frames, sorted({0, a.n_frames // 2, a.n_frames - 1})

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

    def kept_adds(flow_s, idx):
        """Corner adds of one blend that land on the canvas, both halves, from the displacements themselves."""
        S = flow_s.shape[-1]
        cut, pad, P, _ = ops.eulerian_geometry(S)
        inner = flow_s[:, :, cut:S - cut, cut:S - cut]
        yy, xx = torch.meshgrid(torch.arange(P, device=dev), torch.arange(P, device=dev), indexing="ij")
        total = 0
        for sign, steps in ((1.0, idx), (-1.0, n_frames - idx - 1)):
            d = ops.euler_integrate(F.pad(sign * inner, (pad,) * 4, mode="reflect")[0].contiguous(), steps)
            nx, ny = torch.floor(xx + d[0]).long(), torch.floor(yy + d[1]).long()
            for dx in (0, 1):
                for dy in (0, 1):
                    total += int(((nx + dx >= 0) & (nx + dx < P) & (ny + dy >= 0) & (ny + dy < P)).sum())
        return total

    torch.manual_seed(0)
    flow1024 = torch.from_numpy(smooth_flow(1024, a.px))[None].to(dev)
    levels, met = [], True
    with torch.no_grad():
        for S, C in LEVELS:
            feature = torch.randn(1, C, S, S, device=dev)
            flow_s = cg.resize_flow(flow1024, S)
            for idx in idxs:
                routes = {"op_by_op": lambda: cg.warp_one_level(feature, flow1024, idx, n_frames, fused=False),
                          "fused": lambda: cg.warp_one_level(feature, flow1024, idx, n_frames, fused=True)}
                ms = {k: [] for k in routes}
                with gpu_step():
                    for fn in routes.values():
                        fn()
                    torch.cuda.synchronize()
                for _ in range(a.windows):
                    for k, fn in routes.items():                  # alternating windows
                        with gpu_step():
                            ms[k].append(window(fn, a.calls))
                acc = ops.eulerian_blend(feature[0], flow_s[0].contiguous(), idx, n_frames, form=cg._form(C))
                out = torch.empty((C, S, S), device=dev)
                with gpu_step():
                    blend_ms = [window(lambda: ops.eulerian_blend(feature[0], flow_s[0], idx, n_frames, acc=acc, form=cg._form(C)), a.calls)
                                for _ in range(a.windows)]
                    finish_ms = [window(lambda: ops.eulerian_finish(acc, S, out=out), a.calls) for _ in range(a.windows)]
                    adds = kept_adds(flow_s, idx)
                nbytes = adds * (C + 1) * 4
                tbps = nbytes / (statistics.median(blend_ms) * 1e-3) / 1e12
                row = {"S": S, "C": C, "idx": idx, "op_by_op": stats(ms["op_by_op"]), "fused": stats(ms["fused"]),
                       "fused_slowest_beats_op_by_op_fastest": max(ms["fused"]) < min(ms["op_by_op"]),
                       "speedup_of_medians": round(statistics.median(ms["op_by_op"]) / statistics.median(ms["fused"]), 2),
                       "fused_calls": {"eulerian_blend_with_its_clear": stats(blend_ms), "eulerian_finish": stats(finish_ms)},
                       "atomic_added_bytes": nbytes, "atomic_added_TB_per_s_over_the_whole_blend_call": round(tbps, 3),
                       "share_of_the_chip_rate": round(tbps / ATOMIC_TBPS, 3)}
                met = met and row["fused_slowest_beats_op_by_op_fastest"]
                levels.append(row)
                say(f"S {S} C {C} idx {idx}: op-by-op {row['op_by_op']['median_ms']} ms, fused {row['fused']['median_ms']} ms "
                    f"(blend {row['fused_calls']['eulerian_blend_with_its_clear']['median_ms']}, finish "
                    f"{row['fused_calls']['eulerian_finish']['median_ms']}), {tbps:.3f} TB/s added")
                del acc, out
            del feature
            torch.cuda.empty_cache()

        # ---- both accumulation forms for the small channel counts, S = 1024, the middle frame
        forms = []
        for C in (1, 3):
            feature = torch.randn(C, 1024, 1024, device=dev)
            m = flow1024[0].contiguous()
            acc = ops.eulerian_blend(feature, m, n_frames // 2, n_frames)
            ms = {f: [] for f in ops.EULERIAN_FORM}
            for _ in range(a.windows):
                for f in ms:
                    with gpu_step():
                        ms[f].append(window(lambda: ops.eulerian_blend(feature, m, n_frames // 2, n_frames, acc=acc, form=f), a.calls))
            forms.append({"S": 1024, "C": C, "idx": n_frames // 2, **{f: stats(v) for f, v in ms.items()}})
            say(f"forms C {C}: " + ", ".join(f"{f} {statistics.median(v):.3f} ms" for f, v in ms.items()))

        # ---- the pixel video by wall clock
        image = np.random.default_rng(0).integers(0, 256, (1024, 1024, 3), dtype=np.uint8)
        mask = np.full((1024, 1024), 255, np.uint8)
        with gpu_step():
            cg.pixel_video(image, flow1024.cpu(), mask, n_frames=2, size=1024)          # warm-up
            t0 = time.perf_counter()
            frames = cg.pixel_video(image, flow1024.cpu(), mask, n_frames=a.video_frames, size=1024)
            t_video = time.perf_counter() - t0
        say(f"pixel_video: {len(frames)} frames in {t_video:.2f} s")

    out = {"library": N.lib().mom_version().decode(), "device": torch.cuda.get_device_name(0), "n_frames": n_frames,
           "flow": f"smooth, about {a.px} px per frame at 1024, a still region; resized per level by resize_flow",
           "what": "GPU time of one warp_one_level call in ms between two torch.cuda.Event records around --calls calls, the device "
                   "synchronised before and after each window; the two routes' windows alternate in one process",
           "windows": a.windows, "calls_per_window": a.calls, "levels": levels,
           "criterion": {"is": "at every level and frame the fused route's slowest window beats the op-by-op route's fastest", "met": met},
           "fused_is_the_default": bool(cg.FUSED_DEFAULT),
           "small_C_forms": forms, "small_C_form_in_use": cg.SMALL_C_FORM,
           "chip_atomic_rate_TB_per_s": ATOMIC_TBPS,
           "pixel_video": {"frames": len(frames), "size": 1024, "wall_s": round(t_video, 3), "frames_per_s": round(len(frames) / t_video, 2),
                           "includes": "the resize of the inputs, every frame's warp, composite and copy to the host"},
           "not_measured": "no hardware counters (no rocprofv3 run): the atomic rate is counted bytes over the event time of the whole "
                           "blend call, its clear and its Euler chains included"}
    txt = json.dumps(out, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(txt + "\n")
    print(txt)


if __name__ == "__main__":
    main()
