"""What the ordered backward reduction costs (include/mom4d.h, "ordered backward reduction"), on one frame, in one process:

  atomic    mom_raster_backward_render: clear of the accumulator record + render_bwd_kernel<., false> (float atomics)
  ordered   mom_raster_ordered_plan (two launches) + mom_raster_backward_render_ordered: clear of the partials +
            render_bwd_kernel<., true> (plain stores) + the reduction

Frame: config 2's size, 200 000 random Gaussians at 960x540 (tests/scenes.py, the scene of test_backward_parity's largest case),
no depth gradient, as in training.  A sample is --reps calls between two device synchronisations, divided by --reps; a window is
the median of --samples samples; the two routes take turns, window by window, seven windows each.  The record keeps every window,
each route's median, lowest and highest window, their ratio, the slot count and the scratch bytes.  Both routes leave the same
kind of record; the ordered one's is checked to repeat bit for bit and to sit within 2e-5 of the atomic one's scale.

One process; run it under a time limit (timeout -k 10 300 python tools/raster_ordered_time.py ...) and start nothing behind it if it fails.

    python tools/raster_ordered_time.py [--windows 7] [--samples 5] [--reps 10] [--out profiles/raster_ordered_time.json]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--P", type=int, default=200_000)
    ap.add_argument("--W", type=int, default=960)
    ap.add_argument("--H", type=int, default=540)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--samples", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    from hip_helpers import N, RC, _aligned, hip_forward, t
    from scenes import random_gaussians
    lib, stream = N.lib(), N.current_stream()
    P, W, H = a.P, a.W, a.H
    s = random_gaussians(P, seed=14, W=W, H=H, scale=(-5.5, -3.5))
    fw = hip_forward(s)
    (bg, means3D, colors, opacity, scales, rotations, scale_modifier, cov3D, view, proj, tanx, tany, _, _, sh, degree, campos, _, _) = fw["args"]
    args, keep = RC._args(bg, means3D, colors, means3D.new_ones((1,)), scales, rotations, scale_modifier, cov3D, view, proj, tanx, tany,
                          H, W, sh, degree, campos, False, False)
    geom, binning, img = fw["bufs"]
    R = int(fw["R"])
    dcol = t(np.random.default_rng(14).standard_normal((3, H, W)).astype(np.float32))
    u8 = lambda n: torch.empty(n, dtype=torch.uint8, device="cuda")
    plan = u8(lib.mom_raster_ordered_plan_bytes(P))
    total = torch.zeros(1, dtype=torch.int32).pin_memory()
    status = torch.zeros(1, dtype=torch.int32, device="cuda")

    def run_plan():
        N.check(lib.mom_raster_ordered_plan(C.byref(args), geom.data_ptr(), plan.data_ptr(), None, total.data_ptr(), stream), "plan")
    run_plan()
    torch.cuda.synchronize()
    slots = int(total[0]) & 0xFFFFFFFF
    part = u8(lib.mom_raster_ordered_bytes(P, slots))

    def atomic():
        N.check(lib.mom_raster_backward_render(C.byref(args), geom.data_ptr(), binning.data_ptr(), R, img.data_ptr(), dcol.data_ptr(), None,
                                               stream), "backward_render")

    def ordered():
        run_plan()
        N.check(lib.mom_raster_backward_render_ordered(C.byref(args), geom.data_ptr(), binning.data_ptr(), R, img.data_ptr(), dcol.data_ptr(),
                                                       None, plan.data_ptr(), part.data_ptr(), part.numel(), slots, status.data_ptr(), stream),
                "backward_render_ordered")

    lay = N.MomRasterLayout()
    lib.mom_raster_layout(P, W, H, R, C.byref(lay))

    def record():
        torch.cuda.synchronize()
        return _aligned(geom)[lay.geom_gacc:lay.geom_gacc + P * N.GACC_FLOATS * 4].cpu().numpy().view(np.float32).copy()

    def sample(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.reps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6 / a.reps

    routes = {"atomic": atomic, "ordered": ordered}
    recs = {}
    for name, fn in routes.items():                     # both routes warmed up before the first window
        for _ in range(3):
            fn()
        recs[name] = record()
    ordered()
    again = record()
    runs = {name: [] for name in routes}
    for _ in range(a.windows):
        for name, fn in routes.items():
            runs[name].append(statistics.median(sample(fn) for _ in range(a.samples)))
            print(name, round(runs[name][-1], 1), "us", file=sys.stderr, flush=True)
    scale = float(np.abs(recs["atomic"]).max())
    out = {"library": lib.mom_version().decode(), "device": torch.cuda.get_device_name(0), "P": P, "W": W, "H": H,
           "instances_default_binning": R, "slots": slots, "bytes_per_slot": N.ORDERED_SLOT_BYTES,
           "partials_bytes": slots * N.ORDERED_SLOT_BYTES, "plan_bytes": int(plan.numel()),
           "windows": a.windows, "samples_per_window": a.samples, "calls_per_sample": a.reps,
           "order": "atomic, ordered, atomic, ordered, ...: one frame, one process",
           "what": "microseconds per call, host wall time of `calls_per_sample` calls between two device synchronisations; a window is the "
                   "median of its samples; median, lowest and highest window per route",
           "status_bits": int(status.item()),
           "ordered_record_repeats_bit_for_bit": bool(np.array_equal(recs["ordered"].view(np.uint32), again.view(np.uint32))),
           "largest_difference_over_scale": float(np.abs(recs["ordered"] - recs["atomic"]).max() / scale)}
    for name, v in runs.items():
        out[name] = {"median_us": round(statistics.median(v), 1), "min_us": round(min(v), 1), "max_us": round(max(v), 1),
                     "windows_us": [round(r, 1) for r in v]}
    out["ratio_of_medians_ordered_over_atomic"] = round(statistics.median(runs["ordered"]) / statistics.median(runs["atomic"]), 3)
    del keep
    txt = json.dumps(out, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(txt + "\n")
    print(txt)


if __name__ == "__main__":
    main()
