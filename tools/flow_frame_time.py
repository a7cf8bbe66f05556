"""Time of the flow step around stage 1's estimator at the reference's size -- 70 views of 512 x 512, working size 768, 3 hints a
view -- on three routes:

  kernels  ops.hint_field and ops.flow_finish: two launches each for all views (csrc/flow_frame.hip)
  torch    the same steps as torch operations on the same GPU, batched over the views (the hint loop of demo.py:89-94 with a view
           axis, F.interpolate, avg_pool2d): the comparison partner, in the same process, alternating windows
  cpu      the reference's own sequence for ONE view on this host's CPU (flow_frame_cases.hint_restated / finish_restated: its torch
           statements, kornia's blur restated), wall clock; the reference runs it 70 times and builds its estimator as often

A window is --calls calls between a torch.cuda.Event pair, the device synchronised before and after; --windows windows per route
after a warm-up call of each.  Every GPU step runs under an alarm of --step-limit seconds that ends the process; run it under a time
limit as well (timeout -k 10 600 python tools/flow_frame_time.py ...).

The criterion, as elsewhere in this project: a kernel half that is slower than its torch sequence on the device is not used by
estimate_flows.

    python tools/flow_frame_time.py [--windows 5] [--calls 3] [--out profiles/flow_frame_time.json]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
pkg = "iclr2025_3d-mom_amd"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=70)
    ap.add_argument("--side", type=int, default=512)
    ap.add_argument("--size", type=int, default=768)
    ap.add_argument("--hints", type=int, default=3)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--cpu-runs", type=int, default=3)
    ap.add_argument("--step-limit", type=int, default=120, help="seconds any one GPU step may take before the process is ended")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import torch.nn.functional as F
    import flow_frame_cases as fc
    N = importlib.import_module(pkg + "._native")
    ops = importlib.import_module(pkg + ".ops")
    assert torch.cuda.is_available(), "this tool measures on the GPU; there is nothing to fall back to"
    dev = torch.device("cuda", 0)
    say = lambda *s: print(*s, file=sys.stderr, flush=True)
    V, H, W, S, n = a.views, a.side, a.side, a.size, a.hints

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

    rng = np.random.default_rng(0)
    pos_h = rng.integers(0, H, (V, n, 2)).astype(np.int32)
    start_h = pos_h + rng.random((V, n, 2))
    end_h = start_h + rng.normal(0, 40, (V, n, 2))
    sigma_h = rng.integers(H // (n * 2), int(H // (n / 2)), V).astype(np.float32)
    masks_h = np.stack([fc.disc(H, W, W // 2 + 3 * (v % 7), H // 2 - 2 * (v % 5), H // 3) for v in range(V)])
    pos, start, end, sigma, masks = (torch.from_numpy(x).to(dev) for x in (pos_h, start_h, end_h, sigma_h, masks_h))
    count = torch.full((V,), n, dtype=torch.int32, device=dev)
    ys, xs = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float32), torch.arange(W, device=dev, dtype=torch.float32), indexing="ij")
    xs, ys = xs.reshape(1, -1), ys.reshape(1, -1)
    motion = (end - start) / 50.

    def hint_torch():
        dense = torch.zeros(V, 2, H * W, device=dev)
        norm = torch.zeros(V, 1, H * W, device=dev)
        for i in range(n):
            dist = ((xs - pos[:, i, 0:1].float()) ** 2 + (ys - pos[:, i, 1:2].float()) ** 2).sqrt()
            weight = (-(dist / sigma[:, None]) ** 2).exp().unsqueeze(1)
            dense += weight * motion[:, i, :, None]                      # float64 motion: the add is made in float64, as there
            norm += weight
        norm[norm == 0.0] = 1.0
        dense = (dense / norm).view(V, 2, H, W) * (masks != 0)[:, None]
        dense = dense * torch.tensor([S / W, S / H], dtype=torch.float32, device=dev).view(1, 2, 1, 1)
        return (F.interpolate(dense, (S, S), mode="bilinear", align_corners=False),
                F.interpolate((masks != 0)[:, None].float(), (S, S), mode="area"))

    hint_kernel = lambda: ops.hint_field(pos, start, end, count, sigma, masks, S)
    with torch.no_grad():
        with gpu_step():
            hints, mask_s = hint_kernel()
            ht, mt = hint_torch()
            torch.cuda.synchronize()
            agree = {"hints_max_abs_difference": float((hints - ht).abs().max()), "hints_max_abs": float(ht.abs().max()),
                     "mask_s_equal": bool(torch.equal(mask_s, mt))}
            del ht, mt
        pred = hints + 0.05 * torch.randn_like(hints)
        tail_kernel = lambda: ops.flow_finish(pred, mask_s, H, W)
        tail_torch = lambda: fc.finish_restated(pred, mask_s, H, W)
        with gpu_step():
            agree["flow_max_abs_difference"] = float((tail_kernel() - tail_torch()).abs().max())
        say("agreement of the two device routes:", agree)
        result = {}
        for name, routes in (("hint_field", {"kernels": hint_kernel, "torch": hint_torch}),
                             ("flow_finish", {"kernels": tail_kernel, "torch": tail_torch})):
            ms = {k: [] for k in routes}
            for _ in range(a.windows):
                for k, fn in routes.items():                          # alternating windows
                    with gpu_step():
                        ms[k].append(window(fn, a.calls))
                    torch.cuda.empty_cache()
            result[name] = {k: stats(v) for k, v in ms.items()}
            result[name]["kernels_slowest_beats_torch_fastest"] = max(ms["kernels"]) < min(ms["torch"])
            result[name]["speedup_of_medians"] = round(statistics.median(ms["torch"]) / statistics.median(ms["kernels"]), 2)
            say(f"{name}: kernels {result[name]['kernels']['median_ms']} ms, torch {result[name]['torch']['median_ms']} ms for {V} views")

        # ---- the reference's sequence for one view on the CPU
        torch.set_num_threads(16)
        cpu = {"hint_field": [], "flow_finish": []}
        p1, m1 = pred[:1].cpu(), mask_s[:1].cpu()
        for _ in range(a.cpu_runs):
            t0 = time.perf_counter()
            fc.hint_restated(pos_h[0], start_h[0], end_h[0], int(sigma_h[0]), masks_h[0], S)
            t1 = time.perf_counter()
            fc.finish_restated(p1, m1, H, W)
            t2 = time.perf_counter()
            cpu["hint_field"].append((t1 - t0) * 1e3)
            cpu["flow_finish"].append((t2 - t1) * 1e3)
        for k, v in cpu.items():
            result[k]["cpu_one_view"] = stats(v)
            result[k]["cpu_all_views_ms_by_multiplication"] = round(statistics.median(v) * V, 1)
            say(f"{k}: the reference's CPU sequence, one view: {statistics.median(v):.1f} ms")

    out = {"library": N.lib().mom_version().decode(), "device": torch.cuda.get_device_name(0), "views": V, "image": [H, W], "size": S,
           "hints_per_view": n,
           "what": "GPU time of one call for all views in ms between two torch.cuda.Event records around --calls calls, the device "
                   "synchronised before and after each window; the two device routes' windows alternate in one process.  cpu_one_view: "
                   "wall clock of the reference's torch statements for one view on the host, 16 threads",
           "windows": a.windows, "calls_per_window": a.calls, "agreement": agree, **result,
           "criterion": {"is": "a kernel half slower than its torch sequence on the device is not used by estimate_flows",
                         "hint_field_kept": result["hint_field"]["speedup_of_medians"] >= 1.0,
                         "flow_finish_kept": result["flow_finish"]["speedup_of_medians"] >= 1.0},
           "not_measured": "no hardware counters (no rocprofv3 run); the estimator between the two halves is not part of either route"}
    txt = json.dumps(out, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(txt + "\n")
    print(txt)


if __name__ == "__main__":
    main()
