"""GPU time of one scene-flow fit at the reference's size (P = 512 x 512 points, 14 x 5 views, 200 epochs), two forms in one process:

  torch   the reference's loop (train_motion.py:125-207) as torch operations with autograd, SGD and ExponentialLR, every tensor on
          the device: what moving the reference's tensors to the GPU gives
  kernel  motion's path: ops.sceneflow_fit, one launch for all epochs and views (csrc/sceneflow_fit.hip) plus the loss sum

The scene is synthetic: a 512 x 512 depth map (3 + sinusoids) back-projected with the stage-1 intrinsics, 70 poses a few degrees
and centimetres apart, targets of 3 px of noise given at each view's valid points.  Both forms read the same device tensors.
A window is one fit (torch) or --fits fits (kernel, the figure is per fit), bracketed by a torch.cuda.Event pair and one
synchronisation; the two forms take turns, window by window, after one warm-up each.  The record keeps every window, each form's
median, lowest and highest, the criterion of DESIGN.md section 3.6 -- the slowest kernel window over the fastest torch window --
and the kernel's read rate against the V x P x 16 bytes x E of records it has to read.

One process; run it under a time limit (timeout -k 10 900 python tools/sceneflow_fit_time.py ...) and start nothing behind it if it
fails.  --limit stops it between windows once that many seconds have passed.

    python tools/sceneflow_fit_time.py [--windows 5] [--fits 3] [--epochs 200] [--torch-epochs 200] [--out profiles/sceneflow_fit_time.json]
"""
import argparse
import importlib
import json
import math
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
pkg = "iclr2025_3d-mom_amd"
STREAM_TBPS = (6.0, 6.3)          # streaming reads of one MI355X as measured for the microarchitecture notes DESIGN.md cites


def rot(ax, ay):
    cx, sx, cy, sy = math.cos(ax), math.sin(ax), math.cos(ay), math.sin(ay)
    return np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])


def make_scene(side, n_render, n_internal, seed=7):
    motion = importlib.import_module(pkg + ".motion")
    rng = np.random.default_rng(seed)
    H = W = side
    K = motion.stage1_intrinsics(H, W)
    v, u = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    d = 3.0 + 0.3 * np.sin(u * (7 * math.pi / W) + 0.4) + 0.2 * np.sin(v * (5 * math.pi / H) + 1.1)
    pts = np.stack([(u - K[0, 2]) / K[0, 0] * d, (v - K[1, 2]) / K[1, 1] * d, d]).reshape(3, -1).astype(np.float32)
    w2c = []
    for i in range(n_render):
        a = rng.uniform(-0.06, 0.06, 2)
        Ri, Ti = rot(a[0], a[1]), rng.uniform(-0.15, 0.15, (3, 1))
        for j in range(n_internal):
            b = rng.uniform(-0.03, 0.03, 2) * (j > 0)
            Rj, Tj = rot(b[0], b[1]), rng.uniform(-0.05, 0.05, (3, 1)) * (j > 0)
            w2c.append((Rj @ Ri, Rj @ Ti + Tj))
    views = motion.prepare_views(pts, K, w2c, H, W)
    gt = [(rng.standard_normal((2, len(idx))) * 3.0).astype(np.float32) for idx in views.valid]
    return pts, K, views, gt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=512, help="the point cloud is side x side")
    ap.add_argument("--render", type=int, default=14)
    ap.add_argument("--internal", type=int, default=5)
    ap.add_argument("--epochs", type=int, default=200)
    ap.add_argument("--torch-epochs", type=int, default=None, help="epochs of a torch window (default: --epochs); its time is "
                    "scaled to --epochs and the record says so")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--fits", type=int, default=3, help="kernel fits per window")
    ap.add_argument("--limit", type=float, default=800.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    N = importlib.import_module(pkg + "._native")
    ops = importlib.import_module(pkg + ".ops")
    motion = importlib.import_module(pkg + ".motion")
    t_start = time.perf_counter()
    dev = torch.device("cuda", 0)
    E, Et = a.epochs, a.torch_epochs or a.epochs
    pts, K, views, gt = make_scene(a.side, a.render, a.internal)
    V, P = views.V, views.P
    rec, bits = motion.pack_views(views, gt)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    d_pts, d_R, d_T, d_w = up(pts), up(views.R), up(views.T), up(motion.view_weights(views, V))
    d_rec, d_bits, d_lr = up(rec), up(bits), up(motion.learning_rates(E))
    del rec
    d_idx = [up(i.astype(np.int64)) for i in views.valid]
    d_pix0, d_gt, d_K = [up(p) for p in views.pix0], [up(g) for g in gt], up(K)
    flow = torch.zeros(3, P, device=dev)
    loss = torch.zeros(E, device=dev)
    flow2d = torch.zeros(V, P, 2, device=dev)
    print(f"P {P}  V {V}  E {E}  valid per view {min(map(len, views.valid))}..{max(map(len, views.valid))}  "
          f"setup {time.perf_counter() - t_start:.1f} s", file=sys.stderr, flush=True)

    def kernel_fit():
        flow.zero_()
        ops.sceneflow_fit(d_pts, K, d_R, d_T, d_w, d_rec, d_bits, d_lr, flow, loss, flow2d)

    def torch_fit(epochs):
        f = torch.zeros(3, P, device=dev, requires_grad=True)
        opt = torch.optim.SGD([f], lr=0.5)
        sched = torch.optim.lr_scheduler.ExponentialLR(opt, gamma=0.97)
        for _ in range(epochs):
            total = 0
            for j in range(V):
                h = torch.matmul(d_K, torch.matmul(d_R[j], d_pts + f) + d_T[j].reshape(3, 1))
                new = h[:2, d_idx[j]] / h[-1:, d_idx[j]] - d_pix0[j]
                total = total + torch.abs(new - d_gt[j]).mean()
            out = total / V
            opt.zero_grad()
            out.backward()
            opt.step()
            sched.step()
        return f.detach()

    def timed(fn):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0.record()
        fn()
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1)

    # warm-up and parity: twelve epochs of both forms from the same tensors
    lr12 = up(motion.learning_rates(12))
    f12 = torch.zeros(3, P, device=dev)
    ops.sceneflow_fit(d_pts, K, d_R, d_T, d_w, d_rec, d_bits, lr12, f12)
    t12 = torch_fit(12)
    s12 = float(t12.abs().max())
    dist = (f12 - t12).abs().max(0).values / s12
    parity = {"epochs": 12, "largest_distance_over_scale": float(dist.max()), "scale": s12,
              "points_beyond_2e-6": int((dist > 2e-6).sum()), "points": P}
    print("parity", parity, file=sys.stderr, flush=True)
    kernel_fit()
    torch.cuda.synchronize()

    runs = {"torch": [], "kernel": []}
    for wdw in range(a.windows):
        if time.perf_counter() - t_start > a.limit:
            print(f"stopped after {wdw} windows: --limit {a.limit} s", file=sys.stderr)
            sys.exit(3)
        runs["torch"].append(timed(lambda: torch_fit(Et)) * (E / Et))
        runs["kernel"].append(timed(lambda: [kernel_fit() for _ in range(a.fits)]) / a.fits)
        print(f"window {wdw}: torch {runs['torch'][-1]:.1f} ms  kernel {runs['kernel'][-1]:.3f} ms", file=sys.stderr, flush=True)
    # the kernel alone without its optional outputs (no loss sum, no last-epoch store): how much of a fit they are
    bare = statistics.median(timed(lambda: ops.sceneflow_fit(d_pts, K, d_R, d_T, d_w, d_rec, d_bits, d_lr, flow)) for _ in range(3))

    rec_bytes = V * P * 16 * E
    med = statistics.median(runs["kernel"])
    tbps = rec_bytes / (med * 1e-3) / 1e12
    out = {"library": N.lib().mom_version().decode(), "device": torch.cuda.get_device_name(0), "P": P, "V": V, "E": E,
           "valid_per_view_min_max": [min(map(len, views.valid)), max(map(len, views.valid))],
           "windows": a.windows, "kernel_fits_per_window": a.fits, "torch_epochs_per_window": Et,
           "torch_time_scaled_to_E": Et != E,
           "order": "torch, kernel, torch, kernel, ...: one process, the same device tensors",
           "what": "GPU time of one fit in ms between two torch.cuda.Event records, device synchronised before and after each window"}
    for name, v in runs.items():
        out[name] = {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3),
                     "windows_ms": [round(r, 3) for r in v]}
    out["ratio_of_medians_torch_over_kernel"] = round(statistics.median(runs["torch"]) / med, 1)
    out["criterion"] = {"slowest_kernel_over_fastest_torch": round(max(runs["kernel"]) / min(runs["torch"]), 6),
                        "kernel_wins_every_window": max(runs["kernel"]) < min(runs["torch"])}
    out["kernel_without_optional_outputs_ms"] = round(bare, 3)
    out["record_bytes_read"] = rec_bytes
    out["kernel_record_TB_per_s"] = round(tbps, 3)
    out["streaming_read_TB_per_s_of_the_device"] = list(STREAM_TBPS)
    out["share_of_streaming_rate"] = round(tbps / STREAM_TBPS[0], 3)
    out["nearer_to"] = "memory" if tbps >= 0.5 * STREAM_TBPS[0] else "instruction issue"
    out["parity_with_torch_on_the_device"] = parity
    out["not_measured"] = "no hardware counters (no rocprofv3 run): memory against issue is judged from the read rate alone"
    txt = json.dumps(out, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(txt + "\n")
    print(txt)


if __name__ == "__main__":
    main()
