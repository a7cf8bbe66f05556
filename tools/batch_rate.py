"""Steps and cameras per second of a training iteration over a BATCH of cameras on one GPU (opt.batch_size = B,
train_4DGS.py:172-229), on two paths in the same process and call:

  fused      Trainer(fused=True): the cameras one after the other inside one fused step (fused_step.py; cameras 2..B through the
             accumulating projection backward)
  autograd   Trainer(fused=False): render() per camera, one loss over the stack, loss.backward() -- what a batch size above one
             took before the fused step accepted a list

for B in {1, 2, 4, 8}, the fine and the coarse stage, L1 and L1 + 0.2 SSIM.  Both paths get the same camera lists over a window of
iterations with no densify / prune / opacity-reset / SH boundary (fine 5001.., coarse 2601..): 10 warm-up and 80 timed steps
whatever B -- the 80 walked again until the window has lasted --min-seconds --, with trainer.drain() and a device synchronisation before the clock stops (the convention of tools/coarse_rate.py).
Every cell is timed --repeats times per path, the two paths alternating on two trainers that live for the whole cell; the
document keeps every window's rate, the spread of each path, the ratio of the medians and the worst-case ratio (slowest fused
window over fastest autograd window).  Same-call pairs are the only valid comparison between machines of a pool.

    python tools/batch_rate.py [--configs c1 c2] [--batches 1 2 4 8] [--steps 80] [--warmup 10] [--repeats 3] [--out profiles/batch_rate.json]

Prints one JSON document (and writes it to --out)."""
import argparse
import importlib
import importlib.util
import json
import os
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
spec = importlib.util.spec_from_file_location("bench", os.path.join(ROOT, "bench.py"))
bench = importlib.util.module_from_spec(spec)
spec.loader.exec_module(bench)


def _state(cfg, dev, stage, fused, lam, B):
    import torch
    A = importlib.import_module("iclr2025_3d-mom_amd.arguments")
    S = importlib.import_module("iclr2025_3d-mom_amd.scene")
    T = importlib.import_module("iclr2025_3d-mom_amd.train")
    args, lp, op, pp, hp = A.default_args(time_resolution=cfg["time_res"])
    op.lambda_dssim, op.batch_size = lam, B
    torch.manual_seed(6666)
    scene = S.SyntheticScene(cfg["P"], cfg["F"], cfg["W"], cfg["H"], seed=6666)
    g = S.GaussianModel(lp.sh_degree, hp, device=dev)
    scene.init_gaussians(g)
    scene.make_trained_like(g)
    return T.Trainer(scene, g, op, hp, pp, stage=stage, delta_scale=1, sync_every_step=False, fused=fused)


def window(trainer, dev, stage, B, steps, warmup, min_seconds):
    """Steps per second over a timed window after `warmup` iterations, drained and synchronised.  The window is `steps` iterations
    over B cameras each, walked as many times as it takes to last `min_seconds` (estimated from the warm-up's own time): a window
    of a few tens of milliseconds measures the clock and the scheduler.  Every pass walks the same boundary-free iteration numbers
    (they only drive the learning-rate schedule)."""
    import math
    import torch
    cams = trainer.cams
    lists = lambda i: [cams[(i * B + j) % len(cams)] for j in range(B)]
    first = 5001 if stage == "fine" else 2601
    assert warmup + steps <= 98, "the window must end before the next densify / prune boundary"
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(warmup):
        trainer.step(first + i, cams=lists(i))
    trainer.drain()
    torch.cuda.synchronize()
    per_step = (time.perf_counter() - t0) / max(1, warmup)
    passes = max(1, min(50, math.ceil(min_seconds / max(per_step * steps, 1e-9))))
    serial0 = trainer._serial
    t0 = time.perf_counter()
    for k in range(passes):
        for i in range(steps):
            trainer.step(first + warmup + i, cams=lists(warmup + k * steps + i))
    trainer.drain()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    if trainer.fused is not None:
        assert trainer._serial - serial0 == passes * steps and trainer.replayed == 0, "the batch did not take the fused path"
    return passes * steps / dt, dt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", nargs="+", default=["c1", "c2"], choices=sorted(bench.CONFIGS))
    ap.add_argument("--batches", nargs="+", type=int, default=[1, 2, 4, 8])
    ap.add_argument("--stages", nargs="+", default=["fine", "coarse"], choices=["fine", "coarse"])
    ap.add_argument("--lambdas", nargs="+", type=float, default=[0.0, 0.2])
    ap.add_argument("--steps", type=int, default=80, help="iterations of every timed window, whatever B (tools/coarse_rate.py: 80)")
    ap.add_argument("--warmup", type=int, default=10, help="iterations before every timed window (tools/coarse_rate.py: 10)")
    ap.add_argument("--repeats", type=int, default=3, help="timed windows per path and cell, the two paths alternating")
    ap.add_argument("--min-seconds", type=float, default=0.3, help="every timed window lasts at least about this long")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import statistics
    import torch
    N = importlib.import_module("iclr2025_3d-mom_amd._native")
    dev = torch.device("cuda", 0)
    out = {"library": N.lib().mom_version().decode(), "device": torch.cuda.get_device_name(0), "warmup": a.warmup, "steps": a.steps,
           "repeats": a.repeats, "min_seconds": a.min_seconds, "order": "fused, autograd, fused, autograd, ...: one trainer per path, alive for the whole cell",
           "cells": []}
    for name in a.configs:
        cfg = bench.CONFIGS[name]
        for stage in a.stages:
            for lam in a.lambdas:
                for B in a.batches:
                    pair = {"fused": _state(cfg, dev, stage, True, lam, B), "autograd": _state(cfg, dev, stage, False, lam, B)}
                    assert pair["fused"].fused is not None and pair["autograd"].fused is None
                    for t in pair.values():
                        for c in t.cams:
                            c.device_tensors(dev)
                    runs = {"fused": [], "autograd": []}
                    shortest = None
                    for _ in range(a.repeats):
                        for path in ("fused", "autograd"):
                            r, dt = window(pair[path], dev, stage, B, a.steps, a.warmup, a.min_seconds)
                            runs[path].append(r)
                            shortest = dt if shortest is None else min(shortest, dt)
                    med = {k: statistics.median(v) for k, v in runs.items()}
                    cell = {"config": name, "stage": stage, "lambda_dssim": lam, "B": B,
                            "fused_steps_per_s": [round(r, 1) for r in runs["fused"]],
                            "autograd_steps_per_s": [round(r, 1) for r in runs["autograd"]],
                            "fused_cameras_per_s": round(med["fused"] * B, 1), "autograd_cameras_per_s": round(med["autograd"] * B, 1),
                            "ratio_of_medians": round(med["fused"] / med["autograd"], 3),
                            # the pessimistic pairing: the slowest fused window over the fastest autograd window
                            "ratio_worst_case": round(min(runs["fused"]) / max(runs["autograd"]), 3),
                            "spread": {k: round((max(v) - min(v)) / statistics.median(v), 4) for k, v in runs.items()},
                            "shortest_window_s": round(shortest, 4)}
                    out["cells"].append(cell)
                    print(json.dumps(cell), file=sys.stderr, flush=True)
                    del pair
                    torch.cuda.empty_cache()
    txt = json.dumps(out, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(txt + "\n")
    print(txt)


if __name__ == "__main__":
    main()
