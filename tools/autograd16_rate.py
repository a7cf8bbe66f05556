"""Training steps per second of a 16 x 2 HexPlane model (dnerf/eulerian_150_16: two levels of 16-channel planes, 32 features into the
shipped network) on the two routes of the loop an unchanged train_4DGS.py drives -- render() + loss.backward() + optimizer.step(),
Trainer(fused=False) -- in one process:

  node       gradient-mode render() as ONE autograd node (fused_autograd.FusedRenderFunction at 32 features: 16-channel HexPlane
             forward, MLP forward on 32 features, torch's activations, the rasterizer; backward: rasterizer, MLP on 32 features,
             16-channel HexPlane), with 32 in fused_autograd.NODE_WIDTHS
  per_op     the same trainer with pipe.per_op_autograd = True: HexPlane op, MLP op, activations, rasterizer op, some forty small
             launches and autograd nodes per iteration -- the yardstick, in the same process, never a number from another run

Model: synthetic, BASELINE config 2 size -- 200 000 Gaussians, 960 x 540, 60 frames, planes [64, 64, 64, 150], multires [1, 2],
lambda_dssim 0.  Both paths walk the same cameras over a window of iterations with no densify / prune / opacity-reset / SH boundary
(5001..): --warmup and --steps iterations, with trainer.drain() and a device synchronisation before the clock stops (the convention
of tools/step16_rate.py).  The two paths take turns, window by window, on two trainers that live for the whole run; first in the
rasterizer's default "exact" sync mode, then again in "async" mode.  The record keeps every window, each path's median, lowest and
highest window per mode, and the routing rule of DESIGN 3.6: 32 belongs in the default NODE_WIDTHS only if the slowest node window
beats the fastest per-op window in BOTH modes.

One process; run it under a time limit (timeout -k 10 600 python tools/autograd16_rate.py ...) and start nothing behind it if it fails.

    python tools/autograd16_rate.py [--windows 7] [--steps 80] [--warmup 10] [--out profiles/autograd16_rate.json]
"""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
pkg = "iclr2025_3d-mom_amd"
RES, MULTIRES = [64, 64, 64, 150], [1, 2]


def _trainer(a, dev, per_op):
    import torch
    A = importlib.import_module(pkg + ".arguments")
    S = importlib.import_module(pkg + ".scene")
    T = importlib.import_module(pkg + ".train")
    FA = importlib.import_module(pkg + ".fused_autograd")
    kc = {'grid_dimensions': 2, 'input_coordinate_dim': 4, 'output_coordinate_dim': 16, 'resolution': list(RES)}
    args, lp, op, pp, hp = A.default_args(kplanes_config=kc, multires=list(MULTIRES))
    op.lambda_dssim = a.lambda_dssim
    pp.per_op_autograd = per_op
    torch.manual_seed(6666)
    scene = S.SyntheticScene(a.points, a.frames, a.width, a.height, seed=6666)
    g = S.GaussianModel(lp.sh_degree, hp, device=dev)
    scene.init_gaussians(g)
    scene.make_trained_like(g)
    assert FA.node_width(g._deformation.deformation_net) == 32
    trainer = T.Trainer(scene, g, op, hp, pp, stage="fine", delta_scale=1, sync_every_step=False, fused=False)
    assert trainer.fused is None
    return trainer


def window(trainer, steps, warmup, calls):
    """Steps per second over `steps` iterations after `warmup`, drained and synchronised."""
    import torch
    cams = trainer.cams
    first = 5001
    assert warmup + steps <= 98, "the window must end before the next densify / prune boundary"
    for i in range(warmup):
        trainer.step(first + i, cams=[cams[(17 * i) % len(cams)]])
    trainer.drain()
    torch.cuda.synchronize()
    calls0, replayed0 = calls[0], trainer.replayed
    t0 = time.perf_counter()
    for i in range(steps):
        loss = trainer.step(first + warmup + i, cams=[cams[(17 * (warmup + i)) % len(cams)]])
    trainer.drain()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    node = not getattr(trainer.pipe, "per_op_autograd", False)
    assert calls[0] - calls0 == (steps if node else 0), "the window did not take the path it is named for"
    assert trainer.replayed == replayed0, "an iteration was replayed inside the window"
    assert float(loss) == float(loss), "the loss is not a number"
    return steps / dt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=200_000)
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--width", type=int, default=960)
    ap.add_argument("--height", type=int, default=540)
    ap.add_argument("--lambda-dssim", type=float, default=0.0)
    ap.add_argument("--windows", type=int, default=7, help="timed windows per path and mode, the two paths alternating (at least five)")
    ap.add_argument("--steps", type=int, default=80)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.windows >= 5
    import torch
    N = importlib.import_module(pkg + "._native")
    FA = importlib.import_module(pkg + ".fused_autograd")
    DGR = importlib.import_module(pkg + ".diff_gaussian_rasterization")
    shipped = tuple(FA.NODE_WIDTHS)
    FA.NODE_WIDTHS = (64, 32)                       # the measurement decides the default, so it does not depend on it
    calls, node_render = [0], FA.render

    def counted(*args, **kw):
        calls[0] += 1
        return node_render(*args, **kw)
    FA.render = counted
    dev = torch.device("cuda", 0)
    pair = {"node": _trainer(a, dev, False), "per_op": _trainer(a, dev, True)}
    for t in pair.values():
        for c in t.cams:
            c.device_tensors(dev)
    out = {"library": N.lib().mom_version().decode(), "device": torch.cuda.get_device_name(0), "points": a.points,
           "image": [a.width, a.height], "frames": a.frames, "resolution": RES, "multires": MULTIRES, "channels": 16,
           "lambda_dssim": a.lambda_dssim, "windows": a.windows, "steps_per_window": a.steps, "warmup": a.warmup,
           "order": "per mode: node, per_op, node, per_op, ...: one Trainer(fused=False) per path, alive for the whole run",
           "what": "training steps per second (render, torch loss, backward, densification statistics, Adam), drained and "
                   "synchronised per window", "node_widths_shipped": list(shipped), "modes": {}}
    wins = []
    try:
        for mode in ("exact", "async"):
            DGR.set_sync_mode(mode)
            for path in pair:                           # both paths warmed up in this mode before its first timed window
                window(pair[path], 20, a.warmup, calls)
            runs = {"node": [], "per_op": []}
            for _ in range(a.windows):
                for path in ("node", "per_op"):
                    runs[path].append(window(pair[path], a.steps, a.warmup, calls))
                    print(mode, path, round(runs[path][-1], 1), file=sys.stderr, flush=True)
            rec = {}
            for path, v in runs.items():
                rec[path] = {"median_steps_per_s": round(statistics.median(v), 1), "min_steps_per_s": round(min(v), 1),
                             "max_steps_per_s": round(max(v), 1), "windows_steps_per_s": [round(r, 1) for r in v]}
            rec["ratio_of_medians"] = round(statistics.median(runs["node"]) / statistics.median(runs["per_op"]), 3)
            rec["slowest_node_over_fastest_per_op"] = round(min(runs["node"]) / max(runs["per_op"]), 4)
            wins.append(min(runs["node"]) > max(runs["per_op"]))
            out["modes"][mode] = rec
    finally:
        DGR.set_sync_mode("exact")
    out["criterion"] = {"worst_case_ratio": min(m["slowest_node_over_fastest_per_op"] for m in out["modes"].values()),
                        "node_wins_every_window_in_both_modes": all(wins),
                        "default_node_widths": [64, 32] if all(wins) else [64]}
    txt = json.dumps(out, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(txt + "\n")
    print(txt)


if __name__ == "__main__":
    main()
