"""Steps per second of the COARSE stage (no deformation field; train_4DGS.py with stage "coarse") on three paths, and of the fine
fused step at the same config for comparison:

  op-by-op   render() with pipe.per_op_autograd = True (torch activations, the rasterizer node) + loss.backward() + optimizer.step()
  one-node   render() as one autograd node (fused_autograd.render_coarse) + loss.backward() + optimizer.step()
  fused      Trainer(stage="coarse", fused=True): the explicit launch sequence of fused_step.FusedCoarseStep

Every path runs Trainer.step over a window of coarse iterations with no densify / prune / opacity-reset / SH boundary
(2601..2690 by default), after a warm-up inside the same window, and trainer.drain() before the clock stops.

    python tools/coarse_rate.py [--config c2] [--steps 80] [--warmup 10]
"""
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


def _state(cfg, dev, stage, fused, per_op):
    import torch
    A = importlib.import_module("iclr2025_3d-mom_amd.arguments")
    S = importlib.import_module("iclr2025_3d-mom_amd.scene")
    T = importlib.import_module("iclr2025_3d-mom_amd.train")
    args, lp, op, pp, hp = A.default_args(time_resolution=cfg["time_res"])
    pp.per_op_autograd = per_op
    torch.manual_seed(6666)
    scene = S.SyntheticScene(cfg["P"], cfg["F"], cfg["W"], cfg["H"], seed=6666)
    g = S.GaussianModel(lp.sh_degree, hp, device=dev)
    scene.init_gaussians(g)
    scene.make_trained_like(g)
    return T.Trainer(scene, g, op, hp, pp, stage=stage, delta_scale=1, sync_every_step=False, fused=fused)


def rate(cfg, dev, stage, fused, per_op, steps, warmup, first):
    import torch
    trainer = _state(cfg, dev, stage, fused, per_op)
    assert (trainer.fused is not None) == fused
    cams = trainer.cams
    for c in cams:
        c.device_tensors(dev)
    it = first
    for i in range(warmup):
        trainer.step(it, cams=[cams[i % len(cams)]])
        it += 1
    trainer.drain()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        trainer.step(it, cams=[cams[(warmup + i) % len(cams)]])
        it += 1
    trainer.drain()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    return steps / dt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c2", choices=sorted(bench.CONFIGS))
    ap.add_argument("--steps", type=int, default=80)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--first", type=int, default=2601, help="first iteration of the window (no boundary inside it)")
    a = ap.parse_args()
    import torch
    assert a.first + a.warmup + a.steps <= 2700, "the window must end before iteration 2700 (a densify / prune boundary)"
    cfg = bench.CONFIGS[a.config]
    dev = torch.device("cuda", 0)
    out = {"config": a.config, "steps": a.steps, "warmup": a.warmup, "window": [a.first, a.first + a.warmup + a.steps - 1]}
    out["coarse_op_by_op"] = rate(cfg, dev, "coarse", False, True, a.steps, a.warmup, a.first)
    out["coarse_one_node"] = rate(cfg, dev, "coarse", False, False, a.steps, a.warmup, a.first)
    out["coarse_fused"] = rate(cfg, dev, "coarse", True, False, a.steps, a.warmup, a.first)
    out["fine_fused"] = rate(cfg, dev, "fine", True, False, a.steps, a.warmup, a.first)
    out = {k: (round(v, 1) if isinstance(v, float) else v) for k, v in out.items()}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
