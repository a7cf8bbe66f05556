"""Wall time of one densify round, GaussianModel.densify(), on its two routes in one process:

  old   FUSED_DENSIFY = False: densify_and_clone + densify_and_split + prune_points, op by op (three row selections, two
        concatenations of every per-Gaussian tensor and both of its Adam moments, the split's sampling as torch operations)
  new   FUSED_DENSIFY = True: the two masks as torch expressions, then ops.densify_round -- one plan, one host synchronisation for
        three counts, one launch (csrc/densify_round.hip)

Model: bench.build_state at config 2 size (200 000 Gaussians), one optimizer step on seeded gradients so that every per-point group
has its Adam moments, seeded statistics so that a few percent of the rows clone and a few percent split (percent_dense is put at
the median of the candidates' largest scale, so both classes are populated; the record says how many rows each got).  The state
is snapshotted; every sample restores the snapshot, synchronises, times ONE g.densify(...) and synchronises again.  A window is
--rounds samples; the two routes take turns, window by window.  The record keeps every window (its median sample), each route's
median, lowest and highest window, and the criterion of DESIGN 3.6: the slowest new window against the fastest old one.

One process; run it under a time limit (timeout -k 10 600 python tools/densify_round_time.py ...) and start nothing behind it if
it fails.

    python tools/densify_round_time.py [--config c2] [--windows 7] [--rounds 10] [--out profiles/densify_round_time.json]
    python tools/densify_round_time.py --only new --windows 1      # one route alone: what a kernel trace of its own wraps
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
MAX_GRAD = 0.0002
STATS = ("xyz_gradient_accum", "_deformation_accum", "denom", "max_radii2D", "_deformation_table", "_scene_flow")


def seeded_state(cfg, dev, fraction):
    import torch
    import bench
    scene, g, trainer, op = bench.build_state(cfg, dev, fused=True)
    gen = torch.Generator().manual_seed(5)
    n = g.get_xyz.shape[0]
    for grp in g.optimizer.param_groups:
        for p_ in grp["params"]:
            p_.grad = (torch.randn(p_.shape, generator=gen) * 1e-3).to(p_.device).contiguous()
            if p_.dim() == 4:                              # planes are channel-last: keep the parameter's strides
                p_.grad = p_.grad.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    g.optimizer.step()
    g.optimizer.zero_grad(set_to_none=True)
    # a `fraction` of the rows pass the gradient threshold; the scale threshold halves them into clones and splits
    g.xyz_gradient_accum = (torch.rand(n, 1, generator=gen) * (MAX_GRAD / (1.0 - fraction))).to(dev)
    g.denom = torch.ones(n, 1, device=dev)
    g.max_radii2D = (torch.rand(n, generator=gen) * 30).to(dev)
    g._deformation_accum = torch.rand(n, 3, generator=gen).to(dev)
    cand = (g.xyz_gradient_accum.squeeze(1) >= MAX_GRAD)
    g.percent_dense = float(g.get_scaling.max(dim=1).values[cand].median()) / scene.cameras_extent
    return scene, g


def snapshot(g):
    flat = []
    for grp in g._single_groups():
        p = grp["params"][0]
        st = g.optimizer.state[p]
        flat += [p.detach().clone(), st["exp_avg"].clone(), st["exp_avg_sq"].clone()]
    return flat, {k: getattr(g, k).clone() for k in STATS}


def restore(g, snap):
    flat, stats = snap
    it = iter(flat)

    def take(n, t):
        return next(it).clone()
    g._adopt(g._rebuild(take, take))
    for k, v in stats.items():
        setattr(g, k, v.clone())


def one_round(g, scene, snap, fused):
    import torch
    GaussianModel = type(g)
    restore(g, snap)
    torch.manual_seed(11)
    torch.cuda.manual_seed(11)
    GaussianModel.FUSED_DENSIFY = fused
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    g.densify(MAX_GRAD, 0.005, scene.cameras_extent, 20, 5, 5)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c2")
    ap.add_argument("--fraction", type=float, default=0.06, help="share of the rows that clone or split")
    ap.add_argument("--windows", type=int, default=7, help="timed windows per route, the two routes alternating")
    ap.add_argument("--rounds", type=int, default=10, help="rounds (samples) per window")
    ap.add_argument("--only", choices=("old", "new"), default=None, help="one route alone, nothing compared or written")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import bench
    N = importlib.import_module(pkg + "._native")
    ops = importlib.import_module(pkg + ".ops")
    assert getattr(ops.BACKEND, "densify_round", None) is not None
    dev = torch.device("cuda", 0)
    scene, g = seeded_state(bench.CONFIGS[a.config], dev, a.fraction)
    default = type(g).FUSED_DENSIFY
    snap = snapshot(g)
    n0 = g.get_xyz.shape[0]
    routes = {"old": False, "new": True}
    if a.only:
        routes = {a.only: routes[a.only]}
    ends = {}
    for name, fused in routes.items():                 # both routes warmed up (code objects, allocator) before the first window
        for _ in range(3):
            one_round(g, scene, snap, fused)
        ends[name] = {"rows": g.get_xyz.shape[0], "xyz": g._xyz.detach().clone(), "f_rest": g._features_rest.detach().clone(),
                      "m_xyz": g.optimizer.state[g._xyz]["exp_avg"].clone()}
    runs = {name: [] for name in routes}
    for _ in range(a.windows):
        for name, fused in routes.items():
            runs[name].append(statistics.median(one_round(g, scene, snap, fused) for _ in range(a.rounds)))
            print(name, round(runs[name][-1], 3), "ms", file=sys.stderr, flush=True)
    type(g).FUSED_DENSIFY = default
    if a.only:
        print(json.dumps({a.only: runs[a.only], "rows_before": n0, "rows_after": ends[a.only]["rows"]}))
        return
    grads = snap[1]["xyz_gradient_accum"] / snap[1]["denom"]
    cand = grads.squeeze(1) >= MAX_GRAD
    restore(g, snap)
    big = g.get_scaling.max(dim=1).values > g.percent_dense * scene.cameras_extent
    C_, S = int((cand & ~big).sum()), int((cand & big).sum())
    kept = n0 - S + C_
    same = (ends["old"]["rows"] == ends["new"]["rows"] and torch.equal(ends["old"]["xyz"][:kept], ends["new"]["xyz"][:kept])
            and torch.equal(ends["old"]["f_rest"], ends["new"]["f_rest"]) and torch.equal(ends["old"]["m_xyz"], ends["new"]["m_xyz"]))
    child = float((ends["old"]["xyz"][kept:] - ends["new"]["xyz"][kept:]).abs().max()) if S else 0.0
    out = {"library": N.lib().mom_version().decode(), "device": torch.cuda.get_device_name(0), "config": a.config,
           "rows_before": n0, "rows_cloned": C_, "rows_split": S, "rows_after": ends["new"]["rows"], "max_grad": MAX_GRAD,
           "windows": a.windows, "rounds_per_window": a.rounds,
           "order": "old, new, old, new, ...: one model, restored from one snapshot before every round",
           "what": "host wall time of one GaussianModel.densify() call in ms, device synchronised before and after; a window is the "
                   "median of its rounds; median, lowest and highest window per route",
           "outputs_equal_outside_child_positions": bool(same), "largest_child_position_difference": child}
    for name, v in runs.items():
        out[name] = {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3),
                     "windows_ms": [round(r, 3) for r in v]}
    out["ratio_of_medians_old_over_new"] = round(statistics.median(runs["old"]) / statistics.median(runs["new"]), 3)
    out["criterion"] = {"fastest_old_over_slowest_new": round(min(runs["old"]) / max(runs["new"]), 4),
                        "new_wins_every_window": max(runs["new"]) < min(runs["old"])}
    out["fused_densify_default"] = bool(default)
    out["launches_per_round"] = "not measured (no kernel trace taken)"
    txt = json.dumps(out, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(txt + "\n")
    print(txt)


if __name__ == "__main__":
    main()
