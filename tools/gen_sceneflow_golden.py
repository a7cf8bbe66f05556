"""Writes tests/golden/g15_scene_flow_fit.npz: a small scene-flow fit by the REFERENCE's own optimize_motion (train_motion.py:65-207).

Run by hand on a machine that has a checkout of the reference; the tests read only the file it writes.

    python tools/gen_sceneflow_golden.py --reference /path/to/ICLR2025_3D-MOM [--out tests/golden/g15_scene_flow_fit.npz]

train_motion.py imports the whole of stage 1 at module level (depth, the flow estimator, the video GAN and what they need: cv2,
torchvision, mediapy, cupy, lpips, imageio, kornia, av ...).  optimize_motion touches none of it, so every module that is not
installed is replaced by an empty stand-in before the import.  The function is then called unbound on a namespace that carries
the five attributes it reads (render_poses, internel_render_poses, K, H, W).  Two names of the module are wrapped while it runs,
without changing what they return: `interp_grid`, to record the 2D flow it samples at each view's unflowed pixels, and `np.where`,
to record each view's valid index list.

The case: P = 300 points, H = W = 24, 2 x 3 views, 12 epochs, flow images of about 3 px of noise (no target is near 0: a sign
descent on a zero target amplifies rounding noise).  A few points lie outside some views."""
import argparse
import importlib
import importlib.abc
import importlib.machinery
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
STUBS = ("cv2", "torchvision", "mediapy", "cupy", "lpips", "imageio", "kornia", "av")
P, H, W, E = 300, 24, 24, 12


class _Stub(types.ModuleType):
    """A module that has every attribute and every submodule; nothing in it is ever called by optimize_motion."""
    __path__ = []

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        child = _Stub(self.__name__ + "." + name)
        setattr(self, name, child)
        return child

    def __call__(self, *a, **k):
        return self


class _StubFinder(importlib.abc.MetaPathFinder, importlib.abc.Loader):
    """Last on sys.meta_path: serves a stand-in for the listed top-level modules (and their submodules) when nothing else has them."""
    def __init__(self, names):
        self.names, self.used = set(names), set()

    def find_spec(self, fullname, path=None, target=None):
        if fullname.split(".")[0] in self.names:
            return importlib.machinery.ModuleSpec(fullname, self, is_package=True)
        return None

    def create_module(self, spec):
        self.used.add(spec.name.split(".")[0])
        return _Stub(spec.name)

    def exec_module(self, module):
        pass


def import_reference(ref_dir, extra=()):
    finder = _StubFinder(STUBS + tuple(extra))
    sys.meta_path.append(finder)
    sys.path.insert(0, ref_dir)
    cwd = os.getcwd()
    os.chdir(ref_dir)
    try:
        mod = importlib.import_module("train_motion")
    finally:
        os.chdir(cwd)
    return mod, sorted(finder.used)


def rot(ax, ay):
    cx, sx, cy, sy = np.cos(ax), np.sin(ax), np.cos(ay), np.sin(ay)
    return np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])


def make_case(seed=15):
    rng = np.random.default_rng(seed)
    pts = np.stack([rng.uniform(-1.0, 1.0, P), rng.uniform(-1.0, 1.0, P), rng.uniform(2.5, 4.0, P)]).astype(np.float32)
    pts[:, :4] = np.array([[3.5, -3.5, 0.2, 0.1], [0.1, 0.2, 3.5, -3.5], [3.0, 3.0, 3.0, 3.0]], np.float32)     # outside every view
    K = np.array([[30.0, 0, W / 2], [0, 30.0, H / 2], [0, 0, 1]], np.float32)
    render = np.stack([np.concatenate([rot(0.02, -0.05), np.array([[0.05], [0.0], [0.02]])], axis=1),
                       np.concatenate([rot(-0.04, 0.08), np.array([[-0.1], [0.04], [0.0]])], axis=1)])
    internal = np.stack([np.concatenate([rot(0.0, 0.0), np.zeros((3, 1))], axis=1),
                         np.concatenate([rot(0.03, 0.1), np.array([[0.15], [0.0], [0.05]])], axis=1),
                         np.concatenate([rot(-0.06, -0.12), np.array([[-0.2], [0.05], [0.1]])], axis=1)])
    gen = torch.Generator().manual_seed(seed)
    t2c = (torch.randn(len(render) * len(internal), 1, 2, H, W, generator=gen) * 3.0).float()
    return pts, K, render, internal, t2c


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="a checkout of cvsp-lab/ICLR2025_3D-MOM")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "g15_scene_flow_fit.npz"))
    ap.add_argument("--stub", nargs="*", default=[], help="further top-level modules to stand in for")
    a = ap.parse_args()
    tm, used = import_reference(os.path.abspath(a.reference), a.stub)
    print("stand-ins used for:", used)
    pts, K, render, internal, t2c = make_case()
    nv = len(render) * len(internal)
    train_data = {"pcd_points": pts.copy(), "frames": [{"T2C_flow": [t2c[k].clone()], "our_flow": []} for k in range(nv)]}

    sampled, wheres = [], []
    real_interp = tm.interp_grid

    def interp(points, values, xi, **kw):
        out = real_interp(points, values, xi, **kw)
        if len(sampled) < nv:                       # the first nv calls sample the targets (:120); the last nv resample our_flow (:198)
            sampled.append((np.array(xi), np.array(out)))
        return out

    class NumpyProxy:
        def __getattr__(self, name):
            return getattr(np, name)

        @staticmethod
        def where(*args, **kw):
            out = np.where(*args, **kw)
            wheres.append(np.array(out[0]))
            return out

    tm.interp_grid, tm.np = interp, NumpyProxy()
    ns = types.SimpleNamespace(render_poses=render, internel_render_poses=internal, K=K, H=H, W=W)
    torch.manual_seed(0)
    torch.set_num_threads(1)
    try:
        train_data, scene_flow = tm.MotionOptimization.optimize_motion(ns, None, None, train_data, [], E)
    finally:
        tm.interp_grid, tm.np = real_interp, np
    scene_flow = scene_flow.detach().numpy()
    assert scene_flow.shape == (3, P) and np.isfinite(scene_flow).all() and len(sampled) == nv and len(wheres) == nv * (1 + E)
    out = {"points": pts, "K": K, "render_poses": render, "internal_poses": internal, "t2c_flow": t2c.numpy(), "epochs": np.int64(E),
           "H": np.int64(H), "W": np.int64(W), "scene_flow": scene_flow,
           "our_flow": np.stack([train_data["frames"][k]["our_flow"][0].numpy() for k in range(nv)])}
    for k in range(nv):
        out[f"valid_{k}"] = wheres[k].astype(np.int64)
        out[f"pix0_{k}"] = sampled[k][0].T.astype(np.float32)              # as train_motion.py:183 casts it
        out[f"gt_{k}"] = sampled[k][1].T                                   # float64, as griddata returns it
        for e in range(E):                                                 # the training loop recomputes the same valid set
            assert np.array_equal(wheres[nv + e * nv + k], wheres[k])
    np.savez_compressed(a.out, **out)
    print(a.out, os.path.getsize(a.out), "bytes;", "valid per view:", [len(out[f"valid_{k}"]) for k in range(nv)],
          "largest |scene_flow|:", float(np.abs(scene_flow).max()))


if __name__ == "__main__":
    main()
