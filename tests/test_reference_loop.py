"""The reference's OWN training loop (train_4DGS.py:46-301 scene_reconstruction) driven against this package through
install_dropin(): every `from scene import ...`, `from gaussian_renderer import ...`, `from utils... import ...`,
`from arguments import ...` of the script resolves to the mirror, the data comes from a stage-1 directory written by
scene/stage1.py and read back by scene.Scene, and the kernels are the CPU oracle (no GPU here).

(a) The script runs unchanged: oracle/make_reference_run_fixture.py runs it against a checkout of the reference (the file
never enters this repository) and stores, iteration by iteration, the losses and the final model it produced in
tests/golden/g13_reference_loop.npz.  (b) This package's own Trainer produces the same losses and final model from the same
seeds -- i.e. train.Trainer is a faithful restatement of the reference's iteration body."""
import copy
import importlib
import math
import os
import random
import sys
import types

import numpy as np
import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g13_reference_loop.npz")
pkg_name = "iclr2025_3d-mom_amd"


def cuda_to_cpu(monkeypatch):
    """The reference hard-codes device="cuda" (train_4DGS.py:68,193): send those tensors to the CPU."""
    for fn in ("zeros", "ones", "empty", "tensor", "full", "rand", "randn", "zeros_like", "ones_like"):
        orig = getattr(torch, fn)

        def wrap(*a, __orig=orig, **k):
            if "device" in k and str(k["device"]).startswith("cuda"):
                k["device"] = "cpu"
            return __orig(*a, **k)
        monkeypatch.setattr(torch, fn, wrap)
    monkeypatch.setattr(torch.Tensor, "cuda", lambda self, *a, **k: self)

    class Event:
        def __init__(self, enable_timing=False):
            pass

        def record(self):
            pass

        def elapsed_time(self, other):
            return 0.0
    monkeypatch.setattr(torch.cuda, "Event", Event)
    monkeypatch.setattr(torch.cuda, "empty_cache", lambda: None)
    monkeypatch.setitem(sys.modules, "imageio", types.SimpleNamespace(mimwrite=lambda *a, **k: None))


@pytest.fixture()
def cuda_is_cpu(monkeypatch):
    cuda_to_cpu(monkeypatch)
    saved = {k: sys.modules.get(k) for k in list(sys.modules) if k.split(".")[0] in ("scene", "utils", "arguments", "gaussian_renderer",
                                                                                    "simple_knn", "diff_gaussian_rasterization")}
    yield
    for k in [k for k in sys.modules if k.split(".")[0] in ("scene", "utils", "arguments", "gaussian_renderer", "simple_knn",
                                                            "diff_gaussian_rasterization")]:
        del sys.modules[k]
    sys.modules.update({k: v for k, v in saved.items() if v is not None})


def _setup(tmp_path, seed=6666):
    pkg = importlib.import_module(pkg_name)
    A = importlib.import_module(pkg_name + ".arguments")
    S = importlib.import_module(pkg_name + ".scene")
    stage1 = importlib.import_module(pkg_name + ".scene.stage1")
    args, lp, op, pp, hp = A.default_args(time_resolution=6)
    lp.source_path, lp.model_path = str(tmp_path), str(tmp_path)
    synth = S.SyntheticScene(600, 60, 48, 32, seed=11)
    path = stage1.write_stage1_outputs(str(tmp_path), synth)
    assert stage1.check_stage1_dir(str(tmp_path)) == (600, 5, 60)
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)
    g = S.GaussianModel(lp.sh_degree, hp, device="cpu")
    scene = S.Scene(path, str(tmp_path), lp, g, flow_scale=2)
    return pkg, lp, op, pp, hp, g, scene


def _state(g):
    return {k: getattr(g, k).detach().clone() for k in ("_xyz", "_features_dc", "_features_rest", "_scaling", "_rotation", "_opacity")}


def test_reference_scene_reconstruction_runs_on_the_dropin_and_matches_the_trainer(tmp_path, cuda_is_cpu):
    from oracle import cpu_backend
    torch.set_num_threads(1)
    n_coarse, n_fine = 3, 3
    ref = np.load(GOLDEN)
    assert (int(ref["n_coarse"]), int(ref["n_fine"])) == (n_coarse, n_fine)
    losses_ref = ref["losses"]
    assert len(losses_ref) == n_coarse + n_fine and all(np.isfinite(losses_ref))
    final_ref = {k: torch.from_numpy(ref[k]) for k in ("_xyz", "_features_dc", "_features_rest", "_scaling", "_rotation", "_opacity")}
    plane_ref = torch.from_numpy(ref["plane_1_2"])
    with cpu_backend.installed():
        # ---- (b) this package's Trainer from the same seeds
        pkg, lp, op, pp, hp, g2, scene2 = _setup(tmp_path / "b")
        assert len(scene2.getTrainCameras()) == 5 and len(scene2.getTrainCameras_2()) == 65 and len(scene2.getVideoCameras_side()) == 59
        T = importlib.import_module(pkg_name + ".train")
        losses_own = []
        tr = T.Trainer(scene2, g2, op, hp, pp, stage="coarse", sync_every_step=True)
        tr.stack = copy.copy(tr.cams)
        for it in range(1, n_coarse + 1):
            losses_own.append(float(tr.step(it)))
        tr = T.Trainer(scene2, g2, op, hp, pp, stage="fine", delta_scale=1, sync_every_step=True)
        for it in range(1, n_fine + 1):
            losses_own.append(float(tr.step(it)))
    np.testing.assert_allclose(losses_own, losses_ref, rtol=1e-6)
    # The model: the reference's values to rtol 1e-6 / atol 1e-7 (bit for bit where torch's CPU math rounds as on the host that
    # wrote the fixture).  torch takes its sqrt, exp and matmul from MKL, whose last bit depends on the processor, and Adam's eps
    # of 1e-15 turns such a difference in a gradient that cancels to nearly zero into a different step of that element.  So a
    # few elements may stand apart, but none further than two Adam runs from the same start can: twice the largest distance
    # Adam moves an element in the steps taken (_adam_reach) at its group's learning rate.
    s = g2.spatial_lr_scale
    lr = {"_xyz": op.position_lr_init * s, "_features_dc": op.feature_lr, "_features_rest": op.feature_lr / 20.0,
          "_scaling": op.scaling_lr, "_rotation": op.rotation_lr, "_opacity": op.opacity_lr, "plane": op.grid_lr_init * s}
    reach = 2 * _adam_reach(n_coarse) + 2 * _adam_reach(n_fine)        # each stage's Trainer starts a new optimizer
    final_own = _state(g2)
    final_own["plane"], final_ref["plane"] = g2._deformation.deformation_net.grid.grids[1][2].detach(), plane_ref
    for k in final_ref:
        diff = (final_own[k] - final_ref[k]).abs()
        apart = diff > 1e-7 + 1e-6 * final_ref[k].abs()
        assert int(apart.sum()) <= 0.05 * diff.numel(), (k, int(apart.sum()), diff.numel())
        assert float(diff.max()) <= lr[k] * reach, (k, float(diff.max()), lr[k] * reach)


def _adam_reach(steps, b1=0.9, b2=0.999):
    """Bound on sum over Adam's first `steps` steps of |update| / lr: by Cauchy-Schwarz on the two moment sums, step t moves an
    element by at most lr (1-b1) / sqrt(1-b2) * sqrt(sum_{j<t} (b1^2/b2)^j) * sqrt(1-b2^t) / (1-b1^t) (= lr at t = 1)."""
    return sum((1 - b1) / math.sqrt(1 - b2) * math.sqrt(sum((b1 * b1 / b2) ** j for j in range(t)))
               * math.sqrt(1 - b2 ** t) / (1 - b1 ** t) for t in range(1, steps + 1))
