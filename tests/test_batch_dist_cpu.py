"""A trainer with batch_size > 1 on the multi-GPU paths stays what it was before the fused step took batches: parallel.attach()
leaves it WITHOUT a fused step, so every iteration, drain() and save() follow the autograd path's own protocol, sharded Adam and
the tile-row shard are refused as they always were, and a trainer with batch_size 1 keeps its fused step.  No GPU, no process group:
attach() only builds the context."""
import importlib
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CFG = dict(P=300, F=2, W=32, H=32, time_res=4, name="attach")


def _trainer(batch_size, stage="fine"):
    import torch
    A = importlib.import_module("iclr2025_3d-mom_amd.arguments")
    S = importlib.import_module("iclr2025_3d-mom_amd.scene")
    T = importlib.import_module("iclr2025_3d-mom_amd.train")
    from oracle import cpu_backend
    with cpu_backend.installed():
        args, lp, op, pp, hp = A.default_args(time_resolution=CFG["time_res"])
        op.batch_size = batch_size
        torch.manual_seed(1)
        scene = S.SyntheticScene(CFG["P"], CFG["F"], CFG["W"], CFG["H"], seed=1)
        g = S.GaussianModel(lp.sh_degree, hp, device=torch.device("cpu"))
        scene.init_gaussians(g)
        return T.Trainer(scene, g, op, hp, pp, stage=stage, delta_scale=1, sync_every_step=False, fused=True)


def test_attach_leaves_a_batch_trainer_on_the_autograd_path_as_before():
    par = importlib.import_module("iclr2025_3d-mom_amd.parallel")
    RC = importlib.import_module("iclr2025_3d-mom_amd.diff_gaussian_rasterization._C")
    trainer = _trainer(2)
    assert trainer.fused is not None                    # one GPU: the fused step takes the batch
    dc = par.attach(trainer, 0, 2)
    assert trainer.fused is None and trainer.dist is dc and dc.world == 2
    # what Trainer.step / drain / save do now depends on `fused is None` alone: the autograd path's own drain
    calls = []
    trainer.drain_autograd = lambda: calls.append("autograd")
    trainer._alog.append((1, 1, 5001, []))
    old = RC._state["mode"]
    RC._state["mode"] = "async"
    try:
        trainer.drain()
    finally:
        RC._state["mode"] = old
    assert calls == ["autograd"]


def test_sharded_adam_and_the_tile_row_shard_refuse_a_batch_trainer_as_before():
    par = importlib.import_module("iclr2025_3d-mom_amd.parallel")
    with pytest.raises(ValueError, match="shard_adam needs the fused step"):
        par.attach(_trainer(2), 0, 2, shard_adam=True)
    with pytest.raises(ValueError, match="tile-row sharding is implemented by the fused step"):
        par.attach(_trainer(2), 0, 2, mode="tile-row")


def test_a_trainer_with_one_camera_per_rank_keeps_its_fused_step():
    par = importlib.import_module("iclr2025_3d-mom_amd.parallel")
    trainer = _trainer(1)
    fs = trainer.fused
    dc = par.attach(trainer, 1, 2)
    assert trainer.fused is fs and fs.dist is dc and trainer.dist is dc
