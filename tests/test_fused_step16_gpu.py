"""The fused training step (fused_step.FusedStep16, Trainer(fused=True)'s choice through fused_step.fine_step) on a model of the dnerf/eulerian_150_16 shape -- two HexPlane levels of 16-channel
planes, 32 features into the shipped network -- against the render() + loss.backward() path of the same model and against the CPU
oracle.  The step writes no kernel of its own: the one-launch field forward (csrc/deform_field16.hip), the MLP backward on 32
features (csrc/deform_mlp.hip) and the 16-channel HexPlane backward (csrc/hexplane.hip) in the launch sequence of the 32 x 2
step.  Tolerances are those the suite already holds the 32 x 2 step to for the same comparisons (named at each test): both paths
run the same kernels here too and differ in the order of their float atomics.  (The step activates the field's raw outputs with
torch's exp / normalize / sigmoid, as the op-by-op path does: with the kernel's own activated outputs the gradients of the tiny
scene sat up to 1.1e-3 of a tensor's scale apart)"""
import ctypes as C
import functools
import importlib
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

pkg = "iclr2025_3d-mom_amd"
N = importlib.import_module(pkg + "._native")
CFG = dict(P=6000, F=4, W=160, H=96, time_res=10, name="tiny")           # tests/test_whole_step_gpu.py::CFG
# tests/test_whole_step_gpu.py::LIVE: the six Gaussian parameters, two planes of each level, w0 ([64,32] here), b0, head weights, a head bias
LIVE = ("xyz", "f_dc", "f_rest", "scaling", "rotation", "opacity", "plane_0_0", "plane_0_2", "plane_1_3", "plane_1_5", "w0", "b0",
        "w_pos1", "w_pos3", "w_sc1", "w_rot3", "b_rot3")
GAUSSIAN = LIVE[:6]
BOX = "asym_a"                        # tests/hexplane_box_cases.py: the torch form and the contracted form differ at its min faces
SHIFT_Z = 3.0                         # the cloud sits around z = 3 in front of the cameras; the box around the origin


def _tensors(g):
    dn = g._deformation.deformation_net
    return {"xyz": g._xyz, "f_dc": g._features_dc, "f_rest": g._features_rest, "scaling": g._scaling, "rotation": g._rotation,
            "opacity": g._opacity, "plane_0_0": dn.grid.grids[0][0], "plane_0_2": dn.grid.grids[0][2],
            "plane_1_3": dn.grid.grids[1][3], "plane_1_5": dn.grid.grids[1][5], "w0": dn.feature_out[0].weight,
            "b0": dn.feature_out[0].bias, "w_pos1": dn.pos_deform[1].weight, "w_pos3": dn.pos_deform[3].weight,
            "w_sc1": dn.scales_deform[1].weight, "w_rot3": dn.rotations_deform[3].weight, "b_rot3": dn.rotations_deform[3].bias}


def _model(device="cuda", P=CFG["P"], channels=16, multires=(1, 2), res=(64, 64, 64, 150), lambda_dssim=0.0, B=1, box=False):
    """tests/test_hexplane16_gpu.py::_model16 with the shape open.  box: the cloud is moved by -SHIFT_Z along z into the asymmetric
    box BOX, which becomes the field's box, with one Gaussian exactly on the z min face, one on the z max face and one on the min
    corner's z edge; _cams() then moves the cameras by the same amount."""
    A = importlib.import_module(pkg + ".arguments")
    S = importlib.import_module(pkg + ".scene")
    kc = {'grid_dimensions': 2, 'input_coordinate_dim': 4, 'output_coordinate_dim': channels, 'resolution': list(res)}
    args, lp, op, pp, hp = A.default_args(kplanes_config=kc, multires=list(multires))
    assert hp.net_width == 64 and hp.defor_depth == 0 and hp.no_do and hp.no_dshs
    op.lambda_dssim, op.batch_size = lambda_dssim, B
    torch.manual_seed(6666)
    scene = S.SyntheticScene(P, CFG["F"], CFG["W"], CFG["H"], seed=6666)
    g = S.GaussianModel(lp.sh_degree, hp, device=torch.device(device))
    scene.init_gaussians(g)
    scene.make_trained_like(g)
    if box:
        import hexplane_box_cases as hb
        hi, lo, differ = hb.BOXES[BOX]
        assert differ
        for size in (64, 128):         # the emulation of tests/hexplane_box_cases.py at THIS model's plane sizes
            ct, cc = hb.coord_torch_form(lo[2], hi[2], lo[2]), hb.coord_contracted_form(lo[2], hi[2], lo[2])
            assert not hb.clipped(ct, size) and hb.clipped(cc, size)
        g._deformation.deformation_net.set_aabb(list(hi), list(lo))
        with torch.no_grad():
            g._xyz[:, 2] -= SHIFT_Z
            mid = P // 2               # in the middle of the image
            g._xyz[mid, 2], g._xyz[mid + 1, 2], g._xyz[mid + 2, 2] = lo[2], hi[2], lo[2]
            g._xyz[mid + 2, 0] = float(np.nextafter(np.float32(lo[0]), np.float32(hi[0])))      # (far off screen: it is culled)
    return scene, g, op, pp, hp


def _trainer(fused, **kw):
    T = importlib.import_module(pkg + ".train")
    scene, g, op, pp, hp = _model(**kw)
    trainer = T.Trainer(scene, g, op, hp, pp, stage="fine", delta_scale=1, sync_every_step=False, fused=fused)
    assert (trainer.fused is not None) == fused
    return scene, g, trainer


def _cams(trainer, box):
    """The trainer's cameras; for the box model the same cameras moved with the cloud (camera space = world + (0, 0, SHIFT_Z))."""
    if not box:
        return trainer.cams
    if getattr(trainer, "_box_cams", None) is None:
        Camera = importlib.import_module(pkg + ".scene.cameras").Camera
        trainer._box_cams = [Camera(colmap_id=c.colmap_id, R=np.asarray(c.R), T=np.asarray(c.T) + np.array([0.0, 0.0, SHIFT_Z]),
                                    FoVx=c.FoVx, FoVy=c.FoVy, image=c._image_host, gt_alpha_mask=None, image_name=c.image_name,
                                    uid=c.uid, data_device=c.data_device, time=c.time, frame_num=c.frame_num) for c in trainer.cams]
    return trainer._box_cams


def _cam_lists(trainer, it, B, box):
    cams = _cams(trainer, box)
    if B == 1:
        return [cams[(3 * it + 1) % len(cams)]]                                   # tests/test_fused_step_gpu.py::_run
    return [cams[(3 * it + 1 + 4 * j) % len(cams)] for j in range(B)]           # tests/test_batch_step_gpu.py::_cams_of


def _collect(g, moments):
    t = _tensors(g)
    params = {k: v.detach().float().cpu().numpy().copy() for k, v in t.items()}
    for k, v in (("accum", g.xyz_gradient_accum), ("denom", g.denom), ("maxr", g.max_radii2D)):
        params[k] = v.detach().float().cpu().numpy().copy()
    mom = {k: g.optimizer.state[t[k]]["exp_avg"].detach().float().cpu().numpy().copy() for k in LIVE} if moments else {}
    return params, mom


def _run(fused, steps=1, lambda_dssim=0.0, B=1, P=CFG["P"], box=False):
    """tests/test_fused_step_gpu.py::_run on the 16 x 2 model.  Computed once per argument list and shared: callers do not write
    into what it returns."""
    return _run_once(bool(fused), int(steps), float(lambda_dssim), int(B), int(P), bool(box))


@functools.lru_cache(maxsize=None)
def _run_once(fused, steps, lambda_dssim, B, P, box):
    scene, g, trainer = _trainer(fused, P=P, lambda_dssim=lambda_dssim, B=B, box=box)
    if fused:
        assert trainer.fused.F == 32
    losses = []
    for it in range(steps):
        losses.append(float(trainer.step(5001 + it, cams=_cam_lists(trainer, it, B, box))))
    if fused:
        assert trainer._serial == steps and trainer.replayed == 0
        trainer.drain()
    torch.cuda.synchronize()
    params, moments = _collect(g, steps == 1)
    lr_max = max(grp["lr"] for grp in g.optimizer.param_groups)
    for d in (params, moments):
        for a in d.values():
            a.setflags(write=False)
    return tuple(losses), params, moments, lr_max


def _one_step_agrees(lambda_dssim=0.0, B=1, P=CFG["P"], box=False, what=""):
    """Loss at rtol 2e-5; the gradient, read through Adam's first moment after one step ((1 - beta1) x gradient exactly), within
    5e-5 of the tensor's largest magnitude; denom and max_radii2D equal (tests/test_fused_step_gpu.py, tests/test_batch_step_gpu.py)."""
    la, pa, ma, _ = _run(False, 1, lambda_dssim, B, P, box)
    lf, pf, mf, _ = _run(True, 1, lambda_dssim, B, P, box)
    print(what, "loss fused", lf, "autograd", la)
    worst = {}
    for k in LIVE:
        assert ma[k].shape == mf[k].shape and float(np.abs(ma[k]).max()) > 0, k
        worst[k] = float(np.abs(mf[k] - ma[k]).max()) / max(1e-30, float(np.abs(ma[k]).max()))
    print(what, "gradient errors relative to the tensor's max:", {k: "%.2e" % v for k, v in worst.items()})
    acc = float(np.abs(pf["accum"] - pa["accum"]).max()) / max(1e-30, float(np.abs(pa["accum"]).max()))
    print(what, "xyz_gradient_accum error relative to its max: %.2e" % acc)
    np.testing.assert_allclose(lf, la, rtol=2e-5)
    for k, e in worst.items():
        assert e <= 5e-5, ("gradient", what, k, e)
    np.testing.assert_array_equal(pf["denom"], pa["denom"])
    np.testing.assert_array_equal(pf["maxr"], pa["maxr"])
    assert float(pa["denom"].sum()) > 0
    return pa, pf, acc


def _three_steps_agree(lambda_dssim=0.0, B=1, steps=3):
    """tests/test_fused_step_gpu.py's parameter rule: at most 1e-4 of a tensor's elements outside 2e-4 scale + 1e-6 and none beyond
    2 steps lr_max 1.01 (Adam turns the sign of a vanishing gradient into a full learning-rate step)."""
    la, pa, _, lr_max = _run(False, steps, lambda_dssim, B)
    lf, pf, _, _ = _run(True, steps, lambda_dssim, B)
    figures = {}
    for k in LIVE:
        a, b = pf[k], pa[k]
        scale = max(1e-12, float(np.abs(b).max()))
        diff = np.abs(a - b)
        tight = 2e-4 * scale + 1e-6
        figures[k] = (float((diff > tight).mean()), float(diff.max()), tight)
    print("after", steps, "steps: (fraction outside the tight tolerance, largest difference, tight tolerance)",
          {k: "%.1e %.2e %.2e" % v for k, v in figures.items()})
    np.testing.assert_allclose(lf, la, rtol=2e-5)
    for k, (outliers, worst, tight) in figures.items():
        assert outliers <= 1e-4, (k, "fraction of elements outside the tight tolerance", outliers)
        assert worst <= 2.0 * steps * lr_max * 1.01 + tight, (k, worst, lr_max)
    np.testing.assert_array_equal(pf["denom"], pa["denom"])
    np.testing.assert_array_equal(pf["maxr"], pa["maxr"])


# ---------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("lambda_dssim", [0.0, 0.2])
def test_fused_step_matches_autograd_path_on_a_16_x_2_model(lambda_dssim):
    """tests/test_fused_step_gpu.py::test_fused_step_matches_autograd_path on the 16 x 2 model, its figures unchanged: one step
    (loss, gradients), then three (parameters).  Before the fused step took 32 features, Trainer(fused=True) raised MomError here.

    Measured on an MI355X (the printed maxima): loss equal to the bit, gradients within 4.4e-6 (scaling), no element outside the
    tight tolerance after three steps."""
    pa, pf, _ = _one_step_agrees(lambda_dssim, what="lambda %.1f" % lambda_dssim)
    assert pa["w0"].shape == (64, 32) and pa["plane_0_0"].shape[1] == 16
    _three_steps_agree(lambda_dssim)


# ---------------------------------------------------------------------------------------------------------------- 2
def test_the_steps_deformed_state_is_the_models_own():
    """After one forward_backward: pts is forward_dynamic's output under no_grad bit for bit (field16 is the two calls bit for bit),
    and so are the raw scales and rotations; the activated copies against torch.exp / normalize / sigmoid at 1e-6, the allowance
    tests/test_fused_step_gpu.py grants one kernel with expf against torch's ops (measured: 0, the step uses torch's); feat is
    [P,32] and is HexPlaneField's own answer bit for bit."""
    scene, g, trainer = _trainer(True)
    fs, cam = trainer.fused, trainer.cams[2]
    assert float(cam.time) > 0 and cam.frame_num > 0
    fs.forward_backward(cam, 1)
    torch.cuda.synchronize()
    P = g._xyz.shape[0]
    assert tuple(fs.feat.shape) == (P, 32) and tuple(fs.dfeat.shape) == (P, 32) and tuple(fs.a0.shape) == (P, 64)
    dn = g._deformation.deformation_net
    with torch.no_grad():
        pts, sc_raw, rot_raw, op_raw, shs = g._deformation(g._xyz, g._scaling, g._rotation, g._opacity, g.get_features, float(cam.time),
                                                            g.get_flow, cam.frame_num, 1)
        feat = dn.grid(g._xyz, float(cam.time))
    torch.cuda.synchronize()
    assert float((pts - g._xyz).abs().max()) > 0
    assert torch.equal(fs.pts, pts)
    assert torch.equal(fs.sc_d, sc_raw) and torch.equal(fs.rot_d, rot_raw) and torch.equal(op_raw, g._opacity)
    assert torch.equal(fs.feat, feat) and float(feat.abs().max()) > 0
    for got, want, name in ((fs.sc, torch.exp(sc_raw), "scales"), (fs.rot, torch.nn.functional.normalize(rot_raw), "rotations"),
                            (fs.op, torch.sigmoid(op_raw), "opacity")):
        err = float(((got - want).abs() / want.abs().clamp_min(1.0)).max())
        print(name, "largest difference relative to max(1, |value|): %.2e" % err)
        assert got.shape == want.shape and err <= 1e-6, (name, err)


# ---------------------------------------------------------------------------------------------------------------- 3
def test_one_fused_iteration_against_the_cpu_oracle():
    """tests/test_hexplane16_gpu.py::test_one_iteration_and_a_no_grad_render_of_a_16_channel_model with fused=True on the GPU side:
    the tolerances of tests/test_whole_step_gpu.py::_against_the_oracle at its "tiny" size."""
    from test_hexplane16_gpu import _one_step16
    ref_loss, ref_g, ref_s, _ = _one_step16("cpu")
    scene, g, trainer = _trainer(True)
    loss = float(trainer.step(5001, cams=[trainer.cams[1]]))
    trainer.drain()
    torch.cuda.synchronize()
    t = _tensors(g)
    grads = {k: g.optimizer.state[t[k]]["exp_avg"].detach().float().cpu().numpy() * 10.0 for k in LIVE}
    stats = {"accum": g.xyz_gradient_accum.detach().cpu().numpy(), "denom": g.denom.detach().cpu().numpy(),
             "maxr": g.max_radii2D.detach().cpu().numpy()}
    print("loss", loss, "oracle", ref_loss)
    figures = {}
    for k in LIVE:
        a, b = grads[k], ref_g[k]
        assert a.shape == b.shape and float(np.abs(b).max()) > 0, k
        err = np.abs(a - b) / max(float(np.abs(b).max()), 1e-30)
        figures[k] = (float((err > 1e-4).mean()), int((err > 2e-3).sum()), float(err.max()))
        print(k, "fraction beyond 1e-4: %.2e, elements beyond 2e-3: %d, max %.2e" % figures[k])
    acc_scale = max(float(np.abs(ref_s["accum"]).max()), 1e-30)
    e = np.abs(stats["accum"] - ref_s["accum"]) / acc_scale
    print("accum: fraction beyond 1e-4: %.2e, max %.2e" % (float((e > 1e-4).mean()), float(e.max())))
    assert abs(loss - ref_loss) <= 2e-6 * max(1.0, abs(ref_loss)), (loss, ref_loss)
    np.testing.assert_array_equal(stats["denom"], ref_s["denom"])
    dr = np.abs(stats["maxr"] - ref_s["maxr"])
    assert int((dr != 0).sum()) == 0, (int((dr != 0).sum()), float(dr.max()))
    for k, (frac_loose, n_far, worst) in figures.items():
        assert frac_loose <= 1e-3 and n_far == 0 and worst <= 5e-3, (k, frac_loose, n_far, worst)
    assert float((e > 1e-4).mean()) <= 1e-3 and float(e.max()) <= 2e-3, float(e.max())


# ---------------------------------------------------------------------------------------------------------------- 4
@pytest.mark.parametrize("P,box", [(97, True), (6001, False)])
def test_tail_shapes(P, box):
    """Neither 97 nor 6001 is a multiple of the field kernel's 32-Gaussian tile or of the backward's four-unit group; 97 leaves a
    last tile of one Gaussian.  The 97 sit in the asymmetric box of tests/hexplane_box_cases.py with one of them exactly on the z min
    face, where a contracted coordinate would clip and lose its position gradient."""
    pa, pf, _ = _one_step_agrees(0.0, P=P, box=box, what="P %d" % P)
    assert pa["xyz"].shape[0] == P
    if box:
        assert float(pa["denom"][P // 2]) == 1.0           # the Gaussian on the min face was seen


# ---------------------------------------------------------------------------------------------------------------- 5
def test_a_camera_batch_of_two():
    """opt.batch_size = 2, cameras of different timestamps, under the fine-stage tolerances of
    tests/test_batch_step_gpu.py::test_fused_batch_step_matches_the_autograd_path: one step (xyz_gradient_accum within the gradient
    tolerance too), then three."""
    scene, g, trainer = _trainer(False, B=2)
    cams = _cam_lists(trainer, 0, 2, False)
    assert cams[0] is not cams[1] and float(cams[0].time) != float(cams[1].time)
    pa, pf, acc = _one_step_agrees(0.0, B=2, what="B 2")
    assert acc <= 5e-5, "xyz_gradient_accum"
    _three_steps_agree(0.0, B=2)
    la, pa3, _, _ = _run(False, 3, 0.0, 2)
    lf, pf3, _, _ = _run(True, 3, 0.0, 2)
    scale = max(1e-30, float(np.abs(pa3["accum"]).max()))
    assert float(np.abs(pf3["accum"] - pa3["accum"]).max()) <= 5e-5 * scale, "xyz_gradient_accum"


# ---------------------------------------------------------------------------------------------------------------- 6
def test_a_prune_between_two_steps_reslices_the_buffers():
    """Step, prune about a tenth of the Gaussians with a fixed mask through the model's own prune_points (the same on both paths),
    step again: the second step's first moments of the six Gaussian parameters -- the ones whose Adam state the prune re-indexed --
    agree as in test 1, and the fused step's per-Gaussian storage was re-sliced, not re-made."""
    out = {}
    for fused in (False, True):
        scene, g, trainer = _trainer(fused)
        trainer.step(5001, cams=[trainer.cams[1]])
        trainer.drain()
        P = g._xyz.shape[0]
        if fused:
            fs = trainer.fused
            cap, store = fs._rows_cap, {k: v.data_ptr() for k, v in fs._store.items() if torch.is_tensor(v)}
            assert cap == P
        mask = torch.zeros(P, dtype=torch.bool, device="cuda")
        mask[3::10] = True
        g.prune_points(mask)
        assert g._xyz.shape[0] == P - int(mask.sum()) == 5400
        trainer.step(5002, cams=[trainer.cams[4]])
        trainer.drain()
        torch.cuda.synchronize()
        if fused:
            assert fs._rows_cap == cap and fs.P == 5400 and tuple(fs.feat.shape) == (5400, 32)
            assert {k: v.data_ptr() for k, v in fs._store.items() if torch.is_tensor(v)} == store
        t = _tensors(g)
        out[fused] = ({k: g.optimizer.state[t[k]]["exp_avg"].detach().float().cpu().numpy().copy() for k in LIVE},
                      g.denom.detach().cpu().numpy().copy(), g.max_radii2D.detach().cpu().numpy().copy())
    worst = {k: float(np.abs(out[True][0][k] - out[False][0][k]).max()) / max(1e-30, float(np.abs(out[False][0][k]).max())) for k in LIVE}
    print("second step's first moments, error relative to the tensor's max:", {k: "%.2e" % v for k, v in worst.items()})
    for k in GAUSSIAN:
        assert out[True][0][k].shape[0] == 5400 and worst[k] <= 5e-5, (k, worst[k])
    np.testing.assert_array_equal(out[True][1], out[False][1])
    np.testing.assert_array_equal(out[True][2], out[False][2])


# ---------------------------------------------------------------------------------------------------------------- 7
def _launch_counts(lib, fn):
    """Launches per kernel slot of csrc/profile.hip while fn() runs."""
    slots = [k for k in range(32) if lib.mom_profile_name(k)]
    for k in slots:
        N.check(lib.mom_profile_enable(k, 1), "profile")
    try:
        fn()
    finally:
        torch.cuda.synchronize()
        counts = {}
        for k in slots:
            ms, n = C.c_double(), C.c_longlong()
            N.check(lib.mom_profile_read(k, C.byref(ms), C.byref(n), 1), "profile")
            N.check(lib.mom_profile_enable(k, 0), "profile")
            counts[lib.mom_profile_name(k).decode()] = int(n.value)
    return counts


def test_refusals_launch_nothing_and_the_next_step_is_unharmed():
    FS = importlib.import_module(pkg + ".fused_step")
    T = importlib.import_module(pkg + ".train")
    lib = N.lib()
    bg = torch.zeros(3, device="cuda")
    for kw, what in ((dict(multires=(1, 2, 4), P=97), "16 x 3"), (dict(res=(64, 64, 64, 1025), P=97), "a 1025-texel plane")):
        scene, g, op, pp, hp = _model(**kw)

        def build():
            for step in (FS.FusedStep, FS.FusedStep16, FS.fine_step):
                with pytest.raises(N.MomError, match="16 channels"):
                    step(g, op, hp, bg)
            with pytest.raises(N.MomError):
                T.Trainer(scene, g, op, hp, pp, stage="fine", delta_scale=1, sync_every_step=False, fused=True)
        counts = _launch_counts(lib, build)
        assert sum(counts.values()) == 0, (what, counts)

    scene, g, trainer = _trainer(True)
    fs = trainer.fused
    assert type(fs) is FS.FusedStep16
    with pytest.raises(N.MomError):            # each class keeps to its own shape: FusedStep refuses 16 x 2 as it always did
        FS.FusedStep(g, op, hp, bg)
    import bench
    g32 = bench.build_state(CFG, torch.device("cuda"), fused=False)[1]
    with pytest.raises(N.MomError):
        FS.FusedStep16(g32, op, hp, bg)
    assert type(FS.fine_step(g32, op, hp, bg)) is FS.FusedStep

    class Stub:          # what FusedStep asks of a parallel.DistContext before it launches anything
        mode, world, rank = "camera", 2, 0

    fs.dist = Stub()

    def refused():
        with pytest.raises(N.MomError, match="16-channel fields: single GPU only"):
            fs.forward_backward(trainer.cams[1], 1)
    counts = _launch_counts(lib, refused)
    assert sum(counts.values()) == 0 and fs.P == -1, counts          # nothing launched, no buffer made
    fs.dist = None
    # the next valid step: the one-step comparison of test 1 against the shared autograd run
    loss = float(trainer.step(5001, cams=[_cam_lists(trainer, 0, 1, False)[0]]))
    trainer.drain()
    torch.cuda.synchronize()
    la, pa, ma, _ = _run(False, 1, 0.0)
    np.testing.assert_allclose([loss], la, rtol=2e-5)
    t = _tensors(g)
    for k in LIVE:
        got = g.optimizer.state[t[k]]["exp_avg"].detach().float().cpu().numpy()
        assert float(np.abs(got - ma[k]).max()) <= 5e-5 * float(np.abs(ma[k]).max()), k
    np.testing.assert_array_equal(g.denom.detach().cpu().numpy(), pa["denom"])


# ---------------------------------------------------------------------------------------------------------------- 8
def _store_bytes(fs):
    total = 0
    for v in fs._store.values():
        for t in (v if isinstance(v, tuple) else (v,)):
            if t is not None:
                total += t.numel() * t.element_size()
    return total


def test_the_32_x_2_model_allocates_what_it_allocated():
    """The row table before the step took a width: feat 64, a0 64, dfeat 64, pts 3, sc_d 3, rot_d 4, sc 3, rot 4, op 1, gcol 3,
    gcov 6 = 219 floats per Gaussian; beside them the radii and the overflow word (P + 1 ints), the early gradient bucket (59 P + 4
    floats, world 1) and the private d scales / d rotations (3 + 4 floats per Gaussian)."""
    import bench
    scene, g, trainer, op = bench.build_state(CFG, torch.device("cuda"), fused=True)
    fs = trainer.fused
    trainer.step(5001, cams=[trainer.cams[1]])
    trainer.drain()
    P = CFG["P"]
    assert type(fs).__name__ == "FusedStep" and fs.F == 64 and fs.feat.shape[1] == 64 and fs.dfeat.shape[1] == 64 and fs.a0.shape[1] == 64 and fs._rows_cap == P
    rows = 64 + 64 + 64 + 3 + 3 + 4 + 3 + 4 + 1 + 3 + 6
    assert rows == 219 == sum(cols for _, cols, _ in type(fs)._ROW_BUFFERS) and fs._ROW_BUFFERS is type(fs)._ROW_BUFFERS
    want = 4 * (rows * P + (P + 1) + (59 * P + 4) + (3 + 4) * P)
    assert want == 1144 * P + 20 == 6_864_020
    assert _store_bytes(fs) == want
    # the 16 x 2 model: the same table with feat and dfeat at 32 floats
    scene, g, trainer = _trainer(True)
    trainer.step(5001, cams=[trainer.cams[1]])
    trainer.drain()
    assert _store_bytes(trainer.fused) == want - 4 * 2 * 32 * P
