"""The scene-flow fit without a GPU: the yardstick of sceneflow_cases.py IS the reference's optimize_motion (fixture g15, written
by tools/gen_sceneflow_golden.py from the real function), motion.prepare_views and the griddata sampling reproduce what the
reference recorded, the pose recovered from a frame's transform_matrix round-trips, and the C entry points refuse every invalid
call before anything is launched."""
import ctypes as C
import importlib
import os
import re

import numpy as np
import pytest
import torch

import sceneflow_cases as sc

pkg = "iclr2025_3d-mom_amd"
N = importlib.import_module(pkg + "._native")
ops = importlib.import_module(pkg + ".ops")
motion = importlib.import_module(pkg + ".motion")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 1 << 20          # a non-null pointer value, 16-byte aligned; every call below is refused before it could be followed


def test_the_fp32_restatement_is_the_reference():
    d, case = sc.g15(), sc.g15_case()
    flow, loss, _ = case.ref(torch.float32)
    ref = d["scene_flow"]
    assert ref.shape == (3, 300) and int(d["epochs"]) == 12 and case.views.V == 6
    dist = float(np.abs(flow.numpy() - ref).max()) / sc.scale(ref)
    print("fp32 restatement against the reference's scene_flow:", dist, "of the largest magnitude", sc.scale(ref))
    assert dist <= 2e-6
    assert np.all(np.diff(loss) < 0)                       # noise targets: the loss falls every epoch


def test_prepare_views_reproduces_the_recorded_valid_sets_and_pixels():
    d, case = sc.g15(), sc.g15_case()
    assert min(len(v) for v in case.views.valid) < 300
    for j in range(6):
        assert np.array_equal(case.views.valid[j], d[f"valid_{j}"]), j
        assert case.views.pix0[j].dtype == np.float32 and np.array_equal(case.views.pix0[j], d[f"pix0_{j}"]), j   # bit for bit
    assert case.views.R.dtype == case.views.T.dtype == np.float32 and case.views.R.shape == (6, 3, 3) and case.views.T.shape == (6, 3)


def test_a_view_without_a_valid_point_is_refused():
    pts = np.array([[0.0], [0.0], [-1.0]], np.float32)                       # behind the camera
    with pytest.raises(ValueError, match="view 0 sees none"):
        motion.prepare_views(pts, sc.intrinsics(8, 8), [(np.eye(3), np.zeros(3))], 8, 8)


def test_the_mirror_samples_the_recorded_targets():
    pytest.importorskip("scipy")
    d, case = sc.g15(), sc.g15_case()
    H, W = int(d["H"]), int(d["W"])
    pts, K = d["points"], d["K"]
    k = 0
    for Ri in d["render_poses"]:
        for Rj in d["internal_poses"]:
            R, T = Rj[:3, :3] @ Ri[:3, :3], Rj[:3, :3] @ Ri[:3, 3:4] + Rj[:3, 3:4]
            pix = np.matmul(K, R.dot(pts) + T)
            idx = case.views.valid[k]
            got = motion.sample_flow_image(torch.from_numpy(d["t2c_flow"][k]), pix[:2, idx] / pix[-1:, idx], H, W)
            assert got.dtype == np.float64 and np.array_equal(got, d[f"gt_{k}"]), k
            k += 1


def test_optimize_motion_host_side_with_the_restatement_in_the_kernels_place(monkeypatch):
    """Everything of motion.optimize_motion except the launch -- pose composition, sampling, the divisor, our_flow -- against the
    reference's results: the float32 restatement stands in for fit_scene_flow (the GPU suite runs the same check on the kernel)."""
    pytest.importorskip("scipy")
    d = sc.g15()
    seen = {}

    def stand_in(points, K, views, gt, epochs=200, lr=0.5, gamma=0.97, divisor=None, device=None):
        seen["divisor"], seen["epochs"] = divisor, epochs
        flow, loss, last = sc.restate(points, K, views.R, views.T, views.valid, views.pix0, [np.asarray(g, np.float32) for g in gt],
                                      epochs, divisor, torch.float32, lr, gamma)
        flow2d = torch.zeros(views.V, views.P, 2)
        for j, idx in enumerate(views.valid):
            flow2d[j, idx] = last[j].T
        return flow, torch.from_numpy(loss), flow2d
    monkeypatch.setattr(motion, "fit_scene_flow", stand_in)
    train_data, flow = motion.optimize_motion(sc.g15_train_data(), d["render_poses"], d["internal_poses"], d["K"], int(d["H"]),
                                              int(d["W"]), [], int(d["epochs"]))
    assert seen == {"divisor": 6, "epochs": 12}
    print("scene_flow, our_flow against the reference:", sc.check_g15_mirror(train_data, flow.numpy()))


def test_pose_from_transform_matrix_round_trips():
    for R, T in sc.poses(5, seed=3):
        m = motion.transform_matrix_from_pose(R, T)
        assert m.shape == (4, 4) and np.array_equal(m[3], [0, 0, 0, 1])
        R2, T2 = motion.pose_from_transform_matrix(m.tolist())
        np.testing.assert_allclose(R2, R, rtol=0, atol=1e-15)
        np.testing.assert_allclose(T2, T, rtol=0, atol=1e-15)
        # the same convention as the stage-2 reader's: its (R transposed, T) of this matrix is this pose
        readers = importlib.import_module(pkg + ".scene.dataset_readers")
        Rt, Tr = readers._pose_from_c2w(m.tolist())
        np.testing.assert_allclose(Rt.T, R, atol=1e-12)
        np.testing.assert_allclose(Tr.reshape(3, 1), T, atol=1e-12)


def test_learning_rates_and_weights_are_the_schedulers_and_autograds():
    p = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.SGD([p], lr=0.5)
    sched = torch.optim.lr_scheduler.ExponentialLR(opt, gamma=0.97)
    want = []
    for _ in range(200):
        want.append(opt.param_groups[0]["lr"])
        opt.step()
        sched.step()
    assert np.array_equal(motion.learning_rates(200), np.asarray(want, np.float32))
    case = sc.g15_case()
    w = motion.view_weights(case.views, 6)
    assert w.dtype == np.float32
    for j in range(6):
        y = torch.ones(2, len(case.views.valid[j]), requires_grad=True)
        (y.mean() / 6).backward()
        assert float(y.grad[0, 0]) == float(w[j]), j


def test_pack_views_records_and_bits():
    case = sc.one_epoch_case(65, 33)
    rec, bits = motion.pack_views(case.views, case.gt)
    assert rec.shape == (33, 65, 4) and rec.dtype == np.float32 and bits.shape == (2, 65) and bits.dtype == np.int32
    for j in (0, 31, 32):
        idx = case.views.valid[j]
        on = (bits.view(np.uint32)[j // 32] >> np.uint32(j % 32)) & 1
        assert np.array_equal(np.nonzero(on)[0], idx)
        assert np.array_equal(rec[j, idx, :2], case.views.pix0[j].T) and np.array_equal(rec[j, idx, 2:], case.gt[j].T)
    assert not (bits.view(np.uint32)[1] >> np.uint32(1)).any()               # no bit beyond view 32


# ------------------------------------------------------------------------------------------------ the C ABI
def test_the_symbols_exist_and_are_bound():
    lib = N.lib()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mom4d.h")).read(), flags=re.S)
    for name in ("mom_sceneflow_fit_scratch_bytes", "mom_sceneflow_fit"):
        assert hasattr(lib, name) and name in N.EXPORTS and re.search(rf"\b{name}\s*\(", header), name
    assert N.ABI_VERSION == 8 == lib.mom_abi_version()              # additive
    assert lib.mom_sceneflow_fit.argtypes is not None and len(lib.mom_sceneflow_fit.argtypes) == 17
    assert lib.mom_sceneflow_fit_scratch_bytes.restype is C.c_size_t


def test_sizing_needs_no_gpu():
    lib = N.lib()
    assert lib.mom_sceneflow_fit_scratch_bytes(0, 6, 12) > 0 and lib.mom_sceneflow_fit_scratch_bytes(300, 6, 0) > 0
    # a double per wave and epoch
    assert lib.mom_sceneflow_fit_scratch_bytes(300, 6, 12) >= 12 * 8 * 8
    assert lib.mom_sceneflow_fit_scratch_bytes(262144, 70, 200) >= 200 * 4096 * 8
    assert lib.mom_sceneflow_fit_scratch_bytes(262144, 70, 200) == lib.mom_sceneflow_fit_scratch_bytes(262144, 1, 200)


def _fit(lib, P=10, V=2, E=3, K=None, hole=None, scratch_bytes=None, **over):
    k9 = (C.c_float * 9)(*(K if K is not None else [30, 0, 12, 0, 30, 12, 0, 0, 1]))
    names = ["points", "K", "R", "T", "w", "records", "valid", "lr", "flow", "loss", "flow2d_last", "scratch"]
    a = {n: FAKE for n in names}
    a["K"] = k9
    a.update(over)
    if hole is not None:
        a[hole] = None
    need = lib.mom_sceneflow_fit_scratch_bytes(P, V, E)
    return lib.mom_sceneflow_fit(P, V, E, a["points"], a["K"], a["R"], a["T"], a["w"], a["records"], a["valid"], a["lr"], a["flow"],
                                 a["loss"], a["flow2d_last"], a["scratch"], need if scratch_bytes is None else scratch_bytes, None)


def test_every_invalid_call_is_refused_before_anything_is_launched():
    lib = N.lib()
    assert _fit(lib, P=0) == N.MOM_OK                                          # nothing to do, nothing launched
    assert lib.mom_sceneflow_fit(0, 1, 5, None, None, None, None, None, None, None, None, None, None, None, None, 0, None) == N.MOM_OK
    assert _fit(lib, E=0) == N.MOM_OK                                          # no epoch: the flow stays what it is
    assert _fit(lib, P=-1) == N.MOM_EINVAL
    for V in (0, -1):
        assert _fit(lib, V=V) == N.MOM_EINVAL
        assert _fit(lib, P=0, V=V) == N.MOM_EINVAL
    assert _fit(lib, E=-1) == N.MOM_EINVAL
    for hole in ("points", "K", "R", "T", "w", "records", "valid", "lr", "flow"):
        assert _fit(lib, hole=hole) == N.MOM_EINVAL, hole
    assert _fit(lib, hole="scratch") == N.MOM_EINVAL                           # a loss needs the scratch ...
    need = lib.mom_sceneflow_fit_scratch_bytes(10, 2, 3)
    for short in (0, need - 1):
        assert _fit(lib, scratch_bytes=short) == N.MOM_EINVAL, short           # ... all of it
    assert _fit(lib, records=FAKE + 4) == N.MOM_EINVAL                         # 16-byte records
    assert _fit(lib, flow2d_last=FAKE + 4) == N.MOM_EINVAL
    for bad in ([30, 0.5, 12, 0, 30, 12, 0, 0, 1], [30, 0, 12, 0, 30, 12, 0, 0, 2], [30, 0, 12, 0, 30, 12, 0.1, 0, 1]):
        assert _fit(lib, K=bad) == N.MOM_EINVAL, bad                           # not [[fx,0,cx],[0,fy,cy],[0,0,1]]


def test_the_op_refuses_cpu_tensors_and_wrong_shapes():
    case = sc.one_epoch_case(63, 6)
    v = case.views
    rec, bits = motion.pack_views(v, case.gt)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    args = [t(case.points), case.K, t(v.R), t(v.T), t(motion.view_weights(v, 6)), t(rec), t(bits), t(motion.learning_rates(1)),
            torch.zeros(3, 63)]
    with pytest.raises(N.MomError, match="no CPU path"):
        ops.sceneflow_fit(*args)
    with pytest.raises(N.MomError, match="no CPU path"):
        motion.fit_scene_flow(case.points, case.K, v, case.gt, epochs=1, device="cpu")
    with pytest.raises(ValueError, match="targets for"):
        motion.pack_views(v, case.gt[:-1])
    with pytest.raises(ValueError, match="one column per valid point"):
        motion.pack_views(v, [g[:, :-1] for g in case.gt])


def test_refit_refuses_a_directory_without_flow_images(tmp_path):
    S = importlib.import_module(pkg + ".scene")
    stage1 = importlib.import_module(pkg + ".scene.stage1")
    stage1.write_stage1_outputs(str(tmp_path), S.SyntheticScene(60, 3, 24, 16, seed=11))
    with pytest.raises(ValueError, match="no frame carries a T2C_flow"):
        motion.refit_scene_flow(str(tmp_path))


def test_stage1_intrinsics_are_the_readers():
    readers = importlib.import_module(pkg + ".scene.dataset_readers")
    K = motion.stage1_intrinsics(32, 48)
    assert K.dtype == np.float32 and K[0, 0] == np.float32(readers.FOCAL * 1.5) and K[1, 1] == np.float32(readers.FOCAL)
    assert (K[0, 2], K[1, 2], K[2, 2]) == (24.0, 16.0, 1.0)
