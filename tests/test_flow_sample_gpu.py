"""Sampling the views' 2D flow images on the GPU (csrc/flow_sample.hip through ops.flow_sample and motion.sample_flow_images) against
the float64 restatement of flow_sample_cases.py -- which test_flow_sample_cpu.py holds to scipy's griddata -- and against what the
reference run recorded (fixture g15).  The cell diagonals come from fixture g17, so only the end-to-end tests, whose our_flow
resampling is scipy's, need scipy.

Bound on a sampled value: one float32 ulp of the cell's largest corner magnitude, 2^-23 max|f| (flow_sample_cases.check_records has
the reasoning); the unflowed pixels and the zero records of invalid pairs are compared bit for bit."""
import importlib
import os

import numpy as np
import pytest
import torch

import flow_sample_cases as fc
import sceneflow_cases as sc

pytestmark = pytest.mark.gpu
pkg = "iclr2025_3d-mom_amd"
N = importlib.import_module(pkg + "._native")
ops = importlib.import_module(pkg + ".ops")
motion = importlib.import_module(pkg + ".motion")
SENTINEL = 7.5
up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run(case, mask, pix=None, bits=None, channel_last=False):
    """ops.flow_sample on a case, into records pre-filled with a sentinel: every slot must be written."""
    images = case.images.transpose(0, 2, 3, 1) if channel_last else case.images
    rec = torch.full((case.V, case.P, 4), SENTINEL, device="cuda")
    out = ops.flow_sample(up(images), up(case.pix if pix is None else pix), up(case.bits if bits is None else bits),
                          up(motion.pack_diagonals(mask)), rec)
    assert out is rec
    return rec.cpu().numpy()


@pytest.mark.parametrize("P,V", fc.SHAPES)
@pytest.mark.parametrize("H,W", fc.SIZES)
def test_the_kernel_against_the_restatement(H, W, P, V):
    """Under scipy's diagonals, under their complement and under main diagonals only: a kernel that ignored or transposed the bitmap
    cannot pass all three.  The channel-last layout is taken as it is (where the shape can say which one it is)."""
    case = fc.kernel_case(H, W, P, V)
    assert all(len(idx) for idx in case.views.valid)
    for which, mask in fc.mask_variants(H, W).items():
        rec = run(case, mask, channel_last=(which == "flipped" and H != 2))
        fc.check_records(rec, case, case.expected(which), name=f"{H} x {W}, P {P}, V {V}, {which}")


@pytest.mark.parametrize("H,W,P,V", [(2, 2, 65, 33), (37, 53, 300, 6)])
def test_invalid_pairs_write_zeros_and_reach_nothing(H, W, P, V):
    """About a third of the validity bits cleared, their pixel slots filled with NaN, 1e300 and -5, like every slot that never was
    valid: those records are exactly zero, all others as before."""
    case = fc.kernel_case(H, W, P, V)
    rng = np.random.default_rng(H + P)
    pix, bits = case.pix.copy(), case.bits.view(np.uint32).copy()
    junk = np.array([np.nan, 1e300, -5.0])
    on = np.zeros((V, P), bool)
    for j, idx in enumerate(case.views.valid):
        on[j, idx] = True
    keep = on & (rng.random((V, P)) >= 1.0 / 3.0)
    assert 0 < keep.sum() < on.sum()
    pix[~keep] = junk[rng.integers(0, 3, ((~keep).sum(), 2))]
    for j in range(V):
        bits[j // 32] &= ~(np.uint32(1 << (j % 32)) * (~keep[j]).astype(np.uint32))
    valid = [np.nonzero(keep[j])[0] for j in range(V)]
    expected = [tuple(a[keep[j, idx]] for a in case.expected("g17")[j]) for j, idx in enumerate(case.views.valid)]
    rec = run(case, fc.mask_variants(H, W)["g17"], pix=pix, bits=bits.view(np.int32))
    fc.check_records(rec, case, expected, valid=valid, name=f"{H} x {W}, P {P}, V {V}, {int((~keep & on).sum())} bits cleared")


def test_sample_flow_images_gives_the_recorded_g15_records():
    """motion.sample_flow_images on g15's views and flow images against what the reference's griddata calls returned."""
    d, case = sc.g15(), sc.g15_case()
    v = case.views
    rec, bits = motion.sample_flow_images(v, [torch.from_numpy(f) for f in d["t2c_flow"]], diagonals=fc.g17()[0][(24, 24)])
    assert rec.is_cuda and tuple(rec.shape) == (6, 300, 4) and bits.dtype == torch.int32
    rec = rec.cpu().numpy()
    want_rec, want_bits = motion.pack_views(v, case.gt)
    assert np.array_equal(bits.cpu().numpy(), want_bits)
    equal = total = 0
    for j, idx in enumerate(v.valid):
        assert np.array_equal(rec[j, idx, :2].view(np.uint32), d[f"pix0_{j}"].T.view(np.uint32)), j
        _, cmax = fc.restate(d["t2c_flow"][j][0], v.pix64[j].T, fc.g17()[0][(24, 24)], corners=True)
        want = d[f"gt_{j}"].T.astype(np.float32)
        assert (np.abs(rec[j, idx, 2:].astype(np.float64) - want) <= 2.0 ** -23 * cmax).all(), j
        equal += int((rec[j, idx, 2:].view(np.uint32) == want.view(np.uint32)).sum())
        total += want.size
    print(f"g15: gt bit-equal to float32 of the reference's recorded targets in {equal} of {total} elements")
    assert np.array_equal(rec == 0, want_rec == 0)                            # zeros exactly where pack_views has them


def test_two_samplings_and_fits_are_enqueued_without_a_host_synchronisation():
    """sample_flow_images and fit_scene_flow only enqueue: under torch's synchronisation guard two sample-and-fit pairs go onto the
    stream back to back, and both give what they give one at a time."""
    cases = [fc.kernel_case(24, 24, 300, 6), fc.kernel_case(37, 53, 257, 6)]

    def pair(c):
        rec, bits = motion.sample_flow_images(c.views, torch.from_numpy(c.images), diagonals=fc.g17()[0][(c.H, c.W)])
        return (rec,) + motion.fit_scene_flow(c.points, sc.intrinsics(c.H, c.W), c.views, None, epochs=12, records=(rec, bits))
    pair(cases[0])                                                            # code objects loaded, allocator warm
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        together = [pair(c) for c in cases]
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    for c, first in zip(cases, together):
        alone = pair(c)
        torch.cuda.synchronize()
        for x, y in zip(first, alone):
            assert torch.isfinite(x).all() and torch.equal(x, y)
        assert float(first[2][0]) > float(first[2][-1]) > 0                  # the loss falls


# ------------------------------------------------------------------------------------------------ end to end
def test_optimize_motion_with_the_device_sampler_reproduces_the_reference_run():
    pytest.importorskip("scipy")
    d = sc.g15()
    train_data, flow = motion.optimize_motion(sc.g15_train_data(), d["render_poses"], d["internal_poses"], d["K"], int(d["H"]),
                                              int(d["W"]), [], int(d["epochs"]), sampler="device")
    assert flow.is_cuda and tuple(flow.shape) == (3, 300)
    print("sampler=device: scene_flow, our_flow against the reference:", sc.check_g15_mirror(train_data, flow.cpu().numpy()))


def test_refit_scene_flow_with_the_device_sampler(tmp_path):
    """The same directory fitted with both samplers.  The flow images are sceneflow_cases' tie-free magnitudes 0.5 + |n| px under one
    sign per image and channel, so no sampled target is anywhere near 0 (a sign descent cannot be compared point
    by point where a target is)."""
    pytest.importorskip("scipy")
    S = importlib.import_module(pkg + ".scene")
    stage1 = importlib.import_module(pkg + ".scene.stage1")
    H, W, P = 32, 48, 600
    path = stage1.write_stage1_outputs(str(tmp_path), S.SyntheticScene(P, 60, W, H, seed=11))
    data = torch.load(path, weights_only=False)
    for k, fr in enumerate(data["frames"]):
        if k != 3:                                                     # frame 3 stays a view without a flow; frame 4 is the last slot
            mag = np.abs(sc._tiefree(17)(k, np.arange(H * W), None)).reshape(1, 2, H, W)
            sign = np.where(np.random.default_rng(k).random((1, 2, 1, 1)) < 0.5, -1.0, 1.0)
            fr["T2C_flow"].append(torch.from_numpy((mag * sign).astype(np.float32)))
    torch.save(data, path)
    out = os.path.join(str(tmp_path), "MOM", "scene_flow.pth")
    host = motion.refit_scene_flow(str(tmp_path), train_iteration=12, sampler="griddata")
    assert torch.equal(torch.load(out), host)
    dev = motion.refit_scene_flow(str(tmp_path), train_iteration=12, sampler="device")
    written = torch.load(out)
    assert written.dtype == torch.float32 and tuple(written.shape) == (3, P) and not written.is_cuda and torch.equal(written, dev)
    s = float(host.abs().max())
    dist = float((dev - host).abs().max()) / s
    print(f"refit, sampler=device against sampler=griddata: {dist:.3g} of the largest magnitude {s:.3g}; "
          f"{int((dev == host).all(0).sum())} of {P} points bit-equal")
    assert torch.isfinite(dev).all() and s > 0 and dist <= 2e-6
