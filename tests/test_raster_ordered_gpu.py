"""The ordered backward reduction on the GPU (include/mom4d.h, "ordered backward reduction"): its gradients are a function of their
inputs bit for bit, its slots and its order are the documented ones, the gradients are still the right ones, and the switch carries
it through autograd and through the coarse stage's training iteration.  Nothing here asserts that the atomic path differs."""
import importlib
import random

import numpy as np
import pytest
import torch

import raster_ordered_cases as oc
from oracle import raster_oracle as ro
from raster_compare import GRAD_NAMES, GRAD_REL_TOL, ROW_TOL, _cmp_grads, _relerr

pytestmark = pytest.mark.gpu


def _oracle(s):
    ro.set_threads(1)
    return ro.forward(s["means3D"], s["opacities"], s["viewmatrix"], s["projmatrix"], s["campos"], s["W"], s["H"], s["tanfovx"],
                      s["tanfovy"], s["bg"], shs=s["shs"], sh_degree=3, scales=s["scales"], rotations=s["rotations"])


def _same_bits(a, b, what):
    for k in GRAD_NAMES + ("gacc", "partials", "slot_base"):
        assert np.array_equal(oc.bits(a[k]) if a[k].dtype == np.float32 else a[k], oc.bits(b[k]) if b[k].dtype == np.float32 else b[k]), (what, k)


def _within_unordered_gate(g, ref, what):
    """tests/test_raster_gpu.py's comparison of two backwards that differ by the order of their additions only."""
    for k in GRAD_NAMES:
        scale = max(float(np.abs(ref[k]).max()), 1e-30)
        assert np.abs(g[k] - ref[k]).max() <= ROW_TOL * scale, (what, k, float(np.abs(g[k] - ref[k]).max()), scale)


@pytest.fixture(scope="module")
def frames():
    """Per case: the scene, one forward under each binning, the oracle's state, the image gradients and one ordered backward of each
    forward -- computed once, shared, never modified."""
    from hip_helpers import hip_forward
    out = {}
    for name, make in oc.CASES.items():
        s = make()
        dcol, ddep = oc.image_grads(s, seed=ord(name))
        fw, fw_all = hip_forward(s), hip_forward(s, keep_all_tiles=True)
        out[name] = dict(s=s, dcol=dcol, ddep=ddep, fw=fw, fw_all=fw_all, st=_oracle(s),
                         g=oc.ordered_backward(fw, dcol, ddep), g_all=oc.ordered_backward(fw_all, dcol, ddep))
    return out


def test_the_cases_hold_what_they_are_for(frames):
    a, b, c = frames["A"], frames["B"], frames["C"]
    s, fw = a["s"], a["fw"]
    x0, y0, x1, y1 = oc.rects(fw["means2D"], fw["radii"], s["W"], s["H"])
    cnt = (x1 - x0) * (y1 - y0)
    assert (s["W"], s["H"]) == (40, 24) and cnt[20] == 6                                   # the whole 3 x 2 grid
    behind = s["means3D"][:, 2] <= 0.2
    assert behind.any() and (fw["radii"][behind] == 0).all()                               # behind the camera (or its near plane)
    assert ((fw["radii"] == 0) & ~behind).any()                                            # in front of it, off screen
    assert a["fw"]["R"] < a["fw_all"]["R"]                                                 # the default binning culled instances
    assert int(b["fw"]["ranges"][0][1] - b["fw"]["ranges"][0][0]) > 512                    # more than one staging round in tile 0
    assert (b["fw"]["ranges"][1:, 1] == b["fw"]["ranges"][1:, 0]).all()
    assert (c["fw"]["ranges"][:, 1] > c["fw"]["ranges"][:, 0]).all()                       # every tile holds splats


@pytest.mark.parametrize("case", ["A", "B", "C"])
def test_the_gradients_are_a_function_of_their_inputs(frames, case):
    from hip_helpers import hip_forward
    f = frames[case]
    first = f["g"]
    assert first["status"] == 0 and f["g_all"]["status"] == 0
    for fill in (0xFF, 0x3C):                         # fresh outputs; the partials arrive dirty and the call clears them
        again = oc.ordered_backward(f["fw"], f["dcol"], f["ddep"], fresh_fill=fill)
        assert again["status"] == 0
        _same_bits(again, first, (case, "repeat", fill))
    fw2 = hip_forward(f["s"])                         # a fresh forward into new scratch
    g2 = oc.ordered_backward(fw2, f["dcol"], f["ddep"])
    assert g2["status"] == 0
    _same_bits(g2, first, (case, "fresh forward"))
    # keep_all_tiles: other lists, other positions in them, the same per-entry terms (MomRasterArgs.keep_all_tiles) -- and, the slots
    # being the rectangle's, the same partials in the same places
    _same_bits(f["g_all"], first, (case, "keep_all_tiles"))


@pytest.mark.parametrize("depth", [True, False])
def test_with_and_without_a_depth_gradient(frames, depth):
    f = frames["A"]
    ddep = f["ddep"] if depth else None
    g1 = oc.ordered_backward(f["fw"], f["dcol"], ddep, fresh_fill=0xFF)
    g2 = oc.ordered_backward(f["fw_all"], f["dcol"], ddep)
    assert g1["status"] == 0 == g2["status"]
    _same_bits(g1, g2, ("A", depth))
    if depth:
        _same_bits(g1, f["g"], ("A", "shared"))
        assert g1["partials"][:, :, 9].any()
    else:
        assert not g1["partials"][:, :, 9].any() and not g1["gacc"][:, 9].any()       # the depth value stays +0.0
        _cmp_grads({k: g1[k] for k in GRAD_NAMES}, ro.backward(f["st"], f["dcol"]), f["st"])


@pytest.mark.parametrize("case", ["A", "B", "C"])
def test_the_slots_and_the_order_are_the_documented_ones(frames, case):
    from hip_helpers import N
    f = frames[case]
    s, fw, fw_all, st, g = f["s"], f["fw"], f["fw_all"], f["st"], f["g"]
    P = s["means3D"].shape[0]
    sb = g["slot_base"]
    np.testing.assert_array_equal(np.diff(sb.astype(np.int64)), st.tiles_touched.astype(np.int64))
    assert int(sb[P]) == int(st.num_rendered) == g["slots"] == fw_all["R"]
    # every slot of an instance the default binning culled (in the reference's lists, not in ours) holds +0.0 in all four waves
    W, H = s["W"], s["H"]
    gx = (W + 15) // 16
    x0, y0, x1, y1 = oc.rects(fw["means2D"], fw["radii"], W, H)
    np.testing.assert_array_equal((x1 - x0) * (y1 - y0), st.tiles_touched.astype(np.int64))      # (the helper's own rectangles)
    culled = oc.instances(fw_all, W) - oc.instances(fw, W)
    assert not (oc.instances(fw, W) - oc.instances(fw_all, W))
    if case == "A":
        assert len(culled) >= 10
    zero = np.zeros((oc.WAVES, oc.VALUES), np.uint32)
    for gi, tile in culled:
        tx, ty = tile % gx, tile // gx
        slot = int(sb[gi]) + (ty - int(y0[gi])) * int(x1[gi] - x0[gi]) + (tx - int(x0[gi]))
        assert int(sb[gi]) <= slot < int(sb[gi + 1])
        assert np.array_equal(oc.bits(g["partials"][slot]), zero), (gi, tile)
    # ... and an instance that is in our lists and carries a gradient wrote its own slot (the closed form addresses the right one)
    kept = sorted(oc.instances(fw, W))
    hit = 0
    for gi, tile in kept:
        tx, ty = tile % gx, tile // gx
        slot = int(sb[gi]) + (ty - int(y0[gi])) * int(x1[gi] - x0[gi]) + (tx - int(x0[gi]))
        hit += bool(g["partials"][slot].any())
    written = int(g["partials"].reshape(g["slots"], -1).any(axis=1).sum())
    assert hit == written > 0                               # no slot outside the kept instances was written
    # the record is the documented sum of the partials: the library's host twin and the numpy restatement, bit for bit
    host = np.full((P, N.GACC_FLOATS), 7.0, np.float32)
    p = np.ascontiguousarray(g["partials"])
    assert N.lib().mom_raster_ordered_sum_host(P, sb.ctypes.data, p.ctypes.data, host.ctypes.data) == N.MOM_OK
    np.testing.assert_array_equal(oc.bits(g["gacc"]), oc.bits(host))
    np.testing.assert_array_equal(oc.bits(g["gacc"]), oc.bits(oc.record_numpy(sb, p, N.GACC_FLOATS)))
    assert not g["gacc"][fw["radii"] == 0].any()


def test_a_slot_count_that_is_too_small_costs_status_bits_never_a_store_out_of_bounds(frames):
    """The backward is told of half the plan's slots, with a buffer sized for that half: every entry whose slot lies at or beyond
    the claim is skipped and reported, the reduction cuts the ranges that leave the buffer and reports that, and the bytes behind the
    claimed slots keep what they held.  Slots below the claim hold what a complete run puts there."""
    from hip_helpers import N
    f = frames["C"]
    full = f["g"]
    half = full["slots"] // 2
    g = oc.ordered_backward(f["fw"], f["dcol"], f["ddep"], claim=half)
    assert g["status"] == N.ORDERED_BAD_SLOT | N.ORDERED_CUT
    assert len(g["tail"]) >= 4096 and (g["tail"] == 0x5A).all()
    assert np.array_equal(oc.bits(g["partials"]), oc.bits(full["partials"][:half]))
    whole = np.nonzero(full["slot_base"][1:] <= half)[0]                 # Gaussians whose slots all lie below the claim
    assert len(whole) > 10
    assert np.array_equal(oc.bits(g["gacc"][whole]), oc.bits(full["gacc"][whole]))


@pytest.mark.parametrize("case", ["A", "B", "C", "config1"])
def test_still_the_right_gradients(frames, case):
    from hip_helpers import hip_backward, hip_forward
    if case == "config1":
        s = oc.case_config1()
        dcol, ddep = oc.image_grads(s, seed=12)
        fw, st = hip_forward(s), _oracle(s)
        g = oc.ordered_backward(fw, dcol, ddep)
        assert g["status"] == 0 and g["slots"] == int(st.num_rendered)
    else:
        f = frames[case]
        s, dcol, ddep, fw, st, g = f["s"], f["dcol"], f["ddep"], f["fw"], f["st"], f["g"]
    grads = {k: g[k] for k in GRAD_NAMES}
    _cmp_grads(grads, ro.backward(st, dcol, ddep), st)
    _within_unordered_gate(grads, hip_backward(fw, dcol, ddep), case)


def _autograd_pass(s, weights):
    from hip_helpers import DGR, t
    W, H = s["W"], s["H"]
    rs = DGR.GaussianRasterizationSettings(image_height=H, image_width=W, tanfovx=s["tanfovx"], tanfovy=s["tanfovy"], bg=t(s["bg"]),
                                           scale_modifier=1.0, viewmatrix=t(s["viewmatrix"]), projmatrix=t(s["projmatrix"]), sh_degree=3,
                                           campos=t(s["campos"]), prefiltered=False, debug=False)
    rast = DGR.GaussianRasterizer(rs)
    leaves = dict(means3D=t(s["means3D"]).requires_grad_(True), opacities=t(s["opacities"]).requires_grad_(True),
                  shs=t(s["shs"]).requires_grad_(True), scales=t(s["scales"]).requires_grad_(True),
                  rotations=t(s["rotations"]).requires_grad_(True))
    leaves["means2D"] = torch.zeros_like(leaves["means3D"], requires_grad=True)
    img, radii, depth = rast(**leaves)
    (img * weights).sum().backward()
    torch.cuda.synchronize()
    return {k: v.grad.cpu().numpy() for k, v in leaves.items()}


def test_through_autograd_under_the_switch():
    from hip_helpers import RC
    s = oc.case_a()
    wgt = torch.linspace(0.5, 1.5, 3 * s["H"] * s["W"], device="cuda").view(3, s["H"], s["W"])
    assert RC.deterministic() is False
    had_scratch = RC._state["ordered"] is not None        # (only if a test that uses the switch ran earlier in this process: none above does)
    off = _autograd_pass(s, wgt)
    if not had_scratch:
        assert RC._state["ordered"] is None               # off: nothing of the ordered path was allocated
    RC.set_deterministic(True)
    try:
        on1, on2 = _autograd_pass(s, wgt), _autograd_pass(s, wgt)
        assert RC.ordered_status() == 0
    finally:
        RC.set_deterministic(False)
    assert RC._state["ordered"] is not None and RC._state["ordered"]["partials"] is not None
    for k in on1:
        assert np.array_equal(oc.bits(on1[k]), oc.bits(on2[k])), k
    off2 = _autograd_pass(s, wgt)                         # switched off again: the atomic path, within its gates of the ordered one
    st = _oracle(s)
    go = ro.backward(st, wgt.cpu().numpy())
    oracle_name = dict(means3D="dL_dmeans3D", means2D="dL_dmeans2D", opacities="dL_dopacity", shs="dL_dsh", scales="dL_dscales",
                       rotations="dL_drotations")
    for k, n in oracle_name.items():
        assert _relerr(on1[k], go[n]) <= GRAD_REL_TOL, k
        for other in (off, off2):
            scale = max(float(np.abs(on1[k]).max()), 1e-30)
            assert np.abs(other[k] - on1[k]).max() <= ROW_TOL * scale, k


def _coarse_run(iterations, **trainer_kw):
    pkg = "iclr2025_3d-mom_amd"
    A, S, T = (importlib.import_module(f"{pkg}.{m}") for m in ("arguments", "scene", "train"))
    args, lp, op, pp, hp = A.default_args(time_resolution=10)
    op.lambda_dssim = 0.0
    torch.manual_seed(6666)
    random.seed(6666)
    np.random.seed(6666)
    scene = S.SyntheticScene(1500, 3, 96, 64, seed=6666)
    g = S.GaussianModel(lp.sh_degree, hp, device=torch.device("cuda"))
    scene.init_gaussians(g)
    scene.make_trained_like(g)
    trainer = T.Trainer(scene, g, op, hp, pp, stage="coarse", delta_scale=1, sync_every_step=False, **trainer_kw)
    for it in range(1, iterations + 1):
        trainer.step(it)
    torch.cuda.synchronize()
    state = {}
    for group in g.optimizer.param_groups:
        for p in group["params"]:
            st = g.optimizer.state.get(p, {})
            state[group["name"]] = (p.detach().clone(), {k: v.detach().clone() for k, v in st.items() if torch.is_tensor(v)})
    return state


def test_the_coarse_stage_repeats_bit_for_bit():
    from hip_helpers import N, RC
    try:
        with pytest.raises(N.MomError, match="deterministic"):
            _coarse_run(0, fused=True, deterministic=True)
        assert RC.deterministic() is False                    # the refusal came before the switch was touched
        a = _coarse_run(6, fused=False, deterministic=True)
        assert RC.deterministic() is True and RC.ordered_status() == 0
        b = _coarse_run(6, fused=False, deterministic=True)
        assert RC.ordered_status() == 0
    finally:
        RC.set_deterministic(False)
    assert set(a) == set(b) and len(a) >= 6
    moments = 0
    for name in a:
        assert torch.equal(a[name][0], b[name][0]), name
        assert set(a[name][1]) == set(b[name][1]), name
        for k in a[name][1]:
            assert torch.equal(a[name][1][k], b[name][1][k]), (name, k)
            moments += 1
    assert moments >= 12                                      # both Adam moments of the six Gaussian parameter groups
