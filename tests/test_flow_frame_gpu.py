"""The flow step's two kernels (csrc/flow_frame.hip through ops.hint_field / ops.flow_finish) against the reference's own output on
the inputs of flow_frame_cases.py (tests/golden/g22_flow_frame.npz; the tail's half of it is the torch restatement, kornia being
absent where it was written) and against the float64 evaluation beside it.

Gates (derived in flow_frame_cases.py, not tuned): per element |kernel - reference| <= the bound of two fp32 evaluations that differ
in expf (hint field) or twice one evaluation's summation bound (tail); |kernel - float64| <= the reference's own largest distance
from float64 + the bound.  mask_s is a count divided twice, correctly
rounded: the reference's bits.  Where the bound is 0 -- masked-out pixels, an all-zero mask, weights that all underflow, windows
that see no non-zero term -- the kernel's value is exactly the reference's 0.  Two calls give the same bits.

Achieved on an MI355X (pytest -s prints them): DESIGN.md 3.20."""
import importlib

import numpy as np
import pytest
import torch

import flow_frame_cases as fc

pytestmark = pytest.mark.gpu
pkg = "iclr2025_3d-mom_amd"
ops = importlib.import_module(pkg + ".ops")
motion = importlib.import_module(pkg + ".motion")
up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)


def hint_inputs():
    frames, sigmas = fc.hint_views()
    args = [motion.hint_arguments(fr, sigma=s) for fr, s in zip(frames, sigmas)]
    n = max(len(a[0]) for a in args)
    pos, start, end = np.zeros((3, n, 2), np.int32), np.zeros((3, n, 2)), np.zeros((3, n, 2))
    for k, (p, s, e, _) in enumerate(args):
        pos[k, :len(p)], start[k, :len(p)], end[k, :len(p)] = p, s, e
    masks = np.stack([np.array(fr["mask"]) for fr in frames])
    return args, masks, (up(pos), up(start), up(end), up(np.asarray([len(a[0]) for a in args], np.int32)),
                         up(np.asarray(sigmas, np.float32)))


def share(d, bound):
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.where(d == 0, 0.0, d / bound).max())


@pytest.mark.parametrize("S", fc.SIZES)
def test_hint_field_against_the_reference(S):
    g = fc.g22("flow_frame")
    args, masks, dev = hint_inputs()
    assert [len(a[0]) for a in args] == [1, 3, 1]
    hints, mask_s = ops.hint_field(*dev, up(masks), S)
    assert hints.shape == (3, 2, S, S) and mask_s.shape == (3, 1, S, S) and hints.dtype == mask_s.dtype == torch.float32
    again = ops.hint_field(*dev, up(masks), S)
    assert torch.equal(again[0], hints) and torch.equal(again[1], mask_s)
    assert np.array_equal(bits(mask_s.cpu().numpy()), bits(g[f"mask_s_{S}"]))
    got = hints.cpu().numpy().astype(np.float64)
    assert np.isfinite(got).all()
    for v, (pos, start, end, sigma) in enumerate(args):
        f64, bound = fc.hint_eval(pos, start, end, sigma, masks[v], S)
        assert np.array_equal(f64, g[f"hints64_{S}"][v])
        d_ref, d64 = np.abs(got[v] - g[f"hints_{S}"][v]), np.abs(got[v] - f64)
        gate64 = g[f"d_ref_{S}"][v] + bound
        print(f"hint field S {S} view {v}: |kernel - reference| max {d_ref.max():.3g}, largest share of the bound {share(d_ref, bound):.3g} "
              f"(outside the subnormal band {share(d_ref, np.where(bound > 1e-3, np.inf, bound)):.3g}); |kernel - float64| max "
              f"{d64.max():.3g}, the reference's {g[f'd_ref_{S}'][v]:.3g}; exact zeros {(bound == 0).mean() * 100:.0f} %")
        assert (d_ref <= bound).all() and (d64 <= gate64).all()
        assert not got[v][bound == 0].any() and (bound == 0).sum() > S          # masked-out pixels: exactly the reference's zero


def test_hint_field_of_an_all_zero_mask_is_exactly_zero():
    args, masks, dev = hint_inputs()
    base = ops.hint_field(*dev, up(masks), 24)
    masks[1] = 0
    hints, mask_s = ops.hint_field(*dev, up(masks), 24)
    assert not hints[1].any() and not mask_s[1].any()
    for v in (0, 2):                                                           # the other views of the launch do not notice
        assert torch.equal(hints[v], base[0][v]) and torch.equal(mask_s[v], base[1][v])


def test_hint_field_refuses_what_it_cannot_index():
    N = importlib.import_module(pkg + "._native")
    args, masks, dev = hint_inputs()
    with pytest.raises(N.MomError):
        ops.hint_field(*dev, up(masks), 0)
    with pytest.raises(N.MomError):
        ops.hint_field(dev[0], dev[1].float(), *dev[2:], up(masks), 24)
    with pytest.raises(N.MomError):
        ops.hint_field(*dev, up(masks[:2]), 24)


@pytest.mark.parametrize("S", fc.FINISH_SIZES)
def test_flow_finish_against_the_restatement(S):
    g = fc.g22("flow_frame")
    pred, mask_s = fc.finish_inputs(S)
    flow = ops.flow_finish(up(pred), up(mask_s), fc.H, fc.W)
    assert flow.shape == (2, 2, fc.H, fc.W) and flow.dtype == torch.float32
    assert torch.equal(ops.flow_finish(up(pred), up(mask_s), fc.H, fc.W), flow)
    got = flow.cpu().numpy().astype(np.float64)
    f64, bound = fc.finish_eval(pred, mask_s, fc.H, fc.W)
    assert np.array_equal(f64, g[f"flow64_{S}"])
    d_ref, d64 = np.abs(got - g[f"flow_{S}"]), np.abs(got - f64)
    gate64 = g[f"flow_d_ref_{S}"] + bound
    zeros = f64 == 0
    print(f"flow tail S {S}: |kernel - restatement| max {d_ref.max():.3g}, share of twice the bound {share(d_ref, 2 * bound):.3g}; "
          f"|kernel - float64| max {d64.max():.3g}, the restatement's {float(g[f'flow_d_ref_{S}']):.3g}; exact zeros {zeros.mean() * 100:.0f} %")
    assert (d_ref <= 2 * bound).all() and (d64 <= gate64).all()
    assert not got[zeros].any() and not g[f"flow_{S}"][zeros].any() and zeros.sum() > fc.W
    if S == 9:                  # view 0: the last two rows and three columns come from row 8 / column 8 alone, which see no term
        assert zeros[0][:, -2:, :].all() and zeros[0][:, :, -3:].all() and not zeros[0][:, :30, :40].any()


def test_flow_finish_of_a_zero_mask_and_of_one_size():
    pred, mask_s = fc.finish_inputs(24)
    mask_s[1] = 0
    flow = ops.flow_finish(up(pred), up(mask_s), fc.H, fc.W)
    assert not flow[1].any() and flow[0].any()
    same = ops.flow_finish(up(pred), up(mask_s), 24, 24)                        # S -> S: the resize is the identity, the scale 1
    want = fc.finish_restated(up(pred), up(mask_s), 24, 24)
    assert same.shape == (2, 2, 24, 24) and float((same - want).abs().max()) <= 2 * 227 * fc.EPS * float(np.abs(pred).max())


def test_estimate_flows_appends_one_flow_per_frame():
    """estimate_flows on the three crafted views: without an estimator the prediction is the hint field; with one, the callable
    sees the resized images, the masks and the hints of all views at once and its output goes through the tail."""
    from PIL import Image
    frames, sigmas = fc.hint_views()
    rng = np.random.default_rng(3)
    for fr in frames:
        fr["image"] = Image.fromarray(rng.integers(0, 256, (fc.H, fc.W, 3), dtype=np.uint8))
        fr["T2C_flow"] = []
    np.random.seed(5)
    drawn = [motion.hint_arguments(fr)[3] for fr in frames]
    np.random.seed(5)
    data = motion.estimate_flows({"frames": frames}, size=24)
    seen = {}

    def estimator(rgbs, mask_s, hints):
        seen.update(rgbs=rgbs, mask_s=mask_s, hints=hints)
        return hints * 2

    np.random.seed(5)
    motion.estimate_flows(data, estimator=estimator, size=24)
    assert seen["rgbs"].shape == (3, 3, 24, 24) and seen["rgbs"].is_cuda and float(seen["rgbs"].min()) >= -1 and float(seen["rgbs"].max()) <= 1
    assert seen["hints"].shape == (3, 2, 24, 24) and seen["mask_s"].shape == (3, 1, 24, 24)
    first = ops.flow_finish(seen["hints"], seen["mask_s"], fc.H, fc.W).cpu()
    for v, fr in enumerate(frames):
        a, b = fr["T2C_flow"]
        assert a.shape == b.shape == (1, 2, fc.H, fc.W) and a.dtype == torch.float32 and not a.is_cuda
        assert torch.equal(a[0], first[v])              # the same seed drew the same sigmas: the first call's hints were these
        assert torch.equal(b, 2 * a)                    # doubling is exact in every product and sum of the tail
    assert all(fr["T2C_flow"][0].abs().max() > 1e-3 for fr in frames) and len(set(drawn)) > 1
