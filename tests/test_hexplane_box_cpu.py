"""The inputs of tests/test_hexplane_box_gpu.py discriminate: pinned here on the oracle alone, without a GPU.

A GPU test that a correct kernel and a wrong one both pass proves nothing.  So, for every box, axis and plane size that test uses:
(a) the oracle's fp32 normalize_aabb leaves the point on a MIN face strictly inside ATen's border clip; (b) the same expression
with product and difference in one rounding (an fma, emulated in fp64) clips it -- and on the control box the two forms agree;
(c) with the GPU test's seeded planes the oracle's d xyz of each min-face point along its face axis is at least 100 times the
absolute tolerance the GPU test applies to that tensor, so a wrongly clipped point cannot hide inside it.  The point on a MAX face
has c = -1 exactly in both forms and is clipped in both: the case that must stay zero."""
import numpy as np
import pytest

import hexplane_box_cases as hb

BOXES, SHAPES = list(hb.BOXES), list(hb.SHAPES)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("box", BOXES)
def test_min_face_point_is_inside_for_torch_and_clipped_when_contracted(box, shape):
    import torch
    from oracle import torch_ref as tr
    hi, lo, diverges = hb.BOXES[box]
    aabb = torch.tensor([hi, lo], dtype=torch.float32)
    c_min = tr.normalize_aabb(torch.tensor([lo], dtype=torch.float32), aabb)[0].numpy()
    c_max = tr.normalize_aabb(torch.tensor([hi], dtype=torch.float32), aabb)[0].numpy()
    for k, sizes in hb.plane_sizes(shape).items():
        ct, cc = hb.coord_torch_form(lo[k], hi[k], lo[k]), hb.coord_contracted_form(lo[k], hi[k], lo[k])
        assert ct == c_min[k], (k, ct, c_min[k])                 # the numpy restatement is the oracle's arithmetic, bit for bit
        assert cc >= ct                                          # (one rounding: 1 - 2^-24 or 1; c + 1 then rounds to 2)
        assert c_max[k] == np.float32(-1.0) and hb.coord_contracted_form(hi[k], hi[k], lo[k]) == np.float32(-1.0)
        for s in sizes:
            assert hb.clipped(cc, s) and hb.clipped(c_max[k], s), (k, s)
            if diverges:
                assert ct < np.float32(1.0) and not hb.clipped(ct, s), (k, s, ct, hb.unnormalize(ct, s))      # (a) against (b)
                assert hb.unnormalize(ct, s) < np.float32(s - 1)
            else:
                assert ct == cc and hb.clipped(ct, s), (k, s, ct)                                             # the control
    assert hb.predicted_divergent_axes(hi, lo, shape) == ([0, 1, 2] if diverges else [])


def test_the_issue_example():
    """(max, min) = (0.5, -1.2) at plane size 8: torch unnormalises to 6.9999995, the contracted form to 7."""
    ct, cc = hb.coord_torch_form(-1.2, 0.5, -1.2), hb.coord_contracted_form(-1.2, 0.5, -1.2)
    assert hb.unnormalize(ct, 8) == np.nextafter(np.float32(7.0), np.float32(0.0)) and hb.unnormalize(cc, 8) == np.float32(7.0)


@pytest.mark.parametrize("channels", [32, 16])
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("box", BOXES)
def test_oracle_gradient_at_the_faces(box, shape, channels):
    """(c), and the zero pattern the GPU test compares: along its face axis a min-face point has a position gradient far above
    the GPU test's tolerance exactly where the two forms differ; max faces and the points well outside have exactly zero.  (One
    ulp to either side of a face the oracle may clip or not -- the rounded scale decides -- and the GPU test takes whichever it
    does.)"""
    diverges = hb.BOXES[box][2]
    _, dxyz, _ = hb.oracle(channels, box, shape)
    atol = hb.grad_atol(dxyz)
    live = list(hb.MIN_FACE.items()) + [(hb.MIN_CORNER, k) for k in range(3)]
    for i, k in live:
        if diverges:
            assert abs(dxyz[i, k]) >= 100 * atol, (i, k, float(dxyz[i, k]), atol)
        else:
            assert dxyz[i, k] == 0, (i, k)
    for i, k in list(hb.MAX_FACE.items()) + [(hb.MAX_CORNER, k) for k in range(3)]:
        assert dxyz[i, k] == 0, (i, k, float(dxyz[i, k]))
    assert dxyz[10, 0] == 0 and dxyz[11, 1] == 0 and dxyz[12, 2] == 0 and not dxyz[13].any() and not dxyz[14].any()
    # every special point keeps the coordinates nobody wrote over strictly inside: those axes carry a gradient
    assert dxyz[10, 1] != 0 and dxyz[10, 2] != 0 and dxyz[0, 1] != 0 and dxyz[0, 2] != 0


def test_the_seeded_clouds_include_boxes_where_the_forms_differ():
    """The cloud property test of the GPU file draws its boxes from the clouds' own extremes; the emulation must predict a
    difference for some of them (about one axis in ten), or that test could not see a wrong clip."""
    per_cloud = []
    for seed in hb.CLOUD_SEEDS:
        pts, hi, lo = hb.cloud(seed)
        assert pts.shape == (hb.P, 3) and (hi > lo).all()
        for i, k, side in hb.defining_points(pts, hi, lo):
            assert pts[i, k] == (lo[k] if side == "min" else hi[k])
        per_cloud.append(len(hb.predicted_divergent_axes(hi, lo, "small")))
    assert sum(1 for n in per_cloud if n) >= 3, per_cloud
