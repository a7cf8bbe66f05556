"""The inputs of tests/test_hexplane_orders_gpu.py do what they exist for: pinned here without a GPU.

(a) Every order family is a permutation with a matching inverse, at the sizes the GPU tests use (nothing else may reach a kernel:
the kernels index with it).  (b) Each family produces the events the scatter's run detection never meets under a fresh sorted
order -- asserted from the counter of tests/hexplane_order_cases.py, so an edit of the helper cannot hollow the GPU tests out.
(c) The walk lengths the multi-chunk cases rely on, recomputed from the launchers' formulas.  (d) How much fp32 summation noise
the large inputs carry: the plane gradients of the fp32 oracle lie within HALF of the suite's gradient tolerance of the float64
evaluation, so a kernel that sums in another order has the other half.  (e) Why float64 is no reference for d xyz or the features.

The library's sorts are emulated here (a stable argsort of the emulated Morton key); the GPU file holds mom_hexplane_orders to
exactly that emulation."""
import numpy as np
import pytest

import hexplane_box_cases as hb
import hexplane_order_cases as oc

SLOTS = [(si, l) for si in range(3) for l in range(2)]


def _lib(shape):
    return lambda pts: oc.emulated_lib_orders(pts, shape)


@pytest.mark.parametrize("P", [1, 33, 300, 131109])
@pytest.mark.parametrize("family", oc.FAMILIES)
def test_every_family_is_a_permutation_with_its_inverse(family, P):
    pts = oc.cloud(P)
    assert pts.shape == (P, 3)
    morton, order, inv = oc.orders(family, pts, "small", _lib("small"))           # (validates)
    assert morton.dtype == order.dtype == inv.dtype == np.int32
    assert oc.is_permutation(morton, P)
    for si, l in SLOTS:
        assert oc.is_permutation(order[si, l], P) and oc.is_permutation(inv[si, l], P)
        assert np.array_equal(inv[si, l][order[si, l]], np.arange(P, dtype=np.int32))
        assert np.array_equal(order[si, l][inv[si, l]], np.arange(P, dtype=np.int32))


def test_validate_refuses_what_is_not_a_permutation():
    morton, order, inv = oc.orders("random", oc.cloud(33), "small")
    bad = order.copy()
    bad[1, 1, 5] = bad[1, 1, 6]
    with pytest.raises(AssertionError):
        oc.validate(morton, bad, inv, 33, 2)
    with pytest.raises(AssertionError):
        oc.validate(morton, order, inv[:, ::-1].copy(), 33, 2)
    with pytest.raises(AssertionError):
        oc.validate(np.full(33, 33, np.int32), order, inv, 33, 2)


def test_the_helpers_field_is_the_box_tests_field():
    """oc.field builds the shapes hexplane_box_cases does not know the way hb.field builds its own: "small" given as a tuple (the
    helper's own construction) has the very planes and box of hb.field's "small"."""
    import torch
    for channels in (32, 16):
        a, b = oc.field(channels, oc.BOX, oc.SHAPES["small"]), hb.field(channels, oc.BOX, "small")
        assert torch.equal(a.aabb, b.aabb) and a.feat_dim == b.feat_dim
        for ga, gb in zip(a.grids, b.grids):
            assert len(ga) == len(gb) == 6
            for pa, pb in zip(ga, gb):
                assert pa.shape == pb.shape and pa.stride() == pb.stride() and torch.equal(pa, pb)


def test_the_clouds():
    hi, lo, _ = hb.BOXES[oc.BOX]
    hi, lo = np.asarray(hi, np.float32), np.asarray(lo, np.float32)
    for P in (131109, 270001):
        p = oc.cloud(P).numpy()
        outside = ((p < lo) | (p > hi)).any(1).mean()
        assert 0.03 < outside < 0.05, outside
    assert np.array_equal(oc.cloud(300).numpy(), hb.points(oc.BOX).numpy())
    # the displacement of the stale family: a few cells for most points, anywhere for one in twenty
    p = oc.cloud(131109)
    d = np.abs(oc.displaced(p, "small").numpy() - p.numpy()) / ((hi - lo) / (np.asarray(oc.level_sizes("small")[-1], np.float32) - 1))
    assert 0.93 < (d <= 3.0001).all(1).mean() < 0.97
    # all in one texel of every plane and level, all distinct; all on the border of every plane
    one = oc.one_cell_cloud()
    assert len({tuple(r) for r in one.numpy().tolist()}) == hb.P
    for c in oc.cells(one, "small").values():
        assert c.interior.all() and len(set(c.cell.tolist())) == 1
    for c in oc.cells(oc.outside_cloud(), "small").values():
        assert not c.interior.any()


def test_the_event_counter_on_a_walk_made_by_hand():
    """A 4 x 4 plane, the time line riding on x.  Cells by (x0, y0): A = (0, 0), B = (2, 0) (the same parity as A: its corners evict
    A's from all four slots), C = (1, 0) (shares A's right-hand corners), and a border position X with x0 = 3."""
    x0 = np.array([0, 0, 2, 0, 3, 0, 1, 1])
    y0 = np.array([0, 0, 0, 0, 0, 0, 0, 1])
    inner = x0 + 1 < 4
    c = oc.Cells(x0, y0, 4, 4, inner, y0 * 4 + x0, x0, inner)
    e = oc.events(np.arange(8), c, 2)
    # A A | B A | X A | C C':  changes at B, A, X, A, C, C' = 6; the run A A does not cross a multiple of 2 ...
    assert e.cell_changes == 6 and e.chunk_crossing_runs == 0
    assert e.sandwiches == 1                                           # A X A
    assert e.row_stays == 1                                            # C -> C' keeps x0 = 1 while y0 changes
    # B evicts A's four rows, A evicts B's four, X (corners x = 3 only: slots 1 and 3) evicts two, A two again (x = 1 rows);
    # C = (1, 0) replaces A's x = 0 rows by x = 2 rows (two), C' = (1, 1) replaces the y = 0 rows by y = 2 rows (two)
    assert e.evictions == 4 + 4 + 2 + 2 + 2 + 2
    # ... and does when the walk is shifted by one
    assert oc.events(np.array([7, 0, 1, 2, 3, 4, 5, 6]), c, 2).chunk_crossing_runs == 1


def test_adversarial_orders_evict_and_sandwich_on_every_plane_and_level():
    pts = oc.cloud(300)
    cs = oc.cells(pts, "small")
    _, order, _ = oc.orders("adversarial", pts, "small")
    for si, l in SLOTS:
        e = oc.events(order[si, l], cs[si, l], 32)
        assert e.evictions > 0 and e.sandwiches > 0, (si, l, e)
        assert e.cell_changes >= 0.9 * 299, (si, l, e)


@pytest.mark.parametrize("P", [300, 131109])
def test_random_orders_change_the_cell_at_nearly_every_position(P):
    pts = oc.cloud(P)
    cs = oc.cells(pts, "mid")
    _, order, _ = oc.orders("random", pts, "mid")
    for si, l in SLOTS:
        e = oc.events(order[si, l], cs[si, l], 32)
        assert e.cell_changes >= 0.9 * P, (si, l, e)
        assert e.evictions > 0


def test_fresh_orders_have_runs_that_cross_a_chunk_boundary_and_stale_ones_have_what_fresh_ones_lack():
    pts = oc.cloud(131109)
    cs = oc.cells(pts, "small")
    _, fresh, _ = oc.orders("fresh", pts, "small", _lib("small"))
    _, stale, _ = oc.orders("stale", pts, "small", _lib("small"))
    for si, l in SLOTS:
        for chunk, walk in ((32, oc.per_half32(131109)), (16, oc.per_group16(131109))):
            assert oc.events(fresh[si, l], cs[si, l], chunk).chunk_crossing_runs > 0, (si, l, chunk)
            assert oc.events(fresh[si, l], cs[si, l], chunk, walk).chunk_crossing_runs > 0, (si, l, chunk, walk)     # inside a walker
        f, s = oc.events(fresh[si, l], cs[si, l], 32), oc.events(stale[si, l], cs[si, l], 32)
        assert f.sandwiches == 0 and s.sandwiches > 0, (si, l, f, s)        # a sorted order keeps the border positions together
        assert s.cell_changes > 10 * f.cell_changes and s.evictions > 10 * f.evictions and s.row_stays > f.row_stays, (si, l, f, s)


def test_walk_lengths_of_the_multi_chunk_cases():
    """hexplane_backward:               per_half  = ceil(P / (512 * 8))  rounded up to 32  (MOM_HEX_SBLOCKS = 512 workgroups, 8 half-waves)
    the same launcher at 16 channels:  per_group = ceil(P / (512 * 16)) rounded up to 16  (the same 512 workgroups, 16 groups)

         P        per_half  chunks   per_group  chunks
      131 072        32       1         16        1
      131 109        64       2         32        2
      270 001        96       3         48        3

    and the gathers (1536 workgroups x 4 waves x 32 points a trip) take a second trip above 196 608 points."""
    want = {131072: (32, 1, 16, 1), 131109: (64, 2, 32, 2), 270001: (96, 3, 48, 3)}
    for P, (ph, c32, pg, c16) in want.items():
        assert (oc.per_half32(P), oc.per_half32(P) // 32, oc.per_group16(P), oc.per_group16(P) // 16) == (ph, c32, pg, c16), P
    assert oc.GATHER_ONE_TRIP == 196608 and 131109 < oc.GATHER_ONE_TRIP < 270001
    assert {P for _, P in oc.LARGE} == set(want)
    # the largest sizes at which the other HexPlane tests meet the oracle walk one chunk
    assert oc.per_half32(20011) == 32 and oc.per_group16(20000) == 16


@pytest.mark.parametrize("shape,P", oc.LARGE)
@pytest.mark.parametrize("channels", [32, 16])
def test_the_large_inputs_carry_little_summation_noise(channels, shape, P):
    """Every plane gradient of the fp32 oracle within half of the suite's tolerance of the float64 one (measured: 0.11 to
    0.15 of it on "small", 0.41 and 0.46 on "mid"): the GPU test compares the kernels with the float64 gradients at the full tolerance."""
    a, b = oc.oracle32(channels, shape, P), oc.oracle64(channels, shape, P)
    worst = 0.0
    for l, (la, lb) in enumerate(zip(a[2], b[2])):
        for i, (ga, gb) in enumerate(zip(la, lb)):
            assert gb.dtype == np.float64 and ga.shape == gb.shape
            worst = max(worst, oc.plane_error_ratio(ga, gb))
            np.testing.assert_allclose(ga, gb, rtol=0.5 * hb.GRAD_RTOL, atol=0.5 * hb.grad_atol(gb), err_msg=f"plane {l} {i}")
    print(f"{channels} channels, {shape}, P = {P}: fp32 oracle against float64, worst plane gradient error {worst:.3f} of the tolerance")


def test_float64_is_no_reference_for_dxyz_or_the_features():
    """A point within rounding of a texel boundary falls into one cell in fp32 and into its neighbour in float64.  The features are
    continuous across the boundary, the slope is not: d xyz of such a point differs at full scale.  So d xyz and the features are
    compared with the fp32 oracle only, and this assertion documents why: at P = 270 001 on "mid" some points exceed the gradient
    tolerance, every one of them is a point whose emulated fp32 cell (or clip decision) differs from the float64 one on some plane
    and level, and everywhere else the two agree within the tolerance."""
    shape, P = "mid", 270001
    a, b = oc.oracle32(32, shape, P), oc.oracle64(32, shape, P)
    pts = oc.cloud(P)
    c32, c64 = oc.cells(pts, shape), oc.cells(pts, shape, ft=np.float64)
    flips = np.zeros(P, bool)
    for k in c32:
        flips |= (c32[k].x0 != c64[k].x0) | (c32[k].y0 != c64[k].y0)
    over = (np.abs(a[1] - b[1]) > hb.grad_atol(a[1]) + hb.GRAD_RTOL * np.abs(a[1])).any(1)
    assert over.any() and flips.any()
    assert not (over & ~flips).any(), np.nonzero(over & ~flips)[0][:10]
    assert float(np.abs(a[1] - b[1]).max()) > 100 * hb.grad_atol(a[1])
