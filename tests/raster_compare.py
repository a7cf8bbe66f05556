"""Comparisons of one rasterizer state with another, shared by the parity tests: a HIP state (hip_helpers.hip_forward) or a
reference state (oracle/ref_gpu.py) on the left, the CPU oracle's or the reference's state on the right.  The gates are the
regression gates of tests/test_raster_gpu.py; a plain module, collected by no test run."""
import numpy as np

# Regression gates, set from what the kernels achieve (tools/parity_stats.py on an MI355X: image mean L1 2.9e-8 .. 4.3e-8, max
# 1.2e-6, no pixel above 1e-5, n_contrib and last contributors identical, gradient norms within 4.6e-6, worst gradient row
# 1.3e-5 of its tensor's scale) -- the north star's 1e-4 is the ceiling, not the gate.  A (pixel, splat) pair whose alpha sits
# within rounding of one of the hard thresholds (1/255, 0.99, T < 1e-4) may legitimately take the other branch under v_exp_f32
# than under expf; such pixels / rows are allowed as COUNTED exceptions and every outlier pixel must be shown to hold such a pair.
NORTH_STAR_L1 = 1e-4
IMG_L1_TOL = 1e-6      # mean per-pixel L1
IMG_PIX_TOL = 1e-5     # per pixel; above it: a counted threshold exception, bounded by IMG_MAX_TOL
IMG_MAX_TOL = 2e-2
MAX_EXC_FRAC = 1e-4    # at most this fraction of the pixels / Gaussian rows (and never fewer than 2 allowed) may be exceptions
GRAD_REL_TOL = 5e-5
ROW_TOL, ROW_MAX = 2e-5, 5e-3


def _allowed(n):
    return max(2, int(MAX_EXC_FRAC * n))


def _near_threshold(st, px, py, W, rel=2e-5):
    """Does pixel (px, py) of the oracle state hold a (pixel, splat) pair whose alpha is within `rel` of 1/255 or 0.99, or whose
    transmittance test T (1 - alpha) < 1e-4 is that close?  (forward.cu:331-345, recomputed from the oracle's own lists.)"""
    gx = (W + 15) // 16
    t = (py // 16) * gx + px // 16
    T = 1.0
    for i in st.point_list[st.ranges[t, 0]:st.ranges[t, 1]]:
        dx, dy = float(st.means2D[i, 0]) - px, float(st.means2D[i, 1]) - py
        cx, cy, cz, op = (float(v) for v in st.conic_opacity[i])
        power = -0.5 * (cx * dx * dx + cz * dy * dy) - cy * dx * dy
        if power > 0:
            continue
        raw = op * np.exp(power)
        alpha = min(0.99, raw)
        if abs(raw - 1.0 / 255.0) <= rel / 255.0 or abs(raw - 0.99) <= rel:
            return True
        if alpha < 1.0 / 255.0:
            continue
        if abs(T * (1 - alpha) - 1e-4) <= rel * 1e-4:
            return True
        if T * (1 - alpha) < 1e-4:
            break
        T *= 1 - alpha
    return False


def _assert_image(fw_img, st_img, st, what):
    d = np.abs(fw_img - st_img)
    assert d.mean() <= IMG_L1_TOL <= NORTH_STAR_L1, (what, d.mean())
    H, W = d.shape[1], d.shape[2]
    ys, xs = np.nonzero(d.max(axis=0) > IMG_PIX_TOL)
    assert len(ys) <= _allowed(W * H) and d.max() <= IMG_MAX_TOL, (what, len(ys), d.max())
    for y, x in zip(ys, xs):
        assert _near_threshold(st, int(x), int(y), W), (what, "pixel off by more than rounding without a threshold pair", x, y)



def _last_contributor(n_contrib, ranges, point_list, W, H):
    """Gaussian index of every pixel's last contributor (-1: none), from a rasterizer state's own lists."""
    gx = (W + 15) // 16
    py, px = np.divmod(np.arange(W * H), W)
    tile = (py // 16) * gx + px // 16
    nc = n_contrib.astype(np.int64)
    pos = ranges[tile, 0].astype(np.int64) + nc - 1
    out = np.full(W * H, -1, dtype=np.int64)
    has = nc > 0
    out[has] = point_list[pos[has]]
    return out


def _cmp_lists_culled(fw, st, W, H):
    """Default binning (MomRasterArgs.keep_all_tiles = 0): every tile's list is the reference's list, in the reference's
    order, less instances that cannot reach alpha >= 1/255 in the tile.  That nothing contributing was dropped is shown by the
    image / gradient comparisons (bit-identical to keep_all_tiles = 1, test_tile_cull_changes_no_output) and, here, by every
    pixel's last contributor being the reference's."""
    assert fw["R"] <= st.num_rendered
    rg = fw["ranges"].astype(np.int64)
    cnt = rg[:, 1] - rg[:, 0]
    assert int(cnt.sum()) == fw["R"]
    for t in range(rg.shape[0]):
        mine = fw["point_list"][rg[t, 0]:rg[t, 1]]
        ref = st.point_list[st.ranges[t, 0]:st.ranges[t, 1]]
        assert len(mine) <= len(ref)
        np.testing.assert_array_equal(ref[np.isin(ref, mine)], mine)          # an order-preserving subsequence
    a = _last_contributor(fw["n_contrib"], fw["ranges"], fw["point_list"], W, H)
    b = _last_contributor(st.n_contrib, st.ranges, st.point_list, W, H)
    bad = np.nonzero(a != b)[0]
    assert len(bad) <= _allowed(W * H), len(bad)
    for p in bad:
        assert _near_threshold(st, int(p % W), int(p // W), W), ("last contributor differs without a threshold pair", p)


def _cmp_forward(fw, st, P, feat=None, walked=True):
    """walked=False: one of the two sides is a state of the reference's own kernels (oracle/ref_gpu.py), which have no
    tile_walked output; every other comparison is made, a reference state on the left being one with keep_all_tiles = True."""
    culled = not fw["keep_all_tiles"]
    if not culled:
        assert fw["R"] == st.num_rendered
    np.testing.assert_array_equal(fw["radii"], st.radii)
    vis = st.radii > 0
    np.testing.assert_array_equal(fw["tiles_touched"], st.tiles_touched)
    # depth keys, pixel centres and conics come out of a contraction-free fp32 pipeline: bit-exact
    np.testing.assert_array_equal(fw["depths"][vis].view(np.uint32), st.depths[vis].view(np.uint32))
    np.testing.assert_array_equal(fw["means2D"][vis].view(np.uint32), st.means2D[vis].view(np.uint32))
    np.testing.assert_array_equal(fw["conic_opacity"][vis].view(np.uint32), st.conic_opacity[vis].view(np.uint32))
    if culled:
        _cmp_lists_culled(fw, st, fw["color"].shape[2], fw["color"].shape[1])
    else:
        np.testing.assert_array_equal(fw["ranges"], st.ranges)
        np.testing.assert_array_equal(fw["point_list"], st.point_list)      # the whole sort, bit for bit
    np.testing.assert_array_equal(fw["clamped"][vis], st.clamped[vis])
    # with precomputed colours the reference leaves geomState.rgb untouched and renders from the input
    ref_rgb = st.rgb if feat is None else feat
    np.testing.assert_allclose(fw["rgb"][vis], ref_rgb[vis], rtol=1e-6, atol=1e-7)
    _assert_image(fw["color"], st.out_color, st, "color")
    dscale = max(1.0, float(st.depths.max()))
    _assert_image(fw["depth"] / dscale, st.out_depth / dscale, st, "depth")
    if not culled:
        W = fw["color"].shape[2]
        bad = np.nonzero((fw["n_contrib"] != st.n_contrib).reshape(-1))[0]
        assert len(bad) <= _allowed(fw["n_contrib"].size), len(bad)
        for p in bad:
            assert _near_threshold(st, int(p % W), int(p // W), W), ("n_contrib differs without a threshold pair", p)
    assert np.abs(fw["final_T"] - st.final_T).mean() <= 1e-8
    # SURVEY 8d's Q: entries each tile's block walks before it exits, in rounds of 256 (forward.cu:305-312): an integer per tile.
    # On the reference's lists it is the oracle's, but for tiles whose last saturating pixel sits on a threshold (the same counted
    # exception as n_contrib above, seen through a 256-entry round: rarer); on culled lists it can only be shorter.
    if not walked:
        return
    cnt = (fw["ranges"][:, 1].astype(np.int64) - fw["ranges"][:, 0])
    assert (fw["tile_walked"] <= cnt).all()
    if not culled:
        off = np.nonzero(fw["tile_walked"] != st.tile_walked)[0]
        assert len(off) <= max(1, len(cnt) // 200), (len(off), len(cnt))
        assert ((fw["tile_walked"][off] % 256 == 0) | (fw["tile_walked"][off] == cnt[off])).all()
    else:
        assert int(fw["tile_walked"].sum()) <= int(st.tile_walked.sum())


def _relerr(a, b):
    return float(np.linalg.norm(a.astype(np.float64) - b) / (np.linalg.norm(b) + 1e-20))


GRAD_NAMES = ("dL_dmeans2D", "dL_dcolors", "dL_dopacity", "dL_dmeans3D", "dL_dcov3D", "dL_dsh", "dL_dscales", "dL_drotations")


def _cmp_grads(g, go, st, names=GRAD_NAMES, what=""):
    for name in names:
        a, b = g[name], go[name].reshape(g[name].shape)
        assert _relerr(a, b) <= GRAD_REL_TOL, (what, name, _relerr(a, b))
        inv = st.radii == 0
        assert np.abs(a[inv]).max(initial=0.0) == 0.0, (what, name)
        # per GAUSSIAN, not only as a whole-tensor norm (a norm hides a few badly wrong rows): the worst element of a row,
        # relative to the tensor's largest element, is within ROW_TOL on all rows but a counted handful (_allowed) and within
        # ROW_MAX on those -- Gaussians with a (pixel, splat) pair whose alpha sits within an ulp of the 1/255 or 0.99
        # thresholds (v_exp_f32 vs expf), where the two implementations legitimately take different branches.
        scale = max(float(np.abs(b).max()), 1e-30)
        row_err = np.abs(a - b).reshape(a.shape[0], -1).max(axis=1) / scale
        n_bad = int((row_err > ROW_TOL).sum())
        assert n_bad <= _allowed(a.shape[0]) and float(row_err.max()) <= ROW_MAX, (what, name, n_bad, float(row_err.max()))
