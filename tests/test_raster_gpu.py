"""GPU parity: libmom4d (HIP, through the reference-shaped `_C` boundary) vs the CPU oracle on identical
Gaussians.  Bar (BASELINE.json north_star): integer tile/sort indices bit-exact; images within 1e-4 per-pixel L1."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import raster_oracle as ro
from raster_compare import (GRAD_NAMES, GRAD_REL_TOL, _allowed, _assert_image, _cmp_forward, _cmp_grads, _last_contributor,
                            _near_threshold, _relerr)
from scenes import (POSES, camera, clamp_some_channels, near_plane_scene, pose, posed_gaussians, quat_left, quat_of, random_gaussians,
                    rigid_move, to_world, view_space)

pytestmark = pytest.mark.gpu

# The SH backward against float64 (hip_helpers.sh_backward_fp64) on the kernel's own dL_dcolors and clamp flags: per-Gaussian
# arithmetic with no threshold in it, so every element is held, relative to the largest element of its Gaussian's row, with no
# exceptions.  Coefficient gradients: measured 3.4e-7 on an MI355X (fp32 direction and basis against fp64).  The view-direction
# term of dL/d mean3D, taken as the difference from a projection backward at degree 0 on the same record (test_sh_layouts_gpu):
# measured within 2.1e-7 of the row's whole dL/d mean3D, the scale at which the two fp32 sums it is the difference of round (the
# term itself is a median 1.3 % (degree 1) to 5.4 % (degree 3) of that scale); DIR_TOL leaves room for the term's own fp32 arithmetic.
SH_EXACT_TOL = 1e-6
DIR_TOL, DIR_SUM_TOL = 1e-5, 1e-6


def _oracle(s, **kw):
    args = dict(shs=s.get("shs"), sh_degree=3, scales=s["scales"], rotations=s["rotations"])
    args.update(kw)
    return ro.forward(s["means3D"], s["opacities"], s["viewmatrix"], s["projmatrix"], s["campos"], s["W"], s["H"],
                      s["tanfovx"], s["tanfovy"], s["bg"], **args)


def _check_sh_fp64(D, dsh, shs, means3D, campos, dcolors, clamped, radii, what=""):
    """dL_dsh [P, M, 3] of a kernel: Y_k(dir) dRGB in float64 on every visible Gaussian, exactly zero above the active degree and
    on every Gaussian with radius 0.  Returns the float64 view-direction term of dL/d mean3D of the visible ones."""
    from hip_helpers import sh_backward_fp64
    vis = radii > 0
    assert vis.any(), what
    want, ddir = sh_backward_fp64(D, shs[vis], means3D[vis], campos, dcolors[vis], clamped[vis])
    got = dsh[vis].astype(np.float64)
    row = np.abs(want).reshape(len(want), -1).max(axis=1)
    err = np.abs(got - want).reshape(len(want), -1).max(axis=1)
    assert (err <= SH_EXACT_TOL * row).all(), (what, D, float((err / np.maximum(row, 1e-30)).max()), int((err > SH_EXACT_TOL * row).sum()))
    used = (D + 1) * (D + 1)
    assert not np.any(dsh[:, used:]), (what, D, "gradient above the active degree")
    assert not np.any(dsh[~vis]), (what, D, "gradient on a Gaussian with radius 0")
    return ddir


def test_wave_sum_selftest():
    from hip_helpers import N
    x = torch.randn(64 * 37, device="cuda")
    out = torch.zeros(37, device="cuda")
    N.check(N.lib().mom_selftest_wave_sum(x.data_ptr(), out.data_ptr(), 37, N.current_stream()), "selftest")
    torch.cuda.synchronize()
    np.testing.assert_allclose(out.cpu().numpy(), x.view(37, 64).double().sum(1).cpu().numpy(), rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("nvals", [9, 10])
def test_row_reduce_selftest(nvals):
    """The compositing backward's reduction as the kernel composes it (DPP reduce-scatter inside the rows with bank-masked
    rotations, then the 4 x 4 transposition over four splats' rows): every one of the 4 x nvals sums of every wave, against
    float64 sums; the inputs are distinct in every lane, so a wrong lane pairing cannot cancel."""
    from hip_helpers import N
    waves = 53
    g = torch.Generator(device="cpu").manual_seed(nvals)
    x = torch.randn(waves, 4, nvals, 64, generator=g).cuda()
    out = torch.full((waves, 4, nvals), float("nan"), device="cuda")
    N.check(N.lib().mom_selftest_row_reduce(x.data_ptr(), out.data_ptr(), waves, nvals, N.current_stream()), "selftest")
    torch.cuda.synchronize()
    np.testing.assert_allclose(out.cpu().numpy(), x.double().sum(-1).cpu().numpy(), rtol=2e-6, atol=2e-6)


@pytest.mark.parametrize("seed,P,W,H,kw", [
    (0, 2000, 128, 96, {}),
    (1, 5000, 256, 256, {}),                       # BASELINE configs[0] geometry: 5k Gaussians, 256x256
    (2, 700, 100, 50, dict(scale=(-3.0, -0.5))),   # ragged image, large splats (wave-cooperative enumeration)
    (3, 64, 33, 17, {}),
    (4, 20000, 320, 180, dict(scale=(-5.0, -3.0))),
    (5, 100000, 480, 270, dict(scale=(-5.5, -3.5))),      # mid size: half of config 2's Gaussians at a quarter of its pixels
    (6, 200000, 960, 540, dict(scale=(-5.5, -3.5))),      # BASELINE configs[1] at full size: 200 k Gaussians, 960x540 (oracle on 16 threads)
])
@pytest.mark.parametrize("keep_all_tiles", [True, False])
def test_forward_parity(seed, P, W, H, kw, keep_all_tiles):
    from hip_helpers import hip_forward
    ro.set_threads(16 if P >= 100000 else 1)
    s = random_gaussians(P, seed=seed, W=W, H=H, **kw)
    _cmp_forward(hip_forward(s, keep_all_tiles=keep_all_tiles), _oracle(s), P)


def test_exact_mode_with_a_guess_that_is_too_small_renders_the_frame_again():
    """diff_gaussian_rasterization._C.exact_render enqueues the compositing into a buffer sized from earlier frames BEFORE it
    waits for this frame's instance count; when the count exceeds the guess it must run the frame's rasterizer stages again with
    the exact size (the truncated scatter has consumed the bucket cursors).  Forced here: a guess of 4096 instances for a frame
    of ~10^5; the result -- count, lists, images -- is the oracle's, and the next frame's guess has grown."""
    from hip_helpers import RC, hip_forward
    ro.set_threads(16)
    s = random_gaussians(20000, seed=4, W=320, H=180, scale=(-5.0, -3.0))
    st = _oracle(s)
    assert st.num_rendered > 3 * 4096
    for keep_all in (True, False):
        RC._state["exact_cap"] = 4096
        fw = hip_forward(s, keep_all_tiles=keep_all)
        _cmp_forward(fw, st, 20000)
        assert RC._state["exact_cap"] >= fw["R"] > 4096
        again = hip_forward(s, keep_all_tiles=keep_all)          # now inside the guess: same result, no second pass needed
        np.testing.assert_array_equal(again["point_list"], fw["point_list"])
        np.testing.assert_array_equal(again["color"], fw["color"])


def test_forward_parity_lower_sh_degree_and_scale_modifier():
    from hip_helpers import hip_forward
    s = random_gaussians(1500, seed=7, W=96, H=80)
    for deg in (0, 1, 2):
        fw = hip_forward(s, sh_degree=deg, scale_modifier=0.7)
        st = _oracle(s, sh_degree=deg, scale_modifier=0.7)
        _cmp_forward(fw, st, 1500)


def test_forward_parity_precomputed_colors_and_cov3d():
    from hip_helpers import hip_forward
    s = random_gaussians(1200, seed=8, W=80, H=64)
    rng = np.random.default_rng(0)
    cols = rng.uniform(0, 1, (1200, 3)).astype(np.float32)
    st0 = _oracle(s)
    fw = hip_forward(s, colors_precomp=cols)
    st = _oracle(s, shs=None, colors_precomp=cols)
    _cmp_forward(fw, st, 1200, feat=cols)
    fw = hip_forward(s, cov3D_precomp=st0.cov3D)
    st = _oracle(s, scales=None, rotations=None, cov3D_precomp=st0.cov3D)
    _cmp_forward(fw, st, 1200)


def test_oversized_tile_bucket_uses_global_sort_path():
    # > 8192 instances in one tile: exercises the global-memory bitonic path; equal depths exercise the idx tiebreak
    from hip_helpers import hip_forward
    P = 9000
    s = random_gaussians(P, seed=9, W=32, H=32, scale=(-5.5, -4.5))
    s["means3D"][:, 0] *= 0.05
    s["means3D"][:, 1] *= 0.05
    s["means3D"][100:, 2] = np.abs(s["means3D"][100:, 2]) + 0.5
    s["means3D"][2000:2500, 2] = 3.0     # exact depth ties
    s["opacities"][:] = 0.02
    fw, st = hip_forward(s, keep_all_tiles=True), _oracle(s)
    assert (st.ranges[:, 1] - st.ranges[:, 0]).max() > 8192
    _cmp_forward(fw, st, P)
    fw = hip_forward(s)
    assert (fw["ranges"][:, 1].astype(np.int64) - fw["ranges"][:, 0]).max() > 8192        # still the global path after the cull
    _cmp_forward(fw, st, P)


def test_empty_and_all_culled():
    from hip_helpers import hip_backward, hip_forward
    s = random_gaussians(10, seed=1, W=48, H=32)
    s0 = {k: (v[:0] if isinstance(v, np.ndarray) and v.shape[:1] == (10,) else v) for k, v in s.items()}
    fw = hip_forward(s0)
    assert fw["R"] == 0 and (fw["color"] == 0).all() and (fw["depth"] == 0).all()
    s["means3D"][:, 2] = -1.0
    fw = hip_forward(s)
    assert fw["R"] == 0 and (fw["radii"] == 0).all()
    np.testing.assert_allclose(fw["color"], np.broadcast_to(s["bg"][:, None, None], (3, 32, 48)))
    # ... and as the FIRST frames of a process (exact mode has no guess yet): every frame of a run of empty frames
    # must still composite -- the background image, as the reference returns for num_rendered == 0 -- and hand back a buffer
    from hip_helpers import RC
    RC._state["exact_cap"] = 0
    s["bg"] = np.array([0.25, 0.5, 0.75], np.float32)
    for _ in range(2):
        fw = hip_forward(s)
        assert fw["R"] == 0 and RC._state["exact_cap"] == 0
        np.testing.assert_array_equal(fw["color"], np.broadcast_to(s["bg"][:, None, None], (3, 32, 48)))
        assert (fw["depth"] == 0).all()
        g = hip_backward(fw, np.ones((3, 32, 48), np.float32))          # the backward of an empty frame: zero gradients
        assert all((v == 0).all() for v in g.values())


@pytest.mark.parametrize("seed,P,W,H,kw", [
    (10, 1500, 128, 96, {}),
    (11, 400, 70, 45, dict(scale=(-3.0, -1.0))),
    (12, 5000, 256, 256, dict(scale=(-5.0, -3.0))),
    (13, 100000, 480, 270, dict(scale=(-5.5, -3.5))),
    (14, 200000, 960, 540, dict(scale=(-5.5, -3.5))),     # BASELINE configs[1] at full size: all eight gradient tensors against the oracle
])
def test_backward_parity(seed, P, W, H, kw):
    from hip_helpers import hip_forward, hip_backward
    ro.set_threads(16 if P >= 100000 else 1)
    s = random_gaussians(P, seed=seed, W=W, H=H, **kw)
    rng = np.random.default_rng(seed)
    dcol = rng.normal(size=(3, H, W)).astype(np.float32)
    ddep = (rng.normal(size=(1, H, W)) * 0.2).astype(np.float32)
    fw = hip_forward(s)
    st = _oracle(s)
    g = hip_backward(fw, dcol, ddep)
    go = ro.backward(st, dcol, ddep)
    _cmp_grads(g, go, st)


def _backward_case(s, seed, hip_kw, oracle_kw, names=GRAD_NAMES, feat=None):
    """Forward and backward through the `_C` drop-in against the oracle on the same inputs, a random image gradient and a nonzero
    depth gradient: the forward at _cmp_forward's gates, the gradients `names` at test_backward_parity's."""
    from hip_helpers import hip_backward, hip_forward
    P, W, H = s["means3D"].shape[0], s["W"], s["H"]
    rng = np.random.default_rng(seed)
    dcol = rng.normal(size=(3, H, W)).astype(np.float32)
    ddep = (rng.normal(size=(1, H, W)) * 0.2).astype(np.float32)
    fw = hip_forward(s, **hip_kw)
    st = _oracle(s, **oracle_kw)
    _cmp_forward(fw, st, P, feat=feat)
    g = hip_backward(fw, dcol, ddep)
    go = ro.backward(st, dcol, ddep)
    _cmp_grads(g, go, st, names, what=str(hip_kw.keys()))
    return fw, st, g, go


@pytest.mark.parametrize("scale_modifier", [1.0, 0.7])
@pytest.mark.parametrize("deg", [0, 1, 2])
def test_backward_parity_lower_sh_degree_and_scale_modifier(deg, scale_modifier):
    """The degrees the coarse stage renders at (0 -> 1 -> 2 over its first 3000 iterations), all 16 coefficients random and
    nonzero: the degree-1 / degree-2 derivatives of the view direction reach dL_dmeans3D, the coefficients above the degree get
    exactly zero."""
    s = random_gaussians(1500, seed=60 + deg, W=128, H=96)
    kw = dict(sh_degree=deg, scale_modifier=scale_modifier)
    fw, st, g, go = _backward_case(s, 60 + deg, kw, kw)
    _check_sh_fp64(deg, g["dL_dsh"], s["shs"], s["means3D"], s["campos"], g["dL_dcolors"], fw["clamped"], fw["radii"], "deg")


@pytest.mark.parametrize("M", [1, 4, 9])
def test_sh_counts_below_16(M):
    """A model with max_sh_degree < 3 hands the `_C` path shs of shape [P, M, 3], M = (max_sh_degree + 1)^2, rendered at that degree."""
    D = int(round(M ** 0.5)) - 1
    s = random_gaussians(1500, seed=70 + M, W=112, H=80)
    s["shs"] = np.ascontiguousarray(s["shs"][:, :M])
    fw, st, g, go = _backward_case(s, 70 + M, dict(sh_degree=D), dict(sh_degree=D))
    assert g["dL_dsh"].shape == (1500, M, 3)
    _check_sh_fp64(D, g["dL_dsh"], s["shs"], s["means3D"], s["campos"], g["dL_dcolors"], fw["clamped"], fw["radii"], "M")


def test_backward_parity_precomputed_colors():
    s = random_gaussians(1200, seed=80, W=96, H=64)
    cols = np.random.default_rng(80).uniform(0, 1, (1200, 3)).astype(np.float32)
    names = tuple(n for n in GRAD_NAMES if n != "dL_dsh")
    fw, st, g, go = _backward_case(s, 80, dict(colors_precomp=cols), dict(shs=None, colors_precomp=cols), names, feat=cols)
    assert float(np.abs(g["dL_dcolors"]).max()) > 0
    assert g["dL_dsh"].size == 0 or not g["dL_dsh"].any()


@pytest.mark.parametrize("deg", [1, 3])
def test_backward_parity_precomputed_cov3d(deg):
    s = random_gaussians(1200, seed=81 + deg, W=96, H=64)
    cov = _oracle(s).cov3D
    names = tuple(n for n in GRAD_NAMES if n not in ("dL_dscales", "dL_drotations"))
    fw, st, g, go = _backward_case(s, 81 + deg, dict(cov3D_precomp=cov, sh_degree=deg),
                                   dict(scales=None, rotations=None, cov3D_precomp=cov, sh_degree=deg), names)
    assert float(np.abs(g["dL_dcov3D"]).max()) > 0
    for n in ("dL_dscales", "dL_drotations"):
        assert g[n].size == 0 or not g[n].any(), n
    _check_sh_fp64(deg, g["dL_dsh"], s["shs"], s["means3D"], s["campos"], g["dL_dcolors"], fw["clamped"], fw["radii"], "cov3D")


@pytest.mark.parametrize("deg", [0, 1, 2, 3])
def test_backward_parity_with_clamped_colour_channels(deg):
    """Strongly negative DC terms in one channel of ~30 % of the Gaussians: that channel's colour clamps at 0 and the backward
    must drop its colour gradient on the way to the SH coefficients and the view direction (dRGB masked per channel)."""
    s = clamp_some_channels(random_gaussians(2000, seed=90 + deg, W=128, H=96), seed=90 + deg)
    kw = dict(sh_degree=deg)
    fw, st, g, go = _backward_case(s, 90 + deg, kw, kw)
    vis = st.radii > 0
    cl = st.clamped[vis].astype(bool)
    assert 0.05 * vis.sum() <= cl.any(axis=1).sum() < vis.sum(), (int(cl.any(axis=1).sum()), int(vis.sum()))
    # the mask matters only where the colour gradient is nonzero: many clamped channels of Gaussians that reach pixels
    dcol = g["dL_dcolors"][vis]
    assert int((cl & (dcol != 0)).sum()) >= 50, int((cl & (dcol != 0)).sum())
    dsh = g["dL_dsh"][vis]
    assert not np.any(np.where(cl[:, None, :], dsh, 0.0)), "a clamped channel received an SH gradient"
    _check_sh_fp64(deg, g["dL_dsh"], s["shs"], s["means3D"], s["campos"], g["dL_dcolors"], fw["clamped"], fw["radii"], "clamped")


def test_dropin_autograd_matches_oracle():
    """Through GaussianRasterizer.forward + loss.backward(), the way gaussian_renderer.render() drives it."""
    from hip_helpers import DGR, t
    P, W, H = 800, 96, 64
    s = random_gaussians(P, seed=21, W=W, H=H)
    rs = DGR.GaussianRasterizationSettings(image_height=H, image_width=W, tanfovx=s["tanfovx"], tanfovy=s["tanfovy"],
                                           bg=t(s["bg"]), scale_modifier=1.0, viewmatrix=t(s["viewmatrix"]),
                                           projmatrix=t(s["projmatrix"]), sh_degree=3, campos=t(s["campos"]),
                                           prefiltered=False, debug=False)
    rast = DGR.GaussianRasterizer(rs)
    means3D = t(s["means3D"]).requires_grad_(True)
    means2D = torch.zeros_like(means3D, requires_grad=True)
    opac = t(s["opacities"]).requires_grad_(True)
    shs = t(s["shs"]).requires_grad_(True)
    scales = t(s["scales"]).requires_grad_(True)
    rots = t(s["rotations"]).requires_grad_(True)
    img, radii, depth = rast(means3D=means3D, means2D=means2D, shs=shs, opacities=opac, scales=scales, rotations=rots)
    wgt = torch.linspace(0.5, 1.5, 3 * H * W, device="cuda").view(3, H, W)
    (img * wgt).sum().backward()
    st = _oracle(s)
    go = ro.backward(st, wgt.cpu().numpy())
    assert _relerr(means3D.grad.cpu().numpy(), go["dL_dmeans3D"]) <= GRAD_REL_TOL
    assert _relerr(means2D.grad.cpu().numpy(), go["dL_dmeans2D"]) <= GRAD_REL_TOL
    assert _relerr(opac.grad.cpu().numpy(), go["dL_dopacity"]) <= GRAD_REL_TOL
    assert _relerr(shs.grad.cpu().numpy(), go["dL_dsh"]) <= GRAD_REL_TOL
    assert _relerr(scales.grad.cpu().numpy(), go["dL_dscales"]) <= GRAD_REL_TOL
    assert _relerr(rots.grad.cpu().numpy(), go["dL_drotations"]) <= GRAD_REL_TOL
    np.testing.assert_array_equal(radii.cpu().numpy(), st.radii)
    with pytest.raises(Exception):
        rast(means3D=means3D, means2D=means2D, opacities=opac, scales=scales, rotations=rots)  # neither shs nor colours
    vis = rast.markVisible(means3D.detach())
    np.testing.assert_array_equal(vis.cpu().numpy(), s["means3D"][:, 2] > 0.2)


@pytest.mark.parametrize("P,W,H,seed", [(200_000, 960, 540, 33), (1_000_000, 1920, 1080, 34), (4_000_000, 1920, 1080, 35)],
                         ids=["config2_200k_960x540", "config3_1M_1920x1080", "config5_4M_1920x1080"])
def test_full_size_properties(P, W, H, seed):
    """BASELINE configs[1], configs[2] and configs[4] (per-GPU model of the camera-batch shard) sizes: size-independent properties instead of the oracle (which would need
    minutes per frame there).  Binning: the instance counts agree three ways, the tile ranges partition the list and
    every tile's list is strictly sorted by (depth bits, index).  Compositing: weights + final transmittance = 1.
    Determinism: same inputs, same bits.  Backward: every gradient is linear in dL/dpixels."""
    from hip_helpers import hip_backward, hip_forward
    s = random_gaussians(P, seed=seed, W=W, H=H, scale=(-6.0, -4.5))
    fw = hip_forward(s)
    R = fw["R"]
    assert R == int(fw["tile_counts"].sum()) <= int(fw["tiles_touched"].sum())
    # binning whole rectangles like the reference: the count is the sum of the rectangles; culling the instances that cannot
    # reach 1/255 in their tile changed no pixel and no transmittance, bit for bit
    fw_all = hip_forward(s, keep_all_tiles=True)
    assert fw_all["R"] == int(fw_all["tiles_touched"].sum()) == int(fw_all["tile_counts"].sum()) and R < fw_all["R"]
    for k in ("color", "depth", "final_T", "radii"):
        np.testing.assert_array_equal(fw[k], fw_all[k])
    pl, rg = fw["point_list"], fw["ranges"]
    dbits = fw["depths"].view(np.uint32)
    pos = 0
    for tile in range(rg.shape[0]):
        a, b = rg[tile]
        if a == b:
            continue
        assert a == pos
        key = (dbits[pl[a:b]].astype(np.uint64) << np.uint64(32)) | pl[a:b].astype(np.uint64)
        assert (np.diff(key.astype(np.int64)) > 0).all()      # strictly sorted by (depth bits, idx)
        pos = b
    assert pos == R
    # weights + T == 1 with unit colours / zero background
    s1 = dict(s, bg=np.zeros(3, np.float32))
    fw1 = hip_forward(s1, colors_precomp=np.ones((P, 3), np.float32))
    np.testing.assert_allclose(fw1["color"][0].reshape(-1) + fw1["final_T"], 1.0, atol=3e-5)
    # idempotence: same inputs, same bits
    fw2 = hip_forward(s)
    np.testing.assert_array_equal(fw2["point_list"], pl)
    np.testing.assert_array_equal(fw2["color"], fw["color"])
    # backward linearity: doubling dL/dpixels doubles every gradient (a power of two: exact up to the order of the atomics)
    rng = np.random.default_rng(seed)
    dcol = rng.standard_normal((3, H, W)).astype(np.float32)
    g1 = hip_backward(fw, dcol)
    g2 = hip_backward(fw, 2.0 * dcol)
    g_all = hip_backward(fw_all, dcol)
    for k in g1:
        scale = float(np.abs(g1[k]).max())
        assert np.isfinite(g1[k]).all() and scale > 0, k
        assert np.abs(g2[k] - 2.0 * g1[k]).max() <= 2e-5 * scale, (k, float(np.abs(g2[k] - 2.0 * g1[k]).max()), scale)
        # same per-pixel arithmetic with or without the cull; only the order of the float atomics can differ
        assert np.abs(g_all[k] - g1[k]).max() <= 2e-5 * scale, (k, float(np.abs(g_all[k] - g1[k]).max()), scale)


@pytest.mark.parametrize("seed,P,W,H,kw,opacity", [
    (40, 3000, 160, 96, {}, None),
    (41, 900, 100, 50, dict(scale=(-3.0, -0.5)), 0.03),      # large faint splats: most of each rectangle is out of reach
    (42, 20000, 320, 180, dict(scale=(-5.0, -3.0)), None),
    (43, 500, 64, 48, dict(scale=(-2.5, -0.5)), 0.004),      # opacity barely above 1/255: reach shrinks to the very centre
    (44, 500, 64, 48, {}, 0.0039),                           # below 1/255: nothing is binned at all
])
def test_tile_cull_changes_no_output(seed, P, W, H, kw, opacity):
    """MomRasterArgs.keep_all_tiles = 0 (default) against 1: the lists shrink; image, depth, transmittance and radii are
    bit-identical; the gradients agree up to the order of their float atomics."""
    from hip_helpers import hip_backward, hip_forward
    s = random_gaussians(P, seed=seed, W=W, H=H, **kw)
    if opacity is not None:
        s["opacities"][:] = opacity
    a, b = hip_forward(s), hip_forward(s, keep_all_tiles=True)
    assert a["R"] < b["R"] == int(b["tiles_touched"].sum())
    if opacity is not None and opacity < 1 / 255:
        assert a["R"] == 0
    for k in ("color", "depth", "final_T", "radii", "tiles_touched"):
        np.testing.assert_array_equal(a[k], b[k])
    np.testing.assert_array_equal(_last_contributor(a["n_contrib"], a["ranges"], a["point_list"], W, H),
                                  _last_contributor(b["n_contrib"], b["ranges"], b["point_list"], W, H))
    rng = np.random.default_rng(seed)
    dcol = rng.standard_normal((3, H, W)).astype(np.float32)
    ddep = (rng.standard_normal((1, H, W)) * 0.2).astype(np.float32)
    ga, gb = hip_backward(a, dcol, ddep), hip_backward(b, dcol, ddep)
    for k in ga:
        scale = max(float(np.abs(gb[k]).max()), 1e-30)
        assert np.abs(ga[k] - gb[k]).max() <= 2e-5 * scale, (k, float(np.abs(ga[k] - gb[k]).max()), scale)


def test_l1_epilogue_of_the_forward_equals_the_l1_kernel():
    """MomRasterArgs.l1_target / l1_grad / l1_sums: the compositing forward leaves the gradient image mom_l1_loss_acc computes
    from the stored image (bit for bit) and adds the same two sums (another order of addition); with l1_partials it stores one
    pair per tile instead (every tile of the image, empty ones included), whose sum is the same value and reproducible."""
    import importlib
    from hip_helpers import N, t
    fs_mod = importlib.import_module("iclr2025_3d-mom_amd.fused_step")
    s = random_gaussians(4000, seed=77, W=176, H=100)
    W, H, P = s["W"], s["H"], 4000
    lib, st = N.lib(), N.current_stream()
    dev = "cuda"
    keep = {k: t(s[k]) for k in ("bg", "means3D", "opacities", "scales", "rotations", "viewmatrix", "projmatrix", "campos", "shs")}
    gt = torch.rand(3, H, W, device=dev)
    a = N.MomRasterArgs()
    a.P, a.D, a.M, a.W, a.H = P, 3, 16, W, H
    a.background, a.means3D, a.shs, a.opacities = keep["bg"].data_ptr(), keep["means3D"].data_ptr(), keep["shs"].data_ptr(), keep["opacities"].data_ptr()
    a.scales, a.rotations = keep["scales"].data_ptr(), keep["rotations"].data_ptr()
    a.viewmatrix, a.projmatrix, a.campos = keep["viewmatrix"].data_ptr(), keep["projmatrix"].data_ptr(), keep["campos"].data_ptr()
    a.scale_modifier, a.tan_fovx, a.tan_fovy = 1.0, s["tanfovx"], s["tanfovy"]
    geom = torch.empty(lib.mom_raster_geom_bytes(P), dtype=torch.uint8, device=dev)
    img = torch.empty(lib.mom_raster_image_bytes(W, H), dtype=torch.uint8, device=dev)
    radii = torch.empty(P, dtype=torch.int32, device=dev)
    nr_dev = torch.zeros(1, dtype=torch.int32, device=dev)
    nr_host = torch.zeros(1, dtype=torch.int32).pin_memory()

    tiles = ((W + 15) // 16) * ((H + 15) // 16)

    def forward(with_epilogue, partials=False):
        dimg = torch.full((3, H, W), float("nan"), device=dev)
        sums = torch.zeros(2, device=dev)
        part = torch.full((tiles, 2), float("nan"), device=dev)
        a.l1_target, a.l1_grad, a.l1_sums = (gt.data_ptr(), dimg.data_ptr(), sums.data_ptr()) if with_epilogue else (None, None, None)
        a.l1_partials = None
        if partials:                     # per-tile pairs instead of the two contended sums (l1_sums may then be null)
            a.l1_sums, a.l1_partials = None, part.data_ptr()
        N.check(lib.mom_raster_forward_geometry(C.byref(a), geom.data_ptr(), img.data_ptr(), radii.data_ptr(), nr_dev.data_ptr(),
                                                nr_host.data_ptr(), st), "geometry")
        torch.cuda.synchronize()
        R = int(nr_host[0])
        binning = torch.empty(lib.mom_raster_binning_bytes(P, W, H, R), dtype=torch.uint8, device=dev)
        color, depth = torch.empty(3, H, W, device=dev), torch.empty(1, H, W, device=dev)
        N.check(lib.mom_raster_forward_render(C.byref(a), geom.data_ptr(), binning.data_ptr(), R, img.data_ptr(), color.data_ptr(),
                                              depth.data_ptr(), None, st), "render")
        if not with_epilogue:
            N.check(lib.mom_l1_loss_acc(3 * H * W, color.data_ptr(), gt.data_ptr(), dimg.data_ptr(), sums.data_ptr(), st), "l1")
        torch.cuda.synchronize()
        return color, dimg, (part.sum(0) if partials else sums)

    c0, d0, s0 = forward(False)
    c1, d1, s1 = forward(True)
    c2, d2, s2 = forward(True, partials=True)
    c3, d3, s3 = forward(True, partials=True)
    assert torch.equal(c0, c2) and torch.equal(d0, d2)
    assert torch.equal(s2, s3), "per-tile pairs added in a fixed order: the same bits every time"
    np.testing.assert_allclose(s2.cpu().numpy(), s0.cpu().numpy(), rtol=2e-6)
    assert torch.equal(c0, c1) and torch.equal(d0, d1) and float(d1.abs().max()) == pytest.approx(1.0 / (3 * H * W))
    np.testing.assert_allclose(s1.cpu().numpy(), s0.cpu().numpy(), rtol=2e-6)
    ref = (c0 - gt).double()
    np.testing.assert_allclose(s1.cpu().numpy(), [float(ref.abs().sum()), float((ref * ref).sum())], rtol=2e-6)
    # l1_grad_scale (a camera-batch shard's 1 / world): the gradient image a scaling pass behind the forward would leave, the sums untouched
    for w in (2, 3, 8):
        a.l1_grad_scale = 1.0 / w
        c4, d4, s4 = forward(True, partials=True)
        assert torch.equal(c4, c0) and torch.equal(d4, d0 * (1.0 / w)) and torch.equal(s4, s2), w
    a.l1_grad_scale = 0.0


def test_status_post_reports_the_frames_own_overflow_with_its_serial():
    """MomRasterArgs.status_post: the compositing forward leaves (serial << 32) | status bits in a pinned host word -- bit 0 set
    exactly when this frame's instances did not fit `capacity` -- so that a host running ahead needs no copy and no event per frame."""
    from hip_helpers import N, t
    s = random_gaussians(3000, seed=5, W=160, H=96)
    W, H, P = s["W"], s["H"], 3000
    lib, st = N.lib(), N.current_stream()
    dev = "cuda"
    keep = {k: t(s[k]) for k in ("bg", "means3D", "opacities", "scales", "rotations", "viewmatrix", "projmatrix", "campos", "shs")}
    a = N.MomRasterArgs()
    a.P, a.D, a.M, a.W, a.H = P, 3, 16, W, H
    a.background, a.means3D, a.shs, a.opacities = keep["bg"].data_ptr(), keep["means3D"].data_ptr(), keep["shs"].data_ptr(), keep["opacities"].data_ptr()
    a.scales, a.rotations = keep["scales"].data_ptr(), keep["rotations"].data_ptr()
    a.viewmatrix, a.projmatrix, a.campos = keep["viewmatrix"].data_ptr(), keep["projmatrix"].data_ptr(), keep["campos"].data_ptr()
    a.scale_modifier, a.tan_fovx, a.tan_fovy = 1.0, s["tanfovx"], s["tanfovy"]
    geom = torch.empty(lib.mom_raster_geom_bytes(P), dtype=torch.uint8, device=dev)
    img = torch.empty(lib.mom_raster_image_bytes(W, H), dtype=torch.uint8, device=dev)
    radii = torch.empty(P, dtype=torch.int32, device=dev)
    nr_dev = torch.zeros(1, dtype=torch.int32, device=dev)
    nr_host = torch.zeros(1, dtype=torch.int32).pin_memory()
    word = torch.zeros(2, dtype=torch.int64).pin_memory()
    color, depth = torch.empty(3, H, W, device=dev), torch.empty(1, H, W, device=dev)

    def frame(serial, capacity, slot):
        a.status_post, a.status_serial = word.data_ptr() + 8 * slot, serial
        N.check(lib.mom_raster_forward_geometry(C.byref(a), geom.data_ptr(), img.data_ptr(), radii.data_ptr(), nr_dev.data_ptr(),
                                                nr_host.data_ptr(), st), "geometry")
        torch.cuda.synchronize()
        R = int(nr_host[0])
        cap = R if capacity is None else capacity
        binning = torch.empty(lib.mom_raster_binning_bytes(P, W, H, cap), dtype=torch.uint8, device=dev)
        N.check(lib.mom_raster_forward_render(C.byref(a), geom.data_ptr(), binning.data_ptr(), cap, img.data_ptr(), color.data_ptr(),
                                              depth.data_ptr(), None, st), "render")
        torch.cuda.synchronize()
        return R, int(word[slot])

    R, v = frame(7, None, 0)
    assert R > 1000 and (v >> 32) & 0xFFFFFFFF == 7 and (v & 1) == 0
    R, v = frame(0xFFFFFFF0, R // 4, 1)                      # a quarter of what the frame needs: flagged, under its own serial
    assert (v >> 32) & 0xFFFFFFFF == 0xFFFFFFF0 and (v & 1) == 1
    assert (int(word[0]) >> 32) & 0xFFFFFFFF == 7             # the other slot is untouched


def test_tile_cull_with_degenerate_splats():
    """Opacity 0, negative, NaN, above 1; needle-thin and huge splats; a NaN position: whatever the compositing kernels make of
    them, they make the same of them with and without the tile cull (bit patterns compared, NaNs included)."""
    from hip_helpers import hip_forward
    P, W, H = 600, 96, 64
    s = random_gaussians(P, seed=91, W=W, H=H)
    op = s["opacities"]
    op[0:40] = 0.0
    op[40:80] = -0.3
    op[80:90] = np.nan
    op[90:130] = 1.7
    op[130:170] = 1.0 / 255.0
    op[170:210] = np.nextafter(np.float32(1.0 / 255.0), np.float32(0))
    s["scales"][210:250, 0] = -9.0           # exp(-9): needles
    s["scales"][250:270] = 1.5               # splats larger than the image
    s["means3D"][270:274, 0] = np.nan
    a, b = hip_forward(s), hip_forward(s, keep_all_tiles=True)
    assert a["R"] <= b["R"]
    for k in ("color", "depth", "final_T"):
        np.testing.assert_array_equal(a[k].view(np.uint32), b[k].view(np.uint32))
    np.testing.assert_array_equal(a["radii"], b["radii"])


@pytest.mark.parametrize("seed,P,W,H,kw", [(51, 6000, 208, 112, {}), (52, 12800, 208, 112, {}), (53, 20000, 160, 96, {})])
def test_tile_sort_inside_the_compositing_forward_changes_nothing(seed, P, W, H, kw, monkeypatch):
    """The compositing forward sorts the tiles of up to 1536 keys itself (csrc/raster_render.hip); MOM_RENDER_SORT=0 leaves every
    tile to the binning's sort launches.  Same per-tile lists, same images, same counters, bit for bit; the second scene has
    tiles on both sides of the 1536-key limit."""
    from hip_helpers import hip_forward
    s = random_gaussians(P, seed=seed, W=W, H=H, **kw)
    monkeypatch.setenv("MOM_RENDER_SORT", "0")
    a = hip_forward(s)
    monkeypatch.setenv("MOM_RENDER_SORT", "1")
    b = hip_forward(s)
    assert a["R"] == b["R"] > 0
    n = (a["ranges"][:, 1] - a["ranges"][:, 0]).astype(np.int64)
    if P == 12800:       # this scene has tiles on both sides of the limit (the first only below, the third only above)
        assert n.max() > 1536 > n[n > 0].min(), (n.min(), n.max())
    for k in ("ranges", "point_list", "color", "depth", "final_T", "n_contrib", "radii"):
        np.testing.assert_array_equal(a[k], b[k])


# ---- under rotated and translated cameras (scenes.pose): every test above sees the identity view matrix and campos = 0, under
# which a transposed view index, a forgotten translation, mean - campos against the mean, and a contracted dot product all give
# the same numbers.  Same helpers, same gates.
# Measured on an MI355X (tools/parity_stats.py posed; every pose, both binnings, the mid-size and the beyond-the-clamp cases):
# image mean L1 4.6e-9 .. 3.6e-8 (gate 1e-6), max 2.3e-5 with at most 1 pixel above 1e-5 (a counted threshold exception),
# n_contrib and last contributors identical, final_T mean within 6.1e-11; gradient norms within 1.2e-5 (gate 5e-5), no row
# above 2e-5 of its tensor's scale, worst row 1.4e-5.

ALL_POSES = ("identity",) + POSES


@pytest.mark.parametrize("pose_name", POSES)
@pytest.mark.parametrize("seed,P,W,H,kw", [
    (201, 5000, 256, 256, {}),
    (202, 700, 100, 50, dict(scale=(-3.0, -0.5))),   # ragged image, large splats
])
def test_forward_parity_under_a_pose(seed, P, W, H, kw, pose_name):
    """Both binnings against one oracle frame.  ref17 is the reference's own camera 17 (golden/g5_cameras.npz): its R is the
    identity, it brings a translation and fovx == fovy on a non-square image; yaw90 and general carry the rotation."""
    from hip_helpers import hip_forward
    ro.set_threads(1)
    s = posed_gaussians(P, pose_name, seed=seed, W=W, H=H, **kw)
    st = _oracle(s)
    assert (st.radii > 0).sum() > P // 2
    for keep_all_tiles in (True, False):
        _cmp_forward(hip_forward(s, keep_all_tiles=keep_all_tiles), st, P)


def test_forward_parity_mid_size_under_a_general_pose():
    from hip_helpers import hip_forward
    ro.set_threads(16)
    P = 100000
    s = posed_gaussians(P, "general", seed=207, W=480, H=270, scale=(-5.5, -3.5))
    st = _oracle(s)
    for keep_all_tiles in (True, False):
        _cmp_forward(hip_forward(s, keep_all_tiles=keep_all_tiles), st, P)


@pytest.mark.parametrize("pose_name", POSES)
@pytest.mark.parametrize("seed,P,W,H,kw", [(210, 1500, 128, 96, {}), (212, 5000, 256, 256, dict(scale=(-5.0, -3.0)))])
def test_backward_parity_under_a_pose(seed, P, W, H, kw, pose_name):
    """All eight gradient tensors, nonzero depth gradient, degree 3; the SH backward against float64 with the pose's campos."""
    ro.set_threads(1)
    s = posed_gaussians(P, pose_name, seed=seed, W=W, H=H, **kw)
    fw, st, g, go = _backward_case(s, seed, {}, {})
    assert float(np.abs(go["dL_ddepths"]).max()) > 0
    _check_sh_fp64(3, g["dL_dsh"], s["shs"], s["means3D"], s["campos"], g["dL_dcolors"], fw["clamped"], fw["radii"], pose_name)


@pytest.mark.parametrize("deg,seed", [(0, 220), (1, 225), (2, 222), (3, 223)])
def test_backward_parity_at_every_sh_degree_under_a_general_pose(deg, seed):
    s = posed_gaussians(1500, "general", seed=seed, W=128, H=96)
    assert float(np.abs(s["campos"]).min()) > 0.1
    kw = dict(sh_degree=deg)
    fw, st, g, go = _backward_case(s, seed, kw, kw)
    _check_sh_fp64(deg, g["dL_dsh"], s["shs"], s["means3D"], s["campos"], g["dL_dcolors"], fw["clamped"], fw["radii"], "general")


def test_backward_parity_precomputed_colors_under_a_general_pose():
    s = posed_gaussians(1200, "general", seed=230, W=96, H=64)
    cols = np.random.default_rng(230).uniform(0, 1, (1200, 3)).astype(np.float32)
    names = tuple(n for n in GRAD_NAMES if n != "dL_dsh")
    fw, st, g, go = _backward_case(s, 230, dict(colors_precomp=cols), dict(shs=None, colors_precomp=cols), names, feat=cols)
    assert float(np.abs(g["dL_dcolors"]).max()) > 0
    assert g["dL_dsh"].size == 0 or not g["dL_dsh"].any()


def test_backward_parity_precomputed_cov3d_under_a_general_pose():
    s = posed_gaussians(1200, "general", seed=231, W=96, H=64)
    cov = _oracle(s).cov3D
    names = tuple(n for n in GRAD_NAMES if n not in ("dL_dscales", "dL_drotations"))
    fw, st, g, go = _backward_case(s, 231, dict(cov3D_precomp=cov), dict(scales=None, rotations=None, cov3D_precomp=cov), names)
    assert float(np.abs(g["dL_dcov3D"]).max()) > 0
    for n in ("dL_dscales", "dL_drotations"):
        assert g[n].size == 0 or not g[n].any(), n
    _check_sh_fp64(3, g["dL_dsh"], s["shs"], s["means3D"], s["campos"], g["dL_dcolors"], fw["clamped"], fw["radii"], "cov3D")


def clamp_census(s, st, margin=1e-5):
    """Of the oracle's visible Gaussians, the fractions beyond the frustum clamp of computeCov2D (|t.x / t.z| > 1.3f tan(fovx/2),
    and the same in y), read off the oracle's own state: its pixel centre is ndc2Pix of t.x / (t.z tan(fovx/2)), so beyond the
    clamp is |ndc| > 1.3.  Asserts from float64 view-space coordinates that no visible Gaussian is within `margin` (relative) of
    the limit -- where a float32 evaluation may take the other branch of the hard threshold -- and, with that, that the float64
    coordinates sort every visible Gaussian to the same side as the oracle's state does."""
    vis = st.radii > 0
    pv = view_space(s["means3D"], s["viewmatrix"])[vis]
    out = []
    for ax, tanfov, size in ((0, s["tanfovx"], s["W"]), (1, s["tanfovy"], s["H"])):
        lim = float(np.float32(1.3)) * tanfov
        r = np.abs(pv[:, ax] / pv[:, 2])
        assert (np.abs(r - lim) > margin * lim).all(), ("pick another seed: a Gaussian sits on the clamp limit", ax)
        ndc = (2.0 * st.means2D[vis, ax].astype(np.float64) + 1.0) / size - 1.0
        beyond = np.abs(ndc) > 1.3
        settled = np.abs(np.abs(ndc) - 1.3) > 1e-4        # (the pixel centre is a float32 of magnitude ~100: ndc to ~1e-7)
        np.testing.assert_array_equal(beyond[settled], (r > lim)[settled])
        out.append(float(beyond.mean()))
    return out


@pytest.mark.parametrize("pose_name,seed", [("identity", 242), ("general", 241)])
def test_parity_beyond_the_frustum_clamp(pose_name, seed):
    """Gaussians drawn out to 2.0 tan(fov) and large enough to reach the image from there: the clamped coordinate in the forward's
    Jacobian and the zero gradient multiplier of the backward (computeCov2D, forward.cu:86-90 / backward.cu:171-176), which
    random_gaussians' default spread of exactly 1.3 never takes."""
    from hip_helpers import hip_forward
    P, W, H = 1500, 128, 96
    s = posed_gaussians(P, pose_name, seed=seed, W=W, H=H, spread=2.0, scale=(-3.0, -0.5))
    fw, st, g, go = _backward_case(s, seed, {}, {})
    fx, fy = clamp_census(s, st)
    assert fx >= 0.05 and fy >= 0.05, (fx, fy)
    _cmp_forward(hip_forward(s, keep_all_tiles=True), st, P)


@pytest.mark.parametrize("seed,P,W,H", [(250, 1500, 128, 96)])
def test_rigid_motion_of_scene_and_camera_on_the_hip_path(seed, P, W, H):
    """scenes.rigid_move at SH degree 0: the identity-pose scene, and the same scene moved together with its camera by the
    `general` pose, are one frame (tests/test_oracle_torch.py shows it for the oracle in float64).  Here the moved inputs are
    rounded to float32, so the two HIP frames are compared at the image and gradient gates, the integers up to the counted
    exceptions, and the gradients after turning them back: dL/dmean = R^T dL/dmean', dL/dq = L(q_R)^T dL/dq' in the plane
    orthogonal to q (the reference uses q unnormalised; the derivative along q does not turn, see the oracle test)."""
    from hip_helpers import hip_backward, hip_forward
    s0 = random_gaussians(P, seed=seed, W=W, H=H)
    kp = pose("general")
    s1 = rigid_move(s0, kp["R"], kp["T"])
    rng = np.random.default_rng(seed)
    dcol = rng.normal(size=(3, H, W)).astype(np.float32)
    ddep = (rng.normal(size=(1, H, W)) * 0.2).astype(np.float32)
    st0 = _oracle(s0, sh_degree=0)
    fw0, fw1 = hip_forward(s0, sh_degree=0), hip_forward(s1, sh_degree=0)
    _cmp_forward(fw0, st0, P)
    for k in ("radii", "tiles_touched"):
        assert int((fw0[k] != fw1[k]).sum()) <= _allowed(P), k
    # every pixel's last contributor (a position in a culled list means nothing across two frames; the Gaussian it names does)
    bad = np.nonzero(_last_contributor(fw0["n_contrib"], fw0["ranges"], fw0["point_list"], W, H)
                     != _last_contributor(fw1["n_contrib"], fw1["ranges"], fw1["point_list"], W, H))[0]
    assert len(bad) <= _allowed(W * H), len(bad)
    for p in bad:
        assert _near_threshold(st0, int(p % W), int(p // W), W), ("last contributor differs without a threshold pair", p)
    _assert_image(fw1["color"], fw0["color"], st0, "color")
    dscale = max(1.0, float(st0.depths.max()))
    _assert_image(fw1["depth"] / dscale, fw0["depth"] / dscale, st0, "depth")
    g0, g1 = hip_backward(fw0, dcol, ddep), hip_backward(fw1, dcol, ddep)
    back = dict(g1)
    back["dL_dmeans3D"] = (g1["dL_dmeans3D"].astype(np.float64) @ kp["R"]).astype(np.float32)
    q0 = s0["rotations"].astype(np.float64)
    tangent = lambda g: g - (g * q0).sum(1, keepdims=True) * q0
    back["dL_drotations"] = tangent(g1["dL_drotations"].astype(np.float64) @ quat_left(quat_of(kp["R"]))).astype(np.float32)
    ref = dict(g0)
    ref["dL_drotations"] = tangent(g0["dL_drotations"].astype(np.float64))
    names = tuple(n for n in GRAD_NAMES if n != "dL_dcov3D")        # (a symmetric tensor: it turns as R . R^T; dL/dscale and dL/dq carry it)
    _cmp_grads(back, ref, st0, names, what="rigid")


@pytest.mark.parametrize("P", [1, 63, 64, 65, 20011])
@pytest.mark.parametrize("pose_name", ALL_POSES)
def test_mark_visible_against_the_oracle(pose_name, P):
    """mom_mark_visible through the `_C` boundary: whole and partial workgroups, a quarter of the means within 1e-4 .. 1e-2 of
    the 0.2 cull on either side of it."""
    from hip_helpers import RC, t
    s, want = near_plane_scene(P, pose_name, seed=260 + P)
    if P == 1:       # near_plane_scene's first Gaussian is behind the camera: put the lone one in front, then behind
        for z, seen in ((0.21, True), (0.19, False)):
            m = to_world(np.array([[0.01, -0.02, z]]), **pose(pose_name)).astype(np.float32)
            got = RC.mark_visible(t(m), t(s["viewmatrix"]), t(s["projmatrix"])).cpu().numpy()
            assert got.dtype == np.bool_ and got.tolist() == [seen] == ro.mark_visible(m, s["viewmatrix"], s["projmatrix"]).tolist()
        return
    got = RC.mark_visible(t(s["means3D"]), t(s["viewmatrix"]), t(s["projmatrix"])).cpu().numpy()
    assert got.dtype == np.bool_
    np.testing.assert_array_equal(got, ro.mark_visible(s["means3D"], s["viewmatrix"], s["projmatrix"]))
    np.testing.assert_array_equal(got, want)
    assert 0 < want.sum() < P
