"""The CPU oracle and the HIP kernels against the reference's OWN kernels: forward.cu, backward.cu, rasterizer_impl.cu and
simple_knn.cu of the reference, built by hipcc for gfx950 (oracle/ref_gpu.py; oracle/_ref/ is git-ignored and built by build()
from a reference checkout) and run on the same inputs as oracle/raster_oracle.c and libmom4d.

Every case runs three ways: R = the reference's kernels, O = the CPU oracle, K = our kernels.  R vs O pins the oracle, which
every other rasterizer test of this suite compares with; K vs R holds our kernels to the reference directly.  The gates are
those K vs O has today (tests/raster_compare.py), none new: radii, tiles_touched, num_rendered, ranges, point_list and clamp
flags equal, depths / means2D / conics bit-equal on visible splats, images, n_contrib and gradient rows inside the counted
threshold exceptions.  R_fma is the same reference source under the compiler's default contraction (as a CUDA build contracts
too): held to the tolerance gates only, its integer outputs to the counted cap instead of to equality.

Each test prints its figures (`PINNED {json}` lines, pytest -s) before it asserts; tools/pinned_table.py turns a log of them into
the tables of oracle/ref_gpu/PINNED.md.
"""
import importlib
import json

import numpy as np
import pytest
import torch

from oracle import raster_oracle as ro
from oracle import ref_gpu as rg
from raster_compare import GRAD_NAMES, _allowed, _assert_image, _cmp_forward, _cmp_grads, _relerr
from scenes import POSES, clamp_some_channels, near_plane_scene, pose, posed_gaussians, random_gaussians, to_world

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not rg.available("off"), reason=f"{rg.lib_path('off')} is absent: build() found no reference checkout")]

STATE_KEYS = ("radii", "tiles_touched", "depths", "means2D", "conic_opacity", "ranges", "point_list", "clamped", "rgb", "n_contrib",
              "final_T")
ALL_GRADS = GRAD_NAMES + ("dL_dconic", "dL_ddepths")      # R and O expose all ten; K the eight of GRAD_NAMES


def _record(case, pair, **figures):
    print("PINNED " + json.dumps(dict(case=case, pair=pair, **figures)))


def _call(forward, s, kw):
    args = dict(shs=s.get("shs"), sh_degree=3, scales=s["scales"], rotations=s["rotations"])
    args.update(kw)
    return forward(s["means3D"], s["opacities"], s["viewmatrix"], s["projmatrix"], s["campos"], s["W"], s["H"], s["tanfovx"],
                   s["tanfovy"], s["bg"], **args)


def _as_forward(st):
    """A reference (or oracle) state in the shape hip_helpers.hip_forward returns: the left-hand side of _cmp_forward."""
    fw = {k: st[k] for k in STATE_KEYS}
    fw.update(R=st.num_rendered, color=st.out_color, depth=st.out_depth, keep_all_tiles=True)
    return fw


def _hip_kw(kw):
    return {k: v for k, v in kw.items() if k in ("sh_degree", "scale_modifier", "colors_precomp", "cov3D_precomp")}


# ---- the cases: name -> builder of (scene, keyword arguments of the oracle's forward, gradient names or None, seed) ----------

def _precomp_colors(seed, P, W, H):
    s = random_gaussians(P, seed=seed, W=W, H=H)
    cols = np.random.default_rng(seed).uniform(0, 1, (P, 3)).astype(np.float32)
    return s, dict(shs=None, colors_precomp=cols)


def _precomp_cov3d(seed, P, W, H):
    s = random_gaussians(P, seed=seed, W=W, H=H)
    cov = _call(rg.forward, s, {}).cov3D                 # the reference's own covariances
    return s, dict(scales=None, rotations=None, cov3D_precomp=cov)


def _oversized_bucket():
    """The scene of test_oversized_tile_bucket_uses_global_sort_path: more than 8192 instances in one tile, 500 exact depth ties."""
    s = random_gaussians(9000, seed=9, W=32, H=32, scale=(-5.5, -4.5))
    s["means3D"][:, 0] *= 0.05
    s["means3D"][:, 1] *= 0.05
    s["means3D"][100:, 2] = np.abs(s["means3D"][100:, 2]) + 0.5
    s["means3D"][2000:2500, 2] = 3.0
    s["opacities"][:] = 0.02
    return s


def _all_behind():
    s = random_gaussians(10, seed=1, W=48, H=32)
    s["means3D"][:, 2] = -1.0
    return s


def _on_the_near_plane():
    """Under the identity view the view-space depth is the mean's z, exactly: eight splats AT float32(0.2), which in_frustum's
    `p_view.z <= 0.2f` culls (auxiliary.h:154), and eight one ulp in front of it, which it keeps; all in the middle of the image, and small
    enough in world units to stay a few pixels wide at that depth.  (At scale (-6, -5) the kept eight cover the whole image at
    transmittance ~0.55 and this becomes a test of eight-factor products over every pixel: R vs O and K vs R pass all the same, R_fma's
    final_T is then 1.0012e-8 from O's in the mean against the 1e-8 gate -- 1 ulp of 0.55 on a sixth of the pixels.)"""
    s = random_gaussians(64, seed=5, W=48, H=32, scale=(-8.0, -7.0))
    s["means3D"][:16, :2] = 0.0
    s["means3D"][:8, 2] = np.float32(0.2)
    s["means3D"][8:16, 2] = np.nextafter(np.float32(0.2), np.float32(1.0))
    return s


def _empty():
    s = random_gaussians(10, seed=1, W=48, H=32)
    return {k: (v[:0] if isinstance(v, np.ndarray) and v.shape[:1] == (10,) else v) for k, v in s.items()}


NO_SH = tuple(n for n in GRAD_NAMES if n != "dL_dsh")
NO_SCALE_ROT = tuple(n for n in GRAD_NAMES if n not in ("dL_dscales", "dL_drotations"))

FORWARD_CASES = {
    "s0_2000_128x96": lambda: (random_gaussians(2000, seed=0, W=128, H=96), {}),
    "s2_700_100x50_large": lambda: (random_gaussians(700, seed=2, W=100, H=50, scale=(-3.0, -0.5)), {}),
    "s3_64_33x17": lambda: (random_gaussians(64, seed=3, W=33, H=17), {}),
    "s1_5000_256x256": lambda: (random_gaussians(5000, seed=1, W=256, H=256), {}),
    **{f"pose_{p}": (lambda p=p: (posed_gaussians(2000, p, seed=0, W=128, H=96), {})) for p in POSES},
    "exactly_on_the_near_plane": lambda: (_on_the_near_plane(), {}),
    "near_plane_general": lambda: (near_plane_scene(1500, "general", seed=270)[0], {}),
    "beyond_clamp_identity": lambda: (posed_gaussians(1500, "identity", seed=242, W=128, H=96, spread=2.0, scale=(-3.0, -0.5)), {}),
    "beyond_clamp_general": lambda: (posed_gaussians(1500, "general", seed=241, W=128, H=96, spread=2.0, scale=(-3.0, -0.5)), {}),
    **{f"sh{d}_scale0.7": (lambda d=d: (random_gaussians(1500, seed=7, W=96, H=80), dict(sh_degree=d, scale_modifier=0.7)))
       for d in (0, 1, 2, 3)},
    "colors_precomp": lambda: _precomp_colors(8, 1200, 80, 64),
    "cov3D_precomp": lambda: _precomp_cov3d(8, 1200, 80, 64),
    "clamped_channels": lambda: (clamp_some_channels(random_gaussians(2000, seed=93, W=128, H=96), seed=93), {}),
    "oversized_bucket_depth_ties": lambda: (_oversized_bucket(), {}),
    "all_behind_the_camera": lambda: (_all_behind(), {}),
    "P0": lambda: (_empty(), {}),
}

BACKWARD_CASES = {          # name -> (builder, gradient names held between all three, seed of dL_dpix / dL_dpix_depth)
    "s10_1500_128x96": (lambda: (random_gaussians(1500, seed=10, W=128, H=96), {}), GRAD_NAMES, 10),
    "s11_400_70x45_large": (lambda: (random_gaussians(400, seed=11, W=70, H=45, scale=(-3.0, -1.0)), {}), GRAD_NAMES, 11),
    "pose_general": (lambda: (posed_gaussians(1500, "general", seed=210, W=128, H=96), {}), GRAD_NAMES, 210),
    "colors_precomp": (lambda: _precomp_colors(80, 1200, 96, 64), NO_SH, 80),
    "cov3D_precomp": (lambda: _precomp_cov3d(84, 1200, 96, 64), NO_SCALE_ROT, 84),
    "clamped_channels": (lambda: (clamp_some_channels(random_gaussians(2000, seed=93, W=128, H=96), seed=93), {}), GRAD_NAMES, 93),
}

_CACHE = {}


def _states(kind, name):
    """One scene, its R, O and R_fma states (and, for a backward case, the three gradient sets), computed once per module run
    and shared, unchanged, by the tests of the case."""
    key = (kind, name)
    if key not in _CACHE:
        ro.set_threads(1)
        if kind == "fwd":
            build, names, seed = FORWARD_CASES[name], None, None
        else:
            build, names, seed = BACKWARD_CASES[name]
        s, kw = build()
        c = dict(s=s, kw=kw, names=names, P=s["means3D"].shape[0], feat=kw.get("colors_precomp"))
        c["R"], c["O"], c["Rf"] = _call(rg.forward, s, kw), _call(ro.forward, s, kw), _call(rg.forward, s, dict(kw, variant="fma"))
        if names is not None:
            rng = np.random.default_rng(seed)          # as test_backward_parity draws them
            c["dcol"] = rng.normal(size=(3, s["H"], s["W"])).astype(np.float32)
            c["ddep"] = (rng.normal(size=(1, s["H"], s["W"])) * 0.2).astype(np.float32)
            c["gR"], c["gO"], c["gRf"] = (b(c[k], c["dcol"], c["ddep"]) for b, k in ((rg.backward, "R"), (ro.backward, "O"), (rg.backward, "Rf")))
        _CACHE[key] = c
    return _CACHE[key]


# ---- figures (printed before anything is asserted) and the two comparisons ------------------------------------------------

def _forward_figures(case, pair, fw, st):
    f = dict(R=[int(fw["R"]), int(st.num_rendered)])
    for k in ("radii", "tiles_touched", "clamped"):
        f[k] = int((fw[k] != st[k]).sum()) if k != "clamped" else int((fw[k][st.radii > 0] != st[k][st.radii > 0]).sum())
    if fw["keep_all_tiles"]:
        same = len(fw["point_list"]) == len(st.point_list)
        f["point_list"] = int((fw["point_list"] != st.point_list).sum()) if same else "length"
        f["n_contrib"] = int((fw["n_contrib"].reshape(-1) != st.n_contrib.reshape(-1)).sum())
    vis = (st.radii > 0) & (fw["radii"] > 0)
    f["geom_bits"] = int(sum((fw[k][vis].view(np.uint32) != st[k][vis].view(np.uint32)).sum() for k in ("depths", "means2D", "conic_opacity")))
    d = np.abs(fw["color"] - st.out_color)
    f["img_mean"], f["img_max"], f["img_over"] = float(d.mean()), float(d.max(initial=0.0)), int((d.max(axis=0) > 1e-5).sum())
    f["depth_max"] = float(np.abs(fw["depth"] - st.out_depth).max(initial=0.0))
    f["final_T_mean"] = float(np.abs(fw["final_T"] - st.final_T).mean()) if st.final_T.size else 0.0
    _record(case, pair, **f)


def _grad_figures(case, pair, g, go, names):
    rel, row = {}, {}
    for n in names:
        a, b = g[n], go[n].reshape(g[n].shape)
        rel[n] = _relerr(a, b)
        row[n] = float((np.abs(a - b).reshape(a.shape[0], -1).max(axis=1) / max(float(np.abs(b).max()), 1e-30)).max(initial=0.0))
    wn, wr = max(rel, key=rel.get), max(row, key=row.get)
    _record(case, pair, grad_norm=[wn, rel[wn]], grad_row=[wr, row[wr]])


def _cmp_contracted(fw, st, P):
    """R_fma against O: the tolerance gates -- images, final_T -- and the integer outputs under the counted cap."""
    N = st.n_contrib.size
    for k in ("radii", "tiles_touched"):
        assert int((fw[k] != st[k]).sum()) <= _allowed(P), k
    assert int((fw["n_contrib"].reshape(-1) != st.n_contrib.reshape(-1)).sum()) <= _allowed(N)
    _assert_image(fw["color"], st.out_color, st, "color")
    dscale = max(1.0, float(st.depths.max()))
    _assert_image(fw["depth"] / dscale, st.out_depth / dscale, st, "depth")
    assert np.abs(fw["final_T"] - st.final_T).mean() <= 1e-8


def _pins_the_oracle(name, c):
    """R vs O at K vs O's gates, and what only these two expose: the inclusive scan, and the sorted 64-bit keys -- which hold
    the oracle's order among equal depths to hipCUB's stable radix sort of the reference's own keys."""
    R, O, P = c["R"], c["O"], c["P"]
    _forward_figures(name, "R-O", _as_forward(R), O)
    if P == 0:
        assert R.num_rendered == O.num_rendered == 0 and not R.out_color.any() and not O.out_color.any()
        return
    _cmp_forward(_as_forward(R), O, P, walked=False)
    np.testing.assert_array_equal(R.point_offsets, O.point_offsets)
    np.testing.assert_array_equal(R.point_list_keys, O.point_list_keys)
    np.testing.assert_array_equal(R.out_color.shape, O.out_color.shape)


def _kernels_match(name, c):
    """K vs R directly, under both binnings."""
    from hip_helpers import hip_forward
    out = {}
    for keep_all in (True, False):
        fw = hip_forward(c["s"], keep_all_tiles=keep_all, **_hip_kw(c["kw"]))
        if c["P"] == 0:
            assert fw["R"] == 0 and not fw["color"].any() and not fw["depth"].any()
            continue
        _forward_figures(name, "K-R" if keep_all else "Kculled-R", fw, c["R"])
        _cmp_forward(fw, c["R"], c["P"], feat=c["feat"], walked=False)
        out[keep_all] = fw
    return out


# ---- forward ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(FORWARD_CASES))
def test_forward_oracle_is_the_reference(name):
    c = _states("fwd", name)
    if name == "oversized_bucket_depth_ties":
        assert (c["R"].ranges[:, 1] - c["R"].ranges[:, 0]).max() > 8192
        depth_bits = c["R"].point_list_keys & np.uint64(0xFFFFFFFF)
        assert int((np.diff(depth_bits.astype(np.int64)) == 0).sum()) >= 499, "no equal keys: the tie order is not exercised"
    if name == "exactly_on_the_near_plane":
        assert not c["R"].radii[:8].any() and (c["R"].radii[8:16] > 0).all()
    if name == "all_behind_the_camera":
        assert c["R"].num_rendered == 0 and not c["R"].radii.any()
    _pins_the_oracle(name, c)


@pytest.mark.parametrize("name", list(FORWARD_CASES))
def test_forward_kernels_match_the_reference(name):
    _kernels_match(name, _states("fwd", name))


@pytest.mark.parametrize("name", list(FORWARD_CASES))
def test_forward_contracted_reference_stays_inside_the_tolerances(name):
    c = _states("fwd", name)
    _forward_figures(name, "Rfma-O", _as_forward(c["Rf"]), c["O"])
    if c["P"]:
        _cmp_contracted(_as_forward(c["Rf"]), c["O"], c["P"])


# ---- backward -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(BACKWARD_CASES))
def test_backward_oracle_is_the_reference(name):
    c = _states("bwd", name)
    names = c["names"] + ("dL_dconic", "dL_ddepths")
    _grad_figures("bwd/" + name, "R-O", c["gR"], c["gO"], names)
    _pins_the_oracle("bwd/" + name, c)
    assert float(np.abs(c["gR"]["dL_ddepths"]).max()) > 0 and float(np.abs(c["gR"]["dL_dconic"]).max()) > 0
    _cmp_grads(c["gR"], c["gO"], c["O"], names, what=name)
    for n in set(ALL_GRADS) - set(names):            # the tensors the case leaves out are zero on both sides
        assert not c["gR"][n].any() and not c["gO"][n].any(), n


@pytest.mark.parametrize("name", list(BACKWARD_CASES))
def test_backward_kernels_match_the_reference(name):
    from hip_helpers import hip_backward
    c = _states("bwd", name)
    fws = _kernels_match("bwd/" + name, c)
    for keep_all, fw in fws.items():
        g = hip_backward(fw, c["dcol"], c["ddep"])
        _grad_figures("bwd/" + name, "K-R" if keep_all else "Kculled-R", g, c["gR"], c["names"])
        _cmp_grads(g, c["gR"], c["R"], c["names"], what=(name, keep_all))


@pytest.mark.parametrize("name", list(BACKWARD_CASES))
def test_backward_contracted_reference_stays_inside_the_tolerances(name):
    c = _states("bwd", name)
    names = c["names"] + ("dL_dconic", "dL_ddepths")
    _forward_figures("bwd/" + name, "Rfma-O", _as_forward(c["Rf"]), c["O"])
    _grad_figures("bwd/" + name, "Rfma-O", c["gRf"], c["gO"], names)
    _cmp_contracted(_as_forward(c["Rf"]), c["O"], c["P"])
    _cmp_grads(c["gRf"], c["gO"], c["O"], names, what=name)


def test_kernels_match_the_reference_with_no_oracle_between():
    """(4, 20000, 320x180, small splats): forward under both binnings and backward, K vs R, both on the device."""
    from hip_helpers import hip_backward, hip_forward
    P, W, H = 20000, 320, 180
    s = random_gaussians(P, seed=4, W=W, H=H, scale=(-5.0, -3.0))
    R = _call(rg.forward, s, {})
    rng = np.random.default_rng(4)
    dcol = rng.normal(size=(3, H, W)).astype(np.float32)
    ddep = (rng.normal(size=(1, H, W)) * 0.2).astype(np.float32)
    gR = rg.backward(R, dcol, ddep)
    for keep_all in (True, False):
        fw = hip_forward(s, keep_all_tiles=keep_all)
        g = hip_backward(fw, dcol, ddep)
        pair = "K-R" if keep_all else "Kculled-R"
        _forward_figures("bwd/s4_20000_320x180_direct", pair, fw, R)
        _grad_figures("bwd/s4_20000_320x180_direct", pair, g, gR, GRAD_NAMES)
        _cmp_forward(fw, R, P, walked=False)
        _cmp_grads(g, gR, R, what=pair)


# ---- distCUDA2 and markVisible ----------------------------------------------------------------------------------------------

def _blob(P, seed):
    rng = np.random.default_rng(seed)          # the blob of test_dist_cuda2_matches_oracle
    return (rng.normal(size=(P, 3)) * [1.0, 2.0, 0.5] + [0.3, -0.2, 3.0]).astype(np.float32)


def _duplicates():
    pts = _blob(3000, 3000)
    rng = np.random.default_rng(1)
    perm = rng.permutation(3000)
    pts[perm[:600]] = pts[perm[600:1200]]      # 600 exact copies of other points: distance 0, equal Morton codes
    return pts


def _negative_octant():
    pts = -np.abs(_blob(3000, 3001)) - np.float32(0.125)
    assert (pts < 0).all()                     # the bounding box's upper corner stays the 0 the reduction is seeded with
    return pts.astype(np.float32)


KNN_CLOUDS = {**{f"blob{P}": (lambda P=P: _blob(P, P)) for P in (5, 1024, 1025, 4096, 4097, 20000)},
              "duplicates": _duplicates, "negative_octant": _negative_octant}


@pytest.mark.parametrize("name", list(KNN_CLOUDS))
def test_dist_cuda2_three_ways(name):
    """Same float operations in the same order on all three: bit-exact.  1024 / 1025 is the box edge, 4096 / 4097 our sort's
    block edge, 20000 reaches the scan's second 1024-chunk."""
    knn = importlib.import_module("iclr2025_3d-mom_amd.simple_knn._C")
    pts = KNN_CLOUDS[name]()
    r, o = rg.knn_mean_dist2(pts), ro.knn_mean_dist2(pts)
    k = knn.distCUDA2(torch.from_numpy(pts).cuda()).cpu().numpy()
    _record(name, "knn", R_O=int((r.view(np.uint32) != o.view(np.uint32)).sum()), K_R=int((k.view(np.uint32) != r.view(np.uint32)).sum()))
    assert np.isfinite(r).all() and (r >= 0).all()
    if name == "duplicates":       # a point and its copy see the same three distances (each other at 0): the same mean, bit for bit
        perm = np.random.default_rng(1).permutation(3000)
        np.testing.assert_array_equal(r[perm[:600]], r[perm[600:1200]])
        assert (r > 0).all()
    np.testing.assert_array_equal(r.view(np.uint32), o.view(np.uint32))
    np.testing.assert_array_equal(k.view(np.uint32), r.view(np.uint32))


@pytest.mark.parametrize("P", [1, 63, 64, 65, 20011])
@pytest.mark.parametrize("pose_name", ["identity", "general"])
def test_mark_visible_three_ways(pose_name, P):
    from hip_helpers import RC, t
    s, want = near_plane_scene(P, pose_name, seed=260 + P)
    clouds = [(s["means3D"], want)]
    if P == 1:       # near_plane_scene's first Gaussian is behind the camera: the lone one in front, then behind
        clouds = [(to_world(np.array([[0.01, -0.02, z]]), **pose(pose_name)).astype(np.float32), np.array([seen]))
                  for z, seen in ((0.21, True), (0.19, False))]
    for m, expect in clouds:
        r = rg.mark_visible(m, s["viewmatrix"], s["projmatrix"])
        o = ro.mark_visible(m, s["viewmatrix"], s["projmatrix"])
        k = RC.mark_visible(t(m), t(s["viewmatrix"]), t(s["projmatrix"])).cpu().numpy()
        np.testing.assert_array_equal(r, o)
        np.testing.assert_array_equal(k, r)
        np.testing.assert_array_equal(r, expect)
