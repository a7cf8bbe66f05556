"""Sampling the 2D flow images for the scene-flow fit, without a GPU: the float64 restatement of flow_sample_cases.py IS scipy's
griddata over the pixel grid (on noise images, and on the targets the reference run recorded in fixture g15) once it is given the
diagonals of scipy's triangulation; motion.grid_diagonals reads those diagonals and fixture g17 holds them; prepare_views keeps the
float64 pixels; the op and the C entry point refuse every invalid call before anything is launched."""
import importlib

import numpy as np
import pytest
import torch

import flow_sample_cases as fc
import sceneflow_cases as sc

pkg = "iclr2025_3d-mom_amd"
N = importlib.import_module(pkg + "._native")
ops = importlib.import_module(pkg + ".ops")
motion = importlib.import_module(pkg + ".motion")
FAKE = 1 << 20          # a non-null pointer value, 16-byte aligned; every call below is refused before it could be followed
BOUND = 1e-12           # of the image's largest magnitude: float64 rounding of another BLAS or Qhull build, never a wrong triangle


@pytest.mark.parametrize("H,W", fc.SIZES)
def test_the_restatement_is_griddata(H, W):
    """Noise images, random pixels over the whole image plus the hand-placed ones; no point is left out."""
    pytest.importorskip("scipy")
    rng = np.random.default_rng(H * 100 + W)
    image = fc.noise_images(1, H, W, seed=H + W, px=1.0)[0]
    pix = np.concatenate([rng.uniform(0.0, 1.0, (400, 2)) * [W - 1, H - 1], fc.hand_pixels(H, W)])
    want = motion.sample_flow_image(torch.from_numpy(image)[None], pix.T, H, W).T
    got = fc.restate(image, pix, motion.grid_diagonals(H, W))
    d = float(np.abs(got - want).max()) / sc.scale(image)
    print(f"{H} x {W}: restatement against griddata at {len(pix)} pixels: {d:.3g} of the image's largest magnitude {sc.scale(image):.3g}")
    assert d <= BOUND
    # the diagonals matter: with main diagonals everywhere the same pixels miss griddata by the scale of the image
    if (H - 1) * (W - 1) > 1:
        assert float(np.abs(fc.restate(image, pix, np.zeros((H - 1, W - 1), bool)) - want).max()) > 1e-3 * sc.scale(image)


def test_the_restatement_samples_the_recorded_targets():
    """g15's gt_j were written by the reference's own griddata calls: every view, every valid point."""
    d, case = sc.g15(), sc.g15_case()
    H, W = int(d["H"]), int(d["W"])
    mask = fc.g17()[0][(H, W)]
    worst, s = 0.0, sc.scale(d["t2c_flow"])
    for j in range(case.views.V):
        got = fc.restate(d["t2c_flow"][j][0], case.views.pix64[j].T, mask)
        worst = max(worst, float(np.abs(got.T - d[f"gt_{j}"]).max()))
    print(f"restatement against g15's recorded targets: {worst / s:.3g} of the images' largest magnitude {s:.3g}")
    assert worst <= BOUND * s


@pytest.mark.parametrize("H,W", fc.SIZES)
def test_grid_diagonals_are_the_fixtures(H, W):
    pytest.importorskip("scipy")
    masks, version = fc.g17()
    m = motion.grid_diagonals(H, W)
    assert m.dtype == np.bool_ and m.shape == (H - 1, W - 1)
    print(f"{H} x {W}: {m.mean():.3f} of the cells split by the anti-diagonal (fixture written with scipy {version})")
    assert np.array_equal(m, masks[(H, W)])
    assert motion.grid_diagonals(H, W) is m                                   # kept per (H, W)
    with pytest.raises(ValueError):
        m[0, 0] = True                                                        # and read-only: every caller shares it


def test_grid_diagonals_refuses_an_image_without_a_cell():
    for H, W in ((1, 5), (5, 1), (0, 0)):
        with pytest.raises(ValueError, match="at least one cell"):
            motion.grid_diagonals(H, W)


def test_pack_diagonals_round_trips():
    """36 x 52 = 1 872 cells, not a whole number of words: bit c % 32 of word c // 32, nothing set behind the last cell."""
    mask = fc.g17()[0][(37, 53)]
    words = motion.pack_diagonals(mask)
    assert words.dtype == np.int32 and words.shape == ((1872 + 31) // 32,)
    w = words.view(np.uint32)
    c = np.arange(1872)
    assert np.array_equal(((w[c // 32] >> (c % 32).astype(np.uint32)) & 1).astype(bool), mask.reshape(-1))
    assert int(w[-1]) >> (1872 % 32) == 0
    assert motion.pack_diagonals(np.ones((1, 1), bool)).tolist() == [1]
    assert motion.pack_diagonals(np.ones((4, 8), bool)).view(np.uint32).tolist() == [0xFFFFFFFF]


def test_prepare_views_keeps_the_float64_pixels():
    d, case = sc.g15(), sc.g15_case()
    v = case.views
    assert len(v.pix64) == v.V
    for j in range(v.V):
        assert v.pix64[j].dtype == np.float64 and v.pix64[j].shape == (2, len(v.valid[j]))
        assert np.array_equal(v.pix64[j].astype(np.float32).view(np.uint32), v.pix0[j].view(np.uint32)), j       # bit for bit
        assert np.array_equal(v.pix64[j].astype(np.float32), d[f"pix0_{j}"]), j
    # a ViewSet built the way it was built before this field existed still builds
    assert motion.ViewSet(P=v.P, H=v.H, W=v.W, R=v.R, T=v.T, valid=v.valid, pix0=v.pix0).pix64 is None
    with pytest.raises(ValueError, match="pix64"):
        motion.sample_flow_images(motion.ViewSet(P=v.P, H=v.H, W=v.W, R=v.R, T=v.T, valid=v.valid, pix0=v.pix0), d["t2c_flow"][:, 0],
                                  diagonals=fc.g17()[0][(24, 24)], device="cpu")


def test_the_op_refuses_cpu_tensors_and_wrong_shapes():
    case = fc.kernel_case(5, 7, 63, 6)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    args = [t(case.images), t(case.pix), t(case.bits), t(motion.pack_diagonals(fc.g17()[0][(5, 7)]))]
    with pytest.raises(N.MomError, match="no CPU path"):
        ops.flow_sample(*args)
    with pytest.raises(N.MomError, match="no CPU path"):
        motion.sample_flow_images(case.views, t(case.images), diagonals=fc.g17()[0][(5, 7)], device="cpu")
    with pytest.raises(ValueError, match="one entry per cell"):
        motion.sample_flow_images(case.views, t(case.images), diagonals=np.zeros((4, 5), bool), device="cpu")
    with pytest.raises(ValueError, match="flow images"):
        motion.sample_flow_images(case.views, t(case.images[:5]), diagonals=fc.g17()[0][(5, 7)], device="cpu")
    with pytest.raises(ValueError, match="sampler"):
        motion.refit_scene_flow("nowhere", sampler="nearest")

    # what the kernel cannot take is refused whatever the device
    with pytest.raises(N.MomError, match=r"pix must be a contiguous torch.float64 \[6, 63, 2\]"):
        ops.flow_sample(args[0], args[1].float(), args[2], args[3])
    with pytest.raises(N.MomError, match=r"valid must be a contiguous torch.int32 \[1, 63\]"):
        ops.flow_sample(args[0], args[1], torch.zeros(2, 63, dtype=torch.int32), args[3])
    with pytest.raises(N.MomError, match=r"diagonals must be a contiguous torch.int32 \[1\]"):
        ops.flow_sample(args[0], args[1], args[2], torch.zeros(2, dtype=torch.int32))
    with pytest.raises(N.MomError, match="flow_images must be a contiguous"):
        ops.flow_sample(args[0].permute(0, 1, 3, 2), args[1], args[2], args[3])
    with pytest.raises(N.MomError, match=r"\[V,2,H,W\] or \[V,H,W,2\]"):
        ops.flow_sample(args[0][:, :1].contiguous(), args[1], args[2], args[3])
    with pytest.raises(N.MomError, match="records must be a contiguous"):
        ops.flow_sample(args[0], args[1], args[2], args[3], torch.zeros(6, 63, 3))


def _sample(lib, P=10, V=2, H=5, W=7, hole=None, **over):
    a = {n: FAKE for n in ("flow", "pix", "valid", "diag", "records")}
    a.update(over)
    if hole is not None:
        a[hole] = None
    return lib.mom_flow_sample(P, V, H, W, a["flow"], a["pix"], a["valid"], a["diag"], a["records"], None)


def test_every_invalid_call_is_refused_before_anything_is_launched():
    lib = N.lib()
    assert "mom_flow_sample" in N.EXPORTS and len(lib.mom_flow_sample.argtypes) == 10
    assert N.ABI_VERSION == 8 == lib.mom_abi_version()                        # additive
    assert _sample(lib, P=0) == N.MOM_OK                                      # nothing to do, nothing launched
    assert lib.mom_flow_sample(0, 1, 2, 2, None, None, None, None, None, None) == N.MOM_OK
    for bad in (dict(W=1), dict(H=1), dict(V=0), dict(V=-1), dict(V=65536), dict(P=-1), dict(P=0, W=1), dict(P=0, V=0)):
        assert _sample(lib, **bad) == N.MOM_EINVAL, bad
    for hole in ("flow", "pix", "valid", "diag", "records"):
        assert _sample(lib, hole=hole) == N.MOM_EINVAL, hole
    assert _sample(lib, records=FAKE + 4) == N.MOM_EINVAL                     # 16-byte records
    assert _sample(lib, pix=FAKE + 8) == N.MOM_EINVAL                         # 16-byte pixels
    assert _sample(lib, flow=FAKE + 4) == N.MOM_EINVAL                        # 8-byte texels
