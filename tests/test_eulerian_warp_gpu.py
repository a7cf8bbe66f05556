"""The video generator's warp on the GPU (csrc/eulerian_warp.hip through ops and cinemagraph) against the numpy restatement of
eulerian_warp_cases.py -- which test_eulerian_warp_cpu.py holds to the reference's own code -- and against fixture g20.

Bounds (derived, not tuned; eps = 2^-24, the unit roundoff of fp32):
  * Euler integration: integers and fp32 adds only, so bit-equal.
  * the summation splat, per element: |got - want| <= (k + 4) eps splat(|input|), k the number of contributions to the element: the
    recursive-summation bound of k fp32 terms added in any order, (k - 1) eps sum|t| to first order, plus the roundings of the two
    products behind each term (the weight and input * weight).  The kernel adds atomically, in no fixed order, so bit-equality with
    an ordered fp32 sum is not asserted.
  * blend_feature / warp_one_level outside the blank pixels: |d| <= (2 k_max + 8) eps blend(|feature|): numerator and denominator each
    carry the splat's bound, then the division; at the blank pixels 50 more terms (49 products and their sum) on the box mean of
    blend(|feature|).  The blank mask itself must be identical: a pixel is blank iff no term reached it.

Achieved maxima as a share of the bound, MI355X (pytest -s prints them; k_max 31-148): fused blend 0.060 (against g20
0.062), fused warp 0.070 (0.052), op-by-op blend 0.094 (0.057), op-by-op warp 0.077 (0.073), the `pixels` form 0.077; the largest
absolute difference 5.2e-07 on features of unit variance."""
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import eulerian_warp_cases as ec

pytestmark = pytest.mark.gpu
pkg = "iclr2025_3d-mom_amd"
N = importlib.import_module(pkg + "._native")
ops = importlib.import_module(pkg + ".ops")
cg = importlib.import_module(pkg + ".cinemagraph")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
bits = lambda a: np.ascontiguousarray(a).view(np.uint32)

BLEND_CASES = ([(32, C, 6, idx) for C in (1, 3, 32, 70) for idx in (0, 1, 3, 5)]
               + [(256, C, 8, idx) for C in (1, 2, 3) for idx in (0, 1, 4, 7)] + [(256, 32, 8, 4)])


def share(d, bound):
    """Largest |d| / bound; a nonzero difference where the bound is zero is infinite."""
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(d == 0, 0.0, d / bound)
    return float(q.max())


# ---------------------------------------------------------------------------------------------------------------- Euler integration
@pytest.mark.parametrize("H,W,steps", [(24, 40, 5), (56, 56, 3), (33, 17, 7), (1, 1, 2), (24, 40, 0)])
def test_euler_integrate_has_the_reference_bits(H, W, steps):
    m = ec.flow(H, W)
    last, every = ops.euler_integrate(up(m), steps), ops.euler_integrate(up(m), steps, all_frames=True)
    want = ec.euler(m, steps, all_frames=True)
    assert last.shape == (2, H, W) and every.shape == (steps + 1, 2, H, W)
    assert np.array_equal(bits(every.cpu().numpy()), bits(want))
    assert np.array_equal(bits(last.cpu().numpy()), bits(want[steps]))
    assert torch.equal(ops.euler_integrate(up(m), steps, all_frames=True), every)          # two runs, the same bits
    if (H, W, steps) == (24, 40, 5):
        g = ec.g20()
        assert np.array_equal(bits(every.cpu().numpy()), bits(g["euler_24x40_all"]))
        assert np.array_equal(bits(last.cpu().numpy()), bits(g["euler_24x40_last"]))
        disp, visible = cg.euler_integration(up(m)[None], steps)
        assert disp.shape == (1, 2, H, W) and visible.shape == (1, 1, H, W) and bool((visible == 1).all())
        assert np.array_equal(bits(disp[0].cpu().numpy()), bits(g["euler_24x40_last"]))
        disp, visible = cg.euler_integration(up(m)[None], steps, return_all_frames=True)
        assert disp.shape == (6, 2, H, W) and visible.shape == (2, 1, H, W)


def test_euler_integrate_survives_non_finite_motion():
    m = ec.flow(24, 40, amp=0.2)
    bad = [(3, 5, np.nan), (10, 20, np.inf), (17, 33, -np.inf), (0, 0, np.nan), (23, 39, np.inf)]
    for y, x, v in bad:
        m[0 if v is np.nan else 1, y, x] = v
    every = ops.euler_integrate(up(m), 6, all_frames=True).cpu().numpy()
    assert np.isfinite(every).all()
    for y, x, _ in bad:
        assert not every[:, :, y, x].any()
    # a chain that never meets one of them is untouched: the same bits as on the field with zeros there
    clean = np.where(np.isfinite(m), m, 0).astype(np.float32)
    want = ec.euler(clean, 6, all_frames=True)
    trail = np.zeros((24, 40), bool)                      # pixels whose chain on the clean field visits a bad pixel
    yy, xx = np.meshgrid(np.arange(24), np.arange(40), indexing="ij")
    for s in range(6):
        py, px = np.rint(yy + want[s, 1]).astype(int), np.rint(xx + want[s, 0]).astype(int)
        for y, x, _ in bad:
            trail |= (py == y) & (px == x)
    assert (~trail).mean() > 0.5
    assert np.array_equal(bits(every[:, :, ~trail]), bits(want[:, :, ~trail]))


# ---------------------------------------------------------------------------------------------------------------- the summation splat
@pytest.mark.parametrize("n,C,H,W", [(1, 3, 24, 40), (2, 2, 32, 32), (1, 1, 7, 5), (1, 70, 9, 11)])
def test_softsplat_sum_against_the_restatement(n, C, H, W):
    rng = np.random.default_rng(n * 1000 + C * 100 + H)
    inp = rng.standard_normal((n, C, H, W)).astype(np.float32)
    flw = np.stack([ec.flow(H, W, amp=1.0 + 0.5 * i) for i in range(n)])
    got = ops.softsplat_sum(up(inp), up(flw)).cpu().numpy()
    want, k, mag = ec.splat(inp, flw)
    bound = (k[:, None] + 4) * ec.EPS * mag
    d = np.abs(got - want)
    print(f"softsplat_sum {n}x{C}x{H}x{W}: k max {int(k.max())}, |d| max {d.max():.3g}, largest share of the bound {share(d, bound):.3g}, "
          f"{(k == 0).mean() * 100:.0f} % of the pixels receive nothing")
    assert (d <= bound).all()
    assert not got[np.broadcast_to((k == 0)[:, None], got.shape)].any()


def test_softsplat_sum_drops_huge_and_non_finite_coordinates():
    inp = np.random.default_rng(5).standard_normal((1, 2, 16, 16)).astype(np.float32)
    flw, away = ec.flow(16, 16, amp=0.5)[None], ec.flow(16, 16, amp=0.5)[None]
    for (y, x), v in {(2, 3): np.nan, (5, 5): np.inf, (9, 1): -np.inf, (12, 12): 3e30, (15, 0): -3e9, (0, 15): 2.0 ** 31}.items():
        flw[0, (y + x) % 2, y, x] = v
        away[0, :, y, x] = -1000.0                      # the restatement's way to drop the pixel: every corner outside the canvas
    got = ops.softsplat_sum(up(inp), up(flw)).cpu().numpy()
    want, k, mag = ec.splat(inp, away)
    assert np.isfinite(got).all() and (np.abs(got - want) <= (k[:, None] + 4) * ec.EPS * mag).all()


@pytest.mark.parametrize("strType", ["summation", "average", "linear", "softmax"])
def test_function_softsplat_types_and_output_size(strType):
    """The four types are torch arithmetic around the summation splat (softmax_splatting.py:325-349): the same arithmetic in float64
    on the restatement's sums of the same (torch-formed) input."""
    rng = np.random.default_rng(11)
    x, f = up(rng.standard_normal((2, 3, 20, 28)).astype(np.float32)), up(np.stack([ec.flow(20, 28, amp=0.6), ec.flow(20, 28, amp=1.1)]))
    metric = up(rng.uniform(0.1, 1.5, (2, 1, 20, 28)).astype(np.float32))
    got = cg.FunctionSoftsplat(x, f, None if strType in ("summation", "average") else metric, strType)
    assert got.shape == (2, 3, 20, 28)
    cropped = cg.ModuleSoftsplat(strType)(x, f, metric, output_size=(12, 9))
    assert cropped.shape == (2, 3, 12, 9)
    full = {"summation": x, "average": torch.cat([x, torch.ones_like(x[:, :1])], 1), "linear": torch.cat([x * metric, metric], 1),
            "softmax": torch.cat([x * metric.exp(), metric.exp()], 1)}[strType]
    s, k, mag = ec.splat(full.cpu().numpy(), f.cpu().numpy())
    if strType == "summation":
        want, bound = s, (k[:, None] + 4) * ec.EPS * mag
    else:
        den = np.where(s[:, -1:] == 0, 1.0, s[:, -1:])
        want, bound = s[:, :-1] / den, (2 * k[:, None] + 8) * ec.EPS * mag[:, :-1] / den
    for g_, w_, b_ in ((got, want, bound), (cropped, want[:, :, :12, :9], bound[:, :, :12, :9])):
        d = np.abs(g_.cpu().numpy() - w_)
        assert (d <= b_).all(), share(d, b_)


# ---------------------------------------------------------------------------------------------------------------- blend and warp
def _check(name, got, want, bound, g_want=None):
    d = np.abs(got - want)
    line = f"{name}: |d| max {d.max():.3g}, largest share of the bound {share(d, bound):.3g}"
    ok = (d <= bound).all()
    if g_want is not None:
        dg = np.abs(got - g_want)
        line += f"; against g20 {dg.max():.3g}, share {share(dg, bound):.3g}"
        ok = ok and (dg <= bound).all()
    print(line)
    return ok


@pytest.mark.parametrize("S,C,n_frames,idx", BLEND_CASES)
def test_blend_and_warp_fused_and_op_by_op(S, C, n_frames, idx):
    b = ec.case(S, C, n_frames, idx)
    cut, pad, P, c0 = ec.geometry(S)
    golden = ec.GOLDEN[S][:3] == (S, C, n_frames)
    g, key, r = ec.g20(), f"s{S}_i{idx}_", ec.STRIDE[S]
    feature, flow = up(b["feature"])[None], up(b["motion"])[None]
    ok = True
    for fused in (True, False):
        tag = f"S {S} C {C} idx {idx} {'fused' if fused else 'op-by-op'}"
        blended = cg.blend_feature(feature, flow, idx, n_frames, fused=fused)
        assert blended.shape == (1, C, P, P) and blended.dtype == torch.float32
        ones = cg.blend_feature(torch.ones(1, 1, S, S, device="cuda"), flow, idx, n_frames, fused=fused)
        blank = (ones[0, 0] == 0).cpu().numpy()
        assert np.array_equal(blank, b["blank"]), tag
        bl = blended[0].cpu().numpy()
        assert not bl[:, b["blank"]].any()
        ok &= _check(tag + " blend", bl, b["blended"], ec.bound_blend(b))
        if golden:
            ok &= _check(tag + " blend (g20's rows)", bl[:, ::r, ::r], b["blended"][:, ::r, ::r], ec.bound_blend(b)[:, ::r, ::r],
                         g[key + "blended"])
        final = cg.warp_one_level(feature, flow, idx, n_frames, fused=fused)
        assert final.shape == (1, C, S, S) and final.dtype == torch.float32
        fn = final[0].cpu().numpy()
        ok &= _check(tag + " warp", fn, b["final"], ec.bound_final(b))
        if golden:
            ok &= _check(tag + " warp (g20's rows)", fn[:, ::r, ::r], b["final"][:, ::r, ::r], ec.bound_final(b)[:, ::r, ::r],
                         g[key + "final"])
    if golden:
        assert np.array_equal(b["blank"], np.unpackbits(g[key + "blank_bits"])[:P * P].reshape(P, P).astype(bool))
    # the fused route's own blank mask, whole and cropped, and both accumulation forms for the small channel counts
    forms = ("channels", "pixels") if C <= 3 else ("channels",)
    for form in forms:
        acc = ops.eulerian_blend(feature[0], flow[0], idx, n_frames, form=form)
        assert acc.shape == (P, P, C + 1)
        full, blank_full = ops.eulerian_finish(acc, S, full=True, return_blank=True)
        crop, blank_crop = ops.eulerian_finish(acc, S, return_blank=True)
        assert np.array_equal(blank_full.cpu().numpy().astype(bool), b["blank"]), form
        assert np.array_equal(blank_crop.cpu().numpy().astype(bool), b["blank_crop"]), form
        ok &= _check(f"S {S} C {C} idx {idx} form {form} blend", full.cpu().numpy(), b["blended"], ec.bound_blend(b))
        ok &= _check(f"S {S} C {C} idx {idx} form {form} warp", crop.cpu().numpy(), b["final"], ec.bound_final(b))
        den = acc[:, :, C].cpu().numpy()
        dd = np.abs(den - b["den"])
        assert (dd <= (b["k"] + 4) * ec.EPS * b["den"]).all()
    assert ok


def test_the_blank_path_runs_inside_the_crop():
    """In each size family some frame has blank pixels inside the crop, so the box mean above was compared, not skipped."""
    for S, (_, C, n_frames, idxs) in ec.GOLDEN.items():
        assert max(int(ec.case(S, C, n_frames, idx)["blank_crop"].sum()) for idx in idxs) > 0


def test_the_accumulator_is_cleared_by_every_call():
    b = ec.case(32, 3, 6, 3)
    acc = torch.full((56, 56, 4), 1e9, device="cuda")
    out = ops.eulerian_blend(up(b["feature"]), up(b["motion"]), 3, 6, acc=acc)
    assert out is acc
    got = ops.eulerian_finish(acc, 32).cpu().numpy()
    assert (np.abs(got - b["final"]) <= ec.bound_final(b)).all()


# ---------------------------------------------------------------------------------------------------------------- the drop-in
def test_install_video_dropin_serves_the_reference_names(tmp_path):
    """A throw-away tree named like the reference's, holding a caller written for this test."""
    utils = tmp_path / "thirdparty" / "StyleCineGAN" / "utils"
    utils.mkdir(parents=True)
    for d in (tmp_path / "thirdparty", tmp_path / "thirdparty" / "StyleCineGAN", utils):
        (d / "__init__.py").write_text("")
    (utils / "softmax_splatting.py").write_text("raise ImportError('the cupy module must not be imported')\n")
    (tmp_path / "caller.py").write_text(
        "from thirdparty.StyleCineGAN.utils.softmax_splatting import FunctionSoftsplat\n"
        "from thirdparty.StyleCineGAN.utils.joint_splatting import joint_splatting, backwarp\n"
        "from thirdparty.StyleCineGAN.utils.cinemagraph_utils import warp_one_level, euler_integration\n")
    saved = {k: v for k, v in sys.modules.items() if k == "caller" or k.split(".")[0] == "thirdparty"}
    for k in saved:
        del sys.modules[k]
    sys.path.insert(0, str(tmp_path))
    try:
        importlib.import_module(pkg).install_video_dropin()
        caller = importlib.import_module("caller")
        assert caller.FunctionSoftsplat is cg.FunctionSoftsplat and caller.joint_splatting is cg.joint_splatting
        assert caller.warp_one_level is cg.warp_one_level and caller.backwarp is cg.backwarp
        assert sys.modules["thirdparty"].__file__.startswith(str(tmp_path))             # the caller's own package, not a stand-in
        b = ec.case(32, 3, 6, 3)
        got = caller.warp_one_level(up(b["feature"])[None], up(b["motion"])[None], 3, 6)[0].cpu().numpy()
        assert (np.abs(got - b["final"]) <= ec.bound_final(b)).all()
        # joint_splatting's other mode goes through grid_sample, as the reference's does
        f = up(b["feature"])[None]
        z = torch.ones(1, 1, 32, 32, device="cuda")
        out = caller.joint_splatting(f, z, torch.zeros(1, 2, 32, 32, device="cuda"), f, z, torch.zeros(1, 2, 32, 32, device="cuda"),
                                     mode="no_forward_warping", output_size=(32, 32))
        assert out.shape == (1, 3, 32, 32)
    finally:
        sys.path.remove(str(tmp_path))
        for k in [k for k in sys.modules if k == "caller" or k.split(".")[0] == "thirdparty"]:
            del sys.modules[k]
        sys.modules.update(saved)


# ---------------------------------------------------------------------------------------------------------------- the pixel video
def _video_inputs(size=32):
    rng = np.random.default_rng(77)
    image = rng.integers(0, 256, (size, size, 3), dtype=np.uint8)
    mask = np.zeros((size, size), np.uint8)
    mask[size // 4:3 * size // 4, size // 4:size] = 255
    return image, torch.from_numpy(ec.flow(size, amp=0.4))[None], mask


def test_pixel_video_frames():
    image, flow, mask = _video_inputs()
    frames = cg.pixel_video(image, flow, mask, n_frames=6, size=32)
    assert len(frames) == 6 and all(f.shape == (32, 32, 3) and f.dtype == np.float32 for f in frames)
    # the input as the generator holds it (ip_utils.to_tensor and to_numpy's arithmetic, by the same torch ops on the same device: a
    # division by a Python scalar there is a multiplication by its reciprocal, which numpy's is not)
    xt = torch.from_numpy(image).float().cuda() / 127.5 - 1
    x, plain = xt.cpu().numpy(), ((xt + 1) / 2).cpu().numpy()
    for f in frames:
        assert np.array_equal(bits(f[mask == 0]), bits(plain[mask == 0]))            # outside the mask: the input, bit for bit
        assert f.min() >= -1e-6 and f.max() <= 1 + 1e-6
    # frame 0: the future half is the identity with weight 1, the past half adds zeros, so the warp returns the input to the blend's
    # bound with k = 8 terms per pixel, (2 * 8 + 8) eps |x|; the composite x m + x (1 - m) and (. + 1) / 2 add four roundings of
    # values of magnitude <= 2
    x64 = x.astype(np.float64)
    want = (x64 + 1) / 2
    assert (np.abs(frames[0] - want) <= 24 * ec.EPS * np.abs(x64) + 4 * ec.EPS * 2).all()
    assert any(np.abs(f - frames[0])[mask > 0].max() > 0.05 for f in frames[1:])     # the masked region moves


def test_motion_main_writes_the_video_frames(tmp_path):
    from PIL import Image
    image, flow, mask = _video_inputs(32)
    W, H = 40, 24
    frame = lambda: {"image": Image.fromarray(image), "mask": Image.fromarray(mask), "our_flow": [flow.clone()],
                     "transform_matrix": np.eye(4).tolist()}
    mom = tmp_path / "scene" / "MOM"
    mom.mkdir(parents=True)
    torch.save({"camera_angle_x": 0.6, "camera_angle_y": 0.6, "W": W, "H": H, "pcd_points": np.zeros((3, 4), np.float32),
                "pcd_colors": np.zeros((4, 3), np.float32), "frames": [frame() for _ in range(3)]}, mom / "train_data.pth")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    code = (f"import importlib; importlib.import_module('{pkg}.motion').main(['--input_dir', r'{tmp_path / 'scene'}', '--video', 'pixels', "
            "'--n_frames', '6', '--video_size', '32'])")
    r = subprocess.run([sys.executable, "-c", code], env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout[-2000:]
    names = sorted(os.listdir(mom / "video"))
    assert names == [f"{i:06d}.png" for i in range(6)]
    for n in names:
        im = Image.open(mom / "video" / n)
        im.load()
        assert im.size == (W, H) and im.mode == "RGB"
