"""The video generator's warp without a GPU: the numpy restatement of eulerian_warp_cases.py against fixture g20 (the reference's
own euler_integration, blend_feature, feature_inpaint_conv and warp_one_level, tools/gen_eulerian_warp_golden.py); the host side
of cinemagraph.py -- cut, padding and crop arithmetic against the shapes the reference recorded, resize_flow, what is refused; and
the C entry points' argument checks, every one before anything is launched."""
import ctypes as C
import importlib

import numpy as np
import pytest
import torch

import eulerian_warp_cases as ec

pkg = "iclr2025_3d-mom_amd"
N = importlib.import_module(pkg + "._native")
ops = importlib.import_module(pkg + ".ops")
cg = importlib.import_module(pkg + ".cinemagraph")
FAKE = 1 << 20          # a non-null pointer value; every call below is refused before it could be followed
FAMILIES = [(S, idx) for S, (_, _, _, idxs) in ec.GOLDEN.items() for idx in idxs]


def _blank(g, key, P):
    return np.unpackbits(g[key + "blank_bits"])[:P * P].reshape(P, P).astype(bool)


def test_euler_restatement_has_the_reference_bits_on_a_non_square_field():
    g, m = ec.g20(), ec.flow(24, 40)
    all_ = ec.euler(m, 5, all_frames=True)
    assert all_.shape == g["euler_24x40_all"].shape == (6, 2, 24, 40)
    assert np.array_equal(all_.view(np.uint32), g["euler_24x40_all"].view(np.uint32))
    assert np.array_equal(ec.euler(m, 5).view(np.uint32), g["euler_24x40_last"].view(np.uint32))
    moved, reset = (np.abs(all_[5]).sum(0) > 0).mean(), (np.abs(all_[5]).sum(0) == 0).mean()
    assert moved > 0.05 and reset > 0.2         # chains that stay inside, and chains that leave (or never move)


@pytest.mark.parametrize("S,idx", FAMILIES)
def test_restatement_against_the_reference(S, idx):
    """Displacements bit-equal, blank masks equal as sets, blended and final maps within the bound of one fp32 rounding of a float64
    result (the fixture's fp32 cast; at blank pixels the reference's fp32 conv2d: the 50-term part of the bound)."""
    g, (_, Cn, n_frames, _), r = ec.g20(), ec.GOLDEN[S], ec.STRIDE[S]
    key = f"s{S}_i{idx}_"
    b = ec.case(S, Cn, n_frames, idx)
    cut, pad, P, crop0 = ec.geometry(S)
    assert list(g[key + "shapes"]) == [Cn, S, cut, pad, P, crop0, n_frames, idx]
    for name in ("future", "past"):
        assert np.array_equal(b[name][:, ::r, ::r].view(np.uint32), g[key + name].view(np.uint32)), name
    assert np.array_equal(b["blank"], _blank(g, key, P))
    d = np.abs(b["blended"][:, ::r, ::r] - g[key + "blended"])
    bound = ec.bound_blend(b)[:, ::r, ::r]
    print(f"S {S} idx {idx}: blended |d| max {d.max():.3g}, largest share of the bound {np.max(d / np.maximum(bound, 1e-300)):.3g}, "
          f"k max {int(b['k'].max())}, blank {int(b['blank'].sum())} ({int(b['blank_crop'].sum())} in the crop)")
    assert (d <= bound).all()
    d = np.abs(b["final"][:, ::r, ::r] - g[key + "final"])
    assert (d <= ec.bound_final(b)[:, ::r, ::r]).all()


@pytest.mark.parametrize("S", sorted(ec.GOLDEN))
def test_some_frame_has_blank_pixels_inside_the_crop(S):
    """The condition on the inputs: the box-filter path cannot pass by not running.  Read from the REFERENCE's output."""
    g = ec.g20()
    _, _, P, c0 = ec.geometry(S)
    inside = [int(_blank(g, f"s{S}_i{idx}_", P)[c0:c0 + S, c0:c0 + S].sum()) for idx in ec.GOLDEN[S][3]]
    assert max(inside) > 0, inside
    assert inside[0] == 0 and inside[-1] == 0       # idx 0 and n_frames-1: one half is the identity, it reaches every pixel


def test_geometry_is_the_reference_recorded_one():
    g = ec.g20()
    for S in ec.GOLDEN:
        want = tuple(int(v) for v in g[f"s{S}_i0_shapes"][2:6])
        assert ops.eulerian_geometry(S) == want == ec.geometry(S)
        assert (cg.cut_size_of(S), cg.pad_size_of(S - 2 * cg.cut_size_of(S))) == want[:2]
    assert ops.eulerian_geometry(1024) == (3, 381, 1780, 378) and ops.eulerian_geometry(512) == (2, 190, 888, 188)
    assert ops.eulerian_geometry(128) == (0, 48, 224, 48) and ops.eulerian_geometry(1) == (0, 0, 1, 0)
    for bad in (0, -4):
        with pytest.raises(N.MomError, match="eulerian_geometry"):
            ops.eulerian_geometry(bad)


def test_pad_crop_and_resize_on_the_host():
    x = torch.arange(2 * 3 * 32 * 32, dtype=torch.float32).reshape(2, 3, 32, 32)
    p = cg.pad_tensor(x)
    assert p.shape == (2, 3, 56, 56) and torch.equal(p[:, :, 12:44, 12:44], x) and torch.equal(p[:, :, 0, 12:44], x[:, :, 12])
    assert torch.equal(cg.crop_padded_tensor(p, 32), x)
    assert cg.pad_tensor(x, mode="constant", number=7.0)[0, 0, 0, 0] == 7.0
    # the cut sizes: crop_padded_tensor starts at pad - cut
    y = torch.zeros(1, 1, 442, 442)
    y[:, :, 93:349, 93:349] = 1
    assert cg.crop_padded_tensor(y, 256).min() == 1 and cg.crop_padded_tensor(y, 256).shape[-1] == 256
    f = torch.from_numpy(ec.flow(32))[None]
    up, down = cg.resize_flow(f, 128), cg.resize_flow(f, 8)
    assert up.shape == (1, 2, 128, 128) and down.shape == (1, 2, 8, 8) and cg.resize_flow(f, 32) is f
    want = torch.nn.functional.interpolate(f, size=(64, 64), mode="bilinear", align_corners=False) * 2
    want = torch.nn.functional.interpolate(want, size=(128, 128), mode="bilinear", align_corners=False) * 2
    assert torch.equal(up, want)
    assert torch.equal(cg.resize_flow(f, 16), torch.nn.functional.interpolate(f, size=(16, 16), mode="bilinear", align_corners=False) / 2)
    with pytest.raises(ValueError, match="halvings or doublings"):
        cg.resize_flow(f, 48)
    assert cg.resize_feature(x, 64).shape == (2, 3, 64, 64) and cg.resize_feature(x, 8).shape == (2, 3, 16, 16)


def test_what_is_not_built_says_why_and_cpu_tensors_are_refused():
    with pytest.raises(NotImplementedError, match="fast-marching"):
        cg.feature_inpaint(None, None, 0, 2)
    x = torch.zeros(1, 2, 4, 4, requires_grad=True)
    with pytest.raises(N.MomError, match="no CPU path"):
        cg.FunctionSoftsplat(x.detach(), torch.zeros(1, 2, 4, 4), None, "summation")
    with pytest.raises(N.MomError, match="no CPU path"):
        ops.euler_integrate(torch.zeros(2, 4, 4), 3)
    with pytest.raises(N.MomError, match=r"\[2,H,W\]"):
        ops.euler_integrate(torch.zeros(1, 2, 4, 4), 3)
    with pytest.raises(N.MomError, match="steps"):
        ops.euler_integrate(torch.zeros(2, 4, 4), -1)
    with pytest.raises(N.MomError, match="square"):
        ops.eulerian_blend(torch.zeros(3, 8, 12), torch.zeros(2, 8, 12), 0, 4)
    with pytest.raises(N.MomError, match="idx"):
        ops.eulerian_blend(torch.zeros(3, 8, 8), torch.zeros(2, 8, 8), 4, 4)
    with pytest.raises(N.MomError, match="form"):
        ops.eulerian_blend(torch.zeros(3, 8, 8), torch.zeros(2, 8, 8), 1, 4, form="tiles")
    with pytest.raises(N.MomError, match=r"acc must be \[14,14,4\]"):
        ops.eulerian_blend(torch.zeros(3, 8, 8), torch.zeros(2, 8, 8), 1, 4, acc=torch.zeros(14, 14, 3))
    with pytest.raises(N.MomError, match="no CPU path"):
        ops.eulerian_blend(torch.zeros(3, 8, 8), torch.zeros(2, 8, 8), 1, 4)
    with pytest.raises(N.MomError, match=r"acc must be \[14,14,C\+1\]"):
        ops.eulerian_finish(torch.zeros(12, 12, 4), 8)
    with pytest.raises(N.MomError, match="N,2,H,W"):
        ops.softsplat_sum(torch.zeros(1, 3, 4, 4), torch.zeros(1, 2, 4, 5))
    with pytest.raises(N.MomError, match="one image at a time"):
        cg.warp_one_level(torch.zeros(2, 3, 8, 8), torch.zeros(2, 2, 8, 8), 1, 4, fused=True)
    with pytest.raises(NotImplementedError, match="no_grad"):
        cg._FunctionSoftsplat.backward(None, None)


def test_every_invalid_call_is_refused_before_anything_is_launched():
    lib = N.lib()
    names = ("mom_euler_integrate", "mom_softsplat_sum", "mom_eulerian_geometry", "mom_eulerian_blend", "mom_eulerian_finish")
    assert all(n in N.EXPORTS for n in names)
    assert N.ABI_VERSION == 8 == lib.mom_abi_version()                         # additive
    euler = lambda H=4, W=5, steps=3, all_=0, m=FAKE, d=FAKE: lib.mom_euler_integrate(H, W, steps, all_, m, d, None)
    for bad in (dict(H=0), dict(W=0), dict(H=-1), dict(steps=-1), dict(m=None), dict(d=None), dict(H=1 << 16, W=1 << 15)):
        assert euler(**bad) == N.MOM_EINVAL, bad
    splat = lambda n=1, c=3, H=4, W=5, i=FAKE, f=FAKE, o=FAKE: lib.mom_softsplat_sum(n, c, H, W, i, f, o, None)
    for bad in (dict(n=0), dict(c=0), dict(H=0), dict(W=0), dict(i=None), dict(f=None), dict(o=None), dict(H=1 << 16, W=1 << 15)):
        assert splat(**bad) == N.MOM_EINVAL, bad
    blend = lambda c=3, H=32, W=32, idx=1, n=6, form=0, f=FAKE, m=FAKE, a=FAKE: lib.mom_eulerian_blend(c, H, W, idx, n, form, f, m, a, None)
    for bad in (dict(c=0), dict(H=32, W=40), dict(H=0, W=0), dict(idx=-1), dict(idx=6), dict(n=1, idx=0), dict(form=2), dict(form=-1),
                dict(f=None), dict(m=None), dict(a=None), dict(H=40000, W=40000)):
        assert blend(**bad) == N.MOM_EINVAL, bad
    finish = lambda c=3, S=32, full=0, a=FAKE, o=FAKE, b=None: lib.mom_eulerian_finish(c, S, full, a, o, b, None)
    for bad in (dict(c=0), dict(S=0), dict(S=-32), dict(a=None), dict(o=None), dict(S=40000, full=1)):
        assert finish(**bad) == N.MOM_EINVAL, bad
    out = [C.c_int(-1) for _ in range(4)]
    assert lib.mom_eulerian_geometry(0, *[C.byref(o) for o in out]) == N.MOM_EINVAL and out[0].value == -1
    assert lib.mom_eulerian_geometry(256, None, None, C.byref(out[2]), None) == N.MOM_OK and out[2].value == 442


def test_video_dropin_is_apart_from_the_training_dropin():
    mod = importlib.import_module(pkg)
    assert not any(k.startswith("thirdparty") for k in mod._DROPIN)
    assert len(mod._VIDEO_DROPIN) == 3 and all(k.startswith("thirdparty.StyleCineGAN.utils.") for k in mod._VIDEO_DROPIN)
