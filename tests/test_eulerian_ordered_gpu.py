"""The ordered splat of the video generator's warp on the GPU (csrc/eulerian_ordered.hip; include/mom4d.h, "ordered splat of the video
generator's warp"): the device result equals the host twin -- which test_eulerian_ordered_cpu.py holds to the documented order -- at
every element; it repeats bit for bit whatever the scratch held; it lies within the atomic form's own summation bound of the atomic
form and of the float64 sums; and the Python layers follow the argument and the process-wide switch."""
import importlib

import numpy as np
import pytest
import torch

import eulerian_ordered_cases as oc
import eulerian_warp_cases as ec

pytestmark = pytest.mark.gpu
N = oc.N
ops = importlib.import_module(oc.pkg + ".ops")
cg = importlib.import_module(oc.pkg + ".cinemagraph")
RC = importlib.import_module(oc.pkg + ".diff_gaussian_rasterization._C")
up = lambda a: torch.from_numpy(np.array(a)).cuda()          # (a copy: the shared cases are read-only arrays)


def device_blend(feature, motion, idx, n_frames, fill=0xA5):
    """mom_eulerian_blend_ordered through ctypes on a scratch of exactly the sized bytes, prefilled with `fill`; acc prefilled too."""
    Cn, S, _ = feature.shape
    P = ec.geometry(S)[2]
    lib = N.lib()
    need = lib.mom_eulerian_ordered_scratch_bytes(Cn, S)
    assert need > 0
    scratch = torch.full((need,), fill, dtype=torch.uint8, device="cuda")
    acc = torch.full((P, P, Cn + 1), float("nan"), device="cuda")
    f, m = up(feature), up(motion)
    N.check(lib.mom_eulerian_blend_ordered(Cn, S, S, idx, n_frames, N.ptr(f), N.ptr(m), N.ptr(acc), N.ptr(scratch), need,
                                           N.current_stream()), "mom_eulerian_blend_ordered")
    return acc


@pytest.mark.parametrize("kind", oc.MOTIONS)
@pytest.mark.parametrize("S,Cn", [(16, 1), (16, 3), (16, 31), (16, 32), (16, 63), (16, 64), (16, 65), (256, 2)])
def test_the_device_accumulator_is_the_host_twins(S, Cn, kind):
    for idx in oc.IDX:
        f, m, want = oc.blend_case(kind, S, Cn, idx)
        got = device_blend(f, m, idx, oc.N_FRAMES)
        assert torch.equal(got.view(torch.int32), up(want).view(torch.int32)), (S, Cn, kind, idx)


@pytest.mark.parametrize("S,Cn,kind", [(16, 3, "random"), (16, 32, "converge"), (256, 2, "nonfinite")])
def test_two_calls_on_different_garbage_are_the_same_bits(S, Cn, kind):
    """(The ordered blend reads no MOM_* switch of the environment -- csrc/eulerian_ordered.hip has no getenv -- so there is no
    setting to vary.)"""
    f, m = oc.features(Cn, S), oc.motion(kind, S)
    one = device_blend(f, m, 2, oc.N_FRAMES, fill=0x00)
    two = device_blend(f, m, 2, oc.N_FRAMES, fill=0xFF)
    assert torch.equal(one.view(torch.int32), two.view(torch.int32))


@pytest.mark.parametrize("S,Cn,n_frames,idx", [(32, 3, 6, 0), (32, 3, 6, 3), (32, 3, 6, 5), (32, 32, 6, 3), (256, 2, 8, 4)])
def test_ordered_against_the_atomic_blend_and_through_finish(S, Cn, n_frames, idx):
    b = ec.case(S, Cn, n_frames, idx)
    f, m = up(b["feature"]), up(b["motion"])
    ordered = device_blend(b["feature"], b["motion"], idx, n_frames)
    atomic = ops.eulerian_blend(f, m, idx, n_frames, ordered=False)
    blank_o, blank_a = (ordered[:, :, Cn] == 0).cpu().numpy(), (atomic[:, :, Cn] == 0).cpu().numpy()
    assert np.array_equal(blank_o, blank_a) and np.array_equal(blank_o, b["blank"])
    bound, keep = ec.bound_blend(b), np.broadcast_to(~b["blank"][None], b["blended"].shape)
    norm = lambda acc: ops.eulerian_finish(acc, S, full=True).cpu().numpy().astype(np.float64)
    d_atomic, d_f64 = np.abs(norm(ordered) - norm(atomic)), np.abs(norm(ordered) - b["blended"])
    print(f"S {S} C {Cn} idx {idx}: largest |ordered - atomic| / bound {float((d_atomic[keep] / bound[keep]).max()):.3g}, "
          f"|ordered - float64| / bound {float((d_f64[keep] / bound[keep]).max()):.3g}")
    assert (d_atomic[keep] <= bound[keep]).all() and (d_f64[keep] <= bound[keep]).all()
    # mom_eulerian_finish takes the ordered accumulator unchanged
    final, blank = ops.eulerian_finish(ordered, S, return_blank=True)
    assert np.array_equal(blank.cpu().numpy().astype(bool), b["blank_crop"])
    assert (np.abs(final.cpu().numpy() - b["final"]) <= ec.bound_final(b)).all()
    again = ops.eulerian_finish(device_blend(b["feature"], b["motion"], idx, n_frames, fill=0x3C), S)
    assert torch.equal(final.view(torch.int32), again.view(torch.int32))


@pytest.mark.parametrize("n,Cn,H,W", [(2, 3, 5, 7), (1, 33, 28, 56)])
def test_the_ordered_splat_is_its_host_twins(n, Cn, H, W):
    inp, flw, out_in = oc.splat_inputs(n, Cn, H, W)
    reached = oc.splat_reached(flw, H, W)
    assert (~reached).any() and reached.any()
    far = np.argwhere(~reached)
    out_in[far[0][0], :, far[0][1], far[0][2]] = -0.0                           # a texel without a term keeps its bits, this one's too
    want = oc.splat_host(inp, flw, out_in)
    lib = N.lib()
    need = lib.mom_softsplat_ordered_scratch_bytes(n, Cn, H, W)
    results = []
    for fill in (0x00, 0xFF):
        scratch = torch.full((need,), fill, dtype=torch.uint8, device="cuda")
        out, i_, f_ = up(out_in), up(inp), up(flw)
        N.check(lib.mom_softsplat_sum_ordered(n, Cn, H, W, N.ptr(i_), N.ptr(f_), N.ptr(out), N.ptr(scratch), need, N.current_stream()),
                "mom_softsplat_sum_ordered")
        results.append(out.cpu().numpy())
    assert np.array_equal(oc.bits(results[0]), oc.bits(want)) and np.array_equal(oc.bits(results[1]), oc.bits(want))
    untouched = np.broadcast_to(~reached[:, None], want.shape)
    assert np.array_equal(oc.bits(results[0])[untouched], oc.bits(out_in)[untouched])
    # ops.softsplat_sum(ordered=True) is the same call onto zeros, and lies within the atomic form's bound of the float64 sums
    got = ops.softsplat_sum(up(inp), up(flw), ordered=True).cpu().numpy()
    assert np.array_equal(oc.bits(got), oc.bits(oc.splat_host(inp, flw, np.zeros_like(out_in))))
    clean = flw.copy()
    clean[~np.isfinite(clean) | (np.abs(clean) >= 2.0 ** 30)] = -1000.0          # the restatement's way to drop an entry
    s64, k, mag = ec.splat(inp, clean)
    assert (np.abs(got - s64) <= (k[:, None] + 4) * ec.EPS * mag).all()


def _warp_cache():
    return RC._state["warp_ordered"]


@pytest.mark.parametrize("fused", [True, False])
def test_warp_one_level_follows_the_argument_and_the_switch(fused):
    S, Cn, n = 32, 3, 6
    x, flow = up(ec.features(Cn, S))[None], up(ec.flow(S))[None]
    assert RC.deterministic() is False
    RC._state["warp_ordered"] = None                                            # (an earlier test of this file may have made it)
    atomic = cg.warp_one_level(x, flow, 3, n, fused=fused)                      # ordered=None with the switch off: the atomic route,
    assert _warp_cache() is None                                                # and nothing was allocated for the ordered one
    one = cg.warp_one_level(x, flow, 3, n, fused=fused, ordered=True)
    two = cg.warp_one_level(x, flow, 3, n, fused=fused, ordered=True)
    assert torch.equal(one.view(torch.int32), two.view(torch.int32)) and _warp_cache() is not None
    b = ec.case(S, Cn, n, 3)
    for got in (atomic, one):
        assert (np.abs(got[0].cpu().numpy() - b["final"]) <= ec.bound_final(b)).all()
    RC.set_deterministic(True)
    try:
        under = cg.warp_one_level(x, flow, 3, n, fused=fused)
        off = cg.warp_one_level(x, flow, 3, n, fused=fused, ordered=False)
    finally:
        RC.set_deterministic(False)
    assert torch.equal(under.view(torch.int32), one.view(torch.int32))
    assert (np.abs(off[0].cpu().numpy() - b["final"]) <= ec.bound_final(b)).all()
    if fused:                                                                   # the fused route's accumulator is the host twin's
        acc = ops.eulerian_blend(x[0], flow[0], 3, n, ordered=True, form="pixels")
        assert np.array_equal(oc.bits(acc.cpu().numpy()), oc.bits(oc.blend_host(b["feature"], b["motion"], 3, n)))


def test_pixel_video_frames_repeat_bit_for_bit():
    rng = np.random.default_rng(7)
    image = rng.integers(0, 256, (32, 32, 3), dtype=np.uint8)
    mask = np.where(np.arange(32)[:, None] + np.arange(32)[None] > 20, 255, 0).astype(np.uint8)
    flow = ec.flow(32, amp=0.4)[None]
    runs = [[f.clone() for f in cg.pixel_video_frames(image, flow, mask, n_frames=5, size=32, ordered=True)] for _ in range(2)]
    assert len(runs[0]) == 5 and all(f.shape == (32, 32, 3) for f in runs[0])
    for a, b in zip(*runs):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert RC.deterministic() is False
