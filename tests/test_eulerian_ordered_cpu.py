"""The ordered splat of the video generator's warp without a GPU (include/mom4d.h, "ordered splat of the video generator's warp"): its
entry points in the C ABI, what they refuse before anything is launched, and the host twins against the documented order restated in
numpy (eulerian_ordered_cases.py) and against the float64 sums of eulerian_warp_cases.py."""
import importlib
import inspect

import numpy as np
import pytest

import eulerian_ordered_cases as oc
import eulerian_warp_cases as ec

N = oc.N
RC = importlib.import_module(oc.pkg + ".diff_gaussian_rasterization._C")
FAKE = 0x10000        # a 256-byte aligned pointer that is never dereferenced: every call below is refused first

NAMES = ("mom_eulerian_ordered_scratch_bytes", "mom_eulerian_blend_ordered", "mom_softsplat_ordered_scratch_bytes",
         "mom_softsplat_sum_ordered", "mom_eulerian_blend_ordered_host", "mom_softsplat_sum_ordered_host")


def test_the_entry_points_are_additive():
    lib = N.lib()
    assert all(n in N.EXPORTS and hasattr(lib, n) for n in NAMES)
    assert N.ABI_VERSION == 8 == lib.mom_abi_version()


def test_scratch_sizes_are_positive_monotone_and_zero_for_what_is_refused():
    lib = N.lib()
    blend, splat = lib.mom_eulerian_ordered_scratch_bytes, lib.mom_softsplat_ordered_scratch_bytes
    for C in (1, 3, 15, 16, 32, 256):
        sizes = [blend(C, S) for S in (1, 2, 16, 17, 128, 200, 1024)]          # (S = 256, 512, 1024 cut their border: 1024 is above all)
        assert sizes[0] > 0 and all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[-1] > sizes[0]
    for S in (16, 128, 1024):
        sizes = [blend(C, S) for C in (1, 2, 3, 15, 16, 17, 32, 64, 256)]
        assert all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[-1] > sizes[0]
        P = ec.geometry(S)[2]
        # the records, the four sort buffers, the segment table and the channel-last copy the header lists fit
        assert blend(32, S) >= 2 * P * P * (16 + 16) + 4 * ((P + 1) ** 2 + 1) + 4 * S * S * 32
    # the atomic blend takes S = 20000 (padded 35000: padded^2 < 2^31); its 2 padded^2 entries do not fit the sort
    assert blend(1, 20000) == 0 and ec.geometry(20000)[2] ** 2 < 2 ** 31 < 2 * ec.geometry(20000)[2] ** 2 * 2
    assert blend(0, 16) == blend(-1, 16) == blend(3, 0) == blend(3, -5) == 0
    assert blend(2 ** 30, 1024) == 0                                             # padded^2 (C + 1) >= 2^40, as the atomic form
    s = [splat(1, 1, H, W) for H, W in ((1, 1), (5, 7), (28, 56), (56, 56), (1531, 3062))]
    assert s[0] > 0 and all(a <= b for a, b in zip(s, s[1:])) and s[-1] > s[0]
    assert splat(1, 3, 5, 7) == splat(2, 3, 5, 7) == splat(2, 33, 5, 7)          # one image after the other; no per-channel part
    assert splat(0, 1, 5, 7) == splat(1, 0, 5, 7) == splat(1, 1, 0, 7) == splat(1, 1, 5, 0) == 0
    assert splat(1, 1, 40000, 40000) == 0                                        # H W in (2^30, 2^31): the atomic splat takes it
    assert splat(1, 1, 1, 2 ** 30) == 0 < splat(1, 1, 1, 2 ** 29)                # 2^30 entries fit, their 2 (2^30 + 1) cells do not


def test_every_invalid_call_is_refused_before_anything_is_launched():
    lib = N.lib()
    need = lib.mom_eulerian_ordered_scratch_bytes(3, 16)

    def blend(C=3, H=16, W=16, idx=2, n=5, feature=FAKE, motion=FAKE, acc=FAKE, scratch=FAKE, nbytes=need):
        return lib.mom_eulerian_blend_ordered(C, H, W, idx, n, feature, motion, acc, scratch, nbytes, None)

    for bad in (dict(C=0), dict(C=-1), dict(H=16, W=17), dict(H=0, W=0), dict(H=-4, W=-4), dict(n=1), dict(idx=-1), dict(idx=5),
                dict(feature=None), dict(motion=None), dict(acc=None),                    # what mom_eulerian_blend refuses
                dict(scratch=None), dict(scratch=FAKE + 4), dict(scratch=FAKE + 128), dict(nbytes=0), dict(nbytes=need - 1),
                dict(H=20000, W=20000, nbytes=2 ** 62),                                   # 2 padded^2 entries > 2^30
                dict(C=2 ** 30, H=1024, W=1024, nbytes=2 ** 62)):
        assert blend(**bad) == N.MOM_EINVAL, bad
    need = lib.mom_softsplat_ordered_scratch_bytes(2, 3, 5, 7)

    def splat(n=2, C=3, H=5, W=7, inp=FAKE, flow=FAKE, out=FAKE, scratch=FAKE, nbytes=need):
        return lib.mom_softsplat_sum_ordered(n, C, H, W, inp, flow, out, scratch, nbytes, None)

    for bad in (dict(n=0), dict(C=0), dict(H=0), dict(W=0), dict(H=65536, W=65536), dict(inp=None), dict(flow=None), dict(out=None),
                dict(scratch=None), dict(scratch=FAKE + 8), dict(nbytes=0), dict(nbytes=need - 1),
                dict(H=40000, W=40000, nbytes=2 ** 62), dict(H=1, W=2 ** 30, nbytes=2 ** 62)):
        assert splat(**bad) == N.MOM_EINVAL, bad
    # the host twins refuse the same shapes and null pointers
    g = np.zeros(16, np.float32).ctypes.data
    host = lib.mom_eulerian_blend_ordered_host
    for args in ((0, 16, 16, 2, 5, g, g, g), (3, 16, 17, 2, 5, g, g, g), (3, 16, 16, 5, 5, g, g, g), (3, 16, 16, 0, 1, g, g, g),
                 (3, 16, 16, 2, 5, None, g, g), (3, 16, 16, 2, 5, g, None, g), (3, 16, 16, 2, 5, g, g, None), (1, 20000, 20000, 2, 5, g, g, g)):
        assert host(*args) == N.MOM_EINVAL, args
    host = lib.mom_softsplat_sum_ordered_host
    for args in ((0, 3, 5, 7, g, g, g), (2, 0, 5, 7, g, g, g), (2, 3, 0, 7, g, g, g), (2, 3, 5, 7, None, g, g), (2, 3, 5, 7, g, None, g),
                 (2, 3, 5, 7, g, g, None), (1, 1, 40000, 40000, g, g, g)):
        assert host(*args) == N.MOM_EINVAL, args


@pytest.mark.parametrize("kind", oc.MOTIONS)
@pytest.mark.parametrize("S", [16, 32])
def test_the_blend_host_twin_adds_in_the_documented_order(S, kind):
    longest = 0
    for C in (1, 3):
        f, m = oc.features(C, S), oc.motion(kind, S)
        for idx in oc.IDX:
            want, cell = oc.blend_numpy(f, m, idx, oc.N_FRAMES)
            got = oc.blend_host(f, m, idx, oc.N_FRAMES)
            np.testing.assert_array_equal(oc.bits(got), oc.bits(want), err_msg=f"C {C} idx {idx}")
            longest = max(longest, cell)
    P = ec.geometry(S)[2]
    if kind == "zero":
        assert longest == 2                               # one entry per half in every cell
    if kind == "converge":                                # several blocks in one class: more than 64 entries, and more than 1024
        assert longest > (64 if S == 16 else 1024), longest
        # ... and the blocks are part of the order: one left-to-right sum over that cell differs somewhere
        f, m = oc.features(3, S), oc.motion(kind, S)
        ox, oy, src, _ = oc.blend_targets(m, S, 2, oc.N_FRAMES)
        cut, pad = ec.geometry(S)[:2]
        c = pad + S // 2 - cut                            # the padded pixel the chains rest on
        inside = np.flatnonzero((np.floor(ox) == c) & (np.floor(oy) == c))
        assert oc.BLOCK < len(inside) <= longest            # (at idx 2; the last frame gathers more)
        w = ((np.float32(c + 1) - ox[inside]).astype(np.float32) * (np.float32(c + 1) - oy[inside]).astype(np.float32)).astype(np.float32)
        terms = ((f.reshape(3, -1)[:, src[inside]].T * np.float32(0.5)).astype(np.float32) * w[:, None]).astype(np.float32)
        seq, blocked = np.zeros(3, np.float32), np.zeros(3, np.float32)
        for j in range(0, len(terms), oc.BLOCK):
            b = np.zeros(3, np.float32)
            for t in terms[j:j + oc.BLOCK]:
                b, seq = b + t, seq + t
            blocked = blocked + b
        assert (oc.bits(seq) != oc.bits(blocked)).any()
    if kind == "leave":
        assert longest >= 2


def test_the_splat_host_twin_adds_in_the_documented_order_onto_a_nonzero_output():
    inp, flw, out_in = oc.splat_inputs(2, 3, 5, 7)
    want = oc.splat_numpy(inp, flw, out_in)
    got = oc.splat_host(inp, flw, out_in)
    np.testing.assert_array_equal(oc.bits(got), oc.bits(want))
    untouched = (oc.bits(want) == oc.bits(out_in)).all(axis=1)
    assert untouched.any() and not untouched.all()        # texels without a term keep their bits; the others moved
    # the dropped entries (NaN, inf, 3e30, -2^31) left nothing non-finite behind
    assert np.isfinite(got).all()


@pytest.mark.parametrize("S,C,n_frames,idx", [(32, 3, 6, 0), (32, 3, 6, 1), (32, 3, 6, 3), (32, 3, 6, 5), (256, 2, 8, 4)])
def test_the_host_twin_lies_within_the_summation_bound_of_the_float64_sums(S, C, n_frames, idx):
    b = ec.case(S, C, n_frames, idx)
    acc = oc.blend_host(b["feature"], b["motion"], idx, n_frames)
    den = acc[:, :, C]
    blank = den == 0
    assert np.array_equal(blank, b["blank"])              # every element: a texel is blank iff no term reached it
    assert np.array_equal(oc.bits(acc[blank]), np.zeros_like(oc.bits(acc[blank])))         # ... and then holds +0.0 in every channel
    with np.errstate(divide="ignore", invalid="ignore"):
        got = (acc[:, :, :C] / den[:, :, None]).transpose(2, 0, 1)
    d = np.abs(got.astype(np.float64) - b["blended"])
    keep = np.broadcast_to(~blank[None], d.shape)
    bound = ec.bound_blend(b)
    print(f"S {S} C {C} idx {idx}: k max {int(b['k'].max())}, largest |d| / bound {float((d[keep] / bound[keep]).max()):.3g}")
    assert (d[keep] <= bound[keep]).all()


def test_the_python_layers_take_the_argument():
    cg, ops, motion = (importlib.import_module(f"{oc.pkg}.{m}") for m in ("cinemagraph", "ops", "motion"))
    for fn in (ops.softsplat_sum, ops.eulerian_blend, cg.FunctionSoftsplat, cg.ModuleSoftsplat.forward, cg.joint_splatting,
               cg.blend_feature, cg.feature_inpaint_conv, cg.warp_one_level, cg.pixel_video_frames, cg.pixel_video,
               motion.write_pixel_video, motion.build_stage1):
        p = inspect.signature(fn).parameters
        assert list(p)[-1] == "ordered" and p["ordered"].default is None, fn.__name__     # last and optional: the reference's calls stand
    assert "warp" in RC.set_deterministic.__doc__
    assert RC.deterministic() is False
    try:
        with pytest.raises(OSError):                       # the switch is set before any work: here, before the folder is missed
            motion.main(["--deterministic", "--video", "pixels", "--input_dir", "/nonexistent/folder"])
        assert RC.deterministic() is True
    finally:
        RC.set_deterministic(False)
