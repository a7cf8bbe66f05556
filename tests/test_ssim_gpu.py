"""The SSIM kernels (csrc/ssim.hip) against float64 within the derived per-pixel bound of tests/ssim_cases.py, at tile seams, on flat
images, where the partial-sum slots wrap and on row slabs; and the call paths of the C entries on their own.  Nothing here is
larger than 128 x 128.  tests/test_ssim_cpu.py shows that the bound holds two float32 evaluations and catches nine planted faults.

  test                                              what it reaches
  every family, every shape                         sum[0], the 63 slots, dm's three maps, the gradient at scale 1 and at -0.2 / n,
                                                    ops.ssim's value and gradient -- each pixel against its own bound
  impulses                                          which pixels a window reaches, from both sides of the seam at 16: exact zeros
  dm == NULL, scale_dev, accumulation, zero sizes   bit-for-bit statements about the call paths
  slabs                                             every rank of three splits of a 96- and a 90-row image as FusedStep forms the
                                                    arguments, one slab that starts on no multiple of 16, one split with an empty rank"""
import importlib

import numpy as np
import pytest
import torch

import ssim_cases as sc

pytestmark = pytest.mark.gpu

ops = importlib.import_module(sc.pkg + ".ops")
N = importlib.import_module(sc.pkg + "._native")
WIN = ops.ssim_window()
SENTINEL = 0x7FC5A5A5         # a quiet NaN no arithmetic produces: memory the kernels must leave alone
GUARD = 4096                  # floats in front of and behind every buffer a slab call writes
LAMBDA = 0.2                  # lambda_dssim of the fine stage


def _dev(a):
    return torch.from_numpy(np.array(sc.fold(a))).cuda()          # (a copy: the cases are read-only)


def _sentinel(n):
    return torch.full((n,), SENTINEL, dtype=torch.int32, device="cuda").view(torch.float32)


def _bits(t):
    return t.contiguous().view(torch.int32).cpu().numpy()


def _forward(x, y, want_dm=True):
    """mom_ssim_forward on [C,H,W] device images: (dm or None, the 64 doubles)."""
    C, H, W = x.shape
    dm = torch.empty((3, C, H, W), dtype=torch.float32, device="cuda") if want_dm else None
    total = torch.full((sc.SLOTS,), 123.0, dtype=torch.float64, device="cuda")            # the call clears it
    N.check(N.lib().mom_ssim_forward(C, H, W, WIN, x.data_ptr(), y.data_ptr(), None if dm is None else dm.data_ptr(),
                                     total.data_ptr(), N.current_stream()), "mom_ssim_forward")
    torch.cuda.synchronize()
    return dm, total.cpu().numpy()


def _backward(x, y, dm, scale, scale_dev=None, into=None):
    C, H, W = x.shape
    out = torch.zeros_like(x) if into is None else into
    N.check(N.lib().mom_ssim_backward(C, H, W, WIN, x.data_ptr(), y.data_ptr(), dm.data_ptr(), scale,
                                      None if scale_dev is None else scale_dev.data_ptr(), out.data_ptr(), N.current_stream()),
            "mom_ssim_backward")
    torch.cuda.synchronize()
    return out


def _loss_scale(c):
    """-lambda / n as the float the step passes."""
    return float(np.float32(-LAMBDA / c["ref"]["map"].size))


def _check_case(c, worst):
    """One case through the C entries and through ops.ssim; adds its error / bound ratios to `worst`."""
    ref, bnd = c["ref"], c["bnd"]
    n = ref["map"].size
    x, y = _dev(c["img"]), _dev(c["gt"])
    dm, slots = _forward(x, y)
    want, e = sc.slot_ref_bound(ref, bnd)
    got = {"sum": abs(slots[0] - want[0]) / e[0], "slots": sc.share(slots[1:], want[1:], e[1:])}
    assert abs(slots[1:].sum() - slots[0]) <= 2.0 ** -46 * np.abs(slots[1:]).sum()           # 63 doubles, added in another order
    for i in range(3):
        got["dm%d" % i] = sc.share(dm[i].cpu().numpy(), ref["dm"][i], bnd["dm"][i])
    for name, s in (("grad", 1.0), ("grad_loss", _loss_scale(c))):
        got[name] = sc.share(_backward(x, y, dm, s).cpu().numpy(), s * ref["grad"], sc.grad_bound(ref, bnd, s))
    # the autograd op: the value as the float it returns; the gradient of lambda (1 - ssim), whose scale is fl(1 / n) * fl(-lambda):
    # two more roundings than grad_bound counts
    xa = torch.from_numpy(np.array(c["img"])).cuda().requires_grad_(True)
    v = ops.ssim(xa, torch.from_numpy(np.array(c["gt"])).cuda())
    (LAMBDA * (1.0 - v)).backward()
    got["value"] = abs(float(v.detach()) - want[0] / n) / sc.value_bound(ref, bnd)
    s = -LAMBDA / n
    got["ops_grad"] = sc.share(sc.fold(xa.grad.cpu().numpy()), s * ref["grad"],
                               sc.grad_bound(ref, bnd, s) + 2 * sc.EPS * np.abs(s * ref["grad"]))
    for k, v in got.items():
        worst[k] = max(worst.get(k, 0.0), v)


@pytest.mark.parametrize("fam", sc.FAMILIES)
def test_every_case_of_the_family_lies_inside_the_bound_at_every_pixel(fam):
    worst = {}
    for name, shape, _ in sc.CASES:
        if name == fam:
            _check_case(sc.case(name, shape), worst)
    print("\nssim error/bound  %-12s kernel %s" % (fam, " ".join("%s %.3f" % kv for kv in worst.items())))
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize("shape", sc.IMPULSE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_an_impulse_reaches_five_pixels_in_the_maps_and_ten_in_the_gradient(shape):
    """img one 1.0 on zeros, gt zero, at the corners, on both sides of the seam at 16 in both directions, in the last row and column
    and in the centre: dm and the gradient within the bound, and where float64 is exactly 0 -- d map / d mu1 farther than 5 pixels
    from the impulse, the gradient farther than 10 -- the kernel's value is exactly 0 (a tile that read a neighbour's column, or a
    window one tap too wide, puts something there)."""
    H, W = shape[-2:]
    rr, cc = np.mgrid[0:H, 0:W]
    worst = {}
    for r, c_ in sc.impulse_positions(shape):
        c = sc.impulse_case(shape, r, c_)
        ref, bnd = c["ref"], c["bnd"]
        x, y = _dev(c["img"]), _dev(c["gt"])
        dm, slots = _forward(x, y)
        grad = _backward(x, y, dm, 1.0).cpu().numpy()
        dm = dm.cpu().numpy()
        got = {"dm%d" % i: sc.share(dm[i], ref["dm"][i], bnd["dm"][i]) for i in range(3)}
        got["grad"] = sc.share(grad, ref["grad"], bnd["grad"])
        s, e = sc.sum_ref_bound(ref, bnd)
        got["sum"] = abs(slots[0] - s) / e
        assert max(got.values()) <= 1.0, ((r, c_), got)
        dist = np.maximum(np.abs(rr - r), np.abs(cc - c_))[None]
        far5, far10 = dist > sc.RADIUS, dist > 2 * sc.RADIUS
        assert (ref["dm"][0][far5] == 0).all() and (bnd["dm"][0][far5] == 0).all() and (ref["dm"][0][~far5] != 0).all()
        assert (dm[0][far5] == 0).all(), (r, c_)
        assert (ref["grad"][far10] == 0).all() and (bnd["grad"][far10] == 0).all() and (ref["grad"][~far10] != 0).all()
        assert (grad[far10] == 0).all(), (r, c_)
        for k, v in got.items():
            worst[k] = max(worst.get(k, 0.0), v)
    print("\nssim error/bound  impulse %-9s kernel %s" % ("x".join(map(str, shape)), " ".join("%s %.3f" % kv for kv in worst.items())))


@pytest.mark.parametrize("shape", sc.WRAP_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_the_partial_sums_wrap_onto_their_slots(shape):
    """63, 64 and 120 blocks: every slot holds the float64 sum of ITS blocks (b, b + 63) within their bound, and the slots add up to
    sum[0].  (The family test compares the same; this one also pins which slots are in use.)"""
    c = sc.case("noise", shape)
    _, slots = _forward(_dev(c["img"]), _dev(c["gt"]))
    want, e = sc.slot_ref_bound(c["ref"], c["bnd"])
    blocks = sc.blocks_of(shape)
    assert (want[1:] != 0).sum() == min(blocks, sc.SLOTS - 1) and (slots[1:] != 0).all()
    assert sc.share(slots, want, e) <= 1.0
    assert abs(slots[1:].sum() - slots[0]) <= 2.0 ** -46 * np.abs(slots[1:]).sum()
    # every block's share is far outside the bound of the slot it belongs to: a block lost or added twice cannot pass
    per_block, _ = sc.block_ref_bound(c["ref"], c["bnd"])
    assert (np.abs(per_block) > 10 * e[1 + np.arange(blocks) % (sc.SLOTS - 1)]).all()


def test_the_forward_without_dm_returns_the_same_sum():
    for name, shape in (("noise", (3, 37, 53)), ("flat_white", (3, 37, 53)), ("noise", (4, 65, 81))):
        c = sc.case(name, shape)
        x, y = _dev(c["img"]), _dev(c["gt"])
        _, with_dm = _forward(x, y)
        _, without = _forward(x, y, want_dm=False)
        n = x.numel()
        assert np.float32(with_dm[0] / n) == np.float32(without[0] / n) and np.float32(with_dm[0]) == np.float32(without[0])
        assert np.array_equal(with_dm, without)               # (a block's float sum is exact in a double: the order cannot show)


def test_a_scale_on_the_device_is_the_same_scale():
    c = sc.case("noise", (3, 37, 53))
    x, y = _dev(c["img"]), _dev(c["gt"])
    dm, _ = _forward(x, y)
    s = _loss_scale(c)
    dev = lambda v: torch.tensor([v], dtype=torch.float32, device="cuda")
    plain = _bits(_backward(x, y, dm, s))
    assert np.abs(plain).max() > 0
    assert np.array_equal(plain, _bits(_backward(x, y, dm, 1.0, dev(s))))
    assert np.array_equal(plain, _bits(_backward(x, y, dm, s, dev(1.0))))
    assert np.array_equal(plain, _bits(_backward(x, y, dm, 0.5, dev(2.0 * s))))        # neither factor 1: 0.5 * 2 s is exact


def test_the_backward_adds_into_what_the_buffer_holds():
    """dimg1 += scale * t compiles to ONE fused multiply-add per pixel, so on a buffer that holds noise the result is
    fl(noise + scale t), one rounding -- not the float32 sum of the noise and the zero-filled run's fl(scale t), which rounds twice
    and differs from it in the last bit of about a quarter of the pixels.  t itself is the zero-filled run at scale 1, exactly; the
    expected bits are ssim_cases.fma32's.  Two calls add twice."""
    c = sc.case("noise", (3, 37, 53))
    x, y = _dev(c["img"]), _dev(c["gt"])
    dm, _ = _forward(x, y)
    s = np.float32(_loss_scale(c))
    t = _backward(x, y, dm, 1.0).cpu().numpy()
    noise = (1e-3 * torch.randn(x.shape, generator=torch.Generator().manual_seed(7))).numpy()          # the size of an L1 gradient
    zero_filled = _backward(x, y, dm, float(s)).cpu().numpy()
    assert np.array_equal(zero_filled.view(np.int32), sc.fma32(s, t, np.zeros_like(t)).view(np.int32))
    buf = torch.from_numpy(noise.copy()).cuda()
    _backward(x, y, dm, float(s), into=buf)
    once = sc.fma32(s, t, noise)
    assert np.array_equal(_bits(buf), once.view(np.int32))
    assert (once != noise + zero_filled).any()                # the two-rounding sum is a different statement ...
    assert (np.abs(once - (noise + zero_filled)) <= np.spacing(np.abs(once)) + np.spacing(np.abs(zero_filled))).all()   # ... an ulp away
    _backward(x, y, dm, float(s), into=buf)
    assert np.array_equal(_bits(buf), sc.fma32(s, t, once).view(np.int32))


def test_calls_without_pixels_clear_the_sum_and_touch_nothing_else():
    lib = N.lib()
    for C, H, W in ((0, 8, 8), (3, 0, 8), (3, 8, 0)):
        dm, dimg, img = _sentinel(3 * 192 + 64), _sentinel(192 + 64), _sentinel(192 + 64)
        total = torch.full((sc.SLOTS + 8,), 123.0, dtype=torch.float64, device="cuda")
        assert lib.mom_ssim_forward(C, H, W, WIN, img.data_ptr(), img.data_ptr(), dm.data_ptr(), total.data_ptr(),
                                    N.current_stream()) == N.MOM_OK
        assert lib.mom_ssim_backward(C, H, W, WIN, img.data_ptr(), img.data_ptr(), dm.data_ptr(), 1.0, None, dimg.data_ptr(),
                                     N.current_stream()) == N.MOM_OK
        assert lib.mom_ssim_forward_slab(C, H, W, 64, 0, H, 0, H, WIN, None, None, None, total.data_ptr(), N.current_stream()) == N.MOM_OK
        torch.cuda.synchronize()
        t = total.cpu().numpy()
        assert (t[:sc.SLOTS] == 0).all() and (t[sc.SLOTS:] == 123.0).all()
        for buf in (dm, dimg, img):
            assert (_bits(buf) == SENTINEL).all()
    # with pixels, the images are needed (the sum is cleared first: that is a launch, so this refusal needs a device)
    total = torch.zeros(sc.SLOTS, dtype=torch.float64, device="cuda")
    assert lib.mom_ssim_forward(1, 4, 4, WIN, None, total.data_ptr(), None, total.data_ptr(), N.current_stream()) == N.MOM_EINVAL
    torch.cuda.synchronize()


def test_cpu_tensors_are_refused():
    c = sc.case("noise", (3, 5, 7))
    with pytest.raises(N.MomError):
        ops.ssim(torch.from_numpy(np.array(c["img"])), torch.from_numpy(np.array(c["gt"])))


# ------------------------------------------------------------------------------------------------------------ row slabs
_WHOLE = {}


def _whole(shape):
    """The whole-image call on a slab image: dm, gradient at the loss's scale, the 64 doubles (computed once)."""
    if shape not in _WHOLE:
        c = sc.case("noise", shape)
        x, y = _dev(c["img"]), _dev(c["gt"])
        dm, slots = _forward(x, y)
        _WHOLE[shape] = dict(c=c, x=x, y=y, dm=_bits(dm), grad=_bits(_backward(x, y, dm, _loss_scale(c))), slots=slots)
    return _WHOLE[shape]


def _run_slab(shape, a):
    """mom_ssim_forward_slab and _backward_slab on full-image buffers between guard bands; the rows of dimg1 inside the slab start
    at zero, everything else holds the sentinel.  Checks all that is stated about one slab; returns (sum[0], its float64 value, its
    bound)."""
    wh = _whole(shape)
    c, ref, bnd = wh["c"], wh["c"]["ref"], wh["c"]["bnd"]
    C, H, W = shape
    n = C * H * W
    ys0, ys1 = a["slab"]
    # what the kernels address stays inside the buffers: the last element is channel C - 1 (map 2), slab row H_slab - 1
    assert a["off"] == ys0 * W and a["H"] == ys1 - ys0 and 0 <= ys0 <= ys1 <= H
    assert a["off"] + (C - 1) * H * W + a["H"] * W <= n
    dm_buf, dimg_buf = _sentinel(GUARD + 3 * n + GUARD), _sentinel(GUARD + n + GUARD)
    dimg_buf[GUARD:GUARD + n].view(C, H, W)[:, ys0:ys1] = 0
    total = torch.full((sc.SLOTS,), 123.0, dtype=torch.float64, device="cuda")
    lib, s = N.lib(), N.current_stream()
    x_ptr, y_ptr = wh["x"].data_ptr() + 4 * a["off"], wh["y"].data_ptr() + 4 * a["off"]
    dm_ptr, dimg_ptr = dm_buf.data_ptr() + 4 * (GUARD + a["off"]), dimg_buf.data_ptr() + 4 * (GUARD + a["off"])
    N.check(lib.mom_ssim_forward_slab(C, a["H"], W, H * W, a["sum"][0], a["sum"][1], a["dm"][0], a["dm"][1], WIN, x_ptr, y_ptr, dm_ptr,
                                      total.data_ptr(), s), "ssim_fwd_slab")
    N.check(lib.mom_ssim_backward_slab(C, a["H"], W, H * W, WIN, x_ptr, y_ptr, dm_ptr, _loss_scale(c), None, dimg_ptr, s), "ssim_bwd_slab")
    torch.cuda.synchronize()
    dm_all, dimg_all = _bits(dm_buf), _bits(dimg_buf)
    dm, dimg = dm_all[GUARD:GUARD + 3 * n].reshape(3, C, H, W), dimg_all[GUARD:GUARD + n].reshape(C, H, W)
    # nothing outside the slab is written: the guard bands, the rows in front of the slab's pointer, and the rows behind the slab
    # in every channel of every map (the gap chan_stride leaves)
    for buf, size in ((dm_all, 3 * n), (dimg_all, n)):
        assert (buf[:GUARD] == SENTINEL).all() and (buf[GUARD + size:] == SENTINEL).all()
    outside = np.ones(H, bool)
    outside[ys0:ys1] = False
    assert (dm[:, :, outside] == SENTINEL).all() and (dimg[:, outside] == SENTINEL).all()
    assert not (dm[:, :, ys0:ys1] == SENTINEL).any() and not (dimg[:, ys0:ys1] == SENTINEL).any()
    # dm: the whole image's bits on the rows of [dm_row0, dm_row1) whose window is inside the slab or cut by an image edge; zero on
    # the slab's other rows
    rows = sc.dm_rows_that_match(a, H)
    assert rows.size and np.array_equal(dm[:, :, rows], wh["dm"][:, :, rows])
    zero = ~outside
    zero[ys0 + a["dm"][0]:ys0 + a["dm"][1]] = False
    assert (dm[:, :, zero].view(np.float32) == 0).all()
    # dimg1: the whole image's gradient on the own rows, bit for bit
    g0, g1 = a["grad"]
    assert g1 > g0 and np.array_equal(dimg[:, g0:g1], wh["grad"][:, g0:g1])
    got = total.cpu().numpy()
    want, e = sc.sum_ref_bound(ref, bnd, (ys0 + a["sum"][0], ys0 + a["sum"][1]))
    assert abs(got[0] - want) <= e, (got[0], want, e)
    assert abs(got[1:].sum() - got[0]) <= 2.0 ** -46 * np.abs(got[1:]).sum()
    return got[0], want, e


@pytest.mark.parametrize("shape", sc.SLAB_IMAGES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("split", range(len(sc.SLAB_SPLITS)))
def test_every_rank_of_a_split_computes_its_rows_of_the_whole_image(shape, split):
    """The arguments FusedStep forms for a tile-row shard (ssim_cases.slab_args): per rank everything _run_slab states; and the ranks'
    sums add up to the whole image's, within the summed bounds."""
    wh = _whole(shape)
    parts = [_run_slab(shape, sc.slab_args(shape[1], shape[2], rows)) for rows in sc.SLAB_SPLITS[split]]
    whole, e_whole = sc.sum_ref_bound(wh["c"]["ref"], wh["c"]["bnd"])
    assert abs(sum(p[1] for p in parts) - whole) <= 1e-12 * abs(whole)          # the ranks' rows are the image's, once each
    assert abs(sum(p[0] for p in parts) - whole) <= sum(p[2] for p in parts)
    assert abs(sum(p[0] for p in parts) - wh["slots"][0]) <= sum(p[2] for p in parts) + e_whole


def test_a_slab_that_starts_on_no_multiple_of_16():
    """Rows 23..71 of the 96-row image, sum and dm rows 28..66: every tile of the slab lies 7 rows off the whole image's, and dm and
    the gradient are still the whole image's bits -- a pixel's arithmetic does not depend on where its tile lies."""
    _run_slab(sc.SLAB_IMAGES[0], sc.unaligned_slab(sc.SLAB_IMAGES[0][2]))


def test_a_rank_without_rows_leaves_a_cleared_sum():
    """FusedStep makes no SSIM call for a rank whose split gave it no tile row and zeroes its sum; a slab call without rows does the
    same and writes nothing.  The other ranks' sums still add up to the whole image's."""
    shape = sc.SLAB_IMAGES[0]
    C, H, W = shape
    wh = _whole(shape)
    dm, dimg = _sentinel(1024), _sentinel(1024)
    total = torch.full((sc.SLOTS,), 123.0, dtype=torch.float64, device="cuda")
    off = 4 * 48 * W
    lib, s = N.lib(), N.current_stream()
    assert lib.mom_ssim_forward_slab(C, 0, W, H * W, 0, 0, 0, 0, WIN, wh["x"].data_ptr() + off, wh["y"].data_ptr() + off, dm.data_ptr(),
                                     total.data_ptr(), s) == N.MOM_OK
    assert lib.mom_ssim_backward_slab(C, 0, W, H * W, WIN, wh["x"].data_ptr() + off, wh["y"].data_ptr() + off, dm.data_ptr(), 1.0, None,
                                      dimg.data_ptr(), s) == N.MOM_OK
    torch.cuda.synchronize()
    assert (total.cpu().numpy() == 0).all() and (_bits(dm) == SENTINEL).all() and (_bits(dimg) == SENTINEL).all()
    parts = [_run_slab(shape, sc.slab_args(H, W, rows)) for rows in ((0, 3), (3, 6))]          # the split (0,3) (3,3) (3,6)
    whole, _ = sc.sum_ref_bound(wh["c"]["ref"], wh["c"]["bnd"])
    assert abs(sum(p[0] for p in parts) + 0.0 - whole) <= sum(p[2] for p in parts)
