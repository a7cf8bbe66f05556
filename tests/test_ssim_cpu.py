"""The SSIM kernels' yardstick without a GPU (tests/ssim_cases.py): the float64 reference against the oracle, the derived bound
against two float32 evaluations on every pixel of every case, the planted faults the bound must catch, and what the C entries
refuse before anything is launched."""
import importlib

import numpy as np
import pytest
import torch

import ssim_cases as sc
from oracle import torch_ref as tr

N = importlib.import_module(sc.pkg + "._native")
FAKE = 0x10000        # a pointer that is never dereferenced: every call below is refused first

ALL = [(n, s) for n, s, _ in sc.CASES]
IDS = ["%s-%s" % (n, "x".join(map(str, s))) for n, s in ALL]
IMPULSES = [(s, r, c) for s in sc.IMPULSE_SHAPES for r, c in sc.impulse_positions(s)]


def _oracle(img, gt, dtype):
    """oracle/torch_ref.ssim and its gradient: (mean, d mean / d img) in `dtype`."""
    x = torch.from_numpy(np.array(img)).to(dtype).requires_grad_(True)
    y = torch.from_numpy(np.array(gt)).to(dtype)
    v = tr.ssim(x if x.dim() == 4 else x[None], y if y.dim() == 4 else y[None])
    v.backward()
    return float(v.detach()), sc.fold(x.grad.numpy())


def test_the_case_table_holds_what_it_is_for():
    assert {n for n, _ in ALL} == set(sc.FAMILIES)
    assert [sc.blocks_of(s) for s in sc.WRAP_SHAPES] == [63, 64, 120]
    shapes = {s for _, s in ALL}
    assert {(1, 1, 1), (1, 1, 40), (1, 40, 1), (3, 5, 7), (1, 11, 11), (1, 15, 17), (1, 16, 16), (1, 17, 15), (2, 32, 48), (3, 37, 53),
            (2, 3, 21, 33)} | set(sc.WRAP_SHAPES) <= shapes
    for s in sc.IMPULSE_SHAPES:
        H, W = s[-2:]
        pos = sc.impulse_positions(s)
        assert {(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (15, 15), (15, 16), (16, 15), (16, 16), (H // 2, W // 2)} <= set(pos)
        assert all(0 <= r < H and 0 <= c < W for r, c in pos)
    for name, shape in ALL:                                  # seeded: a case is a function of its name and shape
        a, b = sc.family(name, shape), sc.family(name, shape)
        assert a[0].dtype == np.float32 and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert sc.family("overshoot", (3, 37, 53))[0].min() < 0 and sc.family("overshoot", (3, 37, 53))[0].max() > 1
    # the slabs: every rank of every split, with the halo and the five rows the step gives them
    assert sc.slab_args(96, 40, (2, 4)) == dict(slab=(16, 80), own=(32, 64), sum=(16, 48), dm=(11, 53), off=640, H=64, grad=(32, 64))
    assert sc.slab_args(90, 40, (5, 6)) == dict(slab=(64, 90), own=(80, 90), sum=(16, 26), dm=(11, 26), off=2560, H=26, grad=(80, 90))
    assert sc.slab_args(96, 40, (0, 1))["dm"] == (0, 21)


@pytest.mark.parametrize("name,shape", ALL, ids=IDS)
def test_reference64_is_the_oracle_in_float64(name, shape):
    """reference64 with the oracle's window (the float32 roundings of w_i w_j) against oracle/torch_ref.ssim on .double() inputs:
    the mean to 1e-12 relative, the gradient to 1e-12 of the terms it sums.  The separable form the other tests use differs from
    it by the window's rounding alone: at most u blur|t| in every moment."""
    c = sc.case(name, shape)
    w = c["w"]
    w2d = np.outer(w, w).astype(np.float32).astype(np.float64)             # g.mm(g.t()).float() of the oracle
    assert np.array_equal(w2d, (torch.from_numpy(w)[:, None].mm(torch.from_numpy(w)[None, :])).double().numpy())
    r = sc.reference64(c["img"], c["gt"], w, window2d=w2d)
    v, g = _oracle(c["img"], c["gt"], torch.float64)
    n = r["map"].size
    assert abs(r["sum"] / n - v) <= 1e-12 * abs(v), (r["sum"] / n, v)
    adm = np.abs(r["dm"])
    b = lambda a: sc.blur64(a, w, w2d)
    terms = b(adm[0]) + 2 * np.abs(r["x"]) * b(adm[1]) + np.abs(r["y"]) * b(adm[2])
    assert np.abs(r["grad"] - g * n).max() <= 1e-12 * terms.max(), (np.abs(r["grad"] - g * n).max(), terms.max())
    sep = c["ref"]
    for key, t in (("mu1", np.abs(sep["x"])), ("mu2", np.abs(sep["y"])), ("e11", sep["x"] ** 2), ("e22", sep["y"] ** 2),
                   ("e12", np.abs(sep["x"] * sep["y"]))):
        assert (np.abs(sep[key] - r[key]) <= sc.EPS * sc.blur64(t, w) * (1 + 1e-9)).all(), key


@pytest.mark.parametrize("shape,label,a,rows", sc.slab_list(), ids=[s[1] for s in sc.slab_list()])
def test_reference64_of_a_slab_is_the_full_image_on_the_rows_that_count(shape, label, a, rows):
    """The slab alone, zero-padded at its own edges: its map on the sum rows, its dm on the dm rows and its gradient on the own
    rows are the full image's.  (This is a statement about the ARGUMENTS: a halo or a dm interval too small breaks it.)"""
    c = sc.case("noise", shape)
    full, s = c["ref"], sc.slab_reference64(c, a)
    ys0 = a["slab"][0]
    close = lambda got, want: np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
    assert close(s["map"][:, a["sum"][0]:a["sum"][1]], full["map"][:, ys0 + a["sum"][0]:ys0 + a["sum"][1]])
    rows = sc.dm_rows_that_match(a, shape[1])
    assert np.array_equal(rows, np.arange(a["dm"][0], a["dm"][1]) + ys0)       # every dm row kept is a true one
    assert close(s["dm"][:, :, rows - ys0], full["dm"][:, :, rows])
    g0, g1 = a["grad"]
    assert g1 > g0 and close(s["grad"][:, g0 - ys0:g1 - ys0], full["grad"][:, g0:g1])


def _shares32(c, r):
    ref, bnd = c["ref"], c["bnd"]
    s, es = sc.sum_ref_bound(ref, bnd)
    return dict(map=sc.share(r["map"], ref["map"], bnd["map"]), dm0=sc.share(r["dm"][0], ref["dm"][0], bnd["dm"][0]),
                dm1=sc.share(r["dm"][1], ref["dm"][1], bnd["dm"][1]), dm2=sc.share(r["dm"][2], ref["dm"][2], bnd["dm"][2]),
                grad=sc.share(r["grad"], ref["grad"], bnd["grad"]), sum=abs(r["sum"] - s) / es if es > 0 else float(r["sum"] != s))


def _oracle32_shares(c):
    ref, bnd = c["ref"], c["bnd"]
    v, g = _oracle(c["img"], c["gt"], torch.float32)
    n = ref["map"].size
    s, _ = sc.sum_ref_bound(ref, bnd)
    # d mean / d img: scale 1 / n, formed by autograd in float32
    return dict(value=abs(v - s / n) / sc.value_bound(ref, bnd), grad=sc.share(g, ref["grad"] / n, sc.grad_bound(ref, bnd, 1.0 / n)))


@pytest.mark.parametrize("fam", sc.FAMILIES + ("impulse",))
def test_both_float32_evaluations_lie_inside_the_bound_at_every_pixel(fam):
    """restatement32 (map, three derivative maps, gradient, sum) and the float32 oracle (value, gradient) against reference64
    within `bound`, no pixel excused; the first-order condition on A B holds on every case.  Prints the family's worst ratios."""
    if fam == "impulse":
        cases = [sc.impulse_case(*k) for k in IMPULSES]
    else:
        cases = [sc.case(n, s) for n, s in ALL if n == fam]
    worst_r, worst_o = {}, {}
    for c in cases:
        assert c["bnd"]["ab_rel"] < 0.125
        for k, v in _shares32(c, sc.restatement32(c["img"], c["gt"], c["w"])).items():
            worst_r[k] = max(worst_r.get(k, 0.0), v)
        for k, v in _oracle32_shares(c).items():
            worst_o[k] = max(worst_o.get(k, 0.0), v)
    print("\nssim error/bound  %-12s restatement32 %s | oracle float32 %s | A B perturbed by <= %.1e"
          % (fam, " ".join("%s %.3f" % kv for kv in worst_r.items()), " ".join("%s %.3f" % kv for kv in worst_o.items()),
             max(c["bnd"]["ab_rel"] for c in cases)))
    assert max(worst_r.values()) <= 1.0, worst_r
    assert max(worst_o.values()) <= 1.0, worst_o


def _slab_shares(c, a, r, H):
    """A slab evaluation (slab coordinates) against the FULL image's reference and bound, on the rows that count."""
    ref, bnd = c["ref"], c["bnd"]
    ys0 = a["slab"][0]
    rows = sc.dm_rows_that_match(a, H)
    g0, g1 = a["grad"]
    s, es = sc.sum_ref_bound(ref, bnd, (ys0 + a["sum"][0], ys0 + a["sum"][1]))
    out = dict(grad=sc.share(r["grad"][:, g0 - ys0:g1 - ys0], ref["grad"][:, g0:g1], bnd["grad"][:, g0:g1]), sum=abs(r["sum"] - s) / es)
    for i in range(3):
        out["dm%d" % i] = sc.share(r["dm"][i][:, rows - ys0], ref["dm"][i][:, rows], bnd["dm"][i][:, rows])
    return out


def _slab32(c, a):
    ys0, ys1 = a["slab"]
    return sc.restatement32(sc.fold(c["img"])[:, ys0:ys1], sc.fold(c["gt"])[:, ys0:ys1], c["w"], a["sum"], a["dm"])


def test_restatement32_of_every_slab_lies_inside_the_full_images_bound():
    worst = {}
    for shape, label, a, _ in sc.slab_list():
        c = sc.case("noise", shape)
        r = _slab32(c, a)
        for k, v in _slab_shares(c, a, r, shape[1]).items():
            worst[k] = max(worst.get(k, 0.0), v)
        out = np.ones(a["H"], bool)
        out[a["dm"][0]:a["dm"][1]] = False
        assert not r["dm"][:, :, out].any()
    print("\nssim error/bound  slabs        restatement32 " + " ".join("%s %.3f" % kv for kv in worst.items()))
    assert max(worst.values()) <= 1.0, worst


def test_every_planted_fault_breaks_the_bound_somewhere():
    """What shows that the GPU tests can fail: each defect, planted in restatement32, leaves the bound on at least one listed
    case.  Every fault is tried on every case of at most 6000 pixels (and on the slot-wrapping shapes); the slab fault on every
    slab.  Prints which cases catch which fault."""
    small = [(n, s) for n, s in ALL if np.prod(s) <= 6000] + [("noise", s) for s in sc.WRAP_SHAPES]
    caught = {}
    for fault in sc.FAULTS:
        for n, s in small:
            c = sc.case(n, s)
            sh = _shares32(c, sc.restatement32(c["img"], c["gt"], c["w"], fault=fault))
            if max(sh.values()) > 1.0:
                caught.setdefault(fault, []).append(("%s-%s" % (n, "x".join(map(str, s))), max(sh, key=sh.get)))
    for shape, label, a, rows in sc.slab_list():
        if rows is None:
            continue
        c = sc.case("noise", shape)
        a4 = sc.slab_args(shape[1], shape[2], rows, keep=4)
        # the dm rows that are kept are right: it is the gradient of the own rows that misses a tap
        if _slab_shares(c, a4, _slab32(c, a4), shape[1])["grad"] > 1.0:
            caught.setdefault("dm4", []).append((label, "grad"))
    print()
    for fault in sc.FAULTS + ("dm4",):
        hits = caught.get(fault, [])
        print("ssim planted fault %-10s caught by %2d: %s" % (fault, len(hits), ", ".join("%s (%s)" % h for h in hits[:6])
                                                              + (" ..." if len(hits) > 6 else "")))
    assert set(caught) == set(sc.FAULTS + ("dm4",)), sorted(set(sc.FAULTS + ("dm4",)) - set(caught))
    # each fault where it belongs: the slot only once a slot is used twice, the seam only where there is a second tile across
    slot = {h[0] for h in caught["slot"]}
    assert slot == {"noise-1x128x128", "noise-4x65x81"}
    assert all(int(h[0].split("x")[-1]) > sc.TILE for h in caught["seam"])
    # a rank at both image edges keeps every dm row whatever `keep` is: all others are caught
    assert len(caught["dm4"]) == sum(1 for s in sc.slab_list() if s[3] is not None)


def test_fma32_rounds_once():
    rng = np.random.default_rng(0)
    a, b, c = (rng.standard_normal(4096).astype(np.float32) for _ in range(3))
    exact = a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)       # itself rounded, but 29 bits finer
    got = sc.fma32(a, b, c)
    assert (np.abs(got.astype(np.float64) - exact) <= np.spacing(np.abs(got)).astype(np.float64) / 2 * (1 + 1e-6)).all()
    assert (got != (a * b + c).astype(np.float32)).any()                             # ... which two roundings do not give
    one, h = np.float32(1), np.float32(2.0 ** -12)
    assert sc.fma32(h, h, one) == one                                                # the exact tie goes to even
    # 1 + 2^-23 + (2^-24 - 2^-70): the double rounds to the midpoint, whose even neighbour is the wrong side
    up = np.nextafter(one, np.float32(2))
    assert sc.fma32(np.float32(2.0 ** -12 + 2.0 ** -35), np.float32(2.0 ** -12 - 2.0 ** -35), up) == up


# ---------------------------------------------------------------------------------------------- the C entries, no device
def test_invalid_calls_are_refused_before_anything_is_launched():
    lib = N.lib()
    win = importlib.import_module(sc.pkg + ".ops").ssim_window()

    def fwd(C=3, H=8, W=8, stride=64, win=win, img1=FAKE, img2=FAKE, dm=FAKE, total=FAKE):
        return lib.mom_ssim_forward_slab(C, H, W, stride, 0, H, 0, H, win, img1, img2, dm, total, None)

    def bwd(C=3, H=8, W=8, stride=64, win=win, img1=FAKE, img2=FAKE, dm=FAKE, dimg=FAKE):
        return lib.mom_ssim_backward_slab(C, H, W, stride, win, img1, img2, dm, 1.0, None, dimg, None)

    for bad in (dict(stride=63), dict(stride=0), dict(C=-1), dict(H=-1), dict(W=-1), dict(win=None)):
        assert fwd(**bad) == N.MOM_EINVAL, bad
        assert bwd(**bad) == N.MOM_EINVAL, bad
    assert fwd(total=None) == N.MOM_EINVAL
    assert fwd(H=0, stride=0, total=None) == N.MOM_EINVAL            # the sum is cleared even by a call without pixels
    for bad in (dict(img1=None), dict(img2=None), dict(dm=None), dict(dimg=None)):
        assert bwd(**bad) == N.MOM_EINVAL, bad
    # the whole-image entries pass H W as the stride: the same refusals
    assert lib.mom_ssim_forward(-1, 8, 8, win, FAKE, FAKE, FAKE, FAKE, None) == N.MOM_EINVAL
    assert lib.mom_ssim_forward(3, 8, 8, None, FAKE, FAKE, FAKE, FAKE, None) == N.MOM_EINVAL
    assert lib.mom_ssim_forward(3, 8, 8, win, FAKE, FAKE, FAKE, None, None) == N.MOM_EINVAL
    assert lib.mom_ssim_backward(3, 8, -8, win, FAKE, FAKE, FAKE, 1.0, None, FAKE, None) == N.MOM_EINVAL
    assert lib.mom_ssim_backward(3, 8, 8, None, FAKE, FAKE, FAKE, 1.0, None, FAKE, None) == N.MOM_EINVAL
    # a backward without pixels has nothing to do and needs no pointer
    for zero in (dict(C=0), dict(H=0, stride=0), dict(W=0, stride=0)):
        assert bwd(img1=None, img2=None, dm=None, dimg=None, **zero) == N.MOM_OK, zero
    assert N.SSIM_SUM_SLOTS == sc.SLOTS
