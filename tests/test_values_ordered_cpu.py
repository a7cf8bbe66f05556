"""The ordered loss values without a GPU (include/mom4d.h, "ordered loss values"): their entry points in the C ABI, what they refuse
before anything is launched, the host twins against the documented order restated in numpy (values_ordered_cases.py), and the trainer
state a run is continued from (train.Trainer.state_dict / load_state_dict).

Every case first shows that it can tell orders apart: the same terms added one by one from the last to the first give other bits.
The one listed size that cannot is n = 1 (one term has one order); it stays as the boundary it is and is said so below.  The SSIM
sum is a fold of float workgroup totals in double: totals of real images (at most 256 each) add exactly in double in any order, so
the cases fold synthetic totals of mixed magnitude at the listed shapes (a flat image has fixture g3's shape: the same list); the
images themselves, the flat pair included, run on the GPU."""
import importlib
import inspect
import random
import types

import numpy as np
import pytest
import torch

import values_ordered_cases as vc

N = vc.N
FAKE = 0x10000        # an aligned pointer that is never dereferenced: every call below is refused first

PROTOS = {
    "mom_l1_loss_ordered_scratch_bytes": ("size_t", ["size_t"]),
    "mom_l1_loss_ordered": ("int", ["size_t", "ptr", "ptr", "ptr", "ptr", "ptr", "size_t", "ptr"]),
    "mom_l1_loss_ordered_host": ("int", ["size_t", "ptr", "ptr", "ptr", "ptr"]),
    "mom_ssim_ordered_scratch_bytes": ("size_t", ["int", "int", "int"]),
    "mom_ssim_forward_ordered": ("int", ["int", "int", "int", "ptr", "ptr", "ptr", "ptr", "ptr", "ptr", "size_t", "ptr"]),
    "mom_ssim_sum_ordered": ("int", ["size_t", "ptr", "ptr", "ptr"]),
    "mom_ssim_sum_ordered_host": ("int", ["size_t", "ptr", "ptr"]),
    "mom_plane_regulation_ordered_scratch_bytes": ("size_t", ["planes", "int"]),
    "mom_plane_regulation_ordered": ("int", ["planes", "int", "ptr", "ptr", "size_t", "ptr"]),
    "mom_plane_regulation_ordered_host": ("int", ["planes", "int", "ptr"]),
}


def test_the_entry_points_are_exported_with_the_declared_argument_lists():
    import ctypes as C
    lib = N.lib()
    kinds = {"int": C.c_int, "size_t": C.c_size_t, "ptr": C.c_void_p, "planes": C.POINTER(N.MomRegPlane)}
    protos = N.parse_prototypes(open(N.HEADER_PATH).read(), N._STRUCTS)
    for name, (ret, args) in PROTOS.items():
        assert name in N.EXPORTS and hasattr(lib, name), name
        assert protos[name] == (kinds[ret], [kinds[a] for a in args]), name
        f = getattr(lib, name)
        assert f.restype is kinds[ret] and list(f.argtypes) == [kinds[a] for a in args], name
    assert N.ABI_VERSION == 8 == lib.mom_abi_version()                      # additive: no struct and no existing entry changed


def test_scratch_sizes_follow_the_documented_layouts():
    lib = N.lib()
    l1 = lib.mom_l1_loss_ordered_scratch_bytes
    assert [l1(n) for n in (0, 1, 4096, 4097, 8192, 8193)] == [0, 8, 8, 16, 16, 24]        # [2][ceil(n / 4096)] floats
    assert l1(2 ** 40) == 8 * 2 ** 28 and l1(2 ** 40 + 1) == 0
    ss = lib.mom_ssim_ordered_scratch_bytes
    assert [ss(*s) for s in vc.SSIM_SHAPES] == [4 * 36, 4 * 3, 4 * 270]
    assert ss(3, 540, 960) == 4 * 6120
    assert ss(0, 4, 4) == ss(3, 0, 4) == ss(3, 4, 0) == ss(-1, 4, 4) == 0
    rg = lib.mom_plane_regulation_ordered_scratch_bytes
    for name, blocks in (("field32", 6 + 3 * 2 + 3 * 2), ("field16", 12), ("wide", 63), ("field32+wide", 18 + 63)):
        planes = vc.reg_case(name)
        assert rg(vc.reg_desc(planes), len(planes)) == 4 * blocks == 4 * vc.reg_numpy(planes)[1], name
    assert rg(None, 0) == 0 and rg(None, 1) == 0 and rg(vc.reg_desc(vc.wide_plane()), N.REG_MAX_PLANES + 1) == 0


def test_every_invalid_call_is_refused_before_anything_is_launched():
    lib = N.lib()

    def l1(n=5000, img=FAKE, gt=FAKE, dimg=FAKE, sums=FAKE, scratch=FAKE, nbytes=16):
        return lib.mom_l1_loss_ordered(n, img, gt, dimg, sums, scratch, nbytes, None)

    for bad in (dict(img=None), dict(gt=None), dict(sums=None), dict(scratch=None), dict(scratch=FAKE + 2), dict(nbytes=15), dict(nbytes=0),
                dict(n=2 ** 40 + 1, nbytes=2 ** 62)):
        assert l1(**bad) == N.MOM_EINVAL, bad
    win = (vc.C.c_float * 11)(*([1 / 11] * 11))

    def ssim(Cn=3, H=37, W=53, w=win, a=FAKE, b=FAKE, total=FAKE, scratch=FAKE, nbytes=144):
        return lib.mom_ssim_forward_ordered(Cn, H, W, w, a, b, None, total, scratch, nbytes, None)

    for bad in (dict(Cn=-1), dict(H=-1), dict(W=-1), dict(w=None), dict(a=None), dict(b=None), dict(total=None), dict(scratch=None),
                dict(scratch=FAKE + 1), dict(nbytes=143), dict(Cn=65536, nbytes=2 ** 40), dict(H=16 * 65536, W=1, nbytes=2 ** 40)):
        assert ssim(**bad) == N.MOM_EINVAL, bad
    assert lib.mom_ssim_sum_ordered(4, None, FAKE, None) == lib.mom_ssim_sum_ordered(4, FAKE, None, None) == N.MOM_EINVAL
    planes = vc.wide_plane()

    def reg(arr=vc.reg_desc(planes, [FAKE]), count=1, value=FAKE, scratch=FAKE, nbytes=4 * 63):
        return lib.mom_plane_regulation_ordered(arr, count, value, scratch, nbytes, None)

    def one(**kw):
        arr = vc.reg_desc(planes, [FAKE])
        for k, v in kw.items():
            setattr(arr[0], k, v)
        return arr

    for bad in (dict(arr=None), dict(count=-1), dict(count=N.REG_MAX_PLANES + 1), dict(value=None), dict(scratch=None),
                dict(scratch=FAKE + 2), dict(nbytes=4 * 63 - 1), dict(arr=one(plane=None)), dict(arr=one(H=0)), dict(arr=one(W=0)),
                dict(arr=one(W=2 ** 24 + 1), nbytes=2 ** 40), dict(arr=one(H=2 ** 24, W=2 ** 24), nbytes=2 ** 40)):
        assert reg(**bad) == N.MOM_EINVAL, bad
    # the host twins refuse the same
    g = np.zeros(16, np.float32).ctypes.data
    assert lib.mom_l1_loss_ordered_host(4, None, g, g, g) == lib.mom_l1_loss_ordered_host(4, g, None, g, g) == N.MOM_EINVAL
    assert lib.mom_l1_loss_ordered_host(4, g, g, g, None) == lib.mom_l1_loss_ordered_host(2 ** 40 + 1, g, g, g, g) == N.MOM_EINVAL
    assert lib.mom_ssim_sum_ordered_host(4, None, g) == lib.mom_ssim_sum_ordered_host(4, g, None) == N.MOM_EINVAL
    assert lib.mom_plane_regulation_ordered_host(one(plane=None), 1, g) == lib.mom_plane_regulation_ordered_host(one(H=0), 1, g) == N.MOM_EINVAL
    assert lib.mom_plane_regulation_ordered_host(vc.reg_desc(planes), 1, None) == N.MOM_EINVAL


@pytest.mark.parametrize("n", vc.L1_SIZES)
def test_the_l1_host_twin_adds_in_the_documented_order(n):
    img, gt = vc.l1_inputs(n)
    a, q, d = vc.l1_terms(img, gt)
    want, want_dimg = vc.l1_numpy(img, gt)
    # the case can tell orders apart (one term has one order: n = 1 is a boundary of the mapping, not of the order)
    other = np.array([vc.reversed_sum(a), vc.reversed_sum(q)], np.float32)
    assert (vc.bits(other) != vc.bits(want)).all() if n > 1 else (vc.bits(other) == vc.bits(want)).all()
    got, dimg = vc.l1_host(img, gt)
    np.testing.assert_array_equal(vc.bits(got), vc.bits(want))
    np.testing.assert_array_equal(vc.bits(dimg), vc.bits(want_dimg))
    assert abs(float(got[0]) - float(a.astype(np.float64).sum())) <= 1e-5 * float(a.astype(np.float64).sum())     # ... and it is the sum
    if n > 70:
        assert dimg[5] == 0 and dimg[66] == -np.float32(1) / np.float32(n)


def test_the_l1_host_twin_takes_no_gradient_pointer_and_no_element():
    img, gt = vc.l1_inputs(65)
    sums = np.full(2, np.nan, np.float32)
    assert N.lib().mom_l1_loss_ordered_host(65, vc.ptr(img), vc.ptr(gt), None, vc.ptr(sums)) == N.MOM_OK
    np.testing.assert_array_equal(vc.bits(sums), vc.bits(vc.l1_numpy(img, gt)[0]))
    assert N.lib().mom_l1_loss_ordered_host(0, vc.ptr(img), vc.ptr(gt), None, vc.ptr(sums)) == N.MOM_OK
    assert (vc.bits(sums) == 0).all()                                        # +0.0 twice


@pytest.mark.parametrize("shape", vc.SSIM_SHAPES)
def test_the_ssim_sum_host_twin_folds_in_double_in_the_documented_order(shape):
    totals = vc.ssim_totals(shape)
    want = vc.fold(totals, np.float64)
    assert vc.bits(np.float64(vc.reversed_sum(totals, np.float64))) != vc.bits(np.float64(want))
    assert vc.bits(np.float64(vc.fold(totals, np.float32))) != vc.bits(np.float64(want))          # ... and a float fold is not it
    got = vc.ssim_sum_host(totals)
    assert vc.bits(np.float64(got)) == vc.bits(np.float64(want))
    out = np.full(1, np.nan)
    assert N.lib().mom_ssim_sum_ordered_host(0, None, vc.ptr(out)) == N.MOM_OK and vc.bits(out)[0] == 0


@pytest.mark.parametrize("name", vc.REG_CASES)
def test_the_regulariser_host_twin_adds_in_the_documented_order(name):
    planes = vc.reg_case(name)
    want, blocks = vc.reg_numpy(planes)
    terms = []
    for p, w_smooth, w_l1 in planes:
        smooth, l1 = vc.reg_plane_terms(p, w_smooth, w_l1)
        terms += [smooth.ravel()] + ([l1.ravel()] if l1 is not None else [])
    terms = np.concatenate(terms)
    assert vc.bits(np.float32(vc.reversed_sum(terms))) != vc.bits(np.float32(want))
    got = vc.reg_host(planes)
    assert vc.bits(np.float32(got)) == vc.bits(np.float32(want))
    ref = float(terms.astype(np.float64).sum())
    assert abs(float(got) - ref) <= 1e-4 * abs(ref)
    if name == "field32+wide":
        assert blocks > vc.BLOCK                                             # the partials fill more than one block


def test_the_python_layers_route_on_the_switch():
    ops, RC, T = (importlib.import_module(f"{vc.pkg}.{m}") for m in ("ops", "diff_gaussian_rasterization._C", "train"))
    for fn, entry in ((ops.L1LossFunction.forward, "mom_l1_loss_ordered"), (ops.SSIMFunction.forward, "mom_ssim_forward_ordered"),
                      (ops.PlaneRegFunction.forward, "mom_plane_regulation_ordered")):
        src = inspect.getsource(fn)
        assert entry in src and "_RC.deterministic()" in src
    assert "value_ordered" in RC._state and RC._state["value_ordered"] is None and RC.deterministic() is False
    assert "loss" in RC.set_deterministic.__doc__
    p = inspect.signature(T.Trainer.save).parameters
    assert list(p) == ["self", "iteration", "stage", "trainer_state"] and p["trainer_state"].default is False


def _bare_trainer(T, n_cams=7, batch=2):
    """A Trainer with the fields its state covers and nothing else: no scene, no model, no GPU."""
    from collections import deque
    t = object.__new__(T.Trainer)
    t.cams = [types.SimpleNamespace(uid=i) for i in range(n_cams)]
    t.stack = list(t.cams)
    t.opt = types.SimpleNamespace(batch_size=batch)
    t.g = types.SimpleNamespace(_xyz=torch.zeros(1))
    t.stage, t.fused, t.ema_loss, t.ema_psnr = "fine", None, 0.0, 0.0
    t._log, t._checks, t._alog = deque(), deque(), deque()
    return t


def test_a_state_round_trip_reproduces_the_camera_draws_and_the_split_samples():
    T = importlib.import_module(vc.pkg + ".train")
    random.seed(11)
    torch.manual_seed(11)
    a = _bare_trainer(T)
    for _ in range(5):
        a._draw()                                            # mid-epoch: the stack is partly used
    a.ema_loss, a.ema_psnr = 0.125, 31.5
    state = a.state_dict(40)
    assert state["iteration"] == 40 and len(state["stack"]) == len(a.stack) < len(a.cams)
    stds = torch.full((6, 3), 0.5)
    want_cams = [[c.uid for c in a._draw()] for _ in range(20)]
    want_normal = torch.normal(mean=torch.zeros(6, 3), std=stds)
    random.seed(99)                                          # whatever happened in between
    torch.manual_seed(99)
    b = _bare_trainer(T)
    assert b.load_state_dict(state) == 40
    assert (b.ema_loss, b.ema_psnr) == (0.125, 31.5)
    assert [[c.uid for c in b._draw()] for _ in range(20)] == want_cams
    assert torch.equal(torch.normal(mean=torch.zeros(6, 3), std=stds), want_normal)
    # a state of another run is refused, not continued
    for key, value in (("stage", "coarse"), ("n_cams", 8), ("version", 0), ("deterministic", True), ("fused", True), ("stack", [0, 7])):
        with pytest.raises(N.MomError):
            _bare_trainer(T).load_state_dict(dict(state, **{key: value}))
