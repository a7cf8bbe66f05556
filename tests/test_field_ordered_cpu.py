"""The ordered field backward without a GPU (include/mom4d.h, "ordered HexPlane backward", "ordered MLP weight gradients"): its entry
points in the C ABI, what they refuse before anything is launched, the host twin of the HexPlane reduction against the documented
order restated in numpy, and the Python switch."""
import ctypes as C
import importlib
import types

import numpy as np
import pytest
import torch

import field_ordered_cases as fc
import hexplane_order_cases as hoc

pkg = fc.pkg
N = fc.N
RC = importlib.import_module(pkg + ".diff_gaussian_rasterization._C")
ops = importlib.import_module(pkg + ".ops")
FAKE = 0x10000        # a pointer that is never dereferenced: every call below is refused first

NAMES = ("mom_hexplane_ordered_scratch_bytes", "mom_hexplane_backward_ordered", "mom_hexplane_ordered_sum_host",
         "mom_deform_backward_ordered_n", "mom_deform_backward_ordered_scratch_bytes")


def _desc(channels=32, levels=2, res=(8, 6, 10, 5), fill=FAKE):
    lv = [[res[0] * (l + 1), res[1] * (l + 1), res[2] * (l + 1), res[3]] for l in range(levels)]
    d = fc.host_desc(channels, hoc.BOX, lv[:4])
    d.levels = levels                                   # (also the refused counts 0 and 5: the arrays hold four)
    for l in range(min(levels, 4)):
        for p in range(6):
            d.planes[l][p] = d.grads[l][p] = fill
    return d


def test_the_entry_points_are_additive():
    lib = N.lib()
    assert all(n in N.EXPORTS for n in NAMES)
    assert N.ABI_VERSION == 8 == lib.mom_abi_version()


def test_scratch_sizes_are_positive_monotone_and_zero_for_what_is_refused():
    lib = N.lib()
    for ch in (16, 32):
        d = _desc(ch)
        sizes = [lib.mom_hexplane_ordered_scratch_bytes(C.byref(d), P) for P in (0, 1, 63, 64, 65, 300, 5000, 200_000)]
        assert sizes[0] > 0 and all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[-1] > sizes[0]
        # the gv rows and the level shares the header places at its head fit
        assert sizes[-1] >= fc.align_up(2 * 6 * 200_000 * ch * 4) + 2 * 200_000 * 12
    for bad in (_desc(8), _desc(64), _desc(levels=0), _desc(levels=5), _desc(res=(0, 6, 10, 5)), _desc(res=(8, 6, 10, 70000)),
                _desc(16, res=(65536, 65536, 4, 4))):
        assert lib.mom_hexplane_ordered_scratch_bytes(C.byref(bad), 10) == 0
    assert lib.mom_hexplane_ordered_scratch_bytes(None, 10) == 0
    assert lib.mom_hexplane_ordered_scratch_bytes(C.byref(_desc()), -1) == 0
    assert lib.mom_hexplane_ordered_scratch_bytes(C.byref(_desc()), 2 ** 30 + 1) == 0 < lib.mom_hexplane_ordered_scratch_bytes(C.byref(_desc()), 2 ** 30)
    m = [lib.mom_deform_backward_ordered_scratch_bytes(P) for P in (0, 1, 31, 33, 300, 8233, 200_000)]
    assert m[0] > 0 and all(a <= b for a, b in zip(m, m[1:])) and m[-1] > m[0]
    assert m[-1] >= 4 * (4 * 200_000 * 64 + fc.MLP_PARTS * fc.MLP_THIN + 4 * fc.MLP_PARTS * fc.MLP_LAYER)
    assert lib.mom_deform_backward_ordered_scratch_bytes(-1) == 0


def test_every_invalid_hexplane_call_is_refused_before_anything_is_launched():
    lib = N.lib()
    good = _desc()
    need = lib.mom_hexplane_ordered_scratch_bytes(C.byref(good), 10)

    def call(d=good, P=10, xyz=FAKE, dfeat=FAKE, dxyz=FAKE, scratch=FAKE, nbytes=need, order=None):
        return lib.mom_hexplane_backward_ordered(None if d is None else C.byref(d), P, xyz, 0.3, order, dfeat, dxyz, scratch, nbytes, None)

    no_plane, no_grad = _desc(), _desc()
    no_plane.planes[1][4] = None
    no_grad.grads[0][2] = None
    for bad in (dict(d=None), dict(d=_desc(8)), dict(d=_desc(64)), dict(d=_desc(levels=0)), dict(d=_desc(levels=5)), dict(P=-1),
                dict(P=2 ** 30 + 1, nbytes=2 ** 62),                                             # the point index would leave an int
                dict(d=_desc(res=(0, 6, 10, 5))), dict(d=_desc(res=(8, 6, 10, 65537))),          # a resolution the key does not pack
                dict(d=_desc(16, res=(65536, 65536, 4, 4))), dict(d=_desc(32, res=(4096, 4096, 4, 4))),   # W H 4 C >= 2^31
                dict(xyz=None), dict(dfeat=None), dict(scratch=None), dict(nbytes=0), dict(nbytes=need - 1),
                dict(d=no_plane), dict(d=no_grad)):
        assert call(**bad) == N.MOM_EINVAL, bad
    # the descriptor's refusals come before the "nothing to do" of P == 0, the pointers' after it
    assert call(d=_desc(8), P=0) == N.MOM_EINVAL
    assert call(P=0, xyz=None, dfeat=None, scratch=None, nbytes=0) == N.MOM_OK
    # the host twin
    g = np.zeros(4, np.float32)
    assert lib.mom_hexplane_ordered_sum_host(None, 1, g.ctypes.data, 0.3, g.ctypes.data, g.ctypes.data, g.ctypes.data) == N.MOM_EINVAL
    assert lib.mom_hexplane_ordered_sum_host(C.byref(_desc(8)), 1, g.ctypes.data, 0.3, g.ctypes.data, g.ctypes.data, g.ctypes.data) == N.MOM_EINVAL
    assert lib.mom_hexplane_ordered_sum_host(C.byref(good), -1, g.ctypes.data, 0.3, g.ctypes.data, g.ctypes.data, g.ctypes.data) == N.MOM_EINVAL
    assert lib.mom_hexplane_ordered_sum_host(C.byref(good), 1, None, 0.3, g.ctypes.data, g.ctypes.data, g.ctypes.data) == N.MOM_EINVAL
    assert lib.mom_hexplane_ordered_sum_host(C.byref(good), 1, g.ctypes.data, 0.3, None, g.ctypes.data, g.ctypes.data) == N.MOM_EINVAL
    assert lib.mom_hexplane_ordered_sum_host(C.byref(good), 1, g.ctypes.data, 0.3, g.ctypes.data, None, g.ctypes.data) == N.MOM_EINVAL
    assert lib.mom_hexplane_ordered_sum_host(C.byref(_desc(fill=None)), 1, g.ctypes.data, 0.3, g.ctypes.data, g.ctypes.data, None) == N.MOM_EINVAL
    assert lib.mom_hexplane_ordered_sum_host(C.byref(good), 0, None, 0.3, None, None, None) == N.MOM_OK


def _mlp(grads=True):
    d = N.MomDeformMLP()
    d.W0 = d.b0 = FAKE
    for k in range(3):
        d.W1[k] = d.b1[k] = d.W2[k] = d.b2[k] = FAKE
    if grads:
        d.dW0 = d.db0 = FAKE
        for k in range(3):
            d.dW1[k] = d.db1[k] = d.dW2[k] = d.db2[k] = FAKE
    return d


def test_every_invalid_mlp_call_is_refused_before_anything_is_launched():
    lib = N.lib()
    need = lib.mom_deform_backward_ordered_scratch_bytes(33)

    def call(d=None, P=33, n_in=32, feat=FAKE, a0=FAKE, dpts=FAKE, dsc=FAKE, dro=FAKE, dfeat=FAKE, scratch=FAKE, nbytes=need):
        return lib.mom_deform_backward_ordered_n(C.byref(d or _mlp()), P, n_in, feat, a0, dpts, dsc, dro, dfeat, scratch, nbytes, None)

    half = _mlp()
    half.dW1[1] = None
    no_w = _mlp()
    no_w.W2[2] = None
    for n_in in (32, 64):
        for bad in (dict(P=-1), dict(feat=None), dict(a0=None), dict(dpts=None), dict(dsc=None), dict(dro=None), dict(dfeat=None),
                    dict(scratch=None), dict(nbytes=0), dict(nbytes=need - 1), dict(d=_mlp(grads=False)), dict(d=half), dict(d=no_w)):
            assert call(n_in=n_in, **bad) == N.MOM_EINVAL, (n_in, bad)
        assert call(n_in=n_in, P=0, feat=None, scratch=None, nbytes=0) == N.MOM_OK
    for n_in in (0, 16, 48, 128):
        assert call(n_in=n_in) == N.MOM_EINVAL
    assert lib.mom_deform_backward_ordered_n(None, 33, 32, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, need, None) == N.MOM_EINVAL


@pytest.mark.parametrize("channels", [16, 32])
def test_the_host_twin_adds_in_the_documented_order(channels):
    shape = fc.SYN_SHAPE
    pts = fc.synthetic_cloud()
    P = len(pts)
    res = fc.level_res(shape)
    time = shape[2]
    L = len(res)
    # the cloud holds what it is for: in the finest (x, y) plane cells of exactly 64, 65 and 129 points, and border positions
    cells = hoc.cells(torch.from_numpy(pts), shape)
    finest = cells[0, L - 1]
    counts = np.bincount(finest.cell)
    assert {64, 65, 129, 3} <= set(counts.tolist())
    assert (~finest.interior).sum() >= 3
    # (this module's cells are hexplane_order_cases' cells)
    for (si, l), c in cells.items():
        key, _, Wd, Hd = fc.plane_samples(pts, time, hoc.BOX, res[l], {0: 0, 1: 1, 2: 3}[si])
        assert (Wd, Hd) == (c.W, c.H) and np.array_equal(key, c.cell)
    rng = np.random.default_rng(channels)
    gv = rng.standard_normal((L, 6, P, channels)).astype(np.float32)
    part = rng.standard_normal((L, P, 3)).astype(np.float32)
    dxyz_in = rng.standard_normal((P, 3)).astype(np.float32)
    grads_in = [[rng.standard_normal((r[cb], r[ca], channels)).astype(np.float32) for ca, cb in fc.PLANES] for r in res]
    got, got_dxyz = fc.host_twin(channels, hoc.BOX, res, pts, time, gv, grads_in, part, dxyz_in)
    want, want_dxyz, stats = fc.hexplane_numpy(pts, time, hoc.BOX, res, gv, grads_in, part, dxyz_in)
    for l in range(L):
        for p in range(6):
            np.testing.assert_array_equal(fc.bits(got[l][p]), fc.bits(want[l][p]), err_msg=f"level {l} plane {p}")
            # a texel without a term keeps its bits (the incoming gradient is not zero anywhere)
            untouched = fc.bits(want[l][p]) == fc.bits(grads_in[l][p])
            assert untouched.all(axis=2).sum() >= want[l][p].shape[0] * want[l][p].shape[1] - stats[l][p]["written"]
    np.testing.assert_array_equal(fc.bits(got_dxyz), fc.bits(want_dxyz))
    st = stats[L - 1][0]
    assert {64, 65, 129} <= st["lengths"] and st["empty_class"] > 0 and st["border"] > 0
    # the three levels meet as (p0 + p1) + p2, which is not p0 + (p1 + p2) everywhere
    other = (dxyz_in + (part[0] + (part[1] + part[2]))).astype(np.float32)
    assert (fc.bits(other) != fc.bits(want_dxyz)).any()
    # ... and the blocks are part of the order: one left-to-right sum over a 129-point cell differs somewhere
    key, w, Wd, Hd = fc.plane_samples(pts, time, hoc.BOX, res[L - 1], 0)
    cell = int(np.flatnonzero(np.bincount(key) == 129)[0])
    gs = np.flatnonzero(key == cell)
    e = (gv[L - 1, 0][gs] * w[gs, 0][:, None]).astype(np.float32)
    assert (fc.bits(fc.seq_sum(e)) != fc.bits(fc.class_sum(e))).any()


def test_the_switch_routes_the_field_and_allocates_nothing_while_off():
    assert RC.deterministic() is False and RC._state["field_ordered"] is None
    ctx = types.SimpleNamespace(times=torch.zeros(3))            # a forward with per-point timestamps
    steps = importlib.import_module(pkg + ".fused_step")
    try:
        RC.set_deterministic(True)
        with pytest.raises(N.MomError, match="set_deterministic"):
            ops.HexPlaneFunction.backward(ctx, None)               # refused before anything is read, allocated or launched
        for cls in (steps.FusedStep, steps.FusedStep16, steps.FusedCoarseStep):
            with pytest.raises(N.MomError, match="set_deterministic"):
                steps._Step.__init__(object.__new__(cls), None, None, None, None)     # every step's first statement, and again in _ensure
        assert ops.mlp_backward_is_ordered(32) is True
    finally:
        RC.set_deterministic(False)
    assert RC._state["field_ordered"] is None and RC._state["ordered"] is None
