"""The two-pass HexPlane backward (32 and 16 channels) under orders it was not sorted for, and on walks of more than one chunk.

HexPlaneField rebuilds its Morton order and its six plane orders every REORDER_EVERY calls only (and may sort them while Adam
writes the positions): 63 of 64 training steps walk an order that was sorted for other positions.  The contract is "an order is
a permutation whatever the keys were, and only speed depends on it".  The scatter kernels (hexplane_bwd5_scatter_kernel<32, false / true>
and hexplane_bwd5_scatter_kernel<16, false> in csrc/hexplane.hip) recompute every cell from the current positions and keep
four texel rows and two line rows pending along the walk; a fresh sorted order shows them long runs of one cell and neighbouring
cells next, any other order shows them a cell change at every position, the same parity slot evicted again and again, border
positions between two positions of one interior cell, a ride row that stays while the cell changes.  And above 131 072 points every
half-wave (32 channels) or group (16) walks more than one chunk: the carry of the previous cell and row, the pending rows (and, in
the one-row form, their values) and the per-chunk records in LDS then live across chunk boundaries; above 196 608 points the gathers
take a second trip through their chunk loop.  tests/hexplane_order_cases.py builds the orders and counts those events;
tests/test_hexplane_orders_cpu.py pins that the orders used here do contain them, and the walk lengths.

References and tolerances are the suite's: oracle.torch_ref.hexplane_features in fp32 on the CPU for the features and d xyz, and
for the plane gradients at P <= 300; the same function in float64 for the plane gradients of the large clouds (sums of thousands
of terms per texel: the CPU file bounds the fp32 oracle's own summation noise there by half the tolerance).  Features rtol 2e-5 /
atol 5e-6, gradients rtol 2e-4 / atol 2e-5 x the tensor's scale, per element, nothing left out.

Every order is validated on the CPU as a permutation with its matching inverse before it is uploaded (hexplane_order_cases.orders):
the kernels index with it."""
import ctypes as C
import functools
import importlib

import numpy as np
import pytest
import torch

import hexplane_box_cases as hb
import hexplane_order_cases as oc

pytestmark = pytest.mark.gpu

pkg = "iclr2025_3d-mom_amd"
ops = importlib.import_module(pkg + ".ops")
N = importlib.import_module(pkg + "._native")

# (channels, form): the lane-per-channel gather with the six-row scatter; the default (gather6 and the one-row scatter, CROWS);
# mom_hexplane_backward_lines on the lines the fused field forward left in the field scratch; 16 channels
FORMS = [(32, "gather5"), (32, "gather6"), (32, "lines"), (16, "two_pass")]


# ---------------------------------------------------------------------------------------- running the kernels
def _lib_orders(fg):
    """positions -> (morton, order, inverse) from the library's sorts, as int32 numpy."""
    levels = [list(g) for g in fg.grids]

    def run(pts):
        x = pts.cuda()
        m = ops.morton_order(x)
        o, i = ops.hexplane_orders(x, levels, fg.aabb, aabb_host=fg.aabb_host())
        torch.cuda.synchronize()
        return m.cpu().numpy(), o.cpu().numpy(), i.cpu().numpy()
    return run


def _orders(family, fg, pts, shape, box=oc.BOX):
    """One family's orders on the GPU; oc.orders has validated them on the CPU."""
    return tuple(torch.from_numpy(a).cuda() for a in oc.orders(family, pts, shape, _lib_orders(fg), box))


def _identity(n):
    return torch.arange(n, dtype=torch.int32, device="cuda")


def _supported(fg):
    hp, keep = ops._hexplane_desc([[p.detach() for p in lv] for lv in fg.grids], fg.aabb, None, aabb_host=fg.aabb_host())
    return N.lib().mom_deform_field_supported(C.byref(hp))


def _per_op(fg, pts, t, w, morton, plane_orders):
    """features, d xyz, [[d plane]] through ops.hexplane_features with caller-supplied orders."""
    levels = [list(g) for g in fg.grids]
    fg.zero_grad()
    p = pts.cuda().requires_grad_(True)
    feat = ops.hexplane_features(p, t, fg.aabb, levels, order=morton, aabb_host=fg.aabb_host(), plane_orders=plane_orders)
    if w is None:
        return feat.detach(), None, None
    (feat * w.cuda()).sum().backward()
    torch.cuda.synchronize()
    return feat.detach(), p.grad, [[q.grad for q in g] for g in fg.grids]


def _fused_lines(fg, pts, t, w, morton, plane_orders):
    """The fused field forward (csrc/deform_field.hip) under the order `morton`, then mom_hexplane_backward_lines on the time lines
    it left in the field scratch: what the fused training step runs."""
    from test_deform_field_gpu import _mlp, _run_forward
    n = pts.shape[0]
    params_cpu, mk = _mlp(7)
    params = [p.cuda() for p in params_cpu]
    xyz = pts.cuda()
    scal, rot, flow, opac = (mk(n, k).cuda() for k in (3, 4, 3, 1))
    feat = _run_forward(fg, params, n, xyz, scal, rot, flow, opac, t, morton, fused=True)["feat"]
    if w is None:
        return feat, None, None
    lib, s = N.lib(), N.current_stream()
    levels = [[p.detach() for p in lv] for lv in fg.grids]
    grads = [[torch.zeros_like(p) for p in lv] for lv in levels]
    hp, keep = ops._hexplane_desc(levels, fg.aabb, grads, aabb_host=fg.aabb_host())
    dfeat = w.cuda().contiguous()
    dxyz = torch.zeros(n, 3, device="cuda")
    scratch = torch.empty(lib.mom_hexplane_backward_scratch_bytes(C.byref(hp), n), dtype=torch.uint8, device="cuda")
    N.check(lib.mom_hexplane_backward_lines(C.byref(hp), n, xyz.data_ptr(), t, morton.data_ptr(), dfeat.data_ptr(), dxyz.data_ptr(),
                                            plane_orders[0].data_ptr(), plane_orders[1].data_ptr(), scratch.data_ptr(),
                                            ops.field_scratch(hp, xyz.device).data_ptr(), s), "mom_hexplane_backward_lines")
    torch.cuda.synchronize()
    return feat, dxyz, grads


def _run(form, fg, pts, t, w, orders, monkeypatch):
    """(features, d xyz, [[d plane]]) of one form under `orders`, and the same form's features under the identity order."""
    if form == "gather5":
        monkeypatch.setenv("MOM_HEX_GATHER", "5")
    else:
        monkeypatch.delenv("MOM_HEX_GATHER", raising=False)
    if form in ("gather6", "lines"):
        assert _supported(fg) == 1          # or the six-row form would run in its place
    morton, po, pinv = orders
    run = _fused_lines if form == "lines" else _per_op
    feat_id = run(fg, pts, t, None, _identity(pts.shape[0]), None)[0].clone()
    return run(fg, pts, t, w, morton, (po, pinv)) + (feat_id,)


# ---------------------------------------------------------------------------------------- comparing
def _ratio(got, ref, rtol, atol):
    return float((np.abs(np.asarray(got, np.float64) - ref) / (atol + rtol * np.abs(ref))).max()) if ref.size else 0.0


def _check(what, out, ref, ref_planes=None, points=True, planes=True):
    """Every feature and every d xyz against `ref` (the fp32 oracle), every plane gradient against `ref_planes` (default: ref's);
    the features also bit for bit against the identity-order features.  Prints the worst error as a fraction of the tolerance."""
    feat, dxyz, grads, feat_id = out
    ref_planes = ref[2] if ref_planes is None else ref_planes
    said = []
    if points:
        f, g = feat.cpu().numpy(), dxyz.cpu().numpy()
        assert f.shape == ref[0].shape and g.shape == ref[1].shape
        assert torch.equal(feat, feat_id), (what, "the features depend on the processing order")
        said.append(f"features {_ratio(f, ref[0], hb.FEAT_RTOL, hb.FEAT_ATOL):.3f}")
        said.append(f"d xyz {_ratio(g, ref[1], hb.GRAD_RTOL, hb.grad_atol(ref[1])):.3f}")
    if planes:
        got = [[q.detach().cpu().numpy() for q in lv] for lv in grads]
        worst = max(oc.plane_error_ratio(a, b) for la, lb in zip(got, ref_planes) for a, b in zip(la, lb))
        said.append(f"plane gradients {worst:.3f}")
    print(f"{what}: worst error / tolerance: " + ", ".join(said))
    if points:
        np.testing.assert_allclose(f, ref[0], rtol=hb.FEAT_RTOL, atol=hb.FEAT_ATOL, err_msg=what + " features")
        np.testing.assert_allclose(g, ref[1], rtol=hb.GRAD_RTOL, atol=hb.grad_atol(ref[1]), err_msg=what + " dxyz")
    if planes:
        for l, (la, lb) in enumerate(zip(got, ref_planes)):
            assert len(la) == len(lb) == 6
            for i, (a, b) in enumerate(zip(la, lb)):
                assert a.shape == b.shape
                np.testing.assert_allclose(a, b, rtol=hb.GRAD_RTOL, atol=hb.grad_atol(b), err_msg=f"{what} plane {l} {i}")


# ---------------------------------------------------------------------------------------- a. any order, small cloud
@pytest.mark.parametrize("family", oc.FAMILIES)
@pytest.mark.parametrize("channels,form", FORMS)
def test_any_order_gives_the_oracles_gradients(channels, form, family, monkeypatch):
    """P = 300 on "small", box asym_a: the face, corner and one-ulp points of hb.points under every order family."""
    ref = oc.oracle32(channels, "small", hb.P)
    fg = oc.field(channels, oc.BOX, "small").cuda()
    pts = oc.cloud(hb.P)
    out = _run(form, fg, pts, oc.SHAPES["small"][2], hb.weights(fg.feat_dim), _orders(family, fg, pts, "small"), monkeypatch)
    _check(f"{channels} channels, {form}, {family}", out, ref)


@pytest.mark.parametrize("channels,form", FORMS)
def test_adversarial_order_on_the_symmetric_box(channels, form, monkeypatch):
    """The control box, on which the min-face points ARE clipped: more border positions to sandwich."""
    ref = hb.oracle(channels, "symmetric", "small")
    fg = oc.field(channels, "symmetric", "small").cuda()
    pts = hb.points("symmetric")
    orders = _orders("adversarial", fg, pts, "small", box="symmetric")
    out = _run(form, fg, pts, oc.SHAPES["small"][2], hb.weights(fg.feat_dim), orders, monkeypatch)
    _check(f"{channels} channels, {form}, adversarial, symmetric box", out, ref)


@pytest.mark.parametrize("channels", [32, 16])
def test_random_order_on_three_levels(channels, monkeypatch):
    """(16, 12, 10, 7) x (1, 2, 4): three levels, which the one-row form does not take -- the six-row scatter, three orders a plane."""
    ref = oc.oracle32(channels, "three_levels", hb.P)
    fg = oc.field(channels, oc.BOX, "three_levels").cuda()
    pts = oc.cloud(hb.P)
    assert channels == 16 or _supported(fg) == 0
    out = _run("two_pass", fg, pts, oc.SHAPES["three_levels"][2], hb.weights(fg.feat_dim), _orders("random", fg, pts, "three_levels"),
               monkeypatch)
    _check(f"{channels} channels, three levels, random", out, ref)


# ---------------------------------------------------------------------------------------- b. degenerate orders, degenerate clouds
@functools.lru_cache(maxsize=None)
def _cloud_of(name):
    return {"one_cell": oc.one_cell_cloud, "outside": oc.outside_cloud}[name]() if isinstance(name, str) else oc.cloud(name)


@functools.lru_cache(maxsize=None)
def _oracle_of(channels, name):
    return oc.oracle32(channels, "small", name) if not isinstance(name, str) else oc.freeze(oc.oracle_for(channels, "small", _cloud_of(name)))


@pytest.mark.parametrize("family", ["fresh", "random"])
@pytest.mark.parametrize("name", [1, 33, "one_cell", "outside"])
@pytest.mark.parametrize("channels,form", [(32, "gather5"), (32, "gather6"), (16, "two_pass")])
def test_degenerate_clouds(channels, form, name, family, monkeypatch):
    """One point; 33 points (one full walker and one position of the next, 32 channels; two full walkers and one position of a
    third, 16: per_half is 32 and per_group 16 here, so no walker takes a second chunk); 300 points in ONE cell
    of every plane and level (one run from end to end, whatever the order); 300 points beyond the box minimum (every position a
    border position: no run at all, corners outside the plane at every step)."""
    pts = _cloud_of(name)
    ref = _oracle_of(channels, name)
    fg = oc.field(channels, oc.BOX, "small").cuda()
    w = hb.weights(fg.feat_dim, n=pts.shape[0])
    out = _run(form, fg, pts, oc.SHAPES["small"][2], w, _orders(family, fg, pts, "small"), monkeypatch)
    assert out[0].shape == (pts.shape[0], 2 * channels)
    _check(f"{channels} channels, {form}, {name}, {family}", out, ref)


# ---------------------------------------------------------------------------------------- c. multi-chunk walks
LARGE_FORMS = [(32, "gather5"), (32, "gather6"), (16, "two_pass")]


def _large(channels, form, shape, P, family, part, monkeypatch):
    fg = oc.field(channels, oc.BOX, shape).cuda()
    pts = oc.cloud(P)
    orders = _orders(family, fg, pts, shape)
    chunks = (oc.per_half32(P) // 32) if channels == 32 else (oc.per_group16(P) // 16)
    if family == "fresh":
        # the library's own order of THIS cloud is the emulation's (the CPU file counted its events on the emulation), and above
        # 131 072 points it does carry runs of one cell across the walkers' chunk boundaries
        got = orders[1].cpu().numpy()
        for (si, l), c in oc.cells(pts, shape).items():
            assert np.array_equal(got[si, l], np.argsort(oc.plane_key(c), kind="stable")), (si, l)
            if chunks > 1:
                chunk, walk = (32, oc.per_half32(P)) if channels == 32 else (16, oc.per_group16(P))
                assert oc.events(got[si, l], c, chunk, walk).chunk_crossing_runs > 0, (si, l)
    out = _run(form, fg, pts, oc.SHAPES[shape][2], hb.weights(fg.feat_dim, n=P), orders, monkeypatch)
    what = f"{channels} channels, {form}, {shape}, P = {P} ({chunks} chunk{'s' * (chunks > 1)} a walker), {family}"
    if part == "points":
        _check(what, out, oc.oracle32(channels, shape, P), planes=False)
    else:
        _check(what, out, None, ref_planes=oc.oracle64(channels, shape, P)[2], points=False)


@pytest.mark.parametrize("part", ["points", "planes"])
@pytest.mark.parametrize("family", ["fresh", "stale", "random"])
@pytest.mark.parametrize("shape,P", oc.LARGE)
@pytest.mark.parametrize("channels,form", LARGE_FORMS)
def test_multi_chunk_walks(channels, form, shape, P, family, part, monkeypatch):
    """131 072 points: one chunk a walker (the control); 131 109: two; 270 001: three, and a second trip of the gathers' chunk
    loops.  "small" has runs of thousands of positions that cross every chunk boundary under a fresh order, "mid" short ones.
    part = points: features and d xyz against the fp32 oracle; planes: the plane gradients against the float64 evaluation (each
    part pays for one oracle at most, and the cache shares it with every other form and family)."""
    _large(channels, form, shape, P, family, part, monkeypatch)


@pytest.mark.parametrize("part", ["points", "planes"])
def test_multi_chunk_walk_of_backward_lines_under_a_stale_order(part, monkeypatch):
    _large(32, "lines", "small", 270001, "stale", part, monkeypatch)


# ---------------------------------------------------------------------------------------- d. the module's cache
@pytest.mark.parametrize("channels", [32, 16])
def test_the_module_walks_its_cached_orders_after_the_positions_moved(channels, monkeypatch):
    """HexPlaneField at positions A builds its orders; the same tensor is then overwritten in place with B (the displacement of the
    stale family) and the module runs again with no refresh due: it must use the very orders of the first call, and features,
    d xyz and plane gradients must be the oracle's for B."""
    monkeypatch.delenv("MOM_HEX_GATHER", raising=False)
    fg = oc.field(channels, oc.BOX, "small").cuda()
    assert fg.REORDER_EVERY > 2
    t = oc.SHAPES["small"][2]
    a_pts = oc.cloud(hb.P)
    b_pts = oc.displaced(a_pts, "small")
    w = hb.weights(fg.feat_dim).cuda()
    x = a_pts.cuda().requires_grad_(True)
    (fg(x, t) * w).sum().backward()
    order, porders = fg._order, fg._porders
    assert order is not None and porders is not None
    for a in (order, *porders):                             # (what the module built is what the helper calls `fresh` for A)
        assert a.dtype == torch.int32
    with torch.no_grad():
        x.copy_(b_pts.cuda())
    x.grad = None
    fg.zero_grad()
    feat = fg(x, t)
    (feat * w).sum().backward()
    torch.cuda.synchronize()
    assert fg._order is order and fg._porders is porders and fg._porders[0] is porders[0] and fg._porders[1] is porders[1]
    fresh_b = _lib_orders(fg)(b_pts)
    assert not np.array_equal(porders[0].cpu().numpy(), fresh_b[1])          # and they are stale: not what B would sort to
    ref = oc.oracle_for(channels, "small", b_pts)
    x_grad, plane_grads = x.grad.clone(), [[q.grad.clone() for q in g] for g in fg.grids]
    feat_id = _per_op(fg, b_pts, t, None, _identity(hb.P), None)[0]        # (clears the module's gradients)
    _check(f"{channels} channels, HexPlaneField with cached orders", (feat.detach(), x_grad, plane_grads, feat_id), ref)


# ---------------------------------------------------------------------------------------- e. the orders themselves
# resolutions whose keys take 1, 2 and 3 passes of the 8-bit radix sort (mom_sort_pairs_u32): plane sizes <= 16: at most 8 key bits;
# 32 and 64: 10 and 12; one axis of 300: 18 on the planes that have it (the result lands in the other pair of buffers than after
# two passes) and 6 on the third
SORT_SHAPES = {1: ((8, 8, 8, 5), (1, 2), 0.3), 2: ((32, 32, 32, 5), (1, 2), 0.3), 3: ((300, 8, 8, 5), (1,), 0.3)}


@pytest.mark.parametrize("P", [1, 255, 4096, 4097, 20011])
@pytest.mark.parametrize("passes", [1, 2, 3])
def test_plane_orders_are_the_stable_sort_of_the_emulated_key(passes, P):
    """mom_hexplane_orders against np.argsort(kind="stable") of the CPU-emulated key (the 2-D Morton interleave of the texel the
    point falls into, as plane_key_kernel forms it): the same permutation, element for element, and its inverse.  4096 is the
    sort's items per workgroup."""
    shape = SORT_SHAPES[passes]
    fg = oc.field(16, oc.BOX, shape).cuda()
    pts = oc.cloud(P)
    _, order, inv = _lib_orders(fg)(pts)
    cs = oc.cells(pts, shape)
    L = len(shape[1])
    assert order.shape == inv.shape == (3, L, P) and order.dtype == inv.dtype == np.int32
    seen = set()
    for (si, l), c in cs.items():
        seen.add((oc.key_bits(c) + 7) // 8)
        assert oc.is_permutation(order[si, l], P), (si, l)
        assert np.array_equal(inv[si, l][order[si, l]], np.arange(P, dtype=np.int32)), (si, l)
        want = np.argsort(oc.plane_key(c), kind="stable").astype(np.int32)
        differ = np.nonzero(order[si, l] != want)[0]
        assert differ.size == 0, (si, l, "first differing positions", differ[:8], order[si, l][differ[:8]], want[differ[:8]])
    assert passes in seen, seen


@pytest.mark.parametrize("name", ["planar", "identical", 4096, 4097])
def test_morton_order_stays_a_permutation(name):
    """A planar cloud (z = 0 for every point: the bounding box has zero extent on that axis), 300 identical points, and the sizes
    around the sort's items per workgroup."""
    if name == "planar":
        pts = oc.cloud(hb.P).clone()
        pts[:, 2] = 0
    elif name == "identical":
        pts = oc.cloud(33)[7:8].repeat(hb.P, 1).contiguous()
    else:
        pts = oc.cloud(name)
    m = ops.morton_order(pts.cuda())
    torch.cuda.synchronize()
    assert m.dtype == torch.int32 and oc.is_permutation(m.cpu().numpy(), pts.shape[0])
