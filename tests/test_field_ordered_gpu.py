"""The ordered field backward on the GPU (include/mom4d.h, "ordered HexPlane backward", "ordered MLP weight gradients"): its gradients
are a function of their inputs bit for bit, its order is the documented one, the gradients are still the right ones, and the switch
carries it through autograd and through the fine stage's training iteration.  Nothing here asserts that the atomic path differs."""
import ctypes as C
import functools
import importlib
import random

import numpy as np
import pytest
import torch

import deform_mlp_cases as dc
import field_ordered_cases as fc
import hexplane_box_cases as hb
import hexplane_order_cases as hoc

pytestmark = pytest.mark.gpu

pkg = fc.pkg
ops = importlib.import_module(pkg + ".ops")
N = fc.N

FIELDS = {"small32": (32, "small"), "small16": (16, "small"), "mid32": (32, "mid"), "mid16": (16, "mid"), "three16": (16, "three_levels")}
CLOUDS = ("points", "one64", "one65", "one300", "outside", "single")
CASES = [(fk, c) for fk in FIELDS for c in CLOUDS] + [("small32", "cloud5000"), ("small16", "cloud5000")]


def _cloud(name, shape):
    if name == "points":
        return hb.points(hoc.BOX)                  # 300 points with the face, corner and one-ulp points
    if name.startswith("one"):
        return hoc.one_cell_cloud(int(name[3:]), shape=shape)       # one segment that crosses the block boundaries in every plane
    if name == "outside":
        return hoc.outside_cloud()                 # every position is a border position
    if name == "single":
        return hb.points(hoc.BOX)[5:6].clone()
    return hoc.cloud(5000)                         # long runs per texel on "small"


def _times(shape):
    return (0.0, hoc.spec(shape)[2], 1.0)          # at 1.0 the upper time row is outside


@functools.lru_cache(maxsize=None)
def _field(fk):
    channels, shape = FIELDS[fk]
    return hoc.field(channels, hoc.BOX, shape).cuda()


def _pattern(n, salt):
    """A known gradient to add onto: never zero, exact in fp32."""
    i = torch.arange(n, dtype=torch.int64)
    return (((i * 37 + salt * 11) % 101).float() - 50.5) / 64.0


def _aligned(buf):
    return buf[(-buf.data_ptr()) % 256:]


def _ordered(f, pts, t, w, order=None, fill=None, prefill=True):
    """One mom_hexplane_backward_ordered: plane gradients [[H, W, C]] and dxyz as numpy, the incoming values, the read-back scratch."""
    lib = N.lib()
    levels = [[p.detach() for p in lv] for lv in f.grids]
    grads, g_in = [], []
    for l, lv in enumerate(levels):
        grads.append([])
        g_in.append([])
        for i, p in enumerate(lv):
            g = torch.zeros_like(p)                          # keeps the channel-last strides
            st = ops.plane_storage(g)
            if prefill:
                st.copy_(_pattern(st.numel(), 6 * l + i).view(st.shape))
            grads[l].append(g)
            g_in[l].append(st.cpu().numpy().copy())
    hp, keep = ops._hexplane_desc(levels, f.aabb, grads, aabb_host=f.aabb_host())
    P = pts.shape[0]
    xyz = pts.cuda().contiguous()
    dfeat = w.cuda().contiguous()
    dxyz = (_pattern(3 * P, 99).view(P, 3) if prefill else torch.zeros(P, 3)).cuda()
    dxyz_in = dxyz.cpu().numpy().copy()
    need = lib.mom_hexplane_ordered_scratch_bytes(C.byref(hp), P)
    assert need > 0
    scratch = torch.empty(need, dtype=torch.uint8, device="cuda")
    if fill is not None:
        scratch.fill_(fill)
    N.check(lib.mom_hexplane_backward_ordered(C.byref(hp), P, xyz.data_ptr(), float(t), None if order is None else order.data_ptr(),
                                              dfeat.data_ptr(), dxyz.data_ptr(), scratch.data_ptr(), scratch.numel(), N.current_stream()),
            "mom_hexplane_backward_ordered")
    torch.cuda.synchronize()
    return dict(grads=[[ops.plane_storage(g).cpu().numpy() for g in lv] for lv in grads], dxyz=dxyz.cpu().numpy(), g_in=g_in,
                dxyz_in=dxyz_in, scratch=_aligned(scratch).cpu().numpy(), levels=hp.levels, channels=hp.channels)


def _same_bits(a, b, what):
    for l, (la, lb) in enumerate(zip(a["grads"], b["grads"])):
        for p, (x, y) in enumerate(zip(la, lb)):
            assert np.array_equal(fc.bits(x), fc.bits(y)), (what, "plane", l, p)
    assert np.array_equal(fc.bits(a["dxyz"]), fc.bits(b["dxyz"])), (what, "dxyz")


@functools.lru_cache(maxsize=None)
def _first(fk, cloud, t):
    """The first ordered backward of a case (incoming gradients prefilled), shared by the tests below and never modified."""
    f = _field(fk)
    pts = _cloud(cloud, FIELDS[fk][1])
    return _ordered(f, pts, t, hb.weights(f.feat_dim, n=pts.shape[0]))


@pytest.mark.parametrize("fk,cloud", CASES)
def test_the_gradients_are_a_function_of_their_inputs(fk, cloud):
    f = _field(fk)
    shape = FIELDS[fk][1]
    pts = _cloud(cloud, shape)
    P = pts.shape[0]
    w = hb.weights(f.feat_dim, n=P)
    morton = ops.morton_order(pts.cuda())
    perm = torch.randperm(P, generator=torch.Generator().manual_seed(31)).to(torch.int32).cuda()
    for t in _times(shape):
        first = _first(fk, cloud, t)
        _same_bits(_ordered(f, pts, t, w), first, (fk, cloud, t, "twice"))
        for fill in (0xFF, 0x3C):
            _same_bits(_ordered(f, pts, t, w, fill=fill), first, (fk, cloud, t, "dirty scratch", fill))
        _same_bits(_ordered(f, pts, t, w, order=morton), first, (fk, cloud, t, "Morton order"))
        _same_bits(_ordered(f, pts, t, w, order=perm, fill=0xFF), first, (fk, cloud, t, "random order"))


@pytest.mark.parametrize("fk,cloud", CASES)
def test_the_order_is_the_documented_one(fk, cloud):
    f = _field(fk)
    channels, shape = FIELDS[fk]
    pts = _cloud(cloud, shape).numpy()
    P = len(pts)
    res = fc.field_res(f)
    for t in _times(shape):
        r = _first(fk, cloud, t)
        gv, part = fc.hex_scratch_views(r["scratch"], r["levels"], channels, P)
        want, want_dxyz = fc.host_twin(channels, hoc.BOX, res, pts, t, gv, r["g_in"], part, r["dxyz_in"])
        for l in range(len(res)):
            for p in range(6):
                assert np.array_equal(fc.bits(r["grads"][l][p]), fc.bits(want[l][p])), (fk, cloud, t, "plane", l, p)
                # a texel none of whose four cells holds a point keeps the bits it had
                key, _, Wd, Hd = fc.plane_samples(pts, t, hoc.BOX, res[l], p)
                occ = np.zeros((Hd, Wd), bool)
                occ[key // Wd, key % Wd] = True
                texel = np.zeros((Hd, Wd), bool)                 # the texels with a term: the corners of the occupied cells
                ys, xs = np.nonzero(occ)
                for dy in (0, 1):
                    for dx in (0, 1):
                        ok = (ys + dy < Hd) & (xs + dx < Wd)
                        texel[ys[ok] + dy, xs[ok] + dx] = True
                same = fc.bits(r["grads"][l][p]) == fc.bits(r["g_in"][l][p])
                assert same[~texel].all(), (fk, cloud, t, "a texel without a term was written", l, p)
        assert np.array_equal(fc.bits(r["dxyz"]), fc.bits(want_dxyz)), (fk, cloud, t, "dxyz")


def _oracles(f, pts, t, w):
    """(fp32 oracle: features, dxyz, planes; float64 oracle's planes) of oracle.torch_ref.hexplane_features at timestamp t."""
    from oracle import torch_ref as tr
    ref32 = hb.oracle_of(f, pts, t, w)
    fcpu = [[q.detach().cpu().double().contiguous().requires_grad_(True) for q in g] for g in f.grids]
    p = pts.double().requires_grad_(True)
    feat = tr.hexplane_features(p, t, f.aabb.detach().cpu().double(), fcpu)
    (feat * w.double()).sum().backward()
    return ref32, [[q.grad.numpy() for q in g] for g in fcpu]


def _atomic(f, pts, t, w):
    """The atomic path on the same inputs (the switch is off): ops.hexplane_features without plane orders."""
    levels = [list(g) for g in f.grids]
    f.zero_grad()
    p = pts.cuda().requires_grad_(True)
    feat = ops.hexplane_features(p, t, f.aabb, levels, aabb_host=f.aabb_host())
    (feat * w.cuda()).sum().backward()
    torch.cuda.synchronize()
    return [[ops.plane_storage(q.grad).cpu().numpy() for q in g] for g in f.grids], p.grad.cpu().numpy()


@pytest.mark.parametrize("fk,cloud", CASES)
def test_still_the_right_gradients(fk, cloud):
    f = _field(fk)
    shape = FIELDS[fk][1]
    pts = _cloud(cloud, shape)
    w = hb.weights(f.feat_dim, n=pts.shape[0])
    for t in _times(shape):
        what = f"{fk} {cloud} t={t}"
        r = _ordered(f, pts, t, w, prefill=False)
        ref32, planes64 = _oracles(f, pts, t, w)
        ref_planes = [[np.ascontiguousarray(q[0].transpose(1, 2, 0)) for q in lv] for lv in planes64]      # [1, C, H, W] -> [H, W, C]
        worst = max(hoc.plane_error_ratio(a, b) for la, lb in zip(r["grads"], ref_planes) for a, b in zip(la, lb))
        atomic_planes, atomic_dxyz = _atomic(f, pts, t, w)
        gate = max(hoc.plane_error_ratio(a, b) for la, lb in zip(atomic_planes, r["grads"]) for a, b in zip(la, lb))
        print(f"{what}: plane gradients / tolerance: ordered against float64 {worst:.3f}, atomic against ordered {gate:.3f}")
        assert worst <= 1, what
        assert gate <= 1, what
        np.testing.assert_allclose(r["dxyz"], ref32[1], rtol=hb.GRAD_RTOL, atol=hb.grad_atol(ref32[1]), err_msg=what + " dxyz")
        np.testing.assert_allclose(atomic_dxyz, r["dxyz"], rtol=hb.GRAD_RTOL, atol=hb.grad_atol(r["dxyz"]), err_msg=what + " atomic dxyz")


# ---------------------------------------------------------------------------------------- MLP
MLP_SIZES = (1, 31, 33, 300, 8233)          # 8233: 258 tiles, so a persistent workgroup takes more than one tile, with an odd tail


@functools.lru_cache(maxsize=None)
def _mlp_dev(P, n_in, kind="dense"):
    c = dc.case(P, n_in, kind)
    up = lambda a: torch.tensor(np.asarray(a)).cuda()
    return dict(params=[up(p) for p in c["params"]], douts=[up(d) for d in c["douts"]], feat=up(c["feat"]))


def _mlp_ordered(P, n_in, kind, a0, fill):
    lib = N.lib()
    g = _mlp_dev(P, n_in, kind)
    grads = [torch.zeros_like(p) for p in g["params"]]
    d = ops.DeformMLPFunction._desc(g["params"], grads)
    dfeat = torch.full((P, n_in), float("nan"), device="cuda")
    need = lib.mom_deform_backward_ordered_scratch_bytes(P)
    scratch = torch.empty(need, dtype=torch.uint8, device="cuda").fill_(fill)
    dpts, dsc, dro = g["douts"]
    N.check(lib.mom_deform_backward_ordered_n(C.byref(d), P, n_in, g["feat"].data_ptr(), a0.data_ptr(), dpts.data_ptr(), dsc.data_ptr(),
                                              dro.data_ptr(), dfeat.data_ptr(), scratch.data_ptr(), need, N.current_stream()),
            "mom_deform_backward_ordered_n")
    torch.cuda.synchronize()
    out = dict(zip(dc.GRAD_NAMES, (t.cpu().numpy() for t in grads)))
    out["dfeat"] = dfeat.cpu().numpy()
    return out, scratch.cpu().numpy().view(np.float32)


@pytest.mark.parametrize("kind", ["dense", "needle"])          # needle: a Gaussian lost or counted twice is an error of 100 % of its bound
@pytest.mark.parametrize("n_in", [32, 64])
@pytest.mark.parametrize("P", MLP_SIZES)
def test_mlp_weight_gradients_are_ordered(P, n_in, kind):
    a0_np, v, e = dc.backward_ref(P, n_in, kind, False)            # the f32 kernels' float64 bounds
    a0 = torch.tensor(a0_np).cuda()
    one, scratch = _mlp_ordered(P, n_in, kind, a0, 0xFF)
    two, _ = _mlp_ordered(P, n_in, kind, a0, 0x3C)
    names = ("dfeat",) + dc.GRAD_NAMES
    for k in names:
        assert np.array_equal(fc.bits(one[k]), fc.bits(two[k])), (P, n_in, k)
    worst = {k: dc.share(one[k], v[k], e[k]) for k in names}
    print(f"ordered backward in={n_in} P={P} {kind} largest share of the bound:", " ".join("%s %.3f" % kv for kv in worst.items()))
    assert not {k: s for k, s in worst.items() if not s <= 1.0}, (P, n_in, worst)
    # the records in the scratch, added up in the documented order in numpy, are the gradients (the buffers held +0.0)
    dx, dw = fc.mlp_scratch_views(scratch, P)
    want = fc.mlp_reduce_numpy(dx, dw, P, n_in, dc.GRAD_NAMES)
    for k in dc.GRAD_NAMES:
        assert np.array_equal(fc.bits(one[k]), fc.bits(want[k])), (P, n_in, k)


@pytest.mark.parametrize("P", [300, 8233])
def test_the_default_64_feature_backward_repeats(P, monkeypatch):
    """csrc/deform_bwd_b3.hip adds its workgroups' partial sums in a fixed order: the form set_deterministic keeps for 64 features."""
    monkeypatch.delenv("MOM_MLP_BWD", raising=False)
    lib = N.lib()
    g = _mlp_dev(P, 64)
    a0 = torch.tensor(dc.backward_ref(P, 64, "dense", True)[0]).cuda()
    runs = []
    for fill in (0xFF, 0x3C):
        grads = [torch.zeros_like(p) for p in g["params"]]
        d = ops.DeformMLPFunction._desc(g["params"], grads)
        dfeat = torch.empty((P, 64), device="cuda")
        scratch = torch.empty(lib.mom_deform_backward_scratch_bytes(P), dtype=torch.uint8, device="cuda").fill_(fill)
        dpts, dsc, dro = g["douts"]
        N.check(lib.mom_deform_backward_n(C.byref(d), P, 64, g["feat"].data_ptr(), a0.data_ptr(), dpts.data_ptr(), dsc.data_ptr(),
                                          dro.data_ptr(), dfeat.data_ptr(), scratch.data_ptr(), N.current_stream()), "mom_deform_backward_n")
        torch.cuda.synchronize()
        runs.append([t.cpu().numpy() for t in grads] + [dfeat.cpu().numpy()])
    for k, (a, b) in enumerate(zip(*runs)):
        assert np.array_equal(fc.bits(a), fc.bits(b)), (P, k)


# ---------------------------------------------------------------------------------------- through autograd and the fine stage
def _autograd_pass(f, n_in):
    c = dc.case(hb.P, n_in, "dense")
    up = lambda a: torch.tensor(np.asarray(a)).cuda()
    params = [up(p).requires_grad_(True) for p in c["params"]]
    xyz = hb.points(hoc.BOX).cuda().requires_grad_(True)
    scal, rot = up(c["scal"]).requires_grad_(True), up(c["rot"]).requires_grad_(True)
    f.zero_grad()
    feat = ops.hexplane_features(xyz, 0.3, f.aabb, [list(g) for g in f.grids], aabb_host=f.aabb_host())
    pts, sc, ro = ops.deform_mlp(feat, xyz, scal, rot, up(c["flow"]), dc.FLOW_COEF, params)
    dpts, dsc, dro = (up(d) for d in c["douts"])
    ((pts * dpts).sum() + (sc * dsc).sum() + (ro * dro).sum()).backward()
    torch.cuda.synchronize()
    leaves = [xyz, scal, rot, *params, *[q for g in f.grids for q in g]]
    return [t.grad.detach().clone() for t in leaves]


@pytest.mark.parametrize("fk,n_in", [("small32", 64), ("small16", 32)])
def test_through_autograd_under_the_switch(fk, n_in):
    from hip_helpers import RC
    f = _field(fk)
    assert f.feat_dim == n_in and RC.deterministic() is False
    RC.set_deterministic(True)
    try:
        one, two = _autograd_pass(f, n_in), _autograd_pass(f, n_in)
        ctx_times = torch.full((hb.P, 1), 0.3, device="cuda")
        xyz = hb.points(hoc.BOX).cuda().requires_grad_(True)
        feat = ops.hexplane_features(xyz, ctx_times, f.aabb, [list(g) for g in f.grids], aabb_host=f.aabb_host())
        with pytest.raises(N.MomError, match="set_deterministic"):          # per-point timestamps: refused, never the atomic kernel
            feat.sum().backward()
    finally:
        RC.set_deterministic(False)
        f.zero_grad()
    fo = RC._state["field_ordered"]
    assert fo is not None and fo["hex"] is not None and fo["mlp"] is not None
    for k, (a, b) in enumerate(zip(one, two)):
        assert torch.equal(a, b), (fk, k)


def _fine_run(iterations, model, per_op, **trainer_kw):
    """tests/test_raster_ordered_gpu.py::_coarse_run's recipe at the fine stage, for the default 32 x 2 model or a 16 x 2 one."""
    A, S, T = (importlib.import_module(f"{pkg}.{m}") for m in ("arguments", "scene", "train"))
    if model == 16:
        kc = {'grid_dimensions': 2, 'input_coordinate_dim': 4, 'output_coordinate_dim': 16, 'resolution': [64, 64, 64, 10]}
        args, lp, op, pp, hp = A.default_args(kplanes_config=kc, multires=[1, 2])
    else:
        args, lp, op, pp, hp = A.default_args(time_resolution=10)
    assert hp.net_width == 64 and hp.kplanes_config["output_coordinate_dim"] == model and list(hp.multires) == [1, 2]
    pp.per_op_autograd = per_op
    op.lambda_dssim = 0.0
    torch.manual_seed(6666)
    random.seed(6666)
    np.random.seed(6666)
    scene = S.SyntheticScene(1500, 3, 96, 64, seed=6666)
    g = S.GaussianModel(lp.sh_degree, hp, device=torch.device("cuda"))
    scene.init_gaussians(g)
    scene.make_trained_like(g)
    trainer = T.Trainer(scene, g, op, hp, pp, stage="fine", delta_scale=1, sync_every_step=False, **trainer_kw)
    for it in range(1, iterations + 1):
        trainer.step(it)
    torch.cuda.synchronize()
    state = {}
    for group in g.optimizer.param_groups:
        for p in group["params"]:
            st = g.optimizer.state.get(p, {})
            key = group["name"] if len(group["params"]) == 1 else (group["name"], len([k for k in state if k[0] == group["name"]]))
            state[key] = (p.detach().clone(), {k: v.detach().clone() for k, v in st.items() if torch.is_tensor(v)})
    return state


@pytest.mark.parametrize("per_op", [True, False])
@pytest.mark.parametrize("model", [32, 16])
def test_the_fine_stage_repeats_bit_for_bit(model, per_op):
    from hip_helpers import RC
    try:
        a = _fine_run(6, model, per_op, fused=False, deterministic=True)
        assert RC.deterministic() is True and RC.ordered_status() == 0
        b = _fine_run(6, model, per_op, fused=False, deterministic=True)
        assert RC.ordered_status() == 0
    finally:
        RC.set_deterministic(False)
    assert set(a) == set(b)
    names = {k if isinstance(k, str) else k[0] for k in a}
    assert {"deformation", "grid"} <= names and len(names) >= 8           # the six Gaussian groups, the MLP and the planes
    moments = 0
    for name in a:
        assert torch.equal(a[name][0], b[name][0]), name
        assert set(a[name][1]) == set(b[name][1]), name
        for k in a[name][1]:
            assert torch.equal(a[name][1][k], b[name][1][k]), (name, k)
            moments += 1
    assert moments >= 16                                                   # both Adam moments: six Gaussian groups, the MLP, the planes
