"""The one-pass densify round on the GPU (csrc/densify_round.hip through ops.densify_round and GaussianModel.densify()):
plan and data movement against plain torch indexing at every size where the scan or the word walk takes another path, the
split's children against float64 with the op-by-op round's own arithmetic as the yardstick, the generator, and the whole round
of a model on both routes."""
import ctypes as C
import importlib

import numpy as np
import pytest
import torch

from densify_round_cases import children_fp64, children_torch, expected_layout, round_masks, xyz_error_scale

pytestmark = pytest.mark.gpu
pkg = "iclr2025_3d-mom_amd"
N = importlib.import_module(pkg + "._native")
ops = importlib.import_module(pkg + ".ops")
GaussianModel = importlib.import_module(pkg + ".scene.gaussian_model").GaussianModel

SIZES = [1, 255, 256, 257, 2047, 2048, 2049, 6000]


# ------------------------------------------------------------------------------------------------ kernel level
def make_tensors(P, gen):
    """Every row width and word path: 1-byte rows (bool), 4, 12, 16 and 180 bytes, a zero-width tensor, and 4-byte rows at an
    odd address (the 1-byte walk).  Quaternions of norm ~1e-3, ~1 and ~1e3, scalings in [-8, 2]."""
    r = lambda *s: torch.randn(*s, generator=gen)
    rot = r(P, 4)
    rot = rot * torch.tensor([1e-3, 1.0, 1e3])[torch.arange(P) % 3][:, None]
    odd = torch.randint(0, 255, (4 * P + 1,), generator=gen, dtype=torch.uint8)
    return {"xyz": r(P, 3) * 3, "scaling": torch.rand(P, 3, generator=gen) * 10 - 8, "rotation": rot,
            "copy": [torch.rand(P, generator=gen) < 0.5, r(P, 1), r(P, 3), r(P, 4), r(P, 15, 3), r(P, 0, 3), odd],
            "moment": [r(P, 3), r(P, 15, 3), r(P, 4)], "zero": [r(P, 1), r(P, 3), r(P)]}


def to_gpu(t):
    g = {k: [x.cuda() for x in v] if isinstance(v, list) else v.cuda() for k, v in t.items()}
    P = t["xyz"].shape[0]
    g["copy"][-1] = g["copy"][-1][1:].view(P, 4)             # [P,4] bytes at base + 1
    assert g["copy"][-1].data_ptr() % 2 == 1 and g["copy"][-1].is_contiguous()
    return g


def on_cpu(t):
    c = dict(t)
    P = t["xyz"].shape[0]
    c["copy"] = list(t["copy"][:-1]) + [t["copy"][-1][1:].view(P, 4)]
    return c


def patterns(P, gen):
    f = lambda: torch.zeros(P, dtype=torch.bool)
    out = [("none", f(), f()), ("all clone", ~f(), f()), ("all split", f(), ~f())]
    i = torch.arange(P)
    out.append(("alternating", i % 3 == 0, i % 3 == 1))
    for name, row in (("first", 0), ("last", P - 1)):
        for kind in (0, 1):
            m = f()
            m[row] = True
            out.append((f"{name} row {'split' if kind else 'clone'}", f() if kind else m, m if kind else f()))
    for frac in (0.1, 0.5):
        u = torch.rand(P, generator=gen)
        out.append((f"random {frac}", u < frac / 2, (u >= frac / 2) & (u < frac)))
    # a run of split rows across a boundary of the scan's workgroups (row 2048) or, below that, of the apply's chunks (row 256)
    edge = 2048 if P > 2048 else 256 if P > 256 else P - 1
    s = f()
    s[max(edge - 9, 0):min(edge + 12, P)] = True
    c = f()
    c[:max(edge - 9, 0):5] = True
    out.append((f"split run over row {edge}", c, s))
    return out


_results = {}


def kernel_cases(P):
    """Every mask pattern at P through ops.densify_round, once; the expected layout from the CPU; the children's errors."""
    if P in _results:
        return _results[P]
    gen = torch.Generator().manual_seed(1000 + P)
    cpu = make_tensors(P, gen)
    gpu, cpu = to_gpu(cpu), on_cpu(cpu)
    rows = []
    for name, clone, split in patterns(P, gen):
        S = int(split.sum())
        z = torch.randn(2 * S, 3, generator=gen) if S else None
        out = ops.densify_round(clone.cuda(), split.cuda(), gpu, z=None if z is None else z.cuda())
        want = expected_layout((clone, split), cpu, z)
        err = None
        if S:
            par = [cpu[k][split] for k in ("xyz", "scaling", "rotation")]
            tx, ts = children_fp64(*par, z)
            yx, ys = children_torch(*[p.cuda() for p in par], z.cuda())                 # the op-by-op round's arithmetic, here
            gx, gs = out["xyz"][-2 * S:], out["scaling"][-2 * S:]
            scale = xyz_error_scale(par[0], par[1], z)
            err = dict(S=S, kx=float(((gx.cpu().double() - tx).abs() / scale).max()),
                       yx=float(((yx.cpu().double() - tx).abs() / scale).max()),
                       ks=float((gs.cpu().double() - ts).abs().max()), ys=float((ys.cpu().double() - ts).abs().max()),
                       same_x=int((gx == yx).all(dim=1).sum()), same_s=int((gs == ys).all(dim=1).sum()))
        rows.append((name, clone, split, out, want, err))
    _results[P] = rows
    return rows


@pytest.mark.parametrize("P", SIZES)
def test_plan_and_movement_match_plain_indexing(P):
    for name, clone, split, out, want, _ in kernel_cases(P):
        C_, S = int(clone.sum()), int(split.sum())
        assert out["counts"] == (P - S, C_, S), name
        n_old = P - S + C_
        for key in ("copy", "moment", "zero"):
            assert len(out[key]) == len(want[key])
            for i, (a, b) in enumerate(zip(out[key], want[key])):
                assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.cpu(), b), (name, key, i)
        assert torch.equal(out["rotation"].cpu(), want["rotation"]), name
        for key in ("xyz", "scaling"):
            assert out[key].shape == want[key].shape, (name, key)
            assert torch.equal(out[key][:n_old].cpu(), want[key][:n_old]), (name, key)       # kept rows and clones: bit-equal
            assert bool(torch.isfinite(out[key]).all()), (name, key)


def test_children_are_as_close_to_float64_as_the_op_by_op_round():
    """Every child row of every case above with S > 0 (quaternions of norm 1e-3 .. 1e3, scalings in [-8, 2]).  Truth: the formulas
    in float64.  Yardstick: the op-by-op round's torch sequence on the GPU, same inputs, same run.  Position error of element
    (row, k): |got - truth| / (max_k |xyz_parent| + sum_k |sigma_k z_k|); scaling error: |got - truth|.  Bound: the kernel's maximum
    is at most twice the yardstick's -- the two may differ in the order of a three-term sum and by an ulp of exp / log.  The maxima
    run over all cases together: a single-row case has six elements, and the maximum of six rounding errors says nothing.
    Measured on an MI355X: positions 3.259e-7 against 3.259e-7, bit-equal on all 42 404 rows; scaling 5.012e-7 against 9.293e-7
    (the kernel rounds the logarithm once from double).  The positions' bit equality rests on torch's
    order for a four-term sum and on the BLAS inner loop, neither a contract, so the bound is what is asserted."""
    kx = yx = ks = ys = 0.0
    rows = same_x = same_s = 0
    for P in SIZES:
        for name, _, _, _, _, e in kernel_cases(P):
            if e is None:
                continue
            print(f"P={P:5d} {name:24s} S={e['S']:5d} xyz kernel {e['kx']:.3e} torch {e['yx']:.3e}   scaling kernel {e['ks']:.3e} "
                  f"torch {e['ys']:.3e}   bit-equal rows xyz {e['same_x']}/{2 * e['S']} scaling {e['same_s']}/{2 * e['S']}")
            kx, yx, ks, ys = max(kx, e["kx"]), max(yx, e["yx"]), max(ks, e["ks"]), max(ys, e["ys"])
            rows, same_x, same_s = rows + 2 * e["S"], same_x + e["same_x"], same_s + e["same_s"]
    print(f"children: xyz kernel {kx:.3e} torch {yx:.3e}; scaling kernel {ks:.3e} torch {ys:.3e}; "
          f"bit-equal rows xyz {same_x}/{rows} scaling {same_s}/{rows}")
    assert rows > 10000 and yx > 0 and ys > 0
    assert kx <= 2 * yx, (kx, yx)
    assert ks <= 2 * ys, (ks, ys)


def test_the_one_workgroup_scan_takes_a_second_trip():
    """P = 256 * 2048 + 1: 257 workgroup counts, so the scan of the counts loops twice.  Plan only, against cumsum on the CPU."""
    P = 256 * 2048 + 1
    gen = torch.Generator().manual_seed(9)
    u = torch.rand(P, generator=gen)
    clone, split = u < 0.2, (u >= 0.2) & (u < 0.5)
    split[-1] = True
    lib = N.lib()
    index = torch.full((3, P), -7, dtype=torch.int32, device="cuda")
    counts_dev = torch.zeros(3, dtype=torch.int32, device="cuda")
    counts_host = torch.zeros(3, dtype=torch.int32).pin_memory()
    scratch = torch.empty(lib.mom_densify_scratch_bytes(P), dtype=torch.uint8, device="cuda")
    cm, sm = clone.cuda().view(torch.uint8), split.cuda().view(torch.uint8)
    N.check(lib.mom_densify_plan(P, cm.data_ptr(), sm.data_ptr(), index[0].data_ptr(), index[1].data_ptr(), index[2].data_ptr(),
                                 counts_dev.data_ptr(), counts_host.data_ptr(), scratch.data_ptr(), N.current_stream()), "plan")
    torch.cuda.synchronize()
    S, C_ = int(split.sum()), int(clone.sum())
    assert counts_host.tolist() == [P - S, C_, S] == counts_dev.cpu().tolist()
    minus = torch.full((P,), -1, dtype=torch.int64)
    kept = torch.where(split, minus, torch.cumsum((~split).long(), 0) - 1)
    crank = torch.where(clone, torch.cumsum(clone.long(), 0) - 1, minus)
    srank = torch.where(split, torch.cumsum(split.long(), 0) - 1, minus)
    got = index.cpu().long()
    assert torch.equal(got[0], kept) and torch.equal(got[1], crank) and torch.equal(got[2], srank)


def test_an_sh_degree_0_model_has_zero_width_rows():
    P = 300
    gen = torch.Generator().manual_seed(4)
    t = {"copy": [torch.randn(P, 0, 3, generator=gen).cuda(), torch.randn(P, 1, 3, generator=gen).cuda()],
         "moment": [torch.zeros(P, 0, 3).cuda()]}
    clone = (torch.arange(P) % 7 == 0).cuda()
    out = ops.densify_round(clone, torch.zeros(P, dtype=torch.bool).cuda(), t)
    C_ = int(clone.sum())
    assert out["counts"] == (P, C_, 0) and out["z"] is None
    assert out["copy"][0].shape == (P + C_, 0, 3) and out["moment"][0].shape == (P + C_, 0, 3)
    assert torch.equal(out["copy"][1], torch.cat([t["copy"][1], t["copy"][1][clone]]))


# ------------------------------------------------------------------------------------------------ the generator
@pytest.mark.parametrize("S", [1, 2, 7, 333, 5000])
def test_normal_with_a_std_tensor_is_randn_times_std_on_the_gpu(S):
    """The fused round draws z = randn(2S, 3) where the op-by-op round calls torch.normal(zeros(2S, 3), std): the same numbers
    from the same Philox offsets, and the same generator state afterwards."""
    std = (torch.rand(2 * S, 3, generator=torch.Generator().manual_seed(S)) * 3 + 0.01).cuda()
    torch.cuda.manual_seed(77)
    a = torch.normal(mean=torch.zeros((2 * S, 3), device="cuda"), std=std)
    state_a = torch.cuda.get_rng_state()
    torch.cuda.manual_seed(77)
    z = torch.randn((2 * S, 3), dtype=torch.float32, device="cuda")
    state_z = torch.cuda.get_rng_state()
    assert torch.equal(a, (z * std).add_(torch.zeros_like(z)))
    assert torch.equal(state_a, state_z)


# ------------------------------------------------------------------------------------------------ whole round, old against new
PARAMS = ("_xyz", "_features_dc", "_features_rest", "_scaling", "_rotation", "_opacity")
GROUP_OF = {"_xyz": "xyz", "_features_dc": "f_dc", "_features_rest": "f_rest", "_scaling": "scaling", "_rotation": "rotation",
            "_opacity": "opacity"}


def _model_state():
    """The recipe of test_ops_gpu.py's round: a tiny bench state, one optimizer step on seeded gradients, seeded statistics."""
    import bench
    cfg = dict(P=6000, F=4, W=160, H=96, time_res=10, name="tiny")
    scene, g, trainer, op = bench.build_state(cfg, torch.device("cuda"), fused=True)
    gen = torch.Generator().manual_seed(5)
    n = g.get_xyz.shape[0]
    for grp in g.optimizer.param_groups:
        for p_ in grp["params"]:
            p_.grad = (torch.randn(p_.shape, generator=gen) * 1e-3).to(p_.device).contiguous()
            if p_.dim() == 4:                              # planes are channel-last: keep the parameter's strides
                p_.grad = p_.grad.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    g.optimizer.step()
    g.optimizer.zero_grad(set_to_none=True)
    g.xyz_gradient_accum = (torch.rand(n, 1, generator=gen) * 4e-4).cuda()
    g.denom = torch.ones(n, 1, device="cuda")
    g.max_radii2D = (torch.rand(n, generator=gen) * 30).cuda()
    g._deformation_accum = torch.rand(n, 3, generator=gen).cuda()
    g._deformation_table = (torch.rand(n, generator=gen) < 0.7).cuda()
    return scene, g, trainer, gen


def _snapshot(g):
    out = {k: getattr(g, k) for k in PARAMS + ("_deformation_table", "_scene_flow", "max_radii2D", "xyz_gradient_accum", "denom",
                                               "_deformation_accum")}
    for k in PARAMS:
        st = g.optimizer.state[getattr(g, k)]
        out["m" + k], out["v" + k] = st["exp_avg"], st["exp_avg_sq"]
    return {k: v.detach().clone() for k, v in out.items()}


def _round(fused, tweak, max_grad):
    scene, g, trainer, gen = _model_state()
    tweak(g, scene)
    before = _snapshot(g)
    saved = GaussianModel.FUSED_DENSIFY
    GaussianModel.FUSED_DENSIFY = fused
    try:
        torch.manual_seed(11)
        torch.cuda.manual_seed(11)
        g.densify(max_grad, 0.005, scene.cameras_extent, 20, 5, 5, scene.model_path, 5100, "fine")
        rng = torch.cuda.get_rng_state()
    finally:
        GaussianModel.FUSED_DENSIFY = saved
    after = _snapshot(g)
    by_name = {grp["name"]: grp["params"][0] for grp in g.optimizer.param_groups if len(grp["params"]) == 1}
    for k in PARAMS:
        assert by_name[GROUP_OF[k]] is getattr(g, k) and getattr(g, k).requires_grad      # the groups name the new Parameters
        assert getattr(g, k) in g.optimizer.state
    n1 = g.get_xyz.shape[0]
    g.max_radii2D = (torch.rand(n1, generator=gen) * 30).cuda()
    g.prune(max_grad, 0.02, scene.cameras_extent, 20)
    assert g.get_xyz.shape[0] <= n1
    loss = trainer.step(5101, cams=[trainer.cams[0]])          # the model still trains after the surgery
    assert np.isfinite(float(loss))
    return before, after, rng, (g.percent_dense, scene.cameras_extent)


def _dense(v):
    def tweak(g, scene):
        g.percent_dense = v
    return tweak


def _balanced(g, scene):
    """The scale threshold at the median of the rows' largest scale: about half of the candidates clone, half split."""
    g.percent_dense = float(g.get_scaling.max(dim=1).values.median()) / scene.cameras_extent


ROUNDS = {"clone and split": (_balanced, 0.0002, True, True),
          "nothing splits": (_dense(1e9), 0.0002, True, False),            # every candidate is small: clones only
          "nothing clones": (_dense(0.0), 0.0002, False, True),            # every candidate is large: splits only
          "nothing at all": (_balanced, 1e9, False, False)}


@pytest.mark.parametrize("case", list(ROUNDS))
def test_whole_round_old_route_against_new(case):
    tweak, max_grad, clones, splits = ROUNDS[case]
    b_old, old, rng_old, (pd, extent) = _round(False, tweak, max_grad)
    b_new, new, rng_new, _ = _round(True, tweak, max_grad)
    for k in b_old:
        assert torch.equal(b_old[k], b_new[k]), k                       # both routes start from one state
    clone, split = round_masks(b_old["xyz_gradient_accum"].clone(), b_old["denom"], b_old["_scaling"], max_grad, pd, extent)
    P, C_, S = clone.shape[0], int(clone.sum()), int(split.sum())
    assert (C_ > 0) == clones and (S > 0) == splits, (C_, S)            # the old route does what the case is named for
    n_old = P - S + C_
    assert old["_xyz"].shape[0] == new["_xyz"].shape[0] == n_old + 2 * S
    assert torch.equal(rng_old, rng_new)                                # the generator is where the op-by-op round leaves it
    for k in old:
        assert old[k].shape == new[k].shape and old[k].dtype == new[k].dtype, k
        if k in ("_xyz", "_scaling"):
            assert torch.equal(old[k][:n_old], new[k][:n_old]), k
        else:
            assert torch.equal(old[k], new[k]), k
    for k in ("max_radii2D", "xyz_gradient_accum", "denom", "_deformation_accum"):
        assert new[k].shape[0] == n_old + 2 * S and float(new[k].abs().sum()) == 0.0, k
    for k in PARAMS:                                                    # moments: kept rows kept, new rows zero
        for m in ("m", "v"):
            assert torch.equal(new[m + k][:P - S], b_new[m + k][~split]) and float(new[m + k][P - S:].abs().sum()) == 0.0, m + k
    if not S:
        assert torch.equal(old["_xyz"], new["_xyz"]) and torch.equal(old["_scaling"], new["_scaling"])
        return
    # the children: every row, under the bound of test_children_are_as_close_to_float64_as_the_op_by_op_round, with the old
    # route's rows as the yardstick
    torch.manual_seed(11)
    torch.cuda.manual_seed(11)
    z = torch.randn((2 * S, 3), dtype=torch.float32, device="cuda")
    par = [b_old[k][split] for k in ("_xyz", "_scaling", "_rotation")]
    tx, ts = children_fp64(*par, z)
    scale = xyz_error_scale(par[0], par[1], z)
    ex = lambda t: float(((t[n_old:].cpu().double() - tx).abs() / scale).max())
    es = lambda t: float((t[n_old:].cpu().double() - ts).abs().max())
    kx, yx, ks, ys = ex(new["_xyz"]), ex(old["_xyz"]), es(new["_scaling"]), es(old["_scaling"])
    print(f"{case}: S={S} xyz kernel {kx:.3e} old route {yx:.3e}; scaling kernel {ks:.3e} old route {ys:.3e}; bit-equal rows xyz "
          f"{int((new['_xyz'][n_old:] == old['_xyz'][n_old:]).all(dim=1).sum())}/{2 * S} scaling "
          f"{int((new['_scaling'][n_old:] == old['_scaling'][n_old:]).all(dim=1).sum())}/{2 * S}")
    assert yx < 1e-5 and ys < 1e-5                                      # (the yardstick itself is the formulas: z is the draw)
    assert kx <= 2 * yx and ks <= 2 * ys, (kx, yx, ks, ys)


def test_a_threshold_of_zero_keeps_the_op_by_op_round_on_the_gpu(monkeypatch):
    scene, g, trainer, gen = _model_state()
    monkeypatch.setattr(GaussianModel, "FUSED_DENSIFY", True)
    calls = []
    real = ops.BACKEND.densify_round
    monkeypatch.setattr(ops.BACKEND, "densify_round", staticmethod(lambda *a, **k: calls.append(1) or real(*a, **k)))
    clone_calls = []
    real_clone = g.densify_and_clone
    g.densify_and_clone = lambda *a, **k: clone_calls.append(1) or real_clone(*a, **k)
    n0 = g.get_xyz.shape[0]
    g.densify(0.0, 0.005, scene.cameras_extent, 20, 5, 5)
    assert calls == [] and clone_calls == [1]
    g.densify(0.0002, 0.005, scene.cameras_extent, 20, 5, 5)
    assert calls == [1] and clone_calls == [1] and g.get_xyz.shape[0] >= n0


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_raise_and_leave_every_tensor_alone():
    """CPU tensors, a float mask, a wrong row count and a non-contiguous source are refused before the plan is launched; what only
    the counts can show (rows are split and there is nothing to make children of, a z of another length) after it and before
    the apply.  No tensor is written either way."""
    P = 100
    gen = torch.Generator().manual_seed(2)
    t = {"xyz": torch.randn(P, 3, generator=gen).cuda(), "scaling": torch.randn(P, 3, generator=gen).cuda(),
         "rotation": torch.randn(P, 4, generator=gen).cuda(), "copy": [torch.randn(P, 5, generator=gen).cuda()],
         "moment": [torch.randn(P, 3, generator=gen).cuda()], "zero": [torch.ones(P, 1).cuda()]}
    clone, split = (torch.arange(P) % 4 == 0).cuda(), (torch.arange(P) % 4 == 1).cuda()
    keep = {k: [x.clone() for x in v] if isinstance(v, list) else v.clone() for k, v in t.items()}
    with pytest.raises(N.MomError):
        ops.densify_round(clone.cpu(), split.cpu(), t)
    with pytest.raises(N.MomError):
        ops.densify_round(clone, split, dict(t, copy=[t["copy"][0].cpu()]))
    with pytest.raises(N.MomError):
        ops.densify_round(clone.float(), split, t)
    with pytest.raises(N.MomError):
        ops.densify_round(clone, split[:50], t)
    with pytest.raises(N.MomError):
        ops.densify_round(clone, split, dict(t, copy=[t["copy"][0][:50]]))
    with pytest.raises(N.MomError):
        ops.densify_round(clone, split, dict(t, moment=[torch.randn(3, P).cuda().t()]))       # not contiguous
    with pytest.raises(N.MomError):
        ops.densify_round(clone, split, dict(t, xyz=t["rotation"]))
    with pytest.raises(N.MomError):
        ops.densify_round(clone, split, dict(t, copy=[t["copy"][0]] * 40))
    with pytest.raises(N.MomError):
        ops.densify_round(clone, split, {"copy": t["copy"]})                                 # rows split, nothing to make children of
    with pytest.raises(N.MomError):
        ops.densify_round(clone, split, t, z=torch.randn(7, 3).cuda())
    for k, v in t.items():                                                                   # nothing was written
        for a, b in zip(v if isinstance(v, list) else [v], keep[k] if isinstance(v, list) else [keep[k]]):
            assert torch.equal(a, b), k
    S = int(split.sum())
    z = torch.randn(2 * S, 3, generator=gen)
    out = ops.densify_round(clone, split, t, z=z.cuda())                                     # a following valid round is unharmed
    cpu = {k: [x.cpu() for x in v] if isinstance(v, list) else v.cpu() for k, v in t.items()}
    want = expected_layout((clone.cpu(), split.cpu()), cpu, z)
    n_old = P - S + int(clone.sum())
    for key in ("copy", "moment", "zero"):
        assert torch.equal(out[key][0].cpu(), want[key][0]), key
    assert torch.equal(out["xyz"][:n_old].cpu(), want["xyz"][:n_old])
    assert torch.allclose(out["xyz"].cpu(), want["xyz"], rtol=1e-4, atol=1e-5)
