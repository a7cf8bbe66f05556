"""GPU parity of the non-rasterizer HIP ops (HexPlane fwd/bwd, fused Adam, L1+PSNR, plane regularisers, distCUDA2)
against the oracle (oracle/torch_ref.py = the reference's torch-op sequence on the CPU; oracle/raster_oracle.c knn)."""
import importlib

import numpy as np
import pytest
import torch

import deform_mlp_cases
from oracle import raster_oracle as ro
from oracle import torch_ref as tr

pytestmark = pytest.mark.gpu

ops = importlib.import_module("iclr2025_3d-mom_amd.ops")
HexPlaneField = importlib.import_module("iclr2025_3d-mom_amd.scene.hexplane").HexPlaneField


def _field(res=(8, 8, 8, 5), multires=(1, 2), seed=0):
    torch.manual_seed(seed)
    cfg = {'grid_dimensions': 2, 'input_coordinate_dim': 4, 'output_coordinate_dim': 32, 'resolution': list(res)}
    f = HexPlaneField(1.6, cfg, list(multires))
    f.set_aabb([1.0, 1.2, 1.4], [-1.0, -1.2, -1.4])
    with torch.no_grad():
        for g in f.grids:
            for p in g:
                p.add_(torch.randn_like(p) * 0.2)
    return f


def _points(n, seed=1):
    g = torch.Generator().manual_seed(seed)
    pts = (torch.rand(n, 3, generator=g) * 2 - 1) * torch.tensor([1.1, 1.3, 1.5])   # some outside the box
    pts[0] = torch.tensor([1.0, 1.2, 1.4])      # exact corners (this symmetric box cannot see a wrong border clip: tests/test_hexplane_box_gpu.py)
    pts[1] = torch.tensor([-1.0, -1.2, -1.4])
    return pts


@pytest.mark.parametrize("res,multires,t", [((8, 8, 8, 5), (1, 2), 0.3), ((64, 64, 64, 50), (1, 2), 0.77),
                                             ((16, 12, 10, 7), (1, 2, 4), 0.0), ((8, 8, 8, 5), (1,), 1.0)])
def test_hexplane_forward_backward_parity(res, multires, t):
    f = _field(res, multires)
    pts = _points(257)
    w = torch.randn(257, f.feat_dim, generator=torch.Generator().manual_seed(3))
    # oracle on the CPU
    p_cpu = pts.clone().requires_grad_(True)
    planes_cpu = [[p.detach().clone().contiguous().requires_grad_(True) for p in g] for g in f.grids]
    feat_ref = tr.hexplane_features(p_cpu, t, f.aabb.detach(), planes_cpu)
    (feat_ref * w).sum().backward()
    # HIP
    fg = f.cuda()
    p_gpu = pts.cuda().requires_grad_(True)
    feat = fg(p_gpu, t)
    (feat * w.cuda()).sum().backward()
    torch.cuda.synchronize()
    np.testing.assert_allclose(feat.detach().cpu().numpy(), feat_ref.detach().numpy(), rtol=2e-5, atol=5e-6)
    def close(a, b):   # sums of signed terms: tolerance relative to the tensor's scale
        np.testing.assert_allclose(a, b, rtol=2e-4, atol=2e-5 * max(1.0, float(np.abs(b).max())))
    close(p_gpu.grad.cpu().numpy(), p_cpu.grad.numpy())
    for gl, gc in zip(fg.grids, planes_cpu):
        for a, b in zip(gl, gc):
            assert a.grad.shape == b.grad.shape
            close(a.grad.cpu().numpy(), b.grad.numpy())
    # the aggregated backward walks a Morton order; with the order disabled (identity) results agree to rounding
    fg.zero_grad()
    fg._order, fg._order_age = torch.arange(257, dtype=torch.int32, device="cuda"), -10**9
    p2 = pts.cuda().requires_grad_(True)
    (fg(p2, t) * w.cuda()).sum().backward()
    close(p2.grad.cpu().numpy(), p_cpu.grad.numpy())
    for gl, gc in zip(fg.grids, planes_cpu):
        for a, b in zip(gl, gc):
            close(a.grad.cpu().numpy(), b.grad.numpy())
    # per-point timestamps (the form the reference passes) give the same result as the scalar
    fg.zero_grad()
    p3 = pts.cuda().requires_grad_(True)
    feat2 = fg(p3, torch.full((257, 1), t, device="cuda"))
    np.testing.assert_array_equal(feat2.detach().cpu().numpy(), feat.detach().cpu().numpy())
    (feat2 * w.cuda()).sum().backward()        # generic (non-aggregated) backward kernel
    close(p3.grad.cpu().numpy(), p_cpu.grad.numpy())
    for gl, gc in zip(fg.grids, planes_cpu):
        for a, b in zip(gl, gc):
            close(a.grad.cpu().numpy(), b.grad.numpy())


def test_fused_adam_matches_torch_adam_incl_tiny_eps():
    torch.manual_seed(0)
    shapes = [(1000, 3), (1000, 1, 3), (1000, 15, 3), (1000, 1), (64, 64), (64,), (7,)]
    ps_ref = [torch.randn(s) for s in shapes]
    plane = ops.make_plane(32, 9, 11)
    plane.copy_(torch.randn(1, 32, 9, 11))
    ps_ref.append(plane.clone())          # keeps the channel-last strides
    ps_hip = [p.clone().cuda() for p in ps_ref]
    assert ps_hip[-1].stride() == ps_ref[-1].stride()
    lrs = [1e-3, 2.5e-3, 1.25e-4, 5e-2, 1.6e-4, 1.6e-4, 0.0, 1.6e-3]
    ref = torch.optim.Adam([{"params": [torch.nn.Parameter(p)], "lr": lr} for p, lr in zip(ps_ref, lrs)], lr=0.0, eps=1e-15)
    hip = ops.FusedAdam([{"params": [torch.nn.Parameter(p)], "lr": lr} for p, lr in zip(ps_hip, lrs)], lr=0.0, eps=1e-15)
    for it in range(3):
        for gr, gh in zip(ref.param_groups, hip.param_groups):
            g = torch.randn_like(gr["params"][0]) * (1e-9 if it == 1 else 1.0)   # tiny grads: eps=1e-15 matters
            if it == 2 and gr["params"][0].shape == (7,):
                continue                                                           # a param without grad is skipped
            gr["params"][0].grad = g.clone()
            # (the device gradients are views at 4-, 8- and 12-byte offsets of a larger buffer in turn -- as the fused step's buckets
            # hand them out when P is odd: the kernel's 16-byte path must step aside for them, tensor by tensor)
            k = (it + gr["params"][0].numel()) % 4
            buf = torch.empty(g.numel() + 4, device="cuda")
            view = buf[k:k + g.numel()].view(g.shape) if g.is_contiguous() else g.clone().cuda()
            view.copy_(g)
            gh["params"][0].grad = view
        ref.step()
        hip.step()
        ref.zero_grad(set_to_none=True)
        hip.zero_grad(set_to_none=True)
    torch.cuda.synchronize()
    for gr, gh in zip(ref.param_groups, hip.param_groups):
        a, b = gh["params"][0].detach().cpu(), gr["params"][0].detach()
        np.testing.assert_allclose(a.numpy(), b.numpy(), rtol=3e-6, atol=1e-7)
        sa, sb = hip.state[gh["params"][0]], ref.state[gr["params"][0]]
        np.testing.assert_allclose(sa["exp_avg"].cpu().numpy(), sb["exp_avg"].numpy(), rtol=2e-6, atol=1e-12)
        np.testing.assert_allclose(sa["exp_avg_sq"].cpu().numpy(), sb["exp_avg_sq"].numpy(), rtol=2e-6, atol=1e-20)
        assert float(sa["step"]) == float(sb["step"])
    # state_dict round trip keeps the torch.optim.Adam layout
    sd = hip.state_dict()
    assert set(sd["state"][0].keys()) == {"step", "exp_avg", "exp_avg_sq"}


def test_l1_and_psnr_sums():
    g = torch.Generator().manual_seed(0)
    img = torch.rand(1, 3, 37, 53, generator=g)
    gt = torch.rand(1, 3, 37, 53, generator=g)
    gt[0, 0, 0, :5] = img[0, 0, 0, :5]      # exact zeros: sign(0) = 0
    a = img.clone().requires_grad_(True)
    loss_ref, sums_ref = tr.l1_loss_with_sums(a, gt)
    loss_ref.backward()
    b = img.cuda().requires_grad_(True)
    loss, sums = ops.l1_loss_with_sums(b, gt.cuda())
    (loss * 1.0).backward()
    torch.cuda.synchronize()
    np.testing.assert_allclose(float(loss), float(loss_ref), rtol=1e-5)
    np.testing.assert_allclose(sums.cpu().numpy(), sums_ref.numpy(), rtol=1e-5)
    np.testing.assert_allclose(b.grad.cpu().numpy(), a.grad.numpy(), rtol=1e-6, atol=0)


def test_plane_regulation_value_and_grads():
    f = _field((8, 8, 8, 5), (1, 2))
    planes_cpu, ws, wl = [], [], []
    for g in f.grids:
        for i, p in enumerate(g):
            planes_cpu.append(p.detach().clone().contiguous().requires_grad_(True))
            ws.append(0.01 if i in (2, 4, 5) else 1e-4)
            wl.append(1e-4 if i in (2, 4, 5) else 0.0)
    val_ref = tr.plane_regulation(planes_cpu, ws, wl)
    (val_ref * 3.0).backward()
    fg = f.cuda()
    planes = [p for g in fg.grids for p in g]
    val = ops.plane_regulation(planes, ws, wl)
    (val * 3.0).backward()
    torch.cuda.synchronize()
    np.testing.assert_allclose(float(val), float(val_ref), rtol=2e-5)
    for a, b in zip(planes, planes_cpu):
        np.testing.assert_allclose(a.grad.cpu().numpy(), b.grad.numpy(), rtol=2e-4, atol=1e-9)


@pytest.mark.parametrize("P", [1, 5, 1024, 1025, 20000])
def test_dist_cuda2_matches_oracle(P):
    knn = importlib.import_module("iclr2025_3d-mom_amd.simple_knn._C")
    rng = np.random.default_rng(P)
    pts = (rng.normal(size=(P, 3)) * [1.0, 2.0, 0.5] + [0.3, -0.2, 3.0]).astype(np.float32)
    got = knn.distCUDA2(torch.from_numpy(pts).cuda()).cpu().numpy()
    exp = ro.knn_mean_dist2(pts)
    np.testing.assert_array_equal(got, exp)      # same float ops in the same order: bit-exact


def test_ops_refuse_cpu_tensors():
    N = importlib.import_module("iclr2025_3d-mom_amd._native")
    with pytest.raises(N.MomError):
        ops.l1_loss_with_sums(torch.zeros(3, 4, 4), torch.zeros(3, 4, 4))
    knn = importlib.import_module("iclr2025_3d-mom_amd.simple_knn._C")
    with pytest.raises(N.MomError):
        knn.distCUDA2(torch.zeros(4, 3))


@pytest.mark.parametrize("P", [1, 31, 64, 65, 1000, 20011])
def test_fused_deform_mlp_forward_backward(P):
    g = torch.Generator().manual_seed(P)
    mk = lambda *s: (torch.randn(*s, generator=g) * 0.3)
    params = [mk(64, 64), mk(64)]
    for nout in (3, 3, 4):
        params += [mk(64, 64), mk(64), mk(nout, 64), mk(nout)]
    feat, xyz, scal, rot, flow = mk(P, 64) * 3, mk(P, 3), mk(P, 3), mk(P, 4), mk(P, 3)
    ws = [mk(P, 3), mk(P, 3), mk(P, 4)]

    def run(dev, fn):
        ps = [p.clone().to(dev).requires_grad_(True) for p in params]
        ins = [t.clone().to(dev).requires_grad_(True) for t in (feat, xyz, scal, rot)]
        o = fn(ins[0], ins[1], ins[2], ins[3], flow.to(dev), 0.7, ps)
        sum((a * w.to(dev)).sum() for a, w in zip(o, ws)).backward()
        return [t.detach().cpu().numpy() for t in o], [t.grad.cpu().numpy() for t in ins], [p.grad.cpu().numpy() for p in ps]

    o_ref, gi_ref, gp_ref = run("cpu", tr.deform_mlp)
    o, gi, gp = run("cuda", ops.deform_mlp)
    for a, b in zip(o, o_ref):
        np.testing.assert_allclose(a, b, rtol=2e-5, atol=2e-5)
    # A hidden unit whose pre-activation is within rounding of 0 may take the other ReLU branch (k-ordered fma chain on the
    # matrix cores vs BLAS on the CPU).  That legitimately changes that one Gaussian's gradient rows, so: per-Gaussian
    # gradients may differ on at most 2 Gaussians, and only on Gaussians the float64 evaluation marks ambiguous for this
    # seed (a pre-activation within the worst-case rounding bound of zero, tests/deform_mlp_cases.py: none at P = 1, so
    # nothing is excused there); parameter gradients are compared in norm (element by element under derived bounds:
    # tests/test_deform_mlp_ref_gpu.py).
    ambiguous = deform_mlp_cases.ambiguous_rows([p.numpy() for p in params], feat.numpy(), bf16=True, margin=1.0, composed=1.0)
    print("ambiguous Gaussians:", int(ambiguous.sum()), "of", P)
    for a, b in zip(gi, gi_ref):
        tol = 2e-4 * np.abs(b) + 2e-5 * max(1.0, float(np.abs(b).max()))
        bad_rows = (np.abs(a - b) > tol).reshape(P, -1).any(1)
        assert not (bad_rows & ~ambiguous).any(), (a.shape, np.flatnonzero(bad_rows & ~ambiguous))
        assert bad_rows.sum() <= 2, (a.shape, int(bad_rows.sum()))
    for a, b in zip(gp, gp_ref):
        rel = np.linalg.norm(a.astype(np.float64) - b) / (np.linalg.norm(b) + 1e-30)
        assert rel <= 2e-3, (a.shape, rel)


def test_morton_order_is_a_permutation_and_matches_oracle_sort():
    rng = np.random.default_rng(0)
    pts = (rng.normal(size=(5000, 3)) * [1.0, 2.0, 0.5] + [0.3, -0.2, 3.0]).astype(np.float32)
    order = ops.morton_order(torch.from_numpy(pts).cuda()).cpu().numpy().astype(np.int64)
    assert np.array_equal(np.sort(order), np.arange(5000))
    # Morton codes as simple_knn.cu:45-61 computes them (bounding box seeded with 0), stable sort
    lo, hi = np.minimum(pts.min(0), 0).astype(np.float32), np.maximum(pts.max(0), 0).astype(np.float32)
    q = (((pts - lo) / (hi - lo)) * np.float32(1023)).astype(np.uint32)

    def prep(x):
        x = (x | (x << 16)) & 0x030000FF
        x = (x | (x << 8)) & 0x0300F00F
        x = (x | (x << 4)) & 0x030C30C3
        x = (x | (x << 2)) & 0x09249249
        return x
    code = prep(q[:, 0]) | (prep(q[:, 1]) << 1) | (prep(q[:, 2]) << 2)
    np.testing.assert_array_equal(order, np.argsort(code, kind="stable"))


# ---------------------------------------------------------------------------------------------- SSIM (survey a13)
def _image_pair(shape, seed):
    g = torch.Generator().manual_seed(seed)
    gt = torch.rand(shape, generator=g)
    img = (gt + 0.15 * torch.randn(shape, generator=g)).clamp(0, 1)
    return img, gt


@pytest.mark.parametrize("shape", [(3, 64, 80), (3, 37, 53), (1, 16, 16), (3, 5, 7), (2, 3, 40, 33)])
def test_ssim_value_and_gradient_match_the_oracle(shape):
    """ops.ssim (one fused HIP kernel per direction) against the reference's five depthwise conv2d on the CPU
    (oracle/torch_ref.ssim, itself pinned by tests/golden/g3_loss.npz).  Ragged sizes exercise the zero padding and the
    partial tiles; the 4-D case the folded batch dimension."""
    img, gt = _image_pair(shape, seed=sum(shape))
    x_ref = img.clone().requires_grad_(True)
    v_ref = tr.ssim(x_ref if x_ref.dim() == 4 else x_ref[None], gt if gt.dim() == 4 else gt[None])
    v_ref.backward()
    x = img.cuda().requires_grad_(True)
    v = ops.ssim(x, gt.cuda())
    (0.2 * (1.0 - v)).backward()                     # the loss term of train_4DGS.py:222-223
    np.testing.assert_allclose(float(v), float(v_ref), rtol=2e-6, atol=1e-7)          # tolerance: fp32 blur order
    g, g_ref = x.grad.cpu().numpy(), (-0.2 * x_ref.grad).numpy()
    assert np.abs(g - g_ref).max() <= 2e-5 * np.abs(g_ref).max() + 1e-9, (np.abs(g - g_ref).max(), np.abs(g_ref).max())


def test_ssim_properties_at_the_benchmark_size():
    """Size-independent properties at 3x540x960: ssim(x, x) = 1 with a vanishing gradient, symmetry of the value, and
    the gradient agrees with a directional finite difference of the HIP forward."""
    img, gt = _image_pair((3, 540, 960), seed=5)
    a, b = img.cuda(), gt.cuda()
    x = a.clone().requires_grad_(True)
    one = ops.ssim(x, a)
    one.backward()
    assert abs(float(one) - 1.0) <= 1e-6
    assert float(x.grad.abs().max()) <= 1e-6
    assert abs(float(ops.ssim(a, b)) - float(ops.ssim(b, a))) <= 1e-6
    x = a.clone().requires_grad_(True)
    ops.ssim(x, b).backward()
    d = torch.randn(a.shape, generator=torch.Generator().manual_seed(9)).cuda()
    eps = 1e-2
    fd = (float(ops.ssim(a + eps * d, b)) - float(ops.ssim(a - eps * d, b))) / (2 * eps)
    an = float((x.grad * d).sum())
    assert abs(fd - an) <= 2e-2 * abs(an) + 1e-6, (fd, an)


def test_loss_utils_ssim_runs_the_hip_kernels_and_refuses_other_windows():
    L = importlib.import_module("iclr2025_3d-mom_amd.utils.loss_utils")
    N = importlib.import_module("iclr2025_3d-mom_amd._native")
    img, gt = _image_pair((3, 48, 48), seed=3)
    v = L.ssim(img.cuda(), gt.cuda())
    np.testing.assert_allclose(float(v), float(tr.ssim(img[None], gt[None])), rtol=2e-6)
    with pytest.raises(N.MomError):
        L.ssim(img.cuda(), gt.cuda(), window_size=7)
    with pytest.raises(N.MomError):
        L.ssim(img, gt)                                  # CPU tensors: no fallback


# ------------------------------------------------------------------------- densification statistics (survey a17)
@pytest.mark.parametrize("P", [1, 257, 20000])
def test_densify_stats_matches_the_mask_indexing_reference(P):
    """ops.densify_stats (one HIP kernel, in place) against the reference's boolean-mask sequence on the CPU
    (oracle/torch_ref.densify_stats = train_4DGS.py:266 + gaussian_model.py:713-715), over several frames so that the
    accumulators carry state; Gaussians a frame did not see (radius 0) must keep their values bit for bit."""
    g = torch.Generator().manual_seed(P)
    max_r, accum, denom = torch.rand(P, generator=g) * 5, torch.rand(P, 1, generator=g), torch.randint(0, 4, (P, 1), generator=g).float()
    ref = [t_.clone() for t_ in (max_r, accum, denom)]
    dev = [t_.cuda() for t_ in (max_r, accum, denom)]
    for frame in range(3):
        radii = (torch.randint(0, 40, (P,), generator=g) * (torch.rand(P, generator=g) > 0.4)).to(torch.int32)
        grad = torch.randn(P, 3, generator=g) * 1e-3
        before = [t_.clone() for t_ in ref]
        tr.densify_stats(radii, grad, *ref)
        ops.densify_stats(radii.cuda(), grad.cuda(), *dev)
        unseen = radii == 0
        for b, r in zip(before, ref):
            assert torch.equal(b.reshape(P)[unseen], r.reshape(P)[unseen])
    for d, r in zip(dev, ref):
        np.testing.assert_allclose(d.cpu().numpy(), r.numpy(), rtol=1e-6, atol=0)       # sqrt(x^2 + y^2): fma vs mul+add
    np.testing.assert_array_equal(dev[0].cpu().numpy(), ref[0].numpy())                 # radii and counts are exact
    np.testing.assert_array_equal(dev[2].cpu().numpy(), ref[2].numpy())
    N = importlib.import_module("iclr2025_3d-mom_amd._native")
    with pytest.raises(N.MomError):
        ops.densify_stats(radii, grad, *ref)                                            # CPU tensors: no fallback
    with pytest.raises(N.MomError):
        ops.densify_stats(radii.cuda().long(), grad.cuda(), *dev)


# ------------------------------------------------------------------------- row selection for densify / prune (survey a17)
@pytest.mark.parametrize("n,p_keep", [(1, 1.0), (7, 0.5), (257, 0.0), (4096, 1.0), (20001, 0.37), (300000, 0.9)])
def test_select_rows_matches_mask_indexing(n, p_keep):
    """ops.select_rows (one scan of the mask, one gather kernel for all tensors) against `tensor[mask]` per tensor, for the
    row shapes and dtypes the optimizer surgery meets: [n,3], [n,1,3], [n,15,3], [n,4], [n,1], [n] floats, a bool table
    (1-byte rows, the byte path) and an int tensor; no row kept, every row kept and ragged sizes."""
    g = torch.Generator().manual_seed(n)
    mask = torch.rand(n, generator=g) < p_keep
    ts = [torch.randn(n, 3, generator=g), torch.randn(n, 1, 3, generator=g), torch.randn(n, 15, 3, generator=g),
          torch.randn(n, 4, generator=g), torch.randn(n, 1, generator=g), torch.randn(n, generator=g),
          torch.rand(n, generator=g) < 0.5, torch.randint(-5, 5, (n, 2), generator=g, dtype=torch.int32)]
    got = ops.select_rows(mask.cuda(), [t_.cuda() for t_ in ts])
    want = tr.select_rows(mask, ts)
    assert len(got) == len(want)
    for a, b in zip(got, want):
        assert a.dtype == b.dtype and tuple(a.shape) == tuple(b.shape)
        assert torch.equal(a.cpu(), b)                       # data movement: exact


def test_select_rows_many_tensors_and_refusals():
    n = 1000
    mask = torch.arange(n) % 3 == 0
    ts = [torch.full((n, 2), float(i)) + torch.arange(n).unsqueeze(1) for i in range(40)]        # more than one launch's worth
    got = ops.select_rows(mask.cuda(), [t_.cuda() for t_ in ts])
    for a, b in zip(got, ts):
        assert torch.equal(a.cpu(), b[mask])
    N = importlib.import_module("iclr2025_3d-mom_amd._native")
    with pytest.raises(N.MomError):
        ops.select_rows(mask, ts)                            # CPU tensors: no fallback
    with pytest.raises(N.MomError):
        ops.select_rows(mask.cuda().float(), [ts[0].cuda()])
    with pytest.raises(N.MomError):
        ops.select_rows(mask.cuda(), [ts[0][:10].cuda()])


def test_densify_and_prune_round_matches_mask_indexing_on_the_gpu():
    """A whole densify + prune round of GaussianModel (clone, split, prune, with the Adam moments) on the GPU: the HIP row
    selection against the reference's per-tensor mask indexing, same seed.  Pure data movement: every tensor must be equal.
    The state before the round is built without training (seeded statistics, one optimizer step on seeded gradients):
    training accumulates with unordered float atomics, so two trained models already differ in their last bits."""
    import bench

    def run(use_hip):
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
        saved = ops.BACKEND.select_rows
        if not use_hip:
            ops.BACKEND.select_rows = staticmethod(tr.select_rows)
        try:
            torch.manual_seed(11)
            torch.cuda.manual_seed(11)
            n0 = g.get_xyz.shape[0]
            g.densify(0.0002, 0.005, scene.cameras_extent, 20, 5, 5, scene.model_path, 5100, "fine")
            n1 = g.get_xyz.shape[0]
            g.max_radii2D = (torch.rand(n1, generator=gen) * 30).cuda()
            g.prune(0.0002, 0.02, scene.cameras_extent, 20)
            n2 = g.get_xyz.shape[0]
        finally:
            ops.BACKEND.select_rows = saved
        out = {"xyz": g._xyz, "f_dc": g._features_dc, "f_rest": g._features_rest, "opacity": g._opacity, "scaling": g._scaling,
               "rotation": g._rotation, "table": g._deformation_table, "flow": g._scene_flow, "maxr": g.max_radii2D,
               "accum": g.xyz_gradient_accum, "denom": g.denom}
        for grp in g.optimizer.param_groups:
            if len(grp["params"]) == 1 and grp["name"] in ("xyz", "f_rest", "opacity"):
                st = g.optimizer.state[grp["params"][0]]
                out["m_" + grp["name"]], out["v_" + grp["name"]] = st["exp_avg"], st["exp_avg_sq"]
        snap = {k: v.detach().cpu().clone() for k, v in out.items()}
        loss = trainer.step(5101, cams=[trainer.cams[0]])      # the model still trains after the surgery
        assert np.isfinite(float(loss))
        return (n0, n1, n2), snap

    (a0, a1, a2), hip = run(True)
    (b0, b1, b2), ref = run(False)
    assert (a0, a1, a2) == (b0, b1, b2) and a1 > a0 and a2 < a1, (a0, a1, a2, b0, b1, b2)
    for k in ref:
        assert torch.equal(hip[k], ref[k]), k


import ctypes as C  # noqa: E402

N = importlib.import_module("iclr2025_3d-mom_amd._native")


def _mlp_state(P, seed):
    g = torch.Generator().manual_seed(seed)
    mk = lambda *s: (torch.randn(*s, generator=g) * 0.3).cuda()
    params = [mk(64, 64), mk(64)]
    for nout in (3, 3, 4):
        params += [mk(64, 64), mk(64), mk(nout, 64), mk(nout)]
    return params, mk


@pytest.mark.parametrize("P", [33, 5000])
def test_deform_forward_activated_equals_forward_plus_activation_kernel(P):
    """mom_deform_forward_activated: the raw outputs are those of mom_deform_forward and the activated ones are, bit for bit,
    what mom_activations_forward makes of them (both go through the same rounding-pinned helpers)."""
    params, mk = _mlp_state(P, 100 + P)
    feat, xyz, scal, rot, flow, opac = mk(P, 64) * 3, mk(P, 3), mk(P, 3), mk(P, 4), mk(P, 3), mk(P, 1)
    d = ops.DeformMLPFunction._desc(params)
    lib, s = N.lib(), N.current_stream()
    e = lambda *sh: torch.full(sh, float("nan"), device="cuda")
    pts, sc_d, rot_d = e(P, 3), e(P, 3), e(P, 4)
    N.check(lib.mom_deform_forward(C.byref(d), P, feat.data_ptr(), xyz.data_ptr(), scal.data_ptr(), rot.data_ptr(), flow.data_ptr(),
                                   0.7, pts.data_ptr(), sc_d.data_ptr(), rot_d.data_ptr(), None, s), "fwd")
    sc, rt, op = e(P, 3), e(P, 4), e(P, 1)
    N.check(lib.mom_activations_forward(P, sc_d.data_ptr(), rot_d.data_ptr(), opac.data_ptr(), sc.data_ptr(), rt.data_ptr(),
                                        op.data_ptr(), s), "act")
    pts2, sc_d2, rot_d2, sc2, rt2, op2 = e(P, 3), e(P, 3), e(P, 4), e(P, 3), e(P, 4), e(P, 1)
    N.check(lib.mom_deform_forward_activated(C.byref(d), P, feat.data_ptr(), xyz.data_ptr(), scal.data_ptr(), rot.data_ptr(),
                                             flow.data_ptr(), 0.7, pts2.data_ptr(), sc_d2.data_ptr(), rot_d2.data_ptr(), None,
                                             opac.data_ptr(), sc2.data_ptr(), rt2.data_ptr(), op2.data_ptr(), s), "fwd_act")
    torch.cuda.synchronize()
    for a, b in ((pts, pts2), (sc_d, sc_d2), (rot_d, rot_d2), (sc, sc2), (rt, rt2), (op, op2)):
        assert torch.isfinite(b).all() and torch.equal(a, b)
    # opacity_act without opacity_raw is refused
    assert lib.mom_deform_forward_activated(C.byref(d), P, feat.data_ptr(), xyz.data_ptr(), scal.data_ptr(), rot.data_ptr(),
                                            flow.data_ptr(), 0.7, pts2.data_ptr(), sc_d2.data_ptr(), rot_d2.data_ptr(), None, None,
                                            None, None, op2.data_ptr(), s) == N.MOM_EINVAL


def test_deform_backward_split_on_a_second_stream_equals_the_single_stream_call():
    P = 7001
    params, mk = _mlp_state(P, 7)
    feat, xyz, scal, rot, flow = mk(P, 64) * 3, mk(P, 3), mk(P, 3), mk(P, 4), mk(P, 3)
    dpts, dsc, drot = mk(P, 3), mk(P, 3), mk(P, 4)
    lib, s = N.lib(), N.current_stream()
    side = torch.cuda.Stream()

    def run(second):
        grads = [torch.zeros_like(p) for p in params]
        d = ops.DeformMLPFunction._desc(params, grads)
        pts, sc_d, rot_d, a0 = (torch.empty(P, k, device="cuda") for k in (3, 3, 4, 64))
        N.check(lib.mom_deform_forward(C.byref(d), P, feat.data_ptr(), xyz.data_ptr(), scal.data_ptr(), rot.data_ptr(),
                                       flow.data_ptr(), 0.7, pts.data_ptr(), sc_d.data_ptr(), rot_d.data_ptr(), a0.data_ptr(), s), "fwd")
        dfeat = torch.empty(P, 64, device="cuda")
        scratch = torch.empty(lib.mom_deform_backward_scratch_bytes(P), dtype=torch.uint8, device="cuda")
        N.check(lib.mom_deform_backward_split(C.byref(d), P, feat.data_ptr(), a0.data_ptr(), dpts.data_ptr(), dsc.data_ptr(),
                                              drot.data_ptr(), dfeat.data_ptr(), scratch.data_ptr(), s,
                                              side.cuda_stream if second else s), "bwd")
        if second:
            torch.cuda.current_stream().wait_stream(side)      # the caller's join
        torch.cuda.synchronize()
        return dfeat, grads

    f1, g1 = run(False)
    f2, g2 = run(True)
    assert torch.equal(f1, f2)
    for a, b in zip(g1, g2):         # float atomics: same terms, possibly another order
        assert float((a - b).abs().max()) <= 1e-5 * max(1.0, float(a.abs().max()))


def test_mlp_backward_forms_by_name_and_an_unknown_name_refused(monkeypatch):
    """MOM_MLP_BWD with a complete descriptor: unset, empty, "b3" and "split" run; "fused" (a form that was removed) and any other
    value return MOM_EINVAL and leave dfeat untouched."""
    P = 1000
    params, mk = _mlp_state(P, 3)
    feat, a0, dpts, dsc, drot = mk(P, 64), mk(P, 64).relu(), mk(P, 3), mk(P, 3), mk(P, 4)
    lib, s = N.lib(), N.current_stream()
    scratch = torch.empty(lib.mom_deform_backward_scratch_bytes(P), dtype=torch.uint8, device="cuda")
    for mode, want in ((None, N.MOM_OK), ("", N.MOM_OK), ("b3", N.MOM_OK), ("split", N.MOM_OK), ("fused", N.MOM_EINVAL), ("f32", N.MOM_EINVAL)):
        if mode is None:
            monkeypatch.delenv("MOM_MLP_BWD", raising=False)
        else:
            monkeypatch.setenv("MOM_MLP_BWD", mode)
        d = ops.DeformMLPFunction._desc(params, [torch.zeros_like(p) for p in params])
        dfeat = torch.full((P, 64), float("nan"), device="cuda")
        rc = lib.mom_deform_backward_split(C.byref(d), P, feat.data_ptr(), a0.data_ptr(), dpts.data_ptr(), dsc.data_ptr(),
                                           drot.data_ptr(), dfeat.data_ptr(), scratch.data_ptr(), s, s)
        torch.cuda.synchronize()
        assert rc == want, (mode, rc)
        assert bool(torch.isfinite(dfeat).all()) == (want == N.MOM_OK), mode


@pytest.mark.parametrize("P", [50021, 4099, 33, 7, 200_000])
def test_deform_backward_one_kernel_bf16_equals_the_two_kernel_f32_backward(P, monkeypatch):
    """The default MLP backward (csrc/deform_bwd_b3.hip: one kernel, role-specialised waves, every product the exact three-way
    bf16 expansion) against the two f32-MFMA kernels (MOM_MLP_BWD=split) and against torch autograd of the reference's layer
    sequence (scene/deformation.py:53-65,97-153): d(features) and every weight and bias gradient -- W0, b0, the three heads' W1,
    b1, W2, b2 -- within 2e-5 of each tensor's scale of the f32 kernels, 1e-4 of autograd (fp32 summation orders); ragged sizes
    (a last tile of 1, 3 and 7 Gaussians) and config 2's size.  Twice in a row: the kernel's LDS hand-over must leave no state.
    (Autograd only up to 5 k Gaussians: a hidden unit whose pre-activation is within rounding of zero takes the other side of the
    ReLU under torch's matmul, which switches that unit's whole contribution on or off -- about one unit in a million.)"""
    params, mk = _mlp_state(P, 11)
    feat, xyz, scal, rot, flow = mk(P, 64) * 3, mk(P, 3), mk(P, 3), mk(P, 4), mk(P, 3)
    dpts, dsc, drot = mk(P, 3), mk(P, 3), mk(P, 4)
    lib, s = N.lib(), N.current_stream()

    def run(mode):
        if mode is None:
            monkeypatch.delenv("MOM_MLP_BWD", raising=False)
        else:
            monkeypatch.setenv("MOM_MLP_BWD", mode)
        grads = [torch.zeros_like(p) for p in params]
        d = ops.DeformMLPFunction._desc(params, grads)
        pts, sc_d, rot_d, a0 = (torch.empty(P, k, device="cuda") for k in (3, 3, 4, 64))
        N.check(lib.mom_deform_forward(C.byref(d), P, feat.data_ptr(), xyz.data_ptr(), scal.data_ptr(), rot.data_ptr(),
                                       flow.data_ptr(), 0.7, pts.data_ptr(), sc_d.data_ptr(), rot_d.data_ptr(), a0.data_ptr(), s), "fwd")
        dfeat = torch.full((P, 64), float("nan"), device="cuda")
        scratch = torch.empty(lib.mom_deform_backward_scratch_bytes(P), dtype=torch.uint8, device="cuda")
        N.check(lib.mom_deform_backward_split(C.byref(d), P, feat.data_ptr(), a0.data_ptr(), dpts.data_ptr(), dsc.data_ptr(),
                                              drot.data_ptr(), dfeat.data_ptr(), scratch.data_ptr(), s, s), "bwd")
        torch.cuda.synchronize()
        return dfeat, grads

    side = torch.cuda.Stream()

    def run_two_streams():
        """As the training step calls it: a second stream for the weight gradients.  The kernel then takes 224 workgroups (the
        rest of the chip is the second stream's) and its partial sums are reduced on that stream; the caller joins before reading."""
        monkeypatch.delenv("MOM_MLP_BWD", raising=False)
        grads = [torch.zeros_like(p) for p in params]
        d = ops.DeformMLPFunction._desc(params, grads)
        pts, sc_d, rot_d, a0 = (torch.empty(P, k, device="cuda") for k in (3, 3, 4, 64))
        N.check(lib.mom_deform_forward(C.byref(d), P, feat.data_ptr(), xyz.data_ptr(), scal.data_ptr(), rot.data_ptr(),
                                       flow.data_ptr(), 0.7, pts.data_ptr(), sc_d.data_ptr(), rot_d.data_ptr(), a0.data_ptr(), s), "fwd")
        dfeat = torch.full((P, 64), float("nan"), device="cuda")
        scratch = torch.empty(lib.mom_deform_backward_scratch_bytes(P), dtype=torch.uint8, device="cuda")
        side.wait_stream(torch.cuda.current_stream())
        N.check(lib.mom_deform_backward_split(C.byref(d), P, feat.data_ptr(), a0.data_ptr(), dpts.data_ptr(), dsc.data_ptr(),
                                              drot.data_ptr(), dfeat.data_ptr(), scratch.data_ptr(), s, side.cuda_stream), "bwd")
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        return dfeat, grads

    f_ref, g_ref = run("split")
    f_one, g_one = run(None)
    f_two, g_two = run_two_streams()
    # the workgroup count changes which tiles a workgroup sums, i.e. the order of the fp32 additions of the weight gradients; dfeat
    # is per Gaussian and must not move at all
    assert torch.equal(f_one, f_two)
    for i, (a, b) in enumerate(zip(g_one, g_two)):
        assert float((a - b).abs().max()) <= 2e-5 * max(1.0, float(a.abs().max())), i
    for rep in range(2):
        f_new, g_new = run(None)
        assert torch.isfinite(f_new).all()
        fs = max(1.0, float(f_ref.abs().max()))
        assert float((f_new - f_ref).abs().max()) <= 2e-5 * fs, (rep, float((f_new - f_ref).abs().max()), fs)
        for i, (a, b) in enumerate(zip(g_ref, g_new)):
            sc = max(1.0, float(a.abs().max()))
            assert float(b.abs().max()) > 0 or float(a.abs().max()) == 0, i
            assert float((a - b).abs().max()) <= 2e-5 * sc, (rep, i, float((a - b).abs().max()), sc)
    if P > 5000:
        return
    # torch autograd of the same layers
    tp = [p.detach().clone().requires_grad_(True) for p in params]
    x = feat.detach().clone().requires_grad_(True)
    a0t = torch.relu(x @ tp[0].t() + tp[1])
    loss = 0
    for k, dout in enumerate((dpts, dsc, drot)):
        W1, b1, W2, b2 = tp[2 + 4 * k: 6 + 4 * k]
        o = torch.relu(a0t @ W1.t() + b1) @ W2.t() + b2
        loss = loss + (o * dout).sum()
    loss.backward()
    assert float((f_new - x.grad).abs().max()) <= 1e-4 * max(1.0, float(x.grad.abs().max()))
    for i, (t_, b) in enumerate(zip(tp, g_new)):
        sc = max(1.0, float(t_.grad.abs().max()))
        assert float((t_.grad - b).abs().max()) <= 1e-4 * sc, (i, float((t_.grad - b).abs().max()), sc)


def test_adam_step_taken_in_two_parts_equals_one_step():
    """FusedAdam.step_partial(some) on a second stream followed by step() (the rest) -- how the fused training step overlaps the
    appearance parameters' update with the deformation backward -- against one step(): bit-identical parameters, moments and
    step counters over several iterations; a parameter is advanced exactly once per iteration."""
    torch.manual_seed(3)
    shapes = [(5000, 3), (5000, 1, 3), (5000, 15, 3), (5000, 4), (1, 32, 64, 64), (64, 64)]
    lrs = [1.6e-4, 2.5e-3, 1.25e-4, 1e-3, 1.6e-3, 1.6e-4]
    init = [torch.randn(*s, device="cuda") for s in shapes]
    grads = [[torch.randn(*s, device="cuda") * 10 ** (-i) for s in shapes] for i in range(3)]

    def run(split):
        ps = [torch.nn.Parameter(p.clone()) for p in init]
        opt = ops.FusedAdam([{"params": [p], "lr": lr} for p, lr in zip(ps, lrs)], lr=0.0, eps=1e-15)
        side = torch.cuda.Stream()
        for gs in grads:
            for p, g in zip(ps, gs):
                p.grad = g.clone()
            if split:
                side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side):
                    opt.step_partial([ps[1], ps[2], ps[3]])
                torch.cuda.current_stream().wait_stream(side)
            opt.step()
            opt.zero_grad(set_to_none=True)
        torch.cuda.synchronize()
        return ps, opt

    pa, oa = run(False)
    pb, ob = run(True)
    for a, b in zip(pa, pb):
        assert torch.equal(a, b)
        sa, sb = oa.state[a], ob.state[b]
        assert float(sa["step"]) == float(sb["step"]) == 3.0
        assert torch.equal(sa["exp_avg"], sb["exp_avg"]) and torch.equal(sa["exp_avg_sq"], sb["exp_avg_sq"])


@pytest.mark.parametrize("res,n,t", [((64, 64, 64, 25), 20011, 0.41), ((16, 12, 10, 7), 1000, 1.0)])
def test_hexplane_backward_gather_in_the_forward_layout_equals_the_lane_per_channel_gather(res, n, t, monkeypatch):
    """hexplane_bwd6_gather (csrc/deform_field.hip: eight lanes per (point, level), the time planes as this frame's lines, both
    levels per wave) against hexplane_bwd5_gather (MOM_HEX_GATHER=5), through the same scatter: plane gradients and position
    gradients agree to the rounding of their different summation orders."""
    f = _field(res, (1, 2)).cuda()
    pts = _points(n)
    w = torch.randn(n, f.feat_dim, generator=torch.Generator().manual_seed(5)).cuda()

    def run(mode):
        monkeypatch.setenv("MOM_HEX_GATHER", mode)
        f.zero_grad()
        p = pts.cuda().requires_grad_(True)
        (f(p, t) * w).sum().backward()
        torch.cuda.synchronize()
        return p.grad.clone(), [[q.grad.clone() for q in g] for g in f.grids]

    g5, p5 = run("5")
    g6, p6 = run("6")
    sc = float(g5.abs().max())
    assert float((g5 - g6).abs().max()) <= 2e-5 * sc
    for la, lb in zip(p5, p6):
        for a, b in zip(la, lb):
            assert float(b.abs().max()) > 0
            assert float((a - b).abs().max()) <= 2e-5 * float(a.abs().max())


def test_hexplane_backward_with_common_factor_rows_equals_the_six_row_form(monkeypatch):
    """The shipped backward: the gather leaves one row per (order slot, position) -- dfeat times the samples of the four planes
    outside the slot -- and the scatter forms the slot's two gv rows itself from the time line's and the space plane's own samples
    (csrc/hexplane.hip, hexplane_bwd5_scatter_kernel<true>).  Same plane and position gradients as the six-row form
    (MOM_HEX_GATHER=5: hexplane_bwd5_gather_kernel + hexplane_bwd5_scatter_kernel<false>), to rounding."""
    f = _field((64, 64, 64, 25), (1, 2)).cuda()
    n, t = 20011, 0.41
    pts = _points(n)
    w = torch.randn(n, f.feat_dim, generator=torch.Generator().manual_seed(6)).cuda()

    def run(mode):
        monkeypatch.setenv("MOM_HEX_GATHER", mode)
        f.zero_grad()
        p = pts.cuda().requires_grad_(True)
        (f(p, t) * w).sum().backward()
        torch.cuda.synchronize()
        return p.grad.clone(), [[q.grad.clone() for q in g] for g in f.grids]

    g0, p0 = run("5")
    g1, p1 = run("6")
    assert float((g0 - g1).abs().max()) <= 2e-5 * float(g0.abs().max())
    for la, lb in zip(p0, p1):
        for a, b in zip(la, lb):
            assert float(b.abs().max()) > 0
            assert float((a - b).abs().max()) <= 2e-5 * float(a.abs().max())


def test_mom_comm_entry_points_on_one_rank_leave_in_place_buffers_as_a_world_of_one_must():
    """include/mom4d.h mom_comm_*: the step's collectives over librccl behind the C ABI (csrc/comm.hip).  A one-GPU box can only
    form a world of one, where every collective is the identity -- which still exercises the whole path the multi-GPU step takes:
    librccl resolved at run time (the copy torch has mapped), communicator from a unique id, in-place all-reduce (sum, max, float
    and int), all-gather, reduce-scatter, a grouped submission, stream ordering through the marks, and parallel.DirectComm on top."""
    import ctypes as C
    par = importlib.import_module("iclr2025_3d-mom_amd.parallel")
    lib = N.lib()
    assert lib.mom_comm_available() == 1, lib.mom_comm_last_error()
    idb = (C.c_char * 128)()
    assert lib.mom_comm_unique_id(idb) == 0
    comm = C.c_void_p()
    assert lib.mom_comm_create(C.byref(comm), idb, 1, 0) == 0, lib.mom_comm_last_error()
    assert lib.mom_comm_world(comm) == 1 and lib.mom_comm_rank(comm) == 0
    s = N.current_stream()
    f = torch.arange(4096, dtype=torch.float32, device="cuda") * 0.5
    i = torch.arange(-100, 924, dtype=torch.int32, device="cuda")
    want_f, want_i = f.clone(), i.clone()
    assert lib.mom_comm_all_reduce(comm, f.data_ptr(), f.numel(), N.COMM_F32, N.COMM_SUM, s) == 0
    assert lib.mom_comm_all_reduce(comm, i.data_ptr(), i.numel(), N.COMM_I32, N.COMM_MAX, s) == 0
    assert lib.mom_comm_all_gather(comm, f.data_ptr(), f.numel(), N.COMM_F32, s) == 0
    assert lib.mom_comm_reduce_scatter(comm, f.data_ptr(), f.numel(), N.COMM_F32, N.COMM_SUM, s) == 0
    assert lib.mom_comm_group_start() == 0
    assert lib.mom_comm_all_reduce(comm, f.data_ptr(), 1024, N.COMM_F32, N.COMM_SUM, s) == 0
    assert lib.mom_comm_all_reduce(comm, i.data_ptr(), i.numel(), N.COMM_I32, N.COMM_MAX, s) == 0
    assert lib.mom_comm_group_end() == 0
    torch.cuda.synchronize()
    assert torch.equal(f, want_f) and torch.equal(i, want_i)
    # bad arguments are refused, not passed on
    assert lib.mom_comm_all_reduce(comm, f.data_ptr(), 16, 7, N.COMM_SUM, s) == N.MOM_EINVAL
    assert lib.mom_comm_all_reduce(None, f.data_ptr(), 16, N.COMM_F32, N.COMM_SUM, s) == N.MOM_EINVAL
    assert lib.mom_comm_create(C.byref(comm), idb, 2, 2) == N.MOM_EINVAL
    assert lib.mom_comm_destroy(comm) == 0
    # the Python layer: DirectComm on its own stream, work handles = stream marks
    dc = par.DirectComm(0, 1, torch.device("cuda", torch.cuda.current_device()))
    g = torch.full((1000,), 3.0, device="cuda")
    w1 = dc.all_reduce(g, "sum")
    with dc.group() as grp:
        dc.reduce_scatter(g, 1000, "sum")
        dc.all_reduce(i, "max")
    dc.wait(w1)
    dc.wait(grp.work)
    h = g * 2                                                      # ordered behind the collectives on the current stream
    torch.cuda.synchronize()
    assert float(h.sum()) == 6000.0 and torch.equal(i, want_i)
    dc.close()
