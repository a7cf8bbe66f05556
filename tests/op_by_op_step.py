"""One fine-stage training iteration on the autograd path (render() + loss.backward() + optimizer.step(), Trainer(fused=False))
of a model the fused steps do not take, on the HIP backend or on the CPU oracle backend, and the comparison of the two under the
gates of tests/test_whole_step_gpu.py::_against_the_oracle at its "tiny" size.  Shared by tests/test_hexplane16_gpu.py (the
eulerian_150_16 shape) and tests/test_model_shapes_gpu.py (the dynerf, hypernerf and bare-default shapes)."""
import contextlib
import importlib

import numpy as np
import torch

pkg = "iclr2025_3d-mom_amd"
DEAD_GROUPS = ("timenet", "opacity_deform", "shs_deform")


def tiny_scene_model(device, **settings):
    """The tiny scene of tests/test_whole_step_gpu.py (CFG), made trained-like, under a model built from `settings` (overrides
    of arguments.default_args) -> scene, gaussians, op, pp, hp."""
    from test_whole_step_gpu import CFG
    A = importlib.import_module(pkg + ".arguments")
    S = importlib.import_module(pkg + ".scene")
    args, lp, op, pp, hp = A.default_args(**settings)
    op.lambda_dssim = 0.0
    torch.manual_seed(6666)
    scene = S.SyntheticScene(CFG["P"], CFG["F"], CFG["W"], CFG["H"], seed=6666)
    g = S.GaussianModel(lp.sh_degree, hp, device=device)
    scene.init_gaussians(g)
    scene.make_trained_like(g)
    return scene, g, op, pp, hp


class _Raster64(torch.autograd.Function):
    """The float64 build of the CPU rasterizer oracle (oracle/raster_oracle.c with -DORACLE_FP64) as an autograd node."""

    @staticmethod
    def forward(ctx, means3D, scales, rotations, opacity, shs, cam):
        from oracle import raster_oracle as ro
        n = lambda t: t.detach().numpy()
        ctx.st = ro.forward(n(means3D), n(opacity), cam["view"], cam["proj"], cam["campos"], cam["W"], cam["H"], cam["tanfovx"],
                            cam["tanfovy"], cam["bg"], shs=n(shs), sh_degree=cam["degree"], scales=n(scales), rotations=n(rotations),
                            scale_modifier=cam["scale_modifier"], fp64=True)
        return torch.from_numpy(ctx.st.out_color.copy())

    @staticmethod
    def backward(ctx, dimg):
        from oracle import raster_oracle as ro
        g = ro.backward(ctx.st, dimg.contiguous().numpy())
        f = torch.from_numpy
        return f(g["dL_dmeans3D"]), f(g["dL_dscales"]), f(g["dL_drotations"]), f(g["dL_dopacity"]), f(g["dL_dsh"]), None


class _Float64Twin:
    """The render loss of a CPU oracle iteration evaluated again in float64 from the same parameters (copied before the step
    changes them) on the same cameras: the deformation network as .double(), the activations, the float64 build of the
    rasterizer oracle, the L1 loss -> d loss / d parameter without float32 rounding.  The distance of the float32 oracle's
    Where the float32 oracle's own arithmetic is the far side (a large, long splat: assert_tiny_gates, `float64_for`), this is the
    gradient HIP is held to."""
    GAUSSIAN = {"xyz": "_xyz", "scaling": "_scaling", "rotation": "_rotation", "opacity": "_opacity", "f_dc": "_features_dc",
                "f_rest": "_features_rest"}

    def __init__(self, g, cams, rc):
        import copy
        self.net = copy.deepcopy(g._deformation).double()
        self.leaves = {k: getattr(g, a).detach().double().clone().requires_grad_(True) for k, a in self.GAUSSIAN.items()}
        self.flow, self.degree = g.get_flow.detach().double().clone(), int(g.active_sh_degree)
        self.gts = [c.device_tensors(torch.device("cpu"))[3][:3].double() for c in cams]
        self.calls, self.cams, self.rc, self.rasterize = [], [], rc, rc.rasterize_gaussians
        self.handle = g._deformation.register_forward_hook(self._seen)
        rc.rasterize_gaussians = self._rasterize

    def _seen(self, module, args, outs):
        rec = {"args": args, "grads": [None] * len(outs)}           # (time, frame_num, delta_scale are read from the call)
        for i, o in enumerate(outs):
            if o.requires_grad:
                o.register_hook(lambda gr, i=i: rec["grads"].__setitem__(i, True))
        self.calls.append(rec)

    def _rasterize(self, bg, means3D, colors, opacity, scales, rotations, scale_modifier, cov3D_precomp, viewmatrix, projmatrix,
                   tan_fovx, tan_fovy, image_height, image_width, sh, degree, campos, prefiltered, debug):
        d = lambda t: t.detach().double().numpy().copy()
        self.cams.append(dict(view=d(viewmatrix), proj=d(projmatrix), campos=d(campos), W=int(image_width), H=int(image_height),
                              tanfovx=float(tan_fovx), tanfovy=float(tan_fovy), bg=d(bg), degree=int(degree),
                              scale_modifier=float(scale_modifier)))
        return self.rasterize(bg, means3D, colors, opacity, scales, rotations, scale_modifier, cov3D_precomp, viewmatrix, projmatrix,
                              tan_fovx, tan_fovy, image_height, image_width, sh, degree, campos, prefiltered, debug)

    def release(self):
        self.handle.remove()
        self.rc.rasterize_gaussians = self.rasterize

    def _named(self, tensors, by_param):
        """{test's name: float64 gradient} for the tensors the twin has (the planes also take the regularisers' gradient, which
        is outside the render loss: they are left out)."""
        out = {}
        grads = dict(self.net.named_parameters())
        for k, p in tensors.items():
            if k in self.leaves:
                out[k] = self.leaves[k].grad
            elif id(p) in by_param and ".grid." not in by_param[id(p)]:
                out[k] = grads[by_param[id(p)]].grad
        return {k: v.float().numpy() for k, v in out.items() if v is not None}

    def gradients(self, tensors, by_param):
        calls = [r for r in self.calls if any(g is not None for g in r["grads"])]          # (the no-grad renders leave none)
        assert len(calls) == len(self.gts) == len(self.cams[-len(calls):])
        L = self.leaves
        images = []
        for rec, cam in zip(calls, self.cams[-len(calls):]):
            time, frame_num, delta_scale = rec["args"][5], rec["args"][7], rec["args"][8]
            outs = self.net(L["xyz"], L["scaling"], L["rotation"], L["opacity"], torch.cat((L["f_dc"], L["f_rest"]), 1), time,
                            self.flow, frame_num, delta_scale)
            images.append(_Raster64.apply(outs[0], torch.exp(outs[1]), torch.nn.functional.normalize(outs[2]),
                                          torch.sigmoid(outs[3]), outs[4], cam))
        (torch.stack(images) - torch.stack(self.gts)).abs().mean().backward()
        return self._named(tensors, by_param)


def one_step(device, make_model, cam_indices=(1,), extra_tensors=None, before_step=None, after_step=None, float64_twin=False):
    """make_model(device) -> scene, gaussians, op, pp, hp.  One iteration (number 5001) on the cameras trainer.cams[i], i in
    cam_indices.  Returns loss, {name: gradient} for test_whole_step_gpu.LIVE and for extra_tensors(gaussians) (Adam's first
    moment after ONE step is 0.1 * gradient exactly), the statistics, per camera (no-grad image, gradient-mode image) rendered
    before the step (HIP only), and which of DEAD_GROUPS received a gradient.  before_step(trainer, gaussians, op, hp): run
    after the renders, after_step the same after the step (HIP only).  float64_twin (CPU oracle only): a sixth result,
    {name: gradient} from _Float64Twin."""
    from oracle import cpu_backend
    from test_whole_step_gpu import LIVE, _tensors
    T = importlib.import_module(pkg + ".train")
    with (cpu_backend.installed() if device == "cpu" else contextlib.nullcontext()):
        scene, g, op, pp, hp = make_model(torch.device(device))
        trainer = T.Trainer(scene, g, op, hp, pp, stage="fine", delta_scale=1, sync_every_step=False, fused=False)
        assert trainer.fused is None
        cams = [trainer.cams[i] for i in cam_indices]
        images = None
        if device != "cpu":
            render = importlib.import_module(pkg + ".gaussian_renderer").render
            images = []
            for cam in cams:
                with torch.no_grad():
                    img_ng = render(cam, g, pp, trainer.background, stage="fine", delta_scale=1)["render"].clone()
                img_g = render(cam, g, pp, trainer.background, stage="fine", delta_scale=1)["render"].detach().clone()
                images.append((img_ng, img_g))
            if before_step is not None:
                before_step(trainer, g, op, hp)
        twin = None
        if float64_twin:
            twin = _Float64Twin(g, cams, importlib.import_module(pkg + ".diff_gaussian_rasterization._C"))
        loss = float(trainer.step(5001, cams=cams))
        if device != "cpu":
            trainer.drain()
            torch.cuda.synchronize()
            if after_step is not None:
                after_step(trainer, g, op, hp)
        t = {k: v for k, v in _tensors(g).items() if k in LIVE}
        if extra_tensors is not None:
            t.update(extra_tensors(g))
        missing = [k for k, p in t.items() if "exp_avg" not in g.optimizer.state.get(p, {})]
        assert not missing, ("no gradient reached these tensors", missing)
        grads = {k: (g.optimizer.state[p]["exp_avg"].detach().float().cpu().numpy() * 10.0) for k, p in t.items()}
        stats = {"accum": g.xyz_gradient_accum.detach().cpu().numpy().copy(), "denom": g.denom.detach().cpu().numpy().copy(),
                 "maxr": g.max_radii2D.detach().cpu().numpy().copy()}
        received = {grp: any(grp in n and p in g.optimizer.state and "exp_avg" in g.optimizer.state[p]
                             and float(g.optimizer.state[p]["exp_avg"].abs().sum()) != 0
                             for n, p in g._deformation.named_parameters()) for grp in DEAD_GROUPS}
        if twin is not None:
            twin.release()
            by_param = {id(p): n for n, p in g._deformation.named_parameters()}
            return loss, grads, stats, images, received, twin.gradients(t, by_param)
    return loss, grads, stats, images, received


def assert_tiny_gates(ref, got, float64_for=()):
    """ref, got: the results of one_step on the CPU oracle and on HIP.  Loss 2e-6, visibility counts and radii exact, per
    gradient tensor at most 1e-3 of the elements beyond 1e-4 of the tensor's scale and none beyond 2e-3, the accumulated
    screen-space gradient norm likewise; every compared gradient nonzero in the reference.  Prints the three figures per tensor.
    float64_for: names of tensors for which the 1e-4 level is asserted against the float64 evaluation of the same iteration (ref
    from one_step(float64_twin=True); _Float64Twin) instead of the float32 oracle's gradient; against the float32 oracle they keep
    "none beyond 2e-3", and its figures are printed."""
    (ref_loss, ref_g, ref_s), (loss, grads, stats) = ref[:3], got[:3]
    assert abs(loss - ref_loss) <= 2e-6 * max(1.0, abs(ref_loss)), (loss, ref_loss)
    np.testing.assert_array_equal(stats["denom"], ref_s["denom"])
    dr = np.abs(stats["maxr"] - ref_s["maxr"])
    assert int((dr != 0).sum()) == 0, (int((dr != 0).sum()), float(dr.max()))
    assert sorted(grads) == sorted(ref_g)
    twin = ref[5] if len(ref) > 5 else {}
    figures = {}
    for k in ref_g:
        a, b = grads[k], ref_g[k]
        assert a.shape == b.shape, k
        assert float(np.abs(b).max()) > 0, (k, "the reference's gradient is zero")
        scale = max(float(np.abs(b).max()), 1e-30)
        err = np.abs(a - b) / scale
        figures[k] = (float((err > 1e-4).mean()), int((err > 2e-3).sum()), float(err.max()))
        print(k, "fraction beyond 1e-4: %.2e, elements beyond 2e-3: %d, max %.2e" % figures[k])
        if k in float64_for:
            e64 = np.abs(a - twin[k]) / scale
            f64 = (float((e64 > 1e-4).mean()), int((e64 > 2e-3).sum()), float(e64.max()))
            print(k, "against float64: fraction beyond 1e-4: %.2e, elements beyond 2e-3: %d, max %.2e" % f64,
                  "(float32 oracle to float64: max %.2e)" % (float(np.abs(b - twin[k]).max()) / scale))
            assert f64[0] <= 1e-3 and f64[1] == 0, (k, "against float64", f64)
            figures[k] = (0.0,) + figures[k][1:]                     # the float32 oracle keeps "none beyond 2e-3" below
    for k, (frac_loose, n_far, worst) in figures.items():
        assert frac_loose <= 1e-3 and n_far == 0 and worst <= 5e-3, (k, frac_loose, n_far, worst)
    acc_scale = max(float(np.abs(ref_s["accum"]).max()), 1e-30)
    e = np.abs(stats["accum"] - ref_s["accum"]) / acc_scale
    print("accum fraction beyond 1e-4: %.2e, max %.2e" % (float((e > 1e-4).mean()), float(e.max())))
    assert float((e > 1e-4).mean()) <= 1e-3 and float(e.max()) <= 2e-3, float(e.max())
    return figures
