"""The deformation MLP of a 32-feature trunk (csrc/deform_mlp.hip at KT = 1; dnerf/eulerian_150_16: two HexPlane levels of 16 channels,
net_width 64, defor_depth 0) beside the 64-feature f32 kernels (the same templates at KT = 2, MOM_MLP_BWD=split) and beside the nn.Linear
sequence Deformation.forward_dynamic ran for this model before the 32-feature kernels existed, on the same tensors: 200 000
Gaussians, forward alone and forward + backward.

Two instruments, both HIP event pairs on the launch stream:
  *_kernels   the event pairs of csrc/profile.hip around the C entry points (slots mlp_fwd and mlp_bwd), summed over a window's
              launches; forward + backward is the sum of the two slots.  An event pair also spans the launch's own dispatch.
  *_autograd  one torch.cuda.Event pair around the whole call as Deformation.forward_dynamic makes it -- ops.deform_mlp, or the
              nn.Linear modules, plus torch.autograd.backward on given output gradients -- so it holds every kernel of the sequence,
              the gaps between them and, where the host cannot keep ahead of the GPU, the host.  This is the pair of figures the
              routing in scene/deformation.py is decided on: the slowest window of the new form against the fastest of nn.Linear.
The forms take turns, window by window, in one process; the record holds each form's median, lowest and highest window.

    python tools/mlp32_time.py [--windows 9] [--launches 40] [--out profiles/mlp32_time.json]
"""
import argparse
import ctypes as C
import importlib
import json
import os
import statistics
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=200_000)
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--launches", type=int, default=40)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import torch.nn as nn
    N = importlib.import_module("iclr2025_3d-mom_amd._native")
    ops = importlib.import_module("iclr2025_3d-mom_amd.ops")
    lib = N.lib()
    slots = {lib.mom_profile_name(k).decode(): k for k in range(32) if lib.mom_profile_name(k)}
    s_fwd, s_bwd = slots["mlp_fwd"], slots["mlp_bwd"]
    P = a.points
    g = torch.Generator().manual_seed(0)
    mk = lambda *s: (torch.randn(*s, generator=g) * 0.3).cuda()
    xyz, scal, rot, flow = mk(P, 3), mk(P, 3), mk(P, 4), mk(P, 3)
    dpts, dsc, drot = mk(P, 3), mk(P, 3), mk(P, 4)
    stream = N.current_stream()
    scratch = torch.empty(lib.mom_deform_backward_scratch_bytes(P), dtype=torch.uint8, device="cuda")
    forms, keep = {}, []

    for n_in in (32, 64):
        params = [mk(64, n_in), mk(64)]
        for nout in (3, 3, 4):
            params += [mk(64, 64), mk(64), mk(nout, 64), mk(nout)]
        feat = mk(P, n_in) * 3
        grads = [torch.zeros_like(p) for p in params]
        d = ops.DeformMLPFunction._desc(params, grads)
        pts, sc_d, rot_d, a0 = (torch.empty(P, k, device="cuda") for k in (3, 3, 4, 64))
        dfeat = torch.empty(P, n_in, device="cuda")
        keep += [params, grads, feat, pts, sc_d, rot_d, a0, dfeat]

        def fwd(d=d, n_in=n_in, feat=feat, pts=pts, sc_d=sc_d, rot_d=rot_d, a0=a0):
            N.check(lib.mom_deform_forward_n(C.byref(d), P, n_in, feat.data_ptr(), xyz.data_ptr(), scal.data_ptr(), rot.data_ptr(),
                                             flow.data_ptr(), 0.7, pts.data_ptr(), sc_d.data_ptr(), rot_d.data_ptr(), a0.data_ptr(),
                                             stream), "fwd")

        def fwd_bwd(fwd=fwd, d=d, n_in=n_in, feat=feat, a0=a0, dfeat=dfeat):
            fwd()
            N.check(lib.mom_deform_backward_n(C.byref(d), P, n_in, feat.data_ptr(), a0.data_ptr(), dpts.data_ptr(), dsc.data_ptr(),
                                              drot.data_ptr(), dfeat.data_ptr(), scratch.data_ptr(), stream), "bwd")

        forms[f"forward_{n_in}_kernels"] = ("slots", fwd, (s_fwd,))
        forms[f"forward_backward_{n_in}_kernels"] = ("slots", fwd_bwd, (s_fwd, s_bwd))

        if n_in == 32:
            # the modules of Deformation.create_net for this model, holding the same numbers as `params`
            head = lambda out: nn.Sequential(nn.ReLU(), nn.Linear(64, 64), nn.ReLU(), nn.Linear(64, out))
            trunk, heads = nn.Sequential(nn.Linear(32, 64)).cuda(), [head(3).cuda(), head(3).cuda(), head(4).cuda()]
            with torch.no_grad():
                trunk[0].weight.copy_(params[0]); trunk[0].bias.copy_(params[1])
                for k, h in enumerate(heads):
                    W1, b1, W2, b2 = params[2 + 4 * k:6 + 4 * k]
                    h[1].weight.copy_(W1); h[1].bias.copy_(b1); h[3].weight.copy_(W2); h[3].bias.copy_(b2)
            mods = [p for m in [trunk] + heads for p in m.parameters()]
            leaves = [t.clone().requires_grad_(True) for t in (feat, xyz, scal, rot)]
            pl = [p.clone().requires_grad_(True) for p in params]
            keep += [trunk, heads, leaves, pl]

            def linear(frame_num=7, delta_scale=0.1):
                # Deformation.forward_dynamic's op-by-op branch (no mask: static_mlp is off)
                hidden = trunk(leaves[0])
                dx = heads[0](hidden) + delta_scale * (frame_num * flow)
                return leaves[1] + dx, leaves[2] + heads[1](hidden), leaves[3] + heads[2](hidden)

            def fused():
                return ops.deform_mlp(leaves[0], leaves[1], leaves[2], leaves[3], flow, 0.7, pl)

            def with_backward(fn, ps):
                def run():
                    for t in leaves + ps:
                        t.grad = None
                    torch.autograd.backward(list(fn()), [dpts, dsc, drot])
                return run

            def no_grad(fn):
                def run():
                    with torch.no_grad():
                        fn()
                return run

            forms["forward_32_linear_autograd"] = ("events", no_grad(linear), None)
            forms["forward_backward_32_linear_autograd"] = ("events", with_backward(linear, mods), None)
            forms["forward_32_fused_autograd"] = ("events", no_grad(fused), None)
            forms["forward_backward_32_fused_autograd"] = ("events", with_backward(fused, pl), None)

    def window(kind, fn, which):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        if kind == "slots":
            for s in which:
                N.check(lib.mom_profile_enable(s, 1), "profile")
            for _ in range(a.launches):
                fn()
            torch.cuda.synchronize()
            total = 0.0
            for s in which:
                ms, cnt = C.c_double(), C.c_longlong()
                N.check(lib.mom_profile_read(s, C.byref(ms), C.byref(cnt), 1), "profile")
                N.check(lib.mom_profile_enable(s, 0), "profile")
                assert int(cnt.value) == a.launches, (int(cnt.value), a.launches)
                total += ms.value
            return total * 1e3 / a.launches
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.launches)]
        for e0, e1 in ev:
            e0.record()
            fn()
            e1.record()
        torch.cuda.synchronize()
        return sum(e0.elapsed_time(e1) for e0, e1 in ev) * 1e3 / a.launches

    os.environ["MOM_MLP_BWD"] = "split"                 # the 64-feature f32 form (read per call; the 32-feature call has no other)
    for name, (kind, fn, which) in forms.items():       # every form warmed up before the first timed window
        window(kind, fn, which)
    times = {name: [] for name in forms}
    for _ in range(a.windows):
        for name, (kind, fn, which) in forms.items():
            times[name].append(window(kind, fn, which))
    out = {"library": lib.mom_version().decode(), "device": torch.cuda.get_device_name(0), "points": P, "windows": a.windows,
           "launches_per_window": a.launches,
           "what": "time per call, us: median window, lowest and highest window; *_kernels = event pairs of csrc/profile.hip "
                   "(slots mlp_fwd [+ mlp_bwd]), *_autograd = one event pair around the call made through torch autograd"}
    for name, v in times.items():
        out[name] = {"median_us": round(statistics.median(v), 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2)}
    new, old = out["forward_backward_32_fused_autograd"], out["forward_backward_32_linear_autograd"]
    out["routing"] = {"criterion": "slowest window of forward_backward_32_fused_autograd < fastest window of "
                                   "forward_backward_32_linear_autograd",
                      "slowest_new_over_fastest_old": round(new["max_us"] / old["min_us"], 4),
                      "new_wins_every_window": new["max_us"] < old["min_us"]}
    txt = json.dumps(out, indent=1)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(txt + "\n")
    print(txt)


if __name__ == "__main__":
    main()
