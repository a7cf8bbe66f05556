"""The deformation field of a 16 x 2 HexPlane model (dnerf/eulerian_150_16) in one launch (csrc/deform_field16.hip) beside the
two calls it stands for (mom_hexplane_forward with channels 16 + mom_deform_forward_activated_n with in_features 32), and what a
no-grad render() of such a model gains from routing to it.

  field      200 000 points, resolution [64, 64, 64, 150], multires [1, 2], Morton order, no saved tensors.  two_calls and one_launch
             leave the same outputs, activated copies included; one_launch_raw is the call fused_render.FusedRender makes for such
             a model: raw outputs only (it activates them with the model's torch functions).  Event pairs of csrc/profile.hip around the C entry points (slots hexplane_fwd and
             mlp_fwd; the one-launch form reports under hexplane_fwd), summed over a window's launches; a pair also spans the launch's
             own dispatch.  The two forms take turns, window by window, in one process.
  render     frames/s of gaussian_renderer.render() under torch.no_grad() over the 59-pose `side` trajectory of a synthetic model
             of that shape (200 000 Gaussians, 960 x 540, async binning capacity): the parent's route (op by op: Deformation.
             _field16_fusable answering False) against the new one (fused_render.FusedRender with the one-launch field), one pass over
             the trajectory per window, taking turns; and the new route on two alternating streams (FusedRenderPool).
The record holds each form's median, lowest and highest window and the routing criterion of DESIGN 3.6 / 3.8: the slowest new
window against the fastest old one.

    python tools/field16_time.py [--windows 9] [--launches 40] [--out profiles/field16_time.json]
"""
import argparse
import ctypes as C
import importlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
pkg = "iclr2025_3d-mom_amd"


def field_times(a, torch, N, ops, lib):
    HexPlaneField = importlib.import_module(pkg + ".scene.hexplane").HexPlaneField
    slots = {lib.mom_profile_name(k).decode(): k for k in range(32) if lib.mom_profile_name(k)}
    s_hex, s_mlp = slots["hexplane_fwd"], slots["mlp_fwd"]
    P, t = a.points, 0.77
    g = torch.Generator().manual_seed(1)
    pts = ((torch.rand(P, 3, generator=g) * 2 - 1) * torch.tensor([1.0, 1.2, 1.4])).cuda()
    mk = lambda *s: (torch.randn(*s, generator=g) * 0.3).cuda()
    scal, rot, flow, opac = mk(P, 3), mk(P, 4), mk(P, 3), mk(P, 1)
    order = ops.morton_order(pts)
    stream = N.current_stream()
    torch.manual_seed(0)
    cfg = {'grid_dimensions': 2, 'input_coordinate_dim': 4, 'output_coordinate_dim': 16, 'resolution': [64, 64, 64, 150]}
    f = HexPlaneField(1.6, cfg, [1, 2])
    f.set_aabb([1.0, 1.2, 1.4], [-1.0, -1.2, -1.4])
    f = f.cuda()
    hp, keep = ops._hexplane_desc([[p.detach() for p in lv] for lv in f.grids], f.aabb, None, aabb_host=f.aabb_host())
    params = [mk(64, 32), mk(64)]
    for nout in (3, 3, 4):
        params += [mk(64, 64), mk(64), mk(nout, 64), mk(nout)]
    md = ops.DeformMLPFunction._desc(params)
    e = lambda *s: torch.empty(*s, device="cuda")
    feat = e(P, 32)
    out = [dict(pts=e(P, 3), sc_d=e(P, 3), rot_d=e(P, 4), sc=e(P, 3), rot=e(P, 4), op=e(P, 1)) for _ in range(2)]
    scratch = torch.empty(lib.mom_deform_field16_scratch_bytes(C.byref(hp), P), dtype=torch.uint8, device="cuda")

    def two_calls(o=out[0]):
        N.check(lib.mom_hexplane_forward(C.byref(hp), P, pts.data_ptr(), None, t, order.data_ptr(), feat.data_ptr(), stream), "hexplane_fwd")
        N.check(lib.mom_deform_forward_activated_n(C.byref(md), P, 32, feat.data_ptr(), pts.data_ptr(), scal.data_ptr(), rot.data_ptr(),
                                                   flow.data_ptr(), 0.7, o["pts"].data_ptr(), o["sc_d"].data_ptr(), o["rot_d"].data_ptr(),
                                                   None, opac.data_ptr(), o["sc"].data_ptr(), o["rot"].data_ptr(), o["op"].data_ptr(),
                                                   stream), "deform_fwd")

    def one_launch(o=out[1]):
        ops.field16_forward(hp, md, P, pts, t, order, scal, rot, flow, 0.7, o["pts"], o["sc_d"], o["rot_d"], None, None, opac, o["sc"],
                            o["rot"], o["op"], stream, scratch=scratch)

    def one_launch_raw(o=out[1]):
        ops.field16_forward(hp, md, P, pts, t, order, scal, rot, flow, 0.7, o["pts"], o["sc_d"], o["rot_d"], None, None, None, None,
                            None, None, stream, scratch=scratch)

    forms = {"two_calls": (two_calls, (s_hex, s_mlp)), "one_launch": (one_launch, (s_hex,)), "one_launch_raw": (one_launch_raw, (s_hex,))}

    def window(fn, which):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
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

    for fn, which in forms.values():                     # both forms warmed up before the first timed window
        window(fn, which)
    two_calls(), one_launch()
    torch.cuda.synchronize()
    same = all(torch.equal(out[0][k], out[1][k]) for k in out[0])
    times = {name: [] for name in forms}
    for _ in range(a.windows):
        for name, (fn, which) in forms.items():
            times[name].append(window(fn, which))
    rec = {name: {"median_us": round(statistics.median(v), 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2)}
           for name, v in times.items()}
    rec["outputs_bit_identical"] = bool(same)
    rec["criterion"] = {"slowest_new_over_fastest_old": round(rec["one_launch"]["max_us"] / rec["two_calls"]["min_us"], 4),
                        "new_wins_every_window": rec["one_launch"]["max_us"] < rec["two_calls"]["min_us"]}
    return rec


def render_rates(a, torch):
    A = importlib.import_module(pkg + ".arguments")
    S = importlib.import_module(pkg + ".scene")
    R = importlib.import_module(pkg + ".gaussian_renderer")
    DGR = importlib.import_module(pkg + ".diff_gaussian_rasterization")
    dev = torch.device("cuda")
    kc = {'grid_dimensions': 2, 'input_coordinate_dim': 4, 'output_coordinate_dim': 16, 'resolution': [64, 64, 64, 150]}
    args, lp, op, pp, hp = A.default_args(kplanes_config=kc, multires=[1, 2])
    torch.manual_seed(6666)
    scene = S.SyntheticScene(a.points, 60, 960, 540, seed=6666)
    g = S.GaussianModel(lp.sh_degree, hp, device=dev)
    scene.init_gaussians(g)
    scene.make_trained_like(g)
    dn = g._deformation.deformation_net
    assert dn._field16_fusable() and not dn._fusable()
    bg = torch.zeros(3, device=dev)
    cams = scene.getVideoCameras_side()
    for c in cams:
        c.device_tensors(dev)
    DGR.set_sync_mode("async")

    def one_pass(route):
        streams = 2 if route == "new_two_streams" else 1
        if route == "old":
            dn._field16_fusable = lambda: False          # the parent's answer: render() goes op by op in both grad modes
        R.set_render_streams(streams)
        try:
            with torch.no_grad():
                for c in cams[:8 * streams]:
                    R.render(c, g, pp, bg, stage="fine", cam_type=scene.dataset_type, delta_scale=1)
                fr = None if route == "old" else (g._fused_render_pool if streams > 1 else g._fused_render)
                if fr is not None:
                    fr.overflowed()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for c in cams:
                    out = R.render(c, g, pp, bg, stage="fine", cam_type=scene.dataset_type, delta_scale=1)["render"]
                bad = fr.overflowed() if fr is not None else []
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
            assert torch.isfinite(out).all()
            return len(cams) / dt, len(bad)
        finally:
            R.set_render_streams(1)
            dn.__dict__.pop("_field16_fusable", None)

    routes = ("old", "new", "new_two_streams")
    for r in routes:
        one_pass(r)
    fps, again = {r: [] for r in routes}, {r: 0 for r in routes}
    for _ in range(a.windows):
        for r in routes:
            v, bad = one_pass(r)
            fps[r].append(v)
            again[r] += bad
    rec = {r: {"median_fps": round(statistics.median(v), 1), "min_fps": round(min(v), 1), "max_fps": round(max(v), 1),
               "frames_flagged_incomplete": again[r]} for r, v in fps.items()}
    rec["what"] = ("no-grad render() frames/s, one pass over the 59-pose side trajectory per window, 960 x 540, async binning capacity; "
                   "old = op by op (the parent's route), new = FusedRender with the one-launch field, new_two_streams = FusedRenderPool")
    rec["criterion"] = {"slowest_new_over_fastest_old": round(rec["new"]["min_fps"] / rec["old"]["max_fps"], 4),
                        "new_wins_every_window": rec["new"]["min_fps"] > rec["old"]["max_fps"]}
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=200_000)
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--launches", type=int, default=40)
    ap.add_argument("--no-render", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    N = importlib.import_module(pkg + "._native")
    ops = importlib.import_module(pkg + ".ops")
    lib = N.lib()
    out = {"library": lib.mom_version().decode(), "device": torch.cuda.get_device_name(0), "points": a.points,
           "resolution": [64, 64, 64, 150], "multires": [1, 2], "windows": a.windows, "launches_per_window": a.launches,
           "what": "field: event-pair time per call, us (csrc/profile.hip; two_calls = hexplane_fwd + mlp_fwd): median window, lowest "
                   "and highest window"}
    out["field"] = field_times(a, torch, N, ops, lib)
    if not a.no_render:
        out["render"] = render_rates(a, torch)
    txt = json.dumps(out, indent=1)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(txt + "\n")
    print(txt)


if __name__ == "__main__":
    main()
