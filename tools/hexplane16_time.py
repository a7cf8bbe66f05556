"""The 16-channel HexPlane forward and two-pass backward beside the 32-channel kernels (two instantiations of the templates of csrc/hexplane.hip)
on the same points and resolutions: 200 000 points, resolution [64, 64, 64, 150], multires [1, 2], Morton order, plane orders given.

Times are the event pairs of csrc/profile.hip around mom_hexplane_forward / mom_hexplane_backward (slots hexplane_fwd and
hexplane_bwd), summed over the launches of a window and divided by their number; an event pair also spans the launch's own
dispatch (tools/acc_kernel_time.py).  The forms take turns, window by window, in one process; the record holds each form's
median window and the spread (lowest and highest window).  The 32-channel backward is timed twice: as a 32 x 2 field gets it (the
common-factor-row form) and in the six-row form the 16-channel kernels are the counterpart of (MOM_HEX_GATHER=5, read per call).

    python tools/hexplane16_time.py [--windows 9] [--launches 40] [--out profiles/hexplane16_time.json]
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
    N = importlib.import_module("iclr2025_3d-mom_amd._native")
    ops = importlib.import_module("iclr2025_3d-mom_amd.ops")
    HexPlaneField = importlib.import_module("iclr2025_3d-mom_amd.scene.hexplane").HexPlaneField
    lib = N.lib()
    slots = {lib.mom_profile_name(k).decode(): k for k in range(32) if lib.mom_profile_name(k)}
    s_fwd, s_bwd = slots["hexplane_fwd"], slots["hexplane_bwd"]
    P, t = a.points, 0.77
    pts = ((torch.rand(P, 3, generator=torch.Generator().manual_seed(1)) * 2 - 1) * torch.tensor([1.0, 1.2, 1.4])).cuda()
    order = ops.morton_order(pts)
    stream = N.current_stream()

    forms = {}
    for ch in (32, 16):
        torch.manual_seed(0)
        cfg = {'grid_dimensions': 2, 'input_coordinate_dim': 4, 'output_coordinate_dim': ch, 'resolution': [64, 64, 64, 150]}
        f = HexPlaneField(1.6, cfg, [1, 2])
        f.set_aabb([1.0, 1.2, 1.4], [-1.0, -1.2, -1.4])
        f = f.cuda()
        levels = [[p.detach() for p in g] for g in f.grids]
        grads = [[torch.zeros_like(p) for p in g] for g in levels]
        d, keep = ops._hexplane_desc(levels, f.aabb, grads, aabb_host=f.aabb_host())
        po = ops.hexplane_orders(pts, levels, f.aabb, aabb_host=f.aabb_host())
        feat = torch.empty(P, 2 * ch, device="cuda")
        dfeat = torch.randn(P, 2 * ch, device="cuda")
        dxyz = torch.zeros(P, 3, device="cuda")
        scratch = torch.empty(lib.mom_hexplane_backward_scratch_bytes(C.byref(d), P), dtype=torch.uint8, device="cuda")

        def fwd(d=d, feat=feat):
            N.check(lib.mom_hexplane_forward(C.byref(d), P, pts.data_ptr(), None, t, order.data_ptr(), feat.data_ptr(), stream), "fwd")

        def bwd(d=d, dfeat=dfeat, dxyz=dxyz, po=po, scratch=scratch):
            N.check(lib.mom_hexplane_backward(C.byref(d), P, pts.data_ptr(), None, t, order.data_ptr(), dfeat.data_ptr(), dxyz.data_ptr(),
                                              po[0].data_ptr(), po[1].data_ptr(), scratch.data_ptr(), stream), "bwd")

        forms[f"forward_{ch}"] = (fwd, s_fwd, None, (keep, grads, f))
        forms[f"backward_{ch}"] = (bwd, s_bwd, None, None)
        if ch == 32:
            forms["backward_32_six_rows"] = (bwd, s_bwd, "5", None)

    def window(fn, slot, gather):
        if gather is not None:
            os.environ["MOM_HEX_GATHER"] = gather
        try:
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            N.check(lib.mom_profile_enable(slot, 1), "profile")
            for _ in range(a.launches):
                fn()
            torch.cuda.synchronize()
            ms, cnt = C.c_double(), C.c_longlong()
            N.check(lib.mom_profile_read(slot, C.byref(ms), C.byref(cnt), 1), "profile")
            N.check(lib.mom_profile_enable(slot, 0), "profile")
            assert int(cnt.value) == a.launches, (int(cnt.value), a.launches)
            return ms.value * 1e3 / a.launches
        finally:
            os.environ.pop("MOM_HEX_GATHER", None)

    for name, (fn, slot, gather, _) in forms.items():       # every shape warmed up before the first timed window
        window(fn, slot, gather)
    times = {name: [] for name in forms}
    for _ in range(a.windows):
        for name, (fn, slot, gather, _) in forms.items():
            times[name].append(window(fn, slot, gather))
    out = {"library": lib.mom_version().decode(), "device": torch.cuda.get_device_name(0), "points": P,
           "resolution": [64, 64, 64, 150], "multires": [1, 2], "windows": a.windows, "launches_per_window": a.launches,
           "what": "event-pair time per call, us (csrc/profile.hip): median window, lowest and highest window"}
    for name, v in times.items():
        out[name] = {"median_us": round(statistics.median(v), 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2)}
    txt = json.dumps(out, indent=1)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(txt + "\n")
    print(txt)


if __name__ == "__main__":
    main()
