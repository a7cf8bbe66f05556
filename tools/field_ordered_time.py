"""What the ordered field backward costs (include/mom4d.h, "ordered HexPlane backward", "ordered MLP weight gradients"), in one process,
at 200 000 points, for the default field (two levels of 32 channels, 64 features) and the 16 x 2 field (32 features):

  hexplane atomic    mom_hexplane_backward on its two-pass path with fresh plane orders (sorted for these positions before the
                     clock starts, as the training step reuses them) -- gather + scatter with float atomics
  hexplane ordered   mom_hexplane_backward_ordered: gather, twelve key / sort / segment / block-sum / texel rounds (its sorts
                     are part of the call), the position gradient
  mlp atomic         mom_deform_backward_n in its two-kernel f32 form (MOM_MLP_BWD=split is set by this tool)
  mlp ordered        mom_deform_backward_ordered_n

A sample is --reps calls between two device synchronisations, divided by --reps; a window is the median of --samples samples; the
two routes of a pair take turns, window by window.  The record keeps every window, each route's median, lowest and highest window,
their ratio and the scratch bytes.  The ordered routes are checked to repeat bit for bit.

One process; run it under a time limit (timeout -k 10 300 python tools/field_ordered_time.py ...) and start nothing behind it if it fails.

    python tools/field_ordered_time.py [--P 200000] [--windows 7] [--samples 5] [--reps 10] [--out profiles/field_ordered_time.json]
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
sys.path[:0] = [ROOT]
os.environ["MOM_MLP_BWD"] = "split"          # the f32 form at 64 features too (read per call by the library)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--P", type=int, default=200_000)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--samples", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    pkg = "iclr2025_3d-mom_amd"
    N = importlib.import_module(pkg + "._native")
    ops = importlib.import_module(pkg + ".ops")
    HexPlaneField = importlib.import_module(pkg + ".scene.hexplane").HexPlaneField
    lib, stream = N.lib(), N.current_stream()
    P = a.P
    u8 = lambda n: torch.empty(n, dtype=torch.uint8, device="cuda")
    gen = torch.Generator().manual_seed(14)
    rnd = lambda *s: torch.randn(*s, generator=gen).cuda()

    def sample(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.reps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6 / a.reps

    def pair(routes):
        for fn in routes.values():                      # both routes warmed up before the first window
            for _ in range(3):
                fn()
        runs = {name: [] for name in routes}
        for _ in range(a.windows):
            for name, fn in routes.items():
                runs[name].append(statistics.median(sample(fn) for _ in range(a.samples)))
                print(name, round(runs[name][-1], 1), "us", file=sys.stderr, flush=True)
        out = {name: {"median_us": round(statistics.median(v), 1), "min_us": round(min(v), 1), "max_us": round(max(v), 1),
                      "windows_us": [round(r, 1) for r in v]} for name, v in runs.items()}
        out["ratio_of_medians_ordered_over_atomic"] = round(statistics.median(runs["ordered"]) / statistics.median(runs["atomic"]), 3)
        return out

    out = {"library": lib.mom_version().decode(), "device": torch.cuda.get_device_name(0), "P": P,
           "windows": a.windows, "samples_per_window": a.samples, "calls_per_sample": a.reps,
           "order": "atomic, ordered, atomic, ordered, ...: one process",
           "what": "microseconds per call, host wall time of `calls_per_sample` calls between two device synchronisations; a window is the "
                   "median of its samples; median, lowest and highest window per route"}
    for channels in (32, 16):
        torch.manual_seed(0)
        cfg = {'grid_dimensions': 2, 'input_coordinate_dim': 4, 'output_coordinate_dim': channels, 'resolution': [64, 64, 64, 150]}
        f = HexPlaneField(1.6, cfg, [1, 2])
        f.set_aabb([1.3, 1.4, 1.5], [-1.2, -1.1, -1.0])
        with torch.no_grad():
            for g in f.grids:
                for p in g:
                    p.add_(torch.randn_like(p) * 0.2)
        f = f.cuda()
        hi, lo = torch.tensor([1.3, 1.4, 1.5]), torch.tensor([-1.2, -1.1, -1.0])
        xyz = (lo + torch.rand(P, 3, generator=gen) * (hi - lo)).cuda().contiguous()
        levels = [[p.detach() for p in lv] for lv in f.grids]
        grads = [[torch.zeros_like(p) for p in lv] for lv in levels]
        hp, keep = ops._hexplane_desc(levels, f.aabb, grads, aabb_host=f.aabb_host())
        F = f.feat_dim
        dfeat, dxyz = rnd(P, F), torch.zeros(P, 3, device="cuda")
        morton = ops.morton_order(xyz)
        po, pinv = ops.hexplane_orders(xyz, levels, f.aabb, aabb_host=f.aabb_host())
        hs = u8(lib.mom_hexplane_backward_scratch_bytes(C.byref(hp), P))
        need = lib.mom_hexplane_ordered_scratch_bytes(C.byref(hp), P)
        os_ = u8(need)

        def hex_atomic():
            N.check(lib.mom_hexplane_backward(C.byref(hp), P, xyz.data_ptr(), None, 0.3, morton.data_ptr(), dfeat.data_ptr(), dxyz.data_ptr(),
                                              po.data_ptr(), pinv.data_ptr(), hs.data_ptr(), stream), "hexplane_bwd")

        def hex_ordered():
            N.check(lib.mom_hexplane_backward_ordered(C.byref(hp), P, xyz.data_ptr(), 0.3, morton.data_ptr(), dfeat.data_ptr(), dxyz.data_ptr(),
                                                      os_.data_ptr(), need, stream), "hexplane_bwd_ordered")

        def hex_bits():
            for lv in grads:
                for g in lv:
                    g.zero_()
            dxyz.zero_()
            hex_ordered()
            torch.cuda.synchronize()
            return [g.clone() for lv in grads for g in lv] + [dxyz.clone()]
        one, two = hex_bits(), hex_bits()
        rec = {"hexplane": pair({"atomic": hex_atomic, "ordered": hex_ordered})}
        rec["hexplane"].update(scratch_bytes_atomic=int(hs.numel()), scratch_bytes_ordered=int(need),
                               ordered_repeats_bit_for_bit=all(torch.equal(x, y) for x, y in zip(one, two)))
        # the MLP at this field's width
        shapes = [(64, F), (64,)]
        for nout in (3, 3, 4):
            shapes += [(64, 64), (64,), (nout, 64), (nout,)]
        params = [rnd(*s) * 0.3 for s in shapes]
        mgrads = [torch.zeros_like(p) for p in params]
        md = ops.DeformMLPFunction._desc(params, mgrads)
        feat, a0 = rnd(P, F), torch.relu(rnd(P, 64))
        dpts, dsc, dro, mdfeat = rnd(P, 3), rnd(P, 3), rnd(P, 4), torch.empty(P, F, device="cuda")
        ms = u8(lib.mom_deform_backward_scratch_bytes(P))
        mneed = lib.mom_deform_backward_ordered_scratch_bytes(P)
        mo = u8(mneed)

        def mlp_atomic():
            N.check(lib.mom_deform_backward_n(C.byref(md), P, F, feat.data_ptr(), a0.data_ptr(), dpts.data_ptr(), dsc.data_ptr(), dro.data_ptr(),
                                              mdfeat.data_ptr(), ms.data_ptr(), stream), "deform_bwd")

        def mlp_ordered():
            N.check(lib.mom_deform_backward_ordered_n(C.byref(md), P, F, feat.data_ptr(), a0.data_ptr(), dpts.data_ptr(), dsc.data_ptr(),
                                                      dro.data_ptr(), mdfeat.data_ptr(), mo.data_ptr(), mneed, stream), "deform_bwd_ordered")

        def mlp_bits():
            for g in mgrads:
                g.zero_()
            mlp_ordered()
            torch.cuda.synchronize()
            return [g.clone() for g in mgrads] + [mdfeat.clone()]
        one, two = mlp_bits(), mlp_bits()
        rec["mlp"] = pair({"atomic": mlp_atomic, "ordered": mlp_ordered})
        rec["mlp"].update(scratch_bytes_atomic=int(ms.numel()), scratch_bytes_ordered=int(mneed),
                          ordered_repeats_bit_for_bit=all(torch.equal(x, y) for x, y in zip(one, two)))
        out[f"field_{channels}x2"] = rec
        del keep
    txt = json.dumps(out, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(txt + "\n")
    print(txt)


if __name__ == "__main__":
    main()
