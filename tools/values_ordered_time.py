"""What the ordered loss values cost (include/mom4d.h, "ordered loss values"), per op, in one process:

  l1      mom_l1_loss (memset + l1_kernel, two atomics per workgroup)   against  mom_l1_loss_ordered (kernel + fold)
  ssim    mom_ssim_forward (memset + kernel + 63-slot fold)             against  mom_ssim_forward_ordered (kernel + fold)
  reg     mom_plane_regulation (memset + plane_reg_kernel)              against  mom_plane_regulation_ordered (kernel + fold)

Sizes: a 3 x 540 x 960 image pair and the twelve planes of the default field (resolution [64, 64, 64, 150], two levels, 32
channels).  A sample is --reps calls between two device synchronisations, divided by --reps; a window is the median of --samples
samples; the two forms of an op take turns, window by window.  The record keeps every window, each form's median, lowest and highest
window, their ratio, and the scratch bytes of the ordered form; each ordered result is checked to repeat bit for bit.

One process; run it under a time limit (timeout -k 10 300 python tools/values_ordered_time.py ...) and start nothing behind it if it fails.

    python tools/values_ordered_time.py [--windows 7] [--samples 5] [--reps 20] [--out profiles/values_ordered_time.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

PLANES = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--W", type=int, default=960)
    ap.add_argument("--H", type=int, default=540)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--samples", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import importlib

    import torch
    pkg = "iclr2025_3d-mom_amd"
    N = importlib.import_module(pkg + "._native")
    ops = importlib.import_module(pkg + ".ops")
    lib, stream = N.lib(), N.current_stream()
    W, H = a.W, a.H
    g = torch.Generator("cpu").manual_seed(3)
    gt = torch.rand(3, H, W, generator=g).cuda()
    img = (gt + 0.05 * torch.randn(3, H, W, generator=g).cuda()).clamp(0, 1)
    n = img.numel()
    u8 = lambda k: torch.empty(max(k, 4), dtype=torch.uint8, device="cuda")
    dimg = torch.empty_like(img)
    sums = torch.empty(2, device="cuda")
    dm = torch.empty(3, 3, H, W, device="cuda")
    total = torch.empty(N.SSIM_SUM_SLOTS, dtype=torch.float64, device="cuda")
    win = ops.ssim_window()
    held, res = [], (64, 64, 64, 150)
    for m in (1, 2):
        r = (res[0] * m, res[1] * m, res[2] * m, res[3])
        held += [torch.randn(r[cb], r[ca], 32, generator=g).cuda() for ca, cb in PLANES]
    arr = (N.MomRegPlane * len(held))()
    for i, p in enumerate(held):
        arr[i].plane, arr[i].grad, arr[i].H, arr[i].W = p.data_ptr(), None, p.shape[0], p.shape[1]
        time_plane = PLANES[i % 6][1] == 3
        arr[i].w_smooth, arr[i].w_l1, arr[i].grad_scale = (1e-2, 1e-4, 0.0) if time_plane else (1e-4, 0.0, 0.0)
    value = torch.empty(1, device="cuda")
    need = {"l1": lib.mom_l1_loss_ordered_scratch_bytes(n), "ssim": lib.mom_ssim_ordered_scratch_bytes(3, H, W),
            "reg": lib.mom_plane_regulation_ordered_scratch_bytes(arr, len(held))}
    scratch = {k: u8(v) for k, v in need.items()}
    ck = N.check
    forms = {
        "l1": (lambda: ck(lib.mom_l1_loss(n, img.data_ptr(), gt.data_ptr(), dimg.data_ptr(), sums.data_ptr(), stream), "l1"),
               lambda: ck(lib.mom_l1_loss_ordered(n, img.data_ptr(), gt.data_ptr(), dimg.data_ptr(), sums.data_ptr(),
                                                  scratch["l1"].data_ptr(), need["l1"], stream), "l1 ordered"),
               lambda: sums.clone()),
        "ssim": (lambda: ck(lib.mom_ssim_forward(3, H, W, win, img.data_ptr(), gt.data_ptr(), dm.data_ptr(), total.data_ptr(), stream), "ssim"),
                 lambda: ck(lib.mom_ssim_forward_ordered(3, H, W, win, img.data_ptr(), gt.data_ptr(), dm.data_ptr(), total.data_ptr(),
                                                         scratch["ssim"].data_ptr(), need["ssim"], stream), "ssim ordered"),
                 lambda: total[:1].clone()),
        "reg": (lambda: ck(lib.mom_plane_regulation(arr, len(held), value.data_ptr(), stream), "reg"),
                lambda: ck(lib.mom_plane_regulation_ordered(arr, len(held), value.data_ptr(), scratch["reg"].data_ptr(), need["reg"], stream),
                           "reg ordered"),
                lambda: value.clone()),
    }

    def sample(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.reps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6 / a.reps

    out = {"library": lib.mom_version().decode(), "device": torch.cuda.get_device_name(0), "W": W, "H": H, "image_elements": n,
           "planes": [list(p.shape) for p in held], "windows": a.windows, "samples_per_window": a.samples, "calls_per_sample": a.reps,
           "order": "atomic, ordered, atomic, ordered, ... per op: one process",
           "what": "microseconds per call, host wall time of `calls_per_sample` calls between two device synchronisations; a window is "
                   "the median of its samples; median, lowest and highest window per form",
           "scratch_bytes": need}
    for op, (atomic, ordered, result) in forms.items():
        for fn in (atomic, ordered):                        # both forms warmed up before the first window
            for _ in range(3):
                fn()
        atomic()
        va = result()
        ordered()
        v1 = result()
        ordered()
        v2 = result()
        torch.cuda.synchronize()
        runs = {"atomic": [], "ordered": []}
        for _ in range(a.windows):
            for name, fn in (("atomic", atomic), ("ordered", ordered)):
                runs[name].append(statistics.median(sample(fn) for _ in range(a.samples)))
                print(op, name, round(runs[name][-1], 1), "us", file=sys.stderr, flush=True)
        rec = {"ordered_repeats_bit_for_bit": bool(torch.equal(v1, v2)),
               "largest_relative_difference_to_atomic": float(((v1.double() - va.double()).abs() / va.double().abs()).max())}
        for name, v in runs.items():
            rec[name] = {"median_us": round(statistics.median(v), 1), "min_us": round(min(v), 1), "max_us": round(max(v), 1),
                         "windows_us": [round(r, 1) for r in v]}
        rec["ratio_of_medians_ordered_over_atomic"] = round(statistics.median(runs["ordered"]) / statistics.median(runs["atomic"]), 3)
        out[op] = rec
    txt = json.dumps(out, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(txt + "\n")
    print(txt)


if __name__ == "__main__":
    main()
