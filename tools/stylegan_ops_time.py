"""Time of StyleGAN2's two native ops (ops.upfirdn2d, ops.fused_bias_act; csrc/stylegan_ops.hip) at every shape
`Generator(1024, 512, 8, channel_multiplier=2)` calls them with from the 128 x 128 level up, against the torch op sequence a ROCm
user would otherwise write, in one process, alternating windows:

  blur        the 4 x 4 FIR after an up-sampling convolution, [1,C,2H+1,2W+1] -> [1,C,2H,2W], pad (1,1): C = 256, 128, 64, 32
  upsample    ToRGB's skip image, [1,3,H,W] -> [1,3,2H,2W], up 2, pad (2,1): H = 64 ... 512
  activation  FusedLeakyReLU on [1,C,S,S]: bias + leaky ReLU + gain
  general     the blur's taps through the general kernel (up (1,1), down (1,1) with a 4 x 3 kernel is no instantiated mode), at the
              1024 level: expected to be slower than the instantiated mode beside it

  torch side  upfirdn2d: zero insertion, F.pad, conv2d with the flipped kernel, stride slice (stylegan_ops_cases.upfirdn2d_torch);
              activation: F.leaky_relu(x + b.view(1, -1, 1, 1), 0.2) * 2 ** 0.5

Algorithmic bytes are the input and the output once each (the taps and the bias are noise); the rate is those bytes over the median
time, beside the 6.0 TB/s measured for streaming on this device.  A window is --calls calls between a torch.cuda.Event
pair, the device synchronised before and after; --windows windows per side after a warm-up call of each.  Every GPU step runs under
an alarm of --step-limit seconds that ends the process; run it under a time limit as well.

    python tools/stylegan_ops_time.py [--windows 5] [--calls 20] [--out profiles/stylegan_ops_time.json]
"""
import argparse
import importlib
import json
import os
import signal
import statistics
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
pkg = "iclr2025_3d-mom_amd"
LEVELS = [(128, 256), (256, 128), (512, 64), (1024, 32)]        # (S, C) of Generator(1024, 512, 8, channel_multiplier=2)
STREAM_TBPS = 6.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20, help="calls per window")
    ap.add_argument("--step-limit", type=int, default=60, help="seconds any one GPU step may take before the process is ended")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import torch.nn.functional as F
    import stylegan_ops_cases as sc
    N = importlib.import_module(pkg + "._native")
    ops = importlib.import_module(pkg + ".ops")
    assert torch.cuda.is_available(), "this tool measures on the GPU; there is nothing to fall back to"
    dev = torch.device("cuda", 0)
    say = lambda *s: print(*s, file=sys.stderr, flush=True)

    class gpu_step:
        """SIGALRM's default action ends the process, inside a blocked runtime call as well."""
        def __enter__(self):
            signal.alarm(a.step_limit)

        def __exit__(self, *exc):
            signal.alarm(0)

    def window(fn):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0.record()
        for _ in range(a.calls):
            fn()
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1) / a.calls

    def stats(ms, nbytes):
        med = statistics.median(ms)
        return {"median_ms": round(med, 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
                "windows_ms": [round(x, 4) for x in ms], "algorithmic_TB_per_s": round(nbytes / (med * 1e-3) / 1e12, 3),
                "share_of_streaming_rate": round(nbytes / (med * 1e-3) / 1e12 / STREAM_TBPS, 3)}

    def compare(what, shape, ours, theirs, nbytes):
        sides = {"hip": ours, "torch": theirs}
        ms = {k: [] for k in sides}
        with gpu_step():
            for fn in sides.values():
                fn()
            torch.cuda.synchronize()
        for _ in range(a.windows):
            for k, fn in sides.items():                         # alternating windows
                with gpu_step():
                    ms[k].append(window(fn))
        row = {"op": what, "input": list(shape), "algorithmic_bytes": nbytes, "hip": stats(ms["hip"], nbytes),
               "torch": stats(ms["torch"], nbytes),
               "speedup_of_medians": round(statistics.median(ms["torch"]) / statistics.median(ms["hip"]), 2),
               "hip_slowest_beats_torch_fastest": max(ms["hip"]) < min(ms["torch"]),
               "hip_is_slower_at_the_median": statistics.median(ms["hip"]) > statistics.median(ms["torch"])}
        say(f"{what} {list(shape)}: hip {row['hip']['median_ms']} ms ({row['hip']['algorithmic_TB_per_s']} TB/s), torch "
            f"{row['torch']['median_ms']} ms, x{row['speedup_of_medians']}")
        return row

    rows = []
    blur = torch.from_numpy(sc.taps(4, 4, 0) * 4).to(dev)
    torch.manual_seed(0)
    with torch.no_grad():
        for S, C in LEVELS:
            x = torch.randn(1, C, S + 1, S + 1, device=dev)
            rows.append(compare("blur", x.shape, lambda: ops.upfirdn2d(x, blur, (1, 1), (1, 1), (1, 1, 1, 1)),
                                lambda: sc.upfirdn2d_torch(x, blur, (1, 1), (1, 1), (1, 1, 1, 1)), 4 * (x.numel() + C * S * S)))
            skip = torch.randn(1, 3, S // 2, S // 2, device=dev)
            rows.append(compare("upsample", skip.shape, lambda: ops.upfirdn2d(skip, blur, (2, 2), (1, 1), (2, 1, 2, 1)),
                                lambda: sc.upfirdn2d_torch(skip, blur, (2, 2), (1, 1), (2, 1, 2, 1)), 4 * (skip.numel() + 3 * S * S)))
            y, b = torch.randn(1, C, S, S, device=dev), torch.randn(C, device=dev)
            rows.append(compare("activation", y.shape, lambda: ops.fused_bias_act(y, b, None, 3, 0, 0.2, 2 ** 0.5),
                                lambda: F.leaky_relu(y + b.view(1, -1, 1, 1), 0.2) * 2 ** 0.5, 8 * y.numel()))
            del x, skip, y
            torch.cuda.empty_cache()
        S, C = LEVELS[-1]
        x, k43 = torch.randn(1, C, S + 1, S + 1, device=dev), torch.randn(4, 3, device=dev)
        rows.append(compare("general (4 x 3 taps)", x.shape, lambda: ops.upfirdn2d(x, k43, (1, 1), (1, 1), (1, 1, 1, 1)),
                            lambda: sc.upfirdn2d_torch(x, k43, (1, 1), (1, 1), (1, 1, 1, 1)), 4 * (x.numel() + C * (S + 1) * S)))

    slower = [f"{r['op']} {r['input']}: hip {r['hip']['median_ms']} ms, torch {r['torch']['median_ms']} ms" for r in rows
              if r["hip_is_slower_at_the_median"]]
    out = {"library": N.lib().mom_version().decode(), "device": torch.cuda.get_device_name(0),
           "what": "GPU time of one call in ms between two torch.cuda.Event records around --calls calls, the device synchronised "
                   "before and after each window; the two sides' windows alternate in one process; output allocation included on "
                   "both sides",
           "windows": a.windows, "calls_per_window": a.calls, "streaming_rate_TB_per_s": STREAM_TBPS, "rows": rows,
           "slower_than_the_torch_sequence": slower,
           "not_measured": "no hardware counters (no rocprofv3 run): rates are counted bytes over event time; at the lower levels "
                           "the tensors fit the 256 MB Infinity Cache, so their rates are not HBM rates"}
    txt = json.dumps(out, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(txt + "\n")
    print(txt)


if __name__ == "__main__":
    main()
