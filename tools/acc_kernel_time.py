"""The projection backward's two forms on the same frames: the store form (the first camera of a batch, every single-camera step)
against the accumulating form (cameras 2..B, mom_raster_backward_acc), inside the fine fused step at configs 2 and 1.

Times are the event pairs of csrc/profile.hip around the launch (slot `preprocess_bwd`), summed over the launches of a run and
divided by their number.  That is NOT the kernel duration of a rocprofv3 kernel trace (profiles/r06_a_*: 27 us for the store form at
config 2): an event pair also spans the launch's own dispatch.  Compare the two forms with each other, measured the same way in one
process; run this script under `rocprofv3 --kernel-trace --stats -- python tools/acc_kernel_time.py` for durations of the
instantiations by name (preprocess_bwd_kernel<STAGED, RAW, ACC>).

Cameras 1 and 4, each once as the first (stored) and once as the second (accumulated) of the pair; the accumulated time of a
camera = (the pair's total - the other camera's stored time) per launch.

    python tools/acc_kernel_time.py [--launches 50] [--out profiles/acc_kernel_time.json]
"""
import argparse
import ctypes as C
import importlib
import importlib.util
import json
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
spec = importlib.util.spec_from_file_location("bench", os.path.join(ROOT, "bench.py"))
bench = importlib.util.module_from_spec(spec)
spec.loader.exec_module(bench)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--configs", nargs="+", default=["c2", "c1"], choices=sorted(bench.CONFIGS))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    N = importlib.import_module("iclr2025_3d-mom_amd._native")
    lib = N.lib()
    slot = next(k for k in range(32) if lib.mom_profile_name(k) == b"preprocess_bwd")
    out = {"library": lib.mom_version().decode(), "device": torch.cuda.get_device_name(0), "launches": a.launches,
           "what": "event-pair time per launch of the projection backward, us (csrc/profile.hip)"}
    for name in a.configs:
        scene, g, trainer, op = bench.build_state(bench.CONFIGS[name], torch.device("cuda"), fused=True, lambda_dssim=0.0)
        fs = trainer.fused
        cams = [trainer.cams[1], trainer.cams[4]]

        def timed(arg):
            for _ in range(3):
                fs.forward_backward(arg, 1)
            torch.cuda.synchronize()
            N.check(lib.mom_profile_enable(slot, 1), "profile")
            for _ in range(a.launches):
                fs.forward_backward(arg, 1)
            torch.cuda.synchronize()
            ms, cnt = C.c_double(), C.c_longlong()
            N.check(lib.mom_profile_read(slot, C.byref(ms), C.byref(cnt), 1), "profile")
            N.check(lib.mom_profile_enable(slot, 0), "profile")
            return ms.value * 1e3, int(cnt.value)

        s1, n1 = timed(cams[0])
        s4, n4 = timed(cams[1])
        p14, n14 = timed(cams)
        p41, n41 = timed(cams[::-1])
        assert n1 == n4 == a.launches and n14 == n41 == 2 * a.launches
        visible = int((fs.radii > 0).sum())
        out[name] = {"P": int(g._xyz.shape[0]), "visible_in_either_camera": visible,
                     "store_us": {"camera 1": round(s1 / n1, 2), "camera 4": round(s4 / n4, 2)},
                     "accumulate_us": {"camera 4": round((p14 - s1 / n1 * a.launches) / a.launches, 2),
                                       "camera 1": round((p41 - s4 / n4 * a.launches) / a.launches, 2)}}
        del scene, g, trainer, fs
        torch.cuda.empty_cache()
    txt = json.dumps(out, indent=1)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(txt + "\n")
    print(txt)


if __name__ == "__main__":
    main()
