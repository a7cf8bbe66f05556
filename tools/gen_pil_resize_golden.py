#!/usr/bin/env python
"""Writes tests/golden/g23_pil_resize.npz: inputs, sizes and what Pillow's Image.resize((OW, OH), Image.BICUBIC) gives for them, so
that the tests of the device resize (csrc/pil_resize.hip) do not depend on the Pillow of the machine they run on.  Per case `name`:
in_<name> uint8 [N,H,W,C], size_<name> int32 (OW, OH), out_<name> uint8 [N,OH,OW,C]; `pillow` holds the version that made them.
Refuses to write unless mom_pil_resize_host gives Pillow's bytes on every case (no GPU is needed: the host entry is host code).
    python tools/gen_pil_resize_golden.py            # rewrite the file
    python tools/gen_pil_resize_golden.py --check    # exit 1 if this Pillow or this library gives something else than the file holds"""
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden", "g23_pil_resize.npz")
LIMIT = 300 * 1024

# name: (N, H, W, C, OH, OW, what the input is)
CASES = {
    "up_rgb": (1, 37, 53, 3, 64, 96, "noise"),              # up both axes, rows not dword-aligned
    "up_l": (1, 37, 53, 1, 64, 96, "noise"),
    "down_rgb": (1, 50, 70, 3, 17, 23, "noise"),            # down both axes
    "h_only": (1, 33, 65, 3, 33, 20, "noise"),              # the vertical pass is skipped
    "copy": (1, 40, 40, 3, 40, 40, "noise"),
    "taps105": (1, 128, 128, 3, 5, 96, "noise"),            # 105 vertical taps; down and up in one call
    "from_one": (1, 1, 1, 3, 7, 3, "noise"),
    "to_one": (1, 9, 9, 3, 1, 1, "noise"),
    "tiny": (1, 5, 7, 3, 11, 3, "noise"),
    "checker": (1, 32, 32, 3, 20, 48, "checker"),           # 0 / 255: both clamps fire under the negative lobes
    "batch": (3, 19, 21, 3, 30, 10, "noise"),               # batch stride, unaligned image bases
}


def make_input(name):
    N, H, W, C, _, _, kind = CASES[name]
    if kind == "checker":
        yy, xx = np.indices((H, W))
        return np.broadcast_to((((yy // 3 + xx // 2) & 1) * 255).astype(np.uint8)[None, :, :, None], (N, H, W, C)).copy()
    seed = int.from_bytes(name.encode(), "little") % (2 ** 32)
    return np.random.default_rng(seed).integers(0, 256, (N, H, W, C), dtype=np.uint8)


def pil_resize(a, OW, OH):
    from PIL import Image
    return np.stack([np.asarray(Image.fromarray(im[..., 0] if im.shape[2] == 1 else im).resize((OW, OH), Image.BICUBIC),
                                np.uint8).reshape(OH, OW, a.shape[3]) for im in a])


def host_resize(a, OW, OH):
    lib = importlib.import_module("iclr2025_3d-mom_amd._native").lib()
    N, H, W, C = a.shape
    a = np.ascontiguousarray(a)
    out = np.empty((N, OH, OW, C), np.uint8)
    rc = lib.mom_pil_resize_host(N, H, W, C, a.ctypes.data, OH, OW, 3, out.ctypes.data)
    assert rc == 0, f"mom_pil_resize_host returned {rc}"
    return out


def golden():
    import PIL
    g = {"pillow": np.frombuffer(PIL.__version__.encode(), np.uint8)}
    for name, (N, H, W, C, OH, OW, _) in CASES.items():
        a = make_input(name)
        ref = pil_resize(a, OW, OH)
        ours = host_resize(a, OW, OH)
        if not np.array_equal(ours, ref):
            sys.exit(f"{name}: mom_pil_resize_host differs from Pillow {PIL.__version__} in {int((ours != ref).sum())} of {ref.size} bytes; "
                     "nothing written")
        g["in_" + name], g["size_" + name], g["out_" + name] = a, np.array([OW, OH], np.int32), ref
    return g


if __name__ == "__main__":
    g = golden()
    if "--check" in sys.argv:
        have = np.load(GOLDEN)
        keys = [k for k in g if k != "pillow"]
        ok = sorted(k for k in have.files if k != "pillow") == sorted(keys) and all(np.array_equal(have[k], g[k]) for k in keys)
        sys.exit(0 if ok else 1)
    np.savez_compressed(GOLDEN, **g)
    size = os.path.getsize(GOLDEN)
    if size > LIMIT:
        os.remove(GOLDEN)
        sys.exit(f"{GOLDEN} would be {size} bytes, above the {LIMIT} this fixture may take; nothing written")
    print("wrote", GOLDEN, size, "bytes")
