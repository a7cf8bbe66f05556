#!/usr/bin/env python
"""Writes tests/golden/g19_jpeg.npz: what Pillow (libjpeg) writes for every case of tests/jpeg_cases.py under the oracle call
    Image.save(buf, "JPEG", quality=Q, subsampling=2, optimize=False, restart_marker_blocks=R)
so that the GPU tests of the device JPEG encoder do not depend on the Pillow of the machine they run on.  Per case: the segments in
front of the scan without APPn and COM (DQT, SOF0, DHT, DRI, SOS) as one byte string, and the scan; for the one 476x896 case a
SHA-256 of the two and their length instead.  The inputs are not stored: jpeg_cases.py makes them from an integer hash or a closed form.
    python tools/gen_jpeg_golden.py            # rewrite the file
    python tools/gen_jpeg_golden.py --check    # exit 1 if this Pillow writes something else than the file holds"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import jpeg_cases as J  # noqa: E402


def golden():
    out = {"restart": np.array([J.RESTART], np.int32)}
    for name, (arr, Q) in J.cases().items():
        data = J.pil_encode(arr, Q)
        segs, scan = J.split(data)
        assert J.tables(segs)[3] == J.RESTART, "this Pillow ignored restart_marker_blocks"
        if name == J.FRAME:
            sha, n = J.digest(data)
            out["sha_" + name] = np.frombuffer(bytes.fromhex(sha), np.uint8)
            out["len_" + name] = np.array([n], np.int64)
        else:
            out["seg_" + name] = np.frombuffer(J.flat(segs), np.uint8)
            out["scan_" + name] = np.frombuffer(scan, np.uint8)
    return out


if __name__ == "__main__":
    g = golden()
    if "--check" in sys.argv:
        have = np.load(J.GOLDEN)
        ok = sorted(have.files) == sorted(g) and all(np.array_equal(have[k], g[k]) for k in g)
        sys.exit(0 if ok else 1)
    np.savez_compressed(J.GOLDEN, **g)
    print("wrote", J.GOLDEN, os.path.getsize(J.GOLDEN), "bytes")
