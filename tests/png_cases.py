"""Inputs and the host-side decoder of the device PNG encoder's tests (test_png_device_cpu.py, test_png_device_gpu.py).

The decoder is the host's: zlib.decompress (which checks the Adler-32 and every block), `unfilter` -- PNG's five row filters
inverted in numpy, written from the PNG specification -- and PIL as a second opinion on the framed file (it checks the chunk CRCs).
The cases are the smallest shapes at which each mechanism of csrc/png_dev.h can break: a segment is ROWS rows, a lane's chunk CHUNK
bytes, a tile LANES chunks."""
import functools
import io
import os
import re
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_src = open(os.path.join(ROOT, "iclr2025_3d-mom_amd", "csrc", "png_dev.h")).read()
ROWS = int(re.search(r"kPngRowsPerSegment = (\d+);", _src).group(1))
CHUNK = int(re.search(r"kPngChunk = (\d+);", _src).group(1))
LANES = int(re.search(r"kPngLanes = (\d+);", _src).group(1))
TILE = CHUNK * LANES
SENTINEL = 0xA5
UNSUPPORTED = [(2, 4, 4), (5, 4, 4), (0, 4, 4), (3, 0, 4), (3, 4, 0), (3, -1, 4), (4, 1 << 15, 1 << 14), (1, 1 << 30, 2)]


def bound_formula(C, H, W):
    """The issue's: zlib header, every segment as stored blocks of at most 65535 bytes (5 bytes of header each), the final empty
    block, the Adler-32."""
    rb = 1 + W * C
    total = 2 + 2 + 4
    for y0 in range(0, H, ROWS):
        n = min(ROWS, H - y0) * rb
        total += n + 5 * -(-n // 65535)
    return total


def _smooth(H, W, C, seed):
    """A bright blob on a gradient with two grey levels of noise: what a render looks like to the coder."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    base = 90 + 60 * np.exp(-((x - 0.4 * W) ** 2 + (y - 0.6 * H) ** 2) / (0.08 * (W * W + H * H) + 1)) + 0.3 * x + 0.2 * y
    img = base[:, :, None] + 9.0 * np.arange(C)[None, None, :] + rng.integers(-1, 2, (H, W, C))
    return np.clip(img, 0, 255).astype(np.uint8)


def _runs():
    """16 x 300 greyscale noise with one run of equal bytes per row: lengths around the shortest match (2, 3, 4) and the longest
    (257..260, 600 -- longer than a row), at offsets that straddle a chunk border, and runs that end at the row's last byte."""
    rng = np.random.default_rng(5)
    H, W = 16, 300
    flat = rng.integers(0, 256, H * W, dtype=np.uint8)
    flat[1:] = np.where(flat[1:] == flat[:-1], flat[1:] ^ 0x55, flat[1:])        # no accidental runs
    lengths = [2, 3, 4, 257, 258, 259, 260, 600]
    for r in range(H):
        L = lengths[r % 8]
        if r < 8:
            start = r * W + 200                 # the filtered stream's chunk borders fall every CHUNK bytes: a row is 301
        else:
            start = (r + 1) * W - min(L, W)     # ends at the row's last byte
        flat[start:start + L] = 77 + r
    return flat[:H * W].reshape(H, W, 1)


@functools.lru_cache(maxsize=None)
def cases():
    """name -> [H,W,C] uint8 array (read-only)."""
    rng = np.random.default_rng(11)
    out = {}
    for C in (1, 3, 4):
        for H, W in ((1, 1), (1, 7), (5, 1), (2, 2), (37, 53)):
            out[f"smooth_{H}x{W}x{C}"] = _smooth(H, W, C, H * 100 + W + C)
    for H in (ROWS - 1, ROWS, ROWS + 1, 3 * ROWS + 1):
        out[f"rows_{H}x53x3"] = _smooth(H, 53, 3, H)
    for WC in (TILE - 1, TILE, TILE + 1):
        out[f"tile_2x{WC}x1"] = _smooth(2, WC, 1, WC)
    out[f"tile_2x{TILE // 3}x3"] = _smooth(2, TILE // 3, 3, 3)
    out[f"tile_2x{TILE // 4}x4"] = _smooth(2, TILE // 4, 4, 4)
    H, W = 37, 53
    for C in (1, 3, 4):
        out[f"zeros_x{C}"] = np.zeros((H, W, C), np.uint8)
        out[f"ones_x{C}"] = np.full((H, W, C), 255, np.uint8)
        out[f"alternating_x{C}"] = (np.arange(H * W * C) % 2 * 255).astype(np.uint8).reshape(H, W, C)
        out[f"noise_x{C}"] = rng.integers(0, 256, (H, W, C), dtype=np.uint8)
    x = np.arange(W)
    y = np.arange(H)
    out["hramp"] = np.broadcast_to((x * 4)[None, :, None] + (y * 97)[:, None, None], (H, W, 3)).astype(np.uint8)
    out["vramp"] = (np.broadcast_to(((y * 5) % 256)[:, None, None], (H, W, 3)) + (x * 37 % 200)[None, :, None]).astype(np.uint8)
    yy, xx = np.mgrid[0:H, 0:W]
    out["blob"] = np.broadcast_to((128 + 100 * np.sin(0.11 * (xx + yy)) * np.exp(-((xx - yy) / 30.0) ** 2))[:, :, None],
                                  (H, W, 3)).astype(np.uint8)
    out["runs"] = _runs()
    out["repeated_pixel"] = np.broadcast_to(np.array([200, 17, 99], np.uint8)[None, None, :], (19, 211, 3)).copy()
    out["stored_multi"] = rng.integers(0, 256, (ROWS, 5500, 4), dtype=np.uint8)      # one segment, longer than a stored block's 65535 bytes
    out["adler"] = np.full((24, 6000, 1), 255, np.uint8)
    for a in out.values():
        a.setflags(write=False)
    return out


def _paeth_row(cur, up, C):
    """Inverts Paeth on one row: cur filtered bytes, up the reconstructed row above; sequential in x, plain ints."""
    cur, up, n = cur.tolist(), up.tolist(), len(cur)
    for i in range(n):
        a = cur[i - C] if i >= C else 0
        b = up[i]
        c = up[i - C] if i >= C else 0
        p = a + b - c
        pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
        cur[i] = (cur[i] + (a if pa <= pb and pa <= pc else b if pb <= pc else c)) & 255
    return np.array(cur, np.uint8)


def unfilter(scanlines, H, W, C):
    """PNG scanlines (a filter byte, then W*C filtered bytes, per row) -> ([H,W,C] uint8, the rows' filter types)."""
    rows = np.frombuffer(scanlines, np.uint8).reshape(H, 1 + W * C)
    out = np.zeros((H, W * C), np.uint8)
    up = np.zeros(W * C, np.uint8)
    for y in range(H):
        f, cur = int(rows[y, 0]), rows[y, 1:]
        if f == 0:
            rec = cur.copy()
        elif f == 1:
            rec = np.cumsum(cur.reshape(W, C).astype(np.uint64), axis=0).astype(np.uint8).reshape(-1)
        elif f == 2:
            rec = cur + up
        elif f == 3:
            rec, u = cur.tolist(), up.tolist()
            for i in range(W * C):
                rec[i] = (rec[i] + (((rec[i - C] if i >= C else 0) + u[i]) >> 1)) & 255
            rec = np.array(rec, np.uint8)
        elif f == 4:
            rec = _paeth_row(cur, up, C)
        else:
            raise AssertionError(f"row {y}: filter type {f}")
        out[y] = up = rec
    return out.reshape(H, W, C), rows[:, 0].copy()


def decode(stream, arr, png_from_zlib_stream):
    """The whole decoder on one stream of the image `arr`: asserts it is `arr` exactly, both ways; returns the rows' filter types."""
    from PIL import Image
    H, W, C = arr.shape
    scan = zlib.decompress(bytes(stream))
    assert len(scan) == H * (1 + W * C)
    got, filters = unfilter(scan, H, W, C)
    assert np.array_equal(got, arr)
    pil = np.asarray(Image.open(io.BytesIO(png_from_zlib_stream(bytes(stream), H, W, C))))
    assert np.array_equal(pil.reshape(H, W, C), arr)
    return filters
