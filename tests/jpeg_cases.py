"""Shared by test_jpeg_device_cpu.py, test_jpeg_device_gpu.py and tools/gen_jpeg_golden.py: the case list of the device JPEG encoder
(csrc/jpeg_encode.hip), the oracle call, a marker parser, a baseline Huffman decoder of a scan to symbols (written from ITU T.81
F.2.2 -- it does not reconstruct pixels, PIL does that) and a parser of the AVI files render.AsyncVideoWriter writes.

Inputs come from an integer hash or a closed form, so the golden file holds only what PIL made of them."""
import hashlib
import io
import os
import struct

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g19_jpeg.npz")
RESTART = 8                 # MCUs per restart interval: csrc/jpeg_dev.h kJpegRestart (mom_jpeg_tables reports it)
HEADER_BYTES = 629          # SOI .. SOS, APP0 included
BLOCK_MAX_BYTES = 208       # a block's longest code, 22 + 63 * 26 bits
SENTINEL = 0xA5
FRAME = "frame_476x896_q90"  # render_set's own frame size: kept in the golden file as a digest only


def _hash8(n, seed):
    """n bytes of splitmix64 of the index."""
    with np.errstate(over="ignore"):
        x = np.arange(n, dtype=np.uint64) + np.uint64(seed) * np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        x = x ^ (x >> np.uint64(31))
    return (x >> np.uint64(24)).astype(np.uint8)


def noise(H, W, seed):
    return _hash8(H * W * 3, seed).reshape(H, W, 3)


def smooth(H, W, seed, amplitude=6):
    """A closed-form gradient with a little noise on it."""
    y, x = np.mgrid[0:H, 0:W]
    base = np.stack([(3 * x + 2 * y) // 4 % 256, 255 - (x + 5 * y) // 7 % 256, (x * y // 97 + 40) % 256], axis=2)
    n = noise(H, W, seed).astype(np.int64) % (amplitude + 1) if amplitude else 0
    return np.clip(base + n, 0, 255).astype(np.uint8)


def spikes(H, W, seed):
    """Flat areas with a sparse pixel of another value: long runs of zero coefficients between the few that survive quantisation."""
    a = np.full((H, W, 3), 118, np.uint8)
    n = _hash8(H * W, seed).reshape(H, W)
    a[n >= 254] = (255, 0, 255)
    a[n == 0] = (0, 255, 0)
    return a


def blocks8(H, W):
    y, x = np.mgrid[0:H, 0:W]
    return np.repeat(((((y // 8) + (x // 8)) % 2) * 255).astype(np.uint8)[:, :, None], 3, axis=2)


def checker(H, W):
    y, x = np.mgrid[0:H, 0:W]
    return np.repeat((((y + x) % 2) * 255).astype(np.uint8)[:, :, None], 3, axis=2)


_CASES = None


def cases():
    """name -> (rgb [H,W,3] uint8, quality)."""
    global _CASES
    if _CASES is None:
        c = {}
        for k, (H, W) in enumerate(((16, 16), (8, 8), (24, 24), (17, 33), (15, 31), (44, 56), (40, 9), (1, 1))):
            for Q in (50, 90, 100):
                c[f"noise_{H}x{W}_q{Q}"] = (noise(H, W, 11 + k), Q)
        c["spikes_48x80_q50"] = (spikes(48, 80, 5), 50)
        c["smooth_33x47_q50"] = (smooth(33, 47, 6), 50)
        c["blocks_32x40_q100"] = (blocks8(32, 40), 100)
        c["checker_24x24_q100"] = (checker(24, 24), 100)
        c["wrap_144x144_q90"] = (smooth(144, 144, 7, 40), 90)          # 81 MCUs: eleven intervals, RST7 is followed by RST0
        c[FRAME] = (smooth(476, 896, 8), 90)
        for a, _ in c.values():
            a.setflags(write=False)
        _CASES = c
    return _CASES


def bound_formula(H, W):
    nmcu = -(-W // 16) * -(-H // 16)
    full, rest = divmod(nmcu, RESTART)
    per = lambda m: 2 * m * 6 * BLOCK_MAX_BYTES + 2
    return HEADER_BYTES + full * per(RESTART) + (per(rest) if rest else 0)


def pil_encode(arr, Q, R=RESTART):
    """The oracle call."""
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(arr)).save(buf, "JPEG", quality=Q, subsampling=2, optimize=False, restart_marker_blocks=R)
    return buf.getvalue()


def pil_decode(data):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def split(data):
    """(segments, scan): segments is the list of (marker, payload) in front of the scan, APPn and COM left out, SOS included; scan is
    everything behind the SOS header up to EOI, restart markers and stuffed zeros included."""
    assert data[:2] == b"\xff\xd8" and data[-2:] == b"\xff\xd9"
    i, segs = 2, []
    while True:
        assert data[i] == 0xFF, i
        m, n = data[i + 1], int.from_bytes(data[i + 2:i + 4], "big")
        if not (0xE0 <= m <= 0xEF or m == 0xFE):
            segs.append((m, bytes(data[i + 4:i + 2 + n])))
        i += 2 + n
        if m == 0xDA:
            return segs, bytes(data[i:-2])


def flat(segs):
    """The segments as one byte string (marker, length, payload), for storing and comparing."""
    return b"".join(bytes([0xFF, m]) + struct.pack(">H", len(p) + 2) + p for m, p in segs)


def digest(data):
    segs, scan = split(data)
    return hashlib.sha256(flat(segs) + scan).hexdigest(), len(flat(segs)) + len(scan)


def tables(segs):
    """quant {id: 64 values in zigzag order}, huff {class << 4 | id: (counts, symbols)}, (H, W), restart interval."""
    quant, huff, size, dri = {}, {}, None, 0
    for m, p in segs:
        if m == 0xDB:
            while p:
                assert p[0] >> 4 == 0
                quant[p[0] & 15] = list(p[1:65])
                p = p[65:]
        elif m == 0xC4:
            while p:
                counts = list(p[1:17])
                n = sum(counts)
                huff[p[0]] = (counts, list(p[17:17 + n]))
                p = p[17 + n:]
        elif m == 0xC0:
            assert p[0] == 8 and p[5] == 3
            size = (int.from_bytes(p[1:3], "big"), int.from_bytes(p[3:5], "big"))
            assert p[6:15] == bytes([1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1])          # 4:2:0, Y on table 0, Cb and Cr on table 1
        elif m == 0xDD:
            dri = int.from_bytes(p[0:2], "big")
    return quant, huff, size, dri


class _Bits:
    def __init__(self, data):
        self.d, self.i, self.acc, self.n, self.stuffed = data, 0, 0, 0, 0

    def bit(self):
        if self.n == 0:
            assert self.i < len(self.d), "the scan ended inside a block"
            b = self.d[self.i]
            self.i += 1
            if b == 0xFF:
                nxt = self.d[self.i]
                assert nxt == 0, f"marker {nxt:#x} inside an interval"
                self.i += 1
                self.stuffed += 1
            self.acc, self.n = b, 8
        self.n -= 1
        return (self.acc >> self.n) & 1

    def bits(self, n):
        v = 0
        for _ in range(n):
            v = (v << 1) | self.bit()
        return v


def _decoder(counts, symbols):
    """T.81 F.2.2.3: {(length, code): symbol}."""
    table, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(counts[length - 1]):
            table[(length, code)] = symbols[k]
            code += 1
            k += 1
        code <<= 1
    return table


def _symbol(bits, table):
    code = 0
    for length in range(1, 17):
        code = (code << 1) | bits.bit()
        s = table.get((length, code))
        if s is not None:
            return s
    raise AssertionError("no Huffman code matches")


def decode_scan(data):
    """The scan's symbols.  Returns a dict:
    blocks   per block in file order: (component 0..2, DC category, DC difference, [AC symbols run << 4 | size], [AC values],
             ended by an EOB symbol)
    rst      the restart markers' numbers in file order
    stuffed  the number of FF 00 pairs
    dri, size"""
    segs, scan = split(data)
    _, huff, (H, W), dri = tables(segs)
    dec = {k: _decoder(*v) for k, v in huff.items()}
    nmcu = -(-W // 16) * -(-H // 16)
    # cut the scan at the restart markers: FF D0..D7 never occurs inside an interval (FF is always followed by 00 there)
    pieces, rst, start, i = [], [], 0, 0
    while i < len(scan) - 1:
        if scan[i] == 0xFF and 0xD0 <= scan[i + 1] <= 0xD7:
            pieces.append(scan[start:i])
            rst.append(scan[i + 1] - 0xD0)
            start = i = i + 2
        elif scan[i] == 0xFF:
            i += 2
        else:
            i += 1
    pieces.append(scan[start:])
    per = dri if dri else nmcu
    assert len(pieces) == -(-nmcu // per)
    blocks, stuffed = [], 0
    for n, piece in enumerate(pieces):
        bits = _Bits(piece)
        for _ in range(min(per, nmcu - n * per)):
            for comp in (0, 0, 0, 0, 1, 2):
                t = 0 if comp == 0 else 1
                cat = _symbol(bits, dec[t])
                v = bits.bits(cat)
                diff = v if (cat == 0 or v >> (cat - 1)) else v - (1 << cat) + 1
                k, syms, vals, eob = 1, [], [], False
                while k < 64:
                    rs = _symbol(bits, dec[0x10 | t])
                    syms.append(rs)
                    r, s = rs >> 4, rs & 15
                    if s == 0:
                        if r == 15:
                            k += 16
                            continue
                        assert r == 0
                        eob = True
                        break
                    k += r
                    assert k < 64
                    v = bits.bits(s)
                    vals.append(v if v >> (s - 1) else v - (1 << s) + 1)
                    k += 1
                blocks.append((comp, cat, diff, syms, vals, eob))
        # what is left of the interval is the pad: fewer than 8 one-bits
        assert bits.i == len(piece), (n, bits.i, len(piece))
        assert bits.acc & ((1 << bits.n) - 1) == (1 << bits.n) - 1
        stuffed += bits.stuffed
    return {"blocks": blocks, "rst": rst, "stuffed": stuffed, "dri": dri, "size": (H, W)}


# ---- AVI ---------------------------------------------------------------------------------------------------------------------
def _chunks(data, start, end):
    out, i = [], start
    while i < end:
        cc, n = data[i:i + 4], struct.unpack("<I", data[i + 4:i + 8])[0]
        out.append((cc, i + 8, n))
        i += 8 + n + (n & 1)
    assert i == end, (i, end)
    return out


def parse_avi(data):
    """The fields of an AVI with one MJPG video stream, every size and offset checked against the bytes: RIFF 'AVI ' = LIST hdrl
    (avih, LIST strl (strh, strf)), LIST movi (00dc ...), idx1."""
    assert data[:4] == b"RIFF" and data[8:12] == b"AVI "
    assert struct.unpack("<I", data[4:8])[0] == len(data) - 8
    top = _chunks(data, 12, len(data))
    assert [c[0] for c in top] == [b"LIST", b"LIST", b"idx1"]
    (_, h0, hn), (_, m0, mn), (_, x0, xn) = top
    assert data[h0:h0 + 4] == b"hdrl" and data[m0:m0 + 4] == b"movi"
    hdrl = _chunks(data, h0 + 4, h0 + hn)
    assert [c[0] for c in hdrl] == [b"avih", b"LIST"]
    (_, a0, an), (_, s0, sn) = hdrl
    assert an == 56 and data[s0:s0 + 4] == b"strl"
    avih = struct.unpack("<14I", data[a0:a0 + 56])
    strl = _chunks(data, s0 + 4, s0 + sn)
    assert [c[0] for c in strl] == [b"strh", b"strf"] and strl[0][2] == 56 and strl[1][2] == 40
    sh = data[strl[0][1]:strl[0][1] + 56]
    strh = {"type": sh[0:4], "handler": sh[4:8]}
    names = ("flags", "priority", "language", "initial", "scale", "rate", "start", "length", "buffer", "quality", "sample_size")
    strh.update(zip(names, struct.unpack("<IHHIIIIIIII", sh[8:48])))
    strh["frame"] = struct.unpack("<4h", sh[48:56])
    bi = struct.unpack("<IiiHHIIiiII", data[strl[1][1]:strl[1][1] + 40])
    strf = dict(zip(("size", "width", "height", "planes", "bits", "compression", "size_image", "xppm", "yppm", "used", "important"), bi))
    frames = []
    for cc, at, n in _chunks(data, m0 + 4, m0 + mn):
        assert cc == b"00dc"
        frames.append((at - 8 - m0, n, bytes(data[at:at + n])))
    assert xn == 16 * len(frames)
    for k, (off, n, _) in enumerate(frames):
        cc, flags, o, size = struct.unpack("<4sIII", data[x0 + 16 * k:x0 + 16 * k + 16])
        assert (cc, flags, o, size) == (b"00dc", 0x10, off, n), k
    return {"avih": dict(zip(("us_per_frame", "max_bytes_per_sec", "padding", "flags", "total_frames", "initial_frames", "streams",
                              "buffer", "width", "height"), avih[:10])),
            "strh": strh, "strf": strf, "frames": [f[2] for f in frames]}


# ---- the golden file (tools/gen_jpeg_golden.py) ------------------------------------------------------------------------------
_GOLDEN = None


def golden():
    global _GOLDEN
    if _GOLDEN is None:
        with np.load(GOLDEN) as f:
            _GOLDEN = {k: f[k] for k in f.files}
        assert int(_GOLDEN["restart"][0]) == RESTART
    return _GOLDEN


def golden_file(name):
    """PIL's file of a case, put together again from the stored segments and scan (no APP0: PIL reads it all the same)."""
    g = golden()
    return b"\xff\xd8" + g["seg_" + name].tobytes() + g["scan_" + name].tobytes() + b"\xff\xd9"


def assert_is_golden(name, data):
    """`data` is a whole JPEG file: every segment but APPn/COM, and the scan, are what PIL wrote for the case."""
    g = golden()
    segs, scan = split(data)
    if name == FRAME:
        sha, n = digest(data)
        assert n == int(g["len_" + name][0]), (n, int(g["len_" + name][0]))
        assert sha == g["sha_" + name].tobytes().hex()
        return
    assert flat(segs) == g["seg_" + name].tobytes(), "a segment in front of the scan differs"
    want = g["scan_" + name].tobytes()
    assert len(scan) == len(want), (len(scan), len(want))
    assert scan == want, next(i for i in range(len(scan)) if scan[i] != want[i])
