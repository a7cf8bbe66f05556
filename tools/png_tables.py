#!/usr/bin/env python
"""Writes iclr2025_3d-mom_amd/csrc/png_tables.h: the constant Huffman tables of the device PNG encoder (csrc/png_encode.hip).
    python tools/png_tables.py            # rewrite the header
    python tools/png_tables.py --check    # exit 1 if the committed header is not what this script writes

Table 0 is deflate's fixed code (RFC 1951 3.2.6).  Tables 1.. are dynamic-block codes built here, once, from a PRIOR instead of from
the image: the bytes the encoder codes are PNG filter residuals, which crowd around 0 modulo 256, so the prior is a two-sided
geometric distribution of the distance from 0 (scale `b` per table), a share of the mass for the run-length symbols and a floor that
gives every symbol a code.  The encoder prices a segment under every table and takes the cheapest, so a table only has to be good
for SOME residual statistics.  Literal/length codes are at most MAX_BITS long: the encoder sizes its LDS image by that.

Per table the header holds the canonical codes bit-reversed (deflate packs Huffman codes most-significant bit first into a stream
that fills bytes from the least-significant bit) with the length in bits 16.., and the block header -- BFINAL = 0, BTYPE, and for a
dynamic block HLIT, HDIST, HCLEN and the run-length coded code lengths (RFC 1951 3.2.7) -- as the bits the encoder copies out."""
import heapq
import math
import os
import sys
import zlib

MAX_BITS = 12
NLIT = 286          # literal/length symbols 0..285
NDIST = 4           # distance codes 0..3 (distances 1..4: the run-length matches use 1 and the pixel size)
HDR_WORDS = 16
SCALES = (1.2, 4.0, 12.0)
OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "iclr2025_3d-mom_amd", "csrc", "png_tables.h")
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)


def huffman_lengths(freqs, limit):
    """Code lengths of a Huffman code of the symbols with freqs > 0, no longer than `limit`: the floor under the frequencies is
    raised until the plain Huffman tree is shallow enough (the result is a complete code: Kraft sum exactly 1)."""
    total = float(sum(freqs))
    floor = 0.0
    while True:
        heap = [(max(f, floor), i, (i,)) for i, f in enumerate(freqs) if f > 0]
        assert len(heap) >= 2
        lengths = [0] * len(freqs)
        heapq.heapify(heap)
        tick = len(freqs)
        while len(heap) > 1:
            a = heapq.heappop(heap)
            b = heapq.heappop(heap)
            for s in a[2] + b[2]:
                lengths[s] += 1
            heapq.heappush(heap, (a[0] + b[0], tick, a[2] + b[2]))
            tick += 1
        if max(lengths) <= limit:
            return lengths
        floor = max(floor * 1.5, total / 2 ** (limit + 2))


def canonical(lengths):
    """RFC 1951 3.2.2: codes in symbol order within each length."""
    count = [0] * 16
    for n in lengths:
        count[n] += 1
    count[0] = 0
    code, nxt = 0, [0] * 16
    for bits in range(1, 16):
        code = (code + count[bits - 1]) << 1
        nxt[bits] = code
    out = []
    for n in lengths:
        out.append(nxt[n] if n else 0)
        if n:
            nxt[n] += 1
    return out


def reverse(code, n):
    return int(format(code, "0%db" % n)[::-1], 2) if n else 0


class Bits:
    def __init__(self):
        self.value, self.n = 0, 0

    def put(self, v, n):                    # n bits of v, least-significant first
        self.value |= (v & ((1 << n) - 1)) << self.n
        self.n += n

    def huff(self, code, n):
        self.put(reverse(code, n), n)

    def bytes(self):
        return self.value.to_bytes((self.n + 7) // 8, "little")


def prior(b):
    f = [0.0] * NLIT
    for v in range(256):
        f[v] = math.exp(-min(v, 256 - v) / b)
    lit = sum(f[:256])
    f[256] = lit * 1e-4                                     # one end-of-block per segment
    share = lit * 0.04                                      # run-length symbols: short runs and the longest are the common ones
    for s in range(257, 286):
        f[s] = share * (0.25 if s == 285 else 0.75 * 0.8 ** (s - 257) * 0.2 / (1 - 0.8 ** 28))
    return f


def run_length(seq):
    """RFC 1951 3.2.7: (symbol, extra value, extra bits) of the code-length sequence."""
    out, i = [], 0
    while i < len(seq):
        v, j = seq[i], i
        while j < len(seq) and seq[j] == v:
            j += 1
        n = j - i
        if v == 0:
            while n >= 11:
                k = min(n, 138)
                out.append((18, k - 11, 7))
                n -= k
            if n >= 3:
                out.append((17, n - 3, 3))
                n = 0
            out += [(0, 0, 0)] * n
        else:
            out.append((v, 0, 0))
            n -= 1
            while n >= 3:
                k = min(n, 6)
                out.append((16, k - 3, 2))
                n -= k
            out += [(v, 0, 0)] * n
        i = j
    return out


def dynamic_table(b):
    lit = huffman_lengths(prior(b), MAX_BITS)
    dist = [1, 0, 2, 2]                                      # distance 1 most often; 3 and 4 for RGB / RGBA pixels; 2 never
    rl = run_length(lit + dist)
    clf = [0] * 19
    for s, _, _ in rl:
        clf[s] += 1
    cl = huffman_lengths(clf, 7)
    clc = canonical(cl)
    hclen = max(i for i, s in enumerate(CL_ORDER) if cl[s]) + 1
    h = Bits()
    h.put(0, 1)                                             # BFINAL
    h.put(2, 2)                                             # BTYPE = dynamic
    h.put(NLIT - 257, 5)
    h.put(NDIST - 1, 5)
    h.put(hclen - 4, 4)
    for s in CL_ORDER[:hclen]:
        h.put(cl[s], 3)
    for s, ev, eb in rl:
        h.huff(clc[s], cl[s])
        h.put(ev, eb)
    return lit, dist, h


def fixed_table():
    lit = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
    dist = [5] * 32
    h = Bits()
    h.put(0, 1)
    h.put(1, 2)
    return lit, dist, h


def check_inflates(lit, h):
    """The header, the end-of-block code and padding are an empty deflate block."""
    codes = canonical(lit)
    tail = Bits()
    tail.value, tail.n = h.value, h.n
    tail.huff(codes[256], lit[256])
    tail.put(0, 3)                                          # the empty stored block the encoder puts behind every segment
    tail.put(0, (-tail.n) % 8)
    tail.put(0xFFFF0000, 32)
    tail.put(3, 10)                                         # a final empty fixed block ends the stream
    d = zlib.decompressobj(-15)
    assert d.decompress(tail.bytes()) == b"" and d.eof


def render():
    rows = []
    for t, (lit, dist, h) in enumerate([fixed_table()] + [dynamic_table(b) for b in SCALES]):
        assert max(lit) <= MAX_BITS and h.n <= 32 * HDR_WORDS, (t, max(lit), h.n)
        assert sum(2.0 ** -n for n in lit if n) == 1.0 and sum(2.0 ** -n for n in dist if n) == 1.0
        check_inflates(lit, h)
        lc, dc = canonical(lit), canonical(dist)
        litw = [reverse(lc[s], lit[s]) | lit[s] << 16 for s in range(NLIT)]
        distw = [reverse(dc[s], dist[s]) | dist[s] << 16 for s in range(NDIST)]
        hw = [(h.value >> (32 * i)) & 0xFFFFFFFF for i in range(HDR_WORDS)]
        fmt = lambda ws: ",".join("0x%x" % w for w in ws)
        rows.append("    {{%s},\n     {%s}, %d,\n     {%s}}" % (fmt(litw), fmt(distw), h.n, fmt(hw)))
    return ("// Generated by tools/png_tables.py -- do not edit; `python tools/png_tables.py --check` compares.\n"
            "// PngTable initialisers: {lit[%d] = bit-reversed code | bits << 16, dist[%d] likewise, header bits, header words}.\n"
            "// Table 0: deflate's fixed code.  Tables 1..%d: dynamic-block codes for residuals with a two-sided geometric prior of\n"
            "// scale %s.\n"
            "#pragma once\n"
            "#define PNG_TABLE_COUNT %d\n#define PNG_TABLE_NLIT %d\n#define PNG_TABLE_NDIST %d\n#define PNG_TABLE_HDR_WORDS %d\n"
            "#define PNG_TABLE_MAX_BITS %d\n"
            "#define PNG_TABLES_INIT {\\\n%s}\n"
            % (NLIT, NDIST, len(SCALES), ", ".join(str(b) for b in SCALES), len(SCALES) + 1, NLIT, NDIST, HDR_WORDS, MAX_BITS,
               ",\\\n".join(r.replace("\n", "\\\n") for r in rows)))


if __name__ == "__main__":
    text = render()
    if "--check" in sys.argv:
        sys.exit(0 if open(OUT).read() == text else 1)
    with open(OUT, "w") as fh:
        fh.write(text)
    print("wrote", OUT)
