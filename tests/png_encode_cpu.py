"""The PNG patch encoder of include/hipac_png.h restated in numpy and plain Python: the definition the device is compared with,
byte for byte.  No zlib and no Pillow in the encode direction.  ``encode_file(level, x, y, P)`` gives the file's bytes;
``encode_file_info`` also says what was chosen on the way (filter types, block types, how often the length limiter fired)."""
import os
import re
import struct

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "hipac_png.h")


def _define(name):
    return int(re.search(rf"#define HIPAC_PNG_{name} (\d+)", open(HEADER).read()).group(1))


BAND_BYTES = _define("BAND_BYTES")
MAX_P = _define("MAX_P")

SIGNATURE = b"\x89PNG\r\n\x1a\n"
LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LENS = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
STORED, FIXED, DYNAMIC = 0, 1, 2

_CRC_TABLE = []
for _n in range(256):
    _c = _n
    for _ in range(8):
        _c = (_c >> 1) ^ 0xEDB88320 if _c & 1 else _c >> 1
    _CRC_TABLE.append(_c)


def crc32(data, crc=0):
    c = crc ^ 0xFFFFFFFF
    t = _CRC_TABLE
    for b in bytes(data):
        c = t[(c ^ b) & 255] ^ (c >> 8)
    return c ^ 0xFFFFFFFF


def adler_part(data):
    """(a, b) of Adler-32 over ``data`` started at (1, 0)."""
    d = np.frombuffer(bytes(data), np.uint8).astype(np.int64)
    n = len(d)
    a = (1 + int(d.sum())) % 65521
    b = (n + int((d * (n - np.arange(n, dtype=np.int64))).sum())) % 65521
    return a, b


def adler_combine(p1, p2, len2):
    (a1, b1), (a2, b2) = p1, p2
    return (a1 + a2 - 1) % 65521, (b1 + b2 + len2 * (a1 - 1)) % 65521


def chunk(kind, data):
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", crc32(kind + data))


def band_rows(P):
    return max(1, BAND_BYTES // (1 + 3 * P))


def n_bands(P):
    r = band_rows(P)
    return (P + r - 1) // r


def file_bound(P):
    """hipac_png_file_bound: all bands stored, plus every chunk and wrapper byte."""
    if not 1 <= P <= MAX_P:
        return 0
    nb = n_bands(P)
    return 8 + 25 + 12 * nb + 2 + P * (1 + 3 * P) + 5 * nb + 5 * (nb - 1) + 16 + 12


def window_pixels(level, x, y, P):
    """uint8[P, P, 3]: the window at (x, y) of ``level`` (uint8[H, W, 3]) on the white canvas."""
    H, W = level.shape[:2]
    out = np.full((P, P, 3), 255, np.uint8)
    x0, y0, x1, y1 = max(x, 0), max(y, 0), min(x + P, W), min(y + P, H)
    if x1 > x0 and y1 > y0:
        out[y0 - y:y1 - y, x0 - x:x1 - x] = level[y0:y1, x0:x1]
    return out


def filter_rows(pix):
    """(uint8[P, 1 + 3 P] filtered stream, the P filter types)."""
    P = pix.shape[0]
    raw = pix.reshape(P, 3 * P).astype(np.int32)
    out = np.zeros((P, 1 + 3 * P), np.uint8)
    types = []
    prev = np.zeros(3 * P, np.int32)
    for r in range(P):
        x = raw[r]
        a = np.concatenate([np.zeros(3, np.int32), x[:-3]])
        b = prev
        c = np.concatenate([np.zeros(3, np.int32), prev[:-3]])
        p = a + b - c
        pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
        paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
        cands = [x, x - a, x - b, x - ((a + b) >> 1), x - paeth]
        cands = [v & 255 for v in cands]
        costs = [int(np.minimum(v, 256 - v).sum()) for v in cands]
        t = costs.index(min(costs))  # the lowest type among equals
        out[r, 0] = t
        out[r, 1:] = cands[t]
        types.append(t)
        prev = x
    return out, types


def band_tokens(data):
    """The tokens of one band: (0, byte) literals and (1, length) distance-1 matches."""
    d = np.frombuffer(bytes(data), np.uint8)
    n = len(d)
    starts = np.concatenate([[0], np.flatnonzero(d[1:] != d[:-1]) + 1, [n]])
    toks = []
    for s, e in zip(starts[:-1].tolist(), starts[1:].tolist()):
        run, v = e - s, int(d[s])
        if run < 4:
            toks.extend([(0, v)] * run)
            continue
        toks.append((0, v))
        q, r = divmod(run - 1, 258)
        toks.extend([(1, 258)] * q)
        if r >= 3:
            toks.append((1, r))
        else:
            toks.extend([(0, v)] * r)
    return toks


def length_code(length):
    c = max(i for i in range(29) if LEN_BASE[i] <= length)
    return c, length - LEN_BASE[c]


def huffman_lengths(counts, limit):
    """Code lengths of the two-queue Huffman tree over the symbols with a non-zero count, leaf before internal node on equal
    weight; counts halved (rounding up) and the tree rebuilt while a code is longer than ``limit``.  Returns (lengths, number
    of halvings)."""
    counts = list(counts)
    halvings = 0
    while True:
        used = sorted((c, s) for s, c in enumerate(counts) if c > 0)
        n = len(used)
        lens = [0] * len(counts)
        if n == 0:
            return lens, halvings
        if n == 1:
            lens[used[0][1]] = 1
            return lens, halvings
        w = [0] * (n - 1)
        leaf_parent, node_parent = [0] * n, [0] * (n - 1)
        i = j = 0
        for m in range(n - 1):
            total = 0
            for _ in range(2):
                if i < n and (j >= m or used[i][0] <= w[j]):
                    total += used[i][0]
                    leaf_parent[i] = m
                    i += 1
                else:
                    total += w[j]
                    node_parent[j] = m
                    j += 1
            w[m] = total
        depth = [0] * (n - 1)
        for k in range(n - 3, -1, -1):
            depth[k] = depth[node_parent[k]] + 1
        for k in range(n):
            lens[used[k][1]] = depth[leaf_parent[k]] + 1
        if max(lens) <= limit:
            return lens, halvings
        counts = [(c + 1) >> 1 if c > 0 else 0 for c in counts]
        halvings += 1


def canonical_codes(lens):
    """Bit-reversed canonical codes (RFC 1951 3.2.2), ready for an LSB-first stream."""
    bl = [0] * 16
    for l in lens:
        bl[l] += 1
    bl[0] = 0
    nxt, code = [0] * 16, 0
    for b in range(1, 16):
        code = (code + bl[b - 1]) << 1
        nxt[b] = code
    out = []
    for l in lens:
        if l == 0:
            out.append(0)
            continue
        c = nxt[l]
        nxt[l] += 1
        out.append(int(format(c, f"0{l}b")[::-1], 2))
    return out


def code_length_tokens(seq):
    """The run-length coding of a code-length sequence: (symbol, extra value, extra bits) each."""
    out, i, n = [], 0, len(seq)
    while i < n:
        v = seq[i]
        e = i
        while e < n and seq[e] == v:
            e += 1
        run, sent = e - i, False
        while run > 0:
            if v == 0 and run >= 11:
                t = min(run, 138)
                out.append((18, t - 11, 7))
            elif v == 0 and run >= 3:
                t = run
                out.append((17, t - 3, 3))
            elif v != 0 and sent and run >= 3:
                t = min(run, 6)
                out.append((16, t - 3, 2))
            else:
                t = 1
                out.append((v, 0, 0))
                sent = True
            run -= t
        i = e
    return out


class BitWriter:
    def __init__(self, prefix=b""):
        self.out = bytearray(prefix)
        self.acc = 0
        self.n = 0

    def put(self, value, bits):
        self.acc |= value << self.n
        self.n += bits
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def align(self):
        if self.n:
            self.out.append(self.acc & 255)
            self.acc = self.n = 0


def encode_band(data, first, last):
    """(bytes of the band: the zlib header when ``first``, one deflate block, the byte alignment; info dict)."""
    data = bytes(data)
    L = len(data)
    toks = band_tokens(data)
    counts = [0] * 286
    extra_total = n_match = 0
    for kind, v in toks:
        if kind == 0:
            counts[v] += 1
        else:
            c, _ = length_code(v)
            counts[257 + c] += 1
            extra_total += LEN_EXTRA[c]
            n_match += 1
    counts[256] = 1
    lens, halvings = huffman_lengths(counts, 15)
    hlit = max(s for s in range(286) if lens[s]) + 1
    hlit = max(hlit, 257)
    cl_toks = code_length_tokens(lens[:hlit] + [1])
    cl_counts = [0] * 19
    for s, _, _ in cl_toks:
        cl_counts[s] += 1
    cl_lens, cl_halvings = huffman_lengths(cl_counts, 7)
    hclen = 19
    while hclen > 4 and cl_lens[CL_ORDER[hclen - 1]] == 0:
        hclen -= 1
    stored_bits = 40 + 8 * L
    fixed_bits = 3 + sum(c * l for c, l in zip(counts, FIXED_LENS)) + extra_total + 5 * n_match
    dyn_bits = (3 + 14 + 3 * hclen + sum(cl_lens[s] + eb for s, _, eb in cl_toks) + sum(c * l for c, l in zip(counts, lens))
                + extra_total + n_match)
    kind, best = STORED, stored_bits
    if fixed_bits < best:
        kind, best = FIXED, fixed_bits
    if dyn_bits < best:
        kind, best = DYNAMIC, dyn_bits
    w = BitWriter(b"\x78\x01" if first else b"")
    w.put(1 if last else 0, 1)
    w.put(kind, 2)
    if kind == STORED:
        w.align()
        w.out += struct.pack("<HH", L, L ^ 0xFFFF) + data
    else:
        if kind == DYNAMIC:
            w.put(hlit - 257, 5)
            w.put(0, 5)
            w.put(hclen - 4, 4)
            for k in range(hclen):
                w.put(cl_lens[CL_ORDER[k]], 3)
            cl_codes = canonical_codes(cl_lens)
            for s, ev, eb in cl_toks:
                w.put(cl_codes[s], cl_lens[s])
                w.put(ev, eb)
            use, dist_bits = lens, 1
        else:
            use, dist_bits = FIXED_LENS, 5
        codes = canonical_codes(use)
        for tk, v in toks:
            if tk == 0:
                w.put(codes[v], use[v])
            else:
                c, ev = length_code(v)
                w.put(codes[257 + c], use[257 + c])
                w.put(ev, LEN_EXTRA[c])
                w.put(0, dist_bits)
        w.put(codes[256], use[256])
    if not last:
        w.put(0, 3)
        w.align()
        w.out += b"\x00\x00\xff\xff"
    else:
        w.align()
    info = dict(kind=kind, halvings=halvings, cl_halvings=cl_halvings, bits=(stored_bits, fixed_bits, dyn_bits), tokens=len(toks))
    return bytes(w.out), info


def encode_pixels_info(pix):
    """The file of a P x P x 3 window, and what was chosen on the way."""
    P = pix.shape[0]
    stream, types = filter_rows(pix)
    rows = band_rows(P)
    nb = n_bands(P)
    out = bytearray(SIGNATURE + chunk(b"IHDR", struct.pack(">IIBBBBB", P, P, 8, 2, 0, 0, 0)))
    adler = (1, 0)
    bands = []
    for k in range(nb):
        data = stream[k * rows:(k + 1) * rows].tobytes()
        body, info = encode_band(data, k == 0, k == nb - 1)
        out += chunk(b"IDAT", body)
        adler = adler_combine(adler, adler_part(data), len(data))
        bands.append(info)
    out += chunk(b"IDAT", struct.pack(">I", adler[1] << 16 | adler[0]))
    out += chunk(b"IEND", b"")
    return bytes(out), dict(types=types, bands=bands, stream=stream.tobytes())


def encode_file_info(level, x, y, P):
    return encode_pixels_info(window_pixels(np.asarray(level), int(x), int(y), int(P)))


def encode_file(level, x, y, P):
    return encode_file_info(level, x, y, P)[0]


def idat_data(png):
    """The concatenated IDAT data of a PNG file, for the decoders the tests put it through."""
    pos, out = 8, bytearray()
    while pos < len(png):
        n, kind = struct.unpack(">I4s", png[pos:pos + 8])
        if kind == b"IDAT":
            out += png[pos + 8:pos + 8 + n]
        pos += 12 + n
    return bytes(out)
