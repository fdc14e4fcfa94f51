"""Tiled pyramidal TIFF / BigTIFF reader feeding the device pyramid.

The reference opens CAMELYON16 slides with openslide (src/main.py:650-655:
``OpenSlide(path)``, ``level_dimensions``, ``level_downsamples``) and pulls every window
through ``read_region(location, level, size)`` (:693-697).  openslide is not available in
this image, so this module reads the container itself: classic TIFF and BigTIFF, tiled
IFDs, 8-bit RGB, compression none / deflate and LZW (TIFF 6.0; predictor none or horizontal) / JPEG (old-style
excluded), one pyramid level per full-resolution or reduced-resolution tiled IFD, largest first
(the "generic tiled TIFF" layout of the CAMELYON16 files).

Tiles are decoded on host threads (Pillow's JPEG / zlib decoders release the GIL) in row
bands and copied band by band into the level's HBM tensor, so the host never holds more
than one band of one level.  Semantics kept from openslide:
  * ``level_dimensions`` / ``level_downsamples`` (downsample = level-0 width / level width),
  * pixels of missing tiles (byte count 0) are transparent black, which the reference's
    ``.convert("RGB")`` turns into (0,0,0) -- here they are written as 0,
  * ``read_region`` (host, RGBA uint8, out-of-bounds = transparent black) for small
    regions and for tests.
"""
from __future__ import annotations

import ctypes as C
import io
import struct
import zlib
from concurrent.futures import ThreadPoolExecutor
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np

_TYPES = {1: ("B", 1), 2: ("c", 1), 3: ("H", 2), 4: ("I", 4), 5: ("II", 8), 6: ("b", 1), 7: ("B", 1), 8: ("h", 2),
          9: ("i", 4), 10: ("ii", 8), 11: ("f", 4), 12: ("d", 8), 16: ("Q", 8), 17: ("q", 8), 18: ("Q", 8)}


class TiffError(ValueError):
    pass


LZW_ABI_VERSION = 1  # include/hipac_lzw.h HIPAC_LZW_ABI_VERSION this binding was written against
LZW_MAX_TILE_BYTES, LZW_MAX_TILES, LZW_MAX_LEVELS = 1 << 20, 65535, 16  # HIPAC_LZW_MAX_*
LZW_OK, LZW_REFUSED, LZW_MISSING, LZW_BAD_TILE = 0, 1, 2, 3  # status_dev values
# name -> (restype, argtypes); must list every symbol include/hipac_lzw.h declares (tests/test_lzw_capi_symbols.py)
LZW_SYMBOLS = {
    "hipac_lzw_abi_version": (C.c_int, []),
    "hipac_lzw_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "hipac_lzw_decode_tiles": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                         C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
}


class LzwLevel(C.Structure):
    """hipac_lzw_level (include/hipac_lzw.h)."""
    _fields_ = [("pixels", C.c_void_p), ("pitch_bytes", C.c_int64), ("W", C.c_int32), ("H", C.c_int32), ("tile_w", C.c_int32),
                ("tile_h", C.c_int32), ("samples", C.c_int32), ("predictor", C.c_int32)]


DEFLATE_ABI_VERSION = 1  # include/hipac_deflate.h HIPAC_DEFLATE_ABI_VERSION this binding was written against
DEFLATE_MAX_TILE_BYTES, DEFLATE_MAX_TILES, DEFLATE_MAX_LEVELS = 1 << 20, 65535, 16  # HIPAC_DEFLATE_MAX_*
DEFLATE_OK, DEFLATE_REFUSED, DEFLATE_MISSING, DEFLATE_BAD_TILE = 0, 1, 2, 3  # status_dev values
# name -> (restype, argtypes); must list every symbol include/hipac_deflate.h declares (tests/test_deflate_capi_symbols.py)
DEFLATE_SYMBOLS = {
    "hipac_deflate_abi_version": (C.c_int, []),
    "hipac_deflate_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "hipac_deflate_decode_tiles": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                             C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
}


class DeflateLevel(C.Structure):
    """hipac_deflate_level (include/hipac_deflate.h): the fields of hipac_lzw_level."""
    _fields_ = LzwLevel._fields_


_lzw_bound = None
_deflate_bound = None


def load_lzw_library():
    """The library of ``capi.load_library()`` with the LZW entry points bound; HipacError on a version mismatch."""
    global _lzw_bound
    from . import capi

    lib = capi.load_library()
    if _lzw_bound is not lib:
        _lzw_bound = capi.bind_symbols(lib, LZW_SYMBOLS, "hipac_lzw_abi_version", LZW_ABI_VERSION, "LZW ABI")
    return lib


def device_lzw_tiles(file_dev, levels, off, cnt, xyl):
    """One ``hipac_lzw_decode_tiles`` call.  ``file_dev``: uint8 tensor of the file's bytes; ``levels``: (tensor uint8[H, Wpad, 3],
    width, height, tile_w, tile_h, samples, predictor) each; ``off`` / ``cnt``: int64[n]; ``xyl``: int32[n, 3].  Returns the
    status of every tile as numpy uint8[n], read once after the call."""
    import torch

    from . import capi

    lib = load_lzw_library()
    device = file_dev.device
    n = int(len(off))
    arr = (LzwLevel * len(levels))()
    for i, (dv, w, h, tw, th, spp, pred) in enumerate(levels):
        arr[i] = LzwLevel(dv.data_ptr(), int(dv.stride(0)), w, h, tw, th, spp, pred)
    tw, th, spp = max(l[3] for l in levels), max(l[4] for l in levels), max(l[5] for l in levels)
    need = max(lib.hipac_lzw_workspace_bytes(l[3], l[4], l[5], n) for l in levels)
    if need == 0:
        raise TiffError(f"LZW tiles of {tw} x {th} x {spp} samples, or {n} of them in one call, are not decoded on the device")
    with torch.cuda.device(device):
        ws = torch.empty(need, dtype=torch.uint8, device=device)
        o = torch.from_numpy(np.ascontiguousarray(off, np.int64)).to(device)
        c = torch.from_numpy(np.ascontiguousarray(cnt, np.int64)).to(device)
        q = torch.from_numpy(np.ascontiguousarray(xyl, np.int32)).to(device)
        status = torch.empty(n, dtype=torch.uint8, device=device)
        capi._check(lib.hipac_lzw_decode_tiles(file_dev.data_ptr(), int(file_dev.numel()), C.addressof(arr), len(levels), o.data_ptr(),
                                               c.data_ptr(), q.data_ptr(), n, ws.data_ptr(), int(ws.numel()), status.data_ptr(),
                                               capi._stream()), "hipac_lzw_decode_tiles")
        return status.cpu().numpy()


def deflate_level_on_device(lv) -> bool:
    """Whether the device decoder takes the tiles of ``lv`` (a TiffLevel with compression 8 or 32946): the limits of
    include/hipac_deflate.h.  Other levels stay with zlib on host threads, as all deflate levels did before."""
    return lv.samples in (1, 3, 4) and lv.predictor in (1, 2) and 1 <= lv.tile_w * lv.tile_h * lv.samples <= DEFLATE_MAX_TILE_BYTES


def load_deflate_library():
    """The library of ``capi.load_library()`` with the deflate entry points bound; HipacError on a version mismatch."""
    global _deflate_bound
    from . import capi

    lib = capi.load_library()
    if _deflate_bound is not lib:
        _deflate_bound = capi.bind_symbols(lib, DEFLATE_SYMBOLS, "hipac_deflate_abi_version", DEFLATE_ABI_VERSION, "deflate ABI")
    return lib


def device_deflate_tiles(file_dev, levels, off, cnt, xyl):
    """One ``hipac_deflate_decode_tiles`` call; the arguments and the result are those of ``device_lzw_tiles``."""
    import torch

    from . import capi

    lib = load_deflate_library()
    device = file_dev.device
    n = int(len(off))
    arr = (DeflateLevel * len(levels))()
    for i, (dv, w, h, tw, th, spp, pred) in enumerate(levels):
        arr[i] = DeflateLevel(dv.data_ptr(), int(dv.stride(0)), w, h, tw, th, spp, pred)
    need = 0
    for _, _, _, tw, th, spp, _ in levels:  # each level by itself: one the decoder refuses is not hidden by the others
        one = lib.hipac_deflate_workspace_bytes(tw, th, spp, n)
        if one == 0:
            raise TiffError(f"deflate tiles of {tw} x {th} x {spp} samples, or {n} of them in one call, are not decoded on the device")
        need = max(need, one)
    with torch.cuda.device(device):
        ws = torch.empty(need, dtype=torch.uint8, device=device)
        o = torch.from_numpy(np.ascontiguousarray(off, np.int64)).to(device)
        c = torch.from_numpy(np.ascontiguousarray(cnt, np.int64)).to(device)
        q = torch.from_numpy(np.ascontiguousarray(xyl, np.int32)).to(device)
        status = torch.empty(n, dtype=torch.uint8, device=device)
        capi._check(lib.hipac_deflate_decode_tiles(file_dev.data_ptr(), int(file_dev.numel()), C.addressof(arr), len(levels), o.data_ptr(),
                                                   c.data_ptr(), q.data_ptr(), n, ws.data_ptr(), int(ws.numel()), status.data_ptr(),
                                                   capi._stream()), "hipac_deflate_decode_tiles")
        return status.cpu().numpy()


@dataclass
class TiffLevel:
    width: int
    height: int
    tile_w: int
    tile_h: int
    compression: int
    photometric: int
    samples: int
    offsets: Sequence[int]
    counts: Sequence[int]
    jpeg_tables: Optional[bytes]
    subfile_type: int
    predictor: int = 1  # tag 317, read for LZW and deflate levels: 1 none, 2 horizontal differencing

    @property
    def tiles_across(self) -> int:
        return (self.width + self.tile_w - 1) // self.tile_w

    @property
    def tiles_down(self) -> int:
        return (self.height + self.tile_h - 1) // self.tile_h


def _parse_ifds(buf) -> List[dict]:
    bo = {b"II": "<", b"MM": ">"}.get(bytes(buf[:2]))
    if bo is None:
        raise TiffError("not a TIFF file")
    magic = struct.unpack(bo + "H", buf[2:4])[0]
    if magic == 42:
        big, off = False, struct.unpack(bo + "I", buf[4:8])[0]
    elif magic == 43:
        big, off = True, struct.unpack(bo + "Q", buf[8:16])[0]
    else:
        raise TiffError(f"bad TIFF magic {magic}")
    ifds = []
    seen = set()
    while off and off not in seen and len(ifds) < 64:
        seen.add(off)
        if big:
            (n,) = struct.unpack(bo + "Q", buf[off:off + 8])
            pos, esz, cw = off + 8, 20, 8
        else:
            (n,) = struct.unpack(bo + "H", buf[off:off + 2])
            pos, esz, cw = off + 2, 12, 4
        tags = {}
        for i in range(n):
            e = buf[pos + i * esz: pos + (i + 1) * esz]
            tag, typ = struct.unpack(bo + "HH", e[:4])
            (cnt,) = struct.unpack(bo + ("Q" if big else "I"), e[4:4 + cw])
            if typ not in _TYPES:
                continue
            fmt, sz = _TYPES[typ]
            nbytes = cnt * sz
            if nbytes <= cw:
                raw = bytes(e[4 + cw:4 + cw + nbytes])
            else:
                (voff,) = struct.unpack(bo + ("Q" if big else "I"), e[4 + cw:4 + 2 * cw])
                raw = bytes(buf[voff:voff + nbytes])
            if typ in (2, 7):
                tags[tag] = raw
            elif typ in (5, 10):
                vals = struct.unpack(bo + fmt[0] * (2 * cnt), raw)
                tags[tag] = [vals[2 * j] / max(1, vals[2 * j + 1]) for j in range(cnt)]
            else:
                tags[tag] = list(struct.unpack(bo + fmt * cnt, raw))
        ifds.append(tags)
        nxt = buf[pos + n * esz: pos + n * esz + cw]
        (off,) = struct.unpack(bo + ("Q" if big else "I"), nxt)
    return ifds


def lzw_decode(data, n_out: int) -> Tuple[bytes, int]:
    """TIFF 6.0 LZW, the definition csrc/lzw.hip is compared with: (``n_out`` bytes, status).

    Codes are MSB-first, 9 to 12 bits; 256 = Clear, 257 = EOI; the width grows one code early (at table sizes 511, 1023,
    2047); the code after a Clear is a literal (further Clears are skipped, EOI ends the stream); a code equal to the next
    free entry is the previous string plus its own first byte (KwKwK); a table filled to 4095 without a Clear stays at 12
    bits and takes no more entries.  Decoding stops at EOI, when ``n_out`` bytes are written, or when fewer bits than one
    code are left; what was not written is 0.  Status 1 (and all bytes 0): the first code is neither Clear nor a literal,
    a code is larger than the next free entry, a Clear is followed by a code above 257, or the stream is of the old
    LSB-first variant (libtiff's test: first byte 0, second byte odd)."""
    data = bytes(data)
    n = len(data)
    zero = bytes(n_out)
    if n >= 2 and data[0] == 0 and data[1] & 1:
        return zero, 1
    out = bytearray(n_out)
    table = [bytes([i]) for i in range(256)] + [b"", b""]
    pos = acc = nb = o = 0
    width, prev, first = 9, None, True
    while o < n_out:
        while nb < width and pos < n:
            acc = (acc << 8) | data[pos]
            pos += 1
            nb += 8
        if nb < width:
            break
        nb -= width
        code = acc >> nb
        acc &= (1 << nb) - 1
        if code == 257:
            if first:
                return zero, 1
            break
        first = False
        if code == 256:
            del table[258:]
            width, prev = 9, None
            continue
        nxt = len(table)
        if prev is None:
            if code > 255:
                return zero, 1
            s = table[code]
        else:
            if code < nxt:
                s = table[code]
            elif code == nxt and nxt < 4096:
                s = prev + prev[:1]
            else:
                return zero, 1
            if nxt < 4096:
                table.append(prev + s[:1])
                if nxt + 2 >= 1 << width and width < 12:
                    width += 1
        m = min(len(s), n_out - o)
        out[o:o + m] = s[:m]
        o += m
        prev = s
    return bytes(out), 0


_LEN_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
_LEN_EXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
_DIST_BASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193,
              12289, 16385, 24577)
_DIST_EXTRA = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)
_CODE_LENGTH_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
_FIXED_LENGTHS = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8


class _Refused(Exception):
    pass


def _huffman_code(lengths, kind: str) -> dict:
    """Canonical Huffman code of RFC 1951 3.2.2 as {(length, code read MSB first): symbol}, with zlib's admission rules:
    an over-subscribed set is refused; an incomplete one is refused too, except a literal/length or distance set that
    consists of a single one-bit code, and a distance set without any code (a block of literals only).  A bit pattern no
    code owns is not in the table: reading it is a refusal.  ``kind``: "codes" | "lens" | "dists"."""
    count = [0] * 16
    for l in lengths:
        count[l] += 1
    count[0] = 0
    left = 1
    for l in range(1, 16):
        left = 2 * left - count[l]
        if left < 0:
            raise _Refused
    longest = max((l for l in range(1, 16) if count[l]), default=0)
    if left > 0 and (kind == "codes" or longest > 1 or (longest == 0 and kind != "dists")):
        raise _Refused  # (a code-length code without codes cannot describe an end-of-block code: zlib fails later, always)
    nxt, code = [0] * 16, 0
    for l in range(1, 16):
        code = (code + count[l - 1]) << 1
        nxt[l] = code
    table = {}
    for sym, l in enumerate(lengths):
        if l:
            table[(l, nxt[l])] = sym
            nxt[l] += 1
    return table


def inflate(data, n_out: int) -> Tuple[bytes, int]:
    """A zlib stream (RFC 1950 around RFC 1951), the definition csrc/deflate.hip is compared with: (``n_out`` bytes, status).

    Status 0: the header is valid (CM = 8, CINFO <= 7, (CMF * 256 + FLG) % 31 == 0, FDICT = 0), every block is well-formed,
    exactly ``n_out`` bytes come out and the big-endian Adler-32 behind the last block matches; bytes behind the checksum
    are ignored, as ``zlib.decompress`` ignores them.  Everything else is status 1 with all bytes 0: block type 3; a stored
    block whose LEN and ~NLEN disagree; more than 286 literal/length or 30 distance code lengths; code-length sets zlib
    rejects (``_huffman_code``); a repeat code without a previous length or past HLIT + HDIST; no end-of-block code; a bit
    pattern no code owns; length symbols 286 and 287, distance symbols 30 and 31; a distance beyond the bytes written so
    far; input that ends mid-stream; output beyond ``n_out`` or short of it; a checksum mismatch.  Production decoding
    stays with ``zlib.decompress``: this restatement is what the tests compare the kernel, and zlib, with."""
    data = bytes(data)
    n = len(data)
    out = bytearray()
    pos = 0  # in bits

    def bits(k: int) -> int:
        nonlocal pos
        if pos + k > 8 * n:
            raise _Refused  # input ends mid-stream
        v = (int.from_bytes(data[pos >> 3:(pos >> 3) + 4], "little") >> (pos & 7)) & ((1 << k) - 1)  # k <= 16
        pos += k
        return v

    def symbol(table: dict) -> int:
        nonlocal pos
        ahead = int.from_bytes(data[pos >> 3:(pos >> 3) + 4], "little") >> (pos & 7)  # bits behind the end read as 0
        code = 0
        for l in range(1, 16):
            code = (code << 1) | (ahead & 1)
            ahead >>= 1
            sym = table.get((l, code))
            if sym is not None:
                if pos + l > 8 * n:
                    raise _Refused  # input ends mid-stream
                pos += l
                return sym
        raise _Refused  # a bit pattern no code owns, or the input ends

    try:
        if n < 2 or (data[0] * 256 + data[1]) % 31 or data[0] & 15 != 8 or data[0] >> 4 > 7 or data[1] & 32:
            raise _Refused
        pos = 16
        final = 0
        while not final:
            final, kind = bits(1), bits(2)
            if kind == 0:
                pos = (pos + 7) & ~7
                length, inverse = bits(16), bits(16)
                if length != inverse ^ 0xFFFF or pos + 8 * length > 8 * n or len(out) + length > n_out:
                    raise _Refused
                out += data[pos >> 3:(pos >> 3) + length]
                pos += 8 * length
                continue
            if kind == 3:
                raise _Refused
            if kind == 1:
                lens, dists = _huffman_code(_FIXED_LENGTHS, "lens"), _huffman_code([5] * 32, "dists")
            else:
                hlit, hdist, hclen = bits(5) + 257, bits(5) + 1, bits(4) + 4
                if hlit > 286 or hdist > 30:
                    raise _Refused
                cl = [0] * 19
                for i in range(hclen):
                    cl[_CODE_LENGTH_ORDER[i]] = bits(3)
                codes = _huffman_code(cl, "codes")
                lengths = []
                while len(lengths) < hlit + hdist:
                    sym = symbol(codes)
                    if sym < 16:
                        lengths.append(sym)
                        continue
                    if sym == 16:
                        if not lengths:
                            raise _Refused
                        value, repeat = lengths[-1], 3 + bits(2)
                    else:
                        value, repeat = 0, 3 + bits(3) if sym == 17 else 11 + bits(7)
                    if len(lengths) + repeat > hlit + hdist:
                        raise _Refused
                    lengths += [value] * repeat
                if lengths[256] == 0:
                    raise _Refused
                lens, dists = _huffman_code(lengths[:hlit], "lens"), _huffman_code(lengths[hlit:], "dists")
            while True:
                sym = symbol(lens)
                if sym < 256:
                    if len(out) >= n_out:
                        raise _Refused
                    out.append(sym)
                    continue
                if sym == 256:
                    break
                if sym > 285:
                    raise _Refused
                length = _LEN_BASE[sym - 257] + bits(_LEN_EXTRA[sym - 257])
                sym = symbol(dists)
                if sym > 29:
                    raise _Refused
                dist = _DIST_BASE[sym] + bits(_DIST_EXTRA[sym])
                if dist > len(out) or len(out) + length > n_out:
                    raise _Refused
                for _ in range(length):
                    out.append(out[-dist])  # byte-serial: an overlapping copy repeats what it has just written
        pos = (pos + 7) & ~7
        check = bits(8) << 24 | bits(8) << 16 | bits(8) << 8 | bits(8)
        s1 = (1 + sum(out)) % 65521
        s2 = (len(out) + sum((len(out) - i) * b for i, b in enumerate(out))) % 65521
        if len(out) != n_out or check != (s2 << 16 | s1):
            raise _Refused
    except _Refused:
        return bytes(n_out), DEFLATE_REFUSED
    return bytes(out), DEFLATE_OK


def lzw_encode(data, clear_when_full: bool = True) -> bytes:
    """The writer's LZW (tests and synthetic data): greedy longest match, Clear first and again when the table reaches
    4094 (as libtiff does), EOI last, early change.  ``clear_when_full=False`` never clears after the first Clear: the
    table fills to 4095 and the stream goes on at 12 bits."""
    data = bytes(data)
    out = bytearray()
    acc = nb = 0
    width, nxt = 9, 258

    def emit(code):
        nonlocal acc, nb
        acc = (acc << width) | code
        nb += width
        while nb >= 8:
            nb -= 8
            out.append((acc >> nb) & 0xFF)
        acc &= (1 << nb) - 1

    def added():  # one more entry: the decoder gets it one code later, and both change width after the same code
        nonlocal width, nxt
        nxt += 1
        if clear_when_full and nxt == 4094:
            emit(256)
            table.clear()
            width, nxt = 9, 258
        elif nxt >= 1 << width and width < 12:
            width += 1

    table = {}
    emit(256)
    if data:
        w = data[0]
        for c in data[1:]:
            k = (w << 8) | c
            got = table.get(k)
            if got is not None:
                w = got
                continue
            emit(w)
            if nxt < 4096:
                table[k] = nxt
                added()
            w = c
        emit(w)
        if nxt < 4096:
            added()
    emit(257)
    if nb:
        out.append((acc << (8 - nb)) & 0xFF)
    return bytes(out)


def undo_predictor(tile: np.ndarray) -> np.ndarray:
    """Predictor 2 undone: per row and sample the running sum mod 256 over the whole tile width.  uint8[h, w, s]."""
    return np.cumsum(tile.astype(np.uint32), axis=1).astype(np.uint8)


def _adobe_rgb_marker() -> bytes:
    # APP14 "Adobe" with transform = 0: the three components are RGB, not YCbCr
    return b"\xff\xee\x00\x0eAdobe\x00\x64\x00\x00\x00\x00\x00"


def _jpeg_tile_stream(raw: bytes, jpeg_tables: Optional[bytes], photometric: int) -> bytes:
    """The complete JPEG stream the host decoder is given for the tile bytes ``raw`` of a directory with that JPEGTables tag
    and photometric tag.  Photometric 2 says the three components ARE R, G, B (what libtiff tells libjpeg, whatever markers
    the tile carries): the stream gets an Adobe marker with transform 0, and loses a JFIF APP0 -- libjpeg takes JFIF as
    "YCbCr" before it looks at Adobe -- and an Adobe marker of its own, which would be read after the inserted one."""
    data = raw
    if jpeg_tables:
        tb = jpeg_tables
        data = tb[:-2] + raw[2:] if tb[-2:] == b"\xff\xd9" and raw[:2] == b"\xff\xd8" else raw
    if photometric != 2 or data[:2] != b"\xff\xd8":
        return data
    out, pos = [data[:2], _adobe_rgb_marker()], 2
    while pos + 4 <= len(data) and data[pos] == 0xFF and data[pos + 1] not in (0xDA, 0xD9, 0xFF):
        end = pos + 2 + int.from_bytes(data[pos + 2:pos + 4], "big")
        seg = data[pos:end]
        if not (seg[1] == 0xE0 and seg[4:9] == b"JFIF\x00") and not (seg[1] == 0xEE and seg[4:9] == b"Adobe"):
            out.append(seg)
        pos = end
    return b"".join(out) + data[pos:]


class TiffPyramid:
    """Tiled TIFF pyramid.  ``level_dimensions`` / ``level_downsamples`` as in openslide."""

    def __init__(self, path: str, samples: Sequence[int] = (3, 4)):
        """``samples``: the samples per pixel a pyramid level may have -- RGB / RGBA for slides; ``read_mask_level`` also
        admits 1 (grayscale evaluation masks)."""
        self.path = path
        self._mm = np.memmap(path, dtype=np.uint8, mode="r")
        self._buf = memoryview(self._mm)
        levels = []
        for t in _parse_ifds(self._buf):
            if 322 not in t or 324 not in t:  # not tiled (label / macro / thumbnail strips): not a pyramid level
                continue
            bits = t.get(258, [8])
            spp = t.get(277, [1])[0]
            if any(b != 8 for b in bits) or spp not in samples or t.get(284, [1])[0] != 1:
                continue
            lv = TiffLevel(width=t[256][0], height=t[257][0], tile_w=t[322][0], tile_h=t[323][0],
                           compression=t.get(259, [1])[0], photometric=t.get(262, [2])[0], samples=spp,
                           offsets=t[324], counts=t[325], jpeg_tables=t.get(347), subfile_type=t.get(254, [0])[0])
            if lv.compression not in (1, 5, 7, 8, 32946):
                raise TiffError(f"unsupported tile compression {lv.compression} (none, LZW, JPEG and deflate are read)")
            if lv.compression in (5, 8, 32946):
                lv.predictor = t.get(317, [1])[0]
                if lv.predictor not in (1, 2):
                    raise TiffError(f"unsupported {'LZW' if lv.compression == 5 else 'deflate'} predictor {lv.predictor} "
                                    "(1 = none and 2 = horizontal are read)")
            levels.append(lv)
        if not levels:
            raise TiffError(f"no tiled 8-bit image directory with {' or '.join(map(str, samples))} samples per pixel found")
        levels.sort(key=lambda l: -l.width * l.height)
        self.levels: List[TiffLevel] = levels
        self.level_count = len(levels)
        self.level_dimensions = tuple((l.width, l.height) for l in levels)
        self.dimensions = self.level_dimensions[0]
        self.level_downsamples = tuple(self.dimensions[0] / l.width for l in levels)

    # ---- tiles -------------------------------------------------------------------------
    def _decode_tile(self, lv: TiffLevel, index: int) -> Optional[np.ndarray]:
        """uint8[tile_h, tile_w, 3] (uint8[tile_h, tile_w, 1] for a grayscale level) or None for a missing tile."""
        off, cnt = lv.offsets[index], lv.counts[index]
        if cnt == 0:
            return None
        raw = bytes(self._buf[off:off + cnt])
        if lv.compression == 1:
            a = np.frombuffer(raw, np.uint8)
        elif lv.compression in (8, 32946):
            a = np.frombuffer(zlib.decompress(raw), np.uint8)
        elif lv.compression == 5:
            data, status = lzw_decode(raw, lv.tile_h * lv.tile_w * lv.samples)
            self.lzw_refused = getattr(self, "lzw_refused", 0) + status  # a refused tile is all 0
            a = np.frombuffer(data, np.uint8).reshape(lv.tile_h, lv.tile_w, lv.samples)
            return (undo_predictor(a) if lv.predictor == 2 else a)[:, :, :3]
        else:
            from PIL import Image

            im = Image.open(io.BytesIO(_jpeg_tile_stream(raw, lv.jpeg_tables, lv.photometric)))
            im.load()
            a = np.asarray(im.convert("L"))[:, :, None] if lv.samples == 1 else np.asarray(im.convert("RGB"))
            if a.shape[0] != lv.tile_h or a.shape[1] != lv.tile_w:
                raise TiffError("JPEG tile size does not match the directory")
            return a
        a = a[: lv.tile_h * lv.tile_w * lv.samples].reshape(lv.tile_h, lv.tile_w, lv.samples)
        return (undo_predictor(a) if lv.predictor == 2 else a)[:, :, :3]  # a deflate level may carry predictor 2

    def read_band(self, level: int, tile_row: int, pool: Optional[ThreadPoolExecutor] = None) -> np.ndarray:
        """uint8[rows, width, 3] of one row of tiles (clipped to the level), missing tiles = 0."""
        lv = self.levels[level]
        y0 = tile_row * lv.tile_h
        rows = min(lv.tile_h, lv.height - y0)
        band = np.zeros((rows, lv.width, 3), np.uint8)
        idx = [tile_row * lv.tiles_across + tx for tx in range(lv.tiles_across)]
        tiles = list(pool.map(lambda i: self._decode_tile(lv, i), idx)) if pool else [self._decode_tile(lv, i) for i in idx]
        for tx, t in enumerate(tiles):
            if t is None:
                continue
            x0 = tx * lv.tile_w
            cols = min(lv.tile_w, lv.width - x0)
            band[:, x0:x0 + cols] = t[:rows, :cols]
        return band

    def read_region(self, location: Tuple[int, int], level: int, size: Tuple[int, int]) -> np.ndarray:
        """openslide semantics: ``location`` in level-0 coordinates, ``size`` in level pixels;
        returns uint8[h, w, 4] RGBA, transparent black outside the level and in missing tiles."""
        lv = self.levels[level]
        ds = self.level_downsamples[level]
        x0, y0 = int(location[0] / ds), int(location[1] / ds)
        w, h = size
        out = np.zeros((h, w, 4), np.uint8)
        for ty in range(max(0, y0 // lv.tile_h), min(lv.tiles_down, (y0 + h - 1) // lv.tile_h + 1)):
            for tx in range(max(0, x0 // lv.tile_w), min(lv.tiles_across, (x0 + w - 1) // lv.tile_w + 1)):
                t = self._decode_tile(lv, ty * lv.tiles_across + tx)
                if t is None:
                    continue
                gx0, gy0 = tx * lv.tile_w, ty * lv.tile_h
                ax0, ay0 = max(gx0, x0), max(gy0, y0)
                ax1 = min(gx0 + lv.tile_w, lv.width, x0 + w)
                ay1 = min(gy0 + lv.tile_h, lv.height, y0 + h)
                if ax1 <= ax0 or ay1 <= ay0:
                    continue
                out[ay0 - y0:ay1 - y0, ax0 - x0:ax1 - x0, :3] = t[ay0 - gy0:ay1 - gy0, ax0 - gx0:ax1 - gx0]
                out[ay0 - y0:ay1 - y0, ax0 - x0:ax1 - x0, 3] = 255
        return out

    # ---- device pyramid ----------------------------------------------------------------
    def _device_jpeg_levels(self, lvs, devs, chunk_bytes: Optional[int] = None):
        """JPEG tiles of the given levels decoded on the device (csrc/jpeg_decode.hip: Huffman one lane per tile, libjpeg's
        integer IDCT, fancy upsampling, YCbCr -> RGB), written into ``devs`` (uint8[H, Wpad, 3] each).  The tiles of ALL levels
        go into the same calls (a call lasts as long as its slowest tile).  Returns, per level, the indices of the tiles the
        device decoder did not take (another sampling, progressive, ...): the caller decodes those on the host."""
        import ctypes as C

        import torch

        from . import capi

        lib = capi.load_library()
        device = devs[0].device
        import warnings

        file_dev = torch.empty(int(self._mm.shape[0]) + 64, dtype=torch.uint8, device=device)  # + slack behind the end
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")  # "the given NumPy array is not writable": it is only read
            file_dev[:self._mm.shape[0]].copy_(torch.from_numpy(self._mm))
        if chunk_bytes is None:  # scratch for as many tiles per call as HBM allows: a call lasts as long as its slowest tile
            free, _ = torch.cuda.mem_get_info(device)
            chunk_bytes = int(max(1 << 30, min(96 << 30, free // 2)))
        tabs = [np.frombuffer(bytes(lv.jpeg_tables), np.uint8) if lv.jpeg_tables else None for lv in lvs]
        arr = (capi.JpegLevel * len(lvs))()
        for i, (lv, dv) in enumerate(zip(lvs, devs)):
            arr[i] = capi.JpegLevel(dv.data_ptr(), int(dv.stride(0)), lv.width, lv.height, lv.tile_w, lv.tile_h, int(lv.photometric), 0,
                                    tabs[i].ctypes.data if tabs[i] is not None else None, int(tabs[i].shape[0]) if tabs[i] is not None else 0)
        off, cnt, xyl, lvl_of, idx_of = [], [], [], [], []
        for i, lv in enumerate(lvs):
            n = lv.tiles_across * lv.tiles_down
            k = np.arange(n)
            off.append(np.asarray(lv.offsets[:n], np.int64)), cnt.append(np.asarray(lv.counts[:n], np.int64))
            xyl.append(np.stack([(k % lv.tiles_across) * lv.tile_w, (k // lv.tiles_across) * lv.tile_h, np.full(n, i)], 1).astype(np.int32))
            lvl_of.append(np.full(n, i)), idx_of.append(k)
        off, cnt, xyl = np.concatenate(off), np.concatenate(cnt), np.concatenate(xyl)
        lvl_of, idx_of = np.concatenate(lvl_of), np.concatenate(idx_of)
        n = off.shape[0]
        tw, th = max(lv.tile_w for lv in lvs), max(lv.tile_h for lv in lvs)
        per_tile = lib.hipac_jpeg_workspace_bytes(tw, th, 1)
        step = int(max(1, min(32768, chunk_bytes // max(per_tile, 1))))
        ws = torch.empty(lib.hipac_jpeg_workspace_bytes(tw, th, min(step, n)), dtype=torch.uint8, device=device)
        left = [[] for _ in lvs]
        with torch.cuda.device(device):
            for i0 in range(0, n, step):
                m = min(step, n - i0)
                status = np.ones(m, np.uint8)
                o, c, q = np.ascontiguousarray(off[i0:i0 + m]), np.ascontiguousarray(cnt[i0:i0 + m]), np.ascontiguousarray(xyl[i0:i0 + m])
                capi._check(lib.hipac_jpeg_decode_tiles(self._mm.ctypes.data, file_dev.data_ptr(), int(self._mm.shape[0]), C.addressof(arr),
                                                        len(lvs), o.ctypes.data, c.ctypes.data, q.ctypes.data, m, ws.data_ptr(),
                                                        int(ws.numel()), status.ctypes.data, capi._stream()), "hipac_jpeg_decode_tiles")
                for k in np.nonzero(status == 1)[0]:
                    left[int(lvl_of[i0 + k])].append(int(idx_of[i0 + k]))
                self.device_decoded = getattr(self, "device_decoded", 0) + int((status == 0).sum())
        return left

    def _device_lzw_levels(self, lvs, devs, step: int = 16384):
        """LZW tiles of the given levels decoded on the device (csrc/lzw.hip: one wavefront per tile, then the predictor and
        the placement), written into ``devs`` (uint8[H, Wpad, 3] each).  The file's bytes go to HBM as they are, without slack:
        the kernels check every read.  Tiles of all levels share the calls.  Returns the number of tiles the decoder refused
        (status 1: malformed streams; their pixels are 0 -- the host decoder is the same definition and refuses them too)."""
        import warnings

        import torch

        device = devs[0].device
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")  # "the given NumPy array is not writable": it is only read
            file_dev = torch.from_numpy(self._mm).to(device)
        table = [(dv, lv.width, lv.height, lv.tile_w, lv.tile_h, lv.samples, lv.predictor) for lv, dv in zip(lvs, devs)]
        off, cnt, xyl = [], [], []
        for i, lv in enumerate(lvs):
            n = lv.tiles_across * lv.tiles_down
            k = np.arange(n)
            off.append(np.asarray(lv.offsets[:n], np.int64)), cnt.append(np.asarray(lv.counts[:n], np.int64))
            xyl.append(np.stack([(k % lv.tiles_across) * lv.tile_w, (k // lv.tiles_across) * lv.tile_h, np.full(n, i)], 1).astype(np.int32))
        off, cnt, xyl = np.concatenate(off), np.concatenate(cnt), np.concatenate(xyl)
        per_tile = max(lv.tile_w * lv.tile_h * lv.samples for lv in lvs)
        free, _ = torch.cuda.mem_get_info(device)
        step = int(max(1, min(step, LZW_MAX_TILES, (free // 2) // max(per_tile, 1))))
        refused = 0
        for i0 in range(0, off.shape[0], step):
            status = device_lzw_tiles(file_dev, table, off[i0:i0 + step], cnt[i0:i0 + step], xyl[i0:i0 + step])
            if (status == LZW_BAD_TILE).any():
                raise TiffError(f"{self.path}: {int((status == LZW_BAD_TILE).sum())} LZW tiles lie outside the file")
            refused += int((status == LZW_REFUSED).sum())
            self.device_decoded = getattr(self, "device_decoded", 0) + int((status == LZW_OK).sum())
        return refused

    def _device_deflate_levels(self, lvs, devs, step: int = 16384):
        """Deflate tiles of the given levels decoded on the device (csrc/deflate.hip: one wavefront per tile, then the
        predictor and the placement), written into ``devs`` as ``_device_lzw_levels`` does.  Returns, per level, the indices of
        the tiles the device refused (status 1; their pixels are 0 so far): the caller hands those to the host decoder, as it
        does with the tiles ``_device_jpeg_levels`` leaves, so a stream zlib takes is never lost and one it rejects raises
        what it raised before."""
        import warnings

        import torch

        device = devs[0].device
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")  # "the given NumPy array is not writable": it is only read
            file_dev = torch.from_numpy(self._mm).to(device)
        table = [(dv, lv.width, lv.height, lv.tile_w, lv.tile_h, lv.samples, lv.predictor) for lv, dv in zip(lvs, devs)]
        off, cnt, xyl, lvl_of, idx_of = [], [], [], [], []
        for i, lv in enumerate(lvs):
            n = lv.tiles_across * lv.tiles_down
            k = np.arange(n)
            off.append(np.asarray(lv.offsets[:n], np.int64)), cnt.append(np.asarray(lv.counts[:n], np.int64))
            xyl.append(np.stack([(k % lv.tiles_across) * lv.tile_w, (k // lv.tiles_across) * lv.tile_h, np.full(n, i)], 1).astype(np.int32))
            lvl_of.append(np.full(n, i)), idx_of.append(k)
        off, cnt, xyl = np.concatenate(off), np.concatenate(cnt), np.concatenate(xyl)
        lvl_of, idx_of = np.concatenate(lvl_of), np.concatenate(idx_of)
        per_tile = max(lv.tile_w * lv.tile_h * lv.samples for lv in lvs)
        free, _ = torch.cuda.mem_get_info(device)
        step = int(max(1, min(step, DEFLATE_MAX_TILES, (free // 2) // max(per_tile, 1))))
        left = [[] for _ in lvs]
        for i0 in range(0, off.shape[0], step):
            status = device_deflate_tiles(file_dev, table, off[i0:i0 + step], cnt[i0:i0 + step], xyl[i0:i0 + step])
            if (status == DEFLATE_BAD_TILE).any():
                raise TiffError(f"{self.path}: {int((status == DEFLATE_BAD_TILE).sum())} deflate tiles lie outside the file")
            for k in np.nonzero(status == DEFLATE_REFUSED)[0]:
                left[int(lvl_of[i0 + k])].append(int(idx_of[i0 + k]))
            self.device_decoded = getattr(self, "device_decoded", 0) + int((status == DEFLATE_OK).sum())
        return left

    def to_device_levels(self, device="cuda", levels: Optional[Sequence[int]] = None, workers: int = 16,
                         device_jpeg: Optional[bool] = None, device_lzw: Optional[bool] = None,
                         device_deflate: Optional[bool] = None):
        """Into uint8[H, Wpad, 3] HBM tensors (row pitch a multiple of 16 pixels, as ``DeviceSlide`` lays levels out).
        JPEG levels on a ROCm device: the compressed file goes to HBM once and the tiles are decoded there
        (``_device_jpeg_levels``; ``device_jpeg=False`` or ``HIPAC_DEVICE_JPEG=0`` keeps the host decoder); tiles the device
        decoder does not take, and the other compressions, are decoded on host threads and copied band by band.
        LZW levels of any sample count on a ROCm device are decoded there as well (``_device_lzw_levels``; ``device_lzw=False``
        or ``HIPAC_DEVICE_LZW=0`` keeps the host decoder); malformed LZW tiles stay 0 and are reported once, as a count.
        Deflate levels (compression 8 and 32946) likewise (``_device_deflate_levels``; ``device_deflate=False`` or
        ``HIPAC_DEVICE_DEFLATE=0`` keeps ``zlib.decompress`` on host threads); tiles the device refuses, and levels whose tiles
        are larger than the device decoder takes (``deflate_level_on_device``), go to the host decoder.
        Returns a list of (tensor, width)."""
        import os

        import torch

        out = []
        use_dev = (device_jpeg if device_jpeg is not None else os.environ.get("HIPAC_DEVICE_JPEG", "1") != "0") and \
            torch.device(device).type == "cuda"
        use = list(range(self.level_count) if levels is None else levels)
        bufs = {}
        for li in use:
            lv = self.levels[li]
            bufs[li] = torch.zeros((lv.height, (lv.width + 15) // 16 * 16, 3), dtype=torch.uint8, device=device)
        on_dev = [li for li in use if use_dev and self.levels[li].compression == 7 and self.levels[li].samples == 3]
        left = dict(zip(on_dev, self._device_jpeg_levels([self.levels[li] for li in on_dev], [bufs[li] for li in on_dev]))) if on_dev else {}
        use_lzw = (device_lzw if device_lzw is not None else os.environ.get("HIPAC_DEVICE_LZW", "1") != "0") and \
            torch.device(device).type == "cuda"
        lzw_dev = [li for li in use if use_lzw and self.levels[li].compression == 5]
        use_deflate = (device_deflate if device_deflate is not None else os.environ.get("HIPAC_DEVICE_DEFLATE", "1") != "0") and \
            torch.device(device).type == "cuda"
        deflate_dev = [li for li in use if use_deflate and self.levels[li].compression in (8, 32946) and deflate_level_on_device(self.levels[li])]
        for i0 in range(0, len(deflate_dev), DEFLATE_MAX_LEVELS):  # a call takes DEFLATE_MAX_LEVELS levels
            part = deflate_dev[i0:i0 + DEFLATE_MAX_LEVELS]
            left.update(zip(part, self._device_deflate_levels([self.levels[li] for li in part], [bufs[li] for li in part])))
        host_refused = getattr(self, "lzw_refused", 0)
        refused = self._device_lzw_levels([self.levels[li] for li in lzw_dev], [bufs[li] for li in lzw_dev]) if lzw_dev else 0
        with ThreadPoolExecutor(max_workers=workers) as pool:
            for li in use:
                lv = self.levels[li]
                dev = bufs[li]
                if li in left:
                    todo = left[li]
                    for idx, t in zip(todo, pool.map(lambda i: self._decode_tile(lv, i), todo)):
                        if t is None:
                            continue
                        ty, tx = divmod(idx, lv.tiles_across)
                        y0, x0 = ty * lv.tile_h, tx * lv.tile_w
                        rows, cols = min(lv.tile_h, lv.height - y0), min(lv.tile_w, lv.width - x0)
                        dev[y0:y0 + rows, x0:x0 + cols] = torch.from_numpy(np.ascontiguousarray(t[:rows, :cols])).to(device)
                    out.append((dev, lv.width))
                    continue
                if li in lzw_dev:
                    out.append((dev, lv.width))
                    continue
                for tr in range(lv.tiles_down):
                    band = torch.from_numpy(self.read_band(li, tr, pool))
                    if dev.is_cuda:
                        band = band.pin_memory()
                    y0 = tr * lv.tile_h
                    dev[y0:y0 + band.shape[0], :lv.width].copy_(band, non_blocking=False)
                out.append((dev, lv.width))
        refused += getattr(self, "lzw_refused", 0) - host_refused
        if refused:
            print(f"{self.path}: {refused} malformed LZW tiles were not decoded and stay 0.")
        return out


def _rocm_device_present(switch: str = "HIPAC_DEVICE_LZW") -> bool:
    import os

    if os.environ.get(switch, "1") == "0":
        return False
    import torch

    return torch.cuda.is_available()


def read_mask_level(path: str, level: int) -> np.ndarray:
    """uint8[H, W] of level ``level`` of an evaluation mask, channel 0 of openslide's ``read_region((0, 0), level, dims)``
    (evaluation_FROC.py:29-30): tiled 8-bit grayscale (1 sample, the value itself), RGB or RGBA (the red sample)
    directories; compression none, deflate, LZW or JPEG.  An LZW or deflate level is decoded on the device when a ROCm device
    is present (``HIPAC_DEVICE_LZW=0`` / ``HIPAC_DEVICE_DEFLATE=0`` keep the host decoders) and channel 0 is copied back.  TiffError for a file with fewer
    than ``level + 1`` levels."""
    p = TiffPyramid(path, samples=(1, 3, 4))
    if level >= p.level_count:
        raise TiffError(f"{path} has {p.level_count} levels, level {level} was asked for")
    lv = p.levels[level]
    if (lv.compression == 5 and _rocm_device_present()) or (lv.compression in (8, 32946) and deflate_level_on_device(lv) and _rocm_device_present("HIPAC_DEVICE_DEFLATE")):
        (dev, width), = p.to_device_levels("cuda", [level])
        return dev[:, :width, 0].contiguous().cpu().numpy()
    out = np.zeros((lv.height, lv.width), np.uint8)
    for tr in range(lv.tiles_down):
        band = p.read_band(level, tr)
        out[tr * lv.tile_h:tr * lv.tile_h + band.shape[0]] = band[:, :, 0]
    return out


def _split_jpeg_tables(data: bytes) -> Tuple[bytes, bytes]:
    """A complete baseline JPEG -> (tables-only stream SOI DQT.. DHT.. EOI, abbreviated image stream without
    DQT / DHT): the two halves of TIFF's JPEGTables (tag 347) scheme, the form CAMELYON16's files use."""
    if data[:2] != b"\xff\xd8":
        raise TiffError("not a JPEG stream")
    pos, tables, rest = 2, b"", b""
    while True:
        if data[pos] != 0xFF:
            raise TiffError("JPEG marker expected")
        m = data[pos + 1]
        if m == 0xDA:  # start of scan: the entropy-coded data and EOI follow
            rest += data[pos:]
            break
        length = int.from_bytes(data[pos + 2:pos + 4], "big")
        seg = data[pos:pos + 2 + length]
        if m in (0xDB, 0xC4):
            tables += seg
        else:
            rest += seg
        pos += 2 + length
    return b"\xff\xd8" + tables + b"\xff\xd9", b"\xff\xd8" + rest


def write_tiled_tiff(path: str, levels: Sequence[np.ndarray], tile: int = 256, compression: str = "jpeg",
                     quality: int = 90, bigtiff: bool = False, missing: Sequence[Tuple[int, int, int]] = (),
                     jpeg_tables: bool = False, subsampling: int = -1, jpeg_options: Optional[dict] = None,
                     predictor: int = 1, clear_when_full: bool = True, deflate: Optional[Tuple[int, int]] = None):
    """Minimal writer of a tiled pyramid (tests and synthetic data only): ``levels`` are uint8[H,W,3]
    arrays, or uint8[H,W] for single-sample (grayscale, MinIsBlack) directories, largest first.  compression: "none" | "deflate" | "jpeg" (YCbCr; every tile a complete JPEG, or with
    ``jpeg_tables=True`` abbreviated streams plus one JPEGTables tag per directory, as real slide files have
    them).  ``missing``: (level, ty, tx) tiles written with byte count 0.  "lzw": ``lzw_encode`` streams, ``predictor`` 1 (tag 317
    absent) or 2 (horizontal differencing over the padded tile); uint8[H,W,4] levels (RGB + unassociated alpha) are
    written with 4 samples for every compression but JPEG.  ``deflate`` = (zlib level, zlib strategy) chooses the
    blocks of "deflate" -- level 0 stored, ``zlib.Z_FIXED`` fixed Huffman, otherwise dynamic -- and admits ``predictor`` 2 with
    it; None is ``zlib.compress(..., 6)`` without a predictor, exactly what the writer did before it knew the keyword."""
    from PIL import Image

    comp = {"none": 1, "deflate": 8, "jpeg": 7, "lzw": 5}[compression]
    if predictor not in (1, 2) or (predictor == 2 and comp != 5 and not (comp == 8 and deflate is not None)):
        raise TiffError("predictor 2 is written for LZW, and for deflate when deflate=(level, strategy) is given")
    bo = "<"
    blobs, ifd_specs = [], []
    pos = 16 if bigtiff else 8
    tables_of_level = []
    for li, img in enumerate(levels):
        h, w = img.shape[:2]
        ta, td = (w + tile - 1) // tile, (h + tile - 1) // tile
        offs, cnts = [], []
        level_tables = None
        for ty in range(td):
            for tx in range(ta):
                if (li, ty, tx) in missing:
                    offs.append(0), cnts.append(0)
                    continue
                t = np.zeros((tile, tile) if img.ndim == 2 else (tile, tile, img.shape[2]), np.uint8)
                part = img[ty * tile:(ty + 1) * tile, tx * tile:(tx + 1) * tile]
                t[:part.shape[0], :part.shape[1]] = part
                if comp == 1:
                    data = t.tobytes()
                elif comp in (5, 8):
                    if predictor == 2:
                        d = t.reshape(tile, tile, -1).copy()
                        d[:, 1:] -= t.reshape(tile, tile, -1)[:, :-1]
                        t = d
                    if comp == 5:
                        data = lzw_encode(t.tobytes(), clear_when_full)
                    elif deflate is None:
                        data = zlib.compress(t.tobytes(), 6)
                    else:
                        z = zlib.compressobj(deflate[0], zlib.DEFLATED, 15, 8, deflate[1])
                        data = z.compress(t.tobytes()) + z.flush()
                else:
                    bio = io.BytesIO()
                    Image.fromarray(t, "L" if img.ndim == 2 else "RGB").save(bio, "JPEG", quality=quality, subsampling=subsampling, **(jpeg_options or {}))
                    data = bio.getvalue()
                    if jpeg_tables:  # fixed quality, default Huffman tables: every tile shares one set
                        tb, data = _split_jpeg_tables(data)
                        if level_tables is not None and tb != level_tables:
                            raise TiffError("tiles of one level do not share their JPEG tables")
                        level_tables = tb
                offs.append(pos), cnts.append(len(data))
                blobs.append(data)
                pos += len(data)
        ifd_specs.append((w, h, ta * td, offs, cnts, 1 if img.ndim == 2 else img.shape[2]))
        tables_of_level.append(level_tables)
    out = bytearray()
    # data area first, then IFDs (offsets known up front)
    body = b"".join(blobs)
    ifd_pos = (16 if bigtiff else 8) + len(body)
    chunks = []
    cur = ifd_pos
    for li, (w, h, nt, offs, cnts, spp) in enumerate(ifd_specs):
        photometric = 1 if spp == 1 else 6 if comp == 7 else 2
        entries = [(254, 4, [1 if li else 0]), (256, 4, [w]), (257, 4, [h]), (258, 3, [8] * spp), (259, 3, [comp]),
                   (262, 3, [photometric]), (277, 3, [spp]), (284, 3, [1]), (322, 4, [tile]), (323, 4, [tile]),
                   (324, 16 if bigtiff else 4, offs), (325, 16 if bigtiff else 4, cnts)]
        if predictor == 2:
            entries.insert(8, (317, 3, [2]))  # Predictor, between 284 and 322: tags stay sorted
        if spp == 4:
            entries.append((338, 3, [2]))  # ExtraSamples: unassociated alpha
        if tables_of_level[li] is not None:
            entries.append((347, 7, list(tables_of_level[li])))  # JPEGTables (UNDEFINED bytes); tags stay sorted
        n = len(entries)
        esz, cw = (20, 8) if bigtiff else (12, 4)
        head = 8 if bigtiff else 2
        ifd_len = head + n * esz + cw
        extra = bytearray()
        ent_bytes = bytearray()
        for tag, typ, vals in entries:
            fmt, sz = _TYPES[typ]
            raw = struct.pack(bo + fmt * len(vals), *vals)
            ent_bytes += struct.pack(bo + "HH", tag, typ) + struct.pack(bo + ("Q" if bigtiff else "I"), len(vals))
            if len(raw) <= cw:
                ent_bytes += raw.ljust(cw, b"\0")
            else:
                ent_bytes += struct.pack(bo + ("Q" if bigtiff else "I"), cur + ifd_len + len(extra))
                extra += raw
                if len(extra) % 2:
                    extra += b"\0"
        nxt = cur + ifd_len + len(extra) if li + 1 < len(ifd_specs) else 0
        blob = (struct.pack(bo + "Q", n) if bigtiff else struct.pack(bo + "H", n)) + bytes(ent_bytes) + \
            struct.pack(bo + ("Q" if bigtiff else "I"), nxt) + bytes(extra)
        chunks.append(blob)
        cur += len(blob)
    if bigtiff:
        out += b"II" + struct.pack(bo + "HHH", 43, 8, 0) + struct.pack(bo + "Q", ifd_pos)
    else:
        out += b"II" + struct.pack(bo + "H", 42) + struct.pack(bo + "I", ifd_pos)
    out += body
    for c in chunks:
        out += c
    with open(path, "wb") as f:
        f.write(out)
