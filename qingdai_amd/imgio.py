"""
qingdai_amd/imgio.py -- 8-bit RGB PNG files with the standard library (zlib + struct), for the true-colour frames.

write_png writes colour type 2, bit depth 8, no interlace, every scanline with filter 0; read_png reads such files back (and any
8-bit RGB, non-interlaced PNG, undoing the five scanline filters), for the tests.
"""
from __future__ import annotations

import struct
import zlib

import numpy as np

_SIG = b"\x89PNG\r\n\x1a\n"


def _chunk(tag, data):
    return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)


def write_png(path, img):
    """img: uint8 [h, w, 3], row 0 at the top."""
    a = np.asarray(img)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3 or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError(f"write_png: expected uint8 [h, w, 3], got {a.dtype} {a.shape}")
    h, w = a.shape[:2]
    rows = np.zeros((h, 1 + 3 * w), dtype=np.uint8)            # filter byte 0 in front of every scanline
    rows[:, 1:] = a.reshape(h, 3 * w)
    data = (_SIG + _chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0)) +
            _chunk(b"IDAT", zlib.compress(rows.tobytes(), 6)) + _chunk(b"IEND", b""))
    with open(path, "wb") as f:
        f.write(data)


def read_png(path):
    """-> uint8 [h, w, 3] of an 8-bit RGB, non-interlaced PNG."""
    with open(path, "rb") as f:
        raw = f.read()
    if raw[:8] != _SIG:
        raise ValueError(f"read_png: '{path}' is not a PNG file")
    pos, idat, hdr = 8, [], None
    while pos + 8 <= len(raw):
        n, tag = struct.unpack(">I4s", raw[pos:pos + 8])
        body = raw[pos + 8:pos + 8 + n]
        if struct.unpack(">I", raw[pos + 8 + n:pos + 12 + n])[0] != (zlib.crc32(tag + body) & 0xFFFFFFFF):
            raise ValueError(f"read_png: bad CRC in chunk {tag!r}")
        if tag == b"IHDR":
            hdr = struct.unpack(">IIBBBBB", body)
        elif tag == b"IDAT":
            idat.append(body)
        elif tag == b"IEND":
            break
        pos += 12 + n
    if hdr is None or hdr[2:] != (8, 2, 0, 0, 0):
        raise ValueError("read_png: only 8-bit RGB, non-interlaced files are supported")
    w, h = hdr[:2]
    stride = 3 * w
    flat = np.frombuffer(zlib.decompress(b"".join(idat)), dtype=np.uint8)
    if flat.size != h * (stride + 1):
        raise ValueError("read_png: image data has the wrong length")
    lines = flat.reshape(h, stride + 1)
    out = np.zeros((h, stride), dtype=np.uint8)
    prev = np.zeros(stride, dtype=np.int64)
    for y in range(h):
        ft, x = int(lines[y, 0]), lines[y, 1:].astype(np.int64)
        if ft == 0:
            cur = x
        elif ft == 2:
            cur = (x + prev) & 255
        elif ft in (1, 3, 4):
            cur = np.zeros(stride, dtype=np.int64)
            for i in range(stride):
                a = cur[i - 3] if i >= 3 else 0
                b = prev[i]
                c = prev[i - 3] if i >= 3 else 0
                if ft == 1:
                    p = a
                elif ft == 3:
                    p = (a + b) // 2
                else:
                    pa, pb, pc = abs(b - c), abs(a - c), abs(a + b - 2 * c)
                    p = a if (pa <= pb and pa <= pc) else (b if pb <= pc else c)
                cur[i] = (x[i] + p) & 255
        else:
            raise ValueError(f"read_png: unknown filter type {ft}")
        out[y] = cur
        prev = cur
    return out.reshape(h, w, 3)
