"""Minimal PNG writer on the standard library (zlib, struct): 8-bit grey, 8-bit RGB and 8-bit palette images, rows top
to bottom, no interlace, filter type 0 on every row.  The export path writes the bytes the export kernels produce, so
what a viewer shows is exactly those bytes; matplotlib and PIL are not needed anywhere in the product path."""
import struct
import zlib

import numpy as np

_SIGNATURE = b"\x89PNG\r\n\x1a\n"
GREY, RGB, PALETTE = 0, 2, 3                 # PNG colour types


def _chunk(kind, payload):
    return struct.pack(">I", len(payload)) + kind + payload + struct.pack(">I", zlib.crc32(kind + payload) & 0xFFFFFFFF)


def encode(pixels, palette=None, level=6):
    """pixels: (H, W) uint8 (grey, or palette indices when `palette` (n <= 256, 3) uint8 is given) or (H, W, 3) uint8
    (RGB) -> the bytes of the PNG file."""
    a = np.asarray(pixels)
    if a.dtype != np.uint8:
        raise ValueError("png: pixels must be uint8 (got %s)" % a.dtype)
    if a.ndim == 2:
        ctype = PALETTE if palette is not None else GREY
    elif a.ndim == 3 and a.shape[2] == 3 and palette is None:
        ctype = RGB
    else:
        raise ValueError("png: expected (H, W) or (H, W, 3) pixels, got shape %s" % (a.shape,))
    H, W = a.shape[:2]
    if H < 1 or W < 1:
        raise ValueError("png: empty image")
    chunks = [_chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, ctype, 0, 0, 0))]
    if ctype == PALETTE:
        pal = np.asarray(palette)
        if pal.dtype != np.uint8 or pal.ndim != 2 or pal.shape[1] != 3 or not 1 <= pal.shape[0] <= 256:
            raise ValueError("png: the palette must be (1..256, 3) uint8")
        if int(a.max()) >= pal.shape[0]:
            raise ValueError("png: index %d outside the palette of %d entries" % (int(a.max()), pal.shape[0]))
        chunks.append(_chunk(b"PLTE", np.ascontiguousarray(pal).tobytes()))
    rows = np.ascontiguousarray(a).reshape(H, -1)
    raw = np.zeros((H, rows.shape[1] + 1), dtype=np.uint8)           # a filter-type byte (0 = none) in front of each row
    raw[:, 1:] = rows
    chunks.append(_chunk(b"IDAT", zlib.compress(raw.tobytes(), level)))
    chunks.append(_chunk(b"IEND", b""))
    return _SIGNATURE + b"".join(chunks)


def save(path, pixels, palette=None, level=6):
    data = encode(pixels, palette=palette, level=level)
    with open(path, "wb") as f:
        f.write(data)


def decode(data):
    """The inverse for files of this writer's subset (8 bit, colour types 0 / 2 / 3, no interlace; all five row filters
    are undone) -> (pixels, palette or None).  Meant for tests and quick inspection."""
    if data[:8] != _SIGNATURE:
        raise ValueError("png: bad signature")
    pos, idat, palette, header = 8, [], None, None
    while pos < len(data):
        n, kind = struct.unpack(">I4s", data[pos:pos + 8])
        payload = data[pos + 8:pos + 8 + n]
        if struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])[0] != (zlib.crc32(kind + payload) & 0xFFFFFFFF):
            raise ValueError("png: CRC mismatch in %r" % kind)
        pos += 12 + n
        if kind == b"IHDR":
            header = struct.unpack(">IIBBBBB", payload)
        elif kind == b"PLTE":
            palette = np.frombuffer(payload, dtype=np.uint8).reshape(-1, 3).copy()
        elif kind == b"IDAT":
            idat.append(payload)
        elif kind == b"IEND":
            break
    W, H, depth, ctype, _, _, interlace = header
    if depth != 8 or ctype not in (GREY, RGB, PALETTE) or interlace:
        raise ValueError("png: only 8-bit grey / RGB / palette without interlace")
    bpp = 3 if ctype == RGB else 1
    stride = W * bpp
    raw = np.frombuffer(zlib.decompress(b"".join(idat)), dtype=np.uint8).reshape(H, stride + 1)
    out = np.zeros((H, stride), dtype=np.uint8)
    for y in range(H):
        ft, line = int(raw[y, 0]), raw[y, 1:].astype(np.int32)
        up = out[y - 1].astype(np.int32) if y else np.zeros(stride, dtype=np.int32)
        if ft == 0:
            cur = line
        elif ft == 2:
            cur = line + up
        else:
            cur = np.zeros(stride, dtype=np.int32)
            for i in range(stride):
                left = cur[i - bpp] if i >= bpp else 0
                ul = up[i - bpp] if i >= bpp else 0
                if ft == 1:
                    pred = left
                elif ft == 3:
                    pred = (left + up[i]) // 2
                elif ft == 4:
                    p = left + up[i] - ul
                    pa, pb, pc = abs(p - left), abs(p - up[i]), abs(p - ul)
                    pred = left if pa <= pb and pa <= pc else (up[i] if pb <= pc else ul)
                else:
                    raise ValueError("png: unknown filter %d" % ft)
                cur[i] = (line[i] + pred) & 0xFF
        out[y] = cur & 0xFF
    return (out.reshape(H, W, 3) if ctype == RGB else out.reshape(H, W)), palette


def load(path):
    with open(path, "rb") as f:
        return decode(f.read())
