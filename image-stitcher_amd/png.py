"""A package-free PNG writer for the composite quick-look pictures: 8-bit RGB, non-interlaced, ``zlib`` and ``struct`` only."""
from __future__ import annotations

import struct
import zlib

import numpy as np

SIGNATURE = b'\x89PNG\r\n\x1a\n'


def _chunk(kind: bytes, data: bytes) -> bytes:
    return struct.pack('>I', len(data)) + kind + data + struct.pack('>I', zlib.crc32(kind + data) & 0xFFFFFFFF)


def encode_rgb8(image, level: int = 1) -> bytes:
    """``image`` [h, w, 3] uint8 -> the bytes of an 8-bit RGB PNG (colour type 2, filter type 0 on every row, one IDAT).
    zlib level 1: a 4096-pixel picture is tens of MB of pixels, and a quick look is wanted quickly."""
    a = np.asarray(image)
    if a.ndim != 3 or a.shape[2] != 3 or a.dtype != np.uint8 or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError(f"expected a uint8 [h, w, 3] image with h, w >= 1, got {a.dtype} {a.shape}")
    h, w = int(a.shape[0]), int(a.shape[1])
    rows = np.zeros((h, 1 + 3 * w), dtype=np.uint8)      # every row is led by its filter type (0: none)
    rows[:, 1:] = a.reshape(h, 3 * w)
    ihdr = struct.pack('>IIBBBBB', w, h, 8, 2, 0, 0, 0)
    return SIGNATURE + _chunk(b'IHDR', ihdr) + _chunk(b'IDAT', zlib.compress(rows.tobytes(), level)) + _chunk(b'IEND', b'')


def write_rgb8(path: str, image, level: int = 1) -> str:
    data = encode_rgb8(image, level)
    with open(path, 'wb') as fh:
        fh.write(data)
    return path
