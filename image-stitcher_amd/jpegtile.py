"""The baseline JPEG stream of one TIFF tile (TIFF Compression 7), stated in numpy: include/squidstitch.h (sq_jpeg_encode_planes)
and DESIGN 5.4p in executable form.  The package needs it for the shared zero-tile stream and for ``PyramidTiff.append_planes``
(the host path); nothing hot runs through it.  It is also the definition the device encoder (csrc/jpeg.hip) is held to, byte for
byte.

A tile of tile_h x tile_w uint8 elements (sides multiples of 8) is one self-contained ITU-T T.81 baseline stream:

    SOI | DQT (table 0) | SOF0 (8 bit, one component, 1 x 1) | DHT (DC 0, AC 0) | DRI (tile_w / 8) | SOS | data | EOI

* one quantisation table: Annex K.1 luminance scaled by libjpeg's quality rule;
* the fixed Annex K.3.3 luminance Huffman tables;
* one restart interval per row of blocks, padded with 1-bits to a byte, RSTm (m mod 8) between intervals, none after the last;
  the DC prediction starts at 0 in every interval;
* FF 00 for every FF of the entropy-coded data;
* the forward transform in integers: x = pixel - 128, N = C x C^T with C = DCT_MATRIX (round(2^10 a(u) cos((2j + 1) u pi / 16)),
  no intermediate rounding), coefficient = sign(N) ((|N| + D / 2) // D) with D = Q 2^20.  |N| <= 128 * 2896^2 < 2^30 and
  D / 2 <= 255 * 2^19 < 2^27: everything fits 32 bits.
"""
from __future__ import annotations

import numpy as np

DCT_SCALE_BITS = 10
# C[u][j] = round(2^10 a(u) cos((2 j + 1) u pi / 16)), a(0) = sqrt(1 / 8), a(u) = 1 / 2: 64 literal integers
DCT_MATRIX = np.array([
    [362, 362, 362, 362, 362, 362, 362, 362],
    [502, 426, 284, 100, -100, -284, -426, -502],
    [473, 196, -196, -473, -473, -196, 196, 473],
    [426, -100, -502, -284, 284, 502, 100, -426],
    [362, -362, -362, 362, 362, -362, -362, 362],
    [284, -502, 100, 426, -426, -100, 502, -284],
    [196, -473, 473, -196, -196, 473, -473, 196],
    [100, -284, 426, -502, 502, -426, 284, -100]], dtype=np.int64)

# Annex K.1, luminance, natural (row-major) order
BASE_TABLE = np.array([
    16, 11, 10, 16, 24, 40, 51, 61,
    12, 12, 14, 19, 26, 58, 60, 55,
    14, 13, 16, 24, 40, 57, 69, 56,
    14, 17, 22, 29, 51, 87, 80, 62,
    18, 22, 37, 56, 68, 109, 103, 77,
    24, 35, 55, 64, 81, 104, 113, 92,
    49, 64, 78, 87, 103, 121, 120, 101,
    72, 92, 95, 98, 112, 100, 103, 99], dtype=np.int64)

# ZIGZAG[k] = natural index of the k-th coefficient in zigzag order
ZIGZAG = np.array([
    0, 1, 8, 16, 9, 2, 3, 10,
    17, 24, 32, 25, 18, 11, 4, 5,
    12, 19, 26, 33, 40, 48, 41, 34,
    27, 20, 13, 6, 7, 14, 21, 28,
    35, 42, 49, 56, 57, 50, 43, 36,
    29, 22, 15, 23, 30, 37, 44, 51,
    58, 59, 52, 45, 38, 31, 39, 46,
    53, 60, 61, 54, 47, 55, 62, 63], dtype=np.int64)

# Annex K.3.3: number of codes of each length 1..16, then the symbols in code order
DC_BITS = (0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0)
DC_VALS = tuple(range(12))
AC_BITS = (0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7D)
AC_VALS = (
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07,
    0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xA1, 0x08, 0x23, 0x42, 0xB1, 0xC1, 0x15, 0x52, 0xD1, 0xF0,
    0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0A, 0x16, 0x17, 0x18, 0x19, 0x1A, 0x25, 0x26, 0x27, 0x28,
    0x29, 0x2A, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49,
    0x4A, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69,
    0x6A, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7A, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89,
    0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9A, 0xA2, 0xA3, 0xA4, 0xA5, 0xA6, 0xA7,
    0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4, 0xB5, 0xB6, 0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3, 0xC4, 0xC5,
    0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xD2, 0xD3, 0xD4, 0xD5, 0xD6, 0xD7, 0xD8, 0xD9, 0xDA, 0xE1, 0xE2,
    0xE3, 0xE4, 0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF1, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8,
    0xF9, 0xFA)

HEADER_BYTES = 2 + (2 + 67) + (2 + 11) + (2 + 2 + 29 + 179) + (2 + 4) + (2 + 8)      # SOI .. SOS: 312
DEFAULT_QUALITY = 90
# T.81 holds sides below 65536; libjpeg (JPEG_MAX_DIMENSION 65500), the decoder behind nearly every TIFF reader, refuses larger ones
MAX_SIDE = 65496
EOB, ZRL = 0x00, 0xF0


def check_quality(quality) -> int:
    q = int(quality)
    if q != quality or not 1 <= q <= 100:
        raise ValueError(f"JPEG quality must be an integer in 1..100, got {quality!r}")
    return q


def quant_table(quality: int) -> np.ndarray:
    """The 64 divisors in NATURAL order: libjpeg's jpeg_quality_scaling and jpeg_add_quant_table (baseline: 1..255)."""
    q = check_quality(quality)
    s = 5000 // q if q < 50 else 200 - 2 * q
    return np.clip((BASE_TABLE * s + 50) // 100, 1, 255)


def _canonical(bits, vals):
    """-> (code[256], length[256]) of the canonical Huffman code of Annex C (0 length: no code)."""
    code = np.zeros(256, np.int64)
    length = np.zeros(256, np.int64)
    c, k = 0, 0
    for ln in range(1, 17):
        for _ in range(bits[ln - 1]):
            code[vals[k]], length[vals[k]] = c, ln
            c += 1
            k += 1
        c <<= 1
    return code, length


DC_CODE, DC_LEN = _canonical(DC_BITS, DC_VALS)
AC_CODE, AC_LEN = _canonical(AC_BITS, AC_VALS)


def header(tile_h: int, tile_w: int, quality: int) -> bytes:
    """SOI .. SOS of a tile: HEADER_BYTES bytes."""
    th, tw = int(tile_h), int(tile_w)
    if th < 8 or tw < 8 or th % 8 or tw % 8 or th > MAX_SIDE or tw > MAX_SIDE:
        raise ValueError(f"JPEG tile sides must be multiples of 8 in 8..{MAX_SIDE}, got {th} x {tw}")
    q = quant_table(quality)
    be16 = lambda v: bytes((v >> 8, v & 255))
    out = b'\xFF\xD8'
    out += b'\xFF\xDB' + be16(67) + b'\x00' + bytes(int(v) for v in q[ZIGZAG])
    out += b'\xFF\xC0' + be16(11) + b'\x08' + be16(th) + be16(tw) + b'\x01' + b'\x01\x11\x00'
    out += (b'\xFF\xC4' + be16(2 + 29 + 179) + b'\x00' + bytes(DC_BITS) + bytes(DC_VALS)
            + b'\x10' + bytes(AC_BITS) + bytes(AC_VALS))
    out += b'\xFF\xDD' + be16(4) + be16(tw // 8)
    out += b'\xFF\xDA' + be16(8) + b'\x01' + b'\x01\x00' + b'\x00\x3F\x00'
    assert len(out) == HEADER_BYTES
    return out


def quantised_blocks(tile: np.ndarray, quality: int) -> np.ndarray:
    """The coefficients of every 8 x 8 block in zigzag order: int64 [block rows, block columns, 64]."""
    tile = np.asarray(tile)
    if tile.dtype != np.uint8 or tile.ndim != 2:
        raise ValueError(f"a JPEG tile is a 2-D uint8 array, got {tile.dtype} {tile.shape}")
    th, tw = tile.shape
    x = tile.astype(np.int64).reshape(th // 8, 8, tw // 8, 8).transpose(0, 2, 1, 3) - 128
    n = DCT_MATRIX @ x @ DCT_MATRIX.T
    d = quant_table(quality).reshape(8, 8) << (2 * DCT_SCALE_BITS)
    c = np.sign(n) * ((np.abs(n) + d // 2) // d)
    return c.reshape(th // 8, tw // 8, 64)[:, :, ZIGZAG]


def _bit_length(v: np.ndarray) -> np.ndarray:
    out = np.zeros(v.shape, np.int64)
    v = v.copy()
    while True:
        nz = v > 0
        if not nz.any():
            return out
        out += nz
        v >>= 1


def _items(z: np.ndarray):
    """(interval, value, bits) of every Huffman code + magnitude of the blocks z [rows, cols, 64], in stream order."""
    rows, cols, _ = z.shape
    nb = rows * cols
    zf = z.reshape(nb, 64)
    stride = 65 * 4          # keys of a block: 4 k + (0..2: ZRLs before coefficient k, 3: the coefficient); k = 64: EOB
    # DC differences, the prediction restarting in every interval (row of blocks)
    dc = z[:, :, 0]
    diff = (dc - np.concatenate([np.zeros((rows, 1), np.int64), dc[:, :-1]], axis=1)).reshape(nb)
    s = _bit_length(np.abs(diff))
    mag = np.where(diff < 0, diff + (1 << s) - 1, diff)
    keys = [np.arange(nb) * stride + 3]
    vals = [(DC_CODE[s] << s) | mag]
    lens = [DC_LEN[s] + s]
    # AC coefficients: run of zeros before each, in units of ZRL (16 zeros) and the rest
    b, k = np.nonzero(zf[:, 1:])
    k = k + 1
    c = zf[b, k]
    first = np.ones(len(b), bool)
    first[1:] = b[1:] != b[:-1]
    prev = np.where(first, 0, np.concatenate([[0], k[:-1]]))
    run = k - prev - 1
    s = _bit_length(np.abs(c))
    mag = np.where(c < 0, c + (1 << s) - 1, c)
    sym = ((run & 15) << 4) | s
    keys.append(b * stride + 4 * k + 3)
    vals.append((AC_CODE[sym] << s) | mag)
    lens.append(AC_LEN[sym] + s)
    nzrl = run >> 4
    at = np.repeat(np.arange(len(b)), nzrl)
    sub = np.arange(len(at)) - np.repeat(np.cumsum(nzrl) - nzrl, nzrl)
    keys.append(b[at] * stride + 4 * k[at] + sub)
    vals.append(np.full(len(at), AC_CODE[ZRL]))
    lens.append(np.full(len(at), AC_LEN[ZRL]))
    # EOB unless coefficient 63 is coded
    eob = np.nonzero(zf[:, 63] == 0)[0]
    keys.append(eob * stride + 4 * 64)
    vals.append(np.full(len(eob), AC_CODE[EOB]))
    lens.append(np.full(len(eob), AC_LEN[EOB]))
    keys, vals, lens = np.concatenate(keys), np.concatenate(vals), np.concatenate(lens)
    order = np.argsort(keys, kind='stable')
    keys, vals, lens = keys[order], vals[order], lens[order]
    return (keys // stride) // cols, vals, lens


def entropy_intervals(z: np.ndarray) -> list:
    """The entropy-coded bytes of every restart interval of the blocks z, padded with 1-bits and stuffed."""
    rows = z.shape[0]
    interval, vals, lens = _items(z)
    shift = lens[:, None] - 1 - np.arange(32)[None, :]
    bits = ((vals[:, None] >> np.maximum(shift, 0)) & 1).astype(np.uint8)[shift >= 0]
    ends = np.cumsum(np.bincount(interval, weights=lens, minlength=rows).astype(np.int64))
    out = []
    for r in range(rows):
        part = bits[ends[r - 1] if r else 0:ends[r]]
        data = np.packbits(np.concatenate([part, np.ones(-len(part) % 8, np.uint8)]))
        ff = np.nonzero(data == 0xFF)[0]
        out.append(np.insert(data, ff + 1, 0).tobytes())
    return out


def encode_tile(tile: np.ndarray, quality: int = DEFAULT_QUALITY) -> bytes:
    """The whole stream of a full tile (uint8 [tile_h, tile_w], sides multiples of 8)."""
    tile = np.asarray(tile)
    th, tw = tile.shape
    head = header(th, tw, quality)
    parts = [head]
    for r, data in enumerate(entropy_intervals(quantised_blocks(tile, quality))):
        if r:
            parts.append(bytes((0xFF, 0xD0 + (r - 1) % 8)))
        parts.append(data)
    parts.append(b'\xFF\xD9')
    return b''.join(parts)


def decode_tile(stream: bytes) -> np.ndarray:
    """A tile stream decoded by Pillow (the reader of the tests; any JPEG decoder reads these streams)."""
    try:
        from PIL import Image
    except ImportError as exc:      # the writer does not need it
        raise RuntimeError("reading JPEG-compressed TIFF tiles needs Pillow, which is not installed") from exc
    import io
    with Image.open(io.BytesIO(stream)) as im:
        if im.mode != 'L':
            raise ValueError(f"expected a grey JPEG tile, got mode {im.mode}")
        return np.asarray(im, dtype=np.uint8).copy()
