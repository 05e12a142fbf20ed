"""The numpy definition of --composite (level choice, block means, windows, render) and a small PNG decoder that shares no
code with the package's writer.  Integers only; the device kernels and the product path must equal this."""
import struct
import zlib

import numpy as np

from image_stitcher_amd import omezarr

MAX_K = 8


def choose_level(height, width, max_side):
    """Smallest k >= 0 with max(ceil(H / 2^k), ceil(W / 2^k)) <= max_side; ValueError beyond k = 8."""
    k = 0
    while max(-(-height // 2 ** k), -(-width // 2 ** k)) > max_side:
        k += 1
    if k > MAX_K:
        raise ValueError(f"smallest max_side that works: {-(-max(height, width) // 2 ** MAX_K)}")
    return k


def block_mean(planes, k):
    """[n, H, W] -> [n, ceil(H / f), ceil(W / f)], f = 2^k: floor(sum over the block's existing pixels / their number)."""
    planes = np.asarray(planes)
    f = 1 << k
    n, h, w = planes.shape
    ho, wo = -(-h // f), -(-w // f)
    padded = np.zeros((n, ho * f, wo * f), dtype=np.int64)
    padded[:, :h, :w] = planes
    sums = padded.reshape(n, ho, f, wo, f).sum(axis=(2, 4))
    ones = np.zeros((ho * f, wo * f), dtype=np.int64)
    ones[:h, :w] = 1
    counts = ones.reshape(ho, f, wo, f).sum(axis=(1, 3))
    return (sums // counts[None]).astype(planes.dtype)


def windows_of(planes, lo, hi):
    """(a_c, b_c) = omezarr.contrast_window(bincount of all H W values of plane c, lo, hi, dtype max)."""
    planes = np.asarray(planes)
    top = int(np.iinfo(planes.dtype).max)
    return [omezarr.contrast_window(np.bincount(p.ravel(), minlength=top + 1), lo, hi, top) for p in planes]


def render(means, windows, colors):
    """[n, h, w] block means, n windows, n colours 0xRRGGBB -> RGB8 [h, w, 3]."""
    means = np.asarray(means).astype(np.int64)
    out = np.zeros(means.shape[1:] + (3,), dtype=np.int64)
    for m, (a, b), col in zip(means, windows, colors):
        v = np.where(m <= a, 0, np.where(m >= b, 255, (m - a) * 255 // (b - a)))
        for j, shift in enumerate((16, 8, 0)):
            out[..., j] += v * ((int(col) >> shift) & 0xFF) // 255
    return np.minimum(out, 255).astype(np.uint8)


def composite(planes, colors, max_side, lo=0.1, hi=99.9):
    """Source planes [n, H, W] -> (RGB8 image, k, windows)."""
    planes = np.asarray(planes)
    k = choose_level(planes.shape[1], planes.shape[2], max_side)
    windows = windows_of(planes, lo, hi)
    return render(block_mean(planes, k), windows, colors), k, windows


def decode_png(data):
    """Bytes of a non-interlaced 8-bit RGB PNG -> [h, w, 3] uint8; all five filter types; CRCs checked."""
    assert data[:8] == b'\x89PNG\r\n\x1a\n', 'signature'
    pos, idat, header, ended = 8, b'', None, False
    while pos < len(data):
        n, kind = struct.unpack('>I4s', data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        crc, = struct.unpack('>I', data[pos + 8 + n:pos + 12 + n])
        assert crc == (zlib.crc32(kind + body) & 0xFFFFFFFF), kind
        pos += 12 + n
        if kind == b'IHDR':
            header = struct.unpack('>IIBBBBB', body)
        elif kind == b'IDAT':
            idat += body
        elif kind == b'IEND':
            ended = True
            break
    assert header is not None and ended and pos == len(data)
    w, h, depth, ctype, comp, flt, interlace = header
    assert (depth, ctype, comp, flt, interlace) == (8, 2, 0, 0, 0), header
    raw = zlib.decompress(idat)
    stride, bpp = 3 * w, 3
    assert len(raw) == h * (stride + 1)
    out = np.zeros((h, stride), dtype=np.uint8)
    prev = bytearray(stride)
    for y in range(h):
        ft = raw[y * (stride + 1)]
        line = bytearray(raw[y * (stride + 1) + 1:(y + 1) * (stride + 1)])
        for i in range(stride):
            a = line[i - bpp] if i >= bpp else 0
            b = prev[i]
            c = prev[i - bpp] if i >= bpp else 0
            if ft == 0:
                pred = 0
            elif ft == 1:
                pred = a
            elif ft == 2:
                pred = b
            elif ft == 3:
                pred = (a + b) // 2
            elif ft == 4:
                p = a + b - c
                pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
                pred = a if (pa <= pb and pa <= pc) else (b if pb <= pc else c)
            else:
                raise AssertionError(f'filter type {ft}')
            line[i] = (line[i] + pred) & 0xFF
        out[y] = np.frombuffer(bytes(line), dtype=np.uint8)
        prev = line
    return out.reshape(h, w, 3)
