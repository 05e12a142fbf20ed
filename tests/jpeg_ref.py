"""An independent reference of the two halves of the JPEG tile encoder (csrc/jpeg.hip, image-stitcher_amd/jpegtile.py), restated
from ITU-T T.81 alone: nothing here imports jpegtile, its tables or its coder, and nothing needs a device.

* ``decode(stream)`` / ``coefficients_of(stream)``: a plain baseline decoder (Annex F) down to the QUANTISED coefficients.  The
  Huffman tables and the divisors come from the stream's own DHT / DQT segments, the geometry from SOF0 and DRI.  Every rule a
  reader may rely on is checked, and a violation raises ``StreamError`` naming the byte offset: FF is followed by 00, by the
  expected RSTm (m counting 0..7 cyclically) or by EOI; an interval's padding is all 1-bits and shorter than 8 bits; EOI follows
  the last interval and nothing follows EOI.
* ``float_coefficients(tile)``: the orthonormal float64 DCT of pixel - 128, unquantised.
* ``transform_bound(C)``: how far the integer transform with the matrix C / 2^bits can be from the float64 one, per position,
  over all blocks of [-128, 128]^64; ``rounding_excess`` holds quantised coefficients to "rounded to nearest under a transform
  this accurate": |c Q - n| <= Q / 2 + E for EVERY coefficient.
"""
from collections import namedtuple

import numpy as np


class StreamError(ValueError):
    pass


def _zigzag():
    """Natural index of the k-th coefficient of the zigzag sequence (T.81 figure 5), by walking the anti-diagonals."""
    out = []
    for d in range(15):
        cells = [(d - x, x) for x in range(8) if 0 <= d - x < 8]      # (row, column), column ascending: walking up-right
        if d % 2:
            cells.reverse()                                           # odd diagonals are walked down-left
        out += [r * 8 + c for r, c in cells]
    return np.array(out, np.int64)


ZIGZAG = _zigzag()

Decoded = namedtuple('Decoded', 'coefficients divisors height width restart_interval pads intervals block_bits')
# coefficients  int64 [block rows, block columns, 64], zigzag order, quantised (not multiplied back)
# divisors      int64 [64], zigzag order, from DQT
# pads          padding bits (0..7) of every interval
# intervals     the un-stuffed bytes of every interval
# block_bits    per interval: the bit position at which every block starts, and the interval's data bits as the last entry


def _fail(at, what):
    raise StreamError(f'byte {at}: {what}')


_LOOKUPS = {}


def _lookup(bits, vals, at):
    """Annex C: the canonical code of (BITS, HUFFVAL) as a table over the next 16 bits -> length << 8 | symbol (0: no code)."""
    key = (tuple(bits), tuple(vals))
    if key not in _LOOKUPS:
        _LOOKUPS[key] = _build_lookup(bits, vals, at)
    return _LOOKUPS[key]


def _build_lookup(bits, vals, at):
    lut = [0] * 65536
    code, k = 0, 0
    for ln in range(1, 17):
        for _ in range(bits[ln - 1]):
            if code >= 1 << ln:
                _fail(at, 'DHT: more codes than the lengths allow')
            first = code << (16 - ln)
            lut[first:first + (1 << (16 - ln))] = [ln << 8 | vals[k]] * (1 << (16 - ln))
            code += 1
            k += 1
        code <<= 1
    return lut


def _segments(s):
    """The header: -> (divisor tables, DC tables, AC tables, (h, w, table ids), restart interval, start of the entropy-coded data)."""
    if s[:2] != b'\xFF\xD8':
        _fail(0, 'no SOI')
    at = 2
    dqt, dc, ac, frame, dri = {}, {}, {}, None, 0
    while True:
        if at + 4 > len(s) or s[at] != 0xFF:
            _fail(at, 'a marker segment was expected')
        marker, n = s[at + 1], s[at + 2] << 8 | s[at + 3]
        body, end = at + 4, at + 2 + n
        if n < 2 or end > len(s):
            _fail(at, f'segment FF{marker:02X} of length {n} leaves the stream')
        p = body
        if marker == 0xDB:
            while p < end:
                if s[p] >> 4 or p + 65 > end:
                    _fail(p, 'DQT: 8-bit tables of 64 entries only')
                dqt[s[p] & 15] = np.frombuffer(s[p + 1:p + 65], np.uint8).astype(np.int64)
                if not dqt[s[p] & 15].all():
                    _fail(p, 'DQT: a divisor of 0')
                p += 65
        elif marker == 0xC4:
            while p < end:
                if p + 17 > end:
                    _fail(p, 'DHT: cut short')
                bits = list(s[p + 1:p + 17])
                vals = list(s[p + 17:p + 17 + sum(bits)])
                if len(vals) != sum(bits) or p + 17 + len(vals) > end:
                    _fail(p, 'DHT: cut short')
                (ac if s[p] >> 4 else dc)[s[p] & 15] = _lookup(bits, vals, p)
                p += 17 + len(vals)
        elif marker == 0xC0:
            if n != 11 or s[body] != 8 or s[body + 5] != 1 or s[body + 7] != 0x11:
                _fail(at, 'SOF0: one 8-bit component sampled 1 x 1 only')
            frame = (s[body + 1] << 8 | s[body + 2], s[body + 3] << 8 | s[body + 4], s[body + 6], s[body + 8])
            if not frame[0] or not frame[1]:
                _fail(at, 'SOF0: an empty frame')
        elif 0xC1 <= marker <= 0xCF:
            _fail(at, f'frame type FF{marker:02X}: baseline only')
        elif marker == 0xDD:
            if n != 4:
                _fail(at, 'DRI: length')
            dri = s[body] << 8 | s[body + 1]
        elif marker == 0xDA:
            if frame is None:
                _fail(at, 'SOS before SOF0')
            if n != 8 or s[body] != 1 or s[body + 1] != frame[2] or s[body + 3:body + 6] != b'\x00\x3F\x00':
                _fail(at, 'SOS: one component, Ss 0, Se 63, Ah Al 0 only')
            td, ta = s[body + 2] >> 4, s[body + 2] & 15
            if frame[3] not in dqt or td not in dc or ta not in ac:
                _fail(at, 'SOS names a table the stream does not define')
            return dqt[frame[3]], dc[td], ac[ta], frame, dri, end
        elif not (0xE0 <= marker <= 0xEF or marker == 0xFE):
            _fail(at, f'marker FF{marker:02X} in the header')
        at = end


def _decode_interval(data, nblocks, dc_lut, ac_lut, where):
    """The blocks of one interval's un-stuffed bytes -> ([nblocks][64] zigzag, padding bits, bit position of every block's
    start + the end).  `where(i)` is the stream offset of un-stuffed byte i."""
    nbits = 8 * len(data)
    words = np.frombuffer(data + b'\x00' * (-len(data) % 4 + 8), '>u4').tolist()
    out, starts = [], []
    pos, pred = 0, 0
    for _ in range(nblocks):
        starts.append(pos)
        blk = [0] * 64
        x = ((words[pos >> 5] << 32 | words[(pos >> 5) + 1]) >> (32 - (pos & 31))) & 0xFFFFFFFF
        e = dc_lut[x >> 16]
        ln, s = e >> 8, e & 255
        if not ln or s > 11:
            _fail(where(pos >> 3), 'no DC code matches the bits' if not ln else f'DC category {s}')
        if s:
            v = (x >> (32 - ln - s)) & ((1 << s) - 1)
            pred += v if v >> (s - 1) else v - (1 << s) + 1
        blk[0] = pred
        pos += ln + s
        k = 1
        while k < 64:
            if pos > nbits:
                break
            x = ((words[pos >> 5] << 32 | words[(pos >> 5) + 1]) >> (32 - (pos & 31))) & 0xFFFFFFFF
            e = ac_lut[x >> 16]
            ln, s = e >> 8, e & 15
            if not ln:
                _fail(where(pos >> 3), 'no AC code matches the bits')
            run = (e >> 4) & 15
            if s == 0:
                pos += ln
                if run == 15:
                    k += 16
                    if k > 63:
                        _fail(where(pos >> 3), 'ZRL runs past coefficient 63')
                    continue
                if run:
                    _fail(where(pos >> 3), f'symbol {e & 255:02X}: end-of-band runs are not baseline')
                break
            if s > 10:
                _fail(where(pos >> 3), f'AC category {s}')
            k += run
            if k > 63:
                _fail(where(pos >> 3), 'a coefficient past position 63')
            v = (x >> (32 - ln - s)) & ((1 << s) - 1)
            blk[k] = v if v >> (s - 1) else v - (1 << s) + 1
            pos += ln + s
            k += 1
        if pos > nbits:
            _fail(where(len(data) - 1) if data else where(0), 'the interval ends inside a block')
        out.append(blk)
    starts.append(pos)
    pad = nbits - pos
    if pad >= 8:
        _fail(where(pos >> 3), f'{pad} bits behind the last block of the interval')
    if pad and data[-1] & ((1 << pad) - 1) != (1 << pad) - 1:
        _fail(where(len(data) - 1), f'the {pad} padding bits are not all 1')
    return out, pad, starts


def decode(stream) -> Decoded:
    s = bytes(stream)
    divisors, dc_lut, ac_lut, (h, w, _, _), dri, start = _segments(s)
    rows, cols = -(-h // 8), -(-w // 8)
    total = rows * cols
    per = dri if dri else total
    n_int = -(-total // per)
    d = np.frombuffer(s, np.uint8)[start:]
    ff = np.flatnonzero(d == 0xFF)
    if len(ff) and ff[-1] == len(d) - 1:
        _fail(start + int(ff[-1]), 'FF ends the stream')
    after = d[ff + 1]
    marks = ff[after != 0]                      # every FF that is not stuffed: a marker
    if len(marks) != n_int:
        at = start + int(marks[min(len(marks), n_int) - 1]) if len(marks) else len(s)
        _fail(at, f'{len(marks)} markers in the entropy-coded data of {n_int} intervals')
    kinds = d[marks + 1]
    want = 0xD0 + np.arange(n_int) % 8
    want[-1] = 0xD9
    wrong = np.flatnonzero(kinds != want)
    if len(wrong):
        i = int(wrong[0])
        _fail(start + int(marks[i]), f'marker FF{int(kinds[i]):02X} behind interval {i}, FF{int(want[i]):02X} expected')
    if int(marks[-1]) + 2 != len(d):
        _fail(start + int(marks[-1]) + 2, f'{len(d) - int(marks[-1]) - 2} bytes behind EOI')
    keep = np.ones(len(d), bool)
    keep[ff[after == 0] + 1] = False            # the stuffed zeros
    index = np.flatnonzero(keep)                # position in d of every un-stuffed byte
    coefs, pads, datas, bits = [], [], [], []
    a = 0
    for i in range(n_int):
        lo, hi = np.searchsorted(index, [a, int(marks[i])])
        part = index[lo:hi]
        data = d[part].tobytes()
        where = lambda j, part=part, a=a: start + (int(part[j]) if j < len(part) else a)
        blocks, pad, starts = _decode_interval(data, min(per, total - i * per), dc_lut, ac_lut, where)
        coefs += blocks
        pads.append(pad)
        datas.append(data)
        bits.append(starts)
        a = int(marks[i]) + 2
    z = np.array(coefs, np.int64).reshape(rows, cols, 64)
    return Decoded(z, divisors, h, w, dri, pads, datas, bits)


def coefficients_of(stream) -> np.ndarray:
    """The quantised coefficients of a stream: int64 [block rows, block columns, 64] in zigzag order."""
    return decode(stream).coefficients


# ---------------------------------------------------------------------------------------------------- the transform
def dct_matrix() -> np.ndarray:
    """A[u, j] = a(u) cos((2 j + 1) u pi / 16), a(0) = sqrt(1 / 8), a(u) = 1 / 2: orthonormal."""
    u, j = np.arange(8)[:, None], np.arange(8)[None, :]
    return np.where(u == 0, np.sqrt(1 / 8), 0.5) * np.cos((2 * j + 1) * u * np.pi / 16)


def float_coefficients(tile) -> np.ndarray:
    """The float64 DCT of pixel - 128 of every 8 x 8 block, unquantised: [block rows, block columns, 64] in NATURAL order."""
    tile = np.asarray(tile)
    th, tw = tile.shape
    assert th % 8 == 0 and tw % 8 == 0
    a = dct_matrix()
    x = tile.astype(np.float64).reshape(th // 8, 8, tw // 8, 8).transpose(0, 2, 1, 3) - 128.0
    return (a @ x @ a.T).reshape(th // 8, tw // 8, 64)


def transform_bound(c, scale_bits=10) -> np.ndarray:
    """E[u, v] = 128 sum_jk |C_uj C_vk / 4^scale_bits - A_uj A_vk|: the largest distance of the integer transform C x C^T /
    4^scale_bits from the float64 one over all blocks x of [-128, 128]^64 (reached where every x_jk = +-128 has the sign of its
    term).  [64] in natural order."""
    c = np.asarray(c, np.float64)
    a = dct_matrix()
    ci = np.einsum('uj,vk->uvjk', c, c) / 4.0 ** scale_bits
    ai = np.einsum('uj,vk->uvjk', a, a)
    return (128.0 * np.abs(ci - ai).sum(axis=(2, 3))).reshape(64)


def rounding_excess(coefficients, divisors, tile, bound):
    """Holds quantised zigzag coefficients to |c Q - n| <= Q / 2 + E (+ 1e-9 for the float64 sums), none exempt; -> the largest
    (|c Q - n| - Q / 2) / E met (below 1, negative where the rounding had room to spare)."""
    n = float_coefficients(tile)[:, :, ZIGZAG]
    q = np.asarray(divisors, np.float64)
    e = np.asarray(bound, np.float64)[ZIGZAG]
    c = np.asarray(coefficients)
    assert c.shape == n.shape, f'{c.shape} coefficients of a tile with {n.shape}'
    off = np.abs(c * q - n) - q / 2
    bad = np.argwhere(off > e + 1e-9)
    assert not len(bad), (f'{len(bad)} coefficients are not the nearest multiple: first at block {tuple(bad[0][:2])} zigzag '
                          f'{bad[0][2]}: c = {c[tuple(bad[0])]}, Q = {q[bad[0][2]]}, float64 value {n[tuple(bad[0])]:.4f}')
    return float((off / e).max())
