"""numpy restatement of the tile streams csrc/deflate.hip writes (include/squidstitch.h, sq_deflate_encode_planes): the rules,
one function each -- predictor, run finding, code lengths with their limit, the block header, Adler-32.  The kernel need not match
these bytes (any valid stream of the same tile is right); tests/test_deflate_cpu.py checks this file against Python's zlib."""
import numpy as np

SEG = 16384
ADLER = 65521
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)


def predict(tile: np.ndarray, predictor: int) -> np.ndarray:
    """TIFF Predictor 2 on a [tile_h, tile_w] uint8 / uint16 tile: every element but the first of a row becomes its difference to
    the element on its left, modulo 2^bits.  Predictor 1: unchanged."""
    if predictor == 1:
        return tile.copy()
    if predictor != 2:
        raise ValueError(f"predictor {predictor}")
    out = tile.copy()
    out[:, 1:] = tile[:, 1:] - tile[:, :-1]      # (unsigned arithmetic wraps)
    return out


def tile_bytes(plane: np.ndarray, ty: int, tx: int, th: int, tw: int, predictor: int) -> bytes:
    """The little-endian bytes a stream encodes: tile (ty, tx) of the plane, zero past the plane's edge, predicted."""
    full = np.zeros((th, tw), plane.dtype)
    part = plane[ty * th:(ty + 1) * th, tx * tw:(tx + 1) * tw]
    full[:part.shape[0], :part.shape[1]] = part
    return predict(full, predictor).astype(plane.dtype.newbyteorder('<')).tobytes()


def unpredict(tile: np.ndarray, predictor: int) -> np.ndarray:
    return tile if predictor == 1 else np.cumsum(tile, axis=1, dtype=tile.dtype)


def adler_sums(seg: bytes):
    """(sum of the bytes, sum of (n - i) * byte i) mod 65521: what one segment contributes."""
    b = np.frombuffer(seg, np.uint8).astype(np.int64)
    n = len(b)
    return int(b.sum() % ADLER), int((b * (n - np.arange(n))).sum() % ADLER)


def adler_combine(parts) -> int:
    """Adler-32 of the concatenation from [(length, s1, s2)] of the segments."""
    a, b = 1, 0
    for n, s1, s2 in parts:
        b = (b + n * a + s2) % ADLER
        a = (a + s1) % ADLER
    return (b << 16) | a


def tokens(seg: bytes, esz: int):
    """Element runs only: [('lit', byte) | ('run', length in bytes)] of one segment.  An element that equals the one before it
    continues a run; a run is cut from its start into pieces of at most 258 bytes, a piece shorter than 3 bytes is literals.  The
    distance of every match is the element size."""
    el = np.frombuffer(seg, np.uint8).reshape(-1, esz)
    nel = len(el)
    eq = np.zeros(nel + 1, bool)
    eq[1:nel] = (el[1:] == el[:-1]).all(axis=1)
    m = 258 // esz
    out, i = [], 0
    while i < nel:
        if not eq[i]:
            out += [('lit', int(v)) for v in el[i]]
            i += 1
            continue
        e = i
        while eq[e]:
            e += 1
        while i < e:
            piece = min(m, e - i)
            if piece * esz >= 3:
                out.append(('run', piece * esz))
            else:
                out += [('lit', int(v)) for k in range(piece) for v in el[i + k]]
            i += piece
    return out


def length_symbol(length: int):
    """Match length 3..258 -> (symbol 257..285, extra bits, their value) (RFC 1951 3.2.5)."""
    if length == 258:
        return 285, 0, 0
    l = length - 3
    if l < 8:
        return 257 + l, 0, 0
    eb = l.bit_length() - 3
    return 257 + 4 * (eb + 1) + ((l >> eb) & 3), eb, l & ((1 << eb) - 1)


def huffman_lengths(counts, limit: int = 15):
    """Code lengths of the symbols with a non-zero count (at least two of them): the minimum-redundancy code of the counts sorted by
    (count, symbol), then the limit -- every length above ``limit`` is counted at ``limit``, and while the Kraft sum exceeds 1 one
    code leaves ``limit`` and the deepest code above it is split in two; the least frequent symbols take the longest codes.
    ``limit=None``: the unlimited code."""
    used = sorted((int(c), s) for s, c in enumerate(counts) if c)
    n = len(used)
    if n < 2:
        raise ValueError("a block has at least two symbols (end of block and one more)")
    a = [c for c, _ in used]
    a[0] += a[1]
    root, leaf = 0, 2
    for nxt in range(1, n - 1):
        if leaf >= n or a[root] < a[leaf]:
            a[nxt] = a[root]
            a[root] = nxt
            root += 1
        else:
            a[nxt] = a[leaf]
            leaf += 1
        if leaf >= n or (root < nxt and a[root] < a[leaf]):
            a[nxt] += a[root]
            a[root] = nxt
            root += 1
        else:
            a[nxt] += a[leaf]
            leaf += 1
    a[n - 2] = 0
    for nxt in range(n - 3, -1, -1):
        a[nxt] = a[a[nxt]] + 1
    depths = []                 # of the leaves, most frequent first
    avbl, use, dpth, root = 1, 0, 0, n - 2
    while avbl > 0:
        while root >= 0 and a[root] == dpth:
            use += 1
            root -= 1
        while avbl > use:
            depths.append(dpth)
            avbl -= 1
        avbl, dpth, use = 2 * use, dpth + 1, 0
    if limit is not None:
        bl = [0] * (limit + 1)
        for d in depths:
            bl[min(d, limit)] += 1
        total = sum(bl[l] << (limit - l) for l in range(1, limit + 1))
        while total > 1 << limit:
            bl[limit] -= 1
            for l in range(limit - 1, 0, -1):
                if bl[l]:
                    bl[l] -= 1
                    bl[l + 1] += 2
                    break
            total -= 1
        depths = [l for l in range(1, limit + 1) for _ in range(bl[l])]
    lengths = [0] * len(counts)
    for (_, s), d in zip(reversed(used), depths):      # depths ascend: the most frequent symbol first
        lengths[s] = d
    return lengths


def canonical_codes(lengths):
    """RFC 1951 3.2.2: codes of equal length ascend with the symbol."""
    top = max(lengths)
    bl = [0] * (top + 2)
    for l in lengths:
        if l:
            bl[l] += 1
    nxt, code = [0] * (top + 2), 0
    for l in range(1, top + 1):
        code = (code + bl[l - 1]) << 1
        nxt[l] = code
    out = [0] * len(lengths)
    for s, l in enumerate(lengths):
        if l:
            out[s] = nxt[l]
            nxt[l] += 1
    return out


class BitWriter:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def bits(self, value: int, count: int):       # LSB first (header fields, extra bits)
        self.acc |= value << self.n
        self.n += count
        while self.n >= 8:
            self.out.append(self.acc & 0xFF)
            self.acc >>= 8
            self.n -= 8

    def code(self, code: int, length: int):       # Huffman codes go out from their most significant bit
        self.bits(int(format(code, f'0{length}b')[::-1], 2), length)

    def align(self):
        if self.n:
            self.bits(0, 8 - self.n)


def dynamic_block(seg: bytes, esz: int, final: bool) -> bytes:
    """One segment as a dynamic-Huffman block; a non-final one ends with an empty stored block (a sync flush)."""
    toks = tokens(seg, esz)
    counts = [0] * 286
    counts[256] = 1
    for kind, v in toks:
        counts[v if kind == 'lit' else length_symbol(v)[0]] += 1
    lengths = huffman_lengths(counts)
    codes = canonical_codes(lengths)
    nlit = max(257, max(s for s, l in enumerate(lengths) if l) + 1)
    dist = [1] if esz == 1 else [0, 1]            # the one distance symbol (distance = element size): one bit, code 0
    w = BitWriter()
    w.bits(1 if final else 0, 1)
    w.bits(2, 2)
    w.bits(nlit - 257, 5)
    w.bits(len(dist) - 1, 5)
    w.bits(15, 4)                                  # all 19 lengths of the code-length code follow
    for s in CL_ORDER:
        w.bits(4 if s < 16 else 0, 3)              # the trivial one: 4-bit codes for the lengths 0..15, no repeat codes
    for l in lengths[:nlit] + dist:
        w.code(l, 4)
    for kind, v in toks:
        if kind == 'lit':
            w.code(codes[v], lengths[v])
        else:
            s, eb, ev = length_symbol(v)
            w.code(codes[s], lengths[s])
            w.bits(ev, eb)
            w.bits(0, 1)
    w.code(codes[256], lengths[256])
    if not final:
        w.bits(0, 3)
        w.align()
        w.out += b'\x00\x00\xff\xff'
    w.align()
    return bytes(w.out)


def stored_block(seg: bytes, final: bool) -> bytes:
    n = len(seg)
    return bytes([1 if final else 0, n & 0xFF, n >> 8, ~n & 0xFF, (~n >> 8) & 0xFF]) + seg


def header_bytes() -> int:
    """What coding a segment on its own may cost over one block of the whole stream: its header -- "about 170 bytes" with the
    trivial code-length code (17 + 57 bits, then 4 bits for each of up to 286 + 2 code lengths: 154 bytes, where zlib's own
    header with repeat codes takes a few dozen) -- and the sync flush that ends it (3 bits, padding, 4 bytes: at most 5).
    The round figure, not the exact 154 + 5, because element runs also pay where byte runs do not: the first element of a run of
    16-bit elements is two literals, Z_RLE's first byte one (a 128 x 128 tile of one uint16 value under predictor 2: 590 bytes
    here, 263 from Z_RLE, two segments -- 9 bytes more than the exact header figure would allow)."""
    return 170 + 5


def compress_tile(data: bytes, esz: int, seg: int = SEG) -> bytes:
    """The zlib stream of one tile's (predicted) bytes; b'' for a tile of zeros."""
    if not any(data):
        return b''
    out, parts = bytearray(b'\x78\x01'), []
    for at in range(0, len(data), seg):
        s = data[at:at + seg]
        final = at + seg >= len(data)
        blk = dynamic_block(s, esz, final)
        out += blk if len(blk) < len(s) + 5 else stored_block(s, final)
        parts.append((len(s),) + adler_sums(s))
    return bytes(out) + adler_combine(parts).to_bytes(4, 'big')


def block_kinds(data: bytes, esz: int, seg: int = SEG) -> str:
    """'S' (stored) or 'D' (dynamic) for every segment of a tile's bytes, by compress_tile's rule."""
    return ''.join('D' if len(dynamic_block(data[at:at + seg], esz, at + seg >= len(data))) < len(data[at:at + seg]) + 5 else 'S'
                   for at in range(0, len(data), seg))


def encode_planes(planes: np.ndarray, th: int, tw: int, predictor: int):
    """[n, H, W] -> the streams in the encoder's order: plane-major, then tile row, then tile column."""
    n, h, w = planes.shape
    return [compress_tile(tile_bytes(planes[p], ty, tx, th, tw, predictor), planes.dtype.itemsize)
            for p in range(n) for ty in range(-(-h // th)) for tx in range(-(-w // tw))]


def expected_tiles(planes: np.ndarray, th: int, tw: int, predictor: int):
    """The bytes every stream must inflate to (b'' for a tile of zeros, whose stream is empty)."""
    n, h, w = planes.shape
    out = []
    for p in range(n):
        for ty in range(-(-h // th)):
            for tx in range(-(-w // tw)):
                b = tile_bytes(planes[p], ty, tx, th, tw, predictor)
                out.append(b if any(b) else b'')
    return out
