"""Cases of tests/test_blosc_edges_gpu.py: LZ4 input streams with a literal run and a match of PLANTED lengths, blocks
whose last bytes are a planted copy, block and chunk sizes at the ends of the format's ranges, a structured fuzz, and the
planes that drive the packing kernels past their first pass.  Every builder returns its input together with the
expectation that follows from how the input was made -- never from a model of the encoder.  Nothing here needs a
device: tests/test_blosc_cpu.py checks that every planted stream is what its builder says it is."""
import numpy as np

BLK = 16384                      # the Blosc block size of csrc/blosc.hip
S1_LEN = 24                      # the first planted match: long enough that a stream with it alone is stored compressed
LIT_TARGETS = (0, 1, 14, 15, 16, 269, 270, 271, 524, 525, 526)        # literal run g, with a match of 19
MATCH_TARGETS = (4, 5, 18, 19, 20, 67, 68, 69, 131, 132, 133, 273, 274, 275, 528, 529, 530)   # match length, with g = 15
END_K = tuple(range(4, 21)) + (200,)                                  # the block's last K bytes copy K earlier ones
SEEDS = 8
MID_L = 1282                     # common length of the mid-block streams (even for the uint16 form, not a multiple of 4)
END_L = 600                      # common length of the end-of-block streams


def _rand(rng, k):
    return rng.integers(1, 256, k, dtype=np.uint8)


def repeats(stream: np.ndarray) -> set:
    """Positions p whose 4 bytes stream[p:p+4] also stand at an earlier position: the only places where an LZ4 match
    can start or continue 4 bytes."""
    s = np.asarray(stream, dtype=np.uint32)
    if len(s) < 4:
        return set()
    v = s[:-3] | (s[1:-2] << 8) | (s[2:-1] << 16) | (s[3:] << 24)
    _, first = np.unique(v, return_index=True)
    return set(range(len(v))) - set(first.tolist())


def _planted(copies) -> set:
    out = set()
    for at, length in copies:
        out |= set(range(at, at + length - 3))
    return out


def mid_stream(g: int, m2: int, seed: int, total: int = MID_L) -> dict:
    """A(64) + S1 + X(3) + S2 + Y(64) + copy(S1) + G(g) + copy(S2) + tail(>= 16), random bytes in 1..255.  The byte after
    each copy differs from the byte after its source, and no 4 bytes repeat outside the two copies, so an LZ4 encoder
    that finds both matches emits exactly: (copy1 literals, S1_LEN), (g literals, m2), (tail literals)."""
    fixed = 64 + S1_LEN + 3 + m2 + 64 + S1_LEN + g + m2
    tail = total - fixed
    assert tail >= 16
    rng = np.random.default_rng([seed, g, m2, 1])
    while True:
        a, s1, x, s2, y, gap, t = (_rand(rng, k) for k in (64, S1_LEN, 3, m2, 64, g, tail))
        stream = np.concatenate([a, s1, x, s2, y, s1, gap, s2, t])
        src1, src2 = 64, 64 + S1_LEN + 3
        copy1 = src2 + m2 + 64
        copy2 = copy1 + S1_LEN + g
        if stream[copy1 + S1_LEN] == stream[src1 + S1_LEN] or stream[copy2 + m2] == stream[src2 + m2]:
            continue
        if repeats(stream) == _planted([(copy1, S1_LEN), (copy2, m2)]):
            break
    return dict(stream=stream, n=total, g=g, m2=m2, seed=seed, src1=src1, src2=src2, copy1=copy1, copy2=copy2,
                sequences=[(copy1, S1_LEN, copy1 - src1, copy1), (g, m2, copy2 - src2, copy2), (tail, None, None, total)])


def end_stream(k: int, seed: int, total: int = END_L) -> dict:
    """A(64 + pad) + S1 + X(3) + E(k) + Y(64) + copy(S1) + G(15) + copy(E): the block ENDS with a copy of k earlier bytes.
    LZ4 may start no match after n - 12 and end none after n - 5, so for k >= 12 the last match is (n - k, length k - 5)
    followed by 5 literals, and for k < 12 the last k bytes are literals."""
    pad = total - (64 + S1_LEN + 3 + k + 64 + S1_LEN + 15 + k)
    assert pad >= 0
    rng = np.random.default_rng([seed, k, 2])
    while True:
        a, s1, x, e, y, gap = (_rand(rng, n) for n in (64 + pad, S1_LEN, 3, k, 64, 15))
        stream = np.concatenate([a, s1, x, e, y, s1, gap, e])
        src1 = 64 + pad
        src3 = src1 + S1_LEN + 3
        copy1 = src3 + k + 64
        copy3 = copy1 + S1_LEN + 15
        assert copy3 + k == total
        if stream[copy1 + S1_LEN] == stream[src1 + S1_LEN]:
            continue
        if repeats(stream) == _planted([(copy1, S1_LEN), (copy3, k)]):
            break
    first = (copy1, S1_LEN, copy1 - src1, copy1)
    if k >= 12:
        sequences = [first, (15, k - 5, copy3 - src3, copy3), (5, None, None, total)]
    else:
        sequences = [first, (15 + k, None, None, total)]
    return dict(stream=stream, n=total, k=k, seed=seed, src1=src1, src3=src3, copy1=copy1, copy3=copy3, sequences=sequences)


def apply_sequences(stream: np.ndarray, sequences) -> bytes:
    """What the given sequences decode to when their literals are taken from `stream` at their own positions: equal to
    the stream itself exactly when every match repeats what stands `offset` bytes earlier."""
    out = bytearray()
    for lit, mlen, offset, out_pos in sequences:
        out += stream[len(out):len(out) + lit].tobytes()
        assert len(out) == out_pos
        if mlen is not None:
            for _ in range(mlen):
                out.append(out[-offset])
    return bytes(out)


# ---- the two element sizes ------------------------------------------------------------------------------------------

def shuffled(chunk: bytes, esz: int) -> bytes:
    """The bytes the LZ4 encoder sees: every 16 KiB block of the chunk byte-shuffled on its own (all low bytes of the
    block's elements, then all high bytes)."""
    if esz == 1:
        return bytes(chunk)
    out = []
    for at in range(0, len(chunk), BLK):
        blk = np.frombuffer(chunk[at:at + BLK], np.uint8)
        nel = len(blk) // esz
        out.append(blk[:nel * esz].reshape(nel, esz).T.tobytes() + blk[nel * esz:].tobytes())
    return b''.join(out)


def pixels_of(stream, esz: int) -> np.ndarray:
    """The row of pixels whose shuffled bytes are `stream`: the bytes themselves as uint8, or per 16 KiB block the uint16
    pixels T[e] | T[nel + e] << 8."""
    t = np.frombuffer(bytes(stream), np.uint8)
    if esz == 1:
        return t.copy()
    assert len(t) % 2 == 0
    out = np.empty(len(t) // 2, np.uint16)
    for at in range(0, len(t), BLK):
        blk = t[at:at + BLK].astype(np.uint16)
        nel = len(blk) // 2
        out[at // 2:at // 2 + nel] = blk[:nel] | (blk[nel:] << 8)
    return out


def rows_plane(streams, esz: int):
    """Equal-length streams as the rows of one plane with chunks of one row: chunk i's LZ4 input is streams[i].
    -> (planes [1, n, L / esz], chunk_h, chunk_w)."""
    rows = np.stack([pixels_of(s, esz) for s in streams])
    return rows[None], 1, rows.shape[1]


def mid_cases():
    """[(kind, target, [stream dict per seed])] for the literal-run and the match-length targets."""
    out = [('lit', g, [mid_stream(g, 19, s) for s in range(SEEDS)]) for g in LIT_TARGETS]
    out += [('match', m, [mid_stream(15, m, s) for s in range(SEEDS)]) for m in MATCH_TARGETS]
    return out


def end_cases():
    return [('end', k, [end_stream(k, s) for s in range(SEEDS)]) for k in END_K]


# ---- block and chunk sizes ------------------------------------------------------------------------------------------

def _texture(h, w, dtype, seed):
    """Compressible and never zero: short horizontal runs of a few values, rows repeating with a period of 5."""
    rng = np.random.default_rng(seed)
    base = rng.integers(1, 200, (5, w // 6 + 1))
    plane = np.repeat(base, 6, axis=1)[:, :w][np.arange(h) % 5]
    if np.dtype(dtype).itemsize == 2:
        plane = plane * 257 + 300
    return plane.astype(dtype)


def size_cases():
    """[(name, plane [h, w], chunk_h, chunk_w, last_block_bytes)]: one real chunk and, five columns further, an
    edge chunk that is zero-padded almost everywhere.  Tiny chunks hold random bytes, the others a compressible texture,
    so the full blocks compress and a short last block beside them is stored raw."""
    out = []
    for n in range(1, 17):
        rng = np.random.default_rng(n)
        plane = _rand(rng, 3 * 2 * n).reshape(3, 2 * n)
        plane[2, :n] = 7                                           # a constant chunk: still raw
        plane[2, n:] = 0                                           # and a zero one
        out.append((f'u8-{n}B', plane, 1, n, n))
    for name, dtype, cy, cx in (('u8-33x33', 'uint8', 33, 33), ('u8-129x127', 'uint8', 129, 127), ('u8-145x113', 'uint8', 145, 113),
                                ('u8-4x4099', 'uint8', 4, 4099), ('u8-19x863', 'uint8', 19, 863), ('u16-3x2731', 'uint16', 3, 2731),
                                ('u16-3x2733', 'uint16', 3, 2733)):
        cb = cy * cx * np.dtype(dtype).itemsize
        out.append((name, _texture(cy, cx + 5, dtype, cb), cy, cx, cb - (cb - 1) // BLK * BLK))
    return out


SIZE_LAST_BLOCKS = {'u8-33x33': 1089, 'u8-129x127': 16383, 'u8-145x113': 1, 'u8-4x4099': 12, 'u8-19x863': 13, 'u16-3x2731': 2,
                    'u16-3x2733': 14}


# ---- structured fuzz ------------------------------------------------------------------------------------------------

FUZZ_CHUNK_BYTES = (300, 4096, BLK, BLK + 14, 3 * BLK + 1000)
FUZZ_CHUNKS = {300: 400, 4096: 300, BLK: 200, BLK + 14: 200, 3 * BLK + 1000: 100}
_EDGE_LENGTHS = sorted(set(LIT_TARGETS) | set(MATCH_TARGETS) | {64, 65, 127, 128, 129, 255, 256})
_SMALL_LENGTHS = tuple(range(1, 13))


def fuzz_stream(rng, n: int) -> np.ndarray:
    """n bytes made of random literal runs and copies of earlier bytes, lengths drawn from the edge values of the format
    and the encoder mixed with small ones, offsets from 1 up (offset < length: an overlapping copy); one stream in
    eight is all random, one in sixteen starts with zeros."""
    if rng.integers(8) == 0:
        return _rand(rng, n)
    out = np.empty(n + 1200, np.uint8)
    at = 0
    if rng.integers(16) == 0:
        at = int(rng.integers(1, 40))
        out[:at] = 0
    while at < n:
        length = int(rng.choice(_EDGE_LENGTHS) if rng.integers(3) == 0 else rng.choice(_SMALL_LENGTHS))
        if at == 0 or rng.integers(2) == 0:
            out[at:at + length] = _rand(rng, length)
        else:
            near = rng.integers(3) > 0
            offset = int(rng.integers(1, min(at, 70 if near else 65535) + 1))
            for k in range(0, length, offset):                      # overlapping copies repeat the last `offset` bytes
                step = min(offset, length - k)
                out[at + k:at + k + step] = out[at + k - offset:at + k - offset + step]
        at += length
    return out[:n].copy()


def fuzz_plane(esz: int, chunk_bytes: int):
    """-> (planes [1, n_chunks, chunk_bytes / esz], chunk_h, chunk_w, [stream per chunk]): chunk i's per-block LZ4 input
    is streams[i]."""
    rng = np.random.default_rng([esz, chunk_bytes, 3])
    streams = [fuzz_stream(rng, chunk_bytes) for _ in range(FUZZ_CHUNKS[chunk_bytes])]
    planes, cy, cx = rows_plane(streams, esz)
    return planes, cy, cx, streams


# ---- the packing kernels past their first pass ----------------------------------------------------------------------

CHUNK_GRIDS = {1023: (33, 31), 1024: (32, 32), 1025: (41, 25), 2049: (3, 683), 3249: (57, 57)}


def count_plane(count: int):
    """-> (plane uint8 [h, w], zero mask per 8 x 8 chunk in chunk order): `count` chunks, random bytes in 1..255, about a
    third of the chunks all zero -- in runs of up to 40 and isolated -- the plane's last rows and columns cut so that
    edge chunks are padded."""
    gy, gx = CHUNK_GRIDS[count]
    assert gy * gx == count
    rng = np.random.default_rng(count)
    zero = np.zeros(count, bool)
    at = 0
    while at < count:
        run = int(rng.choice([1, 1, 1, 2, 3, 7, 40]))
        if rng.integers(3) == 0:
            zero[at:at + run] = True
        at += run
    zero[0], zero[-1] = count % 2 == 0, count % 2 == 1
    h, w = 8 * gy - 3, 8 * gx - 5
    plane = _rand(rng, h * w).reshape(h, w)
    mask = np.kron(zero.reshape(gy, gx).astype(np.uint8), np.ones((8, 8), np.uint8))[:h, :w].astype(bool)
    plane[mask] = 0
    return plane, zero


def chunk_263_plane(full: bool = False):
    """uint16 1000 x 2000 in ONE chunk of 1040 x 2064 (263 blocks, the last one 512 bytes, edge-padded on both axes): bands
    of 12 rows alternate between a smooth gradient, a constant and random pixels.  `full`: the plane fills the chunk,
    so that blocks wholly inside a random band are incompressible and raw and compressed blocks interleave to the end."""
    rng = np.random.default_rng(263)
    h, w = (1040, 2064) if full else (1000, 2000)
    plane = np.empty((h, w), np.uint16)
    band = (np.arange(h) // 12) % 3
    smooth = (1000 + np.arange(w) // 16)[None, :] + (np.arange(h) // 4)[:, None]
    plane[band == 0] = smooth[band == 0]
    plane[band == 1] = 0x1234
    plane[band == 2] = rng.integers(0, 65536, (int((band == 2).sum()), w))
    return plane, 1040, 2064


BIG_PIXELS = {(5, 17): 256, (2048, 100): 0xABCD, (4094, 0): 65535, (4095, 4095): 1}


def chunk_32mib_plane():
    """uint16 4096 x 4096, one chunk of exactly 32 MiB = 2048 blocks: zero but for four pixels -- none in block 0, one in
    the last block, one of value 256 (a zero low byte)."""
    plane = np.zeros((4096, 4096), np.uint16)
    for (y, x), v in BIG_PIXELS.items():
        plane[y, x] = v
    return plane, 4096, 4096
