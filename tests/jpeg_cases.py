"""Inputs of the JPEG tile-encoder tests (csrc/jpeg.hip, image-stitcher_amd/jpegtile.py): plane stacks by content, the tiles they
are cut into and the streams ``jpegtile.encode_tile`` makes of them.  No device here.  tests/test_jpeg_cpu.py holds the contents to
what they are there for; tests/test_jpeg_gpu.py and tests/test_jpeg_edges_gpu.py encode them on the device."""
import numpy as np

from image_stitcher_amd import jpegtile as J

# (name, (planes, h, w), (tile_h, tile_w), padded pitch and plane stride): the smallest shapes at which each mechanism can go wrong
SHAPES = [
    ('edges', (1, 40, 72), (16, 16), False),         # edge tiles in both directions, 2 blocks per interval
    ('padded', (3, 50, 70), (32, 32), True),         # odd pitch: the byte-wise loads; three planes
    ('rounds', (1, 16, 1040), (16, 1040), False),    # 130 blocks per interval: two full rounds of 64 and 2 more
    ('restarts', (1, 144, 64), (144, 64), False),    # 18 intervals: the RST counter wraps twice
]
DEFAULT_SHAPE = ('default', (1, 512, 512), (512, 512), False)
QUALITIES = (1, 50, 90, 100)
# what each content exercises
CONTENTS = {
    'zero': 'no stream at all',
    'pixel': 'one non-zero pixel: one tile with a stream, a few coefficients in one block',
    'const128': 'all-zero blocks: DC difference 0 and EOB only',
    'const255': 'only the DC is non-zero, only in the first block of an interval',
    'uniform': 'uniform noise: long codes, many coefficients, frequent stuffed FF',
    'blocks': '8 x 8 blocks alternating 0 and 255: DC differences of category 11 at quality 100',
    'checker': 'pixels alternating 1 and 255 (-127 / +127): the largest AC coefficient, category 10',
    'ramp': 'a smooth ramp: EOB after a few coefficients',
    'last': 'blocks whose only AC energy is at zigzag 63: three ZRL, no EOB',
    'gaps': 'zero runs of 16, 33 and 47 between coefficients: ZRL once and twice, EOB after 48, none after 63',
}

# ---- the format's and the kernels' edges (tests/test_jpeg_edges_gpu.py): (name, (planes, h, w), (tile_h, tile_w), layout).  layout
# None: dense; else (pitch, plane stride, base offset in bytes behind a 256-byte boundary) inside a buffer of GUARD bytes
GUARD = 0xEE
EDGE_SHAPES = [
    # the 64-bit pixel load needs base, pitch and plane stride all multiples of 8, and takes a block only if it lies inside w
    ('mixed', (2, 24, 70), (16, 16), (72, 24 * 72, 0)),      # an aligned wave whose last block is partial (6 of 8 columns)
] + [(f'phase{k}', (2, 24, 70), (16, 16), (72, 24 * 72, k)) for k in range(1, 8)] + [      # the pointer alone switches it off
    ('stride', (2, 24, 72), (16, 16), (72, 24 * 72 + 4, 0)),     # the plane stride alone does; plane 1's rows are 4 off
    ('round64', (1, 8, 512), (8, 512), None),                # exactly one round of 64 blocks
    ('round65', (1, 8, 520), (8, 520), None),                # one round and one block
    ('tall65', (1, 520, 8), (520, 8), None),                 # jpeg_tile_kernel's second round of 64 intervals: the carry
    ('tall129', (1, 1032, 8), (1032, 8), None),              # two full rounds and one interval
    ('tiles1024', (1, 256, 256), (8, 8), None),              # jpeg_scan_kernel: one tile per thread, every thread busy
    ('tiles1025', (1, 200, 328), (8, 8), None),              # 25 x 41 tiles: two per thread, threads 513.. with lo == hi == n
    ('tiles2625', (3, 200, 280), (8, 8), None),              # 3 x 25 x 35: three per thread
    ('tiny1', (1, 1, 1), (8, 8), None),                      # a plane smaller than a block
    ('tiny79', (1, 7, 9), (16, 16), None),                   # whole blocks and a whole interval past the edge
    # the largest sides: J.MAX_SIDE = 65496 (T.81 itself holds 65528, but libjpeg decodes nothing above 65500)
    ('widest', (1, 8, 2 * J.MAX_SIDE), (8, J.MAX_SIDE), None),      # 8187 blocks per interval: DRI 8187, 128 rounds; two tiles
    ('tallest', (1, J.MAX_SIDE, 8), (J.MAX_SIDE, 8), None),         # 8187 intervals: SOF0 height 0xFFD8, 128 rounds of the tile scan
]
EDGE_CONTENTS = {        # what every edge shape is encoded with: content -> qualities
    'uniform': (100, 50), 'binary': (100, 1), 'ramp': (90,), 'pixel': (100,), 'zero': (50,),
}
# the shapes that also run every content of CONTENTS
FULL_CONTENT_SHAPES = ('round64', 'round65', 'mixed')
FFRUNS_SHAPES = [('round65', (1, 8, 520), (8, 520)), ('wide', (1, 16, 1040), (16, 1040))]
# all-ones magnitudes (31, 63, 127) behind the 16-bit AC codes of long zero runs: FF bytes in a row once un-stuffed
FFRUNS_KINDS = [{16: 63, 32: 63, 48: 63, 63: 63}, {16: 31, 32: 63, 48: 31, 63: 63}, {17: 63, 33: 31, 49: 63, 63: 31},
                {16: 127, 32: 31, 48: 63}, {15: 31, 31: 31, 47: 31, 63: 31}, {16: 63, 33: 63, 50: 63}]
FFRUNS_SEED = 5      # found on the host: both FFRUNS_SHAPES reach every condition tests/test_jpeg_cpu.py holds them to
DCSWEEP_QUALITIES = (50, 75, 90, 100)
SWEEP_SHAPE = (1, 16, 64)


def edge_shape(name):
    return next(s for s in EDGE_SHAPES if s[0] == name)


def edge_content(name, shape_name, quality):
    """The planes of one edge case: tiles1024 / 1025 / 2625 with runs of all-zero tiles, as the scan meets them in a real plane."""
    _, shape, _, _ = edge_shape(shape_name)
    planes = content(name, shape, seed=len(name) + quality)
    if shape_name == 'tiles2625':
        planes[1] = 0
        planes[0, 40:80] = 0
    return planes


def sweep_tile() -> np.ndarray:
    """The tile of the quality sweep: noise with one all-0 and one all-255 block (the extreme DC values under every divisor)."""
    planes = content('uniform', SWEEP_SHAPE, seed=1234)
    planes[0, :8, 8:16] = 0
    planes[0, 8:, 40:48] = 255
    return planes


def guarded(planes: np.ndarray, layout):
    """-> (buffer of GUARD bytes holding the planes, offset of plane 0 in it).  The buffer starts with 256 guard bytes, so with
    the buffer on a 256-byte boundary the planes start `base` bytes behind one; every row and every plane is followed by guard
    bytes, and 64 more close the buffer."""
    pitch, stride, base = layout
    n, h, w = planes.shape
    assert pitch >= w and stride >= (h - 1) * pitch + w
    buf = np.full(256 + base + n * stride + 64, GUARD, np.uint8)
    view = np.lib.stride_tricks.as_strided(buf[256 + base:], (n, h, w), (stride, pitch, 1))
    view[...] = planes
    return buf, 256 + base


def longest_guard_run(planes: np.ndarray) -> int:
    """The longest run of GUARD bytes inside a row of the planes: a window that looks like its guard proves nothing."""
    best = 0
    for row in planes.reshape(-1, planes.shape[-1]):
        run = 0
        for v in (row == GUARD).tolist():
            run = run + 1 if v else 0
            best = max(best, run)
    return best


def ff_places(data: bytes, block_bits) -> list:
    """(word index in its byte-stuffing window, byte of the word 0..3) of every FF among an interval's un-stuffed bytes, as
    csrc/jpeg.hip's stuff_out meets them.  The interval kernel codes 64 blocks a round; the whole 32-bit words of a round leave
    at its end, 64 words a group, and the partial word opens the next round's window: the window of round r starts at the word
    that holds the first bit of block 64 r, and the last window (padding included) at the word behind the last whole one.
    `block_bits`: the bit position of every block's start and of the data's end (jpeg_ref.decode)."""
    bases = [block_bits[b] >> 5 for b in range(0, len(block_bits) - 1, 64)] + [block_bits[-1] >> 5]
    out = []
    for i in np.flatnonzero(np.frombuffer(data, np.uint8) == 0xFF).tolist():
        g = i >> 2
        base = max(b for b in bases if b <= g)
        out.append((g - base, i & 3))
    return out


def longest_ff_run(data: bytes) -> int:
    best = run = 0
    for v in data:
        run = run + 1 if v == 0xFF else 0
        best = max(best, run)
    return best


def _idct_blocks(coefs: dict) -> np.ndarray:
    """An 8 x 8 pixel block (float, around 0) whose orthonormal DCT holds coefs[zigzag position] and zeros."""
    u = np.arange(8)[:, None]
    j = np.arange(8)[None, :]
    a = np.where(u == 0, np.sqrt(1 / 8), 0.5) * np.cos((2 * j + 1) * u * np.pi / 16)
    f = np.zeros(64)
    for k, v in coefs.items():
        f[J.ZIGZAG[k]] = v
    return a.T @ f.reshape(8, 8) @ a


def _tile_blocks(shape, blocks) -> np.ndarray:
    """Planes of `shape` covered by the 8 x 8 pixel blocks, taken in turn along the block diagonals."""
    n, h, w = shape
    by, bx = -(-h // 8), -(-w // 8)
    pick = (np.arange(by)[:, None] + np.arange(bx)[None, :]) % len(blocks)
    full = np.stack(blocks)[pick].transpose(0, 2, 1, 3).reshape(by * 8, bx * 8)
    return np.broadcast_to(full[:h, :w], shape).copy()


def content(name: str, shape, seed: int = 0) -> np.ndarray:
    n, h, w = shape
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    q50 = J.quant_table(50)[J.ZIGZAG]        # the divisors in zigzag order
    if name == 'zero':
        out = np.zeros(shape)
    elif name == 'pixel':
        out = np.zeros(shape)
        out[-1, max(h - 3, 0), max(w - 2, 0)] = 200
    elif name == 'const128':
        out = np.full(shape, 128)
    elif name == 'const255':
        out = np.full(shape, 255)
    elif name == 'uniform':
        out = rng.integers(0, 256, shape)
    elif name == 'blocks':
        out = np.broadcast_to(255 * (((yy // 8) + (xx // 8)) % 2), shape)
    elif name == 'checker':
        out = np.broadcast_to(np.where((yy + xx) % 2, 255, 1), shape)
    elif name == 'ramp':
        out = np.stack([(xx * 0.6 + yy * 0.3 + 10 * p) % 256 for p in range(n)])
    elif name == 'last':
        out = 128 + _tile_blocks(shape, [np.rint(_idct_blocks({63: 2 * q50[63]})), np.rint(_idct_blocks({63: -q50[63]}))])
    elif name == 'gaps':
        a = _idct_blocks({1: 2 * q50[1], 18: -2 * q50[18], 52: q50[52], 63: -q50[63]})
        b = _idct_blocks({48: 2 * q50[48]})
        out = 128 + _tile_blocks(shape, [np.rint(a), np.rint(b)])
    elif name == 'binary':
        out = 255 * rng.integers(0, 2, shape)
    elif name == 'ffruns':
        blocks = [np.rint(_idct_blocks(kind)) for kind in FFRUNS_KINDS]
        pick = np.random.default_rng(FFRUNS_SEED).integers(0, len(blocks), (-(-h // 8), -(-w // 8)))
        full = np.stack(blocks)[pick].transpose(0, 2, 1, 3).reshape(pick.shape[0] * 8, pick.shape[1] * 8)
        out = 128 + np.broadcast_to(full[:h, :w], shape)
    elif name == 'dcsweep':                  # block b (row-major over the planes' blocks) sums to min(b, 64 * 255)
        assert h % 8 == 0 and w % 8 == 0
        total = np.minimum(np.arange(n * (h // 8) * (w // 8)), 64 * 255)
        px = total[:, None] // 64 + (np.arange(64)[None, :] < total[:, None] % 64)
        out = px.reshape(n, h // 8, w // 8, 8, 8).transpose(0, 1, 3, 2, 4).reshape(shape)
    elif name == 'image':                    # smooth + texture + noise: what fidelity is measured on
        out = np.stack([120 + 80 * np.sin(xx / 40 + p) * np.cos(yy / 55) + 20 * np.sin(xx * 0.9) * np.sin(yy * 0.7)
                        + rng.normal(0, 4, (h, w)) for p in range(n)])
    else:
        raise KeyError(name)
    return np.clip(np.asarray(out), 0, 255).astype(np.uint8)


def tiles_of(planes: np.ndarray, th: int, tw: int) -> np.ndarray:
    """The full tiles [n * rows * cols, th, tw] of a plane stack, zero past the plane's edge, in the encoder's order."""
    n, h, w = planes.shape
    gy, gx = -(-h // th), -(-w // tw)
    pad = np.zeros((n, gy * th, gx * tw), np.uint8)
    pad[:, :h, :w] = planes
    return pad.reshape(n, gy, th, gx, tw).transpose(0, 1, 3, 2, 4).reshape(n * gy * gx, th, tw)


def expected_streams(planes: np.ndarray, th: int, tw: int, quality: int) -> list:
    """The stream of every tile as the host definition makes it; b'' for a tile of zeros."""
    return [J.encode_tile(t, quality) if t.any() else b'' for t in tiles_of(planes, th, tw)]


def entropy_data(stream: bytes) -> bytes:
    """What lies between the SOS segment and EOI."""
    assert stream[J.HEADER_BYTES - 10:J.HEADER_BYTES - 8] == b'\xFF\xDA' and stream[-2:] == b'\xFF\xD9'
    return stream[J.HEADER_BYTES:-2]
