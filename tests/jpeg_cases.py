"""Inputs of the JPEG tile-encoder tests (csrc/jpeg.hip, image-stitcher_amd/jpegtile.py): plane stacks by content, the tiles they
are cut into and the streams ``jpegtile.encode_tile`` makes of them.  No device here.  tests/test_jpeg_cpu.py holds the contents to
what they are there for; tests/test_jpeg_gpu.py encodes them on the device."""
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
        out[-1, h - 3, w - 2] = 200
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
