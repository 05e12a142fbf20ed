"""Inputs of the tile-encoder tests (csrc/deflate.hip): plane stacks by content, no device here.  tests/test_deflate_cpu.py holds
them to what they are there for; tests/test_deflate_gpu.py and tests/test_deflate_edges_gpu.py encode them on the device."""
import numpy as np

SEG = 16384

# (name, (n, h, w), tile side): edge tiles in both directions and a tile smaller than a segment; exactly two segments of uint16
# (one of uint8); a partial last segment; three planes (the GPU test gives them a padded pitch and plane stride)
SHAPES = [('edges-40x72-t16', (1, 40, 72), 16), ('two-segments-128-t128', (1, 128, 128), 128),
          ('partial-segment-144-t144', (1, 144, 144), 144), ('three-planes-50x70-t32', (3, 50, 70), 32)]
CONTENTS = ('zero', 'one-pixel', 'constant', 'uniform', 'runs', 'cumsum')


def run_lengths():
    """Every length 1..300, the lengths 258..261 first (so that every shape that holds a few hundred elements meets them)."""
    return [258, 259, 260, 261] + [k for k in range(300, 0, -1) if not 258 <= k <= 261]


def runs(count: int, dtype) -> np.ndarray:
    """`count` elements: runs of the lengths above, repeated, no two neighbouring runs of one value, no zero."""
    top = int(np.iinfo(dtype).max)
    out, k = np.empty(count + 400, dtype), 0
    at = 0
    while at < count:
        for length in run_lengths():
            out[at:at + length] = 1 + k % top
            at += length
            k += 1
            if at >= count:
                break
    return out[:count]


def content(name: str, shape, dtype, seed: int = 0) -> np.ndarray:
    n, h, w = shape
    rng = np.random.default_rng(seed)
    info = np.iinfo(dtype)
    if name == 'zero':
        return np.zeros(shape, dtype)
    if name == 'one-pixel':
        a = np.zeros(shape, dtype)
        a[n - 1, h // 2, w - 1] = info.max - 2
        return a
    if name == 'constant':
        return np.full(shape, 1234 % info.max + 1, dtype)
    if name == 'uniform':
        return rng.integers(0, int(info.max) + 1, shape).astype(dtype)
    if name == 'runs':
        return runs(n * h * w, dtype).reshape(shape)
    if name == 'cumsum':       # rows that are cumulative sums of differences uniform in -256..255 (modulo 2^bits)
        return np.cumsum(rng.integers(-256, 256, shape), axis=2).astype(np.int64).astype(dtype)
    raise ValueError(name)


def every_run_length(dtype) -> np.ndarray:
    """Three planes whose row-major elements are runs of every length 1..300: 144 x 144 uint8 (a plane = one tile of a segment and
    a partial one) or 128 x 128 uint16 (two segments), so that runs also cross segment boundaries."""
    side = 144 if np.dtype(dtype).itemsize == 1 else 128
    return runs(3 * side * side, dtype).reshape(3, side, side)


def fibonacci_segment() -> np.ndarray:
    """One 128 x 128 uint8 plane = one segment of 16384 literals whose value counts are Fibonacci numbers scaled to the segment (the
    unlimited Huffman code is then deeper than 15), arranged so that no value repeats back to back (no runs)."""
    fib = [1, 1]
    while len(fib) < 22:
        fib.append(fib[-1] + fib[-2])
    f = np.array(fib, float)
    counts = np.maximum(1, (f / f.sum() * 16000).astype(int))
    counts[-1] += SEG - counts.sum()
    assert counts[-1] <= SEG // 2
    values = np.repeat(np.arange(1, len(counts) + 1)[::-1], counts[::-1]).astype(np.uint8)      # most frequent first
    out = np.empty(SEG, np.uint8)
    half = (SEG + 1) // 2
    out[0::2] = values[:half]
    out[1::2] = values[half:]
    return out.reshape(1, 128, 128)


def fibonacci_segment_u16() -> np.ndarray:
    """One 64 x 128 uint16 plane = one segment of 8192 elements drawn from 21 values whose counts are Fibonacci numbers scaled to
    the segment, interleaved as above so that no two neighbours are equal (no runs).  Every element is v * 257: its low and its
    high byte are both the literal v, so that the pair of codes one element sends is two codes of the same -- up to the limit's --
    length."""
    n = SEG // 2
    fib = [1, 1]
    while len(fib) < 21:
        fib.append(fib[-1] + fib[-2])
    f = np.array(fib, float)
    counts = np.maximum(1, (f / f.sum() * 8000).astype(int))
    counts[-1] += n - counts.sum()
    assert counts[-1] <= n // 2
    values = np.repeat(np.arange(1, len(counts) + 1)[::-1], counts[::-1]).astype(np.uint16)      # most frequent first
    out = np.empty(n, np.uint16)
    half = (n + 1) // 2
    out[0::2] = values[:half]
    out[1::2] = values[half:]
    return (out * 257).reshape(1, 64, 128)


def mixed_segments(dtype) -> np.ndarray:
    """Two planes, each one tile of segments that do not shrink next to segments that do: uniform random over the full range, the
    lower half of plane 0 and the upper half of plane 1 one non-zero constant.  uint16: 128 x 128, two segments a plane (stored,
    dynamic / dynamic, stored); uint8: 256 x 256, four (SSDD / DDSS).  The halves are whole segments and whole rows, so the kinds
    are the same under either predictor."""
    dtype = np.dtype(dtype)
    side = 128 if dtype.itemsize == 2 else 256
    rng = np.random.default_rng(77)
    a = rng.integers(0, int(np.iinfo(dtype).max) + 1, (2, side, side)).astype(dtype)
    a[0, side // 2:] = 201
    a[1, :side // 2] = 201
    return a


MIXED_KINDS = {'uint16': ('SD', 'DS'), 'uint8': ('SSDD', 'DDSS')}


def all_ones(shape, dtype) -> np.ndarray:
    """Every byte 0xFF: the largest Adler-32 partial sums a segment can have."""
    return np.full(shape, np.iinfo(dtype).max, dtype)


# Tile shapes that are no TIFF tiles (the C ABI takes any tile_h, tile_w >= 1): (name, content, (n, h, w), (tile_h, tile_w)).
# A one-element tile; tiles far smaller than a wave's round; a row of exactly one round; the whole odd-sized plane as one tile;
# a uint16 tile whose second segment ends 16 elements into a round; one whose second segment has 8191 elements (63 into the last
# round, and odd) -- as uint8 one segment of 16383; a plane smaller than its tile in both directions.
OFF_GRID = [('t1x1', 'cumsum', (2, 11, 15), (1, 1)), ('t5x7', 'cumsum', (2, 37, 53), (5, 7)),
            ('t3x64', 'cumsum', (2, 37, 53), (3, 64)), ('t37x53', 'cumsum', (2, 37, 53), (37, 53)),
            ('t100x100-runs', 'runs', (1, 100, 100), (100, 100)), ('t129x127', 'cumsum', (1, 129, 127), (129, 127)),
            ('plane10x10-t16x32', 'cumsum', (1, 10, 10), (16, 32))]


def off_grid(name: str, dtype):
    """-> (planes, tile_h, tile_w) of the OFF_GRID case.  The 1 x 1 tiles are cut from the (2, 37, 53) stack's corner."""
    _, kind, shape, (th, tw) = next(c for c in OFF_GRID if c[0] == name)
    if name == 't1x1':
        return np.ascontiguousarray(content(kind, (2, 37, 53), dtype, seed=4)[:, :shape[1], :shape[2]]), th, tw
    return content(kind, shape, dtype, seed=4), th, tw


def last_segment_elements(th: int, tw: int, dtype) -> int:
    """Elements of the last segment of a th x tw tile."""
    per = SEG // np.dtype(dtype).itemsize
    return (th * tw - 1) % per + 1
