"""Inputs of the tile-encoder tests (csrc/deflate.hip): plane stacks by content, no device here.  tests/test_deflate_cpu.py holds
them to what they are there for; tests/test_deflate_gpu.py encodes them on the device."""
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
