"""The planes, frames, shapes and pedestals the dark-frame tests share (tests/test_dark_frame_cpu.py, tests/test_dark_frame_gpu.py)."""
import functools

import numpy as np

import dark_ref

DTYPES = ('uint8', 'uint16')
PLANE_NAMES = ('noise', 'maximum', 'zero', 'gradient', 'checkerboard')
FRAME_NAMES = ('zero', 'maximum', 'noise', 'low with warm pixels')

# The kernel's own sizes (csrc/dark.hip): a thread owns one 16-byte vector of columns (VEC = 8 uint16 / 16 uint8), walks down
# RPT = 8 rows and over IPT = SQ_DARK_IMAGES_PER_THREAD images (1 in the library as built: the walk measured slower); a workgroup of 256 threads is tx vectors wide (a power of two up
# to 256: strips of 2048 uint16 / 4096 uint8 columns) and 256 / tx runs of rows tall; a grid takes 65535 groups of IPT images.
RPT, THREADS, IPT, GRID_Y = 8, 256, 1, 65535
VEC = {'uint8': 16, 'uint16': 8}
STRIP = {dt: THREADS * v for dt, v in VEC.items()}


def top(dtype) -> int:
    return int(np.iinfo(np.dtype(dtype)).max)


def pedestals(dtype):
    return (0, 1, top(dtype), top(dtype) // 3)


def constants(dtype):
    """The constant path's frames: 0, M, about M / 600, a middle value."""
    return (0, top(dtype), max(1, top(dtype) // 600), top(dtype) // 2 + 1)


@functools.lru_cache(maxsize=None)
def shapes(dtype):
    vec, strip = VEC[dtype], STRIP[dtype]
    return ((1, 1), (1, 300), (300, 1),                                      # one pixel; one row; one column
            (5, vec - 1), (5, vec), (5, vec + 1), (5, 2 * vec + 1),          # around one vector; two and one element
            (RPT - 1, 11), (RPT, 11), (RPT + 1, 11),                         # around a thread's run of rows
            (37, 53),                                                        # odd x odd
            (3, strip + 1))                                                  # one past a workgroup's strip


@functools.lru_cache(maxsize=None)
def planes(dtype, h, w, n=None):
    """[5, h, w], read-only: uniform full-range noise, all-maximum, all-zero, a gradient over the full range, a 1-pixel
    checkerboard of 0 and M.  With ``n``: n planes of noise."""
    dt = np.dtype(dtype)
    m = top(dt)
    rng = np.random.default_rng(7919 * h + 13 * w + dt.itemsize)
    if n is not None:
        out = rng.integers(0, m + 1, (n, h, w)).astype(dt)
    else:
        yy, xx = np.mgrid[0:h, 0:w]
        gradient = (yy * w + xx) * m // max(1, h * w - 1)
        checker = ((yy + xx) % 2) * m
        out = np.stack([rng.integers(0, m + 1, (h, w)), np.full((h, w), m), np.zeros((h, w), np.int64), gradient,
                        checker]).astype(dt)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def frames(dtype, h, w):
    """[4, h, w], read-only: all 0, all M, noise over the full range, and a camera's: about M / 600 with a little noise and a
    few pixels at M."""
    dt = np.dtype(dtype)
    m = top(dt)
    rng = np.random.default_rng(104723 * h + 17 * w + dt.itemsize)
    low = max(1, m // 600) + rng.integers(0, 3, (h, w))
    warm = rng.integers(0, h * w, max(1, h * w // 50))
    low.reshape(-1)[warm] = m
    out = np.stack([np.zeros((h, w), np.int64), np.full((h, w), m), rng.integers(0, m + 1, (h, w)), low]).astype(dt)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def reference(dtype, h, w, frame, pedestal, n=None):
    """dark_ref of ``planes(dtype, h, w, n)``; ``frame`` is ('frame', i), frame i of ``frames(dtype, h, w)``, or ('constant', c)."""
    kind, value = frame
    d = frames(dtype, h, w)[value] if kind == 'frame' else int(value)
    out = dark_ref.dark_image(planes(dtype, h, w, n), d, pedestal)
    out.setflags(write=False)
    return out
