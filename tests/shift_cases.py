"""The planes, shapes and shifts the channel-shift tests share (tests/test_channel_shift_cpu.py, tests/test_channel_shift_gpu.py)."""
import functools

import numpy as np

import shift_ref

DTYPES = ('uint8', 'uint16')
PLANE_NAMES = ('noise', 'maximum', 'zero', 'gradient', 'checkerboard')

# The kernel's own sizes (csrc/shift.hip): a thread owns one 16-byte vector of dst columns (VEC = 8 uint16 / 16 uint8) and walks
# down RPT = 32 rows; its source span is VEC + 1 columns; a workgroup of 256 threads is tx vectors wide (a power of two up to 256:
# strips of 2048 uint16 / 4096 uint8 columns) and 256 / tx runs of rows tall.
RPT, THREADS = 32, 256
VEC = {'uint8': 16, 'uint16': 8}
STRIP = {dt: THREADS * v for dt, v in VEC.items()}

MIXED = (3 * 256 + 77, -(9 * 256 + 200))
SHIFTS = (
    (0, 0), (1, 1), (-1, -1), (1, -1), (-1, 1), (255, 255),        # the identity; the smallest fractions; the largest
    (256, 0), (0, -256), (128, -128),                              # whole pixels along one axis; the half pixel
    MIXED, (-MIXED[0], -MIXED[1]),                                 # whole pixels and a fraction, both signs on both axes
    (16384, -16384), (-16384, 16384),                              # the range's ends: larger than every side below 64
)


@functools.lru_cache(maxsize=None)
def shapes(dtype):
    vec, strip = VEC[dtype], STRIP[dtype]
    found = [(1, 1), (1, 300), (300, 1), (2, 2),                   # one pixel; one row (V = 0); one column (U = 0)
             (5, vec - 1), (5, vec), (5, vec + 1),                 # one short of, exactly and one past a vector
             (5, 2 * vec), (5, 2 * vec + 1),                       # ... and a vector plus its span's last element; one past
             (RPT - 1, 11), (RPT, 11), (RPT + 1, 11),              # one short of, exactly and one past a thread's run of rows
             (3 * RPT - 2, 3 * vec + 2),                           # three runs of rows, the last one short
             (37, 53), (71, 143)]                                  # odd x odd; ... with sides above the largest shift
    if dtype == 'uint16':
        found += [(3, strip - 1), (3, strip), (3, strip + 1)]      # one short of, exactly and one past a workgroup's strip
    else:
        found += [(3, strip + 1)]
    return tuple(found)


MANY = (RPT + 3, 21, 7)      # (h, w, planes) of the table tests: two runs of rows, seven planes


@functools.lru_cache(maxsize=None)
def planes(dtype, h, w, n=None):
    """[5, h, w], read-only: uniform full-range noise, all-maximum (the blend's largest sums), all-zero, a gradient over the full
    range, a 1-pixel checkerboard of 0 and M.  With ``n``: n planes of noise."""
    dt = np.dtype(dtype)
    top = int(np.iinfo(dt).max)
    rng = np.random.default_rng(104729 * h + 31 * w + dt.itemsize)
    if n is not None:
        out = rng.integers(0, top + 1, (n, h, w)).astype(dt)
    else:
        yy, xx = np.mgrid[0:h, 0:w]
        gradient = (yy * w + xx) * top // max(1, h * w - 1)
        checker = ((yy + xx) % 2) * top
        out = np.stack([rng.integers(0, top + 1, (h, w)), np.full((h, w), top), np.zeros((h, w), np.int64), gradient,
                        checker]).astype(dt)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def reference(dtype, h, w, shift, n=None):
    out = shift_ref.shift_image(planes(dtype, h, w, n), *shift)
    out.setflags(write=False)
    return out
