"""The planes, shapes and coefficients the distortion tests share (tests/test_distortion_cpu.py, tests/test_distortion_gpu.py)."""
import functools

import numpy as np

import warp_ref

DTYPES = ('uint8', 'uint16')
PPMS = (0, 1, -1, 1500, -1500, 50000, -50000)
PLANE_NAMES = ('noise', 'maximum', 'zero', 'gradient', 'checkerboard')

# The kernel's own sizes (csrc/warp.hip): a thread owns a run of RUN = 2 dst columns of one row and walks over WALK = 16 planes
# with one map; the two taps of a row come in one load of a pair of elements, which is (U - 1, U) at the row's end and a single
# element in a plane one column wide; a workgroup is tx runs wide (a power of two up to 64: strips of 128 columns) and 256 / tx
# rows tall (4 rows for tx = 64; more for narrow planes).
RUN, STRIP, ROWS, WALK = 2, 128, 4, 16
SHAPES = (
    (1, 1), (1, 300), (300, 1), (2, 2),            # one pixel; one row (V = 0); one column (U = 0: no pair), one short of a run;
                                                   # R2 = 2
    (7, 10), (10, 7),                              # odd x even and even x odd
    (3, 3), (5, 5),                                # one past a thread's run; one short of and one past a workgroup's run of
                                                   # rows; odd x odd: a centre pixel
    (9, 127), (7, 128), (9, 129),                  # one short of, exactly and one past a workgroup's strip; three runs of rows
    (17, 259),                                     # three strips, five runs of rows, a partial run at the row's end
    (64, 2048),                                    # the width of a camera tile
)
MANY = (5, 6, 23)      # (h, w, planes): more planes than a thread walks over (two runs of planes, the second partial)


@functools.lru_cache(maxsize=None)
def planes(dtype, h, w, n=None):
    """[5, h, w], read-only: uniform full-range noise, all-maximum, all-zero, a gradient over the full range, a 1-pixel
    checkerboard of 0 and M (the blend's largest sums).  With ``n``: n planes of noise."""
    dt = np.dtype(dtype)
    top = int(np.iinfo(dt).max)
    rng = np.random.default_rng(7919 * h + 13 * w + dt.itemsize)
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
def reference(dtype, h, w, ppm, n=None):
    out = warp_ref.warp_image(planes(dtype, h, w, n), ppm)
    out.setflags(write=False)
    return out
