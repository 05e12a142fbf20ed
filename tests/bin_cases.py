"""The planes and shapes the binning tests share (tests/test_binning_cpu.py, tests/test_binning_gpu.py)."""
import functools
import math

import numpy as np

import bin_ref

FACTORS = tuple(range(2, 9))
DTYPES = ('uint8', 'uint16')
PLANE_NAMES = ('noise', 'low-noise', 'maximum', 'zero', 'gradient', 'checkerboard')
LOW_NOISE = PLANE_NAMES.index('low-noise')

# The kernel's own sizes (csrc/bin.hip), all in BINNED pixels: a thread owns a run of OUTS = VEC / gcd(K, VEC) dst columns, VEC
# the elements of 16 bytes (8 uint16 / 16 uint8) -- 1, 2, 4, 8 or 16 columns, depending on K and the dtype -- and walks down 4
# dst rows; a workgroup is tx runs wide (a power of two up to 256: strips of 256 OUTS = 256 ... 4096 dst columns) and 256 / tx
# runs of 4 rows tall.  A source plane of (K hb + ry, K wb + rx) bins to hb x wb.
#   (1, 1)                        one block
#   (1, 300), (300, 1)            with every remainder 1..K - 1 on the long axis: the dropped rows / columns
#   (5, 2 | 3 | 5 | 7 | 9 | 15 | 17)   one short of and one past a thread's run of 2, 4, 8 and 16 (and one past a run of 1); one row
#                                 past a run of rows
#   (5, 257 | 513 | 1025 | 2049 | 4097)    one column past a strip of runs of 1, 2, 4, 8 and 16; one row past the workgroup's run
#                                 of rows (tx = 256: one run); at least three strips for the narrower runs
#   (1, 8200)                     three strips of the widest run
# Those widths are odd, so their rows change phase and the blocks go element by element.  The 16-byte loads and the packed
# store need all K rows of a block on 16-byte boundaries, i.e. a row pitch that is a multiple of 16 bytes, as every real tile
# has (``takes_vector_loads``):
#   (5 K, 16 (3 K + 1))           several runs per row and, where K does not divide 16, a partial run at the row's end
#   (5 K + 1, 112 K)              112 dst columns: whole runs only; one row past a run of rows, a dropped source row
#   (4 K, 2048)                   the width of a camera tile


def shapes(k):
    """The source shapes (h, w) for factor k."""
    out = [(k, k)]
    for r in range(1, k):
        out += [(k, 300 * k + r), (300 * k + r, k)]
    out += [(5 * k, wb * k) for wb in (2, 3, 5, 7, 9, 15, 17, 257, 513, 1025, 2049, 4097)]
    out += [(k + k // 2, 8200 * k + 1)]
    out += [(5 * k, 16 * (3 * k + 1)), (5 * k + 1, 112 * k), (4 * k, 2048)]
    return out


def run_columns(dtype, k):
    """The dst columns of a thread's run (the kernel's OUTS): VEC / gcd(K, VEC)."""
    vec = 16 // np.dtype(dtype).itemsize
    return vec // math.gcd(k, vec)


def takes_vector_loads(dtype, k, h, w, pitch=None, first_element=0):
    """Whether sq_bin_tiles reads a plane stack of (h, w) with row pitch ``pitch`` (elements, default w) whose first element
    is ``first_element`` elements behind a 16-byte boundary with 16-byte loads anywhere -- restated from csrc/bin.hip: the K rows
    of a block keep one phase (the pitch and the plane are multiples of a vector), a shift of the runs puts their source spans
    on boundaries (K * shift = phase mod VEC for a shift below OUTS), and a whole run fits into a row behind that shift."""
    vec = 16 // np.dtype(dtype).itemsize
    outs = run_columns(dtype, k)
    pitch = w if pitch is None else pitch
    shifts = [s for s in range(outs) if (k * s - first_element) % vec == 0]
    wb = w // k
    whole = lambda s: any(r * outs - s >= 0 and (r + 1) * outs - s <= wb for r in range(wb // outs + 2))
    return pitch % vec == 0 and bool(shifts) and all(whole(s) for s in shifts)      # (whichever of them dst makes the host pick)


@functools.lru_cache(maxsize=4)
def planes(dtype, k, h, w):
    """[6, h, w], read-only: uniform full-range noise, uniform noise in [0, 2 M / k^2] (about half of its 'sum' outputs
    saturate), all-maximum, all-zero, a gradient over the full range, a 1-pixel checkerboard of 0 and M."""
    dt = np.dtype(dtype)
    top = int(np.iinfo(dt).max)
    rng = np.random.default_rng(1009 * k + 31 * h + w)
    noise = rng.integers(0, top + 1, (h, w))
    low = rng.integers(0, round(2 * top / (k * k)) + 1, (h, w))      # (the bound to the nearest integer: 8, not 7, for uint8 at K = 8)
    yy, xx = np.mgrid[0:h, 0:w]
    gradient = (yy * w + xx) * top // max(1, h * w - 1)
    checker = ((yy + xx) % 2) * top
    out = np.stack([noise, low, np.full((h, w), top), np.zeros((h, w), np.int64), gradient, checker]).astype(dt)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=4)
def reference(dtype, k, h, w, method):
    out = bin_ref.bin_image(planes(dtype, k, h, w), k, method)
    out.setflags(write=False)
    return out
