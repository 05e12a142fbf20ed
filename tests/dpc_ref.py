"""The definition of the differential phase contrast channel (``--dpc``, sq_dpc_tiles), in numpy.

From the two half-pupil brightfield planes L and R of one dtype (uint8 / uint16, maximum M) and an integer gain g in 1..16:

    S = L + R
    N = S + 2 g (L - R)
    DPC = 0                                  if S == 0
        = clamp(floor(M N / (2 S)), 0, M)    otherwise

``floor`` is the mathematical floor of the exact rational: int64 and ``//`` here (numpy's ``//`` floors, also for a negative
numerator), ``fractions.Fraction`` pixel by pixel in ``loop``.  For g = 1 it is M (0.5 + (L - R) / (L + R)), truncated and
clipped: Squid's generate_dpc without its float rounding, whose NaN -> 0 is the S == 0 case."""
import math
from fractions import Fraction

import numpy as np

MAX_GAIN = 16
CHANNEL = 'DPC'


def dpc_image(left, right, gain=1):
    """[..., H, W] uint8 / uint16 left and right of one shape and dtype -> their DPC, of the same shape and dtype."""
    left, right = np.asarray(left), np.asarray(right)
    if left.dtype not in (np.uint8, np.uint16) or right.dtype != left.dtype or left.shape != right.shape or \
            isinstance(gain, bool) or not 1 <= int(gain) <= MAX_GAIN or int(gain) != gain:
        raise ValueError("uint8 / uint16 planes of one shape and dtype, an integer gain in 1..16")
    m = int(np.iinfo(left.dtype).max)
    l, r = left.astype(np.int64), right.astype(np.int64)
    s = l + r
    n = s + 2 * int(gain) * (l - r)
    q = (m * n) // np.where(s == 0, 1, 2 * s)
    return np.where(s == 0, 0, np.clip(q, 0, m)).astype(left.dtype)


def loop(left, right, gain=1):
    """The definition word for word, pixel by pixel, in exact rationals."""
    m = int(np.iinfo(left.dtype).max)
    out = np.zeros(left.shape, dtype=left.dtype)
    for at in np.ndindex(*left.shape):
        l, r = int(left[at]), int(right[at])
        s = l + r
        if s == 0:
            continue
        n = s + 2 * gain * (l - r)
        out[at] = min(max(math.floor(Fraction(m * n, 2 * s)), 0), m)
    return out


def planted(dtype):
    """(left, right) 1-D: the pixels every test plants -- S = 0; L = 0 < R; R = 0 < L; L = R; L = 3R (N = 2S at gain 1: M);
    3L = R (N = 0: 0); L = R = M (floor(M / 2)) -- and their neighbours one count to either side of the two clamps."""
    m = int(np.iinfo(np.dtype(dtype)).max)
    t = m // 4
    pairs = [(0, 0), (0, 7), (7, 0), (0, m), (m, 0), (9, 9), (3 * t, t), (t, 3 * t), (m, m), (1, 1), (1, 0), (0, 1),
             (3 * t + 1, t), (3 * t - 1, t), (t, 3 * t + 1), (t, 3 * t - 1), (m, m - 1), (m - 1, m), (2, 1), (1, 2), (m, 1), (1, m)]
    a = np.array(pairs, dtype=np.dtype(dtype))
    return a[:, 0].copy(), a[:, 1].copy()


def write_dpc_files(root, left_name, right_name, gain=1):
    """Beside every pair of half files ``<region>_<fov>_<z>_<left>`` / ``<right>`` of the acquisition folder ``root`` the file
    ``<region>_<fov>_<z>_DPC`` a user would have made beforehand.  -> the number of files written."""
    import os
    from image_stitcher_amd import tiffio
    lt, rt = left_name.replace(' ', '_'), right_name.replace(' ', '_')
    n = 0
    for folder, _, names in os.walk(root):
        for name in sorted(names):
            stem, ext = os.path.splitext(name)
            parts = stem.split('_', 3)
            if len(parts) == 4 and parts[3] == lt and ext.lower() in ('.tif', '.tiff'):
                other = os.path.join(folder, '_'.join(parts[:3] + [rt]) + ext)
                if os.path.exists(other):
                    out = dpc_image(tiffio.read_image(os.path.join(folder, name)), tiffio.read_image(other), gain)
                    tiffio.write_tiff(os.path.join(folder, '_'.join(parts[:3] + [CHANNEL]) + ext), out)
                    n += 1
    return n
