"""--channel-shift: per-channel sub-pixel alignment of every tile before anything but the distortion correction sees it
(include/squidstitch.h, sq_shift_tiles; an extension, the reference has nothing like it).  This module holds what the host needs
of it: the option check, the CLI's decimal parser and the shift of one image in numpy, for the readers that touch single files
(``get_tile``, the flatfield estimate's samples).  The staged tiles are shifted on the device.

For a plane I of h x w, uint8 or uint16, and S = (Sy, Sx), two integers in 1/256 pixel, each in -16384..16384 (+-64 px):

    U = w - 1, V = h - 1
    for the output pixel (y, x):
      Y = clamp(256*y + Sy, 0, 256*V),  X = clamp(256*x + Sx, 0, 256*U)           edges replicated
      y0 = Y >> 8, fy = Y & 255, y1 = min(y0 + 1, V);   x0, fx, x1 likewise
      out(y, x) = ( I[y0,x0]*(256-fx)*(256-fy) + I[y0,x1]*fx*(256-fy)
                  + I[y1,x0]*(256-fx)*fy       + I[y1,x1]*fx*fy + 32768 ) >> 16

The output at (y, x) takes the input at (y + Sy/256, x + Sx/256), bilinearly with 8 fractional bits (the blend of distortion.py
under another map): a point imaged at (y, x) in the reference channel and at (y + DY, x + DX) in channel NAME is put right by
``--channel-shift NAME DY DX``.  Integers only, so the device kernel and a second implementation (tests/shift_ref.py) agree bit
for bit.  An RGB image is shifted per colour plane, each with its own pair.  S = (0, 0) is the identity, a shift by whole pixels
a copy with replicated edges."""
from __future__ import annotations

import re
from fractions import Fraction

import numpy as np

from .tiffio import read_image

MAX_SHIFT = 16384      # 1/256 pixel: 64 pixels
MAX_SIDE = 65535
_DECIMAL = re.compile(r'[+-]?[0-9]+(\.[0-9]+)?\Z')


def _component(value, what):
    if isinstance(value, bool) or not isinstance(value, int) or not -MAX_SHIFT <= value <= MAX_SHIFT:
        raise ValueError(f"{what} must be a Python int in -{MAX_SHIFT}..{MAX_SHIFT} (1/256 pixel), got {value!r}")
    return value


def check_option(channel_shifts):
    """The Stitcher's argument, validated: None or a mapping of channel name -> (Sy, Sx), Python ints in 1/256 pixel within
    -16384..16384 (bools, floats and strings are refused) -> a plain dict without the zero entries."""
    if channel_shifts is None:
        return {}
    if not hasattr(channel_shifts, 'items'):
        raise ValueError(f"channel_shifts must be a mapping of channel name -> (Sy, Sx), got {channel_shifts!r}")
    checked = {}
    for name, pair in channel_shifts.items():
        if not isinstance(name, str):
            raise ValueError(f"channel_shifts: a channel name must be a string, got {name!r}")
        if isinstance(pair, (str, bytes)) or not hasattr(pair, '__len__') or len(pair) != 2:
            raise ValueError(f"channel_shifts[{name!r}] must be a pair (Sy, Sx), got {pair!r}")
        sy, sx = (_component(v, f"channel_shifts[{name!r}]") for v in pair)
        if (sy, sx) != (0, 0):
            checked[name] = (sy, sx)
    return checked


def parse_pixels(text) -> int:
    """The CLI's decimal text in pixels -> 1/256 pixel, exactly: a plain decimal literal (no exponent, no '/'), S = floor(256 v
    + 1/2), |v| <= 64; ValueError otherwise."""
    if not isinstance(text, str) or not _DECIMAL.match(text):
        raise ValueError(f"a shift is a plain decimal number of pixels in -64..64, got {text!r}")
    value = Fraction(text)
    if not -64 <= value <= 64:
        raise ValueError(f"a shift is a plain decimal number of pixels in -64..64, got {text!r}")
    return int((256 * value + Fraction(1, 2)).__floor__())


def _shift_plane(img: np.ndarray, sy: int, sx: int) -> np.ndarray:
    h, w = img.shape
    xs = np.clip(256 * np.arange(w, dtype=np.int64)[None, :] + sx, 0, 256 * (w - 1))
    ys = np.clip(256 * np.arange(h, dtype=np.int64)[:, None] + sy, 0, 256 * (h - 1))
    x0, fx, y0, fy = xs >> 8, xs & 255, ys >> 8, ys & 255
    x1, y1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)
    a = img.astype(np.int64)
    acc = a[y0, x0] * ((256 - fx) * (256 - fy)) + a[y0, x1] * (fx * (256 - fy)) + a[y1, x0] * ((256 - fx) * fy) + \
        a[y1, x1] * (fx * fy) + 32768
    return (acc >> 16).astype(img.dtype)


def _pairs(sy, sx, colours):
    """(Sy, Sx) per colour plane: two ints for all of them, or two sequences with one int per plane."""
    if isinstance(sy, (list, tuple)) or isinstance(sx, (list, tuple)):
        if len(sy) != colours or len(sx) != colours:
            raise ValueError(f"an image of {colours} colour planes takes {colours} pairs")
        return [(_component(a, 'a shift'), _component(b, 'a shift')) for a, b in zip(sy, sx)]
    return [(_component(sy, 'a shift'), _component(sx, 'a shift'))] * colours


def shift_image(img: np.ndarray, sy, sx) -> np.ndarray:
    """``img`` [h, w], a [1, h, w] page stack, or [h, w, 3] shifted per colour plane (``sy`` and ``sx`` then may be sequences of
    one int per plane), uint8 / uint16, shifted along h and w."""
    img = np.asarray(img)
    if img.ndim == 3 and img.shape[0] == 1 and img.shape[2] != 3:      # a page stack of one page
        return shift_image(img[0], sy, sx)[None]
    if img.ndim not in (2, 3):
        raise ValueError(f"the shift takes [h, w] or [h, w, colours] images, got shape {img.shape}")
    pairs = _pairs(sy, sx, 1 if img.ndim == 2 else img.shape[2])
    if all(p == (0, 0) for p in pairs):
        return img
    if img.dtype not in (np.uint8, np.uint16):
        raise ValueError(f"the shift takes uint8 / uint16 images, got {img.dtype}")
    if not (1 <= img.shape[0] <= MAX_SIDE and 1 <= img.shape[1] <= MAX_SIDE):
        raise ValueError(f"the shift takes planes with sides in 1..{MAX_SIDE}, got {img.shape[0]} x {img.shape[1]}")
    if img.ndim == 2:
        return _shift_plane(img, *pairs[0])
    return np.stack([_shift_plane(img[:, :, c], *pairs[c]) for c in range(img.shape[2])], axis=2)


def read_shifted(path: str, sy, sx) -> np.ndarray:
    """One file as the run sees it: read, then shifted (the file itself with a zero shift)."""
    return shift_image(read_image(path), sy, sx)
