"""--distortion-correction: radial lens correction of every tile before anything else sees it (include/squidstitch.h,
sq_warp_tiles; an extension, the reference has nothing like it).  This module holds what the host needs of it: the option check,
the map and the correction of one image in numpy, for the readers that touch single files (``get_tile`` and the centre-pair
registration, the flatfield estimate's samples).  The staged tiles and the all-pairs stack are corrected on the device.

For a plane I of h x w, uint8 or uint16, and an integer D in parts per million, -50000..50000, with // the floor division:

    U = w - 1, V = h - 1                         R2 = max(1, U*U + V*V)
    for the output pixel (y, x):
      u = 2*x - U,  v = 2*y - V                  half-pixels from the tile centre
      rho = ((u*u + v*v) << 24) // R2            0 .. 2^24: squared radius, 1.0 at the corners
      s   = D * rho
      du  = (u*s + H) // (2*H),  dv = (v*s + H) // (2*H),   H = 10^6 * 2^16      1/256 pixel, rounded half up
      X = clamp(256*x + du, 0, 256*U),  Y = clamp(256*y + dv, 0, 256*V)           edges replicated
      x0 = X >> 8, fx = X & 255, x1 = min(x0 + 1, U);   y0, fy, y1 likewise
      out(y, x) = ( I[y0,x0]*(256-fx)*(256-fy) + I[y0,x1]*fx*(256-fy)
                  + I[y1,x0]*(256-fx)*fy       + I[y1,x1]*fx*fy + 32768 ) >> 16

The output at radius r takes the input at radius r (1 + D 10^-6 r^2 / R^2), bilinearly with 8 fractional bits: D is the
relative displacement at the tile's corner; positive D samples farther out and so pulls content towards the centre, which
undoes pincushion distortion, negative D undoes barrel distortion.  Integers only, so the device kernel and a second
implementation (tests/warp_ref.py) agree bit for bit.  An RGB image is corrected per colour plane.  D = 0 is the identity."""
from __future__ import annotations

import numpy as np

from .tiffio import read_image

MAX_PPM = 50000
MAX_SIDE = 65535
HALF = 10 ** 6 * 2 ** 16


def check_option(distortion_correction):
    """The Stitcher's argument, validated: an int in -50000..50000; ValueError otherwise (bools, floats and strings too)."""
    if isinstance(distortion_correction, bool) or not isinstance(distortion_correction, (int, np.integer)) or \
            not -MAX_PPM <= int(distortion_correction) <= MAX_PPM:
        raise ValueError(f"distortion_correction must be an integer in -{MAX_PPM}..{MAX_PPM} (parts per million), got "
                         f"{distortion_correction!r}")
    return int(distortion_correction)


def displacement_map(h: int, w: int, ppm: int):
    """(du, dv), int64 [h, w]: the displacement of every output pixel's sample in 1/256 pixel, before the clamp."""
    h, w, ppm = int(h), int(w), check_option(ppm)
    if not (1 <= h <= MAX_SIDE and 1 <= w <= MAX_SIDE):
        raise ValueError(f"the correction takes planes with sides in 1..{MAX_SIDE}, got {h} x {w}")
    u = (2 * np.arange(w, dtype=np.int64) - (w - 1))[None, :]
    v = (2 * np.arange(h, dtype=np.int64) - (h - 1))[:, None]
    r2 = max(1, (w - 1) ** 2 + (h - 1) ** 2)
    s = ppm * (((u * u + v * v) << 24) // r2)
    return (u * s + HALF) // (2 * HALF), (v * s + HALF) // (2 * HALF)      # (numpy's // floors, as Python's does)


def max_displacement(h: int, w: int, ppm: int):
    """(max |du|, max |dv|) of the map in 1/256 pixel, as Python integers.  rho grows with |u| and with |v| and the rounding is
    monotone, so both are reached at a corner: the four corners are evaluated."""
    h, w, ppm = int(h), int(w), check_option(ppm)
    if not (1 <= h <= MAX_SIDE and 1 <= w <= MAX_SIDE):
        raise ValueError(f"the correction takes planes with sides in 1..{MAX_SIDE}, got {h} x {w}")
    r2 = max(1, (w - 1) ** 2 + (h - 1) ** 2)
    du = dv = 0
    for u in (w - 1, 1 - w):
        for v in (h - 1, 1 - h):
            s = ppm * (((u * u + v * v) << 24) // r2)
            du, dv = max(du, abs((u * s + HALF) // (2 * HALF))), max(dv, abs((v * s + HALF) // (2 * HALF)))
    return du, dv


def _warp_plane(img: np.ndarray, du: np.ndarray, dv: np.ndarray) -> np.ndarray:
    h, w = img.shape
    xs = np.clip(256 * np.arange(w, dtype=np.int64)[None, :] + du, 0, 256 * (w - 1))
    ys = np.clip(256 * np.arange(h, dtype=np.int64)[:, None] + dv, 0, 256 * (h - 1))
    x0, fx, y0, fy = xs >> 8, xs & 255, ys >> 8, ys & 255
    x1, y1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)
    a = img.astype(np.int64)
    acc = a[y0, x0] * ((256 - fx) * (256 - fy)) + a[y0, x1] * (fx * (256 - fy)) + a[y1, x0] * ((256 - fx) * fy) + \
        a[y1, x1] * (fx * fy) + 32768
    return (acc >> 16).astype(img.dtype)


def warp_image(img: np.ndarray, ppm: int) -> np.ndarray:
    """``img`` [h, w] or [h, w, colours] (or a [1, h, w] page stack), uint8 / uint16, corrected along h and w."""
    ppm = check_option(ppm)
    img = np.asarray(img)
    if ppm == 0:
        return img
    if img.dtype not in (np.uint8, np.uint16):
        raise ValueError(f"the correction takes uint8 / uint16 images, got {img.dtype}")
    if img.ndim == 3 and img.shape[0] == 1 and img.shape[2] != 3:      # a page stack of one page
        return warp_image(img[0], ppm)[None]
    if img.ndim not in (2, 3):
        raise ValueError(f"the correction takes [h, w] or [h, w, colours] images, got shape {img.shape}")
    du, dv = displacement_map(img.shape[0], img.shape[1], ppm)
    if img.ndim == 2:
        return _warp_plane(img, du, dv)
    return np.stack([_warp_plane(img[:, :, c], du, dv) for c in range(img.shape[2])], axis=2)


def read_warped(path: str, ppm: int) -> np.ndarray:
    """One file as the run sees it: read, then corrected (the file itself with ppm 0)."""
    img = read_image(path)
    return img if ppm == 0 else warp_image(img, ppm)
