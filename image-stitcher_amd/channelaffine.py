"""--channel-affine: per-channel rotation, scale and shear of every tile about its centre, composed with the channel's
--channel-shift (include/squidstitch.h, sq_affine_tiles; an extension, the reference has nothing like it).  This module holds what
the host needs of it: the option check and the map of one image in numpy, for the readers that touch single files (``get_tile``,
the flatfield estimate's samples).  The staged tiles are mapped on the device.

For a plane I of h x w, uint8 or uint16, S = (Sy, Sx) in 1/256 pixel, each in -16384..16384, and A = (Ayy, Ayx, Axy, Axx), integers
in parts per million, each in -50000..50000, with // the floor division:

    U = w - 1, V = h - 1
    for the output pixel (y, x):
      u = 2*x - U,  v = 2*y - V                                   half-pixels from the tile centre
      dv = Sy + (16*(Ayy*v + Ayx*u) + 62500) // 125000            1/256 px, rounded half up
      du = Sx + (16*(Axy*v + Axx*u) + 62500) // 125000
      Y = clamp(256*y + dv, 0, 256*V),  X = clamp(256*x + du, 0, 256*U)           edges replicated
      y0 = Y >> 8, fy = Y & 255, y1 = min(y0 + 1, V);   x0, fx, x1 likewise
      out(y, x) = ( I[y0,x0]*(256-fx)*(256-fy) + I[y0,x1]*fx*(256-fy)
                  + I[y1,x0]*(256-fx)*fy       + I[y1,x1]*fx*fy + 32768 ) >> 16

The output at centre + p takes the input at centre + (1 + A 10^-6) p + S/256: a point imaged at p in the reference channel and at
(1 + A 10^-6) p + S in channel NAME is put right.  A rotation by t is Ayy = Axx = (cos t - 1) 10^6, Ayx = -Axy = sin t 10^6; a
magnification m is Ayy = Axx = (m - 1) 10^6.  Integers only, so the device kernel and a second implementation
(tests/affine_ref.py) agree bit for bit.  An RGB image is mapped per colour plane, each with its own tuples.  With A = 0 this is
channelshift.shift_image."""
from __future__ import annotations

import re

import numpy as np

from .channelshift import MAX_SHIFT, MAX_SIDE

MAX_PPM = 50000
ZERO = (0, 0, 0, 0)
_INTEGER = re.compile(r'[+-]?[0-9]{1,6}\Z')


def _coefficient(value, what):
    if isinstance(value, bool) or not isinstance(value, int) or not -MAX_PPM <= value <= MAX_PPM:
        raise ValueError(f"{what} must be a Python int in -{MAX_PPM}..{MAX_PPM} (parts per million), got {value!r}")
    return value


def _shift_component(value):
    if isinstance(value, bool) or not isinstance(value, int) or not -MAX_SHIFT <= value <= MAX_SHIFT:
        raise ValueError(f"a shift must be a Python int in -{MAX_SHIFT}..{MAX_SHIFT} (1/256 pixel), got {value!r}")
    return value


def check_option(channel_affines):
    """The Stitcher's argument, validated: None or a mapping of channel name -> (Ayy, Ayx, Axy, Axx), Python ints in parts per
    million within -50000..50000 (bools, floats and strings are refused) -> a plain dict without the all-zero entries."""
    if channel_affines is None:
        return {}
    if not hasattr(channel_affines, 'items'):
        raise ValueError(f"channel_affines must be a mapping of channel name -> (Ayy, Ayx, Axy, Axx), got {channel_affines!r}")
    checked = {}
    for name, coeffs in channel_affines.items():
        if not isinstance(name, str):
            raise ValueError(f"channel_affines: a channel name must be a string, got {name!r}")
        if isinstance(coeffs, (str, bytes)) or not hasattr(coeffs, '__len__') or len(coeffs) != 4:
            raise ValueError(f"channel_affines[{name!r}] must be four integers (Ayy, Ayx, Axy, Axx), got {coeffs!r}")
        a = tuple(_coefficient(v, f"channel_affines[{name!r}]") for v in coeffs)
        if a != ZERO:
            checked[name] = a
    return checked


def parse_ppm(text) -> int:
    """The CLI's text -> parts per million: a plain integer literal in -50000..50000; ValueError otherwise."""
    if not isinstance(text, str) or not _INTEGER.match(text):
        raise ValueError(f"a coefficient is a plain integer of parts per million in -{MAX_PPM}..{MAX_PPM}, got {text!r}")
    return _coefficient(int(text), 'a coefficient')


def displacement(h: int, w: int, s, a):
    """(dv, du) of every position of an h x w plane, int64 [h, w] each, in 1/256 pixel."""
    v = (2 * np.arange(h, dtype=np.int64) - (h - 1))[:, None]
    u = (2 * np.arange(w, dtype=np.int64) - (w - 1))[None, :]
    # (numpy's // on int64 is the floor division)
    dv = s[0] + (16 * (a[0] * v + a[1] * u) + 62500) // 125000
    du = s[1] + (16 * (a[2] * v + a[3] * u) + 62500) // 125000
    return dv, du


def max_displacement(h: int, w: int, s, a):
    """(largest |dv|, largest |du|) over the plane, in 1/256 pixel: both are linear, so the corners hold the extremes."""
    v, u = (-(h - 1), h - 1), (-(w - 1), w - 1)
    dv = [s[0] + (16 * (a[0] * vv + a[1] * uu) + 62500) // 125000 for vv in v for uu in u]
    du = [s[1] + (16 * (a[2] * vv + a[3] * uu) + 62500) // 125000 for vv in v for uu in u]
    return max(abs(d) for d in dv), max(abs(d) for d in du)


def _affine_plane(img: np.ndarray, s, a) -> np.ndarray:
    h, w = img.shape
    dv, du = displacement(h, w, s, a)
    ys = np.clip(256 * np.arange(h, dtype=np.int64)[:, None] + dv, 0, 256 * (h - 1))
    xs = np.clip(256 * np.arange(w, dtype=np.int64)[None, :] + du, 0, 256 * (w - 1))
    x0, fx, y0, fy = xs >> 8, xs & 255, ys >> 8, ys & 255
    x1, y1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)
    i = img.astype(np.int64)
    acc = i[y0, x0] * ((256 - fx) * (256 - fy)) + i[y0, x1] * (fx * (256 - fy)) + i[y1, x0] * ((256 - fx) * fy) + \
        i[y1, x1] * (fx * fy) + 32768
    return (acc >> 16).astype(img.dtype)


def _tuples(s, a, colours):
    """(S, A) per colour plane: one pair and one four-tuple for all of them, or sequences of one each per plane."""
    per_plane_s = len(s) == colours and all(isinstance(v, (list, tuple)) for v in s)
    per_plane_a = len(a) == colours and all(isinstance(v, (list, tuple)) for v in a)
    if per_plane_s != per_plane_a:
        raise ValueError(f"an image of {colours} colour planes takes {colours} shifts and {colours} coefficient tuples, or one of each")
    pairs = list(zip(s, a)) if per_plane_s else [(s, a)] * colours
    out = []
    for ss, aa in pairs:
        if len(ss) != 2 or len(aa) != 4:
            raise ValueError(f"a map is a pair (Sy, Sx) and four coefficients (Ayy, Ayx, Axy, Axx), got {ss!r}, {aa!r}")
        out.append((tuple(_shift_component(v) for v in ss), tuple(_coefficient(v, 'a coefficient') for v in aa)))
    return out


def affine_image(img: np.ndarray, s, a) -> np.ndarray:
    """``img`` [h, w], a [1, h, w] page stack, or [h, w, 3] mapped per colour plane (``s`` and ``a`` then may be sequences of one
    pair and one four-tuple per plane), uint8 / uint16, under S = ``s`` (1/256 pixel) and A = ``a`` (parts per million)."""
    img = np.asarray(img)
    if img.ndim == 3 and img.shape[0] == 1 and img.shape[2] != 3:      # a page stack of one page
        return affine_image(img[0], s, a)[None]
    if img.ndim not in (2, 3):
        raise ValueError(f"the map takes [h, w] or [h, w, colours] images, got shape {img.shape}")
    maps = _tuples(s, a, 1 if img.ndim == 2 else img.shape[2])
    if all(m == ((0, 0), ZERO) for m in maps):
        return img
    if img.dtype not in (np.uint8, np.uint16):
        raise ValueError(f"the map takes uint8 / uint16 images, got {img.dtype}")
    if not (1 <= img.shape[0] <= MAX_SIDE and 1 <= img.shape[1] <= MAX_SIDE):
        raise ValueError(f"the map takes planes with sides in 1..{MAX_SIDE}, got {img.shape[0]} x {img.shape[1]}")
    if img.ndim == 2:
        return _affine_plane(img, *maps[0])
    return np.stack([_affine_plane(img[:, :, c], *maps[c]) for c in range(img.shape[2])], axis=2)
