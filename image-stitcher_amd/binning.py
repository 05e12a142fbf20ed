"""--tile-binning: K x K binning of every tile before anything else sees it (include/squidstitch.h, sq_bin_tiles; an extension,
the reference has nothing like it).  This module holds what the host needs of it: the option check, the binned shape and the
binning of one image in numpy, for the readers that touch single files (the metadata probe, ``get_tile`` and the centre-pair
registration, the flatfield estimate's samples).  The staged tiles and the all-pairs stack are binned on the device.

For a plane I of h x w, uint8 or uint16 with maximum M, and an integer K:

    hb = h // K, wb = w // K        the last h - K hb rows and the last w - K wb columns are dropped
    S(y, x) = the sum of I over the K x K block at (K y, K x)
    mean:  floor(S / K^2)           the truncated mean, the rule of --pyramid-method mean
    sum :  min(S, M)                what camera binning does: counts add, and the result saturates

Integers only, so the device kernel and a second implementation (tests/bin_ref.py) agree bit for bit.  An RGB image is binned
per colour plane.  K = 1 is the identity."""
from __future__ import annotations

import numpy as np

from .tiffio import read_image

MAX_FACTOR = 8
METHODS = ('mean', 'sum')


def check_options(tile_binning, tile_binning_method):
    """The Stitcher's two arguments, validated: (int in 1..8, 'mean' or 'sum'); ValueError otherwise."""
    if isinstance(tile_binning, bool) or not isinstance(tile_binning, (int, np.integer)) or \
            not 1 <= int(tile_binning) <= MAX_FACTOR:
        raise ValueError(f"tile_binning must be an integer in 1..{MAX_FACTOR}, got {tile_binning!r}")
    if not isinstance(tile_binning_method, str) or tile_binning_method not in METHODS:
        raise ValueError(f"tile_binning_method must be 'mean' or 'sum', got {tile_binning_method!r}")
    return int(tile_binning), tile_binning_method


def binned_shape(h: int, w: int, factor: int):
    """(hb, wb) of an h x w plane; ValueError when the plane has no K x K block."""
    hb, wb = int(h) // int(factor), int(w) // int(factor)
    if hb < 1 or wb < 1:
        raise ValueError(f"tile_binning {factor} is larger than a side of the {h} x {w} tiles")
    return hb, wb


def bin_image(img: np.ndarray, factor: int, method: str = 'mean') -> np.ndarray:
    """``img`` [h, w] or [h, w, colours] (or a [1, h, w] page stack), uint8 / uint16, binned along h and w."""
    factor, method = check_options(factor, method)
    img = np.asarray(img)
    if factor == 1:
        return img
    if img.dtype not in (np.uint8, np.uint16):
        raise ValueError(f"binning takes uint8 / uint16 images, got {img.dtype}")
    if img.ndim == 3 and img.shape[0] == 1 and img.shape[2] != 3:      # a page stack of one page
        return bin_image(img[0], factor, method)[None]
    if img.ndim not in (2, 3):
        raise ValueError(f"binning takes [h, w] or [h, w, colours] images, got shape {img.shape}")
    hb, wb = binned_shape(img.shape[0], img.shape[1], factor)
    block = img[:hb * factor, :wb * factor].reshape((hb, factor, wb, factor) + img.shape[2:])
    s = block.sum(axis=(1, 3), dtype=np.uint32)
    if method == 'mean':
        return (s // np.uint32(factor * factor)).astype(img.dtype)
    return np.minimum(s, np.uint32(np.iinfo(img.dtype).max)).astype(img.dtype)


def read_binned(path: str, factor: int, method: str = 'mean') -> np.ndarray:
    """One file as the run sees it: read, then binned (the file itself with factor 1)."""
    img = read_image(path)
    return img if factor == 1 else bin_image(img, factor, method)
