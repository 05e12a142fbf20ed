"""--dark-frame: per-channel subtraction of the camera's additive term from every tile before anything else sees it
(include/squidstitch.h, sq_dark_tiles; an extension, the reference has nothing like it).  This module holds what the host needs
of it: the option check, the CLI's source parser, the frame loader and the subtraction of one image in numpy, for the readers
that touch single files (``get_tile``, the centre-pair registration, the flatfield estimate's samples).  The staged tiles are
subtracted on the device.

For a plane I of h x w with dtype maximum M (255 or 65535), a dark frame D of h x w and the same dtype (or a constant) and a
pedestal P in 0..M:

    out(y, x) = clamp(I(y, x) - D(y, x) + P, 0, M)

taken in a wider signed type.  Integers only, so the device kernel and a second implementation (tests/dark_ref.py) agree bit for
bit.  An RGB image is subtracted per colour plane, each with its own frame.  A constant frame equal to P is the identity."""
from __future__ import annotations

import hashlib
import os

import numpy as np

from .tiffio import read_image

WILDCARD = '*'
EXTENSIONS = ('.tif', '.tiff', '.npy')
ORDER = 'first: before the distortion correction, the channel shift / affine and the binning'


def _is_int(value) -> bool:
    return isinstance(value, (int, np.integer)) and not isinstance(value, (bool, np.bool_))


def check_option(dark_frames, dark_pedestal=0):
    """The Stitcher's arguments, validated as far as they can be without the files: None or a mapping of channel name (or '*')
    -> a non-negative int (a constant frame), a 2-D uint8 / uint16 array, or the path of a .tif / .tiff / .npy; the pedestal a
    non-negative int -> (a plain dict, the pedestal).  Shape, dtype and the dtype's maximum are checked by ``load_frame``."""
    if not _is_int(dark_pedestal) or not 0 <= int(dark_pedestal) <= 65535:
        raise ValueError(f"dark_pedestal must be an integer in 0..the dtype's maximum, got {dark_pedestal!r}")
    if dark_frames is None:
        return {}, int(dark_pedestal)
    if not hasattr(dark_frames, 'items'):
        raise ValueError(f"dark_frames must be a mapping of channel name -> int, array or path, got {dark_frames!r}")
    checked = {}
    for name, source in dark_frames.items():
        if not isinstance(name, str):
            raise ValueError(f"dark_frames: a channel name must be a string, got {name!r}")
        if _is_int(source):
            if int(source) < 0:
                raise ValueError(f"dark_frames[{name!r}]: a constant frame is a non-negative integer, got {source!r}")
            source = int(source)
        elif isinstance(source, np.ndarray):
            if source.ndim != 2 or source.dtype not in (np.uint8, np.uint16):
                raise ValueError(f"dark_frames[{name!r}]: a frame is a 2-D uint8 / uint16 array, got {source.dtype} of shape "
                                 f"{source.shape}")
        elif isinstance(source, (str, os.PathLike)):
            source = os.fspath(source)
            if not source.lower().endswith(EXTENSIONS):
                raise ValueError(f"dark_frames[{name!r}]: a frame file is a .tif, .tiff or .npy, got {source!r}")
        else:
            raise ValueError(f"dark_frames[{name!r}] must be an int, a 2-D array or a path, got {source!r}")
        checked[name] = source
    return checked, int(dark_pedestal)


def parse_source(text):
    """The CLI's SOURCE: a plain non-negative decimal integer -> int (a constant frame), anything else -> the path it names
    (a .tif, .tiff or .npy); ValueError otherwise."""
    if not isinstance(text, str) or not text:
        raise ValueError(f"a dark frame's source is an integer or the path of a .tif, .tiff or .npy, got {text!r}")
    if text.isascii() and text.isdigit():
        return int(text)
    if not text.lower().endswith(EXTENSIONS):
        raise ValueError(f"a dark frame's source is a plain non-negative integer or the path of a .tif, .tiff or .npy, got {text!r}")
    return text


def load_frame(source, shape, dtype, name=WILDCARD):
    """``source`` of channel ``name`` as the run uses it: an int in 0..M stays an int, an array or a file becomes a contiguous
    array of exactly ``shape`` and ``dtype``; ValueError, with one message each, for a constant above M, a missing file and a
    frame of another shape or dtype."""
    dtype = np.dtype(dtype)
    top = int(np.iinfo(dtype).max)
    if _is_int(source):
        if not 0 <= int(source) <= top:
            raise ValueError(f"dark_frames[{name!r}]: the constant {source} is outside 0..{top}, the range of {dtype.name} tiles")
        return int(source)
    where = 'an array'
    if isinstance(source, (str, os.PathLike)):
        where = os.fspath(source)
        if not os.path.isfile(where):
            raise ValueError(f"dark_frames[{name!r}]: no such file: {where}")
        frame = np.load(where, allow_pickle=False) if where.lower().endswith('.npy') else read_image(where)
        if frame.ndim == 3 and frame.shape[0] == 1:      # a page stack of one page
            frame = frame[0]
    else:
        frame = np.asarray(source)
    if frame.ndim != 2 or tuple(frame.shape) != tuple(shape) or frame.dtype != dtype:
        raise ValueError(f"dark_frames[{name!r}]: {where} is {frame.dtype} of shape {tuple(frame.shape)}; the tile files are "
                         f"{dtype.name} of shape {tuple(shape)}, and a frame has exactly their shape and dtype")
    return np.ascontiguousarray(frame)


def check_pedestal(pedestal, dtype) -> int:
    top = int(np.iinfo(np.dtype(dtype)).max)
    if not 0 <= pedestal <= top:
        raise ValueError(f"dark_pedestal {pedestal} is outside 0..{top}, the range of {np.dtype(dtype).name} tiles")
    return pedestal


def is_identity(frame, pedestal) -> bool:
    """A constant frame equal to the pedestal changes nothing."""
    return frame is None or (_is_int(frame) and int(frame) == pedestal)


def frame_note(source, frame):
    """What the sidecar says of one channel: the constant, or where the frame came from, the SHA-256 of its bytes and its
    min / max / integer mean."""
    if _is_int(frame):
        return {'constant': int(frame)}
    return {'path': source if isinstance(source, str) else None, 'sha256': hashlib.sha256(frame.tobytes()).hexdigest(),
            'min': int(frame.min()), 'max': int(frame.max()), 'mean': int(frame.sum(dtype=np.int64)) // frame.size}


def param_runs(params, pedestal):
    """The grids sq_dark_tiles issues for a table of (k, c) pairs: one (first, last, k, c) per maximal run of consecutive equal
    pairs, the runs that are the identity (k == -1, c == pedestal) left out."""
    runs, s0, pairs = [], 0, [tuple(int(v) for v in p) for p in params]
    while s0 < len(pairs):
        s1 = s0 + 1
        while s1 < len(pairs) and pairs[s1] == pairs[s0]:
            s1 += 1
        if pairs[s0] != (-1, pedestal):
            runs.append((s0, s1) + pairs[s0])
        s0 = s1
    return runs


def _dark_plane(img, frame, pedestal):
    if is_identity(frame, pedestal):
        return img
    top = int(np.iinfo(img.dtype).max)
    if not _is_int(frame) and (frame.shape != img.shape or frame.dtype != img.dtype):
        raise ValueError(f"a frame of {frame.dtype} {frame.shape} does not fit an image of {img.dtype} {img.shape}")
    wide = img.astype(np.int64) - (int(frame) if _is_int(frame) else frame.astype(np.int64)) + pedestal
    return np.clip(wide, 0, top).astype(img.dtype)


def dark_image(img: np.ndarray, frame, pedestal: int = 0) -> np.ndarray:
    """``img`` [h, w], a [1, h, w] page stack, or [h, w, 3] subtracted per colour plane (``frame`` then may be a list of one
    frame per plane), uint8 / uint16; a frame is an int, an array of the plane's shape and dtype, or None (the identity)."""
    img = np.asarray(img)
    if img.ndim == 3 and img.shape[0] == 1 and img.shape[2] != 3:      # a page stack of one page
        return dark_image(img[0], frame, pedestal)[None]
    if img.ndim not in (2, 3):
        raise ValueError(f"the dark frame takes [h, w] or [h, w, colours] images, got shape {img.shape}")
    if img.dtype not in (np.uint8, np.uint16):
        raise ValueError(f"the dark frame takes uint8 / uint16 images, got {img.dtype}")
    if not _is_int(pedestal) or not 0 <= pedestal <= int(np.iinfo(img.dtype).max):
        raise ValueError(f"the pedestal is an integer in 0..{int(np.iinfo(img.dtype).max)}, got {pedestal!r}")
    colours = 1 if img.ndim == 2 else img.shape[2]
    frames = list(frame) if isinstance(frame, (list, tuple)) else [frame] * colours
    if len(frames) != colours:
        raise ValueError(f"an image of {colours} colour planes takes {colours} frames")
    if all(is_identity(f, pedestal) for f in frames):
        return img
    if img.ndim == 2:
        return _dark_plane(img, frames[0], pedestal)
    return np.stack([_dark_plane(img[:, :, c], frames[c], pedestal) for c in range(colours)], axis=2)
