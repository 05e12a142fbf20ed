"""The definition of the dark-frame subtraction (--dark-frame; include/squidstitch.h, sq_dark_tiles), restated in numpy and as a
per-pixel loop.  For a plane I [h, w] of dtype maximum M (255 or 65535), a dark frame D [h, w] of the same dtype (or a constant)
and a pedestal P in 0..M:

    out(y, x) = clamp(I(y, x) - D(y, x) + P, 0, M)

taken in a wider signed type.  Written apart from image_stitcher_amd/darkframe.py: neither imports the other."""
import numpy as np


def _top(dtype) -> int:
    dtype = np.dtype(dtype)
    if dtype not in (np.dtype('uint8'), np.dtype('uint16')):
        raise ValueError(f'uint8 / uint16 images, got {dtype}')
    return int(np.iinfo(dtype).max)


def _frame(frame_or_int, shape, dtype):
    if isinstance(frame_or_int, (int, np.integer)) and not isinstance(frame_or_int, bool):
        if not 0 <= int(frame_or_int) <= _top(dtype):
            raise ValueError(f'a constant frame lies in 0..{_top(dtype)}, got {frame_or_int}')
        return np.full(shape, int(frame_or_int), dtype=np.int64)
    frame = np.asarray(frame_or_int)
    if frame.shape != tuple(shape) or frame.dtype != np.dtype(dtype):
        raise ValueError(f'a frame of {frame.dtype} {frame.shape} for planes of {np.dtype(dtype)} {tuple(shape)}')
    return frame.astype(np.int64)


def dark_image(img, frame_or_int, pedestal=0):
    """``img`` [h, w] or a stack [n, h, w] with one frame [h, w] (or an int) for all its planes, or [h, w, 3] with a list of one
    frame (or int, or None: the plane stays as it is) per colour plane."""
    img = np.asarray(img)
    top = _top(img.dtype)
    if isinstance(pedestal, bool) or not isinstance(pedestal, (int, np.integer)) or not 0 <= pedestal <= top:
        raise ValueError(f'a pedestal lies in 0..{top}, got {pedestal!r}')
    if isinstance(frame_or_int, (list, tuple)):
        if img.ndim != 3 or img.shape[2] != len(frame_or_int):
            raise ValueError('one frame per colour plane')
        planes = [img[:, :, c] if f is None else dark_image(img[:, :, c], f, pedestal) for c, f in enumerate(frame_or_int)]
        return np.stack(planes, axis=2)
    if img.ndim == 3 and img.shape[2] == 3 and img.shape[0] != 1 and not isinstance(frame_or_int, (int, np.integer)) \
            and np.asarray(frame_or_int).shape == img.shape[:2]:
        return dark_image(img, [frame_or_int] * 3, pedestal)
    d = _frame(frame_or_int, img.shape[-2:], img.dtype)
    return np.clip(img.astype(np.int64) - d + int(pedestal), 0, top).astype(img.dtype)


def dark_file_image(img, frame_or_int, pedestal=0):
    """A tile file's image as read -- [h, w], a [1, h, w] page stack, or [h, w, 3] -- subtracted, in the file's layout."""
    return dark_image(img, frame_or_int, pedestal)


def loop(img, frame_or_int, pedestal=0):
    """The definition pixel by pixel in Python integers (small planes only)."""
    img = np.asarray(img)
    top = _top(img.dtype)
    h, w = img.shape
    out = np.empty_like(img)
    for y in range(h):
        for x in range(w):
            d = int(frame_or_int) if isinstance(frame_or_int, (int, np.integer)) else int(frame_or_int[y][x])
            v = int(img[y][x]) - d + int(pedestal)
            out[y][x] = 0 if v < 0 else (top if v > top else v)
    return out
