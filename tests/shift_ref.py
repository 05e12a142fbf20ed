"""The definition of the per-channel translation (``--channel-shift``, sq_shift_tiles), in numpy, integers only.

For a plane I of h x w and S = (Sy, Sx), integers in 1/256 pixel, each in -16384..16384:

    U = w - 1, V = h - 1
    Y = clamp(256*y + Sy, 0, 256*V)      X = clamp(256*x + Sx, 0, 256*U)        (edges replicated)
    y0 = Y >> 8, fy = Y & 255, y1 = min(y0 + 1, V);   x0, fx, x1 likewise
    out(y, x) = ( I[y0,x0]*(256-fx)*(256-fy) + I[y0,x1]*fx*(256-fy)
                + I[y1,x0]*(256-fx)*fy       + I[y1,x1]*fx*fy + 32768 ) >> 16

``loop`` says it pixel by pixel in Python integers; ``shift_image`` is the vectorised form the tests compare against (it is
checked against ``loop``); ``separable`` is the form the device kernel uses (constant weights, clamped tap indices, the
horizontal blend first), which tests/test_channel_shift_cpu.py proves equal.  Written apart from
image-stitcher_amd/channelshift.py: neither imports the other."""
import numpy as np

MAX_SHIFT = 16384


def _check(planes, sy, sx):
    a = np.asarray(planes)
    assert a.dtype in (np.uint8, np.uint16) and a.ndim >= 2 and a.shape[-1] >= 1 and a.shape[-2] >= 1
    for s in (sy, sx):
        assert isinstance(s, int) and not isinstance(s, bool) and -MAX_SHIFT <= s <= MAX_SHIFT
    return a


def loop(plane, sy, sx):
    """[H, W] -> [H, W], one pixel at a time in Python integers."""
    a = _check(plane, sy, sx)
    h, w = a.shape
    U, V = w - 1, h - 1
    out = np.empty_like(a)
    for y in range(h):
        Y = min(max(256 * y + sy, 0), 256 * V)
        y0, fy = Y >> 8, Y & 255
        y1 = min(y0 + 1, V)
        for x in range(w):
            X = min(max(256 * x + sx, 0), 256 * U)
            x0, fx = X >> 8, X & 255
            x1 = min(x0 + 1, U)
            acc = int(a[y0, x0]) * (256 - fx) * (256 - fy) + int(a[y0, x1]) * fx * (256 - fy) \
                + int(a[y1, x0]) * (256 - fx) * fy + int(a[y1, x1]) * fx * fy + 32768
            out[y, x] = acc >> 16
    return out


def positions(n, s):
    """(first tap, second tap, fraction) of the n positions of one axis under the shift s, int64 [n] each."""
    last = n - 1
    p = np.minimum(np.maximum(np.arange(n, dtype=np.int64) * 256 + s, 0), 256 * last)
    first = p // 256
    return first, np.minimum(first + 1, last), p - 256 * first


def shift_image(planes, sy, sx):
    """[..., H, W] uint8 / uint16 -> the same shape and dtype: gathers through flat indices, blended in int64."""
    a = _check(planes, sy, sx)
    h, w = a.shape[-2:]
    y0, y1, fy = (v[:, None] for v in positions(h, sy))
    x0, x1, fx = (v[None, :] for v in positions(w, sx))
    flat = a.reshape(a.shape[:-2] + (h * w,)).astype(np.int64)
    tap = lambda yy, xx: np.take(flat, (yy * w + xx).ravel(), axis=-1).reshape(a.shape)
    gx, gy = 256 - fx, 256 - fy
    acc = tap(y0, x0) * (gx * gy) + tap(y0, x1) * (fx * gy) + tap(y1, x0) * (gx * fy) + tap(y1, x1) * (fx * fy) + 32768
    return (acc // 65536).astype(a.dtype)


def shift_file_image(img, sy, sx):
    """An image as a tile file holds it -- [H, W], or [H, W, 3] RGB shifted per colour plane, ``sy`` and ``sx`` then being
    triples."""
    img = np.asarray(img)
    if img.ndim == 3 and img.shape[2] == 3:
        return np.stack([shift_image(img[:, :, c], sy[c], sx[c]) for c in range(3)], axis=2)
    return shift_image(img, sy, sx)


def separable(planes, sy, sx):
    """The kernel's form: the constant weights (Sy & 255, Sx & 255), the taps at the clamped rows y + (Sy >> 8) and
    y + (Sy >> 8) + 1 and the columns likewise, the horizontal blend Hrow first (below 2^24), then the vertical one in
    unsigned 32 bits -> (the result, the largest Hrow, the largest vertical sum)."""
    a = _check(planes, sy, sx)
    h, w = a.shape[-2:]
    iy, ix, fy, fx = sy >> 8, sx >> 8, sy & 255, sx & 255      # (Python's >> on a negative int is the floor)
    ya = np.clip(np.arange(h) + iy, 0, h - 1)
    yb = np.clip(np.arange(h) + iy + 1, 0, h - 1)
    xa = np.clip(np.arange(w) + ix, 0, w - 1)
    xb = np.clip(np.arange(w) + ix + 1, 0, w - 1)
    v = a.astype(np.uint64)
    hrow = v[..., :, xa] * np.uint64(256 - fx) + v[..., :, xb] * np.uint64(fx)
    acc = hrow[..., ya, :] * np.uint64(256 - fy) + hrow[..., yb, :] * np.uint64(fy) + np.uint64(32768)
    return (acc >> np.uint64(16)).astype(a.dtype), int(hrow.max()), int(acc.max())
