"""The definition of the radial lens correction (``--distortion-correction``, sq_warp_tiles), in numpy, integers only.

For a plane I of h x w (h, w <= 65535), uint8 or uint16, and an integer D in parts per million, -50000 <= D <= 50000, with //
the floor division (also of negative numerators):

    U = w - 1, V = h - 1                         R2 = max(1, U*U + V*V)
    for the output pixel (y, x):
      u = 2*x - U,  v = 2*y - V                  (half-pixels from the tile centre)
      rho = ((u*u + v*v) << 24) // R2            (0 .. 2^24: squared radius, 1.0 at the corners)
      s   = D * rho
      du  = (u*s + H) // (2*H),  dv = (v*s + H) // (2*H),   H = 10^6 * 2^16      (1/256 pixel, rounded half up)
      X = clamp(256*x + du, 0, 256*U),  Y = clamp(256*y + dv, 0, 256*V)           (edges replicated)
      x0 = X >> 8, fx = X & 255, x1 = min(x0 + 1, U);   y0, fy, y1 likewise
      out(y, x) = ( I[y0,x0]*(256-fx)*(256-fy) + I[y0,x1]*fx*(256-fy)
                  + I[y1,x0]*(256-fx)*fy       + I[y1,x1]*fx*fy + 32768 ) >> 16

The output at radius r takes the input at radius r (1 + D 1e-6 r^2 / R^2).  RGB files are corrected per colour plane
(``warp_file_image``).  Written apart from image_stitcher_amd/distortion.py: neither imports the other.  Not a test module."""
import numpy as np

MAX_PPM = 50000
MAX_SIDE = 65535
H = 10 ** 6 * 2 ** 16


def _check(a, ppm):
    a = np.asarray(a)
    if a.dtype not in (np.uint8, np.uint16) or a.ndim < 2:
        raise ValueError("uint8 / uint16 planes [..., H, W]")
    if isinstance(ppm, bool) or not isinstance(ppm, (int, np.integer)) or not -MAX_PPM <= int(ppm) <= MAX_PPM:
        raise ValueError("an integer ppm in -50000..50000")
    if not (1 <= a.shape[-2] <= MAX_SIDE and 1 <= a.shape[-1] <= MAX_SIDE):
        raise ValueError("sides in 1..65535")
    return a, int(ppm)


def pixel_map(h, w, ppm, y, x):
    """(du, dv, X, Y) of one output pixel, word for word, in Python integers."""
    U, V = w - 1, h - 1
    R2 = max(1, U * U + V * V)
    u, v = 2 * x - U, 2 * y - V
    rho = ((u * u + v * v) << 24) // R2
    s = ppm * rho
    du, dv = (u * s + H) // (2 * H), (v * s + H) // (2 * H)
    X = min(max(256 * x + du, 0), 256 * U)
    Y = min(max(256 * y + dv, 0), 256 * V)
    return du, dv, X, Y


def loop(plane, ppm):
    """The definition word for word, pixel by pixel, in Python integers (one [H, W] plane)."""
    a, ppm = _check(plane, ppm)
    h, w = a.shape
    U, V = w - 1, h - 1
    out = np.zeros((h, w), dtype=a.dtype)
    for y in range(h):
        for x in range(w):
            _, _, X, Y = pixel_map(h, w, ppm, y, x)
            x0, fx, y0, fy = X >> 8, X & 255, Y >> 8, Y & 255
            x1, y1 = min(x0 + 1, U), min(y0 + 1, V)
            acc = int(a[y0, x0]) * (256 - fx) * (256 - fy) + int(a[y0, x1]) * fx * (256 - fy) \
                + int(a[y1, x0]) * (256 - fx) * fy + int(a[y1, x1]) * fx * fy + 32768
            out[y, x] = acc >> 16
    return out


def maps(h, w, ppm):
    """(du, dv, X, Y), int64 [h, w] each: the displacements before the clamp and the clamped sample positions, all in 1/256
    pixel.  Floor division by hand -- truncate towards zero on magnitudes, then step down where a negative numerator left a
    remainder -- so that nothing here leans on what ``//`` does to negative int64."""
    U, V = w - 1, h - 1
    R2 = max(1, U * U + V * V)
    v, u = np.meshgrid(2 * np.arange(h, dtype=np.int64) - V, 2 * np.arange(w, dtype=np.int64) - U, indexing='ij')
    rho = np.left_shift(u * u + v * v, 24) // R2                 # (non-negative)
    s = rho * np.int64(ppm)

    def rounded(c):
        n = c * s + H
        mag = np.abs(n)
        q = mag // (2 * H)
        exact = (mag % (2 * H)) == 0
        return np.where(n >= 0, q, np.where(exact, -q, -q - 1))
    du, dv = rounded(u), rounded(v)
    xs = np.arange(w, dtype=np.int64)[None, :] * 256 + du
    ys = np.arange(h, dtype=np.int64)[:, None] * 256 + dv
    X = np.minimum(np.maximum(xs, 0), 256 * U)
    Y = np.minimum(np.maximum(ys, 0), 256 * V)
    return du, dv, X, Y


def warp_image(planes, ppm):
    """[..., H, W] uint8 / uint16 -> the same shape and dtype: gathers through flat indices, blended in int64."""
    a, ppm = _check(planes, ppm)
    h, w = a.shape[-2:]
    _, _, X, Y = maps(h, w, ppm)
    x0, y0 = X // 256, Y // 256
    fx, fy = X - 256 * x0, Y - 256 * y0
    x1, y1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)
    flat = a.reshape(a.shape[:-2] + (h * w,)).astype(np.int64)
    tap = lambda yy, xx: np.take(flat, (yy * w + xx).ravel(), axis=-1).reshape(a.shape)
    gx, gy = 256 - fx, 256 - fy
    acc = tap(y0, x0) * (gx * gy) + tap(y0, x1) * (fx * gy) + tap(y1, x0) * (gx * fy) + tap(y1, x1) * (fx * fy) + 32768
    return (acc // 65536).astype(a.dtype)


def warp_file_image(img, ppm):
    """An image as a tile file holds it -- [H, W], or [H, W, 3] RGB corrected per colour plane."""
    img = np.asarray(img)
    if img.ndim == 3 and img.shape[2] == 3:
        return np.stack([warp_image(img[:, :, c], ppm) for c in range(3)], axis=2)
    return warp_image(img, ppm)


def clamp_active(h, w, ppm):
    """{'left', 'right', 'top', 'bottom'} -> whether the clamp changes a sample position on that border."""
    du, dv, X, Y = maps(h, w, ppm)
    xs = np.arange(w, dtype=np.int64)[None, :] * 256 + du
    ys = np.arange(h, dtype=np.int64)[:, None] * 256 + dv
    return {'left': bool((xs[:, 0] != X[:, 0]).any()), 'right': bool((xs[:, -1] != X[:, -1]).any()),
            'top': bool((ys[0] != Y[0]).any()), 'bottom': bool((ys[-1] != Y[-1]).any())}
