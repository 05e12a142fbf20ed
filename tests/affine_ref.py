"""The definition of the per-channel affine map (``--channel-affine``, sq_affine_tiles), in numpy, integers only.

For a plane I of h x w, S = (Sy, Sx), integers in 1/256 pixel, each in -16384..16384, and A = (Ayy, Ayx, Axy, Axx), integers in
parts per million, each in -50000..50000, with // the floor division, also of negative numerators:

    U = w - 1, V = h - 1
    u = 2*x - U,  v = 2*y - V                                   (half-pixels from the tile centre)
    dv = Sy + (16*(Ayy*v + Ayx*u) + 62500) // 125000            (1/256 px, rounded half up: 128/10^6 = 16/125000)
    du = Sx + (16*(Axy*v + Axx*u) + 62500) // 125000
    Y = clamp(256*y + dv, 0, 256*V),  X = clamp(256*x + du, 0, 256*U)        (edges replicated)
    y0 = Y >> 8, fy = Y & 255, y1 = min(y0 + 1, V);   x0, fx, x1 likewise
    out(y, x) = ( I[y0,x0]*(256-fx)*(256-fy) + I[y0,x1]*fx*(256-fy)
                + I[y1,x0]*(256-fx)*fy       + I[y1,x1]*fx*fy + 32768 ) >> 16

``loop`` says it pixel by pixel in Python integers; ``affine_image`` is the vectorised form the tests compare against (it is
checked against ``loop``), with the floor division done by hand; ``kernel_form`` is the way the device kernel gets at the same
map and taps (the quotient and remainder of a vector's first column stepped along the row, the taps picked out of a span of
VEC + 2 columns of two or three rows, rows and the span's last pair clamped into the plane), which
tests/test_channel_affine_cpu.py proves equal.  Written apart from image-stitcher_amd/channelaffine.py: neither imports the other."""
import numpy as np

MAX_SHIFT = 16384
MAX_PPM = 50000
DEN = 125000


def _check(planes, s, a):
    p = np.asarray(planes)
    assert p.dtype in (np.uint8, np.uint16) and p.ndim >= 2 and p.shape[-1] >= 1 and p.shape[-2] >= 1
    assert len(s) == 2 and len(a) == 4
    for c in s:
        assert isinstance(c, int) and not isinstance(c, bool) and -MAX_SHIFT <= c <= MAX_SHIFT
    for c in a:
        assert isinstance(c, int) and not isinstance(c, bool) and -MAX_PPM <= c <= MAX_PPM
    return p


def loop(plane, s, a):
    """[H, W] -> [H, W], one pixel at a time in Python integers (whose // is the floor division)."""
    p = _check(plane, s, a)
    h, w = p.shape
    U, V = w - 1, h - 1
    out = np.empty_like(p)
    for y in range(h):
        v = 2 * y - V
        for x in range(w):
            u = 2 * x - U
            dv = s[0] + (16 * (a[0] * v + a[1] * u) + 62500) // 125000
            du = s[1] + (16 * (a[2] * v + a[3] * u) + 62500) // 125000
            Y = min(max(256 * y + dv, 0), 256 * V)
            X = min(max(256 * x + du, 0), 256 * U)
            y0, fy, x0, fx = Y >> 8, Y & 255, X >> 8, X & 255
            y1, x1 = min(y0 + 1, V), min(x0 + 1, U)
            acc = int(p[y0, x0]) * (256 - fx) * (256 - fy) + int(p[y0, x1]) * fx * (256 - fy) \
                + int(p[y1, x0]) * (256 - fx) * fy + int(p[y1, x1]) * fx * fy + 32768
            out[y, x] = acc >> 16
    return out


def _floor_div(n, d):
    """Floor division by hand -- truncate towards zero on magnitudes, then step down where a negative numerator left a
    remainder -- so that nothing here leans on what ``//`` does to negative int64."""
    mag = np.abs(n)
    q = mag // d
    exact = (mag % d) == 0
    return np.where(n >= 0, q, np.where(exact, -q, -q - 1))


def maps(h, w, s, a):
    """(dv, du, Y, X), int64 [h, w] each: the displacements before the clamp and the clamped sample positions, in 1/256 pixel."""
    U, V = w - 1, h - 1
    v, u = np.meshgrid(2 * np.arange(h, dtype=np.int64) - V, 2 * np.arange(w, dtype=np.int64) - U, indexing='ij')
    dv = s[0] + _floor_div(16 * (np.int64(a[0]) * v + np.int64(a[1]) * u) + 62500, DEN)
    du = s[1] + _floor_div(16 * (np.int64(a[2]) * v + np.int64(a[3]) * u) + 62500, DEN)
    Y = np.minimum(np.maximum(np.arange(h, dtype=np.int64)[:, None] * 256 + dv, 0), 256 * V)
    X = np.minimum(np.maximum(np.arange(w, dtype=np.int64)[None, :] * 256 + du, 0), 256 * U)
    return dv, du, Y, X


def affine_image(planes, s, a):
    """[..., H, W] uint8 / uint16 -> the same shape and dtype: gathers through flat indices, blended in int64."""
    p = _check(planes, s, a)
    h, w = p.shape[-2:]
    _, _, Y, X = maps(h, w, s, a)
    y0, x0 = Y // 256, X // 256
    fy, fx = Y - 256 * y0, X - 256 * x0
    y1, x1 = np.minimum(y0 + 1, h - 1), np.minimum(x0 + 1, w - 1)
    flat = p.reshape(p.shape[:-2] + (h * w,)).astype(np.int64)
    tap = lambda yy, xx: np.take(flat, (yy * w + xx).ravel(), axis=-1).reshape(p.shape)
    gx, gy = 256 - fx, 256 - fy
    acc = tap(y0, x0) * (gx * gy) + tap(y0, x1) * (fx * gy) + tap(y1, x0) * (gx * fy) + tap(y1, x1) * (fx * fy) + 32768
    return (acc // 65536).astype(p.dtype)


def affine_file_image(img, s, a):
    """An image as a tile file holds it -- [H, W], or [H, W, 3] RGB mapped per colour plane, ``s`` and ``a`` then being triples
    of pairs and of four-tuples."""
    img = np.asarray(img)
    if img.ndim == 3 and img.shape[2] == 3:
        return np.stack([affine_image(img[:, :, c], tuple(s[c]), tuple(a[c])) for c in range(3)], axis=2)
    return affine_image(img, s, a)


def kernel_form(plane, s, a, vec, mis=0):
    """The device kernel's way (csrc/affine.hip), one vector of ``vec`` dst columns at a time, the first one starting ``mis``
    columns in front of the row -> (the result, the number of vectors that took the fast path, the number that took the slow
    one).  Python integers throughout."""
    p = _check(plane, s, a)
    h, w = p.shape
    U, V = w - 1, h - 1
    out = np.zeros_like(p)
    written = np.zeros(p.shape, np.int64)
    vq, vr = divmod(32 * a[1], DEN)
    uq, ur = divmod(32 * a[3], DEN)
    fast_n = slow_n = 0
    for y in range(h):
        v = 2 * y - V
        for xa in range(-mis, w, vec):
            if xa + vec <= 0:
                continue
            u = 2 * max(xa, 0) - U
            qv, rv = divmod(16 * (a[0] * v + a[1] * u) + 62500, DEN)
            qu, ru = divmod(16 * (a[2] * v + a[3] * u) + 62500, DEN)
            X, Y = [], []
            for j in range(vec):
                if j > 0 and 0 < xa + j <= U:
                    qv, rv = qv + vq, rv + vr
                    if rv >= DEN:
                        qv, rv = qv + 1, rv - DEN
                    qu, ru = qu + uq, ru + ur
                    if ru >= DEN:
                        qu, ru = qu + 1, ru - DEN
                assert 0 <= rv < DEN and 0 <= ru < DEN
                x = min(max(xa + j, 0), U)
                Y.append(min(max(256 * y + s[0] + qv, 0), 256 * V))
                X.append(min(max(256 * x + s[1] + qu, 0), 256 * U))
            xs = min((X[j] >> 8) - j for j in range(vec))
            ys, y_top = min(Yj >> 8 for Yj in Y), max(Yj >> 8 for Yj in Y)
            fast = xs >= 0 and xs + vec - 1 <= U and y_top <= ys + 1 and \
                all((X[j] >> 8) - j - xs <= 1 for j in range(vec))
            lo, hi = max(xa, 0), min(xa + vec, w)
            if fast:
                fast_n += 1
                rows = 3 if y_top != ys else 2
                # the rows clamped to the last one; the span's last two columns from a pair that starts at U - 1 at the latest
                pair_at = min(xs + vec, U - 1) - xs
                assert xs + vec - 1 <= U and 0 <= xs + pair_at and xs + pair_at + 1 <= U
                span = []
                for r in range(rows):
                    row = p[min(ys + r, V)]
                    pair = (int(row[xs + pair_at]), int(row[xs + pair_at + 1]))
                    span.append([int(row[xs + c]) for c in range(vec)] + [pair[1] if pair_at < vec else pair[0], pair[1]])
                for j in range(vec):
                    k, m = (X[j] >> 8) - j - xs, (Y[j] >> 8) - ys
                    fx, fy = X[j] & 255, Y[j] & 255
                    acc = 32768
                    for r in range(rows):
                        wy = (256 - fy) if r == m else fy if r == m + 1 else 0
                        hrow = span[r][j + k] * (256 - fx) + span[r][j + k + 1] * fx
                        assert hrow < 1 << 24
                        acc += hrow * wy
                    assert acc < 1 << 32
                    if lo <= xa + j < hi:
                        out[y, xa + j] = acc >> 16
                        written[y, xa + j] += 1
            else:
                slow_n += 1
                first = divmod(16 * (a[0] * v + a[1] * u) + 62500, DEN) + divmod(16 * (a[2] * v + a[3] * u) + 62500, DEN)
                for j in range(vec):
                    if not lo <= xa + j < hi:
                        continue
                    qv, rv, qu, ru = first      # an element's own walk from the vector's first column, as a lane of the wave does it
                    for _ in range(max(xa, 0), xa + j):
                        qv, rv = qv + vq + (rv + vr >= DEN), (rv + vr) % DEN
                        qu, ru = qu + uq + (ru + ur >= DEN), (ru + ur) % DEN
                    assert Y[j] == min(max(256 * y + s[0] + qv, 0), 256 * V) and X[j] == min(max(256 * (xa + j) + s[1] + qu, 0), 256 * U)
                    x0, y0, fx, fy = X[j] >> 8, Y[j] >> 8, X[j] & 255, Y[j] & 255
                    x1, y1 = min(x0 + 1, U), min(y0 + 1, V)
                    top = int(p[y0, x0]) * (256 - fx) + int(p[y0, x1]) * fx
                    bot = int(p[y1, x0]) * (256 - fx) + int(p[y1, x1]) * fx
                    out[y, xa + j] = (top * (256 - fy) + bot * fy + 32768) >> 16
                    written[y, xa + j] += 1
    assert (written == 1).all()
    return out, fast_n, slow_n
