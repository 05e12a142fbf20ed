"""The definition of tile binning (``--tile-binning``, sq_bin_tiles), in numpy, integers only.

For a plane I of h x w, uint8 or uint16 with maximum M, and an integer factor K in 1..8:

    hb = h // K, wb = w // K          the last h - K hb rows and the last w - K wb columns are dropped
    S(y, x) = sum of I(K y + dy, K x + dx), dy, dx in 0..K - 1            (at most 64 * 65535: it fits 32 bits)
    mean:  out(y, x) = floor(S(y, x) / K^2)     the truncated mean (the rule of --pyramid-method mean)
    sum :  out(y, x) = min(S(y, x), M)          camera binning: counts add, and the result saturates

K = 1 is the identity; hb < 1 or wb < 1 is refused.  RGB files are binned per colour plane (``bin_file_image``)."""
import numpy as np

MAX_FACTOR = 8
METHODS = ('mean', 'sum')


def _check(a, factor, method):
    a = np.asarray(a)
    if a.dtype not in (np.uint8, np.uint16) or a.ndim < 2:
        raise ValueError("uint8 / uint16 planes [..., H, W]")
    if isinstance(factor, bool) or not isinstance(factor, (int, np.integer)) or not 1 <= int(factor) <= MAX_FACTOR:
        raise ValueError("an integer factor in 1..8")
    if method not in METHODS:
        raise ValueError("method 'mean' or 'sum'")
    k = int(factor)
    if a.shape[-2] // k < 1 or a.shape[-1] // k < 1:
        raise ValueError(f"planes of {a.shape[-2]} x {a.shape[-1]} have no {k} x {k} block")
    return a, k


def bin_image(planes, factor, method='mean'):
    """[..., H, W] uint8 / uint16 -> [..., H // K, W // K] of the same dtype: shifted slices added in int64."""
    a, k = _check(planes, factor, method)
    if k == 1:
        return a.copy()
    hb, wb = a.shape[-2] // k, a.shape[-1] // k
    s = np.zeros(a.shape[:-2] + (hb, wb), dtype=np.int64)
    for dy in range(k):
        for dx in range(k):
            s += a[..., dy:dy + k * hb:k, dx:dx + k * wb:k]
    m = int(np.iinfo(a.dtype).max)
    out = s // (k * k) if method == 'mean' else np.minimum(s, m)
    return out.astype(a.dtype)


def loop(plane, factor, method='mean'):
    """The definition word for word, pixel by pixel, in Python integers (one [H, W] plane)."""
    a, k = _check(plane, factor, method)
    hb, wb = a.shape[0] // k, a.shape[1] // k
    m = int(np.iinfo(a.dtype).max)
    out = np.zeros((hb, wb), dtype=a.dtype)
    for y in range(hb):
        for x in range(wb):
            s = sum(int(a[k * y + dy, k * x + dx]) for dy in range(k) for dx in range(k))
            out[y, x] = s // (k * k) if method == 'mean' else min(s, m)
    return out


def bin_file_image(img, factor, method='mean'):
    """An image as a tile file holds it -- [H, W], or [H, W, 3] RGB binned per colour plane."""
    img = np.asarray(img)
    if img.ndim == 3 and img.shape[2] == 3:
        return np.stack([bin_image(img[:, :, c], factor, method) for c in range(3)], axis=2)
    return bin_image(img, factor, method)


def saturated_share(out, dtype=None):
    """The share of the outputs ``out`` of a 'sum' binning that are at the dtype's maximum M (S >= M)."""
    out = np.asarray(out)
    return float((out == int(np.iinfo(dtype or out.dtype).max)).mean())
