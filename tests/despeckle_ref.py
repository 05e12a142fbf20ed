"""The definition of the hot-pixel removal (``--despeckle``, sq_despeckle_tiles), in numpy.

    m(y, x) = the median (5th smallest) of the nine values I(clamp(y+dy, 0, H-1), clamp(x+dx, 0, W-1)), dy, dx in {-1, 0, 1}
    hot :  out(y, x) = m(y, x) if I(y, x) - m(y, x) >  T   else I(y, x)
    both:  out(y, x) = m(y, x) if |I(y, x) - m(y, x)| > T  else I(y, x)

The differences are taken in int64.  Every m comes from the unfiltered plane (the filter is not recursive), and the replicated
edge makes the window nine values at every pixel, also for H = 1 or W = 1.  ``both`` with T = 0 is
``scipy.ndimage.median_filter(size=3, mode='nearest')``.  The median is a pad with ``mode='edge'``, the nine shifted views
stacked and ``np.sort(...)[4]`` (``loop`` does the same pixel by pixel, word for word, for small cases)."""
import numpy as np

MODES = ('hot', 'both')


def median9(img):
    """[..., H, W] -> the median of the edge-replicated 3 x 3 window of every pixel, every plane on its own."""
    img = np.asarray(img)
    if img.ndim < 2:
        raise ValueError("planes [..., H, W]")
    h, w = img.shape[-2:]
    p = np.pad(img, [(0, 0)] * (img.ndim - 2) + [(1, 1), (1, 1)], mode='edge')
    views = np.stack([p[..., dy:dy + h, dx:dx + w] for dy in range(3) for dx in range(3)])
    return np.sort(views, axis=0)[4]


def despeckle(img, threshold, mode):
    """[..., H, W] uint8 / uint16 -> (out of the same shape and dtype, fired: the boolean mask of the pixels replaced)."""
    img = np.asarray(img)
    if img.dtype not in (np.uint8, np.uint16) or img.ndim < 2 or mode not in MODES or not 0 <= int(threshold) <= 65535:
        raise ValueError("uint8 / uint16 planes [..., H, W], mode 'hot' or 'both', threshold 0..65535")
    m = median9(img)
    d = img.astype(np.int64) - m.astype(np.int64)
    fired = (d if mode == 'hot' else np.abs(d)) > int(threshold)
    return np.where(fired, m, img).astype(img.dtype), fired


def despeckle_image(img, threshold, mode):
    """What a tile FILE holds: a 2-D plane, or H x W x 3 whose colours are filtered independently.  -> the filtered image."""
    img = np.asarray(img)
    if img.ndim == 3:
        return np.stack([despeckle(img[:, :, k], threshold, mode)[0] for k in range(img.shape[2])], axis=2)
    return despeckle(img, threshold, mode)[0]


def loop(img, threshold, mode):
    """The definition word for word on one plane, pixel by pixel -> (out, fired)."""
    h, w = img.shape
    out = img.copy()
    fired = np.zeros((h, w), dtype=bool)
    for y in range(h):
        for x in range(w):
            nine = sorted(int(img[min(max(y + dy, 0), h - 1), min(max(x + dx, 0), w - 1)]) for dy in (-1, 0, 1) for dx in (-1, 0, 1))
            m = nine[4]
            d = int(img[y, x]) - m
            if (d if mode == 'hot' else abs(d)) > threshold:
                out[y, x] = m
                fired[y, x] = True
    return out, fired
