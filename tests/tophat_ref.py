"""The definition of the white top-hat background removal (``--background-subtract tophat``, sq_tophat_tiles), in numpy.

    E(y, x) = min I over the (2R+1) x (2R+1) window centred on (y, x), clipped to the plane
    O(y, x) = max E over the same clipped window
    out     = I - O

Clipping the window is padding with the dtype's maximum for the minimum and with 0 for the maximum.  The window is a square,
so its extremum is the extremum over the rows of the extrema along the rows: each axis is padded, cut into its 2R+1 shifted
views and reduced (``brute`` does the same with the (2R+1)^2 shifted views of the padded plane, for small cases)."""
import numpy as np


def _window_1d(a, radius, axis, fn, fill):
    pad = [(0, 0)] * a.ndim
    pad[axis] = (radius, radius)
    p = np.pad(a, pad, constant_values=fill)
    views = np.lib.stride_tricks.sliding_window_view(p, 2 * radius + 1, axis=axis)
    return fn(views, axis=-1)


def erode(img, radius):
    top = np.iinfo(img.dtype).max
    return _window_1d(_window_1d(img, radius, -1, np.min, top), radius, -2, np.min, top)


def dilate(img, radius):
    return _window_1d(_window_1d(img, radius, -1, np.max, 0), radius, -2, np.max, 0)


def opening(img, radius):
    return dilate(erode(img, radius), radius)


def tophat(img, radius):
    """[..., H, W] uint8 / uint16 -> the same shape and dtype; every plane on its own."""
    img = np.asarray(img)
    if img.dtype not in (np.uint8, np.uint16) or img.ndim < 2 or radius < 1:
        raise ValueError("uint8 / uint16 planes [..., H, W], radius >= 1")
    o = opening(img, int(radius))
    assert (o <= img).all()
    return img - o


def tophat_image(img, radius):
    """What a tile FILE holds: a 2-D plane, or H x W x 3 whose colours are filtered independently."""
    img = np.asarray(img)
    if img.ndim == 3:
        return np.stack([tophat(img[:, :, k], radius) for k in range(img.shape[2])], axis=2)
    return tophat(img, radius)


def brute(img, radius):
    """The 2-D definition word for word on one plane: (2R+1)^2 shifted views of the padded plane."""
    def win(a, fn, fill):
        h, w = a.shape
        p = np.pad(a, radius, constant_values=fill)
        return fn(np.stack([p[dy:dy + h, dx:dx + w] for dy in range(2 * radius + 1) for dx in range(2 * radius + 1)]), axis=0)
    e = win(img, np.min, np.iinfo(img.dtype).max)
    return img - win(e, np.max, 0)


def sample_planes(dtype, h, w, seed=3):
    """[3, 2, H, W]: two synthetic tiles (scene + noise) and four adversarial planes."""
    from image_stitcher_amd import synth
    dt = np.dtype(dtype)
    top = int(np.iinfo(dt).max)
    out = np.zeros((6, h, w), dtype=dt)
    for i in range(2):
        v = synth.scene_patch(seed + i, 17 * i, 5, h, w) + synth.noise_patch(seed + 7 + i, h, w, 300)
        out[i] = (v >> 8).astype(dt) if dt == np.uint8 else np.clip(v, 0, top).astype(dt)
    spots = [(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1), (h // 2, w // 2)]
    out[2] = top                                  # the maximum everywhere but single zero pixels
    for y, x in spots:
        out[2][y, x] = 0
    for y, x in spots:                            # and the reverse
        out[3][y, x] = top
    ramp = (np.arange(h)[:, None] * 3 + np.arange(w)[None, :] * 2) % (top // 2)
    out[4] = ramp.astype(dt)                      # a ramp with one bright 3 x 3 spot
    out[4][max(0, h // 3 - 1):h // 3 + 2, max(0, w // 3 - 1):w // 3 + 2] = top
    return out.reshape(3, 2, h, w)                # (out[5]: all zeros)



