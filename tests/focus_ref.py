"""Numpy definition of the best-focus (extended depth of field) projection (sq_fuse_project_focus).

Per staged tile k of plane (c, z): I = the raw tile, reads outside it clamped to its edge;
ML(y,x) = |2I(y,x) - I(y,x-1) - I(y,x+1)| + |2I(y,x) - I(y-1,x) - I(y+1,x)|;
F(y,x) = sum over |dy|, |dx| <= R of ML(clamp(y+dy), clamp(x+dx)); key = (F << 32) | (0xFFFFFFFF - z).
The key tiles are placed like the planes (oracle.stitch_oracle.fuse_plane_overwrite, no gains), the winning plane of a
voxel is the one with the largest key (0 = not covered), and the output is that plane's fused value there."""
import numpy as np

from oracle import stitch_oracle as O


def modified_laplacian(tile):
    i = np.asarray(tile).astype(np.int64)
    p = np.pad(i, 1, mode='edge')
    return np.abs(2 * i - p[1:-1, :-2] - p[1:-1, 2:]) + np.abs(2 * i - p[:-2, 1:-1] - p[2:, 1:-1])


def focus_score(tile, radius):
    """F of one full tile (int64 [H, W])."""
    ml = np.pad(modified_laplacian(tile), radius, mode='edge')   # clamp(y + dy), clamp(x + dx), any radius
    n = 2 * radius + 1
    c = np.zeros((ml.shape[0] + 1, ml.shape[1] + 1), dtype=np.int64)
    c[1:, 1:] = ml.cumsum(0).cumsum(1)
    return c[n:, n:] - c[:-n, n:] - c[n:, :-n] + c[:-n, :-n]


def key_tile(tile, z, radius):
    return (focus_score(tile, radius).astype(np.uint64) << np.uint64(32)) | np.uint64(0xFFFFFFFF - int(z))


def focus_reference(groups, canvas_h, canvas_w, radius):
    """groups: [(tiles [Z, N, H, W], rects [N, 6], flats (Z entries, gain image or None) or None, z_levels (Z))] -- the
    planes of one channel, possibly under several plans.  -> (output [Hc, Wc] of the tile dtype, key [Hc, Wc] uint64)."""
    keys, fused = [], []
    for tiles, rects, flats, z_levels in groups:
        for zi, z in enumerate(z_levels):
            ts = list(tiles[zi])
            keys.append(O.fuse_plane_overwrite([key_tile(t, z, radius) for t in ts] or [np.zeros((1, 1), np.uint64)],
                                               np.asarray(rects).reshape(-1, 6), canvas_h, canvas_w))
            ff = None if flats is None else flats[zi]
            dt = np.asarray(tiles).dtype
            fused.append(O.fuse_plane_overwrite(ts, rects, canvas_h, canvas_w, ff) if ts
                         else np.zeros((canvas_h, canvas_w), dtype=dt))
    keys, fused = np.stack(keys), np.stack(fused)
    win = keys.argmax(0)
    out = np.take_along_axis(fused, win[None], 0)[0]
    key = np.take_along_axis(keys, win[None], 0)[0]
    return out, key


def depth_of(key):
    """z* of each voxel, -1 where no plane covers it."""
    key = np.asarray(key, dtype=np.uint64)
    return np.where(key == 0, -1, 0xFFFFFFFF - (key & np.uint64(0xFFFFFFFF)).astype(np.int64))


def focus_reference_region(acq, t, region, read_image, radius, flatfields=None, apply_flat=False, use_registration=False,
                           shifts=None):
    """The best-focus projection of one (t, region) of an acquisition as the oracle stitches it -> (output (1, C, 1, Hc, Wc),
    key (C, Hc, Wc) uint64): key tiles from the raw files (the monochrome component of an RGB file) placed like the tiles
    (oracle.stitch_oracle.place_tile), the output taken from the oracle's fused stack at the winning plane."""
    stack = O.stitch_region(acq, t, region, read_image, use_registration, shifts, flatfields, apply_flat)
    shifts = shifts or {}
    plan = O.plan_region(acq, t, region, use_registration, shifts.get('h_shift', (0, 0)), shifts.get('v_shift', (0, 0)),
                         shifts.get('h_shift_rev'), shifts.get('h_shift_rev_odd', 0), 1)
    keys = np.zeros(stack.shape, dtype=np.uint64)
    for f in plan.files:
        tile = read_image(f['filepath'])
        if f['rgb'] >= 0:
            tile = tile[:, :, f['rgb']]
        O.place_tile(keys, f['c'], f['z'], key_tile(tile, f['z'], radius), f['x_px'], f['y_px'], f['top'], f['bottom'],
                     f['left'], f['right'])
    win = keys[0].argmax(1)[:, None]                                   # (C, 1, Hc, Wc)
    out = np.take_along_axis(stack[0], win, 1)[None]
    return out, np.take_along_axis(keys[0], win, 1)[:, 0]
