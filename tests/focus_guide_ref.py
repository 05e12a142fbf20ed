"""Numpy definition of the best-focus projection with a guide channel (sq_fuse_select_depth), on top of
focus_ref.py: the guide channel g is projected as always; every other channel takes, per voxel, its fused value in the plane
whose z level is the guide's depth -- 0 where the guide is uncovered, and 0 where the channel has no plane at that level or
that plane does not cover the voxel."""
import numpy as np

from focus_ref import depth_of, focus_reference
from oracle import stitch_oracle as O


def fused_stack(groups, canvas_h, canvas_w, num_z):
    """groups as in focus_ref.focus_reference (the planes of ONE channel, possibly under several plans) -> the channel's fused
    stack [num_z, Hc, Wc]; levels without a plane are zeros."""
    dt = np.asarray(groups[0][0]).dtype
    stack = np.zeros((num_z, canvas_h, canvas_w), dtype=dt)
    for tiles, rects, flats, z_levels in groups:
        for zi, z in enumerate(z_levels):
            ts = list(tiles[zi])
            if ts:
                stack[z] = O.fuse_plane_overwrite(ts, rects, canvas_h, canvas_w, None if flats is None else flats[zi])
    return stack


def select_by_depth(stack, depth):
    """np.take_along_axis of a fused stack [Z, Hc, Wc] along z by ``depth`` [Hc, Wc] (-1 = uncovered -> 0)."""
    depth = np.asarray(depth)
    out = np.take_along_axis(stack, depth.clip(0)[None].astype(np.int64), 0)[0]
    return np.where(depth < 0, 0, out).astype(stack.dtype)


def unsigned_depth(depth, num_z):
    """The depth plane handed between the stages and written to disk: z* + 1, 0 = uncovered; uint8 up to 255 levels."""
    return (np.asarray(depth) + 1).astype(np.uint8 if num_z <= 255 else np.uint16)


def focus_guide_reference(channels, guide, canvas_h, canvas_w, radius, num_z):
    """channels: per channel the ``groups`` of focus_ref.focus_reference.  -> (outputs [C, Hc, Wc], depth [Hc, Wc] int64 of the
    guide, -1 = uncovered)."""
    g_out, g_key = focus_reference(channels[guide], canvas_h, canvas_w, radius)
    depth = depth_of(g_key)
    outs = []
    for c, groups in enumerate(channels):
        outs.append(g_out if c == guide else select_by_depth(fused_stack(groups, canvas_h, canvas_w, num_z), depth))
    return np.stack(outs), depth
