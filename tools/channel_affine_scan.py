"""Measure the arguments of --channel-shift and --channel-affine together on an MI355X: for up to N fields of view of one region,
cut the tile into a 3 x 3 grid of windows, register every channel's window against the reference channel's window of the same
(fov, z) (registration.register_pairs, upsample_factor 10: steps of 0.1 px), fit shift + linear term per field by least squares to
the nine window shifts at the window centres -- twice: the second time on the tile mapped by the first fit, which takes the shear
out of the windows -- and print, per channel, the median over the fields as a ready pair of arguments --
and how many fields agree with that median.

    python tools/channel_affine_scan.py -i /path/to/acquisition --reference "Fluorescence 488 nm Ex" [--z 0] [--fovs 16]

What is measured is where the channel shows the reference's content: a point of the reference at centre + p lies at centre +
(1 + M) p + T in the channel.  The option samples the channel's tile at centre + (1 + A 1e-6) p + S, which has to be that place,
so A 1e-6 = M and S = T: the fit is printed as it is, T rounded to 1/256 px and M to parts per million.

Phase correlation needs structure both channels show: beads, brightfield or autofluorescent tissue can be measured this way,
two channels that stain different things cannot -- their "shift" is noise, and few fields agree with the median.  A window is a
ninth of the tile: a tile below about 200 px a side leaves too little in it."""
import argparse
import statistics
import sys

import numpy as np

sys.path.insert(0, '.')
from image_stitcher_amd import channelaffine, native, registration
from image_stitcher_amd.stitcher import Stitcher
from image_stitcher_amd.stitcher_parameters import StitchingParameters
from image_stitcher_amd.tiffio import read_image

STEP = 0.1      # the measurement's resolution at upsample_factor 10
GRID = 3
MAX_PPM, MAX_SHIFT_PX = 50000, 64


def _planes(st, record):
    """{output channel name: [h, w] plane} of one tile file."""
    img = read_image(record['filepath'])
    if img.ndim == 3 and img.shape[0] == 1:
        img = img[0]
    names = st._colour_planes(record['channel'])
    return {names[0]: img} if len(names) == 1 else {name: np.ascontiguousarray(img[:, :, i]) for i, name in enumerate(names)}


def window_side(n):
    """The largest side up to a third of ``n`` that the device registration takes."""
    side = n // GRID
    while side >= 2 and not registration.crop_length_supported(side):
        side -= 1
    if side < 16:
        raise ValueError(f"a tile side of {n} leaves no window the device registration takes")
    return side


def windows(h, w):
    """(window height, window width, [(y0, x0)] of the 3 x 3 windows, row by row): the outer ones touch the tile's edges."""
    wh, ww = window_side(h), window_side(w)
    ys = [i * (h - wh) // (GRID - 1) for i in range(GRID)]
    xs = [j * (w - ww) // (GRID - 1) for j in range(GRID)]
    return wh, ww, [(y0, x0) for y0 in ys for x0 in xs]


def scan(input_folder, reference, z=0, fovs=16, region=None, timepoint=None, device=None):
    """({channel: [per field an array [9, 4] of (py, px, ty, tx)]}, (h, w)): per window the centre, relative to the tile centre,
    of the channel's content that was compared, and its measured displacement in pixels -- the channel at centre + (py, px)
    shows the reference's content from centre + (py - ty, px - tx)."""
    import torch
    st = Stitcher(StitchingParameters(input_folder=input_folder), device=device)
    st.get_timepoints()
    st.extract_acquisition_parameters()
    st.get_pixel_size()
    st.parse_acquisition_metadata()
    if reference not in st.monochrome_channels:
        raise ValueError(f"--reference {reference!r} is not a channel of this acquisition: {st.monochrome_channels}")
    t = int(st.timepoints[0] if timepoint is None else timepoint)
    r = st.regions[0] if region is None else region
    by_fov = {}
    for (_, _, fov, z_level, _), record in st.get_region_data(t, r).items():
        if z_level == z and 'filepath_right' not in record:
            by_fov.setdefault(fov, []).append(record)
    h, w = st.file_height, st.file_width
    wh, ww, origins = windows(h, w)
    centres = np.array([(y0 + (wh - 1) / 2 - (h - 1) / 2, x0 + (ww - 1) / 2 - (w - 1) / 2) for y0, x0 in origins])
    found = {}
    for fov in sorted(by_fov)[:max(1, int(fovs))]:
        planes = {}
        for record in by_fov[fov]:
            planes.update(_planes(st, record))
        if reference not in planes:
            continue
        others = [name for name in st.monochrome_channels if name in planes and name != reference]
        tiles = torch.from_numpy(np.stack([planes[reference]] + [planes[name] for name in others])).to(st.device)
        pairs = np.zeros(len(others) * len(origins), dtype=native.PAIR_DTYPE)
        for k in range(len(others)):
            for i, (y0, x0) in enumerate(origins):
                pairs[k * len(origins) + i] = (0, k + 1, y0, x0, y0, x0)
        shifts, _, _ = registration.register_pairs(tiles, pairs, wh, ww, upsample_factor=10)
        # (the shift that registers the moving window with the reference's, skimage's sign: moving(p) = reference(p + s); the
        # reference's content at p is then at p - s in the channel)
        shifts = np.asarray(shifts, dtype=np.float64).reshape(len(others), len(origins), 2)
        first = [np.concatenate([centres, -s], axis=1) for s in shifts]
        # Second pass.  Under rotation or scale the content of a window is displaced by different amounts at its two ends (half
        # a pixel and more over a ninth of a tile), which flattens the correlation peak and biases it.  So every channel's tile is
        # mapped on the host by its first fit (the option's own definition), and the windows are registered again: what is left
        # is nearly a pure translation per window, measured to the registration's resolution.  A window of the mapped tile at q
        # shows the channel's content from q + t1(q), t1 the first fit's displacement there: with the second shift s2 the
        # channel's window at q + t1(q) is displaced by t1(q) - s2.
        maps = [integer_map(fit(m)) for m in first]
        mapped = [channelaffine.affine_image(planes[name], s1, a1) for name, (s1, a1) in zip(others, maps)]
        tiles = torch.from_numpy(np.stack([planes[reference]] + mapped)).to(st.device)
        shifts, _, _ = registration.register_pairs(tiles, pairs, wh, ww, upsample_factor=10)
        shifts = np.asarray(shifts, dtype=np.float64).reshape(len(others), len(origins), 2)
        for name, (s1, a1), s2 in zip(others, maps, shifts):
            t1 = np.array(s1) / 256 + centres @ (np.array(a1, dtype=np.float64).reshape(2, 2) * 1e-6).T
            found.setdefault(name, []).append(np.concatenate([centres + t1, t1 - s2], axis=1))
    return found, (h, w)


def integer_map(params):
    """A fit -> (S in 1/256 px, A in parts per million), Python ints, clipped to the options' ranges."""
    clip = lambda v, top: int(min(max(int(round(float(v))), -top), top))
    return (tuple(clip(256 * v, 256 * MAX_SHIFT_PX) for v in params[:2]), tuple(clip(1e6 * v, MAX_PPM) for v in params[2:]))


def fit(measured):
    """[9, 4] of (py, px, ty, tx) -> (Ty, Tx, Myy, Myx, Mxy, Mxx): t = T + M p by least squares, per axis.  A window at q in the
    channel that is displaced by t shows the reference's content from p = q - t: that p is the abscissa."""
    design = np.concatenate([np.ones((len(measured), 1)), measured[:, :2] - measured[:, 2:4]], axis=1)
    (ty, myy, myx), (tx, mxy, mxx) = (np.linalg.lstsq(design, measured[:, 2 + axis], rcond=None)[0] for axis in (0, 1))
    return np.array([ty, tx, myy, myx, mxy, mxx])


def corner_displacements(params, h, w):
    """[4, 2]: the fitted displacement at the tile's four corners, pixels."""
    ty, tx, myy, myx, mxy, mxx = params
    return np.array([(ty + myy * py + myx * px, tx + mxy * py + mxx * px)
                     for py in (-(h - 1) / 2, (h - 1) / 2) for px in (-(w - 1) / 2, (w - 1) / 2)])


def summarise(found, shape):
    """[{name, shift_px (DY, DX), affine_ppm (AYY, AYX, AXY, AXX), params (the median fit), agree, fields, windows}]: the median
    over the fields of every fitted parameter; a field agrees when its fit is within 2 steps of the median's at all four corners."""
    h, w = shape
    rows = []
    for name, fields in found.items():
        fits = np.array([fit(m) for m in fields])
        median = np.array([statistics.median_low(fits[:, i].tolist()) for i in range(6)])
        corners = corner_displacements(median, h, w)
        agree = sum(bool((np.abs(corner_displacements(f, h, w) - corners) <= 2 * STEP + 1e-9).all()) for f in fits)
        rows.append(dict(name=name, shift_px=(float(median[0]), float(median[1])),
                         affine_ppm=tuple(int(round(float(v) * 1e6)) for v in median[2:]), params=median, agree=agree,
                         fields=len(fields), windows=fields))
    return rows


def argument_line(row):
    dy, dx = row['shift_px']
    return (f"--channel-shift \"{row['name']}\" {dy:.3f} {dx:.3f} --channel-affine \"{row['name']}\" "
            + " ".join(str(c) for c in row['affine_ppm']))


def main(argv=None):
    parser = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    parser.add_argument('-i', '--input-folder', required=True)
    parser.add_argument('--reference', required=True, metavar='NAME', help="the output channel the others are moved onto")
    parser.add_argument('--z', type=int, default=0)
    parser.add_argument('--fovs', type=int, default=16, metavar='N')
    parser.add_argument('--region', default=None)
    parser.add_argument('--timepoint', type=int, default=None)
    args = parser.parse_args(argv)
    found, shape = scan(args.input_folder, args.reference, args.z, args.fovs, args.region, args.timepoint)
    rows = summarise(found, shape)
    wh, ww, _ = windows(*shape)
    print(f"shift and linear term against {args.reference!r} at z {args.z}, {GRID} x {GRID} windows of {wh} x {ww}, steps of {STEP} px; "
          f"only channels that show the same structure as the reference (beads, brightfield) can be measured this way: trust a "
          f"line whose fields agree")
    for row in rows:
        out_of_range = any(abs(c) > MAX_PPM for c in row['affine_ppm']) or any(abs(v) > MAX_SHIFT_PX for v in row['shift_px'])
        print(f"{argument_line(row)}      # {row['agree']} of {row['fields']} fields within {2 * STEP} px of the median at the "
              f"tile's corners" + (" -- OUTSIDE the options' ranges: not a small misalignment" if out_of_range else ""))
    return rows


if __name__ == '__main__':
    main()
