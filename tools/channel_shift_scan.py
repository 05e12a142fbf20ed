"""Measure the arguments of --channel-shift on an MI355X: for up to N fields of view of one region, register every channel's tile
against the reference channel's tile of the same (fov, z) over the full tile (native.register_pairs, upsample_factor 10: steps
of 0.1 px) and print, per channel, the median shift in the option's sign and units -- a ready --channel-shift line -- and how
many fields agree with that median within one step.

    python tools/channel_shift_scan.py -i /path/to/acquisition --reference "Fluorescence 488 nm Ex" [--z 0] [--fovs 16]

Phase correlation needs structure both channels show: beads, brightfield or autofluorescent tissue can be measured this way,
two channels that stain different things cannot -- their "shift" is noise, and few fields agree with the median."""
import argparse
import statistics
import sys

import numpy as np

sys.path.insert(0, '.')
from image_stitcher_amd import native, registration
from image_stitcher_amd.stitcher import Stitcher
from image_stitcher_amd.stitcher_parameters import StitchingParameters
from image_stitcher_amd.tiffio import read_image

STEP = 0.1      # the measurement's resolution at upsample_factor 10


def _planes(st, record):
    """{output channel name: [h, w] plane} of one tile file."""
    img = read_image(record['filepath'])
    if img.ndim == 3 and img.shape[0] == 1:
        img = img[0]
    names = st._colour_planes(record['channel'])
    return {names[0]: img} if len(names) == 1 else {name: np.ascontiguousarray(img[:, :, i]) for i, name in enumerate(names)}


def scan(input_folder, reference, z=0, fovs=16, region=None, timepoint=None, device=None):
    """{channel: [(DY, DX) per field]} in pixels, in the option's sign: the channel's tile sampled at (y + DY, x + DX) lies on
    the reference's."""
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
    if not (registration.crop_length_supported(h) and registration.crop_length_supported(w)):
        raise ValueError(f"the device registration does not take crops of {h} x {w}")
    found = {}
    for fov in sorted(by_fov)[:max(1, int(fovs))]:
        planes = {}
        for record in by_fov[fov]:
            planes.update(_planes(st, record))
        if reference not in planes:
            continue
        others = [name for name in st.monochrome_channels if name in planes and name != reference]
        tiles = torch.from_numpy(np.stack([planes[reference]] + [planes[name] for name in others])).to(st.device)
        pairs = np.zeros(len(others), dtype=native.PAIR_DTYPE)
        pairs['mov_tile'] = np.arange(1, len(others) + 1)
        shifts, _, _ = registration.register_pairs(tiles, pairs, h, w, upsample_factor=10)
        # (the shift that registers the moving tile with the reference, skimage's sign: moving(p) = reference(p + s); a point
        # of the reference at p is then at p - s in the channel, which is the option's (DY, DX))
        for name, s in zip(others, shifts):
            found.setdefault(name, []).append((-float(s[0]), -float(s[1])))
    return found


def summarise(found):
    """[(channel, median DY, median DX, fields within one step of it, fields)]"""
    rows = []
    for name, values in found.items():
        dy, dx = (statistics.median_low(v[i] for v in values) for i in (0, 1))
        agree = sum(abs(v[0] - dy) <= STEP + 1e-9 and abs(v[1] - dx) <= STEP + 1e-9 for v in values)
        rows.append((name, dy, dx, agree, len(values)))
    return rows


def main(argv=None):
    parser = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    parser.add_argument('-i', '--input-folder', required=True)
    parser.add_argument('--reference', required=True, metavar='NAME', help="the output channel the others are moved onto")
    parser.add_argument('--z', type=int, default=0)
    parser.add_argument('--fovs', type=int, default=16, metavar='N')
    parser.add_argument('--region', default=None)
    parser.add_argument('--timepoint', type=int, default=None)
    args = parser.parse_args(argv)
    rows = summarise(scan(args.input_folder, args.reference, args.z, args.fovs, args.region, args.timepoint))
    print(f"shifts against {args.reference!r} at z {args.z}, full tiles, steps of {STEP} px; only channels that show the same "
          f"structure as the reference (beads, brightfield) can be measured this way: trust a line whose fields agree")
    for name, dy, dx, agree, n in rows:
        print(f"--channel-shift \"{name}\" {dy:.1f} {dx:.1f}      # {agree} of {n} fields within {STEP} px of the median")
    return rows


if __name__ == '__main__':
    main()
