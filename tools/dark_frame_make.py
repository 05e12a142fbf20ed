#!/usr/bin/env python3
"""Build a dark frame for ``--dark-frame`` from a folder of dark exposures (shutter closed, the acquisition's exposure time):

    python tools/dark_frame_make.py -i DARK_FOLDER -o frame.npy [--channel NAME]

Every .tif / .tiff under DARK_FOLDER (with --channel: those whose file name carries that channel, as Squid writes it) must be a
2-D image of one shape and dtype, uint8 or uint16.  Per pixel the frame is the rounded integer mean (sum + n // 2) // n, in numpy
on the host; it is written as .npy (or .tif / .tiff, by the output's extension) in the files' dtype.  Prints the frame's
statistics and a ready ``--dark-frame`` line."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def dark_files(folder, channel=None):
    token = None if channel is None else channel.replace(' ', '_')
    found = []
    for where, _, names in os.walk(folder):
        for name in names:
            if name.lower().endswith(('.tif', '.tiff')) and (token is None or token in name):
                found.append(os.path.join(where, name))
    return sorted(found)


def mean_frame(paths):
    """The rounded integer mean of the images at ``paths``: (sum + n // 2) // n per pixel, in the files' dtype."""
    from image_stitcher_amd import tiffio
    total = first = None
    for path in paths:
        img = tiffio.read_image(path)
        if img.ndim == 3 and img.shape[0] == 1:
            img = img[0]
        if img.ndim != 2 or img.dtype not in (np.uint8, np.uint16):
            raise ValueError(f"{path}: a dark exposure is a 2-D uint8 / uint16 image, got {img.dtype} of shape {img.shape}")
        if first is None:
            first, total = img, np.zeros(img.shape, np.int64)
        elif img.shape != first.shape or img.dtype != first.dtype:
            raise ValueError(f"{path}: {img.dtype} of shape {img.shape}, the first file is {first.dtype} of shape {first.shape}")
        total += img
    if first is None:
        raise ValueError("no dark exposure found")
    n = len(paths)
    return ((total + n // 2) // n).astype(first.dtype)


def main(argv=None):
    parser = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    parser.add_argument('-i', '--input-folder', required=True, help="folder of dark exposures")
    parser.add_argument('-o', '--output', required=True, help="the frame: .npy, .tif or .tiff")
    parser.add_argument('--channel', default=None, help="only the files of this channel; the printed line then names it")
    args = parser.parse_args(argv)
    if not args.output.lower().endswith(('.npy', '.tif', '.tiff')):
        raise SystemExit("the output is a .npy, .tif or .tiff")
    paths = dark_files(args.input_folder, args.channel)
    frame = mean_frame(paths)
    if args.output.lower().endswith('.npy'):
        np.save(args.output, frame)
    else:
        from image_stitcher_amd import tiffio
        tiffio.write_tiff(args.output, frame)
    print(f"{len(paths)} exposures of {frame.shape[0]} x {frame.shape[1]} {frame.dtype}: min {int(frame.min())}, max "
          f"{int(frame.max())}, mean {int(frame.sum(dtype=np.int64)) // frame.size}")
    print(f'--dark-frame "{args.channel or "*"}" {args.output}')
    return frame


if __name__ == '__main__':
    main()
