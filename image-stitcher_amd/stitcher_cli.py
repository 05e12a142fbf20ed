#!/usr/bin/env python3
"""Command line of the stitcher: the reference's flags (stitcher_cli.py:14-62) unchanged,
plus eighteen switches for what this build adds (``--fusion-mode``, ``--normalization``,
``--zarr-compression``, ``--per-region-registration``, ``--flatfield-estimator``, ``--all-pairs-registration``,
``--global-registration``, ``--z-projection``, ``--focus-radius``, ``--pyramid-method``, ``--contrast-limits``,
``--contrast-percentiles``, ``--focus-guide-channel``, ``--focus-depth-map``, ``--composite``, ``--composite-max-side``,
``--composite-z``, ``--composite-channels``).  Two more select the background removal of the staged tiles:
``--background-subtract`` and ``--background-radius``.  ``--despeckle`` and ``--despeckle-threshold`` select the hot-pixel
removal that runs on the staged tiles before it.  ``--tile-qc``, ``--tile-qc-saturation`` and ``--tile-qc-focus-ratio`` select
the per-tile quality report (focus, saturation, intensity) of the tiles as they are in their files.  ``--dpc``,
``--dpc-channels`` and ``--dpc-gain`` add the differential phase contrast channel made of the two half-pupil brightfield tiles.
``--seam-qc``, ``--seam-qc-radius``, ``--seam-qc-min-pixels`` and ``--seam-qc-min-ncc`` select the per-seam alignment report: how
well every pair of overlapping tiles agrees where it is placed, on every (channel, z) plane, and the integer residual displacement
at which it would agree best.  ``--tile-binning`` and ``--tile-binning-method`` stitch K x K binned tiles, binned on the device
before anything else sees them.  ``--distortion-correction`` removes radial lens distortion from every tile, on the device, in
front of all of that.  ``--channel-shift NAME DY DX`` (repeatable) moves every tile of one channel by a constant sub-pixel
translation, on the device, between the two, so that channels that are not registered to each other on the sensor line up;
``--channel-affine NAME AYY AYX AXY AXX`` (repeatable) adds the linear term -- rotation, scale, shear about the tile centre -- to it.
``--dark-frame`` (NAME SOURCE, repeatable) and ``--dark-pedestal`` subtract the camera's additive term -- a dark frame or a constant
-- from every tile of a channel, on the device, in front of all of them.

    python -m image_stitcher_amd.stitcher_cli -i /path/to/acquisition -r -ff --registration-channel "488"
"""
import argparse
import sys

from . import channelaffine, channelshift, darkframe
from .stitcher import Stitcher
from .stitcher_parameters import StitchingParameters


def _ppm(text):
    """--distortion-correction: an integer in -50000..50000 (no float, no exponent)."""
    try:
        value = int(text)
    except ValueError:
        raise argparse.ArgumentTypeError(f"an integer in -50000..50000 (parts per million), got {text!r}")
    if not -50000 <= value <= 50000:
        raise argparse.ArgumentTypeError(f"an integer in -50000..50000 (parts per million), got {text!r}")
    return value


FLAGS = (
    # (names, kwargs) -- names and semantics as in the reference's argparse set-up (stitcher_cli.py:14-62)
    (('--input-folder', '-i'), dict(required=True, help="acquisition folder (timepoint sub-folders with tiles and coordinates.csv)")),
    (('--output-format', '-f'), dict(choices=['.ome.zarr', '.ome.tiff'], default='.ome.zarr', help="container of the stitched output")),
    (('--apply-flatfield', '-ff'), dict(action='store_true', help="divide every tile by its channel's flatfield")),
    (('--use-registration', '-r'), dict(action='store_true', help="register the centre tile pairs and place tiles by the measured shifts")),
    (('--registration-channel',), dict(help="channel the shifts are measured on (first channel when omitted)")),
    (('--registration-z-level',), dict(type=int, default=0, help="z plane the shifts are measured on")),
    (('--dynamic-registration',), dict(action='store_true', help="accepted, stored and ignored, exactly like the reference (stitcher.py:92); see --all-pairs-registration")),
    (('--scan-pattern', '-s'), dict(choices=['Unidirectional', 'S-Pattern'], default='Unidirectional', help="stage scan order")),
    (('--merge-timepoints', '-mt'), dict(action='store_true', help="request one dataset over all timepoints")),
    (('--merge-hcs-regions', '-mw'), dict(action='store_true', help="request one plate dataset over all wells")),
    (('--params-json',), dict(help="JSON file of StitchingParameters; replaces the flags above")),
    # additions of this build
    (('--fusion-mode',), dict(choices=['overwrite', 'feather'], default='overwrite',
                              help="overwrite = the reference's last-writer-wins; feather = distance-weighted blend (extension)")),
    (('--normalization',), dict(choices=['phase', 'none'], default='phase',
                                help="cross-power normalisation: phase = scikit-image >= 0.19 default, none = 0.18 behaviour")),
    (('--zarr-compression',), dict(choices=['blosc', 'zlib', 'none'], default='blosc',
                                   help="OME-Zarr chunk codec: blosc = the reference's default (Blosc-1 frames, shuffle + LZ4), encoded "
                                        "on the device; zlib = host threads; none = raw chunks")),
    (('--ome-tiff-layout',), dict(choices=['planes', 'pyramid'], default='planes',
                                  help="with -f .ome.tiff: planes = one uncompressed strip per plane, level 0 only; pyramid = tiled "
                                       "planes with the pyramid levels in SubIFDs (OME-TIFF 6), streamed batch by batch")),
    (('--ome-tiff-compression',), dict(choices=['deflate', 'none', 'jpeg'], default='deflate',
                                       help="with --ome-tiff-layout pyramid: deflate = Adobe deflate tiles with the horizontal "
                                            "predictor, encoded on the device; none = raw tiles; jpeg = baseline JPEG tiles (TIFF "
                                            "Compression 7, lossy, uint8 acquisitions only), encoded on the device")),
    (('--ome-tiff-quality',), dict(type=int, default=90, metavar='Q',
                                   help="with --ome-tiff-compression jpeg: libjpeg's quality scale, 1..100 (default 90)")),
    (('--per-region-registration',), dict(action='store_true',
                                          help="with -r: register every (timepoint, region) on its own tiles instead of once")),
    (('--all-pairs-registration',), dict(action='store_true',
                                         help="with -r: register EVERY adjacent tile pair of the registration plane (batched on the device, "
                                              "sharded by pair over the ranks) and place tiles by the per-axis median shift, instead of the "
                                              "reference's centre-tile pairs")),
    (('--global-registration',), dict(action='store_true',
                                      help="with -r: register every adjacent tile pair of every (timepoint, region) and place EACH tile at its "
                                           "own position from a least-squares solve over the pairs whose overlap correlates (tiles "
                                           "without one stay on the all-pairs lattice); writes <region>_tile_positions.csv")),
    (('--flatfield-estimator',), dict(choices=['auto', 'basic', 'basicpy', 'mean'], default='auto',
                                      help="with -ff: basicpy's BaSiC fit when that package is installed (auto / basicpy), this "
                                           "build's device restatement of the published BaSiC fit (basic; what auto falls back "
                                           "to), or a plain smoothed mean (mean: not BaSiC)")),
    (('--z-projection',), dict(choices=['none', 'max', 'max-only', 'focus', 'focus-only'], default='none',
                               help="projection over z per channel, computed on the device from the tiles: max = the stack plus "
                                    "the maximum-intensity projection <region>_stitched_mip<format>; focus = the stack plus the "
                                    "best-focus (extended depth of field) projection <region>_stitched_edf<format>; max-only / "
                                    "focus-only = the projection alone (overwrite fusion only)")),
    (('--focus-radius',), dict(type=int, choices=range(0, 16), default=3, metavar='R',
                               help="with --z-projection focus: radius of the focus window, 0..15 (a (2R+1)^2 box sum of the "
                                    "modified Laplacian)")),
    (('--pyramid-method',), dict(choices=['nearest', 'mean'], default='nearest',
                                 help="how the OME-Zarr levels above 0 are made, in every store of the run (stack, _mip, _edf): "
                                      "nearest = the reference's Scaler.nearest decimation; mean = the truncated 2 x 2 mean of "
                                      "the level before, all levels from one read of level 0 on the device.  .ome.tiff output "
                                      "holds level 0 only, so there the option changes nothing")),
    (('--contrast-limits',), dict(choices=['dtype', 'percentile'], default='dtype',
                                  help="channel windows of the OME-Zarr omero block, in every store of the run (stack, _mip, _edf): "
                                       "dtype = the reference's 0 ... dtype max; percentile = two percentiles of the non-zero "
                                       "voxels of the store's own level 0, from exact histograms kept on the device, plus "
                                       "<stem>_histogram.npy and <stem>_stats.json beside the store (.ome.zarr output only)")),
    (('--contrast-percentiles',), dict(type=float, nargs=2, default=(0.1, 99.9), metavar=('LO', 'HI'),
                                       help="with --contrast-limits percentile: the window's start and end percentile, "
                                            "0 <= LO < HI <= 100")),
    (('--focus-guide-channel',), dict(metavar='NAME', default=None,
                                      help="with --z-projection focus / focus-only: decide the depth on this channel (a name out of "
                                           "the output channels, for an RGB file e.g. <base>_G) and give every other channel its "
                                           "value at that depth, instead of a depth of its own per channel")),
    (('--focus-depth-map',), dict(action='store_true',
                                  help="with --z-projection focus / focus-only: also write <region>_stitched_depth<format>, the "
                                       "winning z level + 1 of every voxel (0 = no tile): one plane with --focus-guide-channel, "
                                       "else one per channel; levels by nearest, windows 0 ... number of z levels")),
    (('--composite',), dict(action='store_true',
                            help="also write one colour quick-look picture per (timepoint, region): <region>_stitched[_mip|_edf]"
                                 "_composite.png and .json -- the projection the run writes, else one z plane of the stack, "
                                 "reduced on the device to block means, windowed by --contrast-percentiles of its own values "
                                 "and added in the channel colours")),
    (('--composite-max-side',), dict(type=int, default=4096, metavar='N',
                                     help="with --composite: the picture's longer side is at most N pixels (16..16384); the block "
                                          "size is the smallest power of two, up to 256, that achieves it")),
    (('--composite-z',), dict(type=int, default=None, metavar='Z',
                              help="with --composite and no projection: the z level shown (default: the middle one)")),
    (('--composite-channels',), dict(nargs='+', default=None, metavar='NAME',
                                     help="with --composite: the channels shown, in this order (names out of the output channels, "
                                          "for an RGB file e.g. <base>_G; default: all)")),
    (('--background-subtract',), dict(choices=['none', 'tophat'], default='none',
                                      help="remove the slowly varying additive background of every tile on the device before it is "
                                           "projected or fused: tophat = the tile minus its morphological opening with a square "
                                           "window of --background-radius, clipped to the tile (meant for fluorescence; registration "
                                           "and the flatfield estimate keep reading raw tiles); writes "
                                           "<region>_stitched_background.json")),
    (('--background-radius',), dict(type=int, default=50, metavar='R',
                                    help="with --background-subtract tophat: radius of the window, 1..127 (larger than the "
                                         "structures to keep, smaller than the background's variation)")),
    (('--despeckle',), dict(choices=['none', 'hot', 'both'], default='none',
                            help="replace single-pixel outliers of every tile on the device before anything else touches it "
                                 "(background removal, flatfield divide, projection, fusion): a pixel that differs from the "
                                 "median of its 3 x 3 window (edges replicated) by more than --despeckle-threshold becomes "
                                 "that median; hot = pixels above the median only (hot pixels, cosmic hits), both = below it "
                                 "too (dead pixels).  Registration and the flatfield estimate keep reading raw tiles; writes "
                                 "<region>_stitched_despeckle.json and prints the number of staged pixels replaced, one line per "
                                 "region (one per call where a region is fused in several row-band calls; a tile staged for "
                                 "two bands counts twice)")),
    (('--despeckle-threshold',), dict(type=int, default=1000, metavar='T',
                                      help="with --despeckle hot / both: the difference to the median, in counts of the tiles' "
                                           "own dtype, above which a pixel is replaced, 0..65535 (it must lie below the dtype's "
                                           "maximum: give one for uint8 tiles)")),
    (('--tile-qc',), dict(action='store_true',
                          help="report on every tile plane as it is in its file, from the bytes staged on the device (no pixel of "
                               "any output changes): <region>_stitched_tile_qc.csv with min, max, mean, std, saturated and zero "
                               "pixels, the Brenner focus sums, an exposure-independent focus score, the best z of every (fov, "
                               "channel) and the flags saturated / constant / low_focus, a summary in "
                               "<region>_stitched_tile_qc.json, and one printed line per region")),
    (('--tile-qc-saturation',), dict(type=float, default=0.01, metavar='F',
                                     help="with --tile-qc: a tile plane is flagged saturated when more than this fraction of its "
                                          "pixels is at the dtype's maximum, 0..1")),
    (('--tile-qc-focus-ratio',), dict(type=float, default=0.5, metavar='F',
                                      help="with --tile-qc: a tile plane is flagged low_focus when its focus score is below this "
                                           "fraction of the median over the tiles of its (channel, z) plane, 0..1")),
    (('--dpc',), dict(action='store_true',
                      help="add the channel DPC, the differential phase contrast of the two half-pupil brightfield channels of "
                           "--dpc-channels, made of every pair of tiles on the device before anything else touches them: "
                           "0.5 + (L - R) / (L + R) of the dtype's range, exact in integers and clipped (0 where both are 0) -- "
                           "what a run on a folder that also holds the files <region>_<fov>_<z>_DPC.tiff gives.  The channel "
                           "sits where its name sorts and is fused without a flatfield gain (the ratio cancels it); "
                           "registration and the flatfield estimate keep reading files; writes <region>_stitched_dpc.json")),
    (('--dpc-channels',), dict(nargs=2, default=('BF LED matrix left half', 'BF LED matrix right half'), metavar=('LEFT', 'RIGHT'),
                               help="with --dpc: the names of the left-half and the right-half channel")),
    (('--dpc-gain',), dict(type=int, default=1, metavar='G',
                           help="with --dpc: the difference is multiplied by this integer, 1..16, before the clip: "
                                "0.5 + G (L - R) / (L + R)")),
    (('--seam-qc',), dict(action='store_true',
                          help="report on every pair of overlapping tiles of every (channel, z) plane, from the planes staged on "
                               "the device as the fusion reads them -- after --dpc, --despeckle and --background-subtract, before "
                               "the flatfield divide (no pixel of any output changes): <region>_stitched_seam_qc.csv with the "
                               "pair's placement offset (dy, dx), the pixels compared (the overlap inset by the radius), the mean "
                               "of each side and the mean absolute difference in raw counts, the zero-normalised "
                               "cross-correlation ncc at the placement, the integer residual displacement (best_dy, best_dx) "
                               "within the radius at which the ncc is largest, and the flags unmeasured / featureless / low_ncc "
                               "/ shifted; a summary in <region>_stitched_seam_qc.json (per channel the median ncc per z and a "
                               "histogram of the residuals), and one printed line per region")),
    (('--seam-qc-radius',), dict(type=int, default=2, metavar='R',
                                 help="with --seam-qc: residual displacements up to this many pixels along each axis are tried, "
                                      "0..3")),
    (('--seam-qc-min-pixels',), dict(type=int, default=256, metavar='N',
                                     help="with --seam-qc: two tiles form a seam when their overlap, inset by the radius, has at "
                                          "least this many pixels")),
    (('--seam-qc-min-ncc',), dict(type=float, default=0.5, metavar='C',
                                  help="with --seam-qc: a seam is flagged low_ncc when its ncc at the placement is below this, "
                                       "-1..1")),
    (('--tile-binning',), dict(type=int, choices=range(1, 9), default=1, metavar='K',
                               help="stitch K x K binned tiles, 1..8: a run equals a run without the flag on a folder that holds "
                                    "the binned files, the same coordinates.csv and an acquisition parameters.json whose "
                                    "sensor_pixel_size_um is multiplied by K, byte for byte in every store, sidecar and picture.  "
                                    "The tiles are binned on the device right after the copy (the last h mod K rows and w mod K "
                                    "columns are dropped), before placement, registration, the flatfield estimate and every tile "
                                    "filter see them; writes <region>_stitched_binning.json.  1 = off")),
    (('--tile-binning-method',), dict(choices=['mean', 'sum'], default='mean',
                                      help="with --tile-binning: mean = the truncated mean of the K x K block, floor(S / K^2) (the "
                                           "rule of --pyramid-method mean); sum = min(S, dtype maximum), what camera binning does: "
                                           "counts add, and the result saturates")),
    (('--distortion-correction',), dict(type=_ppm, default=0, metavar='D',
                                        help="remove radial lens distortion from every tile: the output at radius r takes the "
                                             "input at radius r (1 + D 1e-6 r^2 / R^2), R the tile's half diagonal, bilinearly with "
                                             "8 fractional bits and replicated edges, exact in integers; D in parts per million, "
                                             "-50000..50000, is the relative displacement at the tile's corner: positive undoes "
                                             "pincushion, negative barrel distortion (find it with tools/distortion_scan.py).  A run "
                                             "equals a run without the flag on a folder whose tile files were corrected beforehand, "
                                             "byte for byte in every store, sidecar and picture.  The tiles are corrected on the "
                                             "device right after the copy, in sensor pixels, before --tile-binning, placement, "
                                             "registration, the flatfield estimate and every tile filter see them; a supplied "
                                             "flatfield is taken to be in corrected geometry; writes "
                                             "<region>_stitched_distortion.json.  0 = off")),
    (('--channel-shift',), dict(nargs=3, action='append', default=None, metavar=('NAME', 'DY', 'DX'),
                                help="align the tiles of output channel NAME (an RGB file's are <base>_R, <base>_G, <base>_B) to "
                                     "the other channels: a point imaged at (y, x) in the reference channel and at (y + DY, "
                                     "x + DX) in channel NAME is put right by --channel-shift NAME DY DX -- the output at (y, x) "
                                     "takes the input at (y + DY, x + DX), bilinearly with 8 fractional bits and replicated "
                                     "edges, exact in integers.  DY and DX are plain decimal numbers of pixels in -64..64, "
                                     "rounded to 1/256 pixel (find them with tools/channel_shift_scan.py); repeatable, a name "
                                     "once.  A run equals a run without the flag on a folder whose files of the shifted channels "
                                     "were translated beforehand, byte for byte in every store, sidecar and picture.  The tiles "
                                     "are shifted on the device after --distortion-correction and before --tile-binning, in "
                                     "sensor pixels; with -r the registration channel takes no shift, with --dpc neither DPC "
                                     "nor its half-pupil channels do; a supplied flatfield is taken to be in shifted geometry; "
                                     "writes <region>_stitched_channel_shift.json")),
    (('--channel-affine',), dict(nargs=5, action='append', default=None, metavar=('NAME', 'AYY', 'AYX', 'AXY', 'AXX'),
                                 help="rotate, scale or shear the tiles of output channel NAME about the tile centre, together "
                                      "with its --channel-shift: the output at centre + p takes the input at centre + "
                                      "(1 + A 1e-6) p + (DY, DX), A = [[AYY, AYX], [AXY, AXX]], p = (y, x), bilinearly with 8 "
                                      "fractional bits and replicated edges, exact in integers.  The four coefficients are plain "
                                      "integers in parts per million, -50000..50000 (find them with "
                                      "tools/channel_affine_scan.py): a rotation by t is AYY = AXX = (cos t - 1) 1e6, AYX = -AXY "
                                      "= sin t 1e6; a magnification m is AYY = AXX = (m - 1) 1e6.  Repeatable, a name once; a "
                                      "channel may have a shift, an affine, or both.  Everything else is --channel-shift's: the "
                                      "contract, the order, the channels that take none; writes "
                                      "<region>_stitched_channel_affine.json")),
    (('--dark-frame',), dict(nargs=2, action='append', default=None, metavar=('NAME', 'SOURCE'),
                             help="subtract the camera's additive term from every tile of output channel NAME (<base>_R/_G/_B "
                                  "for an RGB file; '*': every file channel without an entry of its own): out = clamp(I - D + P, "
                                  "0, M), P = --dark-pedestal, M the dtype's maximum, exact in integers.  SOURCE is a plain "
                                  "non-negative integer (a constant frame) or the path of a 2-D .tif, .tiff or .npy of exactly the "
                                  "files' shape and dtype (make one with tools/dark_frame_make.py); repeatable, a name once.  A "
                                  "run equals a run without the flag on a folder whose every tile file was subtracted "
                                  "beforehand: the tiles are subtracted on the device before --distortion-correction, "
                                  "--channel-shift / --channel-affine and --tile-binning, in sensor pixels; no file channel is "
                                  "exempt -- the registration channel takes its frame, with --dpc both half-pupil channels take "
                                  "theirs, DPC itself is read from no file and takes none; a supplied flatfield is used as "
                                  "given; a constant equal to the pedestal is the identity; writes "
                                  "<region>_stitched_dark_frame.json")),
    (('--dark-pedestal',), dict(type=int, default=0, metavar='P',
                                help="with --dark-frame: an integer in 0..M added back after the subtraction, so that noise below "
                                     "the dark level is not clipped at 0 (default 0)")),
)


def channel_shifts_of(entries):
    """--channel-shift NAME DY DX, as often as given -> {NAME: (Sy, Sx)} in 1/256 pixel (None when the flag is absent)."""
    if not entries:
        return None
    shifts = {}
    for name, dy, dx in entries:
        if name in shifts:
            raise ValueError(f"--channel-shift: channel {name!r} is given twice")
        shifts[name] = (channelshift.parse_pixels(dy), channelshift.parse_pixels(dx))
    return shifts


def channel_affines_of(entries):
    """--channel-affine NAME AYY AYX AXY AXX, as often as given -> {NAME: (Ayy, Ayx, Axy, Axx)} in parts per million (None when
    the flag is absent)."""
    if not entries:
        return None
    affines = {}
    for name, *coeffs in entries:
        if name in affines:
            raise ValueError(f"--channel-affine: channel {name!r} is given twice")
        affines[name] = tuple(channelaffine.parse_ppm(c) for c in coeffs)
    return affines


def dark_frames_of(entries):
    """--dark-frame NAME SOURCE, as often as given -> {NAME: int or path} (None when the flag is absent)."""
    if not entries:
        return None
    frames = {}
    for name, source in entries:
        if name in frames:
            raise ValueError(f"--dark-frame: channel {name!r} is given twice")
        frames[name] = darkframe.parse_source(source)
    return frames


def parse_args(argv=None) -> argparse.Namespace:
    parser = argparse.ArgumentParser(description="Squid tile stitcher, MI355X core")
    for names, kwargs in FLAGS:
        parser.add_argument(*names, **kwargs)
    return parser.parse_args(argv)


def create_params(args: argparse.Namespace) -> StitchingParameters:
    if args.params_json:
        return StitchingParameters.from_json(args.params_json)
    return StitchingParameters.from_dict({
        'input_folder': args.input_folder, 'output_format': args.output_format,
        'apply_flatfield': args.apply_flatfield, 'use_registration': args.use_registration,
        'registration_channel': args.registration_channel, 'registration_z_level': args.registration_z_level,
        'scan_pattern': args.scan_pattern, 'merge_timepoints': args.merge_timepoints,
        'merge_hcs_regions': args.merge_hcs_regions, 'dynamic_registration': args.dynamic_registration})


def init_distributed():
    """Under torchrun (WORLD_SIZE > 1): one process per GPU, RCCL process group."""
    import os
    world = int(os.environ.get('WORLD_SIZE', '1'))
    if world <= 1:
        return None
    import torch
    import torch.distributed as dist
    local = int(os.environ.get('LOCAL_RANK', '0'))
    backend = os.environ.get('SQ_DIST_BACKEND', 'nccl')
    device = torch.device('cuda', local % max(1, torch.cuda.device_count()))
    torch.cuda.set_device(device)
    os.environ.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
    if not dist.is_initialized():
        if backend == 'nccl':
            dist.init_process_group('nccl', device_id=device)
        else:
            dist.init_process_group(backend)
    return device


def main(argv=None):
    args = parse_args(argv)
    try:
        device = init_distributed()
        params = create_params(args)
        stitcher = Stitcher(params, device=device, fusion_mode=args.fusion_mode,
                            normalization=None if args.normalization == 'none' else 'phase',
                            zarr_compression=args.zarr_compression,
                            per_region_registration=args.per_region_registration,
                            flatfield_estimator=args.flatfield_estimator,
                            all_pairs_registration=args.all_pairs_registration,
                            global_registration=args.global_registration,
                            z_projection=args.z_projection,
                            focus_radius=args.focus_radius,
                            pyramid_method=args.pyramid_method,
                            contrast_limits=args.contrast_limits,
                            contrast_percentiles=tuple(args.contrast_percentiles),
                            focus_guide_channel=args.focus_guide_channel,
                            focus_depth_map=args.focus_depth_map,
                            composite=args.composite,
                            composite_max_side=args.composite_max_side,
                            composite_z=args.composite_z,
                            composite_channels=args.composite_channels,
                            background_subtract=args.background_subtract,
                            background_radius=args.background_radius,
                            despeckle=args.despeckle,
                            despeckle_threshold=args.despeckle_threshold,
                            tile_qc=args.tile_qc,
                            tile_qc_saturation=args.tile_qc_saturation,
                            tile_qc_focus_ratio=args.tile_qc_focus_ratio,
                            seam_qc=args.seam_qc,
                            seam_qc_radius=args.seam_qc_radius,
                            seam_qc_min_pixels=args.seam_qc_min_pixels,
                            seam_qc_min_ncc=args.seam_qc_min_ncc,
                            dpc=args.dpc,
                            dpc_channels=tuple(args.dpc_channels),
                            dpc_gain=args.dpc_gain,
                            tile_binning=args.tile_binning,
                            tile_binning_method=args.tile_binning_method,
                            distortion_correction=args.distortion_correction,
                            channel_shifts=channel_shifts_of(args.channel_shift),
                            channel_affines=channel_affines_of(args.channel_affine),
                            dark_frames=dark_frames_of(args.dark_frame),
                            dark_pedestal=args.dark_pedestal,
                            ome_tiff_layout=args.ome_tiff_layout,
                            ome_tiff_compression=args.ome_tiff_compression,
                            ome_tiff_quality=args.ome_tiff_quality)
        print("Starting stitching with parameters:")
        for k, v in params.to_dict().items():
            print(f"{k}: {v}")
        stitcher.run()
    except Exception as e:   # same contract as the reference: message on stderr, exit 1
        print(f"Error: {e}", file=sys.stderr)
        sys.exit(1)


if __name__ == '__main__':
    main()
