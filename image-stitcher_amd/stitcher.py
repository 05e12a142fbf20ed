"""``Stitcher``: the reference's class surface (stitcher.py:31) over the MI355X core.

Same constructor, same method names / argument meaning / error behaviour for the methods a
front-end touches -- ``run``, ``calculate_shifts``, ``calculate_horizontal_shift``,
``calculate_vertical_shift``, ``normalize_image``, ``apply_flatfield_correction``,
``calculate_output_dimensions``, ``stitch_region`` -- and the same state attributes
(``h_shift``, ``v_shift``, ``h_shift_rev``, ``h_shift_rev_odd``, ``flatfields``,
``acquisition_metadata``, ``x_positions``, ``y_positions``, ...).  What differs is inside:

* registration and fusion run as HIP kernels through the C-ABI (``native``); there is no CPU
  path -- a missing library or GPU raises;
* a region is fused in one launch over all its (channel, z) planes from a device-resident
  tile stack, instead of one dask ``__setitem__`` layer per file;
* metadata lookups are indexed once (the reference rescans per file).

Qt is not required: signals are plain callback lists with ``emit``/``connect``.
"""
from __future__ import annotations

import contextlib
import json
import math
import os
import random
import time
from concurrent.futures import ThreadPoolExecutor
from typing import Dict, List, Optional, Tuple

import numpy as np
try:
    import psutil
except Exception:   # pragma: no cover
    psutil = None      # stitch_planes then assumes 8 GiB of free host memory

from . import alignment, binning, channelaffine, channelshift, composite as composite_mod, darkframe, distortion, native, placement, registration, seamqc, sharding, tileqc
from . import omezarr
from .omezarr import write_ome_zarr
from . import ometiff
from .ometiff import write_ome_tiff
from .placement import Shifts
from .stitcher_parameters import StitchingParameters
from .tiffio import read_image, read_image_into
from .tilechain import TileChain, warp_and_bin

_IMAGE_EXT = ('.bmp', '.tiff', 'tif', 'jpg', 'jpeg', 'png')   # as the reference spells them (stitcher.py:169)


class Signal:
    """Tiny stand-in for a Qt signal (stitcher.py:33-37)."""

    def __init__(self, *types):
        self._slots = []

    def connect(self, fn):
        self._slots.append(fn)

    def emit(self, *args):
        for fn in list(self._slots):
            fn(*args)


class FocusFollower:
    """A ``stitch_planes(project_to=...)`` target for a channel that follows the guide channel of the best-focus projection:
    ``out`` [Hc, Wc] receives, per voxel, the channel's fused value at the guide's depth (sq_fuse_select_depth); ``depth``
    [Hc, Wc] uint8 / uint16 is the guide's unsigned depth plane.  ``guide``: the guide's channel index when its (output, key)
    target is in the same ``project_to`` -- ``depth`` is then derived there once the guide's last plane has been projected --
    or None when ``depth`` is already filled."""
    __slots__ = ('out', 'depth', 'guide')

    def __init__(self, out, depth, guide=None):
        self.out, self.depth, self.guide = out, depth, guide


class Stitcher:
    def __init__(self, params: StitchingParameters, device=None, fusion_mode: str = 'overwrite',
                 normalization: Optional[str] = 'phase', zarr_compression: str = 'blosc',
                 per_region_registration: bool = False, flatfield_estimator: str = 'auto',
                 all_pairs_registration: bool = False, global_registration: bool = False, z_projection: str = 'none',
                 focus_radius: int = 3, pyramid_method: str = 'nearest', contrast_limits: str = 'dtype',
                 contrast_percentiles=(0.1, 99.9), focus_guide_channel: Optional[str] = None, focus_depth_map: bool = False,
                 composite: bool = False, composite_max_side: int = 4096, composite_z: Optional[int] = None,
                 composite_channels=None, background_subtract: str = 'none', background_radius: int = 50,
                 despeckle: str = 'none', despeckle_threshold: int = 1000, tile_qc: bool = False,
                 tile_qc_saturation: float = 0.01, tile_qc_focus_ratio: float = 0.5, dpc: bool = False,
                 dpc_channels=('BF LED matrix left half', 'BF LED matrix right half'), dpc_gain: int = 1,
                 seam_qc: bool = False, seam_qc_radius: int = 2, seam_qc_min_pixels: int = 256, seam_qc_min_ncc: float = 0.5,
                 tile_binning: int = 1, tile_binning_method: str = 'mean', distortion_correction: int = 0,
                 channel_shifts=None, channel_affines=None, dark_frames=None, dark_pedestal=0,
                 ome_tiff_layout: str = 'planes', ome_tiff_compression: str = 'deflate', ome_tiff_quality: int = 90):
        self.update_progress = Signal(int, int)
        self.getting_flatfields = Signal()
        self.starting_stitching = Signal()
        self.starting_saving = Signal(bool)
        self.finished_saving = Signal(str, object)

        self.params = params
        params.validate()
        self.input_folder = params.input_folder
        self.output_folder = params.stitched_folder
        self.output_format = params.output_format
        self.merge_timepoints = getattr(params, 'merge_timepoints', False)
        self.merge_hcs_regions = getattr(params, 'merge_hcs_regions', False)
        self.per_timepoint_region_output_template = os.path.join(
            self.output_folder, "{timepoint}_stitched", "{region}_stitched" + self.output_format)
        self.apply_flatfield = params.apply_flatfield
        self.use_registration = params.use_registration
        if self.use_registration:
            self.registration_channel = params.registration_channel
            self.registration_z_level = params.registration_z_level
            self.dynamic_registration = params.dynamic_registration   # stored and never read, like the reference (stitcher.py:92)
        self.scan_pattern = params.scan_pattern
        if fusion_mode not in ('overwrite', 'feather'):
            raise ValueError("fusion_mode must be 'overwrite' or 'feather'")
        self.fusion_mode = fusion_mode            # 'feather' is an extension the reference lacks
        self.normalization = normalization        # scikit-image >= 0.19 default is 'phase'
        # Extension: per-channel maximum-intensity projection over z from the tiles on the device (sq_fuse_project_max).
        # 'max' writes <region>_stitched_mip<format> beside the stack, 'max-only' writes the projection alone.
        # 'focus' / 'focus-only': the best-focus (extended depth of field) projection instead (sq_fuse_project_focus), written
        # to <region>_stitched_edf<format>; focus_radius is its window radius R (0..15).
        if z_projection not in ('none', 'max', 'max-only', 'focus', 'focus-only'):
            raise ValueError("z_projection must be 'none', 'max', 'max-only', 'focus' or 'focus-only'")
        if z_projection != 'none' and fusion_mode != 'overwrite':
            raise ValueError(f"z_projection={z_projection!r} projects overwrite fusion only; it cannot be combined with "
                             f"fusion_mode={fusion_mode!r}")
        if isinstance(focus_radius, bool) or not isinstance(focus_radius, (int, np.integer)) or \
                not 0 <= int(focus_radius) <= native.SQ_FOCUS_MAX_RADIUS:
            raise ValueError(f"focus_radius must be an integer in 0..{native.SQ_FOCUS_MAX_RADIUS}, got {focus_radius!r}")
        self.z_projection = z_projection
        self.focus_radius = int(focus_radius)
        # Extension of the best-focus projection: focus_guide_channel = a name out of monochrome_channels whose depth decides
        # for every channel (the others take their fused value at the guide's depth: sq_fuse_select_depth);
        # focus_depth_map = also write the depth (z* + 1, 0 = uncovered) to <region>_stitched_depth<format>.
        if (focus_guide_channel is not None or focus_depth_map) and z_projection not in ('focus', 'focus-only'):
            raise ValueError("focus_guide_channel / focus_depth_map belong to the best-focus projection: they need "
                             f"z_projection 'focus' or 'focus-only', got {z_projection!r}")
        if focus_guide_channel is not None and not isinstance(focus_guide_channel, str):
            raise ValueError(f"focus_guide_channel must be a channel name, got {focus_guide_channel!r}")
        self.focus_guide_channel = focus_guide_channel
        self.focus_depth_map = bool(focus_depth_map)
        self._guide = None      # the guide's index in monochrome_channels, once the metadata is parsed
        # Extension: how the OME-Zarr levels above 0 are made.  'nearest' = the reference's Scaler.nearest (stitcher.py:797-798);
        # 'mean' = the truncated 2 x 2 mean its other stitchers store (zarr_stitcher.py:614-719), all levels from one read of
        # level 0 (sq_pyramid_mean).  Applies to every store a run writes (stack, _mip, _edf) and to the pyramid layout of
        # .ome.tiff (ome_tiff_layout below); the planes layout of .ome.tiff holds level 0 only.
        self.pyramid_method = omezarr.check_pyramid_method(pyramid_method)
        # Extension: the channel windows of the omero block.  'dtype' = the reference's 0 ... np.iinfo(dtype).max
        # (stitcher.py:846-850); 'percentile' = contrast_percentiles (lo, hi) of the non-zero voxels of each store's own level 0,
        # from exact histograms the stream writer keeps on the device (sq_histogram_planes), with a _histogram.npy and a
        # _stats.json beside every store.  OME-XML has no rendering window, so .ome.tiff output refuses it.
        self.contrast_limits, self.contrast_percentiles = omezarr.check_contrast(contrast_limits, contrast_percentiles)
        if self.contrast_limits == 'percentile' and not self.output_format.endswith('.zarr'):
            raise ValueError("contrast_limits='percentile' needs .ome.zarr output: OME-XML (.ome.tiff) has no rendering window "
                             "to carry the channel windows")
        # Extension: composite = one colour quick-look PNG (+ JSON sidecar) per (timepoint, region) instead of the reference's
        # dormant _save_debug_slice (stitcher.py:861-885): the projection the run writes, or z plane composite_z (default
        # num_z // 2) of the stack, reduced on the device to block means of at most composite_max_side pixels a side
        # (sq_block_mean), windowed by contrast_percentiles of its own value counts -- whatever contrast_limits says -- and added
        # in the channel colours (sq_composite_render).  composite_channels restricts and orders the channels (names out of
        # monochrome_channels).  Off: nothing is launched and no file appears.
        self.composite, self.composite_max_side, self.composite_z, self.composite_channels = \
            composite_mod.check_options(composite, composite_max_side, composite_z, composite_channels)
        self._composite_pending = []     # (target, pinned counts, event) of streamed regions, see _finish_composites
        self._composite_jobs = []        # PNG encodings under way on the pool
        self._composite_pool = None
        self._composite_async = False    # run(): PNGs are encoded on a worker thread
        # Extension: background_subtract='tophat' removes the slowly varying additive background of every staged tile plane on the
        # device before anything is projected or fused (sq_tophat_tiles): the plane minus its opening with a square window of
        # radius background_radius (1..127), clipped to the tile -- what filtering the files beforehand gives.  It runs on the
        # raw tile, before the flatfield divide; registration and the flatfield estimate keep reading raw tiles.  Meant for
        # fluorescence; on brightfield it is simply what the definition says.  'none': nothing is launched or allocated.  A
        # radius without 'tophat' is accepted and unused.
        if background_subtract not in ('none', 'tophat'):
            raise ValueError(f"background_subtract must be 'none' or 'tophat', got {background_subtract!r}")
        if isinstance(background_radius, bool) or not isinstance(background_radius, (int, np.integer)) or \
                not 1 <= int(background_radius) <= native.SQ_TOPHAT_MAX_RADIUS:
            raise ValueError(f"background_radius must be an integer in 1..{native.SQ_TOPHAT_MAX_RADIUS}, got {background_radius!r}")
        self.background_subtract = background_subtract
        self.background_radius = int(background_radius)
        # Extension: despeckle='hot' / 'both' replaces single-pixel outliers (hot pixels, cosmic hits; 'both': dead pixels too)
        # of every staged tile plane on the device before anything else touches it (sq_despeckle_tiles): a pixel that differs
        # from the median m of its edge-replicated 3 x 3 window by more than despeckle_threshold counts of the tile's own dtype
        # ('hot': I - m > T, 'both': |I - m| > T) becomes m -- what filtering the files beforehand gives.  It runs right after
        # the copy to the device, before the background removal and the flatfield divide; registration and the flatfield
        # estimate keep reading raw tiles.  'none': nothing is launched, allocated or written.  A threshold without a mode is
        # accepted and unused; one at or above the dtype's maximum could never fire and is refused once the dtype is known
        # (_check_despeckle_dtype).
        if despeckle not in ('none', 'hot', 'both'):
            raise ValueError(f"despeckle must be 'none', 'hot' or 'both', got {despeckle!r}")
        if isinstance(despeckle_threshold, bool) or not isinstance(despeckle_threshold, (int, np.integer)) or \
                not 0 <= int(despeckle_threshold) <= native.SQ_DESPECKLE_MAX_THRESHOLD:
            raise ValueError(f"despeckle_threshold must be an integer in 0..{native.SQ_DESPECKLE_MAX_THRESHOLD}, "
                             f"got {despeckle_threshold!r}")
        self.despeckle = despeckle
        self.despeckle_threshold = int(despeckle_threshold)
        # {channel name: staged pixels replaced / staged pixels filtered by this process}.  They count STAGED pixels: a tile
        # that is staged for two row bands (or by two calls) counts twice.
        self.despeckle_replaced: Dict[str, int] = {}
        self.despeckle_staged: Dict[str, int] = {}
        self._despeckle_pending = []     # (timepoint, region, device counts [num_c], staged pixels [num_c]) not read back yet
        # Extension: tile_qc=True reports on every tile plane as it is in its file: the eight words of sq_tile_stats (min, max,
        # sum, sum of squares, pixels at the dtype's maximum and at 0, the Brenner sums along x and y) of every staged plane,
        # taken right after the copy to the device and before the despeckle, and what tileqc.py derives of them (mean, std,
        # focus, best z, the flags 'saturated' above tile_qc_saturation of the pixels, 'constant', 'low_focus' below
        # tile_qc_focus_ratio of the plane's median focus) as <region>_stitched_tile_qc.csv / .json.  It changes no pixel of
        # any output.  False: nothing is launched, allocated, written or synchronised; the two values are accepted and unused.
        self.tile_qc, self.tile_qc_saturation, self.tile_qc_focus_ratio = \
            tileqc.check_options(tile_qc, tile_qc_saturation, tile_qc_focus_ratio)
        self.tile_qc_table: Dict[tuple, List[dict]] = {}      # (timepoint, region) -> the rows of its CSV
        self._tile_qc_words: Dict[tuple, Dict[tuple, tuple]] = {}      # (timepoint, region) -> {(plane, fov): the eight words}
        self._tile_qc_pending = []       # (timepoint, region, device words [planes, tiles, 8], [(plane, fov)]) not read back yet
        self._tile_qc_shared = False     # the ranks share this region: the words are combined before anything is written
        # Extension: seam_qc=True reports on every pair of overlapping tiles of every (channel, z) plane: how well the two
        # agree where they are placed, and the integer residual displacement within +-seam_qc_radius at which they would
        # agree best (sq_seam_stats' exact sums over the overlap inset by the radius; seamqc.py for the definition, the ncc,
        # the flags 'unmeasured', 'featureless', 'low_ncc' below seam_qc_min_ncc and 'shifted') as
        # <region>_stitched_seam_qc.csv / .json.  A pair is a seam when its inset overlap has seam_qc_min_pixels pixels.  The
        # sums are taken of the staged planes as the fusion reads them: after dpc, despeckle and background removal, before the
        # flatfield divide.  The three defaults are design choices, not measurements.  It changes no pixel of any output.
        # False: nothing is launched, allocated, written or synchronised; the three values are checked and unused.
        self.seam_qc, self.seam_qc_radius, self.seam_qc_min_pixels, self.seam_qc_min_ncc = \
            seamqc.check_options(seam_qc, seam_qc_radius, seam_qc_min_pixels, seam_qc_min_ncc)
        self.seam_qc_table: Dict[tuple, List[dict]] = {}      # (timepoint, region) -> the rows of its CSV
        self._seam_qc_words: Dict[tuple, Dict[tuple, tuple]] = {}     # (timepoint, region) -> {(plane, ref fov, mov fov): words}
        self._seam_qc_pending = []       # (timepoint, region, device words [planes, seams, words], plane ids, [(ref, mov)])
        self._seam_qc_tables: Dict[tuple, tuple] = {}      # (rectangle list, fovs) -> (seams, host table, device table)
        self._seam_qc_layouts: Dict[tuple, tuple] = {}     # (timepoint, region) -> (its seams, {plane: fovs with a file}), as staged
        self._seam_qc_planes: Dict[tuple, set] = {}        # (timepoint, region) -> the planes staged so far
        self._seam_qc_shared = False     # the ranks share this region: the words are combined before anything is written
        # Extension: dpc=True adds one derived channel, 'DPC', the differential phase contrast of the two half-pupil brightfield
        # channels dpc_channels = (left, right): with S = L + R, N = S + 2 dpc_gain (L - R) and M the dtype's maximum, 0 where
        # S == 0 and clamp(floor(M N / (2 S)), 0, M) elsewhere (sq_dpc_tiles; tests/dpc_ref.py) -- for gain 1 Squid's
        # generate_dpc, M (0.5 + (L - R) / (L + R)), without its float rounding.  It is made of the staged tiles on the device,
        # right after the copy and before anything else touches them, so a run equals a run without the option on a folder
        # that also holds the files <region>_<fov>_<z>_DPC.tiff: the channel sits where its name sorts, and goes through the
        # tile report, the despeckle, the background removal, the projections and the fusion like a file channel.  The one
        # exception is the flatfield: the ratio cancels a multiplicative gain, so the channel is fused without one and the
        # estimate never samples it.  Registration reads files: it never sees the channel.  False: nothing is parsed
        # differently, allocated, launched or written; the other two values are checked and unused.
        if not isinstance(dpc, (bool, np.bool_)):
            raise ValueError(f"dpc must be True or False, got {dpc!r}")
        if isinstance(dpc_channels, str) or not isinstance(dpc_channels, (tuple, list)) or len(dpc_channels) != 2 or \
                not all(isinstance(n, str) and n for n in dpc_channels):
            raise ValueError(f"dpc_channels must be two channel names (left, right), got {dpc_channels!r}")
        if isinstance(dpc_gain, bool) or not isinstance(dpc_gain, (int, np.integer)) or \
                not 1 <= int(dpc_gain) <= native.SQ_DPC_MAX_GAIN:
            raise ValueError(f"dpc_gain must be an integer in 1..{native.SQ_DPC_MAX_GAIN}, got {dpc_gain!r}")
        self.dpc = bool(dpc)
        self.dpc_channels = tuple(dpc_channels)
        self.dpc_gain = int(dpc_gain)
        self._dpc_index = None      # the derived channel's index in monochrome_channels, once the metadata is parsed
        if self.dpc:
            if self.dpc_channels[0] == self.dpc_channels[1]:
                raise ValueError(f"dpc_channels names one channel twice: {self.dpc_channels[0]!r}")
            if native.DPC_CHANNEL in self.dpc_channels:
                raise ValueError(f"dpc_channels {self.dpc_channels}: {native.DPC_CHANNEL!r} is the derived channel's own name")
            if params.registration_channel == native.DPC_CHANNEL:
                raise ValueError(f"registration_channel {native.DPC_CHANNEL!r} is the derived channel: registration reads files")
        # Extension: tile_binning=K (1..8) stitches K x K binned tiles: with hb = h // K and wb = w // K (the last rows and columns
        # are dropped) and S the sum of a K x K block, tile_binning_method 'mean' gives floor(S / K^2) -- the truncated mean of
        # pyramid_method='mean' -- and 'sum' gives min(S, M), M the dtype's maximum: camera binning (binning.py;
        # tests/bin_ref.py).  A run equals a run without the option on a folder that holds the binned files, the same
        # coordinates.csv and an 'acquisition parameters.json' whose sensor_pixel_size_um is multiplied by K, byte for byte
        # in every store, sidecar and picture: the staged tiles are binned on the device as the first launch after the copy
        # (sq_bin_tiles), the all-pairs stack likewise, and the readers of single files (the metadata probe, get_tile and the
        # centre-pair registration, the flatfield estimate's samples) bin on the host -- placement, registration, the
        # flatfield estimate and every tile filter see binned tiles only.  input_height / input_width are the binned size
        # (file_height / file_width the files'), pixel_size_um the binned pixel's.  1: nothing is launched, allocated, written
        # or parsed differently; the method is checked and unused.
        self.tile_binning, self.tile_binning_method = binning.check_options(tile_binning, tile_binning_method)
        # Extension: distortion_correction=D (an integer in parts per million, -50000..50000) removes radial lens distortion
        # from every tile: the output at radius r takes the input at radius r (1 + D 10^-6 r^2 / R^2), R the tile's half
        # diagonal, bilinearly with 8 fractional bits and replicated edges, exact in integers (distortion.py;
        # tests/warp_ref.py); D > 0 undoes pincushion, D < 0 barrel distortion.  A run equals a run without the option on a
        # folder whose tile files were corrected beforehand, byte for byte in every store, sidecar and picture: the staged
        # tiles are corrected on the device as the first launch after the copy (sq_warp_tiles), the all-pairs stack
        # likewise, and the readers of single files (get_tile and the centre-pair registration, the flatfield estimate's
        # samples) correct on the host -- placement, registration, the flatfield estimate and every tile filter see corrected
        # tiles only.  With tile_binning the tiles are corrected first, in sensor pixels, and binned second.  A supplied
        # flatfield is taken to be in corrected geometry.  0: nothing is launched, allocated, written, synchronised or parsed
        # differently.
        self.distortion_correction = distortion.check_option(distortion_correction)
        # Extension: channel_shifts={output channel name: (Sy, Sx)}, Python ints in 1/256 pixel within -16384..16384, moves
        # every tile of a channel by a constant sub-pixel translation: the output at (y, x) takes the input at (y + Sy/256,
        # x + Sx/256), bilinearly with 8 fractional bits and replicated edges, exact in integers (channelshift.py;
        # tests/shift_ref.py) -- a point imaged at (y, x) in the reference channel and at (y + DY, x + DX) in the named one is
        # put right by (256 DY, 256 DX).  A run equals a run without the option on a folder whose files of the shifted channels
        # were translated beforehand, byte for byte in every store, sidecar and picture: the staged tiles are shifted on the
        # device (sq_shift_tiles) behind the distortion correction and in front of the binning, all in sensor pixels, and the
        # readers of single files (get_tile, the flatfield estimate's samples) shift on the host.  The registration channel
        # is the frame the others are moved into and takes no shift; nor do the channels --dpc reads or derives.  A supplied
        # flatfield is taken to be in shifted geometry.  None, empty or all zero: nothing is launched, allocated, written,
        # synchronised or parsed differently.
        self.channel_shifts = channelshift.check_option(channel_shifts)
        self._channel_shift_index: Dict[int, Tuple[int, int]] = {}      # output channel index -> pair, once the names are known
        # Extension: channel_affines={output channel name: (Ayy, Ayx, Axy, Axx)}, Python ints in parts per million within
        # -50000..50000, adds the linear term to the channel's shift: the output at centre + p takes the input at centre +
        # (1 + A 10^-6) p + S/256, one map, with the shift's blend, exact in integers (channelaffine.py; tests/affine_ref.py) --
        # a second camera that is not mounted square (rotation by t: Ayy = Axx = (cos t - 1) 10^6, Ayx = -Axy = sin t 10^6) or a
        # channel that is magnified differently (m: Ayy = Axx = (m - 1) 10^6).  The contract, the order (correct, shift + affine,
        # bin), the channels that take none and the readers that map on the host are those of channel_shifts; a channel may have
        # a shift, an affine, or both.  The staged tiles go through sq_affine_tiles, one launch per chunk that holds a plane with
        # a non-zero A in the place of the shift's.  None, empty or all zero: nothing is launched, allocated, written,
        # synchronised or parsed differently.
        self.channel_affines = channelaffine.check_option(channel_affines)
        self._channel_affine_index: Dict[int, Tuple[int, int, int, int]] = {}
        # Extension: dark_frames={output channel name, or '*' for every file channel without an entry of its own: a constant
        # int, a 2-D array or the path of a .tif / .tiff / .npy of exactly the files' shape and dtype} with dark_pedestal=P
        # subtracts the camera's additive term from every tile: out = clamp(I - D + P, 0, M), exact in integers (darkframe.py;
        # tests/dark_ref.py) -- the `I - D` of the flatfield correction (I - D) / F.  A run equals a run without the option on
        # a folder whose every tile file was subtracted beforehand, byte for byte in every store, sidecar and picture: the
        # staged tiles and the right halves of --dpc are subtracted on the device (sq_dark_tiles, in place, the first launch of
        # the chain: in front of the distortion correction, the channel shift / affine and the binning, all in sensor pixels),
        # registration's stack takes the registration channel's frame, and the readers of single files (get_tile, the
        # centre-pair registration, the flatfield estimate's samples) subtract on the host.  No file channel is exempt; 'DPC'
        # is read from no file and takes none.  A supplied flatfield is used as given.  A constant equal to P is the identity
        # and launches nothing.  None or empty: nothing is launched, allocated, written, synchronised or parsed differently.
        self.dark_frames, self.dark_pedestal = darkframe.check_option(dark_frames, dark_pedestal)
        self._dark_host: Dict[str, object] = {}               # output channel name -> int or array, the identities left out
        self._dark_params: Dict[int, Tuple[int, int]] = {}    # output channel index -> (k, c), the identities left out
        self._dark_right = None                               # the pair of --dpc's right halves
        self._dark_stack = None                               # the distinct frames [K, fh, fw], host
        self._dark_note: Dict[str, dict] = {}                 # file channel name -> what the sidecar says of its frame
        if zarr_compression not in ('blosc', 'zlib', 'none'):
            raise ValueError("zarr_compression must be 'blosc', 'zlib' or 'none'")
        self.zarr_compression = zarr_compression
        # Extension: how an .ome.tiff is laid out.  'planes' = one uncompressed strip per (t, c, z) plane, level 0 only (the
        # file of write_ome_tiff, from the fused region in host memory); 'pyramid' = the OME-TIFF 6 pyramid -- tiled planes
        # (chunks[3:5], sides multiples of 16), num_pyramid_levels levels in SubIFDs, streamed batch by batch like a store;
        # ome_tiff_compression 'deflate' = Adobe deflate with the horizontal predictor, encoded on the device
        # (sq_deflate_encode_planes), 'none' = raw tiles, 'jpeg' = baseline JPEG tiles (TIFF Compression 7) at ome_tiff_quality
        # (1..100; 90 is a choice, not a measurement), encoded on the device (sq_jpeg_encode_planes): uint8 acquisitions only,
        # refused once the metadata has told the dtype.  Lossy: the depth-map file of --focus-depth-map stays deflate.
        self.ome_tiff_layout, self.ome_tiff_compression = ometiff.check_tiff_options(ome_tiff_layout, ome_tiff_compression,
                                                                                     self.output_format, quality=ome_tiff_quality)
        self.ome_tiff_quality = int(ome_tiff_quality)
        if flatfield_estimator not in ('auto', 'basic', 'basicpy', 'mean'):
            raise ValueError("flatfield_estimator must be 'auto', 'basic', 'basicpy' or 'mean'")
        self.flatfield_estimator = flatfield_estimator
        self.flatfield_estimator_used = None      # set by get_flatfields
        self.flatfield_info = None
        # False: shifts are measured once, on the first timepoint and region, and used everywhere (the
        # reference, stitcher.py:1244-1246).  True: every (timepoint, region) is registered on its own
        # tiles before it is fused (BASELINE config 5: per-well registration).
        self.per_region_registration = bool(per_region_registration) and self.use_registration
        # Extension of this build (the north star's batched registration), behind a flag of its own: every adjacent pair of
        # the registration plane, per-axis median.  The reference's --dynamic-registration is parsed, stored and ignored
        # (stitcher.py:92, stitcher_parameters.py:24), so that flag keeps the centre-pair result here too.
        self.all_pairs_registration = bool(all_pairs_registration) and self.use_registration
        # Extension: every tile at its own integer position from a least-squares solve over all registered pairs
        # (alignment.py).  Positions are per tile, so every (timepoint, region) is registered and solved on its own, as with
        # per_region_registration; the reference's state attributes still get the all-pairs medians.
        self.global_registration = bool(global_registration) and self.use_registration
        self.placements: Dict[tuple, alignment.Placement] = {}     # (timepoint, region) -> solved positions
        self._global_rects: Dict[tuple, dict] = {}
        self.batch_bytes_limit = 4 << 30          # tile bytes staged (pinned + device) per ingest batch
        self._device = device
        self._plan_cache: Dict[tuple, native.FusePlan] = {}
        self._buffer_cache: Dict[tuple, object] = {}
        # the canvas' home: device memory mapped over all memory classes of the card (native.DeviceArena), kept for the next
        # region; canvases below canvas_arena_min_bytes (and every canvas when the platform lacks virtual memory
        # management) come from a plain allocation
        self.canvas_arena_min_bytes = int(os.environ.get('SQ_CANVAS_ARENA_MIN_BYTES', 2 << 30))
        self._arena = None
        self._arena_unsupported = False
        # the stream writer of the .ome.zarr path lives across regions of one geometry (its two slots alternate: the chunks of
        # region k are written while region k + 1 is read, registered and fused); run() drains it once at the end
        self._stream_writer = None
        self._defer_drain = False
        self._contrast_pending = []      # (store, pinned counts, event, device counts) of streamed regions, see _finish_contrast
        self.canvas_arena_info = None
        self.init_stitching_parameters()

    # ------------------------------------------------------------------ state
    def init_stitching_parameters(self):
        """(stitcher.py:98-119)"""
        self.pixel_size_um = None
        self.pixel_binning = 1
        self.acquisition_params = None
        self.timepoints = []
        self.regions = []
        self.channel_names = []
        self.monochrome_channels = []
        self.monochrome_colors = []
        self.num_z = self.num_c = self.num_t = 1
        self.input_height = self.input_width = 0      # the tiles as everything downstream sees them (binned with tile_binning)
        self.file_height = self.file_width = 0        # the tiles as they are in their files
        self.file_pixel_size_um = None
        self.num_pyramid_levels = 5
        self.flatfields = {}
        self.acquisition_metadata = {}
        self.dtype = np.uint16
        self.chunks = None
        self.h_shift = (0, 0)
        if self.scan_pattern == 'S-Pattern':
            self.h_shift_rev = (0, 0)
            self.h_shift_rev_odd = 0
        self.v_shift = (0, 0)
        self.x_positions = set()
        self.y_positions = set()
        self._region_index: Dict[tuple, Dict[tuple, dict]] = {}

    @property
    def device(self):
        import torch
        if self._device is None:
            if not torch.cuda.is_available():
                raise RuntimeError("Stitcher needs an MI355X (torch.cuda is not available); there is no CPU path")
            self._device = torch.device('cuda', torch.cuda.current_device())
        return self._device

    # --------------------------------------------------------------- metadata
    def get_timepoints(self):
        """(stitcher.py:121-124)"""
        self.timepoints = [d for d in os.listdir(self.input_folder)
                           if os.path.isdir(os.path.join(self.input_folder, d)) and d.isdigit()]
        self.timepoints.sort(key=int)
        return self.timepoints

    def extract_acquisition_parameters(self):
        with open(os.path.join(self.input_folder, 'acquisition parameters.json'), 'r') as fh:
            self.acquisition_params = json.load(fh)

    def get_pixel_size(self):
        """(stitcher.py:131-140)"""
        ap = self.acquisition_params
        obj_focal_length_mm = ap['objective']['tube_lens_f_mm'] / ap['objective']['magnification']
        actual_mag = ap['tube_lens_mm'] / obj_focal_length_mm
        self.pixel_binning = ap.get('pixel_binning', 1)
        self.file_pixel_size_um = ap['sensor_pixel_size_um'] / actual_mag
        # (in this order: bit for bit what a folder of binned files, whose sensor pixel is K times as large, gives)
        self.pixel_size_um = (ap['sensor_pixel_size_um'] * self.tile_binning) / actual_mag if self.tile_binning > 1 \
            else self.file_pixel_size_um
        print(f"[metadata] pixel size {self.pixel_size_um} um")

    @staticmethod
    def _read_coordinates(path: str) -> Dict[tuple, Tuple[float, float, float]]:
        """coordinates.csv -> {(region, fov, z): (x mm, y mm, z um)}, first row wins like
        ``coord_row.iloc[0]`` (stitcher.py:176-186)."""
        table: Dict[tuple, Tuple[float, float, float]] = {}
        with open(path) as fh:
            header = [h.strip() for h in fh.readline().rstrip('\n').split(',')]
            col = {name: i for i, name in enumerate(header)}
            for line in fh:
                parts = line.rstrip('\n').split(',')
                if len(parts) < len(header):
                    continue
                key = (parts[col['region']], int(parts[col['fov']]), int(parts[col['z_level']]))
                if key not in table:
                    table[key] = (float(parts[col['x (mm)']]), float(parts[col['y (mm)']]), float(parts[col['z (um)']]))
        return table

    def parse_acquisition_metadata(self):
        """File names -> ``acquisition_metadata`` in sorted-filename order (stitcher.py:143-257)."""
        self.acquisition_metadata = {}
        self._region_index = {}
        regions, channels = set(), set()
        max_z = max_fov = 0
        dpc_unpaired = 0
        for timepoint in self.timepoints:
            image_folder = os.path.join(self.input_folder, str(timepoint))
            print(f"[metadata] timepoint {timepoint}: {image_folder}")
            try:
                coords = self._read_coordinates(os.path.join(image_folder, 'coordinates.csv'))
            except FileNotFoundError:
                print(f"Warning: timepoint {timepoint} has no coordinates.csv, skipped")
                continue
            files = sorted(f for f in os.listdir(image_folder) if f.endswith(_IMAGE_EXT) and 'focus_camera' not in f)
            halves = {}      # --dpc: name of a derived tile's would-be file -> (left file, right file)
            if self.dpc:
                halves, lone = self._dpc_file_pairs(files)
                dpc_unpaired += lone
                files = sorted(files + list(halves))
            for file in files:
                parts = file.split('_', 3)
                region, fov, z_level = parts[0], int(parts[1]), int(parts[2])
                channel = os.path.splitext(parts[3])[0].replace("_", " ").replace("full ", "full_")
                pos = coords.get((region, fov, z_level))
                if pos is None:
                    print(f"Warning: {file} has no row in coordinates.csv, skipped")
                    continue
                key = (int(timepoint), region, fov, z_level, channel)
                rec = {'filepath': os.path.join(image_folder, halves[file][0] if file in halves else file),
                       'x': pos[0], 'y': pos[1], 'z': pos[2],
                       'channel': channel, 'z_level': z_level, 'region': region, 'fov_idx': fov, 't': int(timepoint)}
                if file in halves:      # a derived tile: both halves, at the place its own file would have
                    rec['filepath_right'] = os.path.join(image_folder, halves[file][1])
                    self.acquisition_metadata[key] = rec
                    self._region_index.setdefault((int(timepoint), region), {})[key] = rec
                    continue
                self.acquisition_metadata[key] = rec
                self._region_index.setdefault((int(timepoint), region), {})[key] = rec
                regions.add(region)
                channels.add(channel)
                max_z = max(max_z, z_level)
                max_fov = max(max_fov, fov)
        self.regions = sorted(regions)
        self.channel_names = sorted(channels)
        self.num_t = len(self.timepoints)
        self.num_z = max_z + 1
        self.num_fovs_per_region = max_fov + 1
        if not self.acquisition_metadata:
            raise ValueError(f"No image files with coordinates found under {self.input_folder}")
        if self.dpc:
            for half in self.dpc_channels:
                if half not in channels:
                    raise ValueError(f"dpc_channels: {half!r} is not a channel of this acquisition: {self.channel_names}")
            if dpc_unpaired:
                print(f"Warning: {dpc_unpaired} (fov, z) with only one of the halves {self.dpc_channels}: no "
                      f"{native.DPC_CHANNEL} tile there")
        first_key = next(iter(self.acquisition_metadata))
        first = self.acquisition_metadata[first_key]
        first_image = read_image(first['filepath'])
        self.dtype = first_image.dtype.type
        self._check_despeckle_dtype()
        if self.ome_tiff_compression == 'jpeg' and self._tiff_pyramid():
            ometiff.check_jpeg_dtype(self.dtype)
        if first_image.ndim in (2, 3):
            self.file_height, self.file_width = first_image.shape[:2]
            self.input_height, self.input_width = self.file_height, self.file_width
        else:
            raise ValueError(f"Unexpected image shape: {first_image.shape}")
        if self.tile_binning > 1:      # (refused here when K is larger than a side of the tiles)
            self.input_height, self.input_width = binning.binned_shape(self.file_height, self.file_width, self.tile_binning)
            print(f"[binning] {self.tile_binning} x {self.tile_binning} {self.tile_binning_method}: tiles of "
                  f"{self.file_height} x {self.file_width} stitched as {self.input_height} x {self.input_width} "
                  f"({self.file_height - self.tile_binning * self.input_height} rows, "
                  f"{self.file_width - self.tile_binning * self.input_width} columns dropped), pixel size "
                  f"{self.file_pixel_size_um} -> {self.pixel_size_um} um")
        if self.distortion_correction:
            du, dv = distortion.max_displacement(self.file_height, self.file_width, self.distortion_correction)
            print(f"[distortion] {self.distortion_correction} ppm: tiles of {self.file_height} x {self.file_width} corrected "
                  f"before anything else reads them, samples moved by up to {du / 256:.2f} px along x and {dv / 256:.2f} px "
                  f"along y (bilinear, 8 fractional bits, edges replicated)")
        self.chunks = (1, 1, 1, 512, 512)
        self.monochrome_channels = []
        # (the derived channel sits where its name sorts among the file channels; channel_names stays the file channels)
        for channel in sorted(self.channel_names + [native.DPC_CHANNEL]) if self.dpc else self.channel_names:
            if self.dpc and channel == native.DPC_CHANNEL:
                self.monochrome_channels.append(channel)
                continue
            ck = (first['t'], first['region'], first['fov_idx'], first['z_level'], channel)
            img = read_image(self.acquisition_metadata[ck]['filepath'])
            if img.ndim == 3 and img.shape[2] == 3:
                base = channel.split('_')[0]
                self.monochrome_channels.extend([f"{base}_R", f"{base}_G", f"{base}_B"])
            else:
                self.monochrome_channels.append(channel)
        self.num_c = len(self.monochrome_channels)
        self.monochrome_colors = [self.get_channel_color(n) for n in self.monochrome_channels]
        if self.dpc:
            for half in self.dpc_channels:
                if half not in self.monochrome_channels:
                    raise ValueError(f"dpc_channels: the files of {half!r} are RGB; the halves are monochrome channels")
            self._dpc_index = self.monochrome_channels.index(native.DPC_CHANNEL)
        if self.channel_shifts:
            self._resolve_channel_shifts()
        if self.channel_affines:
            self._resolve_channel_affines()
        if self.dark_frames or self.dark_pedestal:
            self._resolve_dark_frames()
        if self.focus_guide_channel is not None:
            if self.focus_guide_channel not in self.monochrome_channels:
                raise ValueError(f"focus_guide_channel {self.focus_guide_channel!r} is not a channel of this acquisition: "
                                 f"{self.monochrome_channels}")
            self._guide = self.monochrome_channels.index(self.focus_guide_channel)
        if self.composite:
            if self.composite_z is not None and not 0 <= self.composite_z < self.num_z:
                raise ValueError(f"composite_z = {self.composite_z} is outside the acquisition's z levels 0..{self.num_z - 1}")
            unknown = [n for n in (self.composite_channels or []) if n not in self.monochrome_channels]
            if unknown:
                raise ValueError(f"composite_channels {unknown} are not channels of this acquisition: {self.monochrome_channels}")
            if len(self.composite_channels or self.monochrome_channels) > composite_mod.MAX_CHANNELS:
                raise ValueError(f"a composite adds at most {composite_mod.MAX_CHANNELS} channels; name them with "
                                 f"composite_channels ({len(self.monochrome_channels)} in this acquisition)")
        print(f"[metadata] regions {self.regions}; channels {self.channel_names}")
        print(f"[metadata] tile {self.input_height} x {self.input_width} {np.dtype(self.dtype)}")
        print(f"[metadata] {self.num_z} z levels, {self.num_t} timepoints, {self.num_fovs_per_region} fovs per region")
        print(f"[metadata] {self.num_c} output channels: {self.monochrome_channels}")

    def _dpc_file_pairs(self, files):
        """--dpc: ({name the file of a derived tile would have: (left file, right file)}, number of (region, fov, z) with one
        half only) of one timepoint's file names.  A file that is already called like that makes 'DPC' a file channel."""
        left, right = {}, {}
        for file in files:
            parts = file.split('_', 3)
            stem, ext = os.path.splitext(parts[3])
            channel = stem.replace("_", " ").replace("full ", "full_")
            if channel == native.DPC_CHANNEL:
                raise ValueError(f"{file}: the acquisition already has a channel named {native.DPC_CHANNEL!r}, the name of "
                                 "the channel --dpc derives")
            for name, table in zip(self.dpc_channels, (left, right)):
                if channel == name:
                    table[tuple(parts[:3])] = (file, ext)
        pairs = {}
        for at, (file, ext) in left.items():
            if at in right:
                pairs['_'.join(at) + '_' + native.DPC_CHANNEL + ext] = (file, right[at][0])
        return pairs, len(set(left) ^ set(right))

    def get_region_data(self, t, region):
        """(stitcher.py:260-280) -- served from an index built once instead of a full scan."""
        data = self._region_index.get((int(t), region))
        if not data:
            raise ValueError(f"No data found for timepoint {int(t)}, region {region}")
        return data

    def get_channel_color(self, channel_name):
        """(stitcher.py:282-296)"""
        for key, color in (('405', 0x0000FF), ('488', 0x00FF00), ('561', 0xFFCF00), ('638', 0xFF0000),
                           ('730', 0x770000), ('_B', 0x0000FF), ('_G', 0x00FF00), ('_R', 0xFF0000)):
            if key in channel_name:
                return color
        return 0xFFFFFF

    def get_rows_and_columns(self):
        """(stitcher.py:1220-1223)"""
        return sorted(set(r[0] for r in self.regions)), sorted(set(r[1:] for r in self.regions))

    def _colour_planes(self, channel):
        """The output channels a file channel becomes: itself, or the three colour planes of an RGB file."""
        if channel in self.monochrome_channels:
            return [channel]
        base = channel.split('_')[0]
        return [f"{base}_{color}" for color in 'RGB']

    def _resolve_channel_shifts(self) -> None:
        """--channel-shift once the output channels are known: every name is one of them, none is the registration channel's
        (with registration on) or one --dpc reads or derives; the pairs by channel index, and the run's one printed line."""
        for name in self.channel_shifts:
            if name not in self.monochrome_channels:
                raise ValueError(f"channel_shifts: {name!r} is not a channel of this acquisition: {self.monochrome_channels}")
        if self.use_registration:
            # (the channel calculate_shifts will resolve to: the first one when none, or an unknown one, is named)
            reg = self.registration_channel if self.registration_channel in self.channel_names else self.channel_names[0]
            for name in self._colour_planes(reg):
                if name in self.channel_shifts:
                    raise ValueError(f"channel_shifts: {name!r} is the registration channel {reg!r}, the frame the other "
                                     f"channels are moved into: it takes no shift")
        if self.dpc:
            for name in (native.DPC_CHANNEL,) + tuple(self.dpc_channels):
                if name in self.channel_shifts:
                    raise ValueError(f"channel_shifts: {name!r} is a channel --dpc reads or derives; both halves come through "
                                     f"the same optics and take no shift")
        self._channel_shift_index = {self.monochrome_channels.index(name): pair for name, pair in self.channel_shifts.items()}
        print("[channel-shift] tiles of " + ", ".join(
            f"{name} sampled at (y {sy / 256:+.4f}, x {sx / 256:+.4f}) px" for name, (sy, sx) in sorted(self.channel_shifts.items()))
            + f" ({self.file_height} x {self.file_width}; bilinear, 8 fractional bits, edges replicated; after the distortion "
              f"correction, before the binning)")

    def _resolve_channel_affines(self) -> None:
        """--channel-affine once the output channels are known, under the refusals of --channel-shift: every name is an output
        channel, none is the registration channel's (with registration on) or one --dpc reads or derives; the coefficients by
        channel index, and the run's one printed line."""
        for name in self.channel_affines:
            if name not in self.monochrome_channels:
                raise ValueError(f"channel_affines: {name!r} is not a channel of this acquisition: {self.monochrome_channels}")
        if self.use_registration:
            reg = self.registration_channel if self.registration_channel in self.channel_names else self.channel_names[0]
            for name in self._colour_planes(reg):
                if name in self.channel_affines:
                    raise ValueError(f"channel_affines: {name!r} is the registration channel {reg!r}, the frame the other "
                                     f"channels are moved into: it takes no map")
        if self.dpc:
            for name in (native.DPC_CHANNEL,) + tuple(self.dpc_channels):
                if name in self.channel_affines:
                    raise ValueError(f"channel_affines: {name!r} is a channel --dpc reads or derives; both halves come through "
                                     f"the same optics and take no map")
        self._channel_affine_index = {self.monochrome_channels.index(name): a for name, a in self.channel_affines.items()}
        print("[channel-affine] tiles of " + ", ".join(
            f"{name} sampled at centre + (1 + 1e-6 [[{a[0]}, {a[1]}], [{a[2]}, {a[3]}]]) p" + (
                " + (y {:+.4f}, x {:+.4f}) px".format(*(v / 256 for v in self.channel_shifts[name]))
                if name in self.channel_shifts else "")
            for name, a in sorted(self.channel_affines.items()))
            + f" ({self.file_height} x {self.file_width}; bilinear, 8 fractional bits, edges replicated; after the distortion "
              f"correction, before the binning)")

    def _resolve_dark_frames(self) -> None:
        """--dark-frame once the output channels and the files' shape and dtype are known: every name is a file channel's (or
        '*'), every frame has exactly the files' shape and dtype, every constant and the pedestal lie in 0..M; the pairs by
        channel index, the distinct frames as one stack, and the run's one printed line."""
        pedestal = darkframe.check_pedestal(self.dark_pedestal, self.dtype)
        if not self.dark_frames:      # a pedestal alone: no channel has a frame it would be added back to
            return
        shape = (self.file_height, self.file_width)
        file_channels = [n for n in self.monochrome_channels if not (self.dpc and n == native.DPC_CHANNEL)]
        for name in self.dark_frames:
            if name == native.DPC_CHANNEL and name not in file_channels:
                raise ValueError(f"dark_frames: {name!r} is read from no file (--dpc derives it from its half-pupil channels, "
                                 f"which take their frames under their own names): it takes no frame")
            if name != darkframe.WILDCARD and name not in file_channels:
                raise ValueError(f"dark_frames: {name!r} is not a channel of this acquisition: {file_channels}")
        loaded = {name: darkframe.load_frame(source, shape, self.dtype, name) for name, source in self.dark_frames.items()}
        stack, digests, pairs = [], {}, {}
        for name in file_channels:
            key = name if name in loaded else (darkframe.WILDCARD if darkframe.WILDCARD in loaded else None)
            if key is None:
                continue
            frame = loaded[key]
            self._dark_note[name] = darkframe.frame_note(self.dark_frames[key], frame)
            if darkframe.is_identity(frame, pedestal):
                continue
            self._dark_host[name] = frame
            if isinstance(frame, int):
                pairs[name] = (-1, frame)
            else:
                digest = self._dark_note[name]['sha256']
                if digest not in digests:
                    digests[digest] = len(stack)
                    stack.append(frame)
                pairs[name] = (digests[digest], 0)
        self._dark_stack = np.stack(stack) if stack else None
        self._dark_params = {self.monochrome_channels.index(name): pair for name, pair in pairs.items()}
        if self.dpc:      # a derived plane is staged as its left half's file; the right halves have a buffer of their own
            left, right = self.dpc_channels
            if left in pairs:
                self._dark_params[self._dpc_index] = pairs[left]
            self._dark_right = pairs.get(right)
        print("[dark-frame] tiles of " + (", ".join(
            f"{name} minus " + (f"the constant {note['constant']}" if 'constant' in note else
                                f"{note['path'] or 'an array'} (min {note['min']}, max {note['max']}, mean {note['mean']})")
            for name, note in sorted(self._dark_note.items()))) +
            f" plus {pedestal}, clamped to 0..{int(np.iinfo(self.dtype).max)} ({shape[0]} x {shape[1]}; "
            f"{0 if self._dark_stack is None else len(self._dark_stack)} distinct frames on the device; before every other "
            f"per-tile step)")

    def _file_channel_dark(self, channel):
        """The frame of the files of ``channel`` -- for an RGB file a list of three -- or None when none of its planes has one."""
        if not self._dark_host or channel is None:
            return None
        frames = [self._dark_host.get(name) for name in self._colour_planes(channel)]
        if all(f is None for f in frames):
            return None
        return frames[0] if len(frames) == 1 else frames

    def _dark_frames_device(self):
        """The distinct frames [K, fh, fw] on the device, uploaded once and kept with the cached buffers (None without one)."""
        if self._dark_stack is None:
            return None
        import torch
        key = ('dark-frames',) + tuple(self._dark_stack.shape) + (self._dark_stack.dtype.str,)
        return self._cached_buffers(key, lambda: torch.from_numpy(self._dark_stack).to(self.device))

    def _file_channel_affine(self, channel):
        """(S, A) of the files of ``channel`` -- for an RGB file a triple each -- or None when none of its planes has a non-zero
        A (then ``_file_channel_shift`` says what happens to the file)."""
        if not self.channel_affines or channel is None:
            return None
        names = self._colour_planes(channel)
        coeffs = [self.channel_affines.get(name, channelaffine.ZERO) for name in names]
        if not any(a != channelaffine.ZERO for a in coeffs):
            return None
        pairs = [self.channel_shifts.get(name, (0, 0)) for name in names]
        return (pairs[0], coeffs[0]) if len(names) == 1 else (pairs, coeffs)

    def _file_channel_shift(self, channel):
        """(Sy, Sx) of the files of ``channel`` -- for an RGB file a triple each -- or None when none of its planes is shifted."""
        if not self.channel_shifts or channel is None:
            return None
        pairs = [self.channel_shifts.get(name, (0, 0)) for name in self._colour_planes(channel)]
        if not any(pair != (0, 0) for pair in pairs):
            return None
        return pairs[0] if len(pairs) == 1 else ([p[0] for p in pairs], [p[1] for p in pairs])

    def _read_tile_file(self, path, channel=None):
        """One tile file of ``channel`` as the run sees it: corrected (--distortion-correction) first, shifted (--channel-shift)
        or mapped (--channel-affine, with the shift in one map) second, binned (--tile-binning) third, on the host with the integer arithmetic of the device launches; the file itself
        without the options."""
        affine = self._file_channel_affine(channel)
        shift = self._file_channel_shift(channel) if affine is None else None
        dark = self._file_channel_dark(channel)
        if dark is not None:      # the sensor's own term first; everything behind it as without the option
            img = darkframe.dark_image(read_image(path), dark, self.dark_pedestal)
            img = distortion.warp_image(img, self.distortion_correction) if self.distortion_correction else img
        elif not self.distortion_correction and shift is None and affine is None:
            return binning.read_binned(path, self.tile_binning, self.tile_binning_method)
        else:
            img = distortion.read_warped(path, self.distortion_correction)
        if affine is not None:      # the shift and the linear term are one map
            img = channelaffine.affine_image(img, *affine)
        if shift is not None:
            img = channelshift.shift_image(img, *shift)
        return img if self.tile_binning == 1 else binning.bin_image(img, self.tile_binning, self.tile_binning_method)

    def get_tile(self, t, region, x, y, channel, z_level):
        """(stitcher.py:526-542) -> numpy image or None."""
        for value in self.get_region_data(int(t), str(region)).values():
            if value['x'] == x and value['y'] == y and value['channel'] == channel and value['z_level'] == z_level:
                try:
                    return self._read_tile_file(value['filepath'], channel)
                except FileNotFoundError:
                    print(f"Warning: cannot open {value['filepath']}")
                    return None
        print(f"Warning: region {region} has no tile at ({x}, {y}) mm for channel {channel}, z {z_level}")
        return None

    # ------------------------------------------------------------- geometry
    @property
    def _per_unit_registration(self) -> bool:
        """Every (timepoint, region) is registered on its own tiles before it is fused."""
        return self.per_region_registration or self.global_registration

    def _shifts(self) -> Shifts:
        rev = getattr(self, 'h_shift_rev', None) if self.scan_pattern == 'S-Pattern' else None
        return Shifts(tuple(self.h_shift), tuple(self.v_shift), None if rev is None else tuple(rev),
                      int(getattr(self, 'h_shift_rev_odd', 0)))

    def _apply_shifts(self, s: Optional[Shifts]) -> None:
        if s is None:
            return
        self.h_shift, self.v_shift = tuple(s.h_shift), tuple(s.v_shift)
        if s.h_shift_rev is not None:
            self.h_shift_rev, self.h_shift_rev_odd = tuple(s.h_shift_rev), s.h_shift_rev_odd

    def calculate_output_dimensions(self, timepoint, region):
        """(width_pixels, height_pixels); also sets x/y_positions and num_pyramid_levels
        (stitcher.py:298-354)."""
        region_data = self.get_region_data(int(timepoint), region)
        self.x_positions = sorted(set(v['x'] for v in region_data.values()))
        self.y_positions = sorted(set(v['y'] for v in region_data.values()))
        solved = self.placements.get((int(timepoint), region)) if self.global_registration else None
        if solved is not None:      # global registration: the canvas the solved positions span
            height_pixels, width_pixels = solved.canvas_hw
        else:
            width_pixels, height_pixels = placement.canvas_size(
                len(self.x_positions), len(self.y_positions), self.input_width, self.input_height,
                use_registration=self.use_registration, shifts=self._shifts(),
                xs=self.x_positions, ys=self.y_positions, pixel_size_um=self.pixel_size_um)
        max_dimension = 1
        if len(self.regions) > 1:
            rows, columns = self.get_rows_and_columns()
            max_dimension = max(len(rows), len(columns))
        self.num_pyramid_levels = placement.pyramid_levels(width_pixels, height_pixels, max_dimension)
        return width_pixels, height_pixels

    # ---------------------------------------------------------- registration
    def normalize_image(self, img):
        """(stitcher.py:613-617) on the device: full-tile min/max, then the float64 stretch and the
        truncating cast.  ``calculate_*_shift`` never call this: the registration kernels fuse the same
        arithmetic into their first pass."""
        import torch
        img = np.ascontiguousarray(img)
        if img.ndim != 2 or img.dtype not in (np.uint8, np.uint16):
            raise ValueError(f"normalize_image takes a 2-D uint8/uint16 image, got {img.dtype} {img.shape}")
        tiles = torch.from_numpy(img[None]).to(self.device)
        return native.normalize_tiles(tiles)[0].cpu().numpy()

    def _register_two(self, img_a, img_b, max_overlap, vertical: bool):
        import torch
        a, b = np.asarray(img_a), np.asarray(img_b)
        if a.ndim != 2 or b.ndim != 2 or a.shape != b.shape:
            raise ValueError("images must be same shape")
        tiles = torch.from_numpy(np.ascontiguousarray(np.stack([a, b]))).to(self.device)
        h, w = a.shape
        make = registration.vertical_pair if vertical else registration.horizontal_pair
        pair, n0, n1 = make(0, 1, h, w, int(max_overlap))
        s, _, _ = registration.register_pairs(tiles, np.array([pair], dtype=native.PAIR_DTYPE), n0, n1, 10,
                                              self.normalization)
        return s[0], n0, n1

    def calculate_horizontal_shift(self, img_left, img_right, max_overlap):
        """(stitcher.py:500-511) -> (dy, dx) python ints."""
        s, n0, n1 = self._register_two(img_left, img_right, max_overlap, vertical=False)
        return registration.horizontal_shift_from(s, n1)

    def calculate_vertical_shift(self, img_top, img_bot, max_overlap):
        """(stitcher.py:513-524)"""
        s, n0, n1 = self._register_two(img_top, img_bot, max_overlap, vertical=True)
        return registration.vertical_shift_from(s, n0)

    def calculate_shifts(self, t, region):
        """Centre-pair registration (stitcher.py:422-498); sets h_shift / v_shift
        [/ h_shift_rev / h_shift_rev_odd]."""
        region_data = self.get_region_data(t, region)
        x_positions = sorted(set(v['x'] for v in region_data.values()))
        y_positions = sorted(set(v['y'] for v in region_data.values()))
        self.h_shift = (0, 0)
        self.v_shift = (0, 0)
        self.placements.pop((int(t), region), None)
        self._global_rects.pop((int(t), region), None)
        if not self.registration_channel:
            self.registration_channel = self.channel_names[0]
        elif self.registration_channel not in self.channel_names:
            print(f"Warning: Specified registration channel '{self.registration_channel}' not found. "
                  f"Using {self.channel_names[0]}.")
            self.registration_channel = self.channel_names[0]
        self.calculate_output_dimensions(int(t), region)
        max_x_overlap, max_y_overlap = placement.registration_crop_widths(
            sorted(self.x_positions), sorted(self.y_positions), self.input_width, self.input_height,
            self.pixel_size_um, self.pixel_binning)
        print(f"[registration] crop widths from the stage pitch: {max_x_overlap} px horizontal, {max_y_overlap} px vertical")
        registration.check_crop_lengths(self.input_height, self.input_width, max_x_overlap, max_y_overlap)
        if self.global_registration:
            # --global-registration (an addition of this build): the all-pairs table with each pair's overlap ncc, its medians
            # as the reference's state, then every tile's own position from the global solve
            gtime = time.time()
            self._calculate_shifts_all_pairs(t, region, x_positions, y_positions, max_x_overlap, max_y_overlap, global_solve=True)
            print(f"[registration] all pairs: h_shift = {self.h_shift}, v_shift = {self.v_shift}")
            solved = self.placements.get((int(t), region))
            if solved is not None:
                print(solved.summary() + f" ({time.time() - gtime:.3f} s with the registration)")
            self.calculate_output_dimensions(int(t), region)
            return
        if self.all_pairs_registration:
            # --all-pairs-registration (an addition of this build; NOT the reference's --dynamic-registration, which it
            # parses and never reads): every adjacent pair of the registration plane, one batch per direction, per-axis
            # median of the integer shifts
            self._calculate_shifts_all_pairs(t, region, x_positions, y_positions, max_x_overlap, max_y_overlap)
            print(f"[registration] all pairs: h_shift = {self.h_shift}, v_shift = {self.v_shift}")
            return
        cx, cy = (len(x_positions) - 1) // 2, (len(y_positions) - 1) // 2
        center_x, center_y = x_positions[cx], y_positions[cy]
        right_x = bottom_y = None
        get = lambda x, y: self.get_tile(t, region, x, y, self.registration_channel, self.registration_z_level)
        if cx + 1 < len(x_positions):
            right_x = x_positions[cx + 1]
            a, b = get(center_x, center_y), get(right_x, center_y)
            if a is not None and b is not None:
                self.h_shift = self.calculate_horizontal_shift(a, b, max_x_overlap)
            else:
                print(f"Warning: region {region}: centre or right tile missing, h_shift stays {self.h_shift}")
        if cy + 1 < len(y_positions):
            bottom_y = y_positions[cy + 1]
            a, b = get(center_x, center_y), get(center_x, bottom_y)
            if a is not None and b is not None:
                self.v_shift = self.calculate_vertical_shift(a, b, max_y_overlap)
            else:
                print(f"Warning: region {region}: centre or bottom tile missing, v_shift stays {self.v_shift}")
        if self.scan_pattern == 'S-Pattern' and right_x and bottom_y:
            a, b = get(center_x, bottom_y), get(right_x, bottom_y)
            if a is not None and b is not None:
                self.h_shift_rev = self.calculate_horizontal_shift(a, b, max_x_overlap)
                self.h_shift_rev_odd = cy % 2 == 0
                print(f"[registration] reversed rows: h_shift_rev = {self.h_shift_rev}")
            else:
                print(f"Warning: region {region}: tiles of the reversed row missing, h_shift_rev stays {self.h_shift_rev}")
        print(f"[registration] h_shift = {self.h_shift}, v_shift = {self.v_shift}")

    def _calculate_shifts_all_pairs(self, t, region, xs, ys, max_x_overlap, max_y_overlap, global_solve: bool = False):
        """Extension: registration over ALL adjacent tile pairs of the registration plane (batched on the
        device), reduced to the reference's state (h_shift, v_shift[, h_shift_rev]) by a per-axis median --
        a single bad tile (dust, empty field) then cannot derail the whole mosaic.

        Under ``run()`` with several ranks (``self._pair_ranks`` = (rank, world)) the pairs are SHARDED: every rank
        takes one contiguous run of the pair list (tile-row order), reads and uploads only the tiles its pairs touch,
        and the [n_pairs, 3] float64 table {dy, dx, err} is all-gathered (registration.register_all_pairs_sharded);
        the medians are host arithmetic on that table, so every rank sets the same integers.

        ``global_solve`` (--global-registration): the table carries each pair's overlap ncc, and the unit's tile positions
        are solved from it (alignment.solve_positions; with the pairs sharded rank 0 solves and broadcasts the result) and
        kept in ``placements[(t, region)]``."""
        import torch
        n_rows, n_cols = len(ys), len(xs)
        at = {}
        for v in self.get_region_data(t, region).values():
            if v['channel'] == self.registration_channel and v['z_level'] == self.registration_z_level:
                at[(ys.index(v['y']), xs.index(v['x']))] = v['filepath']
        if not at:
            return
        rank, world = getattr(self, '_pair_ranks', None) or (0, 1)
        pairs = registration.grid_pair_list(n_rows, n_cols, present=at)

        def load_cells(cells):
            def one(cell):
                img = read_image(at[cell])
                return img if img.ndim == 2 else img[..., 0]
            with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 4)) as pool:
                images = list(pool.map(one, cells))
            stack = torch.from_numpy(np.ascontiguousarray(np.stack(images))).to(self.device)
            # the raw stack, corrected and binned by the launches the staged tiles go through; in front of them the registration
            # channel's dark frame (of an RGB file: its first colour plane's), in place over this fresh upload
            dark = self._dark_params.get(self.monochrome_channels.index(self._colour_planes(self.registration_channel)[0])) \
                if self._dark_params else None
            return warp_and_bin(stack, self.distortion_correction, self.tile_binning, self.tile_binning_method,
                                darks=dark, dark_frames=self._dark_frames_device() if dark is not None else None,
                                dark_pedestal=self.dark_pedestal)

        table = registration.register_all_pairs_sharded(
            pairs, load_cells, self.input_height, self.input_width, max_x_overlap, max_y_overlap, self.normalization,
            rank=rank, world=world, device=sharding.collective_device(self), with_overlap_ncc=global_solve)
        self.pair_table = table     # [n_pairs, {dy, dx, err[, ncc]}] float64, pair order = registration.grid_pair_list
        med = registration.pair_table_medians(pairs, table, self.input_height, self.input_width, max_x_overlap,
                                              max_y_overlap, n_rows, self.scan_pattern)
        for name, value in med.items():
            setattr(self, name, bool(value) if name == 'h_shift_rev_odd' else tuple(value))
        if not global_solve:
            return
        # the prior: where --all-pairs-registration places every cell of the region (any channel), on the medians' lattice
        cells = sorted({(ys.index(v['y']), xs.index(v['x'])) for v in self.get_region_data(t, region).values()})
        lattice = placement.grid_rects(n_rows, n_cols, self.input_width, self.input_height, self._shifts(), order=cells, crop=False)
        prior = {c: (int(r[4]), int(r[5])) for c, r in zip(cells, lattice)}
        solved = None
        if rank == 0:
            h_crop = placement.horizontal_crop_origins(self.input_height, self.input_width, int(max_x_overlap))[:2] \
                if any(p[0] == registration.PAIR_H for p in pairs) else (0, 0)
            v_crop = placement.vertical_crop_origins(self.input_height, self.input_width, int(max_y_overlap))[:2] \
                if any(p[0] == registration.PAIR_V for p in pairs) else (0, 0)
            solved = alignment.solve_positions(pairs, table, self.input_height, self.input_width, h_crop, v_crop, prior)
        if world > 1:
            solved = sharding.broadcast_object(solved)
        self.placements[(int(t), region)] = solved

    # -------------------------------------------------------------- flatfield
    def apply_flatfield_correction(self, tile, channel_idx):
        """(stitcher.py:607-611) on one host tile through the device kernel."""
        if channel_idx not in self.flatfields:
            return tile
        import torch
        tile = np.ascontiguousarray(tile)
        h, w = tile.shape
        plan = self._plan_for(np.array([(0, 0, h, w, 0, 0)]), h, w, h, w, native.SQ_FUSE_OVERWRITE)
        canvas = torch.empty((1, h, w), dtype=native.torch_dtype_of(tile.dtype), device=self.device)
        flat = torch.from_numpy(np.ascontiguousarray(self.flatfields[channel_idx])).to(self.device)
        native.fuse_planes(plan, torch.from_numpy(tile[None, None]).to(self.device), canvas, [flat])
        return canvas[0].cpu().numpy()

    def get_flatfields(self, progress_callback=None):
        """One gain image per monochrome channel from the reference's sample of tiles -- at most 32 randomly chosen
        per timepoint, stopping once more than 48 are collected (stitcher.py:365-419).

        The reference fits them with a third-party estimator, ``basicpy.BaSiC(get_darkfield=False,
        smoothness_flatfield=1).fit(images).flatfield`` (:374-377).  ``flatfield_estimator``:
          'auto'     basicpy when it is importable (then the very same call is made and the gains are the
                     reference's), else 'basic';
          'basic'    the device restatement of the published BaSiC fit (csrc/basic.hip, defined by
                     oracle/basic_oracle.py).  basicpy and jax are absent offline, so its parity with basicpy is
                     UNPINNED; it recovers planted gains (tests/test_basic_gpu.py);
          'basicpy'  basicpy or an ImportError;
          'mean'     mean of the sample, box-smoothed, mean 1: NOT BaSiC, only on explicit request.
        Which one ran is kept in ``flatfield_estimator_used`` and written to ``flatfield_info.json`` (and
        ``shift_table.json``) beside the output.  Either way the estimate is not on the hot path: the divide by the
        gains is (``apply_flatfield_correction``, in the fusion kernel).  Flatfields already assigned to
        ``self.flatfields`` are left untouched."""
        import torch
        want = self.flatfield_estimator
        BaSiC = None
        if want in ('auto', 'basicpy'):
            try:
                from basicpy import BaSiC
            except Exception:
                if want == 'basicpy':
                    raise ImportError("flatfield_estimator='basicpy' but basicpy cannot be imported")
        used = 'basicpy' if BaSiC is not None else ('mean' if want == 'mean' else 'basic')
        self.flatfield_estimator_used = used
        self.flatfield_info = {'estimator': used, 'channels': {}}
        if used == 'basic':
            print("[flatfield] BaSiC (LADMAP, no darkfield, smoothness 1) on the device: this build's restatement of the "
                  "published algorithm -- basicpy is not installed, parity with it is unpinned")
        elif used == 'mean':
            print("[flatfield] mean / box-smooth estimate on request: this is NOT the reference's BaSiC fit")

        def estimate(images: np.ndarray, channel_name: str):
            channel_index = self.monochrome_channels.index(channel_name)
            if channel_index in self.flatfields:
                return
            info = {}
            if used == 'basicpy':
                basic = BaSiC(get_darkfield=False, smoothness_flatfield=1)
                basic.fit(images)
                self.flatfields[channel_index] = np.asarray(basic.flatfield)
            elif used == 'basic':
                stack = torch.from_numpy(np.ascontiguousarray(images)).to(self.device)
                try:
                    flat, info = native.basic_fit(stack, 1.0)
                except native.NativeError as e:       # SQ_ERR_NUMERIC: the fit gave no finite, positive gains
                    raise native.NativeError(f"flatfield of channel {channel_name} ({len(images)} images): {e}", e.status) from e
                if info.get('capped_rounds', 0) > 0:
                    print(f"WARNING: flatfield of channel {channel_name}: {info['capped_rounds']} of "
                          f"{info['reweight_iterations']} re-weighting rounds of the BaSiC fit stopped at the iteration cap "
                          f"without settling (dim or few images?); the gains are finite and positive but may be poor")
                self.flatfields[channel_index] = flat.cpu().numpy()
            else:
                acc = images.astype(np.float64).mean(axis=0)
                k = max(1, min(acc.shape) // 16)
                csum = np.cumsum(np.cumsum(np.pad(acc, ((k, k), (k, k)), mode='edge'), 0), 1)
                csum = np.pad(csum, ((1, 0), (1, 0)))
                n = 2 * k + 1
                smooth = (csum[n:, n:] - csum[:-n, n:] - csum[n:, :-n] + csum[:-n, :-n]) / (n * n)
                self.flatfields[channel_index] = (smooth / smooth.mean()).astype(np.float32)
            self.flatfield_info['channels'][channel_name] = dict(info, images=int(len(images)))
            if progress_callback:
                progress_callback(channel_index + 1, self.num_c)

        for channel in self.channel_names:
            print(f"Calculating {channel} flatfield...")
            paths = []
            for t in self.timepoints:
                at_t = [v['filepath'] for k, v in self.acquisition_metadata.items()
                        if v['channel'] == channel and k[0] == int(t)]
                if not at_t:
                    print(f"WARNING: No images found for channel {channel} at timepoint {t}")
                    continue
                random.shuffle(at_t)
                paths.extend(at_t[:min(32, len(at_t))])
                if len(paths) > 48:
                    break
            if not paths:
                print(f"WARNING: No images found for channel {channel} across all timepoints")
                continue
            images = np.array([self._read_tile_file(p, channel) for p in paths])
            if images.ndim == 4 and images.shape[1] == 1:       # (N, 1, Y, X) page stacks
                images = images[:, 0]
            if images.ndim == 3:
                estimate(images, channel)
            elif images.ndim == 4 and images.shape[-1] == 3:    # RGB files: one gain image per colour
                base = channel.split('_')[0]
                for i, color in enumerate('RGB'):
                    estimate(np.ascontiguousarray(images[..., i]), f"{base}_{color}")
            else:
                raise ValueError(f"Unexpected number of dimensions in images array: {images.ndim}")

    # ----------------------------------------------------------------- fusion
    def _keep_buffers(self, key, bufs) -> None:
        """Remember staging / slot buffers for the next region of the same geometry (page-locking host
        memory is slow); one entry per kind, so a change of geometry releases the old ones."""
        for k in [k for k in self._buffer_cache if k[0] == key[0] and k != key]:
            del self._buffer_cache[k]
        self._buffer_cache[key] = bufs

    def _cached_buffers(self, key, make):
        """The buffers kept under ``key``, made by ``make()`` and kept when there are none."""
        bufs = self._buffer_cache.get(key)
        if bufs is None:
            bufs = make()
            self._keep_buffers(key, bufs)
        return bufs

    def _plan_for(self, rects, tile_h, tile_w, canvas_h, canvas_w, mode) -> native.FusePlan:
        rects = np.asarray(rects, dtype=np.int64).reshape(-1, 6)
        key = (rects.tobytes(), tile_h, tile_w, canvas_h, canvas_w, mode)
        plan = self._plan_cache.get(key)
        if plan is None:
            if len(self._plan_cache) > 16:
                self._plan_cache.clear()
            # a large overwrite plan has its work list produced on the device (native.FusePlan, csrc/plan_expand.hip):
            # the table is the host planner's byte for byte, 1.5 instead of 5.9 ms for a 32 x 32 grid
            plan = self._plan_cache[key] = native.FusePlan(rects, tile_h, tile_w, canvas_h, canvas_w, mode,
                                                           expand_on_device=len(rects) >= 64)
        return plan

    def _new_arena(self, need: int):
        """A DeviceArena of ``need`` bytes, or None when the canvas has to come from a plain allocation: the platform lacks
        virtual memory management (remembered), or the card cannot give the slices even after PyTorch's cached blocks have been
        handed back (this call only).  Anything else raises."""
        import torch
        for attempt in range(2):
            try:
                return native.DeviceArena(need, self.device)
            except native.NativeError as exc:
                if 'virtual memory management unsupported' in str(exc):
                    print(f"[canvas] no virtual memory management on this platform ({exc}); the canvas comes from a plain allocation")
                    self._arena_unsupported = True
                    return None
                if 'out of memory' not in str(exc).lower():
                    raise
                if attempt == 0:
                    torch.cuda.empty_cache()      # blocks PyTorch's allocator holds but nobody uses
                else:
                    print(f"[canvas] the card cannot give {need / 2**30:.1f} GiB of arena slices ({exc}); the canvas comes from a plain allocation")
        return None

    def _empty_canvas(self, n_planes, hc, wc, tdtype):
        """The canvas of ``stitch_planes`` ([n_planes, hc, wc], planes on 128-byte lines, never zero-filled: stitcher.py:356-362's
        da.zeros is written by the fusion kernel).  From ``canvas_arena_min_bytes`` up it is carved from a DeviceArena --
        physical slices classified by a probe and mapped round-robin over the card's memory classes, so the kernel's
        row-segment writes run at the spread-out rate (0.71 instead of 0.61-0.69 of the HBM peak on config 3, and the same
        on every box; csrc/arena.hip) -- created before the ingest buffers, while the card has memory to choose from, and
        reused for the next region once this region's canvas has been dropped."""
        need = native.canvas_bytes(n_planes, hc, wc, tdtype)
        if need < self.canvas_arena_min_bytes or self._arena_unsupported:
            return native.empty_canvas(n_planes, hc, wc, tdtype, self.device)
        busy = self._arena is not None and self._arena.in_use()      # a caller still holds the last canvas: leave it alone
        if self._arena is None or busy or self._arena.nbytes < need:
            if self._arena is not None and not busy:
                self._arena.close()
            self._arena = self._new_arena(need)
            if self._arena is None:
                return native.empty_canvas(n_planes, hc, wc, tdtype, self.device)
            self.canvas_arena_info = self._arena.info
            print(f"[canvas] arena of {self._arena.nbytes / 2**30:.1f} GiB over {self._arena.info['n_classes']} memory classes "
                  f"{self._arena.info['class_slices']} (slices of {self._arena.info['slice_bytes'] >> 20} MiB), "
                  f"{self._arena.info['create_ms']:.0f} ms")
        self._arena.reset()
        return native.empty_canvas(n_planes, hc, wc, tdtype, self.device, arena=self._arena)

    def _tile_rect(self, tile_info):
        """sq_rect of one file: placement (stitcher.py:656-679) + crop (:570-587)."""
        unit = (int(tile_info['t']), tile_info['region'])
        solved = self.placements.get(unit) if self.global_registration else None
        if solved is not None:      # global registration: the tile's own position, crops at the midpoints of solved overlaps
            rects = self._global_rects.get(unit)
            if rects is None:
                make = alignment.overwrite_rects if self.fusion_mode == 'overwrite' else alignment.full_rects
                rects = self._global_rects[unit] = make(solved, self.input_height, self.input_width)
            return rects[(self.y_positions.index(tile_info['y']), self.x_positions.index(tile_info['x']))]
        if self.use_registration:
            col = self.x_positions.index(tile_info['x'])
            row = self.y_positions.index(tile_info['y'])
            self.col_index, self.row_index = col, row
            return placement.registered_rect(row, col, len(self.y_positions), len(self.x_positions),
                                             self.input_width, self.input_height, self._shifts(),
                                             crop=self.fusion_mode == 'overwrite')
        return placement.coordinate_rect(tile_info['x'], tile_info['y'], min(self.x_positions), min(self.y_positions),
                                         self.input_width, self.input_height, self.pixel_size_um)

    def init_output(self, timepoint, region):
        """Device canvas (1, C, Z, Hc, Wc) (stitcher.py:356-362).  Not zero-filled: the fusion
        kernel writes every voxel, zeros included."""
        import torch
        width, height = self.calculate_output_dimensions(timepoint, region)
        shape = (1, self.num_c, self.num_z, height, width)
        print(f"region {region} timepoint {timepoint} output array dimensions: {shape}")
        return torch.empty(shape, dtype=native.torch_dtype_of(self.dtype), device=self.device)

    def stitch_region(self, timepoint, region, progress_callback=None, device_output: bool = False):
        """Fuse one (timepoint, region) -> 5-D TCZYX array of the input dtype
        (stitcher.py:639-689).  Returns numpy (host) unless ``device_output``."""
        # canvas slots z-major ("spread"): the z planes of a channel -- which share a gain image and go through the
        # fusion kernel together -- then lie num_c planes apart in the canvas allocation instead of side by side; a
        # group of planes writes fastest when they sit in different stretches of device memory (DESIGN.md 5.1 point 8)
        return self._stitch_region(timepoint, region, progress_callback, device_output)

    def _stitch_region(self, timepoint, region, progress_callback=None, device_output: bool = False, project_to=None,
                       composite=None):
        planes, _ = self.stitch_planes(timepoint, region, None, progress_callback, slot_order='spread', project_to=project_to)
        shape = (1, self.num_c, self.num_z, planes.shape[-2], planes.shape[-1])
        by_cz = planes.unflatten(0, (self.num_z, self.num_c)).transpose(0, 1)   # [C, Z, Hc, Wc] view of the [Z * C] slots
        if composite is not None:      # the resident canvas: the source planes are reduced before it leaves the device
            composite.add(by_cz[:, composite.z], [(0, c, composite.z) for c in range(self.num_c)])
        if device_output:       # a strided view: planes sit on 128-byte lines, rows are dense
            return by_cz.unsqueeze(0)
        import torch
        out = torch.empty(shape, dtype=planes.dtype)
        for c in range(self.num_c):
            for z in range(self.num_z):      # one D2H copy per plane (a strided .cpu() would first copy on the device)
                out[0, c, z].copy_(by_cz[c, z])
        return out.numpy()

    def project_region(self, timepoint, region, progress_callback=None, device_output: bool = False):
        """Maximum-intensity projection over z of one (timepoint, region) -> (1, C, 1, Hc, Wc) of the input dtype, equal to
        ``stitch_region(...).max(axis=2)`` bit for bit, without the stack ever existing: the tiles are staged as for
        ``stitch_region`` and every channel's z planes are reduced by one kernel (sq_fuse_project_max; an extension, the
        reference has no projection).  Returns numpy (host) unless ``device_output``."""
        proj = self._new_projection(timepoint, region)
        self.stitch_planes(timepoint, region, None, progress_callback, stack=False,
                           project_to={c: proj[c] for c in range(self.num_c)})
        out = proj.unsqueeze(0).unsqueeze(2)
        return out if device_output else out.cpu().numpy()

    def focus_region(self, timepoint, region, progress_callback=None, device_output: bool = False, return_depth: bool = False):
        """Best-focus (extended depth of field) projection over z of one (timepoint, region) -> (1, C, 1, Hc, Wc) of the input
        dtype: per voxel the value ``stitch_region`` stores in the z plane whose owner tile pixel has the highest focus score
        (the box sum of radius ``focus_radius`` of the raw tile's modified Laplacian; on a tie the lowest z), computed from the
        staged tiles without the stack (sq_fuse_project_focus; an extension, the reference has none).
        ``return_depth``: also the winning z level of every voxel, (C, Hc, Wc) int32, -1 where no tile covers it.
        Returns numpy (host) unless ``device_output``."""
        out, key, _, project_to = self._focus_target(timepoint, region)
        self.stitch_planes(timepoint, region, None, progress_callback, stack=False, project_to=project_to)
        import torch
        img = out.unsqueeze(0).unsqueeze(2)
        if not device_output:
            img = img.cpu().numpy()
        if not return_depth:
            return img
        depth = native.depth_of_keys(key).to(torch.int32)
        if self._guide is not None:      # one depth for all channels: the guide's
            depth = depth.expand(self.num_c, -1, -1)
        return img, (depth if device_output else depth.cpu().numpy())

    def _depth_dtype(self):
        return native.torch_dtype_of(native.depth_dtype_for(self.num_z))

    def _focus_target(self, timepoint, region, rows=None, channels=None, depth=None):
        """Device buffers and the stitch_planes ``project_to`` of the best-focus projection of ``channels`` (None = all) of a
        region (a row band's rows with ``rows``) -> (output [n, Hc, Wc], key [k, Hc, Wc] int64, depth [k, Hc, Wc] unsigned or
        None, project_to).  Without a guide channel every channel has its own key plane (k = n) and no depth plane is taken.
        With one, only the guide has a key plane (k = 1, or 0 when it is not among ``channels``) and the other channels
        follow ``depth`` [1, Hc, Wc]: the caller's, already filled, or a fresh one that stitch_planes derives from the guide's
        key plane -- the guide then has to be among ``channels``."""
        import torch
        chans = list(range(self.num_c)) if channels is None else [int(c) for c in channels]
        out = self._new_projection(timepoint, region, rows, len(chans))
        g = self._guide
        if g is None:
            key = torch.empty(tuple(out.shape), dtype=torch.int64, device=self.device)
            return out, key, None, {c: (out[i], key[i]) for i, c in enumerate(chans)}
        key = torch.empty((1 if g in chans else 0,) + tuple(out.shape[1:]), dtype=torch.int64, device=self.device)
        derive = depth is None
        if derive:
            if g not in chans and len(chans):
                raise ValueError("channels that follow the guide need its depth plane, or the guide among them")
            depth = torch.empty((1,) + tuple(out.shape[1:]), dtype=self._depth_dtype(), device=self.device)
        project_to = {}
        for i, c in enumerate(chans):
            project_to[c] = (out[i], key[0]) if c == g else FocusFollower(out[i], depth[0], g if derive else None)
        return out, key, depth, project_to

    def _new_focus(self, timepoint, region, rows=None, n_channels=None):
        """Device buffers (output [C, Hc, Wc] of the input dtype, key [C, Hc, Wc] int64) of a region's best-focus projections
        (a row band's rows with ``rows``)."""
        import torch
        out = self._new_projection(timepoint, region, rows, n_channels)
        return out, torch.empty(tuple(out.shape), dtype=torch.int64, device=self.device)

    def _new_projection(self, timepoint, region, rows=None, n_channels=None):
        """Device buffer [C, Hc, Wc] (or [n_channels, y1 - y0, Wc] for a row band) of a region's projections, rows dense."""
        import torch
        width, height = self.calculate_output_dimensions(timepoint, region)
        hc = height if rows is None else int(rows[1]) - int(rows[0])
        n = self.num_c if n_channels is None else int(n_channels)
        return torch.empty((n, hc, width), dtype=native.torch_dtype_of(self.dtype), device=self.device)

    def stitch_planes(self, timepoint, region, only_planes=None, progress_callback=None, stream_to=None, row_band=None,
                      slot_order: str = 'plane', project_to=None, stack: bool = True):
        """Fuse the (channel, z) planes ``only_planes`` (plane = channel * num_z + z; None = all) of one
        (timepoint, region) -> (device tensor [n, Hc, Wc], sorted plane ids).  Planes are independent,
        which is what lets several GPUs share one region.

        ``stream_to``: callable ``batch -> omezarr.PlaneStreamWriter``.  When given, no region-sized canvas
        is allocated: every batch of planes is fused into one of the writer's two slots and leaves
        for disk while the next batch is read and fused; the return value is (None, plane ids).

        ``row_band`` = (y0, y1): only these canvas rows of the planes (sharding.row_bands -- one plane shared by
        several GPUs); the canvas is then y1 - y0 rows high, tiles outside the band are not even read.

        ``slot_order``: 'plane' -- the returned tensor's i-th plane is the i-th plane id; 'spread' (all planes only) --
        plane c * num_z + z sits at slot z * num_c + c, so the planes of a channel are num_c slots apart.

        ``project_to``: {channel: device tensor [Hc, Wc]} (the band's rows with ``row_band``) that receives the channel's
        maximum-intensity projection over the z planes among ``only_planes`` (sq_fuse_project_max), computed from the same
        staged tiles as the stack: the first batch of a channel writes, later batches (and other rectangle lists) accumulate;
        a channel no file touches comes out as zeros.  A value (output [Hc, Wc], key [Hc, Wc] int64) receives the channel's
        best-focus projection and its key plane instead (sq_fuse_project_focus, radius ``self.focus_radius``; the windows
        are the full staged tiles, so a row band projects exactly the rows of the whole region's projection).  A
        ``FocusFollower`` value receives the channel's fused value at the guide channel's depth (sq_fuse_select_depth): the
        guide's planes are staged and projected first, over all rectangle lists, its depth plane is derived once
        (sq_focus_depth_plane), and only then are the followers' planes staged.
        ``stack=False``: the projection only -- no canvas, no stream writer, no stack fusion; the return value is then
        (None, plane ids)."""
        import torch
        start_time = time.time()
        region_data = self.get_region_data(int(timepoint), region)
        width, height = self.calculate_output_dimensions(timepoint, region)
        plane_ids = sorted(set(int(p) for p in only_planes)) if only_planes is not None \
            else list(range(self.num_c * self.num_z))
        if plane_ids and (plane_ids[0] < 0 or plane_ids[-1] >= self.num_c * self.num_z):
            raise ValueError(f"plane ids must lie in [0, {self.num_c * self.num_z})")
        slot_of = {p: i for i, p in enumerate(plane_ids)}
        if slot_order == 'spread':
            if only_planes is not None or stream_to is not None:
                raise ValueError("slot_order='spread' lays out ALL planes of a region in one canvas")
            slot_of = {p: (p % self.num_z) * self.num_c + p // self.num_z for p in plane_ids}
        elif slot_order != 'plane':
            raise ValueError(f"slot_order must be 'plane' or 'spread', got {slot_order!r}")
        print(f"region {region} timepoint {timepoint} output array dimensions: "
              f"{(1, self.num_c, self.num_z, height, width)}" + ("" if only_planes is None else f", planes {plane_ids}"))
        # dense rows like the reference's array, every plane on a 128-byte line (native.empty_canvas)
        y0, y1 = (0, height) if row_band is None else (int(row_band[0]), int(row_band[1]))
        if not (0 <= y0 < y1 <= height):
            raise ValueError(f"row band {row_band} outside the {height}-row canvas")
        hc, wc = y1 - y0, width
        if not stack and project_to is None:
            raise ValueError("stack=False leaves nothing to compute without project_to")
        if not stack:
            stream_to = None
        flat_canvas = None if (stream_to is not None or not stack) else \
            self._empty_canvas(len(plane_ids), hc, wc, native.torch_dtype_of(self.dtype))
        th, tw = self.input_height, self.input_width
        # --tile-binning: the files (and so the pinned staging and its device mirror) are fh x fw; everything behind the
        # binning launch is th x tw
        binned = self.tile_binning > 1
        fh, fw = (self.file_height, self.file_width) if binned else (th, tw)
        total_tiles = len(region_data)
        print(f"Beginning stitching of {total_tiles} tiles for region {region} timepoint {timepoint}")
        despeckle = self.despeckle != 'none'
        despeckle_counts = despeckle_staged = None
        self._write_option_notes(timepoint, region)
        # everything between a chunk's copy to the device and its fusion: what it allocates, costs and launches
        chain = TileChain(distortion_ppm=self.distortion_correction, binning=self.tile_binning,
                          binning_method=self.tile_binning_method,
                          dpc_planes=range(self._dpc_index * self.num_z, (self._dpc_index + 1) * self.num_z) if self.dpc else (),
                          dpc_gain=self.dpc_gain, despeckle=self.despeckle, despeckle_threshold=self.despeckle_threshold,
                          tophat_radius=self.background_radius if self.background_subtract == 'tophat' else None,
                          seam_qc_radius=self.seam_qc_radius, file_shape=(fh, fw), tile_shape=(th, tw), dtype=self.dtype,
                          channel_shifts=self._channel_shift_index, num_z=self.num_z,
                          channel_affines=self._channel_affine_index, dark_params=self._dark_params,
                          dark_frames=self._dark_frames_device() if self._dark_params or self._dark_right else None,
                          dark_pedestal=self.dark_pedestal, dark_derived=self._dark_right)

        # group the files by (channel, z) plane, keeping the reference's write order inside a plane
        planes: Dict[int, List[Tuple[dict, int, tuple]]] = {}
        for key, info in region_data.items():
            _, _, fov, z_level, channel = key
            rect = self._tile_rect(info)
            placement.check_rect_fits_like_numpy(rect, height, width)
            if row_band is not None:
                rect = placement.clip_rect_to_rows(rect, y0, y1)
                if rect is None:
                    continue
            if channel in self.monochrome_channels:
                targets = [(self.monochrome_channels.index(channel) * self.num_z + z_level, -1)]
            else:   # RGB file -> three monochrome channels (stitcher.py:551-556)
                base = channel.split('_')[0]
                targets = [(self.monochrome_channels.index(f"{base}_{color}") * self.num_z + z_level, i)
                           for i, color in enumerate('RGB')]
            for p, rgb in targets:
                if p in slot_of:
                    planes.setdefault(p, []).append((info, rgb, rect, fov))

        mode = native.SQ_FUSE_OVERWRITE if self.fusion_mode == 'overwrite' else native.SQ_FUSE_FEATHER
        # planes no file touches still have to come out as zeros
        empty = [p for p in plane_ids if p not in planes] if (stream_to is None and stack) else []   # streamed: fill_value
        if empty:
            zplan = self._plan_for(np.zeros((0, 6)), th, tw, hc, wc, native.SQ_FUSE_OVERWRITE)
            for p in empty:
                native.fuse_planes(zplan, torch.empty((1, 0, th, tw), dtype=flat_canvas.dtype, device=self.device),
                                   flat_canvas[slot_of[p]:slot_of[p] + 1])
        # run() streaming region after region: copies, fusion, pyramid and encoding of a region go to a stream of their own, so
        # that the NEXT region's registration -- it reads its shifts back, i.e. waits for the stream it runs on -- does not wait for
        # them (config 5: a (well, timepoint) unit is one batch; tools/cfg5_probe.py)
        side = None
        if stream_to is not None and self._defer_drain:
            if getattr(self, '_ingest_stream', None) is None:
                self._ingest_stream = torch.cuda.Stream(device=self.device)
            side = self._ingest_stream
            side.wait_stream(torch.cuda.current_stream(self.device))      # whatever the caller enqueued (flatfields, shifts) first
        stream_ctx = torch.cuda.stream(side) if side is not None else contextlib.nullcontext()

        # batch planes that share one rectangle list (normally: all of them)
        groups: Dict[bytes, List[int]] = {}
        rect_of: Dict[bytes, np.ndarray] = {}
        for p, items in planes.items():
            r = np.array([it[2] for it in items], dtype=np.int64).reshape(-1, 6)
            groups.setdefault(r.tobytes(), []).append(p)
            rect_of[r.tobytes()] = r
        # Ingest pipeline: file decode (host threads) -> pinned staging -> async H2D -> fusion, two slots
        # deep, so the files of batch k+1 are read while batch k is copied and fused.  A batch is a
        # few planes: bounded by free HBM, by host memory and by what is sensible to pin.
        free_bytes = torch.cuda.mem_get_info(self.device)[0]
        try:
            host_free = psutil.virtual_memory().available
        except Exception:   # pragma: no cover
            host_free = 8 << 30
        budget = max(1, min(int(free_bytes * 0.2), int(host_free * 0.1), int(self.batch_bytes_limit)))
        processed = 0
        projected = set()      # channels whose projection has been written once: later batches accumulate
        pool = ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 4))
        writer = None
        stream_ctx.__enter__()
        try:
            flats_dev = {}
            if self.apply_flatfield:
                for ci, ff in self.flatfields.items():
                    if binned and tuple(np.shape(ff)) != (th, tw):
                        raise ValueError(f"the flatfield of channel {ci} is {tuple(np.shape(ff))}: with tile_binning "
                                         f"{self.tile_binning} the gains divide the binned tiles of {(th, tw)}, not the files' "
                                         f"{(fh, fw)}")
                    flats_dev[ci] = torch.from_numpy(np.ascontiguousarray(ff)).to(self.device)
            if stream_to is not None and groups:
                widest = chain.writer_plane_bytes(max(len(rect_of[sig]) for sig in groups))      # of the longest list
                if self._tiff_pyramid() and self.ome_tiff_compression == 'jpeg':      # the encoder's packed streams, per slot
                    widest += ometiff.jpeg_buffers_plane_bytes(hc, wc, self.num_pyramid_levels,
                                                               (self.chunks or (1, 1, 1, 512, 512))[3:5])
                writer = stream_to(max(1, min(max(len(pl) for pl in groups.values()), budget // max(1, widest))))
            def parts_of(t):      # the tensors of a target that this call writes
                return t if isinstance(t, tuple) else ((t.out,) if isinstance(t, FocusFollower) else (t,))

            # the guide channel whose depth plane followers of this call wait for (FocusFollower.guide), if any
            followers = {c: t for c, t in (project_to or {}).items() if isinstance(t, FocusFollower)}
            guides = {t.guide for t in followers.values() if t.guide is not None}
            if len(guides) > 1 or any(not isinstance(project_to.get(g), tuple) for g in guides):
                raise ValueError("followers of one call share one guide channel, whose (output, key) target is in project_to")
            guide = guides.pop() if guides else None
            if project_to is not None:
                for t in project_to.values():
                    for u in parts_of(t) + ((t.depth,) if isinstance(t, FocusFollower) else ()):
                        u.record_stream(torch.cuda.current_stream(self.device))
                for c in project_to:
                    if not any(p // self.num_z == c for p in planes):
                        for u in parts_of(project_to[c]):
                            u.zero_()      # no file of this channel: zeros, like its planes of the stack
            # the passes over the rectangle lists: normally one per list.  With a guide channel: its planes first, over ALL lists;
            # then its depth plane; then the channels below and above it (a chunk never mixes the guide with another channel,
            # and never spans the gap it leaves: the stack pass keeps its evenly spaced canvas slots and single launch)
            work = []
            if guide is None:
                work = [(sig, sorted(plist)) for sig, plist in groups.items()]
            else:
                work = [(sig, sorted(p for p in plist if p // self.num_z == guide)) for sig, plist in groups.items()]
                work.append((None, None))
                work += [(sig, sorted(p for p in plist if p // self.num_z < guide)) for sig, plist in groups.items()]
                work += [(sig, sorted(p for p in plist if p // self.num_z > guide)) for sig, plist in groups.items()]
            for sig, plist in work:
                if sig is None:      # every plane of the guide has been projected: its depth plane, once, for all followers
                    depth_planes = {id(t.depth): t.depth for t in followers.values() if t.guide is not None}
                    for d in depth_planes.values():
                        native.focus_depth_plane(project_to[guide][1], out=d)
                    continue
                if not plist:
                    continue
                # ascending plane ids: the canvas slots of a chunk are then consecutive and the whole chunk
                # goes out in ONE launch (region_data is in file-name order, i.e. z varies before channel)
                rects = rect_of[sig]
                # (the winners' scratch is for the planes that are scored: a follower's batch does not pay for it)
                focus = project_to is not None and any(isinstance(project_to.get(p // self.num_z), tuple) for p in plist)
                n = len(rects)
                plan = self._plan_for(rects, th, tw, hc, wc, mode)
                # the best-focus projection's per-tile-pixel winners (5 B per tile pixel, one buffer for the group's calls)
                focus_scratch = torch.empty(native.focus_scratch_bytes(n, th, tw), dtype=torch.uint8, device=self.device) \
                    if focus else None
                staged_budget = budget - (0 if focus_scratch is None else focus_scratch.numel())
                # every buffer of the chain counts against the budget (TileChain.plane_bytes)
                derived_in_list = chain.derived(plist)
                batch = max(1, min(len(plist), staged_budget // max(1, chain.plane_bytes(n, bool(derived_in_list)))))
                if writer is not None:
                    batch = min(batch, writer.batch)
                chunks = [plist[b0:b0 + batch] for b0 in range(0, len(plist), batch)]
                # two slots also for a single chunk when run() streams region after region (config 5: a region is one chunk):
                # the next region's files are then read while this region's copy and fusion are still under way
                pipelined = writer is not None and self._defer_drain
                n_slots = 2 if (len(chunks) > 1 or pipelined) else 1
                # as deep as a chunk can hold derived planes (they are consecutive: plist is ascending)
                deep = min(batch, len(derived_in_list))
                bufs = chain.allocate(self._cached_buffers, self.device, batch, n, deep, n_slots)
                staging, on_dev, done, turn = bufs['ingest']
                # the right halves: one more staged buffer per ingest slot, with events of its own
                right_staging, _, right_done, _ = bufs.get('dpc', (None,) * 4)
                list_counts = None
                if despeckle:
                    if despeckle_counts is None:
                        despeckle_counts = torch.zeros(self.num_c, dtype=torch.int64, device=self.device)
                        despeckle_staged = [0] * self.num_c
                    # the kernel's per-plane counts of this list's planes (plane of plist, tile): every chunk adds into its own
                    # run of it, and it is folded per channel once, behind the last chunk
                    list_counts = torch.zeros((len(plist), n), dtype=torch.int64, device=self.device)
                qc_words = None
                if self.tile_qc:
                    # the words of this list's staged planes (plane of plist, tile): every chunk's launch overwrites its own run
                    # of them; they are read back with the despeckle counts, behind the call's synchronise
                    qc_words = torch.empty((len(plist), n, native.SQ_TILE_STATS_WORDS), dtype=torch.int64, device=self.device)
                    self._tile_qc_pending.append((timepoint, region, qc_words, [(p, it[3]) for p in plist for it in planes[p]]))
                seam_table = seam_words = None
                if self.seam_qc:
                    # the seams among this list's tiles and their words (plane of plist, seam): every chunk's launch overwrites
                    # its own run of them; they are read back with the tile-qc words, behind the call's synchronise
                    seam_table = self._seam_qc_table_of(sig, rects, [tuple(it[3] for it in planes[p]) for p in plist], th, tw)
                    if (int(timepoint), region) not in self._seam_qc_layouts:      # at the placement these launches see
                        self._seam_qc_layouts[(int(timepoint), region)] = self._seam_qc_layout(timepoint, region)
                    if seam_table is None:      # no seam among these tiles: the planes are still reported
                        self._seam_qc_pending.append((timepoint, region, None, list(plist), []))
                    else:
                        seam_words = torch.empty((len(plist), len(seam_table[1]), native.seam_words(self.seam_qc_radius)),
                                                 dtype=torch.int64, device=self.device)
                        self._seam_qc_pending.append((timepoint, region, seam_words, list(plist),
                                                      [(s['ref_fov'], s['mov_fov']) for s in seam_table[0]]))
                for k, chunk in enumerate(chunks):
                    b0 = k * batch      # the chunk is plist[b0:b0 + m]
                    slot = turn[0] % n_slots      # (the turn goes on across calls: the next region starts on the other slot)
                    turn[0] += 1
                    if done[slot] is not None:
                        done[slot].synchronize()      # the slot's previous copy and fusion have finished
                    host = staging[slot].numpy()
                    derived = chain.derived(chunk)      # (consecutive) -- and where their right halves go
                    right_host = None
                    if derived:
                        if right_done[slot] is not None:
                            right_done[slot].synchronize()
                        right_host = right_staging[slot].numpy()

                    def read_tile(path, rgb, dest):
                        if rgb < 0 and read_image_into(path, dest):
                            return      # file -> page-locked staging in one read
                        img = read_image(path)
                        if rgb >= 0:
                            img = img[:, :, rgb]
                        elif img.ndim == 3 and img.shape[0] == 1:
                            img = img[0]
                        if img.shape != (fh, fw):
                            raise ValueError(f"Unexpected tile shape: {img.shape}")
                        dest[...] = img

                    def load(job, host=host, right_host=right_host, first=derived[0] if derived else 0):
                        pi, ti, (info, rgb, _, _) = job
                        read_tile(info['filepath'], rgb, host[pi, ti])
                        if 'filepath_right' in info:      # a derived tile: its left half above, its right half here
                            read_tile(info['filepath_right'], -1, right_host[pi - first, ti])

                    jobs = [(pi, ti, it) for pi, p in enumerate(chunk) for ti, it in enumerate(planes[p])]
                    for _ in pool.map(load, jobs):
                        processed += 1
                        if progress_callback:
                            progress_callback(processed - 1, total_tiles)
                    m = len(chunk)
                    tiles = on_dev[slot][:m]
                    tiles.copy_(staging[slot][:m], non_blocking=True)
                    tiles = chain.run(tiles, slot, derived, b0, bufs, list_counts, qc_words, seam_table, seam_words, chunk)
                    flats = [flats_dev.get(p // self.num_z) for p in chunk] if self.apply_flatfield else None
                    slots = [slot_of[p] for p in chunk]
                    if project_to is not None:
                        # the channels' z planes among this chunk's staged tiles -> their projections (consecutive plane ids)
                        runs: Dict[int, List[int]] = {}
                        for pi, p in enumerate(chunk):
                            if p // self.num_z in project_to:
                                runs.setdefault(p // self.num_z, []).append(pi)
                        for c, pis in runs.items():
                            i0, i1 = pis[0], pis[-1] + 1
                            ff = None if flats is None else flats[i0:i1]
                            if isinstance(project_to[c], FocusFollower):
                                native.fuse_select_depth(plan, tiles[i0:i1], project_to[c].out, project_to[c].depth,
                                                         [p % self.num_z for p in chunk[i0:i1]], ff, accumulate=c in projected)
                            elif isinstance(project_to[c], tuple):
                                out, key = project_to[c]
                                native.fuse_project_focus(plan, tiles[i0:i1], out, key, [p % self.num_z for p in chunk[i0:i1]],
                                                          self.focus_radius, ff, scratch=focus_scratch,
                                                          accumulate=c in projected)
                            else:
                                native.fuse_project_max(plan, tiles[i0:i1], project_to[c], ff, accumulate=c in projected)
                            projected.add(c)
                    if not stack:      # the projection only
                        pass
                    elif writer is not None:
                        native.fuse_planes(plan, tiles, writer.acquire(m), flats)
                        writer.submit([(0, p // self.num_z, p % self.num_z) for p in chunk])
                    elif m == 1 or (slots[1] > slots[0] and all(slots[i + 1] - slots[i] == slots[1] - slots[0] for i in range(m - 1))):
                        # the chunk's canvas slots are evenly spaced (side by side, or num_c apart with slot_order
                        # 'spread'): ONE launch on the strided view
                        step = slots[1] - slots[0] if m > 1 else 1
                        native.fuse_planes(plan, tiles, flat_canvas[slots[0]:slots[0] + (m - 1) * step + 1:step], flats)
                    else:
                        for pi, sl in enumerate(slots):
                            native.fuse_planes(plan, tiles[pi:pi + 1], flat_canvas[sl:sl + 1],
                                               None if flats is None else flats[pi:pi + 1])
                    done[slot] = torch.cuda.Event()
                    done[slot].record()
                if despeckle:      # folded per channel on the device: nothing is read back here
                    of_channel: Dict[int, List[int]] = {}
                    for pi, p in enumerate(plist):
                        of_channel.setdefault(p // self.num_z, []).append(pi)
                    for c, pis in of_channel.items():      # (consecutive: plist is in ascending plane order)
                        despeckle_counts[c] += list_counts[pis[0]:pis[-1] + 1].sum()
                        despeckle_staged[c] += len(pis) * n * th * tw
        finally:
            stream_ctx.__exit__(None, None, None)
            if side is not None and project_to is not None:
                torch.cuda.current_stream(self.device).wait_stream(side)      # whatever reads the projections: after its kernels
            pool.shutdown(wait=True)
            if writer is not None and not self._defer_drain:
                writer.drain()      # everything of this region is on disk when the call returns (run() defers it to its end)
        if despeckle_counts is not None:
            self._despeckle_pending.append((timepoint, region, despeckle_counts, despeckle_staged))
        if not (writer is not None and self._defer_drain):      # (run(): the writer's events order everything; it is drained at the end)
            torch.cuda.synchronize(self.device)
            self._finish_despeckle()
            self._finish_tile_qc()
            self._finish_seam_qc()
        print(f"Time to stitch region {region} timepoint {timepoint}: {time.time() - start_time}")
        return flat_canvas, plane_ids

    def _write_note(self, timepoint, region, suffix, note) -> None:
        """``<t>_stitched/<region>_stitched_<suffix>.json``: the same bytes from every rank and call, put in place atomically."""
        folder = os.path.join(self.output_folder, f"{timepoint}_stitched")
        os.makedirs(folder, exist_ok=True)
        path = os.path.join(folder, f"{region}_stitched_{suffix}.json")
        tmp = f"{path}.{os.getpid()}.tmp"
        with open(tmp, 'w') as fh:
            json.dump(note, fh, indent=1)
        os.replace(tmp, path)

    def _write_option_notes(self, timepoint, region) -> None:
        """One note per per-tile option that is on: what was done to the tiles of every store of this region -- the static
        facts only (the despeckle's counts are in ``despeckle_replaced``)."""
        if self.distortion_correction != 0:
            du, dv = distortion.max_displacement(self.file_height, self.file_width, self.distortion_correction)
            self._write_note(timepoint, region, 'distortion', {
                'ppm': self.distortion_correction, 'tile_shape': [self.file_height, self.file_width],
                'max_abs_du_256': du, 'max_abs_dv_256': dv, 'edges': 'replicated',
                'interpolation': 'bilinear, 8 fractional bits',
                'applies_to': 'every tile, before binning, placement, registration, the flatfield estimate and every tile filter'})
        if self.dark_frames:
            self._write_note(timepoint, region, 'dark_frame', {
                'channels': {name: note for name, note in sorted(self._dark_note.items())},
                'pedestal': self.dark_pedestal, 'definition': native.DARK_DEFINITION,
                'tile_shape': [self.file_height, self.file_width],
                'device_frames': 0 if self._dark_stack is None else len(self._dark_stack),
                'device_frame_bytes': 0 if self._dark_stack is None else int(self._dark_stack.nbytes),
                'order': darkframe.ORDER,
                'applies_to': 'every tile file of the named channels, before registration, the flatfield estimate, the tile '
                              'report and every tile filter'})
        if self._channel_shift_index:
            self._write_note(timepoint, region, 'channel_shift', {
                'channels': {name: {'shift_256': [sy, sx], 'shift_px': [sy / 256, sx / 256]}
                             for name, (sy, sx) in sorted(self.channel_shifts.items())},
                'definition': 'the output at (y, x) takes the input at (y + Sy/256, x + Sx/256)',
                'tile_shape': [self.file_height, self.file_width], 'edges': 'replicated',
                'interpolation': 'bilinear, 8 fractional bits',
                'order': 'after the distortion correction, before the binning',
                'applies_to': 'every tile of the named channels, before placement, the flatfield estimate and every tile filter'})
        if self._channel_affine_index:
            fh, fw = self.file_height, self.file_width
            channels = {}
            for name, a in sorted(self.channel_affines.items()):
                sy, sx = self.channel_shifts.get(name, (0, 0))
                dv, du = channelaffine.max_displacement(fh, fw, (sy, sx), a)
                channels[name] = {'affine_ppm': list(a), 'shift_256': [sy, sx], 'max_abs_dv_256': dv, 'max_abs_du_256': du}
            self._write_note(timepoint, region, 'channel_affine', {
                'channels': channels,
                'definition': 'the output at centre + p takes the input at centre + (1 + A 1e-6) p + S/256, '
                              'A = [[Ayy, Ayx], [Axy, Axx]] in parts per million, p = (y, x)',
                'tile_shape': [fh, fw], 'edges': 'replicated', 'interpolation': 'bilinear, 8 fractional bits',
                'order': 'after the distortion correction, before the binning; one map with the channel shift',
                'applies_to': 'every tile of the named channels, before placement, the flatfield estimate and every tile filter'})
        if self.tile_binning > 1:
            k = self.tile_binning
            self._write_note(timepoint, region, 'binning', {
                'factor': k, 'method': self.tile_binning_method,
                'file_tile_shape': [self.file_height, self.file_width],
                'binned_tile_shape': [self.input_height, self.input_width],
                'rows_dropped': self.file_height - k * self.input_height,
                'columns_dropped': self.file_width - k * self.input_width,
                'file_pixel_size_um': self.file_pixel_size_um, 'pixel_size_um': self.pixel_size_um,
                'applies_to': 'every tile, before placement, registration, the flatfield estimate and every tile filter'})
        if self.background_subtract == 'tophat':
            self._write_note(timepoint, region, 'background', {
                'method': 'tophat', 'radius': self.background_radius, 'window': 2 * self.background_radius + 1,
                'applies_to': 'every staged tile plane, before the flatfield divide'})
        if self.despeckle != 'none':
            self._check_despeckle_dtype()
            self._write_note(timepoint, region, 'despeckle', {
                'mode': self.despeckle, 'threshold': self.despeckle_threshold, 'window': 3,
                'applies_to': 'every staged tile plane, before background removal and the flatfield divide'})
        if self.dpc:
            self._write_note(timepoint, region, 'dpc', {
                'left': self.dpc_channels[0], 'right': self.dpc_channels[1], 'gain': self.dpc_gain,
                'channel': native.DPC_CHANNEL, 'definition': native.DPC_DEFINITION})

    def _check_despeckle_dtype(self) -> None:
        """A threshold at or above the dtype's maximum can never fire (the default on uint8 data): a message, not a silent
        no-op."""
        if self.despeckle != 'none' and self.despeckle_threshold >= int(np.iinfo(self.dtype).max):
            raise ValueError(f"despeckle_threshold {self.despeckle_threshold} can never fire on {np.dtype(self.dtype).name} tiles "
                             f"(maximum {int(np.iinfo(self.dtype).max)}): give a threshold in counts of the tiles' own dtype")

    def _finish_despeckle(self) -> None:
        """Read the pending per-channel counts back (the device has been synchronised: stitch_planes' own synchronise, or the
        writer's final drain in run()), add them to ``despeckle_replaced`` / ``despeckle_staged`` and print them."""
        pending, self._despeckle_pending = self._despeckle_pending, []
        regions: Dict[tuple, list] = {}      # one line per (timepoint, region), whatever number of calls fused it
        for timepoint, region, counts, staged in pending:
            entry = regions.setdefault((timepoint, region), [np.zeros(self.num_c, np.int64), np.zeros(self.num_c, np.int64)])
            entry[0] += counts.cpu().numpy()
            entry[1] += np.asarray(staged, dtype=np.int64)
        for (timepoint, region), (host, staged) in regions.items():
            parts = []
            for c, name in enumerate(self.monochrome_channels):
                if staged[c]:
                    self.despeckle_replaced[name] = self.despeckle_replaced.get(name, 0) + int(host[c])
                    self.despeckle_staged[name] = self.despeckle_staged.get(name, 0) + int(staged[c])
                    parts.append(f"{name}: {int(host[c])} of {int(staged[c])}")
            print(f"[despeckle] region {region} timepoint {timepoint}: staged pixels replaced ({self.despeckle}, threshold "
                  f"{self.despeckle_threshold}) -- " + ", ".join(parts))

    # ------------------------------------------------------------------ tile quality report
    def _finish_tile_qc(self) -> None:
        """Read the pending words back (the device has been synchronised, as for _finish_despeckle), keep them per (timepoint,
        region) -- a tile staged more than once (row bands, several calls) gives the same words and is kept once -- and write
        the report of every region that got new words, from all the words it has so far.  A region the ranks share is written
        by _finish_tile_qc_shared instead."""
        pending, self._tile_qc_pending = self._tile_qc_pending, []
        touched = []
        for timepoint, region, words, keys in pending:
            host = words.cpu().numpy().reshape(-1, native.SQ_TILE_STATS_WORDS)
            have = self._tile_qc_words.setdefault((int(timepoint), region), {})
            for key, row in zip(keys, host):
                row = tuple(int(v) for v in row)
                if have.setdefault(key, row) != row:
                    raise RuntimeError(f"tile-qc: plane {key[0]}, fov {key[1]} of region {region} was staged twice with different words")
            if (int(timepoint), region) not in touched:
                touched.append((int(timepoint), region))
        if not self._tile_qc_shared:
            for timepoint, region in touched:
                self._write_tile_qc(timepoint, region)

    def _write_tile_qc(self, timepoint, region) -> None:
        """The rows of (timepoint, region) from its words, sorted by (output channel, z, fov), into tile_qc_table and the two
        files under <t>_stitched/; one printed line with the flag counts."""
        words = self._tile_qc_words.get((int(timepoint), region), {})
        th, tw = self.input_height, self.input_width
        rows = [tileqc.make_row(region, fov, p % self.num_z, self.monochrome_channels[p // self.num_z], words[(p, fov)], th, tw)
                for p, fov in sorted(words)]
        tileqc.flag_rows(rows, self.tile_qc_saturation, self.tile_qc_focus_ratio)
        self.tile_qc_table[(int(timepoint), region)] = rows
        note = tileqc.write_report(os.path.join(self.output_folder, f"{timepoint}_stitched"), region, rows,
                                   self.monochrome_channels, self.tile_qc_saturation, self.tile_qc_focus_ratio)
        print(f"[tile-qc] region {region} timepoint {timepoint}: {len(rows)} tile planes -- " +
              ", ".join(f"{k}: {v}" for k, v in note['flag_counts'].items()))

    def _finish_tile_qc_shared(self, timepoint, region, rank) -> None:
        """A region the ranks share by planes or bands: every rank's words go into the region's dense table [num_c * num_z,
        n_fov, 9] -- the eight words and a 'present' word, the min as dtype_max - min, absent entries all zero -- which is
        combined with ONE element-wise MAX all-reduce (an entry is absent or identical on every rank that has it, so MAX is
        exact); rank 0 writes the files."""
        import torch
        import torch.distributed as dist
        torch.cuda.synchronize(self.device)
        self._finish_tile_qc()
        top = int(np.iinfo(self.dtype).max)
        dense = np.zeros((self.num_c * self.num_z, self.num_fovs_per_region, native.SQ_TILE_STATS_WORDS + 1), dtype=np.int64)
        for (p, fov), w in self._tile_qc_words.get((int(timepoint), region), {}).items():
            dense[p, fov, :native.SQ_TILE_STATS_WORDS] = w
            dense[p, fov, 0] = top - w[0]
            dense[p, fov, native.SQ_TILE_STATS_WORDS] = 1
        table = torch.from_numpy(dense)
        coll = sharding.collective_device(self)
        if coll is not None:
            table = table.to(coll)
        dist.all_reduce(table, op=dist.ReduceOp.MAX)
        if rank == 0:
            dense = table.cpu().numpy()
            words = {}
            for p, fov in zip(*np.nonzero(dense[:, :, native.SQ_TILE_STATS_WORDS])):
                w = [int(v) for v in dense[p, fov, :native.SQ_TILE_STATS_WORDS]]
                w[0] = top - w[0]
                words[(int(p), int(fov))] = tuple(w)
            self._tile_qc_words[(int(timepoint), region)] = words
            self._write_tile_qc(timepoint, region)

    # ------------------------------------------------------------------ seam alignment report
    def _seam_qc_table_of(self, sig, rects, fov_lists, th, tw):
        """(seams, host pair table, device pair table) of the rectangle list ``rects`` whose i-th tile is fov ``fovs[i]`` --
        the seams both of whose tiles are in the list -- cached per list; None when the list holds no seam."""
        fovs = fov_lists[0]
        if any(f != fovs for f in fov_lists[1:]):
            raise RuntimeError("seam-qc: planes that share one rectangle list name different fovs")
        key = (sig, fovs, th, tw, self.seam_qc_radius, self.seam_qc_min_pixels)
        if key not in self._seam_qc_tables:
            seams = seamqc.region_seams({f: rects[i] for i, f in enumerate(fovs)}, th, tw, self.seam_qc_radius,
                                        self.seam_qc_min_pixels)
            entry = None
            if seams:
                table = native.as_overlaps(seamqc.pair_table(seams, {f: i for i, f in enumerate(fovs)}))
                entry = (seams, table, native.seam_pairs_to_device(table, self.device))
            if len(self._seam_qc_tables) >= 64:
                self._seam_qc_tables.clear()
            self._seam_qc_tables[key] = entry
        return self._seam_qc_tables[key]

    def _finish_seam_qc(self) -> None:
        """Read the pending words back (the device has been synchronised, as for _finish_tile_qc), keep them per (timepoint,
        region) -- a seam measured more than once (row bands, several calls) must give the same words and is kept once -- and
        write the report of every region that got new words, from all the words it has so far.  A region the ranks share is
        written by _finish_seam_qc_shared instead."""
        pending, self._seam_qc_pending = self._seam_qc_pending, []
        touched = []
        for timepoint, region, words, plist, keys in pending:
            have = self._seam_qc_words.setdefault((int(timepoint), region), {})
            self._seam_qc_planes.setdefault((int(timepoint), region), set()).update(int(p) for p in plist)
            host = words.cpu().numpy() if words is not None else None
            for pi, p in enumerate(plist):
                for (ref, mov), row in zip(keys, host[pi] if keys else ()):
                    row = tuple(int(v) for v in row)
                    if have.setdefault((int(p), ref, mov), row) != row:
                        raise RuntimeError(f"seam-qc: the seam of fovs {ref} and {mov} in plane {p} of region {region} was "
                                           "measured twice with different words")
            if (int(timepoint), region) not in touched:
                touched.append((int(timepoint), region))
        if not self._seam_qc_shared:
            for timepoint, region in touched:
                self._write_seam_qc(timepoint, region)

    def _seam_qc_layout(self, timepoint, region):
        """(seams of the whole region, {plane: the fovs that have a file of it}) from the region's files and rectangles."""
        rects, fovs_of = {}, {}
        for key, info in self.get_region_data(int(timepoint), region).items():
            _, _, fov, z_level, channel = key
            rects.setdefault(int(fov), self._tile_rect(info))
            if channel in self.monochrome_channels:
                ids = [self.monochrome_channels.index(channel) * self.num_z + z_level]
            else:
                base = channel.split('_')[0]
                ids = [self.monochrome_channels.index(f"{base}_{color}") * self.num_z + z_level for color in 'RGB']
            for p in ids:
                fovs_of.setdefault(p, set()).add(int(fov))
        seams = seamqc.region_seams(rects, self.input_height, self.input_width, self.seam_qc_radius, self.seam_qc_min_pixels)
        return seams, fovs_of

    def _write_seam_qc(self, timepoint, region) -> None:
        """The rows of (timepoint, region) -- for every plane that has words, the region's seams both of whose files exist,
        sorted by (output channel, z, ref fov, mov fov); a seam without words is 'unmeasured' -- into seam_qc_table and the two
        files under <t>_stitched/; one printed line with the flag counts."""
        words = self._seam_qc_words.get((int(timepoint), region), {})
        seams, fovs_of = self._seam_qc_layouts.get((int(timepoint), region)) or self._seam_qc_layout(timepoint, region)
        rows = []
        for p in sorted(self._seam_qc_planes.get((int(timepoint), region), ())):
            have = fovs_of.get(p, ())
            for s in seams:
                if s['ref_fov'] in have and s['mov_fov'] in have:
                    rows.append(seamqc.make_row(region, self.monochrome_channels[p // self.num_z], p % self.num_z, s,
                                                words.get((p, s['ref_fov'], s['mov_fov'])), self.seam_qc_radius))
        seamqc.flag_rows(rows, self.seam_qc_min_ncc)
        self.seam_qc_table[(int(timepoint), region)] = rows
        note = seamqc.write_report(os.path.join(self.output_folder, f"{timepoint}_stitched"), region, rows,
                                   self.monochrome_channels, self.seam_qc_radius, self.seam_qc_min_pixels, self.seam_qc_min_ncc)
        print(f"[seam-qc] region {region} timepoint {timepoint}: {len(rows)} seams of planes -- " +
              ", ".join(f"{k}: {v}" for k, v in note['flag_counts'].items()))

    def _finish_seam_qc_shared(self, timepoint, region, rank) -> None:
        """A region the ranks share by planes or bands: every rank's words go into the region's dense table [num_c * num_z,
        seams of the region, words + 1] -- the words and a 'present' word, absent entries all zero -- which is combined with
        ONE element-wise MAX all-reduce (every word is >= 0, and an entry is absent or identical on every rank that has it, so
        MAX is exact); rank 0 writes the files."""
        import torch
        import torch.distributed as dist
        torch.cuda.synchronize(self.device)
        self._finish_seam_qc()
        seams, fovs_of = self._seam_qc_layouts.get((int(timepoint), region)) or self._seam_qc_layout(timepoint, region)
        index = {(s['ref_fov'], s['mov_fov']): i for i, s in enumerate(seams)}
        nw = native.seam_words(self.seam_qc_radius)
        dense = np.zeros((self.num_c * self.num_z, len(seams), nw + 1), dtype=np.int64)
        for (p, ref, mov), w in self._seam_qc_words.get((int(timepoint), region), {}).items():
            dense[p, index[(ref, mov)], :nw] = w
            dense[p, index[(ref, mov)], nw] = 1
        table = torch.from_numpy(dense)
        coll = sharding.collective_device(self)
        if coll is not None:
            table = table.to(coll)
        dist.all_reduce(table, op=dist.ReduceOp.MAX)
        if rank == 0:
            dense = table.cpu().numpy()
            words = {}
            for p, i in zip(*np.nonzero(dense[:, :, nw])):
                words[(int(p), seams[i]['ref_fov'], seams[i]['mov_fov'])] = tuple(int(v) for v in dense[p, i, :nw])
            self._seam_qc_words[(int(timepoint), region)] = words
            self._seam_qc_planes[(int(timepoint), region)] = set(fovs_of)      # the ranks staged every plane between them
            self._write_seam_qc(timepoint, region)

    # ------------------------------------------------------------------ output
    # ------------------------------------------------------------------ contrast windows
    def _new_histogram(self):
        """A zeroed histogram target for one store ([C, bins] int64 on the device), or None with contrast_limits='dtype'."""
        if self.contrast_limits != 'percentile':
            return None
        import torch
        return torch.zeros((self.num_c, native.histogram_bins(self.dtype)), dtype=torch.int64, device=self.device)

    def _write_contrast(self, path: str, hist, shared: bool = False) -> None:
        """Windows and sidecars of the store ``path`` from the counts of what was submitted to it.  Reading ``hist`` back waits
        for the stream the histograms were launched on, not for the writer's chunk pipeline.  ``shared``: the ranks of a shared
        region each hold the counts of what they wrote; they are summed (every rank takes part) and rank 0 writes."""
        if hist is None:
            return
        side = getattr(self, '_ingest_stream', None)
        if side is not None:      # run() fuses (and counts) on a stream of its own
            import torch
            torch.cuda.current_stream(self.device).wait_stream(side)
        rank = 0
        if shared:
            import torch.distributed as dist
            rank = dist.get_rank()
            if dist.get_backend() != 'nccl':
                host = hist.cpu()
                dist.all_reduce(host, op=dist.ReduceOp.SUM)
                hist = host
            else:
                dist.all_reduce(hist, op=dist.ReduceOp.SUM)
        if rank == 0:
            lo, hi = self.contrast_percentiles
            omezarr.write_contrast(path, hist.cpu().numpy(), lo, hi, self.dtype)

    def _finish_contrast(self, wait: bool) -> None:
        """Windows and sidecars of the streamed stores whose counts have reached the host (``wait``: of all of them)."""
        while self._contrast_pending and (wait or self._contrast_pending[0][2].query()):
            path, host, event, _ = self._contrast_pending.pop(0)
            event.synchronize()
            lo, hi = self.contrast_percentiles
            omezarr.write_contrast(path, host.numpy(), lo, hi, self.dtype)

    # ------------------------------------------------------------------ composite
    def _composite_kind(self) -> str:
        """What the composite's source is: the projection this run writes ('mip' / 'edf'), else the stack."""
        return self._projection_kind() or 'stack'

    def _new_composite(self, timepoint, region, shared_hist=None):
        """The device target of one region's composite (composite.CompositeTarget), or None without --composite."""
        if not self.composite:
            return None
        kind = self._composite_kind()
        tag = '' if kind == 'stack' else '_' + kind
        folder = os.path.join(self.output_folder, f"{timepoint}_stitched")
        os.makedirs(folder, exist_ok=True)
        width, height = self.calculate_output_dimensions(timepoint, region)
        names = self.composite_channels or self.monochrome_channels
        chans = [self.monochrome_channels.index(n) for n in names]
        z = None if kind != 'stack' else (self.num_z // 2 if self.composite_z is None else self.composite_z)
        return composite_mod.CompositeTarget(
            os.path.join(folder, f"{region}_stitched{tag}_composite"), store=f"{region}_stitched{tag}{self.output_format}",
            kind=kind, z=z, channels=chans, labels=list(names), colors=[self.monochrome_colors[c] for c in chans],
            height=height, width=width, max_side=self.composite_max_side, dtype=self.dtype,
            percentiles=self.contrast_percentiles, device=self.device, shared_hist=shared_hist)

    def _emit_composite(self, comp, windows, rgb) -> None:
        """PNG and sidecar: on a worker thread under run() (finished before it returns), at once otherwise."""
        meta = comp.meta(windows)
        if not self._composite_async:
            composite_mod.write_outputs(comp.stem, rgb, meta)
            return
        if self._composite_pool is None:
            self._composite_pool = ThreadPoolExecutor(max_workers=min(4, os.cpu_count() or 2), thread_name_prefix='composite-png')
        self._composite_jobs.append(self._composite_pool.submit(composite_mod.write_outputs, comp.stem, rgb, meta))

    def _finish_composite(self, comp, shared: bool = False) -> None:
        """Windows from the counts read back, render, PNG and sidecar of a composite whose source planes have all been added.
        ``shared``: the ranks of a shared region each hold the means and counts of what they wrote (zeros elsewhere); both are
        summed (every rank takes part, the means widened to int32) and rank 0 renders and writes."""
        if comp is None:
            return
        import torch
        side = getattr(self, '_ingest_stream', None)
        if side is not None:      # run() fuses (and reduces) on a stream of its own
            torch.cuda.current_stream(self.device).wait_stream(side)
        rank, means = 0, None
        if shared:
            import torch.distributed as dist
            rank = dist.get_rank()
            if dist.get_backend() != 'nccl':
                hist = comp.hist.cpu()
                wide = torch.from_numpy(comp.means.cpu().numpy().astype(np.int32))
            else:
                hist = comp.hist.clone()      # (a projection store's own target is summed again for its windows)
                wide = comp.means.to(torch.int32)
            dist.all_reduce(hist, op=dist.ReduceOp.SUM)
            dist.all_reduce(wide, op=dist.ReduceOp.SUM)
            if rank == 0:
                means = torch.from_numpy(wide.cpu().numpy().astype(comp.dtype)).to(self.device)
            hist = hist.cpu()
        else:
            hist = comp.hist.cpu()
        if rank == 0:
            windows = comp.windows(comp.counts(hist.numpy()))
            self._emit_composite(comp, windows, comp.render(windows, means))

    def _defer_composite(self, comp) -> None:
        """A streamed region under run(): the counts leave the device behind the region's last launch; the picture is rendered
        and written once they have arrived (the next region is not held up, the chunk pipeline is not drained)."""
        import torch
        host = torch.empty(comp.hist.shape, dtype=comp.hist.dtype, pin_memory=True)
        with torch.cuda.stream(self._ingest_stream):
            host.copy_(comp.hist, non_blocking=True)
            event = torch.cuda.Event()
            event.record()
        self._composite_pending.append((comp, host, event))
        self._finish_composites(wait=False)

    def _finish_composites(self, wait: bool) -> None:
        """Pictures of the streamed regions whose counts have reached the host (``wait``: of all of them, and every PNG is on
        disk)."""
        while self._composite_pending and (wait or self._composite_pending[0][2].query()):
            comp, host, event = self._composite_pending.pop(0)
            event.synchronize()      # (the means were written before the counts were copied, on the same stream)
            windows = comp.windows(comp.counts(host.numpy()))
            self._emit_composite(comp, windows, comp.render(windows))
        if wait:
            jobs, self._composite_jobs = self._composite_jobs, []
            for job in jobs:
                job.result()
            self._composite_async = False
            if self._composite_pool is not None:
                self._composite_pool.shutdown(wait=True)
                self._composite_pool = None

    def _zarr_path(self, timepoint, region) -> str:
        return os.path.join(self.output_folder, f"{timepoint}_stitched", f"{region}_stitched.ome.zarr")

    def _dz_um(self) -> float:
        return float(self.acquisition_params.get('dz(um)', 1.0)) if self.acquisition_params else 1.0

    def save_region_ome_zarr(self, timepoint, region, stitched_region):
        """(stitcher.py:771-859) via the package-free writer in omezarr.py; ``stitched_region`` is a
        5-D numpy array or device tensor.  The pyramid levels (Scaler.nearest, :797-798) come from the
        device kernel either way."""
        output_path = self._zarr_path(timepoint, region)
        os.makedirs(os.path.dirname(output_path), exist_ok=True)
        hist = self._new_histogram()
        comp = self._new_composite(timepoint, region) if self._composite_kind() == 'stack' else None
        write_ome_zarr(output_path, stitched_region, pixel_size_um=self.pixel_size_um, dz_um=self._dz_um(),
                       channel_names=self.monochrome_channels, channel_colors=self.monochrome_colors,
                       num_levels=self.num_pyramid_levels, chunks=self.chunks or (1, 1, 1, 512, 512),
                       name=f"{region}_t{timepoint}", compression=self.zarr_compression,
                       pyramid_method=self.pyramid_method, device=self.device, histogram=hist, composite=comp)
        self._write_contrast(output_path, hist)
        self._finish_composite(comp)
        return output_path

    def _projection_kind(self) -> Optional[str]:
        """The file-name tag of the projection this run writes: 'mip' (--z-projection max / max-only), 'edf' (focus /
        focus-only) or None."""
        return {'max': 'mip', 'max-only': 'mip', 'focus': 'edf', 'focus-only': 'edf'}.get(self.z_projection)

    def _projection_target(self, timepoint, region, rows=None, channel=None):
        """A region's (or one channel's row band's) projection buffers -> (the image [n, Hc, Wc] to write, the stitch_planes
        ``project_to`` that fills it): the MIP, or the best-focus output with its key plane."""
        n = None if channel is None else 1
        chans = range(self.num_c) if channel is None else [channel]
        if self._projection_kind() == 'edf':
            out, key = self._new_focus(timepoint, region, rows, n)
            return out, {c: (out[i], key[i]) for i, c in enumerate(chans)}      # (every channel on its own: no guide)
        proj = self._new_projection(timepoint, region, rows, n)
        return proj, {c: proj[i] for i, c in enumerate(chans)}

    def _mip_path(self, timepoint, region, kind: str = 'mip') -> str:
        return os.path.join(self.output_folder, f"{timepoint}_stitched", f"{region}_stitched_{kind}{self.output_format}")

    def save_region_mip(self, timepoint, region, mip, kind: str = 'mip') -> str:
        """``<t>_stitched/<region>_stitched_<kind><format>`` (kind 'mip': the maximum-intensity projection, 'edf': the best-focus
        one): the (1, C, 1, Hc, Wc) projection (numpy or device tensor) with the
        stack's channel names, colours, pixel size and pyramid level count, through the same writers as the stack."""
        output_path = self._mip_path(timepoint, region, kind)
        os.makedirs(os.path.dirname(output_path), exist_ok=True)
        if self.output_format.endswith('.zarr'):
            hist = self._new_histogram()
            # the composite's source is this store: with percentile windows its histogram target holds the same counts
            comp = self._new_composite(timepoint, region, shared_hist=hist) if kind == self._composite_kind() else None
            write_ome_zarr(output_path, mip, pixel_size_um=self.pixel_size_um, dz_um=self._dz_um(),
                           channel_names=self.monochrome_channels, channel_colors=self.monochrome_colors,
                           num_levels=self.num_pyramid_levels, chunks=self.chunks or (1, 1, 1, 512, 512),
                           name=f"{region}_t{timepoint}_{kind}", compression=self.zarr_compression,
                           pyramid_method=self.pyramid_method, device=self.device, histogram=hist, composite=comp)
            self._finish_composite(comp)
            self._write_contrast(output_path, hist)
            return output_path
        comp = self._new_composite(timepoint, region) if kind == self._composite_kind() else None
        if self._tiff_pyramid():
            self._write_pyramid_tiff(output_path, mip, self.monochrome_channels, self.monochrome_colors,
                                     f"{region}_t{timepoint}_{kind}", self.pyramid_method, comp)
            self._finish_composite(comp)
            return output_path
        if comp is not None:      # the projection buffer, while it is on the device
            import torch
            planes = mip if hasattr(mip, 'data_ptr') else torch.from_numpy(np.ascontiguousarray(mip)).to(self.device)
            comp.add(planes.reshape((-1,) + tuple(planes.shape[3:])), [(0, c, 0) for c in range(int(planes.shape[1]))])
            self._finish_composite(comp)
        if hasattr(mip, 'cpu'):
            mip = mip.cpu().numpy()
        print(f"Writing OME-TIFF to: {output_path}")
        write_ome_tiff(output_path, np.asarray(mip), pixel_size_um=self.pixel_size_um, dz_um=self._dz_um(),
                       channel_names=self.monochrome_channels, channel_colors=self.monochrome_colors,
                       name=f"{region}_t{timepoint}_{kind}")
        return output_path

    def create_mip_store(self, timepoint, region, kind: str = 'mip'):
        """Metadata of the region's projection store (Z = 1, no chunks) -> (path, level shapes)."""
        output_path = self._mip_path(timepoint, region, kind)
        os.makedirs(os.path.dirname(output_path), exist_ok=True)
        width, height = self.calculate_output_dimensions(timepoint, region)
        shapes = omezarr.create_store(output_path, (1, self.num_c, 1, height, width), self.dtype,
                                      pixel_size_um=self.pixel_size_um, dz_um=self._dz_um(),
                                      channel_names=self.monochrome_channels, channel_colors=self.monochrome_colors,
                                      num_levels=self.num_pyramid_levels, chunks=self.chunks or (1, 1, 1, 512, 512),
                                      name=f"{region}_t{timepoint}_{kind}", compression=self.zarr_compression,
                                      pyramid_method=self.pyramid_method)
        return output_path, shapes

    def _depth_labels(self) -> List[str]:
        return omezarr.depth_labels(self.monochrome_channels, self.focus_guide_channel)

    def _depths_of_keys(self, key, depth=None):
        """[k, Hc, Wc] key planes -> their unsigned depth planes (``depth``: the guide's, already derived by stitch_planes)."""
        import torch
        if depth is not None:
            return depth
        depth = torch.empty(tuple(key.shape), dtype=self._depth_dtype(), device=self.device)
        for i in range(len(key)):
            native.focus_depth_plane(key[i], out=depth[i])
        return depth

    def save_region_depth(self, timepoint, region, depth) -> str:
        """``<t>_stitched/<region>_stitched_depth<format>``: the (1, K, 1, Hc, Wc) unsigned depth planes of the best-focus
        projection (z* + 1, 0 = uncovered; K = 1 with a guide channel, else one per channel), with the _edf store's pixel size,
        chunking, compression and level count; levels by nearest, windows 0 ... num_z, no histogram sidecars."""
        output_path = self._mip_path(timepoint, region, 'depth')
        os.makedirs(os.path.dirname(output_path), exist_ok=True)
        labels = self._depth_labels()
        if self.output_format.endswith('.zarr'):
            return omezarr.write_depth_store(output_path, depth, num_z=self.num_z, labels=labels,
                                             pixel_size_um=self.pixel_size_um, dz_um=self._dz_um(),
                                             num_levels=self.num_pyramid_levels, chunks=self.chunks or (1, 1, 1, 512, 512),
                                             name=f"{region}_t{timepoint}_depth", compression=self.zarr_compression,
                                             device=depth.device if hasattr(depth, 'data_ptr') else self._device)
        if self._tiff_pyramid():      # (levels by nearest: a mean of depths is no depth; never JPEG: a lossy depth index is wrong)
            return self._write_pyramid_tiff(output_path, depth, labels, [0xFFFFFF] * len(labels), f"{region}_t{timepoint}_depth",
                                            'nearest', None, lossless=True)
        if hasattr(depth, 'cpu'):
            depth = depth.cpu().numpy()
        print(f"Writing OME-TIFF to: {output_path}")
        write_ome_tiff(output_path, np.asarray(depth), pixel_size_um=self.pixel_size_um, dz_um=self._dz_um(),
                       channel_names=labels, channel_colors=[0xFFFFFF] * len(labels), name=f"{region}_t{timepoint}_depth")
        return output_path

    def create_depth_store(self, timepoint, region):
        """Metadata of the region's depth store (no chunks) -> (path, level shapes)."""
        output_path = self._mip_path(timepoint, region, 'depth')
        os.makedirs(os.path.dirname(output_path), exist_ok=True)
        width, height = self.calculate_output_dimensions(timepoint, region)
        labels = self._depth_labels()
        shapes = omezarr.create_store(output_path, (1, len(labels), 1, height, width), native.depth_dtype_for(self.num_z),
                                      pixel_size_um=self.pixel_size_um, dz_um=self._dz_um(), channel_names=labels,
                                      channel_colors=[0xFFFFFF] * len(labels), num_levels=self.num_pyramid_levels,
                                      chunks=self.chunks or (1, 1, 1, 512, 512), name=f"{region}_t{timepoint}_depth",
                                      compression=self.zarr_compression)
        omezarr.set_channel_windows(output_path, [(0, self.num_z)] * len(labels))
        return output_path, shapes

    def create_region_store(self, timepoint, region):
        """Metadata of the region's OME-Zarr store (no chunks) -> (path, level shapes)."""
        output_path = self._zarr_path(timepoint, region)
        os.makedirs(os.path.dirname(output_path), exist_ok=True)
        width, height = self.calculate_output_dimensions(timepoint, region)
        shapes = omezarr.create_store(output_path, (1, self.num_c, self.num_z, height, width), self.dtype,
                                      pixel_size_um=self.pixel_size_um, dz_um=self._dz_um(),
                                      channel_names=self.monochrome_channels, channel_colors=self.monochrome_colors,
                                      num_levels=self.num_pyramid_levels, chunks=self.chunks or (1, 1, 1, 512, 512),
                                      name=f"{region}_t{timepoint}", compression=self.zarr_compression, pyramid_method=self.pyramid_method)
        return output_path, shapes

    def stream_region_to_zarr(self, timepoint, region, only_planes=None, progress_callback=None, create: bool = True,
                              row_band=None, project_to=None, histogram=None, composite=None):
        """stitch_region + save_region_ome_zarr without the region ever existing in one piece: planes
        are fused a batch at a time and stream through pyramid kernel, pinned D2H copy and compression
        threads while the next batch is read and fused.  Same store as
        ``save_region_ome_zarr(t, r, stitch_region(t, r))``.  ``histogram``: the caller's histogram target (a shared region's
        ranks call this once per row band and finish the windows themselves); None: with contrast_limits='percentile' a fresh
        target is taken and the store's windows and sidecars are written when its last plane has been submitted.
        ``composite``: the caller's composite target (a shared region); None: with --composite and the stack as its source a
        fresh one is taken and the picture written."""
        own_composite = composite is None and create and self.composite and self._composite_kind() == 'stack'
        if own_composite:
            composite = self._new_composite(timepoint, region)
        own_histogram = histogram is None and create
        if own_histogram:
            histogram = self._new_histogram()
        if create:
            output_path, shapes = self.create_region_store(timepoint, region)
        else:
            output_path = self._zarr_path(timepoint, region)
            width, height = self.calculate_output_dimensions(timepoint, region)
            shapes = omezarr.level_shapes((1, self.num_c, self.num_z, height, width), self.num_pyramid_levels)
        made = []
        row_offset, level_heights = 0, None
        if row_band is not None:       # this call writes one row band of the planes: its own (smaller) level buffers
            level_heights = [s[3] for s in shapes]
            row_offset = int(row_band[0])
            shapes = omezarr.level_shapes((1, self.num_c, self.num_z, int(row_band[1]) - row_offset, shapes[0][4]), len(shapes))
            if len(shapes) != len(level_heights):
                raise ValueError(f"row band {row_band} is too short for {len(level_heights)} pyramid levels")

        def make_writer(batch):
            chunks = self.chunks or (1, 1, 1, 512, 512)
            w = self._stream_writer
            if w is not None and w.matches(shapes, self.dtype, batch, self.zarr_compression, chunks, self.pyramid_method):
                w.retarget(output_path, row_offset, level_heights)      # the same geometry: the next store through the same writer
                w.histogram = histogram
                w.composite = composite
                made.append(w)
                return w
            self._close_stream_writer()
            key = ('writer', tuple(tuple(s[3:]) for s in shapes), batch, np.dtype(self.dtype).str)
            cached = self._buffer_cache.get(key)
            arena = None
            if cached is None and not self._arena_unsupported:
                # the writer's two slots of level-0 canvases are what the fusion kernel writes on this path: from an arena too
                # (it lives as long as the slot tensors, i.e. with the cached buffers)
                need = 2 * native.canvas_bytes(batch, shapes[0][3], shapes[0][4], native.torch_dtype_of(self.dtype))
                if need >= self.canvas_arena_min_bytes:
                    arena = self._new_arena(need)
            made.append(omezarr.PlaneStreamWriter(output_path, shapes, self.dtype, chunks=self.chunks or (1, 1, 1, 512, 512),
                                                  batch=batch, compression=self.zarr_compression,
                                                  pyramid_method=self.pyramid_method, device=self.device,
                                                  buffers=cached, row_offset=row_offset,
                                                  level_heights=level_heights, canvas_arena=arena))
            self._keep_buffers(key, made[-1].buffers)
            self._stream_writer = made[-1]
            made[-1].histogram = histogram
            made[-1].composite = composite
            return made[-1]

        before = self._stream_writer.bytes_written if self._stream_writer is not None else 0
        _, ids = self.stitch_planes(timepoint, region, only_planes, progress_callback, stream_to=make_writer, row_band=row_band,
                                    project_to=project_to)
        # bytes of this region's chunks (under run() the writer is drained at the end: the count then lags by what is in flight)
        self.last_bytes_written = sum(w.bytes_written for w in set(made)) - (before if self._stream_writer in made else 0)
        for w in made:
            w.histogram = None
            w.composite = None
        if own_composite:
            if self._defer_drain and getattr(self, '_ingest_stream', None) is not None:
                self._defer_composite(composite)
            else:
                self._finish_composite(composite)
        if own_histogram and histogram is not None:
            if self._defer_drain and getattr(self, '_ingest_stream', None) is not None:
                # run() streams region after region on a stream of its own: the counts leave the device behind this region's last
                # launch, and the windows are written once they have arrived (the next region is not held up)
                import torch
                host = torch.empty(histogram.shape, dtype=histogram.dtype, pin_memory=True)
                with torch.cuda.stream(self._ingest_stream):
                    host.copy_(histogram, non_blocking=True)
                    event = torch.cuda.Event()
                    event.record()
                self._contrast_pending.append((output_path, host, event, histogram))
                self._finish_contrast(wait=False)
            else:
                self._write_contrast(output_path, histogram)
        return output_path

    def _tiff_pyramid(self) -> bool:
        return self.ome_tiff_layout == 'pyramid' and not self.output_format.endswith('.zarr')

    def _tiff_meta(self, channel_names, channel_colors, name: str) -> dict:
        """What ome_xml needs beside shape and dtype: the arguments write_ome_tiff gets for the same image."""
        return {'pixel_size_um': self.pixel_size_um, 'dz_um': self._dz_um(), 'channel_names': channel_names,
                'channel_colors': channel_colors, 'name': name}

    def _write_pyramid_tiff(self, output_path, image, channel_names, channel_colors, name, pyramid_method, composite,
                            lossless: bool = False) -> str:
        """A (T, C, Z, Y, X) image that exists in one piece (a projection, a depth map, a region fused by stitch_region) as a
        pyramid OME-TIFF, through the streaming writer.  ``lossless``: deflate where the run's codec is JPEG."""
        compression = 'deflate' if lossless and self.ome_tiff_compression == 'jpeg' else self.ome_tiff_compression
        return ometiff.write_pyramid_tiff(output_path, image, meta=self._tiff_meta(channel_names, channel_colors, name),
                                          num_levels=self.num_pyramid_levels, chunks=self.chunks or (1, 1, 1, 512, 512),
                                          compression=compression, device=self.device,
                                          pyramid_method=pyramid_method, composite=composite, quality=self.ome_tiff_quality)

    def stream_region_to_tiff(self, timepoint, region, progress_callback=None, project_to=None):
        """stream_region_to_zarr's counterpart for ``ome_tiff_layout='pyramid'``: the region streams to
        ``<region>_stitched.ome.tiff`` batch by batch through an ometiff.PyramidTiffWriter (pyramid kernels, tile encoder, one
        write per level per batch) and never exists in one piece.  Regions of one geometry share the writer: the file of
        region k is finished behind its last batch while region k + 1 is read and fused."""
        composite = self._new_composite(timepoint, region) if self.composite and self._composite_kind() == 'stack' else None
        output_path = os.path.join(self.output_folder, f"{timepoint}_stitched", f"{region}_stitched{self.output_format}")
        os.makedirs(os.path.dirname(output_path), exist_ok=True)
        width, height = self.calculate_output_dimensions(timepoint, region)
        shapes = omezarr.level_shapes((1, self.num_c, self.num_z, height, width), self.num_pyramid_levels)
        chunks = self.chunks or (1, 1, 1, 512, 512)
        ometiff.check_tile_shape(chunks[3:5])
        meta = self._tiff_meta(self.monochrome_channels, self.monochrome_colors, f"{region}_t{timepoint}")
        made = []

        def make_writer(batch):
            w = self._stream_writer
            if isinstance(w, ometiff.PyramidTiffWriter) and \
                    w.matches(shapes, self.dtype, batch, self.ome_tiff_compression, chunks, self.pyramid_method,
                              quality=self.ome_tiff_quality):
                w.retarget(output_path, meta=meta)      # the same geometry: the next file through the same writer
            else:
                self._close_stream_writer()
                key = ('tiff-writer', tuple(tuple(s[3:]) for s in shapes), batch, np.dtype(self.dtype).str, self.ome_tiff_compression,
                       tuple(chunks)) + ((self.ome_tiff_quality,) if self.ome_tiff_compression == 'jpeg' else ())
                w = ometiff.PyramidTiffWriter(output_path, shapes, self.dtype, meta=meta, chunks=chunks, batch=batch,
                                              compression=self.ome_tiff_compression, device=self.device,
                                              buffers=self._buffer_cache.get(key), pyramid_method=self.pyramid_method,
                                              quality=self.ome_tiff_quality)
                self._keep_buffers(key, w.buffers)
                self._stream_writer = w
            w.composite = composite
            made.append(w)
            return w

        self.stitch_planes(timepoint, region, None, progress_callback, stream_to=make_writer, project_to=project_to)
        for w in made:
            w.composite = None
        if not made:      # no plane of the region has a tile: a file of zero tiles all the same
            self._close_stream_writer()
            ometiff.PyramidTiff(output_path, shapes, self.dtype, tile=chunks[3:5], compression=self.ome_tiff_compression,
                                quality=self.ome_tiff_quality, xml=ometiff.ome_xml(shapes[0], self.dtype, **{k: meta[k] for k in
                                                    ('channel_names', 'channel_colors', 'pixel_size_um', 'dz_um', 'name')})).close()
        if not self._defer_drain:      # (run() keeps the writer for the next region and closes it at its end)
            self._close_stream_writer()
        if composite is not None:
            if self._defer_drain and getattr(self, '_ingest_stream', None) is not None:
                self._defer_composite(composite)
            else:
                self._finish_composite(composite)
        return output_path

    def close(self) -> None:
        """Give back what the instance holds beyond its Python objects: the stream writer's threads, the canvas arena."""
        self._close_stream_writer()
        if self._arena is not None and not self._arena.in_use():
            self._arena.close()
        self._arena = None

    def __del__(self):
        try:
            self._close_stream_writer()
        except Exception:
            pass

    def _close_stream_writer(self) -> None:
        """Everything submitted is on disk and the writer's threads are gone (end of run(), a change of geometry, an error)."""
        w, self._stream_writer = getattr(self, '_stream_writer', None), None
        if w is not None:
            w.close()

    def _run_region_by_planes(self, timepoint, region, rank, world):
        """One region shared by all ranks.  With at least as many (channel, z) planes as ranks, every
        rank takes one contiguous run of planes (sharding.contiguous_blocks: a channel's z planes stay together);
        with fewer, every plane is cut into row bands of 512 * 2^(levels-1) level-0 rows
        (sharding.row_bands: whole chunk rows at every pyramid level) and the (plane, band) units are dealt instead
        -- a rank then reads only the tiles that reach into its bands.  Chunks of an OME-Zarr store span neither
        planes nor bands, so the ranks write into one store without locking."""
        n_planes = self.num_c * self.num_z
        width, height = self.calculate_output_dimensions(timepoint, region)
        bands = sharding.row_bands(height, self.num_pyramid_levels, (self.chunks or (1, 1, 1, 512, 512))[3])
        units = sharding.plane_band_units(n_planes, bands, rank, world)
        print(f"\nProcessing timepoint {timepoint}, region {region}: (plane, band) units {units} (rank {rank}/{world})")
        stack = self.z_projection not in ('max-only', 'focus-only')
        self._tile_qc_shared = self.tile_qc
        self._seam_qc_shared = self.seam_qc
        if rank == 0:
            if stack:
                self.create_region_store(timepoint, region)
            if self.z_projection != 'none':
                self.create_mip_store(timepoint, region, self._projection_kind())
                if self.focus_depth_map:
                    self.create_depth_store(timepoint, region)
        sharding.barrier()
        self.starting_stitching.emit()
        self.starting_saving.emit(False)
        output_path = self._zarr_path(timepoint, region)
        by_band = {}
        for p, b in units if stack else ():
            by_band.setdefault(b, []).append(p)
        # --contrast-limits percentile: every rank counts what it writes (planes or row bands), per store
        stack_hist = self._new_histogram() if stack else None
        proj_hist = self._new_histogram() if self.z_projection != 'none' else None
        # --composite: every rank reduces what it writes of the source (the projection, else the stack) into a zeroed target
        comp = self._new_composite(timepoint, region, shared_hist=proj_hist)
        stack_comp = comp if self._composite_kind() == 'stack' else None
        for b, planes in by_band.items():
            output_path = self.stream_region_to_zarr(timepoint, region, planes, progress_callback=self.update_progress.emit,
                                                     create=False, row_band=None if b < 0 else bands[b], histogram=stack_hist,
                                                     composite=stack_comp)
        if self.z_projection != 'none':
            output_path = self._project_region_units(timepoint, region, bands, rank, world, histogram=proj_hist, composite=comp)
            if stack:
                output_path = self._zarr_path(timepoint, region)
        self._finish_composite(comp, shared=True)      # means and counts summed over the ranks, rank 0 renders and writes
        # ... and the counts are summed over the ranks (one that was dealt no unit adds zeros), rank 0 writes the windows
        self._write_contrast(self._zarr_path(timepoint, region), stack_hist, shared=True)
        self._write_contrast(self._mip_path(timepoint, region, self._projection_kind() or 'mip'), proj_hist, shared=True)
        if self.tile_qc:
            try:
                self._finish_tile_qc_shared(timepoint, region, rank)
            finally:
                self._tile_qc_shared = False
        if self.seam_qc:
            try:
                self._finish_seam_qc_shared(timepoint, region, rank)
            finally:
                self._seam_qc_shared = False
        sharding.barrier()
        return output_path

    def _project_region_units(self, timepoint, region, bands, rank, world, histogram=None, composite=None) -> str:
        """This rank's share of a shared region's projection: (channel, row band) units dealt like the stack's (plane, band)
        units (sharding.plane_band_units over the channels), each projected from the tiles of its channel that reach its band
        and written as its own chunks of the store rank 0 created.  With 'max' / 'focus' the files of these channels are read a
        second time (the stack pass dealt planes, not channels, so its staged tiles do not line up with these units).  The
        best-focus windows are the full staged tiles, so a band's rows equal those of the whole region's projection."""
        cunits = sharding.plane_band_units(self.num_c, bands, rank, world)
        print(f"Projection of timepoint {timepoint}, region {region}: (channel, band) units {cunits} (rank {rank}/{world})")
        output_path = self._mip_path(timepoint, region, self._projection_kind())
        width, height = self.calculate_output_dimensions(timepoint, region)
        full = omezarr.level_shapes((1, self.num_c, 1, height, width), self.num_pyramid_levels)
        chunks = self.chunks or (1, 1, 1, 512, 512)
        edf = self._projection_kind() == 'edf'
        g = self._guide if edf else None
        band_depth = {}      # with a guide channel: band -> the guide's (depth plane, output), while this rank's units of the band last
        last_of_band = {b: i for i, (_, b) in enumerate(cunits)}

        def write_band(path, plane, dtype, n_channels, c, y0, y1, b, method, hist, comp=None):
            shapes = omezarr.level_shapes((1, n_channels, 1, y1 - y0, width), len(full))
            with omezarr.PlaneStreamWriter(path, shapes, dtype, chunks=chunks, batch=1, compression=self.zarr_compression,
                                           pyramid_method=method, device=self.device, row_offset=y0,
                                           level_heights=None if b < 0 else [s[3] for s in full]) as writer:
                writer.histogram = hist
                writer.composite = comp
                writer.acquire(1).copy_(plane)
                writer.submit([(0, c, 0)])

        def project(chans, y0, y1, b, depth=None):
            out, key, depth, target = self._focus_target(timepoint, region, (y0, y1), chans, depth)
            self.stitch_planes(timepoint, region, [c * self.num_z + z for c in chans for z in range(self.num_z)],
                               self.update_progress.emit, row_band=None if b < 0 else (y0, y1), stack=False, project_to=target)
            return out, key, depth

        depth_path = self._mip_path(timepoint, region, 'depth')
        depth_dtype = native.depth_dtype_for(self.num_z) if edf else None
        for i, (c, b) in enumerate(cunits):
            y0, y1 = (0, height) if b < 0 else bands[b]
            if not edf:
                proj, target = self._projection_target(timepoint, region, (y0, y1), channel=c)
                self.stitch_planes(timepoint, region, [c * self.num_z + z for z in range(self.num_z)],
                                   self.update_progress.emit, row_band=None if b < 0 else (y0, y1), stack=False,
                                   project_to=target)
            elif g is None:
                proj, key, _ = project([c], y0, y1, b)
                if self.focus_depth_map:
                    write_band(depth_path, self._depths_of_keys(key), depth_dtype, self.num_c, c, y0, y1, b, 'nearest', None)
            else:
                # the guide's depth of this band: computed once on this rank (whichever of its units of the band comes first),
                # by projecting the guide's rows -- the windows are whole staged tiles, so they equal the whole region's
                if b not in band_depth:
                    gout, gkey, _ = project([g], y0, y1, b)
                    band_depth[b] = (self._depths_of_keys(gkey), gout)
                if c == g:
                    proj = band_depth[b][1]
                    if self.focus_depth_map:      # written by the rank that was dealt the guide's unit of the band
                        write_band(depth_path, band_depth[b][0], depth_dtype, 1, 0, y0, y1, b, 'nearest', None)
                else:
                    proj = project([c], y0, y1, b, band_depth[b][0])[0]
                if last_of_band[b] == i:
                    del band_depth[b]
            write_band(output_path, proj, self.dtype, self.num_c, c, y0, y1, b, self.pyramid_method, histogram, composite)
        return output_path

    def save_region_aics(self, timepoint, region, stitched_region):
        """OME-TIFF (or, for a '.ome.zarr' format, OME-Zarr) output (stitcher.py:691-769) through the
        package-free writers: same path template, channel names / colours, physical pixel sizes."""
        if self.output_format.endswith('.zarr'):
            return self.save_region_ome_zarr(timepoint, region, stitched_region)
        if self._tiff_pyramid():
            return self._write_pyramid_tiff(os.path.join(self.output_folder, f"{timepoint}_stitched",
                                                         f"{region}_stitched{self.output_format}"), stitched_region,
                                            self.monochrome_channels, self.monochrome_colors, f"{region}_t{timepoint}",
                                            self.pyramid_method, None)
        if hasattr(stitched_region, 'cpu'):
            stitched_region = stitched_region.cpu().numpy()
        output_path = os.path.join(self.output_folder, f"{timepoint}_stitched", f"{region}_stitched{self.output_format}")
        os.makedirs(os.path.dirname(output_path), exist_ok=True)
        print(f"Writing OME-TIFF to: {output_path}")
        dz_um = float(self.acquisition_params.get('dz(um)', 1.0)) if self.acquisition_params else 1.0
        write_ome_tiff(output_path, np.asarray(stitched_region), pixel_size_um=self.pixel_size_um, dz_um=dz_um,
                       channel_names=self.monochrome_channels, channel_colors=self.monochrome_colors,
                       name=f"{region}_t{timepoint}")
        return output_path

    def write_tile_positions(self, timepoint, region) -> Optional[str]:
        """``<output>/<t>_stitched/<region>_tile_positions.csv`` of a globally registered unit: fov, grid row and column,
        canvas (y, x) in pixels and whether pairs or the all-pairs lattice (prior) placed the tile."""
        solved = self.placements.get((int(timepoint), region))
        if solved is None:
            return None
        xs, ys = sorted(set(v['x'] for v in self.get_region_data(timepoint, region).values())), \
            sorted(set(v['y'] for v in self.get_region_data(timepoint, region).values()))
        fov_of = {(ys.index(v['y']), xs.index(v['x'])): int(v['fov_idx']) for v in self.get_region_data(timepoint, region).values()}
        path = os.path.join(self.output_folder, f"{timepoint}_stitched", f"{region}_tile_positions.csv")
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, 'w') as fh:
            fh.write(alignment.positions_csv(solved, fov_of))
        return path

    def _write_shift_table(self, n_units, my_rows, rank, world, coll, shared: bool = False) -> None:
        """``shift_table.json`` in the output folder: the shifts every (timepoint, region) was fused with.
        With per-region registration every rank contributes the rows it measured: one all-gather of
        ceil(units / world) rows of 8 int32 per rank (RCCL over xGMI with the nccl backend) -- the only
        collective on the path."""
        units = [(int(t), region) for t in self.timepoints for region in self.regions]
        if self._per_unit_registration:
            # rows any rank can hold: its block-cyclic share of the units -- or all of them on rank 0 when the
            # ranks share every region plane by plane (fewer units than GPUs) and rank 0 registers each
            per_rank = n_units if shared else -(-n_units // world)
            local = np.zeros((per_rank, sharding.SHIFT_ROW), dtype=np.int32)
            index = np.full(per_rank, -1, dtype=np.int64)
            for slot, (i, row) in enumerate(sorted(my_rows.items())):
                local[slot], index[slot] = row, i
            # the unit index travels in the row's spare high bits of column 0: valid flags use bits 0-1
            local[:, 0] |= ((index + 1).astype(np.int32) << 8)
            table = sharding.all_gather_shift_table(local, device=coll)
            rows = {}
            for row in table:
                i = (int(row[0]) >> 8) - 1
                if i >= 0:
                    clean = row.copy()
                    clean[0] &= 0xFF
                    rows[i] = sharding.row_to_shifts(clean)
        else:
            rows = {i: self._shifts() for i in range(n_units)}
        if rank != 0:
            return
        entries = []
        for i, (t, region) in enumerate(units):
            s = rows.get(i)
            if s is None:
                continue
            e = {'timepoint': t, 'region': region, 'h_shift': [int(v) for v in s.h_shift], 'v_shift': [int(v) for v in s.v_shift]}
            if s.h_shift_rev is not None:
                e.update(h_shift_rev=[int(v) for v in s.h_shift_rev], h_shift_rev_odd=int(s.h_shift_rev_odd))
            entries.append(e)
        with open(os.path.join(self.output_folder, 'shift_table.json'), 'w') as fh:
            json.dump({'per_region_registration': self.per_region_registration, 'shifts': entries,
                       'flatfield_estimator': (getattr(self, 'flatfield_info', None) or {}).get('estimator')
                       if getattr(self, 'apply_flatfield', False) else None},
                      fh, indent=1)

    # --------------------------------------------------------------------- run
    def run(self):
        """(stitcher.py:1226-1299): metadata, [flatfields], [shifts once], then every
        timepoint x region: stitch + save."""
        stime = time.time()
        self.get_timepoints()
        self.extract_acquisition_parameters()
        self.get_pixel_size()
        self.parse_acquisition_metadata()
        # One process per GPU (torchrun): rank 0 registers, the shift table is all-gathered (RCCL
        # over xGMI with the nccl backend), and the (timepoint, region) units are dealt to the ranks
        # block-cyclically -- they are independent, so no image data is ever exchanged.
        rank, world = sharding.rank_and_world()
        self.output_folder = sharding.broadcast_object(self.output_folder)   # the name embeds datetime.now()
        os.makedirs(self.output_folder, exist_ok=True)
        if self.apply_flatfield:
            if rank == 0:
                print("Calculating flatfields...")
                self.getting_flatfields.emit()
                self.get_flatfields(progress_callback=self.update_progress.emit)
                print("Time to calculate flatfields:", time.time() - stime)
            self.flatfields = sharding.broadcast_object(self.flatfields)   # the estimate samples tiles at random
            self.flatfield_info = sharding.broadcast_object(self.flatfield_info)
            if rank == 0 and self.flatfield_info is not None:
                with open(os.path.join(self.output_folder, 'flatfield_info.json'), 'w') as fh:
                    json.dump(self.flatfield_info, fh, indent=1)
        coll = sharding.collective_device(self)
        # all-pairs registration (--all-pairs-registration) is sharded by PAIR: every rank registers its run of the pair
        # list and the float64 pair table is all-gathered (registration.register_all_pairs_sharded); the reference's
        # centre-pair scheme is three tiles' worth of work and stays on rank 0, its 8-int32 row all-gathered
        pair_sharded = world > 1 and (self.all_pairs_registration or self.global_registration)
        if self.use_registration and not self._per_unit_registration:
            if rank == 0 or pair_sharded:
                print(f"\nCalculating shifts on region {self.regions[0]}...")
                self._pair_ranks = (rank, world) if pair_sharded else None
                try:
                    self.calculate_shifts(self.timepoints[0], self.regions[0])
                finally:
                    self._pair_ranks = None
            if world > 1 and not pair_sharded:
                row = sharding.shifts_to_row(self._shifts() if rank == 0 else None)
                table = sharding.all_gather_shift_table(row[None], device=coll)
                self._apply_shifts(sharding.first_valid(table))
        units = [(int(t), region) for t in self.timepoints for region in self.regions]
        n_units = len(units)
        output_path = None
        try:
            self._defer_drain = True      # regions of one geometry stream through ONE writer; it is drained once, below
            self._composite_async = True
            output_path = self._run_units(units, n_units, rank, world, coll, pair_sharded)
        finally:
            self._defer_drain = False
            self._close_stream_writer()
        if self._despeckle_pending or self._tile_qc_pending or self._seam_qc_pending:      # the writer has been drained: every region's launches have finished
            import torch
            torch.cuda.synchronize(self.device)
            self._finish_despeckle()
            self._finish_tile_qc()
            self._finish_seam_qc()
        self._finish_contrast(wait=True)
        self._finish_composites(wait=True)
        sharding.barrier()
        self.starting_saving.emit(True)
        if self.merge_timepoints or self.merge_hcs_regions:
            print("Note: merging timepoints / HCS regions is an output-format step outside the hot-path scope; "
                  "per-(timepoint, region) stores were written.")
        final_path = os.path.join(self.output_folder, f"{self.timepoints[-1]}_stitched",
                                  f"{self.regions[-1]}_stitched{'_' + self._projection_kind() if self.z_projection.endswith('-only') else ''}"
                                  f"{self.output_format}")
        self.finished_saving.emit(final_path, self.dtype)
        print(f"Total processing time: {time.time() - stime}")

    def _run_units(self, units, n_units, rank, world, coll, pair_sharded):
        """The (timepoint, region) loop of run(): returns the last output path."""
        output_path = None
        shared = world > 1 and n_units < world and self.output_format.endswith('.zarr')
        my_rows = {}      # unit index -> shift row measured by this rank (per-region registration)
        if shared:
            # fewer (timepoint, region) units than GPUs: share each region by (channel, z) plane
            # instead -- every rank fuses its planes and writes their chunks into the common store
            for i, (timepoint, region) in enumerate(units):
                if self._per_unit_registration and pair_sharded:
                    # the ranks share this region anyway: they share its pairs too
                    self._pair_ranks = (rank, world)
                    try:
                        self.calculate_shifts(timepoint, region)
                    finally:
                        self._pair_ranks = None
                    if rank == 0:
                        my_rows[i] = sharding.shifts_to_row(self._shifts())
                        self.write_tile_positions(timepoint, region)
                elif self._per_unit_registration:
                    if rank == 0:
                        self.calculate_shifts(timepoint, region)
                        my_rows[i] = sharding.shifts_to_row(self._shifts())
                    row = my_rows.get(i, sharding.shifts_to_row(None))
                    self._apply_shifts(sharding.first_valid(sharding.all_gather_shift_table(row[None], device=coll)))
                output_path = self._run_region_by_planes(timepoint, region, rank, world)
            units = []
        for i in sharding.block_cyclic(len(units), rank, world):
            timepoint, region = units[i]
            rtime = time.time()
            print(f"\nProcessing timepoint {timepoint}, region {region}" + (f" (rank {rank}/{world})" if world > 1 else ""))
            os.makedirs(os.path.join(self.output_folder, f"{timepoint}_stitched"), exist_ok=True)
            if self._per_unit_registration:
                self.calculate_shifts(timepoint, region)
                my_rows[i] = sharding.shifts_to_row(self._shifts())
                self.write_tile_positions(timepoint, region)
            self.starting_stitching.emit()
            # --z-projection: the projection comes from the tiles the stack pass stages (one read of every file)
            proj, project_to, keys, depth = None, None, None, None
            if self._projection_kind() == 'edf':
                proj, keys, depth, project_to = self._focus_target(timepoint, region)
            elif self.z_projection != 'none':
                proj, project_to = self._projection_target(timepoint, region)
            if self.z_projection in ('max-only', 'focus-only'):
                self.starting_saving.emit(False)
                self.stitch_planes(timepoint, region, None, self.update_progress.emit, stack=False, project_to=project_to)
            elif self.output_format.endswith('.zarr'):
                # fused planes stream to the store batch by batch; saving overlaps stitching
                self.starting_saving.emit(False)
                output_path = self.stream_region_to_zarr(timepoint, region, progress_callback=self.update_progress.emit,
                                                         project_to=project_to)
            elif self._tiff_pyramid():
                self.starting_saving.emit(False)
                output_path = self.stream_region_to_tiff(timepoint, region, progress_callback=self.update_progress.emit,
                                                         project_to=project_to)
            else:
                comp = self._new_composite(timepoint, region) if self._composite_kind() == 'stack' else None
                stitched_region = self._stitch_region(timepoint, region, self.update_progress.emit, project_to=project_to,
                                                      composite=comp)
                self._finish_composite(comp)
                self.starting_saving.emit(False)
                output_path = self.save_region_aics(timepoint, region, stitched_region)
            if proj is not None:      # (ordered after the projection kernels: stitch_planes made this stream wait for them)
                mip_path = self.save_region_mip(timepoint, region, proj.unsqueeze(0).unsqueeze(2), self._projection_kind())
                if self.z_projection in ('max-only', 'focus-only'):
                    output_path = mip_path
                if self.focus_depth_map:
                    if self.num_c == 1:
                        depth = None      # no follower: stitch_planes had no reason to derive the guide's depth plane
                    self.save_region_depth(timepoint, region, self._depths_of_keys(keys, depth).unsqueeze(0).unsqueeze(2))
            print(f"Completed region {region} (saved to {output_path}): {time.time() - rtime}")
        if self.use_registration:
            self._write_shift_table(n_units, my_rows, rank, world, coll, shared)
        return output_path
