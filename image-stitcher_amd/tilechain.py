"""The per-tile filter chain between the staged tiles' copy to the device and their fusion (host side: what it allocates,
what that costs per staged plane, and the order of its launches).  ``Stitcher.stitch_planes`` builds one ``TileChain`` per call."""
from __future__ import annotations

import numpy as np

from . import native

# Every device buffer of the chain, once: (cache key name, planes of the files' or the tiles' shape, as deep as a chunk or as
# a chunk's derived planes, the option that allocates it).  Both byte counts and the allocation are read off this table.
BUFFERS = (('ingest', 'file', 'chunk', None),                  # the raw tiles: the ring's slots, see RING
           ('dpc', 'file', 'derived', None),                   # the raw right halves: the ring's, too
           ('distortion', 'file', 'chunk', 'warped'),          # the corrected copy of the staged planes
           ('distortion-dpc', 'file', 'derived', 'warped'),    # ... and of the right halves
           ('shift', 'file', 'chunk', 'shifted'),              # the shifted copy of the staged planes (--channel-shift, --channel-affine)
           ('binning', 'tile', 'chunk', 'binned'),             # the binned copy of the staged planes
           ('binning-dpc', 'tile', 'derived', 'binned'),       # ... and of the right halves
           ('despeckle', 'tile', 'chunk', 'despeckled'),       # the despeckle's destination
           ('tophat', 'tile', 'chunk', 'tophat'))              # the top-hat's scratch: the erosion, as many bytes as the planes
RING = ('ingest', 'dpc')      # per ingest slot: (pinned staging, device mirrors, the events behind each slot's last reader, turn)
WRITER = ('ingest', 'distortion', 'shift', 'binning')          # what the stream writer's batch is sized by


def warp_and_bin(tiles, ppm, factor, method, warped=None, binned=None, shifts=None, shifted=None, channel_affines=None,
                 darks=None, dark_frames=None, dark_pedestal=0):
    """The head of every way tiles reach the device -- the staged planes, the right halves, registration's stack: corrected
    first (in sensor pixels), binned second, into the first planes of ``warped`` / ``binned`` where they are given.  Between
    the two, ``shifts`` (one (Sy, Sx) per plane of ``tiles``, --channel-shift; None: no launch) moves the planes into
    ``shifted``, or ``channel_affines`` (one (Sy, Sx, Ayy, Ayx, Axy, Axx) per plane, --channel-affine composed with the plane's
    shift; None: no launch) maps them there in ONE launch that takes the place of the shift's: the right halves and
    registration's stack pass neither.  In front of everything, ``darks`` (one (k, c) per plane of ``tiles``, --dark-frame: frame
    k of the device tensor ``dark_frames``, or the constant c; None: no launch) subtracts the camera's additive term IN PLACE
    over ``tiles``, under ``dark_pedestal``: a device copy of a plane must pass here exactly once."""
    m = len(tiles)
    if darks is not None:
        native.dark_tiles(tiles, darks, dark_frames, dark_pedestal)
    if ppm:
        tiles = native.warp_tiles(tiles, ppm, out=None if warped is None else warped[:m])
    if channel_affines is not None:
        tiles = native.affine_tiles(tiles, channel_affines, out=None if shifted is None else shifted[:m])
    elif shifts is not None:
        tiles = native.shift_tiles(tiles, shifts, out=None if shifted is None else shifted[:m])
    if factor > 1:
        tiles = native.bin_tiles(tiles, factor, method, out=None if binned is None else binned[:m])
    return tiles


class TileChain:
    def __init__(self, *, distortion_ppm, binning, binning_method, dpc_planes, dpc_gain, despeckle, despeckle_threshold,
                 tophat_radius, seam_qc_radius, file_shape, tile_shape, dtype, channel_shifts=None, num_z=1,
                 channel_affines=None, dark_params=None, dark_frames=None, dark_pedestal=0, dark_derived=None):
        """``dpc_planes``: the derived channel's plane ids (empty without --dpc); ``tophat_radius``: None without the top-hat;
        ``file_shape`` / ``tile_shape``: (fh, fw) of the files and (th, tw) behind the binning (the same without it);
        ``channel_shifts``: {channel index: (Sy, Sx)} in 1/256 pixel (--channel-shift; None or empty: off), the channel of plane
        id p being p // ``num_z``; ``channel_affines``: {channel index: (Ayy, Ayx, Axy, Axx)} in parts per million
        (--channel-affine; None or empty: off); ``dark_params``: {channel index: (k, c)} (--dark-frame; None or empty: off) --
        frame k of the device tensor ``dark_frames`` [K, fh, fw], or the constant c -- for the channels whose pair is not the
        identity (-1, ``dark_pedestal``), the derived channel's being its LEFT half's; ``dark_derived``: the pair of the right
        halves (None: the identity).  Nothing is allocated for it: the launch works in place over the ring slot's device mirror."""
        self.dark_params, self.dark_frames, self.dark_pedestal = dict(dark_params or {}), dark_frames, int(dark_pedestal)
        self.dark_derived = None if dark_derived is None or tuple(dark_derived) == (-1, self.dark_pedestal) else tuple(dark_derived)
        self.channel_shifts, self.num_z = dict(channel_shifts or {}), int(num_z)
        self.channel_affines = dict(channel_affines or {})
        self.ppm, self.factor, self.method = distortion_ppm, binning, binning_method
        self.dpc_planes, self.dpc_gain = dpc_planes, dpc_gain
        self.despeckle, self.despeckle_threshold = despeckle, despeckle_threshold
        self.tophat_radius, self.seam_qc_radius = tophat_radius, seam_qc_radius
        self.shapes = {'file': tuple(file_shape), 'tile': tuple(tile_shape)}
        self.dtype = np.dtype(dtype)
        on = {None: True, 'warped': distortion_ppm != 0, 'shifted': bool(self.channel_shifts or self.channel_affines),
              'binned': binning > 1,
              'despeckled': despeckle != 'none',
              'tophat': tophat_radius is not None}
        self.buffers = [b[:3] for b in BUFFERS if on[b[3]]]

    # ------------------------------------------------------------------ byte accounting (integers only)
    def derived(self, plane_ids):
        """The positions of the derived planes among ``plane_ids`` (consecutive: the ids ascend)."""
        return [i for i, p in enumerate(plane_ids) if p in self.dpc_planes]

    def _plane_bytes(self, n, names):
        return sum(n * self.shapes[shape][0] * self.shapes[shape][1] * self.dtype.itemsize
                   for name, shape, _ in self.buffers if name in names)

    def plane_bytes(self, n, derived: bool) -> int:
        """Device bytes per staged plane of ``n`` tiles, which the batch budget is divided by: every buffer of the chain; with
        derived planes in the list the right halves' buffers count as whole copies, though only those planes have one."""
        return self._plane_bytes(n, [name for name, _, deep in self.buffers if derived or deep == 'chunk'])

    def writer_plane_bytes(self, n) -> int:
        """One staged plane as the stream writer's batch counts it: the raw tiles, their corrected, shifted and binned copy."""
        return self._plane_bytes(n, WRITER)

    # ------------------------------------------------------------------ allocation
    def key(self, name, depth, n, n_slots=None):
        """The buffer-cache key of buffer ``name``, ``depth`` planes of ``n`` tiles deep (the ring's: of ``n_slots`` slots)."""
        shape = next(b[1] for b in BUFFERS if b[0] == name)
        return (name, depth, n) + self.shapes[shape] + (() if n_slots is None else (n_slots,)) + (self.dtype.str,)

    def allocate(self, cached, device, batch, n, deep, n_slots):
        """{name: buffer} for chunks of ``batch`` planes of ``n`` tiles, ``deep`` of them derived at most, through
        ``cached(key, make)``: kept for the next region of the same shape (page-locking host memory is slow).  The ring's
        events live with its buffers: whoever gets the same cached staging must wait for the copy and the launch still
        reading a slot before the loader writes to it again; its turn goes on across calls.

        ONE buffer of every other kind serves both ingest slots: every launch of the chain and the fusion that reads its result are launches of
        one stream, so the next chunk's launch that overwrites a buffer runs after this chunk's fusion has read it; only the
        H2D copy into the OTHER slot's raw tiles overlaps, and nothing reads those but the first launch of their own chunk."""
        import torch
        bufs = {}
        for name, shape, deep_as in self.buffers:
            depth = batch if deep_as == 'chunk' else deep
            if not depth:
                continue
            dims, tdtype = (depth, n) + self.shapes[shape], native.torch_dtype_of(self.dtype)
            if name in RING:
                make = lambda: ([torch.empty(dims, dtype=tdtype, pin_memory=True) for _ in range(n_slots)],
                                [torch.empty(dims, dtype=tdtype, device=device) for _ in range(n_slots)], [None] * n_slots, [0])
            elif name == 'tophat':
                make = lambda: torch.empty(native.tophat_scratch_bytes(depth * n, *self.shapes[shape], self.dtype),
                                           dtype=torch.uint8, device=device)
            else:
                make = lambda: torch.empty(dims, dtype=tdtype, device=device)
            bufs[name] = cached(self.key(name, depth, n, n_slots if name in RING else None), make)
        return bufs

    # ------------------------------------------------------------------ the launches of one chunk
    def plane_shifts(self, plane_ids):
        """One (Sy, Sx) per plane of ``plane_ids``, or None when none of them is shifted (then nothing is launched)."""
        pairs = [self.channel_shifts.get(p // self.num_z, (0, 0)) for p in plane_ids or ()]
        return pairs if any(pair != (0, 0) for pair in pairs) else None

    def plane_darks(self, plane_ids):
        """One (k, c) per plane of ``plane_ids``, or None when every one of them is the identity (then nothing is launched)."""
        same = (-1, self.dark_pedestal)
        pairs = [tuple(self.dark_params.get(p // self.num_z, same)) for p in plane_ids or ()]
        return pairs if any(pair != same for pair in pairs) else None

    def plane_affines(self, plane_ids):
        """One (Sy, Sx, Ayy, Ayx, Axy, Axx) per plane of ``plane_ids`` -- its shift or (0, 0), its A or zeros -- or None when
        none of them has a non-zero A (then the chunk goes today's way: ``plane_shifts``)."""
        zero = (0, 0, 0, 0)
        channels = [p // self.num_z for p in plane_ids or ()]
        if not any(self.channel_affines.get(c, zero) != zero for c in channels):
            return None
        return [tuple(self.channel_shifts.get(c, (0, 0))) + tuple(self.channel_affines.get(c, zero)) for c in channels]

    def run(self, tiles, slot, derived, b0, bufs, list_counts=None, qc_words=None, seam_table=None, seam_words=None,
            plane_ids=None):
        """The staged planes ``tiles`` [m, n, fh, fw] of the chunk in ring slot ``slot`` (their copy enqueued) -> the planes
        the fusion reads.  ``derived``: the positions of the chunk's derived planes, whose right halves are in the slot's
        pinned 'dpc' buffer; ``b0``: the chunk's first row in the list-wide outputs ``list_counts``, ``qc_words`` and
        ``seam_words`` (each None when its option is off); ``plane_ids``: the chunk's plane ids (--channel-shift: a chunk with
        a shifted plane is ONE shift launch over the whole chunk, which copies its unshifted planes; a chunk without one
        launches nothing; --channel-affine: a chunk with a plane whose A is not zero is ONE affine launch over the whole chunk
        in the shift launch's place, every plane under its shift and its A; --dark-frame: the FIRST launch, in place over the
        slot's device mirror, which the chunk's copy has just filled -- every copy of a plane passes it once).  The order is fixed."""
        import torch
        m = len(tiles)
        affines = self.plane_affines(plane_ids) if self.channel_affines else None
        shifts = self.plane_shifts(plane_ids) if self.channel_shifts and affines is None else None
        darks = self.plane_darks(plane_ids) if self.dark_params else None
        tiles = warp_and_bin(tiles, self.ppm, self.factor, self.method, bufs.get('distortion'), bufs.get('binning'),
                             shifts, bufs.get('shift'), affines, darks, self.dark_frames, self.dark_pedestal)
        if derived:     # in place over the left halves, before anything reads the staged planes
            i0, i1 = derived[0], derived[-1] + 1
            staging, on_dev, read, _ = bufs['dpc']
            halves = on_dev[slot][:i1 - i0]
            halves.copy_(staging[slot][:i1 - i0], non_blocking=True)
            halves = warp_and_bin(halves, self.ppm, self.factor, self.method, bufs.get('distortion-dpc'), bufs.get('binning-dpc'),
                                  darks=None if self.dark_derived is None else self.dark_derived, dark_frames=self.dark_frames,
                                  dark_pedestal=self.dark_pedestal)
            native.dpc_tiles(tiles[i0:i1], halves, self.dpc_gain)
            read[slot] = torch.cuda.Event()
            read[slot].record()
        if qc_words is not None:      # the tiles as they are in their files: before anything filters them
            native.tile_stats(tiles, out=qc_words[b0:b0 + m].view(-1, native.SQ_TILE_STATS_WORDS))
        if 'despeckle' in bufs:       # out of place: everything below reads the filtered planes
            tiles = native.despeckle_tiles(tiles, self.despeckle_threshold, self.despeckle, out=bufs['despeckle'][:m],
                                           counts=list_counts[b0:b0 + m].view(-1))
        if 'tophat' in bufs:          # in place: everything below reads the filtered planes
            native.tophat_tiles(tiles, self.tophat_radius, bufs['tophat'])
        if seam_words is not None:    # the planes as the fusion reads them: behind the last filter
            native.seam_stats(tiles, seam_table[1], self.seam_qc_radius, out=seam_words[b0:b0 + m], pairs_dev=seam_table[2])
        return tiles
