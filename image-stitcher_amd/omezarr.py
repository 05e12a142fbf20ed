"""Minimal OME-Zarr (NGFF 0.4, zarr v2 directory store) writer without the ``zarr`` package.

Layout follows what the reference writes through ome_zarr.writer.write_multiscale
(stitcher.py:771-859): a group with arrays "0".."n-1" (TCZYX), chunks (1,1,1,512,512),
``multiscales`` axes t/c/z/y/x with units and per-level scale [1,1,dz,px*2^l,px*2^l],
and an ``omero`` channel block.  Chunk codecs: ``blosc`` = the reference's default (zarr.storage.default_compressor:
Blosc-1 frames, byte shuffle + LZ4), encoded ON THE DEVICE (csrc/blosc.hip) so that only compressed bytes cross PCIe;
``zlib`` (host threads, stdlib) and ``none`` (raw chunks) remain.  The ``blosc`` / ``numcodecs`` packages are absent
offline: frames are checked by an independent pure-Python reader in the tests.

Pyramid levels are what ome_zarr's ``Scaler.nearest`` produces (level l+1 = level l sampled at
[2y+1, 2x+1], floor-halved shape); they are computed on the device (``native.downsample2``,
csrc/pyramid.hip) -- this module only lays chunks out on disk.  With ``pyramid_method='mean'`` the levels are instead what
the reference's other stitchers store (zarr_stitcher.py:614-719: level l+1 = the truncated 2 x 2 mean of level l,
``(a + b + c + d) >> 2``, same shapes), all of them from one read of level 0 (``native.pyramid_mean``,
csrc/pyramid_mean.hip).  ``PlaneStreamWriter`` is the
"next" row 8(f)1: planes leave the GPU batch by batch (pyramid -> pinned D2H -> compression in
host threads) while the next batch is being fused, so a region never has to exist in host memory.
"""
from __future__ import annotations

import json
import os
import zlib
from typing import List, Optional, Sequence

import numpy as np

from .planewriter import SlotRingWriter


def _write_json(path: str, obj) -> None:
    with open(path, 'w') as fh:
        json.dump(obj, fh, indent=1)


def blosc_decode(frame: bytes) -> bytes:
    """Blosc-1 frame -> bytes (LZ4 or memcpy'd frames, byte shuffle; what csrc/blosc.hip and c-blosc's lz4 path emit)."""
    version, versionlz, flags, typesize = frame[0], frame[1], frame[2], frame[3]
    nbytes, blocksize, cbytes = (int.from_bytes(frame[4 + 4 * k:8 + 4 * k], 'little') for k in range(3))
    if version != 2 or cbytes != len(frame):
        raise ValueError("not a Blosc-1 frame")
    if flags & 0x02:
        return bytes(frame[16:16 + nbytes])
    if (flags >> 5) != 1 or versionlz != 1:
        raise ValueError("only LZ4 frames are read here")
    nblocks = -(-nbytes // blocksize) if nbytes else 0
    out = bytearray()
    for b in range(nblocks):
        n = min(blocksize, nbytes - b * blocksize)
        at = int.from_bytes(frame[16 + 4 * b:20 + 4 * b], 'little')
        nsplits = 1 if (flags & 0x10) or typesize > 16 or n // max(typesize, 1) < 128 or n % blocksize else typesize
        raw = bytearray()
        for _ in range(nsplits):
            cb = int.from_bytes(frame[at:at + 4], 'little')
            at += 4
            want = n // nsplits
            raw += frame[at:at + cb] if cb == want else _lz4_block(frame[at:at + cb], want)
            at += cb
        if (flags & 0x01) and typesize > 1:
            nel = n // typesize
            arr = np.frombuffer(bytes(raw[:nel * typesize]), dtype=np.uint8).reshape(typesize, nel).T
            raw = bytearray(arr.tobytes()) + raw[nel * typesize:]
        out += raw
    return bytes(out)


def _lz4_block(src: bytes, n: int) -> bytearray:
    out = bytearray()
    i, end = 0, len(src)
    while i < end:
        token = src[i]
        i += 1
        lit = token >> 4
        if lit == 15:
            while True:
                v = src[i]
                i += 1
                lit += v
                if v != 255:
                    break
        out += src[i:i + lit]
        i += lit
        if i >= end:
            break
        off = src[i] | (src[i + 1] << 8)
        i += 2
        ml = token & 15
        if ml == 15:
            while True:
                v = src[i]
                i += 1
                ml += v
                if v != 255:
                    break
        ml += 4
        start = len(out) - off
        if off == 0 or start < 0:
            raise ValueError("corrupt LZ4 block")
        if off >= ml:
            out += out[start:start + ml]
        else:
            for k in range(ml):
                out.append(out[start + k])
    if len(out) != n:
        raise ValueError(f"LZ4 block decoded to {len(out)} bytes, expected {n}")
    return out


def read_array(path: str) -> np.ndarray:
    """One array of a store back into memory (used by tests to check the store round-trips)."""
    with open(os.path.join(path, '.zarray')) as fh:
        meta = json.load(fh)
    shape, chunks, dt = meta['shape'], meta['chunks'], np.dtype(meta['dtype'])
    codec = (meta.get('compressor') or {}).get('id')
    decode = {None: bytes, 'zlib': zlib.decompress, 'blosc': blosc_decode}[codec]
    out = np.zeros(shape, dtype=dt)
    for idx in np.ndindex(*[-(-s // c) for s, c in zip(shape, chunks)]):
        p = os.path.join(path, *map(str, idx))
        if not os.path.exists(p):
            continue
        with open(p, 'rb') as fh:
            raw = fh.read()
        block = np.frombuffer(decode(raw), dtype=dt).reshape(chunks)
        sl = tuple(slice(i * c, min((i + 1) * c, s)) for i, c, s in zip(idx, chunks, shape))
        out[sl] = block[tuple(slice(0, s.stop - s.start) for s in sl)]
    return out


def level_shapes(shape: Sequence[int], num_levels: int) -> List[tuple]:
    """TCZYX shapes of the pyramid levels: every level halves y and x of the one before, rounding
    down (Scaler.nearest resizes to (Y // 2, X // 2))."""
    out = [tuple(int(v) for v in shape)]
    for _ in range(1, max(1, num_levels)):
        t, c, z, y, x = out[-1]
        if y < 2 or x < 2:
            break
        out.append((t, c, z, y // 2, x // 2))
    return out


PYRAMID_METHODS = ('nearest', 'mean')


def check_pyramid_method(method: str) -> str:
    if method not in PYRAMID_METHODS:
        raise ValueError(f"pyramid_method must be 'nearest' or 'mean', got {method!r}")
    return method


CONTRAST_LIMITS = ('dtype', 'percentile')


def check_contrast(contrast_limits: str, contrast_percentiles) -> tuple:
    """-> (contrast_limits, (lo, hi)) validated: 'dtype' | 'percentile', 0 <= lo < hi <= 100."""
    if contrast_limits not in CONTRAST_LIMITS:
        raise ValueError(f"contrast_limits must be 'dtype' or 'percentile', got {contrast_limits!r}")
    try:
        lo, hi = (float(v) for v in contrast_percentiles)
    except (TypeError, ValueError):
        raise ValueError(f"contrast_percentiles must be two numbers LO HI, got {contrast_percentiles!r}") from None
    if not 0 <= lo < hi <= 100:      # (also refuses NaN)
        raise ValueError(f"contrast_percentiles must satisfy 0 <= LO < HI <= 100, got {lo:g} {hi:g}")
    return contrast_limits, (lo, hi)


def histogram_percentile(hist_row, q: float) -> Optional[int]:
    """The q-th percentile of the NON-ZERO voxels counted in ``hist_row`` (counts per value, bin 0 ignored), or None when there
    is none: the smallest v with cum[v] >= floor(q / 100 * (N - 1)) + 1 -- what ``numpy.percentile(x[x > 0], q,
    method='lower')`` returns.  Python integers throughout (a channel of a large region passes 2^32 voxels)."""
    counts = np.asarray(hist_row).astype(np.int64, copy=False)
    cum = np.cumsum(counts[1:], dtype=np.int64)
    n = int(cum[-1]) if len(cum) else 0
    if n <= 0:
        return None
    # numpy's virtual index is the float64 product q / 100 * (N - 1); its floor is taken the same way here
    rank = min(n - 1, int(np.floor(np.float64(q) / 100 * (n - 1)))) + 1
    return int(np.searchsorted(cum, rank, side='left')) + 1


def contrast_window(hist_row, lo: float, hi: float, dtype_max: int) -> tuple:
    """(start, end) of a channel's rendering window from the exact value counts of what was written: the ``lo``-th and
    ``hi``-th percentile of the non-zero voxels (value 0 is what the canvas holds where no tile reaches).  ``end <= start``
    becomes ``end = start + 1`` (inside the dtype's range); a channel without a non-zero voxel keeps ``0 ... dtype_max``."""
    dtype_max = int(dtype_max)
    start = histogram_percentile(hist_row, lo)
    if start is None:
        return 0, dtype_max
    end = histogram_percentile(hist_row, hi)
    if end <= start:
        end = min(start + 1, dtype_max)
        if end <= start:
            start = end - 1
    return int(start), int(end)


def channel_stats(hist, labels: Sequence[str], lo: float, hi: float, dtype_max: int) -> list:
    """Per channel (row of ``hist``): what ``<stem>_stats.json`` records."""
    out = []
    for i, row in enumerate(np.asarray(hist)):
        row = row.astype(np.int64, copy=False)      # (sums below stay far inside int64: value x count <= 2^16 x 2^47)
        nz = np.nonzero(row[1:])[0]
        voxels, nonzero = int(row.sum()), int(row[1:].sum())
        total = int(np.dot(np.arange(len(row), dtype=np.int64), row))
        start, end = contrast_window(row, lo, hi, dtype_max)
        out.append({'label': labels[i] if i < len(labels) else str(i), 'voxels': voxels, 'nonzero_voxels': nonzero,
                    'min_nonzero': int(nz[0]) + 1 if len(nz) else None, 'max_nonzero': int(nz[-1]) + 1 if len(nz) else None,
                    'mean': (total / voxels) if voxels else None,
                    'percentiles': {f'{lo:g}': histogram_percentile(row, lo), f'{hi:g}': histogram_percentile(row, hi)},
                    'window': {'start': start, 'end': end}})
    return out


def set_channel_windows(path: str, windows: Sequence[tuple]) -> None:
    """Rewrite ``omero.channels[i].window.start / end`` of a store made by ``create_store`` (one (start, end) per channel);
    every other key of ``.zattrs`` stays as it is."""
    zattrs = os.path.join(path, '.zattrs')
    with open(zattrs) as fh:
        attrs = json.load(fh)
    channels = attrs['omero']['channels']
    if len(windows) != len(channels):
        raise ValueError(f"{path}: {len(channels)} channels, {len(windows)} windows given")
    for ch, (start, end) in zip(channels, windows):
        ch['window']['start'], ch['window']['end'] = int(start), int(end)
    _write_json(zattrs, attrs)


def sidecar_paths(path: str) -> tuple:
    """(<stem>_histogram.npy, <stem>_stats.json) beside the store ``path`` (<stem>.ome.zarr)."""
    stem = path[:-len('.ome.zarr')] if path.endswith('.ome.zarr') else os.path.splitext(path)[0]
    return stem + '_histogram.npy', stem + '_stats.json'


def write_contrast(path: str, hist, lo: float, hi: float, dtype) -> list:
    """A store's windows from the histograms of its own level 0 (``hist``: int64 [C, bins], host): ``.zattrs`` rewritten, the
    two sidecars written.  Returns the windows.  Planes (or row bands) that no tile reaches are never submitted -- the store
    holds its fill value 0 there -- so what a channel's counts lack of the store's voxels is added to bin 0."""
    hist = np.array(hist, dtype=np.int64)
    with open(os.path.join(path, '0', '.zarray')) as fh:
        shape = json.load(fh)['shape']
    per_channel = int(np.prod([int(v) for v in shape[:1] + shape[2:]], dtype=object))
    missing = per_channel - hist.sum(axis=1)
    if hist.shape[0] != shape[1] or (missing < 0).any():
        raise ValueError(f"{path}: the histograms {hist.shape} count more voxels than the store holds ({shape})")
    hist[:, 0] += missing
    with open(os.path.join(path, '.zattrs')) as fh:
        labels = [ch['label'] for ch in json.load(fh)['omero']['channels']]
    dtype_max = int(np.iinfo(np.dtype(dtype)).max)
    stats = channel_stats(hist, labels, lo, hi, dtype_max)
    windows = [(s['window']['start'], s['window']['end']) for s in stats]
    set_channel_windows(path, windows)
    npy, js = sidecar_paths(path)
    np.save(npy, hist)
    _write_json(js, {'contrast_percentiles': [lo, hi], 'channels': stats})
    return windows


def _compressor(compression: str, level: int = 1):
    if compression in (None, 'none', 'raw'):
        return None
    if compression == 'zlib':
        return {'id': 'zlib', 'level': int(level)}
    if compression == 'blosc':      # what zarr.storage.default_compressor serialises to (zarr 2.x)
        return {'id': 'blosc', 'cname': 'lz4', 'clevel': 5, 'shuffle': 1, 'blocksize': 0}
    raise ValueError(f"compression must be 'blosc', 'zlib' or 'none', got {compression!r}")


def _zarray_meta(shape, chunks, dtype, compression='zlib', level=1):
    dtype = np.dtype(dtype)
    chunks = tuple(int(min(c, s)) if s else int(c) for c, s in zip(chunks, shape))
    return chunks, {
        'zarr_format': 2, 'shape': list(shape), 'chunks': list(chunks),
        'dtype': dtype.newbyteorder('<').str if dtype.itemsize > 1 else dtype.str,
        'compressor': _compressor(compression, level), 'fill_value': 0, 'order': 'C', 'filters': None,
        'dimension_separator': '/'}


def create_store(path: str, shape: Sequence[int], dtype, *, pixel_size_um: float, dz_um: float = 1.0,
                 channel_names: Sequence[str] = (), channel_colors: Sequence[int] = (), num_levels: int = 1,
                 chunks=(1, 1, 1, 512, 512), name: str = 'stitched', compression: str = 'zlib',
                 pyramid_method: str = 'nearest') -> List[tuple]:
    """Group + array metadata of a multiscale OME-Zarr image, no chunks yet.  Returns the level
    shapes.  Chunks are then added plane by plane (``write_plane_levels``), by any number of processes.
    ``pyramid_method='mean'`` names the downscaling in ``multiscales[0]`` ('type' and 'metadata', NGFF 0.4); the default
    writes neither key."""
    check_pyramid_method(pyramid_method)
    os.makedirs(path, exist_ok=True)
    _write_json(os.path.join(path, '.zgroup'), {'zarr_format': 2})
    shapes = level_shapes(shape, num_levels)
    datasets = []
    for lv, shp in enumerate(shapes):
        os.makedirs(os.path.join(path, str(lv)), exist_ok=True)
        _write_json(os.path.join(path, str(lv), '.zarray'), _zarray_meta(shp, chunks, dtype, compression)[1])
        sc = 2 ** lv
        datasets.append({'path': str(lv), 'coordinateTransformations': [
            {'type': 'scale', 'scale': [1, 1, dz_um, pixel_size_um * sc, pixel_size_um * sc]}]})
    dt = np.dtype(dtype)
    info = np.iinfo(dt) if np.issubdtype(dt, np.integer) else None
    attrs = {
        'multiscales': [{
            'version': '0.4', 'name': name,
            'axes': [{'name': 't', 'type': 'time', 'unit': 'second'}, {'name': 'c', 'type': 'channel'},
                     {'name': 'z', 'type': 'space', 'unit': 'micrometer'},
                     {'name': 'y', 'type': 'space', 'unit': 'micrometer'},
                     {'name': 'x', 'type': 'space', 'unit': 'micrometer'}],
            'datasets': datasets}],
        'omero': {'id': 1, 'name': name, 'version': '0.4', 'channels': [
            {'label': n, 'color': f'{(channel_colors[i] if i < len(channel_colors) else 0xFFFFFF):06X}',
             'window': {'start': 0, 'end': int(info.max) if info else 1, 'min': 0, 'max': int(info.max) if info else 1},
             'active': True, 'coefficient': 1, 'family': 'linear'}
            for i, n in enumerate(channel_names)]},
    }
    if pyramid_method == 'mean':
        attrs['multiscales'][0]['type'] = 'mean'
        attrs['multiscales'][0]['metadata'] = {
            'method': 'truncated 2x2 mean of the level before',
            'description': 'level l+1 [y, x] = (a + b + c + d) >> 2 over the 2 x 2 block of level l at [2y, 2x]; every level '
                           'has floor(half) the rows and columns of the one before (a trailing odd row / column is dropped)'}
    _write_json(os.path.join(path, '.zattrs'), attrs)
    return shapes


def chunk_jobs(levels: Sequence[np.ndarray], coords: Sequence[tuple], chunks=(1, 1, 1, 512, 512), row_offset: int = 0,
               level_heights: Optional[Sequence[int]] = None) -> list:
    """One job per chunk of whole (t, c, z) planes: ``levels[l][i]`` is the 2-D plane ``coords[i]`` at
    pyramid level l.  Chunks never span planes (chunk shape (1,1,1,cy,cx)), so different processes can
    write different planes of one store concurrently.

    ``row_offset`` > 0: the arrays are one ROW BAND of the planes, starting at that level-0 row (sharding.row_bands:
    a multiple of chunk rows x 2^(levels-1), so the band starts on a chunk-row boundary of every level);
    ``level_heights`` are then the heights of the FULL levels (the chunk height of a level is min(512, its height))."""
    if tuple(chunks[:3]) != (1, 1, 1):
        raise ValueError("plane-wise writing needs chunks of shape (1, 1, 1, cy, cx)")
    jobs = []
    for lv, arr in enumerate(levels):
        if arr.ndim != 3 or len(arr) < len(coords):
            raise ValueError(f"level {lv}: expected [n_planes, y, x] with n_planes >= {len(coords)}, got {arr.shape}")
        full_h = arr.shape[1] if level_heights is None else int(level_heights[lv])
        cy, cx = min(chunks[3], full_h), min(chunks[4], arr.shape[2])
        if cy == 0 or cx == 0:
            continue
        y_off = int(row_offset) >> lv
        if y_off % cy:
            raise ValueError(f"row band at level-0 row {row_offset} does not start on a chunk row of level {lv}")
        for i, (t, c, z) in enumerate(coords):
            for y in range(0, arr.shape[1], cy):
                for x in range(0, arr.shape[2], cx):
                    jobs.append((lv, t, c, z, (y_off + y) // cy, x // cx, arr[i], y, x, cy, cx))
    return jobs


HOST_CODECS = (None, 'none', 'raw', 'zlib')


def emit_chunk(path: str, job, compression: str = 'zlib', level: int = 1) -> int:
    """Write one chunk (all-zero chunks are left to fill_value).  Returns the bytes written."""
    lv, t, c, z, iy, ix, plane, y, x, cy, cx = job
    if compression not in HOST_CODECS:
        # 'blosc' chunks are encoded on the device (PlaneStreamWriter / write_ome_zarr): writing zlib bytes under a
        # .zarray that says blosc would make a store nothing can read
        raise ValueError(f"emit_chunk compresses on the host with {sorted(str(c) for c in HOST_CODECS)}; {compression!r} chunks "
                         "come from the device encoder (write_ome_zarr / PlaneStreamWriter)")
    block = plane[y:y + cy, x:x + cx]
    if not block.any():
        return 0
    if block.shape != (cy, cx):
        full = np.zeros((cy, cx), dtype=plane.dtype)
        full[:block.shape[0], :block.shape[1]] = block
        block = full
    cdir = os.path.join(path, str(lv), str(t), str(c), str(z), str(iy))
    os.makedirs(cdir, exist_ok=True)
    raw = memoryview(np.ascontiguousarray(block)).cast('B')     # no second copy: file write / zlib read the buffer
    data = raw if compression in (None, 'none', 'raw') else zlib.compress(raw, level)
    with open(os.path.join(cdir, str(ix)), 'wb') as fh:
        fh.write(data)
    return len(data)


def write_plane_levels(path: str, levels: Sequence[np.ndarray], coords: Sequence[tuple], chunks=(1, 1, 1, 512, 512),
                       compression: str = 'zlib', level: int = 1, workers: Optional[int] = None, pool=None,
                       row_offset: int = 0, level_heights: Optional[Sequence[int]] = None) -> int:
    """Write the chunks of whole planes (or of one row band of them), every pyramid level given (see
    ``chunk_jobs``), into a store made by ``create_store``.  Returns the bytes written."""
    from concurrent.futures import ThreadPoolExecutor
    if compression not in HOST_CODECS:
        raise ValueError(f"write_plane_levels compresses on the host with {sorted(str(c) for c in HOST_CODECS)}; {compression!r} "
                         "chunks come from the device encoder (write_ome_zarr / PlaneStreamWriter)")
    jobs = chunk_jobs(levels, coords, chunks, row_offset, level_heights)
    if pool is not None:
        return sum(pool.map(lambda j: emit_chunk(path, j, compression, level), jobs))
    n = workers if workers is not None else min(32, os.cpu_count() or 4)
    if n <= 1 or len(jobs) < 4:
        return sum(emit_chunk(path, j, compression, level) for j in jobs)
    with ThreadPoolExecutor(max_workers=n) as tp:
        return sum(tp.map(lambda j: emit_chunk(path, j, compression, level), jobs))


def device_levels(planes_dev, n_levels: int, out: Optional[list] = None, method: str = 'nearest') -> list:
    """[planes_dev] + its n_levels - 1 pyramid levels, computed on the device: ``method`` 'nearest' = one sq_downsample2
    launch per level, 'mean' = all levels from one read of ``planes_dev`` (sq_pyramid_mean)."""
    from . import native
    check_pyramid_method(method)
    if method == 'mean':
        outs = None if out is None else [o[:len(planes_dev)] for o in out[:n_levels - 1]]
        return [planes_dev] + native.pyramid_mean(planes_dev, n_levels - 1, outs)
    levels = [planes_dev]
    for lv in range(1, n_levels):
        levels.append(native.downsample2(levels[-1], None if out is None else out[lv - 1][:len(planes_dev)]))
    return levels


def _pad_planes(full, m: int):
    """A partly filled slot: the encoder's buffers are sized for the whole batch, so the planes past ``m`` are
    encoded too -- zero them first, their chunks then have size 0 and nothing is written for them."""
    full[m:].zero_()
    return full


def write_ome_zarr(path: str, image, *, pixel_size_um: float, dz_um: float = 1.0,
                   channel_names: Sequence[str] = (), channel_colors: Sequence[int] = (),
                   num_levels: int = 1, chunks=(1, 1, 1, 512, 512), name: str = 'stitched', compression: str = 'zlib',
                   device=None, pyramid_method: str = 'nearest', histogram=None, composite=None) -> str:
    """Write a (T, C, Z, Y, X) array (numpy, or a device tensor) as a multiscale OME-Zarr image.  The
    pyramid levels come from the device kernel, a batch of planes at a time; with ``num_levels`` 1 no
    GPU is touched for a numpy input.  ``histogram``: a device int64 [C, bins] tensor the value counts of level 0 are added
    to (``PlaneStreamWriter.histogram``); ``composite``: a composite.CompositeTarget that is handed every plane
    (``PlaneStreamWriter.composite``)."""
    if image.ndim != 5:
        raise ValueError(f"expected a 5-D TCZYX array, got {tuple(image.shape)}")
    on_device = hasattr(image, 'data_ptr')
    dtype = np.dtype(str(image.dtype).replace('torch.', '')) if on_device else image.dtype
    shape = tuple(int(v) for v in image.shape)
    shapes = create_store(path, shape, dtype, pixel_size_um=pixel_size_um, dz_um=dz_um, channel_names=channel_names,
                          channel_colors=channel_colors, num_levels=num_levels, chunks=chunks, name=name,
                          compression=compression, pyramid_method=pyramid_method)
    t_, c_, z_ = shape[:3]
    coords = [(t, c, z) for t in range(t_) for c in range(c_) for z in range(z_)]
    planes = image.reshape((-1,) + shape[3:])
    if len(shapes) == 1 and not on_device and compression != 'blosc' and histogram is None and composite is None:
        write_plane_levels(path, [planes], coords, chunks, compression)
        return path
    import torch
    if not on_device:
        from . import native
        native.lib()   # fail loudly: the pyramid is a device kernel, there is no host decimation
        device = device if device is not None else 'cuda:0'
    batch = max(1, (1 << 30) // max(1, shape[3] * shape[4] * dtype.itemsize))
    with PlaneStreamWriter(path, shapes, dtype, chunks=chunks, batch=batch, compression=compression,
                           device=planes.device if on_device else device, pyramid_method=pyramid_method) as writer:
        writer.histogram = histogram
        writer.composite = composite
        for b0 in range(0, len(coords), batch):
            part = planes[b0:b0 + batch]
            dst = writer.acquire(len(part))
            dst.copy_(part if on_device else torch.from_numpy(np.ascontiguousarray(part)), non_blocking=False)
            writer.submit(coords[b0:b0 + batch])
    return path


def depth_labels(channel_names: Sequence[str], guide: Optional[str] = None) -> List[str]:
    """Channel labels of a depth store: ``depth(<guide>)`` alone with a guide channel, else ``depth(<name>)`` per channel."""
    return [f'depth({guide})'] if guide is not None else [f'depth({n})' for n in channel_names]


def write_depth_store(path: str, depth, *, num_z: int, labels: Sequence[str], pixel_size_um: float, dz_um: float = 1.0,
                      num_levels: int = 1, chunks=(1, 1, 1, 512, 512), name: str = 'depth', compression: str = 'zlib',
                      device=None) -> str:
    """The depth map of a best-focus projection as an OME-Zarr image: ``depth`` (1, K, 1, Y, X) uint8 / uint16 (numpy or a
    device tensor) holds z* + 1 per voxel, 0 = uncovered.  The levels above 0 are always the NEAREST decimation (a mean of
    depths is no depth) and every channel's window is 0 ... ``num_z``, whatever the run's pyramid method and contrast limits.
    A numpy array with a host codec is decimated and written on the host; everything else goes through ``write_ome_zarr``."""
    if depth.ndim != 5 or depth.shape[0] != 1 or depth.shape[2] != 1 or depth.shape[1] != len(labels):
        raise ValueError(f"expected a (1, {len(labels)}, 1, Y, X) depth array, got {tuple(depth.shape)}")
    if str(depth.dtype).replace('torch.', '') not in ('uint8', 'uint16'):
        raise ValueError(f"the depth plane is uint8 or uint16, got {depth.dtype}")
    colors = [0xFFFFFF] * len(labels)
    if not hasattr(depth, 'data_ptr') and compression in HOST_CODECS:
        shape = tuple(int(v) for v in depth.shape)
        shapes = create_store(path, shape, depth.dtype, pixel_size_um=pixel_size_um, dz_um=dz_um, channel_names=labels,
                              channel_colors=colors, num_levels=num_levels, chunks=chunks, name=name, compression=compression)
        levels = [np.ascontiguousarray(depth.reshape((-1,) + shape[3:]))]
        for shp in shapes[1:]:      # index 2 o + 1 of the level before (Scaler.nearest, as sq_downsample2)
            levels.append(np.ascontiguousarray(levels[-1][:, 1::2, 1::2][:, :shp[3], :shp[4]]))
        write_plane_levels(path, levels, [(0, c, 0) for c in range(shape[1])], chunks, compression)
    else:
        write_ome_zarr(path, depth, pixel_size_um=pixel_size_um, dz_um=dz_um, channel_names=labels, channel_colors=colors,
                       num_levels=num_levels, chunks=chunks, name=name, compression=compression, device=device,
                       pyramid_method='nearest')
    set_channel_windows(path, [(0, int(num_z))] * len(labels))
    return path


class PlaneStreamWriter(SlotRingWriter):
    """Streams fused planes from the device into a store made by ``create_store`` (the slot ring and its protocol:
    ``planewriter.SlotRingWriter``).  With compression 'blosc' the chunks are encoded on the device (csrc/blosc.hip) and the
    writer thread writes one file per non-empty chunk; otherwise it fans the planes' chunks out to the compression threads."""
    thread_name = 'zarr-writer'

    def __init__(self, path: str, shapes: Sequence[tuple], dtype, *, chunks=(1, 1, 1, 512, 512), batch: int = 1,
                 compression: str = 'zlib', level: int = 1, device='cuda:0', workers: Optional[int] = None, slots: int = 2,
                 buffers=None, row_offset: int = 0, level_heights: Optional[Sequence[int]] = None, canvas_arena=None,
                 pyramid_method: str = 'nearest'):
        from concurrent.futures import ThreadPoolExecutor
        self.path, self.chunks, self.compression, self.level = path, tuple(chunks), compression, level
        self.dtype = np.dtype(dtype)
        # a writer of one row band: ``shapes`` are the band's level shapes, chunks land ``row_offset`` level-0 rows down
        self.row_offset, self.level_heights = int(row_offset), (None if level_heights is None else list(level_heights))
        self._init_ring(shapes, dtype, batch=batch, device=device, slots=slots, buffers=buffers, canvas_arena=canvas_arena,
                        pyramid_method=pyramid_method, encoded=compression == 'blosc')
        self._pool = ThreadPoolExecutor(max_workers=workers if workers is not None else min(32, os.cpu_count() or 4))
        self._thread.start()

    def _make_encoder(self, lv: int, yx, device):
        from . import native
        return native.BloscBuffers(self.batch, yx[0], yx[1], self.dtype, *self._chunk_yx(lv, yx), device)

    def _encode(self, planes, enc) -> None:
        from . import native
        native.blosc_encode_planes(planes, enc.geometry[4], enc.geometry[5], enc)

    def _overflow_message(self) -> str:
        return "sq_blosc_encode_planes: output buffer too small"

    def _target(self) -> tuple:
        return self.path, self.row_offset, self.level_heights

    def _write_planes(self, slot: int, coords: Sequence[tuple], target) -> None:
        path, row_offset, level_heights = target
        levels = [h.numpy() for h in self._host[slot]]
        self.bytes_written += write_plane_levels(path, levels, coords, self.chunks, self.compression, self.level, pool=self._pool,
                                                 row_offset=row_offset, level_heights=level_heights)

    def _shutdown(self, joined: bool) -> None:
        self._pool.shutdown(wait=True)

    def _chunk_yx(self, lv: int, level_yx) -> tuple:
        """Chunk shape of pyramid level ``lv`` in the STORE: zarr clamps a chunk dimension to the array's -- the full
        level's, also when this writer holds only a row band of it."""
        full_h = level_yx[0] if self.level_heights is None else int(self.level_heights[lv])
        return min(self.chunks[3], full_h), min(self.chunks[4], level_yx[1])

    def _write_streams(self, slot: int, coords: Sequence[tuple], target, totals) -> None:
        """Blosc mode: the slot's packed frames are on the host; write one file per non-empty chunk."""
        path, row_offset, _ = target
        # one native call per pyramid level (native.write_files: open / write / close on native threads, straight from the
        # page-locked frame buffer): the paths and the directories are worked out here, a few hundred directories per batch
        from . import native
        written = 0
        for lv, (enc, (frames, offsets, _)) in enumerate(zip(self._enc[slot], self._host[slot])):
            n_planes_geo, h, w, _, cy, cx = enc.geometry
            ncy, ncx = -(-h // cy), -(-w // cx)
            y_off = row_offset >> lv
            cyf = cy
            if y_off % cyf:
                raise ValueError(f"row band at level-0 row {row_offset} does not start on a chunk row of level {lv}")
            off = offsets.numpy()
            per_plane = ncy * ncx
            sizes = np.diff(off[:len(coords) * per_plane + 1])
            keep = np.nonzero(sizes > 0)[0]
            if not len(keep):
                continue
            paths = []
            made = set()
            for k in keep.tolist():
                i, rem = divmod(k, per_plane)
                iy, ix = divmod(rem, ncx)
                t, c, z = coords[i]
                cdir = os.path.join(path, str(lv), str(t), str(c), str(z), str(y_off // cyf + iy))
                if cdir not in made:
                    os.makedirs(cdir, exist_ok=True)
                    made.add(cdir)
                paths.append(os.path.join(cdir, str(ix)))
            # the kept chunks' byte ranges: frames are packed densely, empty chunks take no bytes, so consecutive kept chunks are
            # contiguous in the buffer and [off[k], off[k + 1]) for the kept k is one non-decreasing offset list
            starts = off[keep]
            ends = off[keep + 1]
            if len(keep) > 1 and not np.array_equal(starts[1:], ends[:-1]):
                raise RuntimeError("blosc frames are not packed densely")
            data_offsets = np.concatenate([starts, ends[-1:]]).astype(np.int64)
            written += native.write_files(paths, frames.numpy(), data_offsets, n_threads=self._pool._max_workers)
        self.bytes_written += written

    def retarget(self, path: str, row_offset: int = 0, level_heights: Optional[Sequence[int]] = None) -> None:
        """The planes submitted FROM NOW ON belong to another store of the same geometry (the next well, the next timepoint): what
        is still in flight keeps the target it was submitted with.  One writer then serves a whole run, and the chunks of region k
        reach the disk while region k + 1 is read, registered and fused (``drain`` before anything reads the stores)."""
        self.path = path
        self.row_offset, self.level_heights = int(row_offset), (None if level_heights is None else list(level_heights))

    def matches(self, shapes: Sequence[tuple], dtype, batch: int, compression: str, chunks, pyramid_method: str = 'nearest') -> bool:
        """Can this writer take planes of these level shapes (its buffers are sized for one geometry)?"""
        from . import native
        yx = [tuple(s[3:]) for s in shapes]
        return (self._thread.is_alive() and self.batch == int(batch) and self.compression == compression and self.chunks == tuple(chunks)
                and self.pyramid_method == pyramid_method
                and [tuple(t.shape[1:]) for t in self._dev[0]] == yx
                and self._dev[0][0].dtype == native.torch_dtype_of(np.dtype(dtype).type))
