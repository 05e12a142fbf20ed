"""Minimal OME-TIFF writer (uncompressed BigTIFF, one IFD per (t, c, z) plane, OME-XML in the
first ImageDescription) for the ``.ome.tiff`` output format.

The reference writes this format through aicsimageio's OmeTiffWriter (stitcher.py:742-765:
dim_order TCZYX, channel names, RGB channel colours, physical pixel sizes).  aicsimageio is not on
the hot path and absent offline; this is the package-free equivalent ("next" row 8(f)1).

``--ome-tiff-layout pyramid`` writes the OME-TIFF 6 pyramid instead: tiled planes, Adobe-deflate tiles with the horizontal
predictor encoded ON THE DEVICE (csrc/deflate.hip) -- or, for uint8 planes and ``--ome-tiff-compression jpeg``, baseline JPEG
tiles (TIFF Compression 7, csrc/jpeg.hip; the stream is stated in jpegtile.py) --, reduced levels in SubIFDs.  ``PyramidTiff``
is the container (a BigTIFF that is appended to while planes stream in, its IFDs written at close), ``PyramidTiffWriter``
streams planes into it with ``omezarr.PlaneStreamWriter``'s protocol, ``read_pyramid_tiff`` reads it back for the tests
(JPEG tiles through Pillow), ``read_tile_streams`` returns the tiles' raw bytes.
"""
from __future__ import annotations

import os
import struct
import zlib
from typing import Optional, Sequence
from xml.sax.saxutils import escape

import numpy as np

from .planewriter import SlotRingWriter

_OME_TYPES = {np.dtype('uint8'): 'uint8', np.dtype('uint16'): 'uint16', np.dtype('float32'): 'float'}


def ome_xml(shape, dtype, channel_names: Sequence[str], channel_colors: Sequence[int], pixel_size_um: float,
            dz_um: float, name: str) -> str:
    t, c, z, y, x = (int(v) for v in shape)
    chans = []
    for i in range(c):
        label = escape(channel_names[i]) if i < len(channel_names) else f'Channel:{i}'
        rgb = channel_colors[i] if i < len(channel_colors) else 0xFFFFFF
        # OME colour is a signed 32-bit RGBA
        rgba = ((rgb & 0xFFFFFF) << 8) | 0xFF
        if rgba >= 2 ** 31:
            rgba -= 2 ** 32
        chans.append(f'<Channel ID="Channel:0:{i}" Name="{label}" SamplesPerPixel="1" Color="{rgba}"><LightPath/></Channel>')
    planes = ''.join(f'<TiffData FirstT="{ti}" FirstC="{ci}" FirstZ="{zi}" IFD="{(ti * c + ci) * z + zi}" PlaneCount="1"/>'
                     for ti in range(t) for ci in range(c) for zi in range(z))
    return ('<?xml version="1.0" encoding="UTF-8"?>'
            '<OME xmlns="http://www.openmicroscopy.org/Schemas/OME/2016-06" '
            'xmlns:xsi="http://www.w3.org/2001/XMLSchema-instance" '
            'xsi:schemaLocation="http://www.openmicroscopy.org/Schemas/OME/2016-06 '
            'http://www.openmicroscopy.org/Schemas/OME/2016-06/ome.xsd">'
            f'<Image ID="Image:0" Name="{escape(name)}">'
            f'<Pixels ID="Pixels:0" DimensionOrder="XYZCT" Type="{_OME_TYPES[np.dtype(dtype)]}" '
            f'SizeX="{x}" SizeY="{y}" SizeZ="{z}" SizeC="{c}" SizeT="{t}" '
            f'PhysicalSizeX="{pixel_size_um}" PhysicalSizeXUnit="µm" PhysicalSizeY="{pixel_size_um}" '
            f'PhysicalSizeYUnit="µm" PhysicalSizeZ="{dz_um}" PhysicalSizeZUnit="µm" BigEndian="false">'
            + ''.join(chans) + planes + '</Pixels></Image></OME>')


def write_ome_tiff(path: str, image: np.ndarray, *, pixel_size_um: float, dz_um: float = 1.0,
                   channel_names: Sequence[str] = (), channel_colors: Sequence[int] = (), name: str = 'stitched') -> str:
    """Write a (T, C, Z, Y, X) uint8/uint16/float32 array as an OME-TIFF (BigTIFF)."""
    if image.ndim != 5:
        raise ValueError(f"expected a 5-D TCZYX array, got {image.shape}")
    dt = np.dtype(image.dtype)
    if dt not in _OME_TYPES:
        raise ValueError(f"unsupported dtype {dt}")
    t, c, z, y, x = image.shape
    desc = ome_xml(image.shape, dt, channel_names, channel_colors, pixel_size_um, dz_um, name).encode('utf-8') + b'\0'
    plane_bytes = y * x * dt.itemsize
    n_planes = t * c * z
    sample_format = 3 if dt.kind == 'f' else 1

    def ifd(strip_off, desc_off, next_off):
        ents = [(256, 16, 1, x), (257, 16, 1, y), (258, 3, 1, dt.itemsize * 8), (259, 3, 1, 1), (262, 3, 1, 1)]
        if desc_off is not None:
            ents.append((270, 2, len(desc), desc_off))
        ents += [(273, 16, 1, strip_off), (277, 3, 1, 1), (278, 16, 1, y), (279, 16, 1, plane_bytes),
                 (339, 3, 1, sample_format)]
        ents.sort()
        out = [struct.pack('<Q', len(ents))]
        for tag, typ, cnt, val in ents:
            out.append(struct.pack('<HHQQ', tag, typ, cnt, val))
        out.append(struct.pack('<Q', next_off))
        return b''.join(out)

    ifd_size0 = 8 + 11 * 20 + 8
    ifd_size = 8 + 10 * 20 + 8
    # layout: header(16) | description | IFD0 | IFD1.. | planes
    desc_off = 16
    ifd0_off = (desc_off + len(desc) + 7) & ~7
    data_off = ifd0_off + ifd_size0 + (n_planes - 1) * ifd_size
    data_off = (data_off + 15) & ~15
    with open(path, 'wb') as fh:
        fh.write(struct.pack('<2sHHHQ', b'II', 43, 8, 0, ifd0_off))
        fh.write(desc)
        fh.write(b'\0' * (ifd0_off - desc_off - len(desc)))
        off = ifd0_off
        for p in range(n_planes):
            size = ifd_size0 if p == 0 else ifd_size
            nxt = off + size if p + 1 < n_planes else 0
            fh.write(ifd(data_off + p * plane_bytes, desc_off if p == 0 else None, nxt))
            off += size
        fh.write(b'\0' * (data_off - off))
        flat = image.reshape(n_planes, y, x)
        for p in range(n_planes):
            fh.write(np.ascontiguousarray(flat[p]).astype(dt.newbyteorder('<'), copy=False).tobytes())
    return path


def read_ome_tiff(path: str):
    """Planes and OME-XML back from a file written by write_ome_tiff (tests)."""
    with open(path, 'rb') as fh:
        buf = fh.read()
    bo, ver, osz, _, off = struct.unpack('<2sHHHQ', buf[:16])
    assert bo == b'II' and ver == 43 and osz == 8
    planes, xml = [], None
    while off:
        (n,) = struct.unpack('<Q', buf[off:off + 8])
        tags = {}
        for i in range(n):
            tag, typ, cnt, val = struct.unpack('<HHQQ', buf[off + 8 + 20 * i: off + 28 + 20 * i])
            tags[tag] = (typ, cnt, val)
        w, h, bits = tags[256][2], tags[257][2], tags[258][2]
        fmt = tags.get(339, (3, 1, 1))[2]
        dt = np.dtype('<f4') if fmt == 3 else np.dtype(f'<u{bits // 8}')
        planes.append(np.frombuffer(buf, dtype=dt, count=w * h, offset=tags[273][2]).reshape(h, w))
        if 270 in tags:
            xml = buf[tags[270][2]:tags[270][2] + tags[270][1] - 1].decode('utf-8')
        (off,) = struct.unpack('<Q', buf[off + 8 + 20 * n: off + 16 + 20 * n])
    return planes, xml


# ---------------------------------------------------------------------------------------------- the pyramid layout
TIFF_LAYOUTS = ('planes', 'pyramid')
TIFF_COMPRESSIONS = ('deflate', 'none', 'jpeg')
PREDICTOR_HORIZONTAL = 2
_TIFF_COMPRESSION_TAG = {'none': 1, 'deflate': 8, 'jpeg': 7}
_COMPRESSION_NAMES = "'deflate' or 'none' (or 'jpeg', for uint8 planes)"


def check_tiff_options(layout: str, compression: str, output_format: str, chunks=None, quality=None) -> tuple:
    """-> (layout, compression) validated; the pyramid needs .ome.tiff output and tile sides that are multiples of 16 (TIFF 6);
    'jpeg' is a codec of TIFF tiles only (and ``quality``, when given, lies in 1..100)."""
    if layout not in TIFF_LAYOUTS:
        raise ValueError(f"ome_tiff_layout must be 'planes' or 'pyramid', got {layout!r}")
    if compression not in TIFF_COMPRESSIONS:
        raise ValueError(f"ome_tiff_compression must be {_COMPRESSION_NAMES}, got {compression!r}")
    if quality is not None:
        from . import jpegtile
        jpegtile.check_quality(quality)
    if compression == 'jpeg' and str(output_format).endswith('.zarr'):
        raise ValueError("ome_tiff_compression='jpeg' is a codec of TIFF tiles: it needs .ome.tiff output, not an .ome.zarr store")
    if compression == 'jpeg' and layout != 'pyramid':      # (the planes layout writes raw strips whatever the codec: say so for a lossy one)
        raise ValueError("ome_tiff_compression='jpeg' needs ome_tiff_layout='pyramid' (the planes layout writes uncompressed strips)")
    if layout == 'pyramid':
        if str(output_format).endswith('.zarr'):
            raise ValueError("ome_tiff_layout='pyramid' needs .ome.tiff output (an .ome.zarr store has its own pyramid)")
        check_tile_shape((chunks or (1, 1, 1, 512, 512))[3:5])
    return layout, compression


def check_jpeg_dtype(dtype) -> None:
    if np.dtype(dtype) != np.dtype('uint8'):
        raise ValueError(f"ome_tiff_compression='jpeg' holds uint8 planes (baseline JPEG is 8 bits), got {np.dtype(dtype)}; "
                         f"write this data with 'deflate'")


def jpeg_buffers_plane_bytes(h: int, w: int, num_levels: int, tile, slots: int = 2) -> int:
    """Device bytes the JPEG encoder's packed-stream buffers (native.JpegBuffers.bound: raw tiles + a header each) add per
    plane of a writer's batch, over its levels and slots -- what the stream writer's batch is sized with."""
    from . import jpegtile
    th, tw = (int(v) for v in tile)
    total = 0
    for _ in range(max(1, int(num_levels))):
        total += -(-h // th) * -(-w // tw) * (th * tw + jpegtile.HEADER_BYTES + 2)
        h, w = h // 2, w // 2
        if h < 1 or w < 1:
            break
    return slots * total


def check_tile_shape(tile) -> tuple:
    th, tw = (int(v) for v in tile)
    if th < 16 or tw < 16 or th % 16 or tw % 16:
        raise ValueError(f"TIFF tile sides must be multiples of 16, got {th} x {tw}")
    return th, tw


class PyramidTiff:
    """A little-endian BigTIFF that is appended to: the 16-byte header, then the encoded tiles of whatever is appended, in arrival
    order; ``close`` writes the TileOffsets / TileByteCounts arrays, the IFDs and the OME-XML behind them and patches the header's
    first-IFD offset.  One top-level IFD per (t, c, z) plane, chained in the order (t C + c) Z + z, the OME-XML in the first one's
    ImageDescription; the reduced levels of a plane are SubIFDs (tag 330) of its IFD.  Tiles are always full; a tile of zeros (size
    0 when appended) points at ONE zero-tile stream written when the file is opened -- so does every tile of a plane that is
    never appended."""

    def __init__(self, path: str, shapes: Sequence[tuple], dtype, *, tile=(512, 512), compression: str = 'deflate', xml: str = '',
                 quality: int = 90):
        from . import jpegtile
        self.path = path
        self.dtype = np.dtype(dtype)
        if self.dtype not in (np.dtype('uint8'), np.dtype('uint16')):
            raise ValueError(f"the pyramid layout holds uint8 or uint16 planes, got {self.dtype}")
        if compression not in TIFF_COMPRESSIONS:
            raise ValueError(f"compression must be {_COMPRESSION_NAMES}, got {compression!r}")
        self.quality = jpegtile.check_quality(quality)
        if compression == 'jpeg':
            check_jpeg_dtype(self.dtype)
        self.th, self.tw = check_tile_shape(tile)
        self.compression = compression
        self.shapes = [tuple(int(v) for v in s) for s in shapes]
        t, c, z = self.shapes[0][:3]
        self.n_planes = t * c * z
        self.xml = xml
        self.grid = [(-(-s[3] // self.th), -(-s[4] // self.tw)) for s in self.shapes]
        zero = bytes(self.th * self.tw * self.dtype.itemsize)
        if compression == 'jpeg':       # (a tile of zeros is not the cheapest JPEG block -- grey 128 is -- but it is one stream)
            self.zero_tile = jpegtile.encode_tile(np.zeros((self.th, self.tw), np.uint8), self.quality)
        else:
            self.zero_tile = zlib.compress(zero, 1) if compression == 'deflate' else zero
        self._fh = open(path, 'wb')
        self._fh.write(struct.pack('<2sHHHQ', b'II', 43, 8, 0, 0))
        self._zero_at = 16
        self._fh.write(self.zero_tile)
        self._pos = 16 + len(self.zero_tile)
        # every tile points at the zero tile until its bytes arrive
        self.offsets = [np.full((self.n_planes, gy * gx), self._zero_at, np.uint64) for gy, gx in self.grid]
        self.counts = [np.full((self.n_planes, gy * gx), len(self.zero_tile), np.uint64) for gy, gx in self.grid]
        self.tiles_written = 0
        self.bytes_written = self._pos
        self.closed = False

    def plane_index(self, t: int, c: int, z: int) -> int:
        _, nc, nz = self.shapes[0][:3]
        return (int(t) * nc + int(c)) * nz + int(z)

    def append(self, level: int, planes: Sequence[int], data, sizes) -> int:
        """The tiles of ``planes`` (indices) at ``level``: ``sizes`` [len(planes) * tiles per plane] byte counts in the order plane,
        tile row, tile column (0 = a tile of zeros), ``data`` their bytes packed densely in that order.  One write."""
        sizes = np.asarray(sizes, dtype=np.uint64).reshape(len(planes), -1)
        if sizes.shape[1] != self.offsets[level].shape[1]:
            raise ValueError(f"level {level} has {self.offsets[level].shape[1]} tiles per plane, got {sizes.shape[1]}")
        total = int(sizes.sum())
        view = memoryview(data).cast('B')[:total]
        if len(view) != total:
            raise ValueError("fewer bytes than the sizes add up to")
        starts = self._pos + np.concatenate([[0], np.cumsum(sizes.reshape(-1))[:-1]]).astype(np.uint64).reshape(sizes.shape)
        if total:
            self._fh.write(view)
        real = sizes > 0
        for i, p in enumerate(planes):
            self.offsets[level][p][real[i]] = starts[i][real[i]]
            self.counts[level][p][real[i]] = sizes[i][real[i]]
        self._pos += total
        self.tiles_written += int(real.sum())
        self.bytes_written += total
        return total

    def append_planes(self, level: int, planes: Sequence[int], arrays: np.ndarray) -> int:
        """Host planes [m, y, x] of ``level`` cut into full tiles here (compression 'none', 'deflate' with host zlib -- the
        streams the device encoder's stand in for in the CPU tests -- or 'jpeg' through jpegtile.encode_tile, the very streams of
        the device encoder): zero tiles take no bytes."""
        from . import jpegtile
        gy, gx = self.grid[level]
        m, y, x = arrays.shape
        pad = np.zeros((m, gy * self.th, gx * self.tw), self.dtype.newbyteorder('<'))
        pad[:, :y, :x] = arrays
        tiles = pad.reshape(m, gy, self.th, gx, self.tw).transpose(0, 1, 3, 2, 4).reshape(m * gy * gx, self.th, self.tw)
        chunks, sizes = [], np.zeros(len(tiles), np.uint64)
        for i, tile in enumerate(tiles):
            if not tile.any():
                continue
            if self.compression == 'deflate':
                pred = tile.copy()
                pred[:, 1:] = tile[:, 1:] - tile[:, :-1]
                raw = zlib.compress(pred.tobytes(), 1)
            elif self.compression == 'jpeg':
                raw = jpegtile.encode_tile(tile, self.quality)
            else:
                raw = tile.tobytes()
            chunks.append(raw)
            sizes[i] = len(raw)
        return self.append(level, planes, b''.join(chunks), sizes)

    def _ifd(self, level: int, plane: int, place, sub_offsets, next_off: int, desc) -> bytes:
        s = self.shapes[level]
        n_tiles = self.offsets[level].shape[1]
        ents = [(254, 4, 1, 1 if level else 0), (256, 4, 1, s[4]), (257, 4, 1, s[3]), (258, 3, 1, self.dtype.itemsize * 8),
                (259, 3, 1, _TIFF_COMPRESSION_TAG[self.compression]), (262, 3, 1, 1), (277, 3, 1, 1),
                (322, 4, 1, self.tw), (323, 4, 1, self.th), (339, 3, 1, 1)]
        if self.compression == 'deflate':
            ents.append((317, 3, 1, PREDICTOR_HORIZONTAL))
        if desc is not None:
            ents.append((270, 2, len(desc), place(desc)))
        for tag, arr in ((324, self.offsets[level][plane]), (325, self.counts[level][plane])):
            ents.append((tag, 16, n_tiles, int(arr[0]) if n_tiles == 1 else place(arr.astype('<u8').tobytes())))
        if sub_offsets:
            ents.append((330, 18, len(sub_offsets), sub_offsets[0] if len(sub_offsets) == 1 else
                         place(np.asarray(sub_offsets, '<u8').tobytes())))
        ents.sort()
        return struct.pack('<Q', len(ents)) + b''.join(struct.pack('<HHQQ', *e) for e in ents) + struct.pack('<Q', next_off)

    def close(self) -> dict:
        """Arrays, IFDs, OME-XML, header.  Returns the counts the ``[ome-tiff]`` line prints."""
        if self.closed:
            return self.stats
        base = (self._pos + 15) & ~15
        tail = bytearray()

        def place(blob: bytes) -> int:      # out-of-line data of an entry, 8-byte aligned
            tail.extend(b'\0' * (-len(tail) % 8))
            at = base + len(tail)
            tail.extend(blob)
            return at

        desc = self.xml.encode('utf-8') + b'\0'
        n_levels = len(self.shapes)
        patches = []                        # position in `tail` of every top-level IFD's next pointer
        first_ifd = 0
        for p in range(self.n_planes):
            subs = []
            for lv in range(1, n_levels):
                blob = self._ifd(lv, p, place, None, 0, None)
                subs.append(place(blob))
            body = self._ifd(0, p, place, subs, 0, desc if p == 0 else None)
            at = place(body)        # (behind its out-of-line data; the IFD before it learns the offset now)
            if p == 0:
                first_ifd = at
            else:
                struct.pack_into('<Q', tail, patches[-1], at)
            patches.append(at - base + len(body) - 8)
        self._fh.write(b'\0' * (base - self._pos))
        self._fh.write(tail)
        self._fh.seek(8)
        self._fh.write(struct.pack('<Q', first_ifd))
        self._fh.close()
        self.closed = True
        total_tiles = sum(self.n_planes * gy * gx for gy, gx in self.grid)
        raw = sum(self.n_planes * s[3] * s[4] * self.dtype.itemsize for s in self.shapes)
        self.bytes_written = base + len(tail)
        self.stats = {'levels': n_levels, 'tile': (self.th, self.tw), 'tiles': total_tiles,
                      'zero_tiles': total_tiles - self.tiles_written, 'raw_bytes': raw, 'written_bytes': self.bytes_written,
                      'compression': self.compression, 'quality': self.quality if self.compression == 'jpeg' else None}
        return self.stats


def tiff_summary(path: str, stats: dict) -> str:
    return (f"[ome-tiff] {os.path.basename(path)}: {stats['levels']} levels, tiles {stats['tile'][0]} x {stats['tile'][1]}, "
            f"{stats['tiles']} tiles ({stats['zero_tiles']} zero), {stats['raw_bytes']} -> {stats['written_bytes']} bytes"
            + (f", jpeg quality {stats['quality']}" if stats.get('compression') == 'jpeg' else ''))


def _parse_ifd(buf, off: int):
    (n,) = struct.unpack_from('<Q', buf, off)
    sizes = {1: 1, 2: 1, 3: 2, 4: 4, 16: 8, 18: 8}
    tags = {}
    for i in range(n):
        tag, typ, cnt, val = struct.unpack_from('<HHQQ', buf, off + 8 + 20 * i)
        width = sizes[typ] * cnt
        raw = bytes(buf[off + 20 + 20 * i: off + 20 + 20 * i + width]) if width <= 8 else bytes(buf[val:val + width])
        if typ == 2:
            value = raw
        else:
            value = np.frombuffer(raw, {1: '<u1', 3: '<u2', 4: '<u4', 16: '<u8', 18: '<u8'}[typ]).astype(np.int64)
        tags[tag] = (typ, cnt, value)
    (nxt,) = struct.unpack_from('<Q', buf, off + 8 + 20 * n)
    return tags, nxt


def _read_tiled_plane(buf, tags) -> np.ndarray:
    val = lambda t: int(tags[t][2][0])
    w, h, bits, comp, tw, th = val(256), val(257), val(258), val(259), val(322), val(323)
    pred = val(317) if 317 in tags else 1
    dt = np.dtype(f'<u{bits // 8}')
    gy, gx = -(-h // th), -(-w // tw)
    offs, cnts = tags[324][2], tags[325][2]
    assert len(offs) == len(cnts) == gy * gx
    full = np.zeros((gy * th, gx * tw), dt)
    for k in range(gy * gx):
        raw = bytes(buf[int(offs[k]):int(offs[k]) + int(cnts[k])])
        if comp == 7:
            from . import jpegtile
            tile = jpegtile.decode_tile(raw)      # (Pillow; RuntimeError where it is absent)
            if tile.shape != (th, tw) or dt != np.dtype('uint8'):
                raise ValueError(f"JPEG tile of {tile.shape}, the IFD says {th} x {tw} {dt}")
        else:
            if comp == 8:
                raw = zlib.decompress(raw)
            elif comp != 1:
                raise ValueError(f"compression {comp}")
            tile = np.frombuffer(raw, dt).reshape(th, tw)
        if pred == 2:
            tile = np.cumsum(tile, axis=1, dtype=dt)
        iy, ix = divmod(k, gx)
        full[iy * th:(iy + 1) * th, ix * tw:(ix + 1) * tw] = tile
    return full[:h, :w]


def read_pyramid_structure(path: str):
    """-> (file bytes, [top-level IFD tags, each with key 'sub': the tags of its SubIFDs]) of a BigTIFF; a tag's entry is
    (type, count, values)."""
    with open(path, 'rb') as fh:
        buf = fh.read()
    bo, ver, osz, _, off = struct.unpack('<2sHHHQ', buf[:16])
    if bo != b'II' or ver != 43 or osz != 8:
        raise ValueError(f"{path}: not a little-endian BigTIFF")
    ifds = []
    while off:
        tags, off = _parse_ifd(buf, off)
        tags['sub'] = [_parse_ifd(buf, int(o))[0] for o in tags[330][2]] if 330 in tags else []
        ifds.append(tags)
    return buf, ifds


def read_tile_streams(path: str):
    """The raw bytes of every tile of a file written through ``PyramidTiff`` (tests): ``streams[l][p]`` is the list of the tile
    streams of plane p (IFD order) at level l, in tile order; a tile of zeros shows the shared zero-tile stream."""
    buf, ifds = read_pyramid_structure(path)
    levels = [[] for _ in range(1 + len(ifds[0]['sub']))]
    for tags in ifds:
        for lv, t in enumerate([tags] + tags['sub']):
            levels[lv].append([bytes(buf[int(o):int(o) + int(c)]) for o, c in zip(t[324][2], t[325][2])])
    return levels


def read_pyramid_tiff(path: str):
    """A file written through ``PyramidTiff`` back into memory (tests): -> (levels, xml) with ``levels[l]`` the list of the planes
    of level l in IFD order.  Parses the structure, inflates with ``zlib.decompress``, undoes the predictor with numpy."""
    buf, ifds = read_pyramid_structure(path)
    n_levels = 1 + len(ifds[0]['sub'])
    levels = [[] for _ in range(n_levels)]
    xml = None
    for tags in ifds:
        if 270 in tags and xml is None:
            xml = tags[270][2][:-1].decode('utf-8')
        for lv, t in enumerate([tags] + tags['sub']):
            levels[lv].append(_read_tiled_plane(buf, t))
    return levels, xml


class PyramidTiffWriter(SlotRingWriter):
    """Streams fused planes from the device into a ``PyramidTiff`` through ``planewriter.SlotRingWriter``'s slot ring and protocol
    (acquire / submit / retarget / matches / drain / close; ``histogram`` and ``composite`` hooks), so that
    ``Stitcher.stitch_planes`` drives it like ``omezarr.PlaneStreamWriter``.  With compression 'deflate' or 'jpeg' submit() runs
    the tile encoder (sq_deflate_encode_planes, predictor 2; sq_jpeg_encode_planes at ``quality``, uint8 planes only) behind the
    fusion, and the writer thread appends the packed streams with one write per level per batch, straight from the
    page-locked buffer.  'none': the planes are copied out and cut into tiles on the host.  ``meta``: the keyword arguments of
    ``ome_xml`` but shape and dtype (pixel_size_um, dz_um, channel_names, channel_colors, name)."""
    thread_name = 'tiff-writer'

    def __init__(self, path: str, shapes: Sequence[tuple], dtype, *, meta: dict, chunks=(1, 1, 1, 512, 512), batch: int = 1,
                 compression: str = 'deflate', device='cuda:0', slots: int = 2, buffers=None, canvas_arena=None,
                 pyramid_method: str = 'nearest', verbose: bool = True, quality: int = 90):
        from . import jpegtile
        self.chunks = tuple(chunks)
        self.tile = check_tile_shape(self.chunks[3:5])
        if compression not in TIFF_COMPRESSIONS:
            raise ValueError(f"compression must be {_COMPRESSION_NAMES}, got {compression!r}")
        self.quality = jpegtile.check_quality(quality)
        if compression == 'jpeg':
            check_jpeg_dtype(dtype)
        self.compression = compression
        self.shapes = [tuple(int(v) for v in s) for s in shapes]
        self.dtype = np.dtype(dtype)
        self.row_offset = 0
        self.verbose = verbose
        self._init_ring(self.shapes, self.dtype, batch=batch, device=device, slots=slots, buffers=buffers, canvas_arena=canvas_arena,
                        pyramid_method=pyramid_method, encoded=compression in ('deflate', 'jpeg'))
        self._file = None
        self._open(path, meta)
        self._thread.start()

    def _make_encoder(self, lv: int, yx, device):
        from . import native
        if self.compression == 'jpeg':
            return native.JpegBuffers(self.batch, yx[0], yx[1], self.tile[0], self.tile[1], device)
        return native.DeflateBuffers(self.batch, yx[0], yx[1], self.dtype, self.tile[0], self.tile[1], device)

    def _encode(self, planes, enc) -> None:
        from . import native
        if self.compression == 'jpeg':
            native.jpeg_encode_planes(planes, self.tile[0], self.tile[1], self.quality, enc)
        else:
            native.deflate_encode_planes(planes, self.tile[0], self.tile[1], PREDICTOR_HORIZONTAL, enc)

    def _overflow_message(self) -> str:
        from . import native
        return native.jpeg_overflow_message(self.quality) if self.compression == 'jpeg' else \
            "sq_deflate_encode_planes: output buffer too small"

    def _target(self) -> PyramidTiff:
        return self._file

    @property
    def path(self) -> str:
        return self._file.path

    def _open(self, path: str, meta: dict) -> None:
        xml = ome_xml(self.shapes[0], self.dtype, meta.get('channel_names', ()), meta.get('channel_colors', ()),
                      meta['pixel_size_um'], meta.get('dz_um', 1.0), meta.get('name', 'stitched'))
        self._file = PyramidTiff(path, self.shapes, self.dtype, tile=self.tile, compression=self.compression, xml=xml,
                                 quality=self.quality)

    def _finish(self, file: PyramidTiff) -> None:
        if file.closed:
            return
        stats = file.close()
        self.bytes_written += stats['written_bytes']
        if self.verbose:
            print(tiff_summary(file.path, stats))

    def _write_streams(self, slot: int, coords: Sequence[tuple], file: PyramidTiff, totals) -> None:
        """The slot's packed streams are on the host: append them, one write per level."""
        planes = [file.plane_index(*c) for c in coords]
        for lv, (enc, (frames, offsets, _)) in enumerate(zip(self._enc[slot], self._host[slot])):
            per_plane = enc.n_chunks // self.batch
            file.append(lv, planes, frames.numpy()[:totals[lv]], np.diff(offsets.numpy()[:len(planes) * per_plane + 1]))

    def _write_planes(self, slot: int, coords: Sequence[tuple], file: PyramidTiff) -> None:
        planes = [file.plane_index(*c) for c in coords]
        for lv, h in enumerate(self._host[slot]):
            file.append_planes(lv, planes, h.numpy()[:len(planes)])

    def _last_item(self) -> tuple:
        return None, None, None, self._file

    def _shutdown(self, joined: bool) -> None:
        if not joined and self._file is not None and not self._file.closed:      # the writer thread had died
            self._finish(self._file)

    def retarget(self, path: str, row_offset: int = 0, level_heights=None, meta: Optional[dict] = None) -> None:
        """The planes submitted FROM NOW ON belong to another file of the same geometry: the current one is finished behind what
        is still in flight, the next is opened.  (Row bands of one file are not supported: ranks take whole regions.)"""
        if row_offset or level_heights is not None:
            raise ValueError("a pyramid TIFF is written whole: no row bands")
        if meta is None:
            raise ValueError("retarget needs the next file's metadata")
        self._queue.put(self._last_item())
        self._open(path, meta)

    def matches(self, shapes: Sequence[tuple], dtype, batch: int, compression: str, chunks, pyramid_method: str = 'nearest', *,
                quality: int = 90) -> bool:
        """Can this writer take planes of these level shapes (its buffers are sized for one geometry)?"""
        return (self._thread.is_alive() and self.batch == int(batch) and self.compression == compression
                and (compression != 'jpeg' or self.quality == int(quality))
                and self.chunks == tuple(chunks) and self.pyramid_method == pyramid_method
                and self.shapes == [tuple(int(v) for v in s) for s in shapes] and self.dtype == np.dtype(dtype))


def write_pyramid_tiff(path: str, image, *, meta: dict, num_levels: int = 1, chunks=(1, 1, 1, 512, 512), compression: str = 'deflate',
                       device=None, pyramid_method: str = 'nearest', composite=None, verbose: bool = True, quality: int = 90) -> str:
    """Write a (T, C, Z, Y, X) uint8 / uint16 array (numpy, or a device tensor) as a pyramid OME-TIFF through
    ``PyramidTiffWriter``, a batch of planes at a time (what ``omezarr.write_ome_zarr`` is to a store)."""
    import torch
    from . import omezarr
    if image.ndim != 5:
        raise ValueError(f"expected a 5-D TCZYX array, got {tuple(image.shape)}")
    on_device = hasattr(image, 'data_ptr')
    dtype = np.dtype(str(image.dtype).replace('torch.', '')) if on_device else image.dtype
    shape = tuple(int(v) for v in image.shape)
    shapes = omezarr.level_shapes(shape, num_levels)
    coords = [(t, c, z) for t in range(shape[0]) for c in range(shape[1]) for z in range(shape[2])]
    planes = image.reshape((-1,) + shape[3:])
    batch = max(1, min(len(coords), (1 << 30) // max(1, shape[3] * shape[4] * dtype.itemsize)))
    with PyramidTiffWriter(path, shapes, dtype, meta=meta, chunks=chunks, batch=batch, compression=compression,
                           device=planes.device if on_device else (device if device is not None else 'cuda:0'),
                           pyramid_method=pyramid_method, verbose=verbose, quality=quality) as writer:
        writer.composite = composite
        for b0 in range(0, len(coords), batch):
            part = planes[b0:b0 + batch]
            dst = writer.acquire(len(part))
            dst.copy_(part if on_device else torch.from_numpy(np.ascontiguousarray(part)), non_blocking=False)
            writer.submit(coords[b0:b0 + batch])
    return path
