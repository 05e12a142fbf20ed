"""The rules of the device tile encoder's streams (tests/deflate_ref.py) against Python's zlib, the pyramid TIFF container
(ometiff.PyramidTiff / read_pyramid_tiff) with host-made streams, and the options of the pyramid layout.  No device."""
import os
import re
import zlib

import numpy as np
import pytest

import deflate_cases as K
import deflate_ref as R
from image_stitcher_amd import native, ometiff, omezarr, stitcher_cli
from image_stitcher_amd.stitcher import Stitcher
from image_stitcher_amd.stitcher_parameters import StitchingParameters

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def z_rle(data: bytes) -> int:
    c = zlib.compressobj(1, zlib.DEFLATED, 15, 8, zlib.Z_RLE)
    return len(c.compress(data) + c.flush())


@pytest.mark.parametrize('predictor', [1, 2])
@pytest.mark.parametrize('dtype', [np.uint8, np.uint16])
@pytest.mark.parametrize('content', K.CONTENTS)
@pytest.mark.parametrize('shape_name', [s[0] for s in K.SHAPES])
def test_reference_streams_inflate_to_the_predicted_tiles(shape_name, content, dtype, predictor):
    _, shape, t = next(s for s in K.SHAPES if s[0] == shape_name)
    planes = K.content(content, shape, dtype, seed=len(shape_name))
    streams = R.encode_planes(planes, t, t, predictor)
    want = R.expected_tiles(planes, t, t, predictor)
    n, h, w = shape
    assert len(streams) == n * -(-h // t) * -(-w // t)
    for p in range(n):      # the predicted bytes are what undoing the predictor turns back into the zero-padded tile
        for ty in range(-(-h // t)):
            for tx in range(-(-w // t)):
                i = (p * -(-h // t) + ty) * -(-w // t) + tx
                if not want[i]:
                    assert streams[i] == b'' and not planes[p, ty * t:(ty + 1) * t, tx * t:(tx + 1) * t].any()
                    continue
                assert zlib.decompress(streams[i]) == want[i]
                tile = R.unpredict(np.frombuffer(want[i], planes.dtype.newbyteorder('<')).reshape(t, t), predictor)
                part = planes[p, ty * t:(ty + 1) * t, tx * t:(tx + 1) * t]
                assert np.array_equal(tile[:part.shape[0], :part.shape[1]], part)
                assert not tile[part.shape[0]:].any() and not tile[:, part.shape[1]:].any()
                # never more than every segment stored; and within the segments' own headers of zlib's run-length strategy
                nseg = -(-len(want[i]) // R.SEG)
                assert len(streams[i]) <= 6 + 5 * nseg + len(want[i])
                assert len(streams[i]) <= z_rle(want[i]) + nseg * R.header_bytes()


@pytest.mark.parametrize('dtype', [np.uint8, np.uint16])
def test_runs_of_every_length_cross_segment_boundaries(dtype):
    planes = K.every_run_length(dtype)
    flat = planes.reshape(-1)
    starts = np.flatnonzero(np.r_[True, flat[1:] != flat[:-1]])
    lengths = np.diff(np.r_[starts, len(flat)])
    assert set(range(1, 301)) <= set(lengths.tolist())
    per_seg = R.SEG // planes.dtype.itemsize
    side = planes.shape[1]
    inside = [b for p in range(3) for b in range(p * side * side + per_seg, (p + 1) * side * side, per_seg) if b not in set(starts.tolist())]
    assert inside, 'no segment boundary falls inside a run'
    for pred in (1, 2):
        for s, w in zip(R.encode_planes(planes, side, side, pred), R.expected_tiles(planes, side, side, pred)):
            assert zlib.decompress(s) == w
    # a run of 258..261 elements: whole pieces of 258 bytes, and a rest shorter than 3 bytes goes out as literals
    esz = planes.dtype.itemsize
    for length in (258, 259, 260, 261):
        seg = np.r_[np.array([7], dtype), np.full(length, 9, dtype)].astype(planes.dtype.newbyteorder('<')).tobytes()
        toks = R.tokens(seg, esz)
        assert sum(v if k == 'run' else 1 for k, v in toks) == len(seg)
        assert all(3 <= v <= 258 and v % esz == 0 for k, v in toks if k == 'run')


def test_length_symbols_are_rfc_1951s():
    base = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
    extra = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
    for length in range(3, 259):
        s, eb, ev = R.length_symbol(length)
        assert 257 <= s <= 285 and extra[s - 257] == eb and base[s - 257] + ev == length and ev < (1 << eb) or (eb == 0 and ev == 0)


def test_the_code_length_limit_acts_on_fibonacci_counts():
    seg = K.fibonacci_segment().tobytes()
    assert all(k == 'lit' for k, _ in R.tokens(seg, 1))      # no value repeats back to back
    counts = [0] * 286
    counts[256] = 1
    for b in seg:
        counts[b] += 1
    free = R.huffman_lengths(counts, None)
    assert max(free) > 15
    assert sum(2.0 ** -l for l in free if l) == 1.0
    limited = R.huffman_lengths(counts)
    assert max(limited) == 15 and [bool(l) for l in limited] == [bool(c) for c in counts]
    assert sum(2 ** (15 - l) for l in limited if l) == 1 << 15      # a complete prefix code
    codes = R.canonical_codes(limited)
    words = sorted(format(c, f'0{l}b') for c, l in zip(codes, limited) if l)
    assert all(not b.startswith(a) for a, b in zip(words, words[1:]))
    order = sorted((s for s in range(286) if counts[s]), key=lambda s: counts[s])
    assert all(limited[a] >= limited[b] for a, b in zip(order, order[1:]))      # rarer symbols never get shorter codes
    assert zlib.decompress(R.compress_tile(seg, 1)) == seg


@pytest.mark.parametrize('predictor', [1, 2])
@pytest.mark.parametrize('dtype', [np.uint8, np.uint16])
def test_mixed_segments_are_stored_next_to_dynamic(dtype, predictor):
    planes = K.mixed_segments(dtype)
    side, esz = planes.shape[1], planes.dtype.itemsize
    tiles = [R.tile_bytes(planes[p], 0, 0, side, side, predictor) for p in range(2)]
    assert tuple(R.block_kinds(t, esz) for t in tiles) == K.MIXED_KINDS[planes.dtype.name]
    assert K.MIXED_KINDS == {'uint16': ('SD', 'DS'), 'uint8': ('SSDD', 'DDSS')}
    for t in tiles:
        assert zlib.decompress(R.compress_tile(t, esz)) == t


def test_the_code_length_limit_acts_on_uint16_fibonacci_counts():
    planes = K.fibonacci_segment_u16()
    assert planes.shape == (1, 64, 128) and planes.dtype == np.uint16
    seg = R.tile_bytes(planes[0], 0, 0, 64, 128, 1)
    assert len(seg) == R.SEG and seg[0::2] == seg[1::2]      # low byte = high byte: an element sends one code twice
    toks = R.tokens(seg, 2)
    assert all(k == 'lit' for k, _ in toks) and len(toks) == R.SEG
    counts = [0] * 286
    counts[256] = 1
    for b in seg:
        counts[b] += 1
    assert sum(1 for c in counts if c) == 22
    assert max(R.huffman_lengths(counts, None)) == 16
    limited = R.huffman_lengths(counts)
    assert max(limited) == 15 and sum(2 ** (15 - l) for l in limited if l) == 1 << 15
    assert limited[1] == 15      # the rarest value: its element is two 15-bit codes in one word
    stream = R.compress_tile(seg, 2)
    assert R.block_kinds(seg, 2) == 'D' and len(stream) == 5423
    assert zlib.decompress(stream) == seg


def test_off_grid_tiles_end_inside_a_round_of_64():
    last = {(name, np.dtype(dt).name): K.last_segment_elements(th, tw, dt)
            for name, _, _, (th, tw) in K.OFF_GRID for dt in (np.uint8, np.uint16)}
    assert last['t1x1', 'uint16'] == last['t1x1', 'uint8'] == 1
    assert last['t5x7', 'uint16'] == 35 and last['t3x64', 'uint16'] == 192 and last['t37x53', 'uint16'] == 1961
    assert last['t100x100-runs', 'uint16'] == 1808 and 1808 % 64 == 16 and last['t100x100-runs', 'uint8'] == 10000
    assert last['t129x127', 'uint16'] == 8191 and 8191 % 64 == 63 and last['t129x127', 'uint8'] == 16383
    assert last['plane10x10-t16x32', 'uint16'] == 512
    assert any(v % 2 for v in last.values()) and sum(1 for v in last.values() if v % 64) >= 8
    assert ometiff.check_tile_shape((16, 32)) == (16, 32)
    for name, _, _, tile in K.OFF_GRID[:-1]:      # none of the others is a TIFF tile
        with pytest.raises(ValueError):
            ometiff.check_tile_shape(tile)
    planes, _, _ = K.off_grid('t1x1', np.uint16)
    assert planes.shape == (2, 11, 15) and planes.size == 330


@pytest.mark.parametrize('predictor', [1, 2])
@pytest.mark.parametrize('dtype', [np.uint8, np.uint16])
@pytest.mark.parametrize('name', [c[0] for c in K.OFF_GRID])
def test_reference_streams_of_off_grid_tiles_inflate(name, dtype, predictor):
    planes, th, tw = K.off_grid(name, dtype)
    streams, want = R.encode_planes(planes, th, tw, predictor), R.expected_tiles(planes, th, tw, predictor)
    n, h, w = planes.shape
    assert len(streams) == len(want) == n * -(-h // th) * -(-w // tw)
    assert any(want)
    for s, t in zip(streams, want):
        assert (zlib.decompress(s) if s else b'') == t


def test_reference_stream_of_all_ones_inflates():
    for dtype in (np.uint8, np.uint16):
        planes = K.all_ones((1, 100, 100), dtype)
        assert set(planes.tobytes()) == {0xFF}
        for predictor in (1, 2):
            t = R.tile_bytes(planes[0], 0, 0, 100, 100, predictor)
            assert zlib.decompress(R.compress_tile(t, planes.dtype.itemsize)) == t
    seg = bytes([0xFF]) * R.SEG      # the largest sums a segment contributes, and their combination over 2048 segments
    assert R.adler_combine([(R.SEG,) + R.adler_sums(seg)] * 2048) == zlib.adler32(seg * 2048)


def test_adler_sums_combine_to_zlibs():
    rng = np.random.default_rng(3)
    data = rng.integers(0, 256, 50000).astype(np.uint8).tobytes()
    parts = [(len(data[a:a + R.SEG]),) + R.adler_sums(data[a:a + R.SEG]) for a in range(0, len(data), R.SEG)]
    assert R.adler_combine(parts) == zlib.adler32(data)


# ---------------------------------------------------------------------------------------------------- the container
def _levels(img, shapes):
    lv = [img.reshape((-1,) + img.shape[3:])]
    for s in shapes[1:]:
        lv.append(np.ascontiguousarray(lv[-1][:, 1::2, 1::2][:, :s[3], :s[4]]))
    return lv


@pytest.mark.parametrize('dtype', [np.uint8, np.uint16])
@pytest.mark.parametrize('compression', ['deflate', 'none'])
def test_container_round_trip_with_host_made_streams(tmp_path, dtype, compression):
    rng = np.random.default_rng(0)
    shape = (1, 2, 3, 70, 100)
    shapes = omezarr.level_shapes(shape, 3)
    img = np.cumsum(rng.integers(-40, 41, shape), axis=4).astype(np.int64).astype(dtype)
    img[0, 1, 2] = 0                      # a plane of zero tiles
    img[0, 0, 0, :40, :40] = 0            # one zero tile among others
    xml = ometiff.ome_xml(shape, dtype, ['a', 'b'], [0xFF0000, 0x00FF00], 0.5, 1.5, 'x')
    path = str(tmp_path / 't.ome.tiff')
    f = ometiff.PyramidTiff(path, shapes, dtype, tile=(32, 32), compression=compression, xml=xml)
    levels = _levels(img, shapes)
    for lv, a in enumerate(levels):       # two batches; plane 4 is never appended: its tiles stay the zero tile
        if compression == 'deflate':      # the streams of the restatement, packed densely as the device encoder packs them
            for planes in ([3, 5], [0, 1, 2]):
                streams = R.encode_planes(a[planes], 32, 32, 2)
                f.append(lv, planes, b''.join(streams), [len(s) for s in streams])
        else:
            f.append_planes(lv, [3, 5], a[[3, 5]])
            f.append_planes(lv, [0, 1, 2], a[:3])
    stats = f.close()
    want = [a.copy() for a in levels]
    for a in want:
        a[4] = 0
    got, got_xml = ometiff.read_pyramid_tiff(path)
    assert got_xml == xml and len(got) == 3
    for lv in range(3):
        assert len(got[lv]) == 6
        for k in range(6):
            assert np.array_equal(got[lv][k], want[lv][k]), (lv, k)
    # structure: header, IFD chain in plane order, SubIFDs, tags, one shared zero tile
    buf, ifds = ometiff.read_pyramid_structure(path)
    assert len(ifds) == 6 and all(len(t['sub']) == 2 for t in ifds)
    val = lambda t, tag: int(t[tag][2][0])
    zero_at = 16
    zero_len = len(f.zero_tile)
    for k, top in enumerate(ifds):
        assert (270 in top) == (k == 0)
        for lv, t in enumerate([top] + top['sub']):
            assert val(t, 254) == (1 if lv else 0) and (val(t, 257), val(t, 256)) == shapes[lv][3:]
            assert val(t, 258) == 8 * np.dtype(dtype).itemsize and val(t, 259) == (8 if compression == 'deflate' else 1)
            assert val(t, 262) == 1 and val(t, 277) == 1 and val(t, 339) == 1 and (val(t, 322), val(t, 323)) == (32, 32)
            assert (317 in t) == (compression == 'deflate') and (317 not in t or val(t, 317) == 2)
            assert t[324][0] == t[325][0] == 16 and (330 in t) == (lv == 0) and (lv or t[330][0] == 18)
            offs, cnts = t[324][2], t[325][2]
            tiles = _tiles(want[lv][k], 32)
            for i, tile in enumerate(tiles):
                assert (int(offs[i]) == zero_at and int(cnts[i]) == zero_len) == (not tile.any()), (k, lv, i)
    if compression == 'deflate':
        assert zlib.decompress(bytes(buf[zero_at:zero_at + zero_len])) == bytes(32 * 32 * np.dtype(dtype).itemsize)
    assert stats['zero_tiles'] == sum(not t.any() for lv in range(3) for k in range(6) for t in _tiles(want[lv][k], 32))
    assert stats['written_bytes'] == os.path.getsize(path) and stats['levels'] == 3 and stats['tile'] == (32, 32)
    assert re.fullmatch(r'\[ome-tiff\] t\.ome\.tiff: 3 levels, tiles 32 x 32, \d+ tiles \(\d+ zero\), \d+ -> \d+ bytes',
                        ometiff.tiff_summary(path, stats))
    try:
        from PIL import Image
    except ImportError:
        return
    im = Image.open(path)       # (Pillow does not list the SubIFDs: level 0 only)
    assert im.n_frames == 6
    for k in range(6):
        im.seek(k)
        assert np.array_equal(np.array(im), want[0][k])


def _tiles(plane, t):
    h, w = plane.shape
    pad = np.zeros((-(-h // t) * t, -(-w // t) * t), plane.dtype)
    pad[:h, :w] = plane
    return [pad[y:y + t, x:x + t] for y in range(0, pad.shape[0], t) for x in range(0, pad.shape[1], t)]


def test_container_refuses_what_tiff_cannot_hold(tmp_path):
    shapes = omezarr.level_shapes((1, 1, 1, 64, 64), 1)
    for tile in ((24, 32), (32, 40), (0, 16), (8, 8)):
        with pytest.raises(ValueError, match='multiples of 16'):
            ometiff.PyramidTiff(str(tmp_path / 'a.ome.tiff'), shapes, np.uint16, tile=tile)
    with pytest.raises(ValueError, match='uint8 or uint16'):
        ometiff.PyramidTiff(str(tmp_path / 'a.ome.tiff'), shapes, np.float32, tile=(16, 16))
    with pytest.raises(ValueError, match="'deflate' or 'none'"):
        ometiff.PyramidTiff(str(tmp_path / 'a.ome.tiff'), shapes, np.uint16, tile=(16, 16), compression='lzw')
    assert not os.path.exists(str(tmp_path / 'a.ome.tiff'))


# ---------------------------------------------------------------------------------------------------- options
def test_options_are_checked(tmp_path):
    tiff = StitchingParameters(input_folder=str(tmp_path), output_format='.ome.tiff')
    zarr = StitchingParameters(input_folder=str(tmp_path), output_format='.ome.zarr')
    st = Stitcher(tiff, device='cpu')
    assert (st.ome_tiff_layout, st.ome_tiff_compression) == ('planes', 'deflate') and not st._tiff_pyramid()
    st = Stitcher(tiff, device='cpu', ome_tiff_layout='pyramid', ome_tiff_compression='none', pyramid_method='mean')
    assert st._tiff_pyramid() and st.ome_tiff_compression == 'none'
    assert not Stitcher(zarr, device='cpu')._tiff_pyramid()
    with pytest.raises(ValueError, match='needs .ome.tiff output'):
        Stitcher(zarr, device='cpu', ome_tiff_layout='pyramid')
    with pytest.raises(ValueError, match='ome_tiff_layout'):
        Stitcher(tiff, device='cpu', ome_tiff_layout='strips')
    with pytest.raises(ValueError, match='ome_tiff_compression'):
        Stitcher(tiff, device='cpu', ome_tiff_layout='pyramid', ome_tiff_compression='lzw')
    with pytest.raises(ValueError, match='rendering window'):      # stays refused for TIFF, whatever its layout
        Stitcher(tiff, device='cpu', ome_tiff_layout='pyramid', contrast_limits='percentile')
    with pytest.raises(ValueError, match='multiples of 16'):
        ometiff.check_tiff_options('pyramid', 'deflate', '.ome.tiff', (1, 1, 1, 100, 512))
    assert ometiff.check_tiff_options('planes', 'deflate', '.ome.zarr', (1, 1, 1, 100, 512)) == ('planes', 'deflate')
    st = Stitcher(tiff, device='cpu', ome_tiff_layout='pyramid')
    st.chunks = (1, 1, 1, 40, 64)
    st.num_c = st.num_z = 1
    st.calculate_output_dimensions = lambda t, r: (64, 64)
    with pytest.raises(ValueError, match='multiples of 16'):
        st.stream_region_to_tiff(0, 'R0')


def test_cli_parses_the_flags(tmp_path):
    base = ['-i', str(tmp_path), '-f', '.ome.tiff']
    a = stitcher_cli.parse_args(base)
    assert (a.ome_tiff_layout, a.ome_tiff_compression) == ('planes', 'deflate')
    a = stitcher_cli.parse_args(base + ['--ome-tiff-layout', 'pyramid', '--ome-tiff-compression', 'none'])
    assert (a.ome_tiff_layout, a.ome_tiff_compression) == ('pyramid', 'none')
    for bad in (['--ome-tiff-layout', 'strips'], ['--ome-tiff-compression', 'lzw']):
        with pytest.raises(SystemExit):
            stitcher_cli.parse_args(base + bad)


def test_cli_reports_the_refusal(tmp_path, capsys):
    with pytest.raises(SystemExit) as e:
        stitcher_cli.main(['-i', str(tmp_path), '-f', '.ome.zarr', '--ome-tiff-layout', 'pyramid'])
    assert e.value.code == 1 and 'needs .ome.tiff output' in capsys.readouterr().err


def test_the_abi_declares_the_encoder():
    with open(os.path.join(ROOT, 'include', 'squidstitch.h')) as fh:
        header = fh.read()
    for name in ('sq_deflate_chunk_count', 'sq_deflate_out_bound', 'sq_deflate_scratch_bytes', 'sq_deflate_encode_planes'):
        assert re.search(r'\b' + name + r'\(', header) and name in native.EXPORTS
    assert len(native.EXPORTS['sq_deflate_encode_planes'][1]) == len(native.EXPORTS['sq_blosc_encode_planes'][1]) + 1
    L = native.lib()
    # sizes: tiles are full whatever the plane's size, every segment stored is the bound
    assert L.sq_deflate_chunk_count(3, 40, 72, 16, 16) == 3 * 3 * 5
    assert L.sq_deflate_out_bound(1, 144, 144, native.SQ_U16, 144, 144) == 2 + 4 + 3 * 5 + 144 * 144 * 2
    assert L.sq_deflate_out_bound(2, 10, 10, native.SQ_U8, 16, 32) == 2 * (2 + 4 + 5 + 512)
    assert L.sq_deflate_scratch_bytes(1, 144, 144, native.SQ_U16, 144, 144) >= 3 * (R.SEG + 5)
    assert L.sq_deflate_out_bound(1, 32, 32, native.SQ_F32, 16, 16) == native.SQ_ERR_UNSUPPORTED
    assert L.sq_deflate_chunk_count(1, 0, 32, 16, 16) == native.SQ_ERR_INVALID
    assert L.sq_deflate_out_bound(1, 8192, 8192, native.SQ_U16, 8192, 8192) == native.SQ_ERR_UNSUPPORTED      # a tile above 32 MiB
