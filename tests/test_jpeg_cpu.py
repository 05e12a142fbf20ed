"""The JPEG tile stream as the host states it (image-stitcher_amd/jpegtile.py, what csrc/jpeg.hip is held to byte for byte in
tests/test_jpeg_gpu.py) against libjpeg through Pillow: tables, decodability, fidelity, structure; the contents of
tests/jpeg_cases.py held to what they are there for; the pyramid TIFF container with Compression 7 through the host path; the
files of 'deflate' and 'none' untouched; the refusals; the definition held to the independent reference of tests/jpeg_ref.py (a
baseline decoder and a float64 DCT) on the edge cases of tests/test_jpeg_edges_gpu.py, and those cases to their purpose.  No device."""
import io
import os
import re
import struct
import warnings
import zlib

import numpy as np
import pytest

import jpeg_cases as K
import jpeg_ref as R
from image_stitcher_amd import jpegtile as J
from image_stitcher_amd import native, ometiff, omezarr, stitcher_cli
from image_stitcher_amd.stitcher import Stitcher
from image_stitcher_amd.stitcher_parameters import StitchingParameters

# Ours may be below libjpeg's PSNR by at most this.  The two encoders differ only in the transform's rounding (10-bit cosines and
# one rounding here; libjpeg's default integer DCT rounds twice at 13 bits), i.e. in which way a few near-tie coefficients fall:
# measured on the image below, ours - libjpeg's = +0.0001, +0.0006, +0.0000, +0.0062 dB at quality 50, 75, 90, 95, and on a second
# draw of the same kind +0.0003, -0.0005, -0.0021, +0.0099 dB: either sign, up to 0.01 dB.  0.02 dB is twice that spread, ten
# times the largest deficit seen, and a tenth of what a defect in the definition (a wrong table entry, a biased rounding) costs.
PSNR_MARGIN_DB = 0.02


def pil():
    return pytest.importorskip('PIL.Image')


def decode(stream):
    """Pillow's decode of a stream, any warning an error."""
    Image = pil()
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        with Image.open(io.BytesIO(stream)) as im:
            assert im.format == 'JPEG' and im.mode == 'L'
            out = np.asarray(im).copy()
            assert im.size == (out.shape[1], out.shape[0])
            return out


def psnr(a, b):
    return 10 * np.log10(255.0 ** 2 / np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2))


def segments(stream):
    """[(marker, payload)] up to and including SOS, then the entropy-coded data, then what follows it."""
    assert stream[:2] == b'\xFF\xD8'
    at, out = 2, [(0xD8, b'')]
    while True:
        assert stream[at] == 0xFF
        marker = stream[at + 1]
        (n,) = struct.unpack('>H', stream[at + 2:at + 4])
        out.append((marker, stream[at + 4:at + 2 + n]))
        at += 2 + n
        if marker == 0xDA:
            return out, stream[at:-2], stream[-2:]


# ---------------------------------------------------------------------------------------------------- the definition's constants
def test_the_literals_are_what_the_formulas_give():
    u, j = np.arange(8)[:, None], np.arange(8)[None, :]
    a = np.where(u == 0, np.sqrt(1 / 8), 0.5)
    assert np.array_equal(np.rint(2 ** J.DCT_SCALE_BITS * a * np.cos((2 * j + 1) * u * np.pi / 16)).astype(np.int64), J.DCT_MATRIX)
    assert np.array_equal(J.DCT_MATRIX[:, ::-1], J.DCT_MATRIX * np.where(np.arange(8) % 2, -1, 1)[:, None])      # what dct8 relies on
    # the 32-bit bound of the header: |N| <= 128 (max row sum)^2, and |N| + D / 2 with the largest divisor
    rows = np.abs(J.DCT_MATRIX).sum(axis=1).max()
    assert rows == 2896 and 128 * rows ** 2 < 2 ** 30 and 128 * rows ** 2 + 255 * 2 ** 19 < 2 ** 31
    assert sorted(J.ZIGZAG.tolist()) == list(range(64)) and J.ZIGZAG[:6].tolist() == [0, 1, 8, 16, 9, 2]
    assert sum(J.DC_BITS) == len(J.DC_VALS) == 12 and sum(J.AC_BITS) == len(J.AC_VALS) == 162
    assert (J.AC_CODE[0x00], J.AC_LEN[0x00]) == (0b1010, 4) and (J.AC_CODE[0xF0], J.AC_LEN[0xF0]) == (0b11111111001, 11)
    assert J.DC_LEN.max() == 9 and J.AC_LEN.max() == 16 and len(J.header(16, 16, 50)) == J.HEADER_BYTES == 312


@pytest.mark.parametrize('quality', [1, 25, 50, 75, 90, 95, 100])
def test_quantisation_tables_are_libjpegs(quality):
    Image = pil()

    def table_of(q):
        b = io.BytesIO()
        Image.fromarray(np.zeros((16, 16), np.uint8)).save(b, 'JPEG', quality=q)
        with Image.open(io.BytesIO(b.getvalue())) as im:
            return np.array(im.quantization[0], dtype=np.int64)
    # which order this Pillow reports (it changed between versions) is read off quality 50, where the table is Annex K.1 itself
    k1 = table_of(50)
    natural = np.array_equal(k1, J.BASE_TABLE)
    assert natural or np.array_equal(k1, J.BASE_TABLE[J.ZIGZAG])
    ours = J.quant_table(quality)
    assert np.array_equal(table_of(quality), ours if natural else ours[J.ZIGZAG])
    assert ours.min() >= 1 and ours.max() <= 255
    # and the DQT segment of a stream holds it in zigzag order
    segs, _, _ = segments(J.encode_tile(np.full((8, 8), 7, np.uint8), quality))
    assert segs[1][0] == 0xDB and segs[1][1] == b'\x00' + bytes(ours[J.ZIGZAG].tolist())


# ---------------------------------------------------------------------------------------------------- decoding
@pytest.mark.parametrize('quality', K.QUALITIES)
@pytest.mark.parametrize('shape_name', [s[0] for s in K.SHAPES])
def test_every_case_decodes(shape_name, quality):
    """Every stream of every content opens as a grey JPEG of the tile's size and decodes without a warning; at quality 100 (all
    divisors 1) to within the rounding of the two transforms."""
    _, shape, (th, tw), _ = next(s for s in K.SHAPES if s[0] == shape_name)
    for name in K.CONTENTS:
        planes = K.content(name, shape, seed=len(name) + quality)
        for tile, stream in zip(K.tiles_of(planes, th, tw), K.expected_streams(planes, th, tw, quality)):
            if not tile.any():
                assert stream == b''
                continue
            got = decode(stream)
            assert got.shape == (th, tw) and got.dtype == np.uint8
            if quality == 100:
                assert np.abs(got.astype(int) - tile).max() <= 2, name


@pytest.mark.parametrize('quality', [75, 90, 95, 100])
@pytest.mark.parametrize('value', [0, 128, 255])
def test_constant_tiles_decode_to_the_constant(value, quality):
    """Only the DC is non-zero, and 128 codes all-zero blocks.  (Qualities whose DC step can hold the three values: at quality 1
    the step is 32 grey levels for any encoder; at quality 50 the level 255 is DC 1016 / 16 = 63.5, a tie that libjpeg rounds up to
    256 -> 255 and the 10-bit transform here, whose DC gain is 362^2 / 2^17 = 0.99979, rounds down to 1008 -> 254: DESIGN 5.4p.)"""
    tile = np.full((32, 48), value, np.uint8)
    z = J.quantised_blocks(tile, quality)
    assert not z[:, :, 1:].any() and (z[:, :, 0] != 0).all() == (value != 128)
    assert (decode(J.encode_tile(tile, quality)) == value).all()
    if value == 128:      # per interval: 6 blocks of (DC category 0: 00, EOB: 1010) = 36 bits, padded to 5 bytes
        _, data, _ = segments(J.encode_tile(tile, quality))
        assert len(data) == 4 * 5 + 3 * 2


# ---------------------------------------------------------------------------------------------------- fidelity against libjpeg
@pytest.fixture(scope='module')
def image():
    return K.content('image', (1, 512, 512), seed=3)[0]


@pytest.mark.parametrize('quality', [50, 75, 90, 95])
def test_fidelity_is_libjpegs(image, quality):
    Image = pil()
    ours = J.encode_tile(image, quality)
    b = io.BytesIO()
    Image.fromarray(image).save(b, 'JPEG', quality=quality, optimize=False)
    theirs = b.getvalue()
    p_ours, p_theirs = psnr(decode(ours), image), psnr(decode(theirs), image)
    print(f'quality {quality}: PSNR ours {p_ours:.4f} dB, libjpeg {p_theirs:.4f} dB, difference {p_ours - p_theirs:+.4f} dB; '
          f'{len(ours)} bytes ours (with {image.shape[0] // 8 - 1} restart markers), {len(theirs)} libjpeg')
    assert p_ours >= p_theirs - PSNR_MARGIN_DB
    assert len(ours) < 1.02 * len(theirs) + 2 * (image.shape[0] // 8)      # the same tables: the same size but for the restarts


# ---------------------------------------------------------------------------------------------------- structure
@pytest.mark.parametrize('shape_name', [s[0] for s in K.SHAPES])
def test_marker_sequence_restarts_and_stuffing(shape_name):
    _, shape, (th, tw), _ = next(s for s in K.SHAPES if s[0] == shape_name)
    planes = K.content('uniform', shape, seed=4)
    for tile in K.tiles_of(planes, th, tw)[:3]:
        stream = J.encode_tile(tile, 90)
        segs, data, tail = segments(stream)
        assert [m for m, _ in segs] == [0xD8, 0xDB, 0xC0, 0xC4, 0xDD, 0xDA] and tail == b'\xFF\xD9'      # no APPn, one DHT
        sof, dht, dri, sos = segs[2][1], segs[3][1], segs[4][1], segs[5][1]
        assert sof == b'\x08' + struct.pack('>HH', th, tw) + b'\x01\x01\x11\x00'
        assert dht[0] == 0x00 and dht[1 + 16 + 12] == 0x10 and len(dht) == 1 + 16 + 12 + 1 + 16 + 162
        assert struct.unpack('>H', dri)[0] == tw // 8
        assert sos == b'\x01\x01\x00\x00\x3F\x00'
        # every FF of the data is followed by 00 (stuffing) or by RSTm, m cycling 0..7, block rows - 1 of them
        after = [data[i + 1] for i in range(len(data) - 1) if data[i] == 0xFF]
        assert data[-1] != 0xFF and set(after) <= {0x00} | set(range(0xD0, 0xD8))
        rst = [b for b in after if b != 0]
        assert rst == [0xD0 + k % 8 for k in range(th // 8 - 1)]
    if shape_name == 'restarts':
        assert th // 8 - 1 == 17      # the counter wraps twice
    assert any(b'\xFF\x00' in K.entropy_data(J.encode_tile(t, 100)) for t in K.tiles_of(planes, th, tw))


def test_the_contents_exercise_what_they_are_for():
    shape = (1, 32, 64)
    # category 11 DC differences at quality 100: -1024 <-> +1016
    z = J.quantised_blocks(K.content('blocks', shape)[0], 100)
    assert not z[:, :, 1:].any() and set(np.unique(z[:, :, 0]).tolist()) == {-1024, 1016}
    # the largest AC coefficient: category 10, at (7, 7)
    z = J.quantised_blocks(K.content('checker', shape)[0], 100)
    assert 512 <= np.abs(z[:, :, 63]).max() < 1024 and np.abs(z[:, :, 1:]).max() < 1024
    # EOB after a few coefficients
    z = J.quantised_blocks(K.content('ramp', shape)[0], 50)
    assert all(np.flatnonzero(b).max(initial=0) < 10 for b in z.reshape(-1, 64))
    # only coefficient 63: three ZRL, no EOB
    z = J.quantised_blocks(K.content('last', shape)[0], 50).reshape(-1, 64)
    assert not z[:, :63].any() and set(np.unique(z[:, 63]).tolist()) == {-1, 2}
    items = J._items(z.reshape(4, 8, 64))
    zrl = (J.AC_CODE[J.ZRL], J.AC_LEN[J.ZRL])
    assert sum((v, n) == zrl for v, n in zip(items[1], items[2])) == 3 * len(z)
    assert not any((v, n) == (J.AC_CODE[J.EOB], J.AC_LEN[J.EOB]) for v, n in zip(items[1], items[2]))
    # runs of 16, 33 and 47 zeros
    z = J.quantised_blocks(K.content('gaps', shape)[0], 50).reshape(-1, 64)
    kinds = {tuple(np.flatnonzero(b).tolist()) for b in z}
    assert kinds == {(1, 18, 52, 63), (48,)}
    # frequent FF, long codes
    data = K.entropy_data(J.encode_tile(K.content('uniform', (1, 64, 64), seed=1)[0], 100))
    assert data.count(b'\xFF\x00') > 10 and len(data) > 64 * 64
    # one pixel: one tile with a stream
    assert sum(s != b'' for s in K.expected_streams(K.content('pixel', (1, 40, 72)), 16, 16, 90)) == 1


def test_bad_tiles_and_qualities_are_refused():
    for q in (0, 101, 50.5, -3):
        with pytest.raises(ValueError, match='1..100'):
            J.encode_tile(np.zeros((16, 16), np.uint8), q)
    with pytest.raises(ValueError, match='multiples of 8'):
        J.encode_tile(np.zeros((16, 12), np.uint8), 90)
    with pytest.raises(ValueError, match='uint8'):
        J.encode_tile(np.zeros((16, 16), np.uint16), 90)


# ---------------------------------------------------------------------------------------------------- the container, host path
def _levels(dtype=np.uint8, seed=5):
    shapes = omezarr.level_shapes((1, 2, 3, 100, 150), 3)
    out = []
    for lv, s in enumerate(shapes):
        planes = K.content('image', (6,) + tuple(s[3:]), seed=seed + lv).astype(dtype)
        planes[2] = 0
        planes[4, :40, :70] = 0      # zero tiles inside a plane
        out.append(planes)
    return shapes, out


def _write(path, compression, dtype=np.uint8, **kw):
    shapes, levels = _levels(dtype)
    file = ometiff.PyramidTiff(path, shapes, dtype, tile=(32, 32), compression=compression, xml='<OME>levels</OME>', **kw)
    for lv, planes in enumerate(levels):
        file.append_planes(lv, list(range(6)), planes)
    return file, file.close(), levels


def test_container_with_jpeg_tiles(tmp_path):
    pil()
    path = str(tmp_path / 'j.ome.tiff')
    file, stats, levels = _write(path, 'jpeg', quality=85)
    buf, ifds = ometiff.read_pyramid_structure(path)
    zero = J.encode_tile(np.zeros((32, 32), np.uint8), 85)
    assert bytes(buf[16:16 + len(zero)]) == zero and file.zero_tile == zero
    streams = ometiff.read_tile_streams(path)
    got_levels, xml = ometiff.read_pyramid_tiff(path)
    assert xml == '<OME>levels</OME>' and len(ifds) == 6 and len(streams) == len(got_levels) == 3
    val = lambda t, tag: int(t[tag][2][0])
    for k, top in enumerate(ifds):
        assert len(top['sub']) == 2 and top[330][0] == 18 and (270 in top) == (k == 0)
        for lv, t in enumerate([top] + top['sub']):
            assert val(t, 259) == 7 and val(t, 262) == 1 and 317 not in t and 347 not in t      # no Predictor, no JPEGTables
            assert val(t, 258) == 8 and val(t, 277) == 1 and (val(t, 322), val(t, 323)) == (32, 32)
            assert (val(t, 257), val(t, 256)) == levels[lv].shape[1:]
            tiles = K.tiles_of(levels[lv][k][None], 32, 32)
            assert len(streams[lv][k]) == len(tiles) == t[324][1]
            decoded = []
            for i, (tile, s) in enumerate(zip(tiles, streams[lv][k])):
                is_zero = int(t[324][2][i]) == 16
                assert is_zero == (not tile.any()) and (not is_zero or int(t[325][2][i]) == len(zero))
                assert s == (J.encode_tile(tile, 85) if tile.any() else zero)
                decoded.append(decode(s))
            gy, gx = -(-levels[lv].shape[1] // 32), -(-levels[lv].shape[2] // 32)
            full = np.stack(decoded).reshape(gy, gx, 32, 32).transpose(0, 2, 1, 3).reshape(gy * 32, gx * 32)
            want = full[:levels[lv].shape[1], :levels[lv].shape[2]]
            assert np.array_equal(got_levels[lv][k], want)
            if levels[lv][k].any():
                assert psnr(want, levels[lv][k]) > 30
    assert stats['written_bytes'] == os.path.getsize(path) and stats['compression'] == 'jpeg' and stats['quality'] == 85
    assert re.fullmatch(r'\[ome-tiff\] j\.ome\.tiff: 3 levels, tiles 32 x 32, \d+ tiles \(\d+ zero\), \d+ -> \d+ bytes, jpeg quality 85',
                        ometiff.tiff_summary(path, stats))
    assert stats['written_bytes'] < stats['raw_bytes']
    from PIL import Image, features
    if features.check('libtiff'):      # an outside reader opens the whole BigTIFF: page 0 is level 0 of plane 0
        with Image.open(path) as im:
            assert im.n_frames == 6 and im.mode == 'L' and im.size == (150, 100)
            assert np.array_equal(np.array(im), got_levels[0][0])


@pytest.mark.parametrize('dtype', [np.uint8, np.uint16])
@pytest.mark.parametrize('compression', ['deflate', 'none'])
def test_deflate_and_none_files_are_untouched(tmp_path, compression, dtype):
    """The files of the other two codecs, rebuilt here from the same arrays with zlib and struct alone: the header, the zero
    tile, every tile's bytes in arrival order, and exactly the tags the layout had before (no new one, Compression 8 / 1,
    Predictor 2 only with deflate)."""
    path = str(tmp_path / 'd.ome.tiff')
    file, stats, levels = _write(path, compression, dtype)
    itemsize = np.dtype(dtype).itemsize
    with open(path, 'rb') as fh:
        buf = fh.read()

    def enc(tile):
        tile = tile.astype(np.dtype(dtype).newbyteorder('<'))
        if compression == 'none':
            return tile.tobytes()
        pred = tile.copy()
        pred[:, 1:] = tile[:, 1:] - tile[:, :-1]
        return zlib.compress(pred.tobytes(), 1)
    want = [enc(np.zeros((32, 32), dtype))]
    for lv, planes in enumerate(levels):
        pad = [np.zeros((-(-p.shape[0] // 32) * 32, -(-p.shape[1] // 32) * 32), dtype) for p in planes]
        for p, full in zip(planes, pad):
            full[:p.shape[0], :p.shape[1]] = p
            want += [enc(full[y:y + 32, x:x + 32]) for y in range(0, full.shape[0], 32) for x in range(0, full.shape[1], 32)
                     if full[y:y + 32, x:x + 32].any()]
    body = b''.join(want)
    assert buf[:8] == struct.pack('<2sHHH', b'II', 43, 8, 0) and buf[16:16 + len(body)] == body
    _, ifds = ometiff.read_pyramid_structure(path)
    base = {254, 256, 257, 258, 259, 262, 277, 322, 323, 324, 325, 339} | ({317} if compression == 'deflate' else set())
    for k, top in enumerate(ifds):
        assert set(top) - {'sub'} == base | {330} | ({270} if k == 0 else set())
        for t in top['sub']:
            assert set(t) - {'sub'} == base
        for t in [top] + top['sub']:
            assert int(t[259][2][0]) == (8 if compression == 'deflate' else 1) and int(t[258][2][0]) == 8 * itemsize
    assert re.fullmatch(r'\[ome-tiff\] d\.ome\.tiff: 3 levels, tiles 32 x 32, \d+ tiles \(\d+ zero\), \d+ -> \d+ bytes',
                        ometiff.tiff_summary(path, stats))
    levels_back, _ = ometiff.read_pyramid_tiff(path)
    assert all(np.array_equal(levels_back[lv][k], levels[lv][k]) for lv in range(3) for k in range(6))


# ---------------------------------------------------------------------------------------------------- refusals and options
def test_refusals(tmp_path):
    shapes = omezarr.level_shapes((1, 1, 1, 64, 64), 1)
    path = str(tmp_path / 'a.ome.tiff')
    with pytest.raises(ValueError, match='uint8'):
        ometiff.PyramidTiff(path, shapes, np.uint16, tile=(16, 16), compression='jpeg')
    for q in (0, 101):
        with pytest.raises(ValueError, match='1..100'):
            ometiff.PyramidTiff(path, shapes, np.uint8, tile=(16, 16), compression='jpeg', quality=q)
    assert not os.path.exists(path)
    tiff = StitchingParameters(input_folder=str(tmp_path), output_format='.ome.tiff')
    zarr = StitchingParameters(input_folder=str(tmp_path), output_format='.ome.zarr')
    with pytest.raises(ValueError, match='needs .ome.tiff output'):
        Stitcher(zarr, device='cpu', ome_tiff_compression='jpeg')
    for q in (0, 101):
        with pytest.raises(ValueError, match='1..100'):
            Stitcher(tiff, device='cpu', ome_tiff_layout='pyramid', ome_tiff_compression='jpeg', ome_tiff_quality=q)
    with pytest.raises(ValueError, match="needs ome_tiff_layout='pyramid'"):
        Stitcher(tiff, device='cpu', ome_tiff_compression='jpeg')
    st = Stitcher(tiff, device='cpu', ome_tiff_layout='pyramid', ome_tiff_compression='jpeg')
    assert (st.ome_tiff_compression, st.ome_tiff_quality) == ('jpeg', 90)
    assert Stitcher(tiff, device='cpu', ome_tiff_layout='pyramid', ome_tiff_compression='jpeg', ome_tiff_quality=75).ome_tiff_quality == 75
    with pytest.raises(ValueError, match='uint8'):
        ometiff.check_jpeg_dtype(np.uint16)
    ometiff.check_jpeg_dtype(np.uint8)


def test_cli_flags(tmp_path, capsys):
    base = ['-i', str(tmp_path), '-f', '.ome.tiff', '--ome-tiff-layout', 'pyramid']
    a = stitcher_cli.parse_args(base)
    assert (a.ome_tiff_compression, a.ome_tiff_quality) == ('deflate', 90)
    a = stitcher_cli.parse_args(base + ['--ome-tiff-compression', 'jpeg', '--ome-tiff-quality', '75'])
    assert (a.ome_tiff_compression, a.ome_tiff_quality) == ('jpeg', 75)
    with pytest.raises(SystemExit) as e:
        stitcher_cli.main(['-i', str(tmp_path), '-f', '.ome.zarr', '--ome-tiff-compression', 'jpeg'])
    assert e.value.code == 1 and 'needs .ome.tiff output' in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:
        stitcher_cli.main(base + ['--ome-tiff-compression', 'jpeg', '--ome-tiff-quality', '0'])
    assert e.value.code == 1 and '1..100' in capsys.readouterr().err


def test_abi_and_sizes():
    with open(os.path.join(os.path.dirname(__file__), '..', 'include', 'squidstitch.h')) as fh:
        header = fh.read()
    for name in ('sq_jpeg_chunk_count', 'sq_jpeg_out_bound', 'sq_jpeg_scratch_bytes', 'sq_jpeg_encode_planes'):
        assert re.search(r'\b' + name + r'\(', header) and name in native.EXPORTS
    assert native.EXPORTS['sq_jpeg_encode_planes'] == native.EXPORTS['sq_deflate_encode_planes']
    L = native.lib()
    assert L.sq_version() == 108
    assert L.sq_jpeg_chunk_count(3, 40, 72, 16, 16) == 3 * 3 * 5
    # the true worst case: every block 20 + 63 * 26 bits, every byte stuffed, a marker behind every interval
    assert L.sq_jpeg_out_bound(1, 16, 16, native.SQ_U8, 16, 16) == 312 + 2 * (2 * ((2 * 1658 + 7) // 8) + 2)
    assert L.sq_jpeg_out_bound(2, 10, 10, native.SQ_U8, 16, 32) == 2 * (312 + 2 * (2 * ((4 * 1658 + 7) // 8) + 2))
    assert L.sq_jpeg_out_bound(1, 32, 32, native.SQ_U16, 16, 16) == native.SQ_ERR_UNSUPPORTED
    assert L.sq_jpeg_scratch_bytes(1, 32, 32, native.SQ_F32, 16, 16) == native.SQ_ERR_UNSUPPORTED
    assert L.sq_jpeg_chunk_count(1, 32, 32, 16, 12) == native.SQ_ERR_INVALID
    assert L.sq_jpeg_chunk_count(1, 0, 32, 16, 16) == native.SQ_ERR_INVALID
    assert L.sq_jpeg_out_bound(1, 8192, 8192, native.SQ_U8, 8192, 8192) == native.SQ_ERR_UNSUPPORTED      # above 32 Mi elements
    # no stream of the cases is longer than the bound says
    for name in ('uniform', 'checker', 'blocks'):
        planes = K.content(name, (1, 16, 1040), seed=9)
        assert len(J.encode_tile(planes[0], 100)) <= L.sq_jpeg_out_bound(1, 16, 1040, native.SQ_U8, 16, 1040)
    assert ometiff.jpeg_buffers_plane_bytes(100, 150, 2, (32, 32)) == 2 * ((4 * 5 + 2 * 3) * (32 * 32 + 314))


# ---------------------------------------------------------------------------------------------------- the independent reference
# tests/jpeg_ref.py restates the two halves of the operation -- T.81's baseline decoding down to the quantised coefficients, and a
# float64 DCT -- and the cases below are the ones tests/test_jpeg_edges_gpu.py encodes on the device: here the host definition is
# held to the reference, and every case to what it is there for.
E_BOUND = R.transform_bound(J.DCT_MATRIX, J.DCT_SCALE_BITS)
WORST_EXCESS = {}      # test -> the largest (|c Q - n| - Q / 2) / E it met; printed, and below 1 by rounding_excess's assertion


def _excess(key, coefficients, divisors, tile):
    r = R.rounding_excess(coefficients, divisors, tile, E_BOUND)
    WORST_EXCESS[key] = max(WORST_EXCESS.get(key, -np.inf), r)
    return r


def test_the_reference_is_independent_and_its_bound_is_what_it_says():
    with open(R.__file__) as fh:
        assert 'jpegtile' not in fh.read().split('"""', 2)[2]      # (its docstring names what it is a reference of)
    assert np.array_equal(R.ZIGZAG, J.ZIGZAG)
    a = R.dct_matrix()
    assert np.allclose(a @ a.T, np.eye(8), atol=1e-15)
    assert 0.17 < E_BOUND.min() and E_BOUND.max() < 0.92 and abs(E_BOUND[0] - 0.21875) < 1e-9
    # the bound is reached: the block of +-128 whose signs are those of the terms of position (u, v)
    for u, v in ((0, 0), (1, 1), (7, 7), (3, 6)):
        diff = np.outer(J.DCT_MATRIX[u], J.DCT_MATRIX[v]) / 2.0 ** 20 - np.outer(a[u], a[v])
        x = 128 * np.where(diff >= 0, 1, -1)
        n_int = (J.DCT_MATRIX @ x @ J.DCT_MATRIX.T)[u, v] / 2.0 ** 20
        assert abs(abs(n_int - (a @ x @ a.T)[u, v]) - E_BOUND[8 * u + v]) < 1e-9


def test_the_reference_decoder_refuses_what_a_reader_must_not_meet():
    tile = K.content('uniform', (1, 24, 16), seed=5)[0]
    good = J.encode_tile(tile, 90)
    d = R.decode(good)
    assert (d.height, d.width, d.restart_interval, len(d.pads)) == (24, 16, 2, 3)
    assert np.array_equal(d.coefficients, J.quantised_blocks(tile, 90))
    assert np.array_equal(d.divisors, J.quant_table(90)[J.ZIGZAG])
    rst = [i for i in range(J.HEADER_BYTES, len(good) - 2) if good[i] == 0xFF and good[i + 1] != 0]
    assert [good[i + 1] for i in rst] == [0xD0, 0xD1]
    edit = lambda at, b: good[:at] + bytes([b]) + good[at + 1:]
    cases = {
        'RST1 where RST0 belongs': edit(rst[0] + 1, 0xD1),
        'EOI where RST1 belongs': edit(rst[1] + 1, 0xD9),
        'RST2 where EOI belongs': edit(len(good) - 1, 0xD2),
        'a byte behind EOI': good + b'\x00',
        'no EOI': good[:-2],
        'an interval removed': good[:rst[0]] + good[rst[1]:],
        'FF that is not stuffed': good[:J.HEADER_BYTES + 3] + b'\xFF\x41' + good[J.HEADER_BYTES + 5:],
        'a byte more in an interval': good[:rst[0]] + b'\x7F' + good[rst[0]:],
        'a byte less in an interval': good[:rst[0] - 1] + good[rst[0]:],
        'progressive': good.replace(b'\xFF\xC0\x00\x0B', b'\xFF\xC2\x00\x0B'),
    }
    pads = R.decode(good).pads
    k = next(i for i, p in enumerate(pads) if p)      # padding with a 0 bit in it
    end = rst[k] if k < 2 else len(good) - 2
    cases['a 0 among the padding bits'] = edit(end - 1, good[end - 1] & 0xFE)
    for what, bad in cases.items():
        with pytest.raises(R.StreamError, match=r'^byte \d+: '):
            R.decode(bad)
            pytest.fail(f'{what}: accepted')


@pytest.mark.parametrize('shape_name', ['edges', 'rounds'])
def test_the_definition_rounds_to_nearest_under_its_transform(shape_name):
    """Every existing content at qualities 1, 4, .., 100: every coefficient of the host definition is the nearest multiple of its
    divisor to the float64 DCT, up to the distance E between the two transforms."""
    _, shape, (th, tw), _ = next(s for s in K.SHAPES if s[0] == shape_name)
    for name in K.CONTENTS:
        for tile in K.tiles_of(K.content(name, shape, seed=len(name)), th, tw):
            for quality in range(1, 101, 3):
                _excess(shape_name, J.quantised_blocks(tile, quality), J.quant_table(quality)[J.ZIGZAG], tile)
    print(f'{shape_name}: largest (|cQ - n| - Q/2) / E = {WORST_EXCESS[shape_name]:.4f}')
    assert WORST_EXCESS[shape_name] < 1


def _held_to_the_reference(planes, th, tw, quality, key):
    """Every stream of the planes: Pillow decodes it without a warning at the tile's size, the independent decoder finds exactly
    the definition's coefficients in it, and those are nearest under the float64 transform.  -> the decoded streams."""
    out = []
    for tile, stream in zip(K.tiles_of(planes, th, tw), K.expected_streams(planes, th, tw, quality)):
        if not tile.any():
            assert stream == b''
            out.append(None)
            continue
        assert decode(stream).shape == (th, tw)
        d = R.decode(stream)
        assert (d.height, d.width, d.restart_interval) == (th, tw, tw // 8)
        assert np.array_equal(d.coefficients, J.quantised_blocks(tile, quality)), key
        assert np.array_equal(d.divisors, J.quant_table(quality)[J.ZIGZAG])
        _excess(key, d.coefficients, d.divisors, tile)
        out.append(d)
    return out


def _distinct_edge_shapes():
    """The phase layouts hold the planes of 'mixed': the same tiles, the same streams.  On the host one of them is enough."""
    return [s[0] for s in K.EDGE_SHAPES if not s[0].startswith('phase')]


@pytest.mark.parametrize('shape_name', _distinct_edge_shapes())
def test_every_edge_case_on_the_host(shape_name):
    _, shape, (th, tw), _ = K.edge_shape(shape_name)
    contents = dict(K.EDGE_CONTENTS)
    if shape_name in K.FULL_CONTENT_SHAPES:
        contents.update({name: K.QUALITIES for name in K.CONTENTS if name not in contents})
    streams = 0
    for name, qualities in contents.items():
        for quality in qualities:
            got = _held_to_the_reference(K.edge_content(name, shape_name, quality), th, tw, quality, shape_name)
            streams += sum(d is not None for d in got)
            assert (streams > 0) or name == 'zero' or shape_name.startswith('tiny')
    print(f'{shape_name}: {streams} streams, largest (|cQ - n| - Q/2) / E = {WORST_EXCESS.get(shape_name, float("nan")):.4f}')


def test_the_edge_shapes_reach_what_they_are_there_for():
    geo = {name: (shape, tile, layout) for name, shape, tile, layout in K.EDGE_SHAPES}
    tiles = lambda name: geo[name][0][0] * -(-geo[name][0][1] // geo[name][1][0]) * -(-geo[name][0][2] // geo[name][1][1])
    # the 64-bit load: base, pitch and plane stride all multiples of 8 -- and then only blocks that lie inside the width
    aligned = lambda name: (geo[name][2][0] | geo[name][2][1] | geo[name][2][2]) % 8 == 0
    assert aligned('mixed') and geo['mixed'][0][2] % 8 == 6 and geo['mixed'][2][0] > geo['mixed'][0][2]
    assert [geo[f'phase{k}'][2] for k in range(1, 8)] == [(72, 24 * 72, k) for k in range(1, 8)]
    assert not any(aligned(f'phase{k}') for k in range(1, 8))
    assert not aligned('stride') and geo['stride'][2][0] % 8 == 0 and geo['stride'][2][2] == 0 and geo['stride'][2][1] % 8 == 4
    for name in ['mixed', 'stride'] + [f'phase{k}' for k in range(1, 8)]:
        for content in K.EDGE_CONTENTS:
            planes = K.edge_content(content, name, K.EDGE_CONTENTS[content][0])
            assert K.longest_guard_run(planes) < 3
            buf, at = K.guarded(planes, geo[name][2])
            n, h, w = planes.shape
            pitch, stride, base = geo[name][2]
            assert at == 256 + base
            inside = np.zeros(len(buf), bool)
            for p in range(n):
                for y in range(h):
                    row = at + p * stride + y * pitch
                    assert np.array_equal(buf[row:row + w], planes[p, y])
                    inside[row:row + w] = True
            assert (buf[~inside] == K.GUARD).all() and not inside[:256].any() and not inside[-64:].any()
            if pitch > w:      # guard bytes behind every row; 'stride' has them behind every plane
                assert all(not inside[at + p * stride + y * pitch + w] for p in range(n) for y in range(h))
            assert all(not inside[at + p * stride + (h - 1) * pitch + w] for p in range(n))
    # rounds of 64 blocks, rounds of 64 intervals
    assert (geo['round64'][1][1] // 8, geo['round65'][1][1] // 8) == (64, 65)
    assert (geo['tall65'][1][0] // 8, geo['tall129'][1][0] // 8) == (65, 129)
    # the scan's elements per thread: per = ceil(tiles / 1024); with 1025 tiles the threads from 513 on have lo == hi == n
    assert [tiles(n) for n in ('tiles1024', 'tiles1025', 'tiles2625')] == [1024, 1025, 2625]
    assert [-(-tiles(n) // 1024) for n in ('tiles1024', 'tiles1025', 'tiles2625')] == [1, 2, 3]
    assert min(1025, 513 * 2) == 1025 and min(1025, 512 * 2) < 1025
    planes = K.edge_content('uniform', 'tiles2625', 100)
    sizes = np.array([len(s) for s in K.expected_streams(planes, 8, 8, 100)])
    assert not sizes[875:1750].any() and sizes[1750:].all()                      # plane 1: no tile has a stream
    assert not sizes[5 * 35:10 * 35].any() and sizes[:5 * 35].all() and sizes[10 * 35:875].all()
    # the format's limits
    assert geo['widest'][1] == (8, 65496) and tiles('widest') == 2 and geo['tallest'][1] == (65496, 8) and tiles('tallest') == 1
    assert -(-8187 // 64) == 128
    head = J.header(65496, 8, 50)
    assert head[2 + 69 + 5:2 + 69 + 9] == b'\xFF\xD8\x00\x08'
    assert R.decode(J.encode_tile(np.full((8, 65496), 9, np.uint8), 50)).restart_interval == 8187
    # planes smaller than a block, than a tile
    assert geo['tiny1'][0] == (1, 1, 1) and geo['tiny79'][0] == (1, 7, 9) and tiles('tiny1') == tiles('tiny79') == 1


def _data_bits(d):
    return sum(b[-1] for b in d.block_bits)


def test_binary_is_denser_than_noise():
    shape = (1, 16, 1040)
    bits = {}
    for name in ('uniform', 'binary'):
        tile = K.content(name, shape, seed=8)[0]
        d = R.decode(J.encode_tile(tile, 100))
        bits[name] = _data_bits(d) / (2 * 130)
        if name == 'binary':
            assert np.abs(d.coefficients[:, :, 1:]).max() > 500
    print(f'bits per block at quality 100: uniform {bits["uniform"]:.0f}, binary {bits["binary"]:.0f}')
    assert bits['binary'] > bits['uniform'] + 100


@pytest.mark.parametrize('case', [c[0] for c in K.FFRUNS_SHAPES])
def test_ffruns_puts_ff_where_stuffing_is_hard(case):
    """Among the un-stuffed data: two FF in a row; an FF in the last byte of word 63 of a 64-word group of stuff_out (the next
    lane's output starts behind its stuffed zero in another group); an FF in each of the four bytes of a word."""
    _, shape, (th, tw) = next(c for c in K.FFRUNS_SHAPES if c[0] == case)
    planes = K.content('ffruns', shape)
    (d,) = _held_to_the_reference(planes, th, tw, 100, 'ffruns ' + case)
    places = [p for data, bits in zip(d.intervals, d.block_bits) for p in K.ff_places(data, bits)]
    assert max(K.longest_ff_run(data) for data in d.intervals) >= 2
    assert any(word % 64 == 63 and byte == 3 for word, byte in places)
    assert {byte for _, byte in places} == {0, 1, 2, 3}
    assert max(word for word, _ in places) >= 128      # a round of more than two groups
    print(f'ffruns {case}: {len(places)} FF, {sum(1 for w, b in places if w % 64 == 63 and b == 3)} of them end a group')


def test_dcsweep_crosses_every_rounding_boundary_of_the_dc():
    _, shape, (th, tw), _ = K.edge_shape('widest')
    planes = K.content('dcsweep', shape)
    sums = planes[0].reshape(8, -1, 8).transpose(1, 0, 2).reshape(-1, 64).astype(np.int64).sum(axis=1)
    assert np.array_equal(sums, np.minimum(np.arange(2 * 8187), 16320))
    tiles = K.tiles_of(planes, th, tw)
    for quality, crossed in zip(K.DCSWEEP_QUALITIES, (127, 255, 680, 2040)):
        got = _held_to_the_reference(planes, th, tw, quality, 'dcsweep')
        dc = np.concatenate([d.coefficients[0, :, 0] for d in got])
        # the rule in plain integers: numerator 362^2 (S - 8192), divisor Q 2^20, rounded half away from zero; monotonic in S
        q = int(got[0].divisors[0])
        rule = [(1 if s > 8192 else -1) * ((362 * 362 * abs(s - 8192) + q * 2 ** 19) // (q * 2 ** 20)) for s in (0, 16320)]
        assert np.all(np.diff(dc) >= 0) and [dc[0], dc[-1]] == rule
        assert int((np.diff(dc) != 0).sum()) == rule[1] - rule[0] == crossed
        if quality == 100:
            assert np.array_equal(np.unique(dc), np.arange(-1024, 1017))


def test_noise_on_the_tallest_tile_ends_its_intervals_every_way():
    _, shape, (th, tw), _ = K.edge_shape('tallest')
    (stream,) = K.expected_streams(K.edge_content('uniform', 'tallest', 100), th, tw, 100)
    d = R.decode(stream)
    assert len(d.pads) == 8187 and set(d.pads) == set(range(8))
    last_ff = sum(data[-1] == 0xFF for data in d.intervals)
    assert last_ff > 0
    print(f'tallest uniform q100: {last_ff} of 8187 intervals end with FF; pads {np.bincount(d.pads).tolist()}')


def test_the_quality_sweep_meets_every_divisor():
    rule = set()
    for quality in range(1, 101):
        s = 5000 // quality if quality < 50 else 200 - 2 * quality
        rule |= {min(255, max(1, (int(b) * s + 50) // 100)) for b in J.BASE_TABLE}
    assert len(rule) == 251
    planes = K.sweep_tile()
    assert not planes[0, :8, 8:16].any() and (planes[0, 8:, 40:48] == 255).all()
    met = set()
    for quality in range(1, 101):
        (d,) = _held_to_the_reference(planes, 16, 64, quality, 'sweep')
        met |= set(d.divisors.tolist())
    assert met == rule
    print(f'quality sweep: largest (|cQ - n| - Q/2) / E = {WORST_EXCESS["sweep"]:.4f}')


def test_no_tile_is_larger_than_libjpeg_reads():
    """T.81 holds sides up to 65535, libjpeg (JPEG_MAX_DIMENSION) decodes nothing above 65500: the largest side the definition and
    the library take is the largest multiple of 8 below that, and Pillow decodes it; the next one is refused by both, as Pillow
    refuses its stream."""
    Image = pil()
    assert J.MAX_SIDE == 65496
    L = native.lib()
    for th, tw in ((8, J.MAX_SIDE), (J.MAX_SIDE, 8)):
        tile = K.content('ramp', (1, th, tw))[0]
        got = decode(J.encode_tile(tile, 100))
        assert got.shape == (th, tw) and np.abs(got.astype(int) - tile).max() <= 2
        assert L.sq_jpeg_chunk_count(1, th, tw, th, tw) == 1
        assert L.sq_jpeg_out_bound(1, th, tw, native.SQ_U8, th, tw) > 0 and L.sq_jpeg_scratch_bytes(1, th, tw, native.SQ_U8, th, tw) > 0
    for side in (65504, 65528, 65536):
        for th, tw in ((8, side), (side, 8)):
            with pytest.raises(ValueError, match='8..65496'):
                J.header(th, tw, 90)
            assert L.sq_jpeg_chunk_count(1, th, tw, th, tw) == native.SQ_ERR_UNSUPPORTED
            assert L.sq_jpeg_out_bound(1, th, tw, native.SQ_U8, th, tw) == native.SQ_ERR_UNSUPPORTED
    # what the limit is there for: the same header with the next side in it is a stream libjpeg does not open
    s = bytearray(J.encode_tile(np.full((8, J.MAX_SIDE), 9, np.uint8), 50))
    at = 2 + 69 + 7
    assert s[at:at + 2] == bytes((J.MAX_SIDE >> 8, J.MAX_SIDE & 255))
    s[at:at + 2] = bytes((65504 >> 8, 65504 & 255))
    with pytest.raises(OSError):
        with Image.open(io.BytesIO(bytes(s))) as im:
            im.load()
